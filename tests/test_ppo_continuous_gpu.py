"""PPOContinuous (diagonal-Gaussian PPO, hpc_rll.rl_utils.ppo) against an fp64 restatement on the CPU.

Oracle: ``oracle()`` below -- ``Independent(Normal(mu, sigma), 1)`` log-probabilities and entropy in the formula of
origin/ppo.py (ratio, clipped surrogate, optional dual clip, clipped value loss, weighted entropy, the two monitors), run
in fp64 on the same fp32 inputs; gradients from autograd with the DISTINCT upstream weights 1.3 / 0.7 / 0.9 on the three
losses so that every backward term is exercised.

Bars: losses ``rel_err < 1e-5``; monitors ``1e-4`` (clipfrac counts strict inequalities of fp32 ratios, as in the
categorical PPO tests); gradients through ``conftest.grad_err`` (relative to the tensor's maximum) below
``max(2e-5, 2 * e32)``, where ``e32`` is the error of the SAME restatement run in fp32 on the CPU against its fp64 run,
computed here at run time per tensor.  2e-5 is the project's gradient bar; torch's own fp32 formula subtracts two sums of
size ~A and loses more than that at large A (A = 376: 4-7e-5), which no fp32 result can be held to; the factor 2 allows
for a different summation order.  The kernel accumulates per-dimension differences and is expected to stay well below.

Input conditions, asserted on the fp64 oracle before any GPU result is compared:
  * no sample within 1e-4 of ``ratio = 1 +- clip`` nor of the dual-clip tie ``ratio = dual_clip``: such a sample may
    legitimately take the other branch in fp32.  The count is asserted to be ZERO and no sample is excluded from any
    comparison.  Seeds alone cannot give that at B = 65536 (the expected count is ~2.5e-4 per sample, ~16 samples), so
    ``problem()`` builds the inputs and then shrinks ``mu_new - mu_old`` of the offending rows by 7 % until none is left
    within 5e-4; what is tested is the tensor that results.
  * ``0.05 < clipfrac < 0.95`` (both branches run) for every B >= 7.  With B = 1 the fraction is 0 or 1 by construction;
    ``test_single_sample_both_states`` runs seeds that give both a clipped and an unclipped sample (asserted).
  * ``test_close_policies`` (new parameters within 0.1 / sqrt(A) standard deviations of the old ones) have clipfrac in 0.1-0.3.
"""
import math
import os
import socket

import numpy as np
import pytest
import torch
from torch.distributions import Independent, Normal

from conftest import ROOT, grad_err, rel_err
from guarded import place

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CLIP = 0.2
CO = (1.3, 0.7, 0.9)          # upstream gradients of policy / value / entropy loss
TOL, MON_TOL, GTOL = 1e-5, 1e-4, 2e-5
BIG = ("mu_new", "sigma_new", "mu_old", "sigma_old", "action")


def problem(B, A, seed, delta=0.3, dual=None):
    """fp32 CPU inputs.  Actions are draws from the old policy; the new policy is ``delta / sqrt(A)`` old standard
    deviations away per dimension, so that log ratio has a standard deviation of about ``delta * sqrt(3)`` whatever A."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    x = {}
    x["mu_old"] = r(B, A)
    x["sigma_old"] = torch.exp(0.3 * r(B, A))
    x["action"] = x["mu_old"] + x["sigma_old"] * r(B, A)
    k = delta / math.sqrt(A)
    x["mu_new"] = x["mu_old"] + k * x["sigma_old"] * r(B, A)
    x["sigma_new"] = x["sigma_old"] * torch.exp(k * r(B, A))
    x["value_new"], x["adv"], x["return_"] = r(B), r(B), r(B)
    x["value_old"] = x["value_new"] + 0.3 * r(B)
    x["weight"] = torch.rand(B, generator=g) + 0.5
    for _ in range(40):
        near = near_boundary(log_ratio64(x).exp(), dual, 5e-4)
        if not near.any():
            break
        x["mu_new"][near] = x["mu_old"][near] + 0.93 * (x["mu_new"][near] - x["mu_old"][near])
    return x


def log_ratio64(x):
    d = {k: x[k].double() for k in BIG}
    return (Independent(Normal(d["mu_new"], d["sigma_new"]), 1).log_prob(d["action"]) -
            Independent(Normal(d["mu_old"], d["sigma_old"]), 1).log_prob(d["action"]))


def near_boundary(ratio, dual, margin):
    near = ((ratio - (1 + CLIP)).abs() < margin) | ((ratio - (1 - CLIP)).abs() < margin)
    if dual is not None:
        near |= (ratio - dual).abs() < margin
    return near


def oracle(x, dtype, has_w, uvc, dual):
    """The restatement, on the CPU in ``dtype``: (losses, info, grads of mu_new / sigma_new / value_new, ratio)."""
    t = {k: v.to(dtype) for k, v in x.items()}
    mu, sg, vn = (t[k].clone().requires_grad_(True) for k in ("mu_new", "sigma_new", "value_new"))
    w = t["weight"] if has_w else torch.ones_like(t["adv"])
    new, old = Independent(Normal(mu, sg), 1), Independent(Normal(t["mu_old"], t["sigma_old"]), 1)
    logp_new, logp_old, ent = new.log_prob(t["action"]), old.log_prob(t["action"]), new.entropy()
    ratio = torch.exp(logp_new - logp_old)
    adv, ret = t["adv"], t["return_"]
    inner = torch.min(ratio * adv, ratio.clamp(1 - CLIP, 1 + CLIP) * adv)
    if dual is not None:
        inner = torch.max(inner, dual * adv)
    policy = (-inner * w).mean()
    if uvc:
        vclip = t["value_old"] + (vn - t["value_old"]).clamp(-CLIP, CLIP)
        v = torch.max((ret - vn) ** 2, (ret - vclip) ** 2)
    else:
        v = (ret - vn) ** 2
    value = 0.5 * (v * w).mean()
    entropy = (ent * w).mean()
    (CO[0] * policy + CO[1] * value + CO[2] * entropy).backward()
    with torch.no_grad():
        info = [(logp_old - logp_new).mean().item(),
                ((ratio > 1 + CLIP) | (ratio < 1 - CLIP)).to(dtype).mean().item()]
    return ([policy.item(), value.item(), entropy.item()], info,
            [mu.grad.numpy(), sg.grad.numpy(), vn.grad.numpy()], ratio.detach())


def rel_max(ref, got):
    """grad_err's measure without its asserts (for e32, which is a property of torch's fp32 formula, not of the kernels)."""
    ref, got = np.asarray(ref, np.float64), np.asarray(got, np.float64)
    s = np.abs(ref).max()
    return float(np.abs(ref - got).max() / s) if s > 0 else 0.0


def on_gpu(x, off=0):
    """The inputs on the GPU; ``off`` floats off 16-byte alignment for the five (B,A) tensors (off = 0: torch's own)."""
    d = {k: v.to(DEV) for k, v in x.items()}
    if off:
        for k in BIG:
            d[k] = place(d[k], off)
    for k in ("mu_new", "sigma_new", "value_new"):
        d[k] = d[k].detach().requires_grad_(True)
    return d


def run_gpu(d, has_w, uvc, dual, **kw):
    from hpc_rll.rl_utils.ppo import PPOContinuous
    B, A = d["mu_new"].shape
    loss, info = PPOContinuous(B, A, **kw)(d["mu_new"], d["sigma_new"], d["mu_old"], d["sigma_old"], d["action"],
                                           d["value_new"], d["value_old"], d["adv"], d["return_"],
                                           d["weight"] if has_w else None, CLIP, uvc, dual)
    (CO[0] * loss.policy_loss + CO[1] * loss.value_loss + CO[2] * loss.entropy_loss).sum().backward()
    return loss, info, [d[k].grad for k in ("mu_new", "sigma_new", "value_new")]


def check(B, A, seed, has_w, uvc, dual, delta=0.3, off=0, frac_range=(0.05, 0.95)):
    x = problem(B, A, seed, delta, dual)
    l64, i64, g64, ratio = oracle(x, torch.float64, has_w, uvc, dual)
    assert int(near_boundary(ratio, dual, 1e-4).sum()) == 0, "a sample lies within 1e-4 of a branch boundary"
    if B >= 7:
        assert frac_range[0] < i64[1] < frac_range[1], f"clipfrac {i64[1]} outside {frac_range}: one branch is not exercised"
    _, _, g32, _ = oracle(x, torch.float32, has_w, uvc, dual)
    e32 = [rel_max(a, b) for a, b in zip(g64, g32)]
    d = on_gpu(x, off)
    if off:
        assert all(d[k].data_ptr() % 16 == 4 * off for k in BIG)
    loss, info, grads = run_gpu(d, has_w, uvc, dual)
    assert isinstance(info.approx_kl, float) and isinstance(info.clipfrac, float)
    el = rel_err(l64, [v.item() for v in loss])
    ei = rel_err(i64, list(info))
    eg = [grad_err(a, b.cpu().numpy(), n) for a, b, n in zip(g64, grads, ("grad_mu", "grad_sigma", "grad_value"))]
    print(f"ppo_continuous B={B} A={A} w={has_w} uvc={uvc} dual={dual} delta={delta} off={off} clipfrac={i64[1]:.3f} "
          f"loss_err={el:.2e} info_err={ei:.2e} grad_err(mu,sigma,value)={eg[0]:.2e},{eg[1]:.2e},{eg[2]:.2e} "
          f"e32={e32[0]:.2e},{e32[1]:.2e},{e32[2]:.2e}")
    assert el < TOL, (el, l64)
    assert ei < MON_TOL, (ei, i64, list(info))
    for name, e, e3 in zip(("grad_mu", "grad_sigma", "grad_value"), eg, e32):
        assert e < max(GTOL, 2 * e3), (name, e, e3)
    return i64


VARIANTS = [(w, u, dc) for w in (False, True) for u in (True, False) for dc in (None, 3.0)]
# every (A, B) with B * A <= 2^24 elements per tensor (the fp64 oracle and its autograd hold a dozen of them on the CPU):
# A = 376 and 1024 stop at B = 4096.  The weight / use_value_clip / dual_clip variant cycles through the list.
SHAPES = [(B, A) for A in (1, 3, 6, 17, 64, 130, 376, 1024) for B in (1, 7, 4096, 65536) if B * A <= 1 << 24]


@pytest.mark.parametrize("B,A,variant", [(B, A, i % len(VARIANTS)) for i, (B, A) in enumerate(SHAPES)])
def test_parity_with_fp64_oracle(B, A, variant):
    has_w, uvc, dual = VARIANTS[variant]
    check(B, A, 1000 * A + B, has_w, uvc, dual)


@pytest.mark.parametrize("has_w,uvc,dual", VARIANTS)
@pytest.mark.parametrize("B,A", [(4096, 6), (4099, 64)])
def test_every_variant(B, A, has_w, uvc, dual):
    check(B, A, 77 + A, has_w, uvc, dual)
    if dual is not None:   # the dual clip must actually bind somewhere: a sample with adv < 0 beyond ratio = dual_clip
        x = problem(B, A, 77 + A, 0.3, dual)
        assert int(((log_ratio64(x).exp() > dual) & (x["adv"] < 0)).sum()) > 0


@pytest.mark.parametrize("B,A", [(4096, 6), (65536, 64), (4096, 376)])
def test_close_policies(B, A):
    """New parameters within 0.1 / sqrt(A) standard deviations of the old ones: what a PPO epoch really sees."""
    check(B, A, 5 + A, True, True, None, delta=0.1, frac_range=(0.1, 0.3))


def test_single_sample_both_states():
    seen = set()
    for seed in (3, 4, 5, 6, 7, 8):
        seen.add(check(1, 17, seed, True, True, 3.0)[1])
    assert seen == {0.0, 1.0}, seen


@pytest.mark.parametrize("B,A,off", [(4096, 64, 1), (4099, 17, 1), (7, 1024, 1), (65536, 6, 3), (4096, 376, 2)])
def test_unaligned_views(B, A, off):
    """The five (B,A) inputs as contiguous views that start 4 / 8 / 12 bytes past a 16-byte boundary (a slice of a
    rollout buffer): the 4-byte load and store paths, between guard bands."""
    check(B, A, 31 * A + B, True, True, 3.0, off=off)


@pytest.mark.parametrize("B,A", [(4096, 64), (513, 1024), (65536, 8)])
def test_load_paths_agree(B, A):
    """One problem on torch's aligned allocations (16-byte packs) and on a copy one float off (4-byte accesses)."""
    x = problem(B, A, 9 + A, 0.3, 3.0)
    _, _, g64, _ = oracle(x, torch.float64, True, True, 3.0)
    _, _, g32, _ = oracle(x, torch.float32, True, True, 3.0)
    la, ia, ga = run_gpu(on_gpu(x), True, True, 3.0)
    lo, io, go = run_gpu(on_gpu(x, 1), True, True, 3.0)
    assert rel_err([v.item() for v in la], [v.item() for v in lo]) < TOL and rel_err(list(ia), list(io)) < MON_TOL
    for a, b, r64, r32 in zip(ga, go, g64, g32):
        assert grad_err(a.cpu().numpy(), b.cpu().numpy(), "aligned_vs_offset") < max(GTOL, 2 * rel_max(r64, r32))


@pytest.mark.parametrize("B,A", [(65536, 64), (4099, 17), (300, 1024)])
def test_bitwise_repeatable(B, A):
    x = problem(B, A, 11, 0.3, 3.0)
    runs = []
    for _ in range(2):
        loss, info, grads = run_gpu(on_gpu(x), True, True, 3.0, sync_info=False)
        runs.append([v.detach().clone() for v in loss] + [info.approx_kl, info.clipfrac] + grads)
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_graphed_step_replays_eager_bits():
    """``sync_info=False`` keeps the monitors on the device (0-d tensors), so forward + backward is one hipGraph."""
    import hpc_rll
    from hpc_rll.rl_utils.ppo import PPOContinuous
    B, A = 4096, 24
    d = on_gpu(problem(B, A, 13, 0.3, 3.0))
    args = (d["mu_new"], d["sigma_new"], d["mu_old"], d["sigma_old"], d["action"], d["value_new"], d["value_old"], d["adv"],
            d["return_"])
    step = hpc_rll.graphed(PPOContinuous(B, A, sync_info=False), *args, d["weight"], CLIP, True, 3.0)
    (loss, info), (dmu, dsg, dvn) = step()
    assert isinstance(info.approx_kl, torch.Tensor) and info.approx_kl.is_cuda and info.approx_kl.dim() == 0
    assert isinstance(info.clipfrac, torch.Tensor) and info.clipfrac.is_cuda and info.clipfrac.dim() == 0
    ref_loss, ref_info = PPOContinuous(B, A)(*args, d["weight"], CLIP, True, 3.0)
    sum(ref_loss).sum().backward()
    assert all(torch.equal(a, b.detach()) for a, b in zip(loss, ref_loss))
    assert info.approx_kl.item() == ref_info.approx_kl and info.clipfrac.item() == ref_info.clipfrac
    assert torch.equal(dmu, d["mu_new"].grad) and torch.equal(dsg, d["sigma_new"].grad) and torch.equal(dvn, d["value_new"].grad)


def test_functional_form_and_partial_gradients():
    """``ppo_continuous`` equals the module; a head that does not require grad gets no gradient and the others keep their bits."""
    from hpc_rll.rl_utils.ppo import ppo_continuous
    x = problem(1000, 12, 17, 0.3, None)
    _, _, full = run_gpu(on_gpu(x), False, True, None)
    for frozen in ("mu_new", "sigma_new", "value_new", ("mu_new", "sigma_new")):
        frozen = (frozen,) if isinstance(frozen, str) else frozen
        d = on_gpu(x)
        for k in frozen:
            d[k] = d[k].detach()
        loss, info = ppo_continuous(d["mu_new"], d["sigma_new"], d["mu_old"], d["sigma_old"], d["action"], d["value_new"],
                                    d["value_old"], d["adv"], d["return_"])
        (CO[0] * loss.policy_loss + CO[1] * loss.value_loss + CO[2] * loss.entropy_loss).sum().backward()
        for k, ref in zip(("mu_new", "sigma_new", "value_new"), full):
            assert d[k].grad is None if k in frozen else torch.equal(d[k].grad, ref), (frozen, k)


def test_edges():
    import hpc_rl_utils
    from hpc_rll.rl_utils.ppo import PPOContinuous
    A = 5
    z = lambda *s: torch.zeros(*s, device=DEV)   # noqa: E731
    mu, sg, vn = z(0, A).requires_grad_(True), torch.ones(0, A, device=DEV, requires_grad=True), z(0).requires_grad_(True)
    loss, info = PPOContinuous(0, A)(mu, sg, z(0, A), torch.ones(0, A, device=DEV), z(0, A), vn, z(0), z(0), z(0))
    assert [v.item() for v in loss] == [0.0, 0.0, 0.0] and list(info) == [0.0, 0.0]
    sum(loss).sum().backward()
    assert mu.grad.shape == (0, A) and sg.grad.shape == (0, A) and vn.grad.shape == (0,)

    def call(B=4, A=8, **repl):
        a = dict(mu_new=z(B, A), sigma_new=z(B, A) + 1, mu_old=z(B, A), sigma_old=z(B, A) + 1, action=z(B, A), value_new=z(B),
                 value_old=z(B), adv=z(B), return_=z(B))
        a.update(repl)
        return hpc_rl_utils.ppo_continuous(*a.values())
    assert len(call()) == 4
    with pytest.raises(RuntimeError, match="not supported"):
        call(A=1025)                                           # above the supported maximum
    call(A=1024)
    with pytest.raises(RuntimeError, match="GPU"):
        call(sigma_old=torch.ones(4, 8))                       # a CPU tensor
    with pytest.raises(RuntimeError, match="dtype"):
        call(action=torch.zeros(4, 8, device=DEV, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="dtype"):
        call(mu_new=torch.zeros(4, 8, device=DEV, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="contiguous"):
        call(mu_old=z(8, 4).t())
    with pytest.raises(RuntimeError, match="shape"):
        call(adv=z(5))
    with pytest.raises(RuntimeError, match="shape"):
        call(sigma_new=z(4, 7) + 1)


# ------------------------------------------------------------------------------------------------ sharded, one rank
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _one_rank_worker(port, q):
    import sys
    import traceback
    try:
        for p in (ROOT, os.path.join(ROOT, "di-hpc_amd"), os.path.join(ROOT, "tests")):
            sys.path.insert(0, p)
        import torch.distributed as dist
        os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
        torch.cuda.set_device(DEV)
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=DEV)
        loss, info, grads = run_gpu(on_gpu(problem(640, 20, 21, 0.3, 3.0)), True, True, 3.0, sharded=True)
        q.put(("ok", [v.item() for v in loss], list(info), [g.cpu().numpy() for g in grads]))
        dist.destroy_process_group()
    except BaseException as e:  # noqa: BLE001
        q.put(("error", f"{type(e).__name__}: {e}\n{traceback.format_exc()}"))
        raise


def test_sharded_one_rank_equals_unsharded():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_one_rank_worker, args=(_free_port(), q))
    p.start()
    try:
        res = q.get(timeout=300)
    finally:
        p.join(30)
        if p.is_alive():
            p.kill()
    assert res[0] == "ok", res[1]
    loss, info, grads = run_gpu(on_gpu(problem(640, 20, 21, 0.3, 3.0)), True, True, 3.0)
    assert [v.item() for v in loss] == res[1] and list(info) == res[2]
    assert all(np.array_equal(g.cpu().numpy(), r) for g, r in zip(grads, res[3]))
