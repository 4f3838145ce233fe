"""VTraceContinuous (V-trace for diagonal-Gaussian policies, hpc_rll.rl_utils.vtrace) against an fp64 restatement on the CPU.

Oracle: ``oracle()`` below -- ``Independent(Normal(mu, sigma), 1)`` log-probabilities and entropy feeding the recursion of
``masked_vtrace``'s docstring as a plain reverse loop over T, run in fp64 on the same fp32 inputs (with the fp32 gamma and
gamma*lambda the kernels receive); gradients from autograd with the DISTINCT upstream weights ``CO`` on the three losses.

Bars: losses ``rel_err < 1e-5`` (the project's bar); gradients through ``conftest.grad_err`` (relative to the tensor's
maximum) below ``max(2e-5, 2 * e32)`` per tensor, where ``e32`` is the error of the SAME restatement run in fp32 on the CPU
against its fp64 run, computed here at run time: torch's fp32 log-prob subtracts two sums of size ~A, which no fp32 result can
be held to (tests/test_ppo_continuous_gpu.py has the same bar for the same reason).  The head alone
(``hpc_rll_gaussian_forward``): error relative to the tensor's maximum below ``max(1e-6, 2 * e32)``; the 1e-6 floor (about
8 ulp) allows for the 1-ulp ``v_log`` / ``v_rcp`` per element, which the CPU's libm does not have.

Input condition, asserted on the fp64 oracle before anything is compared: the share of (t,b) with ``IS > 1`` lies in
(0.05, 0.95), so both sides of every clip are active at clip ratio 1.0.  ``problem()`` draws the actions from the behaviour
policy and puts the target ``0.3 / sqrt(A)`` standard deviations away, which gives a share near one half whatever A; the seeds
are fixed functions of the shape and were checked on the CPU.  A single sample (T = B = 1) has a share of 0 or 1 by
construction: there the case runs consecutive seeds and asserts that both ``IS > 1`` and ``IS < 1`` were seen.  The clips are
continuous and ``vs`` / ``adv`` are constants, so no sample sits at a discontinuity and none is excluded anywhere.
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
CO = (1.3, 0.7, 0.9)          # upstream gradients of policy / value / entropy loss
TOL, GTOL, HEAD_TOL = 1e-5, 2e-5, 1e-6
BIG = ("mu_t", "sigma_t", "mu_b", "sigma_b", "action")
F64 = torch.float64


# ------------------------------------------------------------------------------------------------------------- inputs
def problem(T, B, A, seed, delta=0.3):
    """fp32 CPU inputs.  Actions are draws from the behaviour policy; the target policy is ``delta / sqrt(A)`` behaviour
    standard deviations away per dimension, so that the log ratio has a spread of about ``delta * sqrt(3)`` whatever A."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    x = {}
    x["mu_b"] = r(T, B, A)
    x["sigma_b"] = torch.exp(0.3 * r(T, B, A))
    x["action"] = x["mu_b"] + x["sigma_b"] * r(T, B, A)
    k = delta / math.sqrt(A)
    x["mu_t"] = x["mu_b"] + k * x["sigma_b"] * r(T, B, A)
    x["sigma_t"] = x["sigma_b"] * torch.exp(k * r(T, B, A))
    x["value"] = r(T + 1, B)                      # stacked; the next-value form uses rows [:T] and x["next_value"]
    x["next_value"] = r(T, B)
    x["reward"] = r(T, B)
    x["weight"] = torch.rand(T, B, generator=g) + 0.5
    return x


def make_masks(T, B, form, kind, nvf, seed):
    """(done, traj_flag) on the CPU for ``form`` in none / done / both / flag.  Episode ends sit at t = T-1, T-8, T-9 and 0
    (the edges of the 8-step wave chunks) in some columns and at 4 % of the other steps; ``both`` adds truncations
    (done = 0, traj_flag = 1); ``flag`` alone is truncation only.  float32 masks are soft: values in (0, 1]."""
    if form == "none":
        return None, None
    g = torch.Generator().manual_seed(seed)
    ends = torch.rand(T, B, generator=g) < 0.04
    for t, step in ((T - 1, 2), (T - 8, 3), (T - 9, 5), (0, 4)):
        if 0 <= t < T:
            ends[t, ::step] = True
    trunc = (torch.rand(T, B, generator=g) < 0.06) & ~ends
    for t, first in ((T - 1, 1), (T - 8, 1), (T - 9, 2), (0, 1)):
        if 0 <= t < T:
            trunc[t, first::7] = ~ends[t, first::7]
    soft = 0.25 + 0.75 * torch.rand(T, B, generator=g)

    def cast(m):
        if kind == "bool":
            return m
        if kind == "uint8":   # any nonzero byte counts as 1
            return m.to(torch.uint8) * torch.randint(1, 256, (T, B), generator=g).to(torch.uint8)
        out = m.to(torch.float32) * soft
        out[T - 1] = m[T - 1].to(torch.float32)   # (hard ends in the last row as well as soft ones elsewhere)
        return out
    if form == "done":
        return cast(ends), None
    if form == "flag":
        return None, cast(ends | trunc)
    return cast(ends), cast(ends | trunc)


def _keep(m, like, dtype):
    if m is None:
        return torch.ones_like(like)
    if m.dtype == torch.float32:
        return 1.0 - m.to(dtype)
    return (m == 0).to(dtype)


def _g32(gamma, lam):
    g = np.float32(gamma)
    return float(g), float(np.float32(g * np.float32(lam)))


# ------------------------------------------------------------------------------------------------------------- oracle
def heads(x, dtype):
    """(logp_t, entropy, logp_b) of the restatement in ``dtype`` on the CPU, (T,B) each, differentiable wrt mu_t / sigma_t."""
    tgt = Independent(Normal(x["mu_t"].to(dtype), x["sigma_t"].to(dtype)), 1)
    beh = Independent(Normal(x["mu_b"].to(dtype), x["sigma_b"].to(dtype)), 1)
    a = x["action"].to(dtype)
    return tgt.log_prob(a), tgt.entropy(), beh.log_prob(a)


def oracle(x, dtype, done=None, flag=None, nvf=False, has_w=False, clips=(1.0, 1.0, 1.0), gamma=0.99, lam=0.95):
    """The restatement on the CPU in ``dtype``: (losses, [grad mu_t, grad sigma_t, grad value], share of IS > 1)."""
    g, disc = _g32(gamma, lam)
    y = dict(x)
    y["mu_t"] = x["mu_t"].to(dtype).clone().requires_grad_(True)
    y["sigma_t"] = x["sigma_t"].to(dtype).clone().requires_grad_(True)
    v = (x["value"][:-1] if nvf else x["value"]).to(dtype).clone().requires_grad_(True)
    r = x["reward"].to(dtype)
    T, B = r.shape
    lp, ent, lb = heads(y, dtype)
    with torch.no_grad():
        is_w = torch.exp(lp - lb)
        rho, c, rpg = is_w.clamp(max=clips[0]), is_w.clamp(max=clips[1]), is_w.clamp(max=clips[2])
        vd = v.detach()
        nv = x["next_value"].to(dtype) if nvf else vd[1:]
        kd = _keep(done, r, dtype)
        kf = _keep(flag, r, dtype) if flag is not None else kd
        s = torch.zeros(B, dtype=dtype)
        vs, adv = torch.empty_like(r), torch.empty_like(r)
        for t in range(T - 1, -1, -1):
            adv[t] = rpg[t] * (r[t] + g * (kd[t] * nv[t] + kf[t] * s) - vd[t])
            s = rho[t] * (r[t] + g * kd[t] * nv[t] - vd[t]) + disc * kf[t] * c[t] * s
            vs[t] = vd[t] + s
    w = x["weight"].to(dtype) if has_w else torch.ones_like(r)
    pg = -(lp * adv * w).mean()
    vl = (w * (v[:T] - vs) ** 2).mean()
    el = (w * ent).mean()
    grads = torch.autograd.grad(CO[0] * pg + CO[1] * vl + CO[2] * el, (y["mu_t"], y["sigma_t"], v))
    return [pg.item(), vl.item(), el.item()], [t.numpy() for t in grads], float((is_w > 1).to(F64).mean())


def rel_max(ref, got):
    """max |ref - got| / max |ref|: grad_err's measure without its asserts."""
    ref, got = np.asarray(ref, np.float64), np.asarray(got, np.float64)
    s = np.abs(ref).max()
    return float(np.abs(ref - got).max() / s) if s > 0 else 0.0


# --------------------------------------------------------------------------------------------------------------- GPU
def on_gpu(x, nvf=False, off=0, grad=("mu_t", "sigma_t", "value")):
    d = {k: v.to(DEV) for k, v in x.items()}
    if nvf:
        d["value"] = d["value"][:-1].contiguous()
    if off:
        for k in BIG:
            d[k] = place(d[k], off)
            assert d[k].data_ptr() % 16 == 4 * off
    for k in grad:
        d[k] = d[k].detach().requires_grad_(True)
    return d


def to_dev(m):
    return None if m is None else m.to(DEV)


def run_gpu(d, done=None, flag=None, nvf=False, has_w=False, clips=(1.0, 1.0, 1.0), module=None, wrt=("mu_t", "sigma_t", "value")):
    from hpc_rll.rl_utils.vtrace import vtrace_continuous
    fn = module or vtrace_continuous
    out = fn(d["mu_t"], d["sigma_t"], d["mu_b"], d["sigma_b"], d["action"], d["value"], d["reward"], to_dev(done),
             d["weight"] if has_w else None, 0.99, 0.95, clips[0], clips[1], clips[2], d["next_value"] if nvf else None,
             to_dev(flag))
    co = [torch.tensor([c], device=DEV) for c in CO]
    grads = torch.autograd.grad(list(out), [d[k] for k in wrt], co)
    return [v.detach() for v in out], list(grads)


def check(x, tag, **kw):
    """One problem against the oracle; returns the fp64 share of IS > 1.  ``kw``: done, flag, nvf, has_w, clips (+ off)."""
    off = kw.pop("off", 0)
    l64, g64, share = oracle(x, F64, **kw)
    T, B = x["reward"].shape
    if T * B > 1:
        assert 0.05 < share < 0.95, f"{tag}: share of IS > 1 is {share}: one side of the clips is not exercised"
    _, g32, _ = oracle(x, torch.float32, **kw)
    e32 = [rel_max(a, b) for a, b in zip(g64, g32)]
    losses, grads = run_gpu(on_gpu(x, kw.get("nvf", False), off), **kw)
    el = [rel_err(a, b.item()) for a, b in zip(l64, losses)]
    names = ("grad_mu", "grad_sigma", "grad_value")
    eg = [grad_err(a, b.cpu().numpy(), n) for a, b, n in zip(g64, grads, names)]
    print(f"vtrace_continuous {tag} share={share:.3f} loss_err(pg,v,ent)={el[0]:.2e},{el[1]:.2e},{el[2]:.2e} "
          f"grad_err(mu,sigma,value)={eg[0]:.2e},{eg[1]:.2e},{eg[2]:.2e} e32={e32[0]:.2e},{e32[1]:.2e},{e32[2]:.2e}")
    for name, e in zip(("policy", "value", "entropy"), el):
        assert e < TOL, (tag, name, e, l64)
    for name, e, e3 in zip(names, eg, e32):
        assert e < max(GTOL, 2 * e3), (tag, name, e, e3)
    return share


# ---------------------------------------------------------------------------------------------------------- the head
HEAD_A = (1, 2, 3, 4, 5, 8, 12, 16, 17, 32, 64, 100, 128, 256, 260, 376, 512, 1000, 1024)


def head_gpu(d, rows, A):
    import cabi
    out = [torch.full((rows,), float("nan"), device=DEV) for _ in range(3)]
    cabi.call("hpc_rll_gaussian_forward", DEV, *(cabi.ptr(d[k]) for k in BIG), *(cabi.ptr(o) for o in out), rows, A)
    return out


def check_head(rows, A, off):
    x = problem(1, rows, A, 7 * A + rows + off)
    ref64 = [t.detach().reshape(rows).numpy() for t in heads(x, F64)]
    ref32 = [t.detach().reshape(rows).numpy() for t in heads(x, torch.float32)]
    d = on_gpu(x, off=off, grad=())
    got = head_gpu(d, rows, A)
    for name, r64, r32, o in zip(("logp", "entropy", "logp_b"), ref64, ref32, got):
        e32, e = rel_max(r64, r32), rel_max(r64, o.cpu().numpy())
        print(f"gaussian_forward rows={rows} A={A} off={off} {name}: err={e:.2e} e32={e32:.2e}")
        assert torch.isfinite(o).all(), name
        assert e < max(HEAD_TOL, 2 * e32), (name, e, e32)


@pytest.mark.parametrize("A", HEAD_A)
@pytest.mark.parametrize("rows", [35, 1031])
def test_head_parity(rows, A):
    """Every (G, VEC, E) of the 16-byte path (A % 4 == 0) and, for the other A, of the 4-byte path; row tails."""
    check_head(rows, A, 0)


@pytest.mark.parametrize("A", [4, 64, 1024])
@pytest.mark.parametrize("rows", [35, 1031])
def test_head_parity_one_float_off_alignment(rows, A):
    check_head(rows, A, 1)


@pytest.mark.parametrize("A,off", [(1, 0), (17, 0), (64, 0), (64, 1), (1024, 0)])
def test_head_identical_policies_give_identical_logp(A, off):
    rows = 1031
    x = problem(1, rows, A, 3 + A)
    x["mu_b"], x["sigma_b"] = x["mu_t"].clone(), x["sigma_t"].clone()
    d = on_gpu(x, off=off, grad=())
    logp, _, logp_b = head_gpu(d, rows, A)
    assert torch.equal(logp, logp_b)
    d["mu_b"], d["sigma_b"] = d["mu_t"], d["sigma_t"]            # the same tensors
    logp2, _, logp_b2 = head_gpu(d, rows, A)
    assert torch.equal(logp2, logp_b2) and torch.equal(logp2, logp)


def test_head_zero_rows():
    import cabi
    z = torch.zeros(4, device=DEV)
    cabi.call("hpc_rll_gaussian_forward", DEV, *(cabi.ptr(z),) * 8, 0, 4)


# ------------------------------------------------------------------------------------------------------- the full op
SHAPES = [(T, B, A) for (T, B) in ((1, 1), (5, 7), (8, 64), (9, 65), (16, 33), (17, 130), (40, 257))
          for A in (1, 6, 17, 64, 376, 1024) if T * B * A <= 1 << 22]


@pytest.mark.parametrize("T,B,A", SHAPES)
def test_parity_with_fp64_oracle(T, B, A):
    i = SHAPES.index((T, B, A))
    kw = dict(has_w=bool(i % 2), nvf=bool((i // 2) % 2))
    if T * B > 1:
        check(problem(T, B, A, 1000 * A + 10 * T + B), f"T={T} B={B} A={A}", **kw)
        return
    seen = set()
    for seed in range(8):   # a single sample: both IS > 1 and IS < 1 over consecutive seeds
        seen.add(check(problem(T, B, A, 100 * A + seed), f"T=1 B=1 A={A} seed={seed}", **kw))
    assert seen == {0.0, 1.0}, seen


FORMS = [("none", "bool")] + [(f, k) for f in ("done", "both", "flag") for k in ("bool", "uint8", "float32")]


@pytest.mark.parametrize("nvf", [False, True], ids=["stacked", "next_value"])
@pytest.mark.parametrize("form,kind", FORMS)
def test_every_mask_form(form, kind, nvf):
    T, B, A = 17, 65, 6
    x = problem(T, B, A, 41)
    done, flag = make_masks(T, B, form, kind, nvf, 43)
    if form == "both":      # truncation: done = 0 and traj_flag = 1 somewhere, also in the chunk-edge rows
        tr = (done == 0) & (flag != 0)
        assert all(bool(tr[t].any()) for t in (T - 1, T - 8, T - 9, 0))
    if form in ("done", "both"):
        assert all(bool((done[t] != 0).any()) for t in (T - 1, T - 8, T - 9, 0))
    for has_w in (False, True):
        for clips in ((1.0, 1.0, 1.0), (0.8, 1.2, 1.5)):
            check(x, f"{form}/{kind}/{'nv' if nvf else 'stacked'} w={has_w} clips={clips}", done=done, flag=flag, nvf=nvf,
                  has_w=has_w, clips=clips)


def test_truncation_case():
    """Next-value form, done = 0 everywhere, traj_flag = 1 at the truncated steps: the trace is cut, the bootstrap stays."""
    T, B, A = 17, 65, 6
    x = problem(T, B, A, 47)
    _, flag = make_masks(T, B, "flag", "bool", True, 49)
    done = torch.zeros(T, B, dtype=torch.bool)
    check(x, "truncation", done=done, flag=flag, nvf=True, has_w=True)
    a, ga = run_gpu(on_gpu(x, True), done=done, flag=flag, nvf=True, has_w=True)
    b, gb = run_gpu(on_gpu(x, True), flag=flag, nvf=True, has_w=True)            # traj_flag only: done defaults to 0
    assert all(torch.equal(p, q) for p, q in zip(a + ga, b + gb))
    c, _ = run_gpu(on_gpu(x, True), nvf=True, has_w=True)
    assert not torch.equal(a[0], c[0])                                           # the cuts do change the loss


# ------------------------------------------------------------------------------------- same bits as the scan it reuses
@pytest.mark.parametrize("T,B,A", [(17, 65, 6), (8, 64, 64), (40, 257, 17)])
def test_zero_masks_equal_the_mask_free_call_bit_for_bit(T, B, A):
    x = problem(T, B, A, 5 + A)
    for nvf in (False, True):
        ref, gref = run_gpu(on_gpu(x, nvf), nvf=nvf, has_w=True, clips=(1.0, 0.9, 1.1))
        for z in (torch.zeros(T, B, dtype=torch.bool), torch.zeros(T, B, dtype=torch.uint8), torch.zeros(T, B)):
            for kw in ({"done": z}, {"done": z, "flag": z}, {"flag": z}):
                out, g = run_gpu(on_gpu(x, nvf), nvf=nvf, has_w=True, clips=(1.0, 0.9, 1.1), **kw)
                assert all(torch.equal(p, q) for p, q in zip(out + g, ref + gref)), (nvf, z.dtype, list(kw))


@pytest.mark.parametrize("T,B,A", [(1, 1, 3), (17, 65, 6), (9, 65, 64), (40, 257, 17)])
def test_stacked_and_next_value_forms_agree_bit_for_bit(T, B, A):
    x = problem(T, B, A, 9 + A)
    x["next_value"] = x["value"][1:].clone()
    done, flag = make_masks(T, B, "both", "float32", False, 11)
    for kw in ({}, {"done": done}, {"done": done, "flag": flag, "has_w": True}):
        a, ga = run_gpu(on_gpu(x, False), nvf=False, **kw)
        b, gb = run_gpu(on_gpu(x, True), nvf=True, **kw)
        assert all(torch.equal(p, q) for p, q in zip(a, b)), list(kw)
        assert torch.equal(ga[0], gb[0]) and torch.equal(ga[1], gb[1]) and torch.equal(ga[2][:T], gb[2]), list(kw)
        assert not ga[2][T].any()                                                # the stacked bootstrap row gets zero


def test_identical_policies_give_is_one():
    """IS = 1 exactly: with clips at 1 the losses equal those of clips far above 1, bit for bit."""
    T, B, A = 9, 65, 376
    x = problem(T, B, A, 13)
    x["mu_b"], x["sigma_b"] = x["mu_t"].clone(), x["sigma_t"].clone()
    a, ga = run_gpu(on_gpu(x), clips=(1.0, 1.0, 1.0))
    b, gb = run_gpu(on_gpu(x), clips=(7.0, 7.0, 7.0))
    assert all(torch.equal(p, q) for p, q in zip(a + ga, b + gb))


# -------------------------------------------------------------------------------------------------- partial gradients
@pytest.mark.parametrize("nvf", [False, True], ids=["stacked", "next_value"])
def test_partial_gradients(nvf):
    T, B, A = 17, 65, 6
    x = problem(T, B, A, 17)
    done, flag = make_masks(T, B, "both", "bool", nvf, 19)
    _, full = run_gpu(on_gpu(x, nvf), done=done, flag=flag, nvf=nvf, has_w=True)
    for wrt in (("value",), ("mu_t",), ("sigma_t",), ("mu_t", "value")):
        d = on_gpu(x, nvf, grad=wrt)
        _, g = run_gpu(d, done=done, flag=flag, nvf=nvf, has_w=True, wrt=wrt)
        for k, got in zip(wrt, g):
            assert torch.equal(got, full[("mu_t", "sigma_t", "value").index(k)]), (wrt, k)


# ------------------------------------------------------------------------------------------------------------- others
@pytest.mark.parametrize("T,B,A", [(40, 257, 17), (17, 130, 64), (9, 65, 1024)])
def test_bitwise_repeatable(T, B, A):
    x = problem(T, B, A, 23)
    done, flag = make_masks(T, B, "both", "uint8", False, 29)
    runs = [run_gpu(on_gpu(x), done=done, flag=flag, has_w=True) for _ in range(2)]
    assert all(torch.equal(a, b) for a, b in zip(runs[0][0] + runs[0][1], runs[1][0] + runs[1][1]))


def test_graphed_step_replays_eager_bits():
    import hpc_rll
    from hpc_rll.rl_utils.vtrace import VTraceContinuous
    T, B, A = 16, 64, 8
    x = problem(T, B, A, 31)
    done, _ = make_masks(T, B, "done", "bool", False, 37)
    d = on_gpu(x)
    co = [torch.tensor([c], device=DEV) for c in CO]
    args = (d["mu_t"], d["sigma_t"], d["mu_b"], d["sigma_b"], d["action"], d["value"], d["reward"], done.to(DEV), d["weight"])
    mod = VTraceContinuous(T, B, A)
    step = hpc_rll.graphed(mod, *args, grad_outputs=co)
    for trial in range(2):
        if trial:
            with torch.no_grad():      # a new batch written INTO the static buffers
                y = problem(T, B, A, 32)
                for k in BIG + ("value", "reward"):
                    d[k].copy_(y[k])
        losses, grads = step()
        e = on_gpu({k: v.detach().cpu() for k, v in d.items()})
        ref, gref = run_gpu(e, done=done, has_w=True, module=mod)
        assert all(torch.equal(p.detach(), q) for p, q in zip(losses, ref)), trial
        assert all(torch.equal(p, q) for p, q in zip(grads, gref)), trial


@pytest.mark.parametrize("T,B,A,off", [(9, 65, 17, 1), (8, 64, 64, 1), (8, 64, 64, 3), (9, 65, 17, 2)])
def test_unaligned_views(T, B, A, off):
    """The five (T,B,A) inputs as contiguous views 4 / 8 / 12 bytes past a 16-byte boundary, between guard bands."""
    x = problem(T, B, A, 53 + A)
    done, flag = make_masks(T, B, "both", "bool", False, 59)
    check(x, f"T={T} B={B} A={A} off={off}", done=done, flag=flag, has_w=True, off=off)


def test_action_dimension_above_the_maximum_raises():
    import hpc_rl_utils
    z = lambda *s: torch.zeros(*s, device=DEV)   # noqa: E731
    T, B = 2, 3

    def call(A):
        return hpc_rl_utils.vtrace_continuous(z(T, B, A), z(T, B, A) + 1, z(T, B, A), z(T, B, A) + 1, z(T, B, A), z(T + 1, B),
                                              z(T, B))
    with pytest.raises(RuntimeError, match="not supported"):
        call(1025)
    assert len(call(1024)) == 3


def test_empty_batch():
    from hpc_rll.rl_utils.vtrace import vtrace_continuous
    A = 5
    mu = torch.zeros(0, 3, A, device=DEV, requires_grad=True)
    sg = torch.ones(0, 3, A, device=DEV, requires_grad=True)
    v = torch.zeros(1, 3, device=DEV, requires_grad=True)
    out = vtrace_continuous(mu, sg, mu.detach(), sg.detach(), mu.detach(), v, torch.zeros(0, 3, device=DEV))
    assert [o.item() for o in out] == [0.0, 0.0, 0.0]
    sum(out).sum().backward()
    assert mu.grad.shape == (0, 3, A) and sg.grad.shape == (0, 3, A) and v.grad.shape == (1, 3) and not v.grad.any()


# ------------------------------------------------------------------------------------------------ sharded, one rank
SH = dict(T=17, B=40, A=20, seed=61)


def _sharded_case(sharded):
    from hpc_rll.rl_utils.vtrace import VTraceContinuous
    T, B, A = SH["T"], SH["B"], SH["A"]
    x = problem(T, B, A, SH["seed"])
    done, flag = make_masks(T, B, "both", "bool", False, 67)
    return run_gpu(on_gpu(x), done=done, flag=flag, has_w=True, clips=(0.8, 1.2, 1.5),
                   module=VTraceContinuous(T, B, A, sharded=sharded))


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
        losses, grads = _sharded_case(True)
        q.put(("ok", [v.item() for v in losses], [g.cpu().numpy() for g in grads]))
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
    losses, grads = _sharded_case(False)
    assert [v.item() for v in losses] == res[1]
    assert all(np.array_equal(g.cpu().numpy(), r) for g, r in zip(grads, res[2]))
