"""GPU tier of TQC (``hpc_rll.rl_utils.tqc``, csrc/tqc.hip) against the fp64 oracle (tests/tqc_oracle.py) at the project's 1e-5:
every instantiation of the critic kernel at the edges of its lane mapping, the 4-byte variant, ties, NaN atoms, done rows, the
argument forms, the guarded C ABI, the actor half, and one full critic-and-actor step, eager and as a captured graph."""
import numpy as np
import pytest
import torch

import tqc_oracle as O
from conftest import grad_err, rel_err
from test_tqc_cpu import SHAPES

pytestmark = pytest.mark.gpu
TOL = 1e-5
KW = dict(alpha=0.2, gamma=0.97, kappa=1.0)
CAP_ROWS = 4 * 512   # four samples per workgroup, at most kFoldMaxGrid = 512 workgroups: one pass of the capped grid


DEV = torch.device("cuda:0")


def off16(t):   # the same values one float off 16-byte alignment
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    return buf[1:].view(t.shape).copy_(t)


def run(p, drop=0, weight=True, done="bool", alpha=None, grad=True, shift=None):
    """tqc_critic_loss on the GPU: dict(loss, td_error, target_atoms, grad_z, cfg) as numpy"""
    from hpc_rll.rl_utils import tqc
    import hpc_tqc
    t = {k: v.to(DEV) for k, v in p.items()}
    t["done"] = {"bool": t["done"], "u8": t["done"].to(torch.uint8), "f32": t["done"].float(), None: None}[done]
    if shift:
        t[shift] = off16(t[shift])
    z = t["z"].requires_grad_(grad)
    kw = dict(KW, alpha=KW["alpha"] if alpha is None else alpha)
    before = hpc_tqc.tqc_last_config()
    out = tqc.tqc_critic_loss(z, t["target_z"], t["nlp"], t["reward"], t["done"], t["weight"] if weight else None, drop=drop, **kw)
    if grad:
        (2.5 * out.critic_loss).sum().backward()
    cfg = hpc_tqc.tqc_last_config()
    return dict(loss=O.as_numpy(out.critic_loss), td_error=O.as_numpy(out.td_error), target_atoms=O.as_numpy(out.target_atoms),
                grad_z=O.as_numpy(z.grad) / 2.5 if grad else None, cfg=cfg, bwd_launches=cfg[6] - before[6])


def check(p, got, drop=0, weight=True, done=True, period=None):
    """against the oracle; with `period` the rows of p repeat and the oracle sees one period of them"""
    B = p["z"].shape[0]
    u = period or B
    q = {k: v[:u] for k, v in p.items()}
    want = O.critic(q["z"], q["target_z"], q["nlp"], q["reward"], q["done"] if done else None, q["weight"] if weight else None,
                    drop=drop, **KW)
    idx = np.arange(B) % u
    w = p["weight"].double().numpy() if weight else np.ones(B)
    want.update(td_error=want["td_error"][idx], target_atoms=want["target_atoms"][idx], grad_z=want["grad_z"][idx] * (u / B))
    want["loss"] = np.mean(w * want["td_error"]).reshape(1)
    for k in ("loss", "td_error", "target_atoms"):
        assert rel_err(want[k], got[k]) <= TOL, k
    assert grad_err(want["grad_z"], got["grad_z"], "grad_z") <= TOL
    return want


@pytest.mark.parametrize("weight", [True, False])
@pytest.mark.parametrize("B", [1, 3, 5, CAP_ROWS + 1])
@pytest.mark.parametrize("Mt,Nt,drop,M,N", SHAPES)
def test_shape_sweep(Mt, Nt, drop, M, N, B, weight):
    period = min(B, 5)               # past five rows the rows repeat, and the oracle is evaluated on one period
    p = {k: v[torch.arange(B) % period] for k, v in O.problem(period, Mt, Nt, M, N).items()}
    got = run(p, drop, weight)
    check(p, got, drop, weight, period=period)
    R, lw = next(r for r in (1, 2, 4, 8, 16) if r * 64 >= Mt * Nt), 4 if (Mt * Nt) % 4 == 0 else 1
    assert got["cfg"][1:6] == [1, R, lw, min(512, (B + 3) // 4), 3 if weight else 2]


@pytest.mark.parametrize("shift", ["z", "target_z", "nlp", "reward", "weight"])
def test_each_operand_off_16_bytes_takes_the_4_byte_variant(shift):
    p = O.problem(5, 4, 64, 4, 64)
    base, got = run(p, 37), run(p, 37, shift=shift)
    assert base["cfg"][2:4] == [4, 4] and got["cfg"][2:4] == [4, 1]
    assert all(np.array_equal(base[k], got[k]) for k in ("loss", "td_error", "target_atoms", "grad_z"))


@pytest.mark.parametrize("case", ["all_equal", "across_the_cut", "signed_zeros"])
def test_ties(case):
    p = O.problem(3, 5, 25, 5, 25)
    if case == "all_equal":
        p["target_z"][1] = 0.75
    elif case == "across_the_cut":   # the 115th and 116th smallest atoms of row 1 are one value: either copy may be kept
        row = p["target_z"][1].reshape(-1)
        order = torch.argsort(row)
        row[order[115]] = row[order[114]]
    else:
        p["target_z"][1].reshape(-1)[[3, 40, 77, 101]] = torch.tensor([0.0, -0.0, -0.0, 0.0])
    check(p, run(p, 10), 10)


def test_nan_atoms_and_done_rows():
    p = O.problem(5, 5, 25, 5, 25)
    p["done"] = torch.tensor([False, True, False, True, False])
    clean = run(p, 10)
    p["target_z"][0].reshape(-1)[[5, 60, 124]] = float("nan")          # fewer than drop: cut first, the row stays finite
    q = dict(p, target_z=torch.nan_to_num(p["target_z"], nan=float("inf")))
    got = run(p, 10)
    check(q, got, 10)
    assert np.array_equal(got["target_atoms"][[1, 3]], np.repeat(p["reward"].numpy()[[1, 3], None], 115, 1))   # done = 1
    p["target_z"][2].reshape(-1)[:11] = float("nan")                   # more than drop
    bad = run(p, 10)
    assert np.isnan(bad["td_error"][2]) and np.isnan(bad["loss"]).all()
    assert np.array_equal(np.delete(bad["td_error"], [0, 2]), np.delete(clean["td_error"], [0, 2]))


def test_repeats_forms_and_requires_grad():
    p = O.problem(7, 5, 25, 5, 25)
    a, b = run(p, 10), run(p, 10)
    dev_alpha = run(p, 10, alpha=torch.tensor([KW["alpha"]], device=DEV))
    for k in ("loss", "td_error", "target_atoms", "grad_z"):
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], dev_alpha[k]), k
    assert a["cfg"][5] == 3 and dev_alpha["cfg"][5] == 3 | 64 and a["bwd_launches"] == 1
    for done in ("u8", "f32"):
        got = run(p, 10, done=done)
        assert np.array_equal(a["loss"], got["loss"]) and np.array_equal(a["grad_z"], got["grad_z"]), done
    check(p, run(p, 10, done=None), 10, done=False)
    frozen = run(p, 10, grad=False)
    assert frozen["bwd_launches"] == 0 and np.array_equal(frozen["loss"], a["loss"])


@pytest.mark.parametrize("Mt,Nt,status", [(5, 25, 0), (25, 41, -3)])
def test_c_abi_writes_only_its_outputs(Mt, Nt, status):
    import cabi
    B, M, N, drop = 3, 5, 25, 10
    p = {k: v.to(DEV) for k, v in O.problem(B, Mt, Nt, M, N).items()}
    sizes = dict(loss=1, td=B, atoms=B * (Mt * Nt - drop), ws=cabi.lib.hpc_rll_tqc_workspace_floats(B, M * N), grad=B * M * N)
    guard = {k: torch.full((n + 8,), -7.0, device=DEV) for k, n in sizes.items()}   # four poisoned floats on either side
    o = {k: g[4:-4] for k, g in guard.items()}
    st = cabi.lib.hpc_rll_tqc_critic_forward(cabi.ptr(p["z"]), cabi.ptr(p["target_z"]), cabi.ptr(p["nlp"]), cabi.ptr(p["reward"]),
                                             None, 0, None, None, 0.2, cabi.ptr(o["loss"]), cabi.ptr(o["td"]), cabi.ptr(o["atoms"]),
                                             cabi.ptr(o["ws"]), B, M, N, Mt, Nt, drop, 0.97, 1.0, 1.0 / B, cabi.stream_ptr(DEV))
    assert st == status
    if status == 0:
        cabi.call("hpc_rll_tqc_critic_backward", DEV, cabi.ptr(torch.ones(1, device=DEV)), cabi.ptr(o["ws"]), cabi.ptr(o["grad"]), B, M, N)
    torch.cuda.synchronize()
    for k, g in guard.items():
        assert (g[:4] == -7).all() and (g[-4:] == -7).all(), k
        assert bool((o[k] == -7).all()) if status else k == "ws" or bool((o[k] != -7).all()), k


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("M,N", [(1, 1), (1, 63), (5, 25), (8, 128)])
def test_policy_half(M, N, B):
    from hpc_rll.rl_utils import tqc
    p = O.problem(B, 1, 1, M, N)
    want = O.policy(p["lp"], p["new_z"], KW["alpha"])
    for need_lp, need_z in [(True, True), (True, False), (False, True)]:
        lp, nz = p["lp"].to(DEV).requires_grad_(need_lp), p["new_z"].to(DEV).requires_grad_(need_z)
        out = tqc.tqc_policy_loss(lp, nz, KW["alpha"])
        out.policy_loss.sum().backward()
        assert rel_err(want["policy_loss"], O.as_numpy(out.policy_loss)) <= TOL
        assert rel_err(want["entropy"], O.as_numpy(out.entropy)) <= TOL and not out.entropy.requires_grad
        assert (lp.grad is not None) == need_lp and (nz.grad is not None) == need_z
        assert not need_lp or grad_err(want["grad_lp"], O.as_numpy(lp.grad), "grad_lp") <= TOL
        assert not need_z or grad_err(want["grad_nz"], O.as_numpy(nz.grad), "grad_nz") <= TOL


def _step(t, mod, log_alpha):
    from hpc_rll.rl_utils import tqc
    for k in ("z", "mu", "sigma", "la"):
        t[k].grad = None
    action, lp = tqc.tanh_gaussian_rsample(t["mu"], t["sigma"], t["eps"])
    new_z = t["new_z"] + action.sum(-1).reshape(-1, 1, 1)   # a stand-in critic: the quantiles shift with the action
    out = mod(t["z"], t["target_z"], t["nlp"], t["reward"], lp, new_z, done=t["done"], weight=t["weight"], drop=10,
              alpha=log_alpha.detach().exp(), gamma=KW["gamma"])
    a_loss = tqc.sac_alpha_loss(log_alpha, out.entropy, -3.0)
    (out.critic_loss + out.policy_loss + a_loss).sum().backward()
    return [out.critic_loss, out.policy_loss, out.entropy, out.td_error, a_loss, t["z"].grad, t["mu"].grad, t["sigma"].grad,
            log_alpha.grad]


def test_full_step_eager_against_fp64_and_as_a_captured_graph():
    from hpc_rll.rl_utils import tqc
    B, A = 6, 3
    p = O.problem(B, 5, 25, 5, 25, salt=3)
    g = torch.Generator().manual_seed(9)
    p.update(mu=0.3 * torch.randn(B, A, generator=g), sigma=torch.rand(B, A, generator=g) + 0.5, eps=torch.randn(B, A, generator=g),
             la=torch.tensor([-1.2]))
    def leaves(dt, device):   # noqa: E306
        t = {k: (v.to(dt) if v.is_floating_point() else v).to(device) for k, v in p.items()}
        for k in ("z", "mu", "sigma", "la"):
            t[k].requires_grad_(True)
        return t
    t = leaves(torch.float32, DEV)
    eager = [O.as_numpy(x).copy() for x in _step(t, tqc.TQC(), t["la"])]
    d = leaves(torch.float64, "cpu")
    u = d["mu"] + d["sigma"] * d["eps"]
    lp = (torch.distributions.Normal(d["mu"], d["sigma"]).log_prob(u) - 2 * (np.log(2.0) - u - torch.nn.functional.softplus(-2 * u))).sum(-1)
    alpha = d["la"].detach().exp().item()
    c = O.critic(d["z"], d["target_z"], d["nlp"], d["reward"], d["done"], d["weight"], alpha=alpha, gamma=KW["gamma"], drop=10)
    new_z = d["new_z"] + torch.tanh(u).sum(-1).reshape(-1, 1, 1)
    pol = (alpha * lp - new_z.mean(dim=(1, 2))).mean()
    a_loss = -(d["la"] * (lp.detach().mean() - 3.0))
    (pol + a_loss.sum()).backward()
    want = [c["loss"], pol.detach().reshape(1), -lp.detach().mean().reshape(1), c["td_error"], a_loss.detach(), c["grad_z"],
            d["mu"].grad, d["sigma"].grad, d["la"].grad]
    for i, (w, e) in enumerate(zip(want, eager)):
        assert (grad_err if i >= 5 else rel_err)(np.asarray(w), e) <= TOL, i
    s = leaves(torch.float32, DEV)
    mod, side = tqc.TQC(), torch.cuda.Stream()
    with torch.cuda.stream(side):
        _step(s, mod, s["la"])                # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = _step(s, mod, s["la"])
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        for i, (o, e) in enumerate(zip(outs, eager)):
            assert np.array_equal(O.as_numpy(o), e), i
