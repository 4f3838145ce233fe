"""Retrace(lambda) (``hpc_rll.rl_utils.retrace``: ``retrace`` / ``retrace_loss`` / ``Retrace``, csrc/retrace.hip) on an MI355X
(``-m gpu``).

The oracle is this file's own fp64 restatement of the recurrence, a plain Python loop over ``t``::

    qa_t = q[t,b,a_t],  c_t = lambda * min(1, ratio_t),  Q_T = v_T
    Q_t  = r_t + gamma * w_t * (c_{t+1} * (Q_{t+1} - qa_{t+1}) + v_{t+1}),      the c*(Q - qa) term := 0 at t+1 = T
    loss = scale * 0.5 * sum_{t<T,b} lw * (Q_t - qa_t)^2,   grad[t,b,n] = scale * lw * (qa_t - Q_t) * [n = a_t],  row T zero

with ``v = sum softmax(target) * q`` and ``ratio = exp(log pi(a) - log mu(a))`` in the fused form.  Bars are the project's:
``rel_err <= 1e-5`` on the loss, on ``q_retraces`` and on ``v_pred``, ``grad_err <= 2e-5`` on ``grad_q_values``.  Before any
launch the host asserts that the share of ``ratio > 1`` lies in (0.05, 0.95), so both branches of the ``min`` run.

Every launch is followed by ``hpc_rll_retrace_last_config``: exactly one more launch, and the configuration, form, grid and
finalisation written here as LITERALS (the table of tests/test_masked_upgo_gpu.py: V = 1, LC = 8; NW = 16 for fewer than 512
workgroups of 64 columns, halved while NW > ceil(T / 8); SUB 2 / 4 / 8 for narrow batches with long unrolls; the loss folded
into the launch up to 512 workgroups, else the finalize launch).  In the record, ``mm`` bit 0 = weights given, bit 1 =
loss_weight given, ``nvf`` 1 = the drop-in form ``retrace`` (which has no loss: ``fin`` 0, and no loss_weight: two of the four
null combinations).  A wave's chunks count down from T: [T-8, T), [T-16, T-8), ...
"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import grad_err, rel_err
from guarded import GuardedF32

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 1e-5
N = 3
GAMMA = 0.99
FIELDS = ("count", "v", "lc", "nw", "sub", "ntl", "mt", "mm", "nvf", "grid", "fin")
NONE, FOLD, FINALIZE = 0, 1, 2
# (T, B, (V, LC, NW, SUB), grid, finalisation of the fused form, last tile)
CELLS = [
    (5, 128, (1, 8, 1, 1), 2, FOLD, "whole"), (5, 100, (1, 8, 1, 1), 2, FOLD, "ragged"),
    (12, 128, (1, 8, 2, 1), 2, FOLD, "whole"), (12, 100, (1, 8, 2, 1), 2, FOLD, "ragged"),
    (30, 128, (1, 8, 4, 1), 2, FOLD, "whole"), (30, 100, (1, 8, 4, 1), 2, FOLD, "ragged"),
    (100, 128, (1, 8, 8, 1), 2, FOLD, "whole"), (100, 100, (1, 8, 8, 1), 2, FOLD, "ragged"),
    (128, 128, (1, 8, 16, 1), 2, FOLD, "whole"), (121, 100, (1, 8, 16, 1), 2, FOLD, "ragged"),
    (300, 1024, (1, 8, 16, 2), 32, FOLD, "whole"), (300, 1000, (1, 8, 16, 2), 32, FOLD, "ragged"),
    (600, 96, (1, 8, 16, 4), 6, FOLD, "whole"), (600, 100, (1, 8, 16, 4), 7, FOLD, "ragged"),
    (1024, 64, (1, 8, 16, 8), 8, FOLD, "whole"), (1024, 60, (1, 8, 16, 8), 8, FOLD, "ragged"),
    (5, 33000, (1, 8, 1, 1), 516, FINALIZE, "ragged"),           # 516 workgroups: past the fold
]
CONFIGS = sorted({c[2] for c in CELLS})
assert len(CONFIGS) == 8
# (form, weights given, loss_weight given): the drop-in form has no loss_weight
COMBOS = [("retrace", 0, 0), ("retrace", 1, 0)] + [("retrace_loss", hw, hlw) for hw in (0, 1) for hlw in (0, 1)]
COVER = {}     # (cfg, combo) -> {"whole", "ragged"}
FIN = set()


# ---------------------------------------------------------------------------------------------------------------------
# dispatch record
# ---------------------------------------------------------------------------------------------------------------------
def last():
    import cabi
    out = (ctypes.c_int * 11)()
    assert cabi.lib.hpc_rll_retrace_last_config(out) == 0
    return dict(zip(FIELDS, out))


class launches:
    """The body launches the Retrace scan exactly once, and the record names the literal instantiation."""

    def __init__(self, cfg, grid, fin, combo, what=""):
        form, hw, hlw = combo
        drop_in = form == "retrace"
        self.want = dict(v=cfg[0], lc=cfg[1], nw=cfg[2], sub=cfg[3], ntl=0, mt=0, mm=hw | (hlw << 1), nvf=int(drop_in),
                         grid=grid, fin=NONE if drop_in else fin)
        self.what = what

    def __enter__(self):
        self.want["count"] = last()["count"] + 1

    def __exit__(self, et, ev, tb):
        if et is None:
            rec = last()
            assert rec == self.want, (self.what, "ran", rec, "expected", self.want)


def cfg_of(T, B):
    """The literal row of CELLS for a shape used elsewhere in this file."""
    for t, b, cfg, grid, fin, _ in CELLS:
        if (t, b) == (T, B):
            return cfg, grid, fin
    raise KeyError((T, B))


# ---------------------------------------------------------------------------------------------------------------------
# fp64 oracle, written from the recurrence in the module docstring
# ---------------------------------------------------------------------------------------------------------------------
def _f64(x):
    return x.detach().to("cpu", torch.float64)


def recurrence64(r, w, v, c, qa, gamma):
    """r, w, c, qa (T,B), v (T+1,B), all fp64 on the host -> Q (T+1,B)."""
    T = r.shape[0]
    Q = torch.empty_like(v)
    Q[T] = v[T]
    for t in range(T - 1, -1, -1):
        tail = c[t + 1] * (Q[t + 1] - qa[t + 1]) if t + 1 < T else 0.0
        Q[t] = r[t] + gamma * w[t] * (tail + v[t + 1])
    return Q


def heads64(q, tgt, beh, a):
    """-> v (T+1,B), qa (T,B), ratio (T,B) in fp64 from the logits."""
    q, tgt, beh = _f64(q), _f64(tgt), _f64(beh)
    T = beh.shape[0]
    idx = a.detach().cpu().unsqueeze(-1)
    logpi = torch.log_softmax(tgt, dim=-1)
    v = (logpi.exp() * q).sum(-1)
    d = logpi[:T].gather(-1, idx).squeeze(-1) - torch.log_softmax(beh, dim=-1).gather(-1, idx).squeeze(-1)
    return v, q[:T].gather(-1, idx).squeeze(-1), d.exp()


def _clip_share(ratio, what):
    """Both branches of min(1, ratio) must run: asserted on the host before anything is launched."""
    share = float((ratio > 1.0).to(torch.float64).mean())
    assert 0.05 < share < 0.95, f"{what}: the share of ratio > 1 is {share:.3f}"
    return share


def oracle_loss(p, w, lw, gamma=GAMMA, lam=1.0, scale=None, check_clip=True):
    """The fused form -> dict(loss, Q, v, grad) in fp64 (numpy)."""
    v, qa, ratio = heads64(p["q"], p["tgt"], p["beh"], p["a"])
    T, B = qa.shape
    if check_clip:
        _clip_share(ratio, f"T={T} B={B}")
    ones = torch.ones_like(qa)
    w64 = _f64(w) if w is not None else ones
    lw64 = _f64(lw) if lw is not None else ones
    Q = recurrence64(_f64(p["r"]), w64, v, lam * ratio.clamp(max=1.0), qa, gamma)
    scale = 1.0 / (T * B) if scale is None else scale
    loss = scale * 0.5 * (lw64 * (Q[:T] - qa) ** 2).sum()
    grad = torch.zeros(T + 1, B, p["q"].shape[2], dtype=torch.float64)
    grad[:T].scatter_(-1, p["a"].detach().cpu().unsqueeze(-1), (scale * lw64 * (qa - Q[:T])).unsqueeze(-1))
    return dict(loss=float(loss), Q=Q.numpy(), v=v.numpy(), grad=grad.numpy(), ratio=ratio)


def oracle_drop_in(p, w, gamma=GAMMA, lam=1.0):
    """The drop-in form -> Q (T+1,B,1) in fp64 (numpy) from the given v_pred and ratio."""
    idx = p["a"].detach().cpu().unsqueeze(-1)
    T = idx.shape[0]
    ratio = _f64(p["ratio"]).gather(-1, idx).squeeze(-1)
    _clip_share(ratio, f"drop-in T={T} B={idx.shape[1]}")
    qa = _f64(p["q"])[:T].gather(-1, idx).squeeze(-1)
    w64 = _f64(w) if w is not None else torch.ones_like(qa)
    Q = recurrence64(_f64(p["r"]), w64, _f64(p["vp"]).squeeze(-1), lam * ratio.clamp(max=1.0), qa, gamma)
    return Q.unsqueeze(-1).numpy()


# ---------------------------------------------------------------------------------------------------------------------
# problems and runners
# ---------------------------------------------------------------------------------------------------------------------
def _gen(T, B, salt=0):
    return torch.Generator(device=DEV).manual_seed(T * 1000003 + B + 7919 * salt)


def _np(x):
    return x.detach().cpu().numpy()


def _problem(T, B, n=N, salt=0):
    """randn inputs; weights are 1 - done with 5 % of the steps done; loss_weight in [0.5, 1.5)."""
    g = _gen(T, B, salt)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)   # noqa: E731
    return dict(q=rn(T + 1, B, n), tgt=rn(T + 1, B, n), beh=rn(T, B, n), a=torch.randint(0, n, (T, B), device=DEV, generator=g),
                r=rn(T, B), w=(torch.rand(T, B, device=DEV, generator=g) >= 0.05).to(torch.float32),
                lw=torch.rand(T, B, device=DEV, generator=g) + 0.5, vp=rn(T + 1, B, 1), ratio=rn(T, B, n).exp(), g=g)


def _run_loss(p, w=None, lw=None, gamma=GAMMA, lam=1.0):
    """retrace_loss -> (loss (1,), q_retraces (T+1,B), v_pred (T+1,B), grad_q_values (T+1,B,N))."""
    from hpc_rll.rl_utils.retrace import retrace_loss
    q = p["q"].detach().requires_grad_(True)
    loss, Q, v = retrace_loss(q, p["tgt"], p["beh"], p["a"], p["r"], w, lw, gamma, lam)
    assert loss.shape == (1,) and Q.shape == v.shape == p["q"].shape[:2] and not Q.requires_grad and not v.requires_grad
    (gq,) = torch.autograd.grad(loss, q)
    return loss.detach(), Q, v, gq


def _run_drop_in(p, w=None, gamma=GAMMA, lam=1.0):
    from hpc_rll.rl_utils.retrace import retrace
    Q = retrace(p["q"], p["vp"], p["r"], p["a"], w, p["ratio"], gamma, lam)
    assert Q.shape == p["vp"].shape and not Q.requires_grad
    return Q


def _parity(got, want, what):
    loss, Q, v, gq = got
    e_l, e_q, e_v = rel_err(want["loss"], loss.item()), rel_err(want["Q"], _np(Q)), rel_err(want["v"], _np(v))
    print(f"{what}: loss {loss.item():.9g} oracle {want['loss']:.9g} rel_err {e_l:.3g}; q_retraces {e_q:.3g}; v_pred {e_v:.3g}")
    e_g = grad_err(want["grad"], _np(gq), "grad_q_values")
    print(f"{what}: grad_err {e_g:.3g}")
    assert e_l <= TOL, (what, "loss", want["loss"], loss.item())
    assert e_q <= TOL, (what, "q_retraces", e_q)
    assert e_v <= TOL, (what, "v_pred", e_v)
    assert e_g <= 2 * TOL, (what, "grad_q_values", e_g)


def _parity_q(Q, want, what):
    e = rel_err(want, _np(Q))
    print(f"{what}: q_retraces rel_err {e:.3g}")
    assert e <= TOL, (what, "q_retraces", e)


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------------------------
# every configuration, both forms, every null combination of weights and loss_weight; N = 3
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,B,cfg,grid,fin,kind", CELLS)
def test_every_configuration_both_forms(T, B, cfg, grid, fin, kind):
    tile = 64 // cfg[3]
    assert (B % tile == 0) == (kind == "whole")
    p = _problem(T, B)
    for combo in COMBOS:
        form, hw, hlw = combo
        w, lw = (p["w"] if hw else None), (p["lw"] if hlw else None)
        what = f"{form} T={T} B={B} weights={hw} loss_weight={hlw}"
        if form == "retrace":
            want = oracle_drop_in(p, w)
            with launches(cfg, grid, fin, combo, what):
                Q = _run_drop_in(p, w)
            _parity_q(Q, want, what)
        else:
            want = oracle_loss(p, w, lw)
            with launches(cfg, grid, fin, combo, what):
                got = _run_loss(p, w, lw)
            _parity(got, want, what)
            FIN.add(fin)
        COVER.setdefault((cfg, combo), set()).add(kind)


# ---------------------------------------------------------------------------------------------------------------------
# action counts: every head mapping (4-byte rows for N % 4 != 0, 16-byte rows otherwise, 1 .. 64 lanes per row)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 4, 6, 18, 64, 100, 512, 1000, 1024])
def test_action_counts(n):
    T, B = 12, 100
    cfg, grid, fin = cfg_of(T, B)
    p = _problem(T, B, n=n, salt=1)
    want = oracle_loss(p, p["w"], p["lw"], check_clip=n > 1)
    with launches(cfg, grid, fin, ("retrace_loss", 1, 1), f"N={n}"):
        got = _run_loss(p, p["w"], p["lw"])
    _parity(got, want, f"retrace_loss N={n}")
    if n == 1:      # one action: v = q, ratio = 1, and the gradient lands in the only column
        assert bool((want["ratio"] == 1.0).all())
        assert torch.equal(got[2], p["q"][..., 0]), "N = 1: v_pred is not q_values"
        assert bool((got[3][:T, :, 0] != 0).any()) and not bool(got[3][T].any())
    with launches(cfg, grid, fin, ("retrace", 1, 0), f"N={n}"):
        Q = _run_drop_in(p, p["w"])
    _parity_q(Q, oracle_drop_in(p, p["w"]), f"retrace N={n}")


def _host_problem(T, B, seed, n=N):
    """A problem drawn on the host (the same numbers on every machine), then moved to the device."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    p = dict(q=rn(T + 1, B, n), tgt=rn(T + 1, B, n), beh=rn(T, B, n), a=torch.randint(0, n, (T, B), generator=g), r=rn(T, B))
    return {k: x.to(DEV) for k, x in p.items()}


SINGLE_SEEDS = tuple(range(8))


def test_single_sample_takes_both_branches_of_the_clip():
    """T = B = 1 cannot have a share of ratio > 1 inside (0.05, 0.95): eight seeds, and both states must occur across them
    (asserted on the host before the first launch).  T = 2, B = 1 runs too: there c_1 enters Q_0."""
    states = {seed: bool(oracle_loss(_host_problem(1, 1, seed), None, None, check_clip=False)["ratio"][0, 0] > 1.0)
              for seed in SINGLE_SEEDS}
    assert set(states.values()) == {True, False}, states
    for T in (1, 2):
        for seed in SINGLE_SEEDS:
            p = _host_problem(T, 1, seed)
            want = oracle_loss(p, None, None, check_clip=False)
            with launches((1, 8, 1, 1), 1, FOLD, ("retrace_loss", 0, 0), f"T={T} B=1 seed {seed}"):
                got = _run_loss(p)
            _parity(got, want, f"T={T} B=1 seed {seed} ratio > 1: {(want['ratio'] > 1.0).flatten().tolist()}")


# ---------------------------------------------------------------------------------------------------------------------
# chunk edges: weights = 0 at the first and the last step of every chunk [T-8, T), [T-16, T-8), ..., at t = T-1 and t = 0
# ---------------------------------------------------------------------------------------------------------------------
EDGE_CFG = {8: (1, 8, 1, 1), 9: (1, 8, 2, 1), 16: (1, 8, 2, 1), 17: (1, 8, 2, 1), 121: (1, 8, 16, 1)}


@pytest.mark.parametrize("B", [64, 100])
@pytest.mark.parametrize("T", [8, 9, 16, 17, 121])
def test_zero_weights_at_chunk_edges(T, B):
    p = _problem(T, B, salt=2)
    steps = sorted({t for k in range(0, T, 8) for t in (T - k - 1, T - k - 8) if t >= 0} | {0, T - 1})
    w = torch.ones(T, B, device=DEV)
    w[steps] = 0.0
    cfg, grid = EDGE_CFG[T], (B + 63) // 64
    want = oracle_loss(p, w, None)
    with launches(cfg, grid, FOLD, ("retrace_loss", 1, 0), f"edges T={T} B={B}"):
        got = _run_loss(p, w)
    _parity(got, want, f"zero weights at chunk edges T={T} B={B}")
    assert torch.equal(got[1][steps], p["r"][steps]), "a zero weight must give Q_t = r_t exactly"
    with launches(cfg, grid, FOLD, ("retrace", 1, 0), f"edges T={T} B={B}"):
        Q = _run_drop_in(p, w)
    _parity_q(Q, oracle_drop_in(p, w), f"drop-in, zero weights at chunk edges T={T} B={B}")
    assert torch.equal(Q[:T][steps].squeeze(-1), p["r"][steps])


@pytest.mark.parametrize("B", [64, 100])
@pytest.mark.parametrize("T", [1, 2, 3])
def test_short_unrolls(T, B):
    p = _problem(T, B, salt=3)
    cfg, grid = (1, 8, 1, 1), (B + 63) // 64
    want = oracle_loss(p, p["w"], p["lw"])
    with launches(cfg, grid, FOLD, ("retrace_loss", 1, 1), f"short T={T} B={B}"):
        got = _run_loss(p, p["w"], p["lw"])
    _parity(got, want, f"short unroll T={T} B={B}")
    if T == 1:      # Q_0 = r + gamma w v_1
        q0 = _f64(p["r"])[0] + GAMMA * _f64(p["w"])[0] * torch.from_numpy(want["v"])[1]
        assert rel_err(q0.numpy(), _np(got[1][0])) <= TOL
    with launches(cfg, grid, FOLD, ("retrace", 0, 0), f"short T={T} B={B}"):
        Q = _run_drop_in(p)
    _parity_q(Q, oracle_drop_in(p, None), f"drop-in short unroll T={T} B={B}")


@pytest.mark.parametrize("T,B", [(30, 100), (300, 1000)])
def test_lambda(T, B):
    cfg, grid, fin = cfg_of(T, B)
    p = _problem(T, B, salt=4)
    # lambda_ = 0: every trace is cut, Q_t = r_t + gamma w_t v_{t+1}
    want = oracle_loss(p, p["w"], None, lam=0.0)
    one_step = _f64(p["r"]) + GAMMA * _f64(p["w"]) * torch.from_numpy(want["v"])[1:]
    assert np.array_equal(one_step.numpy(), want["Q"][:T])
    with launches(cfg, grid, fin, ("retrace_loss", 1, 0), f"lambda 0 T={T} B={B}"):
        got = _run_loss(p, p["w"], lam=0.0)
    _parity(got, want, f"lambda_=0 T={T} B={B}")
    assert rel_err(one_step.numpy(), _np(got[1][:T])) <= TOL
    for lw in (None, p["lw"]):
        with launches(cfg, grid, fin, ("retrace_loss", 1, int(lw is not None)), f"lambda 0.7 T={T} B={B}"):
            got = _run_loss(p, p["w"], lw, lam=0.7)
        _parity(got, oracle_loss(p, p["w"], lw, lam=0.7), f"lambda_=0.7 T={T} B={B}")
    with launches(cfg, grid, fin, ("retrace", 1, 0), f"lambda 0.7 T={T} B={B}"):
        Q = _run_drop_in(p, p["w"], lam=0.7)
    _parity_q(Q, oracle_drop_in(p, p["w"], lam=0.7), f"drop-in lambda_=0.7 T={T} B={B}")


@pytest.mark.parametrize("T,B,n", [(30, 100, 3), (121, 100, 18), (600, 96, 4)])
def test_the_two_forms_agree(T, B, n):
    """retrace, fed v_pred and ratio computed in fp64 from the same logits and rounded to fp32, gives retrace_loss's targets."""
    cfg, grid, fin = cfg_of(T, B)
    p = _problem(T, B, n=n, salt=5)
    tgt, beh = _f64(p["tgt"]), _f64(p["beh"])
    logpi = torch.log_softmax(tgt, dim=-1)
    p["vp"] = (logpi.exp() * _f64(p["q"])).sum(-1, keepdim=True).to(torch.float32).to(DEV)
    p["ratio"] = (logpi[:T] - torch.log_softmax(beh, dim=-1)).exp().to(torch.float32).to(DEV)
    with launches(cfg, grid, fin, ("retrace_loss", 1, 0)):
        _, Q_fused, v, _ = _run_loss(p, p["w"])
    with launches(cfg, grid, fin, ("retrace", 1, 0)):
        Q = _run_drop_in(p, p["w"])
    e = rel_err(_np(Q.squeeze(-1)).astype(np.float64), _np(Q_fused))
    print(f"T={T} B={B} N={n}: drop-in vs fused q_retraces rel_err {e:.3g}")
    assert e <= TOL
    assert rel_err(_np(p["vp"].squeeze(-1)).astype(np.float64), _np(v)) <= TOL


# ---------------------------------------------------------------------------------------------------------------------
# bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,B", [(30, 100), (300, 1000), (1024, 60), (5, 33000)])
def test_none_and_all_ones_give_the_same_bits_and_runs_repeat(T, B):
    cfg, grid, fin = cfg_of(T, B)
    p = _problem(T, B, salt=6)
    ones = torch.ones(T, B, device=DEV)
    with launches(cfg, grid, fin, ("retrace_loss", 0, 0)):
        plain = _run_loss(p)
    with launches(cfg, grid, fin, ("retrace_loss", 1, 0)):
        assert _same(_run_loss(p, ones), plain), "weights=None and all-ones weights differ"
    with launches(cfg, grid, fin, ("retrace_loss", 0, 1)):
        assert _same(_run_loss(p, None, ones), plain), "loss_weight=None and all-ones loss_weight differ"
    with launches(cfg, grid, fin, ("retrace_loss", 1, 1)):
        assert _same(_run_loss(p, ones, ones), plain)
    with launches(cfg, grid, fin, ("retrace_loss", 1, 1)):
        a = _run_loss(p, p["w"], p["lw"])
    with launches(cfg, grid, fin, ("retrace_loss", 1, 1)):
        assert _same(_run_loss(p, p["w"], p["lw"]), a), "two runs differ"
    with launches(cfg, grid, fin, ("retrace", 0, 0)):
        Q = _run_drop_in(p)
    with launches(cfg, grid, fin, ("retrace", 1, 0)):
        assert torch.equal(_run_drop_in(p, ones), Q)
    with launches(cfg, grid, fin, ("retrace", 0, 0)):
        assert torch.equal(_run_drop_in(p), Q), "two runs differ"


@pytest.mark.parametrize("T,B,n", [(30, 100, 3), (12, 100, 18), (5, 128, 64)])
def test_gradient_structure(T, B, n):
    p = _problem(T, B, n=n, salt=7)
    loss, _, _, gq = _run_loss(p, p["w"], p["lw"])
    assert not bool(gq[T].any()), "row T of the gradient is not zero"
    onehot = torch.zeros(T, B, n, dtype=torch.bool, device=DEV).scatter_(-1, p["a"].unsqueeze(-1), True)
    assert not bool(gq[:T][~onehot].any()), "a non-action column of the gradient is not zero"
    assert bool((gq[:T][onehot] != 0).any()) and loss.item() > 0
    lw = p["lw"].clone()
    lw[:, ::2] = 0.0
    _, _, _, gz = _run_loss(p, p["w"], lw)
    assert not bool(gz[:, ::2].any()) and bool(gz[:, 1::2].any())
    zl, Q, v, gz = _run_loss(p, p["w"], torch.zeros(T, B, device=DEV))
    assert zl.item() == 0.0 and not bool(gz.any()), "a zero loss_weight must zero the loss and the gradient"
    want = oracle_loss(p, p["w"], None)
    assert rel_err(want["Q"], _np(Q)) <= TOL and rel_err(want["v"], _np(v)) <= TOL      # the targets do not depend on it


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,B", [(30, 100), (600, 100), (5, 33000)])
def test_c_abi_writes_nothing_past_its_outputs(T, B):
    """The C entry points on guarded buffers at a ragged B: every output keeps its guard bands, every element of the
    outputs and of the gradient is written, and the bits are the Python API's."""
    import cabi
    L = cabi.lib
    cfg, grid, fin = cfg_of(T, B)
    p = _problem(T, B, salt=8)
    nws = L.hpc_rll_retrace_workspace_floats(T, B)
    assert nws >= 3 * T * B
    loss, Q, v = GuardedF32(1, 1, 0, DEV), GuardedF32(T + 1, B, 0, DEV), GuardedF32(T + 1, B, 0, DEV)
    ws, grad = GuardedF32(1, nws, 0, DEV), GuardedF32(T + 1, B * N, 0, DEV)
    with launches(cfg, grid, fin, ("retrace_loss", 1, 1), f"C ABI T={T} B={B}"):
        st = L.hpc_rll_retrace_loss_forward(p["q"].data_ptr(), p["tgt"].data_ptr(), p["beh"].data_ptr(), p["a"].data_ptr(),
                                            p["r"].data_ptr(), p["w"].data_ptr(), p["lw"].data_ptr(), loss.t.data_ptr(),
                                            Q.t.data_ptr(), v.t.data_ptr(), ws.t.data_ptr(), T, B, N, GAMMA, 1.0,
                                            1.0 / (T * B), cabi.stream_ptr(DEV))
    assert st == 0, st
    st = L.hpc_rll_retrace_loss_backward(None, p["a"].data_ptr(), ws.t.data_ptr(), grad.t.data_ptr(), T, B, N,
                                         cabi.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert st == 0, st
    for name, buf in (("loss", loss), ("q_retraces", Q), ("v_pred", v), ("ws", ws), ("grad", grad)):
        buf.check(f"T={T} B={B} {name}")
    for name, buf in (("loss", loss), ("q_retraces", Q), ("v_pred", v), ("grad", grad)):
        buf.assert_written(name)
    assert not bool(torch.isnan(ws.t[0, :3 * T * B]).any()), "delta / qa / c were not all written"
    ref = _run_loss(p, p["w"], p["lw"])
    assert torch.equal(ref[0], loss.t.view(1)) and torch.equal(ref[1], Q.t) and torch.equal(ref[2], v.t)
    assert torch.equal(ref[3], grad.t.view(T + 1, B, N))
    # the drop-in form: q_retraces and its 2*T*B workspace
    Qd, wsd = GuardedF32(T + 1, B, 0, DEV), GuardedF32(1, 2 * T * B, 0, DEV)
    with launches(cfg, grid, fin, ("retrace", 0, 0), f"C ABI drop-in T={T} B={B}"):
        st = L.hpc_rll_retrace_forward(p["q"].data_ptr(), p["vp"].data_ptr(), p["r"].data_ptr(), p["a"].data_ptr(), None,
                                       p["ratio"].data_ptr(), Qd.t.data_ptr(), wsd.t.data_ptr(), T, B, N, GAMMA, 1.0,
                                       cabi.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert st == 0, st
    Qd.check("drop-in q_retraces")
    wsd.check("drop-in ws")
    Qd.assert_written("drop-in q_retraces")
    wsd.assert_written("drop-in ws")
    assert torch.equal(_run_drop_in(p).squeeze(-1), Qd.t)


def test_gradient_at_a_misaligned_base_and_with_an_upstream_gradient():
    """A gradient buffer off 16-byte alignment takes the 4-byte store kernel; g_loss scales every element."""
    import cabi
    L = cabi.lib
    T, B, n = 12, 100, 6
    p = _problem(T, B, n=n, salt=9)
    ref = _run_loss(p, p["w"], p["lw"])
    nws = L.hpc_rll_retrace_workspace_floats(T, B)
    loss, Q, v, ws = (torch.empty(1, device=DEV), torch.empty(T + 1, B, device=DEV), torch.empty(T + 1, B, device=DEV),
                      torch.empty(nws, device=DEV))
    args = (p["q"].data_ptr(), p["tgt"].data_ptr(), p["beh"].data_ptr(), p["a"].data_ptr(), p["r"].data_ptr(),
            p["w"].data_ptr(), p["lw"].data_ptr(), loss.data_ptr(), Q.data_ptr(), v.data_ptr(), ws.data_ptr(), T, B, n, GAMMA,
            1.0, 1.0 / (T * B), cabi.stream_ptr(DEV))
    assert L.hpc_rll_retrace_loss_forward(*args) == 0
    g = torch.full((1,), 3.0, device=DEV)
    for off in (0, 1, 3):
        grad = GuardedF32(T + 1, B * n, off, DEV)
        assert L.hpc_rll_retrace_loss_backward(g.data_ptr(), p["a"].data_ptr(), ws.data_ptr(), grad.t.data_ptr(), T, B, n,
                                               cabi.stream_ptr(DEV)) == 0
        torch.cuda.synchronize()
        grad.check(f"offset {off}")
        grad.assert_written(f"offset {off}")
        assert torch.equal(grad.t.view(T + 1, B, n), ref[3] * 3.0), off


def test_empty_shapes_zero_the_loss_and_launch_nothing():
    import cabi
    from hpc_rll.rl_utils.retrace import retrace, retrace_loss
    before = last()
    for T, B in ((0, 4), (4, 0)):
        loss = torch.full((1,), float("nan"), device=DEV)
        st = cabi.lib.hpc_rll_retrace_loss_forward(None, None, None, None, None, None, None, loss.data_ptr(), None, None, None,
                                                   T, B, N, GAMMA, 1.0, 1.0, cabi.stream_ptr(DEV))
        torch.cuda.synchronize()
        assert st == 0 and loss.item() == 0.0
        assert cabi.lib.hpc_rll_retrace_forward(None, None, None, None, None, None, None, None, T, B, N, GAMMA, 1.0,
                                                cabi.stream_ptr(DEV)) == 0
        z = lambda *s: torch.zeros(*s, device=DEV)   # noqa: E731
        q = torch.randn(T + 1, B, N, device=DEV, requires_grad=True)
        loss, Q, v = retrace_loss(q, z(T + 1, B, N), z(T, B, N), z(T, B).long(), z(T, B))
        (gq,) = torch.autograd.grad(loss, q)
        assert loss.item() == 0.0 and Q.shape == v.shape == (T + 1, B) and gq.shape == q.shape and not bool(gq.any())
        vp = torch.randn(T + 1, B, 1, device=DEV)
        assert torch.equal(retrace(q.detach(), vp, z(T, B), z(T, B).long(), None, z(T, B, N)), vp)
    assert last() == before, "a call that launches nothing moved the record"


# ---------------------------------------------------------------------------------------------------------------------
# coverage: every configuration x form x null combination, with a whole-tile and a ragged B, and both finalisation paths
# ---------------------------------------------------------------------------------------------------------------------
def test_coverage_of_every_cell():
    """Run the whole file: the cells are recorded by test_every_configuration_both_forms."""
    missing = [(cfg, combo, sorted(COVER.get((cfg, combo), set()))) for cfg in CONFIGS for combo in COMBOS
               if COVER.get((cfg, combo), set()) != {"whole", "ragged"}]
    assert len(CONFIGS) * len(COMBOS) == 48
    assert not missing, f"{len(missing)} cells were not run with both a whole-tile and a ragged B:\n" + \
                        "\n".join(map(str, missing))
    assert FIN == {FOLD, FINALIZE}, FIN
    print(f"covered: {len(CONFIGS)} configurations x {len(COMBOS)} form / null combinations, whole-tile and ragged B, "
          "fold and finalize")
