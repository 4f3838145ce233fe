"""Episode-aware UPGO (``masked_upgo`` / ``MaskedUPGO``, csrc/scan_masked.hip: MaskedUpgoOp) on an MI355X (``-m gpu``).

The oracle is this file's own fp64 restatement of the recurrence, a plain Python loop over ``t``.  ``lam`` is a comparison,
so a near-tie would flip between fp32 and fp64 and move a return by O(1): the inputs are conditioned instead of exempting
samples (``_condition``: where ``|q_{t+1} - V_{t+1}| < 1e-3``, ``reward[t+1]`` gets ``+1e-2``), and the margin is asserted on
the host before any kernel runs.  Bars are the project's: ``rel_err <= 1e-5`` on the loss, ``grad_err <= 2e-5`` on
``grad_target_output``.

Every launch is followed by ``hpc_rll_upgo_masked_last_config``: exactly one more launch, and the configuration, mask form,
grid and finalisation written here as LITERALS.  The rule, by hand (V = 1, LC = 8): wgs = ceil(B / 64), chunks =
ceil(T / 8); NW = 16 for wgs < 512 (4096-wave target), halved while NW > chunks (chunks 1 -> 1, 2..3 -> 2, 4..7 -> 4,
8..15 -> 8, >= 16 -> 16); SUB (NW = 16): 2 if wgs < 256 and chunks >= 32, 4 if also wgs < 128 and chunks >= 64, 8 if also
wgs < 64 and chunks >= 128; grid = ceil(B / (64 / SUB)); the loss is folded into the launch up to 512 workgroups, else the
finalize launch.  A wave's chunks count down from T: [T-8, T), [T-16, T-8), ...
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
FIELDS = ("count", "v", "lc", "nw", "sub", "ntl", "mt", "mm", "nvf", "grid", "fin")
FOLD, FINALIZE = 1, 2
# the 14 mask forms (mask element type, mask mode, next-value form); mode 0 = no masks (u8), 1 = done only, 2 = done and
# traj_flag, 3 = traj_flag only
FORMS = [(0, 0, 0), (0, 0, 1)] + [(mt, mm, nvf) for mt in (0, 1) for mm in (1, 2, 3) for nvf in (0, 1)]
assert len(FORMS) == 14
# (T, B, (V, LC, NW, SUB), grid, finalisation, last tile)
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
COVER = {}     # (cfg, form) -> {"whole", "ragged"}
FIN = set()


# ---------------------------------------------------------------------------------------------------------------------
# dispatch record
# ---------------------------------------------------------------------------------------------------------------------
def last():
    import cabi
    out = (ctypes.c_int * 11)()
    assert cabi.lib.hpc_rll_upgo_masked_last_config(out) == 0
    return dict(zip(FIELDS, out))


class launches:
    """The body launches the masked UPGO scan exactly once, and the record names the literal instantiation."""

    def __init__(self, cfg, grid, fin, form, what=""):
        self.want = dict(v=cfg[0], lc=cfg[1], nw=cfg[2], sub=cfg[3], ntl=0, mt=form[0], mm=form[1], nvf=form[2], grid=grid,
                         fin=fin)
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
# fp64 oracle, written from the recurrence:
#   k^d = 1 - done, k^f = 1 - f (f = traj_flag, default done), nv_t = value[t+1] | next_value[t], V_t = value[t]
#   q_t = r_t + gamma k^d_t nv_t;  lam_{T-1} = 1, lam_t = [q_{t+1} >= value[t+1]];  G_T = nv_{T-1}
#   a_t = gamma k^f_t lam_t;  G_t = r_t + (gamma k^d_t - a_t) nv_t + a_t G_{t+1};  loss = -mean(rho (G - V) log pi(a))
# ---------------------------------------------------------------------------------------------------------------------
def _f64(x):
    return x.detach().to("cpu", torch.float64)


def _mask64(m):
    """bool / uint8: nonzero counts as 1; float32: used as written."""
    if m is None:
        return None
    m = m.detach().cpu()
    return m.to(torch.float64) if m.dtype == torch.float32 else (m != 0).to(torch.float64)


def returns64(r, value, next_value=None, done=None, traj_flag=None, gamma=1.0):
    """-> G (T,B), lam (T,B), margin (T-1,B) = q_{t+1} - value[t+1], all fp64 on the host."""
    r, value = _f64(r), _f64(value)
    T = r.shape[0]
    nv = _f64(next_value) if next_value is not None else value[1:]
    d, f = _mask64(done), _mask64(traj_flag)
    kd = 1.0 - d if d is not None else torch.ones_like(r)
    kf = 1.0 - f if f is not None else kd
    q = r + gamma * kd * nv
    margin = q[1:] - value[1:T]
    G = torch.empty_like(r)
    lam = torch.ones_like(r)
    nxt = nv[T - 1]
    for t in range(T - 1, -1, -1):
        if t < T - 1:
            lam[t] = (q[t + 1] >= value[t + 1]).to(torch.float64)
        a = gamma * kf[t] * lam[t]
        G[t] = r[t] + (gamma * kd[t] - a) * nv[t] + a * nxt
        nxt = G[t]
    return G, lam, margin


def oracle(to, rho, a, r, value, next_value=None, done=None, traj_flag=None, gamma=1.0):
    """-> (loss, grad_target_output (T,B,N)) in fp64; asserts the conditioning of the comparison first."""
    G, _, margin = returns64(r, value, next_value, done, traj_flag, gamma)
    if margin.numel():
        assert float(margin.abs().min()) > 1e-3, "the inputs were not conditioned: a comparison is a near-tie"
    T, B = r.shape
    logsm = torch.log_softmax(_f64(to), dim=-1)
    idx = a.detach().cpu().unsqueeze(-1)
    logp = logsm.gather(-1, idx).squeeze(-1)
    adv = _f64(rho) * (G - _f64(value)[:T])
    loss = -(adv * logp).sum() / (T * B)
    onehot = torch.zeros_like(logsm).scatter_(-1, idx, 1.0)
    grad = (-adv / (T * B)).unsqueeze(-1) * (onehot - logsm.exp())
    return float(loss), grad.numpy()


def _condition(r, value, next_value=None, done=None, gamma=1.0):
    """reward with every comparison margin |q_{t+1} - value[t+1]| above 1e-3: near-ties get +1e-2 on reward[t+1]."""
    _, _, margin = returns64(r, value, next_value, done, None, gamma)
    r = r.clone()
    if margin.numel():
        r[1:] += (margin.abs() < 1e-3).to(r.device, torch.float32) * 1e-2
    return r


# ---------------------------------------------------------------------------------------------------------------------
# problems and runners
# ---------------------------------------------------------------------------------------------------------------------
def _gen(T, B, salt=0):
    return torch.Generator(device=DEV).manual_seed(T * 1000003 + B + 7919 * salt)


def _np(x):
    return x.detach().cpu().numpy()


def _problem(T, B, n=N, salt=0):
    g = _gen(T, B, salt)
    p = dict(to=torch.randn(T, B, n, device=DEV, generator=g), rho=torch.rand(T, B, device=DEV, generator=g) + 0.5,
             a=torch.randint(0, n, (T, B), device=DEV, generator=g), r=torch.randn(T, B, device=DEV, generator=g),
             v=torch.randn(T + 1, B, device=DEV, generator=g), g=g)
    return p


def _masks(g, T, B):
    """done and traj_flag (bool) with columns of density 0, 1, 0.05 and 0.3 side by side; every fourth column ends an
    episode in the last step; traj_flag adds truncations (never on the density-0 columns)."""
    col = torch.arange(B, device=DEV) % 4
    dens = torch.tensor([0.0, 1.0, 0.05, 0.3], device=DEV)[col]
    d = torch.rand(T, B, device=DEV, generator=g) < dens
    d[T - 1, 2::4] = True
    f = d | ((torch.rand(T, B, device=DEV, generator=g) < 0.05) & (col != 0))
    return d, f


def _typed(g, m, mt):
    if mt == 1:
        return m.to(torch.float32)
    byte = torch.randint(1, 256, m.shape, device=DEV, generator=g, dtype=torch.int32).to(torch.uint8)
    return m.to(torch.uint8) * byte          # any nonzero byte counts as 1


def _mask_kw(mm, d, f):
    return [{}, {"done": d}, {"done": d, "traj_flag": f}, {"traj_flag": f}][mm]


def _run(p, r, nvf, kw, gamma, v=None, nv=None):
    """masked_upgo -> (loss (1,), grad_target_output); next-value form from the same data unless nv is given."""
    from hpc_rll.rl_utils.upgo import masked_upgo
    to = p["to"].detach().requires_grad_(True)
    v = p["v"] if v is None else v
    if nvf:
        loss = masked_upgo(to, p["rho"], p["a"], r, v[:r.shape[0]], gamma=gamma,
                           next_value=v[1:] if nv is None else nv, **kw)
    else:
        loss = masked_upgo(to, p["rho"], p["a"], r, v, gamma=gamma, **kw)
    (gt,) = torch.autograd.grad(loss, to)
    return loss.detach(), gt


def _upgo(p, r):
    from hpc_rll.rl_utils.upgo import UPGO
    to = p["to"].detach().requires_grad_(True)
    loss = UPGO(r.shape[0], r.shape[1], p["to"].shape[2])(to, p["rho"], p["a"], r, p["v"])
    (gt,) = torch.autograd.grad(loss, to)
    return loss.detach(), gt


def _parity(got, want, what):
    loss, grad = want
    print(f"{what}: loss {got[0].item():.9g} oracle {loss:.9g} rel_err {rel_err(loss, got[0].item()):.3g}")
    assert rel_err(loss, got[0].item()) <= TOL, (what, "loss", loss, got[0].item())
    e = grad_err(grad, _np(got[1]), "grad_target_output")
    print(f"{what}: grad_err {e:.3g}")
    assert e <= 2 * TOL, (what, "grad_target_output", e)


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---------------------------------------------------------------------------------------------------------------------
# every configuration x every mask form, gamma = 0.97.  One oracle per (shape, mask mode), shared by the element types
# and the two value forms (next_value = value[1:] is the same problem, and must give the same bits).
# ---------------------------------------------------------------------------------------------------------------------
GAMMA = 0.97


@pytest.mark.parametrize("T,B,cfg,grid,fin,kind", CELLS)
def test_every_form(T, B, cfg, grid, fin, kind):
    tile = 64 // cfg[3]
    assert (B % tile == 0) == (kind == "whole")
    p = _problem(T, B)
    g = p["g"]
    d, f = _masks(g, T, B)
    z = torch.zeros_like(d)
    plain = {}
    for mm in range(4):
        r = _condition(p["r"], p["v"], done=d if mm in (1, 2) else None, gamma=GAMMA)
        want = oracle(p["to"], p["rho"], p["a"], r, p["v"], gamma=GAMMA, **_mask_kw(mm, d, f))
        for mt in ((0,) if mm == 0 else (0, 1)):
            kw = _mask_kw(mm, _typed(g, d, mt), _typed(g, f, mt))
            zkw = _mask_kw(mm, _typed(g, z, mt), _typed(g, z, mt))
            got = {}
            for nvf in (0, 1):
                form = (mt, mm, nvf)
                what = f"masked UPGO T={T} B={B} form={form}"
                with launches(cfg, grid, fin, form, what):
                    got[nvf] = _run(p, r, nvf, kw, GAMMA)
                with launches(cfg, grid, fin, form, what + " again"):
                    again = _run(p, r, nvf, kw, GAMMA)
                assert _same(got[nvf], again), what + ": not reproducible"
                # all-zero masks give the mask-free bits (on this mode's reward)
                if mm == 0:
                    plain[nvf] = got[nvf]
                else:
                    with launches(cfg, grid, fin, (0, 0, nvf), what + " no masks"):
                        ref = _run(p, r, nvf, {}, GAMMA)
                    with launches(cfg, grid, fin, form, what + " zero masks"):
                        zero = _run(p, r, nvf, zkw, GAMMA)
                    assert _same(zero, ref), what + ": all-zero masks do not give the mask-free bits"
                COVER.setdefault((cfg, form), set()).add(kind)
                FIN.add(fin)
            assert _same(got[0], got[1]), f"T={T} B={B} ({mt},{mm}): stacked and next-value bits differ"
            _parity(got[0], want, f"masked UPGO T={T} B={B} ({mt},{mm})")


# ---------------------------------------------------------------------------------------------------------------------
# chunk edges.  T = 30 runs 4 waves of 8-step chunks counting down from T: [22,30) [14,22) [6,14) [-2,6), so the last /
# first rows of chunks are 29 | 21, 22 | 13, 14 | 5, 6; T = 32 puts them at 31 | 23, 24 | 15, 16 | 7, 8.  Both position
# sets run at both lengths.  On the even columns the masked steps are built so that done flips the comparison of the step
# before: r_t = V_t - nv_t / 2 gives q_t - V_t = +nv_t / 2 without done and -nv_t / 2 with it.
# ---------------------------------------------------------------------------------------------------------------------
EDGE_SETS = {"issue": (7, 8, 15, 16, 23, 24), "countdown": (5, 6, 13, 14, 21, 22)}


def _edge_problem(T, B, steps):
    p = _problem(T, B, salt=5)
    r, v = p["r"].clone(), p["v"]
    for t in steps:
        r[t, 0::2] = v[t, 0::2] - 0.5 * v[t + 1, 0::2]
    # keep |nv| away from 0 on the built steps so that both margins are far from a tie
    assert float(v[1:][list(steps)][:, 0::2].abs().min()) > 0
    return p, r


@pytest.mark.parametrize("mask_dtype", [torch.bool, torch.float32])
@pytest.mark.parametrize("B", [64, 100])
@pytest.mark.parametrize("T,which", [(30, "issue"), (30, "countdown"), (32, "issue"), (32, "countdown")])
def test_done_at_chunk_edges(T, which, B, mask_dtype):
    steps = EDGE_SETS[which] + (T - 1,)
    p, r = _edge_problem(T, B, steps)
    d = torch.zeros(T, B, dtype=torch.bool, device=DEV)
    d[list(steps)] = True
    # condition for the masked AND the mask-free comparison (the mask-free oracle below is only used for the flip count)
    r = _condition(r, p["v"], done=d)
    _, lam_m, _ = returns64(r, p["v"], done=d)
    _, lam_0, _ = returns64(r, p["v"])
    at = [t - 1 for t in steps if t >= 1]
    flips = float((lam_m[at] != lam_0[at]).to(torch.float64).mean())
    assert flips >= 0.25, f"done flips lam on only {flips:.2f} of the steps before a masked step"
    want = oracle(p["to"], p["rho"], p["a"], r, p["v"], done=d)
    cfg, grid = (1, 8, 4, 1), (B + 63) // 64
    mt = 1 if mask_dtype == torch.float32 else 0
    got = {}
    for nvf in (0, 1):
        with launches(cfg, grid, FOLD, (mt, 1, nvf), f"edges T={T} B={B}"):
            got[nvf] = _run(p, r, nvf, {"done": d.to(mask_dtype)}, 1.0)
        _parity(got[nvf], want, f"done at chunk edges T={T} B={B} {which} nvf={nvf}")
    assert _same(got[0], got[1])


@pytest.mark.parametrize("mask_dtype", [torch.bool, torch.float32])
@pytest.mark.parametrize("B", [64, 100])
@pytest.mark.parametrize("T,which", [(30, "issue"), (30, "countdown"), (32, "issue"), (32, "countdown")])
def test_truncation_at_chunk_edges(T, which, B, mask_dtype):
    """traj_flag-only truncations in the next-value form: the flagged step returns r_t + gamma nv_t with the final
    observation's value in next_value[t]; the comparison of the step before still uses value[t] and next_value[t]."""
    steps = EDGE_SETS[which] + (T - 1,)
    p = _problem(T, B, salt=6)
    f = torch.zeros(T, B, dtype=torch.bool, device=DEV)
    f[list(steps)] = True
    v0 = p["v"][:T].contiguous()
    nv = p["v"][1:].clone()
    nv[list(steps)] = torch.randn(len(steps), B, device=DEV, generator=p["g"])     # final observations' values
    r = _condition(p["r"], v0, next_value=nv, gamma=0.97)
    G_m, _, _ = returns64(r, v0, next_value=nv, traj_flag=f, gamma=0.97)
    G_0, _, _ = returns64(r, v0, next_value=nv, gamma=0.97)
    moved = float(((G_m - G_0).abs()[list(steps[:-1])] > 1e-3).to(torch.float64).mean())
    assert moved >= 0.25, f"the truncation moves the return on only {moved:.2f} of the flagged steps"
    want = oracle(p["to"], p["rho"], p["a"], r, v0, next_value=nv, traj_flag=f, gamma=0.97)
    mt = 1 if mask_dtype == torch.float32 else 0
    with launches((1, 8, 4, 1), (B + 63) // 64, FOLD, (mt, 3, 1), f"truncation T={T} B={B}"):
        got = _run(p, r, 1, {"traj_flag": f.to(mask_dtype)}, 0.97, v=v0, nv=nv)
    _parity(got, want, f"truncation at chunk edges T={T} B={B} {which}")


@pytest.mark.parametrize("T,cfg", [(1, (1, 8, 1, 1)), (2, (1, 8, 1, 1)), (8, (1, 8, 1, 1)), (9, (1, 8, 2, 1))])
@pytest.mark.parametrize("B", [64, 100])
def test_short_unrolls(T, B, cfg):
    """One row, two rows, exactly one chunk, one chunk and one row: done on the last step and (T >= 2) the first; also a
    truncated last step in the next-value form."""
    p = _problem(T, B, salt=7)
    d = torch.zeros(T, B, dtype=torch.bool, device=DEV)
    d[T - 1, 0::2] = True
    d[0, 1::3] = True
    r = _condition(p["r"], p["v"], done=d, gamma=0.97)
    want = oracle(p["to"], p["rho"], p["a"], r, p["v"], done=d, gamma=0.97)
    for nvf in (0, 1):
        with launches(cfg, (B + 63) // 64, FOLD, (0, 1, nvf), f"short T={T} B={B}"):
            got = _run(p, r, nvf, {"done": d}, 0.97)
        _parity(got, want, f"short unroll T={T} B={B} nvf={nvf}")
    f = torch.zeros(T, B, device=DEV)
    f[T - 1] = 1.0
    v0, nv = p["v"][:T].contiguous(), torch.randn(T, B, device=DEV, generator=p["g"])
    r = _condition(p["r"], v0, next_value=nv, done=d, gamma=0.97)
    want = oracle(p["to"], p["rho"], p["a"], r, v0, next_value=nv, done=d, traj_flag=f, gamma=0.97)
    with launches(cfg, (B + 63) // 64, FOLD, (1, 2, 1), f"short T={T} B={B}"):
        got = _run(p, r, 1, {"done": d.to(torch.float32), "traj_flag": f}, 0.97, v=v0, nv=nv)
    _parity(got, want, f"short unroll T={T} B={B} truncated")


# ---------------------------------------------------------------------------------------------------------------------
# bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,B,cfg,grid,fin,kind", CELLS)
def test_gamma_one_stacked_without_masks_is_upgo(T, B, cfg, grid, fin, kind):
    """(a) loss and gradient are UPGO's bits at a whole and a ragged cell of each configuration, and (d) a second run
    gives the same bits.  No conditioning: both sides take every comparison in fp32."""
    p = _problem(T, B, salt=1)
    ref = _upgo(p, p["r"])
    with launches(cfg, grid, fin, (0, 0, 0), f"T={T} B={B}"):
        got = _run(p, p["r"], 0, {}, 1.0)
    with launches(cfg, grid, fin, (0, 0, 0), f"T={T} B={B}"):
        again = _run(p, p["r"], 0, {}, 1.0)
    assert _same(got, ref), f"T={T} B={B}: gamma = 1 without masks does not give UPGO's bits"
    assert _same(got, again), f"T={T} B={B}: not reproducible"
    z = torch.zeros(T, B, dtype=torch.bool, device=DEV)
    with launches(cfg, grid, fin, (0, 2, 0), f"T={T} B={B} zero masks"):
        zero = _run(p, p["r"], 0, {"done": z, "traj_flag": z}, 1.0)
    assert _same(zero, ref), f"T={T} B={B}: all-zero masks do not give UPGO's bits"


@pytest.mark.parametrize("T,B", [(30, 100), (300, 1000), (1024, 60)])
@pytest.mark.parametrize("dtype", [torch.bool, torch.uint8, torch.float32])
def test_zero_masks_of_every_dtype_give_the_mask_free_bits(T, B, dtype):
    """(b) for done, done + traj_flag and traj_flag only, in both value forms."""
    cfg, grid, fin = cfg_of(T, B)
    p = _problem(T, B, salt=2)
    z = torch.zeros(T, B, dtype=dtype, device=DEV)
    mt = 1 if dtype == torch.float32 else 0
    for nvf in (0, 1):
        with launches(cfg, grid, fin, (0, 0, nvf)):
            ref = _run(p, p["r"], nvf, {}, 0.97)
        for mm in (1, 2, 3):
            with launches(cfg, grid, fin, (mt, mm, nvf)):
                got = _run(p, p["r"], nvf, _mask_kw(mm, z, z), 0.97)
            assert _same(got, ref), (T, B, dtype, mm, nvf)


@pytest.mark.parametrize("T,B", [(30, 100), (121, 100), (600, 96)])
def test_stacked_and_next_value_forms_give_the_same_bits(T, B):
    """(c) with hard done masks, and (d) twice."""
    cfg, grid, fin = cfg_of(T, B)
    p = _problem(T, B, salt=3)
    d, f = _masks(p["g"], T, B)
    for kw, mm in (({"done": d}, 1), ({"done": d, "traj_flag": f}, 2)):
        with launches(cfg, grid, fin, (0, mm, 0)):
            a = _run(p, p["r"], 0, kw, 1.0)
        with launches(cfg, grid, fin, (0, mm, 1)):
            b = _run(p, p["r"], 1, kw, 1.0)
        with launches(cfg, grid, fin, (0, mm, 1)):
            c = _run(p, p["r"], 1, kw, 1.0)
        assert _same(a, b) and _same(b, c), (T, B, mm)


# ---------------------------------------------------------------------------------------------------------------------
# independent of this file's oracle: every episode alone through the existing UPGO
# ---------------------------------------------------------------------------------------------------------------------
def test_episodes_match_upgo_run_on_each_episode_alone():
    from hpc_rll.rl_utils.upgo import UPGO
    T, B = 24, 4
    p = _problem(T, B, salt=4)
    ends = [[23], [7, 23], [0, 8, 15, 23], [2, 3, 16, 22, 23]]       # last step of every episode, per column
    d = torch.zeros(T, B, dtype=torch.bool, device=DEV)
    for b, e in enumerate(ends):
        d[e, b] = True
    with launches((1, 8, 2, 1), 1, FOLD, (0, 1, 0)):
        loss, gt = _run(p, p["r"], 0, {"done": d}, 1.0)
    want = torch.zeros_like(gt)
    total = 0.0
    for b, e in enumerate(ends):
        s = 0
        for last_step in e:
            n = last_step - s + 1
            sl = slice(s, last_step + 1)
            to = p["to"][sl, b:b + 1].detach().clone().requires_grad_(True)
            v = torch.cat([p["v"][sl, b:b + 1], torch.zeros(1, 1, device=DEV)])
            seg = UPGO(n, 1, N)(to, p["rho"][sl, b:b + 1].contiguous(), p["a"][sl, b:b + 1].contiguous(),
                                p["r"][sl, b:b + 1].contiguous(), v)
            (g,) = torch.autograd.grad(seg, to)
            want[sl, b:b + 1] = g * (n * 1 / (T * B))
            total += seg.item() * n / (T * B)
            s = last_step + 1
        assert s == T
    e = grad_err(_np(want.double()), _np(gt), "grad_target_output")
    print(f"episodes alone: grad_err {e:.3g}, loss {loss.item():.9g} vs {total:.9g}")
    assert e <= 2 * TOL
    assert rel_err(total, loss.item()) <= TOL


# ---------------------------------------------------------------------------------------------------------------------
# other cases
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,B", [(30, 100), (300, 1000)])
@pytest.mark.parametrize("gamma", [1.0, 0.97])
def test_soft_masks(T, B, gamma):
    """float32 masks in (0,1), done alone and with its own traj_flag, both value forms."""
    cfg, grid, fin = cfg_of(T, B)
    p = _problem(T, B, salt=8)
    g = p["g"]
    d = torch.rand(T, B, device=DEV, generator=g) * 0.98 + 0.01
    f = torch.rand(T, B, device=DEV, generator=g) * 0.98 + 0.01
    assert 0.0 < float(d.min()) and float(d.max()) < 1.0
    r = _condition(p["r"], p["v"], done=d, gamma=gamma)
    for kw, mm in (({"done": d}, 1), ({"done": d, "traj_flag": f}, 2)):
        want = oracle(p["to"], p["rho"], p["a"], r, p["v"], gamma=gamma, **kw)
        for nvf in (0, 1):
            with launches(cfg, grid, fin, (1, mm, nvf)):
                got = _run(p, r, nvf, kw, gamma)
            _parity(got, want, f"soft masks T={T} B={B} gamma={gamma} mm={mm} nvf={nvf}")


@pytest.mark.parametrize("n", [1, 130])
def test_action_counts(n):
    T, B = 30, 100
    p = _problem(T, B, n=n, salt=9)
    d, f = _masks(p["g"], T, B)
    r = _condition(p["r"], p["v"], done=d, gamma=0.97)
    want = oracle(p["to"], p["rho"], p["a"], r, p["v"], done=d, traj_flag=f, gamma=0.97)
    with launches((1, 8, 4, 1), 2, FOLD, (0, 2, 0)):
        got = _run(p, r, 0, {"done": d, "traj_flag": f}, 0.97)
    if n == 1:      # log pi = 0: the loss and the gradient are exactly zero
        assert got[0].item() == 0.0 and not bool(got[1].any())
        assert want[0] == 0.0 and not want[1].any()
    else:
        _parity(got, want, f"N={n}")


def test_zero_rhos_give_a_zero_loss_and_gradient():
    T, B = 30, 100
    p = _problem(T, B, salt=10)
    p["rho"] = torch.zeros(T, B, device=DEV)
    d, _ = _masks(p["g"], T, B)
    loss, gt = _run(p, p["r"], 0, {"done": d}, 0.97)
    assert loss.item() == 0.0 and bool(torch.isfinite(gt).all()) and not bool(gt.any())


def test_minus_inf_logits_on_other_actions():
    """-inf on actions that were not chosen: zero gradient there, finite everywhere, parity on the rest."""
    T, B, n = 30, 100, 5
    p = _problem(T, B, n=n, salt=11)
    other = (p["a"] + 1 + torch.randint(0, n - 1, (T, B), device=DEV, generator=p["g"])) % n
    assert not bool((other == p["a"]).any())
    hole = torch.zeros(T, B, n, dtype=torch.bool, device=DEV).scatter_(-1, other.unsqueeze(-1), True)
    hole &= (torch.rand(T, B, 1, device=DEV, generator=p["g"]) < 0.5)
    p["to"] = p["to"].masked_fill(hole, float("-inf"))
    d, _ = _masks(p["g"], T, B)
    r = _condition(p["r"], p["v"], done=d)
    got = _run(p, r, 0, {"done": d}, 1.0)
    assert bool(torch.isfinite(got[1]).all()) and not bool(got[1][hole].any())
    _parity(got, oracle(p["to"], p["rho"], p["a"], r, p["v"], done=d), "-inf logits")


@pytest.mark.parametrize("T,B", [(30, 100), (600, 100), (5, 33000)])
def test_c_abi_writes_nothing_past_its_outputs(T, B):
    """The C entry point on guarded buffers at a ragged B: loss, workspace and the gradient keep their guard bands, every
    element of the coefficients and of the gradient is written, and the bits are masked_upgo's."""
    import cabi
    cfg, grid, fin = cfg_of(T, B)
    p = _problem(T, B, salt=12)
    d, f = _masks(p["g"], T, B)
    d8, f8 = d.to(torch.uint8), f.to(torch.uint8)
    nws = cabi.lib.hpc_rll_upgo_workspace_floats(T, B)
    assert nws >= 2 * T * B
    loss, ws, grad = GuardedF32(1, 1, 0, DEV), GuardedF32(1, nws, 0, DEV), GuardedF32(T, B * N, 0, DEV)
    v0, nv = GuardedF32(T, B, 0, DEV, p["v"][:-1]), GuardedF32(T, B, 0, DEV, p["v"][1:])
    with launches(cfg, grid, fin, (0, 2, 1), f"C ABI T={T} B={B}"):
        st = cabi.lib.hpc_rll_upgo_masked_forward(p["to"].data_ptr(), p["rho"].data_ptr(), p["a"].data_ptr(),
                                                  p["r"].data_ptr(), v0.t.data_ptr(), nv.t.data_ptr(), d8.data_ptr(),
                                                  f8.data_ptr(), 0, loss.t.data_ptr(), ws.t.data_ptr(), T, B, N, 0.97,
                                                  1.0 / (T * B), cabi.stream_ptr(DEV))
    assert st == 0, st
    one = torch.ones(1, device=DEV)
    st = cabi.lib.hpc_rll_upgo_backward(one.data_ptr(), p["to"].data_ptr(), p["a"].data_ptr(), ws.t.data_ptr(), grad.t.data_ptr(),
                                        T, B, N, cabi.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert st == 0, st
    for name, buf in (("loss", loss), ("ws", ws), ("grad", grad), ("value", v0), ("next_value", nv)):
        buf.check(f"T={T} B={B} {name}")
    loss.assert_written("loss")
    grad.assert_written("grad")
    assert not bool(torch.isnan(ws.t[0, :2 * T * B]).any()), "coefficients / log-probabilities were not all written"
    ref = _run(p, p["r"], 1, {"done": d, "traj_flag": f}, 0.97)
    assert torch.equal(ref[0], loss.t.view(1)) and torch.equal(ref[1], grad.t.view(T, B, N))


def test_empty_shapes_zero_the_loss():
    import cabi
    before = last()
    for T, B in ((0, 4), (4, 0)):
        loss = torch.full((1,), float("nan"), device=DEV)
        st = cabi.lib.hpc_rll_upgo_masked_forward(None, None, None, None, None, None, None, None, 0, loss.data_ptr(), None,
                                                  T, B, N, 1.0, 1.0, cabi.stream_ptr(DEV))
        torch.cuda.synchronize()
        assert st == 0 and loss.item() == 0.0
    assert last() == before, "a call that launches nothing moved the record"


# ---------------------------------------------------------------------------------------------------------------------
# coverage: every configuration x every form, with a whole-tile and a ragged B, and both finalisation paths
# ---------------------------------------------------------------------------------------------------------------------
def test_coverage_of_every_cell():
    """Run the whole file: the cells are recorded by test_every_form."""
    missing = [(cfg, form, sorted(COVER.get((cfg, form), set()))) for cfg in CONFIGS for form in FORMS
               if COVER.get((cfg, form), set()) != {"whole", "ragged"}]
    assert len(CONFIGS) * len(FORMS) == 112
    assert not missing, f"{len(missing)} cells were not run with both a whole-tile and a ragged B:\n" + \
                        "\n".join(map(str, missing))
    assert FIN == {FOLD, FINALIZE}, FIN
    print(f"covered: {len(CONFIGS)} configurations x {len(FORMS)} forms, whole-tile and ragged B, fold and finalize")
