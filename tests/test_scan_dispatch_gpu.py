"""Every kernel the column-scan dispatcher (csrc/colscan.hpp: scan_cfg / launch_colscan / scan_and_finalize) and the
episode-aware GAE dispatcher (csrc/gae_masked.hip: choose_cfg / with_cfg / with_mode) can pick (run with ``-m gpu`` on an
MI355X).

Every launch is followed by ``hpc_rll_scan_last_config``: the record must show exactly one more launch of the op, and the
instantiation, the mask form, the grid and the finalisation path written in this file as LITERALS.  The literals were
derived by hand from the two rules (the derivation is in the comments above each table); nothing here evaluates a copy
of ``scan_cfg`` or ``choose_cfg``.  Results are compared with the fp64 oracles of tests/test_masked_returns_gpu.py,
tests/test_masked_gae_gpu.py and oracle.ref_torch at the project's bars (1e-5 losses / advantages via ``rel_err``, 2e-5
gradients via ``grad_err``) and bit for bit where DESIGN.md promises it.

Cells (asserted by ``test_coverage_of_every_cell`` at the end of the file, each with a whole-tile B and a ragged B):
  * unmasked: 13 TD(lambda) + 8 V-trace + 8 UPGO configurations (V, LC, NW, SUB);
  * masked TD(lambda) / V-trace: (13 + 8) configurations x 14 mask forms = 294;
  * masked GAE: 6 configurations x 14 mask forms, forward and backward = 168;
  * both finalisation paths (folded into the launch / finalize launch) for the five ops that have loss sums.
Exemptions, exactly the ones in ``EXEMPT``: (V=2, NW=16) is never selected (V = 2 needs >= 512 workgroups, where 8 waves
reach the wave target), and the two masked-GAE ops have no loss sums to finalise.
"""
import ctypes
from contextlib import contextmanager

import numpy as np
import pytest
import torch

import test_masked_gae_gpu as MG
import test_masked_returns_gpu as MR
from conftest import grad_err, rel_err
from guarded import GuardedF32

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 1e-5
N = 3                                        # actions: small, so that the scan is what is exercised
TD, VT, UPGO, MTD, MVT, GF, GB = range(7)    # HPC_RLL_SCAN_OP_*
NAMES = ("td_lambda", "vtrace", "upgo", "td_lambda_masked", "vtrace_masked", "gae_masked_fwd", "gae_masked_bwd")
FIELDS = ("count", "v", "lc", "nw", "sub", "ntl", "mt", "mm", "nvf", "grid", "fin")
FOLD, FINALIZE = 1, 2
# the 14 mask forms of masks.hpp: with_mode as (mask element type, mask mode, next-value form); mode 0 = no masks (u8),
# 1 = done only, 2 = done and traj_flag, 3 = traj_flag only
FORMS = [(0, 0, 0), (0, 0, 1)] + [(mt, mm, nvf) for mt in (0, 1) for mm in (1, 2, 3) for nvf in (0, 1)]
assert len(FORMS) == 14

COVER = {}     # (op, (v, lc, nw, sub[, ntl]), form or None) -> {"whole", "ragged"}
FIN = {}       # op -> {FOLD, FINALIZE}


def last(op):
    import cabi
    out = (ctypes.c_int * 11)()
    assert cabi.lib.hpc_rll_scan_last_config(op, out) == 0
    return dict(zip(FIELDS, out))


@contextmanager
def launches(op, cfg, grid, fin, form=(0, 0, 0), ntl=0, what=""):
    """The body launches `op` exactly once, and the record names the literal instantiation."""
    before = last(op)["count"]
    yield
    rec = last(op)
    want = dict(count=before + 1, v=cfg[0], lc=cfg[1], nw=cfg[2], sub=cfg[3], ntl=ntl, mt=form[0], mm=form[1],
                nvf=form[2], grid=grid, fin=fin)
    assert rec == want, (NAMES[op], what, "ran", rec, "expected", want)


def cover(op, cfg, form, kind, fin=0):
    COVER.setdefault((op, cfg, form), set()).add(kind)
    if fin:
        FIN.setdefault(op, set()).add(fin)


def tile_kind(cfg, B, kind):
    tile = 64 * cfg[0] // cfg[3]
    assert (B % tile == 0) == (kind == "whole"), (cfg, B, kind)
    return kind


def _gen(T, B, salt=0):
    return torch.Generator(device=DEV).manual_seed(T * 1000003 + B + 7919 * salt)


def _np(x):
    return x.detach().cpu().numpy()


def _leaf(x):
    return x.detach().requires_grad_(True)


# ---------------------------------------------------------------------------------------------------------------------
# The column-scan rule, by hand.  wgs = ceil(B / 64V), chunks = ceil(T / 8).
#   V  = 2 iff the op may (TD(lambda) only, B even, 8-byte aligned operands) and ceil(B/128) >= 512, i.e. B >= 65409.
#   NW = 16 for wgs < 512, 8 for 512 <= wgs < 1024, 4 from 1024 (the 4096-wave target), then halved while NW > chunks:
#        chunks 1 -> 1, 2..3 -> 2, 4..7 -> 4, 8..15 -> 8, >= 16 -> 16.
#   SUB (V = 1, NW = 16): 2 if wgs < 256 and chunks >= 32 (T >= 249); 4 if also wgs < 128 and chunks >= 64 (T >= 505);
#        8 if also wgs < 64 and chunks >= 128 (T >= 1017).
#   LC = 16 (TD(lambda) only): V = 1, SUB = 1, NW = 16, wgs <= 512 and T > 128.
#   grid = ceil(B / (64 V / SUB)); the loss is folded into the launch up to 512 workgroups, else finalize_sums.
# Rows: (T, B, (V, LC, NW, SUB), grid, finalisation, "whole" | "ragged" last tile).
# ---------------------------------------------------------------------------------------------------------------------
LC16 = (1, 16, 16, 1)
TD_CELLS = [
    (5, 128, (1, 8, 1, 1), 2, FOLD, "whole"), (5, 100, (1, 8, 1, 1), 2, FOLD, "ragged"),
    (12, 128, (1, 8, 2, 1), 2, FOLD, "whole"), (12, 100, (1, 8, 2, 1), 2, FOLD, "ragged"),
    (30, 128, (1, 8, 4, 1), 2, FOLD, "whole"), (30, 100, (1, 8, 4, 1), 2, FOLD, "ragged"),
    (100, 128, (1, 8, 8, 1), 2, FOLD, "whole"), (100, 100, (1, 8, 8, 1), 2, FOLD, "ragged"),
    (128, 128, (1, 8, 16, 1), 2, FOLD, "whole"), (121, 100, (1, 8, 16, 1), 2, FOLD, "ragged"),
    (129, 128, LC16, 2, FOLD, "whole"), (129, 100, LC16, 2, FOLD, "ragged"),
    (300, 1024, (1, 8, 16, 2), 32, FOLD, "whole"), (300, 1000, (1, 8, 16, 2), 32, FOLD, "ragged"),
    (600, 96, (1, 8, 16, 4), 6, FOLD, "whole"), (600, 100, (1, 8, 16, 4), 7, FOLD, "ragged"),
    (1024, 64, (1, 8, 16, 8), 8, FOLD, "whole"), (1024, 60, (1, 8, 16, 8), 8, FOLD, "ragged"),
    (5, 65536, (2, 8, 1, 1), 512, FOLD, "whole"), (5, 65538, (2, 8, 1, 1), 513, FINALIZE, "ragged"),
    (9, 65536, (2, 8, 2, 1), 512, FOLD, "whole"), (9, 65538, (2, 8, 2, 1), 513, FINALIZE, "ragged"),
    (30, 65536, (2, 8, 4, 1), 512, FOLD, "whole"), (30, 65538, (2, 8, 4, 1), 513, FINALIZE, "ragged"),
    (130, 65536, (2, 8, 8, 1), 512, FOLD, "whole"), (130, 65538, (2, 8, 8, 1), 513, FINALIZE, "ragged"),
]
# V-trace and UPGO scan one column per lane with 8-step chunks only (scan_cfg(T, B, false)): the V = 1 rows, LC = 8
VT_CELLS = [c for c in TD_CELLS if c[2][0] == 1 and c[2] != LC16]
TD_CONFIGS = sorted({c[2] for c in TD_CELLS})
VT_CONFIGS = sorted({c[2] for c in VT_CELLS})
assert len(TD_CONFIGS) == 13 and len(VT_CONFIGS) == 8

# Larger shapes of the same configurations, reached through the workgroup count instead of the chunk count, the issue's
# starting table (two of its rows name the wrong configuration: T = 50 has 7 chunks, which halves NW to 4, and T = 20 has
# 3 chunks, which halves NW to 2), and one shape on each side of every threshold of the rule.
TD_MORE = [
    (50, 100, (1, 8, 4, 1), 2, FOLD), (20, 65536, (2, 8, 2, 1), 512, FOLD),
    (200, 40000, (1, 8, 8, 1), 625, FINALIZE), (130, 70001, (1, 8, 4, 1), 1094, FINALIZE),
    (256, 16384, LC16, 256, FOLD), (256, 16385, LC16, 257, FOLD),
    (1024, 8200, (1, 8, 16, 2), 257, FOLD), (1024, 5000, (1, 8, 16, 4), 313, FOLD),
    (130, 131072, (2, 8, 4, 1), 1024, FINALIZE), (130, 131074, (2, 8, 4, 1), 1025, FINALIZE),
    (5, 70000, (2, 8, 1, 1), 547, FINALIZE),
    # workgroup counts 255 / 256, 511 / 512, 1023 / 1024 (V = 1: odd B), and 1023 / 1024 at V = 2
    (300, 16320, (1, 8, 16, 2), 510, FOLD), (300, 16321, LC16, 256, FOLD),
    (300, 32704, LC16, 511, FOLD), (300, 32705, (1, 8, 8, 1), 512, FOLD),
    (100, 65471, (1, 8, 8, 1), 1023, FINALIZE), (100, 65473, (1, 8, 4, 1), 1024, FINALIZE),
    (100, 130944, (2, 8, 8, 1), 1023, FINALIZE), (100, 130946, (2, 8, 4, 1), 1024, FINALIZE),
    # chunk counts 2 NW SUB = 32 / 64 / 128, i.e. T = 248 / 249, 504 / 505, 1016 / 1017; T = 128 / 129 is in TD_CELLS
    (248, 100, LC16, 2, FOLD), (249, 100, (1, 8, 16, 2), 4, FOLD),
    (504, 100, (1, 8, 16, 2), 4, FOLD), (505, 100, (1, 8, 16, 4), 7, FOLD),
    (1016, 100, (1, 8, 16, 4), 7, FOLD), (1017, 100, (1, 8, 16, 8), 13, FOLD),
    # the two-column threshold ceil(B / 128) >= 512
    (100, 65408, (1, 8, 8, 1), 1022, FINALIZE), (100, 65410, (2, 8, 8, 1), 512, FOLD),
]
VT_MORE = [
    (50, 100, (1, 8, 4, 1), 2, FOLD), (129, 100, (1, 8, 16, 1), 2, FOLD), (200, 40000, (1, 8, 8, 1), 625, FINALIZE),
    (130, 70001, (1, 8, 4, 1), 1094, FINALIZE), (256, 16384, (1, 8, 16, 1), 256, FOLD),
    (1024, 8200, (1, 8, 16, 2), 257, FOLD), (1024, 5000, (1, 8, 16, 4), 313, FOLD),
    (300, 16320, (1, 8, 16, 2), 510, FOLD), (300, 16321, (1, 8, 16, 1), 256, FOLD),
    (300, 32704, (1, 8, 16, 1), 511, FOLD), (300, 32705, (1, 8, 8, 1), 512, FOLD),
    (100, 65472, (1, 8, 8, 1), 1023, FINALIZE), (100, 65473, (1, 8, 4, 1), 1024, FINALIZE),
    (248, 100, (1, 8, 16, 1), 2, FOLD), (249, 100, (1, 8, 16, 2), 4, FOLD),
    (504, 100, (1, 8, 16, 2), 4, FOLD), (505, 100, (1, 8, 16, 4), 7, FOLD),
    (1016, 100, (1, 8, 16, 4), 7, FOLD), (1017, 100, (1, 8, 16, 8), 13, FOLD),
]


# ---------------------------------------------------------------------------------------------------------------------
# problems and runners
# ---------------------------------------------------------------------------------------------------------------------
def _td_problem(T, B):
    g = _gen(T, B)
    return (_leaf(torch.randn(T + 1, B, device=DEV, generator=g)), torch.randn(T, B, device=DEV, generator=g),
            torch.rand(T, B, device=DEV, generator=g), g)


def _vt_problem(T, B):
    g = _gen(T, B, 1)
    to, bo, a, v, r = MR._vt_inputs(g, T, B, N)
    return to, bo, a, v, r, torch.rand(T, B, device=DEV, generator=g), g


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


def _td_unmasked(v, r, w):
    from hpc_rll.rl_utils.td import TDLambda
    loss = TDLambda(*r.shape)(v, r, w, 0.9, 0.8)
    (gv,) = torch.autograd.grad(loss, v)
    return loss.detach(), gv


def _td_masked(v, r, w, nvf, kw):
    from hpc_rll.rl_utils.td import masked_td_lambda
    if nvf:
        loss = masked_td_lambda(v[:-1], r, weight=w, gamma=0.9, lambda_=0.8, next_value=v[1:], **kw)
    else:
        loss = masked_td_lambda(v, r, weight=w, gamma=0.9, lambda_=0.8, **kw)
    (gv,) = torch.autograd.grad(loss, v)
    return loss.detach(), gv


VT_ARGS = (0.99, 0.95, 1.0, 0.9, 1.1)
VT_ORACLE = dict(gamma=0.99, lam=0.95, rho_clip=1.0, c_clip=0.9, pg_clip=1.1, co=MR.CO)


def _vt_grads(out, to, v):
    co = [torch.tensor([c], device=DEV) for c in MR.CO]
    gt, gv = torch.autograd.grad(list(out), (to, v), co)
    return [x.detach() for x in out], gt, gv


def _vt_unmasked(to, bo, a, v, r, w):
    from hpc_rll.rl_utils.vtrace import VTrace
    return _vt_grads(VTrace(r.shape[0], r.shape[1], N)(to, bo, a, v, r, w, *VT_ARGS), to, v)


def _vt_masked(to, bo, a, v, r, w, nvf, kw):
    from hpc_rll.rl_utils.vtrace import masked_vtrace
    g, lam, rho, c, pg = VT_ARGS
    common = dict(weight=w, gamma=g, lambda_=lam, rho_clip_ratio=rho, c_clip_ratio=c, rho_pg_clip_ratio=pg, **kw)
    if nvf:
        out = masked_vtrace(to, bo, a, v[:-1], r, next_value=v[1:], **common)
    else:
        out = masked_vtrace(to, bo, a, v, r, **common)
    return _vt_grads(out, to, v)


def _td_parity(got, oracle, what):
    assert rel_err(oracle[0].item(), got[0].item()) <= TOL, (what, "loss", oracle[0].item(), got[0].item())
    assert grad_err(_np(oracle[1]), _np(got[1]), "grad_value") <= 2 * TOL, what


def _vt_parity(got, oracle, what):
    for name, o, x in zip(("policy", "value", "entropy"), oracle[0], got[0]):
        assert rel_err(o, x.item()) <= TOL, (what, name, o, x.item())
    assert grad_err(_np(oracle[1]), _np(got[1]), "grad_target") <= 2 * TOL, what
    assert grad_err(_np(oracle[2]), _np(got[2]), "grad_value") <= 2 * TOL, what


def _same(a, b):
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------
# (a) + (b) unmasked scans: every configuration, and both sides of every threshold
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,B,cfg,grid,fin", [c[:5] for c in TD_CELLS] + TD_MORE)
def test_td_lambda_runs_the_expected_kernel(T, B, cfg, grid, fin):
    v, r, w, _ = _td_problem(T, B)
    what = f"TD(lambda) T={T} B={B}"
    with launches(TD, cfg, grid, fin, what=what):
        got = _td_unmasked(v, r, w)
    _td_parity(got, MR.td_oracle(v, r, weight=w, gamma=0.9, lam=0.8), what)
    with launches(TD, cfg, grid, fin, what=what):
        again = _td_unmasked(v, r, w)
    assert _same(got, again), what + ": not reproducible"
    cover(TD, cfg, None, "whole" if B % (64 * cfg[0] // cfg[3]) == 0 else "ragged", fin)


@pytest.mark.parametrize("T,B,cfg,grid,fin", [c[:5] for c in VT_CELLS] + VT_MORE)
def test_vtrace_runs_the_expected_kernel(T, B, cfg, grid, fin):
    to, bo, a, v, r, w, _ = _vt_problem(T, B)
    what = f"V-trace T={T} B={B}"
    with launches(VT, cfg, grid, fin, what=what):
        got = _vt_unmasked(to, bo, a, v, r, w)
    _vt_parity(got, MR.vtrace_oracle(to, bo, a, v, r, weight=w, **VT_ORACLE), what)
    with launches(VT, cfg, grid, fin, what=what):
        again = _vt_unmasked(to, bo, a, v, r, w)
    assert _same(got, again), what + ": not reproducible"
    cover(VT, cfg, None, "whole" if B % (64 // cfg[3]) == 0 else "ragged", fin)


@pytest.mark.parametrize("T,B,cfg,grid,fin", [c[:5] for c in VT_CELLS] + VT_MORE)
def test_upgo_runs_the_expected_kernel(T, B, cfg, grid, fin):
    from hpc_rll.rl_utils.upgo import UPGO as UpgoModule
    from test_scan_alignment_gpu import _upgo_problem
    base, a, l64, g64 = _upgo_problem(T, B)          # keeps the switch margin above 1e-3
    what = f"UPGO T={T} B={B}"
    res = []
    for _ in range(2):
        to = _leaf(base["to"])
        with launches(UPGO, cfg, grid, fin, what=what):
            loss = UpgoModule(T, B, N)(to, base["rho"], a, base["reward"], base["value"])
        (gt,) = torch.autograd.grad(loss, to)
        res.append((loss.detach(), gt))
    assert rel_err(l64.item(), res[0][0].item()) <= TOL, (what, l64.item(), res[0][0].item())
    assert grad_err(_np(g64), _np(res[0][1]), "grad_target") <= 2 * TOL, what
    assert _same(res[0], res[1]), what + ": not reproducible"
    cover(UPGO, cfg, None, "whole" if B % (64 // cfg[3]) == 0 else "ragged", fin)


# ---------------------------------------------------------------------------------------------------------------------
# (c) fold against finalize: grids of 2, exactly 512 and 513 workgroups; the 512-and-below grids again with the fold
# switched off (tune key 21), which must give the folded loss within the oracle bar.  T = 16: two chunks, two waves.
# ---------------------------------------------------------------------------------------------------------------------
FOLD_GRIDS = [(16, 100, 2, FOLD), (16, 32768, 512, FOLD), (16, 32770, 513, FINALIZE)]


@contextmanager
def fold_switched_off():
    import cabi
    assert cabi.lib.hpc_rll_tune_set(21, 0) == 0
    try:
        yield
    finally:
        assert cabi.lib.hpc_rll_tune_set(21, 1) == 0


@pytest.mark.parametrize("T,B,grid,fin", FOLD_GRIDS)
@pytest.mark.parametrize("op", [TD, VT, UPGO, MTD, MVT])
def test_fold_and_finalize_agree(op, T, B, grid, fin):
    from hpc_rll.rl_utils.upgo import UPGO as UpgoModule
    cfg = (1, 8, 2, 1)
    g = _gen(T, B, 2)
    form = (0, 0, 0)
    if op in (TD, MTD):
        v, r, w, _ = _td_problem(T, B)
        d, f = _masks(g, T, B)
        if op == TD:
            run = lambda: _td_unmasked(v, r, w)                                    # noqa: E731
            oracle = MR.td_oracle(v, r, weight=w, gamma=0.9, lam=0.8)
        else:
            form = (0, 2, 0)
            run = lambda: _td_masked(v, r, w, 0, {"done": d, "traj_flag": f})      # noqa: E731
            oracle = MR.td_oracle(v, r, done=d, traj_flag=f, weight=w, gamma=0.9, lam=0.8)
        parity, losses = _td_parity, (lambda x: [x[0]])
    elif op in (VT, MVT):
        to, bo, a, v, r, w, _ = _vt_problem(T, B)
        d, f = _masks(g, T, B)
        if op == VT:
            run = lambda: _vt_unmasked(to, bo, a, v, r, w)                         # noqa: E731
            oracle = MR.vtrace_oracle(to, bo, a, v, r, weight=w, **VT_ORACLE)
        else:
            form = (1, 1, 0)
            df = d.to(torch.float32)
            run = lambda: _vt_masked(to, bo, a, v, r, w, 0, {"done": df})          # noqa: E731
            oracle = MR.vtrace_oracle(to, bo, a, v, r, done=d, weight=w, **VT_ORACLE)
        parity, losses = _vt_parity, (lambda x: x[0])
    else:
        from test_scan_alignment_gpu import _upgo_problem
        base, a, l64, g64 = _upgo_problem(T, B)
        to = _leaf(base["to"])

        def run():
            loss = UpgoModule(T, B, N)(to, base["rho"], a, base["reward"], base["value"])
            return loss.detach(), torch.autograd.grad(loss, to)[0]

        def parity(got, _, what):
            assert rel_err(l64.item(), got[0].item()) <= TOL, (what, l64.item(), got[0].item())
            assert grad_err(_np(g64), _np(got[1]), "grad_target") <= 2 * TOL, what
        oracle, losses = None, (lambda x: [x[0]])
    what = f"{NAMES[op]} T={T} B={B} grid={grid}"
    with launches(op, cfg, grid, fin, form, what=what):
        first = run()
    with launches(op, cfg, grid, fin, form, what=what):
        second = run()
    assert _same(first, second), what + ": not reproducible"
    parity(first, oracle, what)
    FIN.setdefault(op, set()).add(fin)
    if fin == FOLD:
        with fold_switched_off():
            with launches(op, cfg, grid, FINALIZE, form, what=what + " fold off"):
                plain = run()
            with launches(op, cfg, grid, FINALIZE, form, what=what + " fold off"):
                plain2 = run()
        assert _same(plain, plain2), what + ": finalize path not reproducible"
        parity(plain, oracle, what + " fold off")
        for x, y in zip(losses(first), losses(plain)):
            assert rel_err(x.item(), y.item()) <= TOL, (what, "fold vs finalize", x.item(), y.item())
        assert _same(first[1:], plain[1:]), what + ": the gradients do not depend on who adds the partials"
        FIN[op].add(FINALIZE)


# ---------------------------------------------------------------------------------------------------------------------
# (d) masked TD(lambda) and V-trace: 14 mask forms x every configuration.  One oracle per (shape, mask mode), shared by
# the element types and the two input forms (next_value = value[1:] is the same problem).
# ---------------------------------------------------------------------------------------------------------------------
def _masked_cells(op, unmasked_op, T, B, cfg, grid, fin, kind, problem, run_unmasked, run_masked, oracle_of, parity):
    g = problem[-1]
    d, f = _masks(g, T, B)
    z = torch.zeros_like(d)
    tile_kind(cfg, B, kind)
    with launches(unmasked_op, cfg, grid, fin, what=f"{NAMES[unmasked_op]} T={T} B={B}"):
        ref = run_unmasked()
    for mm in range(4):
        oracle = oracle_of(_mask_kw(mm, d, f))
        for mt in ((0,) if mm == 0 else (0, 1)):
            kw = _mask_kw(mm, _typed(g, d, mt), _typed(g, f, mt))
            zkw = _mask_kw(mm, _typed(g, z, mt), _typed(g, z, mt))
            got = {}
            for nvf in (0, 1):
                form = (mt, mm, nvf)
                what = f"{NAMES[op]} T={T} B={B} form={form}"
                with launches(op, cfg, grid, fin, form, what=what):
                    got[nvf] = run_masked(nvf, kw)
                with launches(op, cfg, grid, fin, form, what=what + " zero masks"):
                    zero = run_masked(nvf, zkw)
                assert _same(zero, ref), what + ": all-zero masks do not give the unmasked op's bits"
                cover(op, cfg, form, kind, fin)
            assert _same(got[0], got[1]), f"{NAMES[op]} T={T} B={B} ({mt},{mm}): stacked and next-value bits differ"
            parity(got[0], oracle, f"{NAMES[op]} T={T} B={B} ({mt},{mm})")


@pytest.mark.parametrize("T,B,cfg,grid,fin,kind", TD_CELLS)
def test_masked_td_lambda_every_form(T, B, cfg, grid, fin, kind):
    p = _td_problem(T, B)
    v, r, w, _ = p
    _masked_cells(MTD, TD, T, B, cfg, grid, fin, kind, p, lambda: _td_unmasked(v, r, w),
                  lambda nvf, kw: _td_masked(v, r, w, nvf, kw),
                  lambda okw: MR.td_oracle(v, r, weight=w, gamma=0.9, lam=0.8, **okw), _td_parity)


@pytest.mark.parametrize("T,B,cfg,grid,fin,kind", VT_CELLS)
def test_masked_vtrace_every_form(T, B, cfg, grid, fin, kind):
    p = _vt_problem(T, B)
    to, bo, a, v, r, w, _ = p
    _masked_cells(MVT, VT, T, B, cfg, grid, fin, kind, p, lambda: _vt_unmasked(to, bo, a, v, r, w),
                  lambda nvf, kw: _vt_masked(to, bo, a, v, r, w, nvf, kw),
                  lambda okw: MR.vtrace_oracle(to, bo, a, v, r, weight=w, **okw, **VT_ORACLE), _vt_parity)


# ---------------------------------------------------------------------------------------------------------------------
# (e) masked GAE.  choose_cfg by hand, wgs = ceil(B / 64):
#   streaming (13 T B >= 300e6): two columns per lane with nontemporal loads and 4 waves when B is even and every pointer
#     8-byte aligned (forward 8-step, backward 16-step chunks), else one column per lane, 8 waves, nontemporal loads;
#   otherwise no nontemporal loads, one column per lane, 8-step chunks: 4 waves from wgs >= 512 (B >= 32705), 8 waves for
#     256 <= wgs < 512 (B >= 16321), 16 waves below, with half-wave (32-column) tiles when T >= 512.
# Rows: (T, B, offset in floats of value and grad_adv, forward (V, LC, NW, SUB, NTL), backward, grid, tile).
# 13 * 353 * 65536 = 300.7e6 and 13 * 352 * 65536 = 299.9e6.
# ---------------------------------------------------------------------------------------------------------------------
GAE_CELLS = [
    (8, 32768, 0, (1, 8, 4, 1, 0), (1, 8, 4, 1, 0), 512, "whole"), (8, 32770, 0, (1, 8, 4, 1, 0), (1, 8, 4, 1, 0), 513, "ragged"),
    (8, 16384, 0, (1, 8, 8, 1, 0), (1, 8, 8, 1, 0), 256, "whole"), (8, 20000, 0, (1, 8, 8, 1, 0), (1, 8, 8, 1, 0), 313, "ragged"),
    (40, 128, 0, (1, 8, 16, 1, 0), (1, 8, 16, 1, 0), 2, "whole"), (40, 100, 0, (1, 8, 16, 1, 0), (1, 8, 16, 1, 0), 2, "ragged"),
    (512, 64, 0, (1, 8, 16, 2, 0), (1, 8, 16, 2, 0), 2, "whole"), (600, 100, 0, (1, 8, 16, 2, 0), (1, 8, 16, 2, 0), 4, "ragged"),
    (353, 65536, 1, (1, 8, 8, 1, 1), (1, 8, 8, 1, 1), 1024, "whole"), (353, 65537, 0, (1, 8, 8, 1, 1), (1, 8, 8, 1, 1), 1025, "ragged"),
    (353, 65536, 0, (2, 8, 4, 1, 1), (2, 16, 4, 1, 1), 512, "whole"), (353, 65538, 0, (2, 8, 4, 1, 1), (2, 16, 4, 1, 1), 513, "ragged"),
]
GAE_CONFIGS = sorted({c[3] for c in GAE_CELLS})
assert len(GAE_CONFIGS) == 6
GAE_BOUNDARIES = [
    (8, 16320, (1, 8, 16, 1, 0), (1, 8, 16, 1, 0), 255), (8, 16321, (1, 8, 8, 1, 0), (1, 8, 8, 1, 0), 256),
    (8, 32704, (1, 8, 8, 1, 0), (1, 8, 8, 1, 0), 511), (8, 32705, (1, 8, 4, 1, 0), (1, 8, 4, 1, 0), 512),
    (511, 100, (1, 8, 16, 1, 0), (1, 8, 16, 1, 0), 2), (512, 100, (1, 8, 16, 2, 0), (1, 8, 16, 2, 0), 4),
    (352, 65536, (1, 8, 4, 1, 0), (1, 8, 4, 1, 0), 1024), (353, 65536, (2, 8, 4, 1, 1), (2, 16, 4, 1, 1), 512),
]
BIG = 1 << 22


def _dev_err(ref, got, gradient, what):
    """conftest.rel_err / grad_err restated on the device in fp64, for the streaming shapes (23 M elements per tensor)."""
    ref = torch.as_tensor(ref, device=DEV)
    got = got.to(torch.float64)
    assert ref.shape == got.shape, (what, ref.shape, got.shape)
    diff = (ref - got).abs()
    if not gradient:
        return float((diff / ref.abs().clamp(min=1.0)).max())
    assert bool(torch.isfinite(got).all()), what + ": gradient is not finite"
    scale, gmax = float(ref.abs().max()), float(got.abs().max())
    if scale == 0.0:
        assert gmax == 0.0, what + ": reference gradient is identically zero, result is not"
        return 0.0
    assert 0.5 * scale < gmax < 2.0 * scale, f"{what}: wrong magnitude: max|got| {gmax:.3e} vs max|ref| {scale:.3e}"
    return float(diff.max()) / scale


def _gae_close(ref, got, gradient, what):
    if got.numel() > BIG:
        e = _dev_err(ref, got, gradient, what)
    else:
        e = grad_err(ref, _np(got), what) if gradient else rel_err(ref, _np(got))
    assert e <= (2 * TOL if gradient else TOL), (what, e)


class GaeProblem:
    """Inputs of one (T, B) in guarded buffers, value and grad_adv `off` floats past a 16-byte boundary; the same buffers
    serve the C ABI and, as tensors, the Python op."""

    def __init__(self, T, B, off):
        g = _gen(T, B, 3)
        self.T, self.B, self.g = T, B, g
        v = torch.randn(T + 1, B, device=DEV, generator=g)
        self.v = GuardedF32(T + 1, B, off, DEV, v).t                 # stacked value
        self.v0 = GuardedF32(T, B, off, DEV, v[:-1]).t               # next-value form: value, next_value
        self.nv = GuardedF32(T, B, 0, DEV, v[1:]).t
        self.r = GuardedF32(T, B, 0, DEV, torch.randn(T, B, device=DEV, generator=g)).t
        self.ga = GuardedF32(T, B, off, DEV, torch.randn(T, B, device=DEV, generator=g)).t
        self.d, self.f = _masks(g, T, B)

    def oracle(self, mm):
        """fp64: adv, then (grad_value, grad_reward) of the stacked form and (grad_value, grad_next_value, grad_reward) of
        the next-value form.  One evaluation: the stacked value gradient is -d in rows t and gamma k^d d in rows t+1."""
        kw = _mask_kw(mm, self.d, self.f)
        adv, gvn, gr, gn = MG.oracle(self.v0, self.r, next_value=self.nv, grad=self.ga, **kw)
        gv = np.zeros((self.T + 1, self.B))
        gv[:self.T] += gvn
        gv[1:] += gn
        if self.T * self.B > BIG:
            adv, gv, gr, gvn, gn = (torch.from_numpy(x).to(DEV) for x in (adv, gv, gr, gvn, gn))
        return adv, {0: (gv, None, gr), 1: (gvn, gn, gr)}


def _c_forward(p, nvf, done, flag, mt):
    import cabi
    adv = GuardedF32(p.T, p.B, 0, DEV)
    value, nv = (p.v0, p.nv) if nvf else (p.v, None)
    st = cabi.lib.hpc_rll_gae_masked_forward(value.data_ptr(), cabi.ptr(nv), p.r.data_ptr(), cabi.ptr(done), cabi.ptr(flag),
                                             mt, adv.t.data_ptr(), p.T, p.B, MG.GAMMA, MG.LAM, cabi.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert st == 0, st
    return adv


def _c_backward(p, nvf, done, flag, mt, want=(True, True, True)):
    """-> guarded (grad_value, grad_next_value, grad_reward); the ones not wanted are allocated, NaN-filled and NOT passed."""
    import cabi
    bufs = [GuardedF32(p.T if nvf else p.T + 1, p.B, 0, DEV), GuardedF32(p.T, p.B, 0, DEV) if nvf else None,
            GuardedF32(p.T, p.B, 0, DEV)]
    ptrs = [b.t.data_ptr() if (b is not None and w) else 0 for b, w in zip(bufs, want)]
    st = cabi.lib.hpc_rll_gae_masked_backward(p.ga.data_ptr(), cabi.ptr(done), cabi.ptr(flag), mt, ptrs[0], ptrs[1], ptrs[2],
                                              0 if nvf else 1, p.T, p.B, MG.GAMMA, MG.LAM, cabi.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert st == 0, st
    return bufs


def _py(p, nvf, kw, need=(True, True, True)):
    """masked_gae on the same buffers -> (adv, [grad_value, grad_next_value, grad_reward] (None where not asked))."""
    from hpc_rll.rl_utils.gae import masked_gae
    value = (p.v0 if nvf else p.v).detach().requires_grad_(need[0])
    nv = p.nv.detach().requires_grad_(need[1]) if nvf else None
    reward = p.r.detach().requires_grad_(need[2])
    return value, nv, reward, masked_gae(value, reward, gamma=MG.GAMMA, lambda_=MG.LAM, next_value=nv, **kw)


@pytest.mark.parametrize("T,B,off,fwd,bwd,grid,kind", GAE_CELLS)
def test_masked_gae_every_form(T, B, off, fwd, bwd, grid, kind):
    tile_kind(fwd, B, kind)
    p = GaeProblem(T, B, off)
    subsets_at = {(0, 1), (1, 2)}                        # (element type, mask mode) of the NULL-gradient subsets
    for mm in range(4):
        o_adv, o_grads = p.oracle(mm)
        for mt in ((0,) if mm == 0 else (0, 1)):
            kw = _mask_kw(mm, _typed(p.g, p.d, mt), _typed(p.g, p.f, mt))
            done, flag = kw.get("done"), kw.get("traj_flag")
            advs = {}
            for nvf in (0, 1):
                form = (mt, mm, nvf)
                what = f"masked GAE T={T} B={B} off={off} form={form}"
                with launches(GF, fwd[:4], grid, 0, form, fwd[4], what + " forward"):
                    adv = _c_forward(p, nvf, done, flag, mt)
                adv.check(what + " adv")
                adv.assert_written(what + " adv")
                advs[nvf] = adv.t
                with launches(GB, bwd[:4], grid, 0, form, bwd[4], what + " backward"):
                    full = _c_backward(p, nvf, done, flag, mt)
                for name, buf, ref in zip(("grad_value", "grad_next_value", "grad_reward"), full, o_grads[nvf]):
                    if buf is None:
                        continue
                    buf.check(f"{what} {name}")
                    buf.assert_written(f"{what} {name}")
                    _gae_close(ref, buf.t, True, f"{what} {name}")
                # the autograd path on the same buffers: the same kernels, the same bits
                with launches(GF, fwd[:4], grid, 0, form, fwd[4], what + " masked_gae"):
                    value, nv, reward, py_adv = _py(p, nvf, kw)
                assert torch.equal(py_adv.detach(), adv.t), what + ": masked_gae and the C ABI differ"
                wrt = [value, nv, reward] if nvf else [value, reward]
                with launches(GB, bwd[:4], grid, 0, form, bwd[4], what + " masked_gae backward"):
                    py_g = torch.autograd.grad(py_adv, wrt, p.ga)
                for x, buf in zip(py_g, [b for b in full if b is not None]):
                    assert torch.equal(x, buf.t), what + ": autograd and C ABI gradients differ"
                cover(GF, fwd, form, kind)
                cover(GB, bwd, form, kind)
                if (mt, mm) in subsets_at:
                    _null_gradient_subsets(p, nvf, done, flag, mt, kw, full, bwd, grid, form, what)
                del full, py_g, py_adv
            assert torch.equal(advs[0], advs[1]), f"T={T} B={B} ({mt},{mm}): stacked and next-value forward bits differ"
            _gae_close(o_adv, advs[0], False, f"masked GAE T={T} B={B} ({mt},{mm}) adv")
    del p
    torch.cuda.empty_cache()


def _null_gradient_subsets(p, nvf, done, flag, mt, kw, full, bwd, grid, form, what):
    """Every non-empty proper subset of the gradient outputs (3 in the stacked form with the full set, 7 in the next-value
    form): what is asked for has the all-outputs bits, what is not passed is not touched."""
    slots = (0, 1, 2) if nvf else (0, 2)
    n = 0
    for bits in range(1, 1 << len(slots)):
        want = [False, False, False]
        for i, s in enumerate(slots):
            want[s] = bool(bits >> i & 1)
        with launches(GB, bwd[:4], grid, 0, form, bwd[4], f"{what} outputs={want}"):
            got = _c_backward(p, nvf, done, flag, mt, want)
        for s in slots:
            got[s].check(f"{what} outputs={want} slot {s}")
            if want[s]:
                assert torch.equal(got[s].t, full[s].t), f"{what} outputs={want}: slot {s} differs from the all-outputs run"
            else:
                got[s].assert_untouched(f"{what} outputs={want} slot {s}")
        n += 1
        del got
    assert n == (7 if nvf else 3)
    # through Python: an input without requires_grad gets no buffer (NULL), the others keep their bits
    for need in ((False, True, True), (True, True, False)):
        value, nv, reward, adv = _py(p, nvf, kw, need)
        wrt = [t for t in ((value, nv, reward) if nvf else (value, reward)) if t.requires_grad]
        refs = [full[s].t for s in slots if (value, nv, reward)[s].requires_grad]
        with launches(GB, bwd[:4], grid, 0, form, bwd[4], f"{what} requires_grad={need}"):
            grads = torch.autograd.grad(adv, wrt, p.ga)
        assert len(grads) == len(refs) and all(torch.equal(x, y) for x, y in zip(grads, refs)), (what, need)


@pytest.mark.parametrize("T,B,fwd,bwd,grid", GAE_BOUNDARIES)
def test_masked_gae_rule_boundaries(T, B, fwd, bwd, grid):
    p = GaeProblem(T, B, 0)
    byte = _typed(p.g, p.d, 0)
    what = f"masked GAE boundary T={T} B={B}"
    o_adv, o_grads = p.oracle(1)
    with launches(GF, fwd[:4], grid, 0, (0, 1, 0), fwd[4], what):
        value, _, reward, adv = _py(p, 0, {"done": byte})
    with launches(GB, bwd[:4], grid, 0, (0, 1, 0), bwd[4], what):
        gv, gr = torch.autograd.grad(adv, [value, reward], p.ga)
    _gae_close(o_adv, adv.detach(), False, what + " adv")
    _gae_close(o_grads[0][0], gv, True, what + " grad_value")
    _gae_close(o_grads[0][2], gr, True, what + " grad_reward")
    del p
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------------
# coverage: every cell, with a whole-tile and a ragged B
# ---------------------------------------------------------------------------------------------------------------------
EXEMPT = {
    (TD, (2, 8, 16, 1)): "V = 2 needs ceil(B/128) >= 512 workgroups, where at most 8 waves are chosen; not instantiated",
    (MTD, (2, 8, 16, 1)): "as TD(lambda): masked TD(lambda) runs its unmasked sibling's rule",
    (GF, "finalisation"): "the masked GAE forward has no loss sums (NACC = 0)",
    (GB, "finalisation"): "the masked GAE backward has no loss sums",
}


def test_coverage_of_every_cell():
    """Run the whole file: the cells are recorded by the tests above."""
    assert len(EXEMPT) == 4
    missing = []

    def need(op, cfg, form):
        got = COVER.get((op, cfg, form), set())
        if got != {"whole", "ragged"}:
            missing.append((NAMES[op], cfg, form, sorted(got)))

    unmasked = [(TD, c) for c in TD_CONFIGS] + [(op, c) for op in (VT, UPGO) for c in VT_CONFIGS]
    masked = [(MTD, c, f) for c in TD_CONFIGS for f in FORMS] + [(MVT, c, f) for c in VT_CONFIGS for f in FORMS]
    gae_bwd = sorted({c[4] for c in GAE_CELLS})
    gae = [(GF, c, f) for c in GAE_CONFIGS for f in FORMS] + [(GB, c, f) for c in gae_bwd for f in FORMS]
    assert (len(unmasked), len(masked), len(gae)) == (13 + 8 + 8, 294, 168)
    assert not any((op, c) in EXEMPT for op, c in unmasked) and not any((op, c) in EXEMPT for op, c, _ in masked)
    for op, cfg in unmasked:
        need(op, cfg, None)
    for op, cfg, form in masked + gae:
        need(op, cfg, form)
    for op in (TD, VT, UPGO, MTD, MVT):
        if FIN.get(op, set()) != {FOLD, FINALIZE}:
            missing.append((NAMES[op], "finalisation paths", sorted(FIN.get(op, set()))))
    assert not FIN.get(GF) and not FIN.get(GB)
    assert not missing, f"{len(missing)} cells were not run with both a whole-tile and a ragged B:\n" + \
                        "\n".join(map(str, missing))
    print(f"covered: {len(unmasked)} unmasked, {len(masked)} masked scan and {len(gae)} masked GAE cells, each with a "
          f"whole-tile and a ragged B; fold and finalize for 5 ops; {len(EXEMPT)} exemptions")
