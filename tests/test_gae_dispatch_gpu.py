"""Every GAE kernel the dispatcher of csrc/gae.hip can pick (run with ``-m gpu`` on an MI355X).

The expert entry points ``hpc_rll_gae_forward_ex`` / ``hpc_rll_gae_backward_ex`` are driven directly, every operand lives
in a guarded buffer (tests/guarded.py: sentinel bands on both sides, NaN-filled outputs) and every launch is followed by
  * ``hpc_rll_gae_last_config``: the kernel that ran is the kernel that was asked for (no clamp, no silent fall-back),
  * parity with the oracle (oracle/gae_ref.c; oracle.ref_torch in fp64 for the long trajectories),
  * both guard bands bit for bit intact and no NaN left in the output.
Groups: (a) every software-pipelined instantiation, bit-identical to the plain kernel of the same triple; (b) half-wave
tiles; (c) what the heuristic picks over a table of shapes, alignments and NULL gradients, with a per-family coverage
assertion; (d) long trajectories and degenerate coefficients with a bound measured from the oracles themselves.
Tolerances are the project's: 1e-5 (rel_err) for the advantage, 2e-5 for the gradients.
"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import rel_err
from guarded import GuardedF32, vmax_of
from test_gae_gpu import cref, oracle_fwd_bwd  # noqa: F401  (cref is a fixture)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 1e-5
EUNSUPPORTED = -3

PF_FWD = [(1, 8), (1, 16), (2, 4), (2, 8), (2, 16), (4, 4), (4, 8)]
PF_BWD = [(1, 8), (2, 2), (2, 4), (2, 8), (4, 2), (4, 4), (4, 8)]
PF_NW = (2, 4, 8)


def last_config(direction):
    import cabi
    out = (ctypes.c_int * 6)()
    assert cabi.lib.hpc_rll_gae_last_config(direction, out) == 0
    return dict(zip(("v", "lc", "nw", "flags", "half", "pipelined"), out))


def coef_table(T, gamma, lam):
    import hpc_rl_utils as U
    return U.gae_coef(T, gamma, lam, DEV)


class Problem:
    """Seeded inputs of one (T, B) on the device, and the sequential fp32 oracle's outputs for them."""

    def __init__(self, cref, T, B, gamma=0.99, lam=0.97, seed=0):
        g = torch.Generator(device=DEV).manual_seed(1000003 * T + B + seed)
        self.T, self.B, self.gamma, self.lam = T, B, gamma, lam
        self.v = torch.randn(T + 1, B, device=DEV, generator=g)
        self.r = torch.randn(T, B, device=DEV, generator=g)
        self.ga = torch.randn(T, B, device=DEV, generator=g)
        self.o_adv, self.o_gv, self.o_gr = oracle_fwd_bwd(cref, self.v.cpu().numpy(), self.r.cpu().numpy(),
                                                          self.ga.cpu().numpy(), gamma, lam)
        self.coef = coef_table(T, gamma, lam)


def forward(p, cfg, offs=(0, 0, 0)):
    """One forward launch on guarded operands -> (status, reported config, adv buffer, vmax of the pointers)."""
    import cabi
    T, B = p.T, p.B
    v = GuardedF32(T + 1, B, offs[0], DEV, p.v)
    r = GuardedF32(T, B, offs[1], DEV, p.r)
    adv = GuardedF32(T, B, offs[2], DEV)
    st = cabi.lib.hpc_rll_gae_forward_ex(v.t.data_ptr(), r.t.data_ptr(), adv.t.data_ptr(), p.coef.data_ptr(), T, B, p.gamma,
                                         *cfg, cabi.stream_ptr(DEV))
    torch.cuda.synchronize()
    return st, last_config(0), adv, vmax_of(B, v.t, r.t, adv.t)


def backward(p, cfg, offs=(0, 0, 0), want=(True, True)):
    """One backward launch -> (status, reported config, grad_value buffer or None, grad_reward buffer or None, vmax)."""
    import cabi
    T, B = p.T, p.B
    ga = GuardedF32(T, B, offs[0], DEV, p.ga)
    gv = GuardedF32(T + 1, B, offs[1], DEV) if want[0] else None
    gr = GuardedF32(T, B, offs[2], DEV) if want[1] else None
    st = cabi.lib.hpc_rll_gae_backward_ex(ga.t.data_ptr(), gv.t.data_ptr() if gv else 0, gr.t.data_ptr() if gr else 0,
                                          p.coef.data_ptr(), T, B, p.gamma, *cfg, cabi.stream_ptr(DEV))
    torch.cuda.synchronize()
    return st, last_config(1), gv, gr, vmax_of(B, ga.t, gv.t if gv else None, gr.t if gr else None)


def check_out(buf, ref, tol, what):
    """Assertions 3 and 5 of every call: guard bands intact, every element written, oracle parity."""
    buf.check(what)
    buf.assert_written(what)
    e = rel_err(ref, buf.t.cpu().numpy())
    assert e < tol, (what, e)


def ran(cfg, v, lc, nw, half=0, pipelined=0):
    return (cfg["v"], cfg["lc"], cfg["nw"], cfg["half"], cfg["pipelined"]) == (v, lc, nw, half, pipelined)


# --------------------------------------------------------------------------------------------------------------------
# (a) every pipelined instantiation
# --------------------------------------------------------------------------------------------------------------------
def _t_grid(lc, nw):
    """One step, under one chunk, exactly one workgroup span, one more, several spans not a multiple of lc."""
    return sorted({1, lc - 1, nw * lc, nw * lc + 1, 3 * nw * lc + lc - 1})


def _b_grid(vec):
    """Whole tiles (the FULLB = true kernels), ragged last tile after several whole ones, less than one tile."""
    grid = (512, 516, 12)
    assert grid[0] % (64 * vec) == 0 and grid[1] % (64 * vec) != 0 and grid[1] > 64 * vec and grid[2] < 64 * vec
    assert all(b % 4 == 0 for b in grid)          # no clamp of vec on B's account
    return grid


@pytest.mark.parametrize("vec,lc", PF_FWD)
def test_pipelined_forward_every_instantiation(cref, vec, lc):
    n = 0
    for nw in PF_NW:
        for T in _t_grid(lc, nw):
            for B in _b_grid(vec):
                p = Problem(cref, T, B)
                for fl in (2, 3):
                    what = f"fwd pf ({vec},{lc},{nw}) flags 8|{fl} T={T} B={B}"
                    st, cfg, adv, _ = forward(p, (vec, lc, nw, 8 | fl))
                    assert st == 0, (what, st)
                    assert ran(cfg, vec, lc, nw, pipelined=1) and cfg["flags"] == fl, (what, cfg)
                    check_out(adv, p.o_adv, TOL, what)
                    st, cfg, plain, _ = forward(p, (vec, lc, nw, fl))
                    assert st == 0 and ran(cfg, vec, lc, nw), (what, "plain", st, cfg)
                    check_out(plain, p.o_adv, TOL, what + " plain")
                    assert torch.equal(adv.t, plain.t), what + ": not the plain kernel's bits"
                    n += 1
    assert n == 2 * 3 * sum(len(_t_grid(lc, nw)) for nw in PF_NW)


@pytest.mark.parametrize("vec,lc", PF_BWD)
def test_pipelined_backward_every_instantiation(cref, vec, lc):
    n = 0
    for nw in PF_NW:
        for T in _t_grid(lc, nw):
            for B in _b_grid(vec):
                p = Problem(cref, T, B)
                for fl in (2, 3):
                    what = f"bwd pf ({vec},{lc},{nw}) flags 8|{fl} T={T} B={B}"
                    st, cfg, gv, gr, _ = backward(p, (vec, lc, nw, 8 | fl))
                    assert st == 0, (what, st)
                    assert ran(cfg, vec, lc, nw, pipelined=1) and cfg["flags"] == fl, (what, cfg)
                    check_out(gv, p.o_gv, 2 * TOL, what + " grad_value")
                    check_out(gr, p.o_gr, 2 * TOL, what + " grad_reward")
                    st, cfg, pv, pr, _ = backward(p, (vec, lc, nw, fl))
                    assert st == 0 and ran(cfg, vec, lc, nw), (what, "plain", st, cfg)
                    check_out(pv, p.o_gv, 2 * TOL, what + " plain grad_value")
                    check_out(pr, p.o_gr, 2 * TOL, what + " plain grad_reward")
                    assert torch.equal(gv.t, pv.t) and torch.equal(gr.t, pr.t), what + ": not the plain kernel's bits"
                    n += 1
    assert n == 2 * 3 * sum(len(_t_grid(lc, nw)) for nw in PF_NW)


def test_pipelined_request_outside_the_instantiated_set_is_refused(cref):
    """flags bit 3 with a triple the pipelined kernels are not built for: HPC_RLL_EUNSUPPORTED, nothing written."""
    p = Problem(cref, 40, 256)
    refused = [0, 0]
    for vec in (1, 2, 4):
        for lc in (2, 4, 8, 16):
            for nw in (1, 2, 4, 8, 16):
                for fl in (8 | 2, 8 | 3):
                    if not ((vec, lc) in PF_FWD and nw in PF_NW):
                        st, _, adv, _ = forward(p, (vec, lc, nw, fl))
                        assert st == EUNSUPPORTED, ("fwd", vec, lc, nw, fl, st)
                        adv.assert_untouched(f"fwd ({vec},{lc},{nw})")
                        adv.check()
                        refused[0] += 1
                    if not ((vec, lc) in PF_BWD and nw in PF_NW):
                        st, _, gv, gr, _ = backward(p, (vec, lc, nw, fl))
                        assert st == EUNSUPPORTED, ("bwd", vec, lc, nw, fl, st)
                        gv.assert_untouched(f"bwd ({vec},{lc},{nw})")
                        gr.assert_untouched(f"bwd ({vec},{lc},{nw})")
                        gv.check()
                        gr.check()
                        refused[1] += 1
    assert refused == [2 * (60 - 21), 2 * (60 - 21)]
    # bit 3 needs all of vec, lc and nw: a request that leaves any to the heuristic is refused too, whatever it would pick
    for cfg_in in ((0, 0, 0, 8 | 2), (0, 8, 4, 8 | 3), (2, 0, 4, 8 | 2), (2, 4, 0, 8 | 2)):
        st, _, adv, _ = forward(p, cfg_in)
        assert st == EUNSUPPORTED, ("fwd", cfg_in, st)
        adv.assert_untouched(f"fwd {cfg_in}")
        st, _, gv, gr, _ = backward(p, cfg_in)
        assert st == EUNSUPPORTED, ("bwd", cfg_in, st)
        gv.assert_untouched(f"bwd {cfg_in}")
        gr.assert_untouched(f"bwd {cfg_in}")


@pytest.mark.parametrize("fl", [0, 1, 2, 3])
@pytest.mark.parametrize("want", [(False, True), (True, False)])
def test_pipelined_backward_with_a_null_gradient_runs_the_plain_kernel_as_asked(cref, fl, want):
    """The pipelined backward writes both gradients; with one of them NULL the plain kernel of the same triple runs with
    the load / store flags that were given (not the nontemporal stores the pipelined kernel implies), and is reported."""
    p = Problem(cref, 300, 516)
    st, cfg, gv, gr, _ = backward(p, (2, 4, 4, 8 | fl), want=want)
    assert st == 0 and ran(cfg, 2, 4, 4, pipelined=0) and cfg["flags"] == fl, (st, cfg)
    if gv:
        check_out(gv, p.o_gv, 2 * TOL, "grad_value")
    if gr:
        check_out(gr, p.o_gr, 2 * TOL, "grad_reward")


# --------------------------------------------------------------------------------------------------------------------
# (b) half-wave tiles: 32-column tiles, 32 virtual waves of lc steps per workgroup
# --------------------------------------------------------------------------------------------------------------------
HALF_B = (1, 31, 32, 33, 64, 100, 2050)
HALF_T = (1, 15, 16, 17, 512, 513, 1500)


@pytest.mark.parametrize("B", HALF_B)
def test_half_wave_tiles(cref, B):
    for T in HALF_T:
        p = Problem(cref, T, B)
        for lc in (8, 16):
            for f in range(4):
                what = f"half (1,{lc},16) flags 4|{f} T={T} B={B}"
                st, cfg, adv, _ = forward(p, (1, lc, 16, 4 | f))
                assert st == 0 and ran(cfg, 1, lc, 16, half=1), (what, st, cfg)
                check_out(adv, p.o_adv, TOL, what + " adv")
                st, cfg, gv, gr, _ = backward(p, (1, lc, 16, 4 | f))
                assert st == 0 and ran(cfg, 1, lc, 16, half=1), (what, st, cfg)
                check_out(gv, p.o_gv, 2 * TOL, what + " grad_value")
                check_out(gr, p.o_gr, 2 * TOL, what + " grad_reward")


@pytest.mark.parametrize("triple", [(1, 8, 8), (1, 4, 16), (2, 8, 16)])
def test_half_wave_request_with_an_illegal_triple_reports_what_ran(cref, triple):
    p = Problem(cref, 300, 100)
    st, cfg, adv, _ = forward(p, (*triple, 4 | 2))
    assert st == 0 and ran(cfg, *triple, half=0), (st, cfg)
    check_out(adv, p.o_adv, TOL, f"fwd {triple}")
    st, cfg, gv, gr, _ = backward(p, (*triple, 4 | 2))
    assert st == 0 and ran(cfg, *triple, half=0), (st, cfg)
    check_out(gv, p.o_gv, 2 * TOL, f"bwd {triple} grad_value")
    check_out(gr, p.o_gr, 2 * TOL, f"bwd {triple} grad_reward")


# --------------------------------------------------------------------------------------------------------------------
# (c) what the heuristic picks, and that it is right
# --------------------------------------------------------------------------------------------------------------------
def _streaming_T(B):
    """Smallest T with 12*T*B >= 300e6 (choose_cfg's streaming regime)."""
    T = int(np.ceil(300e6 / (12.0 * B)))
    assert 12.0 * T * B >= 300e6 > 12.0 * (T - 1) * B
    return T


T64K = _streaming_T(65536)
# (T, B, operand offsets in floats (forward: value, reward, adv; backward: grad_adv, grad_value, grad_reward),
#  backward outputs wanted (grad_value, grad_reward))
AUTO_TABLE = (
    [(100, 257, (0, 0, 0), (True, True)),                    # cache-resident plain
     (1024, 64, (0, 0, 0), (True, True)),                    # half-wave tiles
     (1024, 20000, (0, 0, 0), (True, True)),                 # cache-resident pipelined, ragged last tile
     (512, 16384, (0, 0, 0), (True, True))]                  # cache-resident pipelined, whole tiles
    + [(_streaming_T(B), B, (0, 0, 0), (True, True)) for B in (32768, 65536, 131072, 262144)]
    + [(T64K, B, (0, 0, 0), (True, True)) for B in (65537, 65538, 65540)]     # vmax 1, 2, 4 with a ragged tile
    + [(T64K, 65536, tuple(off if k == i else 0 for k in range(3)), (True, True)) for i in range(3) for off in (1, 2)]
    + [(T64K, 65536, (0, 0, 0), (False, True)), (T64K, 65536, (0, 0, 0), (True, False))]   # pipelined -> plain backward
    + [(8, 4194304, (0, 0, 0), (True, True))]                # nw cut to 1: pipelining switches itself off
)
FAMILIES = ("plain v=1", "plain v=2", "v=4", "half-wave", "pipelined whole tiles", "pipelined ragged tile")


def _families(cfg, B):
    out = set()
    if cfg["half"]:
        out.add("half-wave")
    if cfg["pipelined"]:
        out.add("pipelined whole tiles" if B % (64 * cfg["v"]) == 0 else "pipelined ragged tile")
    elif not cfg["half"] and cfg["v"] in (1, 2):
        out.add(f"plain v={cfg['v']}")
    if cfg["v"] == 4:
        out.add("v=4")
    return out


@pytest.mark.parametrize("direction", ["forward", "backward"])
def test_auto_dispatch_table_and_family_coverage(cref, direction):
    """Every row: status 0, reported v <= the vmax of B and the pointers, oracle parity, guards.  The (lc, nw) the
    heuristic returns are not pinned; instead every kernel family must have been reached by some row."""
    AUTO = (0, 0, 0, -1)
    reached, failures, last, p = {}, [], None, None
    for T, B, offs, want in AUTO_TABLE:
        if direction == "forward" and want != (True, True):
            continue
        if (T, B) != last:                                   # rows of one shape are adjacent: one shape alive at a time
            last, p = (T, B), Problem(cref, T, B)
        what = f"{direction} auto T={T} B={B} offsets={offs} outputs={want}"
        try:
            if direction == "forward":
                st, cfg, adv, vmax = forward(p, AUTO, offs)
                assert st == 0, (what, st)
                assert cfg["v"] <= vmax, (what, cfg, vmax)
                check_out(adv, p.o_adv, TOL, what)
            else:
                st, cfg, gv, gr, vmax = backward(p, AUTO, offs, want)
                assert st == 0, (what, st)
                assert cfg["v"] <= vmax, (what, cfg, vmax)
                if want != (True, True):
                    assert not cfg["pipelined"], (what, "the pipelined backward writes both gradients", cfg)
                if gv:
                    check_out(gv, p.o_gv, 2 * TOL, what + " grad_value")
                if gr:
                    check_out(gr, p.o_gr, 2 * TOL, what + " grad_reward")
            if T == 8:
                assert cfg["nw"] == 1 and not cfg["pipelined"], (what, cfg)
            print(f"{what}: {cfg} vmax={vmax}")
            for fam in _families(cfg, B):
                reached.setdefault(fam, []).append((T, B, offs, cfg["v"], cfg["lc"], cfg["nw"]))
        except AssertionError as e:                          # every row is asserted: collect, report all at the end
            failures.append(f"{what}: {e}")
    assert not failures, "\n".join(failures)
    for fam in FAMILIES:
        assert fam in reached, f"{direction}: no row of AUTO_TABLE reaches the '{fam}' kernels any more: add a shape " \
                               f"that does (reached: {sorted(reached)})"
    print(f"{direction}: families reached: " + "; ".join(f"{f}: {len(reached[f])} rows" for f in FAMILIES))


# --------------------------------------------------------------------------------------------------------------------
# (d) long trajectories, degenerate coefficients
# --------------------------------------------------------------------------------------------------------------------
def _fp64(v, r, ga, gamma, lam):
    from oracle import ref_torch as R
    adv = R.gae(v.double().cpu(), r.double().cpu(), gamma, lam)
    gv, gr = R.gae_backward(ga.double().cpu(), gamma, lam)
    return adv.numpy(), gv.numpy(), gr.numpy()


@pytest.mark.parametrize("T", [4097, 10000])
@pytest.mark.parametrize("B", [3, 130])
@pytest.mark.parametrize("gamma,lam", [(0.99, 0.97), (1.0, 1.0), (1.0, 0.0), (0.5, 0.0)])
def test_long_trajectories_and_degenerate_coefficients(cref, T, B, gamma, lam):
    """Hundreds of passes through the double-buffered LDS carry slot (T <= 2000 elsewhere), lambda = 0 (every chunk
    product is 0) and lambda = 1 (coefficients (k-1)/k), auto-dispatched and as (1,16,16).

    These lie outside the envelope the project tolerances were set for, so the bound is measured, not assumed: the error
    of the sequential fp32 oracle (oracle/gae_ref.c) against the fp64 oracle (oracle.ref_torch) on the same inputs,
    times 4 (chunked re-association of an affine scan changes the rounding order, not the error's growth law; a wrong
    carry is off by orders of magnitude), floored at the project tolerance (1e-5 advantage, 2e-5 gradients).  Both
    oracles and the kernel get the same fp32-rounded gamma and lambda.  Run with ``-s`` for the figures.

    Measured on an MI355X, largest over the four (T, B): fp32 oracle vs fp64 -> kernel vs fp64 (adv, grad_value,
    grad_reward; auto and (1,16,16) give the same bits: the carry walk is sequential whatever the workgroup span):
      gamma 0.99 lambda 0.97: 4.8e-6 2.2e-6 5.0e-6 -> 3.4e-6 1.5e-6 3.3e-6   (inside the project tolerance)
      gamma 1    lambda 1   : 1.1e-4 2.1e-5 1.4e-4 -> 1.1e-4 2.1e-5 1.4e-4   (worst kernel / bound: 0.56, T=10000 B=3)
      gamma 1    lambda 0   : 2.4e-7 6.0e-8 0      -> 2.4e-7 6.0e-8 0
      gamma 0.5  lambda 0   : 1.7e-7 6.0e-8 0      -> 1.7e-7 6.0e-8 0
    """
    gamma, lam = float(np.float32(gamma)), float(np.float32(lam))
    p = Problem(cref, T, B, gamma, lam)
    r_adv, r_gv, r_gr = _fp64(p.v, p.r, p.ga, gamma, lam)
    base = (rel_err(r_adv, p.o_adv), rel_err(r_gv, p.o_gv), rel_err(r_gr, p.o_gr))
    bound = (max(TOL, 4 * base[0]), max(2 * TOL, 4 * base[1]), max(2 * TOL, 4 * base[2]))
    for cfg_in in ((0, 0, 0, -1), (1, 16, 16, -1)):
        what = f"T={T} B={B} gamma={gamma:g} lambda={lam:g} cfg={cfg_in}"
        st, cfg, adv, _ = forward(p, cfg_in)
        assert st == 0, (what, st)
        st, cfg_b, gv, gr, _ = backward(p, cfg_in)
        assert st == 0, (what, st)
        if cfg_in[0]:
            assert ran(cfg, 1, 16, 16) and ran(cfg_b, 1, 16, 16), (what, cfg, cfg_b)
        got = []
        for buf in (adv, gv, gr):
            buf.check(what)
            buf.assert_written(what)
            got.append(buf.t.cpu().numpy())
        err = (rel_err(r_adv, got[0]), rel_err(r_gv, got[1]), rel_err(r_gr, got[2]))
        print(f"{what}: fwd {cfg} bwd {cfg_b}\n    fp32 oracle vs fp64 (adv, grad_value, grad_reward) = "
              f"{base[0]:.3e} {base[1]:.3e} {base[2]:.3e}; kernel vs fp64 = {err[0]:.3e} {err[1]:.3e} {err[2]:.3e}; "
              f"bound = {bound[0]:.3e} {bound[1]:.3e} {bound[2]:.3e}")
        for name, e, b in zip(("adv", "grad_value", "grad_reward"), err, bound):
            assert e <= b, (what, name, e, b)
