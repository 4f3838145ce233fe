"""Every forward kernel the C51, IQN and QR-DQN dispatchers can pick (csrc/dist_ops.hip), called directly through the C ABI on
an MI355X (``-m gpu``) at the smallest batches that still exercise the tails, and compared with the fp64 oracle
(oracle/ref_torch.py) -- the kernel families against the oracle, not only against each other.

How a launch is checked.  Every operand and every output lives in a buffer with sentinel bands on both sides
(tests/guarded.py), outputs are pre-filled with NaN.  After EVERY forward launch: ``hpc_rll_dist_last_config`` shows exactly one
more launch of that op, the other two ops' records have not moved, and the record names the family, G, SW, FULL, the layout,
the grid and the kind of finalisation that the test holds as LITERALS (the family, G and FULL stand in the parametrize lists, the
grid is ``ceil(B / S)`` for the literal S of the case); both bands of every buffer are intact and the operands unchanged; no
NaN is left in ``loss``, ``td_err``, ``buf``.  The samples-per-wave kernels, which the dispatcher takes from B = 16384 / 32768 on,
are forced at these sizes with tune key 24 (restored in ``finally``), the separate finalize launch with key 21 = 0.

Batch sizes.  A kernel with S samples per workgroup runs at B in {1, S - 1, S + 1, 2 S + 5}: S = 4 SW for the samples-per-wave
kernels, 4 * 64 / G for the group kernels, 4 for the wave kernels.  None of these is a multiple of 64 / G, so the last wave holds
groups past the end of the batch (which store sample B - 1 a second time in the FULL instantiations) and, at B = 1 ... S - 1,
EVERY lane of phase A is clamped.  The last sample's action is N - 1 (N in {1, 3}; 4 and 5 where the IQN backward needs them): its
row ends where the guard band begins.  ``weight`` / ``value_gamma`` NULL or given, ``nstep`` in {0 with reward = NULL, 1, 3, 4, 8, 9}
(the reward loads come in clamped chunks of 8) and ``done`` binary or drawn from {0, 0, 0, 1, 0.5, -1, 3} are spread over the
cases by ``C51_AXES`` / ``Q_AXES``: every samples-per-wave width meets all of their rows.

Bars.  Against the fp64 oracle ``rel_err <= 2e-5`` on loss and td_err and ``grad_err <= 2e-5`` on buf against the action rows of
the AUTOGRAD gradient (the bar of test_c51_integral_positions_stay_outside_the_runs and of the IQN / QR-DQN oracle tests in
tests/test_losses_gpu.py).  Between families on the same inputs the bars tests/test_losses_gpu.py already pins: C51 BATCH against
WAVE64 buf within 4e-7 of the maximum (td_err, a 64-term sum in butterfly against DPP order, within 1e-6); QR-DQN BATCH against
GROUP buf bit for bit -- FULL included, which only a misaligned operand reaches --, QUAD against GROUP 4e-6, td_err 2e-6; the
two IQN layouts the same bits.  The backward entry points run once per case with a device scalar g = 1.75: the gradient is
``g * buf`` on the action row bit for bit and exactly 0 elsewhere.

C51 and fp64.  floor / ceil of the projected position is discontinuous, so the fp64 oracle is a reference only where every position
is exact in both precisions: supports whose delta_z is a power of two, gamma in {1, 0.5}, rewards that are multiples of 1/16 and
``done`` from the sets above (``C51_GRIDS``).  There no sample is left out.  On the usual grid (51 atoms on [-10, 10], gamma =
0.95) the reference is the fp32 oracle under the rule of test_dntd_oracle_reference_shape, with at most 1 % of the samples left out.

A width without a kernel.  ``hpc_rll_tune_set`` takes only 0, 1 and the four widths for key 24; behind it the dispatchers refuse
any other width the rule leaves above 1 with HPC_RLL_EUNSUPPORTED before anything is enqueued
(test_a_width_without_an_instantiation_is_refused writes the variable behind the key to get there).

Not covered, and why: 64-bit element offsets (B * N * n_atom >= 2^31) and the by-batch-size thresholds themselves (B >= 16384 /
32768 / 262144) need batches far outside a test of seconds; tests/test_full_size_gpu.py and the large-batch tests of
tests/test_losses_gpu.py and tests/test_fuzz_gpu.py stay the only cover of those.
"""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

from conftest import grad_err, rel_err
from guarded import GuardedF32, GuardedI64
from oracle import ref_torch as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 2e-5                                 # fp32 kernels against the fp64 oracle (tests/test_losses_gpu.py)
G_UP = 1.75                                # the device scalar grad_loss of the backward entry points
C51, IQN, QR = 0, 1, 2                     # HPC_RLL_DIST_OP_* (tests/test_dist_td_cpu.py asserts them against the header)
WAVE, GROUP, BATCH, QUAD, WAVE64, GENERAL = range(6)     # HPC_RLL_DIST_FAMILY_*
OP_NAMES = ("c51", "iqn", "qrdqn")
FAMILY_NAMES = ("WAVE", "GROUP", "BATCH", "QUAD", "WAVE64", "GENERAL")
FIELDS = ("count", "family", "g", "sw", "full", "layout", "grid", "folded")
DONE_SET = (0., 0., 0., 1., 0.5, -1., 3.)
WIDTHS = (8, 16, 32, 64)

COVER = set()      # (op, family, g, sw, full, layout) of every record this file has seen
WORST = {}         # (op name, family name) -> [worst loss, td_err, buf error against the oracle]


# ---------------------------------------------------------------------------------------------------------------------
# dispatch record, tune keys
# ---------------------------------------------------------------------------------------------------------------------
def last(op):
    import cabi
    out = (ctypes.c_int * 8)()
    assert cabi.lib.hpc_rll_dist_last_config(op, out) == 0
    return dict(zip(FIELDS, out))


def want(family, g, sw, full, layout, B, S, folded=1):
    """The literal record of a launch of B samples by a kernel with S samples per workgroup."""
    return dict(family=family, g=g, sw=sw, full=full, layout=layout, grid=-(-B // S), folded=folded)


class launches:
    """The body launches exactly one forward kernel of ``op`` and the record names the literal instantiation."""

    def __init__(self, op, rec, what):
        self.op, self.want, self.what = op, dict(rec), what

    def __enter__(self):
        self.want["count"] = last(self.op)["count"] + 1
        self.others = [last(o) for o in (C51, IQN, QR) if o != self.op]

    def __exit__(self, et, ev, tb):
        if et is None:
            rec = last(self.op)
            assert rec == self.want, (self.what, "ran", rec, "expected", self.want)
            assert [last(o) for o in (C51, IQN, QR) if o != self.op] == self.others, (self.what, "another op's record moved")
            COVER.add((self.op, rec["family"], rec["g"], rec["sw"], rec["full"], rec["layout"]))


@contextlib.contextmanager
def tuned(sw, fold=1):
    """Tune key 24 = ``sw`` (1: the per-sample kernels, 8 ... 64: samples per wave) and key 21 = ``fold`` for the body."""
    import cabi
    try:
        assert cabi.lib.hpc_rll_tune_set(24, sw) == 0 and cabi.lib.hpc_rll_tune_set(21, fold) == 0
        yield
    finally:
        assert cabi.lib.hpc_rll_tune_set(24, 0) == 0 and cabi.lib.hpc_rll_tune_set(21, 1) == 0


# ---------------------------------------------------------------------------------------------------------------------
# buffers
# ---------------------------------------------------------------------------------------------------------------------
class Operands:
    """The inputs of a case on the device, each between guard bands, float32 ones ``off`` floats past a 16-byte boundary."""

    def __init__(self):
        self.f, self.i = {}, {}

    def add(self, name, x, off=0):
        if x is not None:
            self.f[name] = (GuardedF32(1, x.numel(), off, DEV, src=x.reshape(1, -1).to(DEV)), x.clone())

    def add_actions(self, name, a):
        self.i[name] = GuardedI64(a, DEV)

    def ptr(self, name):
        if name in self.i:
            return self.i[name].t.data_ptr()
        return self.f[name][0].t.data_ptr() if name in self.f else None

    def check(self, what):
        for name, (g, x) in self.f.items():
            g.check(f"{what}: {name}")
            assert torch.equal(g.t.flatten().cpu(), x.flatten()), f"{what}: {name} was overwritten"
        for name, g in self.i.items():
            g.check(f"{what}: {name}")


class Outputs:
    def __init__(self, B, K, off_buf=0):
        self.B, self.K = B, K
        import cabi
        self.loss, self.td = GuardedF32(1, 1, 0, DEV), GuardedF32(1, B, 0, DEV)
        self.buf = GuardedF32(B, K, off_buf, DEV)
        self.partials = GuardedF32(1, int(cabi.lib.hpc_rll_partials_floats(B)), 0, DEV)

    def ptrs(self):
        return [x.t.data_ptr() for x in (self.loss, self.td, self.buf, self.partials)]

    def check(self, what):
        for name in ("loss", "td", "buf", "partials"):
            getattr(self, name).check(f"{what}: {name}")
        for name in ("loss", "td", "buf"):
            getattr(self, name).assert_written(f"{what}: {name}")

    def host(self):
        return float(self.loss.t.item()), self.td.t.flatten().cpu(), self.buf.t.cpu()


def forward(fn, op, ops, names, out, scalars, rec, what):
    import cabi
    with launches(op, rec, what):
        cabi.call(fn, DEV, *[ops.ptr(n) for n in names], *out.ptrs(), *scalars)
    torch.cuda.synchronize()
    ops.check(what)
    out.check(what)
    return out.host()


def backward(fn, op, ops, out, shape, dims, off, what):
    """One launch of a backward entry point on ``out.buf``: the gradient (of ``shape``) on the host; no record moves."""
    import cabi
    what = f"{what}: {fn}"
    g = GuardedF32(1, 1, 0, DEV, src=torch.tensor([[G_UP]], device=DEV))
    grad = GuardedF32(1, int(np.prod(shape)), off, DEV)
    before = [last(o) for o in (C51, IQN, QR)]
    kept = out.buf.t.clone()
    cabi.call(fn, DEV, g.t.data_ptr(), out.buf.t.data_ptr(), ops.ptr("action"), grad.t.data_ptr(), *dims)
    torch.cuda.synchronize()
    assert [last(o) for o in (C51, IQN, QR)] == before, (what, "a backward launch moved a forward record")
    for b in (g, grad, out.buf):
        b.check(what)
    ops.check(what)
    grad.assert_written(what)
    assert torch.equal(out.buf.t, kept) and float(g.t.item()) == G_UP, (what, "an input was overwritten")
    return grad.t.view(shape).cpu()


def onehot_rows(buf, a, N):
    """(B, N, K): g * buf on the action rows (one fp32 multiplication, as the kernels do it), exactly 0 elsewhere."""
    B, K = buf.shape
    ref = torch.zeros(B, N, K)
    ref[torch.arange(B), a] = torch.tensor(G_UP, dtype=torch.float32) * buf
    return ref


def note(op, family, errs):
    w = WORST.setdefault((OP_NAMES[op], FAMILY_NAMES[family]), [0.0, 0.0, 0.0])
    for i, e in enumerate(errs):
        w[i] = max(w[i], e)


def batch_sizes(S, G=64):
    sizes = (1, S - 1, S + 1, 2 * S + 5)
    assert all(b >= 1 and (G == 64 or b % (64 // G)) for b in sizes), sizes
    return sizes


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def f32(rng, *shape):
    return torch.from_numpy(rng.standard_normal(shape).astype(np.float32))


def draw_actions(rng, B, N):
    a = torch.from_numpy(rng.integers(0, N, B).astype(np.int64))
    a[0] = 0
    a[-1] = N - 1                                # the last sample's row ends where the guard band begins
    return a


def draw_done(rng, B, mode):
    if mode == "bin":
        return torch.from_numpy((rng.random(B) < 0.3).astype(np.float32))
    return torch.from_numpy(rng.choice(np.asarray(DONE_SET, dtype=np.float32), B))


# (gamma, nstep, done, weight given, N): gamma^nstep (1 - done) = 1, 0.5, 0.125, 1/16 on the samples with done = 0 -- runs of 1-2,
# 2, 8 and 16 sources, both ballot branches of the segmented scan --, +-2 gamma^nstep and 0.5 gamma^nstep on the non-binary ones,
# 0 on the terminal ones (one run of all atoms)
C51_AXES = [(1.0, 3, "bin", True, 3), (0.5, 1, "set", False, 1), (0.5, 3, "bin", False, 3), (0.5, 4, "set", True, 3),
            (1.0, 0, "bin", True, 1), (1.0, 8, "set", False, 3), (0.5, 9, "bin", True, 3), (1.0, 1, "set", True, 1)]
# n_atom -> (v_min, v_max) with delta_z a power of two
C51_GRIDS = {2: (0., 1.), 3: (-1., 1.), 17: (-8., 8.), 18: (-4.25, 4.25), 33: (-8., 8.), 51: (-12.5, 12.5), 64: (-32., 31.),
             65: (-8., 8.), 129: (-8., 8.)}
for _n, (_lo, _hi) in C51_GRIDS.items():
    assert np.log2((_hi - _lo) / (_n - 1)) % 1 == 0, _n


class C51Inputs:
    """``exact``: rewards are multiples of 1/16 whose n-step return spans ``reach`` x the support around its centre (clamped,
    integral sources at both ends); else standard normal times ``spread``."""

    def __init__(self, seed, B, N, n_atom, v_min, v_max, gamma, nstep, done, weighted, exact=True, reach=1.25, spread=4.0):
        rng = np.random.default_rng(seed)
        self.B, self.N, self.n_atom, self.v_min, self.v_max, self.gamma, self.nstep = B, N, n_atom, v_min, v_max, gamma, nstep
        self.dist = f32(rng, B, N, n_atom).abs() + 1e-3
        self.nd = f32(rng, B, N, n_atom).abs()
        self.a, self.na = draw_actions(rng, B, N), draw_actions(rng, B, N)
        if exact:
            c, h = 0.5 * (v_min + v_max), 0.5 * reach * (v_max - v_min)
            r = rng.integers(-16, 17, (nstep, B)) / 16.0
            if nstep:
                r[0] = rng.integers(int(np.floor((c - h) * 16)), int(np.ceil((c + h) * 16)) + 1, B) / 16.0
            self.r = torch.from_numpy(r.astype(np.float32))
        else:
            self.r = f32(rng, nstep, B) * spread
        self.done = draw_done(rng, B, done)
        self.w = torch.from_numpy(rng.random(B).astype(np.float32)) if weighted else None

    def oracle(self, dtype=torch.float64):
        """(loss, td_err, action rows of the autograd gradient) of the mean loss in ``dtype``."""
        d = self.dist.to(dtype).clone().requires_grad_(True)
        loss, per = R.dist_nstep_td_error(d, self.nd.to(dtype), self.a, self.na, self.r.to(dtype), self.done.to(dtype),
                                          None if self.w is None else self.w.to(dtype), self.gamma, self.v_min, self.v_max,
                                          self.n_atom)
        loss.backward()
        return loss.item(), per.detach(), d.grad[torch.arange(self.B), self.a]

    def place(self, off=0):
        ops = Operands()
        ops.add("dist", self.dist, off)
        ops.add("next_dist", self.nd, off)
        ops.add_actions("action", self.a)
        ops.add_actions("next_action", self.na)
        ops.add("reward", self.r if self.nstep else None)
        ops.add("done", self.done)
        ops.add("weight", self.w)
        return ops


C51_NAMES = ("dist", "next_dist", "action", "next_action", "reward", "done", "weight")


def c51_forward(inp, ops, sw, off=0, fold=1, what=""):
    """One forward launch with tune key 24 = ``sw`` -> (loss, td_err, buf) on the host and the output buffers."""
    fam, S = (GENERAL, 4) if inp.n_atom > 64 else (WAVE64, 4) if sw == 1 else (BATCH, 4 * sw)
    rec = want(fam, 64, sw if fam == BATCH else 0, 0, 0, inp.B, S, fold)
    out = Outputs(inp.B, inp.n_atom, off)
    with tuned(sw, fold):
        res = forward("hpc_rll_dist_nstep_td_forward", C51, ops, C51_NAMES, out,
                      [inp.nstep, inp.B, inp.N, inp.n_atom, inp.gamma, inp.v_min, inp.v_max, 1.0 / inp.B], rec,
                      f"{what} c51 {FAMILY_NAMES[fam]} sw={sw} B={inp.B} n_atom={inp.n_atom} off={off} fold={fold}")
    return res, out


def c51_backward(inp, ops, out, res, off, what):
    grad = backward("hpc_rll_dist_nstep_td_backward", C51, ops, out, (inp.B, inp.N, inp.n_atom), [inp.B, inp.N, inp.n_atom],
                    off, what)
    assert torch.equal(grad, onehot_rows(res[2], inp.a, inp.N)), (what, "grad_dist is not g * buf on the action rows, 0 elsewhere")


def against_oracle(op, family, ref, res, what, tol=TOL):
    (l_ref, p_ref, g_ref), (loss, td, buf) = ref, res
    errs = (rel_err(l_ref, loss), rel_err(p_ref.numpy(), td.numpy()), grad_err(g_ref.numpy(), buf.numpy(), "buf"))
    note(op, family, errs)
    print(f"{what}: loss / td_err / buf error against the oracle {errs[0]:.3g} {errs[1]:.3g} {errs[2]:.3g}")
    assert max(errs) <= tol, (what, errs)


def c51_families_agree(base, res, what):
    """BATCH against WAVE64 on the same inputs: the bars of test_c51_run_sum_projection_against_the_gather_kernel_and_the_oracle."""
    (l1, p1, g1), (l0, p0, g0) = base, res
    eg = float((g0 - g1).abs().max()) / max(float(g1.abs().max()), 1e-30)
    ep = float((p0 - p1).abs().max()) / max(float(p1.abs().max()), 1e-30)
    print(f"{what}: BATCH against WAVE64 buf {eg:.3g} td_err {ep:.3g} of the maximum")
    assert eg < 4e-7 and ep < 1e-6 and abs(l0 - l1) <= 1e-6 * abs(l1), (what, eg, ep, l0, l1)


# ---------------------------------------------------------------------------------------------------------------------
# C51
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sw", WIDTHS)
@pytest.mark.parametrize("n_atom", [2, 3, 18, 33, 51, 64])
def test_c51_samples_per_wave_kernel_on_exact_grids(n_atom, sw):
    """dist_nstep_fwd_batch_kernel<SW> and, on the same inputs, dist_nstep_fwd64_kernel<1>: each against the fp64 oracle, and
    against each other."""
    v_min, v_max = C51_GRIDS[n_atom]
    case = [2, 3, 18, 33, 51, 64].index(n_atom) * 4 + WIDTHS.index(sw)
    for k, B in enumerate(batch_sizes(4 * sw)):
        gamma, nstep, done, weighted, N = C51_AXES[(case + k) % 8]
        inp = C51Inputs(1000 * n_atom + 10 * sw + k, B, N, n_atom, v_min, v_max, gamma, nstep, done, weighted)
        ops, ref = inp.place(), inp.oracle()
        base, _ = c51_forward(inp, ops, 1)
        against_oracle(C51, WAVE64, ref, base, f"WAVE64 n_atom={n_atom} B={B}")
        res, out = c51_forward(inp, ops, sw)
        against_oracle(C51, BATCH, ref, res, f"BATCH sw={sw} n_atom={n_atom} B={B}")
        c51_families_agree(base, res, f"sw={sw} n_atom={n_atom} B={B}")
    c51_backward(inp, ops, out, res, 0, f"n_atom={n_atom} sw={sw}")


@pytest.mark.parametrize("n_atom", [2, 3, 18, 33, 51, 64, 65, 129])
def test_c51_wave_per_sample_kernels_on_exact_grids(n_atom):
    """dist_nstep_fwd64_kernel<1> (n_atom <= 64) and dist_nstep_fwd_kernel (above) at B = 1, 3, 5, 13 against the fp64 oracle."""
    v_min, v_max = C51_GRIDS[n_atom]
    fam = GENERAL if n_atom > 64 else WAVE64
    for k, B in enumerate(batch_sizes(4)):
        gamma, nstep, done, weighted, N = C51_AXES[(n_atom + k) % 8]
        inp = C51Inputs(77 * n_atom + k, B, N, n_atom, v_min, v_max, gamma, nstep, done, weighted)
        ops = inp.place()
        res, out = c51_forward(inp, ops, 1)
        against_oracle(C51, fam, inp.oracle(), res, f"{FAMILY_NAMES[fam]} n_atom={n_atom} B={B}")
    c51_backward(inp, ops, out, res, 0, f"n_atom={n_atom}")


@pytest.mark.parametrize("n_atom,sw", [(129, 1), (17, 1), (17, 8), (64, 64)])
def test_c51_operands_four_bytes_off_alignment(n_atom, sw):
    """dist, next_dist, buf and grad_dist each one float past a 16-byte boundary, one case per family (BATCH at both ends of
    its widths)."""
    v_min, v_max = C51_GRIDS[n_atom]
    for k, B in enumerate(batch_sizes(4 * sw)):
        gamma, nstep, done, weighted, N = C51_AXES[(2 * k + 3) % 8]
        inp = C51Inputs(31 * n_atom + sw + k, B, N, n_atom, v_min, v_max, gamma, nstep, done, weighted)
        ops = inp.place(off=1)
        res, out = c51_forward(inp, ops, sw, off=1)
        fam = GENERAL if n_atom > 64 else WAVE64 if sw == 1 else BATCH
        against_oracle(C51, fam, inp.oracle(), res, f"off=1 {FAMILY_NAMES[fam]} n_atom={n_atom} B={B}")
    c51_backward(inp, ops, out, res, 1, f"off=1 n_atom={n_atom} sw={sw}")


LEFT_OUT = []      # share of samples left out by the inexact-grid cases (printed by the coverage test)


@pytest.mark.parametrize("sw", (1,) + WIDTHS)
def test_c51_usual_grid_against_the_fp32_oracle(sw):
    """51 atoms on [-10, 10], gamma = 0.95: positions are inexact, so a return that rounds to the other side of an atom in another
    summation order moves a whole source.  The rule of test_dntd_oracle_reference_shape: a sample on which the fp32 and the fp64
    oracle differ by more than 1e-5 of the maximum is left out -- at most 1 % of the batch here --, every other sample and its
    gradient row agree with the fp32 oracle to 1e-4."""
    B, N, n_atom = 517, 3, 51
    inp = C51Inputs(4242 + sw, B, N, n_atom, -10., 10., 0.95, 3, "bin", True, exact=False)
    l32, p32, g32 = inp.oracle(torch.float32)
    _, p64, _ = inp.oracle()
    scale = float(p64.abs().max())
    edge = (p32.double() - p64).abs() > 1e-5 * scale
    LEFT_OUT.append(float(edge.double().mean()))
    print(f"sw={sw}: {int(edge.sum())} of {B} samples left out")
    assert float(edge.double().mean()) <= 0.01, float(edge.double().mean())
    ops = inp.place()
    (loss, td, buf), out = c51_forward(inp, ops, sw)
    ok = ~edge
    e_p = float((p32.double() - td.double())[ok].abs().max()) / scale
    e_g = grad_err(g32[ok].numpy(), buf[ok].numpy(), "buf")
    print(f"sw={sw}: td_err {e_p:.3g} of the maximum, buf {e_g:.3g}")
    assert e_p < 1e-4 and e_g < 1e-4, (sw, e_p, e_g)
    if not edge.any():
        assert rel_err(l32, loss) < 1e-4
    c51_backward(inp, ops, out, (loss, td, buf), 0, f"usual grid sw={sw}")


def test_c51_clamped_top_of_64_atoms_keeps_its_mass_in_fp32():
    """64 atoms on [-10, 10]: the fp32 quotient (v_max - v_min) / delta_z is one ulp BELOW 63, so a source clamped to v_max sits
    between atoms 62 and 63 in fp32 and keeps its mass, while in fp64 the position is integral (l == u) and the reference drops
    it.  With returns that leave the support the fp32 and the fp64 oracle differ on 21-46 % of the samples (measured on the oracle
    alone; 0.2 % at most at 51 atoms): fp64 is no reference here.  With gamma = 1, binary done and rewards that are multiples of
    1/16 the n-step sum is exact and the kernels' fp32 steps are those of the fp32 oracle, which is the reference, at the
    project's fp32-oracle bar (1e-4) with no sample left out; the families among themselves at 4e-7."""
    B, N, n_atom = 517, 3, 64
    inp = C51Inputs(6464, B, N, n_atom, -10., 10., 1.0, 3, "bin", True)
    l32, p32, g32 = inp.oracle(torch.float32)
    _, p64, _ = inp.oracle()
    differ = float(((p32.double() - p64).abs() > 1e-5 * float(p64.abs().max())).double().mean())
    print(f"fp32 and fp64 oracle differ on {100 * differ:.1f} % of the samples")
    assert differ > 0.05, differ                    # the inputs do reach the clamped top
    ops = inp.place()
    base = None
    for sw in (1,) + WIDTHS:
        (loss, td, buf), out = c51_forward(inp, ops, sw)
        scale = float(p32.abs().max())
        e_p = float((p32 - td).abs().max()) / scale
        e_g = grad_err(g32.numpy(), buf.numpy(), "buf")
        print(f"sw={sw}: against the fp32 oracle td_err {e_p:.3g} of the maximum, buf {e_g:.3g}, loss {rel_err(l32, loss):.3g}")
        assert e_p < 1e-4 and e_g < 1e-4 and rel_err(l32, loss) < 1e-4, (sw, e_p, e_g)
        if sw == 1:
            base = (loss, td, buf)
        else:
            c51_families_agree(base, (loss, td, buf), f"64 atoms on [-10, 10] sw={sw}")


@pytest.mark.parametrize("n_atom", [15, 57])
def test_c51_quotient_above_the_last_atom_stays_in_bounds(n_atom):
    """[-3.5, 1.25] with 15 or 57 atoms: the fp32 quotient (v_max - v_min) / delta_z is ABOVE n_atom - 1, so ceil gives atom index
    n_atom for a source clamped to v_max.  The reference would raise there (scatter_add_ out of range): no oracle.  The kernels
    must stay in bounds, leave finite outputs and agree with each other."""
    B, N = 261, 3
    inp = C51Inputs(350 + n_atom, B, N, n_atom, -3.5, 1.25, 1.0, 3, "bin", True, reach=2.0)
    top = (inp.r.sum(0) > 1.25).double().mean()
    assert top > 0.1, top                           # returns above v_max: every source of such a sample is clamped to the top
    ops = inp.place()
    base, _ = c51_forward(inp, ops, 1)
    for sw in WIDTHS:
        res, out = c51_forward(inp, ops, sw)
        for x in res[1:]:
            assert bool(torch.isfinite(x).all())
        c51_families_agree(base, res, f"[-3.5, 1.25] n_atom={n_atom} sw={sw}")
    c51_backward(inp, ops, out, res, 0, f"[-3.5, 1.25] n_atom={n_atom}")


# ---------------------------------------------------------------------------------------------------------------------
# QR-DQN
# ---------------------------------------------------------------------------------------------------------------------
# (nstep, done, weight given, value_gamma given, N)
Q_AXES = [(3, "bin", True, True, 3), (1, "set", False, False, 1), (0, "bin", False, True, 3), (8, "set", True, False, 3),
          (9, "bin", True, True, 1), (3, "set", False, True, 3), (1, "bin", True, False, 3), (9, "set", False, False, 1)]
GAMMA = 0.95


class QrInputs:
    def __init__(self, seed, B, N, tau, nstep, done, weighted, with_vg):
        rng = np.random.default_rng(seed)
        self.B, self.N, self.tau, self.nstep = B, N, tau, nstep
        self.q, self.nq = f32(rng, B, N, tau), f32(rng, B, N, tau)
        self.a, self.na = draw_actions(rng, B, N), draw_actions(rng, B, N)
        self.r = f32(rng, nstep, B)
        self.done = draw_done(rng, B, done)
        self.w = torch.from_numpy(rng.random(B).astype(np.float32)) if weighted else None
        self.vg = torch.from_numpy((0.9 + 0.1 * rng.random(B)).astype(np.float32)) if with_vg else None

    def oracle(self):
        q = self.q.double().requires_grad_(True)
        loss, per = R.qrdqn_nstep_td_error(q, self.nq.double(), self.a, self.na, self.r.double(), self.done.double(), self.tau,
                                           None if self.w is None else self.w.double(), GAMMA,
                                           None if self.vg is None else self.vg.double())
        loss.backward()
        return loss.item(), per.detach(), q.grad[torch.arange(self.B), self.a]

    def place(self, off_q=0, off_nq=0):
        ops = Operands()
        ops.add("q", self.q, off_q)
        ops.add("next_q", self.nq, off_nq)
        ops.add_actions("action", self.a)
        ops.add_actions("next_action", self.na)
        ops.add("reward", self.r if self.nstep else None)
        ops.add("done", self.done)
        ops.add("weight", self.w)
        ops.add("value_gamma", self.vg)
        return ops


QR_NAMES = ("q", "next_q", "action", "next_action", "reward", "done", "weight", "value_gamma")


def qr_forward(inp, ops, sw, rec, off_buf=0, fold=1, what=""):
    """One forward launch with tune key 24 = ``sw``; tau_value is the quantile count, as the Python op passes it by default."""
    out = Outputs(inp.B, inp.tau, off_buf)
    with tuned(sw, fold):
        res = forward("hpc_rll_qrdqn_nstep_td_forward", QR, ops, QR_NAMES, out,
                      [inp.tau, inp.nstep, inp.B, inp.N, GAMMA, float(inp.tau), 1.0 / inp.B], rec,
                      f"{what} qrdqn {FAMILY_NAMES[rec['family']]} G={rec['g']} sw={sw} full={rec['full']} tau={inp.tau} B={inp.B}")
    return res, out


def qr_backward(inp, ops, out, res, off, what):
    grad = backward("hpc_rll_qrdqn_nstep_td_backward", QR, ops, out, (inp.B, inp.N, inp.tau), [inp.tau, inp.B, inp.N], off, what)
    assert torch.equal(grad, onehot_rows(res[2], inp.a, inp.N)), (what, "grad_q is not g * buf on the action rows, 0 elsewhere")


def qr_group_want(G, B, fold=1):
    return want(GROUP, G, 0, 0, 0, B, 4 * (64 // G), fold)


def qr_families_agree(base, res, bitwise, what):
    """A samples-per-wave kernel against the group kernel: the bars of test_qrdqn_samples_per_wave_kernel_equals_group_kernel."""
    (l1, p1, g1), (l0, p0, g0) = base, res
    eg = float((g0 - g1).abs().max()) / float(g1.abs().max())
    ep = float((p0 - p1).abs().max()) / float(p1.abs().max())
    print(f"{what}: against GROUP buf {eg:.3g} td_err {ep:.3g} of the maximum")
    if bitwise:
        assert torch.equal(g0, g1), (what, eg, int((g0 != g1).sum()), (g0 != g1).nonzero()[:4].tolist())
    else:
        assert eg < 4e-6, (what, eg)
    assert ep < 2e-6 and abs(l0 - l1) <= 2e-6 * abs(l1), (what, ep, l0, l1)


def qr_samples_per_wave_case(family, G, sw, full, tau, case, offs=(0, 0, 0)):
    """The batch sizes of one (kernel, tau): GROUP and the samples-per-wave kernel on the same operands, each against the fp64
    oracle, then against each other; the backward on the last one.  ``offs``: floats q, next_q, buf are off alignment."""
    Gg = 8 if tau <= 8 else 16 if tau <= 16 else 32 if tau <= 32 else 64
    for k, B in enumerate(batch_sizes(4 * sw, G)):
        nstep, done, weighted, with_vg, N = Q_AXES[(case + k) % 8]
        inp = QrInputs(7919 * tau + 100 * sw + 10 * family + k, B, N, tau, nstep, done, weighted, with_vg)
        ops, ref = inp.place(offs[0], offs[1]), inp.oracle()
        base, _ = qr_forward(inp, ops, 1, qr_group_want(Gg, B), offs[2])
        against_oracle(QR, GROUP, ref, base, f"GROUP tau={tau} B={B}")
        res, out = qr_forward(inp, ops, sw, want(family, G, sw, full, 0, B, 4 * sw), offs[2])
        against_oracle(QR, family, ref, res, f"{FAMILY_NAMES[family]} G={G} sw={sw} full={full} tau={tau} B={B}")
        qr_families_agree(base, res, family == BATCH, f"{FAMILY_NAMES[family]} G={G} sw={sw} tau={tau} B={B}")
    qr_backward(inp, ops, out, res, offs[2], f"tau={tau} sw={sw}")


@pytest.mark.parametrize("tau", [65, 80])
def test_qrdqn_wave_kernel(tau):
    for k, B in enumerate(batch_sizes(4)):
        nstep, done, weighted, with_vg, N = Q_AXES[(tau + k) % 8]
        inp = QrInputs(tau + k, B, N, tau, nstep, done, weighted, with_vg)
        ops = inp.place()
        res, out = qr_forward(inp, ops, 0, want(WAVE, 64, 0, 0, 0, B, 4))
        against_oracle(QR, WAVE, inp.oracle(), res, f"WAVE tau={tau} B={B}")
    qr_backward(inp, ops, out, res, 0, f"tau={tau}")


@pytest.mark.parametrize("tau,G", [(1, 8), (5, 8), (8, 8), (9, 16), (16, 16), (17, 32), (32, 32), (39, 64), (64, 64)])
def test_qrdqn_group_kernel(tau, G):
    """qrdqn_fwd_group_kernel<G> as the dispatcher picks it at these sizes (tune key 24 = 0)."""
    for k, B in enumerate(batch_sizes(4 * (64 // G), G)):
        nstep, done, weighted, with_vg, N = Q_AXES[(tau + k) % 8]
        inp = QrInputs(3 * tau + k, B, N, tau, nstep, done, weighted, with_vg)
        ops = inp.place()
        res, out = qr_forward(inp, ops, 0, qr_group_want(G, B))
        against_oracle(QR, GROUP, inp.oracle(), res, f"GROUP tau={tau} B={B}")
    qr_backward(inp, ops, out, res, 0, f"tau={tau}")


@pytest.mark.parametrize("sw", WIDTHS)
@pytest.mark.parametrize("tau,G", [(3, 8), (7, 8), (9, 16), (13, 16), (17, 32), (31, 32), (33, 64), (63, 64)])
def test_qrdqn_batch_kernel_with_a_tail(tau, G, sw):
    """qrdqn_fwd_batch_kernel<G, SW, false>: tau < G."""
    qr_samples_per_wave_case(BATCH, G, sw, 0, tau, tau + WIDTHS.index(sw))


@pytest.mark.parametrize("sw", WIDTHS)
@pytest.mark.parametrize("tau", [8, 16, 32, 64])
def test_qrdqn_full_batch_kernel_through_a_misaligned_operand(tau, sw):
    """qrdqn_fwd_batch_kernel<G, SW, true>: tau == G, fully unrolled, the duplicate store of sample B - 1 without a branch.  Every
    such tau is a multiple of 4, so aligned operands take the quad kernel: one of q, next_q, buf is 4 bytes off here, each of
    them in turn over the cases."""
    which = ([8, 16, 32, 64].index(tau) + WIDTHS.index(sw)) % 3
    offs = tuple(1 if i == which else 0 for i in range(3))
    qr_samples_per_wave_case(BATCH, tau, sw, 1, tau, tau // 8 + WIDTHS.index(sw), offs)


@pytest.mark.parametrize("sw", WIDTHS)
@pytest.mark.parametrize("tau,G,full", [(8, 8, 0), (20, 8, 0), (28, 8, 0), (32, 8, 1), (36, 16, 0), (52, 16, 0), (64, 16, 1)])
def test_qrdqn_quad_kernel(tau, G, full, sw):
    """qrdqn_fwd_quad_kernel<G, SW, FULL>: four quantiles per lane, tau a multiple of 4 on aligned operands."""
    qr_samples_per_wave_case(QUAD, G, sw, full, tau, tau // 4 + WIDTHS.index(sw))


# ---------------------------------------------------------------------------------------------------------------------
# IQN
# ---------------------------------------------------------------------------------------------------------------------
KAPPA = 0.8


class IqnInputs:
    """q (tau,B,N), next_q (tau',B,N) as the default layout holds them; ``bnt`` places the permuted (B,N,tau) copies."""

    def __init__(self, seed, B, N, tau, taup, nstep, done, weighted, with_vg):
        rng = np.random.default_rng(seed)
        self.B, self.N, self.tau, self.taup, self.nstep = B, N, tau, taup, nstep
        self.q, self.nq = f32(rng, tau, B, N), f32(rng, taup, B, N)
        self.a, self.na = draw_actions(rng, B, N), draw_actions(rng, B, N)
        self.r = f32(rng, nstep, B)
        self.done = draw_done(rng, B, done)
        self.rq = torch.from_numpy(rng.random((tau, B)).astype(np.float32))
        self.w = torch.from_numpy(rng.random(B).astype(np.float32)) if weighted else None
        self.vg = torch.from_numpy((0.9 + 0.1 * rng.random(B)).astype(np.float32)) if with_vg else None

    def oracle(self):
        q = self.q.double().requires_grad_(True)
        loss, per = R.iqn_nstep_td_error(q, self.nq.double(), self.a, self.na, self.r.double(), self.done.double(),
                                         self.rq.double(), None if self.w is None else self.w.double(), GAMMA, KAPPA,
                                         None if self.vg is None else self.vg.double())
        loss.backward()
        return loss.item(), per.detach(), q.grad[:, torch.arange(self.B), self.a].transpose(0, 1).contiguous()

    def place(self, bnt):
        ops = Operands()
        ops.add("q", self.q.permute(1, 2, 0).contiguous() if bnt else self.q)
        ops.add("next_q", self.nq.permute(1, 2, 0).contiguous() if bnt else self.nq)
        ops.add_actions("action", self.a)
        ops.add_actions("next_action", self.na)
        ops.add("reward", self.r if self.nstep else None)
        ops.add("done", self.done)
        ops.add("replay_quantiles", self.rq)
        ops.add("weight", self.w)
        ops.add("value_gamma", self.vg)
        return ops


IQN_NAMES = ("q", "next_q", "action", "next_action", "reward", "done", "replay_quantiles", "weight", "value_gamma")


def iqn_forward(inp, ops, bnt, family, G, fold=1, what=""):
    S = 4 if family == WAVE else 4 * (64 // G)
    out = Outputs(inp.B, inp.tau)
    with tuned(0, fold):
        res = forward("hpc_rll_iqn_nstep_td_forward_bnt" if bnt else "hpc_rll_iqn_nstep_td_forward", IQN, ops, IQN_NAMES, out,
                      [inp.tau, inp.taup, inp.nstep, inp.B, inp.N, GAMMA, KAPPA, 1.0 / inp.B],
                      want(family, G, 0, 0, int(bnt), inp.B, S, fold),
                      f"{what} iqn {FAMILY_NAMES[family]} G={G} bnt={bnt} tau={inp.tau} tau'={inp.taup} B={inp.B}")
    return res, out


def iqn_backwards(inp, ops, ops_bnt, out, out_bnt, res, off, what):
    """Both backward entries: grad_q (tau,B,N) of the default layout, (B,N,tau) of the other."""
    rows = onehot_rows(res[2], inp.a, inp.N)                                       # (B, N, tau)
    grad = backward("hpc_rll_iqn_nstep_td_backward", IQN, ops, out, (inp.tau, inp.B, inp.N), [inp.tau, inp.B, inp.N], off, what)
    assert torch.equal(grad, rows.permute(2, 0, 1)), (what, "grad_q (tau,B,N) is not g * buf on the action columns, 0 elsewhere")
    grad = backward("hpc_rll_iqn_nstep_td_backward_bnt", IQN, ops_bnt, out_bnt, (inp.B, inp.N, inp.tau),
                    [inp.tau, inp.B, inp.N], off, what)
    assert torch.equal(grad, rows), (what, "grad_q (B,N,tau) is not g * buf on the action rows, 0 elsewhere")


def iqn_case(tau, taup, family, G, case, N=None, off_grad=0):
    for k, B in enumerate(batch_sizes(4 if family == WAVE else 4 * (64 // G), G)):
        nstep, done, weighted, with_vg, n = Q_AXES[(case + k) % 8]
        inp = IqnInputs(131 * tau + taup + k, B, N or n, tau, taup, nstep, done, weighted, with_vg)
        ref = inp.oracle()
        ops, ops_bnt = inp.place(False), inp.place(True)
        res, out = iqn_forward(inp, ops, False, family, G)
        against_oracle(IQN, family, ref, res, f"{FAMILY_NAMES[family]} G={G} tau={tau} tau'={taup} B={B}")
        res_bnt, out_bnt = iqn_forward(inp, ops_bnt, True, family, G)
        assert res_bnt[0] == res[0] and torch.equal(res_bnt[1], res[1]) and torch.equal(res_bnt[2], res[2]), \
            (tau, taup, B, "the two layouts differ on permuted inputs")
    iqn_backwards(inp, ops, ops_bnt, out, out_bnt, res, off_grad, f"tau={tau} tau'={taup}")


# tau decides G / tau' decides G; an odd tau' (the single-target tail of the pair loop), tau' = 1, tau = 1.  The default
# layout's backward takes the 16-byte plane kernel for N % 4 == 0 on an aligned grad_q (N = 4) and iqn_bwd_kernel otherwise:
# N % 4 != 0 (N = 1, 3, 5), or grad_q 4 bytes off (off_grad = 1 with N = 4)
@pytest.mark.parametrize("tau,taup,G,N,off_grad", [
    (8, 5, 8, 4, 0), (5, 8, 8, None, 0), (1, 1, 8, 4, 1), (16, 7, 16, None, 0), (9, 13, 16, 4, 0), (32, 1, 32, 5, 0),
    (1, 32, 32, 4, 1), (64, 33, 64, None, 0), (40, 64, 64, 4, 0)])
def test_iqn_group_kernel_both_layouts(tau, taup, G, N, off_grad):
    iqn_case(tau, taup, GROUP, G, tau + taup, N, off_grad)


@pytest.mark.parametrize("tau,taup,N,off_grad", [(65, 10, 4, 0), (10, 70, None, 0), (66, 67, 4, 1)])
def test_iqn_wave_kernel_both_layouts(tau, taup, N, off_grad):
    iqn_case(tau, taup, WAVE, 64, tau + taup, N, off_grad)


# ---------------------------------------------------------------------------------------------------------------------
# tune key 24 at a width that has no instantiation
# ---------------------------------------------------------------------------------------------------------------------
EINVAL, EUNSUPPORTED = -1, -3              # HPC_RLL_EINVAL, HPC_RLL_EUNSUPPORTED


@contextlib.contextmanager
def width_behind_key_24(sw):
    """``hpc_rll_tune_set(24, sw)`` itself answers HPC_RLL_EINVAL for a width without kernels (asserted here), so the dispatchers'
    own refusal is reached by writing the variable behind the key, the library's ``hpc_rll::g_sample_batch``; 0 in ``finally``."""
    import cabi
    var = ctypes.c_int.in_dll(cabi.lib, "_ZN7hpc_rll14g_sample_batchE")
    try:
        assert cabi.lib.hpc_rll_tune_set(24, sw) == EINVAL and var.value == 0
        var.value = sw
        yield
    finally:
        var.value = 0
        assert cabi.lib.hpc_rll_tune_set(24, 0) == 0


def refused(fn, ops, names, out, scalars, sw, what):
    """With the width ``sw`` behind tune key 24 the forward returns HPC_RLL_EUNSUPPORTED and has done nothing: no record moved, the
    NaN prefill of loss, td_err and buf is in place, every guard band is intact and the operands are unchanged."""
    import cabi
    what = f"{what} key 24 = {sw}"
    before = [last(o) for o in (C51, IQN, QR)]
    with width_behind_key_24(sw):
        status = getattr(cabi.lib, fn)(*[ops.ptr(n) for n in names], *out.ptrs(), *scalars, cabi.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert status == EUNSUPPORTED, (what, "returned", status)
    assert [last(o) for o in (C51, IQN, QR)] == before, (what, "a refused call moved a dispatch record")
    for name in ("loss", "td", "buf"):
        getattr(out, name).assert_untouched(f"{what}: {name}")
    for name in ("loss", "td", "buf", "partials"):
        getattr(out, name).check(f"{what}: {name}")
    ops.check(what)


def test_a_width_without_an_instantiation_is_refused():
    """The samples-per-wave kernels exist at 8 / 16 / 32 / 64.  hpc_rll_tune_set refuses any other width for key 24; should the
    variable behind the key hold one all the same (2, 12, 63 here), a forward whose rule leaves it above 1 refuses before anything
    is enqueued -- it used to launch nothing and return 0 with loss unwritten --, and where the rule itself brings the width down
    to 1 (n_atom > 64, or a width below 64 / G) the per-sample kernel runs as always."""
    B, N = 9, 3
    for sw in (2, 12, 63):
        inp = C51Inputs(2400 + sw, B, N, 51, *C51_GRIDS[51], 0.5, 3, "set", True)
        refused("hpc_rll_dist_nstep_td_forward", inp.place(), C51_NAMES, Outputs(B, 51),
                [inp.nstep, B, N, 51, inp.gamma, inp.v_min, inp.v_max, 1.0 / B], sw, "c51 n_atom=51")
        inp = C51Inputs(2465 + sw, B, N, 65, *C51_GRIDS[65], 0.5, 3, "set", True)
        with width_behind_key_24(sw):                               # n_atom > 64: the width is 1, GENERAL
            res = forward("hpc_rll_dist_nstep_td_forward", C51, inp.place(), C51_NAMES, Outputs(B, 65),
                          [inp.nstep, B, N, 65, inp.gamma, inp.v_min, inp.v_max, 1.0 / B], want(GENERAL, 64, 0, 0, 0, B, 4),
                          f"c51 n_atom=65 key 24 = {sw}")
        against_oracle(C51, GENERAL, inp.oracle(), res, f"GENERAL n_atom=65 B={B} key 24 = {sw}")
        inp = QrInputs(2440 + sw, B, N, 40, 3, "set", True, True)
        refused("hpc_rll_qrdqn_nstep_td_forward", inp.place(), QR_NAMES, Outputs(B, 40),
                [40, inp.nstep, B, N, GAMMA, 40.0, 1.0 / B], sw, "qrdqn tau=40")
        inp = QrInputs(2408 + sw, B, N, 8, 3, "set", True, True)
        if sw == 2:                                                 # below 64 / G = 8: the width is 1, GROUP
            with width_behind_key_24(sw):
                res = forward("hpc_rll_qrdqn_nstep_td_forward", QR, inp.place(), QR_NAMES, Outputs(B, 8),
                              [8, inp.nstep, B, N, GAMMA, 8.0, 1.0 / B], qr_group_want(8, B), f"qrdqn tau=8 key 24 = {sw}")
            against_oracle(QR, GROUP, inp.oracle(), res, f"GROUP tau=8 B={B} key 24 = {sw}")
        else:
            refused("hpc_rll_qrdqn_nstep_td_forward", inp.place(), QR_NAMES, Outputs(B, 8),
                    [8, inp.nstep, B, N, GAMMA, 8.0, 1.0 / B], sw, "qrdqn tau=8")


# ---------------------------------------------------------------------------------------------------------------------
# the separate finalize launch, the coverage of the whole file
# ---------------------------------------------------------------------------------------------------------------------
def same_but_for_the_total(res, folded):
    """The same kernel: td_err and buf bit for bit, the loss up to the fp32 rounding of the total."""
    assert abs(res[0] - folded[0]) <= 1e-6 * abs(folded[0]) and torch.equal(res[1], folded[1]) and torch.equal(res[2], folded[2])


def test_separate_finalisation_of_every_family():
    """Tune key 21 = 0: the kernels leave partials and finalize_sums adds them in a second launch.  One case per family; the record
    says so, the loss is the folded launch's up to the fp32 rounding of the total and the oracle's to 2e-5."""
    B = 69
    for n_atom, sws in ((129, (1,)), (33, (1, 16))):
        inp = C51Inputs(9 + n_atom, B, 3, n_atom, -8., 8., 0.5, 3, "set", True)
        ops, ref = inp.place(), inp.oracle()
        for sw in sws:
            folded, _ = c51_forward(inp, ops, sw)
            res, _ = c51_forward(inp, ops, sw, fold=0)
            fam = GENERAL if n_atom > 64 else WAVE64 if sw == 1 else BATCH
            against_oracle(C51, fam, ref, res, f"fold=0 c51 n_atom={n_atom} sw={sw}")
            same_but_for_the_total(res, folded)
    for tau, sw, rec in ((70, 0, want(WAVE, 64, 0, 0, 0, B, 4, 0)), (20, 1, qr_group_want(32, B, 0)),
                         (21, 8, want(BATCH, 32, 8, 0, 0, B, 32, 0)), (20, 8, want(QUAD, 8, 8, 0, 0, B, 32, 0))):
        inp = QrInputs(tau + sw, B, 3, tau, 3, "set", True, True)
        ops, ref = inp.place(), inp.oracle()
        folded, _ = qr_forward(inp, ops, sw, dict(rec, folded=1))
        res, _ = qr_forward(inp, ops, sw, rec, fold=0)
        against_oracle(QR, rec["family"], ref, res, f"fold=0 qrdqn tau={tau} sw={sw}")
        same_but_for_the_total(res, folded)
    for tau, family, G in ((70, WAVE, 64), (20, GROUP, 32)):
        inp = IqnInputs(tau, B, 3, tau, 9, 3, "set", True, True)
        ref = inp.oracle()
        for bnt in (False, True):
            ops = inp.place(bnt)
            folded, _ = iqn_forward(inp, ops, bnt, family, G)
            res, _ = iqn_forward(inp, ops, bnt, family, G, fold=0)
            against_oracle(IQN, family, ref, res, f"fold=0 iqn tau={tau} bnt={bnt}")
            same_but_for_the_total(res, folded)


def test_coverage_of_every_kernel():
    """Run the whole file: the records are collected by every launch above.  The literal set of (op, family, G, SW, FULL, layout)
    the dispatchers can pick -- 6 + 10 + 53 tuples; a threshold, alignment test or quad rule that moves a shape onto another
    kernel leaves one of them out."""
    expect = {(C51, GENERAL, 64, 0, 0, 0), (C51, WAVE64, 64, 0, 0, 0)} | {(C51, BATCH, 64, sw, 0, 0) for sw in WIDTHS}
    expect |= {(IQN, GROUP, G, 0, 0, lay) for G in (8, 16, 32, 64) for lay in (0, 1)} | {(IQN, WAVE, 64, 0, 0, lay) for lay in (0, 1)}
    expect |= {(QR, WAVE, 64, 0, 0, 0)} | {(QR, GROUP, G, 0, 0, 0) for G in (8, 16, 32, 64)}
    expect |= {(QR, BATCH, G, sw, full, 0) for G in (8, 16, 32, 64) for sw in WIDTHS for full in (0, 1)}
    expect |= {(QR, QUAD, G, sw, full, 0) for G in (8, 16) for sw in WIDTHS for full in (0, 1)}
    assert len(expect) == 6 + 10 + 1 + 4 + 32 + 16
    for key, (e_l, e_p, e_g) in sorted(WORST.items()):
        print(f"worst error against the oracle, {key[0]} {key[1]}: loss {e_l:.3g} td_err {e_p:.3g} buf {e_g:.3g}")
    if LEFT_OUT:
        print(f"usual C51 grid: {100 * min(LEFT_OUT):.2f} - {100 * max(LEFT_OUT):.2f} % of the samples left out")
    missing, extra = sorted(expect - COVER), sorted(COVER - expect)
    assert not missing and not extra, f"not run: {missing}\nnot expected: {extra}"
