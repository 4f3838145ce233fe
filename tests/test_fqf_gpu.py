"""GPU tier of FQF (``hpc_rll.rl_utils.fqf``, csrc/fqf.hip): every kernel the seven dispatchers can pick, against the fp64 oracle
of tests/fqf_oracle.py.

The kernels are called directly through the C ABI on guarded buffers (tests/guarded.py): every operand sits between sentinel
bands, the float ones each one float off a 16-byte boundary in turn, outputs are pre-filled with NaN and must be fully written,
inputs must come back bit for bit.  Every launch is pinned with ``hpc_rll_fqf_last_config``: the part of its kind moves by one
and names the literal family, G, grid, folded flag and vector width; no other part moves.  The public Python layer is covered by
the equality with ``IQNNStepTDError``, the autograd cases and the composition test at the end.

Bars: the project's ``TOL = 2e-5`` (tests/test_dist_td_gpu.py) -- ``rel_err`` on losses, ``td_err`` and outputs, ``grad_err``
(relative to the gradient tensor's own scale) on gradients.  Where the expected gradient is an exact fp32 product of saved
values (the one-hot TD backward, the fraction-loss backward) the comparison is bit for bit.

An action outside ``[0, N)`` (the 64-bit case: ``2^32 + 1``, whose low word alone would be a valid index) never addresses
memory and reads as 0: the reference is the oracle on operands with an extra all-zero action column.

The last test lists the literal set of launch records the dispatchers can pick; run the whole file."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import fqf_oracle as O
from conftest import grad_err, rel_err
from guarded import GuardedF32, GuardedI64

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 2e-5                                  # fp32 kernels against the fp64 oracle (tests/test_dist_td_gpu.py:55)
G_UP = 1.75                                 # the device scalar grad_loss of the backward entry points
TD_F, TD_B, FL_F, FL_B, FR_F, FR_B, QV = range(7)        # HPC_RLL_FQF_LAUNCH_*
WAVE, GROUP, STREAM, STREAM_ARGMAX = range(4)            # HPC_RLL_FQF_FAMILY_*
FIELDS = ("count", "family", "g", "grid", "folded", "vec")
DONE_SET = (0., 0., 0., 1., 0.5, -1., 3.)
EUNSUPPORTED = -3

COVER = set()      # (kind, family, g, vec) of every record this file has seen
WORST = {}         # op -> worst error against the oracle


def worst(name, err):
    WORST[name] = max(WORST.get(name, 0.0), float(err))
    return err


def records():
    import cabi
    out = (ctypes.c_int * 42)()
    assert cabi.lib.hpc_rll_fqf_last_config(out) == 0
    v = list(out)
    return [dict(zip(FIELDS, v[6 * k:6 * k + 6])) for k in range(7)]


class launches:
    """The body launches exactly one kernel of ``kind`` and the record names the literal instantiation."""

    def __init__(self, kind, family, g, grid, vec, folded=0, what=""):
        self.kind, self.want, self.what = kind, dict(family=family, g=g, grid=grid, folded=folded, vec=vec), what

    def __enter__(self):
        self.before = records()

    def __exit__(self, et, ev, tb):
        if et is None:
            now = records()
            want = dict(self.want, count=self.before[self.kind]["count"] + 1)
            assert now[self.kind] == want, (self.what, "ran", now[self.kind], "expected", want)
            for k in range(7):
                assert k == self.kind or now[k] == self.before[k], (self.what, "the record of another kind moved", k)
            COVER.add((self.kind, want["family"], want["g"], want["vec"]))


@contextlib.contextmanager
def unfolded():
    """Tune key 21 = 0 for the body: the loss is finalised by the separate launch."""
    import cabi
    try:
        assert cabi.lib.hpc_rll_tune_set(21, 0) == 0
        yield
    finally:
        assert cabi.lib.hpc_rll_tune_set(21, 1) == 0


def group_lanes(n):
    return 8 if n <= 8 else 16 if n <= 16 else 32 if n <= 32 else 64


def per_block(n):
    """Samples (rows) per workgroup of the kernel that takes width n, and its (family, G)."""
    if n > 64:
        return 4, WAVE, 64
    g = group_lanes(n)
    return 4 * (64 // g), GROUP, g


def fin(x, off=0):
    """A float32 input on the device between guard bands, ``off`` floats past a 16-byte boundary (None stays None)."""
    if x is None:
        return None
    x = x.to(torch.float32)
    g = GuardedF32(1, x.numel(), off, DEV, src=x.reshape(1, -1).to(DEV))
    g.src = x.clone()
    return g


def fout(n, off=0):
    return GuardedF32(1, n, off, DEV)


def ptr(g):
    return None if g is None else g.t.data_ptr()


def check_inputs(what, *gs):
    for g in gs:
        if g is None:
            continue
        g.check(what)
        if isinstance(g, GuardedF32):
            assert torch.equal(g.t.flatten().cpu(), g.src.flatten()), f"{what}: an input was overwritten"


def check_outputs(what, *gs):
    for g in gs:
        g.check(what)
        g.assert_written(what)


def partials_for(B):
    import cabi
    return fout(int(cabi.lib.hpc_rll_partials_floats(B)))


# ---------------------------------------------------------------------------------------------------------------------
# TD loss
# ---------------------------------------------------------------------------------------------------------------------
class TdCase:
    def __init__(self, K, Kp, B, N, nstep, has_w, has_vg, seed, kappa=1.0, gamma=0.9):
        g = torch.Generator().manual_seed(seed)
        f = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
        self.K, self.Kp, self.B, self.N, self.nstep, self.kappa, self.gamma = K, Kp, B, N, nstep, kappa, gamma
        self.q, self.nq, self.r = f(B, K, N), f(B, Kp, N), f(nstep, B)
        self.a, self.na = torch.randint(0, N, (B,), generator=g), torch.randint(0, N, (B,), generator=g)
        self.a[0], self.na[0], self.a[-1], self.na[-1] = N - 1, 0, 0, N - 1          # first and last actions
        self.done = torch.tensor(DONE_SET)[torch.randint(0, len(DONE_SET), (B,), generator=g)]   # not a flag
        self.qh = torch.rand(B, K, generator=g)
        self.w = torch.rand(B, generator=g) + 0.5 if has_w else None
        self.vg = torch.rand(B, generator=g) if has_vg else None

    def oracle(self, q=None, nq=None, a=None, na=None):
        D = lambda x: None if x is None else x.double()  # noqa: E731
        q = (self.q if q is None else q).double().requires_grad_(True)
        nq = self.nq if nq is None else nq
        a, na = self.a if a is None else a, self.na if na is None else na
        loss, td = O.nstep_td_error(q, D(nq), a, na, D(self.r), D(self.done), D(self.qh), D(self.w), self.gamma, self.kappa,
                                    D(self.vg))
        (grad,) = torch.autograd.grad(loss, q)
        return loss.item(), td.detach().numpy(), grad.numpy()


class TdRun:
    """One forward launch of a case; ``off`` names the operand placed one float off its 16-byte boundary."""

    def __init__(self, c, off=None, fold=1, what=""):
        import cabi
        o = lambda n: 1 if n == off else 0  # noqa: E731
        self.c, self.what = c, f"{what} td K={c.K} K'={c.Kp} B={c.B} N={c.N} nstep={c.nstep} off={off}"
        self.ins = [fin(c.q, o("q")), fin(c.nq, o("next_n_q")), GuardedI64(c.a, DEV), GuardedI64(c.na, DEV),
                    fin(c.r, o("reward")) if c.nstep else None, fin(c.done, o("done")), fin(c.qh, o("quantiles_hats")),
                    fin(c.w, o("weight")), fin(c.vg, o("value_gamma"))]
        self.loss, self.td, self.buf = fout(1), fout(c.B, o("td_err")), fout(c.B * c.K, o("buf"))
        self.partials = partials_for(c.B)
        S, family, G = per_block(max(c.K, c.Kp))
        with launches(TD_F, family, G, -(-c.B // S), 1, folded=fold, what=self.what):
            cabi.call("hpc_rll_fqf_nstep_td_forward", DEV, *[ptr(x) for x in self.ins], ptr(self.loss), ptr(self.td),
                      ptr(self.buf), ptr(self.partials), c.K, c.Kp, c.nstep, c.B, c.N, c.gamma, c.kappa, 1.0 / c.B)
        torch.cuda.synchronize()
        check_inputs(self.what, *self.ins)
        check_outputs(self.what, self.loss, self.td, self.buf)
        self.partials.check(self.what)

    def host(self):
        return float(self.loss.t.item()), self.td.t.flatten().cpu().numpy(), self.buf.t.view(self.c.B, self.c.K).cpu()

    def against(self, ref, a=None):
        loss, td, buf = self.host()
        a = self.c.a if a is None else a
        ok = (a >= 0) & (a < self.c.N)
        ref_buf = np.zeros((self.c.B, self.c.K))
        idx = torch.arange(self.c.B)[ok]
        ref_buf[idx] = ref[2][idx, :, a[ok]]
        e = (rel_err(ref[0], loss), rel_err(ref[1], td), grad_err(ref_buf[idx.numpy()], buf.numpy()[idx.numpy()], "buf"))
        for name, x in zip(("td loss", "td td_err", "td buf"), e):
            worst(name, x)
        assert max(e) <= TOL, (self.what, e)

    def backward(self, off_grad=0, a=None):
        """One launch of the backward on this run's buf: bit for bit the one-hot rows of g * buf."""
        import cabi
        c = self.c
        what = f"{self.what} backward off={off_grad}"
        g, grad = fin(torch.tensor([G_UP])), fout(c.B * c.K * c.N, off_grad)
        vec = 4 if c.N % 4 == 0 and off_grad == 0 else 1
        nc = c.N // vec
        rpb = 1 if nc >= 256 else 256 // nc
        kept = self.buf.t.clone()
        with launches(TD_B, STREAM, 0, min(-(-c.B * c.K // rpb), 32768), vec, what=what):
            cabi.call("hpc_rll_fqf_nstep_td_backward", DEV, ptr(g), ptr(self.buf), ptr(self.ins[2]), ptr(grad), c.K, c.B, c.N)
        torch.cuda.synchronize()
        check_inputs(what, g, self.ins[2])
        check_outputs(what, grad)
        self.buf.check(what)
        assert torch.equal(self.buf.t, kept), (what, "buf was overwritten")
        a = c.a if a is None else a
        ok = (a >= 0) & (a < c.N)
        ref = torch.zeros(c.B, c.K, c.N)
        idx = torch.arange(c.B)[ok]
        ref[idx, :, a[ok]] = (torch.tensor(G_UP, dtype=torch.float32) * self.buf.t.view(c.B, c.K).cpu())[idx]
        got = grad.t.view(c.B, c.K, c.N).cpu()
        assert torch.equal(got, ref), (what, "grad_q is not the one-hot rows of g * buf")
        chosen = torch.zeros(c.B, c.K, c.N, dtype=torch.bool)
        chosen[idx, :, a[ok]] = True
        assert bool((got[~chosen] == 0).all()), (what, "a never-chosen action has a gradient")


TD_PAIRS = ((1, 1), (2, 7), (7, 2), (8, 8), (9, 16), (16, 9), (17, 32), (32, 17), (32, 32), (33, 64), (64, 33), (64, 64),
            (65, 1), (1, 65), (130, 65), (65, 130))
NS = (1, 3, 4, 64, 65)


@pytest.mark.parametrize("K,Kp", TD_PAIRS)
def test_td_every_kernel_against_the_oracle(K, Kp):
    """B in {1, S-1, S+1, 2S+5} of the kernel's S samples per workgroup; N, nstep 0..5, weight / value_gamma present or None and
    the misaligned operand rotate with the case; the backward takes the 16-byte path where N % 4 == 0 and the scalar path
    otherwise or on a misaligned grad_q."""
    S = per_block(max(K, Kp))[0]
    names = ("q", "next_n_q", "reward", "done", "quantiles_hats", "weight", "value_gamma", "td_err", "buf")
    for i, B in enumerate(sorted({1, max(S - 1, 1), S + 1, 2 * S + 5})):
        j = i + K + Kp
        c = TdCase(K, Kp, B, NS[j % 5], j % 6, j % 2 == 0, j % 3 != 0, 100 * K + Kp + i, kappa=(1.0, 0.6)[j % 2])
        run = TdRun(c, off=names[j % len(names)])
        run.against(c.oracle())
        run.backward(off_grad=(0, 0, 1)[j % 3])


def test_td_each_operand_one_float_off_in_turn_and_identical_bits():
    c = TdCase(32, 32, 21, 4, 3, True, True, 7)
    ref = c.oracle()
    base = TdRun(c).host()
    for name in ("q", "next_n_q", "reward", "done", "quantiles_hats", "weight", "value_gamma", "td_err", "buf"):
        run = TdRun(c, off=name)
        run.against(ref)
        got = run.host()
        assert got[0] == base[0] and np.array_equal(got[1], base[1]) and torch.equal(got[2], base[2]), (name, "bits differ")
    first = TdRun(c)
    first.backward(0)
    first.backward(1)
    first.backward(3)


def test_td_errors_exactly_at_kappa_and_zero():
    """done = 1 and nstep = 1: every target is the reward, a small integer; q sits exactly kappa below, kappa above and on it."""
    K, Kp, B, N, kappa = 9, 5, 12, 3, 0.5
    c = TdCase(K, Kp, B, N, 1, True, False, 11, kappa=kappa)
    c.done = torch.ones(B)
    c.r = torch.randint(-3, 4, (1, B)).float()
    step = torch.tensor([kappa, -kappa, 0.0])[torch.arange(K) % 3]
    c.q = (c.r[0][:, None, None] + step[None, :, None]).expand(B, K, N).contiguous()
    ref = c.oracle()
    e = c.r[0][:, None].double() - c.q[:, :, 0].double()
    assert set(e.flatten().tolist()) == {kappa, -kappa, 0.0}
    run = TdRun(c)
    run.against(ref)
    run.backward(0)


def test_td_sixty_four_bit_actions_never_address_memory():
    """action / next action 2^32 + 1 and -1: the low word alone would be a valid index.  The selected value reads as 0 (the
    oracle on operands with an all-zero extra column) and the gradient rows of such a sample are zero."""
    for K, Kp in ((8, 8), (70, 3)):
        c = TdCase(K, Kp, 9, 3, 2, True, True, 13)
        c.a[2], c.a[5], c.na[3], c.na[5] = 2 ** 32 + 1, -1, 2 ** 32 + 1, -(2 ** 40)
        ext = lambda x: torch.cat([x, torch.zeros(x.shape[0], x.shape[1], 1)], 2)  # noqa: E731
        a_ref, na_ref = c.a.clone(), c.na.clone()
        a_ref[(c.a < 0) | (c.a >= c.N)] = c.N
        na_ref[(c.na < 0) | (c.na >= c.N)] = c.N
        ref = c.oracle(ext(c.q), ext(c.nq), a_ref, na_ref)
        ref = (ref[0], ref[1], ref[2][:, :, :c.N])
        run = TdRun(c)
        run.against(ref, a=c.a)
        run.backward(0, a=c.a)


def test_td_unfolded_gives_the_same_per_sample_results():
    for K in (20, 70):
        c = TdCase(K, K, 13, 3, 1, True, True, 17)
        ref = c.oracle()
        folded = TdRun(c).host()
        with unfolded():
            run = TdRun(c, fold=0)
        run.against(ref)
        got = run.host()
        assert np.array_equal(got[1], folded[1]) and torch.equal(got[2], folded[2])
        assert rel_err(folded[0], got[0]) <= 4e-7


def _api_td(c, mod=None, requires_grad=True):
    from hpc_rll.rl_utils import fqf
    G = lambda x: None if x is None else x.to(DEV)  # noqa: E731
    q = c.q.to(DEV).requires_grad_(requires_grad)
    if mod is None:
        loss, td = fqf.fqf_nstep_td_error(fqf.fqf_nstep_td_data(q, G(c.nq), G(c.a), G(c.na), G(c.r), G(c.done), G(c.qh), G(c.w)),
                                          c.gamma, c.nstep, c.kappa, G(c.vg))
    else:
        loss, td = mod(q, G(c.nq), G(c.a), G(c.na), G(c.r), G(c.done), G(c.qh), c.gamma, c.kappa, G(c.w), G(c.vg))
    return q, loss, td


@pytest.mark.parametrize("K,Kp,N", [(8, 5, 3), (32, 32, 4), (64, 33, 6), (70, 9, 4)])
def test_td_equals_iqn_on_the_permuted_operands(K, Kp, N):
    """The public op against ``IQNNStepTDError`` on ``q.permute(1,0,2)`` and ``quantiles_hats.t()``: the families' own bar, 4e-7 of
    the maximum (tests/test_dist_td_gpu.py), on loss, td_err and the gradient; and against the oracle."""
    from hpc_rll.rl_utils.fqf import FQFNStepTDError
    from hpc_rll.rl_utils.td import IQNNStepTDError
    c = TdCase(K, Kp, 37, N, 3, True, True, 19, kappa=0.8)
    G = lambda x: x.to(DEV)  # noqa: E731
    q, loss, td = _api_td(c)
    assert loss.shape == (1,) and td.shape == (c.B,) and not td.requires_grad
    (2.5 * loss).sum().backward()
    q2, loss2, td2 = _api_td(c, FQFNStepTDError())
    (2.5 * loss2).sum().backward()
    assert torch.equal(loss, loss2) and torch.equal(td, td2) and torch.equal(q.grad, q2.grad)        # identical bits on a second run
    qi = c.q.permute(1, 0, 2).contiguous().to(DEV).requires_grad_(True)
    li, tdi = IQNNStepTDError(K, Kp, c.nstep, c.B, N)(qi, G(c.nq.permute(1, 0, 2).contiguous()), G(c.a), G(c.na), G(c.r), G(c.done),
                                                       G(c.qh.t().contiguous()), c.gamma, c.kappa, G(c.w), G(c.vg))
    (2.5 * li).sum().backward()
    gi = qi.grad.permute(1, 0, 2)
    for name, x, y in (("loss", loss, li), ("td_err", td, tdi), ("grad", q.grad, gi)):
        d, m = float((x.detach() - y.detach()).abs().max()), float(y.detach().abs().max())
        assert d <= 4e-7 * max(m, 1e-30), (name, d, m)
    ref = c.oracle()
    assert rel_err(ref[0], loss.item()) <= TOL and rel_err(ref[1], td.cpu().numpy()) <= TOL
    assert worst("td grad_q (autograd)", grad_err(2.5 * ref[2], q.grad.cpu().numpy(), "grad_q")) <= TOL


def test_td_no_backward_launch_when_q_needs_no_gradient():
    from hpc_rll.rl_utils import fqf
    c = TdCase(8, 8, 6, 4, 1, True, False, 23)
    G = lambda x: x.to(DEV)  # noqa: E731
    w = G(c.w).requires_grad_(True)                                # keeps the node alive; weight itself gets no gradient
    loss, _ = fqf.fqf_nstep_td_error((G(c.q), G(c.nq), G(c.a), G(c.na), G(c.r), G(c.done), G(c.qh), w), c.gamma)
    before = records()
    loss.sum().backward()
    assert records() == before and w.grad is None
    q, loss, _ = _api_td(c)
    loss.sum().backward()
    now = records()
    assert now[TD_B]["count"] == before[TD_B]["count"] + 1 and now[TD_B]["vec"] == 4 and q.grad is not None


def test_extension_names_wrong_arguments():
    from hpc_rll.rl_utils import fqf
    z = lambda *s, **k: torch.zeros(*s, device=DEV, **k)  # noqa: E731
    B, K, N = 5, 4, 3
    td = [z(B, K, N), z(B, K, N), z(B, dtype=torch.int64), z(B, dtype=torch.int64), z(1, B), z(B), z(B, K), None]
    bad = lambda i, x: td[:i] + [x] + td[i + 1:]  # noqa: E731
    for i, x, msg in ((0, z(B, K, N, dtype=torch.float64), r"q: dtype"), (0, z(B, K), r"q: expected \(B,K,N\)"),
                      (1, z(B + 1, K, N), r"next_n_q: shape"), (2, z(B), r"action: dtype"), (3, z(B + 1, dtype=torch.int64), r"next_n_action: shape"),
                      (4, z(B), r"reward: expected"), (5, z(B, 1), r"done: shape"), (6, z(B, K + 1), r"quantiles_hats: shape"),
                      (7, z(B + 1), r"weight: shape")):
        with pytest.raises(RuntimeError, match=msg):
            fqf.fqf_nstep_td_error(bad(i, x), 0.99, nstep=x.shape[0] if i == 4 else 1)
    with pytest.raises(RuntimeError, match=r"value_gamma: shape"):
        fqf.fqf_nstep_td_error(td, 0.99, value_gamma=z(B, 2))
    with pytest.raises(RuntimeError, match=r"kappa: expected > 0"):
        fqf.fqf_nstep_td_error(td, 0.99, kappa=0.0)
    with pytest.raises(RuntimeError, match=r"logits: dtype"):
        fqf.fqf_fractions(z(B, K, dtype=torch.float64))
    with pytest.raises(RuntimeError, match=r"logits: expected \(B,K\)"):
        fqf.fqf_fractions(z(B))
    with pytest.raises(RuntimeError, match=r"hpc_rll_fqf_fractions_forward \(1 <= K <= 1024\)"):
        fqf.fqf_fractions(z(2, 1025))
    with pytest.raises(RuntimeError, match=r"q_tau_i: shape"):
        fqf.fqf_calculate_fraction_loss(z(B, K, N), z(B, K, N), z(B, K + 1), z(B, dtype=torch.int64))
    with pytest.raises(RuntimeError, match=r"quantiles: shape"):
        fqf.fqf_calculate_fraction_loss(z(B, K - 1, N), z(B, K, N), z(B, K), z(B, dtype=torch.int64))
    with pytest.raises(RuntimeError, match=r"actions: dtype"):
        fqf.fqf_calculate_fraction_loss(z(B, K - 1, N), z(B, K, N), z(B, K + 1), z(B))
    with pytest.raises(RuntimeError, match=r"quantiles: shape"):
        fqf.fqf_q_value(z(B, K, N), z(B, K))
    with pytest.raises(RuntimeError, match=r"q: must be contiguous"):
        fqf.fqf_q_value(z(B, N, K).permute(0, 2, 1), z(B, K + 1))


# ---------------------------------------------------------------------------------------------------------------------
# fraction loss
# ---------------------------------------------------------------------------------------------------------------------
def fraction_rows(kind, B, K, N, g):
    """q_tau_i (B,K-1,N), q_value (B,K,N), actions: on the action's column the 2K-1 interleaved values h_0 s_0 h_1 .. h_{K-1} are
    ascending (``sorted``), descending (``reversed``), small integers with ties between neighbours (``ties``) or random."""
    a = torch.randint(0, N, (B,), generator=g)
    a[0], a[-1] = N - 1, 0
    qv, qt = torch.randn(B, K, N, generator=g), torch.randn(B, K - 1, N, generator=g)
    if kind == "ties":
        allv = torch.randint(0, 3, (B, 2 * K - 1), generator=g).float()
    else:
        allv = torch.sort(torch.randn(B, 2 * K - 1, generator=g), dim=1, descending=kind == "reversed").values
    if kind != "random":
        idx = torch.arange(B)
        qv[idx, :, a], qt[idx, :, a] = allv[:, 0::2], allv[:, 1::2]
    return qt, qv, a


def run_fraction_loss(qt, qv, quant, a, off=None, fold=1, what=""):
    import cabi
    B, K, N = qv.shape
    o = lambda n: 1 if n == off else 0  # noqa: E731
    what = f"{what} fraction loss K={K} B={B} N={N} off={off}"
    ins = [fin(qt, o("q_tau_i")) if K > 1 else None, fin(qv, o("q_value")), fin(quant, o("quantiles")), GuardedI64(a, DEV)]
    loss, g, partials = fout(1), fout(B * (K - 1), o("g")) if K > 1 else None, partials_for(B)
    S, family, G = per_block(K)
    with launches(FL_F, family, G, -(-B // S), 1, folded=fold, what=what):
        cabi.call("hpc_rll_fqf_fraction_loss_forward", DEV, *[ptr(x) for x in ins], ptr(loss), ptr(g), ptr(partials), K, B, N,
                  1.0 / B)
    torch.cuda.synchronize()
    check_inputs(what, *ins)
    check_outputs(what, *([loss] + ([g] if K > 1 else [])))
    partials.check(what)
    return float(loss.t.item()), g


@pytest.mark.parametrize("K", [1, 2, 3, 8, 9, 17, 33, 64, 65])
def test_fraction_loss_against_the_oracle(K):
    """Sorted, reversed, tied and random rows; all four sign branches occur; the backward puts g_loss * scale * g into columns
    1..K-1 and zeros into columns 0 and K, bit for bit."""
    import cabi
    S = per_block(K)[0]
    gen = torch.Generator().manual_seed(31 + K)
    seen1, seen2 = set(), set()
    offs = ("q_tau_i", "q_value", "quantiles", "g", None)
    for i, (kind, B, N) in enumerate((("sorted", 1, 1), ("reversed", max(S - 1, 1), 3), ("ties", S + 1, 4), ("random", 2 * S + 5, 6),
                                      ("ties", 3, 64))):
        qt, qv, a = fraction_rows(kind, B, K, N, gen)
        quant = O.fractions(torch.randn(B, K, generator=gen).double())[0].float()
        g64, s1, s2 = O.fraction_g(qt.double(), qv.double(), a)
        if K > 1 and kind == "sorted":
            assert bool(s1.all()) and bool(s2.all())
        if K > 1 and kind == "reversed":
            assert not bool(s1.any()) and not bool(s2.any())
        seen1 |= set(s1.flatten().tolist())
        seen2 |= set(s2.flatten().tolist())
        ref = O.fraction_loss(qt.double(), qv.double(), quant.double(), a).item()
        loss, g = run_fraction_loss(qt, qv, quant, a, off=offs[i], what=kind)
        assert worst("fraction loss", rel_err(ref, loss)) <= TOL, (kind, B, N, ref, loss)
        if K == 1:
            assert loss == 0.0
            continue
        got = g.t.view(B, K - 1).cpu()
        if kind == "ties":
            assert torch.equal(got.double(), g64), "small integers: g is exact"
        assert worst("fraction g", grad_err(g64.numpy(), got.numpy(), "g")) <= TOL or not g64.any()
        # backward on the saved g
        what = f"fraction loss backward K={K} B={B}"
        gl, gq = fin(torch.tensor([G_UP])), fout(B * (K + 1), i % 2)
        with launches(FL_B, STREAM, 0, -(-B * (K + 1) // 256), 1, what=what):
            cabi.call("hpc_rll_fqf_fraction_loss_backward", DEV, ptr(gl), ptr(g), ptr(gq), K, B, 1.0 / B)
        torch.cuda.synchronize()
        check_inputs(what, gl)
        check_outputs(what, gq)
        g.check(what)
        ref_g = torch.zeros(B, K + 1)
        ref_g[:, 1:K] = (torch.tensor(G_UP, dtype=torch.float32) * torch.tensor(1.0 / B, dtype=torch.float32)) * got
        out = gq.t.view(B, K + 1).cpu()
        assert torch.equal(out, ref_g) and bool((out[:, 0] == 0).all()) and bool((out[:, K] == 0).all())
    if K > 1:
        assert seen1 == {True, False} and seen2 == {True, False}, "a sign branch did not occur"


def test_fraction_loss_autograd_and_out_of_range_action():
    """Through the public function: the gradient reaches quantiles[:,1:K] only; q_tau_i and q_value get none.  An action outside
    [0, N) reads both values as 0: g = 0 for that sample."""
    from hpc_rll.rl_utils.fqf import fqf_calculate_fraction_loss
    gen = torch.Generator().manual_seed(37)
    B, K, N = 19, 32, 6
    qt, qv, a = fraction_rows("random", B, K, N, gen)
    a[4] = 2 ** 32 + 2
    logits = torch.randn(B, K, generator=gen)
    q64 = O.fractions(logits.double())[0].requires_grad_(True)
    ok = (a >= 0) & (a < N)
    a_ref = torch.where(ok, a, torch.zeros_like(a))
    m = ok.double()[:, None, None]
    ref = O.fraction_loss(qt.double() * m, qv.double() * m, q64, a_ref)
    (ref_g,) = torch.autograd.grad(ref, q64)
    quant = q64.detach().float().to(DEV).requires_grad_(True)
    qtd, qvd = qt.to(DEV).requires_grad_(True), qv.to(DEV).requires_grad_(True)
    before = records()
    loss = fqf_calculate_fraction_loss(qtd, qvd, quant, a.to(DEV))
    assert loss.shape == (1,) and rel_err(ref.item(), loss.item()) <= TOL
    (3.0 * loss).sum().backward()
    assert qtd.grad is None and qvd.grad is None
    got = quant.grad.cpu()
    assert bool((got[:, 0] == 0).all()) and bool((got[:, K] == 0).all()) and bool((got[4] == 0).all())
    assert worst("fraction loss grad_quantiles", grad_err(3.0 * ref_g.numpy(), got.numpy(), "grad_quantiles")) <= TOL
    now = records()
    assert now[FL_F]["count"] == before[FL_F]["count"] + 1 and now[FL_B]["count"] == before[FL_B]["count"] + 1
    loss = fqf_calculate_fraction_loss(qtd, qvd, quant.detach(), a.to(DEV))   # quantiles need no gradient: no backward launch
    loss.sum().backward()
    assert records()[FL_B] == now[FL_B]
    with unfolded():
        l0, _ = run_fraction_loss(qt, qv, quant.detach().cpu(), a, fold=0)
    assert rel_err(loss.item(), l0) <= 4e-7


# ---------------------------------------------------------------------------------------------------------------------
# fractions
# ---------------------------------------------------------------------------------------------------------------------
def fraction_logits(kind, B, K, g):
    x = 2.0 * torch.randn(B, K, generator=g)
    if kind == "equal":
        x = torch.full((B, K), 0.75)
    elif kind == "dominant":
        x[torch.arange(B), torch.randint(0, K, (B,), generator=g)] += 20.0   # p = 1 in fp32, resolved in fp64
    elif kind == "neginf" and K > 1:
        m = torch.rand(B, K, generator=g) < 0.3
        m[:, 0] = False                                            # at least one finite logit per row
        m[0, 1:] = True                                            # and a row with a single one
        x[m] = -float("inf")
    return x


@pytest.mark.parametrize("K", [1, 2, 8, 9, 32, 33, 64, 65, 257, 1024])
def test_fractions_against_the_oracle(K):
    """Forward and the three backward forms (g_tau only, g_H only, both) on random, all-equal, one-dominant and -inf logits; the
    operand one float off alignment rotates.  All-equal logits with g_H alone have an identically zero gradient (log p = -H in
    every column): there the result is held to TOL of the size of the terms that cancel, max |g_H| p H."""
    import cabi
    S, family, G = per_block(K)
    gen = torch.Generator().manual_seed(41 + K)
    names = ("logits", "quantiles", "quantiles_hats", "entropies", "grad_quantiles", "grad_entropies", "grad_logits", None)
    for i, (kind, B) in enumerate((("random", 1), ("equal", max(S - 1, 1)), ("dominant", S + 1), ("neginf", 2 * S + 5))):
        off = names[(i + K) % len(names)]
        o = lambda n: 1 if n == off else 0  # noqa: E731
        what = f"fractions {kind} K={K} B={B} off={off}"
        x = fraction_logits(kind, B, K, gen)
        q64, h64, e64 = O.fractions(x.double())
        lg, qo, ho, eo = fin(x, o("logits")), fout(B * (K + 1), o("quantiles")), fout(B * K, o("quantiles_hats")), fout(B, o("entropies"))
        with launches(FR_F, family, G, -(-B // S), 1, what=what):
            cabi.call("hpc_rll_fqf_fractions_forward", DEV, ptr(lg), ptr(qo), ptr(ho), ptr(eo), B, K)
        torch.cuda.synchronize()
        check_inputs(what, lg)
        check_outputs(what, qo, ho, eo)
        quant, hats, ent = qo.t.view(B, K + 1).cpu(), ho.t.view(B, K).cpu(), eo.t.view(B, 1).cpu()
        e = (rel_err(q64.numpy(), quant.numpy()), rel_err(h64.numpy(), hats.numpy()), rel_err(e64.numpy(), ent.numpy()))
        for name, v in zip(("fractions quantiles", "fractions quantiles_hats", "fractions entropies"), e):
            worst(name, v)
        assert max(e) <= TOL, (what, e)
        assert bool((quant[:, 0] == 0).all()) and bool((quant[:, 1:] >= quant[:, :-1]).all())
        last = float((quant[:, K].double() - 1).abs().max())
        worst("fractions |last - 1| / (K 2^-23)", last / (K * 2.0 ** -23))
        assert last <= K * 2.0 ** -23, (what, last)
        assert torch.equal(hats, 0.5 * (quant[:, :-1] + quant[:, 1:])), "quantiles_hats are the midpoints of the stored fractions"
        gt, gh = torch.randn(B, K + 1, generator=gen), torch.randn(B, 1, generator=gen)
        for mode, g_tau, g_h in (("tau", gt, None), ("H", None, gh), ("both", gt, gh)):
            whatb = f"{what} backward {mode}"
            ref = O.fractions_grad(x.double(), torch.zeros(B, K + 1, dtype=torch.float64) if g_tau is None else g_tau.double(),
                                   torch.zeros(B, 1, dtype=torch.float64) if g_h is None else g_h.double()).numpy()
            gq, ghd, out = fin(g_tau, o("grad_quantiles")), fin(g_h, o("grad_entropies")), fout(B * K, o("grad_logits"))
            with launches(FR_B, family, G, -(-B // S), 1, what=whatb):
                cabi.call("hpc_rll_fqf_fractions_backward", DEV, ptr(lg), ptr(eo), ptr(gq), ptr(ghd), ptr(out), B, K)
            torch.cuda.synchronize()
            check_inputs(whatb, lg, gq, ghd)
            check_outputs(whatb, out)
            got = out.t.view(B, K).cpu().numpy()
            if (kind == "equal" or K == 1) and mode == "H":
                bound = TOL * float(gh.abs().max()) * float(e64.max()) / K
                assert float(np.abs(got).max()) <= bound, (whatb, float(np.abs(got).max()), bound)
            elif K == 1:
                assert not got.any(), (whatb, "one fraction: the gradient is identically zero")
            else:
                assert worst(f"fractions grad_logits ({mode})", grad_err(ref, got, "grad_logits")) <= TOL, whatb
            if kind == "neginf":
                assert not got[np.isinf(x.numpy())].any(), (whatb, "a -inf logit has a gradient")


def test_fractions_refuses_more_than_1024_and_writes_nothing():
    import cabi
    B, K = 3, 1025
    lg, qo, ho, eo, out = fin(torch.randn(B, K)), fout(B * (K + 1)), fout(B * K), fout(B), fout(B * K)
    before = records()
    st = cabi.stream_ptr(DEV)
    assert cabi.lib.hpc_rll_fqf_fractions_forward(ptr(lg), ptr(qo), ptr(ho), ptr(eo), B, K, st) == EUNSUPPORTED
    assert cabi.lib.hpc_rll_fqf_fractions_backward(ptr(lg), ptr(eo), ptr(qo), None, ptr(out), B, K, st) == EUNSUPPORTED
    torch.cuda.synchronize()
    for g in (qo, ho, eo, out):
        g.check("refused")
        g.assert_untouched("refused")
    assert records() == before


def test_fractions_autograd():
    """Through the public function: quantiles_hats is detached, each upstream gradient alone and both together."""
    from hpc_rll.rl_utils.fqf import fqf_fractions
    gen = torch.Generator().manual_seed(43)
    for K in (32, 100):
        B = 11
        x = fraction_logits("random", B, K, gen)
        gt, gh = torch.randn(B, K + 1, generator=gen), torch.randn(B, 1, generator=gen)
        for mode in ("tau", "H", "both"):
            x64 = x.double().requires_grad_(True)
            q64, _, e64 = O.fractions(x64)
            ref = (q64 * gt.double()).sum() * (mode != "H") + (e64 * gh.double()).sum() * (mode != "tau")
            (ref_g,) = torch.autograd.grad(ref, x64)
            xd = x.to(DEV).requires_grad_(True)
            quant, hats, ent = fqf_fractions(xd)
            assert quant.shape == (B, K + 1) and hats.shape == (B, K) and ent.shape == (B, 1) and not hats.requires_grad
            loss = (quant * gt.to(DEV)).sum() if mode == "tau" else (ent * gh.to(DEV)).sum() if mode == "H" else \
                (quant * gt.to(DEV)).sum() + (ent * gh.to(DEV)).sum()
            loss.backward()
            assert worst(f"fractions grad_logits ({mode})", grad_err(ref_g.numpy(), xd.grad.cpu().numpy(), "grad_logits")) <= TOL


# ---------------------------------------------------------------------------------------------------------------------
# expected value and greedy action
# ---------------------------------------------------------------------------------------------------------------------
def run_q_value(q, quant, argmax, off=0, what=""):
    import cabi
    B, K, N = q.shape
    what = f"{what} q_value K={K} B={B} N={N} argmax={argmax} off={off}"
    qg, tg, lo = fin(q, off), fin(quant), fout(B * N, 0)
    act = GuardedI64(torch.full((B,), -7, dtype=torch.int64), DEV) if argmax else None
    vec = 4 if N % 4 == 0 and off == 0 else 1
    G = group_lanes(N // vec)
    with launches(QV, STREAM_ARGMAX if argmax else STREAM, G, -(-B // (4 * (64 // G))), vec, what=what):
        cabi.call("hpc_rll_fqf_q_value", DEV, ptr(qg), ptr(tg), ptr(lo), ptr(act), B, K, N)
    torch.cuda.synchronize()
    check_inputs(what, qg, tg)
    check_outputs(what, lo)
    a = None
    if argmax:
        assert bool((act.raw[:act.lo] == act.raw[0]).all()) and bool((act.raw[act.hi:] == act.raw[0]).all()), (what, "guard moved")
        a = act.t.cpu()
    return lo.t.view(B, N).cpu(), a


@pytest.mark.parametrize("K", [1, 2, 8, 9, 32, 33, 64, 65, 257, 1024])
def test_q_value_against_the_oracle(K):
    """N in {1, 3, 4, 6, 64, 65, 1000} and 10, 30, 100 (the group widths the others leave out); q aligned (16-byte loads where
    N % 4 == 0) and one float off (scalar loads).  The returned action's fp64 expected value is within TOL * scale of the fp64
    maximum; with and without the argmax the values have identical bits."""
    gen = torch.Generator().manual_seed(47 + K)
    for i, N in enumerate((1, 3, 4, 6, 64, 65, 1000, 10, 30, 100)):
        for off in ((0, 1) if N % 4 == 0 else (0,)):
            vec = 4 if N % 4 == 0 and off == 0 else 1
            S = 4 * (64 // group_lanes(N // vec))
            B = (1, max(S - 1, 1), S + 1, 2 * S + 5)[(i + K) % 4] if K * N < 200000 else 5
            q = torch.randn(B, K, N, generator=gen)
            quant = O.fractions(torch.randn(B, K, generator=gen).double())[0].float()
            ref = O.q_value(q.double(), quant.double()).numpy()
            logit, a = run_q_value(q, quant, True, off)
            plain, _ = run_q_value(q, quant, False, off)
            assert torch.equal(logit, plain)
            assert worst("q_value logit", rel_err(ref, logit.numpy())) <= TOL, (K, N, off)
            assert a.dtype == torch.int64 and bool(((a >= 0) & (a < N)).all())
            best = ref.max(1)
            gap = (best - ref[np.arange(B), a.numpy()]) / np.maximum(1.0, np.abs(best))
            assert worst("q_value greedy action gap", float(gap.max())) <= TOL, (K, N, off, gap.max())


def test_q_value_ties_return_the_lowest_index():
    """Power-of-two widths and small integers: every sum is exact, so columns built from the same values tie exactly."""
    gen = torch.Generator().manual_seed(53)
    quant = torch.tensor([0.0, 0.5, 0.75, 0.875, 1.0])
    for N in (6, 64, 65, 1000):
        B = 9
        pool = torch.randint(-4, 5, (B, 4, 3), generator=gen).float()
        pick = torch.randint(0, 3, (B, N), generator=gen)
        q = torch.gather(pool, 2, pick[:, None, :].expand(B, 4, N)).contiguous()
        ref = O.q_value(q.double(), quant.double().expand(B, 5))
        want = torch.tensor([int((ref[b] == ref[b].max()).nonzero()[0]) for b in range(B)])
        assert any(int((ref[b] == ref[b].max()).sum()) > 1 for b in range(B)), "no tie in this case"
        for off in (0, 1):
            logit, a = run_q_value(q, quant.expand(B, 5).contiguous(), True, off, "ties")
            assert torch.equal(logit.double(), ref) and torch.equal(a, want), (N, off, a, want)
    from hpc_rll.rl_utils.fqf import fqf_q_value
    qd, td = q.to(DEV), quant.expand(B, 5).contiguous().to(DEV)
    logit, a = fqf_q_value(qd, td, return_action=True)
    assert torch.equal(a.cpu(), want) and not logit.requires_grad and torch.equal(fqf_q_value(qd, td), logit)


# ---------------------------------------------------------------------------------------------------------------------
# composition
# ---------------------------------------------------------------------------------------------------------------------
def test_a_full_learner_step_through_the_public_api():
    """fractions -> TD loss -> fraction loss -> target expected value, against the oracle: the three losses and the gradients on
    logits and q."""
    from hpc_rll.rl_utils import fqf
    gen = torch.Generator().manual_seed(59)
    B, K, N, nstep, gamma = 45, 32, 6, 3, 0.95
    f = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    logits, q, q_tau, tq, tlog = f(B, K), f(B, K, N), f(B, K - 1, N), f(B, K, N), f(B, K)
    a, r, done = torch.randint(0, N, (B,), generator=gen), f(nstep, B), (torch.rand(B, generator=gen) < 0.2).float()
    w = torch.rand(B, generator=gen) + 0.5
    # ours
    lg, qd = logits.to(DEV).requires_grad_(True), q.to(DEV).requires_grad_(True)
    quant, hats, ent = fqf.fqf_fractions(lg)
    tquant, _, _ = fqf.fqf_fractions(tlog.to(DEV))
    tlogit, na = fqf.fqf_q_value(tq.to(DEV), tquant.detach(), return_action=True)
    td_loss, td_err = fqf.fqf_nstep_td_error(fqf.fqf_nstep_td_data(qd, tq.to(DEV), a.to(DEV), na, r.to(DEV), done.to(DEV), hats,
                                                                    w.to(DEV)), gamma, nstep)
    fr_loss = fqf.fqf_calculate_fraction_loss(q_tau.to(DEV), qd.detach(), quant, a.to(DEV))
    ent_loss = -0.01 * ent.mean()
    (td_loss + 0.5 * fr_loss + ent_loss).sum().backward()
    # oracle (the greedy action is ours, checked against the fp64 expected value first)
    l64, q64 = logits.double().requires_grad_(True), q.double().requires_grad_(True)
    oq, oh, oe = O.fractions(l64)
    ref_t = O.q_value(tq.double(), O.fractions(tlog.double())[0]).numpy()
    assert rel_err(ref_t, tlogit.cpu().numpy()) <= TOL
    na_c = na.cpu()
    assert float(((ref_t.max(1) - ref_t[np.arange(B), na_c.numpy()]) / np.maximum(1.0, np.abs(ref_t.max(1)))).max()) <= TOL
    o_td, o_err = O.nstep_td_error(q64, tq.double(), a, na_c, r.double(), done.double(), oh, w.double(), gamma)
    o_fr = O.fraction_loss(q_tau.double(), q64.detach(), oq, a)
    o_ent = -0.01 * oe.mean()
    (o_td + 0.5 * o_fr + o_ent).backward()
    e = (rel_err(o_td.item(), td_loss.item()), rel_err(o_fr.item(), fr_loss.item()), rel_err(o_ent.item(), ent_loss.item()),
         rel_err(o_err.detach().numpy(), td_err.cpu().numpy()))
    assert max(e) <= TOL, e
    assert worst("composition grad_logits", grad_err(l64.grad.numpy(), lg.grad.cpu().numpy(), "grad_logits")) <= TOL
    assert worst("composition grad_q", grad_err(q64.grad.numpy(), qd.grad.cpu().numpy(), "grad_q")) <= TOL


def test_coverage_of_every_kernel():
    """Run the whole file: the records are collected by every launch above.  The literal set of (kind, family, G, vector width)
    the seven dispatchers can pick -- 5 + 2 + 5 + 1 + 5 + 5 + 16 tuples."""
    W = (8, 16, 32, 64)
    expect = {(TD_F, GROUP, g, 1) for g in W} | {(TD_F, WAVE, 64, 1)} | {(TD_B, STREAM, 0, 1), (TD_B, STREAM, 0, 4)}
    expect |= {(FL_F, GROUP, g, 1) for g in W} | {(FL_F, WAVE, 64, 1), (FL_B, STREAM, 0, 1)}
    expect |= {(k, GROUP, g, 1) for k in (FR_F, FR_B) for g in W} | {(FR_F, WAVE, 64, 1), (FR_B, WAVE, 64, 1)}
    expect |= {(QV, fam, g, v) for fam in (STREAM, STREAM_ARGMAX) for g in W for v in (1, 4)}
    assert len(expect) == 5 + 2 + 5 + 1 + 5 + 5 + 16
    for name, e in sorted(WORST.items()):
        print(f"worst error against the oracle, {name}: {e:.3g}")
    missing, extra = sorted(expect - COVER), sorted(COVER - expect)
    assert not missing and not extra, f"not run: {missing}\nnot expected: {extra}"
