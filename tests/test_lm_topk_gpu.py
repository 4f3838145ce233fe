"""GPU tier of the top-k teacher ops (``hpc_rll.rl_utils.lm_topk``, csrc/lm_topk.hip).

The oracle is this file's own, on the host: the selection is a stable descending sort of the clamped row, the
log-probabilities a float64 ``log_softmax`` of the whole row, and the two divergences the definitions of the module docstring
in float64 through autograd, the student's tail mass summed over the entries outside the set.  bfloat16 inputs are upcast
exactly.  Indices are compared as integers.  Bars, those of test_lm_kl_gpu.py: ``rel_err`` <= 1e-5 on a value or a
log-probability; ``grad_err`` <= 2e-5 on a float32 gradient; a bfloat16 gradient per element
``|got - exact| <= 2^-8 |exact| + 2e-5 max|grad|``."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import grad_err, rel_err
from lm_rows import DTYPES, GRID_MAX, WAVE_ROW_MAX, dev, place

pytestmark = pytest.mark.gpu

FLT_MAX = float(np.finfo(np.float32).max)
INF = float("inf")
TAILS = ("renorm", "bucket")


def select(x, k, T=1.0):
    """(index (..., k) int64, logp (..., k) float64) of host logits: the order of the raw row, log_softmax(x / T) at it."""
    key = torch.nan_to_num(x.float(), nan=-FLT_MAX, posinf=INF, neginf=-FLT_MAX) + 0.0
    idx = torch.sort(key, dim=-1, descending=True, stable=True).indices[..., :k]
    a = torch.nan_to_num(x.double() / T, nan=-FLT_MAX, posinf=INF, neginf=-FLT_MAX).clamp(min=-FLT_MAX)
    lp = torch.log_softmax(a, -1).gather(-1, idx)
    masked = ~(x.float().gather(-1, idx) > -INF)
    return idx, torch.where(masked, torch.full_like(lp, -INF), lp)


def check_topk(x, k, got, T=1.0, w=None, what=""):
    idx, lp = select(x, k, T)
    if w is not None:
        idx, lp = torch.where(w[..., None] != 0, idx, -1), torch.where(w[..., None] != 0, lp, -INF)
    gl, gi = got[0].double().cpu(), got[1].cpu()
    assert gi.dtype == torch.int32 and gl.shape == gi.shape == idx.shape
    assert torch.equal(gi.long(), idx), what
    assert torch.equal(gl == -INF, lp == -INF), what
    e = rel_err(torch.nan_to_num(lp, neginf=0.0).numpy(), torch.nan_to_num(gl, neginf=0.0).numpy())
    print(f"{what}: logp err {e:.2e}")
    assert e <= 1e-5, what


def kl_oracle(x, idx, lp, w=None, g=None, tail="renorm", T=1.0):
    """(kl, d sum(g kl) / dx) as float64 numpy arrays, from host tensors."""
    a = x.double().clone().requires_grad_(True)
    V, zero = x.shape[-1], torch.zeros((), dtype=torch.float64)
    live = torch.ones(x.shape[:-1], dtype=torch.bool) if w is None else w != 0
    ok = (idx >= 0) & (idx < V) & (lp > -INF)
    ls_all = torch.log_softmax(torch.where(live[..., None], a, zero) / T, -1)
    at = idx.long().clamp(0, V - 1)
    ls = ls_all.gather(-1, at)
    q, lq = torch.where(ok, lp.double().exp(), zero), torch.where(ok, lp.double(), zero)
    Q = q.sum(-1).clamp(max=1.0)
    if tail == "renorm":
        Qs = torch.where(Q > 0, Q, torch.ones_like(Q))[..., None]
        val = (q / Qs * (lq - Qs.log() - ls)).sum(-1)
    else:
        inset = torch.zeros(x.shape, dtype=torch.int64).scatter_add_(-1, at, ok.long()) > 0
        rest_p, rest_q = torch.where(inset, zero, ls_all.exp()).sum(-1), 1.0 - Q   # 1 - P: summed, not subtracted
        both = (rest_q > 0) & (rest_p > 0)
        one = torch.ones_like(Q)
        val = (q * (lq - ls)).sum(-1) + torch.where(both, rest_q * (torch.where(both, rest_q, one).log() - torch.where(both, rest_p, one).log()), zero)
    val = torch.where(live & ok.any(-1), val, zero)
    (val * (1.0 if g is None else g.double())).sum().backward()
    return val.detach().numpy(), a.grad.numpy()


def run_kl(x, idx, lp, w=None, g=None, tail="renorm", T=1.0, off=0):
    from hpc_rll.rl_utils.lm_topk import token_topk_kl_div
    xd = place(x, off).requires_grad_(True)
    kl = token_topk_kl_div(xd, idx.to(dev()), lp.to(dev()), place(w), tail, T)
    assert kl.dtype == torch.float32 and kl.shape == x.shape[:-1]
    kl.backward(torch.ones_like(kl) if g is None else g.to(dev()))
    assert xd.grad.dtype == x.dtype and xd.grad.shape == x.shape
    return kl.detach().double().cpu().numpy(), xd.grad.double().cpu().numpy(), xd


def check(ref, got, dtype, what):
    e_val = rel_err(ref[0], got[0])
    gmax = float(np.abs(ref[1]).max()) if ref[1].size else 0.0
    if dtype == torch.float32:
        e_grad = grad_err(ref[1], got[1], what)
        print(f"{what}: value err {e_val:.2e}, grad err {e_grad:.2e} (max|grad| {gmax:.2e})")
        assert e_grad <= 2e-5, what
    else:
        excess = np.abs(got[1] - ref[1]) - (2.0 ** -8 * np.abs(ref[1]) + 2e-5 * gmax)
        print(f"{what}: value err {e_val:.2e}, bf16 grad worst excess over the bar {excess.max(initial=0.0):.2e} (max|grad| {gmax:.2e})")
        assert excess.max(initial=0.0) <= 0, what
    assert e_val <= 1e-5, what


def draw(rows, V, dtype, seed, scale=1.0):
    return (torch.randn(rows, V, generator=torch.Generator().manual_seed(seed)) * scale).to(dtype)


def expect(x, grad, rows, V, k, per_row=False):
    """[element type, bytes per access, threads per row, rows per workgroup, workgroups, k]: 16 bytes when every base of the launch
    and the pitch lie on 16; the producer (per_row) a workgroup per row at every V, the consumer a wave per row up to WAVE_ROW_MAX."""
    e = x.element_size()
    wide = all(t.data_ptr() % 16 == 0 for t in (x, grad)) and (V * e) % 16 == 0
    nt, rpw = (256, 1) if per_row or V > WAVE_ROW_MAX else (64, 4)
    return [0 if e == 4 else 1, 16 if wide else e, nt, rpw, min(-(-rows // rpw), GRID_MAX), k]


@pytest.mark.parametrize("off", (0, 1))
@pytest.mark.parametrize("name", DTYPES)
@pytest.mark.parametrize("k", (1, 2, 20, 64, 256))
@pytest.mark.parametrize("V", (1, 3, 255, 1025, 2048, 2049, 4099, 16388, 151936))
def test_selection_at_every_width(V, k, name, off):
    """randn rows; bfloat16 at V = 151936 has a few thousand distinct values: heavy ties at every cut."""
    import hpc_lm_topk
    from hpc_rll.rl_utils.lm_topk import token_topk
    rows, k, T = 5 if V <= WAVE_ROW_MAX else 2, min(k, V), (1.0, 2.0)[off]
    x = draw(rows, V, DTYPES[name], seed=V + k)
    xd = place(x, off)
    got = token_topk(xd, k, None, T)
    assert hpc_lm_topk.lm_topk_last_config()[1:7] == expect(xd, xd, rows, V, k, per_row=True)
    check_topk(x, k, got, T, what=f"V={V} k={k} {name} off={off}")


CASES = ("equal", "cut_in_lower_run", "cut_in_upper_run", "ramp_up", "ramp_down", "straddle", "dominant", "zeros", "masked", "k_is_V",
         "dropped")


@pytest.mark.parametrize("name", DTYPES)
@pytest.mark.parametrize("k", (20, 256))
@pytest.mark.parametrize("V", (2049, 16388))
@pytest.mark.parametrize("case", CASES)
def test_selection_on_adversarial_rows(case, V, k, name):
    from hpc_rll.rl_utils.lm_topk import token_topk
    if case == "k_is_V":
        V = k
    i, w, span = torch.arange(V), None, -(-V // 4)          # span: the part of the row a wave owns in the tie pass
    x = draw(2, V, torch.float32, seed=V + k)                # row 1 stays random
    if case == "equal":
        x[0] = 1.5
    elif case == "cut_in_lower_run":                         # fewer upper values than k
        x[0] = torch.where(i % (V // 7) == 3, 2.0, 1.0)
    elif case == "cut_in_upper_run":                         # more upper values than k
        x[0] = torch.where(i % 3 == 1, 2.0, 1.0)
    elif case == "ramp_up":
        x[0] = i.float()
    elif case == "ramp_down":
        x[0] = -i.float()
    elif case == "straddle":                                 # the equal run starts ten entries before a span boundary
        x[0] = (i >= span - 10).float()
        x[1] = ((i >= 2 * span - 3) & (i % 2 == 0)).float() + (i == 5).float() * 3
    elif case == "dominant":
        x[0, 7] = 50.0
    elif case == "zeros":
        x[0] = torch.where(i % 2 == 0, -0.0, 0.0)
        x[1] = torch.where(i % 3 == 0, 0.0, -0.0) - (i % 5 == 0).float()
    elif case == "masked":                                   # fewer than k finite entries: the rest are the lowest masked indices
        x[0] = torch.where(i % 5 == 0, float("nan"), -INF)
        x[0, 3:V:V // 9] = torch.randn(len(range(3, V, V // 9)))
        x[1, 1::2] = -INF
    elif case == "dropped":
        w = torch.tensor([0.0, 1.0])
        x[0] = float("nan")
    x = x.to(DTYPES[name])
    check_topk(x, k, token_topk(place(x), k, place(w)), w=w, what=f"{case} V={V} k={k} {name}")


def teacher(rows, V, k, seed):
    idx, lp = select(draw(rows, V, torch.float32, seed), min(k, V))
    return idx.int(), lp.float()


@pytest.mark.parametrize("off", (0, 1))
@pytest.mark.parametrize("name", DTYPES)
@pytest.mark.parametrize("tail", TAILS)
@pytest.mark.parametrize("k", (1, 20, 256))
@pytest.mark.parametrize("V", (3, 255, 1025, 2049, 4099, 16388, 151936))
def test_divergence_at_every_width(V, k, tail, name, off):
    import hpc_lm_topk
    rows, T = 5 if V <= WAVE_ROW_MAX else 2, (1.0, 2.0)[off]
    x, (idx, lp) = draw(rows, V, DTYPES[name], seed=V, scale=2.0), teacher(rows, V, k, seed=V + 1)
    g = torch.randn(rows, generator=torch.Generator().manual_seed(V + 2))
    kl, grad, xd = run_kl(x, idx, lp, None, g, tail, T, off)
    cfg = hpc_lm_topk.lm_topk_last_config()
    assert cfg[8:14] == expect(xd, xd, rows, V, idx.shape[-1]) and cfg[15:21] == expect(xd, xd.grad, rows, V, idx.shape[-1])
    check(kl_oracle(x, idx, lp, None, g, tail, T), (kl, grad), DTYPES[name], f"{tail} V={V} k={k} {name} off={off}")


@pytest.mark.parametrize("name", DTYPES)
@pytest.mark.parametrize("tail", TAILS)
def test_concentrated_student(tail, name):
    """The student puts all but 1e-4 of its mass on the teacher's first entry: 1 - P by subtraction loses the value."""
    rows, V, k = 3, 4099, 20
    x, (idx, lp) = draw(rows, V, torch.float32, seed=1), teacher(rows, V, k, seed=2)
    x[torch.arange(rows), idx[:, 0].long()] = 18.0
    x = x.to(DTYPES[name])
    g = torch.tensor([1.0, -0.5, 2.0])
    kl, grad, _ = run_kl(x, idx, lp, None, g, tail)
    check(kl_oracle(x, idx, lp, None, g, tail), (kl, grad), DTYPES[name], f"concentrated {tail} {name}")


@pytest.mark.parametrize("tail", TAILS)
@pytest.mark.parametrize("case", ("padding", "all_padding", "dropped_nan", "q_above_one", "pipeline", "grid_loop"))
def test_divergence_edges(case, tail):
    from hpc_rll.rl_utils.lm_topk import token_topk
    rows, V, k, w, g = 6, 4099, 20, None, None
    if case == "grid_loop":                                  # more rows than one pass of the capped grid holds, both ops
        rows, V, k = 4 * GRID_MAX + 5, 3, 2
        g = torch.randn(rows, generator=torch.Generator().manual_seed(5))
    if case == "q_above_one":                                # k = V and the teacher's mass rounds above 1
        V = k = 200
    x, (idx, lp) = draw(rows, V, torch.float32, seed=21, scale=2.0), teacher(rows, V, k, seed=22)
    if case in ("padding", "all_padding"):                   # index -1, index V and logp -inf, mixed into live entries
        idx[:, 1::4], idx[:, 2::4], lp[:, 3::4] = -1, V, -INF
        if case == "all_padding":
            idx[2], lp[4] = V, -INF
    elif case == "dropped_nan":
        w = torch.tensor([1.0, 0.0, 0.5, 0.0, 2.0, 1.0])
        x[w == 0] = float("nan")
    elif case == "q_above_one":
        lp = lp + 1e-6
    elif case in ("pipeline", "grid_loop"):                  # the producer's output, fed straight into the consumer
        lpd, idxd = token_topk(place(draw(rows, V, torch.float32, seed=22)), k)
        check_topk(draw(rows, V, torch.float32, seed=22), k, (lpd, idxd), what=case)
        idx, lp = idxd.cpu(), lpd.cpu()
    kl, grad, _ = run_kl(x, idx, lp, w, g, tail)
    assert np.isfinite(kl).all() and np.isfinite(grad).all()
    check(kl_oracle(x, idx, lp, w, g, tail), (kl, grad), torch.float32, f"{case} {tail}")
    if case == "all_padding":
        assert not kl[[2, 4]].any() and not grad[[2, 4]].any()
    if case == "dropped_nan":
        assert not kl[w.numpy() == 0].any() and not grad[w.numpy() == 0].any()
    kl2, grad2, _ = run_kl(x, idx.long(), lp, w, g, tail)    # int64 indices, a second run: identical bits
    assert np.array_equal(kl, kl2) and np.array_equal(grad, grad2)


@pytest.mark.parametrize("name", DTYPES)
@pytest.mark.parametrize("V", (1024, 4099))                 # 16-byte accesses by a wave per row; one element by a workgroup
def test_c_abi_writes_nothing_outside_its_outputs(V, name):
    """Every output lies inside a buffer of sentinels: the k entries per row and the gradient rows are all that changes."""
    import cabi
    rows, k, code = 3, 20, 0 if name == "f32" else 1
    x, y, SENT = place(draw(rows, V, DTYPES[name], seed=9, scale=2.0)), place(draw(rows, V, DTYPES[name], seed=10)), -77.0

    def guarded(n, dtype):
        buf = torch.full((n + 64,), SENT, dtype=dtype, device=dev())
        return buf, buf[32:32 + n]

    (bl, lp), (bi, ix), (bg, grad), (bs, sv) = guarded(rows * k, torch.float32), guarded(rows * k, torch.int32), guarded(rows * V, x.dtype), guarded(4 * rows, torch.float32)
    cabi.call("hpc_rll_lm_topk_forward", dev(), y.data_ptr(), code, None, lp.data_ptr(), ix.data_ptr(), rows, V, k, 1.0)
    s = [sv[i * rows:].data_ptr() for i in range(4)]
    g = place(torch.ones(rows))
    cabi.call("hpc_rll_lm_topk_kl_forward", dev(), x.data_ptr(), code, ix.data_ptr(), 0, lp.data_ptr(), None, *s, rows, V, k, 1, 1.0)
    cabi.call("hpc_rll_lm_topk_kl_backward", dev(), g.data_ptr(), x.data_ptr(), code, ix.data_ptr(), 0, lp.data_ptr(), None, *s[1:],
              grad.data_ptr(), rows, V, k, 1, 1.0)
    cfg = (ctypes.c_int * 21)()
    assert cabi.lib.hpc_rll_lm_topk_last_config(cfg) == 0 and list(cfg)[6] == list(cfg)[13] == list(cfg)[20] == k
    for buf, n in ((bl, rows * k), (bi, rows * k), (bg, rows * V), (bs, 4 * rows)):
        assert (buf[:32] == SENT).all() and (buf[32 + n:] == SENT).all() and not (buf[32:32 + n] == SENT).any()
    check_topk(y.cpu(), k, (lp.view(rows, k), ix.view(rows, k)), what="c abi")
    ref = kl_oracle(x.cpu(), ix.view(rows, k).cpu(), lp.view(rows, k).cpu(), tail="bucket")
    check(ref, (sv[:rows].double().cpu().numpy(), grad.view(rows, V).double().cpu().numpy()), DTYPES[name], "c abi")
