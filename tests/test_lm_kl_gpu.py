"""GPU tier of the full-vocabulary divergences (``hpc_rll.rl_utils.lm_kl``, csrc/lm_kl.hip).

The oracle is this file's own: the definitions of the module docstring (not its gradient table) in float64 on the host through
autograd.  bfloat16 inputs are upcast exactly, so input rounding is in no bar.

Bars (the project's, those of test_grpo_gpu.py): ``conftest.rel_err`` <= 1e-5 on a value; ``conftest.grad_err`` <= 2e-5 on a
float32 gradient; a bfloat16 gradient per element ``|got - exact| <= 2^-8 |exact| + 2e-5 max|grad|``.  Logits are drawn at
scale 1.  The same oracle run in float32 by torch on the host errs against float64, over the cases of the width test, by up
to 1.4e-5 on a value and 1.3e-5 of the gradient's maximum (forward, V = 262144, bfloat16, T = 1), 4.6e-6 / 7.2e-7 (reverse,
V = 151936) and 6.7e-7 / 8.9e-6 (jsd, V = 262144): above the value bar at one case.  No case takes a wider bar all the same:
the kernels form lx - ly and the mixture's logarithm from differences, not from two sums of size ln V, and stay within the
project's bars at every width."""
import numpy as np
import pytest
import torch

from conftest import grad_err, rel_err
from lm_rows import DTYPES, GRID_MAX, WAVE_ROW_MAX, WIDTHS, dev, place

pytestmark = pytest.mark.gpu

MODES = ("forward", "reverse", "jsd")


def oracle(x, y, w=None, g=None, mode="forward", beta=0.5, T=1.0, dt=torch.float64):
    """(kl, d sum(g kl) / dx) as numpy arrays, from host tensors; a token with ``w == 0`` is selected away before anything."""
    a = x.to(dt).clone().requires_grad_(True)
    live = torch.ones(x.shape[:-1], dtype=torch.bool) if w is None else w != 0
    zero = torch.zeros((), dtype=dt)
    lp = torch.log_softmax(torch.where(live[..., None], a, zero) / T, -1)
    lq = torch.log_softmax(torch.where(live[..., None], y.to(dt), zero) / T, -1)

    def kl(la, lb):   # sum e^la (la - lb); an entry of probability 0 adds nothing
        return (la.exp() * torch.where(la.exp() > 0, la - lb, zero)).sum(-1)

    if mode == "jsd":
        m = beta * lq.exp() + (1 - beta) * lp.exp()
        lm = torch.log(torch.where(m > 0, m, torch.ones_like(m)))
        val = beta * kl(lq, lm) + (1 - beta) * kl(lp, lm)
    else:
        val = kl(lq, lp) if mode == "forward" else kl(lp, lq)
    val = torch.where(live, val, zero)
    (val * (1.0 if g is None else g.to(dt))).sum().backward()
    return val.detach().double().numpy(), a.grad.double().numpy()


def run(x, y, w=None, g=None, mode="forward", beta=0.5, T=1.0, off=0):
    """The same through the public function on the device: (kl, grad) as float64 numpy arrays, and the device tensors."""
    from hpc_rll.rl_utils.lm_kl import token_kl_div
    xd, yd = place(x, off).requires_grad_(True), place(y, off)
    kl = token_kl_div(xd, yd, place(w), mode, beta, T)
    assert kl.dtype == torch.float32 and kl.shape == x.shape[:-1] and not yd.requires_grad
    kl.backward(torch.ones_like(kl) if g is None else g.to(dev()))
    assert xd.grad.dtype == x.dtype and xd.grad.shape == x.shape
    return kl.detach().double().cpu().numpy(), xd.grad.double().cpu().numpy(), xd, yd


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


def draw(rows, V, dtype, seed=0):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(rows, V, generator=gen).to(dtype), torch.randn(rows, V, generator=gen).to(dtype),
            torch.randn(rows, generator=gen))


def expect(x, y, grad, rows, V, mode):
    """[element type, bytes per access, threads per row, rows per workgroup, workgroups, mode] of a launch over these bases:
    16 bytes when every base and the pitch lie on 16, a wave per row up to WAVE_ROW_MAX, the grid capped at GRID_MAX."""
    e = x.element_size()
    wide = all(t.data_ptr() % 16 == 0 for t in (x, y, grad)) and (V * e) % 16 == 0
    nt, rpw = (256, 1) if V > WAVE_ROW_MAX else (64, 4)
    return [0 if e == 4 else 1, 16 if wide else e, nt, rpw, min(-(-rows // rpw), GRID_MAX), MODES.index(mode)]


@pytest.mark.parametrize("off", (0, 1))
@pytest.mark.parametrize("name", DTYPES)
@pytest.mark.parametrize("V", WIDTHS)
@pytest.mark.parametrize("mode", MODES)
def test_values_and_gradients_at_every_width(mode, V, name, off):
    import hpc_lm_kl
    rows = 5 if V <= WAVE_ROW_MAX else 2          # a partial last workgroup; the LDS parity flips between the two rows
    T, beta = (1.0, 0.1) if off == 0 else (2.0, 0.5)
    x, y, g = draw(rows, V, DTYPES[name], seed=V)
    kl, grad, xd, yd = run(x, y, None, g, mode, beta, T, off)
    cfg = hpc_lm_kl.lm_kl_last_config()
    assert cfg[1:7] == expect(xd, yd, xd, rows, V, mode) and cfg[8:14] == expect(xd, yd, xd.grad, rows, V, mode)
    check(oracle(x, y, None, g, mode, beta, T), (kl, grad), DTYPES[name], f"{mode} V={V} {name} off={off}")


@pytest.mark.parametrize("offs", ((1, 0, 0), (0, 1, 0), (0, 0, 1)))
@pytest.mark.parametrize("name", DTYPES)
@pytest.mark.parametrize("mode", MODES)
def test_one_base_off_16_bytes_takes_the_one_element_path(mode, name, offs):
    """Student, teacher and gradient in turn, through the C ABI (the public function allocates the gradient itself)."""
    import cabi
    import ctypes
    rows, V, m = 5, 1024, MODES.index(mode)
    x, y, g = draw(rows, V, DTYPES[name], seed=3)
    xd, yd, grad, gd = place(x, offs[0]), place(y, offs[1]), place(torch.zeros_like(x), offs[2]), place(g)
    out = torch.zeros(4, rows, device=dev())
    o = [out[i].data_ptr() for i in range(4)]
    code = 0 if name == "f32" else 1
    cabi.call("hpc_rll_lm_kl_forward", dev(), xd.data_ptr(), yd.data_ptr(), code, None, *o, rows, V, m, 0.5, 1.0)
    cabi.call("hpc_rll_lm_kl_backward", dev(), gd.data_ptr(), xd.data_ptr(), yd.data_ptr(), code, None, *o, grad.data_ptr(), rows, V,
              m, 0.5, 1.0)
    cfg = (ctypes.c_int * 14)()
    assert cabi.lib.hpc_rll_lm_kl_last_config(cfg) == 0
    assert list(cfg)[1:7] == expect(xd, yd, xd, rows, V, mode) and list(cfg)[8:14] == expect(xd, yd, grad, rows, V, mode)
    assert list(cfg)[9] == x.element_size() and (list(cfg)[2] == 16) == (offs[2] == 1)
    check(oracle(x, y, None, g, mode), (out[0].double().cpu().numpy(), grad.double().cpu().numpy()), DTYPES[name], f"{mode} {name} {offs}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", ("masked", "dominant", "dropped_nan", "grid_loop", "no_rows", "lead_shape", "zero_upstream"))
def test_edges(case, mode):
    V, w, g = 4099, None, None
    x, y, _ = draw(6, V, torch.float32, seed=11)
    if case == "masked":                           # -inf in both rows: contributes nothing, gradient exactly 0
        x[:, 5:4000:3] = y[:, 5:4000:3] = -float("inf")
    elif case == "dominant":                       # one entry holds 96 % of the mass, a different one in either row
        x[:, 0] += 12.0                            # (the reverse gradient there is p0 (1 - p0) (t0 - mean t): float32 resolves
        y[:, 1] += 12.0                            # it against the 2e-5 bar only while 1 - p0 stays far above 1e-7 / 2e-5)
    elif case == "dropped_nan":                    # NaN rows under weight 0: value 0, zero gradient row, neighbours untouched
        w = torch.tensor([1.0, 0.0, 0.5, 0.0, 2.0, 1.0])
        x[w == 0] = y[w == 0] = float("nan")
    elif case == "grid_loop":                      # more rows than one pass of the capped grid holds
        x, y, g = draw(4 * GRID_MAX + 5, 3, torch.float32, seed=12)
    elif case == "no_rows":
        x, y = x[:0], y[:0]
    elif case == "lead_shape":
        x, y = x[:, :600].reshape(2, 3, 2, 300).contiguous(), y[:, :600].reshape(2, 3, 2, 300).contiguous()
    elif case == "zero_upstream":
        g = torch.zeros(6)
    kl, grad, xd, yd = run(x, y, w, g, mode)
    assert np.isfinite(kl).all() and np.isfinite(grad).all()
    check(oracle(x, y, w, g, mode), (kl, grad), torch.float32, f"{case} {mode}")
    if case == "masked":
        assert not grad[:, 5:4000:3].any()
    if case == "dropped_nan":
        assert not kl[w.numpy() == 0].any() and not grad[w.numpy() == 0].any()
    if case == "zero_upstream":
        assert not grad.any()
    kl2, grad2, _, _ = run(x, y, w, g, mode)       # no atomics: identical bits on a repeat
    assert np.array_equal(kl, kl2) and np.array_equal(grad, grad2)


@pytest.mark.parametrize("name", DTYPES)
@pytest.mark.parametrize("mode", MODES)
def test_equal_rows_have_no_divergence(mode, name):
    """x == y: value 0 within the value bar; the gradient is p times a difference that vanishes, so 2e-5 of max p bounds it."""
    x, _, _ = draw(3, 4099, DTYPES[name], seed=5)
    kl, grad, _, _ = run(x, x.clone(), mode=mode, beta=0.1)
    pmax = float(torch.softmax(x.double(), -1).max())
    assert np.abs(kl).max() <= 1e-5 and np.abs(grad).max() <= 2e-5 * pmax


def test_identities():
    from hpc_rll.rl_utils.lm_kl import GKDLoss, token_kl_div
    x, y, _ = draw(5, 1025, torch.float32, seed=7)
    assert rel_err(run(x, y, mode="forward")[0], run(y, x, mode="reverse")[0]) <= 1e-5
    assert rel_err(run(x, y, mode="jsd", beta=0.5)[0], run(y, x, mode="jsd", beta=0.5)[0]) <= 1e-5
    xd, yd = place(x.reshape(1, 5, 1025)).requires_grad_(True), place(y.reshape(1, 5, 1025))
    mask = place(torch.tensor([[1.0, 1.0, 0.0, 1.0, 0.0]]))
    for agg in ("token", "sequence"):              # one sequence: both aggregates are the masked mean
        loss = GKDLoss("jsd", 0.3, 2.0, agg)(xd, yd, mask)
        kl = token_kl_div(xd, yd, mask, "jsd", 0.3, 2.0)
        assert torch.equal(loss, (mask * kl).sum() / mask.sum())
    loss.backward()
    ref = oracle(x.reshape(1, 5, 1025), y.reshape(1, 5, 1025), mask.cpu(), mask.cpu() / 3, "jsd", 0.3, 2.0)
    check(ref, (kl.detach().double().cpu().numpy(), xd.grad.double().cpu().numpy()), torch.float32, "GKDLoss")
