"""Misaligned operands and odd B in the column-scan family (scan_ops.hip, scan_masked.hip, gae_masked.hip; run with
``-m gpu`` on an MI355X).

Which of these ops have an alignment fallback to enter:
  * TD(lambda), unmasked and masked, takes two columns per lane only when B is even and value, reward, weight, next_value
    and the OUTPUT grad_buf are 8-byte (byte masks 2-byte) aligned, and only from B >= 65409;
  * masked GAE (forward and backward) the same over its operands and outputs, only when one launch moves >= 300 MB;
  * V-trace and UPGO always scan one column per lane (scan_ops.hip: ``scan_cfg(T, B, false)``; scan_masked.hip: "V = 1 for
    V-trace"), so their scans have NO such branch: the tests of them here are robustness checks on misaligned views, not
    coverage of a fallback.  Their categorical kernels do choose a path on the 16-byte alignment of the logits and of
    grad_target_output, which a 4-byte-only view turns off.
Torch allocations are 256-byte aligned, so the fallbacks are entered by passing contiguous views that start 4 (or 8)
bytes past a 16-byte boundary, byte masks at odd addresses, odd B and ``next_value = value_buffer[1:]`` -- what a slice
of a rollout buffer gives a user.  Every operand that is moved lives in a guarded buffer (tests/guarded.py); no pointer
is less than 4-byte aligned (1-byte for byte masks).

Outputs: the Python API allocates them (aligned), so an output pointer only takes part in the choice through the entry
points that accept caller-provided outputs.  Those are driven at the end of this file with NaN-filled outputs between
sentinel bands: ``hpc_rl_utils.TdLambdaForward`` / ``TdLambdaBackward`` (grad_buf is in TD(lambda)'s alignment rule),
the C ABI's ``hpc_rll_td_lambda_masked_forward`` (hpc_rl_utils has no list form of the masked ops), and the native
lists of ``VTraceForward`` / ``VTraceBackward`` / ``UpgoForward`` / ``UpgoBackward`` (workspace and gradients).
``GaeForward`` / ``GaeBackward`` pass their outputs to ``hpc_rll_gae_forward`` / ``_backward``, i.e. the auto dispatch
that tests/test_gae_dispatch_gpu.py drives with each output 1 and 2 floats off alignment between the same bands.

Losses and gradients are compared with the fp64 oracles of tests/test_masked_returns_gpu.py,
tests/test_masked_gae_gpu.py and oracle.ref_torch, with the project's tolerances (1e-5 losses / returns, 2e-5 gradients).
"""
import pytest
import torch

import test_masked_gae_gpu as MG
import test_masked_returns_gpu as MR
from conftest import grad_err, rel_err
from guarded import GuardedF32, place, place_mask

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 1e-5
N = 3
SHAPES = [(T, B) for B in (65536, 65537, 65538, 131072 + 2) for T in (9, 130)]


def _gen(T, B, salt=0):
    return torch.Generator(device=DEV).manual_seed(T * 1000003 + B + salt)


def _moved(tensors, name, off):
    """The dict of float tensors with ``name`` (or nothing, name = None) re-placed ``off`` floats off alignment."""
    out = dict(tensors)
    if name is not None:
        out[name] = place(tensors[name], off)
    return out


def _leaf(x):
    return x.detach().requires_grad_(True)


def _np(x):
    return x.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------------------- TD(lambda)
def _td_inputs(T, B):
    g = _gen(T, B)
    return dict(value=torch.randn(T + 1, B, device=DEV, generator=g), reward=torch.randn(T, B, device=DEV, generator=g),
                weight=torch.rand(T, B, device=DEV, generator=g))


@pytest.mark.parametrize("T,B", SHAPES)
def test_td_lambda_float_operands_off_alignment(T, B):
    from hpc_rll.rl_utils.td import TDLambda
    base = _td_inputs(T, B)
    for name in (None, "value", "reward", "weight"):
        x = _moved(base, name, 1)
        v = _leaf(x["value"])
        loss = TDLambda(T, B)(v, x["reward"], x["weight"], 0.9, 0.8)
        (gv,) = torch.autograd.grad(loss, v)
        o_loss, o_gv = MR.td_oracle(v, x["reward"], weight=x["weight"], gamma=0.9, lam=0.8)
        assert rel_err(o_loss.item(), loss.item()) <= TOL, (name, o_loss.item(), loss.item())
        assert grad_err(_np(o_gv), _np(gv), "grad_value") <= 2 * TOL, name
        MR.check_td(v, x["reward"], weight=x["weight"])                       # the masked entry point without masks


@pytest.mark.parametrize("T,B", SHAPES)
def test_masked_td_lambda_masks_and_forms_off_alignment(T, B):
    base = _td_inputs(T, B)
    g = _gen(T, B, 1)
    for kind, off in (("bool", 1), ("uint8", 1), ("uint8", 0), ("float32", 1)):
        done = MR._mask(g, T, B, 0.05, kind)
        flag = ((done != 0) | MR._mask(g, T, B, 0.05, "bool")).to(done.dtype)
        d, f = place_mask(done, off), place_mask(flag, off)
        v = _leaf(base["value"])
        MR.check_td(v, base["reward"], done=d, weight=base["weight"])                     # mask moved, floats aligned
        MR.check_td(v, base["reward"], done=done, traj_flag=f)                            # only traj_flag moved
        buf = _leaf(place(base["value"], 1))
        MR.check_td(buf, base["reward"], done=d, traj_flag=f, weight=base["weight"])      # stacked, value moved too
        # next-value form on one rollout buffer: value = buf[:-1], next_value = buf[1:] (4-byte aligned only when B is odd)
        for b in (base["value"], place(base["value"], 1)):
            b = b.detach()
            MR.check_td(_leaf(b[:-1]), base["reward"], done=d, traj_flag=f, next_value=b[1:], weight=base["weight"])


# ----------------------------------------------------------------------------------------------------------- V-trace
def _vt_inputs(T, B):
    g = _gen(T, B, 2)
    return dict(to=torch.randn(T, B, N, device=DEV, generator=g), bo=torch.randn(T, B, N, device=DEV, generator=g),
                value=torch.randn(T + 1, B, device=DEV, generator=g), reward=torch.randn(T, B, device=DEV, generator=g),
                weight=torch.rand(T, B, device=DEV, generator=g)), torch.randint(0, N, (T, B), device=DEV, generator=g)


KW_VT = dict(gamma=0.99, lam=0.95, rho_clip=1.0, c_clip=0.9, pg_clip=1.1, co=MR.CO)


@pytest.mark.parametrize("T,B", SHAPES)
def test_vtrace_float_operands_off_alignment(T, B):
    from hpc_rll.rl_utils.vtrace import VTrace
    base, a = _vt_inputs(T, B)
    co = [torch.tensor([c], device=DEV) for c in MR.CO]
    for name in (None, "to", "bo", "value", "reward", "weight"):
        x = _moved(base, name, 1)
        to, v = _leaf(x["to"]), _leaf(x["value"])
        out = VTrace(T, B, N)(to, x["bo"], a, v, x["reward"], x["weight"], 0.99, 0.95, 1.0, 0.9, 1.1)
        gt, gv = torch.autograd.grad(list(out), (to, v), co)
        o_losses, o_gt, o_gv = MR.vtrace_oracle(to, x["bo"], a, v, x["reward"], weight=x["weight"], **KW_VT)
        for k, o, y in zip(("policy", "value", "entropy"), o_losses, out):
            assert rel_err(o, y.item()) <= TOL, (name, k, o, y.item())
        assert grad_err(_np(o_gt), _np(gt), "grad_target") <= 2 * TOL, name
        assert grad_err(_np(o_gv), _np(gv), "grad_value") <= 2 * TOL, name
        MR.check_vt(to, x["bo"], a, v, x["reward"], weight=x["weight"])       # the masked entry point without masks


@pytest.mark.parametrize("T,B", SHAPES)
def test_masked_vtrace_masks_and_forms_off_alignment(T, B):
    base, a = _vt_inputs(T, B)
    g = _gen(T, B, 3)
    to = _leaf(base["to"])
    for kind, off in (("bool", 1), ("uint8", 1), ("float32", 1)):
        done = MR._mask(g, T, B, 0.05, kind)
        flag = ((done != 0) | MR._mask(g, T, B, 0.05, "bool")).to(done.dtype)
        d, f = place_mask(done, off), place_mask(flag, off)
        MR.check_vt(to, base["bo"], a, _leaf(base["value"]), base["reward"], done=d, weight=base["weight"])
        buf = place(base["value"], 1).detach()
        MR.check_vt(to, base["bo"], a, _leaf(buf), base["reward"], done=d, traj_flag=f)
        MR.check_vt(to, base["bo"], a, _leaf(buf[:-1]), base["reward"], done=d, traj_flag=f, next_value=buf[1:],
                    weight=base["weight"])


# -------------------------------------------------------------------------------------------------------------- UPGO
def _upgo_problem(T, B):
    """Inputs whose switch margin |r_{t+1} + V_{t+2} - V_{t+1}| stays above 1e-3 (fp32 and fp64 then take the same branch
    everywhere, cf. test_losses_gpu.test_upgo_oracle), and the fp64 oracle's loss and gradient for them."""
    from oracle import ref_torch as R
    g = _gen(T, B, 4)
    base = dict(to=torch.randn(T, B, N, device=DEV, generator=g), rho=torch.rand(T, B, device=DEV, generator=g) + 0.5,
                reward=torch.randn(T, B, device=DEV, generator=g), value=torch.randn(T + 1, B, device=DEV, generator=g))
    a = torch.randint(0, N, (T, B), device=DEV, generator=g)
    margin = base["reward"] + base["value"][1:] - base["value"][:-1]
    base["reward"] = base["reward"] + (margin.abs() < 1e-3) * 0.01
    margin = base["reward"].double() + base["value"][1:].double() - base["value"][:-1].double()
    assert float(margin.abs().min()) > 1e-4
    to64 = base["to"].double().requires_grad_(True)
    l64 = R.upgo_loss(to64, base["rho"].double(), a, base["reward"].double(), base["value"].double())
    (g64,) = torch.autograd.grad(l64, to64)
    return base, a, l64, g64


@pytest.mark.parametrize("T,B", SHAPES)
def test_upgo_float_operands_off_alignment(T, B):
    """UPGO switches between the return and the value on the sign of r_{t+1} + V_{t+2} - V_{t+1}; the inputs keep that
    margin above 1e-3 so that fp32 and fp64 take the same branch everywhere (cf. test_losses_gpu.test_upgo_oracle)."""
    from hpc_rll.rl_utils.upgo import UPGO
    base, a, l64, g64 = _upgo_problem(T, B)
    for name in (None, "to", "rho", "reward", "value"):
        x = _moved(base, name, 1)
        to = _leaf(x["to"])
        loss = UPGO(T, B, N)(to, x["rho"], a, x["reward"], x["value"])
        (gt,) = torch.autograd.grad(loss, to)
        assert rel_err(l64.item(), loss.item()) <= TOL, (name, l64.item(), loss.item())
        assert grad_err(_np(g64), _np(gt), "grad_target") <= 2 * TOL, name


# --------------------------------------------------------------------------------- all-zero masks: the unmasked bits
@pytest.mark.parametrize("T,B", SHAPES)
def test_zero_masks_on_misaligned_inputs_give_the_unmasked_bits(T, B):
    """scan_masked.hip's promise: without episode ends a masked call gives its unmasked sibling's bits.  Both run on the
    SAME misaligned float operands (one column per lane in both); neither is compared with an aligned run, whose chunking
    may differ."""
    from hpc_rll.rl_utils.td import TDLambda, masked_td_lambda
    from hpc_rll.rl_utils.vtrace import VTrace, masked_vtrace
    td = _td_inputs(T, B)
    v, r, w = _leaf(place(td["value"], 1)), place(td["reward"], 1), place(td["weight"], 1)
    ref = TDLambda(T, B)(v, r, w, 0.9, 0.8)
    (ref_g,) = torch.autograd.grad(ref, v)
    vt, a = _vt_inputs(T, B)
    to, bo, vv = _leaf(place(vt["to"], 1)), place(vt["bo"], 1), _leaf(place(vt["value"], 1))
    co = [torch.tensor([c], device=DEV) for c in MR.CO]
    vref = VTrace(T, B, N)(to, bo, a, vv, r, w, 0.99, 0.95, 1.0, 0.9, 1.1)
    vref_g = torch.autograd.grad(list(vref), (to, vv), co)
    zeros = [torch.zeros(T, B, dtype=torch.bool, device=DEV), torch.zeros(T, B, dtype=torch.uint8, device=DEV),
             torch.zeros(T, B, device=DEV)]
    for z in zeros:
        m = place_mask(z, 1)
        for kw in ({"done": m}, {"done": m, "traj_flag": m}, {"traj_flag": m}):
            loss = masked_td_lambda(v, r, weight=w, gamma=0.9, lambda_=0.8, **kw)
            (gv,) = torch.autograd.grad(loss, v)
            assert torch.equal(loss, ref) and torch.equal(gv, ref_g), ("td", z.dtype, sorted(kw))
        out = masked_vtrace(to, bo, a, vv, r, m, w, 0.99, 0.95, 1.0, 0.9, 1.1)
        gg = torch.autograd.grad(list(out), (to, vv), co)
        assert all(torch.equal(x, y) for x, y in zip(out, vref)), ("vtrace", z.dtype)
        assert all(torch.equal(x, y) for x, y in zip(gg, vref_g)), ("vtrace", z.dtype)


# -------------------------------------------------------------------------------------------------------- masked GAE
# T = 353 at B = 65536 is the smallest T whose launch moves >= 300 MB: the two-columns-per-lane kernels of gae_masked.hip,
# which T in {9, 130} (one column per lane at every alignment) never select
GAE_SHAPES = SHAPES + [(353, 65536), (353, 65538)]


@pytest.mark.parametrize("T,B", GAE_SHAPES)
def test_masked_gae_operands_off_alignment(T, B):
    assert (T, B) in SHAPES or 13.0 * T * B >= 300e6
    g = _gen(T, B, 5)
    value = torch.randn(T + 1, B, device=DEV, generator=g)
    reward = torch.randn(T, B, device=DEV, generator=g)
    ga = torch.randn(T, B, device=DEV, generator=g)
    done = MG._mask(g, T, B, 0.05, "bool")
    MG._check(_leaf(value), _leaf(reward), ga, done=done)                                # everything aligned
    for off in (1, 2):
        MG._check(_leaf(place(value, off)), _leaf(reward), ga, done=done)
        MG._check(_leaf(value), _leaf(place(reward, off)), ga, done=done)
        MG._check(_leaf(value), _leaf(reward), place(ga, off), done=done)                # the backward's input
        soft = torch.rand(T, B, device=DEV, generator=g)
        MG._check(_leaf(value), _leaf(reward), ga, done=place(soft, off))                # float32 soft mask
        buf = place(value, off).detach()                                                 # next-value form on one buffer
        MG._check(_leaf(buf[:-1]), _leaf(reward), ga, done=done, next_value=_leaf(buf[1:]))
    for kind in ("bool", "uint8"):
        m = MG._mask(g, T, B, 0.05, kind)
        f = ((m != 0) | MG._mask(g, T, B, 0.05, "bool")).to(m.dtype)
        MG._check(_leaf(value), _leaf(reward), ga, done=place_mask(m, 1))                # byte mask at an odd address
        MG._check(_leaf(value), _leaf(reward), ga, done=m, traj_flag=place_mask(f, 1))
        MG._check(_leaf(value), _leaf(reward), ga, done=place_mask(m, 0), traj_flag=place_mask(f, 0))


# ------------------------------------------------------------------- caller-provided outputs between sentinel bands
def _written_and_guarded(buf, what):
    torch.cuda.synchronize()
    buf.check(what)
    buf.assert_written(what)


@pytest.mark.parametrize("T,B", SHAPES)
@pytest.mark.parametrize("gb_off,gv_off", [(0, 1), (1, 1), (1, 0)])
def test_td_lambda_list_entry_points_with_guarded_outputs(T, B, gb_off, gv_off):
    """grad_buf 4-byte-only aligned with every input aligned: the one output pointer in TD(lambda)'s two-column rule."""
    import hpc_rl_utils as U
    x = _td_inputs(T, B)
    o_loss, o_gv = MR.td_oracle(x["value"], x["reward"], weight=x["weight"], gamma=0.9, lam=0.8)
    loss = GuardedF32(1, 1, 0, DEV)
    gb = GuardedF32(T, B, gb_off, DEV)
    gv = GuardedF32(T + 1, B, gv_off, DEV)
    U.TdLambdaForward([x["value"], x["reward"], x["weight"]], [loss.t.view(1), gb.t], 0.9, 0.8)
    _written_and_guarded(gb, "grad_buf")
    _written_and_guarded(loss, "loss")
    U.TdLambdaBackward([torch.ones(1, device=DEV), gb.t], [gv.t])
    _written_and_guarded(gv, "grad_value")
    assert rel_err(o_loss.item(), loss.t.item()) <= TOL, (o_loss.item(), loss.t.item())
    assert grad_err(_np(o_gv), _np(gv.t), "grad_value") <= 2 * TOL


@pytest.mark.parametrize("T,B", SHAPES)
@pytest.mark.parametrize("gb_off", [0, 1])
@pytest.mark.parametrize("kind", ["bool", "float32"])
def test_masked_td_lambda_c_abi_with_guarded_outputs(T, B, gb_off, kind):
    """hpc_rll_td_lambda_masked_forward (both input forms) with grad_buf, loss and partials of the caller."""
    import cabi
    x = _td_inputs(T, B)
    g = _gen(T, B, 6)
    done = MR._mask(g, T, B, 0.05, kind)
    flag = ((done != 0) | MR._mask(g, T, B, 0.05, "bool")).to(done.dtype)
    code = 1 if kind == "float32" else 0
    npart = int(cabi.lib.hpc_rll_partials_floats(B))
    for stacked in (True, False):
        v = x["value"] if stacked else x["value"][:-1]
        nv = None if stacked else x["value"][1:]
        o_loss, o_gv = MR.td_oracle(v, x["reward"], done=done, traj_flag=flag, next_value=nv, weight=x["weight"])
        loss, part = GuardedF32(1, 1, 0, DEV), GuardedF32(1, npart, 0, DEV)
        gb = GuardedF32(T, B, gb_off, DEV)
        cabi.call("hpc_rll_td_lambda_masked_forward", DEV, v.data_ptr(), cabi.ptr(nv), x["reward"].data_ptr(),
                  x["weight"].data_ptr(), 2, done.data_ptr(), flag.data_ptr(), code, loss.t.data_ptr(), gb.t.data_ptr(),
                  part.t.data_ptr(), T, B, 0.9, 0.8, 1.0 / (T * B))
        _written_and_guarded(gb, "grad_buf")
        _written_and_guarded(loss, "loss")
        part.check("partials")
        gv = GuardedF32(T + 1, B, 1, DEV)
        one = torch.ones(1, device=DEV)
        cabi.call("hpc_rll_td_lambda_backward", DEV, one.data_ptr(), gb.t.data_ptr(), gv.t.data_ptr(), T, B)
        _written_and_guarded(gv, "grad_value")
        assert rel_err(o_loss.item(), loss.t.item()) <= TOL, (stacked, o_loss.item(), loss.t.item())
        assert grad_err(_np(o_gv), _np(gv.t[:o_gv.shape[0]]), "grad_value") <= 2 * TOL, stacked
        assert not bool(gv.t[T].any()), "the bootstrap row gets a zero gradient"


@pytest.mark.parametrize("T,B", SHAPES)
@pytest.mark.parametrize("off", [0, 1])
def test_vtrace_list_entry_points_with_guarded_outputs(T, B, off):
    import cabi
    import hpc_rl_utils as U
    base, a = _vt_inputs(T, B)
    o_losses, o_gt, o_gv = MR.vtrace_oracle(base["to"], base["bo"], a, base["value"], base["reward"],
                                            weight=base["weight"], **KW_VT)
    losses = GuardedF32(1, 3, off, DEV)
    ws = GuardedF32(1, int(cabi.lib.hpc_rll_vtrace_workspace_floats(T, B)), off, DEV)
    U.VTraceForward([base["to"], base["bo"], a, base["value"], base["reward"], base["weight"]],
                    [losses.t.view(3), ws.t.view(-1)], 0.99, 0.95, 1.0, 0.9, 1.1)
    _written_and_guarded(losses, "losses")
    ws.check("workspace")
    gt, gv = GuardedF32(T, B * N, off, DEV), GuardedF32(T + 1, B, 1, DEV)
    co = [torch.tensor([c], device=DEV) for c in MR.CO]
    U.VTraceBackward(co + [base["to"], a, ws.t.view(-1)], [gt.t.view(T, B, N), gv.t])
    _written_and_guarded(gt, "grad_target_output")
    _written_and_guarded(gv, "grad_value")
    ws.check("workspace after the backward")
    for k, o, y in zip(("policy", "value", "entropy"), o_losses, losses.t.view(3)):
        assert rel_err(o, y.item()) <= TOL, (k, o, y.item())
    assert grad_err(_np(o_gt), _np(gt.t.view(T, B, N)), "grad_target") <= 2 * TOL
    assert grad_err(_np(o_gv), _np(gv.t), "grad_value") <= 2 * TOL


@pytest.mark.parametrize("T,B", SHAPES)
@pytest.mark.parametrize("off", [0, 1])
def test_upgo_list_entry_points_with_guarded_outputs(T, B, off):
    import cabi
    import hpc_rl_utils as U
    base, a, l64, g64 = _upgo_problem(T, B)
    loss = GuardedF32(1, 1, off, DEV)
    ws = GuardedF32(1, int(cabi.lib.hpc_rll_upgo_workspace_floats(T, B)), off, DEV)
    U.UpgoForward([base["to"], base["rho"], a, base["reward"], base["value"]], [loss.t.view(1), ws.t.view(-1)])
    _written_and_guarded(loss, "loss")
    ws.check("workspace")
    gt = GuardedF32(T, B * N, off, DEV)
    U.UpgoBackward([torch.ones(1, device=DEV), base["to"], a, ws.t.view(-1)], [gt.t.view(T, B, N)])
    _written_and_guarded(gt, "grad_target_output")
    assert rel_err(l64.item(), loss.t.item()) <= TOL, (l64.item(), loss.t.item())
    assert grad_err(_np(g64), _np(gt.t.view(T, B, N)), "grad_target") <= 2 * TOL
