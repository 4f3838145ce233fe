"""CPU tier of the R2D2 sequence loss (``hpc_rll.rl_utils.r2d2``, csrc/r2d2.hip): the parts that need no GPU -- the new C entry
points are declared and exported and answer argument errors with status codes before any HIP call (nulls, then sizes, then
alignment, then the N limit, then empty shapes), the workspace formula, the extension rejects CPU tensors and names wrong
arguments, and the Python signatures.  Parity and everything that launches is in tests/test_r2d2_gpu.py."""
import ctypes
import inspect

import pytest
import torch

FWD, BWD, LAST, WS = ("hpc_rll_r2d2_forward", "hpc_rll_r2d2_backward", "hpc_rll_r2d2_last_config",
                      "hpc_rll_r2d2_workspace_floats")
EINVAL, EALIGN, EUNSUPPORTED = -1, -2, -3
T, B, N = 9, 3, 4


def test_c_entry_points_declared_and_exported():
    import cabi
    for name, nargs in ((FWD, 23), (BWD, 10), (LAST, 1)):
        assert name in cabi.SIGNATURES, name
        assert hasattr(cabi.lib, name), name
        assert cabi.SIGNATURES[name][0] is ctypes.c_int and len(cabi.SIGNATURES[name][1]) == nargs, name
    assert cabi.SIGNATURES[WS][0] is ctypes.c_int64 and len(cabi.SIGNATURES[WS][1]) == 2
    assert cabi.lib.hpc_rll_abi_version() == 6


def test_workspace_holds_the_documented_layout():
    """delta | qa | v, T*B floats each, then one partial sum per workgroup of the window launch (at most 512)."""
    import cabi
    ws = cabi.lib.hpc_rll_r2d2_workspace_floats
    for t, b in ((1, 1), (9, 3), (120, 64), (128, 4096), (5, 33000)):
        assert 3 * t * b + 512 <= ws(t, b) <= 3 * t * b + 8192, (t, b)
    assert ws(0, 7) >= 0 and ws(7, 0) >= 0
    assert ws(-1, 4) == EINVAL and ws(4, -1) == EINVAL


@pytest.fixture(scope="module")
def buf():
    """A small host buffer as a stand-in for device memory: the calls below return before anything reads it."""
    b = (ctypes.c_float * 64)()
    assert ctypes.addressof(b) % 8 == 0
    return b


def _caller(fn, names, base, tail):
    def call(**kw):
        a = list(base)
        for k, v in kw.items():
            a[names.index(k)] = v
        return fn(*a, *tail, None)
    return call


def test_forward_argument_errors_are_status_codes(buf):
    import cabi
    P = ctypes.addressof(buf)
    names = ["q", "target_q", "action", "reward", "done", "mask_dtype", "weight", "weight_mode", "loss", "td_error", "priority",
             "ws", "T", "B", "N", "nstep", "burnin"]
    call = _caller(cabi.lib.hpc_rll_r2d2_forward, names, [P, P, P, P, None, 0, None, 0, P, P, P, P, 9, 4, 3, 2, 1],
                   (0.997, 1, 1, 0.9, 1.0))
    for name in ("q", "target_q", "action", "reward", "loss", "td_error", "priority", "ws"):
        assert call(**{name: None}) == EINVAL, name
    assert call(T=-1) == EINVAL
    assert call(B=-1) == EINVAL
    assert call(N=0) == EINVAL
    assert call(N=-3) == EINVAL
    assert call(nstep=0) == EINVAL
    assert call(nstep=-2) == EINVAL
    assert call(burnin=-1) == EINVAL
    assert call(mask_dtype=2) == EINVAL
    assert call(weight_mode=3) == EINVAL
    assert call(weight_mode=1) == EINVAL                       # a mode without its weight
    assert call(weight=P) == EINVAL                            # a weight without its mode
    assert call(q=P + 2) == EALIGN
    assert call(weight=P + 1, weight_mode=2) == EALIGN
    assert call(action=P + 4) == EALIGN                        # int64 off 8-byte alignment
    assert call(done=P + 2, mask_dtype=1) == EALIGN            # a float mask off 4
    assert call(N=1025) == EUNSUPPORTED
    assert call(N=2048, weight=P, weight_mode=1) == EUNSUPPORTED
    assert call(N=2048, reward=None) == EINVAL                 # nulls come before the N limit
    assert call(N=2048, nstep=0) == EINVAL                     # and so do the sizes
    assert call(N=2048, q=P + 2) == EALIGN                     # and alignment
    assert call(T=0, loss=None) == EINVAL                      # an empty batch still needs somewhere to write the zero
    assert call(T=0, N=2048) == EUNSUPPORTED                   # the N limit comes before the empty return
    assert call(T=0, B=-1) == EINVAL


def test_backward_argument_errors_are_status_codes(buf):
    import cabi
    P = ctypes.addressof(buf)
    names = ["g_loss", "action", "ws", "grad_q", "T", "B", "N", "nstep", "burnin"]
    call = _caller(cabi.lib.hpc_rll_r2d2_backward, names, [P, P, P, P, 9, 4, 3, 2, 1], ())
    for name in ("action", "ws", "grad_q"):
        assert call(**{name: None}) == EINVAL, name
    assert call(T=-1) == EINVAL
    assert call(B=-1) == EINVAL
    assert call(N=0) == EINVAL
    assert call(nstep=0) == EINVAL
    assert call(burnin=-1) == EINVAL
    assert call(grad_q=P + 2) == EALIGN
    assert call(g_loss=P + 1) == EALIGN
    assert call(action=P + 4) == EALIGN
    assert call(N=1025) == EUNSUPPORTED
    assert call(N=2048, ws=None) == EINVAL
    assert call(N=2048, grad_q=P + 2) == EALIGN
    assert call(B=0) == 0 and call(T=0) == 0                   # empty: nothing launched
    assert call(B=0, action=None, ws=None, grad_q=None) == 0


def test_record_is_empty_and_argument_errors_leave_it_so(buf):
    import cabi
    P = ctypes.addressof(buf)
    L = cabi.lib
    out = (ctypes.c_int * 17)(*([77] * 17))
    assert L.hpc_rll_r2d2_last_config(None) == EINVAL
    assert list(out) == [77] * 17
    assert L.hpc_rll_r2d2_last_config(out) == 0
    before = list(out)
    if not any(before[i] for i in (0, 7, 12, 14)):             # nothing in this tier launches; a GPU test of the same process may have
        assert before == [0] + [-1] * 6 + [0] + [-1] * 4 + [0, -1] + [0, -1, -1], before
    assert L.hpc_rll_r2d2_forward(P, P, P, P, None, 0, None, 0, P, P, P, P, 9, 4, 2048, 2, 1, 0.997, 1, 1, 0.9, 1.0, None) == EUNSUPPORTED
    assert L.hpc_rll_r2d2_backward(P, P, P, P, 9, 0, 3, 2, 1, None) == 0
    assert L.hpc_rll_r2d2_last_config(out) == 0 and list(out) == before


def _args(n=N, t=T):
    z = torch.zeros
    return z(t, B, n), z(t, B, n), z(t, B, dtype=torch.int64), z(t, B)


def test_cpu_tensors_are_a_runtime_error():
    import hpc_rl_utils
    from hpc_rll.rl_utils.r2d2 import R2D2TD, r2d2_td
    with pytest.raises(RuntimeError, match="GPU"):
        hpc_rl_utils.r2d2_td(*_args())
    with pytest.raises(RuntimeError, match="GPU"):
        r2d2_td(*_args(), done=torch.zeros(T, B, dtype=torch.bool), weight=torch.zeros(B), nstep=2, burnin=1)
    with pytest.raises(RuntimeError, match="GPU"):
        R2D2TD(T, B, N)(*_args())
    with pytest.raises(RuntimeError, match="GPU"):
        hpc_rl_utils.r2d2_td(*_args(), None, None, 0.997, 5, 0, True, True, 0.9, 0.25)   # with a scale


def test_wrong_arguments_are_named():
    from hpc_rll.rl_utils.r2d2 import r2d2_td
    a = _args()
    with pytest.raises(RuntimeError, match=r"q: expected \(T,B,N\)"):
        r2d2_td(torch.zeros(T, B), *a[1:])
    with pytest.raises(RuntimeError, match=r"target_q: shape"):
        r2d2_td(a[0], torch.zeros(T + 1, B, N), *a[2:])
    with pytest.raises(RuntimeError, match=r"action: dtype"):
        r2d2_td(*a[:2], torch.zeros(T, B), a[3])
    with pytest.raises(RuntimeError, match=r"reward: shape"):
        r2d2_td(*a[:3], torch.zeros(T, B, 1))
    with pytest.raises(RuntimeError, match=r"done: dtype"):
        r2d2_td(*a, done=torch.zeros(T, B, dtype=torch.int32))
    with pytest.raises(RuntimeError, match=r"done: shape"):
        r2d2_td(*a, done=torch.zeros(T, dtype=torch.bool))
    with pytest.raises(RuntimeError, match=r"weight: shape"):
        r2d2_td(*a, weight=torch.zeros(T))
    with pytest.raises(RuntimeError, match=r"weight: dtype"):
        r2d2_td(*a, weight=torch.zeros(T, B, dtype=torch.float64))
    with pytest.raises(RuntimeError, match=r"nstep = 0"):
        r2d2_td(*a, nstep=0)
    with pytest.raises(RuntimeError, match=r"burnin = -1"):
        r2d2_td(*a, burnin=-1)
    with pytest.raises(RuntimeError, match=r"not supported .*1 <= N <= 1024"):
        r2d2_td(*_args(1025))


def test_python_signatures():
    from hpc_rll.rl_utils.r2d2 import R2D2TD, r2d2_td
    E = inspect.Parameter.empty
    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]   # noqa: E731
    want = [("q", E), ("target_q", E), ("action", E), ("reward", E), ("done", None), ("weight", None), ("gamma", 0.997),
            ("nstep", 5), ("burnin", 0), ("value_rescale", True), ("double_q", True), ("priority_eta", 0.9)]
    assert sig(r2d2_td) == want
    assert sig(R2D2TD.forward) == [("self", E)] + want
    assert sig(R2D2TD.__init__) == [("self", E), ("T", E), ("B", E), ("N", E), ("sharded", False), ("group", None)]
    m = R2D2TD(T, B, N)
    assert isinstance(m, torch.nn.Module) and (m.T, m.B, m.N, m.sharded, m.group) == (T, B, N, False, None)
    import hpc_rll.rl_utils.r2d2 as mod
    assert "1e-8" in mod.__doc__ and "NaN" in mod.__doc__ and "outside" in mod.__doc__   # the deviation and the limits are documented
    assert "NaN" in r2d2_td.__doc__ and "1e-8" in r2d2_td.__doc__
