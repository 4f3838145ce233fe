"""CPU tier of Retrace (``hpc_rll.rl_utils.retrace``, csrc/retrace.hip): the parts that need no GPU -- the new C entry points
are declared and exported and answer argument errors with status codes before any HIP call (nulls, then sizes, then
alignment, then the N limit, then empty shapes), the extension rejects CPU tensors and names wrong arguments, and the Python
signatures.  Parity and everything that launches is in tests/test_retrace_gpu.py."""
import ctypes
import inspect

import pytest
import torch

FWD, LOSS_FWD, LOSS_BWD, LAST = ("hpc_rll_retrace_forward", "hpc_rll_retrace_loss_forward", "hpc_rll_retrace_loss_backward",
                                 "hpc_rll_retrace_last_config")
EINVAL, EALIGN, EUNSUPPORTED = -1, -2, -3
T, B, N = 5, 3, 4


def test_c_entry_points_declared_and_exported():
    import cabi
    for name, nargs in ((FWD, 14), (LOSS_FWD, 18), (LOSS_BWD, 8), (LAST, 1)):
        assert name in cabi.SIGNATURES, name
        assert hasattr(cabi.lib, name), name
        assert cabi.SIGNATURES[name][0] is ctypes.c_int and len(cabi.SIGNATURES[name][1]) == nargs, name
    assert cabi.SIGNATURES["hpc_rll_retrace_workspace_floats"][0] is ctypes.c_int64
    assert cabi.lib.hpc_rll_abi_version() == 6


def test_workspace_holds_the_documented_layout():
    """delta | qa | c, T*B floats each, then at least one partial sum per workgroup of the narrowest tile (8 columns)."""
    import cabi
    ws = cabi.lib.hpc_rll_retrace_workspace_floats
    for t, b in ((1, 1), (5, 3), (5, 33000), (1024, 60), (256, 16384)):
        assert ws(t, b) >= 3 * t * b + (b + 7) // 8, (t, b)
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
    names = ["q_values", "v_pred", "rewards", "actions", "weights", "ratio", "q_retraces", "ws", "T", "B", "N"]
    call = _caller(cabi.lib.hpc_rll_retrace_forward, names, [P, P, P, P, None, P, P, P, 4, 4, 3], (0.99, 1.0))
    for name in ("q_values", "v_pred", "rewards", "actions", "ratio", "q_retraces", "ws"):
        assert call(**{name: None}) == EINVAL, name
    assert call(T=-1) == EINVAL
    assert call(B=-1) == EINVAL
    assert call(N=0) == EINVAL
    assert call(N=-3) == EINVAL
    assert call(q_values=P + 2) == EALIGN
    assert call(weights=P + 1) == EALIGN
    assert call(actions=P + 4) == EALIGN                       # int64 off 8-byte alignment
    assert call(N=1025) == EUNSUPPORTED
    assert call(N=2048) == EUNSUPPORTED
    assert call(N=2048, weights=P) == EUNSUPPORTED
    assert call(N=2048, ratio=None) == EINVAL                  # nulls come before the N limit
    assert call(N=2048, q_values=P + 2) == EALIGN              # and so does alignment
    assert call(T=0) == 0 and call(B=0) == 0                   # empty: nothing to do, nothing launched
    assert call(T=0, q_values=None, v_pred=None, rewards=None, actions=None, ratio=None, q_retraces=None, ws=None) == 0
    assert call(T=0, N=2048) == EUNSUPPORTED                   # the N limit comes before the empty return
    assert call(T=0, B=-1) == EINVAL


def test_loss_forward_argument_errors_are_status_codes(buf):
    import cabi
    P = ctypes.addressof(buf)
    names = ["q_values", "target_output", "behaviour_output", "action", "reward", "weights", "loss_weight", "loss",
             "q_retraces", "v_pred", "ws", "T", "B", "N"]
    call = _caller(cabi.lib.hpc_rll_retrace_loss_forward, names, [P, P, P, P, P, None, None, P, P, P, P, 4, 4, 3],
                   (0.99, 1.0, 1.0))
    for name in ("q_values", "target_output", "behaviour_output", "action", "reward", "loss", "q_retraces", "v_pred", "ws"):
        assert call(**{name: None}) == EINVAL, name
    assert call(T=-1) == EINVAL
    assert call(B=-1) == EINVAL
    assert call(N=0) == EINVAL
    assert call(target_output=P + 2) == EALIGN
    assert call(loss_weight=P + 1) == EALIGN
    assert call(weights=P + 3) == EALIGN
    assert call(action=P + 4) == EALIGN
    assert call(N=1025) == EUNSUPPORTED
    assert call(N=2048) == EUNSUPPORTED
    assert call(N=2048, weights=P, loss_weight=P) == EUNSUPPORTED
    assert call(N=2048, behaviour_output=None) == EINVAL       # nulls come before the N limit
    assert call(N=2048, ws=None) == EINVAL
    assert call(T=0, loss=None) == EINVAL                      # an empty batch still needs somewhere to write the zero
    assert call(T=0, N=2048) == EUNSUPPORTED


def test_loss_backward_argument_errors_are_status_codes(buf):
    import cabi
    P = ctypes.addressof(buf)
    names = ["g_loss", "action", "ws", "grad_q_values", "T", "B", "N"]
    call = _caller(cabi.lib.hpc_rll_retrace_loss_backward, names, [P, P, P, P, 4, 4, 3], ())
    for name in ("action", "ws", "grad_q_values"):
        assert call(**{name: None}) == EINVAL, name
    assert call(T=-1) == EINVAL
    assert call(B=-1) == EINVAL
    assert call(N=0) == EINVAL
    assert call(grad_q_values=P + 2) == EALIGN
    assert call(g_loss=P + 1) == EALIGN
    assert call(N=1025) == EUNSUPPORTED
    assert call(N=2048) == EUNSUPPORTED
    assert call(N=2048, ws=None) == EINVAL
    assert call(B=0) == 0 and call(T=0) == 0                   # empty: nothing launched
    assert call(B=0, action=None, ws=None, grad_q_values=None) == 0


def test_record_is_empty_and_argument_errors_leave_it_so(buf):
    import cabi
    P = ctypes.addressof(buf)
    L = cabi.lib
    out = (ctypes.c_int * 11)(*([77] * 11))
    assert L.hpc_rll_retrace_last_config(None) == EINVAL
    assert list(out) == [77] * 11
    assert L.hpc_rll_retrace_last_config(out) == 0
    before = list(out)
    if before[0] == 0:                                         # nothing in this tier launches; a GPU test of the same process may have
        assert before == [0] + [-1] * 10, before
    assert L.hpc_rll_retrace_forward(P, P, P, P, None, P, P, P, 0, 4, 3, 0.99, 1.0, None) == 0
    assert L.hpc_rll_retrace_forward(P, P, P, P, None, P, P, P, 4, 4, 2048, 0.99, 1.0, None) == EUNSUPPORTED
    assert L.hpc_rll_retrace_last_config(out) == 0 and list(out) == before
    assert L.hpc_rll_scan_last_config(7, out) == EINVAL and L.hpc_rll_scan_last_config(8, out) == EINVAL   # still private


def _loss_args(n=N):
    z = torch.zeros
    return z(T + 1, B, n), z(T + 1, B, n), z(T, B, n), z(T, B, dtype=torch.int64), z(T, B)


def _args(n=N):
    z = torch.zeros
    return z(T + 1, B, n), z(T + 1, B, 1), z(T, B), z(T, B, dtype=torch.int64), z(T, B), z(T, B, n)


def test_cpu_tensors_are_a_runtime_error():
    import hpc_rl_utils
    from hpc_rll.rl_utils.retrace import Retrace, retrace, retrace_loss
    with pytest.raises(RuntimeError, match="GPU"):
        hpc_rl_utils.retrace(*_args())
    with pytest.raises(RuntimeError, match="GPU"):
        retrace(*_args())
    a = _args()
    with pytest.raises(RuntimeError, match="GPU"):
        retrace(*a[:4], None, a[5], gamma=0.99, lambda_=0.7)
    with pytest.raises(RuntimeError, match="GPU"):
        hpc_rl_utils.retrace_loss(*_loss_args())
    with pytest.raises(RuntimeError, match="GPU"):
        retrace_loss(*_loss_args(), weights=torch.zeros(T, B), loss_weight=torch.zeros(T, B))
    with pytest.raises(RuntimeError, match="GPU"):
        Retrace(T, B, N)(*_loss_args())
    with pytest.raises(RuntimeError, match="GPU"):
        hpc_rl_utils.retrace_loss(*_loss_args(), None, None, 0.99, 1.0, 0.25)   # with a scale


def test_wrong_arguments_are_named():
    from hpc_rll.rl_utils.retrace import retrace, retrace_loss
    a = _loss_args()
    with pytest.raises(RuntimeError, match=r"q_values: expected \(T\+1,B,N\)"):
        retrace_loss(torch.zeros(T, B), *a[1:])
    with pytest.raises(RuntimeError, match=r"target_output: shape"):
        retrace_loss(a[0], torch.zeros(T, B, N), *a[2:])
    with pytest.raises(RuntimeError, match=r"behaviour_output: shape"):
        retrace_loss(*a[:2], torch.zeros(T + 1, B, N), *a[3:])
    with pytest.raises(RuntimeError, match=r"action: dtype"):
        retrace_loss(*a[:3], torch.zeros(T, B), a[4])
    with pytest.raises(RuntimeError, match=r"loss_weight: shape"):
        retrace_loss(*a, loss_weight=torch.zeros(B))
    with pytest.raises(RuntimeError, match=r"weights: dtype"):
        retrace_loss(*a, weights=torch.zeros(T, B, dtype=torch.bool))
    with pytest.raises(RuntimeError, match=r"not supported .*1 <= N <= 1024"):
        retrace_loss(*_loss_args(1025))
    b = _args()
    with pytest.raises(RuntimeError, match=r"v_pred: shape"):
        retrace(b[0], torch.zeros(T + 1, B), *b[2:])
    with pytest.raises(RuntimeError, match=r"ratio: shape"):
        retrace(*b[:5], torch.zeros(T, B))
    with pytest.raises(RuntimeError, match=r"actions: dtype"):
        retrace(*b[:3], torch.zeros(T, B, dtype=torch.int32), *b[4:])
    with pytest.raises(RuntimeError, match=r"not supported .*1 <= N <= 1024"):
        retrace(*_args(2048))


def test_python_signatures():
    from hpc_rll.rl_utils.retrace import Retrace, retrace, retrace_loss
    E = inspect.Parameter.empty
    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]   # noqa: E731
    # DI-engine's compute_q_retraces: names and the gamma default; lambda_ is this library's addition
    assert sig(retrace) == [("q_values", E), ("v_pred", E), ("rewards", E), ("actions", E), ("weights", E), ("ratio", E),
                            ("gamma", 0.9), ("lambda_", 1.0)]
    want = [("q_values", E), ("target_output", E), ("behaviour_output", E), ("action", E), ("reward", E), ("weights", None),
            ("loss_weight", None), ("gamma", 0.9), ("lambda_", 1.0)]
    assert sig(retrace_loss) == want
    assert sig(Retrace.forward) == [("self", E)] + want
    assert sig(Retrace.__init__) == [("self", E), ("T", E), ("B", E), ("N", E), ("sharded", False), ("group", None)]
    m = Retrace(T, B, N)
    assert isinstance(m, torch.nn.Module) and (m.T, m.B, m.N, m.sharded, m.group) == (T, B, N, False, None)
    assert "1e-8" in retrace_loss.__doc__ and "compute_q_retraces" in retrace.__doc__
    import hpc_rll.rl_utils.retrace as mod
    assert "outside" in mod.__doc__ and "qa = 0" in mod.__doc__      # the out-of-range action is documented
