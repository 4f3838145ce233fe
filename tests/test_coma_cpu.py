"""CPU tier of COMA (``hpc_rll.rl_utils.coma``, csrc/coma.hip): the parts that need no GPU -- the new C entry points are
declared and exported and answer argument errors with status codes before any HIP call (nulls, then sizes, then alignment,
then the N limit, then empty shapes), the workspace size, the extension rejects CPU tensors and names wrong arguments, and the
Python signatures and namedtuples.  Parity and everything that launches is in tests/test_coma_gpu.py."""
import ctypes
import inspect

import pytest
import torch

WS, FWD, BWD, LAST = "hpc_rll_coma_workspace_floats", "hpc_rll_coma_forward", "hpc_rll_coma_backward", "hpc_rll_coma_last_config"
EINVAL, EALIGN, EUNSUPPORTED = -1, -2, -3
U8, F32 = 0, 1
NREC = 25
T, B, A, N = 5, 3, 2, 4


def test_c_entry_points_declared_and_exported():
    import cabi
    for name, nargs in ((WS, 3), (FWD, 19), (BWD, 15), (LAST, 1)):
        assert name in cabi.SIGNATURES, name
        assert hasattr(cabi.lib, name), name
        assert len(cabi.SIGNATURES[name][1]) == nargs, name
        assert cabi.SIGNATURES[name][0] is (ctypes.c_int64 if name == WS else ctypes.c_int), name
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert cabi.SIGNATURES[WS][1] == [I] * 3
    assert cabi.SIGNATURES[FWD][1] == [P] * 7 + [I] + [P] * 2 + [I] * 4 + [F] * 4 + [P]
    assert cabi.SIGNATURES[BWD][1] == [P] * 9 + [I] * 4 + [F] + [P]
    assert cabi.SIGNATURES[LAST][1] == [P]
    assert cabi.lib.hpc_rll_abi_version() == 6
    hdr = open(cabi.HEADER_PATH).read()
    assert "#define HPC_RLL_COMA_CONFIG_INTS (25)" in hdr
    assert "#define HPC_RLL_SCAN_OPS (7)" in hdr and "#define HPC_RLL_SCAN_CONFIG_INTS (11)" in hdr


def test_the_scan_op_list_did_not_grow():
    """COMA's scan record is private: hpc_rll_scan_last_config still accepts ops 0..6 only."""
    import cabi
    out = (ctypes.c_int * 11)()
    assert cabi.lib.hpc_rll_scan_last_config(6, out) == 0
    for op in (7, 8, 9, 10):
        assert cabi.lib.hpc_rll_scan_last_config(op, out) == EINVAL, op


def test_workspace_is_monotone_and_rejects_negatives():
    """Six floats per row, the heads' three sums per workgroup of at most 512, one sum per workgroup of the scan."""
    import cabi
    ws = cabi.lib.hpc_rll_coma_workspace_floats
    for t, b, a in ((1, 1, 1), (5, 3, 2), (6, 11000, 3), (256, 2048, 8)):
        n = ws(t, b, a)
        assert n >= 6 * t * b * a + 3 * 512 + (b * a + 7) // 8, (t, b, a)
        assert ws(t + 1, b, a) > n and ws(t, b + 1, a) > n and ws(t, b, a + 1) > n, (t, b, a)
    assert ws(0, 7, 2) >= 0 and ws(7, 0, 2) >= 0 and ws(7, 2, 0) >= 0
    assert ws(0, 7, 2) <= ws(1, 7, 2)
    assert ws(-1, 4, 2) == EINVAL and ws(4, -1, 2) == EINVAL and ws(4, 2, -1) == EINVAL
    assert ws(1, 1 << 20, 1 << 12) == EINVAL                     # B*A past an int
    assert ws(1 << 20, 1 << 20, 1 << 10) > 1 << 50               # 64-bit


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
    names = ["logit", "action", "q_value", "target_q_value", "reward", "weight", "done", "mask_dtype", "loss", "ws", "T", "B",
             "A", "N"]
    call = _caller(cabi.lib.hpc_rll_coma_forward, names, [P, P, P, P, P, None, None, U8, P, P, 4, 4, 2, 3],
                   (0.99, 0.8, 1.0, 1.0))
    for name in ("logit", "action", "q_value", "target_q_value", "reward", "loss", "ws"):
        assert call(**{name: None}) == EINVAL, name
    assert call(T=-1) == EINVAL
    assert call(B=-1) == EINVAL
    assert call(A=-1) == EINVAL
    assert call(N=0) == EINVAL
    assert call(N=-3) == EINVAL
    assert call(B=1 << 20, A=1 << 12) == EINVAL                  # B*A past an int
    assert call(mask_dtype=2) == EINVAL and call(mask_dtype=-1) == EINVAL
    assert call(logit=P + 2) == EALIGN
    assert call(q_value=P + 1) == EALIGN
    assert call(target_q_value=P + 3) == EALIGN
    assert call(reward=P + 2) == EALIGN
    assert call(weight=P + 2) == EALIGN
    assert call(action=P + 4) == EALIGN                          # int64 off 8-byte alignment
    assert call(done=P + 1, mask_dtype=F32) == EALIGN            # a float mask off 4 bytes
    assert call(done=P + 1, mask_dtype=U8, N=2048) == EUNSUPPORTED   # a byte mask has no alignment
    assert call(loss=P + 2) == EALIGN and call(ws=P + 1) == EALIGN
    assert call(N=1025) == EUNSUPPORTED
    assert call(N=2048, weight=P, done=P, mask_dtype=F32) == EUNSUPPORTED
    assert call(N=2048, q_value=None) == EINVAL                  # nulls come before the N limit
    assert call(N=2048, logit=P + 2) == EALIGN                   # and so does alignment
    assert call(N=2048, T=-1) == EINVAL
    assert call(T=0, loss=None) == EINVAL                        # an empty batch still needs somewhere to write the zeros
    for empty in (dict(T=0), dict(B=0), dict(A=0)):
        assert call(N=2048, **empty) == EUNSUPPORTED             # the N limit comes before the empty return
        assert call(N=0, **empty) == EINVAL
    assert call(T=0, B=-1) == EINVAL


def test_backward_argument_errors_are_status_codes(buf):
    import cabi
    P = ctypes.addressof(buf)
    names = ["g_policy", "g_q", "g_entropy", "logit", "action", "weight", "ws", "grad_logit", "grad_q_value", "T", "B", "A", "N"]
    call = _caller(cabi.lib.hpc_rll_coma_backward, names, [P, P, P, P, P, None, P, P, P, 4, 4, 2, 3], (1.0,))
    for name in ("logit", "action", "ws"):
        assert call(**{name: None}) == EINVAL, name
    assert call(T=-1) == EINVAL and call(B=-1) == EINVAL and call(A=-1) == EINVAL
    assert call(N=0) == EINVAL
    assert call(B=1 << 20, A=1 << 12) == EINVAL
    assert call(grad_logit=P + 2) == EALIGN
    assert call(grad_q_value=P + 1) == EALIGN
    assert call(g_policy=P + 1) == EALIGN and call(g_q=P + 2) == EALIGN and call(g_entropy=P + 3) == EALIGN
    assert call(weight=P + 2) == EALIGN
    assert call(action=P + 4) == EALIGN
    assert call(N=1025) == EUNSUPPORTED
    assert call(N=2048, ws=None) == EINVAL
    assert call(N=2048, logit=P + 2) == EALIGN
    # nothing to do: empty shapes, or neither output wanted (logit and the rest may then be absent)
    assert call(T=0) == 0 and call(B=0) == 0 and call(A=0) == 0
    assert call(grad_logit=None, grad_q_value=None) == 0
    assert call(grad_logit=None, grad_q_value=None, logit=None, action=None, ws=None) == 0
    assert call(grad_logit=None, grad_q_value=None, N=2048) == EUNSUPPORTED
    assert call(T=0, N=2048) == EUNSUPPORTED


def test_record_is_empty_and_argument_errors_leave_it_so(buf):
    import cabi
    P = ctypes.addressof(buf)
    L = cabi.lib
    out = (ctypes.c_int * NREC)(*([77] * NREC))
    assert L.hpc_rll_coma_last_config(None) == EINVAL
    assert list(out) == [77] * NREC
    assert L.hpc_rll_coma_last_config(out) == 0
    before = list(out)
    for lo, n in ((0, 11), (11, 7), (18, 7)):                    # the scan, the heads, the backward
        if before[lo] == 0:                                      # nothing in this tier launches; a GPU test of the same process may have
            assert before[lo:lo + n] == [0] + [-1] * (n - 1), (lo, before)
    assert L.hpc_rll_coma_forward(P, P, P, P, P, None, None, U8, P, P, 4, 4, 2, 2048, 0.99, 0.8, 1.0, 1.0, None) == EUNSUPPORTED
    assert L.hpc_rll_coma_backward(P, P, P, P, P, None, P, None, None, 4, 4, 2, 3, 1.0, None) == 0
    assert L.hpc_rll_coma_backward(P, P, P, P, P, None, P, P, P, 4, 4, 2, 2048, 1.0, None) == EUNSUPPORTED
    assert L.hpc_rll_coma_last_config(out) == 0 and list(out) == before


def _args(n=N, t=T):
    z = torch.zeros
    return [z(t, B, A, n), z(t, B, A, dtype=torch.int64), z(t, B, A, n), z(t, B, A, n), z(t, B)]


def test_cpu_tensors_are_a_runtime_error():
    import hpc_rl_utils
    from hpc_rll.rl_utils.coma import COMA, coma, coma_data, coma_error
    with pytest.raises(RuntimeError, match="GPU"):
        hpc_rl_utils.coma(*_args())
    with pytest.raises(RuntimeError, match="GPU"):
        coma(*_args(), weight=torch.zeros(T, B, A), done=torch.zeros(T, B, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="GPU"):
        coma(*_args(), done=torch.zeros(T, B))
    with pytest.raises(RuntimeError, match="GPU"):
        coma_error(coma_data(*_args(), None), 0.99, 0.8)
    with pytest.raises(RuntimeError, match="GPU"):
        COMA(T, B, A, N)(*_args())
    with pytest.raises(RuntimeError, match="GPU"):
        hpc_rl_utils.coma(*_args(), None, None, 0.99, 0.8, (0.25, 0.5))   # with the two scales


def test_wrong_arguments_are_named():
    from hpc_rll.rl_utils.coma import coma
    a = _args()
    with pytest.raises(RuntimeError, match=r"logit: expected \(T,B,A,N\)"):
        coma(torch.zeros(T, B, N), *a[1:])
    with pytest.raises(RuntimeError, match=r"logit: dtype"):
        coma(a[0].double(), *a[1:])
    with pytest.raises(RuntimeError, match=r"action: dtype"):
        coma(a[0], torch.zeros(T, B, A), *a[2:])
    with pytest.raises(RuntimeError, match=r"action: shape"):
        coma(a[0], torch.zeros(T, B, dtype=torch.int64), *a[2:])
    with pytest.raises(RuntimeError, match=r"q_value: shape"):
        coma(*a[:2], torch.zeros(T, B, A, N + 1), *a[3:])
    with pytest.raises(RuntimeError, match=r"target_q_value: shape"):
        coma(*a[:3], torch.zeros(T + 1, B, A, N), a[4])
    with pytest.raises(RuntimeError, match=r"target_q_value: dtype"):
        coma(*a[:3], a[3].half(), a[4])
    with pytest.raises(RuntimeError, match=r"reward: shape"):
        coma(*a[:4], torch.zeros(T, B, A))
    with pytest.raises(RuntimeError, match=r"weight: shape"):
        coma(*a, weight=torch.zeros(T, B))
    with pytest.raises(RuntimeError, match=r"weight: dtype"):
        coma(*a, weight=torch.zeros(T, B, A, dtype=torch.float64))
    with pytest.raises(RuntimeError, match=r"done: shape"):
        coma(*a, done=torch.zeros(T, B, A, dtype=torch.bool))
    with pytest.raises(RuntimeError, match=r"done: dtype .* expected bool, uint8 or float32"):
        coma(*a, done=torch.zeros(T, B, dtype=torch.int64))
    with pytest.raises(RuntimeError, match=r"not supported .*1 <= N <= 1024"):
        coma(*_args(1025, 1))


def test_python_signatures_and_namedtuples():
    from hpc_rll.rl_utils.coma import COMA, coma, coma_data, coma_error, coma_loss
    E = inspect.Parameter.empty
    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]   # noqa: E731
    want = [("logit", E), ("action", E), ("q_value", E), ("target_q_value", E), ("reward", E), ("weight", None), ("done", None),
            ("gamma", 0.99), ("lambda_", 0.8)]
    assert sig(coma) == want
    assert sig(COMA.forward) == [("self", E)] + want
    assert sig(COMA.__init__) == [("self", E), ("T", E), ("B", E), ("A", E), ("N", E), ("sharded", False), ("group", None)]
    # DI-engine's names and field order
    assert sig(coma_error) == [("data", E), ("gamma", E), ("lambda_", E)]
    assert coma_data._fields == ("logit", "action", "q_value", "target_q_value", "reward", "weight")
    assert coma_loss._fields == ("policy_loss", "q_value_loss", "entropy_loss")
    m = COMA(T, B, A, N)
    assert isinstance(m, torch.nn.Module) and (m.T, m.B, m.A, m.N, m.sharded, m.group) == (T, B, A, N, False, None)
    import hpc_rll.rl_utils.coma as mod
    for word in ("-inf", "outside", "T = 1", "N = 1", "weight=None", "done=None", "no 0.5", "1 - done"):
        assert word in mod.__doc__, word
