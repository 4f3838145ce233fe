"""CPU tier of ACER's actor loss (``hpc_rll.rl_utils.acer``, csrc/acer.hip): the parts that need no GPU -- the new C entry
points are declared and exported and answer argument errors with status codes before any HIP call (nulls, then sizes, then
alignment, then the N limit, then empty shapes), the extension rejects CPU tensors and names wrong arguments, and the Python
signatures.  Parity and everything that launches is in tests/test_acer_gpu.py."""
import ctypes
import inspect

import pytest
import torch

WS, FWD, BWD, TR, LAST = ("hpc_rll_acer_policy_workspace_floats", "hpc_rll_acer_policy_forward", "hpc_rll_acer_policy_backward",
                          "hpc_rll_acer_trust_region", "hpc_rll_acer_last_config")
EINVAL, EALIGN, EUNSUPPORTED = -1, -2, -3
T, B, N = 5, 3, 4


def test_c_entry_points_declared_and_exported():
    import cabi
    for name, nargs in ((WS, 2), (FWD, 19), (BWD, 8), (TR, 7), (LAST, 1)):
        assert name in cabi.SIGNATURES, name
        assert hasattr(cabi.lib, name), name
        assert len(cabi.SIGNATURES[name][1]) == nargs, name
        assert cabi.SIGNATURES[name][0] is (ctypes.c_int64 if name == WS else ctypes.c_int), name
    P, I, F, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_int64
    assert cabi.SIGNATURES[FWD][1] == [P] * 11 + [I] * 3 + [F] * 4 + [P]
    assert cabi.SIGNATURES[BWD][1] == [P] * 3 + [I] * 4 + [P]
    assert cabi.SIGNATURES[TR][1] == [P] * 3 + [L, I, F, P]
    assert cabi.SIGNATURES[LAST][1] == [P]
    assert cabi.lib.hpc_rll_abi_version() == 6
    hdr = open(cabi.HEADER_PATH).read()
    assert "#define HPC_RLL_ACER_CONFIG_INTS (8)" in hdr


def test_workspace_holds_the_partial_sums():
    """Four sums per workgroup of a forward that never launches more than 512 workgroups, whatever the shape."""
    import cabi
    ws = cabi.lib.hpc_rll_acer_policy_workspace_floats
    for t, b in ((1, 1), (5, 3), (5, 33000), (256, 16384)):
        assert ws(t, b) >= 4 * 512, (t, b)
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


def test_policy_forward_argument_errors_are_status_codes(buf):
    import cabi
    P = ctypes.addressof(buf)
    names = ["target_output", "behaviour_output", "avg_output", "q_values", "q_retraces", "v_pred", "action", "weights", "out4",
             "unit_grad", "ws", "T", "B", "N"]
    call = _caller(cabi.lib.hpc_rll_acer_policy_forward, names, [P, P, None, P, P, P, P, None, P, None, P, 4, 4, 3],
                   (10.0, 0.0, 1.0, 1.0))
    for name in ("target_output", "behaviour_output", "q_values", "q_retraces", "v_pred", "action", "out4", "ws"):
        assert call(**{name: None}) == EINVAL, name
    assert call(T=-1) == EINVAL
    assert call(B=-1) == EINVAL
    assert call(N=0) == EINVAL
    assert call(N=-3) == EINVAL
    assert call(target_output=P + 2) == EALIGN
    assert call(avg_output=P + 1) == EALIGN
    assert call(weights=P + 3) == EALIGN
    assert call(unit_grad=P + 2) == EALIGN
    assert call(action=P + 4) == EALIGN                        # int64 off 8-byte alignment
    assert call(N=1025) == EUNSUPPORTED
    assert call(N=2048) == EUNSUPPORTED
    assert call(N=2048, weights=P, avg_output=P, unit_grad=P) == EUNSUPPORTED
    assert call(N=2048, behaviour_output=None) == EINVAL       # nulls come before the N limit
    assert call(N=2048, q_values=P + 2) == EALIGN              # and so does alignment
    assert call(T=0, out4=None) == EINVAL                      # an empty batch still needs somewhere to write the zeros
    assert call(T=0, N=2048) == EUNSUPPORTED                   # the N limit comes before the empty return
    assert call(T=0, B=-1) == EINVAL


def test_trust_region_argument_errors_are_status_codes(buf):
    import cabi
    P = ctypes.addressof(buf)
    names = ["actor_gradient", "avg_logit", "out", "rows", "N"]
    call = _caller(cabi.lib.hpc_rll_acer_trust_region, names, [P, P, P, 4, 3], (1.0,))
    for name in ("actor_gradient", "avg_logit", "out"):
        assert call(**{name: None}) == EINVAL, name
    assert call(rows=-1) == EINVAL
    assert call(N=0) == EINVAL
    assert call(avg_logit=P + 2) == EALIGN
    assert call(out=P + 1) == EALIGN
    assert call(N=1025) == EUNSUPPORTED
    assert call(N=2048, out=None) == EINVAL
    assert call(N=2048, out=P + 2) == EALIGN
    assert call(rows=0) == 0                                   # empty: nothing launched
    assert call(rows=0, actor_gradient=None, avg_logit=None, out=None) == 0
    assert call(rows=0, N=2048) == EUNSUPPORTED


def test_backward_argument_errors_are_status_codes(buf):
    import cabi
    P = ctypes.addressof(buf)
    names = ["g_loss", "unit_grad", "grad_target_output", "T", "B", "N", "target_rows"]
    call = _caller(cabi.lib.hpc_rll_acer_policy_backward, names, [P, P, P, 4, 4, 3, 4], ())
    for name in ("g_loss", "unit_grad", "grad_target_output"):
        assert call(**{name: None}) == EINVAL, name
    assert call(T=-1, target_rows=-1) == EINVAL
    assert call(B=-1) == EINVAL
    assert call(N=0) == EINVAL
    assert call(target_rows=3) == EINVAL and call(target_rows=6) == EINVAL      # T or T+1
    assert call(grad_target_output=P + 2) == EALIGN
    assert call(g_loss=P + 1) == EALIGN
    assert call(N=1025) == EUNSUPPORTED
    assert call(N=2048, target_rows=5) == EUNSUPPORTED
    assert call(N=2048, unit_grad=None) == EINVAL
    assert call(B=0) == 0 and call(T=0, target_rows=1) == 0    # empty: nothing launched
    assert call(B=0, g_loss=None, unit_grad=None, grad_target_output=None) == 0


def test_record_is_empty_and_argument_errors_leave_it_so(buf):
    import cabi
    P = ctypes.addressof(buf)
    L = cabi.lib
    out = (ctypes.c_int * 8)(*([77] * 8))
    assert L.hpc_rll_acer_last_config(None) == EINVAL
    assert list(out) == [77] * 8
    assert L.hpc_rll_acer_last_config(out) == 0
    before = list(out)
    if before[0] == 0:                                         # nothing in this tier launches; a GPU test of the same process may have
        assert before == [0] + [-1] * 7, before
    assert L.hpc_rll_acer_trust_region(P, P, P, 0, 3, 1.0, None) == 0
    assert L.hpc_rll_acer_trust_region(P, P, P, 4, 2048, 1.0, None) == EUNSUPPORTED
    assert L.hpc_rll_acer_policy_forward(P, P, None, P, P, P, P, None, P, None, P, 4, 4, 2048, 10.0, 0.0, 1.0, 1.0,
                                         None) == EUNSUPPORTED
    assert L.hpc_rll_acer_last_config(out) == 0 and list(out) == before


def _args(n=N, rows=T + 1):
    z = torch.zeros
    return z(rows, B, n), z(T, B, n), z(rows, B, n), z(rows, B), z(rows, B), z(T, B, dtype=torch.int64)


def test_cpu_tensors_are_a_runtime_error():
    import hpc_rl_utils
    from hpc_rll.rl_utils.acer import ACERPolicy, acer_policy_loss, acer_trust_region_update
    for rows in (T, T + 1):
        with pytest.raises(RuntimeError, match="GPU"):
            hpc_rl_utils.acer_policy_loss(*_args(rows=rows))
        with pytest.raises(RuntimeError, match="GPU"):
            acer_policy_loss(*_args(rows=rows), weights=torch.zeros(T, B), avg_output=torch.zeros(T, B, N))
    with pytest.raises(RuntimeError, match="GPU"):
        ACERPolicy(T, B, N)(*_args())
    with pytest.raises(RuntimeError, match="GPU"):
        hpc_rl_utils.acer_policy_loss(*_args(), None, None, 10.0, 0.0, 1.0, 0.25)   # with a scale
    with pytest.raises(RuntimeError, match="GPU"):
        acer_trust_region_update([torch.zeros(T, B, N)], None, torch.zeros(T, B, N), 1.0)
    with pytest.raises(RuntimeError, match="GPU"):
        hpc_rl_utils.acer_trust_region_update(torch.zeros(B, N), torch.zeros(B, N), 1.0)


def test_wrong_arguments_are_named():
    from hpc_rll.rl_utils.acer import acer_policy_loss, acer_trust_region_update
    a = _args()
    with pytest.raises(RuntimeError, match=r"target_output: expected \(T,B,N\) or \(T\+1,B,N\)"):
        acer_policy_loss(torch.zeros(T, B), *a[1:])
    with pytest.raises(RuntimeError, match=r"target_output: shape"):
        acer_policy_loss(torch.zeros(T + 2, B, N), *a[1:])
    with pytest.raises(RuntimeError, match=r"behaviour_output: shape"):
        acer_policy_loss(a[0], torch.zeros(T + 1, B, N), *a[2:])
    with pytest.raises(RuntimeError, match=r"q_values: shape"):
        acer_policy_loss(*a[:2], torch.zeros(T, B, N + 1), *a[3:])
    with pytest.raises(RuntimeError, match=r"q_retraces: shape"):
        acer_policy_loss(*a[:3], torch.zeros(T + 1, B, 1), *a[4:])
    with pytest.raises(RuntimeError, match=r"v_pred: shape"):
        acer_policy_loss(*a[:4], torch.zeros(T - 1, B), a[5])
    with pytest.raises(RuntimeError, match=r"action: dtype"):
        acer_policy_loss(*a[:5], torch.zeros(T, B))
    with pytest.raises(RuntimeError, match=r"action: expected \(T,B\)"):
        acer_policy_loss(*a[:5], torch.zeros(T, dtype=torch.int64))
    with pytest.raises(RuntimeError, match=r"weights: shape"):
        acer_policy_loss(*a, weights=torch.zeros(B))
    with pytest.raises(RuntimeError, match=r"avg_output: shape"):
        acer_policy_loss(*a, avg_output=torch.zeros(T + 1, B, N))
    with pytest.raises(RuntimeError, match=r"avg_output: dtype"):
        acer_policy_loss(*a, avg_output=torch.zeros(T, B, N, dtype=torch.float64))
    with pytest.raises(RuntimeError, match=r"not supported .*1 <= N <= 1024"):
        acer_policy_loss(*_args(1025))
    with pytest.raises(RuntimeError, match=r"avg_logit: shape"):
        acer_trust_region_update([torch.zeros(T, B, N)], None, torch.zeros(T, B, N + 1), 1.0)
    with pytest.raises(RuntimeError, match=r"actor_gradients: dtype"):
        acer_trust_region_update([torch.zeros(T, B, N, dtype=torch.float64)], None, torch.zeros(T, B, N), 1.0)
    with pytest.raises(RuntimeError, match=r"not supported .*1 <= N <= 1024"):
        acer_trust_region_update([torch.zeros(B, 2048)], None, torch.zeros(B, 2048), 1.0)


def test_python_signatures():
    from hpc_rll.rl_utils.acer import ACERPolicy, acer_policy_loss, acer_trust_region_update
    E = inspect.Parameter.empty
    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]   # noqa: E731
    want = [("target_output", E), ("behaviour_output", E), ("q_values", E), ("q_retraces", E), ("v_pred", E), ("action", E),
            ("weights", None), ("avg_output", None), ("c_clip_ratio", 10.0), ("entropy_weight", 0.0),
            ("trust_region_value", 1.0)]
    assert sig(acer_policy_loss) == want
    assert sig(ACERPolicy.forward) == [("self", E)] + want
    assert sig(ACERPolicy.__init__) == [("self", E), ("T", E), ("B", E), ("N", E), ("sharded", False), ("group", None)]
    # DI-engine's acer_trust_region_update
    assert sig(acer_trust_region_update) == [("actor_gradients", E), ("target_logit", E), ("avg_logit", E),
                                             ("trust_region_value", E)]
    m = ACERPolicy(T, B, N)
    assert isinstance(m, torch.nn.Module) and (m.T, m.B, m.N, m.sharded, m.group) == (T, B, N, False, None)
    import hpc_rll.rl_utils.acer as mod
    assert "1e-8" in mod.__doc__ and "per-sample" in mod.__doc__     # the two deviations from DI-engine are documented
    assert "outside" in mod.__doc__ and "-inf" in mod.__doc__ and "N = 1" in mod.__doc__
