"""CPU tier of VTraceContinuous (V-trace for diagonal-Gaussian policies): the parts that need no GPU -- the three new C entry
points are declared and exported and answer argument errors with status codes before any HIP call, the extension rejects
CPU tensors, and the Python signatures.  Parity and everything that launches is in tests/test_vtrace_continuous_gpu.py."""
import ctypes
import inspect

import pytest
import torch

HEAD, FWD, BWD = "hpc_rll_gaussian_forward", "hpc_rll_vtrace_continuous_forward", "hpc_rll_vtrace_continuous_backward"
EINVAL, EALIGN, EUNSUPPORTED = -1, -2, -3
T, B, A = 5, 3, 4


def test_c_entry_points_declared_and_exported():
    import cabi
    for name, nargs in ((HEAD, 11), (FWD, 24), (BWD, 14)):
        assert name in cabi.SIGNATURES, name
        assert hasattr(cabi.lib, name), name
        assert cabi.SIGNATURES[name][0] is ctypes.c_int and len(cabi.SIGNATURES[name][1]) == nargs, name
    assert cabi.lib.hpc_rll_abi_version() == 6


@pytest.fixture(scope="module")
def buf():
    """A small host buffer as a stand-in for device memory: the calls below return before anything reads it."""
    b = (ctypes.c_float * 64)()
    assert ctypes.addressof(b) % 4 == 0
    return b


def test_head_argument_errors_are_status_codes(buf):
    import cabi
    P = ctypes.addressof(buf)
    head = cabi.lib.hpc_rll_gaussian_forward

    def call(rows=4, A=4, **repl):
        a = dict(mu=P, sigma=P, mu_b=P, sigma_b=P, action=P, logp=P, entropy=P, logp_b=P)
        a.update(repl)
        return head(*a.values(), rows, A, None)
    for name in ("mu", "sigma", "mu_b", "sigma_b", "action", "logp", "entropy", "logp_b"):   # all eight are required
        assert call(**{name: None}) == EINVAL, name
    assert call(rows=-1) == EINVAL
    assert call(A=0) == EINVAL
    assert call(A=-2) == EINVAL
    assert call(mu=P + 2) == EALIGN
    assert call(logp_b=P + 1) == EALIGN
    assert call(A=2048) == EUNSUPPORTED                       # pointers are there: the size is what is wrong
    assert call(A=1025) == EUNSUPPORTED
    assert call(A=2048, sigma=None) == EINVAL                 # nulls come before the A limit
    assert call(rows=0) == 0                                  # nothing to do, nothing launched


def test_forward_argument_errors_are_status_codes(buf):
    import cabi
    P = ctypes.addressof(buf)
    fwd = cabi.lib.hpc_rll_vtrace_continuous_forward
    names = ["mu_t", "sigma_t", "mu_b", "sigma_b", "action", "value", "next_value", "reward", "weight", "done", "traj_flag",
             "dt", "losses", "ws", "T", "B", "A"]
    base = [P, P, P, P, P, P, None, P, None, None, None, 0, P, P, 4, 4, 3]

    def call(**kw):
        a = list(base)
        for k, v in kw.items():
            a[names.index(k)] = v
        return fwd(*a, 0.99, 0.95, 1.0, 1.0, 1.0, 1.0, None)
    for name in ("mu_t", "sigma_t", "mu_b", "sigma_b", "action", "value", "reward", "losses", "ws"):
        assert call(**{name: None}) == EINVAL, name
    assert call(T=-1) == EINVAL
    assert call(B=-1) == EINVAL
    assert call(A=0) == EINVAL
    assert call(A=-5) == EINVAL
    assert call(dt=2) == EINVAL
    assert call(dt=-1) == EINVAL
    assert call(mu_t=P + 2) == EALIGN
    assert call(weight=P + 1) == EALIGN
    assert call(dt=1, done=P + 2) == EALIGN                   # a float32 mask off 4-byte alignment
    assert call(A=2048) == EUNSUPPORTED
    assert call(A=2048, dt=1, done=P, traj_flag=P, next_value=P, weight=P) == EUNSUPPORTED
    assert call(A=2048, mu_b=None) == EINVAL                  # nulls come before the A limit
    assert call(A=2048, ws=None) == EINVAL
    assert call(T=0, losses=None) == EINVAL                   # an empty batch still needs somewhere to write zeros


def test_backward_argument_errors_are_status_codes(buf):
    import cabi
    P = ctypes.addressof(buf)
    bwd = cabi.lib.hpc_rll_vtrace_continuous_backward
    names = ["g_pg", "g_value", "g_ent", "mu_t", "sigma_t", "action", "ws", "grad_mu", "grad_sigma", "grad_value", "T", "B", "A"]
    base = [P, P, P, P, P, P, P, P, P, P, 4, 4, 3]

    def call(**kw):
        a = list(base)
        for k, v in kw.items():
            a[names.index(k)] = v
        return bwd(*a, None)
    for name in ("mu_t", "sigma_t", "action", "ws", "g_value"):
        assert call(**{name: None}) == EINVAL, name
    assert call(T=-1) == EINVAL
    assert call(B=-1) == EINVAL
    assert call(A=0) == EINVAL
    assert call(grad_sigma=P + 2) == EALIGN
    assert call(A=2048) == EUNSUPPORTED
    assert call(A=2048, ws=None) == EINVAL
    assert call(grad_mu=None, grad_sigma=None, grad_value=None) == 0                         # no gradient wanted: nothing to do
    assert call(grad_mu=None, grad_sigma=None, grad_value=None, mu_t=None, ws=None) == 0
    assert call(T=0, grad_value=None) == 0                                                   # no rows: nothing launched


def _args(stacked=True, A=A):
    z = torch.zeros
    return (z(T, B, A), z(T, B, A) + 1, z(T, B, A), z(T, B, A) + 1, z(T, B, A), z(T + 1 if stacked else T, B), z(T, B))


@pytest.mark.parametrize("kw", [{}, {"done": torch.zeros(T, B, dtype=torch.bool)},
                                {"done": torch.zeros(T, B), "traj_flag": torch.zeros(T, B, dtype=torch.uint8)}])
def test_cpu_tensors_are_a_runtime_error(kw):
    import hpc_rl_utils
    from hpc_rll.rl_utils.vtrace import VTraceContinuous, vtrace_continuous
    with pytest.raises(RuntimeError, match="GPU"):
        hpc_rl_utils.vtrace_continuous(*_args(), **kw)
    with pytest.raises(RuntimeError, match="GPU"):
        vtrace_continuous(*_args(), **kw)
    with pytest.raises(RuntimeError, match="GPU"):
        vtrace_continuous(*_args(False), next_value=torch.zeros(T, B), weight=torch.zeros(T, B), **kw)
    with pytest.raises(RuntimeError, match="GPU"):
        VTraceContinuous(T, B, A)(*_args(), **kw)
    with pytest.raises(RuntimeError, match="GPU"):
        hpc_rl_utils.vtrace_continuous(*_args(), None, None, None, None, 0.99, 0.95, 1.0, 1.0, 1.0, 0.25)   # with a scale


def test_wrong_arguments_are_named():
    from hpc_rll.rl_utils.vtrace import vtrace_continuous
    a = _args()
    with pytest.raises(RuntimeError, match=r"sigma_behaviour: shape"):
        vtrace_continuous(*a[:3], torch.ones(T, B, A + 1), *a[4:])
    with pytest.raises(RuntimeError, match=r"action: dtype"):
        vtrace_continuous(*a[:4], torch.zeros(T, B, A, dtype=torch.int64), *a[5:])
    with pytest.raises(RuntimeError, match=r"mu_target: expected \(T,B,A\)"):
        vtrace_continuous(torch.zeros(T, B), *a[1:])
    with pytest.raises(RuntimeError, match=r"value: shape .*\(T\+1,B\)"):
        vtrace_continuous(*a[:5], torch.zeros(T, B), a[6])
    with pytest.raises(RuntimeError, match=r"weight: shape"):
        vtrace_continuous(*a, weight=torch.zeros(B))
    with pytest.raises(RuntimeError, match=r"done: dtype .* expected bool, uint8 or float32"):
        vtrace_continuous(*a, done=torch.zeros(T, B, dtype=torch.int64))
    with pytest.raises(RuntimeError, match=r"not supported .*1 <= A <= 1024"):
        vtrace_continuous(*_args(A=1025))


def test_python_signatures():
    from hpc_rll.rl_utils.vtrace import MaskedVTrace, VTrace, VTraceContinuous, hpc_vtrace_loss, masked_vtrace, vtrace_continuous
    E = inspect.Parameter.empty
    want = [("mu_target", E), ("sigma_target", E), ("mu_behaviour", E), ("sigma_behaviour", E), ("action", E), ("value", E),
            ("reward", E), ("done", None), ("weight", None), ("gamma", 0.99), ("lambda_", 0.95), ("rho_clip_ratio", 1.0),
            ("c_clip_ratio", 1.0), ("rho_pg_clip_ratio", 1.0), ("next_value", None), ("traj_flag", None)]
    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]   # noqa: E731
    assert sig(vtrace_continuous) == want
    assert sig(VTraceContinuous.forward) == [("self", E)] + want
    assert sig(VTraceContinuous.__init__) == [("self", E), ("T", E), ("B", E), ("A", E), ("sharded", False), ("group", None)]
    m = VTraceContinuous(T, B, A)
    assert isinstance(m, torch.nn.Module) and (m.T, m.B, m.A, m.sharded, m.group) == (T, B, A, False, None)
    assert "sigma > 0" in vtrace_continuous.__doc__ and "traj_flag" in vtrace_continuous.__doc__
    assert hpc_vtrace_loss._fields == ("policy_loss", "value_loss", "entropy_loss")
    # the categorical ops are untouched
    cat = [("target_output", E), ("behaviour_output", E), ("action", E), ("value", E), ("reward", E)]
    tail = [("gamma", 0.99), ("lambda_", 0.95), ("rho_clip_ratio", 1.0), ("c_clip_ratio", 1.0), ("rho_pg_clip_ratio", 1.0)]
    masked = cat + [("done", None), ("weight", None)] + tail + [("next_value", None), ("traj_flag", None)]
    assert sig(VTrace.forward) == [("self", E)] + cat + [("weight", None)] + tail
    assert sig(masked_vtrace) == masked and sig(MaskedVTrace.forward) == [("self", E)] + masked
    init = [("self", E), ("T", E), ("B", E), ("N", E), ("sharded", False), ("group", None)]
    assert sig(VTrace.__init__) == init and sig(MaskedVTrace.__init__) == init
