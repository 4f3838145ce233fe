"""CPU tier of the episode-aware TD(lambda) and V-trace (``masked_td_lambda`` / ``MaskedTDLambda``, ``masked_vtrace`` /
``MaskedVTrace``, ``hpc_rl_utils.td_lambda_masked`` / ``vtrace_masked``): the API exists with its signatures, host
tensors are rejected loudly (no CPU path), wrong mask dtypes and mismatched shapes are named, and the two C entry points
are declared in the header, exported by the library and answer argument errors with status codes."""
import ctypes
import inspect

import pytest
import torch


def Z(*s, dtype=torch.float32):
    return torch.zeros(*s, dtype=dtype)


T, B, N = 5, 3, 4
TD_PARAMS = ["value", "reward", "done", "weight", "gamma", "lambda_", "next_value", "traj_flag"]
VT_PARAMS = ["target_output", "behaviour_output", "action", "value", "reward", "done", "weight", "gamma", "lambda_",
             "rho_clip_ratio", "c_clip_ratio", "rho_pg_clip_ratio", "next_value", "traj_flag"]


def _vt_args(stacked=True):
    return (Z(T, B, N), Z(T, B, N), Z(T, B, dtype=torch.long), Z(T + 1 if stacked else T, B), Z(T, B))


def test_api_exists():
    import hpc_rl_utils
    from hpc_rll.rl_utils.td import MaskedTDLambda, TDLambda, masked_td_lambda
    from hpc_rll.rl_utils.vtrace import MaskedVTrace, VTrace, masked_vtrace
    assert callable(hpc_rl_utils.td_lambda_masked) and callable(hpc_rl_utils.vtrace_masked)
    assert list(inspect.signature(masked_td_lambda).parameters) == TD_PARAMS
    assert list(inspect.signature(MaskedTDLambda.forward).parameters) == ["self"] + TD_PARAMS
    assert list(inspect.signature(masked_vtrace).parameters) == VT_PARAMS
    assert list(inspect.signature(MaskedVTrace.forward).parameters) == ["self"] + VT_PARAMS
    sig = inspect.signature(masked_td_lambda).parameters
    assert (sig["gamma"].default, sig["lambda_"].default) == (0.9, 0.8)
    sig = inspect.signature(masked_vtrace).parameters
    assert (sig["gamma"].default, sig["lambda_"].default, sig["rho_clip_ratio"].default) == (0.99, 0.95, 1.0)
    m = MaskedTDLambda(T, B)
    assert isinstance(m, torch.nn.Module) and (m.T, m.B, m.sharded) == (T, B, False)
    v = MaskedVTrace(T, B, N, sharded=False)
    assert isinstance(v, torch.nn.Module) and (v.T, v.B, v.N) == (T, B, N)
    assert "traj_flag" in masked_td_lambda.__doc__ and "TDLambda" in masked_td_lambda.__doc__
    assert "traj_flag" in masked_vtrace.__doc__ and "VTrace" in masked_vtrace.__doc__
    assert MaskedTDLambda is not TDLambda and MaskedVTrace is not VTrace


@pytest.mark.parametrize("kw", [{}, {"done": Z(T, B, dtype=torch.bool)}, {"done": Z(T, B, dtype=torch.uint8)},
                                {"done": Z(T, B), "traj_flag": Z(T, B, dtype=torch.bool)}])
def test_host_tensors_are_rejected(kw):
    from hpc_rll.rl_utils.td import MaskedTDLambda, masked_td_lambda
    from hpc_rll.rl_utils.vtrace import MaskedVTrace, masked_vtrace
    with pytest.raises(RuntimeError, match="GPU"):
        masked_td_lambda(Z(T + 1, B), Z(T, B), **kw)
    with pytest.raises(RuntimeError, match="GPU"):
        masked_td_lambda(Z(T, B), Z(T, B), next_value=Z(T, B), weight=Z(B), **kw)
    with pytest.raises(RuntimeError, match="GPU"):
        MaskedTDLambda(T, B)(Z(T + 1, B), Z(T, B), **kw)
    with pytest.raises(RuntimeError, match="GPU"):
        masked_vtrace(*_vt_args(), **kw)
    with pytest.raises(RuntimeError, match="GPU"):
        masked_vtrace(*_vt_args(False), next_value=Z(T, B), weight=Z(T, B), **kw)
    with pytest.raises(RuntimeError, match="GPU"):
        MaskedVTrace(T, B, N)(*_vt_args(), **kw)


@pytest.mark.parametrize("name", ["done", "traj_flag"])
@pytest.mark.parametrize("dtype", [torch.int64, torch.int32, torch.float64, torch.float16])
def test_wrong_mask_dtype_names_the_accepted_ones(name, dtype):
    from hpc_rll.rl_utils.td import masked_td_lambda
    from hpc_rll.rl_utils.vtrace import masked_vtrace
    msg = rf"{name}: dtype .* expected bool, uint8 or float32"
    with pytest.raises(RuntimeError, match=msg):
        masked_td_lambda(Z(T + 1, B), Z(T, B), **{name: Z(T, B, dtype=dtype)})
    with pytest.raises(RuntimeError, match=msg):
        masked_vtrace(*_vt_args(), **{name: Z(T, B, dtype=dtype)})


def test_mismatched_shapes_are_named():
    from hpc_rll.rl_utils.td import masked_td_lambda
    from hpc_rll.rl_utils.vtrace import masked_vtrace
    for fn, args in ((masked_td_lambda, lambda v: (v, Z(T, B))),
                     (masked_vtrace, lambda v: _vt_args()[:3] + (v, Z(T, B)))):
        with pytest.raises(RuntimeError, match=r"done: shape"):
            fn(*args(Z(T + 1, B)), done=Z(T + 1, B, dtype=torch.bool))
        with pytest.raises(RuntimeError, match=r"traj_flag: shape"):
            fn(*args(Z(T + 1, B)), traj_flag=Z(T, B + 1))
        with pytest.raises(RuntimeError, match=r"value: shape .*\(T\+1,B\)"):
            fn(*args(Z(T, B)))
        with pytest.raises(RuntimeError, match=r"value: shape .*\(T,B\)"):
            fn(*args(Z(T + 1, B)), next_value=Z(T, B))
        with pytest.raises(RuntimeError, match=r"next_value: shape"):
            fn(*args(Z(T, B)), next_value=Z(T + 1, B))
        with pytest.raises(RuntimeError, match=r"weight: shape"):
            fn(*args(Z(T + 1, B)), weight=Z(T + 1, B))
        with pytest.raises(RuntimeError, match=r"weight: dtype"):
            fn(*args(Z(T + 1, B)), weight=Z(T, B, dtype=torch.float64))
    with pytest.raises(RuntimeError, match=r"weight: shape"):    # V-trace takes weight (T,B) only
        masked_vtrace(*_vt_args(), weight=Z(B))
    with pytest.raises(RuntimeError, match=r"action: "):
        masked_vtrace(*(_vt_args()[:2] + (Z(T, B),) + _vt_args()[3:]))
    with pytest.raises(RuntimeError, match=r"behaviour_output: shape"):
        masked_vtrace(Z(T, B, N), Z(T, B, N + 1), *_vt_args()[2:])


def test_c_entry_points_declared_and_exported():
    import cabi
    td, vt = "hpc_rll_td_lambda_masked_forward", "hpc_rll_vtrace_masked_forward"
    for name in (td, vt):
        assert name in cabi.SIGNATURES, name
        assert hasattr(cabi.lib, name), name
    assert cabi.SIGNATURES[td][0] is ctypes.c_int and len(cabi.SIGNATURES[td][1]) == 17
    assert cabi.SIGNATURES[vt][0] is ctypes.c_int and len(cabi.SIGNATURES[vt][1]) == 22
    assert cabi.lib.hpc_rll_abi_version() == 6


def test_c_argument_errors_are_status_codes():
    """Rejected before any HIP call is made (no GPU needed).  Fake, aligned addresses stand in for device buffers."""
    import cabi
    L = cabi.lib
    P = 4096       # an aligned non-null stand-in
    td = L.hpc_rll_td_lambda_masked_forward
    #         value nv    reward weight mode done flag dt  loss grad part  T  B   gamma lam  scale stream
    assert td(None, None, None, None, 0, None, None, 0, P, P, P, 4, 4, 0.9, 0.8, 1.0, None) == -1    # null value
    assert td(P, None, P, None, 0, None, None, 0, None, P, P, 4, 4, 0.9, 0.8, 1.0, None) == -1       # null loss
    assert td(P, None, P, None, 0, None, None, 7, P, P, P, 4, 4, 0.9, 0.8, 1.0, None) == -1          # mask dtype
    assert td(P, None, P, None, 3, None, None, 0, P, P, P, 4, 4, 0.9, 0.8, 1.0, None) == -1          # weight mode
    assert td(P, None, P, None, 1, None, None, 0, P, P, P, 4, 4, 0.9, 0.8, 1.0, None) == -1          # mode 1, no weight
    assert td(P, None, P, None, 0, None, None, 0, P, P, P, -1, 4, 0.9, 0.8, 1.0, None) == -1         # T < 0
    assert td(P, None, P, None, 0, None, None, 0, P, P, P, 4, -3, 0.9, 0.8, 1.0, None) == -1         # B < 0
    assert td(P, None, P, None, 0, None, None, 0, P, None, P, 4, 4, 0.9, 0.8, 1.0, None) == -1       # null grad_buf
    assert td(P + 2, None, P, None, 0, None, None, 0, P, P, P, 4, 4, 0.9, 0.8, 1.0, None) == -2     # misaligned
    assert td(P, None, P, None, 0, P + 1, None, 1, P, P, P, 4, 4, 0.9, 0.8, 1.0, None) == -2         # f32 mask align
    vt = L.hpc_rll_vtrace_masked_forward
    #         tgt beh act val nv reward weight done flag dt losses ws T B N gamma lam rho c pg scale stream
    args = [P, P, P, P, None, P, None, None, None, 0, P, P, 4, 4, 3, 0.99, 0.95, 1.0, 1.0, 1.0, 1.0, None]

    def call(**kw):
        a = list(args)
        for k, v in kw.items():
            a[{"tgt": 0, "val": 3, "dt": 9, "losses": 10, "ws": 11, "T": 12, "B": 13, "N": 14, "done": 7}[k]] = v
        return vt(*a)
    assert call(tgt=None) == -1
    assert call(val=None) == -1
    assert call(ws=None) == -1
    assert call(losses=None) == -1
    assert call(dt=2) == -1
    assert call(T=-1) == -1
    assert call(B=-1) == -1
    assert call(N=0) == -1
    assert call(tgt=P + 2) == -2
    assert call(dt=1, done=P + 2) == -2
