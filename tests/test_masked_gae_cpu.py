"""CPU tier of the episode-aware GAE (``masked_gae`` / ``MaskedGAE`` / ``hpc_rl_utils.gae_masked``): the API exists,
host tensors are rejected loudly (no CPU path), wrong mask dtypes and mismatched shapes are named, and the two C entry
points are declared in the header and exported by the library."""
import inspect

import pytest
import torch


def Z(*s, dtype=torch.float32):
    return torch.zeros(*s, dtype=dtype)


T, B = 5, 3


def test_api_exists():
    import hpc_rl_utils
    from hpc_rll.rl_utils.gae import GAE, MaskedGAE, masked_gae
    assert callable(hpc_rl_utils.gae_masked)
    params = list(inspect.signature(masked_gae).parameters)
    assert params == ["value", "reward", "done", "gamma", "lambda_", "next_value", "traj_flag"]
    fwd = list(inspect.signature(MaskedGAE.forward).parameters)
    assert fwd == ["self"] + params
    m = MaskedGAE(T, B)
    assert isinstance(m, torch.nn.Module) and (m.T, m.B) == (T, B)
    assert "GAE" in masked_gae.__doc__ and "traj_flag" in masked_gae.__doc__
    assert MaskedGAE is not GAE


@pytest.mark.parametrize("kw", [{}, {"done": Z(T, B, dtype=torch.bool)}, {"done": Z(T, B, dtype=torch.uint8)},
                                {"done": Z(T, B), "traj_flag": Z(T, B, dtype=torch.bool)}])
def test_host_tensors_are_rejected(kw):
    from hpc_rll.rl_utils.gae import MaskedGAE, masked_gae
    with pytest.raises(RuntimeError, match="GPU"):
        masked_gae(Z(T + 1, B), Z(T, B), **kw)
    with pytest.raises(RuntimeError, match="GPU"):
        masked_gae(Z(T, B), Z(T, B), next_value=Z(T, B), **kw)
    with pytest.raises(RuntimeError, match="GPU"):
        MaskedGAE(T, B)(Z(T + 1, B), Z(T, B), **kw)


@pytest.mark.parametrize("name", ["done", "traj_flag"])
@pytest.mark.parametrize("dtype", [torch.int64, torch.int32, torch.float64, torch.float16])
def test_wrong_mask_dtype_names_the_accepted_ones(name, dtype):
    from hpc_rll.rl_utils.gae import masked_gae
    with pytest.raises(RuntimeError, match=rf"{name}: dtype .* expected bool, uint8 or float32"):
        masked_gae(Z(T + 1, B), Z(T, B), **{name: Z(T, B, dtype=dtype)})


def test_mismatched_shapes_are_named():
    from hpc_rll.rl_utils.gae import masked_gae
    with pytest.raises(RuntimeError, match=r"done: shape"):
        masked_gae(Z(T + 1, B), Z(T, B), done=Z(T + 1, B, dtype=torch.bool))
    with pytest.raises(RuntimeError, match=r"traj_flag: shape"):
        masked_gae(Z(T + 1, B), Z(T, B), traj_flag=Z(T, B + 1))
    with pytest.raises(RuntimeError, match=r"value: shape .*\(T\+1,B\)"):
        masked_gae(Z(T, B), Z(T, B))
    with pytest.raises(RuntimeError, match=r"value: shape .*\(T,B\)"):
        masked_gae(Z(T + 1, B), Z(T, B), next_value=Z(T, B))
    with pytest.raises(RuntimeError, match=r"next_value: shape"):
        masked_gae(Z(T, B), Z(T, B), next_value=Z(T + 1, B))
    with pytest.raises(RuntimeError, match=r"reward: expected \(T,B\)"):
        masked_gae(Z(T + 1, B), Z(T))


def test_c_entry_points_declared_and_exported():
    import ctypes
    import cabi
    for name in ("hpc_rll_gae_masked_forward", "hpc_rll_gae_masked_backward"):
        assert name in cabi.SIGNATURES, name
        assert hasattr(cabi.lib, name), name
    fwd, bwd = cabi.SIGNATURES["hpc_rll_gae_masked_forward"], cabi.SIGNATURES["hpc_rll_gae_masked_backward"]
    assert fwd[0] is ctypes.c_int and len(fwd[1]) == 12
    assert bwd[0] is ctypes.c_int and len(bwd[1]) == 13
    hdr = open(cabi.HEADER_PATH).read()
    assert "#define HPC_RLL_MASK_U8 (0)" in hdr and "#define HPC_RLL_MASK_F32 (1)" in hdr


def test_c_argument_errors_are_status_codes():
    """Rejected before any HIP call is made (no GPU needed)."""
    import cabi
    L = cabi.lib
    assert L.hpc_rll_gae_masked_forward(None, None, None, None, None, 0, None, 4, 4, 0.99, 0.97, None) == -1  # nulls
    assert L.hpc_rll_gae_masked_forward(None, None, None, None, None, 0, None, -1, 4, 0.99, 0.97, None) == -1
    assert L.hpc_rll_gae_masked_forward(None, None, None, None, None, 7, None, 0, 4, 0.99, 0.97, None) == -1  # dtype code
    assert L.hpc_rll_gae_masked_forward(None, None, None, None, None, 1, None, 0, 4, 0.99, 0.97, None) == 0   # empty
    assert L.hpc_rll_gae_masked_backward(None, None, None, 0, None, None, None, 1, 4, -2, 0.99, 0.97, None) == -1
    assert L.hpc_rll_gae_masked_backward(None, None, None, 2, None, None, None, 1, 4, 4, 0.99, 0.97, None) == -1
    assert L.hpc_rll_gae_masked_backward(None, None, None, 0, None, None, None, 3, 4, 4, 0.99, 0.97, None) == -1  # stacked
    assert L.hpc_rll_gae_masked_backward(None, None, None, 0, None, None, None, 1, 4, 4, 0.99, 0.97, None) == -1  # grad_adv
    assert L.hpc_rll_gae_masked_backward(None, None, None, 0, None, 8, None, 1, 4, 4, 0.99, 0.97, None) == -1  # nv + stacked
    assert L.hpc_rll_gae_masked_backward(None, None, None, 0, None, None, None, 0, 4, 0, 0.99, 0.97, None) == 0
