"""CPU tier of PPOContinuous (diagonal-Gaussian PPO): the parts that need no GPU -- argument errors of the three new C
entry points are status codes returned before any HIP call, the workspace size, the extension's rejection of CPU tensors,
and the Python signature.  Parity and everything that launches is in tests/test_ppo_continuous_gpu.py."""
import inspect

import pytest
import torch


def test_c_entry_points_reject_bad_arguments_before_any_hip_call():
    import cabi
    L = cabi.lib
    for name in ("hpc_rll_ppo_continuous_workspace_floats", "hpc_rll_ppo_continuous_forward",
                 "hpc_rll_ppo_continuous_backward"):
        assert name in cabi.SIGNATURES, name
    n10 = (None,) * 10
    assert L.hpc_rll_ppo_continuous_forward(*n10, None, None, 4, 4, 0.2, 1, 0.0, 0.25, None) == -1      # null pointers
    assert L.hpc_rll_ppo_continuous_forward(*n10, None, None, -1, 4, 0.2, 1, 0.0, 0.25, None) == -1     # negative B
    assert L.hpc_rll_ppo_continuous_forward(*n10, None, None, 4, 0, 0.2, 1, 0.0, 0.25, None) == -1      # A = 0
    assert L.hpc_rll_ppo_continuous_forward(*n10, None, None, 4, -3, 0.2, 1, 0.0, 0.25, None) == -1
    assert L.hpc_rll_ppo_continuous_forward(*n10, None, None, 0, 4, 0.2, 1, 0.0, 0.25, None) == -1      # B = 0 still needs out5
    assert L.hpc_rll_ppo_continuous_forward(*n10, None, None, 4, 2048, 0.2, 1, 0.0, 0.25, None) == -1   # nulls come before the A limit
    n7 = (None,) * 7
    assert L.hpc_rll_ppo_continuous_backward(*n7, None, None, None, 4, 4, None) == -1                    # no workspace
    assert L.hpc_rll_ppo_continuous_backward(*n7, None, None, None, -1, 4, None) == -1
    assert L.hpc_rll_ppo_continuous_backward(*n7, None, None, None, 4, 0, None) == -1
    assert L.hpc_rll_ppo_continuous_backward(*n7, None, None, None, 0, 4, None) == 0                     # B = 0: nothing to do, no launch
    assert L.hpc_rll_ppo_continuous_workspace_floats(-1) == -1


@pytest.mark.parametrize("B", [0, 1, 7, 4096, 65536, 1 << 22])
def test_workspace_holds_three_floats_per_sample_and_the_partials(B):
    import cabi
    assert cabi.lib.hpc_rll_ppo_continuous_workspace_floats(B) >= 3 * B + 5 * 512


def test_cpu_tensor_is_a_runtime_error():
    import hpc_rl_utils
    z = torch.zeros
    with pytest.raises(RuntimeError, match="GPU"):
        hpc_rl_utils.ppo_continuous(z(4, 3), z(4, 3) + 1, z(4, 3), z(4, 3) + 1, z(4, 3), z(4), z(4), z(4), z(4))
    with pytest.raises(RuntimeError, match="GPU"):
        hpc_rl_utils.ppo_continuous(z(4, 3), z(4, 3) + 1, z(4, 3), z(4, 3) + 1, z(4, 3), z(4), z(4), z(4), z(4), None, 0.2,
                                    True, 3.0, 0.25)


def test_python_signatures():
    from hpc_rll.rl_utils.ppo import PPO, PPOContinuous, ppo_continuous
    E = inspect.Parameter.empty
    want = [("mu_new", E), ("sigma_new", E), ("mu_old", E), ("sigma_old", E), ("action", E), ("value_new", E),
            ("value_old", E), ("adv", E), ("return_", E), ("weight", None), ("clip_ratio", 0.2), ("use_value_clip", True),
            ("dual_clip", None)]
    got = [(p.name, p.default) for p in inspect.signature(PPOContinuous.forward).parameters.values()]
    assert got == [("self", E)] + want
    fn = list(inspect.signature(ppo_continuous).parameters.values())
    assert [(p.name, p.default) for p in fn[:len(want)]] == want
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is not E for p in fn[len(want):])
    init = inspect.signature(PPOContinuous.__init__).parameters
    assert [(p.name, p.default) for p in init.values()] == [("self", E), ("B", E), ("A", E), ("sharded", False), ("group", None),
                                                            ("sync_info", True)]
    assert init["sync_info"].kind is inspect.Parameter.KEYWORD_ONLY
    assert [p for p in inspect.signature(PPO.__init__).parameters][1:3] == ["B", "N"]     # the categorical op is untouched


@pytest.mark.parametrize("dual_clip", [1.0, 0.5, 0.0, -2.0])
def test_dual_clip_must_exceed_one(dual_clip):
    """The assert fires before anything touches the tensors (they are CPU tensors here)."""
    from hpc_rll.rl_utils.ppo import PPOContinuous, ppo_continuous
    z = torch.zeros
    args = (z(2, 3), z(2, 3) + 1, z(2, 3), z(2, 3) + 1, z(2, 3), z(2), z(2), z(2), z(2))
    with pytest.raises(AssertionError, match="dual_clip"):
        PPOContinuous(2, 3)(*args, dual_clip=dual_clip)
    with pytest.raises(AssertionError, match="dual_clip"):
        ppo_continuous(*args, dual_clip=dual_clip)
