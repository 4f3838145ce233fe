"""CPU tier of TQC (``hpc_rll.rl_utils.tqc``, csrc/tqc.hip): what needs no GPU -- the fp64 oracle (tests/tqc_oracle.py) against
the quantile-Huber oracle of IQN / QR-DQN, the branch shares of the default problem, the fp32 evaluation of the oracle at the GPU
tier's shapes, the C ABI's refusals and the host messages.  Everything that launches is in tests/test_tqc_gpu.py."""
import numpy as np
import pytest
import torch

import tqc_oracle as O
from conftest import rel_err
from oracle import ref_torch as R

EINVAL, EALIGN, EUNSUPPORTED = -1, -2, -3
SHAPES = [(1, 1, 0, 1, 1), (5, 25, 10, 5, 25), (1, 63, 0, 1, 63), (1, 64, 3, 2, 32), (5, 13, 0, 3, 7), (4, 64, 37, 4, 64),
          (8, 64, 100, 2, 25), (8, 128, 300, 8, 128), (5, 25, 124, 5, 25)]   # (M', N', drop, M, N): the GPU tier's sweep


def test_single_net_without_truncation_is_the_quantile_huber_of_the_quantile_learners():
    B, N = 6, 25
    p = O.problem(B, 1, N, 1, N, salt=1)
    got = O.critic(p["z"], p["target_z"], p["nlp"], p["reward"], p["done"], p["weight"], alpha=0.0, gamma=0.97, kappa=1.0)
    tau = ((2 * torch.arange(N, dtype=torch.float64) + 1) / (2 * N)).reshape(N, 1).expand(N, B)
    q = p["z"].double().reshape(B, N).t().reshape(N, B, 1)
    tq = p["target_z"].double().reshape(B, N).t().reshape(N, B, 1)
    zero = torch.zeros(B, dtype=torch.long)
    loss, per = R.iqn_nstep_td_error(q, tq, zero, zero, p["reward"].double().reshape(1, B), p["done"].double(), tau,
                                     p["weight"].double(), 0.97, 1.0)
    assert rel_err(per.numpy() / N, got["td_error"]) <= 1e-12    # theirs sums over the online quantiles, TQC takes the mean
    assert rel_err(loss.reshape(1).numpy() / N, got["loss"]) <= 1e-12


def test_default_problem_fills_both_huber_branches_and_both_signs():
    p = O.problem(5, 5, 25, 5, 25)
    o = O.critic(p["z"], p["target_z"], p["nlp"], p["reward"], p["done"], p["weight"], drop=10)
    assert 0.1 <= o["share_neg"] <= 0.9 and 0.1 <= o["share_lin"] <= 0.9, (o["share_neg"], o["share_lin"])


@pytest.mark.parametrize("Mt,Nt,drop,M,N", SHAPES)
def test_fp32_oracle_stays_inside_the_bound_at_the_gpu_tiers_shapes(Mt, Nt, drop, M, N):
    p = O.problem(5, Mt, Nt, M, N)
    a = (p["z"], p["target_z"], p["nlp"], p["reward"], p["done"], p["weight"])
    o64, o32 = O.critic(*a, drop=drop), O.critic(*a, drop=drop, dtype=torch.float32)
    for k in ("loss", "td_error", "target_atoms"):
        assert rel_err(o64[k], o32[k]) <= 1e-5, k
    assert np.abs(o64["grad_z"] - o32["grad_z"]).max() <= 1e-5 * np.abs(o64["grad_z"]).max()


def test_c_abi_refuses_the_limits_and_bad_arguments_before_touching_anything():
    import cabi
    L = cabi.lib
    p = 4096   # a non-null, aligned stand-in: the checks run before any pointer is read
    def fwd(M, N, Mt, Nt, drop, z=p, kappa=1.0, rows=2):   # noqa: E306
        return L.hpc_rll_tqc_critic_forward(z, p, p, p, None, 0, None, None, 0.2, p, p, p, p, rows, M, N, Mt, Nt, drop, 0.99,
                                            kappa, 0.5, None)
    assert fwd(8, 128, 8, 128, 0, z=None) == EINVAL
    assert fwd(8, 129, 5, 25, 0) == EUNSUPPORTED            # M N = 1032
    assert fwd(5, 25, 25, 41, 0) == EUNSUPPORTED            # n = 1025
    assert fwd(5, 25, 5, 25, 125) == EINVAL and fwd(5, 25, 5, 25, -1) == EINVAL
    assert fwd(5, 25, 5, 25, 0, kappa=0.0) == EINVAL and fwd(5, 0, 5, 25, 0) == EINVAL and fwd(5, 25, 5, 25, 0, rows=-1) == EINVAL
    assert fwd(5, 25, 5, 25, 0, z=p + 2) == EALIGN
    assert L.hpc_rll_tqc_critic_backward(p, p, p, 2, 8, 129, None) == EUNSUPPORTED
    assert L.hpc_rll_tqc_policy_forward(p, p, None, 0.2, p, p, 2, 1025, 0.5, None) == EUNSUPPORTED
    assert L.hpc_rll_tqc_policy_backward(None, p, p, p, 2, 1025, None) == EUNSUPPORTED
    assert L.hpc_rll_tqc_workspace_floats(3, 125) > 3 * 125 and L.hpc_rll_tqc_workspace_floats(-1, 125) == EINVAL
    assert L.hpc_rll_tqc_last_config(None) == EINVAL
    assert L.hpc_rll_abi_version() == 6


def test_host_messages():
    from hpc_rll.rl_utils import tqc
    assert tqc.tanh_gaussian_rsample is not None and tqc.sac_alpha_loss is not None
    B = 4
    z, tz, v = torch.zeros(B, 5, 25), torch.zeros(B, 5, 25), torch.zeros(B)
    for args, kw, msg in [((z[0], tz, v, v), {}, r"z: expected \(B, M, N\)"),
                          ((z, tz[0], v, v), {}, r"target_z: expected \(B, M', N'\)"),
                          ((z[:3], tz, v, v), {}, "z: shape .* has 3 rows, target_z .* has 4"),
                          ((z, tz, v, v.reshape(B, 1)), {}, "reward: .*trailing dimension of 1"),
                          ((z, tz, v.reshape(B, 1), v), {}, "next_log_prob: shape"),
                          ((z, tz, v, v), dict(drop=125), "drop: 125 is out of range"),
                          ((z, tz, v, v), dict(drop=-1), "drop: -1 is out of range"),
                          ((torch.zeros(B, 8, 129), tz, v, v), {}, "must both lie in 1 .. 1024"),
                          ((z, tz, v, v), dict(done=torch.zeros(B, dtype=torch.int32)), "done: dtype"),
                          ((z, tz, v, v), {}, "z: must live on a GPU")]:
        with pytest.raises(RuntimeError, match=msg):
            tqc.tqc_critic_loss(*args, **kw)
    for args, msg in [((v, z[0]), r"new_z: expected \(B, M, N\)"), ((v.reshape(B, 1), z), "log_prob: .*trailing dimension of 1"),
                      ((v[:3], z), "log_prob: shape"), ((v, z), "new_z: must live on a GPU")]:
        with pytest.raises(RuntimeError, match=msg):
            tqc.tqc_policy_loss(*args)
