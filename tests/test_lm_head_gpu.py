"""GPU tier of what csrc/lm_head.hpp shares between the GRPO unit and the LM-PPO unit: both launch their heads and gradients
through the same dispatcher, and each keeps its own record.

(The two heads are instances of one kernel, without and with the entropy moment, but their ``logp`` and ``lse`` are NOT bit-equal:
the compiler contracts the two instances differently, 1 ulp in a few rows, before and after the sharing;
profiles/r20_lm_head_share.txt has the figures.  Each is checked against float64 in its own test file.)"""
import ctypes

import pytest
import torch

from lm_rows import expect_grad, expect_head, place

pytestmark = pytest.mark.gpu


def records():
    import cabi
    g, l = (ctypes.c_int * 16)(), (ctypes.c_int * 24)()
    assert cabi.lib.hpc_rll_grpo_last_config(g) == 0 and cabi.lib.hpc_rll_lm_ppo_last_config(l) == 0
    return list(g), list(l)


def test_the_records_stay_apart():
    """A GRPO head and gradient launch leaves all 24 ints of the LM-PPO record as they were, and the reverse."""
    from hpc_rll.rl_utils.grpo import token_log_prob
    from hpc_rll.rl_utils.lm_ppo import token_log_prob_entropy
    rows, V = 3, 8
    gen = torch.Generator().manual_seed(1)
    x, act = torch.randn(rows, V, generator=gen), torch.randint(0, V, (rows,), generator=gen)
    up = place(torch.randn(rows, generator=gen))
    g0, l0 = records()
    xd = place(x).requires_grad_(True)
    token_log_prob(xd, place(act)).backward(up)
    g1, l1 = records()
    assert l1 == l0, (l0, l1)
    assert g1[0] == g0[0] + 1 and g1[10] == g0[10] + 1       # the head and the gradient launch were noted, in GRPO's record
    assert g1[1:7] == expect_head(xd, rows, V) and g1[11:16] == expect_grad(xd, xd.grad, rows, V)
    xd = place(x).requires_grad_(True)
    logp, H = token_log_prob_entropy(xd, place(act))
    torch.autograd.backward([logp, H], [up, up])
    g2, l2 = records()
    assert g2 == g1, (g1, g2)
    assert l2[0] == l1[0] + 1 and l2[18] == l1[18] + 1
    assert l2[1:7] == expect_head(xd, rows, V) and l2[19:24] == expect_grad(xd, xd.grad, rows, V)
