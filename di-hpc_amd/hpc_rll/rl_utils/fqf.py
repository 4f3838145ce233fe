"""``hpc_rll.rl_utils.fqf`` -- FQF, the Fully parameterized Quantile Function (Yang et al. 2019): the fourth distributional
Q-learner next to ``DistNStepTD`` (C51), ``QRDQNNStepTDError`` and ``IQNNStepTDError``.  No reference counterpart; the
functions restate DI-engine's ``fqf_nstep_td_error`` and ``fqf_calculate_fraction_loss`` (``ding/rl_utils/td.py``) and the
fraction proposal and expected value of its ``FQFHead`` (kernels: csrc/fqf.hip).

``K`` is the number of fractions (DI-engine ``num_quantiles``), ``N`` the number of actions, ``B`` the batch.  All floats are
fp32 contiguous GPU tensors, actions are int64.  One learner step::

    quantiles, quantiles_hats, entropies = fqf_fractions(logits)               # logits (B,K) of the proposal network
    # q = F(quantiles_hats), q_tau_i = F(quantiles[:, 1:-1]): the quantile network, (B,K,N) and (B,K-1,N)
    loss, td_err = fqf_nstep_td_error(fqf_nstep_td_data(q, next_n_q, action, next_n_action, reward, done, quantiles_hats,
                                                        weight), gamma, nstep)
    fraction_loss = fqf_calculate_fraction_loss(q_tau_i.detach(), q.detach(), quantiles, action)
    logit, greedy = fqf_q_value(target_q, target_quantiles, return_action=True)   # next_n_action of the next step

* :func:`fqf_fractions`: ``p = softmax(logits)``, ``quantiles = [0, cumsum(p)]`` (B,K+1), ``quantiles_hats`` the midpoints
  (B,K, detached), ``entropies = -sum p log p`` (B,1).  ``1 <= K <= 1024``.  A logit of ``-inf`` has ``p = 0`` and adds
  exactly 0 to the entropy.
* :func:`fqf_nstep_td_error`: the quantile Huber loss of IQN with per-sample fractions ``quantiles_hats[b,i]`` on DI-engine's
  layout ``q (B,K,N)``, ``next_n_q (B,K',N)``.  It equals ``IQNNStepTDError`` on ``q.permute(1,0,2)`` with
  ``replay_quantiles = quantiles_hats.t()``.  The gradient flows to ``q`` only.
* :func:`fqf_calculate_fraction_loss`: ``mean_b sum_i g_i * quantiles[b,i+1]`` with the constant ``g`` of Proposition 1 and
  DI-engine's sign corrections for non-monotone rows; the comparisons are made on the raw inputs.  The gradient flows to
  ``quantiles[:, 1:K]`` only.
* :func:`fqf_q_value`: ``sum_i (quantiles[:,i+1] - quantiles[:,i]) * q[:,i,:]`` and, when asked, its argmax over the actions
  (ties to the lowest index) from the same launch.  Forward only.

An action outside ``[0, N)`` never addresses memory: the value it would select reads as 0 and its gradient row is zero.  None
of the ops synchronises with the host; the loss sums are added in a fixed order."""
from collections import namedtuple
from typing import Optional

import torch

import hpc_rl_utils
from hpc_rll.rl_utils.td import _ShardedLoss

fqf_nstep_td_data = namedtuple('fqf_nstep_td_data', ['q', 'next_n_q', 'action', 'next_n_action', 'reward', 'done',
                                                     'quantiles_hats', 'weight'])


def fqf_fractions(logits: torch.Tensor):
    """``logits (B,K)`` -> ``(quantiles (B,K+1), quantiles_hats (B,K), entropies (B,1))``.  ``quantiles`` and ``entropies``
    are differentiable with respect to ``logits``; ``quantiles_hats`` is detached, as in DI-engine."""
    return tuple(hpc_rl_utils.fqf_fractions(logits))


def fqf_nstep_td_error(data, gamma: float, nstep: int = 1, kappa: float = 1.0,
                       value_gamma: Optional[torch.Tensor] = None):
    """DI-engine's ``fqf_nstep_td_error``: ``data`` is the 8-tuple ``(q (B,K,N), next_n_q (B,K',N), action (B,),
    next_n_action (B,), reward (nstep,B), done (B,) float, quantiles_hats (B,K), weight (B,) or None)``.  Returns
    ``(loss (1,), td_err (B,))``; ``td_err`` is unweighted and detached."""
    q, next_n_q, action, next_n_action, reward, done, quantiles_hats, weight = data
    assert reward.shape[0] == nstep, (tuple(reward.shape), nstep)
    loss, td_err = hpc_rl_utils.fqf_nstep_td(q, next_n_q, action, next_n_action, reward, done, quantiles_hats, weight,
                                             value_gamma, gamma, kappa, None)
    return loss, td_err


def fqf_calculate_fraction_loss(q_tau_i: torch.Tensor, q_value: torch.Tensor, quantiles: torch.Tensor,
                                actions: torch.Tensor):
    """DI-engine's ``fqf_calculate_fraction_loss``: ``q_tau_i (B,K-1,N)`` (the quantile network at ``quantiles[:,1:-1]``),
    ``q_value (B,K,N)`` (at ``quantiles_hats``), ``quantiles (B,K+1)``, ``actions (B,)`` -> loss (1,).  Both value tensors are
    constants; ``K = 1`` gives 0."""
    return hpc_rl_utils.fqf_fraction_loss(q_tau_i, q_value, quantiles, actions, None)


def fqf_q_value(q: torch.Tensor, quantiles: torch.Tensor, return_action: bool = False):
    """``q (B,K,N)``, ``quantiles (B,K+1)`` -> the expected value ``(B,N)``; with ``return_action`` a pair ``(logit, action)``
    where ``action (B,)`` int64 is the argmax over the actions, ties to the lowest index.  Outputs are detached."""
    logit, action = hpc_rl_utils.fqf_q_value(q, quantiles, return_action)
    return (logit, action) if return_action else logit


class FQFNStepTDError(_ShardedLoss):
    """Module form of :func:`fqf_nstep_td_error` with the data-parallel option of ``IQNNStepTDError``: ``sharded=True``
    splits the batch over the ranks, each rank scales with 1/(global B) and the loss takes one all-reduce.  ``td_err`` is
    per sample and stays local."""

    def __init__(self, sharded: bool = False, group=None):
        super().__init__()
        self.sharded, self.group = sharded, group

    def forward(self, q, next_n_q, action, next_n_action, reward, done, quantiles_hats, gamma: float, kappa: float = 1.0,
                weight: Optional[torch.Tensor] = None, value_gamma: Optional[torch.Tensor] = None):
        loss, td_err = hpc_rl_utils.fqf_nstep_td(q, next_n_q, action, next_n_action, reward, done, quantiles_hats, weight,
                                                 value_gamma, gamma, kappa, self._scale(q.shape[0]))
        return self._reduce(loss), td_err
