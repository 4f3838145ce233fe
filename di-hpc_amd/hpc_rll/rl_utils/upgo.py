"""``hpc_rll.rl_utils.upgo`` -- drop-in for /root/reference/hpc_rll/rl_utils/upgo.py (``UPGO(T,B,N)``, forward
signature upgo.py:58, returns the (1,) loss).  Backward recomputes the softmax instead of saving a (T,B,N) buffer.
The autograd node is ``hpc_rl_utils.upgo`` (compiled torch::autograd::Function).

``masked_upgo`` / ``MaskedUPGO`` (no reference counterpart) are episode-aware UPGO with ``done`` and ``traj_flag`` masks,
the conventions of ``hpc_rll.rl_utils.td.masked_td_lambda``; see ``masked_upgo``."""
import torch

import hpc_rl_utils
from hpc_rll import dist as _dp


class UPGO(torch.nn.Module):
    """Importance-sampled UPGO loss: -mean(rho * (upgo_return - V) * log pi(a))."""

    def __init__(self, T, B, N, sharded: bool = False, group=None):
        super().__init__()
        self.T, self.B, self.N, self.sharded, self.group = T, B, N, sharded, group

    def forward(self, target_output, rhos, action, rewards, bootstrap_values):
        """target_output (T,B,N), rhos (T,B), action (T,B) int64, rewards (T,B), bootstrap_values (T+1,B)."""
        assert target_output.is_cuda
        assert rhos.is_cuda
        assert action.is_cuda
        assert rewards.is_cuda
        assert bootstrap_values.is_cuda
        scale = _dp.loss_scale(rewards.numel(), self.group, True) if self.sharded else None
        loss = hpc_rl_utils.upgo(target_output, rhos, action, rewards, bootstrap_values, scale)
        if self.sharded:
            _dp.all_reduce_losses_(loss.detach(), self.group, True)
        return loss


def masked_upgo(target_output, rhos, action, rewards, bootstrap_values, done=None, gamma: float = 1.0, next_value=None,
                traj_flag=None):
    r"""Episode-aware importance-sampled UPGO loss with done and truncation masks.

    ``target_output`` (T,B,N) logits, ``rhos`` (T,B), ``action`` (T,B) int64, ``rewards`` (T,B); the values are either
    stacked, ``bootstrap_values`` (T+1,B), or in the next-value form, ``bootstrap_values`` (T,B) with ``next_value`` (T,B).
    With ``k^d_t = 1 - done_t``, ``k^f_t = 1 - f_t`` (``f = traj_flag``, default: ``done``), ``V_t = bootstrap_values[t]``,
    ``nv_t = bootstrap_values[t+1]`` (stacked) or ``next_value[t]`` (next-value form) and ``G_T = nv_{T-1}``, for
    ``t = T-1 .. 0``::

        q_t   = rewards_t + gamma*k^d_t*nv_t                          (one-step target of step t)
        lam_t = 1 for t = T-1, else [q_{t+1} >= V_{t+1}]              (V_{t+1} is row t+1 of bootstrap_values in both forms)
        a_t   = gamma*k^f_t*lam_t
        G_t   = rewards_t + (gamma*k^d_t - a_t)*nv_t + a_t*G_{t+1}
        loss  = -mean(rhos * (G - V[:T]) * log pi(action)),           G a constant of the loss

    ``k^d`` weights the bootstrap value, ``k^f`` the trace: a ``done`` step returns ``rewards_t``, and the comparison for
    step ``t`` uses step ``t+1``'s own ``done``, so a terminal step's target is ``rewards_{t+1}``.  Masks are (T,B)
    ``bool``, ``uint8`` (nonzero counts as 1) or ``float32`` (soft masks, ``1 - m`` used as written); callers set
    ``traj_flag_t = 1`` wherever ``done_t = 1``.  Time-limit truncation: next-value form, ``done_t = 0``,
    ``traj_flag_t = 1`` and the final observation's value in ``next_value[t]``; that step returns
    ``rewards_t + gamma*nv_t``.  The gradient flows to ``target_output`` only.

    How it differs from :class:`UPGO`: that op carries both the return and the comparison
    ``r_{t+1} + V_{t+2} >= V_{t+1}`` across an episode end and has no discount.  With ``gamma = 1``, the stacked form and
    no masks (or all-zero masks) this one gives its loss and gradient bit for bit.  Returns the (1,) loss.
    """
    return hpc_rl_utils.upgo_masked(target_output, rhos, action, rewards, bootstrap_values, done, traj_flag, next_value,
                                    gamma)


class MaskedUPGO(torch.nn.Module):
    """Module form of :func:`masked_upgo`, with the data-parallel option of :class:`UPGO` (``sharded=True``:
    1/(global count) scale and one all-reduce of the loss)."""

    def __init__(self, T, B, N, sharded: bool = False, group=None):
        super().__init__()
        self.T, self.B, self.N, self.sharded, self.group = T, B, N, sharded, group

    def forward(self, target_output, rhos, action, rewards, bootstrap_values, done=None, gamma: float = 1.0,
                next_value=None, traj_flag=None):
        scale = _dp.loss_scale(rewards.numel(), self.group, True) if self.sharded else None
        loss = hpc_rl_utils.upgo_masked(target_output, rhos, action, rewards, bootstrap_values, done, traj_flag,
                                        next_value, gamma, scale)
        if self.sharded:
            _dp.all_reduce_losses_(loss.detach(), self.group, True)
        return loss
