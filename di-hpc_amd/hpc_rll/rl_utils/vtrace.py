"""``hpc_rll.rl_utils.vtrace`` -- drop-in for /root/reference/hpc_rll/rl_utils/vtrace.py (``VTrace(T,B,N)``,
forward signature vtrace.py:83, returns the ``hpc_vtrace_loss`` namedtuple of three (1,) tensors).

Backward recomputes the softmax from ``target_output`` instead of saving three (T,B,N) gradient buffers
(reference vtrace.py:70-72): forward writes 24 B per (t,b) of scratch instead of 12*N B.  The autograd node is
``hpc_rl_utils.vtrace`` (compiled torch::autograd::Function).

``masked_vtrace`` / ``MaskedVTrace`` (no reference counterpart) are episode-aware V-trace with ``done`` and ``traj_flag``
masks, the conventions of ``hpc_rll.rl_utils.gae.masked_gae``; see ``masked_vtrace``.

``vtrace_continuous`` / ``VTraceContinuous`` (no reference counterpart) are ``masked_vtrace`` for diagonal-Gaussian policies
(continuous actions, DI-engine's ``vtrace_error_continuous_action``); see ``vtrace_continuous``."""
from collections import namedtuple

import torch

import hpc_rl_utils
from hpc_rll import dist as _dp

hpc_vtrace_loss = namedtuple('hpc_vtrace_loss', ['policy_loss', 'value_loss', 'entropy_loss'])


class VTrace(torch.nn.Module):
    """IMPALA V-trace actor-critic losses (arXiv:1802.01561)."""

    def __init__(self, T, B, N, sharded: bool = False, group=None):
        super().__init__()
        self.T, self.B, self.N, self.sharded, self.group = T, B, N, sharded, group

    def forward(self, target_output, behaviour_output, action, value, reward, weight=None, gamma: float = 0.99,
                lambda_: float = 0.95, rho_clip_ratio: float = 1.0, c_clip_ratio: float = 1.0,
                rho_pg_clip_ratio: float = 1.0):
        """target/behaviour_output (T,B,N), action (T,B) int64, value (T+1,B), reward (T,B), weight (T,B) or None."""
        assert target_output.is_cuda
        assert behaviour_output.is_cuda
        assert action.is_cuda
        assert value.is_cuda
        assert reward.is_cuda
        if weight is not None:
            assert weight.is_cuda
        scale = _dp.loss_scale(reward.numel(), self.group, True) if self.sharded else None
        pg, v, e = hpc_rl_utils.vtrace(target_output, behaviour_output, action, value, reward, weight, gamma, lambda_,
                                       rho_clip_ratio, c_clip_ratio, rho_pg_clip_ratio, scale)
        if self.sharded:
            pg, v, e = _dp.all_reduce_sum((pg, v, e), self.group)     # the three scalars in ONE all-reduce
        return hpc_vtrace_loss(pg, v, e)


def masked_vtrace(target_output, behaviour_output, action, value, reward, done=None, weight=None, gamma: float = 0.99,
                  lambda_: float = 0.95, rho_clip_ratio: float = 1.0, c_clip_ratio: float = 1.0,
                  rho_pg_clip_ratio: float = 1.0, next_value=None, traj_flag=None):
    r"""Episode-aware IMPALA V-trace losses (arXiv:1802.01561 with per-step discounts) with done and truncation masks.

    ``IS = exp(logp_target - logp_behaviour)``, ``rho``, ``c``, ``rho_pg`` its clips and the entropy as in
    :class:`VTrace`.  With ``k^d_t = 1 - done_t``, ``k^f_t = 1 - f_t`` (``f = traj_flag``, default: ``done``), ``nv_t``
    as in :func:`hpc_rll.rl_utils.td.masked_td_lambda` (``value[t+1]`` stacked, ``next_value[t]`` in the next-value form)
    and ``s_T = 0``, for ``t = T-1 .. 0``::

        s_t   = rho_t * (reward_t + gamma*k^d_t*nv_t - value_t) + gamma*lambda_*k^f_t*c_t * s_{t+1}    (vs_t = value_t + s_t)
        adv_t = rho_pg_t * (reward_t + gamma*(k^d_t*nv_t + k^f_t*s_{t+1}) - value_t)

    policy_loss = -mean(logp_target * adv * weight), value_loss = mean(weight * (value - vs)^2), entropy_loss =
    mean(weight * entropy), ``vs`` and ``adv`` constants.  ``k^d`` weights the bootstrap value, ``k^f`` the trace.  Masks
    are (T,B) ``bool``, ``uint8`` (nonzero counts as 1) or ``float32`` (soft masks); callers set ``traj_flag_t = 1``
    wherever ``done_t = 1``; time-limit truncation: next-value form, ``done_t = 0``, ``traj_flag_t = 1`` and the final
    observation's value in ``next_value[t]``.  ``weight`` is None or (T,B).  Gradients flow to ``target_output`` and
    ``value`` (rows ``t < T``; the stacked bootstrap row gets zero).

    How it differs from :class:`VTrace`: that op carries the trace and the bootstrap value across an episode end; without
    masks (or with all-zero masks) this one gives its losses and gradients bit for bit.  With ``f = done`` and soft
    masks it is the per-step-discount V-trace with ``discounts = gamma*(1 - m)``.  Returns ``hpc_vtrace_loss``.
    """
    pg, v, e = hpc_rl_utils.vtrace_masked(target_output, behaviour_output, action, value, reward, done, traj_flag,
                                          next_value, weight, gamma, lambda_, rho_clip_ratio, c_clip_ratio,
                                          rho_pg_clip_ratio)
    return hpc_vtrace_loss(pg, v, e)


class MaskedVTrace(torch.nn.Module):
    """Module form of :func:`masked_vtrace`, with the data-parallel option of :class:`VTrace` (``sharded=True``:
    1/(global count) scale and the three losses in one all-reduce)."""

    def __init__(self, T, B, N, sharded: bool = False, group=None):
        super().__init__()
        self.T, self.B, self.N, self.sharded, self.group = T, B, N, sharded, group

    def forward(self, target_output, behaviour_output, action, value, reward, done=None, weight=None,
                gamma: float = 0.99, lambda_: float = 0.95, rho_clip_ratio: float = 1.0, c_clip_ratio: float = 1.0,
                rho_pg_clip_ratio: float = 1.0, next_value=None, traj_flag=None):
        scale = _dp.loss_scale(reward.numel(), self.group, True) if self.sharded else None
        pg, v, e = hpc_rl_utils.vtrace_masked(target_output, behaviour_output, action, value, reward, done, traj_flag,
                                              next_value, weight, gamma, lambda_, rho_clip_ratio, c_clip_ratio,
                                              rho_pg_clip_ratio, scale)
        if self.sharded:
            pg, v, e = _dp.all_reduce_sum((pg, v, e), self.group)     # the three scalars in ONE all-reduce
        return hpc_vtrace_loss(pg, v, e)


def vtrace_continuous(mu_target, sigma_target, mu_behaviour, sigma_behaviour, action, value, reward, done=None,
                      weight=None, gamma: float = 0.99, lambda_: float = 0.95, rho_clip_ratio: float = 1.0,
                      c_clip_ratio: float = 1.0, rho_pg_clip_ratio: float = 1.0, next_value=None, traj_flag=None):
    r"""Episode-aware V-trace losses for diagonal-Gaussian policies (continuous actions; the semantics of DI-engine's
    ``vtrace_error_continuous_action``, with the masks of :func:`masked_vtrace`).

    ``mu_*``, ``sigma_*`` and ``action`` are (T,B,A) float32, ``1 <= A <= 1024``; ``sigma`` is the standard deviation and
    ``sigma > 0`` is the caller's contract (device values are not checked).  With ``z = (action - mu) / sigma`` per
    dimension, summed over the A dimensions::

        logp    = sum(-z^2/2 - log(sigma)) - A*log(2*pi)/2            (target and behaviour policy alike)
        entropy = A*(1/2 + log(2*pi)/2) + sum(log(sigma_target))
        IS      = exp(logp_target - logp_behaviour)

    which are ``Independent(Normal(mu, sigma), 1).log_prob(action)`` and ``.entropy()``.  The log ratio is accumulated as a
    sum of per-dimension differences, so it does not lose precision as A grows, and identical policies give ``IS = 1``
    exactly.  From ``IS`` on -- ``rho``, ``c``, ``rho_pg``, the recursion for ``vs`` and ``adv`` with ``done`` /
    ``traj_flag`` / ``next_value``, ``weight`` (None or (T,B)) and the three mean losses -- everything is
    :func:`masked_vtrace`, bit for bit for equal log-probabilities: policy_loss = -mean(logp_target * adv * weight),
    value_loss = mean(weight * (value - vs)^2), entropy_loss = mean(weight * entropy).

    Gradients flow to ``mu_target``, ``sigma_target`` and ``value`` (rows ``t < T``; the stacked bootstrap row gets zero);
    nothing flows to the behaviour policy, ``action``, ``reward``, ``next_value`` or the masks.  Returns ``hpc_vtrace_loss``.
    """
    pg, v, e = hpc_rl_utils.vtrace_continuous(mu_target, sigma_target, mu_behaviour, sigma_behaviour, action, value, reward,
                                              done, traj_flag, next_value, weight, gamma, lambda_, rho_clip_ratio,
                                              c_clip_ratio, rho_pg_clip_ratio)
    return hpc_vtrace_loss(pg, v, e)


class VTraceContinuous(torch.nn.Module):
    """Module form of :func:`vtrace_continuous`, with the data-parallel option of :class:`MaskedVTrace`
    (``sharded=True``: 1/(global count) scale and the three losses in one all-reduce)."""

    def __init__(self, T, B, A, sharded: bool = False, group=None):
        super().__init__()
        self.T, self.B, self.A, self.sharded, self.group = T, B, A, sharded, group

    def forward(self, mu_target, sigma_target, mu_behaviour, sigma_behaviour, action, value, reward, done=None,
                weight=None, gamma: float = 0.99, lambda_: float = 0.95, rho_clip_ratio: float = 1.0,
                c_clip_ratio: float = 1.0, rho_pg_clip_ratio: float = 1.0, next_value=None, traj_flag=None):
        scale = _dp.loss_scale(reward.numel(), self.group, True) if self.sharded else None
        pg, v, e = hpc_rl_utils.vtrace_continuous(mu_target, sigma_target, mu_behaviour, sigma_behaviour, action, value,
                                                  reward, done, traj_flag, next_value, weight, gamma, lambda_,
                                                  rho_clip_ratio, c_clip_ratio, rho_pg_clip_ratio, scale)
        if self.sharded:
            pg, v, e = _dp.all_reduce_sum((pg, v, e), self.group)     # the three scalars in ONE all-reduce
        return hpc_vtrace_loss(pg, v, e)
