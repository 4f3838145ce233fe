"""``hpc_rll.rl_utils.gae`` -- drop-in for the reference module of the same path
(/root/reference/hpc_rll/rl_utils/gae.py:6-61): same class name, constructor ``GAE(T, B)`` and
``forward(value, reward, gamma=0.99, lambda_=0.97)``.

Differences, all deliberate:
  * outputs are allocated per call from torch's caching allocator instead of being a module buffer
    that every call overwrites (reference gae.py:39);
  * backward exists: the reference returns None for every input (gae.py:17-18), here
    ``adv.backward(g)`` yields d/dvalue and d/dreward (analytic adjoint of hpc_rll.origin.gae).

The autograd node lives in the compiled extension (``hpc_rl_utils.gae``, a torch::autograd::Function): one pybind
call per forward, backward runs entirely inside the autograd engine.

``masked_gae`` / ``MaskedGAE`` (no reference counterpart) are episode-aware GAE with ``done`` and ``traj_flag`` masks,
DI-engine's semantics; see ``masked_gae``.
"""
import torch

import hpc_rl_utils


class GAE(torch.nn.Module):
    """Generalized Advantage Estimator (arXiv:1506.02438), truncation-normalised variant of the reference.

    Arguments of the constructor are kept for API compatibility (trajectory length T, batch size B);
    the kernels take the sizes from the tensors, so any (T, B) works with one instance.
    """

    def __init__(self, T, B):
        super().__init__()
        self.T, self.B = T, B

    def forward(self, value, reward, gamma: float = 0.99, lambda_: float = 0.97) -> torch.FloatTensor:
        """value (T+1,B), reward (T,B) -> adv (T,B); all fp32 contiguous on the GPU."""
        assert value.is_cuda
        assert reward.is_cuda
        return hpc_rl_utils.gae(value, reward, gamma, lambda_)


def masked_gae(value, reward, done=None, gamma: float = 0.99, lambda_: float = 0.97, next_value=None,
               traj_flag=None) -> torch.FloatTensor:
    r"""Episode-aware GAE (arXiv:1506.02438) with done and truncation masks: textbook GAE, as DI-engine's ``gae``.

    With ``f = traj_flag`` (default: ``done``) and ``adv_T = 0``, for ``t = T-1 .. 0``::

        nv_t    = next_value[t]                  (next-value form: value (T,B), next_value (T,B))
                = value[t+1]                     (stacked form: value (T+1,B), row T the bootstrap value)
        delta_t = reward_t + gamma * (1 - done_t) * nv_t - value_t
        adv_t   = delta_t + gamma * lambda_ * (1 - f_t) * adv_{t+1}

    ``done`` / ``traj_flag`` are (T,B) ``bool``, ``uint8`` (nonzero counts as 1) or ``float32`` (``1 - m`` used as
    written: soft masks); ``done=None`` means no episode ends.  Time-limit truncation: use the next-value form with
    ``done_t = 0``, ``traj_flag_t = 1`` and the final observation's value in ``next_value[t]`` (in the stacked form row
    ``t+1`` already holds the value of the reset state).

    Differentiable wrt ``value``, ``next_value`` and ``reward`` (analytic adjoint; masks get no gradient):
    ``d_t = g_t + gamma*lambda_*(1 - f_{t-1})*d_{t-1}``, ``dL/dreward_t = d_t``; next-value form ``dL/dvalue_t = -d_t``,
    ``dL/dnext_value_t = gamma*(1 - done_t)*d_t``; stacked form
    ``dL/dvalue_t = -d_t [t<T] + gamma*(1 - done_{t-1})*d_{t-1} [t>=1]``.

    How it differs from :class:`GAE`: ``GAE`` keeps the reference's truncation normalisation (coefficients
    ``gamma*lambda*D_{t+1}/D_t``) and no masks; ``masked_gae`` without masks is plain textbook GAE, so
    its values differ from ``GAE``'s.  All tensors live on one GPU and are contiguous; value / reward fp32.
    """
    return hpc_rl_utils.gae_masked(value, reward, done, traj_flag, next_value, gamma, lambda_)


class MaskedGAE(torch.nn.Module):
    """Module form of :func:`masked_gae`.  ``T``, ``B`` are kept for symmetry with :class:`GAE`; the kernels take the
    sizes from the tensors."""

    def __init__(self, T, B):
        super().__init__()
        self.T, self.B = T, B

    def forward(self, value, reward, done=None, gamma: float = 0.99, lambda_: float = 0.97, next_value=None,
                traj_flag=None) -> torch.FloatTensor:
        return masked_gae(value, reward, done, gamma, lambda_, next_value, traj_flag)
