"""``hpc_rll.rl_utils.sac`` -- Soft Actor-Critic for discrete actions (Christodoulou 2019), fused into one forward launch and
one streaming backward (no reference counterpart; the formulas restate DI-engine's ``DiscreteSACPolicy._forward_learn`` with
``q_v_1step_td_error``).

``logit`` (the actor at ``s``), ``next_logit`` (the actor at ``s'``), ``q1``, ``q2`` (the online critics at ``s``) and
``target_q1``, ``target_q2`` (the target critics at ``s'``) are ``(..., N)``; ``action`` (int64), ``reward``, ``done`` and
``weight`` have the leading shape, ``(B,)`` in the usual case.  Per sample, with ``x``, ``y`` the rows of ``logit`` and
``next_logit``, ``a`` the action, ``k = 1 - done`` and ``w`` the weight::

    l' = log_softmax(y)   p' = exp(l')   m' = min(target_q1, target_q2)     V' = sum_n p'_n * (m'_n - alpha * l'_n)
    G  = reward + gamma * k * V'                                             (a constant of every loss)
    d_i = q_i[a] - G      critic_loss_i = mean_b(w * d_i^2)                  td_error[b] = mean_i d_i^2  (unweighted, detached)
    l  = log_softmax(x)   p = exp(l)     m = min(q1, q2)  (detached)         f = sum_n p_n * (alpha * l_n - m_n)
    policy_loss = mean_b(f)              H = -sum_n p_n * l_n                entropy = mean_b(H)         (a detached monitor)

    grad_q_i[b,n]   = g_i * 2 * w * d_i / rows * [n = a]
    grad_logit[b,n] = g_p * p_n * ((alpha * l_n - m_n) - f) / rows

``g_1``, ``g_2``, ``g_p`` are the upstream gradients of ``critic_loss``, ``twin_critic_loss`` and ``policy_loss``.  As in
DI-engine ``weight`` multiplies the critic losses only; the policy loss and the entropy are plain means.  ``q1`` and ``q2`` get
no gradient through ``m``; ``next_logit``, the target critics, ``reward`` and ``alpha`` get none at all.

Conventions:

* ``q2`` and ``target_q2`` are both given or both ``None`` (a single critic: ``m = q1``, ``m' = target_q1``); one without the
  other is an error.  ``twin_critic_loss`` is ``None`` for a single critic;
* ``done`` may be ``None``, bool, uint8 (nonzero counts as 1) or float32 (a soft mask); ``weight`` may be ``None`` or have the
  leading shape.  ``None`` gives the same bits as an all-zero ``done`` and an all-one ``weight``;
* ``alpha`` is a Python float or a 1-element fp32 GPU tensor, for example ``log_alpha.detach().exp()``.  The kernel reads the
  tensor on the device: there is no ``.item()`` and no host synchronisation anywhere in the op;
* a logit of ``-inf`` (a masked action) is clamped to the most negative finite float: its column has ``p_n = 0``, every sum
  selects on ``p_n > 0`` and never multiplies by ``p_n``, so the column adds exactly 0 to ``V'``, ``f`` and ``H`` and gets
  gradient 0 -- even when the critic value in that column is ``+-inf`` or NaN;
* an ``action`` outside ``[0, N)`` never addresses memory: ``d_i = 0``, ``td_error = 0`` and the critic gradient rows are
  zero; the policy part of the sample is unaffected;
* no rows (a zero in the leading shape) gives zero losses, zero-size ``td_error`` / ``target_q`` and launches nothing;
* ``N = 1`` gives ``policy_loss = -mean(m)`` and an identically zero logit gradient;
* fp32 contiguous GPU tensors, ``1 <= N <= 1024``.

Two deviations from DI-engine: the next state uses ``log_softmax`` exactly where DI-engine takes ``log(softmax + 1e-8)``, and
``td_error`` is the mean of the two squared errors, DI-engine's ``(td1 + td2) / 2``, as one tensor."""
from collections import namedtuple

import torch

import hpc_rl_utils
from hpc_rll import dist as _dp

sac_discrete_output = namedtuple('sac_discrete_output', ['policy_loss', 'critic_loss', 'twin_critic_loss', 'entropy',
                                                         'td_error', 'target_q'])


def _call(logit, next_logit, q1, q2, target_q1, target_q2, action, reward, done, weight, alpha, gamma, scale):
    a_t = alpha if isinstance(alpha, torch.Tensor) else None
    out = hpc_rl_utils.sac_discrete(logit, next_logit, q1, q2, target_q1, target_q2, action, reward, done, weight,
                                    0.0 if a_t is not None else float(alpha), a_t, gamma, scale)
    return list(out)


def _pack(out, twin):
    return sac_discrete_output(out[0], out[1], out[2] if twin else None, out[3], out[4], out[5])


def sac_discrete_loss(logit, next_logit, q1, q2, target_q1, target_q2, action, reward, done=None, weight=None,
                      alpha=0.2, gamma: float = 0.99):
    """The discrete SAC losses of one batch: a :data:`sac_discrete_output` ``(policy_loss, critic_loss, twin_critic_loss,
    entropy, td_error, target_q)``.  The first four are (1,) tensors (``twin_critic_loss`` is ``None`` when ``q2`` and
    ``target_q2`` are ``None``), ``td_error`` and ``target_q`` have the shape of ``action``; ``entropy``, ``td_error`` and
    ``target_q`` carry no gradient.  The gradient flows to ``logit`` (from ``policy_loss``), ``q1`` (from ``critic_loss``) and
    ``q2`` (from ``twin_critic_loss``); each is formed only when its tensor requires it."""
    return _pack(_call(logit, next_logit, q1, q2, target_q1, target_q2, action, reward, done, weight, alpha, gamma, None),
                 q2 is not None)


def sac_alpha_loss(log_alpha, entropy, target_entropy):
    """The temperature loss of discrete SAC, without a kernel.  DI-engine's form is
    ``mean_b(-sum_n p_n * log_alpha * (log p_n + target_entropy))``; with ``sum_n p_n = 1`` and ``H = -sum_n p_n log p_n``
    that is ``log_alpha * (H - target_entropy)`` exactly, so the ``entropy`` :func:`sac_discrete_loss` returns (the batch mean
    of ``H``) is all it needs: ``log_alpha * (entropy.detach() - target_entropy)``.  The gradient flows to ``log_alpha``
    only and equals ``entropy - target_entropy``."""
    return log_alpha * (entropy.detach() - target_entropy)


class SACDiscrete(torch.nn.Module):
    """Module form of :func:`sac_discrete_loss`, with the data-parallel option of :class:`hpc_rll.rl_utils.coma.COMA` and
    :class:`hpc_rll.rl_utils.r2d2.R2D2TD`: ``sharded=True`` splits the rows over the ranks; each rank scales with
    1/(global rows) and the four scalars are summed with one all-reduce of one packed tensor.  ``td_error`` and ``target_q``
    are per sample and stay local."""

    def __init__(self, sharded: bool = False, group=None):
        super().__init__()
        self.sharded, self.group = sharded, group

    def forward(self, logit, next_logit, q1, q2, target_q1, target_q2, action, reward, done=None, weight=None,
                alpha=0.2, gamma: float = 0.99):
        scale = _dp.loss_scale(action.numel(), self.group, True) if self.sharded else None
        out = _call(logit, next_logit, q1, q2, target_q1, target_q2, action, reward, done, weight, alpha, gamma, scale)
        if self.sharded:
            packed = _dp.all_reduce_losses_(torch.cat([t.detach() for t in out[:4]]), self.group, True)   # one all-reduce
            for i, t in enumerate(out[:4]):
                t.detach().copy_(packed[i:i + 1])
        return _pack(out, q2 is not None)
