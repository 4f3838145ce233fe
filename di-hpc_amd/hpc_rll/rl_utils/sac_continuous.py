"""``hpc_rll.rl_utils.sac_continuous`` -- Soft Actor-Critic for continuous actions (Haarnoja 2018) with a tanh-squashed Gaussian
policy: the reparameterised head in one launch each way and the losses in one launch each way (no reference counterpart; the
formulas restate DI-engine's ``SACPolicy._forward_learn`` with ``q_v_1step_td_error``).

**The head**, :func:`tanh_gaussian_rsample`.  ``mu``, ``sigma`` and ``eps`` are ``(..., A)``; ``eps`` is standard-normal noise
and a constant of the op (``eps=None`` draws ``torch.randn_like(mu)`` here in Python; there is no RNG in the kernel, so a given
``eps`` keeps the op deterministic and capturable).  ``sigma > 0`` is the caller's contract.  Per row::

    u_j  = mu_j + sigma_j * eps_j
    a_j  = tanh(u_j)                                                   -> action (..., A)
    logp = sum_j [ -eps_j^2/2 - log sigma_j - log(2 pi)/2
                   + 2|u_j| + 2 log1p(exp(-2|u_j|)) - 2 log 2 ]         -> log_prob (...)

    gu_j         = g_a_j * (1 - a_j^2) + 2 * g_l * a_j
    grad_mu_j    = gu_j
    grad_sigma_j = gu_j * eps_j - g_l / sigma_j

The last three terms of ``logp`` are ``-log(1 - tanh(u_j)^2)`` exactly.  ``g_a`` and ``g_l`` are the upstream gradients of
``action`` and ``log_prob``; one that is absent is not read.  The backward re-reads ``sigma``, ``eps`` and the saved
``action``; nothing else of size ``(..., A)`` is kept.  Where ``a = +-1`` exactly the ``g_a`` part of the gradient is exactly 0.

**The losses**, :func:`sac_continuous_loss`.  Every operand is one float per sample with the leading shape ``(...)`` of
``reward``, ``(B,)`` in the usual case.  With ``k = 1 - done`` and ``w = weight``::

    m' = min(target_q1, target_q2)    G = reward + gamma * k * (m' - alpha * next_log_prob)    (a constant; -> target_q)
    d_i = q_i - G                     critic_loss_i = mean(w * d_i^2)                           td_error = mean_i d_i^2  (unweighted, detached)
    m  = min(new_q1, new_q2)          policy_loss = mean(alpha * log_prob - m)                  entropy = -mean(log_prob)  (a detached monitor)

    grad_q_i      = g_i * 2 * w * d_i / rows
    grad_log_prob = g_p * alpha / rows
    grad_new_q_i  = -g_p / rows * s_i

``s_i`` is 1 for the strictly smaller of ``new_q1`` and ``new_q2``, 0 for the other and 1/2 each at a tie
(``torch.minimum``'s rule).  ``q_i`` are the online critics at the replayed action, ``new_q_i`` the online critics at the
action the head has just sampled (``log_prob`` is its log-probability), ``target_q_i`` the target critics at the next
state's sampled action (``next_log_prob``).  Nothing flows to the target critics, ``next_log_prob``, ``reward`` or ``alpha``.

Conventions:

* ``q2``, ``target_q2`` and ``new_q2`` are all given or all ``None`` (a single critic: ``m = new_q1``, ``m' = target_q1``);
  ``twin_critic_loss`` is then ``None``;
* ``done`` may be ``None``, bool, uint8 (nonzero counts as 1) or float32 (a soft mask); ``weight`` may be ``None``.  ``None``
  gives the same bits as an all-zero ``done`` and an all-one ``weight``.  As in DI-engine ``weight`` multiplies the critic
  losses only;
* ``alpha`` is a Python float or a 1-element fp32 GPU tensor, for example ``log_alpha.detach().exp()``.  The kernel reads the
  tensor on the device: there is no ``.item()`` and no host synchronisation anywhere in the op;
* a trailing dimension of 1 (a critic that returns ``(B, 1)``) is the caller's to ``squeeze(-1)``: it is refused with a message;
* no rows (a zero in the leading shape) gives zero losses and launches nothing;
* both minima propagate a NaN from either side, as ``torch.minimum`` does, and ``0 * NaN`` is NaN: a NaN in ``target_q2`` of a
  ``done = 1`` row still poisons that row's ``G``, its ``td_error`` and the critic losses;
* the critic half (``q*``, ``target_q*``, ``next_log_prob``, ``reward``, ``done``, ``weight``) and the actor half
  (``log_prob``, ``new_q*``) may each be used alone, for learners that update the critic before they evaluate the actor:
  :func:`sac_continuous_critic_loss` and :func:`sac_continuous_policy_loss`.  The outputs of the absent half are ``None``;
* fp32 contiguous GPU tensors, ``1 <= A <= 1024``.

The temperature loss of continuous SAC is :func:`sac_alpha_loss` of :mod:`hpc_rll.rl_utils.sac`, re-exported here without a
kernel: with ``entropy = -mean(log_prob)`` it is DI-engine's ``-(log_alpha * (log_prob + target_entropy).detach()).mean()``.

One deviation from DI-engine: ``log_prob`` is formed from ``u``, never from the rounded ``a``, where DI-engine takes
``log(1 - a^2 + 1e-6)``.  In fp32 ``a`` is exactly +-1 from ``|u|`` of about 9, where ``log(1 - a^2)`` would be ``-inf``.  The
two agree to ``1e-6 / (1 - tanh(u)^2)`` per dimension (1.0e-4 at ``|u| = 3``) and part completely once ``1 - a^2 < 1e-6``."""
from collections import namedtuple

import torch

import hpc_sac
from hpc_rll import dist as _dp
from hpc_rll.rl_utils.sac import sac_alpha_loss  # noqa: F401  (re-exported: the continuous temperature loss is the same)

sac_continuous_output = namedtuple('sac_continuous_output', ['policy_loss', 'critic_loss', 'twin_critic_loss', 'entropy',
                                                             'td_error', 'target_q'])


def tanh_gaussian_rsample(mu, sigma, eps=None):
    """``(action, log_prob)`` of the tanh-squashed Gaussian ``tanh(mu + sigma * eps)``: ``action`` has the shape of ``mu``,
    ``log_prob`` its leading shape.  ``eps=None`` draws ``torch.randn_like(mu)``.  The gradient flows to ``mu`` and ``sigma``
    from both outputs; each is formed only when its tensor requires it."""
    if eps is None:
        eps = torch.randn_like(mu)
    action, log_prob = hpc_sac.tanh_gaussian_rsample(mu, sigma, eps)
    return action, log_prob


def _call(q1, q2, target_q1, target_q2, next_log_prob, reward, done, weight, log_prob, new_q1, new_q2, alpha, gamma, scale):
    a_t = alpha if isinstance(alpha, torch.Tensor) else None
    out = hpc_sac.sac_continuous(q1, q2, target_q1, target_q2, next_log_prob, reward, done, weight, log_prob, new_q1, new_q2,
                                 0.0 if a_t is not None else float(alpha), a_t, gamma, scale)
    return list(out)


def _pack(out, critic, actor, twin):
    return sac_continuous_output(out[0] if actor else None, out[1] if critic else None, out[2] if critic and twin else None,
                                 out[3] if actor else None, out[4] if critic else None, out[5] if critic else None)


def sac_continuous_loss(q1, q2, target_q1, target_q2, next_log_prob, reward, log_prob, new_q1, new_q2, done=None, weight=None,
                        alpha=0.2, gamma: float = 0.99):
    """The continuous SAC losses of one batch: a :data:`sac_continuous_output` ``(policy_loss, critic_loss, twin_critic_loss,
    entropy, td_error, target_q)``.  The first four are (1,) tensors (``twin_critic_loss`` is ``None`` for a single critic),
    ``td_error`` and ``target_q`` have the shape of ``reward``; ``entropy``, ``td_error`` and ``target_q`` carry no gradient.
    The gradient flows to ``q1`` (from ``critic_loss``), ``q2`` (from ``twin_critic_loss``), ``log_prob``, ``new_q1`` and
    ``new_q2`` (from ``policy_loss``); each is formed only when its tensor requires it."""
    if q1 is None or log_prob is None:
        raise RuntimeError("sac_continuous_loss: q1 and log_prob are required; for one half alone use "
                           "sac_continuous_critic_loss or sac_continuous_policy_loss")
    out = _call(q1, q2, target_q1, target_q2, next_log_prob, reward, done, weight, log_prob, new_q1, new_q2, alpha, gamma, None)
    return _pack(out, True, True, q2 is not None)


def sac_continuous_critic_loss(q1, q2, target_q1, target_q2, next_log_prob, reward, done=None, weight=None, alpha=0.2,
                               gamma: float = 0.99):
    """The critic half alone: ``critic_loss``, ``twin_critic_loss``, ``td_error`` and ``target_q`` of a
    :data:`sac_continuous_output`; ``policy_loss`` and ``entropy`` are ``None``."""
    if q1 is None:
        raise RuntimeError("sac_continuous_critic_loss: q1 is required")
    out = _call(q1, q2, target_q1, target_q2, next_log_prob, reward, done, weight, None, None, None, alpha, gamma, None)
    return _pack(out, True, False, q2 is not None)


def sac_continuous_policy_loss(log_prob, new_q1, new_q2, alpha=0.2):
    """The actor half alone: ``policy_loss`` and ``entropy`` of a :data:`sac_continuous_output`; the other four are ``None``."""
    if log_prob is None:
        raise RuntimeError("sac_continuous_policy_loss: log_prob is required")
    out = _call(None, None, None, None, None, None, None, None, log_prob, new_q1, new_q2, alpha, 0.0, None)
    return _pack(out, False, True, new_q2 is not None)


class SACContinuous(torch.nn.Module):
    """Module form of :func:`sac_continuous_loss`, with the data-parallel option of
    :class:`hpc_rll.rl_utils.sac.SACDiscrete`: ``sharded=True`` splits the rows over the ranks; each rank scales with
    1/(global rows) and the four scalars are summed with one all-reduce of one packed tensor.  ``td_error`` and ``target_q``
    are per sample and stay local."""

    def __init__(self, sharded: bool = False, group=None):
        super().__init__()
        self.sharded, self.group = sharded, group

    def forward(self, q1, q2, target_q1, target_q2, next_log_prob, reward, log_prob, new_q1, new_q2, done=None, weight=None,
                alpha=0.2, gamma: float = 0.99):
        if q1 is None or log_prob is None:
            raise RuntimeError("SACContinuous: q1 and log_prob are required")
        scale = _dp.loss_scale(reward.numel(), self.group, True) if self.sharded else None
        out = _call(q1, q2, target_q1, target_q2, next_log_prob, reward, done, weight, log_prob, new_q1, new_q2, alpha, gamma,
                    scale)
        if self.sharded:
            packed = _dp.all_reduce_losses_(torch.cat([t.detach() for t in out[:4]]), self.group, True)   # one all-reduce
            for i, t in enumerate(out[:4]):
                t.detach().copy_(packed[i:i + 1])
        return _pack(out, True, True, q2 is not None)
