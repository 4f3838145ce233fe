"""``hpc_rll.rl_utils.grpo`` -- the language-model policy losses: the per-token log-probability of the chosen token over a
large vocabulary, and GRPO's clipped-ratio + k3-KL token loss with per-sequence masked means (no reference counterpart; the
formulas restate DI-engine's ``grpo_policy_error`` / ``rloo_policy_error`` and the ``log_prob_utils`` helper they share).

``logit_new`` is ``(B,S,V)``, float32 or bfloat16, ``1 <= V <= 262144``; ``old`` and ``ref`` are each either logits
``(B,S,V)`` (float32 or bfloat16, independently) or per-token log-probs ``(B,S)`` float32 -- the number of dimensions decides;
``ref`` may be ``None``: no KL term, ``mean_kl = 0`` and ``beta`` is ignored (RLOO / token-level PPO); ``action`` ``(B,S)``
int64, ``adv`` ``(B,)``, ``weight`` ``(B,S)`` or ``None``.  Per token, with ``lp(x) = x[a] - logsumexp(x)``::

    pn = lp(logit_new)   po = lp(old) or old   pr = lp(ref) or ref
    d  = pr - pn         kl = exp(d) - d - 1
    r  = exp(pn - po)    rc = clamp(r, 1 - clip, 1 + clip)
    l  = -min(r adv_b, rc adv_b) + beta kl
    loss = 1/B sum_b ( sum_s w l / sum_s w )
    dl/dpn = -adv_b r [the clipped term is not strictly smaller] - beta (exp(d) - 1)
    grad_logit_new[b,s,v] = g w / (B sum_s w) dl/dpn ([v = a] - exp(x_v - lse))
    info: sum w x / sum w over all tokens, for x = kl, r, [r > 1 + clip or r < 1 - clip]

The logits are read once per launch in their own dtype (no float32 copy of a bfloat16 tensor is made) and the gradient is
written once, in ``logit_new``'s dtype (bfloat16: rounded to nearest even).  What is kept for the backward is ``logit_new``
itself, ``action`` and the per-token workspace (``lse`` and the coefficient), not a ``(B,S,V)`` softmax.

Conventions:

* ``weight=None`` gives the bits of all-ones;
* a token with ``w == 0``, or with an ``action`` outside ``[0, V)`` (so ``-100`` works as an ignore index), is dropped by
  selection: it adds nothing to any sum, its gradient row is exact zeros and its logits are not read -- they may hold
  anything, NaN included;
* a sequence with ``sum_s w = 0`` contributes 0 and still counts in ``B`` (deviation: DI-engine gives NaN there);
* ``info`` holds weight-masked means (deviation: DI-engine takes plain means, which are the same when ``weight=None``);
* ``-inf`` logits are masked vocabulary entries of probability 0; a chosen token whose own logit is ``-inf`` is not supported;
* NaN in the logits of a LIVE token is not propagated: it is clamped like ``-inf`` and counts with probability 0, so a
  diverged model gives a finite loss here (check the logits themselves if that matters);
* ``B``, ``S`` or ``V`` of size 0 gives a zero loss and launches nothing;
* contiguous GPU tensors.

Out of scope: fusing the LM head's matrix product, in-place gradients, float16, and vocabularies split over ranks (tensor
parallelism).  The entropy over the vocabulary is not formed here: ``hpc_rll.rl_utils.lm_ppo.token_log_prob_entropy`` gives it
with the log-probability from the same single read of the logits, and ``lm_ppo_loss`` is the token-level PPO loss on top."""
from collections import namedtuple

import torch

import hpc_rl_utils
from hpc_rll import dist as _dp

grpo_policy_data = namedtuple("grpo_policy_data", ["logit_new", "logit_old", "logit_ref", "action", "adv", "weight"])
grpo_policy_loss_t = namedtuple("grpo_policy_loss", ["policy_loss"])
grpo_info = namedtuple("grpo_info", ["mean_kl", "mean_ratio", "mean_clipped"])
rloo_policy_data = namedtuple("rloo_policy_data", ["logit_new", "logit_old", "action", "reward", "weight"])


def token_log_prob(logits, action):
    """``logits[..., a] - logsumexp(logits)`` per token: ``(..., V)`` float32 or bfloat16 logits and ``(...)`` int64 actions
    give ``(...)`` float32.  Differentiable in ``logits`` (the gradient has their dtype).  An ``action`` outside ``[0, V)``
    gives 0 and a zero gradient row, and its logits are not read (NaN there is harmless)."""
    return hpc_rl_utils.token_log_prob(logits, action)


def grpo_policy_loss(logit_new, old, ref, action, adv, weight=None, clip_ratio: float = 0.2, beta: float = 0.1):
    """``(loss (1,), info)`` with ``info = grpo_info(mean_kl, mean_ratio, mean_clipped)``, detached ``(1,)`` tensors.  The
    gradient flows to ``logit_new`` only, in its own dtype, and is formed only when ``logit_new`` requires it.  Dropped tokens
    (``w == 0`` or an ``action`` outside ``[0, V)``) may hold NaN; a sequence without weight contributes 0."""
    loss, kl, ratio, clipped = hpc_rl_utils.grpo_policy_loss(logit_new, old, ref, action, adv, weight, clip_ratio, beta)
    return loss, grpo_info(kl, ratio, clipped)


def grpo_policy_error(data, clip_ratio: float = 0.2, beta: float = 0.1):
    """DI-engine's form: ``data`` is a ``grpo_policy_data``; returns ``(grpo_policy_loss(policy_loss), grpo_info(...))``."""
    loss, info = grpo_policy_loss(data.logit_new, data.logit_old, data.logit_ref, data.action, data.adv, data.weight,
                                  clip_ratio, beta)
    return grpo_policy_loss_t(loss), info


def rloo_policy_error(data, clip_ratio: float = 0.2):
    """DI-engine's RLOO form (``rloo_policy_data``; ``reward`` ``(B,)`` takes the place of the advantage): the same call
    without a reference policy."""
    loss, info = grpo_policy_loss(data.logit_new, data.logit_old, None, data.action, data.reward, data.weight, clip_ratio, 0.0)
    return grpo_policy_loss_t(loss), info


class GRPO(torch.nn.Module):
    """Module form of :func:`grpo_policy_loss`, with the data-parallel option of :class:`hpc_rll.rl_utils.r2d2.R2D2TD`:
    ``sharded=True`` splits ``B`` over the ranks; each rank scales with 1/(global B) and the loss is summed with one
    all-reduce.  ``info`` is per rank and stays local."""

    def __init__(self, B, S, V, sharded: bool = False, group=None):
        super().__init__()
        self.B, self.S, self.V, self.sharded, self.group = B, S, V, sharded, group

    def forward(self, logit_new, old, ref, action, adv, weight=None, clip_ratio: float = 0.2, beta: float = 0.1):
        scale = _dp.loss_scale(action.shape[0], self.group, True) if self.sharded else None
        loss, kl, ratio, clipped = hpc_rl_utils.grpo_policy_loss(logit_new, old, ref, action, adv, weight, clip_ratio, beta,
                                                                 scale)
        if self.sharded:
            _dp.all_reduce_losses_(loss.detach(), self.group, True)
        return loss, grpo_info(kl, ratio, clipped)
