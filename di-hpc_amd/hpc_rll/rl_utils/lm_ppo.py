"""``hpc_rll.rl_utils.lm_ppo`` -- token-level PPO for language models, the critic half of LM fine-tuning next to
``hpc_rll.rl_utils.grpo``: the per-token log-probability AND entropy over a large vocabulary from one read of the logits, GAE
on the ``(B,S)`` layout under a response mask, and the clipped token loss with value loss and entropy (no reference
counterpart; the semantics are those of TRL's and OpenRLHF's PPO trainers).

``logits`` are ``(B,S,V)``, float32 or bfloat16, ``1 <= V <= 262144``, read in their own dtype; everything per token is float32.

:func:`token_log_prob_entropy` -- per lane an online triple ``(m, s = sum e^(x-m), u = sum e^(x-m) (x-m))``; then
``lse = m + ln s``, ``logp = x[a] - lse``, ``H = ln s - u/s``.  Both outputs are differentiable::

    grad[r,v] = g_lp[r] ([v = a] - p_v) - g_H[r] p_v (x_v - lse + H)

written by one streaming launch in the logits' dtype (bfloat16: rounded to nearest even); ``lse`` and ``H`` (8 bytes per
token) are what is kept for it, not a ``(B,S,V)`` softmax.

:func:`lm_gae` -- the live tokens ``j_1 < ... < j_L`` of a sequence (``w != 0``) are its trajectory, dropped ones are skipped::

    r_i = reward_i - beta kl_i          delta_i = r_i + gamma V_{i+1} - V_i          V_{L+1} = A_{L+1} = 0
    A_i = delta_i + gamma lam A_{i+1}   ret_i = A_i + V_i
    whiten: adv = (A - mu) rsqrt(var + 1e-8), mu and the biased var over all n live tokens of the batch

``reward`` is ``(B,S)``, or ``(B,)``: a terminal score credited to the last live token (the number of dimensions decides).
For a contiguous response mask (prompt left, padding right) this equals TRL's / OpenRLHF's loop over zero-masked entries; for a
mask with holes it deliberately does not (deviation: they feed ``V = 0`` into the recurrence at a hole, here the hole is
skipped).  ``n = 0`` gives zeros, ``n = 1`` with ``whiten`` gives ``adv = 0``.  No gradient.

:func:`lm_ppo_loss` -- per live token, with ``pn``, ``H`` from the head::

    r = exp(pn - po)   rc = clamp(r, 1 - eps, 1 + eps)   l = max(-A r, -A rc)
    dual_clip = c > 1 and A < 0:  l = min(l, -c A)
    dl/dpn = -A r where the unclipped term is the maximum (a tie counts as unclipped) and the dual clip is not active, else 0
    lv = max((v - ret)^2, (vc - ret)^2) / 2,  vc = v_old + clamp(v - v_old, -value_clip, value_clip)   (value_clip=None: plain)

aggregated with ``agg='token'``: ``sum w x / sum w`` over the batch, or ``agg='sequence'``: GRPO's
``1/B sum_b (sum_s w x / sum_s w)``.  Returns ``lm_ppo_output(policy_loss, value_loss, entropy)``, each ``(1,)`` and each
differentiable (the caller forms ``policy_loss + c_v value_loss - c_e entropy``), ``value_loss`` ``None`` without value
operands, and ``lm_ppo_info(approx_kl, mean_ratio, clipfrac)``, detached: the aggregates of ``(r - 1) - log r``, ``r`` and
``[r outside 1 +- eps]``.

Conventions (those of ``grpo``):

* ``weight=None`` gives the bits of all-ones;
* a token with ``w == 0``, or (head and loss) with an ``action`` outside ``[0, V)`` (so ``-100`` works as an ignore index), is
  dropped by selection: it adds nothing to any sum, its outputs are 0, its gradient row is exact zeros and its operands are not
  used -- they may hold anything, NaN included;
* a sequence without weight contributes 0 and still counts in ``B``; ``sum w = 0`` gives zeros;
* ``-inf`` logits are masked vocabulary entries of probability 0, they add exactly 0 to the entropy; NaN in the logits of a
  LIVE token is clamped like ``-inf``;
* ``B``, ``S`` or ``V`` of size 0 gives zeros and launches nothing;
* contiguous GPU tensors;
* nothing in the op synchronises with the host, so a learner step can be captured with ``hpc_rll.graphed``.

Out of scope: fusing the LM head's matrix product, a reference-policy KL inside the loss (it goes into the reward through
``kl``; ``grpo`` has the in-loss form), ``old`` given as logits, bootstrapping a truncated sequence with a nonzero
``V_{L+1}``, whitening statistics across ranks (use ``whiten=False``), float16, vocabularies split over ranks."""
from collections import namedtuple

import torch

import hpc_rl_utils
from hpc_rll import dist as _dp

lm_ppo_output = namedtuple("lm_ppo_output", ["policy_loss", "value_loss", "entropy"])
lm_ppo_info = namedtuple("lm_ppo_info", ["approx_kl", "mean_ratio", "clipfrac"])

_AGG = ("token", "sequence")


def token_log_prob_entropy(logits, action, weight=None):
    """``(logp, entropy)``, each ``(...)`` float32, from ``(..., V)`` logits and ``(...)`` int64 actions in one read of the
    logits.  A row with ``weight == 0`` or an ``action`` outside ``[0, V)`` is not read and gives ``logp = entropy = 0``."""
    logp, ent = hpc_rl_utils.token_log_prob_entropy(logits, action, weight)
    return logp, ent


def lm_gae(value, weight, reward, kl=None, beta: float = 0.0, gamma: float = 1.0, lam: float = 0.95, whiten: bool = True):
    """``(adv, ret)``, each ``(B,S)``; dropped positions are exact zeros.  ``ret`` comes from the unwhitened advantage."""
    return hpc_rl_utils.lm_gae(value, weight, reward, kl, beta, gamma, lam, whiten)


def _check_agg(agg):
    if agg not in _AGG:
        raise ValueError(f"agg: expected 'token' or 'sequence', got {agg!r}")
    return agg == "sequence"


def lm_ppo_loss(logit_new, old_logp, action, adv, weight=None, value_new=None, value_old=None, ret=None,
                clip_ratio: float = 0.2, dual_clip=None, value_clip=0.2, agg: str = "token"):
    """``(lm_ppo_output, lm_ppo_info)``.  The gradient flows to ``logit_new`` (in its own dtype) and ``value_new`` and is formed
    only for the one that requires it."""
    p, v, e, kl, ratio, clipfrac, _ = hpc_rl_utils.lm_ppo_loss(logit_new, old_logp, action, adv, weight, value_new, value_old,
                                                               ret, clip_ratio, dual_clip, value_clip, _check_agg(agg), False)
    return lm_ppo_output(p, v if value_new is not None else None, e), lm_ppo_info(kl, ratio, clipfrac)


class LMPPO(torch.nn.Module):
    """Module form of :func:`lm_ppo_loss`.  ``sharded=True`` splits ``B`` over the ranks: every rank forms the numerators of
    its shard, ONE all-reduce of one packed tensor carries them and, in ``'token'`` mode, ``sum w``; losses and gradients
    equal the unsharded call on the concatenated batch.  ``info`` is per rank and stays local."""

    def __init__(self, sharded: bool = False, group=None, agg: str = "token"):
        super().__init__()
        _check_agg(agg)
        self.sharded, self.group, self.agg = sharded, group, agg

    def forward(self, logit_new, old_logp, action, adv, weight=None, value_new=None, value_old=None, ret=None,
                clip_ratio: float = 0.2, dual_clip=None, value_clip=0.2):
        if not self.sharded:
            return lm_ppo_loss(logit_new, old_logp, action, adv, weight, value_new, value_old, ret, clip_ratio, dual_clip,
                               value_clip, self.agg)
        seq = self.agg == "sequence"
        scale = _dp.loss_scale(action.shape[0], self.group, True) if seq else None
        p, v, e, kl, ratio, clipfrac, den = hpc_rl_utils.lm_ppo_loss(logit_new, old_logp, action, adv, weight, value_new,
                                                                     value_old, ret, clip_ratio, dual_clip, value_clip, seq,
                                                                     True, scale)
        local = torch.where(den != 0, den, torch.ones_like(den))
        ws = _dp.world_size(self.group)
        # 'sequence': the monitors carry 1/(global B); per rank they are means over the local B
        info = lm_ppo_info(*((x * ws if seq else torch.where(den != 0, x / local, torch.zeros_like(x)))
                             for x in (kl, ratio, clipfrac)))
        if seq:
            p, v, e = _dp.all_reduce_sum((p, v, e), self.group)
        else:
            p, v, e, den = _dp.all_reduce_sum((p, v, e, den), self.group)
            inv = torch.where(den != 0, 1.0 / torch.where(den != 0, den, torch.ones_like(den)), torch.zeros_like(den))
            p, v, e = p * inv, v * inv, e * inv
        return lm_ppo_output(p, v if value_new is not None else None, e), info
