"""``hpc_rll.rl_utils.lm_policy`` -- the policy losses of language-model RL on per-token LOG-PROBABILITIES (no reference
counterpart): what consumes the differentiable ``(B,S)`` ``logp`` (and entropy) of
``hpc_rll.rl_utils.lm_linear.lm_head_log_prob``, so that a step that never materialises logits does not fall back to eager
torch for its loss.  ``grpo_policy_loss`` and ``lm_ppo_loss`` take ``logit_new (B,S,V)``; this op has no vocabulary axis.

``lm_policy_loss(logp, old_logp, adv, weight=None, ref_logp=None, entropy=None, value_new=None, value_old=None, ret=None, *,
ratio="token", objective="clip", clip_low=0.2, clip_high=0.2, dual_clip=None, kl="k3", agg="token", norm_len=None,
value_clip=0.2)`` returns ``(lm_policy_output(policy_loss, kl_loss, value_loss, entropy), lm_policy_info(approx_kl, mean_ratio,
clipfrac, mean_kl))``, every entry ``(1,)``.  All tensors are float32, contiguous, on the GPU; all are ``(B,S)`` except ``adv``,
which is ``(B,)`` or ``(B,S)`` (the number of dimensions decides, as ``lm_gae``'s ``reward``).

With ``pn = logp``, ``po = old_logp``, ``pr = ref_logp``, ``A = adv``, ``d = pn - po``, ``W_b = sum_s w``,
``lo = 1 - clip_low``, ``hi = 1 + clip_high`` (``clip_high > clip_low`` is DAPO's clip-higher)::

    ratio="token"       r = exp(d)
    ratio="sequence"    r = s_b = exp(sum_s w d / W_b) for every token of the sequence; its derivative with respect to that
                        token's pn is s_b (the GSPO-token form)
    objective="clip"    l = max(-A r, -A rc), rc = clamp(r, lo, hi)
                        dl/dpn = -A r where the unclipped term is the maximum (a tie counts as unclipped), else 0
                        dual_clip = c > 1 and A < 0:  l = min(l, -c A), no gradient where it is active
                        (lm_ppo_loss's rule, with two bounds)
    objective="cispo"   l = -rc A pn with rc detached: dl/dpn = -rc A always; dual_clip must be None
    kl (with ref_logp), e = pr - pn:
        "k1"  k = -e                dk/dpn = 1
        "k2"  k = e^2 / 2           dk/dpn = -e
        "k3"  k = exp(e) - e - 1    dk/dpn = 1 - exp(e)
    value loss          lm_ppo_loss's: lv = max((v - ret)^2, (vc - ret)^2) / 2, vc = v_old + clamp(v - v_old, +-value_clip)
                        (value_clip=None: plain); value_new, value_old and ret are given all three or none
    agg="token"         sum w x / sum w                      (divided on the device)
    agg="sequence"      1/B sum_b (sum_s w x / W_b)
    agg="constant"      sum w x / (B norm_len)               (Dr. GRPO; norm_len is required and positive here, refused otherwise)

Identity: ``ratio="sequence"`` with ``adv (B,)`` and ``agg="sequence"`` is GSPO -- the value is
``1/B sum_b max(-A_b s_b, -A_b clamp(s_b, lo, hi))`` and the gradient is the one autograd gives that per-sequence loss, since
``d s_b / d pn_t = s_b w_t / W_b``.

``kl_loss`` is the aggregate of ``k`` (``None`` without ``ref_logp``); ``mean_kl`` is the same number, detached (0 without
``ref_logp``); the caller forms ``policy_loss + beta * kl_loss``.  ``value_loss`` is ``None`` without value operands;
``entropy`` is the aggregate of the given entropy, differentiable into it (0 when none is given).  ``info`` holds the
aggregates, under the same ``agg``, of ``(r - 1) - log r``, ``r`` and ``[r > hi or r < lo]``.

The gradient flows to ``logp``, ``entropy`` and ``value_new``, each formed only when that operand requires it; each of the four
outputs is differentiable on its own.  One streaming launch writes them from coefficients the forward saved (4 bytes per token
and wanted gradient).

Conventions (those of ``grpo`` and ``lm_ppo``):

* ``weight=None`` gives the bits of all-ones;
* a token with ``w == 0`` is dropped by selection: it adds nothing to any sum, its gradients are exact zeros and its operands
  are not used -- they may hold NaN;
* a sequence without weight contributes 0 and still counts in ``B``; ``sum w = 0`` gives zeros;
* ``B == 0`` or ``S == 0`` gives zeros and launches nothing;
* nothing synchronises with the host, so a step captures with ``hpc_rll.graphed``;
* no float atomics: the same bits on every run.

Two mappings (``csrc/lm_policy.hip``): a wave per sequence for ``S <= 1024`` (a threshold nobody has measured), and above it a
workgroup per (sequence, chunk of 1024 tokens), so that a few very long sequences still fill the device; a split sequence's
totals are summed in one fixed order by every workgroup that needs them.

Out of scope: ``sharded=True``; a truncated-importance-sampling operand (a detached non-negative per-token factor folded into
``adv (B,S)`` gives it for the ``"clip"`` objective); a clamp of the log-ratio; bfloat16 per-token operands."""
from collections import namedtuple

import torch

import hpc_lm_policy

lm_policy_output = namedtuple("lm_policy_output", ["policy_loss", "kl_loss", "value_loss", "entropy"])
lm_policy_info = namedtuple("lm_policy_info", ["approx_kl", "mean_ratio", "clipfrac", "mean_kl"])

RATIOS = {"token": 0, "sequence": 1}
OBJECTIVES = {"clip": 0, "cispo": 1}
KLS = {"k1": 0, "k2": 1, "k3": 2}
AGGS = {"token": 0, "sequence": 1, "constant": 2}


def _code(name, value, table):
    if value not in table:
        raise ValueError(f"{name}: {value!r}, expected one of {sorted(table)}")
    return table[value]


def _options(ratio, objective, clip_low, clip_high, dual_clip, kl, agg, norm_len, value_clip):
    """The keyword options as the extension takes them; string and combination errors are raised here."""
    codes = (_code("ratio", ratio, RATIOS), _code("objective", objective, OBJECTIVES), _code("kl", kl, KLS), _code("agg", agg, AGGS))
    if agg == "constant" and (norm_len is None or not norm_len > 0):
        raise ValueError(f"norm_len: agg='constant' needs a positive value, got {norm_len!r}")
    if agg != "constant" and norm_len is not None:
        raise ValueError(f"norm_len: only agg='constant' takes it, got {norm_len!r}")
    if objective == "cispo" and dual_clip is not None:
        raise ValueError(f"dual_clip: must be None with objective='cispo', got {dual_clip!r}")
    return dict(ratio=codes[0], objective=codes[1], clip_low=float(clip_low), clip_high=float(clip_high), dual_clip=dual_clip,
                kl=codes[2], agg=codes[3], norm_len=norm_len, value_clip=value_clip)


def lm_policy_loss(logp, old_logp, adv, weight=None, ref_logp=None, entropy=None, value_new=None, value_old=None, ret=None, *,
                   ratio: str = "token", objective: str = "clip", clip_low: float = 0.2, clip_high: float = 0.2, dual_clip=None,
                   kl: str = "k3", agg: str = "token", norm_len=None, value_clip=0.2, mapping: int = 0):
    """``(lm_policy_output, lm_policy_info)`` as in the module docstring.  ``mapping``: 0 = by rule, 1 = a wave per sequence,
    2 = a workgroup per (sequence, chunk); the results agree to rounding."""
    opts = _options(ratio, objective, clip_low, clip_high, dual_clip, kl, agg, norm_len, value_clip)
    p, k, v, e, akl, mr, cf = hpc_lm_policy.lm_policy_loss(logp, old_logp, adv, weight, ref_logp, entropy, value_new, value_old, ret,
                                                           mapping=int(mapping), **opts)
    out = lm_policy_output(p, k if ref_logp is not None else None, v if value_new is not None else None, e)
    return out, lm_policy_info(akl, mr, cf, k.detach())


class LMPolicyLoss(torch.nn.Module):
    """Module form of :func:`lm_policy_loss`: the keyword options are fixed at construction, ``forward`` takes the tensors."""

    def __init__(self, ratio: str = "token", objective: str = "clip", clip_low: float = 0.2, clip_high: float = 0.2, dual_clip=None,
                 kl: str = "k3", agg: str = "token", norm_len=None, value_clip=0.2):
        super().__init__()
        _options(ratio, objective, clip_low, clip_high, dual_clip, kl, agg, norm_len, value_clip)
        self.options = dict(ratio=ratio, objective=objective, clip_low=clip_low, clip_high=clip_high, dual_clip=dual_clip, kl=kl,
                            agg=agg, norm_len=norm_len, value_clip=value_clip)

    def forward(self, logp, old_logp, adv, weight=None, ref_logp=None, entropy=None, value_new=None, value_old=None, ret=None):
        return lm_policy_loss(logp, old_logp, adv, weight, ref_logp, entropy, value_new, value_old, ret, **self.options)
