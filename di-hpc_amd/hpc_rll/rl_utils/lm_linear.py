"""``hpc_rll.rl_utils.lm_linear`` -- the language-model head fused with its bfloat16 matrix product: the per-token
log-probability (and the entropy over the vocabulary) of given tokens straight from the hidden states and the head's weight,
without a ``(..., V)`` logits tensor (no reference counterpart).

It serves the operands an RLHF step evaluates WITHOUT gradient, the old and the reference policy: their log-probs are what
``hpc_rll.rl_utils.grpo.grpo_policy_loss`` and ``hpc_rll.rl_utils.lm_ppo.lm_ppo_loss`` take as ``(B,S)`` tensors.  With
``x = (hidden @ lm_weight.T) / temperature`` held in the float32 accumulators of the matrix instructions (never rounded to
bfloat16, never written to memory)::

    logp    = x[a] - logsumexp(x)
    entropy = logsumexp(x) - sum_v p_v x_v

``hidden`` is ``(..., H)`` bfloat16, ``lm_weight`` ``(V, H)`` bfloat16 (``nn.Linear.weight``'s own layout, passed as it is),
``action`` ``(...)`` int64, ``weight`` ``(...)`` float32 or ``None``; ``32 <= H <= 16384`` with ``H % 32 == 0``,
``1 <= V <= 262144``, ``temperature > 0``, any number of rows (offsets are 64-bit).

Conventions, those of ``grpo`` and ``lm_ppo``:

* ``weight=None`` gives the bits of all-ones;
* a row with ``weight == 0``, or with an ``action`` outside ``[0, V)`` (so ``-100`` works as an ignore index), is dropped:
  ``logp = entropy = 0``, and whatever its ``hidden`` holds, NaN included, touches no other row;
* no rows gives empty tensors and launches nothing;
* contiguous GPU tensors whose bases lie on 16 bytes; nothing synchronises with the host;
* NO gradient: under grad mode an operand that requires grad is a ``RuntimeError`` that names ``torch.no_grad()`` -- a
  gradient is never dropped silently.

Out of scope: the gradient with respect to ``hidden`` and ``lm_weight`` (the differentiable policy still goes through its
logits and ``token_log_prob`` / ``grpo_policy_loss`` / ``lm_ppo_loss``), float32 and float16 operands, a bias, logit
soft-capping, and vocabularies or rows split over ranks."""
import hpc_lm_linear


def linear_token_log_prob(hidden, lm_weight, action, weight=None, temperature: float = 1.0, return_entropy: bool = False):
    """``logp`` ``(...)`` float32, or ``(logp, entropy)`` with ``return_entropy=True``, of the tokens ``action`` under the head
    ``lm_weight`` applied to ``hidden``.  Two launches whatever the sizes: the fused product with the online softmax statistic
    over vocabulary splits, and the merge of the splits in a fixed order (the same bits on every run)."""
    out = hpc_lm_linear.linear_token_log_prob(hidden, lm_weight, action, weight, float(temperature), bool(return_entropy))
    return (out[0], out[1]) if return_entropy else out[0]
