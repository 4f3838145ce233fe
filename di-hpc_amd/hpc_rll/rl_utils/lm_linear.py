"""``hpc_rll.rl_utils.lm_linear`` -- the language-model head fused with its bfloat16 matrix product: the per-token
log-probability (and the entropy over the vocabulary) of given tokens straight from the hidden states and the head's weight,
without a ``(..., V)`` logits tensor (no reference counterpart).

Two functions, one per kind of policy in an RLHF step:

* ``linear_token_log_prob`` serves the operands evaluated WITHOUT gradient, the old and the reference policy: their log-probs
  are what ``hpc_rll.rl_utils.grpo.grpo_policy_loss`` and ``hpc_rll.rl_utils.lm_ppo.lm_ppo_loss`` take as ``(B,S)`` tensors;
* ``lm_head_log_prob`` serves the policy BEING TRAINED: the same forward, and a backward that gives ``hidden.grad`` and
  ``lm_weight.grad`` without a ``(..., V)`` tensor either.

With ``x = (hidden @ lm_weight.T) / temperature`` held in the float32 accumulators of the matrix instructions (never rounded to
bfloat16, never written to memory)::

    logp    = x[a] - logsumexp(x)
    entropy = logsumexp(x) - sum_v p_v x_v

``hidden`` is ``(..., H)`` bfloat16, ``lm_weight`` ``(V, H)`` bfloat16 (``nn.Linear.weight``'s own layout, passed as it is),
``action`` ``(...)`` int64, ``weight`` ``(...)`` float32 or ``None``; ``32 <= H <= 16384`` with ``H % 32 == 0``,
``1 <= V <= 262144``, ``temperature > 0``, any number of rows (offsets are 64-bit).

Conventions, those of ``grpo`` and ``lm_ppo``:

* ``weight=None`` gives the bits of all-ones;
* a row with ``weight == 0``, or with an ``action`` outside ``[0, V)`` (so ``-100`` works as an ignore index), is dropped:
  ``logp = entropy = 0``, its gradient towards ``hidden`` is exactly 0, and whatever its ``hidden`` holds, NaN included,
  touches no other row and no entry of ``lm_weight.grad``;
* no rows gives empty tensors and launches nothing (the gradients are then zeros);
* contiguous GPU tensors whose bases lie on 16 bytes; nothing synchronises with the host;
* ``linear_token_log_prob`` has NO gradient: under grad mode an operand that requires grad is a ``RuntimeError`` that names
  ``torch.no_grad()`` -- a gradient is never dropped silently.

The gradient.  Per live row, with ``p_v = exp(x_v - lse)``, ``H`` the row's entropy and the upstream ``gl``, ``ge``::

    g_v     = (gl (1[v = a] - p_v) - ge p_v (log p_v + H)) / temperature
    dhidden = G @ lm_weight          dW = G.T @ hidden

The backward walks the vocabulary in chunks (the forward saves ``lse``, which makes them independent): a chunk's logits are
recomputed with the forward's product, ``g`` is formed on the float32 accumulators and rounded to bfloat16 once, and ONE
bfloat16 matrix kernel forms both products.  ``dhidden`` is accumulated in float32 across chunks and rounded once; a chunk's
rows of ``dW`` are written once.  The workspace is ``G`` and ``G.T`` of one chunk -- chosen so that they stay within 256 MiB
together, a constant that has not been measured -- plus ``rows x H`` float32 when there is more than one chunk.  An operand
that does not require grad costs neither its product nor its workspace (a frozen head, LoRA).  The same bits on every run.

Out of scope: float32 and float16 operands, a bias, logit soft-capping, compaction of the live rows, vocabularies or rows
split over ranks, capture into a graph, and loss functions that take a differentiable ``(B,S)`` ``logp`` (until then the loss
on top of ``lm_head_log_prob`` is a few elementwise torch operations)."""
import hpc_lm_linear


def linear_token_log_prob(hidden, lm_weight, action, weight=None, temperature: float = 1.0, return_entropy: bool = False):
    """``logp`` ``(...)`` float32, or ``(logp, entropy)`` with ``return_entropy=True``, of the tokens ``action`` under the head
    ``lm_weight`` applied to ``hidden``, WITHOUT gradient: for the old and the reference policy (the policy being trained takes
    ``lm_head_log_prob``).  Two launches whatever the sizes: the fused product with the online softmax statistic over
    vocabulary splits, and the merge of the splits in a fixed order (the same bits on every run)."""
    out = hpc_lm_linear.linear_token_log_prob(hidden, lm_weight, action, weight, float(temperature), bool(return_entropy))
    return (out[0], out[1]) if return_entropy else out[0]


def lm_head_log_prob(hidden, lm_weight, action, weight=None, temperature: float = 1.0, return_entropy: bool = False):
    """``linear_token_log_prob`` for the policy BEING TRAINED: the same values (the same kernels, the same bits), differentiable
    towards ``hidden`` and ``lm_weight``.  Their gradients are bfloat16 and only those of the operands that require grad are
    computed; with grad mode off, or neither operand requiring grad, this is the plain forward.  The old and the reference
    policy take ``linear_token_log_prob``."""
    out = hpc_lm_linear.lm_head_log_prob(hidden, lm_weight, action, weight, float(temperature), bool(return_entropy))
    return (out[0], out[1]) if return_entropy else out[0]
