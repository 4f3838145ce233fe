"""``hpc_rll.rl_utils.lm_kl`` -- the exact divergence over the whole vocabulary between two sets of logits, per token, for
on-policy distillation / GKD, a full-KL penalty in place of the k3 estimate of ``grpo_policy_loss``, and KL-to-reference
monitors (no reference counterpart).

``logits`` (the student, ``x``) and ``teacher_logits`` (``y``) are ``(..., V)``, both float32 or both bfloat16.  With
``p = softmax(x / T)``, ``q = softmax(y / T)``::

    mode="forward"   KL(q || p) = sum_v q_v (log q_v - log p_v)             teacher-weighted (mass covering)
    mode="reverse"   KL(p || q) = sum_v p_v (log p_v - log q_v)             student-weighted (mode seeking)
    mode="jsd"       beta KL(q || m) + (1 - beta) KL(p || m),  m = beta q + (1 - beta) p,  0 < beta < 1   (TRL's GKD convention)

The result is float32 with the leading shape of the logits.  The gradient flows to ``logits`` only, in their dtype; a teacher
that requires grad is a ``RuntimeError`` (detach it, or compute it under ``torch.no_grad()``).

One launch forward, one backward, no ``(..., V)`` temporary: the forward reads both rows once (``jsd``: twice -- the mixture
needs both ``logsumexp`` first) and keeps 12 bytes per token (``jsd``: 16) for the backward, which re-reads both rows and
writes the gradient.  No atomics: the same bits on every run.

Conventions, those of ``grpo`` and ``lm_ppo``:

* ``weight`` ``(...)`` float32 or ``None`` only selects: a token with ``weight == 0`` is not read, its value is 0, its gradient
  row exact zeros, and whatever its logits hold, NaN included, touches nothing else.  The value is NOT multiplied by the weight;
* ``-inf`` entries are masked entries.  One that is ``-inf`` in both rows contributes exactly nothing and gets gradient
  exactly 0.  An entry that one policy gives probability 0 and the other weights makes the divergence ``+inf`` mathematically;
  the op then returns some non-NaN number, and avoiding the case is the caller's;
* ``1 <= V <= 262144``, ``temperature > 0``; no tokens gives an empty result and launches nothing;
* contiguous GPU tensors; a base or a row pitch off 16 bytes takes the one-element path of the kernels.

Out of scope: mixed element types, different vocabularies, and fusing the LM head's matrix product.  A teacher kept as its top-k
log-probabilities and indices is served by ``hpc_rll.rl_utils.lm_topk``."""
import torch

import hpc_lm_kl

MODES = {"forward": 0, "reverse": 1, "jsd": 2}


def token_kl_div(logits, teacher_logits, weight=None, mode: str = "forward", beta: float = 0.5, temperature: float = 1.0):
    """The divergence of every token, ``(...)`` float32, between ``softmax(logits / temperature)`` and
    ``softmax(teacher_logits / temperature)``; ``mode`` as in the module docstring, ``beta`` only for ``"jsd"``."""
    if mode not in MODES:
        raise ValueError(f"mode: {mode!r}, expected one of {sorted(MODES)}")
    return hpc_lm_kl.token_kl_div(logits, teacher_logits, weight, MODES[mode], float(beta), float(temperature))


class GKDLoss(torch.nn.Module):
    """The distillation loss on top of ``token_kl_div``: its masked mean, taken in torch.  ``aggregate="token"``:
    ``sum(mask * kl) / sum(mask)`` over the batch; ``"sequence"``: the mean over the sequences (all dimensions but the last) of
    each sequence's masked mean, a sequence without mask counting as 0.  A zero denominator gives 0."""

    def __init__(self, mode: str = "jsd", beta: float = 0.5, temperature: float = 1.0, aggregate: str = "token"):
        super().__init__()
        if mode not in MODES:
            raise ValueError(f"mode: {mode!r}, expected one of {sorted(MODES)}")
        if aggregate not in ("token", "sequence"):
            raise ValueError(f"aggregate: {aggregate!r}, expected 'token' or 'sequence'")
        self.mode, self.beta, self.temperature, self.aggregate = mode, float(beta), float(temperature), aggregate

    def forward(self, logits, teacher_logits, mask=None):
        kl = token_kl_div(logits, teacher_logits, mask, self.mode, self.beta, self.temperature)
        w = torch.ones_like(kl) if mask is None else mask
        if self.aggregate == "token":
            num, den = (w * kl).sum(), w.sum()
            return num / torch.where(den != 0, den, torch.ones_like(den))
        num, den = (w * kl).sum(-1), w.sum(-1)
        return (num / torch.where(den != 0, den, torch.ones_like(den))).mean()
