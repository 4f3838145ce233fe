"""``hpc_rll.rl_utils.lm_topk`` -- distillation from a top-k teacher (no reference counterpart).

``token_kl_div`` needs the teacher's whole row of logits; offline and cross-process pipelines keep the teacher's ``k`` largest
log-probabilities and their indices per token instead.  Two ops:

``token_topk(logits, k, weight=None, temperature=1.0) -> (topk_logp, topk_index)``, the producer, on the teacher's side.
``logits`` ``(..., V)`` float32 or bfloat16; ``topk_index`` ``(..., k)`` int32, ``topk_logp`` ``(..., k)`` float32 equal to
``log_softmax(logits / temperature)`` over the WHOLE row at the chosen entries, from the same read of the row as the
selection.  The order is ``torch.sort(stable=True, descending=True)[:k]`` of the row with ``-inf`` and NaN clamped to the
lowest float: the ``k`` largest, descending, equal values (``-0 == +0``) by ascending index; it does not depend on the
temperature.  A chosen entry that was NaN or ``-inf`` carries ``-inf``.  ``1 <= k <= min(V, 256)``.  No gradient: an operand
that requires grad under grad mode is a ``RuntimeError``.

``token_topk_kl_div(logits, topk_index, topk_logp, weight=None, tail="renorm", temperature=1.0) -> kl (...)``, the consumer,
on the student's side.  ``topk_index`` int32 or int64; an entry with an index outside ``[0, V)`` or ``logp == -inf`` is
padding (ragged ``k``); the indices of a token are distinct.  ``temperature`` scales the student only.  With
``p = softmax(logits / T)``, ``q_j = exp(logp_j)``, ``Q = min(sum q_j, 1)`` and ``P = sum_j p[i_j]``::

    tail="renorm"   sum_j (q_j / Q) (log(q_j / Q) - log p[i_j])                the teacher renormalised over its entries
    tail="bucket"   sum_j q_j (logp_j - log p[i_j]) + (1 - Q) (log(1 - Q) - log(1 - P))
                    the KL of the k + 1 outcomes "entries + everything else", a lower bound of the full KL; the student's tail
                    mass 1 - P is summed over the entries outside the set, never formed by subtraction

The gradient flows to ``logits`` only, in their dtype.  One launch each way and no ``(..., V)`` temporary; the forward keeps 12
bytes per token.  No float atomics: the same bits on every run.

Conventions, those of ``lm_kl``: ``weight`` only selects -- a token with ``weight == 0`` is not read (``token_topk``: index -1,
logp ``-inf``; the divergence: value 0, gradient row exact zeros), as is a token without a live entry; ``1 <= V <= 262144``;
contiguous GPU tensors; a base or a row pitch off 16 bytes takes the one-element path of the kernels.

Out of scope: reverse / JSD against a top-k teacher, top-p and sampling, ``k > 256``, fusing the LM head's matrix product."""
import torch

import hpc_lm_topk

TAILS = {"renorm": 0, "bucket": 1}


def token_topk(logits, k: int, weight=None, temperature: float = 1.0):
    """``(topk_logp, topk_index)``, both ``(..., k)``: the ``k`` largest entries of every row of ``logits`` and
    ``log_softmax(logits / temperature)`` at them, as in the module docstring."""
    return hpc_lm_topk.token_topk(logits, int(k), weight, float(temperature))


def token_topk_kl_div(logits, topk_index, topk_logp, weight=None, tail: str = "renorm", temperature: float = 1.0):
    """The divergence of every token, ``(...)`` float32, between a teacher given by its top entries and
    ``softmax(logits / temperature)``; ``tail`` as in the module docstring."""
    if tail not in TAILS:
        raise ValueError(f"tail: {tail!r}, expected one of {sorted(TAILS)}")
    return hpc_lm_topk.token_topk_kl_div(logits, topk_index, topk_logp, weight, TAILS[tail], float(temperature))


class TopKDistillLoss(torch.nn.Module):
    """The distillation loss on top of ``token_topk_kl_div``: its masked mean, taken in torch, with the aggregates of
    ``lm_kl.GKDLoss``.  ``aggregate="token"``: ``sum(mask * kl) / sum(mask)`` over the batch; ``"sequence"``: the mean over the
    sequences (all dimensions but the last) of each sequence's masked mean.  A zero denominator gives 0."""

    def __init__(self, tail: str = "renorm", temperature: float = 1.0, aggregate: str = "token"):
        super().__init__()
        if tail not in TAILS:
            raise ValueError(f"tail: {tail!r}, expected one of {sorted(TAILS)}")
        if aggregate not in ("token", "sequence"):
            raise ValueError(f"aggregate: {aggregate!r}, expected 'token' or 'sequence'")
        self.tail, self.temperature, self.aggregate = tail, float(temperature), aggregate

    def forward(self, logits, topk_index, topk_logp, mask=None):
        kl = token_topk_kl_div(logits, topk_index, topk_logp, mask, self.tail, self.temperature)
        w = torch.ones_like(kl) if mask is None else mask
        if self.aggregate == "token":
            num, den = (w * kl).sum(), w.sum()
            return num / torch.where(den != 0, den, torch.ones_like(den))
        num, den = (w * kl).sum(-1), w.sum(-1)
        return (num / torch.where(den != 0, den, torch.ones_like(den))).mean()
