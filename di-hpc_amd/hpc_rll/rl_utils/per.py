"""``hpc_rll.rl_utils.per`` -- prioritized experience replay (Schaul et al. 2016) as an index that lives in device memory: a
sum tree and a min tree over ``capacity`` slots with fan-out 64, one node per wave-wide read (no reference counterpart; the
semantics restate DI-engine's ``AdvancedReplayBuffer`` with its ``SumSegmentTree`` / ``MinSegmentTree``).  It closes the loop
of the learners that produce priorities (``r2d2_td``, ``muzero_loss``, the ``td_error`` of the n-step, distributional, discrete
SAC and QMIX losses) without a device-to-host copy, a Python loop over the batch and a host-to-device copy per step.  The
index stores priorities only; the transitions stay wherever the caller keeps them, addressed by the returned indices.

* leaf: ``(p + eps) ** alpha`` of a priority ``p``.  A negative, NaN or infinite priority counts as ``max_priority``, a device
  scalar that starts at 1 and is raised by every finite priority written; ``per_update(state, idx, None)`` writes
  ``max_priority``, which is how new transitions enter.  A slot never written holds 0 and is never sampled;
* update: when an index occurs several times in one call the last occurrence wins, as in a sequential loop, and indices
  outside ``[0, capacity)`` are skipped.  Nodes are recomputed from their 64 children in a fixed order, never adjusted: the same
  bits on every run, no drift, and a tree of integer-valued leaves with a total below 2**24 is exact;
* sample: the target mass of sample ``k`` is ``((k + u_k) / B) * total`` (stratified) or ``u_k * total`` for uniforms ``u`` in
  ``[0, 1)``; ``prob = leaf / total``, ``weight = (size * prob) ** -beta`` divided by the buffer's largest weight
  (``normalize='buffer'``, DI-engine's rule, from the min tree), the batch's largest (``'batch'``, the rule of Dopamine, SB3 and
  CleanRL) or nothing (``'none'``).  An empty index gives ``idx = -1`` and ``weight = 0``;
* nothing is differentiable and nothing synchronises with the host; everything that changes from call to call lives in the
  state tensor, so update and sample can be captured with ``hpc_rll.graphed`` / ``torch.cuda.graph`` and replayed;
* int64 indices, fp32 priorities and uniforms, contiguous GPU tensors, ``1 <= capacity <= 2**24``.  The state is an int32 tensor
  (its bits are fp32 nodes and int32 stamps) whose length determines the capacity."""
import torch
import torch.nn as nn

import hpc_replay

_NORMALIZE = {'none': 0, 'buffer': 1, 'batch': 2}
MAX_CAPACITY = 1 << 24


def per_init(capacity: int, device) -> torch.Tensor:
    """The state of an empty index over ``capacity`` slots on ``device``."""
    if not isinstance(capacity, int) or isinstance(capacity, bool):
        raise TypeError(f"capacity: expected an int, got {type(capacity).__name__}")
    state = torch.empty(hpc_replay.per_state_words(capacity), dtype=torch.int32, device=device)
    hpc_replay.per_init(state)
    return state


def per_update(state, idx, priority=None, alpha: float = 0.6, eps: float = 1e-6) -> None:
    """Write ``(priority + eps) ** alpha`` at ``idx (M,)``, or the leaf of ``max_priority`` when ``priority`` is None; in place."""
    hpc_replay.per_update(state, idx, priority, alpha, eps)


def per_rebuild(state, priorities, alpha: float = 0.6, eps: float = 1e-6) -> None:
    """Replace the whole index by the one of ``priorities (capacity,)``; a negative, NaN or infinite entry is an empty slot."""
    hpc_replay.per_rebuild(state, priorities, alpha, eps)


def per_sample(state, batch_size: int, beta: float, size, u=None, stratified: bool = True, normalize: str = 'buffer',
               generator=None):
    """``(idx, weight, prob)``, each ``(batch_size,)``.  ``size`` is the number of stored transitions, an int or a 1-element
    int64 tensor on the device; ``u`` the uniforms in ``[0, 1)``, drawn with ``torch.rand`` on the device when not given."""
    if normalize not in _NORMALIZE:
        raise ValueError(f"normalize: expected one of {sorted(_NORMALIZE)}, got {normalize!r}")
    if u is None:
        u = torch.rand(batch_size, device=state.device, dtype=torch.float32, generator=generator)
    elif u.dim() != 1 or u.shape[0] != batch_size:
        raise RuntimeError(f"u: shape {tuple(u.shape)}, expected ({batch_size},)")
    if isinstance(size, torch.Tensor):
        idx, weight, prob = hpc_replay.per_sample(state, u, beta, 1, size.reshape(1), stratified, _NORMALIZE[normalize])
    else:
        idx, weight, prob = hpc_replay.per_sample(state, u, beta, int(size), None, stratified, _NORMALIZE[normalize])
    return idx, weight, prob


class PrioritizedReplayIndex(nn.Module):
    """The index as a module: its state is a buffer, so ``state_dict`` / ``load_state_dict`` / ``.to`` carry it.  The ring
    pointer and ``size`` are host integers kept as extra state; :meth:`append` is the one member that is not graph-capturable,
    because it advances them."""

    def __init__(self, capacity: int, alpha: float = 0.6, eps: float = 1e-6, device=None):
        super().__init__()
        if device is None:
            device = torch.device('cuda', torch.cuda.current_device())
        self.capacity, self.alpha, self.eps = capacity, float(alpha), float(eps)
        self.register_buffer('state', per_init(capacity, device))
        self._layout = hpc_replay.per_layout(capacity)
        self.next, self.size = 0, 0

    def get_extra_state(self):
        return {'next': self.next, 'size': self.size}

    def set_extra_state(self, extra):
        self.next, self.size = int(extra['next']), int(extra['size'])

    def append(self, n: int) -> torch.Tensor:
        """The next ``n`` ring indices ``(n,)`` on the device, written at ``max_priority``.  Not graph-capturable."""
        if not 0 <= n <= self.capacity:
            raise ValueError(f"n: expected 0 .. capacity = {self.capacity} new transitions, got {n}")
        idx = (torch.arange(n, device=self.state.device, dtype=torch.int64) + self.next) % self.capacity
        per_update(self.state, idx, None, self.alpha, self.eps)
        self.next = (self.next + n) % self.capacity
        self.size = min(self.size + n, self.capacity)
        return idx

    def update(self, idx, priority) -> None:
        per_update(self.state, idx, priority, self.alpha, self.eps)

    def sample(self, batch_size: int, beta: float, u=None, stratified: bool = True, normalize: str = 'buffer', generator=None):
        """``(idx, weight, prob)`` of ``batch_size`` draws; ``size`` is the number of transitions appended so far."""
        return per_sample(self.state, batch_size, beta, max(self.size, 1), u, stratified, normalize, generator)

    def _floats(self, offset, n):
        return self.state.view(torch.float32)[offset:offset + n]

    @property
    def total(self) -> torch.Tensor:
        """The root of the sum tree, ``(1,)`` on the device (a view of the state)."""
        return self._floats(self._layout[2], 1)

    @property
    def max_priority(self) -> torch.Tensor:
        """``(1,)`` on the device (a view of the state)."""
        return self._floats(self._layout[22], 1)

    def priorities(self) -> torch.Tensor:
        """The leaves ``(capacity,)``, that is ``(p + eps) ** alpha`` per slot and 0 for an empty one (a view of the state)."""
        return self._floats(self._layout[2 + 2 * self._layout[0]], self.capacity)
