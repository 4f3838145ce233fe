"""TEST-ONLY oracle of the prioritized-replay index (``hpc_rll.rl_utils.per``, csrc/per.hip), in numpy.

``Index64`` is the plain restatement in fp64: a sequential update in which the last occurrence of an index wins, ``cumsum`` and
``searchsorted(side='right')`` over the positive leaves, and the weight formulas.  ``Tree32`` is the bit-faithful fp32
restatement of the node order the header states (the prefixes of a node's 64 children by the steps ``x_j += x_{j-s}``, s = 1,
2, .., 32; the node is the last prefix), with the descent rule of the sampler; it is what the exact cases compare internal
nodes with.  Neither imports the product."""
import numpy as np

FAN = 64
LEAF_MAX = 1e30
NONE, BUFFER, BATCH = 0, 1, 2


def depth_of(capacity):
    d, r = 1, FAN
    while r < capacity:
        r *= FAN
        d += 1
    return d


def level_sizes(capacity):
    """n_l for l = 0 (root) .. depth (leaves)."""
    d = depth_of(capacity)
    n, out = capacity, []
    for _ in range(d + 1):
        out.append(n)
        n = (n + FAN - 1) // FAN
    return out[::-1]


def pad64(n):
    return (n + FAN - 1) // FAN * FAN


def state_words(capacity, scalar_words):
    return 2 * sum(pad64(n) for n in level_sizes(capacity)) + scalar_words + capacity


def usable(p):
    p = np.asarray(p, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.isfinite(p) & (p >= 0)


def leaf_of(p, alpha, eps):
    """The fp32 leaf of the priorities p as fp64 numbers; alpha and eps reach the kernels as fp32 values."""
    a, e = float(np.float32(alpha)), float(np.float32(eps))
    b = np.asarray(p, dtype=np.float64) + e
    v = b if a == 1.0 else (np.ones_like(b) if a == 0.0 else b ** a)
    return np.minimum(v.astype(np.float32), np.float32(LEAF_MAX)).astype(np.float64)


class Index64:
    def __init__(self, capacity):
        self.capacity = capacity
        self.leaves = np.zeros(capacity, dtype=np.float64)
        self.max_priority = 1.0

    def update(self, idx, priority, alpha, eps):
        idx = np.asarray(idx, dtype=np.int64)
        valid = (idx >= 0) & (idx < self.capacity)
        p = np.full(idx.shape, self.max_priority) if priority is None else np.asarray(priority, dtype=np.float64).copy()
        ok = usable(p)
        p[~ok] = self.max_priority                       # the value before the call
        if priority is not None and (ok & valid).any():
            self.max_priority = max(self.max_priority, float(p[ok & valid].max()))
        vi, vp = idx[valid], leaf_of(p[valid], alpha, eps)
        _, first = np.unique(vi[::-1], return_index=True)     # the last occurrence of every index
        last = len(vi) - 1 - first
        self.leaves[vi[last]] = vp[last]

    def rebuild(self, priorities, alpha, eps):
        p = np.asarray(priorities, dtype=np.float64)
        ok = usable(p)
        self.leaves = np.where(ok, leaf_of(np.where(ok, p, 0.0), alpha, eps), 0.0)
        self.max_priority = max(1.0, float(p[ok].max())) if ok.any() else 1.0

    @property
    def total(self):
        return float(self.leaves.sum())

    @property
    def min_leaf(self):
        live = self.leaves[self.leaves > 0]
        return float(live.min()) if live.size else float("inf")

    def mass(self, u, stratified):
        u = np.nan_to_num(np.asarray(u, dtype=np.float64), nan=0.0)
        B = u.shape[0]
        return ((np.arange(B) + u) / B if stratified else u) * self.total

    def boundaries(self):
        """(pos, C): the indices of the positive leaves and their inclusive cumulative sums."""
        pos = np.flatnonzero(self.leaves > 0)
        return pos, np.cumsum(self.leaves[pos])

    def sample(self, u, stratified=True):
        B = len(u)
        if not self.total > 0:
            return np.full(B, -1, dtype=np.int64)
        pos, C = self.boundaries()
        j = np.searchsorted(C, self.mass(u, stratified), side="right")
        return pos[np.minimum(j, len(pos) - 1)]

    def prob(self, idx):
        return self.leaves[idx] / self.total

    def weight(self, idx, beta, size, normalize):
        """The weights of the GIVEN indices (so that a sample on a boundary does not count as a weight error)."""
        b = float(np.float32(beta))
        if not self.total > 0:
            return np.zeros(len(idx))
        w = (size * self.prob(idx)) ** -b
        if normalize == BUFFER:
            w = w / (size * self.min_leaf / self.total) ** -b
        elif normalize == BATCH:
            w = w / w.max()
        return w

    def near_boundary(self, u, stratified, tol):
        """Which samples have their target within tol of a boundary between two positive leaves."""
        _, C = self.boundaries()
        m = self.mass(u, stratified)
        j = np.clip(np.searchsorted(C, m), 0, len(C) - 1)
        d = np.abs(C[j] - m)
        d = np.minimum(d, np.abs(C[np.maximum(j - 1, 0)] - m))
        return d <= tol


# ---------------------------------------------------------------------------------------------------------------------
# bit-faithful fp32
# ---------------------------------------------------------------------------------------------------------------------
def scan32(c):
    """Inclusive prefixes along the last axis (64) in the kernels' order, fp32."""
    x = np.array(c, dtype=np.float32)
    assert x.shape[-1] == FAN
    s = 1
    while s < FAN:
        y = x.copy()
        x[..., s:] = y[..., s:] + y[..., :-s]
        s *= 2
    return x


class Tree32:
    """Both trees, level by level (index 0 the root level), padded as the state is."""

    def __init__(self, leaves):
        leaves = np.asarray(leaves, dtype=np.float32)
        self.capacity = leaves.shape[0]
        self.depth = depth_of(self.capacity)
        self.n = level_sizes(self.capacity)
        s = np.zeros(pad64(self.capacity), dtype=np.float32)
        s[:self.capacity] = leaves
        m = np.where(s > 0, s, np.float32(np.inf)).astype(np.float32)
        self.sum, self.min = [s], [m]
        for l in range(self.depth - 1, -1, -1):
            ps = np.zeros(pad64(self.n[l]), dtype=np.float32)
            pm = np.full(pad64(self.n[l]), np.inf, dtype=np.float32)
            ps[:self.n[l]] = scan32(self.sum[0].reshape(-1, FAN))[:self.n[l], FAN - 1]
            pm[:self.n[l]] = self.min[0].reshape(-1, FAN)[:self.n[l]].min(axis=1)
            self.sum.insert(0, ps)
            self.min.insert(0, pm)

    @property
    def total(self):
        return self.sum[0][0]

    def sample(self, u, stratified=True):
        """(idx, leaf): the descent of the sampler, step for step."""
        u = np.nan_to_num(np.asarray(u, dtype=np.float32), nan=0.0)
        B = u.shape[0]
        total = self.total
        if not (total > 0 and np.isfinite(total)):
            return np.full(B, -1, dtype=np.int64), np.zeros(B, dtype=np.float32)
        k = np.arange(B, dtype=np.float64)
        md = (k + u.astype(np.float64)) / B * np.float64(total) if stratified else u.astype(np.float64) * np.float64(total)
        m = md.astype(np.float32)
        node = np.zeros(B, dtype=np.int64)
        leaf = np.zeros(B, dtype=np.float32)
        rows = np.arange(B)
        for l in range(self.depth):
            c = self.sum[l + 1].reshape(-1, FAN)[node]
            P = scan32(c)
            live = c > 0
            hit = live & (m[:, None] < P)
            first = hit.argmax(axis=1)
            last = FAN - 1 - live[:, ::-1].argmax(axis=1)
            j = np.where(hit.any(axis=1), first, last)
            below = np.where(j > 0, P[rows, np.maximum(j - 1, 0)], np.float32(0)).astype(np.float32)
            cj = c[rows, j]
            m = (m - below).astype(np.float32)
            m = np.where(m >= 0, m, np.float32(0)).astype(np.float32)
            m = np.where(m >= cj, np.nextafter(cj, np.float32(0)), m).astype(np.float32)
            node = node * FAN + j
            leaf = cj
        return node, leaf


# ---------------------------------------------------------------------------------------------------------------------
# the cases the CPU and the GPU tier share
# ---------------------------------------------------------------------------------------------------------------------
EXACT_CAPACITIES = (1, 63, 64, 65, 4095, 4096, 4097, 262145)


def exact_leaves(capacity, seed=0):
    """Integers in 1..8 whose sum is a power of two in (2 capacity, 4 capacity]."""
    rng = np.random.default_rng(seed + capacity)
    v = rng.integers(1, 9, size=capacity)
    target = 1 << int(np.floor(np.log2(4 * capacity)))
    order = rng.permutation(capacity)
    diff = target - int(v.sum())
    for i in order:
        if diff == 0:
            break
        step = min(8 - v[i], diff) if diff > 0 else max(1 - v[i], diff)
        v[i] += step
        diff -= step
    assert diff == 0 and v.min() >= 1 and v.max() <= 8 and int(v.sum()) == target
    return v.astype(np.float32)


def dyadic_u(B, seed, bits=8):
    return (np.random.default_rng(seed).integers(0, 1 << bits, size=B) / float(1 << bits)).astype(np.float32)


# (capacity, live leaves): log-uniform priorities over six decades on `live` slots spread over the capacity.  At most ~300
# live leaves: the targets within tol = 1e-5 total of a boundary are then under 1 % of a batch (each boundary takes 2e-5).
GENERAL_CASES = ((64, 64), (300, 300), (4097, 300), (262145, 300))
GENERAL_B = 2048
TOL_REL = 1e-5


def general_case(capacity, live, seed=5):
    """(slots (live,) int64 ascending, priorities (live,) fp32)."""
    rng = np.random.default_rng(seed + capacity)
    slots = np.sort(rng.choice(capacity, size=live, replace=False)).astype(np.int64)
    if capacity > live:
        slots[0], slots[-1] = 0, capacity - 1
    pri = (10.0 ** rng.uniform(-3, 3, size=live)).astype(np.float32)
    return slots, pri


def general_u(capacity, seed=9):
    return np.random.default_rng(seed + capacity).random(GENERAL_B, dtype=np.float32)
