"""The prioritized-replay index (``hpc_rll.rl_utils.per``, csrc/per.hip) on an MI355X (``-m gpu``), through the C ABI on
guarded buffers (tests/guarded.py), every call pinned with ``hpc_rll_per_last_config``.

* exact cases: integer leaves with a power-of-two total and dyadic uniforms, where the fp64 search of tests/per_oracle.py is
  the only right answer -- indices equal it with no exclusions, and every node of both trees equals the fp32 restatement of
  the node order bit for bit;
* general priorities, log-uniform over six decades: each index within ``tol = 1e-5 total`` of the fp64 cumulative sums
  (a little over three times the 48 * 2^-24 = 2.9e-6 bound of the header), ``prob`` and ``weight`` within 1e-5 relative given the
  returned index, and under 1 % of the batch on the other side of a boundary;
* the update's duplicate rule, bad indices, sanitising, ``max_priority``, the min tree, the three normalisations, NaN
  uniforms, grids of more than one pass, rebuild, the module's ring and state_dict, the composition with ``r2d2_td`` and a
  captured update + sample replayed with other contents."""
import ctypes

import numpy as np
import pytest
import torch

import per_oracle as O
from guarded import GUARD, SENTINEL64, GuardedF32, GuardedI64, place

pytestmark = pytest.mark.gpu

NONE, BUFFER, BATCH = 0, 1, 2
SEEN = set()            # (part, kernel, depth) of every pinned call of this module


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def config():
    import cabi
    out = (ctypes.c_int * 12)()
    assert cabi.lib.hpc_rll_per_last_config(out) == 0
    out = list(out)
    return out[:6], out[6:]


class OutI64:
    """An int64 output between two sentinel bands, pre-filled with a value no call returns."""

    def __init__(self, n, dev):
        self.raw = torch.full((GUARD + n + GUARD,), SENTINEL64, dtype=torch.int64, device=dev)
        self.t = self.raw[GUARD:GUARD + n]
        self.t.fill_(-777)

    def check(self, what=""):
        n = self.t.numel()
        assert bool((self.raw[:GUARD] == SENTINEL64).all()) and bool((self.raw[GUARD + n:] == SENTINEL64).all()), \
            f"{what}: a guard word around idx was overwritten"
        assert not bool((self.t == -777).any()), f"{what}: an index was never written"


class Index:
    """A state on a guarded buffer, `off` floats past a 16-byte boundary."""

    def __init__(self, capacity, dev, off=0):
        import cabi
        self.cabi, self.dev, self.capacity = cabi, dev, capacity
        lay = (ctypes.c_int64 * 26)()
        assert cabi.lib.hpc_rll_per_layout(capacity, lay) == 0
        self.lay = list(lay)
        self.depth, words = self.lay[0], self.lay[1]
        assert 4 * words == cabi.lib.hpc_rll_per_state_bytes(capacity)
        self.g = GuardedF32(1, words, off, dev)
        self.state = self.g.t.view(-1)
        cabi.call("hpc_rll_per_init", dev, self.state.data_ptr(), capacity)
        self.g.check("init")
        self.g.assert_written("init")

    def level(self, tree, l, padded=False):
        base = 2 if tree == "sum" else 12
        off, n = self.lay[base + 2 * l], self.lay[base + 2 * l + 1]
        return self.state[off:off + (O.pad64(n) if padded else n)].cpu().numpy()

    def leaves(self):
        return self.level("sum", self.depth)

    @property
    def total(self):
        return self.level("sum", 0)[0]

    @property
    def max_priority(self):
        return float(self.state[self.lay[22]])

    def stamps_clear(self):
        return not bool(self.state.view(torch.int32)[self.lay[24]:self.lay[24] + self.capacity].any())

    def update(self, idx, pri, alpha=1.0, eps=0.0, kernel=None):
        idx = np.asarray(idx, dtype=np.int64)
        before = config()[0][0]
        gi = GuardedI64(torch.from_numpy(idx), self.dev)
        gp = None if pri is None else place(torch.from_numpy(np.asarray(pri, dtype=np.float32)).to(self.dev), 1)
        self.cabi.call("hpc_rll_per_update", self.dev, self.state.data_ptr(), self.capacity, gi.t.data_ptr(),
                       None if gp is None else gp.data_ptr(), len(idx), alpha, eps)
        gi.check("update")
        self.g.check("update")
        assert self.stamps_clear(), "stamps left behind"
        cfg = config()[0]
        assert cfg[0] == before + 1 and cfg[2] == self.depth and cfg[4] == 2 + self.depth, cfg
        n = O.level_sizes(self.capacity)
        full = sum(1 << l for l in range(self.depth) if n[l] <= len(idx))
        assert cfg[5] == full and cfg[1] == (1 if full & ~1 else 0), (cfg, full)
        items = n[self.depth - 1] if full & (1 << (self.depth - 1)) else len(idx)
        assert cfg[3] == min((items + 3) // 4, 2048), cfg
        if kernel is not None:
            assert cfg[1] == kernel, cfg
        SEEN.add(("update", cfg[1], self.depth))
        return cfg

    def rebuild(self, pri, alpha=1.0, eps=0.0):
        gp = place(torch.from_numpy(np.asarray(pri, dtype=np.float32)).to(self.dev), 3)
        self.cabi.call("hpc_rll_per_rebuild", self.dev, self.state.data_ptr(), self.capacity, gp.data_ptr(), alpha, eps)
        self.g.check("rebuild")
        cfg = config()[0]
        assert cfg[1] == 2 and cfg[2] == self.depth and cfg[4] == 2 + self.depth and cfg[5] == (1 << self.depth) - 1, cfg
        SEEN.add(("update", 2, self.depth))

    def sample(self, u, stratified=True, normalize=BUFFER, beta=0.4, size=None, size_dev=None, weight=True, prob=True):
        u = np.asarray(u, dtype=np.float32)
        B = len(u)
        before = config()[1][0]
        gu = place(torch.from_numpy(u).to(self.dev), 1)
        gi = OutI64(B, self.dev)
        gw = GuardedF32(1, B, 3, self.dev) if weight else None
        gp = GuardedF32(1, B, 2, self.dev) if prob else None
        self.cabi.call("hpc_rll_per_sample", self.dev, self.state.data_ptr(), self.capacity, gu.data_ptr(), gi.t.data_ptr(),
                       gw.t.data_ptr() if weight else None, gp.t.data_ptr() if prob else None, B, int(stratified), normalize,
                       beta, self.capacity if size is None else size, None if size_dev is None else size_dev.data_ptr())
        gi.check("sample")
        self.g.check("sample")
        for g in (gw, gp):
            if g is not None:
                g.check("sample")
                g.assert_written("sample")
        cfg = config()[1]
        flags = int(stratified) | (2 if weight else 0) | (4 if prob else 0) | (8 if size_dev is not None else 0)
        launches = 2 if (weight and normalize == BATCH) else 1
        assert cfg == [before + 1, normalize, self.depth, min((B + 3) // 4, 2048), launches, flags], cfg
        SEEN.add(("sample", normalize, self.depth))
        return (gi.t.cpu().numpy(), gw.t.view(-1).cpu().numpy() if weight else None,
                gp.t.view(-1).cpu().numpy() if prob else None)

    def assert_nodes(self, leaves32=None):
        """Every node of both trees, padding included, against the fp32 restatement built on the device's own leaves."""
        t = O.Tree32(self.leaves() if leaves32 is None else leaves32)
        for l in range(self.depth + 1):
            for tree, want in (("sum", t.sum[l]), ("min", t.min[l])):
                got = self.level(tree, l, padded=True)
                assert got.shape == want.shape and np.array_equal(got.view(np.int32), want.view(np.int32)), (tree, l)
        return t


def rel(a, b):
    return np.abs(a - b) / np.abs(b)


# ---------------------------------------------------------------------------------------------------------------------
# exact cases
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity", O.EXACT_CAPACITIES)
def test_exact_integer_leaves(dev, capacity):
    leaves = O.exact_leaves(capacity)
    total = int(leaves.sum())
    ix = Index(capacity, dev)
    ix.update(np.arange(capacity), leaves)                       # M = capacity: every level in full
    assert np.array_equal(ix.leaves(), leaves)
    ix.assert_nodes(leaves)
    assert float(ix.total) == total and float(ix.level("min", 0)[0]) == leaves.min()
    o = O.Index64(capacity)
    o.rebuild(leaves, 1.0, 0.0)
    for B in (1, 256):
        u = O.dyadic_u(B, capacity + B)
        for stratified in (True, False):
            idx, w, p = ix.sample(u, stratified, size=capacity)
            assert np.array_equal(idx, o.sample(u, stratified)), (B, stratified)
            assert np.array_equal(p, (leaves[idx] / np.float32(total)))          # a quotient by a power of two
            assert rel(w, o.weight(idx, 0.4, capacity, BUFFER)).max() < 1e-5
    idx, _, _ = ix.sample(np.full(total, 0.5, dtype=np.float32), weight=False, prob=False)
    assert np.array_equal(np.bincount(idx, minlength=capacity), leaves.astype(np.int64))
    assert np.array_equal(idx, np.repeat(np.arange(capacity), leaves.astype(np.int64)))


# ---------------------------------------------------------------------------------------------------------------------
# general priorities
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", (0.0, 0.6, 1.0))
@pytest.mark.parametrize("capacity,live", O.GENERAL_CASES)
def test_general_float_priorities(dev, capacity, live, alpha):
    slots, pri = O.general_case(capacity, live)
    ix = Index(capacity, dev, off=1)
    ix.update(slots, pri, alpha, 1e-6)
    o = O.Index64(capacity)
    o.update(slots, pri, alpha, 1e-6)
    assert rel(ix.leaves()[slots].astype(np.float64), o.leaves[slots]).max() < 2e-7     # an fp32 rounding of the fp64 power
    assert not ix.leaves()[np.setdiff1d(np.arange(capacity), slots)].any()
    t = ix.assert_nodes()
    assert abs(float(ix.total) - o.total) <= 48 * 2.0 ** -24 * o.total
    assert ix.max_priority == max(1.0, float(pri.max()))
    tol = O.TOL_REL * o.total
    C = np.cumsum(o.leaves)
    u = O.general_u(capacity)
    for stratified in (True, False):
        for normalize in (BUFFER, BATCH, NONE):
            idx, w, p = ix.sample(u, stratified, normalize, beta=0.4, size=live)
            m = o.mass(u, stratified)
            assert (o.leaves[idx] > 0).all()
            lo = np.where(idx > 0, C[np.maximum(idx - 1, 0)], 0.0)
            assert ((lo - tol <= m) & (m < C[idx] + tol)).all()
            other = idx != o.sample(u, stratified)
            if normalize == BUFFER:
                print(f"capacity {capacity} alpha {alpha} stratified {stratified}: {int(other.sum())} of {len(u)} on the "
                      f"other side of a boundary, {int(o.near_boundary(u, stratified, tol).sum())} within tol of one")
            assert other.sum() < 0.01 * len(u)
            assert rel(p, o.prob(idx)).max() < 1e-5
            assert rel(w, o.weight(idx, 0.4, live, normalize)).max() < 1e-5
            assert np.array_equal(idx, t.sample(u, stratified)[0])                # the descent, step for step
            if normalize == BATCH:
                assert w.max() == 1.0
            if normalize == BUFFER:
                assert w.max() <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# never an unfilled slot; an empty index
# ---------------------------------------------------------------------------------------------------------------------
def test_never_an_unfilled_slot(dev):
    ix = Index(4097, dev)
    live = np.array([0, 2000, 4096])
    ix.update(live, np.array([0.3, 1e-4, 7.0], dtype=np.float32))
    t = ix.assert_nodes()
    below_one = np.nextafter(np.float32(1), np.float32(0))
    u = np.array([0.0, below_one, 0.0, below_one, 0.5, 0.999, below_one], dtype=np.float32)
    for stratified in (True, False):
        idx, w, p = ix.sample(u, stratified, size=3)
        assert set(idx) <= set(live) and (p > 0).all() and (w > 0).all(), idx
        assert np.array_equal(idx, t.sample(u, stratified)[0])
    idx = ix.sample(u, False, size=3)[0]
    assert idx[0] == 0 and idx[1] == 4096 and idx[6] == 4096
    assert ix.sample(u, True, size=3)[0][6] == 4096                   # (6 + u) / 7 * total rounds to the total
    # out-of-range uniforms are clamped, not followed into the padding
    idx = ix.sample(np.array([1.0, 2.0, -1.0, np.inf, -np.inf], dtype=np.float32), False, size=3)[0]
    assert list(idx) == [4096, 4096, 0, 4096, 0]


def test_empty_index_gives_minus_one_and_zero_weights(dev):
    for capacity in (1, 65, 4097):
        ix = Index(capacity, dev)
        for normalize in (NONE, BUFFER, BATCH):
            idx, w, p = ix.sample(np.linspace(0, 0.9, 7, dtype=np.float32), normalize=normalize)
            assert (idx == -1).all() and not w.any() and not p.any()
        ix.update(np.array([0]), np.array([0.0], dtype=np.float32))              # a leaf of exactly 0 is an empty slot
        assert float(ix.total) == 0.0 and np.isinf(ix.level("min", 0)[0])
        assert (ix.sample(np.zeros(3, dtype=np.float32))[0] == -1).all()


# ---------------------------------------------------------------------------------------------------------------------
# update
# ---------------------------------------------------------------------------------------------------------------------
def test_update_duplicates_the_last_wins_with_the_same_bits_on_every_run(dev):
    rng = np.random.default_rng(4)
    calls = [(np.array(i), rng.uniform(0.1, 5.0, size=len(i)).astype(np.float32))
             for i in ([7, 7], [100] * 64, [4096] * 300, list(rng.integers(0, 4097, size=1000)) + [7] * 5)]
    words = []
    for run in range(2):
        ix, o = Index(4097, dev), O.Index64(4097)
        for idx, pri in calls:
            ix.update(idx, pri, 0.6, 1e-6)
            o.update(idx, pri, 0.6, 1e-6)
            last = O.leaf_of(pri[-1], 0.6, 1e-6)                 # the highest position wins
            assert rel(float(ix.leaves()[idx[-1]]), last) < 2e-7 and o.leaves[idx[-1]] == last
        assert np.array_equal(ix.leaves() > 0, o.leaves > 0)
        assert rel(ix.leaves()[o.leaves > 0].astype(np.float64), o.leaves[o.leaves > 0]).max() < 2e-7
        ix.assert_nodes()
        words.append(ix.state.view(torch.int32).cpu().numpy())
    assert np.array_equal(words[0], words[1])


@pytest.mark.parametrize("capacity,M", [(4097, 1), (4097, 255), (4097, 256), (4097, 257), (4097, 262144 + 300),
                                        (64 * 9000, 8500)])
def test_update_sizes_around_a_workgroups_share_and_past_one_pass(dev, capacity, M):
    """256 entries per workgroup in the stamp and leaf launches, 1024 workgroups a pass; 4 parents per workgroup in a level
    launch, 2048 workgroups a pass (capacity 576000: 8500 touched parents among 9000)."""
    rng = np.random.default_rng(M)
    if capacity == 4097:
        idx = rng.integers(0, capacity, size=M)
    else:
        idx = (rng.permutation(9000)[:M] * 64 + rng.integers(0, 64, size=M)).astype(np.int64)
    pri = rng.integers(1, 9, size=M).astype(np.float32)
    ix, o = Index(capacity, dev), O.Index64(capacity)
    cfg = ix.update(idx, pri)
    o.update(idx, pri, 1.0, 0.0)
    assert np.array_equal(ix.leaves(), o.leaves.astype(np.float32))
    ix.assert_nodes()
    assert float(ix.total) == o.total
    if capacity != 4097:
        assert cfg[3] == 2048 and not cfg[5] & (1 << (ix.depth - 1))       # more than one pass over the touched parents


def test_update_edges_bad_indices_and_where_two_entries_meet(dev):
    capacity = 262145
    ix, o = Index(capacity, dev), O.Index64(capacity)
    for idx in ([0, capacity - 1], [5, 6], [5, 70], [5, 200000], [capacity - 1, capacity - 2, 0],
                [-1, capacity, 3, -2 ** 40, 2 ** 40, capacity + 63, 9], [-5, capacity]):
        pri = np.arange(1, len(idx) + 1, dtype=np.float32)
        ix.update(np.array(idx), pri)
        o.update(np.array(idx), pri, 1.0, 0.0)
        assert np.array_equal(ix.leaves(), o.leaves.astype(np.float32)), idx
        ix.assert_nodes()
        assert float(ix.total) == o.total and ix.max_priority == o.max_priority
    assert ix.leaves()[3] == 3.0 and ix.leaves()[9] == 7.0 and ix.max_priority == 7.0


def test_sanitising_max_priority_eps_alpha_and_none(dev):
    ix, o = Index(300, dev), O.Index64(300)
    seen = [ix.max_priority]
    assert seen == [1.0]
    for idx, pri, alpha, eps in (([1, 2, 3, 4], [np.nan, -1.0, np.inf, 0.5], 1.0, 0.0),
                                 ([5, 6, 7], [4.0, np.nan, 2.0], 1.0, 0.0),          # NaN takes the max BEFORE the call
                                 ([8, 9], [np.nan, -np.inf], 0.6, 0.25),
                                 ([10, 11], None, 1.0, 0.0), ([12], None, 0.6, 1e-6), ([13], [0.0], 0.5, 0.04),
                                 ([14, 15], [3e38, 1.0], 1.0, 0.0), ([16], [9.0], 0.0, 0.0)):
        pri = None if pri is None else np.array(pri, dtype=np.float32)
        ix.update(np.array(idx), pri, alpha, eps)
        o.update(np.array(idx), pri, alpha, eps)
        seen.append(ix.max_priority)
        assert ix.max_priority == o.max_priority
    got = ix.leaves().astype(np.float64)
    assert list(got[1:5]) == [1.0, 1.0, 1.0, 0.5] and list(got[5:8]) == [4.0, 1.0, 2.0]
    assert rel(got[8:10], np.full(2, 4.25 ** float(np.float32(0.6)))).max() < 2e-7
    assert list(got[10:12]) == [4.0, 4.0] and rel(got[12], (4.0 + 1e-6) ** 0.6) < 2e-7
    assert rel(got[13], 0.2) < 2e-7 and got[14] == np.float32(1e30) and got[15] == 1.0 and got[16] == 1.0
    assert seen == sorted(seen) and seen[-1] == float(np.float32(3e38))
    ix.assert_nodes()


def test_min_tree_follows_a_raised_minimum_and_ignores_unfilled_leaves(dev):
    ix = Index(4097, dev)
    ix.update(np.array([10, 2000, 4096]), np.array([0.5, 0.25, 3.0], dtype=np.float32))
    assert float(ix.level("min", 0)[0]) == 0.25
    idx, w, _ = ix.sample(np.array([0.0, 0.19, 0.9], dtype=np.float32), False, BUFFER, beta=1.0, size=3)
    assert list(idx) == [10, 2000, 4096] and w[1] == 1.0 and rel(w[0], 0.5) < 1e-6 and rel(w[2], 0.25 / 3.0) < 1e-6
    ix.update(np.array([2000]), np.array([2.0], dtype=np.float32))
    assert float(ix.level("min", 0)[0]) == 0.5
    ix.update(np.array([10]), np.array([0.0], dtype=np.float32))      # emptied: no longer counts
    assert float(ix.level("min", 0)[0]) == 2.0
    ix.assert_nodes()


# ---------------------------------------------------------------------------------------------------------------------
# weights, uniforms, grids
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta", (0.0, 0.4, 1.0))
def test_weights_in_the_three_normalisations(dev, beta):
    slots, pri = O.general_case(4097, 300)
    ix, o = Index(4097, dev), O.Index64(4097)
    ix.update(slots, pri, 0.6, 1e-6)
    o.update(slots, pri, 0.6, 1e-6)
    u = O.general_u(4097)[:512]
    size_dev = torch.tensor([123], dtype=torch.int64, device=dev)
    for normalize in (NONE, BUFFER, BATCH):
        idx, w, p = ix.sample(u, True, normalize, beta, size=123)
        idx2, w2, p2 = ix.sample(u, True, normalize, beta, size=1, size_dev=size_dev)
        assert np.array_equal(idx, idx2) and np.array_equal(w, w2) and np.array_equal(p, p2)
        assert rel(w, o.weight(idx, beta, 123, normalize)).max() < 1e-5
        assert rel(p, o.prob(idx)).max() < 1e-5
        if beta == 0.0:
            assert (w == 1.0).all()
        idx3, w3, p3 = ix.sample(u, True, normalize, beta, size=123, prob=False)
        idx4, w4, p4 = ix.sample(u, True, normalize, beta, size=123, weight=False)
        assert p3 is None and w4 is None and np.array_equal(w3, w) and np.array_equal(p4, p) and np.array_equal(idx3, idx4)
    # the minimum leaf has weight 1 under the buffer's rule
    lowest = slots[np.argmin(pri)]
    C = np.cumsum(o.leaves)
    um = np.array([(C[lowest] - 0.5 * o.leaves[lowest]) / o.total], dtype=np.float32)
    idx, w, _ = ix.sample(um, False, BUFFER, beta, size=123)
    assert idx[0] == lowest and w[0] == 1.0


def test_nan_uniforms_count_as_zero_and_the_unstratified_mode(dev):
    leaves = O.exact_leaves(4097)
    ix, o = Index(4097, dev), O.Index64(4097)
    ix.rebuild(leaves)
    o.rebuild(leaves, 1.0, 0.0)
    u = O.dyadic_u(64, 1)
    u[::5] = np.nan
    for stratified in (True, False):
        idx = ix.sample(u, stratified)[0]
        assert np.array_equal(idx, o.sample(u, stratified))
    assert (ix.sample(u, False)[0][::5] == 0).all()


@pytest.mark.parametrize("B", (1, 8192, 8193, 9000))
def test_sample_grid_of_one_wave_and_of_more_than_one_pass(dev, B):
    leaves = O.exact_leaves(262145)
    ix, o = Index(262145, dev), O.Index64(262145)
    ix.rebuild(leaves)
    o.rebuild(leaves, 1.0, 0.0)
    u = np.random.default_rng(B).random(B, dtype=np.float32)
    t = O.Tree32(leaves)
    for normalize in (BUFFER, BATCH):
        idx, w, p = ix.sample(u, True, normalize, 0.4, size=262145)
        assert np.array_equal(idx, t.sample(u)[0])
        near = o.near_boundary(u, True, 1e-5 * o.total)
        assert np.array_equal(idx[~near], o.sample(u)[~near])
        assert rel(w, o.weight(idx, 0.4, 262145, normalize)).max() < 1e-5
        assert normalize != BATCH or w.max() == 1.0


# ---------------------------------------------------------------------------------------------------------------------
# rebuild, the module
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity", (63, 4097, 262145))
def test_rebuild_gives_the_bits_of_a_sequence_of_updates(dev, capacity):
    rng = np.random.default_rng(capacity)
    pri = (10.0 ** rng.uniform(-3, 3, size=capacity)).astype(np.float32)
    pri[rng.random(capacity) < 0.3] = -1.0                       # empty slots
    pri[0] = np.nan
    a, b = Index(capacity, dev), Index(capacity, dev, off=2)
    a.update(np.arange(capacity), np.zeros(capacity, dtype=np.float32), 0.6, 1e-6)    # b.rebuild must not depend on what was there
    a.rebuild(pri, 0.6, 1e-6)
    order = rng.permutation(np.flatnonzero(pri >= 0))
    for part in np.array_split(order, 3):
        b.update(part, pri[part], 0.6, 1e-6)
    assert np.array_equal(a.state.view(torch.int32).cpu().numpy(), b.state.view(torch.int32).cpu().numpy())
    a.assert_nodes()
    assert a.max_priority == max(1.0, float(pri[pri >= 0].max()))
    assert not a.leaves()[~(pri >= 0)].any()


def test_module_state_dict_round_trip_and_ring_wrap(dev):
    from hpc_rll.rl_utils.per import PrioritizedReplayIndex
    m = PrioritizedReplayIndex(100, alpha=1.0, eps=0.0, device=dev)
    assert float(m.total) == 0.0 and float(m.max_priority) == 1.0 and m.priorities().shape == (100,)
    first = m.append(60)
    assert first.tolist() == list(range(60)) and (m.next, m.size) == (60, 60) and float(m.total) == 60.0
    m.update(first[:3], torch.tensor([5.0, 2.0, 0.5], device=dev))
    assert float(m.max_priority) == 5.0
    second = m.append(70)                                        # wraps: 60..99, then 0..29, at the new max priority
    assert second.tolist() == list(range(60, 100)) + list(range(30)) and (m.next, m.size) == (30, 100)
    want = np.full(100, 5.0)
    want[30:60] = 1.0
    assert np.array_equal(m.priorities().cpu().numpy(), want) and float(m.total) == want.sum()
    with pytest.raises(ValueError, match="capacity"):
        m.append(101)
    u = torch.rand(64, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    idx, w, p = m.sample(64, 0.4, u=u)
    assert idx.dtype == torch.int64 and not idx.requires_grad and not w.requires_grad
    o = O.Index64(100)
    o.rebuild(want, 1.0, 0.0)
    assert np.array_equal(idx.cpu().numpy(), o.sample(u.cpu().numpy()))
    assert rel(w.cpu().numpy(), o.weight(idx.cpu().numpy(), 0.4, 100, BUFFER)).max() < 1e-5
    # drawn uniforms: same generator state, same batch
    g = torch.Generator(device=dev)
    a = m.sample(32, 0.4, generator=g.manual_seed(7))
    b = m.sample(32, 0.4, generator=g.manual_seed(7))
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and bool((a[0] >= 0).all())
    sd = {k: (v.clone() if torch.is_tensor(v) else dict(v)) for k, v in m.state_dict().items()}
    m2 = PrioritizedReplayIndex(100, alpha=1.0, eps=0.0, device=dev)
    m2.load_state_dict(sd)
    assert torch.equal(m2.state, m.state) and (m2.next, m2.size) == (30, 100)
    assert all(torch.equal(x, y) for x, y in zip(m2.sample(64, 0.4, u=u), (idx, w, p)))
    m3 = PrioritizedReplayIndex(100, device=dev).double()        # a dtype cast leaves the int32 state alone
    assert m3.state.dtype == torch.int32 and float(m3.max_priority) == 1.0
    with pytest.raises(RuntimeError):
        PrioritizedReplayIndex(101, device=dev).load_state_dict(sd)


def test_composition_with_r2d2_priorities(dev):
    from hpc_rll.rl_utils.per import per_init, per_sample, per_update
    from hpc_rll.rl_utils.r2d2 import r2d2_td
    T, B, N = 12, 96, 6
    g = torch.Generator(device=dev).manual_seed(2)
    q, tq = torch.randn(T, B, N, device=dev, generator=g), torch.randn(T, B, N, device=dev, generator=g)
    action = torch.randint(0, N, (T, B), device=dev, generator=g)
    reward = torch.randn(T, B, device=dev, generator=g)
    priority = r2d2_td(q, tq, action, reward, nstep=3)[2]
    assert priority.shape == (B,)
    state = per_init(300, dev)
    slots = torch.randperm(300, device=dev, generator=g)[:B]
    per_update(state, slots, priority, 0.6, 1e-6)
    u = torch.rand(128, device=dev, generator=g)
    idx, w, p = per_sample(state, 128, 0.4, B, u=u)
    o = O.Index64(300)
    o.update(slots.cpu().numpy(), priority.cpu().numpy(), 0.6, 1e-6)
    un = u.cpu().numpy()
    idx = idx.cpu().numpy()
    near = o.near_boundary(un, True, 1e-5 * o.total)
    assert np.array_equal(idx[~near], o.sample(un)[~near]) and near.sum() <= 2
    assert rel(p.cpu().numpy(), o.prob(idx)).max() < 1e-5 and rel(w.cpu().numpy(), o.weight(idx, 0.4, B, BUFFER)).max() < 1e-5


def test_captured_update_and_sample_replay_with_other_contents(dev):
    """Everything that changes from call to call lives in the state: a graph captured once gives, on every replay, the bits
    of the eager calls with the same contents."""
    from hpc_rll.rl_utils.per import per_init, per_sample, per_update
    capacity, M, B = 4097, 200, 128
    rng = np.random.default_rng(8)
    rounds = []
    for r in range(4):
        idx = rng.integers(0, capacity, size=M)
        idx[:20] = idx[20:40]                                    # duplicates
        pri = rng.uniform(0.0, 10.0 * (r + 1), size=M).astype(np.float32)
        pri[3] = np.nan                                          # takes max_priority, which the earlier rounds raised
        rounds.append((torch.from_numpy(idx).to(dev), torch.from_numpy(pri).to(dev),
                       torch.from_numpy(rng.random(B, dtype=np.float32)).to(dev)))
    eager_state, graph_state = per_init(capacity, dev), per_init(capacity, dev)
    s_idx, s_pri, s_u = (t.clone() for t in rounds[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                # warm-up on the side stream, as torch asks
        per_update(graph_state, s_idx, s_pri, 0.6, 1e-6)
        per_sample(graph_state, B, 0.4, capacity, u=s_u, normalize='batch')
    torch.cuda.current_stream().wait_stream(side)
    per_update(eager_state, *rounds[0][:2], 0.6, 1e-6)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        per_update(graph_state, s_idx, s_pri, 0.6, 1e-6)
        out = per_sample(graph_state, B, 0.4, capacity, u=s_u, normalize='batch')
    for idx, pri, u in rounds[1:]:
        s_idx.copy_(idx)
        s_pri.copy_(pri)
        s_u.copy_(u)
        graph.replay()
        per_update(eager_state, idx, pri, 0.6, 1e-6)
        want = per_sample(eager_state, B, 0.4, capacity, u=u, normalize='batch')
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(out, want))
        assert torch.equal(graph_state, eager_state)
        assert bool((out[0] >= 0).all())


# ---------------------------------------------------------------------------------------------------------------------
# coverage
# ---------------------------------------------------------------------------------------------------------------------
def test_every_depth_and_every_kernel_was_hit(dev):
    """Runs the calls itself, so that it also holds when selected alone: updates through the touched parents (0) and with a
    level below the root in full (1), the rebuild (2) and the three sample kernels at every depth 1..4."""
    for capacity in (64, 65, 4097, 262145):
        ix = Index(capacity, dev)
        ix.update(np.arange(capacity), np.ones(capacity, dtype=np.float32), kernel=1 if capacity > 64 else 0)
        ix.update(np.array([capacity - 1]), np.array([2.0], dtype=np.float32), kernel=0)
        ix.rebuild(np.ones(capacity, dtype=np.float32))
        for normalize in (NONE, BUFFER, BATCH):
            ix.sample(np.array([0.5, 0.25], dtype=np.float32), normalize=normalize)
    want = {("update", k, d) for k in (0, 1, 2) for d in (1, 2, 3, 4)} | {("sample", k, d) for k in (0, 1, 2) for d in (1, 2, 3, 4)}
    want.discard(("update", 1, 1))      # depth 1 has no level below the root
    assert want <= SEEN, sorted(want - SEEN)
