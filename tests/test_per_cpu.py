"""CPU tier of the prioritized-replay index (``hpc_rll.rl_utils.per``, csrc/per.hip, ext/replay.cpp): the parts that need no
GPU -- the layout and the size of the state against the oracle's restatement; the C entry points are declared and exported and
answer argument errors with status codes before any HIP call, in the documented order, and write nothing; the dispatch record
before any launch; identities of the fp64 oracle and of the fp32 restatement of the node order; the shares of boundary samples
of the seeds tests/test_per_gpu.py uses; the host messages; the pybind surface of ``hpc_replay`` against
tests/golden/ext_signatures_replay.json (written only by tests/tools/write_replay_signatures.py).  Everything that launches is
in tests/test_per_gpu.py."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import per_oracle as O
from conftest import ROOT

EINVAL, EALIGN, EUNSUPPORTED = -1, -2, -3
NAMES = ("hpc_rll_per_state_bytes", "hpc_rll_per_capacity_of", "hpc_rll_per_layout", "hpc_rll_per_init", "hpc_rll_per_update",
         "hpc_rll_per_rebuild", "hpc_rll_per_sample", "hpc_rll_per_last_config")
CAPACITIES = (1, 63, 64, 65, 4096, 4097, 262144, 262145, 2 ** 24)
DEPTHS = (1, 1, 1, 2, 2, 3, 3, 4, 4)
SCALAR_WORDS = 8256


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_c_entry_points_declared_and_exported():
    import cabi
    P, I, F, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_int64
    want = {NAMES[0]: (L, [L]), NAMES[1]: (L, [L]), NAMES[2]: (I, [L, P]), NAMES[3]: (I, [P, L, P]),
            NAMES[4]: (I, [P, L, P, P, L, F, F, P]), NAMES[5]: (I, [P, L, P, F, F, P]),
            NAMES[6]: (I, [P, L, P, P, P, P, L, I, I, F, L, P, P]), NAMES[7]: (I, [P])}
    for name, sig in want.items():
        assert hasattr(cabi.lib, name), name
        assert cabi.SIGNATURES[name] == sig, name
    assert sorted(n for n in cabi.SIGNATURES if "_per_" in n) == sorted(want)
    assert cabi.lib.hpc_rll_abi_version() == 6
    hdr = open(cabi.HEADER_PATH).read()
    for line in ("#define HPC_RLL_PER_NORM_NONE (0)", "#define HPC_RLL_PER_NORM_BUFFER (1)", "#define HPC_RLL_PER_NORM_BATCH (2)",
                 "#define HPC_RLL_PER_MAX_CAPACITY (16777216)", f"#define HPC_RLL_PER_SCALAR_WORDS ({SCALAR_WORDS})",
                 "#define HPC_RLL_PER_LAYOUT_INTS (26)", "#define HPC_RLL_PER_CONFIG_INTS (12)"):
        assert line in hdr, line


@pytest.mark.parametrize("capacity,depth", list(zip(CAPACITIES, DEPTHS)))
def test_layout_and_state_bytes(capacity, depth):
    import cabi
    out = (ctypes.c_int64 * 26)(*([77] * 26))
    assert cabi.lib.hpc_rll_per_layout(capacity, out) == 0
    out = list(out)
    n = O.level_sizes(capacity)
    assert out[0] == depth == O.depth_of(capacity) and len(n) == depth + 1 and n[0] == 1 and n[-1] == capacity
    words = O.state_words(capacity, SCALAR_WORDS)
    assert out[1] == words and cabi.lib.hpc_rll_per_state_bytes(capacity) == 4 * words
    assert cabi.lib.hpc_rll_per_capacity_of(4 * words) == capacity
    off = 0
    for tree in (2, 12):                                    # the sum tree's levels, then the min tree's
        for l in range(5):
            o, ln = out[tree + 2 * l], out[tree + 2 * l + 1]
            if l <= depth:
                assert (o, ln) == (off, n[l]) and o % 64 == 0, (tree, l)
                off += O.pad64(n[l])
            else:
                assert (o, ln) == (-1, 0), (tree, l)
    assert out[22:] == [off, SCALAR_WORDS, off + SCALAR_WORDS, capacity]
    for l in range(depth):                                  # the 64 children of every node lie inside the padded level below
        assert 64 * n[l] == O.pad64(n[l + 1])


def test_sizes_that_are_refused_and_the_inverse():
    import cabi
    L = cabi.lib
    out = (ctypes.c_int64 * 26)(*([77] * 26))
    assert L.hpc_rll_per_state_bytes(2 ** 24 + 1) == EUNSUPPORTED and L.hpc_rll_per_layout(2 ** 24 + 1, out) == EUNSUPPORTED
    assert L.hpc_rll_per_state_bytes(0) == EINVAL and L.hpc_rll_per_state_bytes(-5) == EINVAL
    assert L.hpc_rll_per_layout(0, out) == EINVAL and L.hpc_rll_per_layout(64, None) == EINVAL
    assert list(out) == [77] * 26
    sizes = [L.hpc_rll_per_state_bytes(c) for c in range(1, 300)]
    assert all(b > a for a, b in zip(sizes, sizes[1:]))     # strictly increasing: the length of a state names its capacity
    for c in (1, 64, 65, 299, 4097, 2 ** 24):
        b = L.hpc_rll_per_state_bytes(c)
        assert L.hpc_rll_per_capacity_of(b) == c
        assert L.hpc_rll_per_capacity_of(b + 4) in (EINVAL, c + 1) and L.hpc_rll_per_capacity_of(b + 2) == EINVAL
    assert L.hpc_rll_per_capacity_of(0) == EINVAL and L.hpc_rll_per_capacity_of(-4) == EINVAL
    assert L.hpc_rll_per_capacity_of(2 ** 40) == EINVAL


def test_argument_errors_are_statuses_in_the_documented_order():
    """Nulls and sizes, then alignment, then the capacity limit, then empty shapes: all before any HIP call, nothing written."""
    import cabi
    L = cabi.lib
    buf = (ctypes.c_float * 64)(*([7.0] * 64))
    P = ctypes.addressof(buf)
    assert P % 8 == 0
    upd = lambda state=P, cap=100, idx=P, pri=P, M=4, alpha=0.6, eps=1e-6: L.hpc_rll_per_update(state, cap, idx, pri, M, alpha, eps, None)
    reb = lambda state=P, cap=100, pri=P, alpha=0.6, eps=1e-6: L.hpc_rll_per_rebuild(state, cap, pri, alpha, eps, None)
    smp = lambda state=P, cap=100, u=P, idx=P, w=P, pr=P, B=4, strat=1, norm=1, beta=0.4, size=10, sd=None: \
        L.hpc_rll_per_sample(state, cap, u, idx, w, pr, B, strat, norm, beta, size, sd, None)
    # EINVAL
    assert L.hpc_rll_per_init(None, 100, None) == EINVAL and L.hpc_rll_per_init(P, 0, None) == EINVAL
    assert upd(state=None) == EINVAL and upd(idx=None) == EINVAL and upd(cap=0) == EINVAL and upd(M=-1) == EINVAL
    assert upd(M=2 ** 31) == EINVAL and upd(alpha=-0.5) == EINVAL and upd(eps=-1.0) == EINVAL
    assert upd(alpha=float("nan")) == EINVAL and upd(eps=float("inf")) == EINVAL
    assert reb(state=None) == EINVAL and reb(pri=None) == EINVAL and reb(cap=-1) == EINVAL and reb(alpha=-1.0) == EINVAL
    assert smp(state=None) == EINVAL and smp(u=None) == EINVAL and smp(idx=None) == EINVAL and smp(B=-1) == EINVAL
    assert smp(norm=3) == EINVAL and smp(norm=-1) == EINVAL and smp(beta=-0.1) == EINVAL and smp(size=0) == EINVAL
    assert smp(cap=0) == EINVAL and smp(beta=float("nan")) == EINVAL
    # EINVAL comes before EALIGN, EALIGN before EUNSUPPORTED
    assert upd(state=P + 2, M=-1) == EINVAL and upd(state=P + 2, cap=2 ** 24 + 1) == EALIGN
    assert L.hpc_rll_per_init(P + 2, 100, None) == EALIGN and L.hpc_rll_per_init(P + 1, 2 ** 24 + 1, None) == EALIGN
    assert upd(state=P + 2) == EALIGN and upd(idx=P + 4) == EALIGN and upd(pri=P + 2) == EALIGN
    assert reb(state=P + 2) == EALIGN and reb(pri=P + 1) == EALIGN
    for name in ("state", "u", "w", "pr"):
        assert smp(**{name: P + 2}) == EALIGN, name
    assert smp(idx=P + 4) == EALIGN and smp(sd=P + 4) == EALIGN
    # EUNSUPPORTED
    assert L.hpc_rll_per_init(P, 2 ** 24 + 1, None) == EUNSUPPORTED
    assert upd(cap=2 ** 24 + 1) == EUNSUPPORTED and reb(cap=2 ** 24 + 1) == EUNSUPPORTED and smp(cap=2 ** 24 + 1) == EUNSUPPORTED
    assert upd(cap=2 ** 24 + 1, M=0) == EUNSUPPORTED and smp(cap=2 ** 24 + 1, B=0) == EUNSUPPORTED
    # empty shapes succeed without a launch; the optional operands may be NULL
    assert upd(M=0) == 0 and upd(M=0, idx=None, pri=None) == 0 and upd(M=0, cap=2 ** 24) == 0
    assert smp(B=0) == 0 and smp(B=0, u=None, idx=None, w=None, pr=None) == 0 and smp(B=0, size=0, sd=P) == 0
    assert list(buf) == [7.0] * 64


def test_last_config_before_any_launch():
    code = f"""
import ctypes, sys
sys.path.insert(0, {os.path.join(ROOT, "tests")!r})
import cabi
L = cabi.lib
assert L.hpc_rll_per_last_config(None) == -1
out = (ctypes.c_int * 12)(*([77] * 12))
assert L.hpc_rll_per_update(out, 100, None, None, 0, 0.6, 1e-6, None) == 0
assert L.hpc_rll_per_sample(out, 100, None, None, None, None, 0, 1, 1, 0.4, 5, None, None) == 0
assert L.hpc_rll_per_update(out, 100, None, None, 4, 0.6, 1e-6, None) == -1
assert list(out) == [77] * 12
assert L.hpc_rll_per_last_config(out) == 0
assert list(out) == ([0] + [-1] * 5) * 2, list(out)
print("per diag ok")
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "per diag ok" in r.stdout, (r.returncode, r.stdout, r.stderr)


# ---------------------------------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------------------------------
def test_oracle_update_is_the_sequential_loop():
    rng = np.random.default_rng(1)
    idx = rng.integers(-3, 45, size=200)
    pri = rng.uniform(0, 3, size=200).astype(np.float32)
    pri[5], pri[17], pri[40] = np.nan, -1.0, np.inf
    o = O.Index64(40)
    o.update(idx, pri, 0.6, 1e-6)
    want, pmax = np.zeros(40), 1.0
    for i, p in zip(idx, pri):
        if 0 <= i < 40:
            v = float(p) if np.isfinite(p) and p >= 0 else 1.0       # max_priority before the call
            pmax = max(pmax, v)
            want[i] = np.float32((v + float(np.float32(1e-6))) ** float(np.float32(0.6)))
    assert np.array_equal(o.leaves, want) and o.max_priority == pmax
    o.update(np.array([3, 3, 3]), None, 1.0, 0.0)
    assert o.leaves[3] == np.float32(pmax) and o.max_priority == pmax


def test_oracle_probabilities_sum_to_one_and_buffer_weights_peak_at_the_minimum_leaf():
    slots, pri = O.general_case(300, 300)
    o = O.Index64(300)
    o.update(slots, pri, 0.6, 1e-6)
    everything = np.arange(300)
    assert abs(o.prob(everything).sum() - 1.0) < 1e-12
    for beta in (0.0, 0.4, 1.0):
        w = o.weight(everything, beta, 300, O.BUFFER)
        assert w.max() <= 1.0 + 1e-12 and abs(w[np.argmin(o.leaves)] - 1.0) < 1e-12
        assert abs(o.weight(everything, beta, 300, O.BATCH).max() - 1.0) < 1e-15
    assert np.allclose(o.weight(everything, 0.0, 300, O.NONE), 1.0)


@pytest.mark.parametrize("capacity", O.EXACT_CAPACITIES[:-1])
def test_oracle_stratified_counts_equal_integer_leaves_and_the_fp32_tree_is_exact(capacity):
    leaves = O.exact_leaves(capacity)
    total = int(leaves.sum())
    assert total & (total - 1) == 0 and total < 2 ** 24
    o = O.Index64(capacity)
    o.rebuild(leaves, 1.0, 0.0)
    u = np.full(total, 0.5, dtype=np.float32)
    idx = o.sample(u)
    assert np.array_equal(np.bincount(idx, minlength=capacity), leaves.astype(np.int64))
    t = O.Tree32(leaves)
    assert float(t.total) == total and float(t.min[0][0]) == leaves.min()
    idx32, leaf32 = t.sample(u)
    assert np.array_equal(idx32, idx) and np.array_equal(leaf32, leaves[idx])
    ud = O.dyadic_u(256, capacity)
    assert np.array_equal(t.sample(ud)[0], o.sample(ud)) and np.array_equal(t.sample(ud, False)[0], o.sample(ud, False))


def test_scan32_is_the_pairwise_order_and_unfilled_slots_are_never_drawn():
    c = np.random.default_rng(2).uniform(0, 1, size=64).astype(np.float32)
    x = c.copy()
    while x.size > 1:
        x = (x[0::2] + x[1::2]).astype(np.float32)           # ((c0+c1)+(c2+c3))+...
    assert O.scan32(c)[63] == x[0]
    assert np.allclose(O.scan32(c), np.cumsum(c.astype(np.float64)), rtol=1e-6)
    leaves = np.zeros(4097, dtype=np.float32)
    leaves[[0, 2000, 4096]] = (0.3, 1e-4, 7.0)
    t, o = O.Tree32(leaves), O.Index64(4097)
    o.rebuild(leaves, 1.0, 0.0)
    u = np.array([0.0, np.nextafter(np.float32(1), np.float32(0)), np.nan, 0.5], dtype=np.float32)
    for stratified in (True, False):
        assert set(t.sample(u, stratified)[0]) <= {0, 2000, 4096} and set(o.sample(u, stratified)) <= {0, 2000, 4096}
    assert t.sample(u, False)[0][0] == 0 and t.sample(u, False)[0][1] == 4096
    assert np.array_equal(O.Tree32(np.zeros(70, dtype=np.float32)).sample(u)[0], [-1] * 4)


@pytest.mark.parametrize("capacity,live", O.GENERAL_CASES)
@pytest.mark.parametrize("alpha", (0.0, 0.6, 1.0))
def test_boundary_samples_of_the_gpu_tiers_seeds_are_under_one_percent(capacity, live, alpha):
    slots, pri = O.general_case(capacity, live)
    assert pri.max() / pri.min() > 1e5 and len(set(slots)) == live
    o = O.Index64(capacity)
    o.update(slots, pri, alpha, 1e-6)
    u = O.general_u(capacity)
    for stratified in (True, False):
        near = o.near_boundary(u, stratified, O.TOL_REL * o.total)
        assert near.sum() < 0.01 * O.GENERAL_B, (stratified, int(near.sum()))
    # the fp32 descent agrees with the fp64 search off the boundaries
    idx32, _ = O.Tree32(o.leaves).sample(u)
    differ = idx32 != o.sample(u)
    assert not (differ & ~o.near_boundary(u, True, O.TOL_REL * o.total)).any()


# ---------------------------------------------------------------------------------------------------------------------
# the bindings and the Python API
# ---------------------------------------------------------------------------------------------------------------------
def test_bindings_name_the_wrong_argument_on_host_tensors():
    import hpc_replay as R
    words = R.per_state_words(100)
    assert words == O.state_words(100, SCALAR_WORDS) and R.per_layout(100)[0] == 2
    state = torch.zeros(words, dtype=torch.int32)
    assert R.per_capacity(state) == 100
    idx, pri, u = torch.zeros(4, dtype=torch.int64), torch.zeros(4), torch.zeros(4)
    for fn, args, msg in (
            (R.per_state_words, (0,), "capacity: expected at least 1"),
            (R.per_state_words, (2 ** 24 + 1,), "capacity: at most 16777216"),
            (R.per_init, (state.float(),), "state: dtype"),
            (R.per_init, (state.view(2, -1),), "state: shape"),
            (R.per_init, (state[:10],), "the state of no capacity"),
            (R.per_update, (state, idx.int(), pri), "idx: dtype"),
            (R.per_update, (state, idx.view(2, 2), pri), "idx: shape"),
            (R.per_update, (state, idx, pri.double()), "priority: dtype"),
            (R.per_update, (state, idx, pri[:3]), "priority: shape"),
            (R.per_update, (state, idx, pri, -0.5), "alpha: expected a value >= 0"),
            (R.per_update, (state, idx, pri, 0.6, -1.0), "eps: expected a value >= 0"),
            (R.per_rebuild, (state, torch.zeros(99)), "priorities: shape"),
            (R.per_rebuild, (state, torch.zeros(100).double()), "priorities: dtype"),
            (R.per_sample, (state, u.double(), 0.4, 10), "u: dtype"),
            (R.per_sample, (state, u.view(2, 2), 0.4, 10), "u: shape"),
            (R.per_sample, (state, u, -0.4, 10), "beta: expected a value >= 0"),
            (R.per_sample, (state, u, 0.4, 0), "size: expected at least 1"),
            (R.per_sample, (state, u, 0.4, 1, torch.zeros(1)), "size: dtype"),
            (R.per_sample, (state, u, 0.4, 1, torch.zeros(2, dtype=torch.int64)), "size: shape"),
            (R.per_sample, (state, u, 0.4, 10, None, True, 3), "normalize: unknown mode 3"),
            (R.per_init, (state,), "state: must live on a GPU"),
            (R.per_update, (state, idx, pri), "state: must live on a GPU"),
            (R.per_rebuild, (state, torch.zeros(100)), "state: must live on a GPU"),
            (R.per_sample, (state, u, 0.4, 10), "state: must live on a GPU")):
        with pytest.raises(RuntimeError, match=re.escape(msg)):
            fn(*args)


def test_python_api_messages_and_signatures():
    import inspect
    from hpc_rll.rl_utils import per as M
    state = torch.zeros(M.hpc_replay.per_state_words(64), dtype=torch.int32)
    with pytest.raises(ValueError, match="normalize"):
        M.per_sample(state, 4, 0.4, 10, normalize="max")
    with pytest.raises(RuntimeError, match=re.escape("u: shape (3,), expected (4,)")):
        M.per_sample(state, 4, 0.4, 10, u=torch.zeros(3))
    with pytest.raises(TypeError, match="capacity"):
        M.per_init(64.0, "cpu")
    with pytest.raises(RuntimeError, match="must live on a GPU"):
        M.per_init(64, "cpu")
    with pytest.raises(RuntimeError, match="must live on a GPU"):
        M.per_sample(state, 4, 0.4, 10, generator=torch.Generator().manual_seed(0))
    with pytest.raises(RuntimeError, match="must live on a GPU"):
        M.PrioritizedReplayIndex(64, device="cpu")
    assert list(inspect.signature(M.per_init).parameters) == ["capacity", "device"]
    assert list(inspect.signature(M.per_update).parameters) == ["state", "idx", "priority", "alpha", "eps"]
    assert list(inspect.signature(M.per_rebuild).parameters) == ["state", "priorities", "alpha", "eps"]
    assert list(inspect.signature(M.per_sample).parameters) == ["state", "batch_size", "beta", "size", "u", "stratified",
                                                                "normalize", "generator"]
    assert inspect.signature(M.per_update).parameters["alpha"].default == 0.6
    assert inspect.signature(M.per_sample).parameters["normalize"].default == "buffer"
    for name in ("append", "update", "sample", "total", "max_priority", "priorities"):
        assert hasattr(M.PrioritizedReplayIndex, name), name
    assert "not graph-capturable" in M.PrioritizedReplayIndex.append.__doc__.lower()


def test_pybind_surface_matches_the_record():
    import hpc_replay
    snap = os.path.join(ROOT, "tests", "golden", "ext_signatures_replay.json")
    got = {n: getattr(hpc_replay, n).__doc__ for n in dir(hpc_replay)
           if not n.startswith("__") and callable(getattr(hpc_replay, n))}
    want = json.load(open(snap))["hpc_replay"]
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], f"hpc_replay.{name}:\n{got[name]}\n-- recorded --\n{want[name]}"
    assert {"per_init", "per_update", "per_rebuild", "per_sample", "per_layout", "per_state_words", "per_last_config"} <= set(got)
