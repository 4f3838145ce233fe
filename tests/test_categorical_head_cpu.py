"""CPU tier of the categorical head's dispatch record (``hpc_rll_categorical_last_config``, csrc/categorical.hip): the parts
that need no GPU -- the entry point and its constants are declared and exported, it refuses a NULL output and an unknown
direction, reports "no launch yet" as {0, -1 ...}, and calls that return before launching leave it as it was.  Everything
that launches is in tests/test_categorical_head_gpu.py."""
import ctypes

import pytest

LAST, FWD, BWD = "hpc_rll_categorical_last_config", "hpc_rll_categorical_forward", "hpc_rll_categorical_backward"
EINVAL = -1
INTS = 8


def test_c_entry_point_declared_and_exported():
    import cabi
    P, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert LAST in cabi.SIGNATURES and hasattr(cabi.lib, LAST)
    assert cabi.SIGNATURES[LAST] == (I, [I, P])
    assert cabi.SIGNATURES[FWD] == (I, [P, P, P, P, L, I, P])
    assert cabi.SIGNATURES[BWD] == (I, [P] * 7 + [L, I, P])
    assert cabi.lib.hpc_rll_abi_version() == 6
    hdr = open(cabi.HEADER_PATH).read()
    assert f"#define HPC_RLL_CATEGORICAL_CONFIG_INTS ({INTS})" in hdr
    assert "#define HPC_RLL_CAT_DIR_FORWARD (0)" in hdr and "#define HPC_RLL_CAT_DIR_BACKWARD (1)" in hdr
    for i, name in enumerate(("ROW", "SMALL", "BLOCKROW", "LDSROW", "LONG", "PPO_FUSED")):
        assert f"#define HPC_RLL_CAT_FAMILY_{name} ({i})" in hdr, name


@pytest.fixture(scope="module")
def buf():
    """A small host buffer as a stand-in for device memory: the calls below return before anything reads it."""
    b = (ctypes.c_float * 64)()
    assert ctypes.addressof(b) % 8 == 0
    return b


def test_null_and_unknown_directions_are_refused():
    import cabi
    L = cabi.lib
    out = (ctypes.c_int * INTS)(*([77] * INTS))
    for d in (0, 1):
        assert L.hpc_rll_categorical_last_config(d, None) == EINVAL
    for d in (-1, 2, 3, 1 << 20):
        assert L.hpc_rll_categorical_last_config(d, out) == EINVAL, d
    assert list(out) == [77] * INTS                                # a refused call writes nothing


def test_record_is_empty_and_calls_that_launch_nothing_leave_it_so(buf):
    import cabi
    P = ctypes.addressof(buf)
    L = cabi.lib
    before = []
    for d in (0, 1):
        out = (ctypes.c_int * INTS)(*([77] * INTS))
        assert L.hpc_rll_categorical_last_config(d, out) == 0
        before.append(list(out))
        if out[0] == 0:                                            # nothing in this tier launches; a GPU test of the same process may have
            assert list(out) == [0] + [-1] * (INTS - 1), (d, list(out))
    # empty: nothing launched
    assert L.hpc_rll_categorical_forward(P, P, P, P, 0, 6, None) == 0
    assert L.hpc_rll_categorical_backward(P, P, P, None, None, None, P, 0, 6, None) == 0
    # argument errors: sizes, then nulls
    assert L.hpc_rll_categorical_forward(P, P, P, P, -1, 6, None) == EINVAL
    assert L.hpc_rll_categorical_forward(P, P, P, P, 4, 0, None) == EINVAL
    for null in range(3):
        a = [P, P, P, P]
        a[null] = None
        assert L.hpc_rll_categorical_forward(*a, 4, 6, None) == EINVAL, null
    assert L.hpc_rll_categorical_backward(P, P, P, None, None, None, P, -1, 6, None) == EINVAL
    assert L.hpc_rll_categorical_backward(P, P, P, None, None, None, P, 4, -2, None) == EINVAL
    for null in (0, 1, 2, 6):
        a = [P, P, P, None, None, None, P]
        a[null] = None
        assert L.hpc_rll_categorical_backward(*a, 4, 6, None) == EINVAL, null
    for d in (0, 1):
        out = (ctypes.c_int * INTS)()
        assert L.hpc_rll_categorical_last_config(d, out) == 0 and list(out) == before[d], d
