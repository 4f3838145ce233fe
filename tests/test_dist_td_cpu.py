"""CPU tier of the dispatch record of the distributional TD ops (``hpc_rll_dist_last_config``, csrc/dist_ops.hip): the parts
that need no GPU -- the entry point and its constants are declared and exported, it refuses a NULL output and an unknown op,
a fresh process reports "no launch yet" as {0, -1 ...} for each of the three ops, and calls that return before launching
leave every record as it was.  Everything that launches is in tests/test_dist_td_gpu.py."""
import ctypes
import os
import subprocess
import sys

import pytest

LAST = "hpc_rll_dist_last_config"
EINVAL = -1
INTS = 8
OPS = (0, 1, 2)                                                    # C51, IQN, QR-DQN


def test_c_entry_point_declared_and_exported():
    import cabi
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert LAST in cabi.SIGNATURES and hasattr(cabi.lib, LAST)
    assert cabi.SIGNATURES[LAST] == (I, [I, P])
    assert cabi.SIGNATURES["hpc_rll_dist_nstep_td_forward"] == (I, [P] * 11 + [I] * 4 + [F] * 4 + [P])
    assert cabi.SIGNATURES["hpc_rll_iqn_nstep_td_forward"] == (I, [P] * 13 + [I] * 5 + [F] * 3 + [P])
    assert cabi.SIGNATURES["hpc_rll_iqn_nstep_td_forward_bnt"] == cabi.SIGNATURES["hpc_rll_iqn_nstep_td_forward"]
    assert cabi.SIGNATURES["hpc_rll_qrdqn_nstep_td_forward"] == (I, [P] * 12 + [I] * 4 + [F] * 3 + [P])
    assert cabi.lib.hpc_rll_abi_version() == 6
    hdr = open(cabi.HEADER_PATH).read()
    assert f"#define HPC_RLL_DIST_CONFIG_INTS ({INTS})" in hdr
    for i, name in enumerate(("C51", "IQN", "QRDQN")):
        assert f"#define HPC_RLL_DIST_OP_{name} ({i})" in hdr, name
    assert "#define HPC_RLL_DIST_OPS (3)" in hdr
    for i, name in enumerate(("WAVE", "GROUP", "BATCH", "QUAD", "WAVE64", "GENERAL")):
        assert f"#define HPC_RLL_DIST_FAMILY_{name} ({i})" in hdr, name


def test_null_and_unknown_ops_are_refused():
    import cabi
    L = cabi.lib
    out = (ctypes.c_int * INTS)(*([77] * INTS))
    for op in OPS:
        assert L.hpc_rll_dist_last_config(op, None) == EINVAL
    for op in (-1, 3, 4, 1 << 20, -(1 << 31)):
        assert L.hpc_rll_dist_last_config(op, out) == EINVAL, op
    assert list(out) == [77] * INTS                                # a refused call writes nothing


def test_a_fresh_process_reports_no_launch_for_every_op():
    """In a process of its own (this one may have launched: the GPU tier runs in the same session on a GPU machine)."""
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import ctypes, sys; sys.path.insert(0, %r); import cabi\n"
            "for op in (0, 1, 2):\n"
            "    out = (ctypes.c_int * %d)(*([77] * %d))\n"
            "    assert cabi.lib.hpc_rll_dist_last_config(op, out) == 0\n"
            "    print(op, list(out))\n" % (here, INTS, INTS))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    want = "".join(f"{op} {[0] + [-1] * (INTS - 1)}\n" for op in OPS)
    assert r.stdout == want, r.stdout


@pytest.fixture(scope="module")
def buf():
    """A small host buffer as a stand-in for device memory: the calls below return before anything reads it."""
    b = (ctypes.c_float * 64)()
    assert ctypes.addressof(b) % 8 == 0
    return b


def _records():
    import cabi
    recs = []
    for op in OPS:
        out = (ctypes.c_int * INTS)(*([77] * INTS))
        assert cabi.lib.hpc_rll_dist_last_config(op, out) == 0
        recs.append(list(out))
    return recs


def test_calls_that_launch_nothing_leave_the_records_as_they_were(buf):
    import cabi
    P = ctypes.addressof(buf)
    L = cabi.lib
    before = _records()
    for rec in before:
        if rec[0] == 0:                                            # nothing in this tier launches; a GPU test of the same process may have
            assert rec == [0] + [-1] * (INTS - 1), rec
    c51 = lambda ptrs, nstep=1, B=4, N=3, n_atom=51: L.hpc_rll_dist_nstep_td_forward(   # noqa: E731
        *ptrs, nstep, B, N, n_atom, 0.9, -10.0, 10.0, 0.25, None)
    iqn = lambda fn, ptrs, tau=8, taup=8, nstep=1, B=4, N=3, kappa=1.0: getattr(L, fn)(   # noqa: E731
        *ptrs, tau, taup, nstep, B, N, 0.9, kappa, 0.25, None)
    qr = lambda ptrs, tau=8, nstep=1, B=4, N=3: L.hpc_rll_qrdqn_nstep_td_forward(        # noqa: E731
        *ptrs, tau, nstep, B, N, 0.9, 8.0, 0.25, None)
    # C51: dist, next_dist, action, next_action, reward, done, weight (optional), loss, td_err, buf, partials
    full = [P] * 11
    assert c51(full, nstep=-1) == EINVAL and c51(full, B=-1) == EINVAL and c51(full, N=0) == EINVAL
    assert c51(full, n_atom=1) == EINVAL
    for null in (0, 1, 2, 3, 4, 5, 7, 8, 9, 10):
        a = list(full)
        a[null] = None
        assert c51(a) == EINVAL, null
    # IQN, both layouts: q, next_q, action, next_action, reward, done, replay_quantiles, weight, value_gamma (both optional),
    # loss, td_err, buf, partials
    full = [P] * 13
    for fn in ("hpc_rll_iqn_nstep_td_forward", "hpc_rll_iqn_nstep_td_forward_bnt"):
        assert iqn(fn, full, tau=0) == EINVAL and iqn(fn, full, taup=0) == EINVAL and iqn(fn, full, nstep=-1) == EINVAL
        assert iqn(fn, full, B=-1) == EINVAL and iqn(fn, full, N=0) == EINVAL and iqn(fn, full, kappa=0.0) == EINVAL
        for null in (0, 1, 2, 3, 4, 5, 6, 9, 10, 11, 12):
            a = list(full)
            a[null] = None
            assert iqn(fn, a) == EINVAL, (fn, null)
    # QR-DQN: q, next_q, action, next_action, reward, done, weight, value_gamma (both optional), loss, td_err, buf, partials
    full = [P] * 12
    assert qr(full, tau=0) == EINVAL and qr(full, nstep=-1) == EINVAL and qr(full, B=-1) == EINVAL and qr(full, N=0) == EINVAL
    for null in (0, 1, 2, 3, 4, 5, 8, 9, 10, 11):
        a = list(full)
        a[null] = None
        assert qr(a) == EINVAL, null
    assert _records() == before
