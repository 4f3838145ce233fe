"""CPU tier of the pad / unpad / scatter family (csrc/pad_scatter.hip): the parts that need no GPU -- the dispatch record
``hpc_rll_pad_scatter_last_config`` is declared and exported with its constants, refuses a NULL output and an unknown op, and
reads {0, -1 ...} for each of the six ops in a fresh process; the six launching entry points answer argument errors and empty
shapes with statuses before any HIP call and leave every record as it was; the float32 row formula of
``pad1d_packed_wave_kernel`` is exact on its whole domain; ``packed_rows_per_wg`` restated at the widths where it changes.
Everything that launches is in tests/test_pad_scatter_direct_gpu.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np

import padsc

LAST = "hpc_rll_pad_scatter_last_config"
EINVAL, EUNSUPPORTED = -1, -3
OP_NAMES = ("PAD", "UNPAD", "PAD_PACKED", "UNPAD_PACKED", "SCATTER_FWD", "SCATTER_BWD")
KERNEL_NAMES = ("PAD", "PAD4", "PAD1D4", "UNPAD", "UNPAD1D4", "PAD1D_PACKED", "PAD1D_PACKED_WAVE", "UNPAD1D_PACKED", "HANDED_OVER",
                "SCATTER_OUT", "SCATTER_OUT4", "SCATTER_OUT_LDS", "SCATTER_BWD_LDS", "SCATTER_BWD_TILE", "SCATTER_BWD_DIRECT",
                "SCATTER_BWD_MEMSET")


def test_c_entry_point_declared_and_exported():
    import cabi
    P, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert LAST in cabi.SIGNATURES and hasattr(cabi.lib, LAST)
    assert cabi.SIGNATURES[LAST] == (I, [I, P])
    assert cabi.SIGNATURES["hpc_rll_pad_forward"] == (I, [P, P, P, L, I, I, I, I, P])             # no signature moved
    assert cabi.SIGNATURES["hpc_rll_unpad_forward"] == (I, [P, P, P, L, L, I, I, I, P])
    assert cabi.SIGNATURES["hpc_rll_pad1d_packed_forward"] == (I, [P, P, P, P, L, I, I, P])
    assert cabi.SIGNATURES["hpc_rll_unpad1d_packed_forward"] == (I, [P, P, P, L, L, I, P])
    assert cabi.SIGNATURES["hpc_rll_scatter_connection_forward"] == (I, [P, P, P, P, I, I, I, I, I, I, P])
    assert cabi.SIGNATURES["hpc_rll_scatter_connection_backward"] == (I, [P, P, P, I, I, I, I, I, P])
    assert cabi.lib.hpc_rll_abi_version() == 6
    hdr = open(cabi.HEADER_PATH).read()
    assert "#define HPC_RLL_PAD_SCATTER_CONFIG_INTS (8)" in hdr and padsc.INTS == 8
    for i, name in enumerate(OP_NAMES):
        assert f"#define HPC_RLL_PADSC_OP_{name} ({i})" in hdr, name
    assert "#define HPC_RLL_PADSC_OPS (6)" in hdr
    for i, name in enumerate(KERNEL_NAMES):
        assert f"#define HPC_RLL_PADSC_KERNEL_{name} ({i})" in hdr, name
    assert f"#define HPC_RLL_PADSC_KERNELS ({len(KERNEL_NAMES)})" in hdr
    assert sorted(padsc.K) == sorted(KERNEL_NAMES) and sorted(padsc.OP) == sorted(OP_NAMES)


def test_null_and_unknown_ops_are_refused():
    import cabi
    L = cabi.lib
    out = (ctypes.c_int * 8)(*([77] * 8))
    for op in range(6):
        assert L.hpc_rll_pad_scatter_last_config(op, None) == EINVAL
    for op in (-1, 6, 7, 1 << 20, -(1 << 31)):
        assert L.hpc_rll_pad_scatter_last_config(op, out) == EINVAL, op
    assert list(out) == [77] * 8                                       # a refused call writes nothing


def test_a_fresh_process_reports_no_launch_for_every_op():
    """In a process of its own (this one may have launched: the GPU tier runs in the same session on a GPU machine)."""
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import ctypes, sys; sys.path.insert(0, %r); import cabi\n"
            "for op in range(6):\n"
            "    out = (ctypes.c_int * 8)(*([77] * 8))\n"
            "    assert cabi.lib.hpc_rll_pad_scatter_last_config(op, out) == 0\n"
            "    print(op, list(out))\n" % here)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout == "".join(f"{op} {[0] + [-1] * 7}\n" for op in range(6)), r.stdout


def test_argument_statuses_come_before_any_launch_and_leave_the_records_alone():
    """Sizes, then empty shapes (which need no pointers), then null operands, then the limits -- the order the six entry
    points check in.  The pointers are host memory: none of these calls reads them."""
    import cabi
    L = cabi.lib
    buf = (ctypes.c_float * 64)(*([7.0] * 64))
    P = ctypes.addressof(buf)
    before = [padsc.config(op) for op in range(6)]
    for rec in before:
        if rec[0] == 0:                                                # nothing in this tier launches; a GPU test of the same process may have
            assert rec == [0] + [-1] * 7, rec
    pad = lambda table=P, new_x=P, mask=P, n=2, m0=1, m1=1, m2=4, value=0: L.hpc_rll_pad_forward(table, new_x, mask, n, m0, m1, m2, value, None)   # noqa: E731
    unpad = lambda padded=P, table=P, flat=P, n=2, total=5, m0=1, m1=1, m2=4: L.hpc_rll_unpad_forward(padded, table, flat, n, total, m0, m1, m2, None)   # noqa: E731
    ppad = lambda flat=P, table=P, new_x=P, mask=P, n=2, L_=4, value=0: L.hpc_rll_pad1d_packed_forward(flat, table, new_x, mask, n, L_, value, None)   # noqa: E731
    punpad = lambda padded=P, table=P, flat=P, n=2, total=5, L_=4: L.hpc_rll_unpad1d_packed_forward(padded, table, flat, n, total, L_, None)   # noqa: E731
    fwd = lambda x=P, loc=P, out=P, ws=P, B=1, M=2, N=3, H=2, W=2, add=0: L.hpc_rll_scatter_connection_forward(x, loc, out, ws, B, M, N, H, W, add, None)   # noqa: E731
    bwd = lambda go=P, loc=P, gx=P, B=1, M=2, N=3, H=2, W=2: L.hpc_rll_scatter_connection_backward(go, loc, gx, B, M, N, H, W, None)   # noqa: E731
    # list pad
    assert pad(n=-1) == EINVAL and pad(m0=-1) == EINVAL and pad(m1=-1) == EINVAL and pad(m2=-1) == EINVAL
    assert pad(m0=2048, m1=1024, m2=1024) == EUNSUPPORTED and pad(m0=2048, m1=1024, m2=1024, n=0) == EUNSUPPORTED
    assert pad(n=0) == 0 and pad(m2=0) == 0 and pad(n=0, table=None, new_x=None, mask=None) == 0
    assert pad(table=None) == EINVAL and pad(new_x=None) == EINVAL and pad(mask=None) == EINVAL
    # list unpad
    assert unpad(n=-1) == EINVAL and unpad(total=-1) == EINVAL and unpad(m0=-1) == EINVAL and unpad(m2=-1) == EINVAL
    assert unpad(n=0) == 0 and unpad(total=0) == 0 and unpad(total=0, padded=None, table=None, flat=None) == 0
    assert unpad(padded=None) == EINVAL and unpad(table=None) == EINVAL and unpad(flat=None) == EINVAL
    # packed pad / unpad
    assert ppad(n=-1) == EINVAL and ppad(L_=-1) == EINVAL and ppad(n=0) == 0 and ppad(L_=0) == 0
    assert ppad(n=0, flat=None, table=None, new_x=None, mask=None) == 0
    assert ppad(flat=None) == EINVAL and ppad(table=None) == EINVAL and ppad(new_x=None) == EINVAL and ppad(mask=None) == EINVAL
    assert punpad(n=-1) == EINVAL and punpad(total=-1) == EINVAL and punpad(L_=-1) == EINVAL
    assert punpad(n=0) == 0 and punpad(total=0) == 0 and punpad(L_=0) == 0 and punpad(n=0, padded=None, table=None, flat=None) == 0
    assert punpad(padded=None) == EINVAL and punpad(table=None) == EINVAL and punpad(flat=None) == EINVAL
    # scatter forward
    for name in ("B", "M", "N", "H", "W"):
        assert fwd(**{name: -1}) == EINVAL, name
        assert bwd(**{name: -1}) == EINVAL, name
    assert fwd(B=0) == 0 and fwd(N=0) == 0 and fwd(H=0) == 0 and fwd(W=0, out=None, ws=None) == 0
    assert fwd(out=None) == EINVAL and fwd(ws=None) == EINVAL and fwd(x=None) == EINVAL and fwd(loc=None) == EINVAL
    assert fwd(B=65536) == EUNSUPPORTED and fwd(H=65536, W=32768) == EUNSUPPORTED
    assert fwd(B=65536, out=None) == EINVAL                              # the null check comes first
    # scatter backward (an empty map with entities clears grad_x with a memset: that one needs a GPU)
    assert bwd(B=0) == 0 and bwd(M=0) == 0 and bwd(N=0) == 0 and bwd(M=0, go=None, loc=None, gx=None) == 0
    assert bwd(loc=None) == EINVAL and bwd(gx=None) == EINVAL and bwd(go=None) == EINVAL
    assert list(buf) == [7.0] * 64
    assert [padsc.config(op) for op in range(6)] == before


def test_wave_kernel_row_formula_is_exact_on_its_whole_domain():
    """pad1d_packed_wave_kernel finds the row of a quad as (unsigned)(((float)t + 0.5f) * (1.0f / (float)L)), t < L + 1024 the
    offset from the start of the tile's first row: equal to t // L for EVERY 32 <= L <= 16384, as its comment claims."""
    bad = 0
    for L in range(32, 16385):
        t = np.arange(L + 1024, dtype=np.int64)
        inv = np.float32(1.0) / np.float32(L)
        rr = ((t.astype(np.float32) + np.float32(0.5)) * inv)
        assert rr.dtype == np.float32
        bad += int((rr.astype(np.uint32) != t // L).sum())
    assert bad == 0, bad


def test_rows_per_workgroup_of_the_packed_kernels():
    """min(16, (15360 - 160) / max_len): where it leaves 16, where it reaches 1 and where no row fits (the hand-over, and the
    widths only the wave kernel takes)."""
    r = padsc.rows_per_wg
    assert [r(L) for L in (1, 31, 127, 950, 951, 1013, 7600, 7601, 15200, 15201, 16384, 16385)] == [16, 16, 16, 16, 15, 15, 2, 1, 1, 0, 0, 0]
    assert padsc.packed_lds(16, 127) == (16 * 127 + 8) * 4 + 17 * 8 and padsc.packed_lds(1, 15200) <= 64 * 1024
    assert padsc.packed_lds(15, 951) == ((15 * 951 + 8 + 1) & ~1) * 4 + 16 * 8
