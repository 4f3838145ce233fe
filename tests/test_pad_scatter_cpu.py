"""CPU tier of the pad / unpad / scatter family (csrc/pad_scatter.hip): the parts that need no GPU -- the dispatch record
``hpc_rll_pad_scatter_last_config`` is declared and exported with its constants, refuses a NULL output and an unknown op, and
reads {0, -1 ...} for each of the six ops in a fresh process; the six launching entry points answer argument errors and empty
shapes with statuses before any HIP call and leave every record as it was; the float32 row formula of
``pad1d_packed_wave_kernel`` is exact on its whole domain; ``packed_rows_per_wg`` restated at the widths where it changes; the
planners of csrc/padsc_plan.hpp, compiled alone by the host compiler, against tests/padsc.py over a sweep, with every LDS carve.
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


BASE = 1 << 20                                                          # a 16-byte aligned address for the sweep's pointers
OFFS = (0, 4, 8)
CUS = (256, 304, 64, 8)


def plan_sweep():
    """-> [(input line of tests/padsc_plan_main.cpp, the record by tests/padsc.py, the list op's record or None)].
    Scatter: every (B, M, N, map, add) of the sets below; the 108 / 27 combinations of pointer offsets and tune keys are dealt
    over them in turn, six / four per shape, so that the sweep stays at some 60 000 lines and every combination occurs many
    times; the CU count takes 256, 304, 64 and 8 in turn.  Pad: the whole cross product."""
    import itertools as it
    out = []
    Bs, Ms, Ns = (1, 3, 4, 8, 65535), (0, 5, 256, 257, 300, 3000, 4096, 4097), (1, 3, 4, 7, 8, 64, 70, 128)
    maps = ((0, 4), (3, 5), (4, 4), (16, 16), (32, 32), (45, 46), (64, 64), (96, 96), (128, 64), (136, 136), (184, 184))
    fwd_opts = list(it.product(OFFS, OFFS, (0, 1), (0, 4, 64), (0, 1)))          # x, out, key 17, key 18, key 37
    bwd_opts = list(it.product(OFFS, (0, 1, 2), (0, 1, 2)))                      # grad_out, key 38, key 40
    i = j = 0
    for B, M, N, (H, W) in it.product(Bs, Ms, Ns, maps):
        for add in (0, 1):
            for _ in range(6):
                xo, oo, k17, k18, k37 = fwd_opts[i % len(fwd_opts)]
                i += 1
                out.append((f"fwd {B} {M} {N} {H} {W} {add} {BASE + xo} {BASE + oo} {k17} {k18} {k37} {CUS[(i // 7) % len(CUS)]}",
                            padsc.scatter_fwd_rule(B, M, N, H, W, add, BASE + xo, BASE + oo, k17, k18, k37), None))
        for _ in range(4):
            go, k38, k40 = bwd_opts[j % len(bwd_opts)]
            j += 1
            out.append((f"bwd {B} {M} {N} {H} {W} {BASE + go} {k38} {k40}", padsc.scatter_bwd_rule(B, M, N, H, W, BASE + go, k38, k40), None))
    Ls = (1, 5, 31, 32, 33, 950, 951, 7600, 7601, 15200, 15201, 16384, 16385)
    for n, L in it.product((1, 3, 4, 50, 70000), Ls):
        for m0, m1 in ((1, 1), (1, 2), (2, 3)):
            total = max(1, n * m0 * m1 * L // 2)                                 # flat elements of the unpad
            for a, b in it.product(OFFS, OFFS):
                out.append((f"pad {n} {m0} {m1} {L} {BASE + a} {BASE + b}", padsc.pad_rule(n, m0, m1, L, BASE + a, BASE + b), None))
            for a in OFFS:
                out.append((f"unpad {n} {total} {m0} {m1} {L} {BASE + a}", padsc.unpad_rule(n, total, m0, m1, L, BASE + a), None))
        total = max(1, n * L // 2)
        for f, a, b, k28 in it.product(OFFS, OFFS, OFFS, (0, 1)):
            out.append((f"ppad {n} {L} {BASE + f} {BASE + a} {BASE + b} {k28}",) + padsc.pad_packed_rule(n, L, BASE + a, BASE + b, k28))
        for a, f in it.product(OFFS, OFFS):
            out.append((f"punpad {n} {total} {L} {BASE + a} {BASE + f}",) + padsc.unpad_packed_rule(n, total, L, BASE + a))
    return out


def build_plan_program(tmp_path):
    """tests/padsc_plan_main.cpp by the host compiler: c++, else the clang++ the library itself was built with."""
    import shutil
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    cxx = shutil.which("c++") or "/opt/rocm/llvm/bin/clang++"
    exe = os.path.join(str(tmp_path), "padsc_plan")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(root, "include"), "-I" + os.path.join(root, "di-hpc_amd", "csrc"),
                    os.path.join(here, "padsc_plan_main.cpp"), "-o", exe], check=True, timeout=300)
    return exe


def test_the_planners_agree_with_the_restated_rules_and_every_carve_fits(tmp_path):
    """csrc/padsc_plan.hpp, compiled without HIP, against tests/padsc.py on the sweep above: every record, both records of a
    hand-over, for every plan with dynamic LDS the end of the kernel's carve within the bytes the plan requests, and the
    staging prefetch distance of the forward's LDS kernel: half of the workgroups the chip holds (two per CU, one where a
    workgroup's LDS is above 80 KB), rounded down to a multiple of 8."""
    sweep = plan_sweep()
    exe = build_plan_program(tmp_path)
    r = subprocess.run([exe], input="".join(s[0] + "\n" for s in sweep), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = r.stdout.splitlines()
    assert len(got) == len(sweep)
    print(f"{len(sweep)} sweep lines")
    kernels, with_lds = set(), 0
    for (line, own, handed), g in zip(sweep, got):
        t = g.split()
        assert [int(v) for v in t[:7]] == own, (line, g, own)
        kernels.add(own[0])
        rest = t[7:]
        if handed is not None:
            assert rest[0] == "H" and [int(v) for v in rest[1:8]] == handed, (line, g, handed)
            rest = rest[8:]
        if own[4]:
            assert rest[0] == "E" and 0 < int(rest[1]) <= own[4], (line, g)
            with_lds += 1
            rest = rest[2:]
        if own[0] == padsc.K["SCATTER_OUT_LDS"]:
            cus = int(line.split()[-1])
            assert rest[0] == "P" and int(rest[1]) == (cus * (2 if own[4] * 2 <= 160 * 1024 else 1) // 2) & ~7, (line, g)
            rest = rest[2:]
        assert not rest, (line, g)
    assert kernels == set(range(padsc.KERNELS)) and with_lds > 1000


def test_rows_per_workgroup_of_the_packed_kernels():
    """min(16, (15360 - 160) / max_len): where it leaves 16, where it reaches 1 and where no row fits (the hand-over, and the
    widths only the wave kernel takes)."""
    r = padsc.rows_per_wg
    assert [r(L) for L in (1, 31, 127, 950, 951, 1013, 7600, 7601, 15200, 15201, 16384, 16385)] == [16, 16, 16, 16, 15, 15, 2, 1, 1, 0, 0, 0]
    assert padsc.packed_lds(16, 127) == (16 * 127 + 8) * 4 + 17 * 8 and padsc.packed_lds(1, 15200) <= 64 * 1024
    assert padsc.packed_lds(15, 951) == ((15 * 951 + 8 + 1) & ~1) * 4 + 16 * 8
