"""TEST-ONLY: the dispatch rules of csrc/pad_scatter.hip restated in Python, for tests/test_pad_scatter_direct_gpu.py and
tests/test_pad_scatter_cpu.py.  Every function returns the seven ints ``hpc_rll_pad_scatter_last_config`` must show after
the launch count -- {kernel, grid.x, grid.y * grid.z, threads, dynamic LDS bytes, two ints by op} -- computed from the shapes,
the ADDRESSES and the tune keys alone, by the rules the planners of csrc/padsc_plan.hpp and include/hpc_rll_hip.h state.  The rules are also checked against the C++
on the CPU: tests/test_pad_scatter_cpu.py compiles the planners alone (tests/padsc_plan_main.cpp) and compares them with
these functions over a sweep of shapes, addresses and keys.
The constants are read from the header, so they cannot drift from it."""
import ctypes
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hpc_rll_hip.h")
_DEFS = dict(re.findall(r"#define HPC_RLL_PADSC_(\w+) \((\d+)\)", open(HEADER).read()))
OP = {k[3:]: int(v) for k, v in _DEFS.items() if k.startswith("OP_")}
K = {k[7:]: int(v) for k, v in _DEFS.items() if k.startswith("KERNEL_")}
OPS, KERNELS = int(_DEFS["OPS"]), int(_DEFS["KERNELS"])
INTS = int(re.search(r"#define HPC_RLL_PAD_SCATTER_CONFIG_INTS \((\d+)\)", open(HEADER).read()).group(1))
COLL_ROWS = 32            # kScatterCollRows


def config(op):
    import cabi
    out = (ctypes.c_int * INTS)(*([77] * INTS))
    assert cabi.lib.hpc_rll_pad_scatter_last_config(OP[op] if isinstance(op, str) else op, out) == 0
    return list(out)


def cdiv(a, b):
    return (a + b - 1) // b


def al16(*ptrs):
    return all(p % 16 == 0 for p in ptrs)


def rows_per_wg(L):
    """packed_rows_per_wg: the rows of max_len floats that 60 KB of LDS hold beside 160 floats of slack, 16 at the most."""
    return min(16, (60 * 1024 // 4 - 160) // max(L, 1))


def packed_lds(RB, L):
    return ((RB * L + 8 + 1) & ~1) * 4 + (RB + 1) * 8


def pad_rule(n, m0, m1, m2, new_x, mask, handed=0):
    total = n * m0 * m1 * m2
    v4 = total % 4 == 0 and al16(new_x, mask)
    kernel = K["PAD1D4"] if v4 and m0 == 1 and m1 == 1 and total < 2 ** 32 else K["PAD4"] if v4 else K["PAD"]
    return [kernel, min(cdiv(total // 4 if v4 else total, 256), 4096), 1, 256, 0, 4 if v4 else 1, handed]


def unpad_rule(n, total, m0, m1, m2, padded, handed=0):
    pt = n * m0 * m1 * m2
    if m0 == 1 and m1 == 1 and m2 > 0 and pt % 4 == 0 and pt < 2 ** 32 and al16(padded):
        return [K["UNPAD1D4"], min(cdiv(pt // 4, 256), 4096), 1, 256, 0, 4, handed]
    return [K["UNPAD"], min(cdiv(total, 256), 4096), 1, 256, 0, 1, handed]


def pad_packed_rule(n, L, new_x, mask, key28=1):
    """-> (the packed op's record, the list op's record or None)."""
    RB = rows_per_wg(L)
    al = al16(new_x, mask)
    if al and 32 <= L <= 16384 and key28:
        return [K["PAD1D_PACKED_WAVE"], min(cdiv(cdiv(n * L, 1024), 4), 1 << 20), 1, 256, 0, RB, 0], None
    if al and RB >= 1:
        return [K["PAD1D_PACKED"], min(cdiv(n, RB), 1 << 20), 1, 256, packed_lds(RB, L), RB, 0], None
    return [K["HANDED_OVER"], 0, 0, 0, 0, RB, 1], pad_rule(n, 1, 1, L, new_x, mask, handed=1)


def unpad_packed_rule(n, total, L, padded):
    RB = rows_per_wg(L)
    if RB >= 1 and al16(padded):
        return [K["UNPAD1D_PACKED"], min(cdiv(n, RB), 1 << 20), 1, 256, packed_lds(RB, L), RB, 0], None
    return [K["HANDED_OVER"], 0, 0, 0, 0, RB, 1], unpad_rule(n, total, 1, 1, L, padded, handed=1)


def fwd_flags(add, build, parts, vec):
    return int(bool(add)) | (2 if build else 0) | (parts << 2) | (16 if vec else 0)


def scatter_fwd_rule(B, M, N, H, W, add, x, out, key17=1, key18=0, key37=1):
    HW = H * W
    index_parts = (3 if M > 256 else 1) if add else 2
    build = bool(key37 and W > 0 and (not add or (M <= 256 and HW >= 1024)))
    lds_pays = (not add) or HW * 4 <= 8192 or key18 != 0 or build
    if key17 and lds_pays and HW % 4 == 0 and al16(out) and M > 0 and HW * 4 <= 32 * 1024:
        ab = bool(add and build)
        fixed = HW * 4 + (M * 4 if add else 0) + ((((M + 3) & ~3) * 4 + 16 + (2 * COLL_ROWS + 2) * 4) if ab else 0)
        rows = M + (COLL_ROWS if ab else 0)
        cap = (100 if key18 else 60 if ab else 52) * 1024
        npb = 0
        for c in ([key18] if key18 else [64, 32, 16, 8, 4]):
            if 1 <= c <= 64 and rows * (c + 1) * 4 + 16 + fixed <= cap:
                npb = c
                break
        if npb > N:
            npb = (N + 3) // 4 * 4
        if npb >= 1 and rows * (npb + 1) * 4 + 16 + fixed <= cap:
            lds = ((rows * (npb + 1) + 3) & ~3) * 4 + fixed
            vec = N % 4 == 0 and npb % 4 == 0 and al16(x)
            return [K["SCATTER_OUT_LDS"], cdiv(N, npb), B, 1024, lds, npb, fwd_flags(add, build, 0 if build else index_parts, vec)]
    v4 = HW % 4 == 0 and N % 4 == 0 and al16(x, out)
    tpb = 1024 if v4 and HW >= 4096 else 256
    cell_blocks = (HW + (4 * tpb - 1 if v4 else 255)) // (4 * tpb if v4 else 256)
    npb = N
    while npb > 4 and B * cell_blocks * cdiv(N, npb) < 2048:
        npb = (npb // 2 + 3) // 4 * 4
    if v4:
        return [K["SCATTER_OUT4"], cell_blocks, cdiv(N, npb) * B, tpb, 0, npb, fwd_flags(add, False, index_parts, True)]
    return [K["SCATTER_OUT"], cell_blocks, cdiv(N, npb) * B, 256, 0, npb, fwd_flags(add, False, index_parts, N % 4 == 0 and al16(x))]


def scatter_bwd_rule(B, M, N, H, W, grad_out, key38=1, key40=0):
    HW = H * W
    if HW == 0:
        return [K["SCATTER_BWD_MEMSET"], 0, 0, 0, 0, 0, 0]
    plane = HW * 4
    pieces = min(N, max(1, 65536 // plane)) * 4
    tile_rule = key40 == 2 or (key40 == 0 and pieces <= 16 and M * 16 >= HW)
    if tile_rule and W % 4 == 0 and M <= 4096 and B <= 65535 and al16(grad_out) and N * W * 4 <= 65536:
        TR = min(65536 // (N * W * 4), H)
        TR = 1 << (TR.bit_length() - 1)
        cells = TR * W
        pays = (cells * 4 >= 1024 and M * 16 >= HW) or (cells * 4 >= 512 and M * 4 >= HW)
        if pays or key40 == 2:
            return [K["SCATTER_BWD_TILE"], cdiv(H, TR), B, 1024, N * cells * 4 + 16 + M * 8, TR, 0]
    if plane <= 128 * 1024 and B <= 65535:
        NG = min(N, max(1, 65536 // plane), 32)
        gx = cdiv(N, NG)
        xo = int((key38 == 2 or (key38 == 1 and NG * 4 <= 32)) and (gx * B) % 8 == 0 and gx > 1)
        return [K["SCATTER_BWD_LDS"], gx, B, 1024, NG * plane, NG, 2 if xo and B % 8 == 0 else xo]
    return [K["SCATTER_BWD_DIRECT"], min(cdiv(B * M * N, 256), 8192), 1, 256, 0, 0, 0]
