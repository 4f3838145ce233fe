// padsc_plan.hpp -- what each call of the six pad / scatter entry points of pad_scatter.hip launches, decided from the sizes,
// the ADDRESSES, the tune keys and the CU count alone.  No HIP, no globals, no environment: the entry points fill the
// arguments, the launchers of pad_scatter.hip issue what the plan says, the dispatch record is noted from the plan, and
// tests/padsc_plan_main.cpp evaluates the same functions on the CPU against tests/padsc.py.
// Also here, because kernel and host must agree on them: the layouts of the dynamic LDS of the kernels that carve it.
#pragma once
#include <stdint.h>

#include <algorithm>

#include "hpc_rll_hip.h"

#ifdef __HIPCC__
#define PADSC_HD __host__ __device__
#else
#define PADSC_HD
#endif

namespace hpc_rll {

// the tune keys the planners read (hpc_rll_tune_set, tune.hip), filled from the g_* globals by the caller
struct PadscKeys {
    int pad_wave;           // key 28
    int scatter_lds_fwd;    // key 17
    int scatter_npb;        // key 18
    int scatter_build;      // key 37
    int scatter_bwd_xcd;    // key 38
    int scatter_bwd_tile;   // key 40
};

// One launch.  The first eight members are the dispatch record (hpc_rll_pad_scatter_last_config) after the launch count;
// the rest is what the launcher of the op passes to the kernel beyond the sizes.
struct PadscLaunch {
    int kernel;                  // HPC_RLL_PADSC_KERNEL_*
    unsigned gx, gy, gz;         // the record holds gx and gy * gz
    int threads;
    uint64_t lds;                // dynamic LDS bytes
    int a, b;                    // the two ints by op
    // scatter forward
    int npb;                     // channels per workgroup: npb of the LDS kernel, n_per_block of the other two
    int add, build;
    int index_parts;             // `parts` of the scatter_index_kernel launch in front of the kernel, 0 = no such launch
    int vec;                     // x is staged / read with 16-byte loads
    int pf_wgs;                  // staging prefetch distance of the LDS kernel (HPC_RLL_SCATTER_PF overrides it in the launcher)
    // scatter backward
    int TR, swz, NG, xcd;
    // pad
    int RB, v4;
};

// a packed pad / unpad call: its own launch, or kernel HANDED_OVER and the launch of the list entry point in its stead
struct PadscPacked {
    PadscLaunch own, list;
};

constexpr long kPadGridCap = 256L * 16;       // workgroups of the list pad / unpad kernels (their threads loop)
constexpr long kPackedGridCap = 1L << 20;     // workgroups of the packed kernels
constexpr long kScatterBwdDirectCap = 8192;
constexpr int kScatterCollRows = 32;          // extra x-tile rows for the cells with several entities (add, in-kernel tables)
constexpr int kScatterThreads = 1024;         // threads per workgroup of the cells-per-thread kernel on maps of >= 4096 cells
constexpr long kScatterBwdLdsBytes = 64 * 1024;   // planes staged per backward workgroup (profiles/r04_scatter_bwd_lds.txt)

inline bool padsc_al16(uintptr_t p) { return (p & 15) == 0; }

// ------------------------------------------------------------------------------------------------ LDS layouts
// The packed kernels: RB rows of L floats and 8 of slack, rounded to an 8-byte boundary, then RB + 1 int64 offsets (s_off).
PADSC_HD inline uint64_t packed_tile_floats(int RB, unsigned L) { return ((uint64_t)RB * L + 8 + 1) & ~(uint64_t)1; }
inline uint64_t packed_lds_bytes(int RB, unsigned L) { return packed_tile_floats(RB, L) * 4 + (uint64_t)(RB + 1) * 8; }

// scatter_out_lds_kernel<ADD, BUILD>, in 4-byte units from the start of the dynamic LDS.  The host does not size the launch
// from this (scatter_fwd_lds_bytes does); `end` is there to be checked against it.
struct ScatterFwdCarve {
    long x;        // [rows][npb + 1] floats, rows = M (+ kScatterCollRows for add with in-kernel tables)
    long first;    // [HW]  head (add) / last (cover), 16-byte aligned
    long next;     // [M]   add only
    long cell;     // [M rounded to 4]   add with in-kernel tables
    long coll;     // [kScatterCollRows] cells, [kScatterCollRows] chain heads
    long ncoll;    // the counter
    long end;      // one past the last int the variant touches
    PADSC_HD ScatterFwdCarve(int M, int HW, int npb, bool ADD, bool BUILD) {
        const int rows = M + (ADD && BUILD ? kScatterCollRows : 0), m4 = (M + 3) & ~3;
        x = 0;
        first = ((long)rows * (npb + 1) + 3) & ~3L;
        next = first + HW;
        cell = next + m4;
        coll = next + 2 * m4;
        ncoll = coll + 2 * kScatterCollRows;
        end = !ADD ? next : !BUILD ? next + M : ncoll + 1;
    }
};

// scatter_bwd_tile_kernel: N plane pieces of `cells` floats, the counter (4 ints), the entity list (2 ints per entity)
struct ScatterBwdTileCarve {
    uint64_t cnt, list, end;   // 4-byte units
    PADSC_HD ScatterBwdTileCarve(int M, int N, int cells) {
        cnt = (uint64_t)N * cells;
        list = cnt + 4;
        end = list + 2 * (uint64_t)M;
    }
};

// ------------------------------------------------------------------------------------------------ pad / unpad
inline long padsc_cdiv(long a, long b) { return (a + b - 1) / b; }

// rows per workgroup of the LDS-staged packed kernels: 16 (tests/tools/micro/padbw.hip at n = 2^20, L = 127: 16 rows and
// one workgroup per 16 rows 270 us, 64 rows 303 us, the per-thread kernel 328 us), fewer when 60 KB of LDS hold fewer
inline int packed_rows_per_wg(int L) {
    const long cap = (60L * 1024 / 4 - 160) / (L > 0 ? L : 1);
    return (int)(cap > 16 ? 16 : cap);
}

inline PadscLaunch padsc_launch(int kernel, long gx, long gy, long gz, int threads, uint64_t lds, int a, int b) {
    PadscLaunch p = {};
    p.kernel = kernel;
    p.gx = (unsigned)gx, p.gy = (unsigned)gy, p.gz = (unsigned)gz;
    p.threads = threads;
    p.lds = lds;
    p.a = a, p.b = b;
    return p;
}

// List pad (n * m0 * m1 * m2 > 0): four output elements per thread where the total is a multiple of 4 and new_x and mask are
// 16-byte aligned -- pad1d4_kernel for rank 1 (m0 = m1 = 1) below 2^32 elements, else pad4_kernel -- otherwise pad_kernel.
inline PadscLaunch plan_pad(long n, int m0, int m1, int m2, uintptr_t new_x, uintptr_t mask) {
    const long total = n * m0 * m1 * m2;
    const bool v4 = (total % 4) == 0 && padsc_al16(new_x) && padsc_al16(mask);
    const int kernel = v4 && m0 == 1 && m1 == 1 && total < (1L << 32) ? HPC_RLL_PADSC_KERNEL_PAD1D4
                       : v4                                           ? HPC_RLL_PADSC_KERNEL_PAD4
                                                                      : HPC_RLL_PADSC_KERNEL_PAD;
    PadscLaunch p = padsc_launch(kernel, std::min(padsc_cdiv(v4 ? total / 4 : total, 256), kPadGridCap), 1, 1, 256, 0, v4 ? 4 : 1, 0);
    p.v4 = v4;
    return p;
}

// List unpad (n, total > 0): a quad of the padded tensor per thread for rank 1 where n * m2 is a multiple of 4 below 2^32 and
// `padded` is 16-byte aligned (unpad1d4_kernel), otherwise one flat element per thread (unpad_kernel).
inline PadscLaunch plan_unpad(long n, long total, int m0, int m1, int m2, uintptr_t padded) {
    const long padded_total = n * m0 * m1 * m2;
    const bool v4 = m0 == 1 && m1 == 1 && m2 > 0 && (padded_total % 4) == 0 && padded_total < (1L << 32) && padsc_al16(padded);
    PadscLaunch p = padsc_launch(v4 ? HPC_RLL_PADSC_KERNEL_UNPAD1D4 : HPC_RLL_PADSC_KERNEL_UNPAD,
                                 std::min(padsc_cdiv(v4 ? padded_total / 4 : total, 256), kPadGridCap), 1, 1, 256, 0, v4 ? 4 : 1, 0);
    p.v4 = v4;
    return p;
}

inline PadscLaunch padsc_handed_over(int RB) { return padsc_launch(HPC_RLL_PADSC_KERNEL_HANDED_OVER, 0, 0, 0, 0, 0, RB, 1); }

// Packed pad (n, max_len > 0).  new_x and mask 16-byte aligned, flat 4-byte aligned, and
//   32 <= max_len <= 16384 with key 28 = 1   the wave kernel (its tiles are 1024 elements whatever the row width: no RB);
//   otherwise, RB >= 1 (max_len <= 15200)     the workgroup kernel, RB rows through LDS;
//   otherwise -- a misaligned pointer, or max_len > 15200 with key 28 = 0 or beyond 16384 -- the call is handed over to the
//   list pad at the shape (1, 1, max_len), which computes the same values: `list` is its launch, noted with handed = 1.
// The record's first by-op int is RB on every path.
inline PadscPacked plan_pad_packed(long n, int max_len, uintptr_t flat, uintptr_t new_x, uintptr_t mask, const PadscKeys& keys) {
    PadscPacked p = {};
    const int RB = packed_rows_per_wg(max_len);
    const bool al = padsc_al16(new_x) && padsc_al16(mask) && (flat & 3) == 0;
    if (al && max_len >= 32 && max_len <= 16384 && keys.pad_wave) {
        // one 1024-element tile per wave, four waves per workgroup
        // (fewer, persistent workgroups -- the shape that makes a pure fill fast, profiles/r04_writebw.txt -- are SLOWER here:
        // 1 / 2 / 4 / 8 workgroups per CU 612 / 466 / 324 / 315 us against 270 for the API call: a tile is a chain of table
        // lookups, source loads, LDS and stores that needs many tiles in flight per CU; the 8192-workgroup cap of the first
        // version, four tiles per wave, was 2.5 % slower)
        const long ntiles = (long)(((unsigned long)n * (unsigned long)max_len + 1023) / 1024);
        p.own = padsc_launch(HPC_RLL_PADSC_KERNEL_PAD1D_PACKED_WAVE, std::min((ntiles + 3) / 4, kPackedGridCap), 1, 1, 256, 0, RB, 0);
    } else if (al && RB >= 1) {
        p.own = padsc_launch(HPC_RLL_PADSC_KERNEL_PAD1D_PACKED, std::min(padsc_cdiv(n, RB), kPackedGridCap), 1, 1, 256,
                             packed_lds_bytes(RB, (unsigned)max_len), RB, 0);
    } else {
        p.own = padsc_handed_over(RB);
        p.list = plan_pad(n, 1, 1, max_len, new_x, mask);
        p.list.b = 1;
    }
    p.own.RB = RB;
    return p;
}

// Packed unpad (n, total, max_len > 0).  `padded` 16-byte aligned, flat 4-byte aligned and RB >= 1 (max_len <= 15200: at least
// one row fits the LDS tile): the workgroup kernel.  Otherwise the call is handed over to the list unpad at (1, 1, max_len);
// there is no wave kernel in this direction.
inline PadscPacked plan_unpad_packed(long n, long total, int max_len, uintptr_t padded, uintptr_t flat) {
    PadscPacked p = {};
    const int RB = packed_rows_per_wg(max_len);
    if (RB >= 1 && padsc_al16(padded) && (flat & 3) == 0) {
        p.own = padsc_launch(HPC_RLL_PADSC_KERNEL_UNPAD1D_PACKED, std::min(padsc_cdiv(n, RB), kPackedGridCap), 1, 1, 256,
                             packed_lds_bytes(RB, (unsigned)max_len), RB, 0);
    } else {
        p.own = padsc_handed_over(RB);
        p.list = plan_unpad(n, total, 1, 1, max_len, padded);
        p.list.b = 1;
    }
    p.own.RB = RB;
    return p;
}

// ------------------------------------------------------------------------------------------------ scatter forward
// LDS of scatter_out_lds_kernel: the x tile (`rows` rows of npb + 1 floats, rounded to 16 bytes), the owner table (HW ints),
// for add the chain links (M ints), for add with in-kernel tables the cell list (M rounded to 4), 16 bytes and the collision
// list (2 * kScatterCollRows + 2 ints).
inline uint64_t scatter_fwd_table_bytes(long HW, int M, bool add, bool build) {
    return (uint64_t)HW * 4 + (add ? (uint64_t)M * 4 : 0) +
           (add && build ? (uint64_t)((M + 3) & ~3) * 4 + 16 + ((uint64_t)2 * kScatterCollRows + 2) * 4 : 0);
}
inline uint64_t scatter_fwd_lds_bytes(uint64_t rows, int npb, long HW, int M, bool add, bool build) {
    return ((rows * (npb + 1) + 3) & ~(uint64_t)3) * 4 + scatter_fwd_table_bytes(HW, M, add, build);
}
// The fit test counts the tile unrounded and 16 bytes of slack: a bound on scatter_fwd_lds_bytes (the rounding adds 12 at the most).
// It is not that function, because the tables are no multiple of 16 bytes for add and the two would then part at the cap.
inline bool scatter_fwd_fits(uint64_t rows, int npb, long HW, int M, bool add, bool build, uint64_t cap) {
    return npb >= 1 && npb <= 64 && rows * (npb + 1) * 4 + 16 + scatter_fwd_table_bytes(HW, M, add, build) <= cap;
}

// flags of the forward's record: 1 = add, 2 = tables built in the kernel, parts << 2 (0 when built in the kernel), 16 = vec
inline int scatter_fwd_flags(const PadscLaunch& p) { return p.add | (p.build ? 2 : 0) | (p.index_parts << 2) | (p.vec ? 16 : 0); }

// Scatter forward (B * N * H * W > 0, B <= 65535, H * W < 2^31).
//
// LDS-staged streaming kernel (key 17): the owner table (HW ints) and an M x NPB tile of x must fit in LDS with room for
// several workgroups per CU (so that one workgroup's staging overlaps the others' stores).  In-process A/B
// (tests/tools/r02_scatter_probe.py, profiles/r02_scatter_probe.json): configs[4] cover 0.953 -> 0.919 ms (4.81 ->
// 4.99 TB/s), reference test shape (16x16 maps) cover 51 -> 46 us, add 68 -> 53 us; `add` on large maps is a tie at
// 64 channels per workgroup (0.893 ms, 5.13 TB/s) and a loss at 32, so it keeps the cells-per-thread kernel there.
// In-kernel index build (round 4, key 37): cover for every M (an LDS atomic per entity); add where the LDS kernel is taken
// anyway (maps up to 8 KB) and the quadratic chain search is small against the workgroup's output
// (add: measured -13 % at 32 x 32 maps with 128 entities, +15 % at the reference's 16 x 16 test shape with 256, where four
// workgroups per batch element each repeat a build that outweighs their 64 KB of output).
// (`add` on large maps, rounds 4-5 before the prefetch: the LDS kernel + build at 32 / 64 channels per workgroup lost to the
// cells-per-thread kernel behind the index launch, 0.837 / 0.89 against 0.828 ms -- DESIGN.md 4.5.  Round 5, with the staging
// prefetch: at C5 the LDS kernel + build at 32 channels per workgroup runs `add` in 0.811 ms against 0.823 for the
// cells-per-thread kernel behind its index launch -- and has no second launch: taken wherever the tables are built in the kernel.)
//
// Otherwise the cells-per-thread kernels behind the index launch: scatter_out4_kernel where H * W and N are multiples of 4 and
// x and out are 16-byte aligned, else scatter_out_kernel.
inline PadscLaunch plan_scatter_fwd(int B, int M, int N, int H, int W, int add, uintptr_t x, uintptr_t out, const PadscKeys& keys,
                                    int cus) {
    const long HW = (long)H * W;
    const int index_parts = add ? (M > 256 ? 3 : 1) : 2;
    const bool build = keys.scatter_build && W > 0 && (!add || (M <= 256 && HW >= 1024));
    const bool lds_pays = !add || HW * 4 <= 8 * 1024 || keys.scatter_npb != 0 || build;
    if (keys.scatter_lds_fwd && lds_pays && M > 0 && (HW % 4) == 0 && HW * 4 <= 32 * 1024 && padsc_al16(out)) {
        const uint64_t rows = (uint64_t)M + (add && build ? kScatterCollRows : 0);   // x tile rows (+ the rows of the cells with several entities)
        const uint64_t cap = (uint64_t)(keys.scatter_npb ? 100 : add && build ? 60 : 52) * 1024;   // two workgroups per CU
        int npb = 0;
        if (keys.scatter_npb) {
            if (scatter_fwd_fits(rows, keys.scatter_npb, HW, M, add, build, cap)) npb = keys.scatter_npb;
        } else {
            for (int c = 64; c >= 4 && !npb; c /= 2)
                if (scatter_fwd_fits(rows, c, HW, M, add, build, cap)) npb = c;
        }
        if (npb > N) npb = (N + 3) / 4 * 4;
        if (scatter_fwd_fits(rows, npb, HW, M, add, build, cap)) {
            PadscLaunch p = padsc_launch(HPC_RLL_PADSC_KERNEL_SCATTER_OUT_LDS, (N + npb - 1) / npb, B, 1, 1024,
                                         scatter_fwd_lds_bytes(rows, npb, HW, M, add, build), npb, 0);
            p.npb = npb;
            p.add = add ? 1 : 0;
            p.build = build;
            p.index_parts = build ? 0 : index_parts;
            // vec: every workgroup stages its x tile with 16-byte loads (stage_x: nn, N and n0 multiples of 4, x aligned)
            p.vec = (N % 4) == 0 && (npb % 4) == 0 && padsc_al16(x);
            // staging prefetch distance (see the kernel): half of the workgroups the chip holds -- two 1024-thread workgroups per
            // CU, fewer when LDS limits -- rounded to a multiple of 8
            p.pf_wgs = (cus * (p.lds * 2 <= 160 * 1024 ? 2 : 1) / 2) & ~7;
            p.b = scatter_fwd_flags(p);
            return p;
        }
    }
    const bool v4 = (HW % 4) == 0 && (N % 4) == 0 && padsc_al16(x) && padsc_al16(out);
    const int tpb = (v4 && HW >= 4096) ? kScatterThreads : 256;
    const int cell_blocks = (int)((HW + (v4 ? 4 * tpb - 1 : 255)) / (v4 ? 4 * tpb : 256));
    // enough workgroups to cover the chip: split the channel axis when B * cell_blocks is small
    int n_per_block = N;
    while (n_per_block > 4 && (long)B * cell_blocks * ((N + n_per_block - 1) / n_per_block) < 2048) n_per_block = (n_per_block / 2 + 3) / 4 * 4;
    PadscLaunch p = padsc_launch(v4 ? HPC_RLL_PADSC_KERNEL_SCATTER_OUT4 : HPC_RLL_PADSC_KERNEL_SCATTER_OUT, cell_blocks,
                                 (N + n_per_block - 1) / n_per_block, B, tpb, 0, n_per_block, 0);
    p.npb = n_per_block;
    p.add = add ? 1 : 0;
    p.index_parts = index_parts;
    p.vec = v4 || ((N % 4) == 0 && padsc_al16(x));
    p.b = scatter_fwd_flags(p);
    return p;
}

// ------------------------------------------------------------------------------------------------ scatter backward
// Scatter backward (B * M * N > 0).  H * W = 0: every gradient row is zero, a memset and no kernel.
//
// Which kernel (round 6, profiles/r06_scatter_bwd_probe.txt).  The plane kernel writes NG*4-byte pieces of every entity's row
// from N/NG workgroups; where those pieces are 16 bytes or less (maps of 4096 cells and more) AND the entity rows are a
// sizeable part of the traffic (M*16 >= H*W: C5 exactly), the spatial-tile kernel -- full rows from one writer -- is faster
// (M = 1024, N = 128: 1086 -> 946 us; C5: 741 -> 724 us mean of 50 buffer sets on five boxes) and half as sensitive to where
// grad_out and grad_x lie relative to each other (C5: +5 % instead of +12 % on an unlucky pair).  Few entities per map
// (B = 8192, M = 64: 656 vs 710 us) and small maps (32 x 32: 249 vs 288) keep the plane kernel.  Key 40 forces either.
// The tile kernel needs W % 4 == 0, M <= 4096, B <= 65535, grad_out 16-byte aligned and one map row of all planes in 64 KB;
// its plane pieces must be 1 KB and more where entity rows are a sixteenth of the planes (C5), 512 bytes only where they are a
// quarter (N = 128, M = 1024: 1070 -> 945 us; N = 128, M = 256 keeps the plane kernel: 714 vs 747).
// The plane kernel takes planes up to 128 KB and B <= 65535; everything else gathers from memory (the direct kernel).
inline PadscLaunch plan_scatter_bwd(int B, int M, int N, int H, int W, uintptr_t grad_out, const PadscKeys& keys) {
    const long HW = (long)H * W;
    if (HW == 0) return padsc_launch(HPC_RLL_PADSC_KERNEL_SCATTER_BWD_MEMSET, 0, 0, 0, 0, 0, 0, 0);
    const long plane_bytes = HW * 4;
    const long planes = std::min<long>(N, std::max<long>(1, kScatterBwdLdsBytes / plane_bytes));   // that 64 KB hold
    const bool tile_rule = keys.scatter_bwd_tile == 2 || (keys.scatter_bwd_tile == 0 && planes * 4 <= 16 && (long)M * 16 >= HW);
    if (tile_rule && (W % 4) == 0 && M <= 4096 && B <= 65535 && (long)N * W * 4 <= 64 * 1024 && padsc_al16(grad_out)) {
        int TR = (int)std::min<long>(64L * 1024 / ((long)N * W * 4), H);
        while (TR & (TR - 1)) TR &= TR - 1;              // a power of two (the swizzle XORs inside a plane piece)
        const int cells = TR * W;
        const bool pays = ((long)cells * 4 >= 1024 && (long)M * 16 >= HW) || ((long)cells * 4 >= 512 && (long)M * 4 >= HW);
        if (pays || keys.scatter_bwd_tile == 2) {
            PadscLaunch p = padsc_launch(HPC_RLL_PADSC_KERNEL_SCATTER_BWD_TILE, (H + TR - 1) / TR, B, 1, 1024,
                                         (uint64_t)N * cells * 4 + 16 + (uint64_t)M * 8, TR, 0);
            p.TR = TR;
            if ((cells & (cells - 1)) == 0 && cells >= 8) p.swz = std::min(cells / 4 - 1, 63);
            return p;
        }
    }
    if (plane_bytes <= 128 * 1024 && B <= 65535) {
        const int NG = (int)std::min<long>(planes, 32);
        PadscLaunch p = padsc_launch(HPC_RLL_PADSC_KERNEL_SCATTER_BWD_LDS, (N + NG - 1) / NG, B, 1, 1024, (uint64_t)NG * plane_bytes, NG, 0);
        p.NG = NG;
        // measured (profiles/r04_scatter_bwd_xcd.txt): 16-byte pieces (64 x 64 maps, NG = 4) -8 % at C5 and -31 % at M = 1024, N = 128;
        // 64-byte pieces (32 x 32 maps) +6 %, whole lines (16 x 16) +4 % -- only pieces below a 64-byte sector pair profit
        const bool xcd = (keys.scatter_bwd_xcd == 2 || (keys.scatter_bwd_xcd == 1 && NG * 4 <= 32)) && ((long)p.gx * p.gy) % 8 == 0 && p.gx > 1;
        // (round 6) with B a multiple of 8 the XCDs take NEIGHBOURING batch elements (order 2: -1 % on every shape measured)
        p.xcd = p.b = xcd ? (B % 8 == 0 ? 2 : 1) : 0;
        return p;
    }
    return padsc_launch(HPC_RLL_PADSC_KERNEL_SCATTER_BWD_DIRECT, std::min(padsc_cdiv((long)B * M * N, 256), kScatterBwdDirectCap), 1, 1, 256, 0, 0, 0);
}

}  // namespace hpc_rll
