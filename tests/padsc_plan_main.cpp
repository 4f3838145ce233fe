// TEST-ONLY: the planners of csrc/padsc_plan.hpp as a stand-alone host program (no HIP, no library), for
// tests/test_pad_scatter_cpu.py.  Reads one call per line from stdin --
//   pad    n m0 m1 m2 new_x mask
//   unpad  n total m0 m1 m2 padded
//   ppad   n max_len flat new_x mask key28
//   punpad n total max_len padded flat
//   fwd    B M N H W add x out key17 key18 key37 cus
//   bwd    B M N H W grad_out key38 key40
// (pointers as integers) -- and prints per line the seven ints the dispatch record must hold after the launch count, for a
// hand-over " H" and the seven of the list op's record, for a plan with dynamic LDS " E" and the number of bytes the
// kernel's carve of that LDS ends at, and for the forward's LDS kernel " P" and the plan's prefetch distance pf_wgs.
// Of the four carves two are layouts of their own, stated apart from the request (ScatterFwdCarve, ScatterBwdTileCarve); the
// packed kernels' tile and the plane kernel's NG planes ARE the request (packed_tile_floats is shared by kernel and host), so
// their " E" can only show that the shared function is the one the plan used.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "padsc_plan.hpp"

using namespace hpc_rll;

static void print_record(const PadscLaunch& p) {
    std::printf("%d %u %u %d %" PRIu64 " %d %d", p.kernel, p.gx, p.gy * p.gz, p.threads, p.lds, p.a, p.b);
}

static void print_packed(const PadscPacked& p, int max_len) {
    print_record(p.own);
    if (p.own.kernel == HPC_RLL_PADSC_KERNEL_HANDED_OVER) {
        std::printf(" H ");
        print_record(p.list);
    }
    if (p.own.lds) std::printf(" E %" PRIu64, packed_tile_floats(p.own.RB, (unsigned)max_len) * 4 + (uint64_t)(p.own.RB + 1) * 8);
}

int main() {
    char op[16];
    long long v[12];
    int lines = 0;
    while (std::scanf("%15s", op) == 1) {
        const int want = !std::strcmp(op, "pad") || !std::strcmp(op, "unpad") || !std::strcmp(op, "ppad") ? 6
                         : !std::strcmp(op, "punpad")                                                      ? 5
                         : !std::strcmp(op, "fwd")                                                         ? 12
                         : !std::strcmp(op, "bwd")                                                         ? 8
                                                                                                           : -1;
        if (want < 0) { std::fprintf(stderr, "line %d: unknown op %s\n", lines + 1, op); return 2; }
        for (int i = 0; i < want; ++i)
            if (std::scanf("%lld", &v[i]) != 1) { std::fprintf(stderr, "line %d: %s needs %d numbers\n", lines + 1, op, want); return 2; }
        PadscKeys keys = {1, 1, 0, 1, 1, 0};
        if (!std::strcmp(op, "pad")) {
            print_record(plan_pad(v[0], (int)v[1], (int)v[2], (int)v[3], (uintptr_t)v[4], (uintptr_t)v[5]));
        } else if (!std::strcmp(op, "unpad")) {
            print_record(plan_unpad(v[0], v[1], (int)v[2], (int)v[3], (int)v[4], (uintptr_t)v[5]));
        } else if (!std::strcmp(op, "ppad")) {
            keys.pad_wave = (int)v[5];
            print_packed(plan_pad_packed(v[0], (int)v[1], (uintptr_t)v[2], (uintptr_t)v[3], (uintptr_t)v[4], keys), (int)v[1]);
        } else if (!std::strcmp(op, "punpad")) {
            print_packed(plan_unpad_packed(v[0], v[1], (int)v[2], (uintptr_t)v[3], (uintptr_t)v[4]), (int)v[2]);
        } else if (!std::strcmp(op, "fwd")) {
            keys.scatter_lds_fwd = (int)v[8], keys.scatter_npb = (int)v[9], keys.scatter_build = (int)v[10];
            const int M = (int)v[1], H = (int)v[3], W = (int)v[4];
            const PadscLaunch p = plan_scatter_fwd((int)v[0], M, (int)v[2], H, W, (int)v[5], (uintptr_t)v[6], (uintptr_t)v[7], keys, (int)v[11]);
            print_record(p);
            if (p.lds) std::printf(" E %" PRIu64 " P %d", (uint64_t)ScatterFwdCarve(M, H * W, p.npb, p.add, p.build).end * 4, p.pf_wgs);
        } else {
            keys.scatter_bwd_xcd = (int)v[6], keys.scatter_bwd_tile = (int)v[7];
            const int M = (int)v[1], N = (int)v[2], H = (int)v[3], W = (int)v[4];
            const PadscLaunch p = plan_scatter_bwd((int)v[0], M, N, H, W, (uintptr_t)v[5], keys);
            print_record(p);
            if (p.kernel == HPC_RLL_PADSC_KERNEL_SCATTER_BWD_TILE) std::printf(" E %" PRIu64, ScatterBwdTileCarve(M, N, p.TR * W).end * 4);
            else if (p.lds) std::printf(" E %" PRIu64, (uint64_t)p.NG * H * W * 4);   // s_plane[NG][H * W]
        }
        std::printf("\n");
        ++lines;
    }
    return 0;
}
