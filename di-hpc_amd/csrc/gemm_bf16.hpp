// gemm_bf16.hpp -- the bf16 product tile of the fused LM head (lm_linear.hip) and the ONE matrix form its gradients need.
//
//   C (M x N) (+)= A (M x K) * B (K x N)      A bf16 row-major, contiguous along K;  B bf16 row-major, contiguous along N
// with fp32 accumulation in v_mfma_f32_32x32x16_bf16.  Both gradients of the head have this shape:
//   dhidden[r,h] = sum_v G[r,v] W[v,h]         A = G (the chunk's logit gradients), B = the chunk's rows of lm_weight as they lie
//   dW[v,h]      = sum_r G^T[v,r] hidden[r,h]  A = G^T,                             B = hidden as it lies
//
// Tiling, that of lm_linear_kernel: a workgroup of four waves owns 128 x 128 of C and walks K in steps of 64 through two LDS
// buffers (register staging: the global loads of step k+1 are issued before the matrix instructions of step k and stored after
// them; one barrier per step).  Both LDS tiles are [128 rows][64 k] at a pitch of 144 bytes.  The A tile is staged like the
// forward's operands (16-byte chunks, nothing moves).  The B tile is the new part: its contraction index is strided in memory
// while the instruction wants 8 consecutive k per lane, so it is staged TRANSPOSED.  A thread loads four 16-byte pieces, rows
// k .. k+3 of the same 8 columns (16 consecutive threads cover 256 contiguous bytes of a row), transposes the 4 x 8 block in
// registers (16 and/or/shift operations) and writes eight 8-byte pieces, one per column: [n][k .. k+3].  (An 8 x 8 block per
// thread, the full form of the transpose, would leave half of the 256 threads without a block at this tile size.)
// The product is formed with C's n on the instruction's M side and C's m on its N side, so a lane holds one row m = lane % 32
// and, per accumulator, four runs of 4 consecutive n: an fp32 result leaves the registers as 16-byte stores, a bf16 result is
// staged through the (now free) LDS so that it leaves as 16-byte row pieces as well.
// Edges: rows of A past M are loaded clamped (their results are not stored), k >= K is zeros on both sides, rows of B at
// k >= K_valid and rows that the optional liveness (action, weight) drops are ZEROS WITHOUT BEING READ, columns past N are zeros.
// No split-K, no atomics: one fp32 chain per output in k order, the same bits on every run.
#pragma once
#include <hip/hip_runtime.h>

#include "lm_head.hpp"

namespace hpc_rll {

constexpr int kBM = 128, kBN = 128, kBK = 64;   // rows, columns and contraction elements of a workgroup's step
constexpr int kPitch = kBK + 8;                 // LDS row pitch in bf16: 144 bytes
constexpr int kTileElems = 128 * kPitch;        // one operand tile of one buffer (kBM == kBN == 128 rows)
constexpr int kLdsBytes = 2 * 2 * kTileElems * 2;
constexpr int kChunks = 128 * (kBK / 8) / 256;  // 16-byte chunks of one operand tile per thread: 4
constexpr int kSlabElems = 2 * kTileElems / 4;  // a wave's private quarter of one LDS buffer: 9216 bytes
constexpr int kSlabPitch = kBN + 8;             // 272 bytes: 32 rows fit the slab, 16-byte pieces stay aligned
static_assert(kBM == 128 && kBN == 128 && kBK == 64 && kChunks == 4, "the thread mappings are written for these");
static_assert(32 * kSlabPitch <= kSlabElems && (kSlabPitch * 2) % 16 == 0, "a wave's 32 x 128 bf16 tile fits its slab");

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef unsigned int vuint2 __attribute__((ext_vector_type(2)));
typedef float vfloat4 __attribute__((ext_vector_type(4)));

// The layout of a wave's accumulators in every kernel built on this tile: acc[j][i] belongs to the wave's row lane % 32 and
// to column 32 j + 8 (i / 4) + 4 (lane / 32) + i % 4 of the 128.
// A wave's 32 x 128 values, rounded to bf16 once, as row-major 16-byte pieces: through the wave's slab, then row `r` of the
// 32 to dst + r ld (elements), the 16 pieces of a row by 16 consecutive lanes.  `rows` and `cols` (a multiple of 8) bound
// what is stored.  The caller's barriers keep the slab free before and after.
__device__ __forceinline__ void store_wave_tile_bf16(uint16_t* slab, const floatx16 (&acc)[4], uint16_t* dst, size_t ld, long rows,
                                                     int cols, int lane) {
    const int r = lane & 31, half = lane >> 5;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const vuint2 v = {bf16_bits(acc[j][4 * g]) | (bf16_bits(acc[j][4 * g + 1]) << 16),
                              bf16_bits(acc[j][4 * g + 2]) | (bf16_bits(acc[j][4 * g + 3]) << 16)};
            *reinterpret_cast<vuint2*>(&slab[r * kSlabPitch + 32 * j + 8 * g + 4 * half]) = v;
        }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int c = lane + 64 * q, row = c >> 4, col = (c & 15) * 8;
        if (row < rows && col < cols)
            *reinterpret_cast<vuint4*>(dst + (size_t)row * ld + col) = *reinterpret_cast<const vuint4*>(&slab[row * kSlabPitch + col]);
    }
}

// One K step of the tile on a wave: the fragment of its 32 rows once, the four 32-column fragments against it.
__device__ __forceinline__ void tile_step(const uint16_t* cols_tile, const uint16_t* rows_tile, int wave_row, int lane,
                                          floatx16 (&acc)[4]) {
    const uint16_t* la = cols_tile + (lane & 31) * kPitch + (lane >> 5) * 8;
    const uint16_t* lb = rows_tile + wave_row * kPitch + (lane >> 5) * 8;
#pragma unroll
    for (int q = 0; q < kBK / 16; ++q) {
        const bf16x8 b = *reinterpret_cast<const bf16x8*>(lb + q * 16);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bf16x8 a = *reinterpret_cast<const bf16x8*>(la + j * 32 * kPitch + q * 16);
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc[j], 0, 0, 0);
        }
    }
}

enum GemmBf16Mode { kStoreBf16 = 0, kStoreF32 = 1, kAddF32 = 2, kAddF32StoreBf16 = 3 };

struct GemmBf16Args {
    const uint16_t* A; const uint16_t* B; uint16_t* Cb; float* Cf;
    const int64_t* act; const float* wt;   // the liveness of B's rows: action in [0, actV) and weight != 0; act NULL = all live
    long M, K, Kv;                         // Kv <= K: rows of B from Kv on are zeros
    size_t lda, ldb, ldc;
    int N, actV;
};

template <int MODE> __global__ __launch_bounds__(256) void gemm_bf16_kernel(const GemmBf16Args p) {
    __shared__ __attribute__((aligned(16))) uint16_t lds[2][2][kTileElems];   // [buffer][0: B transposed (n rows), 1: A (m rows)]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long m0 = (long)blockIdx.x * kBM;
    const int n0 = (int)blockIdx.y * kBN;
    const long nk = (p.K + kBK - 1) / kBK;

    // ---- A: rows (tid >> 3) + 32 i, 8 bf16 at column (tid & 7) 8 of the K step
    const int lr = tid >> 3, kc = (tid & 7) * 8;
    const uint16_t* ap[kChunks];
#pragma unroll
    for (int i = 0; i < kChunks; ++i) {
        long m = m0 + lr + 32 * i;
        m = m < p.M ? m : p.M - 1;                                 // clamped: never past the last row
        ap[i] = p.A + (size_t)m * p.lda + kc;
    }
    // ---- B: rows 4 (tid >> 4) + i of the K step, the 8 columns from (tid & 15) 8
    const int nb = (tid & 15) * 8, kb = (tid >> 4) * 4;
    const bool nok = n0 + nb < p.N;                                // N is a multiple of 8: a piece is inside or outside as a whole
    vuint4 ra[kChunks], rb[kChunks];
    auto gload = [&](long ks) {
        const long k = ks * kBK;
        const vuint4 z = {0u, 0u, 0u, 0u};
        const bool aok = k + kc < p.K;                             // K is a multiple of 8
#pragma unroll
        for (int i = 0; i < kChunks; ++i) {
            ra[i] = z;
            if (aok) ra[i] = *reinterpret_cast<const vuint4*>(ap[i] + k);
            const long kk = k + kb + i;
            bool ok = nok && kk < p.Kv;
            if (ok && p.act) {
                const long a = p.act[kk];
                const float w = p.wt ? p.wt[kk] : 1.f;
                ok = a >= 0 && a < (long)p.actV && w != 0.f;
            }
            rb[i] = z;
            if (ok) rb[i] = *reinterpret_cast<const vuint4*>(p.B + (size_t)kk * p.ldb + n0 + nb);
        }
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int i = 0; i < kChunks; ++i) *reinterpret_cast<vuint4*>(&lds[buf][1][(lr + 32 * i) * kPitch + kc]) = ra[i];
#pragma unroll
        for (int d = 0; d < 4; ++d) {                              // dword d of a piece holds columns 2 d and 2 d + 1
            const vuint2 even = {(rb[0][d] & 0xffffu) | (rb[1][d] << 16), (rb[2][d] & 0xffffu) | (rb[3][d] << 16)};
            const vuint2 odd = {(rb[0][d] >> 16) | (rb[1][d] & 0xffff0000u), (rb[2][d] >> 16) | (rb[3][d] & 0xffff0000u)};
            *reinterpret_cast<vuint2*>(&lds[buf][0][(nb + 2 * d) * kPitch + kb]) = even;
            *reinterpret_cast<vuint2*>(&lds[buf][0][(nb + 2 * d + 1) * kPitch + kb]) = odd;
        }
    };

    floatx16 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[j][i] = 0.f;
    if (nk > 0) {
        gload(0);
        lstore(0);
    }
    __syncthreads();
    int cur = 0;
    for (long ks = 0; ks < nk; ++ks) {
        const bool more = ks + 1 < nk;
        if (more) gload(ks + 1);
        tile_step(&lds[cur][0][0], &lds[cur][1][0], wv * 32 + (lane & 31), lane, acc);
        if (more) lstore(cur ^ 1);
        __syncthreads();
        cur ^= 1;
    }

    // ---- C: row m of this lane, columns n0 + 32 j + 8 g + 4 half + (0 .. 3)
    const int half = lane >> 5;
    const long m = m0 + wv * 32 + (lane & 31);
    if constexpr (MODE != kStoreBf16) {
        if (m < p.M) {
            float* crow = p.Cf + (size_t)m * p.ldc;
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int n = n0 + 32 * j + 8 * g + 4 * half;
                    if (n < p.N) {
                        vfloat4* c = reinterpret_cast<vfloat4*>(crow + n);
                        vfloat4 v = {acc[j][4 * g], acc[j][4 * g + 1], acc[j][4 * g + 2], acc[j][4 * g + 3]};
                        if constexpr (MODE != kStoreF32) v += *c;
                        if constexpr (MODE == kAddF32StoreBf16) {
#pragma unroll
                            for (int e = 0; e < 4; ++e) acc[j][4 * g + e] = v[e];
                        } else {
                            *c = v;
                        }
                    }
                }
        }
    }
    if constexpr (MODE == kStoreBf16 || MODE == kAddF32StoreBf16) {   // the loop's last barrier has freed the LDS
        const long mw = m0 + wv * 32;
        store_wave_tile_bf16(&lds[0][0][0] + wv * kSlabElems, acc, p.Cb + (size_t)mw * p.ldc + n0, p.ldc, p.M - mw, p.N - n0, lane);
    }
}

inline int launch_gemm_bf16(const GemmBf16Args& p, int mode, hipStream_t st) {
    const dim3 grid((unsigned)((p.M + kBM - 1) / kBM), (unsigned)((p.N + kBN - 1) / kBN));
    switch (mode) {
        case kStoreBf16: hipLaunchKernelGGL(gemm_bf16_kernel<kStoreBf16>, grid, dim3(256), 0, st, p); break;
        case kStoreF32: hipLaunchKernelGGL(gemm_bf16_kernel<kStoreF32>, grid, dim3(256), 0, st, p); break;
        case kAddF32: hipLaunchKernelGGL(gemm_bf16_kernel<kAddF32>, grid, dim3(256), 0, st, p); break;
        default: hipLaunchKernelGGL(gemm_bf16_kernel<kAddF32StoreBf16>, grid, dim3(256), 0, st, p); break;
    }
    return last_error();
}

}  // namespace hpc_rll
