// lm_linear.hip -- the language-model head fused with its bf16 matrix product on gfx950: the log-probability (and the entropy)
// of given tokens straight from the hidden states and the head's weight.  No logit is ever written to memory.
//
// hidden (rows, H) bf16, w (V, H) bf16 (nn.Linear.weight's own layout), action (rows) int64, weight (rows) fp32 or NULL.
// With x = (hidden w^T) inv_temperature held in fp32:  logp = x[a] - logsumexp(x),  entropy = logsumexp(x) - sum p x.
//
// The forward, two launches:
//   * lm_linear_kernel<ENT>: grid (row tiles, vocabulary splits), row tile fastest, so that the workgroups that run together
//     read the same weight tiles and share them in L2.  A workgroup of four waves owns kBM = 128 tokens and walks the column
//     tiles (kBN = 128 vocabulary entries) of its split; inside a tile it walks H in steps of kBK = 64 through double-buffered
//     LDS (register staging: the 16-byte global loads of step k+1 are issued before the matrix instructions of step k and
//     stored after them; one barrier per step, also across tile boundaries).  Both operands are contiguous along H, which is
//     what v_mfma_f32_32x32x16_bf16 takes: 8 consecutive bf16 per lane.  Nothing is transposed; every global and LDS access is a
//     16-byte vector; the LDS row pitch is 144 bytes, which spreads the 16-byte reads of 16 consecutive rows over all banks.
//     The TRANSPOSED product is formed: weight rows on the instruction's M side, tokens on its N side.  A wave owns 32 tokens
//     and all 128 vocabulary entries of the tile (four accumulators of 16 floats), so lane l holds 64 logits of token
//     l % 32 and the softmax statistic is in-lane arithmetic on the accumulators: RowStat's online (m, s, u) of lm_head.hpp,
//     one rescale per tile.  A token lives in the two lanes l and l + 32 of ONE wave; they meet in one shuffle at the end of
//     the split -- no LDS, no barrier (the wave-per-32-tokens split costs five LDS fragment reads per four matrix instructions
//     instead of four, and saves the cross-wave merge).  One partial (m, s, u, x[a]) per (row, split) goes to the workspace.
//     Weight rows past V and token rows past `rows` are loaded clamped to the last valid row, K chunks past H are zeros;
//     columns past V are selected to -FLT_MAX in the epilogue.  A workgroup whose 128 rows are all dropped exits after reading
//     action and weight.
//   * lm_linear_combine_kernel: a thread per row merges the row's partials in split order and writes logp and entropy (zeros
//     for dropped rows); a workgroup of 128 rows is a row tile, and the tiles without a live row are counted (an integer
//     add) for the launch record.
// No floating-point atomics: the same bits on every run for the same split count.
//
// The gradient (hpc_rll_lm_linear_backward) walks the vocabulary in chunks, which lse -- one more output of the combine launch
// -- makes independent.  Per chunk:
//   * lm_linear_grad_logits_kernel<WG, WT> recomputes the chunk's logits with the forward's product loop (product_walk, shared,
//     not copied), forms g = inv_t (gl (1[v = a] - p) - ge p (log p + H)) on the accumulators, rounds once to bf16 and writes
//     G (Rp x VC, through the free LDS buffer as 16-byte row pieces) and G^T (VC x Rp, straight from the registers: the 32 lanes
//     of a half-wave hold 32 consecutive tokens of one entry), zeros explicitly wherever nothing is live;
//   * gemm_bf16_kernel (gemm_bf16.hpp), one matrix form for both products: dhidden (+)= G W[chunk] in fp32 across chunks,
//     dW[chunk] = G^T hidden with the dropped rows of hidden loaded as zeros.
// No atomics there either: the same bits on every run for the same chunk size.
#include <hip/hip_runtime.h>

#include "gemm_bf16.hpp"
#include "hostutil.hpp"
#include "hpc_rll_hip.h"
#include "lm_head.hpp"

namespace hpc_rll {
namespace {

constexpr int kMaxSplits = 64, kMinH = 32, kMaxH = 16384;

constexpr int kConfigInts = 10;   // the host part of the record; the skipped row tiles are read from the device
LaunchRecord<kConfigInts> g_rec;
int* g_skipped_dev[64] = {};      // one device word per device, allocated at the first launch there and kept
int* g_skipped_last = nullptr;
hipStream_t g_stream_last = nullptr;

// ---- what the forward and the gradient's recompute share ---------------------------------------------------------------------
// Which of the workgroup's 128 rows are live (s_act: the action, -1 for a dropped row or one past `rows`); 0 when none is.
__device__ __forceinline__ int live_rows(int (&s_act)[kBM], const int64_t* action, const float* weight, long row0, long rows, int V) {
    int live = 0;
    if (threadIdx.x < kBM) {
        const long r = row0 + threadIdx.x;
        long a = -1;
        float w = 1.f;
        if (r < rows) {
            a = action[r];
            if (weight) w = weight[r];
        }
        live = a >= 0 && a < (long)V && w != 0.f;
        s_act[threadIdx.x] = live ? (int)a : -1;
    }
    return __syncthreads_or(live);
}

// The product loop: the logits of the workgroup's 128 tokens (from row0) against the column tiles [t0, t1) of the vocabulary,
// flattened over (column tile, K step) so that the prefetch also crosses tile boundaries.  Register staging, two LDS buffers,
// one barrier per step; the transposed product, a wave owning 32 tokens x 128 entries (gemm_bf16.hpp: tile_step).  When a
// tile's logits are complete, epi(vt, free) sees them in acc (the layout documented there, row = token, column = entry of the
// tile); `free` is the LDS buffer no wave reads before the next barrier.  epi runs in all 256 threads and leaves acc zeroed.
template <class Epi>
__device__ __forceinline__ void product_walk(uint16_t (&lds)[2][2][kTileElems], const uint16_t* hidden, const uint16_t* w, long rows,
                                             int H, int V, long row0, int t0, int t1, floatx16 (&acc)[4], Epi&& epi) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int nk = (H + kBK - 1) / kBK;
    const long steps = (long)(t1 - t0) * nk;

    // ---- the 16-byte chunks this thread moves: rows (tid >> 3) + 32 i, 8 bf16 at column (tid & 7) 8 of the K step
    const int lr = tid >> 3, kc = (tid & 7) * 8;
    const uint16_t* hp[kChunks];
#pragma unroll
    for (int i = 0; i < kChunks; ++i) {
        long r = row0 + lr + 32 * i;
        r = r < rows ? r : rows - 1;                           // clamped: never past the last row
        hp[i] = hidden + (size_t)r * (size_t)H + kc;
    }
    vuint4 ra[kChunks], rb[kChunks];
    auto gload = [&](int vt, int ks) {
        const int k = ks * kBK;
        const bool ok = k + kc < H;                            // H is a multiple of 32: a chunk is inside or outside as a whole
        const vuint4 z = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < kChunks; ++i) {
            long v = (long)vt * kBN + lr + 32 * i;
            v = v < (long)V ? v : (long)V - 1;                 // clamped: the epilogue selects such columns away
            ra[i] = z;
            rb[i] = z;
            if (ok) {
                ra[i] = *reinterpret_cast<const vuint4*>(w + (size_t)v * (size_t)H + k + kc);
                rb[i] = *reinterpret_cast<const vuint4*>(hp[i] + k);
            }
        }
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int i = 0; i < kChunks; ++i) {
            const int o = (lr + 32 * i) * kPitch + kc;
            *reinterpret_cast<vuint4*>(&lds[buf][0][o]) = ra[i];
            *reinterpret_cast<vuint4*>(&lds[buf][1][o]) = rb[i];
        }
    };

#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[j][i] = 0.f;
    if (steps > 0) {
        gload(t0, 0);
        lstore(0);
    }
    __syncthreads();
    int vt = t0, ks = 0, cur = 0;
    for (long it = 0; it < steps; ++it) {
        int nvt = vt, nks = ks + 1;
        if (nks == nk) {
            nks = 0;
            ++nvt;
        }
        const bool more = it + 1 < steps;
        if (more) gload(nvt, nks);
        tile_step(&lds[cur][0][0], &lds[cur][1][0], wv * 32 + (lane & 31), lane, acc);
        if (ks == nk - 1) epi(vt, cur ^ 1);
        if (more) lstore(cur ^ 1);
        __syncthreads();
        cur ^= 1;
        vt = nvt;
        ks = nks;
    }
}

struct LinArgs {
    const uint16_t* hidden; const uint16_t* w; const int64_t* action; const float* weight;
    float4* ws; int* skipped; long rows; int H, V; float inv_t;
};

template <bool ENT>
__global__ __launch_bounds__(256) void lm_linear_kernel(const LinArgs p) {
    __shared__ __attribute__((aligned(16))) uint16_t lds[2][2][kTileElems];   // [buffer][0: weight rows, 1: tokens]
    __shared__ int s_act[kBM];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long row0 = (long)blockIdx.x * kBM;
    const int sp = blockIdx.y, nsp = gridDim.y;
    if (blockIdx.x == 0 && sp == 0 && tid == 0) *p.skipped = 0;   // the combine launch counts into it

    // ---- a tile without a live row is not computed
    if (!live_rows(s_act, p.action, p.weight, row0, p.rows, p.V)) return;

    const int tok = wv * 32 + (lane & 31), half = lane >> 5;
    const long my_row = row0 + tok;
    const int my_act = s_act[tok];

    // ---- the column tiles of this split: [t0, t1) of ceil(V / 128)
    const long nct = ((long)p.V + kBN - 1) / kBN;
    const int t0 = (int)(nct * sp / nsp), t1 = (int)(nct * (sp + 1) / nsp);

    floatx16 acc[4];
    RowStat<ENT> st{-kFltMaxG, 0.f};
    if constexpr (ENT) st.u = 0.f;
    float xa = 0.f;
    product_walk(lds, p.hidden, p.w, p.rows, p.H, p.V, row0, t0, t1, acc, [&](int vt, int) {
        // ---- acc[j][i] is vocabulary entry vt 128 + 32 j + 8 (i / 4) + 4 half + i % 4
        const int vb = vt * kBN + half * 4;
        const int left = p.V - vb, da = my_act - vb;           // entry e (a constant below) exists iff e < left
        float bm = -kFltMaxG;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int e = 32 * j + 8 * (i >> 2) + (i & 3);
                float x = clampf(acc[j][i] * p.inv_t);
                x = e < left ? x : -kFltMaxG;
                xa = da == e ? x : xa;
                acc[j][i] = x;
                bm = fmaxf(bm, x);
            }
        RowStat<ENT> n = stat_shift(st, fmaxf(st.m, bm));
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float t = acc[j][i] - n.m;
                const float ex = ex2(t * kLog2eG);
                n.s += ex;
                if constexpr (ENT) n.u = fmaf(ex, ex == 0.f ? 0.f : t, n.u);
                acc[j][i] = 0.f;
            }
        st = n;
    });

    // ---- the two lanes of a token meet; one partial per (row, split)
    RowStat<ENT> o{__shfl_xor(st.m, 32, 64), __shfl_xor(st.s, 32, 64)};
    if constexpr (ENT) o.u = __shfl_xor(st.u, 32, 64);
    st = stat_merge(st, o);
    xa += __shfl_xor(xa, 32, 64);
    if (half == 0 && my_row < p.rows) {
        float4 out = make_float4(-kFltMaxG, 0.f, 0.f, 0.f);   // a dropped row, or a split without columns: the identity
        if (my_act >= 0 && t1 > t0) {
            out.x = st.m;
            out.y = st.s;
            if constexpr (ENT) out.z = st.u;
            out.w = xa;
        }
        p.ws[(size_t)sp * (size_t)p.rows + (size_t)my_row] = out;
    }
}

// ---- the gradient's recompute: the logit gradients of one vocabulary chunk ---------------------------------------------------
// Columns [c0, c0 + 128 ntiles) of the vocabulary, c0 a multiple of 128.  With x as in the forward, p_v = exp(x_v - lse):
//     g_v = inv_t ( gl (1[v = a] - p_v) - ge p_v (log p_v + H_r) ),   a p_v of 0 contributing exactly 0 by selection,
// rounded to bf16 once and written as G (Rp x VC, row-major; WG) and as G^T (VC x Rp; WT).  Zeros are written explicitly for
// rows past `rows`, columns past V and dropped rows; a row tile without a live row is zero-filled without the product.
struct GradArgs {
    const uint16_t* hidden; const uint16_t* w; const int64_t* action; const float* weight;
    const float* lse; const float* ent; const float* gl; const float* ge;   // ge NULL: no entropy term (ent is then not read)
    uint16_t* G; uint16_t* GT;
    long rows, Rp; int H, V, c0, VC, ntiles; float inv_t;
};

template <bool WG, bool WT>
__global__ __launch_bounds__(256, 2) void lm_linear_grad_logits_kernel(const GradArgs p) {
    __shared__ __attribute__((aligned(16))) uint16_t lds[2][2][kTileElems];
    __shared__ int s_act[kBM];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long row0 = (long)blockIdx.x * kBM;
    const int sp = blockIdx.y, nsp = gridDim.y;
    const int l0 = (int)((long)p.ntiles * sp / nsp), l1 = (int)((long)p.ntiles * (sp + 1) / nsp);   // this split's tiles of the chunk

    if (!live_rows(s_act, p.action, p.weight, row0, p.rows, p.V)) {
        const vuint4 z = {0u, 0u, 0u, 0u};
        const int pieces = (l1 - l0) * (kBN / 8);              // 16-byte pieces per row of G; G^T has 16 per entry
        if constexpr (WG)
            for (int i = tid; i < kBM * pieces; i += 256)
                *reinterpret_cast<vuint4*>(p.G + (size_t)(row0 + i / pieces) * (size_t)p.VC + (size_t)l0 * kBN + (size_t)(i % pieces) * 8) = z;
        if constexpr (WT)
            for (int i = tid; i < (l1 - l0) * kBN * (kBM / 8); i += 256)
                *reinterpret_cast<vuint4*>(p.GT + ((size_t)l0 * kBN + (size_t)(i >> 4)) * (size_t)p.Rp + (size_t)row0 + (size_t)(i & 15) * 8) = z;
        return;
    }

    const int tok = wv * 32 + (lane & 31), half = lane >> 5;
    const long my_row = row0 + tok;                            // < Rp
    const int my_act = s_act[tok];
    float lse = 0.f, hr = 0.f, gl = 0.f, ge = 0.f;
    if (my_act >= 0) {
        lse = p.lse[my_row];
        if (p.gl) gl = p.gl[my_row];
        if (p.ge) {
            ge = p.ge[my_row];
            hr = p.ent[my_row];
        }
    }
    const int tile0 = p.c0 / kBN;

    floatx16 acc[4];
    product_walk(lds, p.hidden, p.w, p.rows, p.H, p.V, row0, tile0 + l0, tile0 + l1, acc, [&](int vt, int free) {
        const int vb = vt * kBN + half * 4;
        const int left = my_act >= 0 ? p.V - vb : 0, da = my_act - vb;
        const int lt = vt - tile0;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int e = 32 * j + 8 * (i >> 2) + (i & 3);
                const float t = clampf(acc[j][i] * p.inv_t) - lse;                 // log p_v
                const float pv = ex2(t * kLog2eG);
                const float pt = pv == 0.f ? 0.f : pv * fmaf(ge, t + hr, gl);
                const float g = p.inv_t * ((da == e ? gl : 0.f) - pt);
                acc[j][i] = e < left ? g : 0.f;
                if constexpr (WT)   // the 32 lanes of a half-wave hold 32 consecutive tokens of one entry
                    p.GT[((size_t)lt * kBN + (size_t)(e + half * 4)) * (size_t)p.Rp + (size_t)my_row] = (uint16_t)bf16_bits(acc[j][i]);
            }
        if constexpr (WG) {
            store_wave_tile_bf16(&lds[free][0][0] + wv * kSlabElems, acc, p.G + (size_t)(row0 + wv * 32) * (size_t)p.VC + (size_t)lt * kBN,
                                 (size_t)p.VC, 32, kBN, lane);
            __syncthreads();                                   // the slabs are read before the next step is stored over them
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[j][i] = 0.f;
    });
}

__global__ __launch_bounds__(kBM) void lm_linear_combine_kernel(const float4* __restrict__ ws, const int64_t* __restrict__ action,
                                                                const float* __restrict__ weight, float* __restrict__ logp,
                                                                float* __restrict__ entropy, float* __restrict__ lse,
                                                                int* __restrict__ skipped, long rows, int V, int splits) {
    const long r = (long)blockIdx.x * kBM + threadIdx.x;
    int live = 0;
    if (r < rows) {
        const long a = action[r];
        const float w = weight ? weight[r] : 1.f;
        live = a >= 0 && a < (long)V && w != 0.f;
        float lp = 0.f, h = 0.f, l = 0.f;
        if (live) {
            const float4 q = ws[r];
            RowStat<true> st{q.x, q.y, q.z};
            float xa = q.w;
            for (int s = 1; s < splits; ++s) {
                const float4 t = ws[(size_t)s * (size_t)rows + (size_t)r];
                st = stat_merge(st, RowStat<true>{t.x, t.y, t.z});
                xa += t.w;
            }
            const float ls = __builtin_amdgcn_logf(st.s) * kLn2G;   // s is in [1, V]: the bare log2
            l = st.m + ls;
            lp = xa - l;
            h = ls - st.u / st.s;
        }
        logp[r] = lp;
        if (entropy) entropy[r] = h;
        if (lse) lse[r] = l;
    }
    if (!__syncthreads_or(live) && threadIdx.x == 0) atomicAdd(skipped, 1);
}

// the split count by rule: the grid fills the CUs' workgroup slots (two per CU by LDS) in about whole rounds
int splits_by_rule(long row_tiles, long col_tiles) {
    const int cus = device_cus();
    const long slots = 2L * (cus > 0 ? cus : 256);
    long s = row_tiles >= slots ? 1 : slots / row_tiles;
    if (s > col_tiles) s = col_tiles;
    if (s > kMaxSplits) s = kMaxSplits;
    return s < 1 ? 1 : (int)s;
}

int* skipped_word() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    if (!g_skipped_dev[dev] && hipMalloc(reinterpret_cast<void**>(&g_skipped_dev[dev]), 16) != hipSuccess) {
        (void)hipGetLastError();
        g_skipped_dev[dev] = nullptr;
    }
    return g_skipped_dev[dev];
}

// ---- the backward's plan ---------------------------------------------------------------------------------------------------
// What G (and G^T) of one vocabulary chunk may take when the chunk size is chosen by rule.  NOT MEASURED: 256 MiB is a guess
// that keeps the workspace far below the logits it replaces and a chunk's products large enough to fill the device;
// tests/tools/lm_head_grad_bench.py records the call time at 128, 256 and 512 MiB for whoever revisits it.
constexpr int64_t kChunkBudgetBytes = 256LL << 20;

LaunchRecord<6> g_bwd_rec;    // [calls, chunk columns, chunks, dhidden products, dW products, grad-logits launches] of the last call
LaunchRecord<6> g_gemm_rec;   // [launches, BM, BN, BK, threads, LDS bytes] of the last product

struct BwdPlan {
    int64_t Rp;          // rows rounded up to the row tile: the rows of G, the pitch of G^T
    int VC, chunks;      // chunk columns (a multiple of 128), number of chunks
    int64_t g_bytes, gt_bytes, acc_bytes;   // the three parts of the workspace, in this order
};
int plan_backward(int64_t rows, int H, int V, int chunk, bool dh, bool dw, BwdPlan& pl) {
    if (rows < 0 || H <= 0 || V <= 0 || chunk < 0 || chunk % kBN != 0) return HPC_RLL_EINVAL;
    pl.Rp = (rows + kBM - 1) / kBM * kBM;
    const int64_t cap = ((int64_t)V + kBN - 1) / kBN * kBN, nbuf = (dh ? 1 : 0) + (dw ? 1 : 0);
    int64_t vc = chunk;
    if (!vc) vc = (pl.Rp && nbuf) ? kChunkBudgetBytes / (pl.Rp * 2 * nbuf) / kBN * kBN : cap;
    vc = vc < kBN ? kBN : (vc > cap ? cap : vc);
    pl.VC = (int)vc;
    pl.chunks = (int)((V + vc - 1) / vc);
    pl.g_bytes = dh ? pl.Rp * vc * 2 : 0;
    pl.gt_bytes = dw ? pl.Rp * vc * 2 : 0;
    pl.acc_bytes = dh && pl.chunks > 1 ? rows * (int64_t)H * 4 : 0;
    return HPC_RLL_OK;
}

int gemm_noted(const GemmBf16Args& g, int mode, hipStream_t st) {
    const int rc = launch_gemm_bf16(g, mode, st);
    if (!rc) g_gemm_rec.note({kBM, kBN, kBK, 256, kLdsBytes});
    return rc;
}

}  // namespace
}  // namespace hpc_rll

using namespace hpc_rll;

// one float4 (m, s, u, x[a]) per (row, split); splits == 0 asks for what any split count by rule needs
extern "C" int64_t hpc_rll_lm_linear_workspace_bytes(int64_t rows, int splits) {
    if (rows < 0 || splits < 0 || splits > kMaxSplits) return HPC_RLL_EINVAL;
    return rows * (int64_t)(splits ? splits : kMaxSplits) * (int64_t)sizeof(float4);
}

extern "C" int hpc_rll_lm_linear_forward(const void* hidden, const void* w, const int64_t* action, const float* weight,
                                         int64_t rows, int H, int V, float inv_temperature, int splits, void* ws, float* logp,
                                         float* entropy, void* stream) {
    return hpc_rll_lm_linear_forward_lse(hidden, w, action, weight, rows, H, V, inv_temperature, splits, ws, logp, entropy, nullptr,
                                         stream);
}

// the forward that also writes lse (rows), what the backward needs; lse == NULL is hpc_rll_lm_linear_forward
extern "C" int hpc_rll_lm_linear_forward_lse(const void* hidden, const void* w, const int64_t* action, const float* weight,
                                             int64_t rows, int H, int V, float inv_temperature, int splits, void* ws, float* logp,
                                             float* entropy, float* lse, void* stream) {
    if (rows < 0 || H <= 0 || V <= 0 || splits < 0 || splits > kMaxSplits || !(inv_temperature > 0.f) ||
        !(inv_temperature <= kFltMaxG))
        return HPC_RLL_EINVAL;
    if (rows > 0 && (!hidden || !w || !action || !ws || !logp)) return HPC_RLL_EINVAL;
    if (!(aligned(hidden, 16) && aligned(w, 16) && aligned(ws, 16) && aligned(action, 8) && aligned(weight, 4) &&
          aligned(logp, 4) && aligned(entropy, 4) && aligned(lse, 4)))
        return HPC_RLL_EALIGN;
    if (H < kMinH || H > kMaxH || H % 32 != 0 || V > kGrpoMaxV) return HPC_RLL_EUNSUPPORTED;
    if (rows == 0) return HPC_RLL_OK;
    const long row_tiles = (rows + kBM - 1) / kBM, col_tiles = ((long)V + kBN - 1) / kBN;
    if (row_tiles > 0x7fffffffL) return HPC_RLL_EUNSUPPORTED;
    const int ns = splits ? splits : splits_by_rule(row_tiles, col_tiles);
    int* skipped = skipped_word();
    if (!skipped) return (int)hipErrorOutOfMemory;
    hipStream_t st = (hipStream_t)stream;
    const LinArgs p{static_cast<const uint16_t*>(hidden), static_cast<const uint16_t*>(w), action, weight,
                    static_cast<float4*>(ws), skipped, (long)rows, H, V, inv_temperature};
    const dim3 grid((unsigned)row_tiles, (unsigned)ns);
    if (entropy) hipLaunchKernelGGL(lm_linear_kernel<true>, grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL(lm_linear_kernel<false>, grid, dim3(256), 0, st, p);
    int rc = last_error();
    if (rc) return rc;
    hipLaunchKernelGGL(lm_linear_combine_kernel, dim3((unsigned)row_tiles), dim3(kBM), 0, st, static_cast<const float4*>(ws),
                       action, weight, logp, entropy, lse, skipped, (long)rows, V, ns);
    rc = last_error();
    if (rc) return rc;
    g_rec.note({kBM, kBN, kBK, ns, (int)row_tiles, ns, 256, kLdsBytes + (int)sizeof(int) * kBM, entropy ? 1 : 0});
    g_skipped_last = skipped;
    g_stream_last = st;
    return HPC_RLL_OK;
}

// The record of the last launch.  out[10], the row tiles the last call skipped, is counted on the device: this call waits
// for the stream of that launch and copies the word (a diagnostic, not part of the op).
extern "C" int hpc_rll_lm_linear_last_config(int* out) {
    if (!out) return HPC_RLL_EINVAL;
    g_rec.read(out);
    out[kConfigInts] = -1;
    if (g_skipped_last) {
        int rc = (int)hipStreamSynchronize(g_stream_last);
        if (!rc) rc = (int)hipMemcpy(out + kConfigInts, g_skipped_last, sizeof(int), hipMemcpyDeviceToHost);
        if (rc) return rc;
    }
    return HPC_RLL_OK;
}
static_assert(HPC_RLL_LM_LINEAR_CONFIG_INTS == kConfigInts + 1, "the layout documented in hpc_rll_hip.h");

// G (Rp x VC bf16) when dhidden is wanted, G^T (VC x Rp bf16) when dW is, and the fp32 accumulator of dhidden (rows x H) when
// it is wanted and there is more than one chunk; Rp = 128 ceil(rows / 128), VC = the chunk columns (chunk, or by rule for 0),
// capped by 128 ceil(V / 128)
extern "C" int64_t hpc_rll_lm_linear_backward_workspace_bytes(int64_t rows, int H, int V, int chunk, int want_dhidden,
                                                              int want_dw) {
    BwdPlan pl;
    const int rc = plan_backward(rows, H, V, chunk, want_dhidden != 0, want_dw != 0, pl);
    return rc ? rc : pl.g_bytes + pl.gt_bytes + pl.acc_bytes;
}

extern "C" int hpc_rll_lm_linear_gemm(const void* A, int64_t lda, const void* B, int64_t ldb, int64_t M, int N, int64_t K,
                                      int64_t K_valid, const int64_t* live_action, const float* live_weight, int live_V, int mode,
                                      void* C_bf16, float* C_f32, int64_t ldc, void* stream) {
    if (M < 0 || N < 0 || K < 0 || K_valid < 0 || K_valid > K || mode < kStoreBf16 || mode > kAddF32StoreBf16 || lda < K ||
        ldb < N || ldc < N || (live_weight && !live_action))
        return HPC_RLL_EINVAL;
    const bool to_bf16 = mode == kStoreBf16 || mode == kAddF32StoreBf16, f32 = mode != kStoreBf16;
    if (M > 0 && N > 0 && ((K > 0 && !A) || (K_valid > 0 && !B) || (to_bf16 && !C_bf16) || (f32 && !C_f32))) return HPC_RLL_EINVAL;
    if (!(aligned(A, 16) && aligned(B, 16) && aligned(C_bf16, 16) && aligned(C_f32, 16) && aligned(live_action, 8) &&
          aligned(live_weight, 4)))
        return HPC_RLL_EALIGN;
    if (N % 8 || K % 8 || lda % 8 || ldb % 8 || ldc % 8 || (M + kBM - 1) / kBM > 0x7fffffffL || (N + kBN - 1) / kBN > 65535)
        return HPC_RLL_EUNSUPPORTED;
    if (M == 0 || N == 0) return HPC_RLL_OK;
    const GemmBf16Args g{static_cast<const uint16_t*>(A), static_cast<const uint16_t*>(B), static_cast<uint16_t*>(C_bf16), C_f32,
                         live_action, live_weight, (long)M, (long)K, (long)K_valid, (size_t)lda, (size_t)ldb, (size_t)ldc, N, live_V};
    return gemm_noted(g, mode, (hipStream_t)stream);
}

extern "C" int hpc_rll_lm_linear_backward(const float* g_logp, const float* g_entropy, const void* hidden, const void* w,
                                          const int64_t* action, const float* weight, const float* lse, const float* entropy,
                                          int64_t rows, int H, int V, float inv_temperature, int chunk, void* ws, void* grad_hidden,
                                          void* grad_w, void* stream) {
    BwdPlan pl;
    const bool dh = grad_hidden != nullptr, dw = grad_w != nullptr;
    if (plan_backward(rows, H, V, chunk, dh, dw, pl) || !(inv_temperature > 0.f) || !(inv_temperature <= kFltMaxG))
        return HPC_RLL_EINVAL;
    if (rows > 0 && (!hidden || !w || !action || !lse || !ws || (g_entropy && !entropy))) return HPC_RLL_EINVAL;
    if (!(aligned(hidden, 16) && aligned(w, 16) && aligned(ws, 16) && aligned(grad_hidden, 16) && aligned(grad_w, 16) &&
          aligned(action, 8) && aligned(weight, 4) && aligned(g_logp, 4) && aligned(g_entropy, 4) && aligned(lse, 4) &&
          aligned(entropy, 4)))
        return HPC_RLL_EALIGN;
    const long row_tiles = (long)(pl.Rp / kBM);
    if (H < kMinH || H > kMaxH || H % 32 != 0 || V > kGrpoMaxV || row_tiles > 0x7fffffffL) return HPC_RLL_EUNSUPPORTED;
    if (rows == 0 || (!dh && !dw)) return HPC_RLL_OK;
    hipStream_t st = (hipStream_t)stream;
    const uint16_t* hp = static_cast<const uint16_t*>(hidden);
    const uint16_t* wp = static_cast<const uint16_t*>(w);
    uint16_t* G = static_cast<uint16_t*>(ws);
    uint16_t* GT = reinterpret_cast<uint16_t*>(static_cast<char*>(ws) + pl.g_bytes);
    float* acc = reinterpret_cast<float*>(static_cast<char*>(ws) + pl.g_bytes + pl.gt_bytes);
    int n_dh = 0, n_dw = 0, n_grad = 0;
    for (int c = 0; c < pl.chunks; ++c) {
        const int c0 = c * pl.VC, ncols = V - c0 < pl.VC ? V - c0 : pl.VC, ntiles = (ncols + kBN - 1) / kBN;
        const GradArgs ga{hp, wp, action, weight, lse, entropy, g_logp, g_entropy, G, GT, (long)rows, (long)pl.Rp,
                          H, V, c0, pl.VC, ntiles, inv_temperature};
        const dim3 grid((unsigned)row_tiles, (unsigned)splits_by_rule(row_tiles, ntiles));
        if (dh && dw) hipLaunchKernelGGL((lm_linear_grad_logits_kernel<true, true>), grid, dim3(256), 0, st, ga);
        else if (dh) hipLaunchKernelGGL((lm_linear_grad_logits_kernel<true, false>), grid, dim3(256), 0, st, ga);
        else hipLaunchKernelGGL((lm_linear_grad_logits_kernel<false, true>), grid, dim3(256), 0, st, ga);
        int rc = last_error();
        if (rc) return rc;
        ++n_grad;
        if (dh) {   // dhidden (+)= G W[c0 ..]: fp32 across chunks in chunk order, bf16 from the last (or only) one
            const int mode = pl.chunks == 1 ? kStoreBf16 : c == 0 ? kStoreF32 : c + 1 < pl.chunks ? kAddF32 : kAddF32StoreBf16;
            const GemmBf16Args g{G, wp + (size_t)c0 * (size_t)H, static_cast<uint16_t*>(grad_hidden), acc, nullptr, nullptr,
                                 (long)rows, (long)ntiles * kBN, (long)ncols, (size_t)pl.VC, (size_t)H, (size_t)H, H, 0};
            if ((rc = gemm_noted(g, mode, st))) return rc;
            ++n_dh;
        }
        if (dw) {   // dW[c0 ..] = G^T hidden: the chunk's rows, written once; dropped rows of hidden load as zeros
            const GemmBf16Args g{GT, hp, static_cast<uint16_t*>(grad_w) + (size_t)c0 * (size_t)H, nullptr, action, weight,
                                 (long)ncols, (long)pl.Rp, (long)rows, (size_t)pl.Rp, (size_t)H, (size_t)H, H, V};
            if ((rc = gemm_noted(g, kStoreBf16, st))) return rc;
            ++n_dw;
        }
    }
    g_bwd_rec.note({pl.VC, pl.chunks, n_dh, n_dw, n_grad});
    return HPC_RLL_OK;
}

// The records of the backward and of the product: plain host ints, nothing is waited for.
extern "C" int hpc_rll_lm_linear_backward_last_config(int* out) {
    if (!out) return HPC_RLL_EINVAL;
    g_bwd_rec.read(out);
    g_gemm_rec.read(out + 6);
    return HPC_RLL_OK;
}
static_assert(HPC_RLL_LM_LINEAR_BACKWARD_CONFIG_INTS == 12, "the layout documented in hpc_rll_hip.h");
