// lm_linear.hip -- the language-model head fused with its bf16 matrix product on gfx950: the log-probability (and the entropy)
// of given tokens straight from the hidden states and the head's weight.  No logit is ever written to memory.
//
// hidden (rows, H) bf16, w (V, H) bf16 (nn.Linear.weight's own layout), action (rows) int64, weight (rows) fp32 or NULL.
// With x = (hidden w^T) inv_temperature held in fp32:  logp = x[a] - logsumexp(x),  entropy = logsumexp(x) - sum p x.
// No gradient: the differentiable head needs two further matrix forms and is not here.
//
// Two launches:
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
#include <hip/hip_runtime.h>

#include "hostutil.hpp"
#include "hpc_rll_hip.h"
#include "lm_head.hpp"

namespace hpc_rll {
namespace {

constexpr int kBM = 128, kBN = 128, kBK = 64;   // tokens, vocabulary entries and contraction elements of a workgroup's step
constexpr int kPitch = kBK + 8;                 // LDS row pitch in bf16: 144 bytes
constexpr int kTileElems = 128 * kPitch;        // one operand tile of one buffer (kBM == kBN == 128 rows)
constexpr int kLdsBytes = 2 * 2 * kTileElems * 2;
constexpr int kMaxSplits = 64, kMinH = 32, kMaxH = 16384;
constexpr int kChunks = 128 * (kBK / 8) / 256;  // 16-byte chunks of one operand tile per thread: 4
static_assert(kBM == 128 && kBN == 128 && kBK == 64 && kChunks == 4, "the thread mapping below is written for these");

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float floatx16 __attribute__((ext_vector_type(16)));

constexpr int kConfigInts = 10;   // the host part of the record; the skipped row tiles are read from the device
LaunchRecord<kConfigInts> g_rec;
int* g_skipped_dev[64] = {};      // one device word per device, allocated at the first launch there and kept
int* g_skipped_last = nullptr;
hipStream_t g_stream_last = nullptr;

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

    // ---- which of the 128 rows are live; a tile without one is not computed
    int live = 0;
    if (tid < kBM) {
        const long r = row0 + tid;
        long a = -1;
        float w = 1.f;
        if (r < p.rows) {
            a = p.action[r];
            if (p.weight) w = p.weight[r];
        }
        live = a >= 0 && a < (long)p.V && w != 0.f;
        s_act[tid] = live ? (int)a : -1;
    }
    if (!__syncthreads_or(live)) return;

    const int tok = wv * 32 + (lane & 31), half = lane >> 5;
    const long my_row = row0 + tok;
    const int my_act = s_act[tok];

    // ---- the column tiles of this split: [t0, t1) of ceil(V / 128)
    const long nct = ((long)p.V + kBN - 1) / kBN;
    const int t0 = (int)(nct * sp / nsp), t1 = (int)(nct * (sp + 1) / nsp);
    const int nk = (p.H + kBK - 1) / kBK;
    const long steps = (long)(t1 - t0) * nk;

    // ---- the 16-byte chunks this thread moves: rows (tid >> 3) + 32 i, 8 bf16 at column (tid & 7) 8 of the K step
    const int lr = tid >> 3, kc = (tid & 7) * 8;
    const uint16_t* hp[kChunks];
#pragma unroll
    for (int i = 0; i < kChunks; ++i) {
        long r = row0 + lr + 32 * i;
        r = r < p.rows ? r : p.rows - 1;                       // clamped: never past the last row
        hp[i] = p.hidden + (size_t)r * (size_t)p.H + kc;
    }
    vuint4 ra[kChunks], rb[kChunks];
    auto gload = [&](int vt, int ks) {
        const int k = ks * kBK;
        const bool ok = k + kc < p.H;                          // H is a multiple of 32: a chunk is inside or outside as a whole
        const vuint4 z = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < kChunks; ++i) {
            long v = (long)vt * kBN + lr + 32 * i;
            v = v < (long)p.V ? v : (long)p.V - 1;             // clamped: the epilogue selects such columns away
            ra[i] = z;
            rb[i] = z;
            if (ok) {
                ra[i] = *reinterpret_cast<const vuint4*>(p.w + (size_t)v * (size_t)p.H + k + kc);
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

    floatx16 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[j][i] = 0.f;
    RowStat<ENT> st{-kFltMaxG, 0.f};
    if constexpr (ENT) st.u = 0.f;
    float xa = 0.f;

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
        // ---- four K sub-steps of 16: the token fragment once, the four weight fragments against it
        const uint16_t* la = &lds[cur][0][(lane & 31) * kPitch + half * 8];
        const uint16_t* lb = &lds[cur][1][tok * kPitch + half * 8];
#pragma unroll
        for (int q = 0; q < kBK / 16; ++q) {
            const bf16x8 b = *reinterpret_cast<const bf16x8*>(lb + q * 16);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bf16x8 a = *reinterpret_cast<const bf16x8*>(la + j * 32 * kPitch + q * 16);
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc[j], 0, 0, 0);
            }
        }
        if (ks == nk - 1) {
            // ---- the tile's logits are complete: acc[j][i] is vocabulary entry vt 128 + 32 j + 8 (i / 4) + 4 half + i % 4
            const int vb = vt * kBN + half * 4;
            const int left = p.V - vb, da = my_act - vb;       // entry e (a constant below) exists iff e < left
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
        }
        if (more) lstore(cur ^ 1);
        __syncthreads();
        cur ^= 1;
        vt = nvt;
        ks = nks;
    }

    // ---- the two lanes of a token meet; one partial per (row, split)
    RowStat<ENT> o{__shfl_xor(st.m, 32, 64), __shfl_xor(st.s, 32, 64)};
    if constexpr (ENT) o.u = __shfl_xor(st.u, 32, 64);
    st = stat_merge(st, o);
    xa += __shfl_xor(xa, 32, 64);
    if (half == 0 && my_row < p.rows) {
        float4 out = make_float4(-kFltMaxG, 0.f, 0.f, 0.f);   // a dropped row, or a split without columns: the identity
        if (my_act >= 0 && steps > 0) {
            out.x = st.m;
            out.y = st.s;
            if constexpr (ENT) out.z = st.u;
            out.w = xa;
        }
        p.ws[(size_t)sp * (size_t)p.rows + (size_t)my_row] = out;
    }
}

__global__ __launch_bounds__(kBM) void lm_linear_combine_kernel(const float4* __restrict__ ws, const int64_t* __restrict__ action,
                                                                const float* __restrict__ weight, float* __restrict__ logp,
                                                                float* __restrict__ entropy, int* __restrict__ skipped, long rows,
                                                                int V, int splits) {
    const long r = (long)blockIdx.x * kBM + threadIdx.x;
    int live = 0;
    if (r < rows) {
        const long a = action[r];
        const float w = weight ? weight[r] : 1.f;
        live = a >= 0 && a < (long)V && w != 0.f;
        float lp = 0.f, h = 0.f;
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
            lp = xa - (st.m + ls);
            h = ls - st.u / st.s;
        }
        logp[r] = lp;
        if (entropy) entropy[r] = h;
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
    if (rows < 0 || H <= 0 || V <= 0 || splits < 0 || splits > kMaxSplits || !(inv_temperature > 0.f) ||
        !(inv_temperature <= kFltMaxG))
        return HPC_RLL_EINVAL;
    if (rows > 0 && (!hidden || !w || !action || !ws || !logp)) return HPC_RLL_EINVAL;
    if (!(aligned(hidden, 16) && aligned(w, 16) && aligned(ws, 16) && aligned(action, 8) && aligned(weight, 4) &&
          aligned(logp, 4) && aligned(entropy, 4)))
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
                       action, weight, logp, entropy, skipped, (long)rows, V, ns);
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
