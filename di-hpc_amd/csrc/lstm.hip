// lstm.hip -- multi-layer LayerNorm-LSTM forward + full BPTT backward for gfx950.
//
// Replaces LstmForward/LstmBackward (src/torch_utils/network/lstm.cu:29-379, lstm_kernel.h:12-183).
// Semantics: hpc_rll/origin/rnn.py:193-248:
//     gate = LN_x(x_s Wx) + LN_h(h Wh) + bias ;  i,f,o = sigmoid, u = tanh (order i,f,o,u)
//     c = f*c + i*u ;  h = o*tanh(c) ;  dropout between layers only.
//
// Reference structure per (layer, step): cublasSgemm + layernorm kernel + activation kernel (3 launches), a cuBLAS
// handle created per call, LayerNorm of the x-branch as a separate pass over (S*B,4H), per-step SGEMMs with beta=1
// for dWx/dWh, float atomics for dbias/dgamma/dbeta, and the incoming dh/dc of the final states are zeroed
// (lstm.cu:309-310: gradients through hn/cn are dropped).  Here:
//   * all GEMMs are exact-fp32 MFMA (gemm_f32.hpp); the x-branch GEMM, dWx, dWh and dx are ONE large GEMM per
//     layer each (K = S*B for the weight gradients) instead of S small accumulating ones;
//   * per step: 1 GEMM + 1 fused cell kernel.  The cell kernel does BOTH LayerNorms (two-pass mean/variance in
//     registers), bias, gates and the state update; the x-branch LN is never materialised;
//   * backward: 1 fused cell kernel (gate adjoint + both LayerNorm adjoints) + 1 GEMM per step; bias / gamma /
//     beta gradients are a single deterministic column reduction over the saved gate gradients per layer (no
//     atomics); gradients through hn / cn are propagated (the correct adjoint, matches the oracle).
//   * dropout masks are a stateless hash of (seed, layer, element): nothing to store, backward recomputes them
//     (the reference draws cuRAND numbers seeded from /dev/urandom: parity-unpinned, tests use dropout = 0).
#include <hip/hip_runtime.h>

#include <atomic>

#include "gemm_f32.hpp"
#include "hostutil.hpp"
#include "hpc_rll_hip.h"
#include "wave.hpp"

namespace hpc_rll {
// path switches that tests flip (hpc_rll_tune_set, tune.hip); the measured launch parameters of round 1-4 are constants now
int g_gemm_dma = 1;       // key 25: LDS-DMA staging of the NT / TN / NN products (gemm_f32.hpp: DmaStage); 0 = register staging
int g_gemm_tile256 = 1;   // key 16: 256x256x16 tiles (16 waves) for interior products that fill the chip in whole rounds
constexpr int g_cell_vec4 = 3;        // smallest ceil(H/256) that takes the 16-byte forward cell kernel
constexpr int g_lstm_dh_big = 1;      // dh_prev of large batches on the weight-gradient tiling (128x128, own split-K)
constexpr int g_lstm_nn_bwd = 1;      // backward products of large batches against transposed weight copies
constexpr int g_cell_rows_wgs = 512;  // workgroups of the row-walking backward cell
namespace {

constexpr float kLnEps = 1e-5f;

// Sum K values over the 256 threads of the workgroup; every thread gets the totals.  `lds` holds >= K*4 floats.
template <int K>
__device__ __forceinline__ void block_allsum(float (&v)[K], float* lds) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const float s = wave_sum(v[k]);
        if (lane == 0) lds[k * 4 + w] = s;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = (lds[k * 4] + lds[k * 4 + 1]) + (lds[k * 4 + 2] + lds[k * 4 + 3]);
    __syncthreads();
}

// Gate pre-activation and activations: ONE definition shared by the forward cells and by the backward cells that
// recompute the gates instead of loading saved ones (the same expression tree, hence the same contraction).
__device__ __forceinline__ float gate_pre(float x, float mx, float rx, float gx, float bx, float h, float mh, float rh,
                                          float gh, float bh, float b) {
    return (x - mx) * rx * gx + bx + (h - mh) * rh * gh + bh + b;
}
__device__ __forceinline__ float gate_sigmoid(float a) { return 1.f / (1.f + expf(-a)); }

// Large batches do not SAVE the four activated gates (S*B*4H floats written by the forward, read by the backward: 27 % of
// the forward cell's bytes and 12 % of the backward cell's at the C4 shape): the backward recomputes them from what it
// reads anyway (both pre-LayerNorm products, the row statistics, gamma) plus bias / beta, parked in the workspace by the
// forward.  Shape-only predicate (forward and backward must agree, whatever the tuning knobs say).
inline bool cell_recompute_gates(int B, int H) { return (long)B * H >= (1L << 19); }

// Layout of the (rows, 4H) pre-activation tensors (xw, hw, dxw, dhw).  Standard: gate g of hidden unit u at column
// g*H + u (the reference's, lstm_kernel.h:46-60).  GATE-INTERLEAVED (PERM; large batches, lstm_perm_shape): at column
// 4*u + g, produced by multiplying with column-permuted weight copies -- a matrix-core lane of the NN kernels owns four
// CONSECUTIVE output columns, so in this layout it owns the four gates of one unit and the cell can run in the product's
// own epilogue (lstm_block.hpp).  LayerNorm over a row does not care about the column order.  Four consecutive units x
// four gates are one 16-byte access per gate (standard) or per unit (interleaved: 64 contiguous bytes, a 4x4 transpose in
// registers).
inline bool lstm_perm_shape(int B, int H) {
    return cell_recompute_gates(B, H) && H % 64 == 0 && H >= 768 && H <= 1024 && B % 256 == 0 && B >= 4096;
}
template <bool PERM, bool NT>
__device__ __forceinline__ void load_gq(const float* row, int H, int u0, vfloat4 (&v)[4]) {
    if (PERM) {
        vfloat4 t[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) t[i] = ld<NT>(reinterpret_cast<const vfloat4*>(row + 4 * (u0 + i)));
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int i = 0; i < 4; ++i) v[g][i] = t[i][g];
    } else {
#pragma unroll
        for (int g = 0; g < 4; ++g) v[g] = ld<NT>(reinterpret_cast<const vfloat4*>(row + g * H + u0));
    }
}
template <bool PERM, bool NT>
__device__ __forceinline__ void store_gq(float* row, int H, int u0, const vfloat4 (&v)[4]) {
    if (PERM) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            vfloat4 t;
#pragma unroll
            for (int g = 0; g < 4; ++g) t[g] = v[g][i];
            st<NT>(reinterpret_cast<vfloat4*>(row + 4 * (u0 + i)), t);
        }
    } else {
#pragma unroll
        for (int g = 0; g < 4; ++g) st<NT>(reinterpret_cast<vfloat4*>(row + g * H + u0), v[g]);
    }
}

// ------------------------------------------------------------------------------------------------ forward cell
// one workgroup per batch row; thread t owns hidden units j = t, t+256, ... (JPT of them) x 4 gates x 2 branches.
template <int JPT>
__global__ __launch_bounds__(256) void lstm_cell_fwd_kernel(
    const float* __restrict__ xw, const float* hw /* nsplit partial products, stride part_stride */, int nsplit,
    long part_stride, float* hw_out /* summed h-branch pre-activation (saved for backward); may alias hw */,
    const float* __restrict__ bias, const float* __restrict__ gamma, const float* __restrict__ beta,
    const float* __restrict__ c_prev, float* __restrict__ gates, float* __restrict__ c_out,
    float* __restrict__ h_out, float* __restrict__ stats, int H) {
    __shared__ float red[16];
    const int b = blockIdx.x;
    const int G = 4 * H;
    const float* __restrict__ xr = xw + (size_t)b * G;
    const float* hr = hw + (size_t)b * G;
    float x[JPT][4], h[JPT][4];
    float s[2] = {0.f, 0.f};
#pragma unroll
    for (int q = 0; q < JPT; ++q) {
        const int j = threadIdx.x + q * 256;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            x[q][g] = (j < H) ? xr[g * H + j] : 0.f;
            h[q][g] = (j < H) ? hr[g * H + j] : 0.f;
        }
    }
    // split-K partials: summed in slice order (deterministic).  The slice loop is outermost and takes ZC slices
    // per round so that 4*ZC*JPT loads are in flight together (element by element this was ~10 us of dependent round
    // trips at nsplit = 8).
    constexpr int ZC = JPT <= 2 ? 4 : JPT <= 4 ? 2 : 1;   // slices per round (register budget)
    for (int z = 1; z < nsplit; z += ZC) {
        float p[ZC][JPT][4];
#pragma unroll
        for (int zz = 0; zz < ZC; ++zz)
#pragma unroll
            for (int q = 0; q < JPT; ++q) {
                const int j = threadIdx.x + q * 256;
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    p[zz][q][g] = (j < H && z + zz < nsplit) ? hr[(size_t)(z + zz) * part_stride + g * H + j] : 0.f;
            }
#pragma unroll
        for (int zz = 0; zz < ZC; ++zz)
#pragma unroll
            for (int q = 0; q < JPT; ++q)
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    if (z + zz < nsplit) h[q][g] += p[zz][q][g];
    }
#pragma unroll
    for (int q = 0; q < JPT; ++q) {
        const int j = threadIdx.x + q * 256;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            if (nsplit > 1 && j < H) hw_out[(size_t)b * G + g * H + j] = h[q][g];
            s[0] += x[q][g];
            s[1] += h[q][g];
        }
    }
    // parameters and c_prev do not depend on the reductions: fetch them now so their latency hides behind the two
    // block sums (at small B this kernel is a chain of memory round trips, not arithmetic)
    constexpr bool kPrefetch = JPT <= 2;
    float pgx[kPrefetch ? JPT : 1][4], pgh[kPrefetch ? JPT : 1][4], pbs[kPrefetch ? JPT : 1][4], pc[kPrefetch ? JPT : 1];
    float pbx[kPrefetch ? JPT : 1][4], pbh[kPrefetch ? JPT : 1][4];
    if (kPrefetch) {
#pragma unroll
        for (int q = 0; q < JPT; ++q) {
            const int j = threadIdx.x + q * 256;
            pc[q] = (j < H) ? c_prev[(size_t)b * H + j] : 0.f;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int col = g * H + j;
                pgx[q][g] = (j < H) ? gamma[col] : 0.f;
                pgh[q][g] = (j < H) ? gamma[G + col] : 0.f;
                pbs[q][g] = (j < H) ? bias[col] : 0.f;
                pbx[q][g] = (j < H) ? beta[col] : 0.f;
                pbh[q][g] = (j < H) ? beta[G + col] : 0.f;
            }
        }
    }
    block_allsum<2>(s, red);
    const float inv_g = 1.f / (float)G;
    const float mx = s[0] * inv_g, mh = s[1] * inv_g;
    float v[2] = {0.f, 0.f};
#pragma unroll
    for (int q = 0; q < JPT; ++q) {
        const int j = threadIdx.x + q * 256;
        if (j < H) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                v[0] += (x[q][g] - mx) * (x[q][g] - mx);
                v[1] += (h[q][g] - mh) * (h[q][g] - mh);
            }
        }
    }
    block_allsum<2>(v, red);
    const float rx = rsqrtf(v[0] * inv_g + kLnEps), rh = rsqrtf(v[1] * inv_g + kLnEps);
    if (threadIdx.x == 0) {
        float* st = stats + (size_t)b * 4;
        st[0] = mx; st[1] = rx; st[2] = mh; st[3] = rh;
    }
#pragma unroll
    for (int q = 0; q < JPT; ++q) {
        const int j = threadIdx.x + q * 256;
        if (j < H) {
            float a[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int col = g * H + j;
                const float gxv = kPrefetch ? pgx[kPrefetch ? q : 0][g] : gamma[col];
                const float ghv = kPrefetch ? pgh[kPrefetch ? q : 0][g] : gamma[G + col];
                const float bv = kPrefetch ? pbs[kPrefetch ? q : 0][g] : bias[col];
                const float bxv = kPrefetch ? pbx[kPrefetch ? q : 0][g] : beta[col];
                const float bhv = kPrefetch ? pbh[kPrefetch ? q : 0][g] : beta[G + col];
                a[g] = gate_pre(x[q][g], mx, rx, gxv, bxv, h[q][g], mh, rh, ghv, bhv, bv);
            }
            const float ig = gate_sigmoid(a[0]);
            const float fg = gate_sigmoid(a[1]);
            const float og = gate_sigmoid(a[2]);
            const float ug = tanhf(a[3]);
            const float c = fg * (kPrefetch ? pc[kPrefetch ? q : 0] : c_prev[(size_t)b * H + j]) + ig * ug;
            if (gates) {   // null: the backward recomputes them (cell_recompute_gates)
                float* gr = gates + (size_t)b * G;
                gr[j] = ig; gr[H + j] = fg; gr[2 * H + j] = og; gr[3 * H + j] = ug;
            }
            c_out[(size_t)b * H + j] = c;
            h_out[(size_t)b * H + j] = og * tanhf(c);
        }
    }
}

// The same cell with 16-byte memory operations (H % 4 == 0, 16-byte aligned rows): thread t owns the unit QUADS
// (t + qq*256)*4 .. +3, so every load/store of a wave is one contiguous 1 KiB span instead of 256 B of 4-byte
// accesses (the scalar kernel ran at 4.2 TB/s at the C4 shape; a streaming read reaches 7).  Same arithmetic, same
// summation order inside a thread up to the unit mapping; the block sums are order-insensitive to fp32 rounding only
// within the usual 1e-7.
template <int NQ, bool PERM = false>
__global__ __launch_bounds__(256) void lstm_cell_fwd4_kernel(
    const float* __restrict__ xw, const float* hw, int nsplit, long part_stride, float* hw_out,
    const float* __restrict__ bias, const float* __restrict__ gamma, const float* __restrict__ beta,
    const float* __restrict__ c_prev, float* __restrict__ gates, float* __restrict__ c_out,
    float* __restrict__ h_out, float* __restrict__ stats, int H) {
    __shared__ float red[16];
    const int b = blockIdx.x;
    const int G = 4 * H;
    const float* __restrict__ xr = xw + (size_t)b * G;
    const float* hr = hw + (size_t)b * G;
    vfloat4 x[NQ][4], h[NQ][4];
    const vfloat4 zero4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int qq = 0; qq < NQ; ++qq) {
        const int u0 = ((int)threadIdx.x + qq * 256) * 4;
        if (u0 < H) {
            load_gq<PERM, true>(xr, H, u0, x[qq]);
            load_gq<PERM, false>(hr, H, u0, h[qq]);
        } else {
#pragma unroll
            for (int g = 0; g < 4; ++g) x[qq][g] = h[qq][g] = zero4;
        }
    }
    for (int z = 1; z < nsplit; ++z) {   // split-K partials, in slice order
        vfloat4 p[NQ][4];
#pragma unroll
        for (int qq = 0; qq < NQ; ++qq) {
            const int u0 = ((int)threadIdx.x + qq * 256) * 4;
            if (u0 < H) load_gq<PERM, false>(hr + (size_t)z * part_stride, H, u0, p[qq]);
            else {
#pragma unroll
                for (int g = 0; g < 4; ++g) p[qq][g] = zero4;
            }
        }
#pragma unroll
        for (int qq = 0; qq < NQ; ++qq)
#pragma unroll
            for (int g = 0; g < 4; ++g) h[qq][g] += p[qq][g];
    }
    float s[2] = {0.f, 0.f};
#pragma unroll
    for (int qq = 0; qq < NQ; ++qq) {
        const int u0 = ((int)threadIdx.x + qq * 256) * 4;
        if (nsplit > 1 && u0 < H) store_gq<PERM, false>(hw_out + (size_t)b * G, H, u0, h[qq]);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                s[0] += x[qq][g][i];
                s[1] += h[qq][g][i];
            }
        }
    }
    block_allsum<2>(s, red);
    const float inv_g = 1.f / (float)G;
    const float mx = s[0] * inv_g, mh = s[1] * inv_g;
    float v[2] = {0.f, 0.f};
#pragma unroll
    for (int qq = 0; qq < NQ; ++qq) {
        const int u0 = ((int)threadIdx.x + qq * 256) * 4;
        if (u0 < H) {
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    v[0] += (x[qq][g][i] - mx) * (x[qq][g][i] - mx);
                    v[1] += (h[qq][g][i] - mh) * (h[qq][g][i] - mh);
                }
        }
    }
    block_allsum<2>(v, red);
    const float rx = rsqrtf(v[0] * inv_g + kLnEps), rh = rsqrtf(v[1] * inv_g + kLnEps);
    if (threadIdx.x == 0) {
        float* st = stats + (size_t)b * 4;
        st[0] = mx; st[1] = rx; st[2] = mh; st[3] = rh;
    }
#pragma unroll
    for (int qq = 0; qq < NQ; ++qq) {
        const int u0 = ((int)threadIdx.x + qq * 256) * 4;
        if (u0 < H) {
            vfloat4 act[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int col = g * H + u0;
                const vfloat4 gxv = *reinterpret_cast<const vfloat4*>(gamma + col);
                const vfloat4 ghv = *reinterpret_cast<const vfloat4*>(gamma + G + col);
                const vfloat4 bxv = *reinterpret_cast<const vfloat4*>(beta + col);
                const vfloat4 bhv = *reinterpret_cast<const vfloat4*>(beta + G + col);
                const vfloat4 bv = *reinterpret_cast<const vfloat4*>(bias + col);
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    act[g][i] = gate_pre(x[qq][g][i], mx, rx, gxv[i], bxv[i], h[qq][g][i], mh, rh, ghv[i], bhv[i], bv[i]);
            }
            const vfloat4 cp = *reinterpret_cast<const vfloat4*>(c_prev + (size_t)b * H + u0);
            vfloat4 ig, fg, og, ug, cn, hn;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                ig[i] = gate_sigmoid(act[0][i]);
                fg[i] = gate_sigmoid(act[1][i]);
                og[i] = gate_sigmoid(act[2][i]);
                ug[i] = tanhf(act[3][i]);
                cn[i] = fg[i] * cp[i] + ig[i] * ug[i];
                hn[i] = og[i] * tanhf(cn[i]);
            }
            if (gates) {   // null: the backward recomputes them (cell_recompute_gates)
                float* gr = gates + (size_t)b * G + u0;
                *reinterpret_cast<vfloat4*>(gr) = ig;
                *reinterpret_cast<vfloat4*>(gr + H) = fg;
                *reinterpret_cast<vfloat4*>(gr + 2 * H) = og;
                *reinterpret_cast<vfloat4*>(gr + 3 * H) = ug;
            }
            *reinterpret_cast<vfloat4*>(c_out + (size_t)b * H + u0) = cn;
            *reinterpret_cast<vfloat4*>(h_out + (size_t)b * H + u0) = hn;
        }
    }
}

// ------------------------------------------------------------------------------------------------ backward cell
// dh = dh_a + dh_b (either may be null); outputs dgate, dXW, dHW rows and dc_prev.
template <int JPT>
__global__ __launch_bounds__(256) void lstm_cell_bwd_kernel(
    const float* __restrict__ dh_a, const float* __restrict__ dh_b /* nsplit partials, stride part_stride */,
    int nsplit, long part_stride, const float* dc_in /* may alias dc_prev */,
    const float* __restrict__ gates, const float* __restrict__ c_new, const float* __restrict__ c_prev,
    const float* __restrict__ xw, const float* __restrict__ hw, const float* __restrict__ stats,
    const float* __restrict__ gamma, const float* __restrict__ beta /* with bias: read only when gates == null */,
    const float* __restrict__ bias, float* __restrict__ dgate, float* __restrict__ dxw, float* __restrict__ dhw,
    float* dc_prev, int H) {
    __shared__ float red[16];
    const int b = blockIdx.x;
    const int G = 4 * H;
    const float* st = stats + (size_t)b * 4;
    const float mx = st[0], rx = st[1], mh = st[2], rh = st[3];
    float da[JPT][4], xh[JPT][4], hh[JPT][4];   // gate adjoint, normalised x-branch, normalised h-branch
    float r[4] = {0.f, 0.f, 0.f, 0.f};          // sum dy_g (x), sum dy_g*xhat (x), same for h
    float dh_tot[JPT];                          // dh = dh_a + sum of the split-K partials, in slice order
#pragma unroll
    for (int q = 0; q < JPT; ++q) {
        const int j = threadIdx.x + q * 256;
        dh_tot[q] = (dh_a && j < H) ? dh_a[(size_t)b * H + j] : 0.f;
    }
    if (dh_b) {
        for (int z = 0; z < nsplit; z += 4) {   // four slices (4*JPT loads) in flight per round
            float p[4][JPT];
#pragma unroll
            for (int zz = 0; zz < 4; ++zz)
#pragma unroll
                for (int q = 0; q < JPT; ++q) {
                    const int j = threadIdx.x + q * 256;
                    p[zz][q] = (j < H && z + zz < nsplit) ? dh_b[(size_t)(z + zz) * part_stride + (size_t)b * H + j] : 0.f;
                }
#pragma unroll
            for (int zz = 0; zz < 4; ++zz)
#pragma unroll
                for (int q = 0; q < JPT; ++q)
                    if (z + zz < nsplit) dh_tot[q] += p[zz][q];
        }
    }
#pragma unroll
    for (int q = 0; q < JPT; ++q) {
        const int j = threadIdx.x + q * 256;
        if (j < H) {
            const size_t o = (size_t)b * H + j;
            float xv[4], hv[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                xv[g] = xw[(size_t)b * G + g * H + j];
                hv[g] = hw[(size_t)b * G + g * H + j];
            }
            float ig, fg, og, ug;
            if (gates) {
                const float* gr = gates + (size_t)b * G;
                ig = gr[j]; fg = gr[H + j]; og = gr[2 * H + j]; ug = gr[3 * H + j];
            } else {   // recompute (cell_recompute_gates): the forward's own expression
                float a[4];
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int col = g * H + j;
                    a[g] = gate_pre(xv[g], mx, rx, gamma[col], beta[col], hv[g], mh, rh, gamma[G + col], beta[G + col], bias[col]);
                }
                ig = gate_sigmoid(a[0]); fg = gate_sigmoid(a[1]); og = gate_sigmoid(a[2]); ug = tanhf(a[3]);
            }
            const float dh = dh_tot[q];
            const float tc = tanhf(c_new[o]);
            const float dc = (dc_in ? dc_in[o] : 0.f) + dh * og * (1.f - tc * tc);
            da[q][0] = dc * ug * ig * (1.f - ig);
            da[q][1] = dc * c_prev[o] * fg * (1.f - fg);
            da[q][2] = dh * tc * og * (1.f - og);
            da[q][3] = dc * ig * (1.f - ug * ug);
            dc_prev[o] = dc * fg;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int col = g * H + j;
                xh[q][g] = (xv[g] - mx) * rx;
                hh[q][g] = (hv[g] - mh) * rh;
                const float dyx = da[q][g] * gamma[col], dyh = da[q][g] * gamma[G + col];
                r[0] += dyx; r[1] += dyx * xh[q][g];
                r[2] += dyh; r[3] += dyh * hh[q][g];
                dgate[(size_t)b * G + col] = da[q][g];
            }
        }
    }
    block_allsum<4>(r, red);
    const float inv_g = 1.f / (float)G;
#pragma unroll
    for (int q = 0; q < JPT; ++q) {
        const int j = threadIdx.x + q * 256;
        if (j < H) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int col = g * H + j;
                const float dyx = da[q][g] * gamma[col], dyh = da[q][g] * gamma[G + col];
                dxw[(size_t)b * G + col] = rx * (dyx - r[0] * inv_g - xh[q][g] * r[1] * inv_g);
                dhw[(size_t)b * G + col] = rh * (dyh - r[2] * inv_g - hh[q][g] * r[3] * inv_g);
            }
        }
    }
}

// The same backward cell with 16-byte memory operations (H % 4 == 0, 16-byte aligned rows; the unit-quad mapping of
// lstm_cell_fwd4_kernel): every load / store of a wave is one contiguous 1 KiB span.  Same arithmetic per element and
// the same slice order for dh; the four row sums are accumulated per thread over its quads in a different order than
// the 4-byte kernel's (fp32 rounding only).  Split into a LOAD half (issues every per-row memory read of a thread's
// quads, no use) and a COMPUTE half, so that a workgroup that walks several rows can request row b+1 before it
// computes row b.
struct CellBwdArgs {
    const float *dh_a, *dh_b;   // dh = dh_a + sum of nsplit partials of dh_b (stride part_stride), either may be null
    int nsplit;
    long part_stride;
    const float* dc_in;         // may alias dc_prev
    const float *gates /* null: recompute */, *c_new, *c_prev, *xw, *hw, *stats, *gamma, *beta, *bias;
    float *dgate, *dxw, *dhw, *dc_prev;
    int H;
};
template <int NQ, bool SAVED /* gates are loaded, not recomputed */> struct CellBwdRow {
    vfloat4 xv[NQ][4], hv[NQ][4], gv[SAVED ? NQ : 1][SAVED ? 4 : 1], cn[NQ], cp[NQ], dci[NQ], dh[NQ];
    float mx, rx, mh, rh;
};
template <int NQ, bool SAVED>
__device__ __forceinline__ void cell_bwd4_load(const CellBwdArgs& a, int b, CellBwdRow<NQ, SAVED>& r) {
    const int H = a.H, G = 4 * H;
    const vfloat4 zero4 = {0.f, 0.f, 0.f, 0.f};
    const float* st = a.stats + (size_t)b * 4;
    r.mx = st[0]; r.rx = st[1]; r.mh = st[2]; r.rh = st[3];
#pragma unroll
    for (int qq = 0; qq < NQ; ++qq) {
        const int u0 = ((int)threadIdx.x + qq * 256) * 4;
        const int uu = u0 < H ? u0 : 0;   // idle quads re-read quad 0 (no divergent branch around a load), results unused
        const size_t o = (size_t)b * H + uu;
        const size_t og0 = (size_t)b * G + uu;
        load_gq<false, true>(a.xw + (size_t)b * G, H, uu, r.xv[qq]);
        load_gq<false, true>(a.hw + (size_t)b * G, H, uu, r.hv[qq]);
#pragma unroll
        for (int g = 0; g < 4; ++g)
            if (SAVED) r.gv[SAVED ? qq : 0][SAVED ? g : 0] = __builtin_nontemporal_load(reinterpret_cast<const vfloat4*>(a.gates + og0 + g * H));
        r.cn[qq] = __builtin_nontemporal_load(reinterpret_cast<const vfloat4*>(a.c_new + o));
        r.cp[qq] = *reinterpret_cast<const vfloat4*>(a.c_prev + o);
        r.dci[qq] = a.dc_in ? *reinterpret_cast<const vfloat4*>(a.dc_in + o) : zero4;
        r.dh[qq] = a.dh_a ? *reinterpret_cast<const vfloat4*>(a.dh_a + o) : zero4;
    }
}
// ACC: instead of storing the gate adjoint `da` for a later column-reduction pass over (S*B, 4H), the workgroup adds
// da, da*xhat_x, da*xhat_h of its row to per-column accumulators in LDS (`acc`, 3 x 4H floats, every column owned by
// exactly one thread: no synchronisation) -- see lstm_cell_bwd4_rows_kernel.
template <int NQ, bool SAVED, bool ACC>
__device__ __forceinline__ void cell_bwd4_compute(const CellBwdArgs& a, int b, const CellBwdRow<NQ, SAVED>& r, float* red,
                                                  float* acc) {
    const int H = a.H, G = 4 * H;
    const float mx = r.mx, rx = r.rx, mh = r.mh, rh = r.rh;
    const vfloat4 zero4 = {0.f, 0.f, 0.f, 0.f};
    vfloat4 da[NQ][4];   // (the normalised operands xhat are recomputed from the row's x / h where needed: registers)
    float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int qq = 0; qq < NQ; ++qq) {
        const int u0 = ((int)threadIdx.x + qq * 256) * 4;
        if (u0 >= H) {
#pragma unroll
            for (int g = 0; g < 4; ++g) da[qq][g] = zero4;
            continue;
        }
        const size_t o = (size_t)b * H + u0;
        const size_t og0 = (size_t)b * G + u0;
        vfloat4 gxv[4], ghv[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            gxv[g] = *reinterpret_cast<const vfloat4*>(a.gamma + g * H + u0);
            ghv[g] = *reinterpret_cast<const vfloat4*>(a.gamma + G + g * H + u0);
        }
        vfloat4 dh = r.dh[qq];
        // split-K partials of dh (written by the product just before this launch: cache hits), four in flight, slice order
        for (int z = 0; a.dh_b && z < a.nsplit; z += 4) {
            vfloat4 p[4];
#pragma unroll
            for (int zz = 0; zz < 4; ++zz)
                p[zz] = (z + zz < a.nsplit) ? *reinterpret_cast<const vfloat4*>(a.dh_b + (size_t)(z + zz) * a.part_stride + o) : zero4;
#pragma unroll
            for (int zz = 0; zz < 4; ++zz)
                if (z + zz < a.nsplit) dh += p[zz];
        }
        vfloat4 gv[4];
        if (SAVED) {
#pragma unroll
            for (int g = 0; g < 4; ++g) gv[g] = r.gv[SAVED ? qq : 0][SAVED ? g : 0];
        } else {   // recompute (cell_recompute_gates): the forward's own expression
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const vfloat4 bxv = *reinterpret_cast<const vfloat4*>(a.beta + g * H + u0);
                const vfloat4 bhv = *reinterpret_cast<const vfloat4*>(a.beta + G + g * H + u0);
                const vfloat4 bv = *reinterpret_cast<const vfloat4*>(a.bias + g * H + u0);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float pre = gate_pre(r.xv[qq][g][i], mx, rx, gxv[g][i], bxv[i], r.hv[qq][g][i], mh, rh, ghv[g][i],
                                               bhv[i], bv[i]);
                    gv[g][i] = g < 3 ? gate_sigmoid(pre) : tanhf(pre);
                }
            }
        }
        vfloat4 dcp;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float ig = gv[0][i], fg = gv[1][i], og = gv[2][i], ug = gv[3][i];
            const float tc = tanhf(r.cn[qq][i]);
            const float dc = r.dci[qq][i] + dh[i] * og * (1.f - tc * tc);
            da[qq][0][i] = dc * ug * ig * (1.f - ig);
            da[qq][1][i] = dc * r.cp[qq][i] * fg * (1.f - fg);
            da[qq][2][i] = dh[i] * tc * og * (1.f - og);
            da[qq][3][i] = dc * ig * (1.f - ug * ug);
            dcp[i] = dc * fg;
        }
        *reinterpret_cast<vfloat4*>(a.dc_prev + o) = dcp;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            vfloat4 xh, hh;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                xh[i] = (r.xv[qq][g][i] - mx) * rx;
                hh[i] = (r.hv[qq][g][i] - mh) * rh;
                const float dyx = da[qq][g][i] * gxv[g][i], dyh = da[qq][g][i] * ghv[g][i];
                s[0] += dyx; s[1] += dyx * xh[i];
                s[2] += dyh; s[3] += dyh * hh[i];
            }
            if (ACC) {
                vfloat4* a0 = reinterpret_cast<vfloat4*>(acc + g * H + u0);
                vfloat4* a1 = reinterpret_cast<vfloat4*>(acc + G + g * H + u0);
                vfloat4* a2 = reinterpret_cast<vfloat4*>(acc + 2 * G + g * H + u0);
                *a0 += da[qq][g];
                *a1 += da[qq][g] * xh;
                *a2 += da[qq][g] * hh;
            } else {
                __builtin_nontemporal_store(da[qq][g], reinterpret_cast<vfloat4*>(a.dgate + og0 + g * H));
            }
        }
    }
    block_allsum<4>(s, red);
    const float inv_g = 1.f / (float)G;
    const float a0 = s[0] * inv_g, a1 = s[1] * inv_g, a2 = s[2] * inv_g, a3 = s[3] * inv_g;
#pragma unroll
    for (int qq = 0; qq < NQ; ++qq) {
        const int u0 = ((int)threadIdx.x + qq * 256) * 4;
        if (u0 >= H) continue;
        vfloat4 ox[4], oh[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const vfloat4 gxv = *reinterpret_cast<const vfloat4*>(a.gamma + g * H + u0);
            const vfloat4 ghv = *reinterpret_cast<const vfloat4*>(a.gamma + G + g * H + u0);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float dyx = da[qq][g][i] * gxv[i], dyh = da[qq][g][i] * ghv[i];
                ox[g][i] = rx * (dyx - a0 - (r.xv[qq][g][i] - mx) * rx * a1);
                oh[g][i] = rh * (dyh - a2 - (r.hv[qq][g][i] - mh) * rh * a3);
            }
        }
        store_gq<false, true>(a.dxw + (size_t)b * G, H, u0, ox);
        store_gq<false, false>(a.dhw + (size_t)b * G, H, u0, oh);   // read next by this step's dh product: keep it cached
    }
}

template <int NQ, bool SAVED>
__global__ __launch_bounds__(256) void lstm_cell_bwd4_kernel(const CellBwdArgs a) {
    __shared__ float red[16];
    CellBwdRow<NQ, SAVED> r;
    cell_bwd4_load<NQ, SAVED>(a, blockIdx.x, r);
    cell_bwd4_compute<NQ, SAVED, false>(a, blockIdx.x, r, red, nullptr);
}

// Workgroup w walks the batch rows [w*B/nwg, (w+1)*B/nwg) one after the other and keeps the three per-column sums the
// parameter gradients need (sum da -> dbias, dbeta ; sum da*xhat_x -> dgamma_x ; sum da*xhat_h -> dgamma_h) in LDS,
// carried from step to step through `colacc` (nwg, 3, 4H) -- read at the start of the launch (`acc_init` = 0), written
// at its end; lstm_colfinal_kernel adds the nwg rows once per layer.  Against storing `da` per step and reducing
// (S*B, 4H) x 3 operands afterwards this removes S*B*4H floats of stores per step and a 3 x S*B*4H pass per layer
// (C4: 64 MB per step and 26 GB = 4.05 ms per layer).  Fixed summation order (rows ascending inside a workgroup, steps
// descending, workgroups ascending): deterministic, no atomics.  Measured at C4 (tests/tools/r02_lstm_cellrows_probe.py,
// backward, ms): one row per workgroup + reduction pass 144.3; 512 workgroups x 8 rows 140.9; 768 (5-6 rows: uneven)
// 144.6; 1024 x 4 rows (1.33 rounds of the chip) 142.6; requesting row b+1 before computing row b needs > 256 registers
// and spills (147.3).  At B = 1024..2048 the row walk loses 2-3 % (too few rows per workgroup to pay for the
// accumulator round trip), so it starts at 8 rows per workgroup; B = 8192: H = 1024 36.2 -> 35.5 ms (S = 16), H = 512
// 43.1 -> 43.5 (S = 32, L = 2), so it starts at H = 768.
__global__ __launch_bounds__(256) void lstm_cell_bwd4_rows_kernel(const CellBwdArgs a, float* __restrict__ colacc,
                                                                  int acc_init, int B) {
    __shared__ float red[16];
    extern __shared__ __attribute__((aligned(16))) float acc[];   // [3][4H]
    const int G = 4 * a.H;
    float* mine = colacc + (size_t)blockIdx.x * 3 * G;
    const vfloat4 zero4 = {0.f, 0.f, 0.f, 0.f};
    const int r0 = (int)((long)blockIdx.x * B / gridDim.x), r1 = (int)((long)(blockIdx.x + 1) * B / gridDim.x);
    for (int i = threadIdx.x * 4; i < 3 * G; i += 1024)
        *reinterpret_cast<vfloat4*>(acc + i) = acc_init ? zero4 : *reinterpret_cast<const vfloat4*>(mine + i);
    __syncthreads();   // (the owner of a column in the row function is another thread than here unless H % 256 == 0)
    for (int b = r0; b < r1; ++b) {
        CellBwdRow<1, false> r;   // (this path always recomputes the gates: cell_rows_shape)
        cell_bwd4_load<1, false>(a, b, r);
        cell_bwd4_compute<1, false, true>(a, b, r, red, acc);
    }
    __syncthreads();
    for (int i = threadIdx.x * 4; i < 3 * G; i += 1024)
        *reinterpret_cast<vfloat4*>(mine + i) = *reinterpret_cast<const vfloat4*>(acc + i);
}

// The row-walking backward cell for GATE-INTERLEAVED pre-activations (lstm_perm_shape).  Thread t owns the hidden units
// t, t + 256, t + 512, t + 768 (those below H): a unit's four gates are ONE float4 of xw / hw / dxw / dhw and consecutive
// lanes hold consecutive units, so every access instruction of a wave is one contiguous span -- 1 KB for the (rows, 4H)
// tensors, 256 B for the (rows, H) ones.  (The unit-QUAD mapping of the standard layout would make a lane's data 64
// contiguous bytes moved as four 16-byte pieces at a 64-byte lane stride: harmless for loads, but the streaming stores of
// dxw / dhw then reach memory as quarter lines -- 90 -> 127 us per step at C4; redistributing through LDS instead cost
// more than it saved: 176 us.)  Same arithmetic per element as cell_bwd4_compute; the four row sums and the per-column
// accumulators are summed in another order (fp32 rounding).  `pp`: gamma_x, gamma_h, beta_x, beta_h, bias of the layer in
// the interleaved column order ([5][4H], perm_params_kernel); the column accumulators are interleaved too
// (lstm_colfinal_kernel un-permutes).
constexpr int kPermUnits = 4;   // H <= 1024
struct PermRow { vfloat4 xv[kPermUnits], hv[kPermUnits]; float cn[kPermUnits], cp[kPermUnits], dci[kPermUnits], dh[kPermUnits]; float mx, rx, mh, rh; };
__device__ __forceinline__ void cell_bwd_perm_load(const CellBwdArgs& a, int b, PermRow& r) {
    const int H = a.H, G = 4 * H;
    const float* st = a.stats + (size_t)b * 4;
    r.mx = st[0]; r.rx = st[1]; r.mh = st[2]; r.rh = st[3];
#pragma unroll
    for (int k = 0; k < kPermUnits; ++k) {
        const int u = (int)threadIdx.x + 256 * k;
        const int uu = u < H ? u : 0;   // idle units re-read unit 0 (no divergent branch around a load), results unused
        const size_t o = (size_t)b * H + uu;
        r.xv[k] = __builtin_nontemporal_load(reinterpret_cast<const vfloat4*>(a.xw + (size_t)b * G + 4 * uu));
        r.hv[k] = __builtin_nontemporal_load(reinterpret_cast<const vfloat4*>(a.hw + (size_t)b * G + 4 * uu));
        r.cn[k] = __builtin_nontemporal_load(a.c_new + o);
        r.cp[k] = a.c_prev[o];
        r.dci[k] = a.dc_in ? a.dc_in[o] : 0.f;
        r.dh[k] = a.dh_a ? a.dh_a[o] : 0.f;
    }
}
__device__ __forceinline__ void cell_bwd_perm_compute(const CellBwdArgs& a, int b, const PermRow& r, float* red, float* acc,
                                                      const float* __restrict__ pp) {
    const int H = a.H, G = 4 * H;
    const float mx = r.mx, rx = r.rx, mh = r.mh, rh = r.rh;
    vfloat4 da[kPermUnits];
    float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < kPermUnits; ++k) {
        const int u = (int)threadIdx.x + 256 * k;
        if (u >= H) {
            da[k] = vfloat4{0.f, 0.f, 0.f, 0.f};
            continue;
        }
        const size_t o = (size_t)b * H + u;
        const vfloat4 gxv = *reinterpret_cast<const vfloat4*>(pp + 4 * u);
        const vfloat4 ghv = *reinterpret_cast<const vfloat4*>(pp + G + 4 * u);
        const vfloat4 bxv = *reinterpret_cast<const vfloat4*>(pp + 2 * G + 4 * u);
        const vfloat4 bhv = *reinterpret_cast<const vfloat4*>(pp + 3 * G + 4 * u);
        const vfloat4 bv = *reinterpret_cast<const vfloat4*>(pp + 4 * G + 4 * u);
        float dh = r.dh[k];
        // split-K partials of dh (written by the product just before this launch: cache hits), four in flight, slice order
        for (int z = 0; a.dh_b && z < a.nsplit; z += 4) {
            float p[4];
#pragma unroll
            for (int zz = 0; zz < 4; ++zz) p[zz] = (z + zz < a.nsplit) ? a.dh_b[(size_t)(z + zz) * a.part_stride + o] : 0.f;
#pragma unroll
            for (int zz = 0; zz < 4; ++zz)
                if (z + zz < a.nsplit) dh += p[zz];
        }
        float gv[4];   // the forward's own expression (the gates are not saved at these shapes)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float pre = gate_pre(r.xv[k][g], mx, rx, gxv[g], bxv[g], r.hv[k][g], mh, rh, ghv[g], bhv[g], bv[g]);
            gv[g] = g < 3 ? gate_sigmoid(pre) : tanhf(pre);
        }
        const float ig = gv[0], fg = gv[1], og = gv[2], ug = gv[3];
        const float tc = tanhf(r.cn[k]);
        const float dc = r.dci[k] + dh * og * (1.f - tc * tc);
        da[k] = vfloat4{dc * ug * ig * (1.f - ig), dc * r.cp[k] * fg * (1.f - fg), dh * tc * og * (1.f - og), dc * ig * (1.f - ug * ug)};
        a.dc_prev[o] = dc * fg;
        vfloat4 xh, hh;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            xh[g] = (r.xv[k][g] - mx) * rx;
            hh[g] = (r.hv[k][g] - mh) * rh;
            const float dyx = da[k][g] * gxv[g], dyh = da[k][g] * ghv[g];
            s[0] += dyx; s[1] += dyx * xh[g];
            s[2] += dyh; s[3] += dyh * hh[g];
        }
        vfloat4* a0 = reinterpret_cast<vfloat4*>(acc + 4 * u);
        vfloat4* a1 = reinterpret_cast<vfloat4*>(acc + G + 4 * u);
        vfloat4* a2 = reinterpret_cast<vfloat4*>(acc + 2 * G + 4 * u);
        *a0 += da[k];
        *a1 += da[k] * xh;
        *a2 += da[k] * hh;
    }
    block_allsum<4>(s, red);
    const float inv_g = 1.f / (float)G;
    const float a0 = s[0] * inv_g, a1 = s[1] * inv_g, a2 = s[2] * inv_g, a3 = s[3] * inv_g;
#pragma unroll
    for (int k = 0; k < kPermUnits; ++k) {
        const int u = (int)threadIdx.x + 256 * k;
        if (u >= H) continue;
        const vfloat4 gxv = *reinterpret_cast<const vfloat4*>(pp + 4 * u);
        const vfloat4 ghv = *reinterpret_cast<const vfloat4*>(pp + G + 4 * u);
        vfloat4 ox, oh;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float dyx = da[k][g] * gxv[g], dyh = da[k][g] * ghv[g];
            ox[g] = rx * (dyx - a0 - (r.xv[k][g] - mx) * rx * a1);
            oh[g] = rh * (dyh - a2 - (r.hv[k][g] - mh) * rh * a3);
        }
        __builtin_nontemporal_store(ox, reinterpret_cast<vfloat4*>(a.dxw + (size_t)b * G + 4 * u));
        *reinterpret_cast<vfloat4*>(a.dhw + (size_t)b * G + 4 * u) = oh;   // read next by this step's dh product: keep it cached
    }
}
__global__ __launch_bounds__(256) void lstm_cell_bwd_perm_rows_kernel(const CellBwdArgs a, const float* __restrict__ pp,
                                                                      float* __restrict__ colacc, int acc_init, int B) {
    __shared__ float red[16];
    extern __shared__ __attribute__((aligned(16))) float acc[];   // [3][4H], interleaved columns
    const int G = 4 * a.H;
    float* mine = colacc + (size_t)blockIdx.x * 3 * G;
    const vfloat4 zero4 = {0.f, 0.f, 0.f, 0.f};
    const int r0 = (int)((long)blockIdx.x * B / gridDim.x), r1 = (int)((long)(blockIdx.x + 1) * B / gridDim.x);
    for (int i = threadIdx.x * 4; i < 3 * G; i += 1024)
        *reinterpret_cast<vfloat4*>(acc + i) = acc_init ? zero4 : *reinterpret_cast<const vfloat4*>(mine + i);
    __syncthreads();
    for (int b = r0; b < r1; ++b) {
        PermRow r;
        cell_bwd_perm_load(a, b, r);
        cell_bwd_perm_compute(a, b, r, red, acc, pp);
    }
    __syncthreads();
    for (int i = threadIdx.x * 4; i < 3 * G; i += 1024)
        *reinterpret_cast<vfloat4*>(mine + i) = *reinterpret_cast<const vfloat4*>(acc + i);
}
// pp[k][4u + g] = the k-th parameter vector (gamma_x, gamma_h, beta_x, beta_h, bias) at its standard position g*H + u
__global__ __launch_bounds__(256) void perm_params_kernel(const float* __restrict__ gamma, const float* __restrict__ beta,
                                                          const float* __restrict__ bias, float* __restrict__ pp, int H) {
    const int q = blockIdx.x * 256 + threadIdx.x, G = 4 * H;
    if (q >= G) return;
    const int u = q >> 2, g = q & 3, col = g * H + u;
    pp[q] = gamma[col];
    pp[G + q] = gamma[G + col];
    pp[2 * G + q] = beta[col];
    pp[3 * G + q] = beta[G + col];
    pp[4 * G + q] = bias[col];
}

// ------------------------------------------------------------------------------------------------ column reductions
// dbias[col] = sum_rows dgate ; dbeta (both halves) = the same sum ; dgamma_x[col] = sum dgate * xhat_x ; dgamma_h
// likewise.  Two deterministic stages: grid (column tiles of 64, row chunks) -> partials[chunk][3][G], then one
// pass over the chunks in a fixed order.  (A single stage with one workgroup per 64 columns walked 26 GB through
// 64 workgroups: 61 ms at the C4 shape.)
constexpr int kColChunks = 128;
__global__ __launch_bounds__(256) void lstm_colreduce_kernel(const float* __restrict__ dgate,
                                                             const float* __restrict__ xw,
                                                             const float* __restrict__ hw,
                                                             const float* __restrict__ stats, long rows, int G,
                                                             float* __restrict__ partials) {
    __shared__ float red[3][4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int col = blockIdx.x * 64 + lane;
    const long per = (rows + gridDim.y - 1) / gridDim.y;
    const long r0 = (long)blockIdx.y * per;
    const long r1 = r0 + per < rows ? r0 + per : rows;
    float sb = 0.f, sx = 0.f, sh = 0.f;
    if (col < G) {
        for (long row = r0 + w; row < r1; row += 4) {
            const float* st = stats + row * 4;
            const float d = dgate[row * G + col];
            sb += d;
            sx = fmaf(d, (xw[row * G + col] - st[0]) * st[1], sx);
            sh = fmaf(d, (hw[row * G + col] - st[2]) * st[3], sh);
        }
    }
    red[0][w][lane] = sb; red[1][w][lane] = sx; red[2][w][lane] = sh;
    __syncthreads();
    if (w < 3 && col < G)
        partials[((size_t)blockIdx.y * 3 + w) * G + col] =
            (red[w][0][lane] + red[w][1][lane]) + (red[w][2][lane] + red[w][3][lane]);
}
__global__ __launch_bounds__(256) void lstm_colfinal_kernel(const float* __restrict__ partials, int chunks, int G,
                                                            float* __restrict__ dbias, float* __restrict__ dgamma,
                                                            float* __restrict__ dbeta, int perm /* partial columns are gate-interleaved */) {
    const int pc = blockIdx.x * 256 + threadIdx.x;   // position in the partials
    if (pc >= G) return;
    const int col = perm ? (pc & 3) * (G / 4) + (pc >> 2) : pc;
    float s[3] = {0.f, 0.f, 0.f};
#pragma unroll 8   // 24 independent loads in flight per thread (512 chunks after the row-walking cell: 212 -> ~30 us)
    for (int c = 0; c < chunks; ++c)
#pragma unroll
        for (int k = 0; k < 3; ++k) s[k] += partials[((size_t)c * 3 + k) * G + pc];
    dbias[col] = s[0];
    dbeta[col] = s[0];
    dbeta[G + col] = s[0];
    dgamma[col] = s[1];
    dgamma[G + col] = s[2];
}

// out (cols, rows) = in (rows, cols)^T, 32x32 tiles through LDS.  Used once per layer and backward call to turn the
// two "NT" products of the backward pass (dHW @ Wh^T per step, dXW @ Wx^T per layer) into "NN" products: the NT form
// needs a register transpose of BOTH operands when staging and ran at 84-91 TFLOP/s (dh) / 112 (dx) against 117 / 122
// for NN at the same sizes; transposing a 16 MB weight once costs ~10 us.
__global__ __launch_bounds__(256) void transpose_kernel(const float* __restrict__ in, float* __restrict__ out, int rows,
                                                        int cols) {
    __shared__ float tile[32][33];
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
#pragma unroll
    for (int k = 0; k < 32; k += 8) {
        const int r = r0 + ty + k, c = c0 + tx;
        tile[ty + k][tx] = (r < rows && c < cols) ? in[(size_t)r * cols + c] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 32; k += 8) {
        const int c = c0 + ty + k, r = r0 + tx;
        if (c < cols && r < rows) out[(size_t)c * rows + r] = tile[tx][ty + k];
    }
}
inline void launch_transpose(const float* in, float* out, int rows, int cols, hipStream_t st) {
    hipLaunchKernelGGL(transpose_kernel, dim3((cols + 31) / 32, (rows + 31) / 32), dim3(256), 0, st, in, out, rows, cols);
}

// ------------------------------------------------------------------------------------------------ dropout
__device__ __forceinline__ uint32_t mix_hash(uint64_t seed, uint64_t idx) {
    uint64_t z = seed + idx * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((z ^ (z >> 31)) >> 32);
}
// out[i] = in[i] * keep(i) / (1-p); keep(i) = hash > p * 2^32 (the reference's rule, lstm_kernel.h:88-94)
__global__ __launch_bounds__(256) void dropout_kernel(const float* in, float* out, long n,  // in == out allowed
                                                      uint64_t seed, uint32_t threshold, float scale) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256)
        out[i] = (mix_hash(seed, (uint64_t)i) > threshold) ? in[i] * scale : 0.f;
}

// out[i] = sum_z parts[z*n + i]  (fixed order)
__global__ __launch_bounds__(256) void sum_parts_kernel(const float* __restrict__ parts, int nparts, long n,
                                                        float* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = parts[i];
    for (int z = 1; z < nparts; ++z) s += parts[(size_t)z * n + i];
    out[i] = s;
}

// out[r, 4u + g] = in[r, g*H + u]: the gate-interleaved copy of a (rows, 4H) weight (lstm_perm_shape).  One thread per
// output quad = the four gates of one unit: four 4-byte gathers, one 16-byte store.
__global__ __launch_bounds__(256) void perm_cols_kernel(const float* __restrict__ in, float* __restrict__ out, long rows, int H) {
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    if (q >= rows * H) return;
    const long r = q / H;
    const int u = (int)(q - r * H);
    const float* p = in + r * 4 * H + u;
    *reinterpret_cast<vfloat4*>(out + r * 4 * H + 4 * u) = vfloat4{p[0], p[H], p[2 * (long)H], p[3 * (long)H]};
}
inline void launch_perm_cols(const float* in, float* out, long rows, int H, hipStream_t st) {
    hipLaunchKernelGGL(perm_cols_kernel, dim3((unsigned)((rows * H + 255) / 256)), dim3(256), 0, st, in, out, rows, H);
}
// out[r, g*H + u] = sum_z parts[z*n + r*4H + 4u + g]  (fixed order): the split-K summation of a weight gradient computed in
// the gate-interleaved layout, written back in the standard one.  One thread per interleaved quad.
__global__ __launch_bounds__(256) void sum_parts_unperm_kernel(const float* __restrict__ parts, int nparts, long n, long rows,
                                                               int H, float* __restrict__ out) {
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    if (q >= rows * H) return;
    const long r = q / H;
    const int u = (int)(q - r * H);
    vfloat4 s = *reinterpret_cast<const vfloat4*>(parts + r * 4 * H + 4 * u);
    for (int z = 1; z < nparts; ++z) s += *reinterpret_cast<const vfloat4*>(parts + (size_t)z * n + r * 4 * H + 4 * u);
    float* o = out + r * 4 * H + u;
    o[0] = s.x; o[H] = s.y; o[2 * (long)H] = s.z; o[3 * (long)H] = s.w;
}

template <class... Args>
inline void launch_cell_fwd_scalar(int H, int B, hipStream_t st, Args... a) {
    const int jpt = (H + 255) / 256;
    if (jpt <= 1) hipLaunchKernelGGL(lstm_cell_fwd_kernel<1>, dim3(B), dim3(256), 0, st, a..., H);
    else if (jpt <= 2) hipLaunchKernelGGL(lstm_cell_fwd_kernel<2>, dim3(B), dim3(256), 0, st, a..., H);
    else if (jpt <= 4) hipLaunchKernelGGL(lstm_cell_fwd_kernel<4>, dim3(B), dim3(256), 0, st, a..., H);
    else hipLaunchKernelGGL(lstm_cell_fwd_kernel<8>, dim3(B), dim3(256), 0, st, a..., H);
}
inline bool cell_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
// The persistent small-batch kernels exchange {value, tag} pairs as ONE 8-byte atomic word (lstm_persist.hpp: xchg_put /
// xchg_get); every workspace region starts a multiple of 16 bytes behind ws, so the words are whole only if ws itself lies
// on an 8-byte boundary.  On a workspace 4 bytes off, value and tag of a word arrive separately and a reader can pair a
// fresh tag with a stale value: the step kernels take such a call.
inline bool xchg_al8(const void* ws) { return (reinterpret_cast<uintptr_t>(ws) & 7) == 0; }

inline void launch_cell_fwd(int H, int B, hipStream_t st, const float* xw, const float* hw, int nsplit, long part_stride,
                            float* hw_out, const float* bias, const float* gamma, const float* beta, const float* c_prev,
                            float* gates, float* c_out, float* h_out, float* stats, bool perm = false) {
    const int jpt = (H + 255) / 256;
    if (perm) {   // gate-interleaved pre-activations (lstm_perm_shape: H % 64 == 0, H <= 1024, workspace tensors 16-byte aligned)
        hipLaunchKernelGGL((lstm_cell_fwd4_kernel<1, true>), dim3(B), dim3(256), 0, st, xw, hw, nsplit, part_stride, hw_out, bias,
                           gamma, beta, c_prev, gates, c_out, h_out, stats, H);
        return;
    }
    if (g_cell_vec4 && jpt >= g_cell_vec4 && (H % 4) == 0 && (part_stride % 4) == 0 && cell_al16(xw) && cell_al16(hw) &&
        cell_al16(hw_out) && cell_al16(bias) && cell_al16(gamma) && cell_al16(beta) && cell_al16(c_prev) &&
        cell_al16(gates) && cell_al16(c_out) && cell_al16(h_out)) {
        if (H <= 1024)
            hipLaunchKernelGGL(lstm_cell_fwd4_kernel<1>, dim3(B), dim3(256), 0, st, xw, hw, nsplit, part_stride, hw_out, bias,
                               gamma, beta, c_prev, gates, c_out, h_out, stats, H);
        else
            hipLaunchKernelGGL(lstm_cell_fwd4_kernel<2>, dim3(B), dim3(256), 0, st, xw, hw, nsplit, part_stride, hw_out, bias,
                               gamma, beta, c_prev, gates, c_out, h_out, stats, H);
        return;
    }
    launch_cell_fwd_scalar(H, B, st, xw, hw, nsplit, part_stride, hw_out, bias, gamma, beta, c_prev, gates, c_out, h_out,
                           stats);
}

inline void launch_cell_bwd(int B, hipStream_t st, const CellBwdArgs& a) {
    const int H = a.H;
    const int jpt = (H + 255) / 256;
    if (g_cell_vec4 && jpt >= g_cell_vec4 && (H % 4) == 0 && H <= 2048 && (a.part_stride % 4) == 0 && cell_al16(a.dh_a) &&
        cell_al16(a.dh_b) && cell_al16(a.dc_in) && cell_al16(a.gates) && cell_al16(a.c_new) && cell_al16(a.c_prev) &&
        cell_al16(a.xw) && cell_al16(a.hw) && cell_al16(a.gamma) && cell_al16(a.beta) && cell_al16(a.bias) &&
        cell_al16(a.dgate) && cell_al16(a.dxw) && cell_al16(a.dhw) && cell_al16(a.dc_prev)) {
        if (H <= 1024 && a.gates) hipLaunchKernelGGL((lstm_cell_bwd4_kernel<1, true>), dim3(B), dim3(256), 0, st, a);
        else if (H <= 1024) hipLaunchKernelGGL((lstm_cell_bwd4_kernel<1, false>), dim3(B), dim3(256), 0, st, a);
        else if (a.gates) hipLaunchKernelGGL((lstm_cell_bwd4_kernel<2, true>), dim3(B), dim3(256), 0, st, a);
        else hipLaunchKernelGGL((lstm_cell_bwd4_kernel<2, false>), dim3(B), dim3(256), 0, st, a);
        return;
    }
#define HPC_RLL_CELL_BWD(J)                                                                                               \
    hipLaunchKernelGGL(lstm_cell_bwd_kernel<J>, dim3(B), dim3(256), 0, st, a.dh_a, a.dh_b, a.nsplit, a.part_stride, a.dc_in, \
                       a.gates, a.c_new, a.c_prev, a.xw, a.hw, a.stats, a.gamma, a.beta, a.bias, a.dgate, a.dxw, a.dhw,      \
                       a.dc_prev, H)
    if (jpt <= 1) HPC_RLL_CELL_BWD(1);
    else if (jpt <= 2) HPC_RLL_CELL_BWD(2);
    else if (jpt <= 4) HPC_RLL_CELL_BWD(4);
    else HPC_RLL_CELL_BWD(8);
#undef HPC_RLL_CELL_BWD
}

// Large-batch backward cells with the parameter-gradient column sums folded in (lstm_cell_bwd4_rows_kernel).
constexpr int kCellRowsMaxWgs = 1024;
inline bool cell_rows_shape(int B, int H) {
    return cell_recompute_gates(B, H) && H % 4 == 0 && H >= 768 && H <= 1024 && g_cell_rows_wgs > 0 && B >= 8 * g_cell_rows_wgs;
}
inline void launch_cell_bwd_rows(int B, int nwg, hipStream_t st, const CellBwdArgs& a, float* colacc, int acc_init,
                                 const float* pp = nullptr /* interleaved layout: its parameter table */) {
    const size_t lds = (size_t)3 * 4 * a.H * sizeof(float);
    if (pp) hipLaunchKernelGGL(lstm_cell_bwd_perm_rows_kernel, dim3(nwg), dim3(256), lds, st, a, pp, colacc, acc_init, B);
    else hipLaunchKernelGGL(lstm_cell_bwd4_rows_kernel, dim3(nwg), dim3(256), lds, st, a, colacc, acc_init, B);
}

}  // namespace
}  // namespace hpc_rll
#include "lstm_persist.hpp"
#include "lstm_wave.hpp"
#include "lstm_block.hpp"
#include "lstm_mid.hpp"
namespace hpc_rll {
namespace {

// workspace carving --------------------------------------------------------------------------------------------
struct LayerWs { float *xw, *hw, *gates, *c, *hseq, *stats, *xin_next; };
struct Ws {
    LayerWs layer[16];
    float *pstash;   // bias (L,4H) then ln_beta (L,2,4H), parked by the forward for a gate-recomputing backward
    float *dgate, *dxw, *dhw, *dh, *dc, *dseq_a, *dseq_b, *colpart, *hw_part, *xchg, *wpart, *dwave, *whT, *wxT;
    float *whP, *wxP, *blk_part, *blk_flags, *pperm;   // gate-interleaved weight copies, row-block exchange, interleaved
                                                       // parameter table of the layer (lstm_perm_shape only)
    float *mid;      // mid-batch persistent forward: flags + LayerNorm partials (lstm_mid_shape only)
    size_t total;
};
inline Ws carve(float* base, int S, int B, int I, int H, int L, bool dropout) {
    Ws w;
    size_t off = 0;
    auto take = [&](size_t n) { float* p = base ? base + off : nullptr; off += (n + 3) / 4 * 4; return p; };
    const size_t SB = (size_t)S * B, G = 4 * (size_t)H;
    for (int l = 0; l < L; ++l) {
        w.layer[l].xw = take(SB * G);
        w.layer[l].hw = take(SB * G);
        w.layer[l].gates = cell_recompute_gates(B, H) ? nullptr : take(SB * G);   // not saved at large batch
        w.layer[l].c = take(SB * H);
        w.layer[l].hseq = take(SB * H);
        w.layer[l].stats = take(SB * 4);
        w.layer[l].xin_next = (dropout && l < L - 1) ? take(SB * H) : w.layer[l].hseq;
    }
    w.pstash = take(cell_recompute_gates(B, H) ? (size_t)L * 3 * G : 0);
    w.dgate = take(SB * G);
    w.dxw = take(SB * G);
    w.dhw = take(SB * G);
    // split-K partials of dh_prev = dHW @ Wh^T (either tiling of that product)
    w.dh = take((size_t)std::max(gemm_splitk(B, H, (int)G), gemm_splitk_big(B, H, (int)G)) * B * H);
    w.hw_part = take((size_t)gemm_splitk(B, (int)G, H) * B * G);   // split-K partials of h @ Wh
    w.dc = take((size_t)B * H);
    const size_t widest = SB * (size_t)(I > H ? I : H);
    w.dseq_a = take(widest);
    w.dseq_b = take(widest);
    w.colpart = take((size_t)(kCellRowsMaxWgs > kColChunks ? kCellRowsMaxWgs : kColChunks) * 3 * G);
    w.whT = take((size_t)H * G);                          // Wh^T of the layer being processed (backward)
    w.wxT = take((size_t)(I > H ? I : H) * G);            // Wx^T of that layer
    const bool perm = lstm_perm_shape(B, H);
    w.whP = take(perm ? (size_t)H * G : 0);
    w.wxP = take(perm ? (size_t)(I > H ? I : H) * G : 0);
    w.blk_part = take(perm ? block_part_floats(B, H) : 0);
    w.blk_flags = take(perm ? block_flag_words(B) : 0);
    w.pperm = take(perm ? 5 * G : 0);
    // (forward and backward of the mid-batch kernels share the region: never live at the same time)
    w.mid = take(std::max<size_t>(mid_ws_floats(S, B, H), mid_bwd_ws_floats(S, B, H)));
    {   // persistent small-batch paths: {value, tag} exchange words (per-layer kernels / layer wavefront)
        size_t words = xchg_layout(B, H).total_words;
        WaveCfg wc{};
        if (wave_shape_ok(S, B, H, L, 256, &wc, true) && wc.hx_words + wc.sx_words > words) words = wc.hx_words + wc.sx_words;
        const bool wb = wave_bwd_shape_ok(S, B, H, L, 256, &wc, true);
        if (wb && 2 * wc.hx_words + wc.sx_words > words) words = 2 * wc.hx_words + wc.sx_words;
        w.xchg = take(2 * words);
        w.dwave = take(wb ? (size_t)L * 3 * SB * G : 0);   // per-layer dgate/dXW/dHW (all layers are live at once)
    }
    {   // split-K partials of the weight gradients (dWh: 1 + sk parts, dWx: sk parts), largest layer
        size_t need = 0;
        const int skh = S > 1 ? gemm_splitk_big(H, (int)G, (int)((S - 1) * (size_t)B)) : 1;
        if (skh > 1) need = (size_t)(skh + 1) * H * G;
        for (int l = 0; l < L; ++l) {
            const int in_l = l == 0 ? I : H;
            const int skx = gemm_splitk_big(in_l, (int)G, (int)SB);
            if (skx > 1 && (size_t)skx * in_l * G > need) need = (size_t)skx * in_l * G;
            // under-filled x-branch / d(xin) products at small S*B (latency regime): partials + one summation pass
            const int skf = gemm_splitk((int)SB, (int)G, in_l), skd = gemm_splitk((int)SB, in_l, (int)G);
            if (skf > 1 && (size_t)skf * SB * G > need) need = (size_t)skf * SB * G;
            if (skd > 1 && (size_t)skd * SB * in_l > need) need = (size_t)skd * SB * in_l;
            // gate-interleaved layers compute dWx / dWh into this buffer even without split-K (un-permuted on the way out)
            if (perm && (size_t)in_l * G > need) need = (size_t)in_l * G;
            if (perm && (size_t)H * G > need) need = (size_t)H * G;
        }
        w.wpart = take(need);
    }
    w.total = off;
    return w;
}

inline int copy_async(float* dst, const float* src, size_t n, hipStream_t st) {
    return (int)hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, st);
}

// The recurrence paths, by the codes documented above hpc_rll_lstm_last_forward_path.
enum LstmPath { kStep = 0, kPersist = 1, kWave = 2, kStepPerm = 3, kBlock = 4, kMid = 5 };

std::atomic<int> g_lstm_last_path{-1};   // hpc_rll_lstm_last_forward_path (diagnostic)
std::atomic<int> g_lstm_last_bwd_path{-1};   // hpc_rll_lstm_last_backward_path
// ... and of THIS host thread (a binding that reads the path right after its own call must not see another
// thread's forward): hpc_rll_lstm_last_forward_path() answers with it once the calling thread has run a forward.
thread_local int t_lstm_last_path = -1;
void record_fwd_path(LstmPath p) { g_lstm_last_path.store(p, std::memory_order_relaxed); t_lstm_last_path = p; }
void record_bwd_path(LstmPath p) { g_lstm_last_bwd_path.store(p, std::memory_order_relaxed); }

// hpc_rll_lstm_forward_y leaves the workspace's own last-layer h-sequence slot UNWRITTEN (y is that sequence) on every path
// but the layer wavefront: a later hpc_rll_lstm_backward WITHOUT y on that workspace would read uninitialised memory
// (ADVICE r04).  Host-side record, keyed by the workspace address, of what the most recent forward on it was: no device
// work, no synchronisation.  (Addresses are recycled by the caller's allocator: every forward overwrites its entry.)
std::mutex g_ws_pair_mu;
std::map<const void*, bool> g_ws_y_external;
void ws_pair_record(const void* ws, bool y_external) {
    std::lock_guard<std::mutex> lk(g_ws_pair_mu);
    if (!y_external) { g_ws_y_external.erase(ws); return; }
    if (g_ws_y_external.size() >= 4096) g_ws_y_external.clear();   // bounded: forgetting only loses the diagnosis
    g_ws_y_external[ws] = true;
}
bool ws_pair_needs_y(const void* ws) {
    std::lock_guard<std::mutex> lk(g_ws_pair_mu);
    return g_ws_y_external.count(ws) != 0;
}

// one call ---------------------------------------------------------------------------------------------------------
// incoming gradients (each may be null: none through that output) and the gradients to write
struct BwdIo { const float *dy, *dhn, *dcn; float *dx, *dh0, *dc0, *dwx, *dwh, *dbias, *dln_gamma, *dln_beta; };
// Layer l of a call: its workspace buffers, its input sequence (x, or the -- dropped-out -- h sequence of the layer below)
// and its parameters.  Backward: gradients of its final states and of its output sequence (d_out: dy for the top layer,
// then d(input) of the layer above; each may be null), its slices of dh0 / dc0; perm: wx_l / wh_l are interleaved copies.
struct Layer : LayerWs {
    int l, in_l;
    const float *xin, *wx_l, *wh_l, *bias_l, *gamma_l, *beta_l, *h0_l, *c0_l;
    size_t wx_off;   // of wx_l in wx, and of this layer's dWx in dwx
    const float *dh, *dc; float *dh0_l, *dc0_l; bool perm; const float* d_out;   // backward only
};
struct LstmCall {   // sizes, stream, dropout constants (on, threshold of the mask's hash, 1 / (1 - p)), operands, workspace
    int S, B, I, H, L;
    size_t SB, G, BH;
    hipStream_t st; uint64_t seed;
    bool dropout; uint32_t drop_thr; float drop_scale;
    const float *x, *h0, *c0, *wx, *wh, *bias, *gamma, *beta;   // (backward: bias / beta are the forward's copies in pstash)
    float* ws;
    Ws w;
    float *y, *hn, *cn; BwdIo g;   // outputs: forward / backward
    Layer layer(int l) const {
        const size_t wx_off = l == 0 ? 0 : ((size_t)I + (size_t)(l - 1) * H) * G, o = (size_t)l * BH;
        return {w.layer[l], l, l == 0 ? I : H, l == 0 ? x : w.layer[l - 1].xin_next, wx + wx_off, wh + (size_t)l * H * G,
                bias + (size_t)l * G, gamma + (size_t)l * 2 * G, beta + (size_t)l * 2 * G, h0 + o, c0 + o, wx_off,
                g.dhn ? g.dhn + o : nullptr, g.dcn ? g.dcn + o : nullptr, g.dh0 ? g.dh0 + o : nullptr,
                g.dc0 ? g.dc0 + o : nullptr, false, nullptr};
    }
};
inline LstmCall make_call(float* ws, int S, int B, int I, int H, int L, float dropout_p, uint64_t seed, void* stream,
                          const float* x, const float* h0, const float* c0, const float* wx, const float* wh,
                          const float* bias, const float* gamma, const float* beta) {
    const bool drop = dropout_p > 0.f;
    return {S, B, I, H, L, (size_t)S * B, 4 * (size_t)H, (size_t)B * H, (hipStream_t)stream, seed, drop,
            drop ? (uint32_t)((double)dropout_p * 4294967295.0) : 0u, drop ? 1.f / (1.f - dropout_p) : 1.f,
            x, h0, c0, wx, wh, bias, gamma, beta, ws, carve(ws, S, B, I, H, L, drop), nullptr, nullptr, nullptr, {}};
}
inline bool all_al16(std::initializer_list<const void*> ps) {
    for (const void* p : ps) if (!cell_al16(p)) return false;
    return true;
}
// pieces every path uses -------------------------------------------------------------------------------------------
inline void sum_parts(const LstmCall& c, const float* parts, int nparts, size_t n, float* out) {
    hipLaunchKernelGGL(sum_parts_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c.st, parts, nparts, (long)n, out);
}
inline void row_stats(const LstmCall& c, const Layer& y) {
    hipLaunchKernelGGL(lstm_rowstats_kernel, dim3((unsigned)c.SB), dim3(256), 0, c.st, (const float*)y.xw, (int)c.G, y.stats);
}
// Inter-layer dropout of an (S,B,H) sequence, in == out allowed; the mask is keyed to the upper layer k of the pair.
inline void dropout(const LstmCall& c, const float* in, float* out, int k) {
    const long n = (long)(c.SB * c.H), blocks = (n + 255) / 256;
    hipLaunchKernelGGL(dropout_kernel, dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), dim3(256), 0, c.st, in, out, n,
                       c.seed + 0x1000003ull * (uint64_t)k, c.drop_thr, c.drop_scale);
}
inline int clear_xchg(const LstmCall& c, size_t words) {   // the words a persistent small-batch kernel polls
    return hipMemsetAsync(c.w.xchg, 0, words * sizeof(u64), c.st) != hipSuccess ? last_error() : HPC_RLL_OK;
}
// xw = xin @ Wx of a layer; split-K partials at small S*B (latency regime) are summed in slice order.
inline void x_branch(const LstmCall& c, const Layer& y, bool may_transpose) {
    const int SB = (int)c.SB, G = (int)c.G, skf = gemm_splitk(SB, G, y.in_l);
    // Products whose tiles take the LDS-DMA kernel run as NT against a weight copy transposed once per layer
    // (~10 us): both operands k-contiguous is what the DMA staging needs (gemm_f32.hpp: DmaStage)
    // (not when the product takes the NN DMA kernel with Wx as it lies: 141.3 against 140.1 TFLOP/s on the C4 shape)
    const bool nt = may_transpose && !gemm_nn_dma_ok(SB, G, y.in_l, skf) && gemm_dma_ok(SB, G, y.in_l, skf);
    if (nt) launch_transpose(y.wx_l, c.w.wxT, y.in_l, G, c.st);   // (in, G) -> (G, in): B(k=i, n=g) = wxT[g*in + i]
    GemmArgs g{y.xin, nt ? (const float*)c.w.wxT : y.wx_l, skf > 1 ? c.w.wpart : y.xw, SB, G, y.in_l, y.in_l, 1,
               nt ? 1 : (long)G, nt ? (long)y.in_l : 1, (long)G, 0, skf, (long)(c.SB * c.G)};
    launch_gemm(g, c.st);
    if (skf > 1) sum_parts(c, c.w.wpart, skf, c.SB * c.G, y.xw);
}
// after a layer's recurrence: hn / cn from the last step, the dropped-out sequence for the layer above and the backward
inline int finish_layer_fwd(const LstmCall& c, const Layer& y) {
    const size_t last = (size_t)(c.S - 1) * c.BH, o = (size_t)y.l * c.BH;
    int rc = copy_async(c.hn + o, y.hseq + last, c.BH, c.st);
    if (!rc) rc = copy_async(c.cn + o, y.c + last, c.BH, c.st);
    if (!rc && c.dropout && y.l < c.L - 1) dropout(c, y.hseq, y.xin_next, y.l + 1);
    return rc;
}
inline int copy_y(const LstmCall& c) {   // y inside the workspace (hpc_rll_lstm_workspace_y_offset): already written
    const float* hseq = c.w.layer[c.L - 1].hseq;
    const int rc = c.y != hseq ? copy_async(c.y, hseq, c.SB * c.H, c.st) : 0;
    return rc ? rc : last_error();
}
// which path -------------------------------------------------------------------------------------------------------
// clear_persist: the per-layer persistent kernels can run, their exchange words are cleared (backward: wavefront or not)
struct PathChoice { LstmPath path; int status; bool clear_persist; WaveCfg wc; PersistCfg pc; XchgLayout xl; };
// The *_ok(..., st) predicates query the runtime: each stands last in its condition, behind the path's shape and
// alignment, and a path is asked about only once the ones before it have declined.
inline PathChoice choose_fwd_path(const LstmCall& c) {
    PathChoice f{kStep, HPC_RLL_OK, false, {}, {}, xchg_layout(c.B, c.H)};
    // B <= 4: {value, tag} exchange words in the workspace, whole only on an 8-byte boundary (xchg_al8)
    if (xchg_al8(c.ws) && wave_fwd_ok(c.S, c.B, c.H, c.L, &f.wc, c.st)) f.path = kWave;
    else if (xchg_al8(c.ws) && persist_cfg(c.B, c.H, c.H, &f.pc) && persist_fwd_ok(f.pc, c.st))
        f.path = kPersist, f.clear_persist = true;
    // large batches: xw / hw gate-interleaved (shape-only: the backward must agree), one persistent kernel per layer
    // when the device can hold a row block's workgroups co-resident
    else if (lstm_perm_shape(c.B, c.H)) {
        if (!all_al16({c.x, c.h0, c.c0, c.wx, c.wh, c.bias, c.gamma, c.beta, c.y, c.hn, c.cn, c.ws}) || c.I % 4 != 0)
            f.status = HPC_RLL_EALIGN;   // these shapes run 16-byte kernels only
        else f.path = block_fwd_ok(c.B, c.H, c.st) ? kBlock : kStepPerm;
    }
    // mid-size batches: one persistent kernel per layer (lstm_mid.hpp), 16-byte accesses to the workspace and h0
    else if (cell_al16(c.ws) && cell_al16(c.h0) && mid_fwd_ok(c.B, c.H, c.st)) f.path = kMid;
    return f;
}
// (all of this holds for every layer of the call; the step kernels' row-walking cell is decided per layer, run_step_bwd)
inline PathChoice choose_bwd_path(const LstmCall& c, const float* y_ext) {
    PathChoice b{kStep, HPC_RLL_OK, false, {}, {}, xchg_layout(c.B, c.H)};
    b.clear_persist = xchg_al8(c.ws) && persist_cfg(c.B, c.H, 4 * c.H, &b.pc) && persist_bwd_ok(b.pc, c.st);
    // gate-interleaved xw / hw (what the forward wrote at these shapes): 16-byte kernels only
    const bool perm = lstm_perm_shape(c.B, c.H);
    if (perm && (!all_al16({c.g.dy, c.g.dhn, c.g.dcn, c.x, c.h0, c.c0, c.wx, c.wh, c.gamma, c.ws, c.g.dx, c.g.dh0, c.g.dc0,
                            c.g.dwx, c.g.dwh, y_ext}) || c.I % 4 != 0))
        b.status = HPC_RLL_EALIGN;
    else if (c.w.dwave && xchg_al8(c.ws) && wave_bwd_ok(c.S, c.B, c.H, c.L, &b.wc, c.st)) b.path = kWave;
    else if (b.clear_persist) b.path = kPersist;
    // large batches on the interleaved layout: the whole backward recurrence of a layer in one persistent kernel
    else if (perm) b.path = block_bwd_ok(c.B, c.H, c.st) ? kBlock : kStepPerm;
    // mid-size batches (lstm_mid.hpp): saved gates, 16-byte accesses to the workspace
    else if (c.w.layer[0].gates && cell_al16(c.ws) && mid_bwd_ok(c.B, c.H, c.st)) b.path = kMid;
    return b;
}
// forward: the paths -----------------------------------------------------------------------------------------------
// 1: one kernel walks the whole sequence of the layer (lstm_persist.hpp); its exchange words were cleared once per call
inline int run_persist_fwd(const LstmCall& c, const Layer& y, const PathChoice& f) {
    x_branch(c, y, true);
    row_stats(c, y);
    PersistFwd a{y.xw, y.wh_l, y.bias_l, y.gamma_l, y.beta_l, y.h0_l, y.c0_l, y.hw, y.gates, y.c, y.hseq, y.stats,
                 (u64*)c.w.xchg, (u64*)c.w.xchg + 2 * f.xl.big_par, c.S, c.B, c.H, f.pc.nwg, g_lstm_xchg_rep, f.xl.big_par,
                 f.xl.sums_par, f.xl.big_rep, f.xl.sums_rep, (uint32_t)((size_t)y.l * c.S), persist_prof()};
    const int rc = launch_persist_fwd(f.pc, a, c.st);
    if (!rc) persist_prof_report("fwd", y.l, c.S, c.st);
    return rc;
}
// 5: the same for mid-size batches (lstm_mid.hpp)
inline int run_mid_fwd(const LstmCall& c, const Layer& y) {
    x_branch(c, y, true);
    row_stats(c, y);
    MidFwd a{y.xw, y.wh_l, y.bias_l, y.gamma_l, y.beta_l, y.h0_l, y.c0_l, y.hw, y.gates, y.c, y.hseq, y.stats,
             nullptr, nullptr, nullptr, nullptr, c.S, c.B, 0, c.H, 0, 0, 0, 0, nullptr};
    return launch_mid_fwd(a, c.w.mid, y.l, c.st);
}
// 3 and 4: the layer's interleaved weight copies and the x-branch product against them; stats: with the row statistics
inline void perm_x_branch(const LstmCall& c, const Layer& y, bool stats) {
    launch_perm_cols(y.wx_l, c.w.wxP, y.in_l, c.H, c.st);
    launch_perm_cols(y.wh_l, c.w.whP, c.H, c.H, c.st);
    GemmArgs g{y.xin, c.w.wxP, y.xw, (int)c.SB, (int)c.G, y.in_l, y.in_l, 1, (long)c.G, 1, (long)c.G, 0};
    g.rowpart = y.hw;   // (free until the recurrence writes it: 2 * S*B * 4H/128 floats of it are borrowed)
    if (stats && gemm_nn_rowstats_ok(g)) {
        launch_gemm_nn_rowstats(g, c.st);
        hipLaunchKernelGGL(lstm_xstats_kernel, dim3((unsigned)((c.SB + 255) / 256)), dim3(256), 0, c.st,
                           (const float*)y.hw, (int)(c.G / 128), (long)c.SB, y.stats);
        return;
    }
    g.rowpart = nullptr;
    launch_gemm(g, c.st);
    if (stats) row_stats(c, y);
}
// 0 and 3 (perm: interleaved layout, no split-K): one product and one cell launch per step
inline int run_step_fwd(const LstmCall& c, const Layer& y, bool perm) {
    const int B = c.B, H = c.H, G = (int)c.G;
    const size_t BG = (size_t)B * G, BH = c.BH;
    int sk = 1; bool nt = false;
    if (perm) perm_x_branch(c, y, false);
    else {
        x_branch(c, y, true);
        sk = gemm_splitk(B, G, H);
        nt = !gemm_nn_dma_ok(B, G, H, sk) && gemm_dma_ok(B, G, H, sk);
        if (nt) launch_transpose(y.wh_l, c.w.whT, H, G, c.st);      // (H, G) -> (G, H): B(k=h, n=g) = whT[g*H + h]
    }
    const float* wh = perm ? c.w.whP : nt ? c.w.whT : y.wh_l;
    for (int s = 0; s < c.S; ++s) {
        const float* h_prev = s == 0 ? y.h0_l : y.hseq + (s - 1) * BH;
        const float* c_prev = s == 0 ? y.c0_l : y.c + (s - 1) * BH;
        float* hw_s = y.hw + s * BG;
        float* hw_raw = sk > 1 ? c.w.hw_part : hw_s;   // the product's (partial) output, which the cell sums and normalises
        GemmArgs g{h_prev, wh, hw_raw, B, G, H, H, 1, nt ? 1 : (long)G, nt ? (long)H : 1, (long)G, 0, sk, perm ? 0 : (long)BG};
        launch_gemm(g, c.st);
        launch_cell_fwd(H, B, c.st, (const float*)(y.xw + s * BG), (const float*)hw_raw, sk, (long)BG, hw_s, y.bias_l,
                        y.gamma_l, y.beta_l, c_prev, y.gates ? y.gates + s * BG : (float*)nullptr, y.c + s * BH,
                        y.hseq + s * BH, y.stats + (size_t)s * B * 4, perm);
    }
    return HPC_RLL_OK;
}
// 4: the layer's recurrence in one persistent row-block kernel (lstm_block.hpp)
inline int run_block_fwd(const LstmCall& c, const Layer& y) {
    perm_x_branch(c, y, true);
    BlockFwd a{y.xw, c.w.whP, y.bias_l, y.gamma_l, y.beta_l, y.h0_l, y.c0_l, y.hw, y.c, y.hseq, y.stats,
               nullptr, nullptr, c.S, c.B, c.H, 0, 0, 0, nullptr, 0};
    return launch_block_fwd(a, c.w.blk_part, reinterpret_cast<unsigned*>(c.w.blk_flags), c.st);
}
// 2: all layers in one launch (lstm_wave.hpp).  It addresses every layer's buffers with one stride: the h sequences
// stay in the workspace and y is filled by the copy at the end -- a few KB at B <= 4.
inline int run_wave_fwd(const LstmCall& c, const WaveCfg& wc) {
    const Layer l0 = c.layer(0);
    x_branch(c, l0, false);
    row_stats(c, l0);
    int rc = clear_xchg(c, wc.hx_words + wc.sx_words);
    if (rc) return rc;
    WaveFwd a{l0.xw, c.wx, c.wh, c.bias, c.gamma, c.beta, c.h0, c.c0, l0.xw, l0.hw, l0.gates, l0.c, l0.hseq, l0.stats,
              (size_t)(c.w.layer[1].xw - l0.xw), (u64*)c.w.xchg, (u64*)c.w.xchg + wc.hx_words, c.S, c.B, c.I, c.H, c.L,
              wc.nwg, c.seed, c.drop_thr, c.drop_scale};
    if ((rc = launch_wave_fwd(wc, a, c.st))) return rc;
    for (int l = 0; l < c.L; ++l)   // (the dropped-out sequences are for the backward's products)
        if ((rc = finish_layer_fwd(c, c.layer(l)))) return rc;
    return copy_y(c);
}
// y_hseq: y doubles as the last layer's h sequence (the caller hands the SAME y to the backward, which reads it there):
// the cells write y directly, the workspace's own slot for it stays unused, no (S,B,H) copy.
int lstm_forward_impl(const float* x, const float* h0, const float* c0, const float* wx, const float* wh, const float* bias,
                      const float* ln_gamma, const float* ln_beta, float* y, float* hn, float* cn, float* ws, int S, int B,
                      int I, int H, int L, float dropout_p, uint64_t seed, bool y_hseq, void* stream) {
    if (S < 0 || B < 0 || I <= 0 || H <= 0 || L <= 0 || L > 16) return HPC_RLL_EINVAL;
    if (H > 2048) return HPC_RLL_EUNSUPPORTED;
    if (!(dropout_p >= 0.f && dropout_p < 1.f)) return HPC_RLL_EINVAL;
    if (persist_async_status()) return HPC_RLL_ETIMEOUT;   // an earlier persistent launch gave up: see the header
    if (B == 0) return HPC_RLL_OK;
    if (!h0 || !c0 || !wx || !wh || !bias || !ln_gamma || !ln_beta || !hn || !cn) return HPC_RLL_EINVAL;
    if (S > 0 && (!x || !y || !ws)) return HPC_RLL_EINVAL;
    if (S == 0) {   // no step: the final states are the initial ones
        record_fwd_path(kStep), ws_pair_record(ws, false);
        int rc = copy_async(hn, h0, (size_t)L * B * H, (hipStream_t)stream);
        if (!rc) rc = copy_async(cn, c0, (size_t)L * B * H, (hipStream_t)stream);
        return rc ? rc : last_error();
    }
    LstmCall c = make_call(ws, S, B, I, H, L, dropout_p, seed, stream, x, h0, c0, wx, wh, bias, ln_gamma, ln_beta);
    c.y = y, c.hn = hn, c.cn = cn;
    if (cell_recompute_gates(B, H)) {   // the backward recomputes the gates: it needs bias and beta (not in its list)
        int rc = copy_async(c.w.pstash, bias, (size_t)L * c.G, c.st);
        if (!rc) rc = copy_async(c.w.pstash + (size_t)L * c.G, ln_beta, (size_t)L * 2 * c.G, c.st);
        if (rc) return rc;
    }
    const PathChoice f = choose_fwd_path(c);
    record_fwd_path(f.path);
    ws_pair_record(ws, y_hseq && f.path != kWave && y != c.w.layer[L - 1].hseq);
    if (f.status) return f.status;
    if (f.path == kWave) return run_wave_fwd(c, f.wc);
    if (y_hseq) c.w.layer[L - 1].hseq = y;
    int rc = f.clear_persist ? clear_xchg(c, f.xl.total_words) : 0;
    for (int l = 0; l < L && !rc; ++l) {
        const Layer ly = c.layer(l);
        switch (f.path) {
            case kPersist: rc = run_persist_fwd(c, ly, f); break;
            case kMid: rc = run_mid_fwd(c, ly); break;
            case kBlock: rc = run_block_fwd(c, ly); break;
            default: rc = run_step_fwd(c, ly, f.path == kStepPerm); break;
        }
        if (!rc) rc = last_error();
        if (!rc) rc = finish_layer_fwd(c, ly);
    }
    return rc ? rc : copy_y(c);
}
// backward ---------------------------------------------------------------------------------------------------------
// (rows, 4H) weight gradient from its `nparts` partial products in wpart (interleaved layout: always via wpart)
inline void sum_weight_parts(const LstmCall& c, bool perm, int nparts, size_t rows, float* out) {
    if (perm)
        hipLaunchKernelGGL(sum_parts_unperm_kernel, dim3((unsigned)((rows * c.H + 255) / 256)), dim3(256), 0, c.st,
                           (const float*)c.w.wpart, nparts, (long)(rows * c.G), (long)rows, c.H, out);
    else if (nparts > 1) sum_parts(c, c.w.wpart, nparts, rows * c.G, out);
}
// Weight / parameter gradients of a layer from its gate-gradient buffers, and (if `dxin`) d(layer input);
// summed_chunks > 0: colpart already holds that many rows of column sums.
inline void layer_grads(const LstmCall& c, const Layer& y, const float* p_dgate, const float* p_dxw, const float* p_dhw,
                        float* dxin, int summed_chunks) {
    const int S = c.S, B = c.B, H = c.H, G = (int)c.G, in_l = y.in_l, SB = (int)c.SB;
    const Ws& w = c.w;
    hipStream_t st = c.st;
    // dWh (H,G) = [h0 ; hseq[0..S-2]]^T @ dHW ; dWx (in,G) = xin^T @ dXW.  K = S*B is long and the output tiles
    // alone may not fill the chip: slices of K go to partial buffers, summed in slice order (deterministic).
    // (perm: the products come out gate-interleaved; always via the partial buffer, un-permuted by the summation)
    const size_t HG = (size_t)H * G;
    const int skh = S > 1 ? gemm_splitk_big(H, G, (int)((S - 1) * (size_t)B)) : 1;
    float* dwh_l = c.g.dwh + (size_t)y.l * HG;
    float* first = (skh > 1 || y.perm) ? w.wpart : dwh_l;
    GemmArgs g0{y.h0_l, p_dhw, first, H, G, B, 1, (long)H, (long)G, 1, (long)G, 0};
    launch_gemm(g0, st);
    if (S > 1) {
        GemmArgs g1{y.hseq, p_dhw + (size_t)B * G, skh > 1 ? w.wpart + HG : first, H, G, (int)((S - 1) * (size_t)B), 1,
                    (long)H, (long)G, 1, (long)G, skh > 1 ? 0 : 1, skh, (long)HG, 1};
        launch_gemm(g1, st);
    }
    sum_weight_parts(c, y.perm, skh > 1 ? skh + 1 : 1, H, dwh_l);
    const int skx = gemm_splitk_big(in_l, G, SB);
    float* dwx_l = c.g.dwx + y.wx_off;
    GemmArgs gx{y.xin, p_dxw, (skx > 1 || y.perm) ? w.wpart : dwx_l, in_l, G, SB, 1, (long)in_l, (long)G, 1, (long)G, 0,
                skx, (long)((size_t)in_l * G), 1};
    launch_gemm(gx, st);
    sum_weight_parts(c, y.perm, skx > 1 ? skx : 1, in_l, dwx_l);
    if (dxin) {   // d xin (S*B, in) = dXW @ Wx^T : B(k=g, n=i) = Wx[i*G + g]
        const size_t n = c.SB * in_l;
        const int skd = gemm_splitk(SB, in_l, G);
        // NN against a transposed copy only where it was measured to win (C4: -2 %; B <= 1024: +2..5 %)
        // (with LDS-DMA staging the NT form -- the weights as they lie -- is the fast one: no transposed copy)
        // (... unless the NN form itself takes the NN DMA kernel, which is the faster of the two: then NN it stays)
        const bool nn = g_lstm_nn_bwd && (double)c.SB * in_l >= (double)(1u << 28) &&
                        (gemm_nn_dma_ok(SB, in_l, G, skd) || !gemm_dma_ok(SB, in_l, G, skd));
        if (nn) launch_transpose(y.wx_l, w.wxT, in_l, G, st);   // (in, G) -> (G, in): B(k=g, n=i) = wxT[g*in + i]
        GemmArgs g{p_dxw, nn ? (const float*)w.wxT : y.wx_l, skd > 1 ? w.wpart : dxin, SB, in_l, G, (long)G, 1,
                   nn ? (long)in_l : 1, nn ? 1 : (long)G, (long)in_l, 0, skd, (long)n};
        launch_gemm(g, st);
        if (skd > 1) sum_parts(c, w.wpart, skd, n, dxin);
    }
    const int chunks = summed_chunks > 0 ? summed_chunks : (int)(c.SB < (size_t)kColChunks * 8 ? (c.SB + 7) / 8 : kColChunks);
    if (summed_chunks <= 0)
        hipLaunchKernelGGL(lstm_colreduce_kernel, dim3((unsigned)((G + 63) / 64), chunks), dim3(256), 0, st, p_dgate,
                           (const float*)y.xw, (const float*)y.hw, (const float*)y.stats, (long)c.SB, G, w.colpart);
    hipLaunchKernelGGL(lstm_colfinal_kernel, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, st, (const float*)w.colpart,
                       chunks, G, c.g.dbias + (size_t)y.l * G, c.g.dln_gamma + (size_t)y.l * 2 * G,
                       c.g.dln_beta + (size_t)y.l * 2 * G, y.perm ? 1 : 0);
}
// The step kernels' dh_prev (B,H) = dHW_s (B,G) @ Wh^T: NN against a transposed copy of Wh, or NT against Wh as it lies.
struct DhForm { bool nn, big; int sk; };
inline DhForm dh_form(const LstmCall& c) {
    const int B = c.B, H = c.H, G = (int)c.G;
    const bool nn = g_lstm_nn_bwd != 0 && (long)B * H >= (1L << 22);   // large batches only (measured)
    // NN form: 128x128x16 tiles with their own split-K (one round of ~1024 workgroups), like the forward product
    const bool big = nn && g_lstm_dh_big;
    const int sk = big ? gemm_splitk_big(B, H, G) : gemm_splitk(B, H, G);
    // ... unless that product takes the LDS-DMA kernel as NT against Wh as it lies (no transposed copy)
    return {nn && (gemm_nn_dma_ok(B, H, G, sk) || !gemm_dma_ok(B, H, G, sk)), big, sk};
}
// 0 and 3: one cell launch and one product per step; *summed_chunks: rows of column sums the cells left in colpart
inline int run_step_bwd(const LstmCall& c, const Layer& y, int* summed_chunks) {
    const int S = c.S, B = c.B, H = c.H, G = (int)c.G;
    const size_t BG = (size_t)B * G, BH = c.BH;
    const Ws& w = c.w;
    const DhForm f = dh_form(c);
    if (f.nn) launch_transpose(y.wh_l, w.whT, H, G, c.st);   // (H, G) -> (G, H): B(k=g, n=h) = whT[g*H + h]
    // large batches: the cell walks several rows per workgroup and keeps the bias / gamma / beta column sums (no
    // dgate buffer, no reduction pass) -- 16-byte accesses: every base pointer 16-byte aligned, d_out being this layer's
    const int rows_wgs = y.perm ? (g_cell_rows_wgs > 0 ? g_cell_rows_wgs : 512)   // (the only cell of this layout)
                         : (cell_rows_shape(B, H) && all_al16({y.d_out, c.g.dhn, c.g.dcn, c.c0, c.ws, c.gamma}))
                             ? (B < g_cell_rows_wgs ? B : g_cell_rows_wgs) : 0;
    const float *dh = y.dh, *dc = y.dc;
    int dh_parts = 1;   // how many split-K partials dh consists of
    for (int s = S - 1; s >= 0; --s) {
        const float* c_prev = s == 0 ? y.c0_l : y.c + (s - 1) * BH;
        const CellBwdArgs ca{y.d_out ? y.d_out + s * BH : (const float*)nullptr, dh, dh_parts, (long)BH, dc,
                             y.gates ? (const float*)(y.gates + s * BG) : (const float*)nullptr, y.c + s * BH, c_prev,
                             y.xw + s * BG, y.hw + s * BG, y.stats + (size_t)s * B * 4, y.gamma_l, y.beta_l, y.bias_l,
                             w.dgate + s * BG, w.dxw + s * BG, w.dhw + s * BG, w.dc, H};
        if (rows_wgs) launch_cell_bwd_rows(B, rows_wgs, c.st, ca, w.colpart, s == S - 1 ? 1 : 0, y.perm ? w.pperm : nullptr);
        else launch_cell_bwd(B, c.st, ca);
        GemmArgs g{w.dhw + s * BG, f.nn ? (const float*)w.whT : y.wh_l, w.dh, B, H, G, (long)G, 1, f.nn ? (long)H : 1,
                   f.nn ? 1 : (long)G, (long)H, 0, f.sk, (long)BH, f.big ? 1 : 0};
        launch_gemm(g, c.st);
        dh = w.dh, dc = w.dc, dh_parts = f.sk;
    }
    const int rc = last_error();
    if (rc) return rc;
    *summed_chunks = rows_wgs;
    sum_parts(c, w.dh, dh_parts, BH, y.dh0_l);
    return copy_async(y.dc0_l, w.dc, BH, c.st);
}
// 1: one kernel walks the whole sequence of the layer backwards (lstm_persist.hpp)
inline int run_persist_bwd(const LstmCall& c, const Layer& y, const PathChoice& b) {
    const Ws& w = c.w;
    PersistBwd a{y.d_out, y.dh, y.dc, y.gates, y.c, y.c0_l, y.xw, y.hw, y.stats, y.gamma_l, y.wh_l, w.dgate, w.dxw, w.dhw,
                 y.dh0_l, y.dc0_l, (u64*)w.xchg, (u64*)w.xchg + 2 * b.xl.big_par, c.S, c.B, c.H, b.pc.nwg, g_lstm_xchg_rep,
                 b.xl.big_par, b.xl.sums_par, b.xl.big_rep, b.xl.sums_rep, (uint32_t)((size_t)(c.L - 1 - y.l) * c.S),
                 persist_prof()};
    const int rc = launch_persist_bwd(b.pc, a, c.st);
    if (!rc) persist_prof_report("bwd", y.l, c.S, c.st);
    return rc;
}
// 5: the same for mid-size batches (lstm_mid.hpp)
inline int run_mid_bwd(const LstmCall& c, const Layer& y) {
    MidBwd a{y.d_out, y.dh, y.dc, y.gates, y.c, y.c0_l, y.xw, y.hw, y.stats, y.gamma_l, y.wh_l, c.w.dgate, c.w.dxw, c.w.dhw,
             y.dh0_l, y.dc0_l, nullptr, nullptr, nullptr, nullptr, c.S, c.B, c.H, 0, 0, 0, 0, nullptr};
    return launch_mid_bwd(a, c.w.mid, y.l, c.st);
}
// 4: the same on the gate-interleaved layout (lstm_block.hpp); it leaves B / 128 rows of column sums in colpart
inline int run_block_bwd(const LstmCall& c, const Layer& y) {
    const Ws& w = c.w;
    // (the step kernels' transposed Wh, which nothing reads here: kept so that a call's launches stay what they were)
    if (dh_form(c).nn) launch_transpose(y.wh_l, w.whT, c.H, (int)c.G, c.st);
    BlockBwd a{y.d_out, y.dh, y.dc, y.xw, y.hw, y.c, y.c0_l, y.stats, w.pperm, w.whP, w.dxw, w.dhw, w.dgate, w.dc,
               y.dh0_l, y.dc0_l, nullptr, nullptr, nullptr, c.S, c.B, c.H, 0, 0, 0, nullptr, 0};
    return launch_block_bwd(a, w.blk_part, reinterpret_cast<unsigned*>(w.blk_flags), w.colpart, c.st);
}
// 2: the recurrences of all layers in one launch (lstm_wave.hpp), then each layer's weight and parameter gradients
inline int run_wave_bwd(const LstmCall& c, const WaveCfg& wc) {
    const Ws& w = c.w;
    int rc = clear_xchg(c, 2 * wc.hx_words + wc.sx_words);
    if (rc) return rc;
    const LayerWs& l0 = w.layer[0];
    const size_t SBG = c.SB * c.G;
    WaveBwd a{c.g.dy, c.g.dhn, c.g.dcn, l0.gates, l0.c, l0.xw, l0.hw, l0.stats, (size_t)(w.layer[1].xw - l0.xw), c.c0,
              c.gamma, c.wx, c.wh, w.dwave, w.dwave + SBG, w.dwave + 2 * SBG, 3 * SBG, c.g.dh0, c.g.dc0, (u64*)w.xchg,
              (u64*)w.xchg + wc.hx_words, (u64*)w.xchg + 2 * wc.hx_words, c.S, c.B, c.I, c.H, c.L, wc.nwg, c.seed,
              c.drop_thr, c.drop_scale};
    if ((rc = launch_wave_bwd(wc, a, c.st))) return rc;
    for (int l = c.L - 1; l >= 0; --l) {
        const float* base = w.dwave + (size_t)l * 3 * SBG;
        layer_grads(c, c.layer(l), base, base + SBG, base + 2 * SBG, l == 0 ? c.g.dx : nullptr, 0);
    }
    return last_error();
}
// y_ext != null: the last layer's h sequence lives in y (see lstm_forward_impl), not in the workspace
int lstm_backward_impl(const float* dy, const float* dhn, const float* dcn, const float* x, const float* h0, const float* c0,
                       const float* wx, const float* wh, const float* ln_gamma, const float* y_ext, float* ws, float* dx,
                       float* dh0, float* dc0, float* dwx, float* dwh, float* dbias, float* dln_gamma, float* dln_beta, int S,
                       int B, int I, int H, int L, float dropout_p, uint64_t seed, void* stream) {
    if (S <= 0 || B <= 0 || I <= 0 || H <= 0 || L <= 0 || L > 16) return HPC_RLL_EINVAL;
    if (H > 2048) return HPC_RLL_EUNSUPPORTED;
    if (persist_async_status()) return HPC_RLL_ETIMEOUT;
    // dx may be NULL: the caller does not need the gradient of the layer-0 input (its S*B x I x 4H product is skipped)
    if (!x || !h0 || !c0 || !wx || !wh || !ln_gamma || !ws || !dh0 || !dc0 || !dwx || !dwh || !dbias ||
        !dln_gamma || !dln_beta)
        return HPC_RLL_EINVAL;
    LstmCall c = make_call(ws, S, B, I, H, L, dropout_p, seed, stream, x, h0, c0, wx, wh, nullptr, ln_gamma, nullptr);
    c.bias = c.w.pstash;                       // (L,4H), then ln_beta (L,2,4H): parked by a gate-recomputing forward
    c.beta = c.w.pstash + (size_t)L * c.G;
    c.g = {dy, dhn, dcn, dx, dh0, dc0, dwx, dwh, dbias, dln_gamma, dln_beta};
    if (!y_ext && ws_pair_needs_y(ws)) return HPC_RLL_EINVAL;    // forward_y on this workspace pairs with backward_y only
    if (y_ext) c.w.layer[L - 1].hseq = const_cast<float*>(y_ext);   // read only on this side
    const PathChoice b = choose_bwd_path(c, y_ext);
    if (b.status) return b.status;
    int rc = b.clear_persist ? clear_xchg(c, b.xl.total_words) : 0;
    if (rc) return rc;
    record_bwd_path(b.path);
    if (b.path == kWave) return run_wave_bwd(c, b.wc);
    const bool perm = b.path == kStepPerm || b.path == kBlock;
    const float* d_out = dy;
    float* seq_bufs[2] = {c.w.dseq_a, c.w.dseq_b};
    for (int l = L - 1, flip = 0; l >= 0; --l) {
        Layer y = c.layer(l);
        y.d_out = d_out, y.perm = perm;
        if (perm) {   // this layer's interleaved weight copies (the forward's were overwritten by the layers above)
            launch_perm_cols(y.wh_l, c.w.whP, H, H, c.st);
            launch_perm_cols(y.wx_l, c.w.wxP, y.in_l, H, c.st);
            hipLaunchKernelGGL(perm_params_kernel, dim3((unsigned)((c.G + 255) / 256)), dim3(256), 0, c.st, y.gamma_l,
                               y.beta_l, y.bias_l, c.w.pperm, H);
            y.wh_l = c.w.whP, y.wx_l = c.w.wxP;
        }
        int summed_chunks = 0;
        switch (b.path) {
            case kPersist: rc = run_persist_bwd(c, y, b); break;
            case kMid: rc = run_mid_bwd(c, y); break;
            case kBlock: rc = run_block_bwd(c, y); summed_chunks = B / 128; break;
            default: rc = run_step_bwd(c, y, &summed_chunks); break;
        }
        if (!rc) rc = last_error();
        if (rc) return rc;
        float* dxin = l == 0 ? dx : seq_bufs[flip];
        layer_grads(c, y, c.w.dgate, c.w.dxw, c.w.dhw, dxin, summed_chunks);
        if (l > 0) {
            if (c.dropout) dropout(c, dxin, dxin, l);   // backward of the dropout between layer l-1 and l: same mask, same scale
            d_out = dxin;
            flip ^= 1;
        }
        if ((rc = last_error())) return rc;
    }
    return HPC_RLL_OK;
}
} }  // namespace hpc_rll::(anonymous)

using namespace hpc_rll;

extern "C" int64_t hpc_rll_lstm_workspace_floats(int S, int B, int I, int H, int L, float dropout_p) {
    if (S < 0 || B < 0 || I < 0 || H < 0 || L < 0 || L > 16) return -1;
    return (int64_t)carve(nullptr, S, B, I, H, L, dropout_p > 0.f).total;
}

// Float offset, inside the workspace, of the last layer's h sequence (S,B,H) -- which IS y.  A caller that passes
// y = ws + this offset gets y written in place by the cells and no copy (2.1 GB each way at C4: 0.8 ms of a 74 ms forward).
extern "C" int64_t hpc_rll_lstm_workspace_y_offset(int S, int B, int I, int H, int L, float dropout_p) {
    if (S < 0 || B < 0 || I < 0 || H < 0 || L <= 0 || L > 16) return -1;
    float* const fake = reinterpret_cast<float*>((uintptr_t)1 << 20);
    return (int64_t)(carve(fake, S, B, I, H, L, dropout_p > 0.f).layer[L - 1].hseq - fake);
}

extern "C" int hpc_rll_lstm_forward(const float* x, const float* h0, const float* c0, const float* wx,
                                    const float* wh, const float* bias, const float* ln_gamma, const float* ln_beta,
                                    float* y, float* hn, float* cn, float* ws, int S, int B, int I, int H, int L,
                                    float dropout_p, uint64_t seed, void* stream) {
    return lstm_forward_impl(x, h0, c0, wx, wh, bias, ln_gamma, ln_beta, y, hn, cn, ws, S, B, I, H, L, dropout_p, seed, false,
                             stream);
}
extern "C" int hpc_rll_lstm_backward(const float* dy, const float* dhn, const float* dcn, const float* x,
                                     const float* h0, const float* c0, const float* wx, const float* wh,
                                     const float* ln_gamma, float* ws, float* dx, float* dh0, float* dc0, float* dwx,
                                     float* dwh, float* dbias, float* dln_gamma, float* dln_beta, int S, int B, int I,
                                     int H, int L, float dropout_p, uint64_t seed, void* stream) {
    return lstm_backward_impl(dy, dhn, dcn, x, h0, c0, wx, wh, ln_gamma, nullptr, ws, dx, dh0, dc0, dwx, dwh, dbias, dln_gamma,
                              dln_beta, S, B, I, H, L, dropout_p, seed, stream);
}
// Which kernels the most recent hpc_rll_lstm_forward* call of this process ran its recurrence on (a diagnostic, like
// hpc_rll_gae_last_config): 0 = one product + one cell launch per step, 1 = per-layer persistent kernels (B <= 4),
// 2 = layer wavefront (B <= 4, L >= 2), 3 = step kernels on gate-interleaved pre-activations (large batch), 4 = persistent
// row-block kernel (large batch, lstm_block.hpp), 5 = persistent mid-batch kernel (lstm_mid.hpp); -1 = no forward yet.  The
// calling thread's own most recent forward if it ran one, else the process's.
extern "C" int hpc_rll_lstm_last_forward_path(void) {
    return t_lstm_last_path >= 0 ? t_lstm_last_path : g_lstm_last_path.load(std::memory_order_relaxed);
}
// ... and the most recent hpc_rll_lstm_backward* call (last layer processed): same codes.
extern "C" int hpc_rll_lstm_last_backward_path(void) { return g_lstm_last_bwd_path.load(std::memory_order_relaxed); }

// The pair a framework binding uses (ABI 4): y is the caller's own (S,B,H) tensor AND the last layer's saved h sequence.
// The forward's cells write it directly (no copy, nothing of the workspace is handed out), the backward gets the same y
// back.  A holder of y pins S*B*H floats, not the workspace; modifying y between the two calls invalidates the backward
// (the binding's job to detect: torch's saved-tensor version counter does).
extern "C" int hpc_rll_lstm_forward_y(const float* x, const float* h0, const float* c0, const float* wx,
                                      const float* wh, const float* bias, const float* ln_gamma, const float* ln_beta,
                                      float* y, float* hn, float* cn, float* ws, int S, int B, int I, int H, int L,
                                      float dropout_p, uint64_t seed, void* stream) {
    return lstm_forward_impl(x, h0, c0, wx, wh, bias, ln_gamma, ln_beta, y, hn, cn, ws, S, B, I, H, L, dropout_p, seed, true,
                             stream);
}
extern "C" int hpc_rll_lstm_backward_y(const float* dy, const float* dhn, const float* dcn, const float* x,
                                       const float* h0, const float* c0, const float* wx, const float* wh,
                                       const float* ln_gamma, const float* y, float* ws, float* dx, float* dh0, float* dc0,
                                       float* dwx, float* dwh, float* dbias, float* dln_gamma, float* dln_beta, int S, int B,
                                       int I, int H, int L, float dropout_p, uint64_t seed, void* stream) {
    if (!y) return HPC_RLL_EINVAL;
    return lstm_backward_impl(dy, dhn, dcn, x, h0, c0, wx, wh, ln_gamma, y, ws, dx, dh0, dc0, dwx, dwh, dbias, dln_gamma,
                              dln_beta, S, B, I, H, L, dropout_p, seed, stream);
}

extern "C" int hpc_rll_gemm_f32(const float* A, const float* B, float* C, int M, int N, int K, int64_t a_sm,
                                int64_t a_sk, int64_t b_sk, int64_t b_sn, int64_t ldc, int accumulate, void* stream) {
    if (M < 0 || N < 0 || K < 0) return HPC_RLL_EINVAL;
    if (M == 0 || N == 0) return HPC_RLL_OK;
    if (!C || (K > 0 && (!A || !B))) return HPC_RLL_EINVAL;
    GemmArgs g{A, B, C, M, N, K, (long)a_sm, (long)a_sk, (long)b_sk, (long)b_sn, (long)ldc, accumulate};
    launch_gemm(g, (hipStream_t)stream);
    return last_error();
}

// Sticky asynchronous status of the persistent LSTM kernels (see include/hpc_rll_hip.h).
extern "C" int hpc_rll_async_error(void) { return hpc_rll::persist_async_status(); }

extern "C" int hpc_rll_clear_async_error(void) {
    using namespace hpc_rll;
    PersistRuntime& r = persist_rt();
    if (!persist_async_status()) return HPC_RLL_OK;
    // residency was demonstrably not available in this deployment: the step kernels take over for good
    r.disabled = true;
    *(volatile unsigned*)r.host_status = 0u;
    return HPC_RLL_OK;
}

// Test hook: polls a persistent kernel waits before giving up, on the CURRENT device (0 = the shipped ~seconds).
extern "C" int hpc_rll_test_set_persist_spin_limit(int64_t polls) {
    using namespace hpc_rll;
    if (polls < 0) return HPC_RLL_EINVAL;
    const long v = polls == 0 ? kSpinLimit : (long)polls;
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_persist_spin_limit), &v, sizeof(v));
}

// Test hook: launch a kernel that keeps every CU busy for ~`ms` milliseconds on `stream` (tests/test_lstm_gpu.py runs
// the persistent LSTM on another stream meanwhile).  Not part of the operator set.
namespace hpc_rll { namespace {
__global__ __launch_bounds__(1024) void hog_kernel(long long ticks, unsigned* sink) {
    extern __shared__ float hog_lds[];
    const long long t0 = wall_clock64();
    unsigned x = threadIdx.x;
    while (wall_clock64() - t0 < ticks) x = x * 1664525u + 1013904223u;
    hog_lds[threadIdx.x] = (float)x;
    if (x == 0xdeadbeefu && sink) *sink = x;
}
} }
extern "C" int hpc_rll_test_occupy_device(int ms, int blocks, void* stream) {
    using namespace hpc_rll;
    if (ms < 0 || ms > 2000 || blocks < 0) return HPC_RLL_EINVAL;
    const int cus = persist_cu_count();
    if (cus <= 0) return HPC_RLL_EUNSUPPORTED;
    // a 1024-thread workgroup is 16 of a CU's 32 wave slots; with 80 KB of LDS exactly two fit a CU and fill it
    // completely (waves AND LDS).  blocks = 0: 2 x CUs = the whole device; fewer: the rest of the device stays free.
    const int n = blocks > 0 ? (blocks < 2 * cus ? blocks : 2 * cus) : 2 * cus;
    const size_t lds = 80 * 1024;
    if (hipFuncSetAttribute((const void*)hog_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return last_error();
    hipLaunchKernelGGL(hog_kernel, dim3(n), dim3(1024), lds, (hipStream_t)stream, (long long)ms * 100000LL,
                       (unsigned*)nullptr);   // wall_clock64 ticks at 100 MHz
    return last_error();
}
