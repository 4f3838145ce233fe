// gae_masked.hip -- episode-aware GAE (done / traj_flag masks) forward + analytic backward for gfx950 (MI355X).
//
// Textbook GAE with masks (DI-engine's `gae` with `done` and `traj_flag`), NOT the truncation-normalised variant of
// gae.hip.  With k^d_t = 1 - done_t, k^f_t = 1 - f_t (f = traj_flag, defaulting to done) and nv_t the next value
// (value[t+1] in the stacked form, next_value[t] in the next-value form):
//     forward : adv_t = delta_t + a_t * adv_{t+1},   delta_t = r_t + gamma*k^d_t*nv_t - V_t,   a_t = gamma*lambda*k^f_t
//     backward: d_t   = g_t + a_{t-1} * d_{t-1};  dL/dr_t = d_t;
//               next-value form: dL/dV_t = -d_t,  dL/dnv_t = gamma*k^d_t*d_t
//               stacked form   : dL/dV_t = -d_t [t<T] + gamma*k^d_{t-1}*d_{t-1} [t>=1]   (t = 0 .. T)
// Forward: an Op of the generic reverse column scan (colscan.hpp, s_t = b_t + a_t * s_{t+1}) with b = delta,
// a = gamma*lambda*k^f and no loss sums (NACC = 0).  The coefficient differs per column, so the chunk product is per lane,
// as in every colscan Op; the stacked form loads LC+1 value rows per chunk (`link` takes value[t+1] from the next row).
// Backward: its own kernel, the same chunked scan run forward in time (chunks aligned to t = 0, wave 0 earliest).  It was
// also run as a colscan Op on the time-reversed view u = T-1-t (bit-identical), and measured 6-11 % slower at C2 and at
// T=1024, B=4096 (profiles/r08_masked_gae_colscan_ab.txt), so it stays here.
//
//   * masks are loaded as they are stored (masks.hpp, shared with the masked TD(lambda) / V-trace of scan_masked.hip):
//     V bytes per lane for bool / uint8 (one dword for V = 4), V floats for float32.  traj_flag == NULL reuses the `done`
//     registers (no second mask stream).
//   * out-of-range columns load the last pack of the row and store nothing.  Backward loads are unconditional (row indices
//     of the ragged chunk are clamped into [0, T)); the forward's rows before t = 0 load row 0 (colscan).
//   * grid = ceil(B / TILE) workgroups, no inter-workgroup communication, no atomics: results are bit-reproducible, and
//     a column's result does not depend on the other columns.  Batch shards get the full batch's forward bits (every
//     configuration uses 8-step chunks); backward bits when the shard runs the same backward chunk length, otherwise
//     agreement within rounding (the streaming two-column backward uses 16-step chunks, every other one 8).
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <type_traits>

#include "colscan.hpp"
#include "hpc_rll_hip.h"
#include "masks.hpp"

namespace hpc_rll {
namespace {

// Forward Op: row t holds V_t, nv_t, r_t and the masks of step t; the stacked form takes nv_t from row t+1's V.
// NACC = 0: `finish` receives the kernel's one-element placeholder for the sums.
template <int MT, int MM, bool NVF, bool NTL>
struct MaskedGaeFwdOp {
    static constexpr int NACC = 0, DIAG_OP = HPC_RLL_SCAN_OP_GAE_MASKED_FWD, DIAG_MT = MT, DIAG_MM = MM, DIAG_NVF = NVF,
                         DIAG_NTL = NTL;
    static constexpr bool HD = has_done(MM), HF = has_flag(MM);
    const float* value; const float* next_value; const float* reward; const void* done; const void* flag;
    float* adv; int T, B; float gamma, gl;   // gl = gamma*lambda
    template <int V> struct Row { Pack<V> v0, v1, r; MaskRow<V, MT> md, mf; };

    template <int V> __device__ void init(long, bool, float (&carry)[V]) const {
#pragma unroll
        for (int k = 0; k < V; ++k) carry[k] = 0.f;
    }
    template <int V> __device__ void load(Row<V>& row, int t, long col, bool ok, bool next_in_regs) const {
        const size_t o = (size_t)t * B + (ok ? col : (long)B - V);
        row.v0 = load_pack<V, NTL>(value + o);
        if (NVF) row.v1 = load_pack<V, NTL>(next_value + o);
        else if (!next_in_regs) row.v1 = load_pack<V, NTL>(value + o + B);
        row.r = load_pack<V, NTL>(reward + o);
        if (HD) row.md.template load<NTL>(done, o);
        if (HF) row.mf.template load<NTL>(flag, o);
    }
    template <int V> __device__ void link(Row<V>& row, const Row<V>& nxt) const {
        if (!NVF) row.v1 = nxt.v0;
    }
    template <int V> __device__ void coeffs(const Row<V>& row, int, float (&a)[V], float (&b)[V]) const {
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const float gd = HD ? gamma * row.md.keep(k) : gamma;
            a[k] = HF ? gl * row.mf.keep(k) : (HD ? gl * row.md.keep(k) : gl);
            b[k] = fmaf(gd, row.v1.v[k], row.r.v[k]) - row.v0.v[k];
        }
    }
    template <int V> __device__ void finish(const Row<V>&, int t, long col, bool ok, const float (&s)[V],
                                            const float (&)[V], float (&)[1]) const {
        if (!ok) return;
        Pack<V> o;
#pragma unroll
        for (int k = 0; k < V; ++k) o.v[k] = s[k];
        store_pack<V, true>(adv + (size_t)t * B + col, o);
    }
};

// ------------------------------------------------------------------------------------------------
// backward: forward-time scan d_t = g_t + a_{t-1} d_{t-1}, chunks aligned to t = 0, wave 0 earliest.
// Mask row r of a chunk is time step t0 - 1 + r (r = 0 .. LC): a_{t-1} needs f_{t-1}, the value gradients need
// done_{t-1} (stacked) or done_t (next-value form).
// ------------------------------------------------------------------------------------------------
template <int V, int LC, int NW, bool HALF, bool NTL, int MT, int MM, bool NVF>
__global__ __launch_bounds__(NW * 64) void gae_masked_bwd_kernel(const float* __restrict__ grad_adv,
                                                                 const void* __restrict__ done,
                                                                 const void* __restrict__ flag,
                                                                 float* __restrict__ grad_value,
                                                                 float* __restrict__ grad_next_value,
                                                                 float* __restrict__ grad_reward, int T, int B,
                                                                 float gamma, float gl) {
    static_assert(!HALF || V == 1, "half-wave tiles hold one column per lane");
    constexpr bool HD = has_done(MM), HF = has_flag(MM);
    constexpr int NWV = HALF ? 2 * NW : NW;
    constexpr int TILE = HALF ? 32 : 64 * V;
    __shared__ float lds[4 * NWV * TILE];
    float* const s_l0 = lds;
    float* const s_p0 = lds + 2 * NWV * TILE;

    const int lane = threadIdx.x & 63;
    const int wr = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int cl = HALF ? (lane & 31) : lane;
    const int w = HALF ? 2 * wr + (lane >> 5) : wr;
    const long col = (long)blockIdx.x * TILE + (long)cl * V;
    const bool col_ok = col < (long)B;
    const long lcol = col_ok ? col : (long)B - V;

    float carry[V];
#pragma unroll
    for (int k = 0; k < V; ++k) carry[k] = 0.f;

    constexpr int SPAN = NWV * LC;
    const int n_iter = (T + SPAN - 1) / SPAN;

    for (int it = 0; it < n_iter; ++it) {
        const int t0 = (it * NWV + w) * LC;
        const int buf = it & 1;

        float L[LC][V];
        float Q[LC][V];
        MaskRow<V, MT> md[HD ? LC + 1 : 1], mf[HF ? LC : 1];
        auto body = [&](auto guard_) {
            constexpr bool GUARD = decltype(guard_)::value != 0;
            auto row = [&](int t) { return t < 0 ? 0 : ((GUARD && t > T - 1) ? T - 1 : t); };
            Pack<V> g[LC];
#pragma unroll
            for (int j = 0; j < LC; ++j) g[j] = load_pack<V, NTL>(grad_adv + (size_t)row(t0 + j) * B + lcol);
#pragma unroll
            for (int r = 0; r <= LC; ++r) {
                const size_t o = (size_t)row(t0 - 1 + r) * B + lcol;
                if (HD) md[r].template load<NTL>(done, o);
                if (HF && r < LC) mf[r].template load<NTL>(flag, o);
            }
            float a[V], q[V];
#pragma unroll
            for (int k = 0; k < V; ++k) { a[k] = 0.f; q[k] = 1.f; }
#pragma unroll
            for (int j = 0; j < LC; ++j) {
                const int t = t0 + j;
                if (!GUARD || t < T) {
                    const bool first = j == 0 && t0 == 0;   // a_{-1} = 0
#pragma unroll
                    for (int k = 0; k < V; ++k) {
                        const float kf = HF ? mf[j].keep(k) : (HD ? md[j].keep(k) : 1.f);
                        const float c = first ? 0.f : gl * kf;
                        a[k] = fmaf(c, a[k], g[j].v[k]);
                        q[k] *= c;
                    }
                }
#pragma unroll
                for (int k = 0; k < V; ++k) { L[j][k] = a[k]; Q[j][k] = q[k]; }
            }
        };
        if (t0 + LC <= T) body(std::integral_constant<int, 0>{});
        else body(std::integral_constant<int, 1>{});

#pragma unroll
        for (int k = 0; k < V; ++k) {
            s_l0[(buf * NWV + w) * TILE + cl * V + k] = L[LC - 1][k];
            s_p0[(buf * NWV + w) * TILE + cl * V + k] = Q[LC - 1][k];
        }
        __syncthreads();

        float A[V], Aw[V];
#pragma unroll
        for (int k = 0; k < V; ++k) { A[k] = carry[k]; Aw[k] = 0.f; }
#pragma unroll
        for (int u = 0; u < NWV; ++u) {
            if (u == w) {
#pragma unroll
                for (int k = 0; k < V; ++k) Aw[k] = A[k];
            }
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const int s = (buf * NWV + u) * TILE + cl * V + k;
                A[k] = fmaf(s_p0[s], A[k], s_l0[s]);
            }
        }
#pragma unroll
        for (int k = 0; k < V; ++k) carry[k] = A[k];

        if (col_ok) {
            float prev[V];   // d_{t-1} (0 before t = 0: the carry into the first chunk is zero)
#pragma unroll
            for (int k = 0; k < V; ++k) prev[k] = Aw[k];
#pragma unroll
            for (int j = 0; j < LC; ++j) {
                const int t = t0 + j;
                if (t < T) {
                    Pack<V> d, gv, gn;
#pragma unroll
                    for (int k = 0; k < V; ++k) {
                        d.v[k] = fmaf(Q[j][k], Aw[k], L[j][k]);
                        if (NVF) {
                            gv.v[k] = -d.v[k];
                            gn.v[k] = (HD ? gamma * md[j + 1].keep(k) : gamma) * d.v[k];
                        } else {
                            gv.v[k] = fmaf(HD ? gamma * md[j].keep(k) : gamma, prev[k], -d.v[k]);
                        }
                        prev[k] = d.v[k];
                    }
                    if (grad_reward) store_pack<V, true>(grad_reward + (size_t)t * B + col, d);
                    if (grad_value) store_pack<V, true>(grad_value + (size_t)t * B + col, gv);
                    if (NVF && grad_next_value) store_pack<V, true>(grad_next_value + (size_t)t * B + col, gn);
                    if (!NVF && grad_value && t == T - 1) {   // bootstrap row: dL/dV_T = gamma * k^d_{T-1} * d_{T-1}
                        Pack<V> last;
#pragma unroll
                        for (int k = 0; k < V; ++k) last.v[k] = (HD ? gamma * md[j + 1].keep(k) : gamma) * d.v[k];
                        store_pack<V, true>(grad_value + (size_t)T * B + col, last);
                    }
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// host side: configuration heuristic + dispatch
// ------------------------------------------------------------------------------------------------
// The instantiated launch configurations form a closed list (with_cfg below; no tune-table keys, no expert entry point):
//   streaming (one launch moves >= 300 MB): two columns per lane with nontemporal loads, 4 waves per workgroup; forward
//   8-step chunks, backward 16-step chunks (C2 in one process, backward (2,4,4) / (2,8,4) / (2,16,4): 200 / 152-159 /
//   134-143 us: profiles/r07_masked_gae_bwd_ab.txt); one column per lane for odd B;
//   cache-resident: one column per lane, 8-step chunks, up to 16 waves so that ~2048 waves cover the chip, half-wave
//   tiles when the 64-column tiling gives fewer than 256 workgroups and T has enough chunks.
// Depends on (T, B, vmax) only -- never on the input form or the mask dtype -- so that the stacked and the
// next-value form of the same problem run the same chunking and give the same bits.
inline int choose_cfg(int T, int B, int vmax) {
    const bool streaming = 13.0 * (double)T * (double)B >= 300e6;
    if (streaming) return vmax >= 2 ? 5 : 4;
    const int wgs = (B + 63) / 64;
    int nw = 4;
    while (nw < 16 && wgs * nw < 2048) nw <<= 1;
    if (nw == 16) return (wgs < 256 && T >= 512) ? 3 : 2;
    return nw == 8 ? 1 : 0;
}

// Calls f(I<V>, I<LC>, I<NW>, I<HALF>, I<NTL>) for entry `idx` of the configuration list.
template <bool FWD, class F>
inline void with_cfg(int idx, F&& f) {
    switch (idx) {
        case 0: f(I<1>{}, I<8>{}, I<4>{}, I<0>{}, I<0>{}); break;
        case 1: f(I<1>{}, I<8>{}, I<8>{}, I<0>{}, I<0>{}); break;
        case 2: f(I<1>{}, I<8>{}, I<16>{}, I<0>{}, I<0>{}); break;
        case 3: f(I<1>{}, I<8>{}, I<16>{}, I<1>{}, I<0>{}); break;
        case 4: f(I<1>{}, I<8>{}, I<8>{}, I<0>{}, I<1>{}); break;
        default:
            if constexpr (FWD) f(I<2>{}, I<8>{}, I<4>{}, I<0>{}, I<1>{});
            else f(I<2>{}, I<16>{}, I<4>{}, I<0>{}, I<1>{});
            break;
    }
}

// One scan launch of `op` in configuration (V, LC, NW, HALF); HALF: 32-column tiles, two half-waves per wave (SUB = 2).
template <int V, int LC, int NW, bool HALF, class Op>
inline void launch(const Op& op, int T, int B, hipStream_t st) {
    constexpr int TILE = HALF ? 32 : 64 * V;
    const unsigned grid = (unsigned)((B + TILE - 1) / TILE);
    hipLaunchKernelGGL((colscan_rev_kernel<Op, V, LC, NW, HALF ? 2 : 1>), dim3(grid), dim3(NW * 64), 0, st, op, T, B,
                       (float*)nullptr, ScanFold{});
    scan_note<Op, V, LC, NW, HALF ? 2 : 1>((long)grid);   // hpc_rll_scan_last_config: the instantiation just launched
}

}  // namespace
}  // namespace hpc_rll

using namespace hpc_rll;

extern "C" int hpc_rll_gae_masked_forward(const float* value, const float* next_value, const float* reward,
                                          const void* done, const void* traj_flag, int mask_dtype, float* adv, int T,
                                          int B, float gamma, float lambda, void* stream) {
    if (T < 0 || B < 0) return HPC_RLL_EINVAL;
    if (mask_dtype != HPC_RLL_MASK_U8 && mask_dtype != HPC_RLL_MASK_F32) return HPC_RLL_EINVAL;
    if (T == 0 || B == 0) return HPC_RLL_OK;
    if (!value || !reward || !adv) return HPC_RLL_EINVAL;
    if (!aligned(value, 4) || !aligned(next_value, 4) || !aligned(reward, 4) || !aligned(adv, 4)) return HPC_RLL_EALIGN;
    if (mask_dtype == HPC_RLL_MASK_F32 && (!aligned(done, 4) || !aligned(traj_flag, 4))) return HPC_RLL_EALIGN;
    int vmax = max_vec(B, mask_dtype, {value, next_value, reward, adv}, {done, traj_flag});
    int idx = choose_cfg(T, B, vmax);
    const float gl = gamma * lambda;
    hipStream_t st = (hipStream_t)stream;
    with_cfg<true>(idx, [&](auto V_, auto LC_, auto NW_, auto H_, auto N_) {
        with_mode(mask_dtype, mask_mode(done, traj_flag), next_value != nullptr, [&](auto MT_, auto MM_, auto NV_) {
            const MaskedGaeFwdOp<decltype(MT_)::value, decltype(MM_)::value, decltype(NV_)::value != 0,
                                 decltype(N_)::value != 0>
                op{value, next_value, reward, done, traj_flag, adv, T, B, gamma, gl};
            launch<decltype(V_)::value, decltype(LC_)::value, decltype(NW_)::value, decltype(H_)::value != 0>(op, T, B, st);
        });
    });
    return last_error();
}

extern "C" int hpc_rll_gae_masked_backward(const float* grad_adv, const void* done, const void* traj_flag,
                                           int mask_dtype, float* grad_value, float* grad_next_value,
                                           float* grad_reward, int stacked, int T, int B, float gamma, float lambda,
                                           void* stream) {
    if (T < 0 || B < 0 || (stacked != 0 && stacked != 1)) return HPC_RLL_EINVAL;
    if (mask_dtype != HPC_RLL_MASK_U8 && mask_dtype != HPC_RLL_MASK_F32) return HPC_RLL_EINVAL;
    if (stacked && grad_next_value) return HPC_RLL_EINVAL;   // the stacked form has no next_value input
    if (B == 0) return HPC_RLL_OK;
    if (T == 0) {   // stacked: grad_value has one row (the bootstrap value), which adv does not depend on
        if (stacked && grad_value)
            return (int)hipMemsetAsync(grad_value, 0, sizeof(float) * (size_t)B, (hipStream_t)stream);
        return HPC_RLL_OK;
    }
    if (!grad_adv) return HPC_RLL_EINVAL;
    if (!grad_value && !grad_next_value && !grad_reward) return HPC_RLL_OK;
    if (!aligned(grad_adv, 4) || !aligned(grad_value, 4) || !aligned(grad_next_value, 4) || !aligned(grad_reward, 4))
        return HPC_RLL_EALIGN;
    if (mask_dtype == HPC_RLL_MASK_F32 && (!aligned(done, 4) || !aligned(traj_flag, 4))) return HPC_RLL_EALIGN;
    int vmax = max_vec(B, mask_dtype, {grad_adv, grad_value, grad_next_value, grad_reward}, {done, traj_flag});
    int idx = choose_cfg(T, B, vmax);
    const float gl = gamma * lambda;
    hipStream_t st = (hipStream_t)stream;
    with_cfg<false>(idx, [&](auto V_, auto LC_, auto NW_, auto H_, auto N_) {
        constexpr int V = decltype(V_)::value, LC = decltype(LC_)::value, NW = decltype(NW_)::value;
        constexpr bool HALF = decltype(H_)::value != 0, NTL = decltype(N_)::value != 0;
        constexpr int TILE = HALF ? 32 : 64 * V;
        const unsigned grid = (unsigned)((B + TILE - 1) / TILE);
        with_mode(mask_dtype, mask_mode(done, traj_flag), !stacked, [&](auto MT_, auto MM_, auto NV_) {
            constexpr int MT = decltype(MT_)::value, MM = decltype(MM_)::value;
            constexpr bool NVF = decltype(NV_)::value != 0;
            hipLaunchKernelGGL((gae_masked_bwd_kernel<V, LC, NW, HALF, NTL, MT, MM, NVF>), dim3(grid), dim3(NW * 64), 0, st,
                               grad_adv, done, traj_flag, grad_value, grad_next_value, grad_reward, T, B, gamma, gl);
            scan_note_launch(HPC_RLL_SCAN_OP_GAE_MASKED_BWD, V, LC, NW, HALF ? 2 : 1, NTL, MT, MM, NVF, (long)grid);
        });
    });
    return last_error();
}
