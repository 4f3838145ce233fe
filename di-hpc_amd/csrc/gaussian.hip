// gaussian.hip -- PPO for diagonal-Gaussian policy heads (continuous actions) on gfx950: one forward and one backward launch.
//
// No reference counterpart: the reference's only PPO op takes a categorical head (ppo_kernel.h); DI-engine's
// ppo_error_continuous is the semantics.  With z_j = (a_j - mu_j) / sigma_j,
//   logp = sum_j [-z_j^2/2 - log sigma_j - log(2 pi)/2],   H = sum_j [1/2 + log(2 pi)/2 + log sigma_j]   (new policy)
// and from ratio = exp(logp_new - logp_old) onward the arithmetic is PpoOp::apply (ppo_op.hpp), shared with the categorical op.
//
// Mapping (rowgroup.hpp): a row of A values is owned by a GROUP of G lanes (G = 1..64, a power of two), lane gl holds a
// RowSlice -- E pieces of VEC consecutive floats, piece e at column (e*G + gl)*VEC -- of each of the five (B,A) inputs; R rows
// per group and iteration give R independent load + reduction chains: 5 (forward) or 3 (backward) inputs x R rows x E*VEC
// floats per lane stay within ~80 VGPRs.  A Gaussian row needs no maximum, so one pass forms the two sums.
//   * logp_new - logp_old is accumulated as a sum of PER-DIMENSION differences
//         (z_old - z_new)(z_old + z_new)/2 + (log sigma_old - log sigma_new):
//     log(2 pi) cancels and no two sums of size ~A are subtracted (torch's fp32 formula loses 7e-5 of max|grad_mu| at A = 376 to
//     that cancellation).  PpoOp::apply is called with that difference as logp_new and 0 as logp_old;
//   * sums over the group are the DPP butterflies of wave.hpp (no LDS, no barrier), the total is in the group's LAST lane, which
//     applies the per-sample arithmetic and keeps the five running sums; workgroup sums -> partials -> the last workgroup folds
//     them (colscan.hpp), exactly as ppo_fwd_fused_kernel does;
//   * every load is unconditional: padding lanes re-read column 0, idle groups re-read the last row;
//   * forward saves 3 floats per sample (coef_logp, coef_ent, gv_unit); backward RECOMPUTES z from mu_new, sigma_new, action:
//         grad_mu_j    = k1 z_j / sigma_j,   grad_sigma_j = (k1 (z_j^2 - 1) + k2) / sigma_j,
//         k1 = g_policy coef_logp,  k2 = g_ent coef_ent,   grad_value = g_value gv_unit (the group's last lane, same launch).
// No float atomics: results are bit-identical from run to run.
//
// Algorithmic HBM bytes per sample: forward 20 A + 16 (+4 weight, +4 value_old) read, 12 written;
//                                   backward 12 A + 12 read, 8 A + 4 written.
//
// V-trace for the same heads (hpc_rll_vtrace_continuous_*; DI-engine's vtrace_error_continuous_action is the semantics):
// gauss_heads_fwd_kernel is the head alone, for a PAIR of policies over one action.  Per row it writes logp of the target
// policy, its entropy and logp_b = logp_t - d, with d the same sum of per-dimension differences as above (identical policies
// give d = 0 and logp_b == logp_t bit for bit).  For V-trace it writes d itself in place of logp_b: logp_t is of size ~1.4 A, so
// logp_b rounded to fp32 would give d back only to half an ulp of logp_t (6e-5 at A = 1024), and the scan forms IS = exp(d).
// The three (T,B) arrays feed MaskedVtraceOp<.., LR> (scan_masked.hip); the backward is ppo_gauss_bwd_kernel with V-trace's saved
// coef_pg / coef_ent as c1 / c2 and no value output.  Bytes per row: 20 A read, 12 written; backward 12 A + 8 read, 8 A written.
#include <hip/hip_runtime.h>

#include "hpc_rll_hip.h"
#include "wave.hpp"
#include "colscan.hpp"
#include "heads.hpp"
#include "hostutil.hpp"
#include "ppo_op.hpp"
#include "rowgroup.hpp"

namespace hpc_rll {
namespace {

constexpr int kGaussMaxA = kRowTableMaxN;               // 64 lanes x 16 floats per lane and input
constexpr float kLn2 = 0.69314718055994530942f;
constexpr float kEntConst = 1.41893853320467274178f;    // 1/2 + log(2 pi)/2: entropy of a unit normal
constexpr float kHalfLn2Pi = 0.91893853320467274178f;   // log(2 pi)/2

// log sigma as log2: sigma > 0 is the caller's contract, the bare v_log_f32 is within 1 ulp
__device__ __forceinline__ float log2_(float s) { return __builtin_amdgcn_logf(s); }

template <int G, int VEC, int E>
__global__ __launch_bounds__(256) void ppo_gauss_fwd_kernel(const float* __restrict__ mu_new,
                                                            const float* __restrict__ sigma_new,
                                                            const float* __restrict__ mu_old,
                                                            const float* __restrict__ sigma_old,
                                                            const float* __restrict__ action, const PpoOp op, long rows,
                                                            int A, float* __restrict__ partials, const ScanFold fold) {
    constexpr int GPB = 256 / G;
    constexpr int R = RowsPerIter<VEC, E>::value;
    const int gl = threadIdx.x % G;
    const int gi = threadIdx.x / G;
    const bool full = A == G * VEC * E;   // uniform: no padding lanes
    const float hconst = (float)A * kEntConst;
    const long stride = (long)gridDim.x * GPB * R;
    float acc[PpoOp::NACC];
#pragma unroll
    for (int k = 0; k < PpoOp::NACC; ++k) acc[k] = 0.f;
    for (long bb = (long)blockIdx.x * GPB * R; bb < rows; bb += stride) {
        RowSlice<G, VEC, E> mn[R], sn[R], mo[R], so[R], ac[R];
        PpoOp::In in[R];
#pragma unroll
        for (int k = 0; k < R; ++k) {
            long row = bb + (long)k * GPB + gi;
            if (row >= rows) row = rows - 1;             // (re-reads the last row; the sample op below is guarded)
            const long off = row * (long)A;
            mn[k].load(mu_new + off, A, gl);
            sn[k].load(sigma_new + off, A, gl);
            mo[k].load(mu_old + off, A, gl);
            so[k].load(sigma_old + off, A, gl);
            ac[k].load(action + off, A, gl);
            in[k] = op.load(row);                        // (every lane: the same address per group, one request)
        }
#pragma unroll
        for (int k = 0; k < R; ++k) {
            float d = 0.f, h = 0.f;   // this lane's part of logp_new - logp_old and of sum log2 sigma_new
#pragma unroll
            for (int e = 0; e < E; ++e)
#pragma unroll
                for (int q = 0; q < VEC; ++q) {
                    const int i = e * VEC + q;
                    const bool ok = full || (e * G + gl) * VEC + q < A;
                    const float a = ac[k].x[i];
                    const float zn = (a - mn[k].x[i]) * __builtin_amdgcn_rcpf(sn[k].x[i]);
                    const float zo = (a - mo[k].x[i]) * __builtin_amdgcn_rcpf(so[k].x[i]);
                    const float ln = log2_(sn[k].x[i]), lo = log2_(so[k].x[i]);
                    const float t = fmaf(0.5f * (zo - zn), zo + zn, (lo - ln) * kLn2);
                    d += ok ? t : 0.f;
                    h += ok ? ln : 0.f;
                }
            d = group_sum_last<G>(d);
            h = group_sum_last<G>(h);
            const long row = bb + (long)k * GPB + gi;
            if (gl == G - 1 && row < rows) op.apply(row, in[k], d, fmaf(h, kLn2, hconst), 0.f, acc);
        }
    }
    publish_block_sums<PpoOp::NACC, 256>(acc, partials, fold);
}

// c1 / c2 / c3 = the forward's coef_logp / coef_ent / gv_unit; g_* device scalars (NULL = 1); any of the three outputs may be NULL
template <int G, int VEC, int E>
__global__ __launch_bounds__(256) void ppo_gauss_bwd_kernel(const float* __restrict__ mu_new,
                                                            const float* __restrict__ sigma_new,
                                                            const float* __restrict__ action, const float* __restrict__ c1,
                                                            const float* __restrict__ c2, const float* __restrict__ c3,
                                                            const float* __restrict__ g_p, const float* __restrict__ g_e,
                                                            const float* __restrict__ g_v, float* __restrict__ grad_mu,
                                                            float* __restrict__ grad_sigma, float* __restrict__ grad_value,
                                                            long rows, int A) {
    constexpr int GPB = 256 / G;
    constexpr int R = RowsPerIter<VEC, E>::value;
    const int gl = threadIdx.x % G;
    const int gi = threadIdx.x / G;
    const float u1 = g_p ? g_p[0] : 1.f;
    const float u2 = g_e ? g_e[0] : 1.f;
    const float u3 = (grad_value && g_v) ? g_v[0] : 1.f;
    const long stride = (long)gridDim.x * GPB * R;
    for (long bb = (long)blockIdx.x * GPB * R; bb < rows; bb += stride) {
        RowSlice<G, VEC, E> mn[R], sn[R], ac[R];
        float k1[R], k2[R], k3[R];
#pragma unroll
        for (int k = 0; k < R; ++k) {
            long row = bb + (long)k * GPB + gi;
            if (row >= rows) row = rows - 1;             // (re-reads the last row; the stores below are guarded)
            const long off = row * (long)A;
            mn[k].load(mu_new + off, A, gl);
            sn[k].load(sigma_new + off, A, gl);
            ac[k].load(action + off, A, gl);
            k1[k] = u1 * c1[row];
            k2[k] = u2 * c2[row];
            k3[k] = grad_value ? u3 * c3[row] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const long row = bb + (long)k * GPB + gi;
            if (row >= rows) continue;
            const long off = row * (long)A;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const int c0 = (e * G + gl) * VEC;
                float om[VEC], os[VEC];
#pragma unroll
                for (int q = 0; q < VEC; ++q) {
                    const int i = e * VEC + q;
                    const float inv = __builtin_amdgcn_rcpf(sn[k].x[i]);
                    const float z = (ac[k].x[i] - mn[k].x[i]) * inv;
                    om[q] = k1[k] * z * inv;
                    os[q] = fmaf(k1[k], fmaf(z, z, -1.f), k2[k]) * inv;
                }
                if (c0 < A) {
                    if (grad_mu) store_piece<VEC>(grad_mu + off + c0, om);
                    if (grad_sigma) store_piece<VEC>(grad_sigma + off + c0, os);
                }
            }
            if (grad_value && gl == G - 1) grad_value[row] = k3[k];
        }
    }
}

// The heads of two policies (t = target, b = behaviour) over one action, no loss: per row
//   logp_t = -q/2 - sum log sigma_t - A log(2 pi)/2 (q = sum z_t^2),  ent = A (1/2 + log(2 pi)/2) + sum log sigma_t,
//   logp_b = logp_t - d,  d = sum [(z_b - z_t)(z_b + z_t)/2 + (log sigma_b - log sigma_t)]  (the forward's difference above,
//   with z_b - z_t formed from sigma_t - sigma_b and mu_t - mu_b: an fp32 emulation leaves 3e-7 rms in d at A = 376 against
//   4e-6 from the difference of the two rounded z, which the V-trace policy loss inherits as a relative error);
//   with log_ratio the third output is d itself (what the V-trace scan takes: d loses nothing to the size of logp_t).
// Three sums per row, stored by the group's last lane; no LDS, no barrier, nothing accumulated across rows.
template <int G, int VEC, int E>
__global__ __launch_bounds__(256) void gauss_heads_fwd_kernel(const float* __restrict__ mu_t,
                                                              const float* __restrict__ sigma_t,
                                                              const float* __restrict__ mu_b,
                                                              const float* __restrict__ sigma_b,
                                                              const float* __restrict__ action, float* __restrict__ logp_t,
                                                              float* __restrict__ ent, float* __restrict__ logp_b,
                                                              const bool log_ratio, long rows, int A) {
    constexpr int GPB = 256 / G;
    constexpr int R = RowsPerIter<VEC, E>::value;
    const int gl = threadIdx.x % G;
    const int gi = threadIdx.x / G;
    const bool full = A == G * VEC * E;   // uniform: no padding lanes
    const float hconst = (float)A * kEntConst, lconst = (float)A * kHalfLn2Pi;
    const long stride = (long)gridDim.x * GPB * R;
    for (long bb = (long)blockIdx.x * GPB * R; bb < rows; bb += stride) {
        RowSlice<G, VEC, E> mt[R], st[R], mb[R], sb[R], ac[R];
#pragma unroll
        for (int k = 0; k < R; ++k) {
            long row = bb + (long)k * GPB + gi;
            if (row >= rows) row = rows - 1;             // (re-reads the last row; the stores below are guarded)
            const long off = row * (long)A;
            mt[k].load(mu_t + off, A, gl);
            st[k].load(sigma_t + off, A, gl);
            mb[k].load(mu_b + off, A, gl);
            sb[k].load(sigma_b + off, A, gl);
            ac[k].load(action + off, A, gl);
        }
#pragma unroll
        for (int k = 0; k < R; ++k) {
            float q = 0.f, h = 0.f, d = 0.f;   // this lane's part of sum z_t^2, sum log2 sigma_t and logp_t - logp_b
#pragma unroll
            for (int e = 0; e < E; ++e)
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    const int i = e * VEC + j;
                    const bool ok = full || (e * G + gl) * VEC + j < A;
                    const float a = ac[k].x[i];
                    const float rt = __builtin_amdgcn_rcpf(st[k].x[i]);
                    const float zt = (a - mt[k].x[i]) * rt;
                    const float zb = (a - mb[k].x[i]) * __builtin_amdgcn_rcpf(sb[k].x[i]);
                    const float lt = log2_(st[k].x[i]), lb = log2_(sb[k].x[i]);
                    // z_b - z_t = (z_b (sigma_t - sigma_b) + (mu_t - mu_b)) / sigma_t: from the small differences of the
                    // parameters, not from two rounded z of size ~1 (whose difference is good to 1e-7 |z| only)
                    const float dz = fmaf(zb, st[k].x[i] - sb[k].x[i], mt[k].x[i] - mb[k].x[i]) * rt;
                    const float t = fmaf(0.5f * dz, zb + zt, (lb - lt) * kLn2);
                    q += ok ? zt * zt : 0.f;
                    h += ok ? lt : 0.f;
                    d += ok ? t : 0.f;
                }
            q = group_sum_last<G>(q);
            h = group_sum_last<G>(h);
            d = group_sum_last<G>(d);
            const long row = bb + (long)k * GPB + gi;
            if (gl == G - 1 && row < rows) {
                const float lp = fmaf(-0.5f, q, -fmaf(h, kLn2, lconst));
                logp_t[row] = lp;
                ent[row] = fmaf(h, kLn2, hconst);
                logp_b[row] = log_ratio ? d : lp - d;
            }
        }
    }
}

int gauss_forward(const float* mu_new, const float* sigma_new, const float* mu_old, const float* sigma_old,
                  const float* action, const PpoOp& op, long rows, int A, float* partials, const float* scales, float* out5,
                  hipStream_t st) {
    const bool v4 = aligned(mu_new, 16) && aligned(sigma_new, 16) && aligned(mu_old, 16) && aligned(sigma_old, 16) &&
                    aligned(action, 16);
    return with_row4(row_cfg(A, v4, kRow4Pieces), [&](auto G_, auto V_, auto E_) {
        constexpr int G = G_, V = V_, E = E_;
        long grid = 0;
        return launch_rows_folded(rows, (256 / G) * RowsPerIter<V, E>::value, PpoOp::NACC, scales, out5, partials, st, &grid,
                                  [&](unsigned blocks, const ScanFold& fold) {
            hipLaunchKernelGGL((ppo_gauss_fwd_kernel<G, V, E>), dim3(blocks), dim3(256), 0, st, mu_new, sigma_new, mu_old,
                               sigma_old, action, op, rows, A, partials, fold);
        });
    });
}

int gauss_backward(const float* mu_new, const float* sigma_new, const float* action, const float* c1, const float* c2,
                   const float* c3, const float* g_p, const float* g_e, const float* g_v, float* grad_mu, float* grad_sigma,
                   float* grad_value, long rows, int A, hipStream_t st) {
    const bool v4 = aligned(mu_new, 16) && aligned(sigma_new, 16) && aligned(action, 16) && aligned(grad_mu, 16) &&
                    aligned(grad_sigma, 16);   // (a gradient that is not asked for restricts nothing)
    return with_row4(row_cfg(A, v4, kRow4Pieces), [&](auto G_, auto V_, auto E_) {
        constexpr int G = G_, V = V_, E = E_;
        const unsigned grid = row_grid(rows, (256 / G) * RowsPerIter<V, E>::value, kUnfoldedGridCap);
        hipLaunchKernelGGL((ppo_gauss_bwd_kernel<G, V, E>), dim3(grid), dim3(256), 0, st, mu_new, sigma_new, action, c1, c2,
                           c3, g_p, g_e, g_v, grad_mu, grad_sigma, grad_value, rows, A);
        return last_error();
    });
}

}  // namespace

// Internal C++ entry point used by scan_masked.hip (same library), as categorical_forward is: the head alone.
int gaussian_heads_forward(const float* mu_t, const float* sigma_t, const float* mu_b, const float* sigma_b,
                           const float* action, float* logp_t, float* ent, float* logp_b, bool log_ratio, long rows, int A,
                           hipStream_t st) {
    if (rows < 0 || A <= 0) return HPC_RLL_EINVAL;
    if (rows > 0 && (!mu_t || !sigma_t || !mu_b || !sigma_b || !action || !logp_t || !ent || !logp_b)) return HPC_RLL_EINVAL;
    for (const void* p : {(const void*)mu_t, (const void*)sigma_t, (const void*)mu_b, (const void*)sigma_b,
                          (const void*)action, (const void*)logp_t, (const void*)ent, (const void*)logp_b})
        if (!aligned(p, 4)) return HPC_RLL_EALIGN;
    if (A > kGaussMaxA) return HPC_RLL_EUNSUPPORTED;
    if (rows == 0) return HPC_RLL_OK;
    const bool v4 = aligned(mu_t, 16) && aligned(sigma_t, 16) && aligned(mu_b, 16) && aligned(sigma_b, 16) && aligned(action, 16);
    return with_row4(row_cfg(A, v4, kRow4Pieces), [&](auto G_, auto V_, auto E_) {
        constexpr int G = G_, V = V_, E = E_;
        const unsigned grid = row_grid(rows, (256 / G) * RowsPerIter<V, E>::value, kUnfoldedGridCap);
        hipLaunchKernelGGL((gauss_heads_fwd_kernel<G, V, E>), dim3(grid), dim3(256), 0, st, mu_t, sigma_t, mu_b, sigma_b,
                           action, logp_t, ent, logp_b, log_ratio, rows, A);
        return last_error();
    });
}

}  // namespace hpc_rll

using namespace hpc_rll;

// ws layout (floats): [coef_logp B | coef_ent B | gv_unit B | partials: 5 sums x at most kFoldMaxGrid workgroups]
extern "C" int64_t hpc_rll_ppo_continuous_workspace_floats(int B) {
    if (B < 0) return HPC_RLL_EINVAL;
    return 3 * (int64_t)B + 8 * (kFoldMaxGrid + 1);
}

extern "C" int hpc_rll_ppo_continuous_forward(const float* mu_new, const float* sigma_new, const float* mu_old,
                                              const float* sigma_old, const float* action, const float* value_new,
                                              const float* value_old, const float* adv, const float* ret,
                                              const float* weight, float* out5, float* ws, int B, int A, float clip_ratio,
                                              int use_value_clip, float dual_clip, float scale, void* stream) {
    if (B < 0 || A <= 0 || !out5) return HPC_RLL_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (B > 0 && (!mu_new || !sigma_new || !mu_old || !sigma_old || !action || !value_new || !value_old || !adv || !ret || !ws))
        return HPC_RLL_EINVAL;
    if (A > kGaussMaxA) return HPC_RLL_EUNSUPPORTED;
    if (B == 0) return (int)hipMemsetAsync(out5, 0, 5 * sizeof(float), st);
    float *coef_logp = ws, *coef_ent = ws + B, *gv_unit = ws + 2 * (size_t)B, *partials = ws + 3 * (size_t)B;
    const PpoOp op{nullptr, nullptr, nullptr, value_new, value_old, adv, ret, weight, coef_logp, coef_ent, gv_unit,
                   clip_ratio, dual_clip, scale, use_value_clip};
    // approx_kl and clipfrac are plain (unweighted) means over the LOCAL batch: scale by 1/B
    const float sc[5] = {scale, 0.5f * scale, scale, 1.f / (float)B, 1.f / (float)B};
    return gauss_forward(mu_new, sigma_new, mu_old, sigma_old, action, op, B, A, partials, sc, out5, st);
}

extern "C" int hpc_rll_ppo_continuous_backward(const float* g_policy, const float* g_value, const float* g_ent,
                                               const float* mu_new, const float* sigma_new, const float* action,
                                               const float* ws, float* grad_mu, float* grad_sigma, float* grad_value, int B,
                                               int A, void* stream) {
    if (B < 0 || A <= 0) return HPC_RLL_EINVAL;
    if (B > 0 && !ws) return HPC_RLL_EINVAL;
    if (B > 0 && (grad_mu || grad_sigma) && (!mu_new || !sigma_new || !action)) return HPC_RLL_EINVAL;
    if (A > kGaussMaxA) return HPC_RLL_EUNSUPPORTED;
    if (B == 0) return HPC_RLL_OK;
    hipStream_t st = (hipStream_t)stream;
    if (!grad_mu && !grad_sigma) {   // only the value head asks for a gradient: no row work
        if (!grad_value) return HPC_RLL_OK;
        if (!g_value) return HPC_RLL_EINVAL;
        return scale_rows(g_value, ws + 2 * (size_t)B, grad_value, B, B, st);
    }
    return gauss_backward(mu_new, sigma_new, action, ws, ws + B, ws + 2 * (size_t)B, g_policy, g_ent, g_value, grad_mu,
                          grad_sigma, grad_value, B, A, st);
}

extern "C" int hpc_rll_gaussian_forward(const float* mu, const float* sigma, const float* mu_b, const float* sigma_b,
                                        const float* action, float* logp, float* entropy, float* logp_b, int64_t rows,
                                        int A, void* stream) {
    return gaussian_heads_forward(mu, sigma, mu_b, sigma_b, action, logp, entropy, logp_b, /*log_ratio=*/false, (long)rows,
                                  A, (hipStream_t)stream);
}

// The forward (hpc_rll_vtrace_continuous_forward) is in scan_masked.hip, next to MaskedVtraceOp.  ws as hpc_rll_vtrace_forward:
// coef_pg at 0, coef_ent at T*B, gv_unit at 2*T*B.  grad_value is the STACKED form's (T+1,B), bootstrap row zeroed.
extern "C" int hpc_rll_vtrace_continuous_backward(const float* g_pg, const float* g_value, const float* g_ent,
                                                  const float* mu_target, const float* sigma_target, const float* action,
                                                  const float* ws, float* grad_mu, float* grad_sigma, float* grad_value,
                                                  int T, int B, int A, void* stream) {
    if (T < 0 || B < 0 || A <= 0) return HPC_RLL_EINVAL;
    const size_t TB = (size_t)T * B;
    const bool heads = TB && (grad_mu || grad_sigma);
    if (grad_value && (!g_value || (TB && !ws))) return HPC_RLL_EINVAL;
    if (heads && (!mu_target || !sigma_target || !action || !ws)) return HPC_RLL_EINVAL;
    for (const void* p : {(const void*)g_pg, (const void*)g_value, (const void*)g_ent, (const void*)mu_target,
                          (const void*)sigma_target, (const void*)action, (const void*)ws, (const void*)grad_mu,
                          (const void*)grad_sigma, (const void*)grad_value})
        if (!aligned(p, 4)) return HPC_RLL_EALIGN;
    if (A > kGaussMaxA) return HPC_RLL_EUNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    if (grad_value) {
        const int rc = scale_rows(g_value, ws + 2 * TB, grad_value, (long)TB, (long)TB + B, st);
        if (rc) return rc;
    }
    if (!heads) return HPC_RLL_OK;
    return gauss_backward(mu_target, sigma_target, action, ws, ws + TB, nullptr, g_pg, g_ent, nullptr, grad_mu, grad_sigma,
                          nullptr, (long)TB, A, st);
}
