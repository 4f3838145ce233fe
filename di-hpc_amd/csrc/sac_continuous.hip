// sac_continuous.hip -- Soft Actor-Critic for continuous actions on gfx950: the tanh-squashed Gaussian head (a reparameterised
// sample and its log-probability, one launch each way) and the SAC losses over per-sample vectors (one launch each way).
//
// No reference counterpart; the semantics restate DI-engine's SACPolicy._forward_learn with q_v_1step_td_error.
//
// The head.  mu, sigma, eps: `rows` rows of A floats; eps is standard-normal noise and a constant of the op (no RNG here).
//   u_j  = mu_j + sigma_j eps_j,    a_j = tanh(u_j)                                                       -> action (rows,A)
//   logp = sum_j [ -eps_j^2/2 - log sigma_j - log(2 pi)/2 + 2|u_j| + 2 log1p(exp(-2|u_j|)) - 2 log 2 ]    -> log_prob (rows)
// The last three terms are -log(1 - tanh^2 u_j) exactly.  log_prob is formed from u, never from the rounded a: in fp32 a is
// exactly +-1 from |u| ~ 9, where log(1 - a^2) is -inf (DI-engine takes log(1 - a^2 + 1e-6) instead).  With t = exp(-2|u|),
// one v_exp, a = sign(u) (1 - t) / (1 + t) (one v_rcp; gfx950 has no tanh instruction) and log1p(t) = log(1 + t) with
// 1 + t in (1, 2] (one v_log; the other is log sigma).  t underflows to 0 from |u| ~ 44 and 1 +- t round to 1 from
// |u| ~ 8.7: a is then +-1 exactly and never exceeds 1 in magnitude.
// Backward, from the upstream g_a (rows,A) and g_l (rows), either of which may be absent (zero, not read):
//   gu_j = g_a_j (1 - a_j^2) + 2 g_l a_j,     grad_mu_j = gu_j,     grad_sigma_j = gu_j eps_j - g_l / sigma_j.
// It re-reads sigma, eps (for grad_sigma alone), the saved action and g_a; tanh is not recomputed; 1 - a^2 is one fma and is
// exactly 0 where a = +-1.
//
// Mapping of the head (rowgroup.hpp), that of gauss_heads_fwd_kernel / ppo_gauss_bwd_kernel: a row is owned by a group of G
// lanes, lane gl holds E pieces of VEC floats of each (rows,A) input, R rows per group and iteration.  Every load is
// unconditional (padding lanes re-read column 0, idle groups the last row), every store is guarded.  The row sum is a DPP
// butterfly (group_sum_last) and the group's last lane stores it; no LDS, no barrier, nothing accumulated across rows.
// Algorithmic HBM bytes per row: forward 12 A read, 4 A + 4 written; backward 16 A + 4 read, 8 A written.
//
// The losses.  One float per sample in every operand; k = 1 - done (1 without), w = weight (1 without):
//   m' = min(target_q1, target_q2)    G = reward + gamma k (m' - alpha next_log_prob)   (a constant; -> target_q)
//   d_i = q_i - G                     critic_i = scale sum w d_i^2                      td_error = mean_i d_i^2 (unweighted)
//   m  = min(new_q1, new_q2)          policy = scale sum (alpha log_prob - m)           entropy = -scale sum log_prob
//   grad_q_i = g_i 2 scale w d_i,     grad_log_prob = g_p alpha scale,                  grad_new_q_i = -g_p scale s_i
// with s_i = 1 for the strictly smaller critic, 0 for the other and 1/2 each at a tie (torch.minimum's rule).  Both minima
// propagate a NaN from either side, as torch.minimum does, and G = fma(gamma k, ., reward) keeps 0 * NaN = NaN: a NaN target
// critic poisons its row even when done = 1.  A thread per sample, at most kFoldMaxGrid workgroups which loop; the four sums
// leave through publish_block_sums (partials in a fixed order, the last workgroup folds them: no float atomics, bit-identical
// from run to run).  The forward leaves 2 scale w d_1, 2 scale w d_2 and s_1 per sample and (alpha scale, scale) once in the
// workspace; the backward scales them by the device scalars g_p, g_1, g_2 and writes only the gradients asked for.  The
// critic half (q*, target_q*, next_log_prob, reward, done, weight) and the actor half (log_prob, new_q*) may each be absent.
#include <hip/hip_runtime.h>

#include "colscan.hpp"
#include "hostutil.hpp"
#include "hpc_rll_hip.h"
#include "rowgroup.hpp"
#include "wave.hpp"

namespace hpc_rll {
namespace {

constexpr int kSacCMaxA = kRowTableMaxN;                // 64 lanes x 16 floats per lane and input
constexpr float kLn2 = 0.69314718055994530942f;
constexpr float kLog2e = 1.44269504088896340736f;
constexpr float kRowConst = 2.30523289432456335062f;    // log(2 pi)/2 + 2 log 2: what every dimension subtracts

// ================================================================================================
// the head
// ================================================================================================
template <int G, int VEC, int E>
__global__ __launch_bounds__(256) void tanh_gauss_fwd_kernel(const float* __restrict__ mu, const float* __restrict__ sigma,
                                                             const float* __restrict__ eps, float* __restrict__ action,
                                                             float* __restrict__ logp, long rows, int A) {
    constexpr int GPB = 256 / G;
    constexpr int R = RowsPerIter<VEC, E>::value;
    const int gl = threadIdx.x % G;
    const int gi = threadIdx.x / G;
    const bool full = A == G * VEC * E;   // uniform: no padding lanes
    const long stride = (long)gridDim.x * GPB * R;
    for (long bb = (long)blockIdx.x * GPB * R; bb < rows; bb += stride) {
        RowSlice<G, VEC, E> m[R], s[R], n[R];
#pragma unroll
        for (int k = 0; k < R; ++k) {
            long row = bb + (long)k * GPB + gi;
            if (row >= rows) row = rows - 1;             // (re-reads the last row; the stores below are guarded)
            const long off = row * (long)A;
            m[k].load(mu + off, A, gl);
            s[k].load(sigma + off, A, gl);
            n[k].load(eps + off, A, gl);
        }
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const long row = bb + (long)k * GPB + gi;
            const bool live = row < rows;
            float* out = action + row * (long)A;
            // This lane's part of log_prob, whole terms: the constant is subtracted per dimension and the two logarithms
            // are added per dimension, so the running sum is of the size of log_prob itself.  (Sums of 2|u| - eps^2/2 and of
            // the logarithms kept apart and A (log(2 pi)/2 + 2 log 2) subtracted at the end cancel three numbers of size
            // ~2.3 A: an fp32 emulation of that form left 1e-5 in log_prob at A = 64, this one 2e-6.)
            float lp = 0.f;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const int c0 = (e * G + gl) * VEC;
                float o[VEC];
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    const int i = e * VEC + j;
                    const bool ok = full || c0 + j < A;
                    const float z = n[k].x[i];
                    const float u = fmaf(s[k].x[i], z, m[k].x[i]);
                    const float au = fabsf(u);
                    const float t = __builtin_amdgcn_exp2f(au * (-2.f * kLog2e));
                    o[j] = copysignf((1.f - t) * __builtin_amdgcn_rcpf(1.f + t), u);
                    const float a = fmaf(-0.5f * z, z, fmaf(2.f, au, -kRowConst));
                    const float b = fmaf(2.f, __builtin_amdgcn_logf(1.f + t), -__builtin_amdgcn_logf(s[k].x[i]));
                    lp += ok ? fmaf(b, kLn2, a) : 0.f;
                }
                if (live && c0 < A) store_piece<VEC>(out + c0, o);
            }
            lp = group_sum_last<G>(lp);
            if (gl == G - 1 && live) logp[row] = lp;
        }
    }
}

// g_a / g_l may be NULL (zero, not read); grad_mu / grad_sigma may be NULL (not formed; sigma and eps are read for
// grad_sigma alone): uniform run-time branches
template <int G, int VEC, int E>
__global__ __launch_bounds__(256) void tanh_gauss_bwd_kernel(const float* __restrict__ g_a, const float* __restrict__ g_l,
                                                             const float* __restrict__ sigma, const float* __restrict__ eps,
                                                             const float* __restrict__ action, float* __restrict__ grad_mu,
                                                             float* __restrict__ grad_sigma, long rows, int A) {
    constexpr int GPB = 256 / G;
    constexpr int R = RowsPerIter<VEC, E>::value;
    const int gl = threadIdx.x % G;
    const int gi = threadIdx.x / G;
    const long stride = (long)gridDim.x * GPB * R;
    for (long bb = (long)blockIdx.x * GPB * R; bb < rows; bb += stride) {
        RowSlice<G, VEC, E> s[R], n[R], ac[R], ga[R];
        float gl_[R];
#pragma unroll
        for (int k = 0; k < R; ++k) {
            long row = bb + (long)k * GPB + gi;
            if (row >= rows) row = rows - 1;             // (re-reads the last row; the stores below are guarded)
            const long off = row * (long)A;
            ac[k].load(action + off, A, gl);
            if (g_a) ga[k].load(g_a + off, A, gl);
            if (grad_sigma) {
                s[k].load(sigma + off, A, gl);
                n[k].load(eps + off, A, gl);
            }
            gl_[k] = g_l ? g_l[row] : 0.f;               // (every lane: the same address per group, one request)
        }
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const long row = bb + (long)k * GPB + gi;
            if (row >= rows) continue;
            const long off = row * (long)A;
            const float two_gl = 2.f * gl_[k];
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const int c0 = (e * G + gl) * VEC;
                float om[VEC], os[VEC];
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    const int i = e * VEC + j;
                    const float a = ac[k].x[i];
                    float gu = two_gl * a;
                    if (g_a) gu = fmaf(ga[k].x[i], fmaf(-a, a, 1.f), gu);   // (1 - a^2 is exactly 0 at a = +-1)
                    om[j] = gu;
                    os[j] = grad_sigma ? fmaf(gu, n[k].x[i], -gl_[k] * __builtin_amdgcn_rcpf(s[k].x[i])) : 0.f;
                }
                if (c0 < A) {
                    if (grad_mu) store_piece<VEC>(grad_mu + off + c0, om);
                    if (grad_sigma) store_piece<VEC>(grad_sigma + off + c0, os);
                }
            }
        }
    }
}

// ================================================================================================
// the losses
// ================================================================================================
constexpr int kSacCSums = 4;                                   // the order of out4: policy, critic, twin critic, entropy
constexpr int64_t kSacCPartials = 8 * (kFoldMaxGrid + 1);      // floats of the partial-sum region
constexpr int64_t kSacCConsts = kSacCSums * kFoldMaxGrid;      // (alpha scale, scale) behind the partials, inside that region
static_assert(kSacCConsts + 2 <= kSacCPartials, "the two constants lie inside the partial-sum region");

struct SacCArgs {
    const float* q1; const float* q2; const float* tq1; const float* tq2; const float* nlp; const float* reward;
    const void* done; int done_f32; const float* weight; const float* lp; const float* nq1; const float* nq2;
    const float* alpha_dev; float alpha;
    float* td_error; float* target_q; float* unit1; float* unit2; float* s1; float* consts; long rows; float gamma, scale;
};

// the smaller of a and b, a NaN from either side (torch.minimum)
__device__ __forceinline__ float min_nan(float a, float b) { return (a < b || a != a) ? a : b; }

__global__ __launch_bounds__(256) void sac_continuous_fwd_kernel(const SacCArgs p, float* __restrict__ partials,
                                                                 const ScanFold fold) {
    const float alpha = p.alpha_dev ? p.alpha_dev[0] : p.alpha;
    const bool critic = p.q1 != nullptr, actor = p.lp != nullptr;
    const bool twin_c = p.q2 != nullptr, twin_a = p.nq2 != nullptr;
    float acc[kSacCSums];
#pragma unroll
    for (int k = 0; k < kSacCSums; ++k) acc[k] = 0.f;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        p.consts[0] = alpha * p.scale;
        p.consts[1] = p.scale;
    }
    const long stride = (long)gridDim.x * 256;
    for (long row = (long)blockIdx.x * 256 + threadIdx.x; row < p.rows; row += stride) {
        if (critic) {
            const float q1 = p.q1[row], r1 = p.tq1[row], nl = p.nlp[row], rew = p.reward[row];
            const float q2 = twin_c ? p.q2[row] : 0.f, r2 = twin_c ? p.tq2[row] : 0.f;
            const float wt = p.weight ? p.weight[row] : 1.f;
            float keep = 1.f;
            if (p.done) {
                if (p.done_f32) keep = 1.f - static_cast<const float*>(p.done)[row];
                else keep = static_cast<const uint8_t*>(p.done)[row] ? 0.f : 1.f;
            }
            const float mt = twin_c ? min_nan(r1, r2) : r1;
            const float tgt = fmaf(p.gamma * keep, fmaf(-alpha, nl, mt), rew);
            const float d1 = q1 - tgt, d2 = twin_c ? q2 - tgt : 0.f;
            const float wd1 = wt * d1, wd2 = wt * d2;
            acc[1] = fmaf(wd1, d1, acc[1]);
            if (twin_c) acc[2] = fmaf(wd2, d2, acc[2]);
            p.td_error[row] = twin_c ? 0.5f * fmaf(d1, d1, d2 * d2) : d1 * d1;
            p.target_q[row] = tgt;
            p.unit1[row] = (2.f * wd1) * p.scale;
            if (twin_c) p.unit2[row] = (2.f * wd2) * p.scale;
        }
        if (actor) {
            const float lp = p.lp[row], n1 = p.nq1[row];
            float m = n1, s = 1.f;
            if (twin_a) {
                const float n2 = p.nq2[row];
                m = min_nan(n1, n2);
                s = n1 < n2 ? 1.f : (n1 == n2 ? 0.5f : 0.f);
            }
            acc[0] += fmaf(alpha, lp, -m);
            acc[3] -= lp;
            p.s1[row] = s;
        }
    }
    publish_block_sums<kSacCSums, 256>(acc, partials, fold);
}

struct SacCBwdArgs {
    const float* g_p; const float* g_1; const float* g_2; const float* unit1; const float* unit2; const float* s1;
    const float* consts; float* grad_q1; float* grad_q2; float* grad_lp; float* grad_nq1; float* grad_nq2; long rows;
};

// every given output written once per sample; the gradients that are not asked for are uniform run-time branches
__global__ __launch_bounds__(256) void sac_continuous_bwd_kernel(const SacCBwdArgs p) {
    const float gp = p.g_p ? p.g_p[0] : 1.f;
    const float g1 = (p.grad_q1 && p.g_1) ? p.g_1[0] : 1.f;
    const float g2 = (p.grad_q2 && p.g_2) ? p.g_2[0] : 1.f;
    const float glp = gp * p.consts[0], gs = gp * p.consts[1];
    const long stride = (long)gridDim.x * 256;
    for (long row = (long)blockIdx.x * 256 + threadIdx.x; row < p.rows; row += stride) {
        if (p.grad_q1) p.grad_q1[row] = g1 * p.unit1[row];
        if (p.grad_q2) p.grad_q2[row] = g2 * p.unit2[row];
        if (p.grad_lp) p.grad_lp[row] = glp;
        if (p.grad_nq1 || p.grad_nq2) {
            const float s = p.s1[row];
            if (p.grad_nq1) p.grad_nq1[row] = -(gs * s);
            if (p.grad_nq2) p.grad_nq2[row] = -(gs * (1.f - s));
        }
    }
}

// The dispatch records (hpc_rll_sac_continuous_last_config): {launches so far, G, VEC, E, R, flags, grid} of the head
// forward, the head backward, the loss forward and the loss backward
constexpr int kLaunchInts = 7;
LaunchRecord<kLaunchInts> g_head_fwd, g_head_bwd, g_loss_fwd, g_loss_bwd;

}  // namespace
}  // namespace hpc_rll

using namespace hpc_rll;

extern "C" int hpc_rll_tanh_gaussian_rsample_forward(const float* mu, const float* sigma, const float* eps, float* action,
                                                     float* log_prob, int64_t rows, int A, void* stream) {
    if (rows > 0 && (!mu || !sigma || !eps || !action || !log_prob)) return HPC_RLL_EINVAL;
    if (rows < 0 || A <= 0) return HPC_RLL_EINVAL;
    if (!aligned(mu, 4) || !aligned(sigma, 4) || !aligned(eps, 4) || !aligned(action, 4) || !aligned(log_prob, 4))
        return HPC_RLL_EALIGN;
    if (A > kSacCMaxA) return HPC_RLL_EUNSUPPORTED;
    if (rows == 0) return HPC_RLL_OK;
    hipStream_t st = (hipStream_t)stream;
    const bool v4 = aligned(mu, 16) && aligned(sigma, 16) && aligned(eps, 16) && aligned(action, 16);
    return with_row4(row_cfg(A, v4, kRow4Pieces), [&](auto G_, auto V_, auto E_) {
        constexpr int G = G_, V = V_, E = E_, R = RowsPerIter<V, E>::value;
        const unsigned grid = row_grid(rows, (256 / G) * R, kUnfoldedGridCap);
        hipLaunchKernelGGL((tanh_gauss_fwd_kernel<G, V, E>), dim3(grid), dim3(256), 0, st, mu, sigma, eps, action, log_prob,
                           (long)rows, A);
        const int rc = last_error();
        if (!rc) g_head_fwd.note({G, V, E, R, 0, (int)grid});
        return rc;
    });
}

extern "C" int hpc_rll_tanh_gaussian_rsample_backward(const float* g_action, const float* g_log_prob, const float* sigma,
                                                      const float* eps, const float* action, float* grad_mu,
                                                      float* grad_sigma, int64_t rows, int A, void* stream) {
    const bool empty = rows == 0 || (!grad_mu && !grad_sigma);
    if (!empty && (!action || (grad_sigma && (!sigma || !eps)))) return HPC_RLL_EINVAL;
    if (rows < 0 || A <= 0) return HPC_RLL_EINVAL;
    if (!aligned(g_action, 4) || !aligned(g_log_prob, 4) || !aligned(sigma, 4) || !aligned(eps, 4) || !aligned(action, 4) ||
        !aligned(grad_mu, 4) || !aligned(grad_sigma, 4))
        return HPC_RLL_EALIGN;
    if (A > kSacCMaxA) return HPC_RLL_EUNSUPPORTED;
    if (empty) return HPC_RLL_OK;
    hipStream_t st = (hipStream_t)stream;
    // a gradient that is not asked for restricts nothing; sigma and eps count only when they are read
    const bool v4 = aligned(action, 16) && aligned(g_action, 16) && aligned(grad_mu, 16) && aligned(grad_sigma, 16) &&
                    (!grad_sigma || (aligned(sigma, 16) && aligned(eps, 16)));
    const int flags = (g_action ? 1 : 0) | (g_log_prob ? 2 : 0) | (grad_mu ? 4 : 0) | (grad_sigma ? 8 : 0);
    return with_row4(row_cfg(A, v4, kRow4Pieces), [&](auto G_, auto V_, auto E_) {
        constexpr int G = G_, V = V_, E = E_, R = RowsPerIter<V, E>::value;
        const unsigned grid = row_grid(rows, (256 / G) * R, kUnfoldedGridCap);
        hipLaunchKernelGGL((tanh_gauss_bwd_kernel<G, V, E>), dim3(grid), dim3(256), 0, st, g_action, g_log_prob, sigma, eps,
                           action, grad_mu, grad_sigma, (long)rows, A);
        const int rc = last_error();
        if (!rc) g_head_bwd.note({G, V, E, R, flags, (int)grid});
        return rc;
    });
}

// ws (floats): unit_1 | unit_2 | s_1 (rows each) | the partial sums, with (alpha scale, scale) behind them
extern "C" int64_t hpc_rll_sac_continuous_workspace_floats(int64_t rows) {
    if (rows < 0 || rows > (INT64_MAX - kSacCPartials) / 3) return HPC_RLL_EINVAL;
    return 3 * rows + kSacCPartials;
}

extern "C" int hpc_rll_sac_continuous_forward(const float* q1, const float* q2, const float* target_q1,
                                              const float* target_q2, const float* next_log_prob, const float* reward,
                                              const void* done, int mask_dtype, const float* weight, const float* log_prob,
                                              const float* new_q1, const float* new_q2, const float* alpha_dev, float alpha,
                                              float* out4, float* td_error, float* target_q, float* ws, int64_t rows,
                                              float gamma, float scale, void* stream) {
    const bool empty = rows == 0;
    const bool critic = q1 != nullptr, actor = log_prob != nullptr;
    if (!out4) return HPC_RLL_EINVAL;
    if (!empty) {
        if (critic && (!target_q1 || !next_log_prob || !reward || !td_error || !target_q)) return HPC_RLL_EINVAL;
        if (actor && !new_q1) return HPC_RLL_EINVAL;
        if (!ws) return HPC_RLL_EINVAL;
    }
    // the second critics of the halves that are given: all or none; none for a half that is absent
    if ((q2 == nullptr) != (target_q2 == nullptr)) return HPC_RLL_EINVAL;
    if (!empty && ((!critic && q2) || (!actor && new_q2))) return HPC_RLL_EINVAL;
    if (critic && actor && (q2 == nullptr) != (new_q2 == nullptr)) return HPC_RLL_EINVAL;
    if (!empty && !critic && !actor) return HPC_RLL_EINVAL;
    if (rows < 0) return HPC_RLL_EINVAL;
    if (mask_dtype != HPC_RLL_MASK_U8 && mask_dtype != HPC_RLL_MASK_F32) return HPC_RLL_EINVAL;
    if (!aligned(q1, 4) || !aligned(q2, 4) || !aligned(target_q1, 4) || !aligned(target_q2, 4) || !aligned(next_log_prob, 4) ||
        !aligned(reward, 4) || !aligned(done, mask_dtype == HPC_RLL_MASK_F32 ? 4 : 1) || !aligned(weight, 4) ||
        !aligned(log_prob, 4) || !aligned(new_q1, 4) || !aligned(new_q2, 4) || !aligned(alpha_dev, 4) || !aligned(out4, 4) ||
        !aligned(td_error, 4) || !aligned(target_q, 4) || !aligned(ws, 4))
        return HPC_RLL_EALIGN;
    hipStream_t st = (hipStream_t)stream;
    if (empty) return (int)hipMemsetAsync(out4, 0, kSacCSums * sizeof(float), st);
    float* partials = ws + 3 * rows;
    const SacCArgs p{q1, q2, target_q1, target_q2, next_log_prob, reward, critic ? done : nullptr,
                     mask_dtype == HPC_RLL_MASK_F32 ? 1 : 0, critic ? weight : nullptr, log_prob, new_q1, new_q2, alpha_dev,
                     alpha, td_error, target_q, ws, ws + rows, ws + 2 * rows, partials + kSacCConsts, (long)rows, gamma,
                     scale};
    const float sc[kSacCSums] = {scale, scale, scale, scale};
    const int flags = (p.weight ? 1 : 0) | (p.done ? (p.done_f32 ? 4 : 2) : 0) | ((q2 || new_q2) ? 8 : 0) |
                      (critic ? 16 : 0) | (actor ? 32 : 0) | (alpha_dev ? 64 : 0);
    long grid = 0;
    const int rc = launch_rows_folded(rows, 256, kSacCSums, sc, out4, partials, st, &grid,
                                      [&](unsigned blocks, const ScanFold& fold) {
        hipLaunchKernelGGL(sac_continuous_fwd_kernel, dim3(blocks), dim3(256), 0, st, p, partials, fold);
    });
    if (grid) g_loss_fwd.note({0, 0, 0, 0, flags, (int)grid});
    return rc;
}

extern "C" int hpc_rll_sac_continuous_backward(const float* g_policy, const float* g_critic, const float* g_twin,
                                               const float* ws, float* grad_q1, float* grad_q2, float* grad_log_prob,
                                               float* grad_new_q1, float* grad_new_q2, int64_t rows, void* stream) {
    const bool empty = rows == 0 || (!grad_q1 && !grad_q2 && !grad_log_prob && !grad_new_q1 && !grad_new_q2);
    if (!empty && !ws) return HPC_RLL_EINVAL;
    if (rows < 0) return HPC_RLL_EINVAL;
    if (!aligned(g_policy, 4) || !aligned(g_critic, 4) || !aligned(g_twin, 4) || !aligned(ws, 4) || !aligned(grad_q1, 4) ||
        !aligned(grad_q2, 4) || !aligned(grad_log_prob, 4) || !aligned(grad_new_q1, 4) || !aligned(grad_new_q2, 4))
        return HPC_RLL_EALIGN;
    if (empty) return HPC_RLL_OK;
    hipStream_t st = (hipStream_t)stream;
    const SacCBwdArgs p{g_policy, g_critic, g_twin, ws, ws + rows, ws + 2 * rows, ws + 3 * rows + kSacCConsts, grad_q1,
                        grad_q2, grad_log_prob, grad_new_q1, grad_new_q2, (long)rows};
    const int flags = (grad_q1 ? 1 : 0) | (grad_q2 ? 2 : 0) | (grad_log_prob ? 4 : 0) | (grad_new_q1 ? 8 : 0) |
                      (grad_new_q2 ? 16 : 0);
    const unsigned grid = row_grid(rows, 256, kUnfoldedGridCap);
    hipLaunchKernelGGL(sac_continuous_bwd_kernel, dim3(grid), dim3(256), 0, st, p);
    const int rc = last_error();
    if (!rc) g_loss_bwd.note({0, 0, 0, 0, flags, (int)grid});
    return rc;
}

extern "C" int hpc_rll_sac_continuous_last_config(int* out) {
    if (!out) return HPC_RLL_EINVAL;
    g_head_fwd.read(out);
    g_head_bwd.read(out + kLaunchInts);
    g_loss_fwd.read(out + 2 * kLaunchInts);
    g_loss_bwd.read(out + 3 * kLaunchInts);
    return HPC_RLL_OK;
}
static_assert(HPC_RLL_SAC_CONTINUOUS_CONFIG_INTS == 4 * 7, "the layout documented in hpc_rll_hip.h");
