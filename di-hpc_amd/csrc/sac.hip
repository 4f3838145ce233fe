// sac.hip -- Soft Actor-Critic for discrete actions on gfx950: the soft state value of the next state, the TD target, both
// critic losses, the policy loss, the entropy and the unit gradient of the logits in ONE forward launch; one streaming
// backward.
//
// No reference counterpart; the semantics restate DI-engine's DiscreteSACPolicy._forward_learn with q_v_1step_td_error.  Per
// sample b with x, y the rows of logit (actor at s) and next_logit (actor at s'), q1, q2 the online critics at s, r1, r2 the
// target critics at s', a = action, k = 1 - done (1 without done), w = weight (1 without), alpha the temperature:
//   l' = log_softmax(y)   p' = exp l'   m' = min(r1, r2)        V' = sum_n p'_n (m'_n - alpha l'_n)
//   G  = reward + gamma k V'                                      (a constant of every loss)
//   d_i = q_i[a] - G      critic_i = scale sum_b w d_i^2          td_error[b] = mean_i d_i^2      (unweighted)
//   l  = log_softmax(x)   p = exp l     m = min(q1, q2) (const)   t_n = alpha l_n - m_n            f = sum_n p_n t_n
//   policy = scale sum_b f               H = -sum_n p_n l_n       entropy = scale sum_b H          (a monitor)
//   unit[b,n]    = scale p_n (t_n - f)                            grad_logit = g_policy * unit
//   delta_i[b]   = 2 scale w d_i                                  grad_q_i[b,n] = g_i delta_i[b] [n = a]
// A single critic (q2 and target_q2 absent) has m = q1, m' = r1 and no second critic sum.
//
// Mapping (rowgroup.hpp): a row of N values is owned by a group of G lanes; lane gl holds a RowSlice of three rows at a time,
// R samples per group and iteration.  Six inputs of up to 16 floats per lane do not fit in registers at once, so a sample is
// two passes over the same code (softmax_pass): the next-state triple (y, r1, r2) leaves V', then the current-state triple (x,
// q1, q2) leaves f and, when the gradient is wanted, p and t in the registers of q1 and x.  Each pass is a group maximum and
// a group sum; l = (x - max) - log s in ONE expression from the row's statistics.  V' and the two selected q_i[a] are group
// sums (at most one lane holds a nonzero selected value); f is reduced over the group only when the gradient needs it.
// The four loss sums are kept per LANE over the samples it visits (f and H as the lane's part, the critic terms by lane 0 of
// a group), then per workgroup, and leave through publish_sums (colscan.hpp): partials in a fixed order, no float atomics,
// bit-identical from run to run.  The row work uses no LDS and no barrier; every load is unconditional and in bounds (padding
// lanes re-read column 0, idle groups the last row).  weight, done and its element type are uniform run-time branches around
// one scalar load per sample: a null weight multiplies by an exact 1 and a null done by k = 1, the same bits as all-ones /
// all-zero tensors.  alpha is read from the device when it is given as a pointer: no host synchronisation.
//
// -inf logits (masked actions) are clamped to the most negative finite float, as categorical.hip and acer.hip do.  Such a
// column has p_n = 0 and every sum SELECTS on p_n > 0 instead of multiplying: it adds exactly 0 to V', f and H and its
// gradient is 0, whatever the critics hold there (inf, NaN).  An action outside [0,N) matches no column: d_i = 0,
// td_error = 0 and delta_i = 0; the policy part of the sample is unaffected.  N = 1: l = 0, p = 1, f = t exactly and the
// unit gradient is identically zero.
//
// Algorithmic HBM bytes per sample, twin critics (single: 8 N less in the forward's reads):
//   gradient STORED by the forward (this file): forward 24 N read + 4 N written (+ 12 for action and reward, + 4 weight,
//     + 1 or 4 done; 16 written: td_error, target_q, delta_1, delta_2);  backward 4 N read, 4 N written for grad_logit and
//     4 N written per critic gradient (+ 8 action, + 8 delta).                    Sum for the logit gradient: 36 N.
//   gradient RECOMPUTED by the backward from saved (lse, f): forward 24 N read;  backward 12 N read (x, q1, q2), 4 N
//     written, and the exp / log-softmax work a second time.                      Sum for the logit gradient: 40 N.
// The stored form was chosen on these bytes (a tie at 28 N for a single critic); the two were not measured against each other.
// A forward whose logit needs no gradient stores nothing.
#include <hip/hip_runtime.h>

#include "colscan.hpp"
#include "hostutil.hpp"
#include "hpc_rll_hip.h"
#include "rowgroup.hpp"
#include "wave.hpp"

namespace hpc_rll {
namespace {

constexpr int kSacMaxN = kRowTableMaxN;   // 64 lanes x 16 floats per lane and input
constexpr int kSacSums = 4;               // the order of out4: policy, critic, twin critic, entropy

struct SacArgs {
    const float* logit; const float* next_logit; const float* q1; const float* q2; const float* tq1; const float* tq2;
    const int64_t* action; const float* reward; const void* done; int done_f32; const float* weight;
    const float* alpha_dev; float alpha;
    float* td_error; float* target_q; float* unit; float* delta1; float* delta2; long rows; int N; float gamma, scale;
};

// One softmax pass over a triple of slices: z the logits, c1 / c2 the critic rows (c2 unused without TWIN).  Returns the
// lane's part of sum_n p_n (sign (alpha l_n - m_n)) in `part` (sign = -1: the soft value's summand m - alpha l, formed as the
// exact negation) and of sum_n p_n l_n in `pl`.  With KEEP the slices are overwritten: z <- t = alpha l - m, c1 <- p.
template <int G, int VEC, int E, bool TWIN, bool KEEP>
__device__ __forceinline__ void softmax_pass(float* z, float* c1, const float* c2, int N, int gl, float alpha, float& part,
                                             float& pl) {
    const float mx = row_max_finite<G, VEC, E>(z, N, gl);
    // ---- partition sum; z <- z - max (clamped: finite)
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < E; ++e)
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const int i = e * VEC + j;
            const bool in = (e * G + gl) * VEC + j < N;
            z[i] = fmaxf(z[i], -kFltMax) - mx;
            s += in ? __expf(z[i]) : 0.f;
        }
    s = group_all<G, AddOp>(s);
    const float ls = logf(s);
    part = 0.f;
    pl = 0.f;
#pragma unroll
    for (int e = 0; e < E; ++e)
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const int i = e * VEC + j;
            const int c = (e * G + gl) * VEC + j;
            const float l = z[i] - ls;
            const float p = (c < N) ? expf(l) : 0.f;
            const bool sel = p > 0.f;
            const float m = TWIN ? fminf(c1[i], c2[i]) : c1[i];
            const float t = fmaf(alpha, l, -m);
            part += sel ? p * t : 0.f;
            pl += sel ? p * l : 0.f;
            if (KEEP) {
                z[i] = t;
                c1[i] = p;
            }
        }
}

// TWIN: q2 and target_q2 given; GRAD: the unit gradient row of logit is stored
template <int G, int VEC, int E, bool TWIN, bool GRAD>
__global__ __launch_bounds__(256) void sac_discrete_fwd_kernel(const SacArgs p, float* __restrict__ partials,
                                                               const ScanFold fold) {
    constexpr int GPB = 256 / G;
    constexpr int R = RowsPerIter<VEC, E>::value;
    const int gl = threadIdx.x % G;
    const int gi = threadIdx.x / G;
    const float alpha = p.alpha_dev ? p.alpha_dev[0] : p.alpha;
    const long stride = (long)gridDim.x * GPB * R;
    float acc[kSacSums];
#pragma unroll
    for (int k = 0; k < kSacSums; ++k) acc[k] = 0.f;
    for (long bb = (long)blockIdx.x * GPB * R; bb < p.rows; bb += stride) {
        // N is an opaque value in every iteration: the c < N predicates of up to 16 columns per lane are then formed inside
        // the iteration instead of being kept as 64-bit lane masks across the loop (up to 19 VGPRs and 10 scalar registers
        // kept in vector lanes less)
        int N = p.N;
        asm volatile("" : "+s"(N));
        float vnext[R];
        // ---- the next state: V' = sum p' (m' - alpha l')
        {
            RowSlice<G, VEC, E> ys[R], r1[R], r2[R];
#pragma unroll
            for (int k = 0; k < R; ++k) {
                long row = bb + (long)k * GPB + gi;
                if (row >= p.rows) row = p.rows - 1;       // (re-reads the last row; sums and stores below are guarded)
                const long off = row * (long)N;
                ys[k].load(p.next_logit + off, N, gl);
                r1[k].load(p.tq1 + off, N, gl);
                if (TWIN) r2[k].load(p.tq2 + off, N, gl);
            }
#pragma unroll
            for (int k = 0; k < R; ++k) {
                float part, pl;
                softmax_pass<G, VEC, E, TWIN, false>(ys[k].x, r1[k].x, TWIN ? r2[k].x : r1[k].x, N, gl, alpha, part, pl);
                vnext[k] = -group_all<G, AddOp>(part);
            }
        }
        // ---- the current state
        RowSlice<G, VEC, E> xs[R], q1[R], q2[R];
        long a[R];
        float rew[R], keep[R], wt[R];
#pragma unroll
        for (int k = 0; k < R; ++k) {
            long row = bb + (long)k * GPB + gi;
            if (row >= p.rows) row = p.rows - 1;
            const long off = row * (long)N;
            xs[k].load(p.logit + off, N, gl);
            q1[k].load(p.q1 + off, N, gl);
            if (TWIN) q2[k].load(p.q2 + off, N, gl);
            a[k] = p.action[row];                          // (every lane: the same address per group, one request)
            rew[k] = p.reward[row];
            wt[k] = p.weight ? p.weight[row] : 1.f;
            keep[k] = 1.f;
            if (p.done) {
                if (p.done_f32) keep[k] = 1.f - static_cast<const float*>(p.done)[row];
                else keep[k] = static_cast<const uint8_t*>(p.done)[row] ? 0.f : 1.f;
            }
        }
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const long row = bb + (long)k * GPB + gi;
            const bool live = row < p.rows;
            const int ai = action_index(a[k], N);
            // the selected critic values, before the slices are overwritten; at most one lane holds a nonzero value
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int e = 0; e < E; ++e)
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    const int c = (e * G + gl) * VEC + j;
                    s1 = (c == ai) ? q1[k].x[e * VEC + j] : s1;
                    if (TWIN) s2 = (c == ai) ? q2[k].x[e * VEC + j] : s2;
                }
            s1 = group_all<G, AddOp>(s1);
            if (TWIN) s2 = group_all<G, AddOp>(s2);
            float fpart, pl;
            softmax_pass<G, VEC, E, TWIN, GRAD>(xs[k].x, q1[k].x, TWIN ? q2[k].x : q1[k].x, N, gl, alpha, fpart, pl);
            const float tgt = fmaf(p.gamma * keep[k], vnext[k], rew[k]);
            const float d1 = ai >= 0 ? s1 - tgt : 0.f;
            const float d2 = (TWIN && ai >= 0) ? s2 - tgt : 0.f;
            const float wd1 = wt[k] * d1, wd2 = wt[k] * d2;
            if (live) {
                acc[0] += fpart;
                acc[3] -= pl;
                if (gl == 0) {
                    acc[1] = fmaf(wd1, d1, acc[1]);
                    if (TWIN) acc[2] = fmaf(wd2, d2, acc[2]);
                    p.td_error[row] = TWIN ? 0.5f * fmaf(d1, d1, d2 * d2) : d1 * d1;
                    p.target_q[row] = tgt;
                    p.delta1[row] = (2.f * wd1) * p.scale;
                    if (TWIN) p.delta2[row] = (2.f * wd2) * p.scale;
                }
            }
            if (!GRAD) continue;
            // ---- unit = scale p (t - f): xs holds t, q1 holds p
            const float f = group_all<G, AddOp>(fpart);
            float* out = p.unit + row * (long)N;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const int c0 = (e * G + gl) * VEC;
                float o[VEC];
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    const int i = e * VEC + j;
                    const float pn = q1[k].x[i];
                    o[j] = (pn > 0.f) ? (p.scale * pn) * (xs[k].x[i] - f) : 0.f;
                }
                if (live && c0 < N) store_piece<VEC>(out + c0, o);
            }
        }
    }
    publish_block_sums<kSacSums, 256>(acc, partials, fold);   // (the only LDS and barriers of the kernel)
}

// ================================================================================================
// backward: `rows` rows of N floats per wanted output, each float written once; no reduction, no atomics
// ================================================================================================
struct SacBwdArgs {
    const float* g_p; const float* g_1; const float* g_2; const float* unit; const int64_t* action; const float* delta1;
    const float* delta2; float* grad_logit; float* grad_q1; float* grad_q2; long rows; int N;
};

// GL: grad_logit wanted (the unit gradient is read); the critic gradients are uniform run-time branches
template <int G, int VEC, int E, bool GL>
__global__ __launch_bounds__(256) void sac_discrete_bwd_kernel(const SacBwdArgs p) {
    constexpr int GPB = 256 / G;
    constexpr int R = RowsPerIter<VEC, E>::value;
    const int gl = threadIdx.x % G;
    const int gi = threadIdx.x / G;
    const int N = p.N;
    const bool w1 = p.grad_q1 != nullptr, w2 = p.grad_q2 != nullptr;
    const float gp = (GL && p.g_p) ? p.g_p[0] : 1.f;
    const float g1 = (w1 && p.g_1) ? p.g_1[0] : 1.f;
    const float g2 = (w2 && p.g_2) ? p.g_2[0] : 1.f;
    const long stride = (long)gridDim.x * GPB * R;
    for (long bb = (long)blockIdx.x * GPB * R; bb < p.rows; bb += stride) {
        RowSlice<G, VEC, E> us[R];
        long a[R];
        float c1[R], c2[R];
#pragma unroll
        for (int k = 0; k < R; ++k) {
            long row = bb + (long)k * GPB + gi;
            if (row >= p.rows) row = p.rows - 1;           // (re-reads the last row; the stores below are guarded)
            if (GL) us[k].load(p.unit + row * (long)N, N, gl);
            a[k] = p.action[row];
            c1[k] = w1 ? g1 * p.delta1[row] : 0.f;
            c2[k] = w2 ? g2 * p.delta2[row] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const long row = bb + (long)k * GPB + gi;
            if (row >= p.rows) continue;
            const int ai = action_index(a[k], N);
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const int c0 = (e * G + gl) * VEC;
                if (c0 >= N) continue;
                const long o = row * (long)N + c0;
                // (not store_piece: with three outputs behind run-time branches that form measured slower, r18_rowgroup_share.txt)
                if (VEC == 4) {
                    vfloat4 t;
                    if (GL) {
                        t.x = gp * us[k].x[e * 4 + 0]; t.y = gp * us[k].x[e * 4 + 1];
                        t.z = gp * us[k].x[e * 4 + 2]; t.w = gp * us[k].x[e * 4 + 3];
                        __builtin_nontemporal_store(t, reinterpret_cast<vfloat4*>(p.grad_logit + o));
                    }
                    if (w1) {
                        t.x = (c0 + 0 == ai) ? c1[k] : 0.f; t.y = (c0 + 1 == ai) ? c1[k] : 0.f;
                        t.z = (c0 + 2 == ai) ? c1[k] : 0.f; t.w = (c0 + 3 == ai) ? c1[k] : 0.f;
                        __builtin_nontemporal_store(t, reinterpret_cast<vfloat4*>(p.grad_q1 + o));
                    }
                    if (w2) {
                        t.x = (c0 + 0 == ai) ? c2[k] : 0.f; t.y = (c0 + 1 == ai) ? c2[k] : 0.f;
                        t.z = (c0 + 2 == ai) ? c2[k] : 0.f; t.w = (c0 + 3 == ai) ? c2[k] : 0.f;
                        __builtin_nontemporal_store(t, reinterpret_cast<vfloat4*>(p.grad_q2 + o));
                    }
                } else {
                    if (GL) __builtin_nontemporal_store(gp * us[k].x[e], p.grad_logit + o);
                    if (w1) __builtin_nontemporal_store((c0 == ai) ? c1[k] : 0.f, p.grad_q1 + o);
                    if (w2) __builtin_nontemporal_store((c0 == ai) ? c2[k] : 0.f, p.grad_q2 + o);
                }
            }
        }
    }
}

// The dispatch records of the forward and the backward (hpc_rll_sac_discrete_last_config):
// {launches so far, G, VEC, E, R, flags, grid}
constexpr int kLaunchInts = 7;
LaunchRecord<kLaunchInts> g_sac_fwd, g_sac_bwd;

template <bool TWIN, bool GRAD>
int sac_forward(const SacArgs& p, float* partials, float* out4, hipStream_t st) {
    const bool v4 = aligned(p.logit, 16) && aligned(p.next_logit, 16) && aligned(p.q1, 16) && aligned(p.q2, 16) &&
                    aligned(p.tq1, 16) && aligned(p.tq2, 16) && aligned(p.unit, 16);   // (an absent operand restricts nothing)
    const float sc[kSacSums] = {p.scale, p.scale, p.scale, p.scale};
    const int flags = (p.weight ? 1 : 0) | (p.done ? (p.done_f32 ? 4 : 2) : 0) | (TWIN ? 8 : 0) | (GRAD ? 16 : 0);
    return with_row4(row_cfg(p.N, v4, kRow4Pieces), [&](auto G_, auto V_, auto E_) {
        constexpr int G = G_, V = V_, E = E_, R = RowsPerIter<V, E>::value;
        long grid = 0;
        const int rc = launch_rows_folded(p.rows, (256 / G) * R, kSacSums, sc, out4, partials, st, &grid,
                                          [&](unsigned blocks, const ScanFold& fold) {
            hipLaunchKernelGGL((sac_discrete_fwd_kernel<G, V, E, TWIN, GRAD>), dim3(blocks), dim3(256), 0, st, p, partials,
                               fold);
        });
        if (grid) g_sac_fwd.note({G, V, E, R, flags, (int)grid});
        return rc;
    });
}

template <bool GL>
int sac_backward(const SacBwdArgs& p, hipStream_t st) {
    // an absent operand restricts nothing; the unit gradient counts only when it is read
    const RowCfg cfg = row_cfg(p.N, aligned(GL ? p.unit : nullptr, 16) && aligned(p.grad_logit, 16) &&
                                        aligned(p.grad_q1, 16) && aligned(p.grad_q2, 16), kRow4Pieces);
    const int flags = (GL ? 1 : 0) | (p.grad_q1 ? 2 : 0) | (p.grad_q2 ? 4 : 0);
    return with_row4(cfg, [&](auto G_, auto V_, auto E_) {
        constexpr int G = G_, V = V_, E = E_, R = RowsPerIter<V, E>::value;
        const unsigned grid = row_grid(p.rows, (256 / G) * R, kUnfoldedGridCap);
        hipLaunchKernelGGL((sac_discrete_bwd_kernel<G, V, E, GL>), dim3(grid), dim3(256), 0, st, p);
        const int rc = last_error();
        if (!rc) g_sac_bwd.note({G, V, E, R, flags, (int)grid});
        return rc;
    });
}

// floats of the partial-sum region: kSacSums per workgroup of at most kFoldMaxGrid
constexpr int64_t kSacPartials = 8 * (kFoldMaxGrid + 1);

}  // namespace
}  // namespace hpc_rll

using namespace hpc_rll;

// ws (floats): delta_1 | delta_2 (rows each) | the partial sums
extern "C" int64_t hpc_rll_sac_discrete_workspace_floats(int64_t rows) {
    if (rows < 0 || rows > (INT64_MAX - kSacPartials) / 2) return HPC_RLL_EINVAL;
    return 2 * rows + kSacPartials;
}

extern "C" int hpc_rll_sac_discrete_forward(const float* logit, const float* next_logit, const float* q1, const float* q2,
                                            const float* target_q1, const float* target_q2, const int64_t* action,
                                            const float* reward, const void* done, int mask_dtype, const float* weight,
                                            const float* alpha_dev, float alpha, float* out4, float* td_error,
                                            float* target_q, float* unit_grad, float* ws, int64_t rows, int N, float gamma,
                                            float scale, void* stream) {
    const bool empty = rows == 0;
    if (!out4) return HPC_RLL_EINVAL;
    if (!empty && (!logit || !next_logit || !q1 || !target_q1 || !action || !reward || !td_error || !target_q || !ws))
        return HPC_RLL_EINVAL;
    if ((q2 == nullptr) != (target_q2 == nullptr)) return HPC_RLL_EINVAL;   // both critics of the twin or neither
    if (rows < 0 || N <= 0) return HPC_RLL_EINVAL;
    if (mask_dtype != HPC_RLL_MASK_U8 && mask_dtype != HPC_RLL_MASK_F32) return HPC_RLL_EINVAL;
    if (!aligned(logit, 4) || !aligned(next_logit, 4) || !aligned(q1, 4) || !aligned(q2, 4) || !aligned(target_q1, 4) ||
        !aligned(target_q2, 4) || !aligned(action, 8) || !aligned(reward, 4) ||
        !aligned(done, mask_dtype == HPC_RLL_MASK_F32 ? 4 : 1) || !aligned(weight, 4) || !aligned(alpha_dev, 4) ||
        !aligned(out4, 4) || !aligned(td_error, 4) || !aligned(target_q, 4) || !aligned(unit_grad, 4) || !aligned(ws, 4))
        return HPC_RLL_EALIGN;
    if (N > kSacMaxN) return HPC_RLL_EUNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    if (empty) return (int)hipMemsetAsync(out4, 0, kSacSums * sizeof(float), st);
    const SacArgs p{logit, next_logit, q1, q2, target_q1, target_q2, action, reward, done,
                    mask_dtype == HPC_RLL_MASK_F32 ? 1 : 0, weight, alpha_dev, alpha, td_error, target_q, unit_grad,
                    ws, ws + rows, (long)rows, N, gamma, scale};
    float* partials = ws + 2 * rows;
    if (q2) return unit_grad ? sac_forward<true, true>(p, partials, out4, st) : sac_forward<true, false>(p, partials, out4, st);
    return unit_grad ? sac_forward<false, true>(p, partials, out4, st) : sac_forward<false, false>(p, partials, out4, st);
}

extern "C" int hpc_rll_sac_discrete_backward(const float* g_policy, const float* g_critic, const float* g_twin,
                                             const float* unit_grad, const int64_t* action, const float* ws,
                                             float* grad_logit, float* grad_q1, float* grad_q2, int64_t rows, int N,
                                             void* stream) {
    const bool empty = rows == 0 || (!grad_logit && !grad_q1 && !grad_q2);
    if (!empty && (!action || !ws || (grad_logit && !unit_grad))) return HPC_RLL_EINVAL;
    if (rows < 0 || N <= 0) return HPC_RLL_EINVAL;
    if (!aligned(g_policy, 4) || !aligned(g_critic, 4) || !aligned(g_twin, 4) || !aligned(unit_grad, 4) ||
        !aligned(action, 8) || !aligned(ws, 4) || !aligned(grad_logit, 4) || !aligned(grad_q1, 4) || !aligned(grad_q2, 4))
        return HPC_RLL_EALIGN;
    if (N > kSacMaxN) return HPC_RLL_EUNSUPPORTED;
    if (empty) return HPC_RLL_OK;
    const SacBwdArgs p{g_policy, g_critic, g_twin, unit_grad, action, ws, ws + rows, grad_logit, grad_q1, grad_q2,
                       (long)rows, N};
    hipStream_t st = (hipStream_t)stream;
    return grad_logit ? sac_backward<true>(p, st) : sac_backward<false>(p, st);
}

extern "C" int hpc_rll_sac_discrete_last_config(int* out) {
    if (!out) return HPC_RLL_EINVAL;
    g_sac_fwd.read(out);
    g_sac_bwd.read(out + kLaunchInts);
    return HPC_RLL_OK;
}
static_assert(HPC_RLL_SAC_CONFIG_INTS == 2 * 7, "the layout documented in hpc_rll_hip.h");
