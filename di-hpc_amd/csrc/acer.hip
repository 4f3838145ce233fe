// acer.hip -- ACER's actor loss for discrete actions on gfx950: truncated importance sampling, bias correction, entropy bonus
// and the trust-region projection against an average policy, with the chain through log_softmax, in ONE forward launch.
//
// No reference counterpart; the semantics restate DI-engine's acer_policy_error and acer_trust_region_update.  Per sample
// (t,b), t < T, with x, y, u the rows of target_output, behaviour_output, avg_output (logits), q the row of q_values,
// a = action, l = log_softmax(x), pi = exp l, d_n = l_n - log_softmax(y)_n, k = softmax(u), A^ret = q_retraces - v_pred,
// A_n = q_n - v_pred, c = c_clip_ratio, beta = entropy_weight, delta = trust_region_value:
//   ca   = min(c, exp d_a) A^ret                          bc_n = max(0, 1 - c exp(-d_n)) pi_n A_n      (constants of the loss)
//   La   = ca l_a      Lb = sum_n bc_n l_n      H = -sum_n pi_n l_n
//   loss = -scale sum_{t<T,b} w (La + Lb + beta H);       monitors: scale sum w La, scale sum w Lb, scale sum w H
//   g_n  = -([n = a] ca + bc_n - beta pi_n (l_n + 1))     the gradient of -(La + Lb + beta H) w.r.t. l
//   s    = max(0, (sum k_n g_n - delta) / sum k_n^2)      (0 without avg_output),      z_n = g_n - s k_n
//   unit[t,b,n] = w scale (z_n - pi_n sum_m z_m)          and grad_target_output = g_loss * unit.
// The projection acts on the per-sample g, before w and scale (the ACER paper's form).
//
// Mapping (rowgroup.hpp): a row of N values is owned by a group of G lanes; lane gl holds a RowSlice of the x, y, q (and u)
// rows, R rows per group and iteration.  Three rounds of group all-reduces, everything else is per lane:
//   1. the maxima of x, y, u;  the slices become x - max, y - max, exp(u - max);
//   2. the partition sums;  then per element l = (x - mx) - log sx and d = ((x - mx) - (y - my)) - (log sx - log sy), each in
//      ONE expression from the rows' statistics (no two separately rounded log-probabilities), pi, k, bc, g.  The slices are
//      overwritten in place: x -> g, y -> pi, u -> k (four inputs per row leave no room for copies);
//   3. sum k g, sum k^2, sum g and sum k over the selected columns;  sum z = sum g - s sum k.
// l_a and d_a need no reduction: the lane that holds column a forms ca and adds La.  La, Lb and H are summed per LANE over
// the rows it visits (x w), then per workgroup, and leave through publish_sums (colscan.hpp): partials in a fixed order, no
// float atomics, bit-identical from run to run.  The row work uses no LDS and no barrier; every load is unconditional and
// in bounds (padding lanes re-read column 0, idle groups the last row).
//
// -inf target logits (masked actions) are clamped to the most negative finite float, as categorical.hip and retrace.hip do.
// Such a column has pi_n = 0 and every sum SELECTS on pi_n > 0 instead of multiplying (0 * -inf and -inf - -inf are the
// traps): it adds exactly 0 to Lb, H and sum z and its gradient is 0.  An action outside [0,N) matches no column: ca = 0.
// N = 1: z - pi sum z is fmaf(-pi, sum z, z) with pi = 1 and sum z formed by the same fmaf as z: exactly 0.
//
// Algorithmic HBM bytes per row: forward 16 N read (12 N without avg_output) + 4 N written when the gradient is wanted, + 20
// for action, q_retraces, v_pred (+ 4 weights); backward (scale_rows, reduce.hip) 4 N read, 4 N written.  Recomputing in the
// backward as PPOContinuous does would read the four rows twice (32 N + 4 N against 24 N): this form was chosen on bytes,
// it was not measured against the other.
//
// acer_trust_region_kernel is the projection alone, the drop-in for acer_trust_region_update: out = g - max(0, (sum k g -
// delta) / sum k^2) k with k = exp(avg_logit) (log-probabilities in, as DI-engine's); two rows read, one written.
#include <hip/hip_runtime.h>

#include "colscan.hpp"
#include "hostutil.hpp"
#include "hpc_rll_hip.h"
#include "rowgroup.hpp"
#include "wave.hpp"

namespace hpc_rll {
namespace {

constexpr int kAcerMaxN = kRowTableMaxN;   // 64 lanes x 16 floats per lane and input
constexpr int kAcerSums = 4;               // w (La + Lb + beta H), w La, w Lb, w H

struct AcerArgs {
    const float* target; const float* behaviour; const float* avg; const float* q; const float* q_ret; const float* v;
    const int64_t* action; const float* weights; float* unit; long rows; int N; float c, beta, delta, scale;
};

// HW: weights given; HAVG: avg_output given (the projection); GRAD: the unit gradient row is stored
template <int G, int VEC, int E, bool HW, bool HAVG, bool GRAD>
__global__ __launch_bounds__(256) void acer_policy_fwd_kernel(const AcerArgs p, float* __restrict__ partials,
                                                              const ScanFold fold) {
    constexpr int GPB = 256 / G;
    constexpr int R = RowsPerIter<VEC, E>::value;
    const int gl = threadIdx.x % G;
    const int gi = threadIdx.x / G;
    const int N = p.N;
    const long stride = (long)gridDim.x * GPB * R;
    float acc[kAcerSums];
#pragma unroll
    for (int k = 0; k < kAcerSums; ++k) acc[k] = 0.f;
    for (long bb = (long)blockIdx.x * GPB * R; bb < p.rows; bb += stride) {
        RowSlice<G, VEC, E> xs[R], ys[R], us[R], qs[R];
        long a[R];
        float qr[R], vp[R], wt[R];
#pragma unroll
        for (int k = 0; k < R; ++k) {
            long row = bb + (long)k * GPB + gi;
            if (row >= p.rows) row = p.rows - 1;           // (re-reads the last row; sums and stores below are guarded)
            const long off = row * (long)N;
            xs[k].load(p.target + off, N, gl);
            ys[k].load(p.behaviour + off, N, gl);
            if (HAVG) us[k].load(p.avg + off, N, gl);
            qs[k].load(p.q + off, N, gl);
            a[k] = p.action[row];                          // (every lane: the same address per group, one request)
            qr[k] = p.q_ret[row];
            vp[k] = p.v[row];
            wt[k] = HW ? p.weights[row] : 1.f;
        }
#pragma unroll
        for (int k = 0; k < R; ++k) {
            float* x = xs[k].x;
            float* y = ys[k].x;
            float* u = us[k].x;
            const float* q = qs[k].x;
            const long row = bb + (long)k * GPB + gi;
            const bool live = row < p.rows;
            const int ai = action_index(a[k], N);
            // ---- 1. maxima; x <- x - mx, y <- y - my (clamped: finite), u <- exp(u - mu)
            const float mx = row_max_finite<G, VEC, E>(x, N, gl);
            const float my = row_max_finite<G, VEC, E>(y, N, gl);
            const float mu = HAVG ? row_max_finite<G, VEC, E>(u, N, gl) : 0.f;
            float sx = 0.f, sy = 0.f, su = 0.f;
#pragma unroll
            for (int e = 0; e < E; ++e)
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    const int i = e * VEC + j;
                    const bool in = (e * G + gl) * VEC + j < N;
                    x[i] = fmaxf(x[i], -kFltMax) - mx;
                    y[i] = fmaxf(y[i], -kFltMax) - my;
                    sx += in ? __expf(x[i]) : 0.f;
                    sy += in ? __expf(y[i]) : 0.f;
                    if (HAVG) {
                        u[i] = in ? __expf(fmaxf(u[i], -kFltMax) - mu) : 0.f;
                        su += u[i];
                    }
                }
            // ---- 2. partition sums; x <- g, y <- pi, u <- k
            sx = group_all<G, AddOp>(sx);
            sy = group_all<G, AddOp>(sy);
            if (HAVG) su = group_all<G, AddOp>(su);
            const float lsx = logf(sx), dls = lsx - logf(sy);
            const float inv_su = HAVG ? 1.f / su : 0.f;
            const float adv_ret = qr[k] - vp[k];
            float la = 0.f, lb = 0.f, hs = 0.f;            // this lane's part of La, Lb and sum pi l
            float kg = 0.f, kk = 0.f, sg = 0.f, sk = 0.f;
#pragma unroll
            for (int e = 0; e < E; ++e)
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    const int i = e * VEC + j;
                    const int c = (e * G + gl) * VEC + j;
                    const float l = x[i] - lsx;
                    const float d = (x[i] - y[i]) - dls;
                    const float pi = (c < N) ? expf(l) : 0.f;
                    const bool sel = pi > 0.f;
                    const float bcf = fmaxf(0.f, 1.f - p.c * expf(-d));
                    const float bc = sel ? bcf * pi * (q[i] - vp[k]) : 0.f;
                    const float ca = (sel && c == ai) ? fminf(p.c, expf(d)) * adv_ret : 0.f;
                    const float pl = sel ? pi * l : 0.f;
                    la = fmaf(ca, sel ? l : 0.f, la);
                    lb = fmaf(bc, sel ? l : 0.f, lb);
                    hs += pl;
                    const float g = -((ca + bc) - p.beta * (pl + pi));
                    x[i] = g;
                    y[i] = pi;
                    sg += g;
                    if (HAVG) {
                        const float kn = u[i] * inv_su;
                        u[i] = kn;
                        kg = fmaf(kn, g, kg);
                        kk = fmaf(kn, kn, kk);
                        sk += sel ? kn : 0.f;
                    }
                }
            if (live) {
                const float t = (la + lb) - p.beta * hs;
                acc[0] = fmaf(wt[k], t, acc[0]);
                acc[1] = fmaf(wt[k], la, acc[1]);
                acc[2] = fmaf(wt[k], lb, acc[2]);
                acc[3] = fmaf(wt[k], -hs, acc[3]);
            }
            if (!GRAD) continue;
            // ---- 3. the projection and the chain through log_softmax
            sg = group_all<G, AddOp>(sg);
            float s = 0.f, sz = sg;
            if (HAVG) {
                kg = group_all<G, AddOp>(kg);
                kk = group_all<G, AddOp>(kk);
                sk = group_all<G, AddOp>(sk);
                s = fmaxf(0.f, (kg - p.delta) / kk);
                sz = fmaf(-s, sk, sg);
            }
            const float ws = HW ? wt[k] * p.scale : p.scale;
            float* out = p.unit + row * (long)N;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const int c0 = (e * G + gl) * VEC;
                float o[VEC];
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    const int i = e * VEC + j;
                    const float z = HAVG ? fmaf(-s, u[i], x[i]) : x[i];
                    o[j] = (y[i] > 0.f) ? ws * fmaf(-y[i], sz, z) : 0.f;
                }
                if (live && c0 < N) store_piece<VEC>(out + c0, o);
            }
        }
    }
    publish_block_sums<kAcerSums, 256>(acc, partials, fold);   // (the only LDS and barriers of the kernel)
}

// out = g - max(0, (sum k g - delta) / sum k^2) k,  k = exp(avg_logit): the projection alone
template <int G, int VEC, int E>
__global__ __launch_bounds__(256) void acer_trust_region_kernel(const float* __restrict__ grad,
                                                                const float* __restrict__ avg_logit,
                                                                float* __restrict__ out, long rows, int N, float delta) {
    constexpr int GPB = 256 / G;
    constexpr int R = RowsPerIter<VEC, E>::value;
    const int gl = threadIdx.x % G;
    const int gi = threadIdx.x / G;
    const long stride = (long)gridDim.x * GPB * R;
    for (long bb = (long)blockIdx.x * GPB * R; bb < rows; bb += stride) {
        RowSlice<G, VEC, E> gs[R], ks[R];
#pragma unroll
        for (int k = 0; k < R; ++k) {
            long row = bb + (long)k * GPB + gi;
            if (row >= rows) row = rows - 1;               // (re-reads the last row; the stores below are guarded)
            gs[k].load(grad + row * (long)N, N, gl);
            ks[k].load(avg_logit + row * (long)N, N, gl);
        }
#pragma unroll
        for (int k = 0; k < R; ++k) {
            float kg = 0.f, kk = 0.f;
#pragma unroll
            for (int e = 0; e < E; ++e)
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    const int i = e * VEC + j;
                    const bool in = (e * G + gl) * VEC + j < N;
                    const float kn = in ? expf(ks[k].x[i]) : 0.f;
                    ks[k].x[i] = kn;
                    kg = in ? fmaf(kn, gs[k].x[i], kg) : kg;
                    kk = fmaf(kn, kn, kk);
                }
            kg = group_all<G, AddOp>(kg);
            kk = group_all<G, AddOp>(kk);
            const float s = fmaxf(0.f, (kg - delta) / kk);
            const long row = bb + (long)k * GPB + gi;
            if (row >= rows) continue;
            float* o = out + row * (long)N;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const int c0 = (e * G + gl) * VEC;
                if (c0 >= N) continue;
                float z[VEC];
#pragma unroll
                for (int j = 0; j < VEC; ++j) z[j] = fmaf(-s, ks[k].x[e * VEC + j], gs[k].x[e * VEC + j]);
                store_piece<VEC>(o + c0, z);
            }
        }
    }
}

// The dispatch record (hpc_rll_acer_last_config): {launches so far, G, VEC, E, R, flags, grid, drop-in}
LaunchRecord<HPC_RLL_ACER_CONFIG_INTS> g_acer_last;

template <bool HW, bool HAVG, bool GRAD>
int acer_forward(const AcerArgs& p, float* partials, const float* scales, float* out4, hipStream_t st) {
    const bool v4 = aligned(p.target, 16) && aligned(p.behaviour, 16) && aligned(p.avg, 16) && aligned(p.q, 16) &&
                    aligned(p.unit, 16);   // (an absent operand restricts nothing)
    return with_row4(row_cfg(p.N, v4, kRow4Pieces), [&](auto G_, auto V_, auto E_) {
        constexpr int G = G_, V = V_, E = E_, R = RowsPerIter<V, E>::value;
        long grid = 0;
        const int rc = launch_rows_folded(p.rows, (256 / G) * R, kAcerSums, scales, out4, partials, st, &grid,
                                          [&](unsigned blocks, const ScanFold& fold) {
            hipLaunchKernelGGL((acer_policy_fwd_kernel<G, V, E, HW, HAVG, GRAD>), dim3(blocks), dim3(256), 0, st, p,
                               partials, fold);
        });
        if (grid) g_acer_last.note({G, V, E, R, (HW ? 1 : 0) | (HAVG ? 2 : 0) | (GRAD ? 4 : 0), (int)grid, 0});
        return rc;
    });
}

int acer_trust_region(const float* grad, const float* avg_logit, float* out, long rows, int N, float delta, hipStream_t st) {
    const RowCfg cfg = row_cfg(N, aligned(grad, 16) && aligned(avg_logit, 16) && aligned(out, 16), kRow4Pieces);
    return with_row4(cfg, [&](auto G_, auto V_, auto E_) {
        constexpr int G = G_, V = V_, E = E_, R = RowsPerIter<V, E>::value;
        const unsigned grid = row_grid(rows, (256 / G) * R, kUnfoldedGridCap);
        hipLaunchKernelGGL((acer_trust_region_kernel<G, V, E>), dim3(grid), dim3(256), 0, st, grad, avg_logit, out, rows, N,
                           delta);
        const int rc = last_error();
        if (!rc) g_acer_last.note({G, V, E, R, 0, (int)grid, 1});
        return rc;
    });
}

}  // namespace
}  // namespace hpc_rll

using namespace hpc_rll;

// ws (floats): the partial sums, 4 per workgroup of at most kFoldMaxGrid
extern "C" int64_t hpc_rll_acer_policy_workspace_floats(int T, int B) {
    if (T < 0 || B < 0) return HPC_RLL_EINVAL;
    return 8 * (kFoldMaxGrid + 1);
}

extern "C" int hpc_rll_acer_policy_forward(const float* target_output, const float* behaviour_output,
                                           const float* avg_output, const float* q_values, const float* q_retraces,
                                           const float* v_pred, const int64_t* action, const float* weights, float* out4,
                                           float* unit_grad, float* ws, int T, int B, int N, float c_clip_ratio,
                                           float entropy_weight, float trust_region_value, float scale, void* stream) {
    const bool empty = T == 0 || B == 0;
    if (!out4) return HPC_RLL_EINVAL;
    if (!empty && (!target_output || !behaviour_output || !q_values || !q_retraces || !v_pred || !action || !ws))
        return HPC_RLL_EINVAL;
    if (T < 0 || B < 0 || N <= 0) return HPC_RLL_EINVAL;
    if (!aligned(target_output, 4) || !aligned(behaviour_output, 4) || !aligned(avg_output, 4) || !aligned(q_values, 4) ||
        !aligned(q_retraces, 4) || !aligned(v_pred, 4) || !aligned(action, 8) || !aligned(weights, 4) || !aligned(out4, 4) ||
        !aligned(unit_grad, 4) || !aligned(ws, 4))
        return HPC_RLL_EALIGN;
    if (N > kAcerMaxN) return HPC_RLL_EUNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    if (empty) return (int)hipMemsetAsync(out4, 0, kAcerSums * sizeof(float), st);
    const AcerArgs p{target_output, behaviour_output, avg_output, q_values, q_retraces, v_pred, action, weights, unit_grad,
                     (long)T * B, N, c_clip_ratio, entropy_weight, trust_region_value, scale};
    const float sc[kAcerSums] = {-scale, scale, scale, scale};
    int rc = HPC_RLL_OK;
    auto run = [&](auto HW_, auto HAVG_) {
        constexpr bool HW = decltype(HW_)::value, HAVG = decltype(HAVG_)::value;
        rc = unit_grad ? acer_forward<HW, HAVG, true>(p, ws, sc, out4, st) : acer_forward<HW, HAVG, false>(p, ws, sc, out4, st);
    };
    using Yes = std::true_type;
    using No = std::false_type;
    if (weights) {
        if (avg_output) run(Yes{}, Yes{});
        else run(Yes{}, No{});
    } else {
        if (avg_output) run(No{}, Yes{});
        else run(No{}, No{});
    }
    return rc;
}

extern "C" int hpc_rll_acer_policy_backward(const float* g_loss, const float* unit_grad, float* grad_target_output, int T,
                                            int B, int N, int target_rows, void* stream) {
    const bool empty = T == 0 || B == 0;
    if (!empty && (!g_loss || !unit_grad || !grad_target_output)) return HPC_RLL_EINVAL;
    if (T < 0 || B < 0 || N <= 0 || (target_rows != T && target_rows != T + 1)) return HPC_RLL_EINVAL;
    if (!aligned(g_loss, 4) || !aligned(unit_grad, 4) || !aligned(grad_target_output, 4)) return HPC_RLL_EALIGN;
    if (N > kAcerMaxN) return HPC_RLL_EUNSUPPORTED;
    if (empty) return HPC_RLL_OK;   // T == 0: the caller zeroes the (1,B,N) gradient of a bootstrap row itself
    const long n_in = (long)T * B * N;
    return scale_rows(g_loss, unit_grad, grad_target_output, n_in, (long)target_rows * B * N, (hipStream_t)stream);
}

extern "C" int hpc_rll_acer_trust_region(const float* actor_gradient, const float* avg_logit, float* out, int64_t rows,
                                         int N, float trust_region_value, void* stream) {
    if (rows > 0 && (!actor_gradient || !avg_logit || !out)) return HPC_RLL_EINVAL;
    if (rows < 0 || N <= 0) return HPC_RLL_EINVAL;
    if (!aligned(actor_gradient, 4) || !aligned(avg_logit, 4) || !aligned(out, 4)) return HPC_RLL_EALIGN;
    if (N > kAcerMaxN) return HPC_RLL_EUNSUPPORTED;
    if (rows == 0) return HPC_RLL_OK;
    return acer_trust_region(actor_gradient, avg_logit, out, (long)rows, N, trust_region_value, (hipStream_t)stream);
}

extern "C" int hpc_rll_acer_last_config(int* out) {
    if (!out) return HPC_RLL_EINVAL;
    g_acer_last.read(out);
    return HPC_RLL_OK;
}
