// grpo.hip -- the language-model policy losses on gfx950: the per-token log-probability of a chosen token over a large
// vocabulary, GRPO's clipped-ratio + k3-KL token loss with per-sequence masked means, and the streaming gradient.
//
// No reference counterpart; the semantics restate DI-engine's rl_utils grpo_policy_error / rloo_policy_error and the
// log_prob_utils helper they share.  logits (rows, V) fp32 or bf16 (rows = B*S), action (rows) int64, per token, with
// lp(x) = x[a] - logsumexp(x):
//   pn = lp(logit_new)   po = lp(old) or old   pr = lp(ref) or ref
//   d  = pr - pn         kl = exp(d) - d - 1
//   r  = exp(pn - po)    rc = clamp(r, 1 - clip, 1 + clip)
//   l  = -min(r adv_b, rc adv_b) + beta kl
//   loss = scale sum_b (sum_s w l / sum_s w)                                           (scale = 1/B unless a sharded caller gives it)
//   dl/dpn = -adv_b r [not (rc adv_b < r adv_b)] - beta (exp(d) - 1)
//   grad[b,s,v] = g w scale / (sum_s w) dl/dpn ([v = a] - exp(x_v - lse))
//
// Three kernels; what they have in common with lm_ppo.hip's (the statistic and the row walk of the head, the head kernel and
// its launcher, the row loops of the gradient, the first pass of the token loss, the dispatch) is in lm_head.hpp:
//   * lm_head_kernel<Elem, ALIGNED, NT, false> (lm_head.hpp): ONE read of the row, an online (max, sum exp) pair per lane and
//     no entropy moment.  NT = 256: a workgroup per row (V above kWaveRowMaxV); NT = 64: a wave per row, four rows per
//     workgroup.  A dropped row (action outside [0,V), or weight 0) is not read: logp = lse = 0.
//   * grpo_token_kernel: a wave per sequence walks s twice (seq_weight_sum, then everything); wave butterflies in a fixed
//     order, the batch sums leave through publish_wave_sums (colscan.hpp).  No float atomics.
//   * token_grad_kernel<Elem, WIDE, NT>: reads the row once, writes c ([v = a] - exp(x - lse)) through stream_row.  A row
//     whose coefficient is exactly 0 is zero-filled WITHOUT reading its logits (zero_row); the decision is the device's.  A
//     row is live on `action` alone: a zero weight arrives as coef == 0.
// -inf logits are clamped to the most negative finite float on load (probability exactly 0), as categorical.hip does; the same
// clamp turns a NaN logit of a LIVE row into an entry of probability 0: NaN there is not propagated to the loss or the gradient.
#include <hip/hip_runtime.h>

#include "colscan.hpp"
#include "hostutil.hpp"
#include "hpc_rll_hip.h"
#include "lm_head.hpp"
#include "wave.hpp"

namespace hpc_rll {
namespace {

constexpr int kGrpoSums = 5;         // loss, sum w kl, sum w r, sum w clipped, sum w

// The dispatch records (hpc_rll_grpo_last_config)
constexpr int kHeadInts = 7, kTokenInts = 3, kGradInts = 6;
LaunchRecord<kHeadInts> g_grpo_head;
LaunchRecord<kTokenInts> g_grpo_token;
LaunchRecord<kGradInts> g_grpo_grad;

// the head without the entropy: logp[row] = x[a] - lse, lse[row] (lse may be NULL)
int token_logp_any(const void* x, int elem, const int64_t* action, const float* weight, float* logp, float* lse, long rows,
                   int V, hipStream_t st) {
    return lm_head_launch<false>(x, elem, action, weight, logp, lse, nullptr, rows, V, st, g_grpo_head);
}

// ================================================================================================
// the token loss: a wave per sequence
// ================================================================================================
struct GrpoTokenArgs {
    const float *pn, *po, *pr; const int64_t* action; const float* adv; const float* weight; float* coef;
    int B, S, V; float clip, beta, scale;
};

__global__ __launch_bounds__(256) void grpo_token_kernel(const GrpoTokenArgs p, float* __restrict__ partials,
                                                         const ScanFold fold) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const float lo = 1.f - p.clip, hi = 1.f + p.clip;
    float acc[kGrpoSums] = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (long b = (long)blockIdx.x * 4 + wv; b < (long)p.B; b += (long)gridDim.x * 4) {
        const size_t base = (size_t)b * (size_t)p.S;
        const float sw = seq_weight_sum(p.action, p.weight, base, p.S, p.V, lane);
        const float adv = p.adv[b];
        const float inv = sw != 0.f ? 1.f / sw : 0.f;   // a sequence without weight contributes 0 and still counts in B
        const float cs = p.scale * inv;
        float sl = 0.f, skl = 0.f, sr = 0.f, sc = 0.f;
        for (int s = lane; s < p.S; s += 64) {
            const size_t i = base + s;
            const long a = p.action[i];
            float w = p.weight ? p.weight[i] : 1.f;
            const bool live = a >= 0 && a < (long)p.V && w != 0.f;
            float pn = p.pn[i], po = p.po[i];
            float pr = p.pr ? p.pr[i] : pn;
            w = live ? w : 0.f;                          // a dropped token: selected away, whatever its values are
            pn = live ? pn : 0.f;
            po = live ? po : 0.f;
            pr = live ? pr : 0.f;
            const float d = pr - pn;
            const float em1 = expm1f(d);
            const float kl = em1 - d;
            const float r = expf(pn - po);
            const float rc = fminf(fmaxf(r, lo), hi);
            const float t1 = r * adv, t2 = rc * adv;
            const float l = -(t2 < t1 ? t2 : t1) + p.beta * kl;
            const float dl = -(t2 < t1 ? 0.f : t1) - p.beta * em1;
            const float clipped = (r > hi || r < lo) ? 1.f : 0.f;
            sl = fmaf(w, l, sl);
            skl = fmaf(w, kl, skl);
            sr = fmaf(w, r, sr);
            sc = fmaf(w, clipped, sc);
            p.coef[i] = live ? (w * cs) * dl : 0.f;
        }
        sl = wave_sum(sl);
        skl = wave_sum(skl);
        sr = wave_sum(sr);
        sc = wave_sum(sc);
        acc[0] += sl * inv;
        acc[1] += skl;
        acc[2] += sr;
        acc[3] += sc;
        acc[4] += sw;
    }
    publish_wave_sums<kGrpoSums>(acc, partials, fold);
}

// sums = scale * loss sum, sum w kl, sum w r, sum w clipped, sum w  ->  out4 = loss, mean_kl, mean_ratio, mean_clipped
__global__ __launch_bounds__(64) void grpo_info_kernel(const float* __restrict__ sums, float* __restrict__ out4) {
    const int k = threadIdx.x;
    if (k >= 4) return;
    const float sw = sums[4];
    out4[k] = k == 0 ? sums[0] : (sw != 0.f ? sums[k] / sw : 0.f);
}

// ================================================================================================
// the gradient: grad[row, v] = c ([v = a] - exp(x_v - lse)),  c = coef[row] g  (g NULL = 1; an action outside: c = 0)
// ================================================================================================
template <class Elem, bool WIDE, int NT>
__global__ __launch_bounds__(256) void token_grad_kernel(const Elem* __restrict__ x, const int64_t* __restrict__ action,
                                                         const float* __restrict__ lse, const float* __restrict__ coef,
                                                         const float* __restrict__ g, Elem* __restrict__ grad, long rows,
                                                         int V) {
    constexpr int RPW = 256 / NT;
    const int tid = threadIdx.x % NT, sub = threadIdx.x / NT;
    const float u = g ? g[0] : 1.f;
    for (long r0 = (long)blockIdx.x * RPW; r0 < rows; r0 += (long)gridDim.x * RPW) {
        const long row = r0 + sub;
        if (row >= rows) continue;
        const long a = action[row];
        const bool inr = a >= 0 && a < (long)V;
        const float c = inr ? coef[row] * u : 0.f;
        const int ai = inr ? (int)a : -1;
        const Elem* p = x + (size_t)row * (size_t)V;
        Elem* o = grad + (size_t)row * (size_t)V;
        if (c == 0.f) {
            zero_row<Elem, WIDE, NT>(o, V, tid);
            continue;
        }
        const float l = lse[row];
        stream_row<Elem, WIDE, NT>(p, o, V, tid, ai, [&](float xv, bool chosen) {
            const float e = ex2((clampf(xv) - l) * kLog2eG);
            return fmaf(-c, e, chosen ? c : 0.f);
        });
    }
}

int token_grad_any(const void* xv, int elem, const int64_t* action, const float* lse, const float* coef, const float* g,
                   void* gradv, long rows, int V, hipStream_t st) {
    return with_elem(elem, [&](auto e) {
        using Elem = decltype(e);
        const Elem* x = static_cast<const Elem*>(xv);
        Elem* grad = static_cast<Elem*>(gradv);
        const RowLaunch L = row_launch<Elem>(x, grad, rows, V);
        with_row_kernel(L, [&](auto W, auto NT) {
            hipLaunchKernelGGL((token_grad_kernel<Elem, decltype(W)::value, decltype(NT)::value>), dim3((unsigned)L.grid),
                               dim3(256), 0, st, x, action, lse, coef, g, grad, rows, V);
        });
        const int rc = last_error();
        if (!rc) g_grpo_grad.note({ElemIO<Elem>::kCode, L.wide ? 16 : (int)sizeof(Elem), L.nt, L.rpw, (int)L.grid});
        return rc;
    });
}

}  // namespace
}  // namespace hpc_rll

using namespace hpc_rll;

extern "C" int hpc_rll_token_logp_forward(const void* logits, int elem, const int64_t* action, const float* weight,
                                          float* logp, float* lse, int64_t rows, int V, void* stream) {
    const bool empty = rows == 0 || V == 0;
    if (!empty && (!logits || !action || !logp)) return HPC_RLL_EINVAL;
    if (const int bad = lm_shape_status(rows, 1, V, elem, aligned(logits, elem_size(elem)) && aligned(action, 8) &&
                                        aligned(weight, 4) && aligned(logp, 4) && aligned(lse, 4)))
        return bad;
    if (empty) {   // V == 0 with rows: no token has a probability; zeros
        if (rows > 0 && logp) {
            int rc = (int)hipMemsetAsync(logp, 0, (size_t)rows * sizeof(float), (hipStream_t)stream);
            if (!rc && lse) rc = (int)hipMemsetAsync(lse, 0, (size_t)rows * sizeof(float), (hipStream_t)stream);
            return rc;
        }
        return HPC_RLL_OK;
    }
    return token_logp_any(logits, elem, action, weight, logp, lse, (long)rows, V, (hipStream_t)stream);
}

extern "C" int hpc_rll_token_logp_backward(const float* g_logp, const void* logits, int elem, const int64_t* action,
                                           const float* lse, void* grad_logits, int64_t rows, int V, void* stream) {
    const bool empty = rows == 0 || V == 0;
    if (!empty && (!g_logp || !logits || !action || !lse || !grad_logits)) return HPC_RLL_EINVAL;
    if (const int bad = lm_shape_status(rows, 1, V, elem, aligned(logits, elem_size(elem)) && aligned(grad_logits, elem_size(elem)) &&
                                        aligned(action, 8) && aligned(g_logp, 4) && aligned(lse, 4)))
        return bad;
    if (empty) return HPC_RLL_OK;
    return token_grad_any(logits, elem, action, lse, g_logp, nullptr, grad_logits, (long)rows, V, (hipStream_t)stream);
}

// ws (floats), R = B*S: lse (R) | coef (R) | logp of logit_new (R) | logp of old (R) | logp of ref (R) | the five sums (8) |
// partial sums, five per workgroup of the token launch
extern "C" int64_t hpc_rll_grpo_workspace_floats(int B, int S) {
    if (B < 0 || S < 0) return HPC_RLL_EINVAL;
    return 5 * (int64_t)B * S + 8 + 8 * (kFoldMaxGrid + 1);
}

extern "C" int hpc_rll_grpo_forward(const void* logit_new, int elem_new, const void* old, int old_kind, const void* ref,
                                    int ref_kind, const int64_t* action, const float* adv, const float* weight, float* out4,
                                    float* ws, int B, int S, int V, float clip_ratio, float beta, float scale, void* stream) {
    const bool empty = B == 0 || S == 0 || V == 0;
    auto kind_ok = [](int k) { return elem_ok(k) || k == HPC_RLL_GRPO_LOGP; };
    if (!out4) return HPC_RLL_EINVAL;
    if (!empty && (!logit_new || !old || !action || !adv || !ws)) return HPC_RLL_EINVAL;
    if (!kind_ok(old_kind) || (ref && !kind_ok(ref_kind))) return HPC_RLL_EINVAL;
    if (const int bad = lm_shape_status(B, S, V, elem_new, aligned(logit_new, elem_size(elem_new)) && aligned(old, elem_size(old_kind)) &&
                                        aligned(ref, elem_size(ref_kind)) && aligned(action, 8) && aligned(adv, 4) &&
                                        aligned(weight, 4) && aligned(out4, 4) && aligned(ws, 4)))
        return bad;
    hipStream_t st = (hipStream_t)stream;
    if (empty) return (int)hipMemsetAsync(out4, 0, 4 * sizeof(float), st);
    const long R = (long)B * S;
    float *lse = ws, *coef = ws + R, *pn = ws + 2 * R, *po_ws = ws + 3 * R, *pr_ws = ws + 4 * R, *sums = ws + 5 * R,
          *partials = ws + 5 * R + 8;
    int rc = token_logp_any(logit_new, elem_new, action, weight, pn, lse, R, V, st);
    if (rc) return rc;
    const float* po = static_cast<const float*>(old);
    if (old_kind != HPC_RLL_GRPO_LOGP) {
        rc = token_logp_any(old, old_kind, action, weight, po_ws, nullptr, R, V, st);
        if (rc) return rc;
        po = po_ws;
    }
    const float* pr = nullptr;
    if (ref) {
        pr = static_cast<const float*>(ref);
        if (ref_kind != HPC_RLL_GRPO_LOGP) {
            rc = token_logp_any(ref, ref_kind, action, weight, pr_ws, nullptr, R, V, st);
            if (rc) return rc;
            pr = pr_ws;
        }
    }
    const float sc = scale > 0.f ? scale : 1.f / (float)B;
    const GrpoTokenArgs p{pn, po, pr, action, adv, weight, coef, B, S, V, clip_ratio, ref ? beta : 0.f, sc};
    long grid = ((long)B + 3) / 4;
    if (grid > kFoldMaxGrid) grid = kFoldMaxGrid;
    const float scales[kGrpoSums] = {sc, 1.f, 1.f, 1.f, 1.f};
    const ScanFold fold = make_fold(st, kGrpoSums, scales, sums, grid);
    hipLaunchKernelGGL(grpo_token_kernel, dim3((unsigned)grid), dim3(256), 0, st, p, partials, fold);
    rc = last_error();
    if (rc) return rc;
    if (!fold.out) {
        rc = finalize_sums(partials, (int)grid, kGrpoSums, scales, sums, st);
        if (rc) return rc;
    }
    g_grpo_token.note({256, (int)grid});
    hipLaunchKernelGGL(grpo_info_kernel, dim3(1), dim3(64), 0, st, sums, out4);
    return last_error();
}

extern "C" int hpc_rll_grpo_backward(const float* g_loss, const void* logit_new, int elem, const int64_t* action,
                                     const float* ws, void* grad_logit, int B, int S, int V, void* stream) {
    const bool empty = B == 0 || S == 0 || V == 0;
    if (!empty && (!logit_new || !action || !ws || !grad_logit)) return HPC_RLL_EINVAL;
    if (const int bad = lm_shape_status(B, S, V, elem, aligned(logit_new, elem_size(elem)) && aligned(grad_logit, elem_size(elem)) &&
                                        aligned(action, 8) && aligned(g_loss, 4) && aligned(ws, 4)))
        return bad;
    if (empty) return HPC_RLL_OK;
    const long R = (long)B * S;
    return token_grad_any(logit_new, elem, action, ws, ws + R, g_loss, grad_logit, R, V, (hipStream_t)stream);
}

extern "C" int hpc_rll_grpo_last_config(int* out) {
    if (!out) return HPC_RLL_EINVAL;
    g_grpo_head.read(out);
    g_grpo_token.read(out + kHeadInts);
    g_grpo_grad.read(out + kHeadInts + kTokenInts);
    return HPC_RLL_OK;
}
static_assert(HPC_RLL_GRPO_CONFIG_INTS == kHeadInts + kTokenInts + kGradInts, "the layout documented in hpc_rll_hip.h");