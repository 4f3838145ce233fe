// scan_masked.hip -- episode-aware TD(lambda), V-trace and UPGO (done / traj_flag masks) on the generic reverse column scan
// (colscan.hpp) for gfx950.  No reference counterpart: hpc_rll/origin/td.py:152-154 and :220-222 leave terminal states
// to the caller, which only works when a column holds one episode.
//
// With k^d_t = 1 - done_t, k^f_t = 1 - f_t (f = traj_flag, defaulting to done; masks.hpp) and nv_t the next value
// (value[t+1] in the stacked form, next_value[t] in the next-value form), disc = gamma*lambda and rest = gamma - disc
// rounded as TdLambdaOp rounds them:
//   TD(lambda): G_T := nv_{T-1},  G_t = r_t + (gamma*k^d_t - disc*k^f_t) * nv_t + disc*k^f_t * G_{t+1}
//               scan form a_t = disc*k^f_t, b_t = fmaf(gamma*k^d_t - disc*k^f_t, nv_t, r_t); loss and grad_buf as TdLambdaOp
//   V-trace   : s_T = 0,  s_t = rho_t*(fmaf(gamma, k^d_t*nv_t, r_t) - V_t) + (disc*k^f_t)*c_t * s_{t+1}
//               adv_t = rho_pg_t*(fmaf(gamma, k^d_t*nv_t + k^f_t*s_{t+1}, r_t) - V_t); losses and saved coefficients as
//               VtraceOp
//   UPGO      : G_T := nv_{T-1},  q_t = fmaf(gamma, k^d_t*nv_t, r_t),  lam_t = [q_{t+1} >= V_{t+1}] (1 at t = T-1; V_{t+1} is
//               row t+1 of `value` in both forms, q_{t+1} uses step t+1's own done),  a_t = gamma*k^f_t*lam_t,
//               G_t = fmaf(gamma*k^d_t - a_t, nv_t, r_t) + a_t*G_{t+1}; loss and saved coefficient as UpgoOp.  With gamma = 1
//               fmaf(1, x, r) rounds once like r + x and 1 - lam is exactly 0 or 1: UpgoOp's bits.  UpgoOp itself has no
//               discount and carries the return and the comparison across an episode end.
// Without masks (MM_NONE) every expression is the unmasked Op's; with all-zero masks every k is 1.0f and x*1.0f is exact,
// so the bits are the same too.  Only the forward scans change: the returns are constants of the losses, and the existing
// backward entry points (hpc_rll_td_lambda_backward / hpc_rll_vtrace_backward / hpc_rll_upgo_backward /
// hpc_rll_scale_rows) consume the saved per-sample coefficients unchanged.
//
// Configuration: the unmasked op's rule for the same (T, B) -- scan_cfg(T, B, v2, lc16) for TD(lambda), V = 1 for
// V-trace and UPGO -- where v2 also asks 8-byte float / 2-byte (u8) or 8-byte (f32) mask alignment, which torch allocations meet.
// A masked call therefore runs the chunking of its unmasked sibling and, without episode ends, gives its bits.
// Instantiations (a closed list): 14 mask forms (with_mode: MM_NONE with u8 + 3 mask modes x 2 dtypes, times stacked /
// next-value) x 13 scan configurations for TD(lambda) (launch_colscan with V2 and LC16) + 14 x 8 for V-trace (V = 1) +
// 14 x 8 for UPGO (V = 1) + 14 x 8 for V-trace over a log ratio (LR, the Gaussian head): 518 kernels, none using scratch
// (tests/tools/kernel_regs.py scan_masked).
#include <hip/hip_runtime.h>

#include "colscan.hpp"
#include "heads.hpp"
#include "hpc_rll_hip.h"
#include "masks.hpp"

namespace hpc_rll {
namespace {

// ================================================================================================
// TD(lambda) with masks: loss = 0.5 * scale * sum w (G_t - V_t)^2 ;  grad_buf_t = -w (G_t - V_t) * scale
// ================================================================================================
template <int MT, int MM, bool NVF>
struct MaskedTdLambdaOp {
    static constexpr int NACC = 1, DIAG_OP = HPC_RLL_SCAN_OP_TD_LAMBDA_MASKED, DIAG_MT = MT, DIAG_MM = MM, DIAG_NVF = NVF;
    static constexpr bool HD = has_done(MM), HF = has_flag(MM), ANY = HD || HF;
    const float* value; const float* next_value; const float* reward; const float* weight; int weight_mode;
    const void* done; const void* flag; float* grad_buf; int T, B; float gamma, disc, rest, scale;
    // The next-value form holds nv in registers of its own; there `finish` loads w (one row per call) instead of holding LC
    // rows of it through the scan, which keeps every configuration within 128 VGPRs (no scratch).
    template <int V> struct Row { Pack<V> v0, v1, r, w; MaskRow<V, MT> md, mf; };

    template <int V> __device__ void init(long col, bool ok, float (&carry)[V]) const {   // G_T := nv_{T-1}
        const Pack<V> nv = load_pack<V>(NVF ? next_value + row_off(T - 1, col, ok, B, V) : value + row_off(T, col, ok, B, V));
#pragma unroll
        for (int k = 0; k < V; ++k) carry[k] = nv.v[k];
    }
    template <int V> __device__ void load(Row<V>& row, int t, long col, bool ok, bool next_in_regs) const {
        const size_t o = row_off(t, col, ok, B, V);
        row.v0 = load_pack<V>(value + o);
        if (NVF) row.v1 = load_pack<V>(next_value + o);
        else if (!next_in_regs) row.v1 = load_pack<V>(value + o + B);
        row.r = load_pack<V>(reward + o);
        if (!NVF) load_w<V>(row.w, t, col, ok);
        if (HD) row.md.template load<false>(done, o);
        if (HF) row.mf.template load<false>(flag, o);
    }
    template <int V> __device__ void load_w(Pack<V>& w, int t, long col, bool ok) const {
        if (weight_mode == 2) w = load_pack<V>(weight + row_off(t, col, ok, B, V));
        else if (weight_mode == 1) w = load_pack<V>(weight + (ok ? col : (long)B - V));
        else {
#pragma unroll
            for (int k = 0; k < V; ++k) w.v[k] = 1.f;
        }
    }
    template <int V> __device__ void link(Row<V>& row, const Row<V>& nxt) const {
        if (!NVF) row.v1 = nxt.v0;
    }
    template <int V> __device__ void coeffs(const Row<V>& row, int, float (&a)[V], float (&b)[V]) const {
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const float kd = HD ? row.md.keep(k) : 1.f;
            const float kf = HF ? row.mf.keep(k) : kd;
            a[k] = ANY ? disc * kf : disc;
            b[k] = fmaf(ANY ? gamma * kd - disc * kf : rest, row.v1.v[k], row.r.v[k]);
        }
    }
    template <int V> __device__ void finish(const Row<V>& row, int t, long col, bool ok, const float (&s)[V],
                                            const float (&)[V], float (&acc)[NACC]) const {
        Pack<V> w;
        if (NVF) load_w<V>(w, t, col, ok);
        else w = row.w;
        if (!ok) return;
        Pack<V> g;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const float d = s[k] - row.v0.v[k];
            acc[0] = fmaf(w.v[k] * d, d, acc[0]);
            g.v[k] = -w.v[k] * d * scale;
        }
        store_pack<V, true>(grad_buf + (size_t)t * B + col, g);
    }
};

// ================================================================================================
// V-trace with masks: IS, rho, c, rho_pg, entropy, the three losses and the saved coefficients as VtraceOp
//   (coef_pg = -w adv scale, coef_ent = w scale, gv_unit = 2 w (V_t - vs_t) scale = -2 w s_t scale)
// ================================================================================================
// LR: the logp_b slot holds the log ratio logp_t - logp_b itself (the Gaussian head: hpc_rll_vtrace_continuous_forward), not logp_b
template <int MT, int MM, bool NVF, bool LR = false>
struct MaskedVtraceOp {
    static constexpr int NACC = 3, DIAG_OP = HPC_RLL_SCAN_OP_VTRACE_MASKED, DIAG_MT = MT, DIAG_MM = MM, DIAG_NVF = NVF;
    static constexpr bool HD = has_done(MM), HF = has_flag(MM), ANY = HD || HF;
    const float* value; const float* next_value; const float* reward; const float* weight; const float* logp_t;
    const float* logp_b; const float* ent; const void* done; const void* flag; float* coef_pg; float* coef_ent;
    float* gv_unit; int T, B; float gamma, disc, rho_clip, c_clip, pg_clip, scale;
    // The entropy (and, in the next-value form, w) is only needed by `finish`, which loads it one row per call instead of
    // holding LC rows of it through the scan: that keeps every configuration within 128 VGPRs (no scratch).
    template <int V> struct Row { Pack<V> v0, v1, r, w, is, lp; MaskRow<V, MT> md, mf; };

    template <int V> __device__ void init(long, bool, float (&carry)[V]) const {
#pragma unroll
        for (int k = 0; k < V; ++k) carry[k] = 0.f;
    }
    template <int V> __device__ void link(Row<V>& row, const Row<V>& nxt) const {
        if (!NVF) row.v1 = nxt.v0;
    }
    template <int V> __device__ void load(Row<V>& row, int t, long col, bool ok, bool next_in_regs) const {
        const size_t o = row_off(t, col, ok, B, V);
        row.v0 = load_pack<V>(value + o);
        if (NVF) row.v1 = load_pack<V>(next_value + o);
        else if (!next_in_regs) row.v1 = load_pack<V>(value + o + B);
        row.r = load_pack<V>(reward + o);
        row.lp = load_pack<V>(logp_t + o);
        const Pack<V> lb = load_pack<V>(logp_b + o);
        if (weight && !NVF) row.w = load_pack<V>(weight + o);
        if (HD) row.md.template load<false>(done, o);
        if (HF) row.mf.template load<false>(flag, o);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            row.is.v[k] = expf(LR ? lb.v[k] : row.lp.v[k] - lb.v[k]);
            if (!weight) row.w.v[k] = 1.f;
        }
    }
    template <int V> __device__ void coeffs(const Row<V>& row, int, float (&a)[V], float (&b)[V]) const {
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const float kd = HD ? row.md.keep(k) : 1.f;
            const float kf = HF ? row.mf.keep(k) : kd;
            a[k] = (ANY ? disc * kf : disc) * fminf(row.is.v[k], c_clip);
            b[k] = fminf(row.is.v[k], rho_clip) * (fmaf(gamma, HD ? kd * row.v1.v[k] : row.v1.v[k], row.r.v[k]) - row.v0.v[k]);
        }
    }
    template <int V> __device__ void finish(const Row<V>& row, int t, long col, bool ok, const float (&s)[V],
                                            const float (&s_next)[V], float (&acc)[NACC]) const {
        const size_t o = row_off(t, col, ok, B, V);
        const Pack<V> h = load_pack<V>(ent + o);
        const Pack<V> wt = (weight && NVF) ? load_pack<V>(weight + o) : row.w;   // row.w = 1 without weight
        if (!ok) return;
        Pack<V> cp, ce, gv;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const float w = wt.v[k];
            const float kd = HD ? row.md.keep(k) : 1.f;
            const float kf = HF ? row.mf.keep(k) : kd;
            const float vs_next = ANY ? kd * row.v1.v[k] + kf * s_next[k] : row.v1.v[k] + s_next[k];
            const float adv = fminf(row.is.v[k], pg_clip) * (fmaf(gamma, vs_next, row.r.v[k]) - row.v0.v[k]);
            acc[0] -= row.lp.v[k] * adv * w;
            acc[1] = fmaf(w * s[k], s[k], acc[1]);   // (V_t - vs_t)^2 = s_t^2
            acc[2] = fmaf(w, h.v[k], acc[2]);
            cp.v[k] = -w * adv * scale;
            ce.v[k] = w * scale;
            gv.v[k] = -2.f * w * s[k] * scale;
        }
        store_pack<V, true>(coef_pg + o, cp);
        store_pack<V, true>(coef_ent + o, ce);
        store_pack<V, true>(gv_unit + o, gv);
    }
};

// ================================================================================================
// UPGO with masks: q_t = fmaf(gamma, k^d_t nv_t, r_t), lam_t = [q_{t+1} >= V_{t+1}] (1 at t = T-1), a_t = gamma k^f_t lam_t,
//   G_t = fmaf(gamma k^d_t - a_t, nv_t, r_t) + a_t G_{t+1};  loss = -scale sum rho (G_t - V_t) logp, saved coef as UpgoOp
// ================================================================================================
template <int MT, int MM, bool NVF>
struct MaskedUpgoOp {
    static constexpr int NACC = 1, DIAG_OP = kScanOpUpgoMasked, DIAG_MT = MT, DIAG_MM = MM, DIAG_NVF = NVF;
    static constexpr bool HD = has_done(MM), HF = has_flag(MM), ANY = HD || HF;
    const float* value; const float* next_value; const float* reward; const float* rho; const float* logp;
    const void* done; const void* flag; float* coef; int T, B; float gamma, scale;
    // rho and logp are only needed by `finish`, which loads them one row per call instead of holding LC rows of them
    // through the scan: that keeps every configuration within 128 VGPRs (no scratch).
    template <int V> struct Row { Pack<V> v0, v1, r; float lam[V]; MaskRow<V, MT> md, mf; };

    template <int V> __device__ void init(long col, bool ok, float (&carry)[V]) const {   // G_T := nv_{T-1}
        const Pack<V> nv = load_pack<V>(NVF ? next_value + row_off(T - 1, col, ok, B, V) : value + row_off(T, col, ok, B, V));
#pragma unroll
        for (int k = 0; k < V; ++k) carry[k] = nv.v[k];
    }
    // the one-step target of a step from its reward, successor value and done mask
    template <int V> __device__ float target(const Pack<V>& r, const Pack<V>& nv, const MaskRow<V, MT>& md, int k) const {
        return fmaf(gamma, HD ? md.keep(k) * nv.v[k] : nv.v[k], r.v[k]);
    }
    // row t+1 in registers (already linked: rows are linked from the end of the chunk backwards), t+1 <= T-1 there:
    // V_{t+1} = its v0 in both forms, q_{t+1} from its r, v1 and done
    template <int V> __device__ void link(Row<V>& row, const Row<V>& nxt) const {
        if (!NVF) row.v1 = nxt.v0;
#pragma unroll
        for (int k = 0; k < V; ++k) row.lam[k] = (target<V>(nxt.r, nxt.v1, nxt.md, k) >= nxt.v0.v[k]) ? 1.f : 0.f;
    }
    template <int V> __device__ void load(Row<V>& row, int t, long col, bool ok, bool next_in_regs) const {
        const size_t o = row_off(t, col, ok, B, V);
        row.v0 = load_pack<V>(value + o);
        if (NVF) row.v1 = load_pack<V>(next_value + o);
        row.r = load_pack<V>(reward + o);
        if (HD) row.md.template load<false>(done, o);
        if (HF) row.mf.template load<false>(flag, o);
        if (next_in_regs) return;
        // A chunk's last row: step t+1 belongs to another wave (or t = T-1).  Its reward, value, successor value and done
        // are fetched here, unconditionally (a load under a branch is waited for before the branch joins): at t = T-1 the
        // row itself stands in for step t+1 (every address stays inside the arrays) and lam_t = 1.
        const bool inner = t < T - 1;
        const size_t o1 = inner ? o + B : o;
        if (!NVF) row.v1 = load_pack<V>(value + o + B);
        const Pack<V> r1 = load_pack<V>(reward + o1);
        const Pack<V> vn = NVF ? load_pack<V>(value + o1) : row.v1;            // V_{t+1}: row t+1 of `value` in both forms
        const Pack<V> nv1 = load_pack<V>(NVF ? next_value + o1 : value + o1 + B);
        MaskRow<V, MT> md1{};
        if (HD) md1.template load<false>(done, o1);
#pragma unroll
        for (int k = 0; k < V; ++k) row.lam[k] = (!inner || target<V>(r1, nv1, md1, k) >= vn.v[k]) ? 1.f : 0.f;
    }
    template <int V> __device__ void coeffs(const Row<V>& row, int, float (&a)[V], float (&b)[V]) const {
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const float kd = HD ? row.md.keep(k) : 1.f;
            const float kf = HF ? row.mf.keep(k) : kd;
            a[k] = (ANY ? gamma * kf : gamma) * row.lam[k];
            b[k] = fmaf((HD ? gamma * kd : gamma) - a[k], row.v1.v[k], row.r.v[k]);
        }
    }
    template <int V> __device__ void finish(const Row<V>& row, int t, long col, bool ok, const float (&s)[V],
                                            const float (&)[V], float (&acc)[NACC]) const {
        const size_t o = row_off(t, col, ok, B, V);
        const Pack<V> rh = load_pack<V>(rho + o);
        const Pack<V> lp = load_pack<V>(logp + o);
        if (!ok) return;
        Pack<V> c;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const float adv = rh.v[k] * (s[k] - row.v0.v[k]);
            acc[0] -= adv * lp.v[k];
            c.v[k] = -adv * scale;
        }
        store_pack<V, true>(coef + (size_t)t * B + col, c);
    }
};

inline bool valid_mask_dtype(int mt) { return mt == HPC_RLL_MASK_U8 || mt == HPC_RLL_MASK_F32; }

// The V-trace scan over a workspace whose logp_t | ent | logp_b slots a head (categorical or Gaussian) has filled:
// ws layout of hpc_rll_vtrace_forward (scan_ops.hip), coef_pg | coef_ent | gv_unit | logp_t | ent | logp_b | partials.
// LR: the logp_b slot holds logp_t - logp_b.
template <bool LR>
int vtrace_masked_scan(const float* value, const float* next_value, const float* reward, const float* weight,
                       const void* done, const void* traj_flag, int mask_dtype, float* losses, float* ws, int T, int B,
                       float gamma, float lambda, float rho_clip, float c_clip, float rho_pg_clip, float scale,
                       hipStream_t st) {
    const size_t TB = (size_t)T * B;
    float *coef_pg = ws, *coef_ent = ws + TB, *gv_unit = ws + 2 * TB, *logp_t = ws + 3 * TB, *ent = ws + 4 * TB,
          *logp_b = ws + 5 * TB, *partials = ws + 6 * TB;
    const ScanCfg c = scan_cfg(T, B, false);   // V = 1, as hpc_rll_vtrace_forward
    const float sc[3] = {scale, scale, scale};
    int rc = HPC_RLL_OK;
    with_mode(mask_dtype, mask_mode(done, traj_flag), next_value != nullptr, [&](auto MT_, auto MM_, auto NV_) {
        using Op = MaskedVtraceOp<decltype(MT_)::value, decltype(MM_)::value, decltype(NV_)::value != 0, LR>;
        const Op op{value, next_value, reward, weight, logp_t, logp_b, ent, done, traj_flag, coef_pg, coef_ent, gv_unit,
                    T, B, gamma, gamma * lambda, rho_clip, c_clip, rho_pg_clip, scale};
        rc = scan_and_finalize<Op, false>(op, c, T, B, partials, 3, sc, losses, st);
    });
    return rc;
}

}  // namespace
}  // namespace hpc_rll

using namespace hpc_rll;

// ------------------------------------------------------------------------------------------------ TD(lambda)
extern "C" int hpc_rll_td_lambda_masked_forward(const float* value, const float* next_value, const float* reward,
                                                const float* weight, int weight_mode, const void* done,
                                                const void* traj_flag, int mask_dtype, float* loss, float* grad_buf,
                                                float* partials, int T, int B, float gamma, float lambda, float scale,
                                                void* stream) {
    if (T < 0 || B < 0 || weight_mode < 0 || weight_mode > 2 || !valid_mask_dtype(mask_dtype)) return HPC_RLL_EINVAL;
    if (!loss) return HPC_RLL_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (T == 0 || B == 0) return (int)hipMemsetAsync(loss, 0, sizeof(float), st);
    if (!value || !reward || !grad_buf || !partials || (weight_mode != 0 && !weight)) return HPC_RLL_EINVAL;
    if (!aligned(value, 4) || !aligned(next_value, 4) || !aligned(reward, 4) || !aligned(weight, 4) ||
        !aligned(grad_buf, 4) || !aligned(partials, 4) || !aligned(loss, 4))
        return HPC_RLL_EALIGN;
    if (mask_dtype == HPC_RLL_MASK_F32 && (!aligned(done, 4) || !aligned(traj_flag, 4))) return HPC_RLL_EALIGN;
    const bool v2 = max_vec(B, mask_dtype, {value, next_value, reward, weight, grad_buf}, {done, traj_flag}) == 2;
    const ScanCfg c = scan_cfg(T, B, v2, true);
    const float disc = gamma * lambda;   // as hpc_rll_td_lambda_forward
    const float sc = 0.5f * scale;
    int rc = HPC_RLL_OK;
    with_mode(mask_dtype, mask_mode(done, traj_flag), next_value != nullptr, [&](auto MT_, auto MM_, auto NV_) {
        using Op = MaskedTdLambdaOp<decltype(MT_)::value, decltype(MM_)::value, decltype(NV_)::value != 0>;
        const Op op{value, next_value, reward, weight, weight_mode, done, traj_flag, grad_buf, T, B,
                    gamma, disc, gamma - disc, scale};
        rc = scan_and_finalize<Op, true, true>(op, c, T, B, partials, 1, &sc, loss, st);
    });
    return rc;
}

// ------------------------------------------------------------------------------------------------ V-trace
extern "C" int hpc_rll_vtrace_masked_forward(const float* target_output, const float* behaviour_output,
                                             const int64_t* action, const float* value, const float* next_value,
                                             const float* reward, const float* weight, const void* done,
                                             const void* traj_flag, int mask_dtype, float* losses, float* ws, int T,
                                             int B, int N, float gamma, float lambda, float rho_clip, float c_clip,
                                             float rho_pg_clip, float scale, void* stream) {
    if (T < 0 || B < 0 || N <= 0 || !losses || !valid_mask_dtype(mask_dtype)) return HPC_RLL_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (T == 0 || B == 0) return (int)hipMemsetAsync(losses, 0, 3 * sizeof(float), st);
    if (!target_output || !behaviour_output || !action || !value || !reward || !ws) return HPC_RLL_EINVAL;
    if (!aligned(target_output, 4) || !aligned(behaviour_output, 4) || !aligned(action, 8) || !aligned(value, 4) ||
        !aligned(next_value, 4) || !aligned(reward, 4) || !aligned(weight, 4) || !aligned(losses, 4) || !aligned(ws, 4))
        return HPC_RLL_EALIGN;
    if (mask_dtype == HPC_RLL_MASK_F32 && (!aligned(done, 4) || !aligned(traj_flag, 4))) return HPC_RLL_EALIGN;
    const size_t TB = (size_t)T * B;   // ws layout of hpc_rll_vtrace_forward (scan_ops.hip)
    float *logp_t = ws + 3 * TB, *ent = ws + 4 * TB, *logp_b = ws + 5 * TB;
    int rc = categorical_forward(target_output, action, logp_t, ent, (long)TB, N, st);
    if (rc) return rc;
    rc = categorical_forward(behaviour_output, action, logp_b, nullptr, (long)TB, N, st);
    if (rc) return rc;
    return vtrace_masked_scan<false>(value, next_value, reward, weight, done, traj_flag, mask_dtype, losses, ws, T, B, gamma,
                                     lambda, rho_clip, c_clip, rho_pg_clip, scale, st);
}

// V-trace for diagonal-Gaussian policies (gaussian.hip: gauss_heads_fwd_kernel): one head launch writes logp_t, ent and the
// log ratio d = logp_t - logp_b into the workspace, and from there on this is hpc_rll_vtrace_masked_forward
// (vtrace_masked_scan): the same Op, with IS = exp(d) instead of exp(logp_t - logp_b), the same configuration for the same
// (T, B), and its dispatch record.  d goes to the scan as it is because logp_t is of size ~1.4 A: a logp_b = logp_t - d rounded to
// fp32 gives d back only to half an ulp of logp_t (6e-5 at A = 1024), which the policy loss inherits whatever T*B is.
extern "C" int hpc_rll_vtrace_continuous_forward(const float* mu_target, const float* sigma_target,
                                                 const float* mu_behaviour, const float* sigma_behaviour,
                                                 const float* action, const float* value, const float* next_value,
                                                 const float* reward, const float* weight, const void* done,
                                                 const void* traj_flag, int mask_dtype, float* losses, float* ws, int T,
                                                 int B, int A, float gamma, float lambda, float rho_clip, float c_clip,
                                                 float rho_pg_clip, float scale, void* stream) {
    if (T < 0 || B < 0 || A <= 0 || !losses || !valid_mask_dtype(mask_dtype)) return HPC_RLL_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const bool empty = T == 0 || B == 0;
    if (!empty && (!mu_target || !sigma_target || !mu_behaviour || !sigma_behaviour || !action || !value || !reward || !ws))
        return HPC_RLL_EINVAL;
    if (!aligned(mu_target, 4) || !aligned(sigma_target, 4) || !aligned(mu_behaviour, 4) || !aligned(sigma_behaviour, 4) ||
        !aligned(action, 4) || !aligned(value, 4) || !aligned(next_value, 4) || !aligned(reward, 4) || !aligned(weight, 4) ||
        !aligned(losses, 4) || !aligned(ws, 4))
        return HPC_RLL_EALIGN;
    if (mask_dtype == HPC_RLL_MASK_F32 && (!aligned(done, 4) || !aligned(traj_flag, 4))) return HPC_RLL_EALIGN;
    if (A > 1024) return HPC_RLL_EUNSUPPORTED;   // the head's limit (gaussian.hip), after the null checks
    if (empty) return (int)hipMemsetAsync(losses, 0, 3 * sizeof(float), st);
    const size_t TB = (size_t)T * B;   // ws layout of hpc_rll_vtrace_forward (scan_ops.hip)
    float *logp_t = ws + 3 * TB, *ent = ws + 4 * TB, *logp_b = ws + 5 * TB;
    int rc = gaussian_heads_forward(mu_target, sigma_target, mu_behaviour, sigma_behaviour, action, logp_t, ent, logp_b,
                                    /*log_ratio=*/true, (long)TB, A, st);
    if (rc) return rc;
    return vtrace_masked_scan<true>(value, next_value, reward, weight, done, traj_flag, mask_dtype, losses, ws, T, B, gamma,
                                    lambda, rho_clip, c_clip, rho_pg_clip, scale, st);
}

// ------------------------------------------------------------------------------------------------ UPGO
extern "C" int hpc_rll_upgo_masked_forward(const float* target_output, const float* rho, const int64_t* action,
                                           const float* reward, const float* value, const float* next_value,
                                           const void* done, const void* traj_flag, int mask_dtype, float* loss, float* ws,
                                           int T, int B, int N, float gamma, float scale, void* stream) {
    if (T < 0 || B < 0 || N <= 0 || !loss || !valid_mask_dtype(mask_dtype)) return HPC_RLL_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (T == 0 || B == 0) return (int)hipMemsetAsync(loss, 0, sizeof(float), st);
    if (!target_output || !rho || !action || !reward || !value || !ws) return HPC_RLL_EINVAL;
    if (!aligned(target_output, 4) || !aligned(rho, 4) || !aligned(action, 8) || !aligned(reward, 4) || !aligned(value, 4) ||
        !aligned(next_value, 4) || !aligned(loss, 4) || !aligned(ws, 4))
        return HPC_RLL_EALIGN;
    if (mask_dtype == HPC_RLL_MASK_F32 && (!aligned(done, 4) || !aligned(traj_flag, 4))) return HPC_RLL_EALIGN;
    const size_t TB = (size_t)T * B;   // ws layout of hpc_rll_upgo_forward (scan_ops.hip)
    float *coef = ws, *logp = ws + TB, *partials = ws + 2 * TB;
    int rc = categorical_forward(target_output, action, logp, nullptr, (long)TB, N, st);
    if (rc) return rc;
    const ScanCfg c = scan_cfg(T, B, false);   // V = 1, as hpc_rll_upgo_forward
    with_mode(mask_dtype, mask_mode(done, traj_flag), next_value != nullptr, [&](auto MT_, auto MM_, auto NV_) {
        using Op = MaskedUpgoOp<decltype(MT_)::value, decltype(MM_)::value, decltype(NV_)::value != 0>;
        const Op op{value, next_value, reward, rho, logp, done, traj_flag, coef, T, B, gamma, scale};
        rc = scan_and_finalize<Op, false>(op, c, T, B, partials, 1, &scale, loss, st);
    });
    return rc;
}
