// coma.hip -- COMA, the counterfactual multi-agent actor-critic loss, on gfx950: the three losses of DI-engine's coma_error
// over (T,B,A,N) logits and action values in a head launch, a scan launch and one streaming backward.
//
// No reference counterpart; the semantics restate DI-engine's coma_error (Foerster et al. 2018).  Per row (t,b,i) with x the
// logit row, q and q' the rows of q_value and target_q_value, a the action and w the weight:
//   l = log_softmax(x), pi = exp l, H = -sum_n pi_n l_n, qa = q[a], tqa = q'[a], adv = qa - sum_n pi_n q_n   (adv: a constant)
// and per column (b,i), with k_t = 1 - done[t,b] (1 without done), disc = gamma*lambda (fp32), rest = gamma - disc:
//   R_{T-2} = r[T-2,b] + k_{T-2} gamma tqa_{T-1},     R_t = r[t,b] + k_t (disc R_{t+1} + rest tqa_{t+1})      (R: a constant)
//   policy = -mean_{T,B,A} w l_a adv,   entropy = mean_{T,B,A} w H,   q = mean_{T-1,B,A} w (R_t - qa_t)^2
//   grad_logit[n]   = -g_p w adv scale_pe ([n = a] - pi_n) + g_e w scale_pe (-pi_n (l_n + H))
//   grad_q_value[n] =  g_q 2 w (qa - R) scale_q [n = a]   (t < T-1; row T-1 is zero).
//
// Three stages:
//   * coma_heads_fwd_kernel on the mapping of rowgroup.hpp over rows = T*B*A: a row of N values is owned by a group of G
//     lanes, lane gl holds a RowSlice of the logit, q_value and target_q_value rows.  Softmax statistics and the selected
//     logit as Retrace's heads form them, then one group reduction each for the baseline sum e_n q_n and for sum e_n (x_n - m)
//     (H = log s - that / s), and the two selected values.  l_a = (x_a - m) - log s in ONE expression.  Per row it stores
//     qa and tqa for the scan and the three floats the backward needs to do without a reduction: lse = m + log s, H and
//     the policy coefficient w adv scale_pe.  The policy and entropy sums leave through publish_sums (at most kFoldMaxGrid
//     looping workgroups); the launch publishes THREE sums in the order of loss[3], the middle one zero: the scan's fold
//     overwrites it later on the same stream, and T = 1 (no scan) needs nothing more.
//   * ComaOp on the shared reverse column scan: T-1 steps over C = B*A columns, V = 1, scan_cfg(T-1, C, false).  Row t loads
//     tqa[t+1], qa[t], the action (whether the q term counts), and reward / done at (t, col / A): up to A neighbouring lanes
//     share those addresses.  init gives s = tqa[T-1] (disc + rest = gamma), finish accumulates w d^2 with d = qa - R and
//     stores delta = 2 w d scale_q with a nontemporal store.
//   * coma_bwd_kernel, again on the rowgroup mapping (DESIGN.md says why not stream_write.hpp's): the logit row is read
//     once, pi_n = exp(x_n - lse) is recomputed, and both gradient rows are written once, 16 bytes per store where the bases
//     and N allow it.  An absent output is neither computed nor written.
//
// -inf logits (masked actions) are clamped to the most negative finite float, as categorical.hip, retrace.hip and acer.hip
// do.  Such a column has e_n = 0 and every sum SELECTS on e_n > 0 (pi_n > 0 in the backward) instead of multiplying: it adds
// exactly 0 to H and the baseline, whatever its q is, and its gradient is 0.  An action outside [0,N) matches no column:
// qa = tqa = 0, the policy coefficient is 0 and the scan drops the row's q term; nothing is addressed with it.
// N = 1: lse = x exactly, pi = 1, l = H = 0 and the one-hot part cancels cp * pi exactly: the gradient is identically zero.
//
// Algorithmic HBM bytes per row (t,b,i): heads 12 N + 8 (+ 4 weight) read, 20 written; scan 16 read (qa, tqa, action: 8)
// + 4 weight + (4 + mask element) / A, 4 written; backward 4 N + 8 + 12 (+ 4 weight) + 4 read, 8 N written (4 N per output).
#include <hip/hip_runtime.h>

#include "colscan.hpp"
#include "hostutil.hpp"
#include "hpc_rll_hip.h"
#include "masks.hpp"
#include "rowgroup.hpp"
#include "wave.hpp"

namespace hpc_rll {
namespace {

constexpr int kComaMaxN = kRowTableMaxN;   // 64 lanes x 16 floats per lane and input
constexpr int kComaSums = 3;               // the order of loss[3]: policy, q (zero here: the scan's), entropy

// ================================================================================================
// the heads
// ================================================================================================
struct ComaHeadArgs {
    const float* logit; const float* q; const float* tq; const int64_t* action; const float* weight;
    float* qa; float* tqa; float* lse; float* ent; float* pc; long rows; int N; float scale_pe;
};

// HW: weight given (the null case loads nothing)
template <int G, int VEC, int E, bool HW>
__global__ __launch_bounds__(256) void coma_heads_fwd_kernel(const ComaHeadArgs p, float* __restrict__ partials,
                                                             const ScanFold fold) {
    constexpr int GPB = 256 / G;
    constexpr int R = RowsPerIter<VEC, E>::value;
    const int gl = threadIdx.x % G;
    const int gi = threadIdx.x / G;
    const int N = p.N;
    const long stride = (long)gridDim.x * GPB * R;
    float acc[kComaSums] = {0.f, 0.f, 0.f};   // policy, q (zero here: the scan's), entropy
    for (long bb = (long)blockIdx.x * GPB * R; bb < p.rows; bb += stride) {
        RowSlice<G, VEC, E> xs[R], qs[R], ts[R];
        long a[R];
        float wt[R];
#pragma unroll
        for (int k = 0; k < R; ++k) {
            long row = bb + (long)k * GPB + gi;
            if (row >= p.rows) row = p.rows - 1;           // (re-reads the last row; sums and stores below are guarded)
            const long off = row * (long)N;
            xs[k].load(p.logit + off, N, gl);
            qs[k].load(p.q + off, N, gl);
            ts[k].load(p.tq + off, N, gl);
            a[k] = p.action[row];                          // (every lane: the same address per group, one request)
            wt[k] = HW ? p.weight[row] : 1.f;
        }
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const float* x = xs[k].x;
            const float* q = qs[k].x;
            const float* tq = ts[k].x;
            const int ai = action_index(a[k], N);
            const float m = row_max_finite<G, VEC, E>(x, N, gl);
            // ---- partition sum, baseline, sum e (x - m) and the three selected entries
            float s = 0.f, bq = 0.f, sxm = 0.f, xa = 0.f, qsel = 0.f, tsel = 0.f;
#pragma unroll
            for (int e = 0; e < E; ++e)
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    const int i = e * VEC + j;
                    const int c = (e * G + gl) * VEC + j;
                    const float d = fmaxf(x[i], -kFltMax) - m;
                    const float ex = (c < N) ? __expf(d) : 0.f;
                    const bool sel = ex > 0.f;
                    s += ex;
                    bq = sel ? fmaf(ex, q[i], bq) : bq;
                    sxm = sel ? fmaf(ex, d, sxm) : sxm;
                    xa = (c == ai) ? d : xa;
                    qsel = (c == ai) ? q[i] : qsel;
                    tsel = (c == ai) ? tq[i] : tsel;
                }
            s = group_all<G, AddOp>(s);
            bq = group_all<G, AddOp>(bq);
            sxm = group_all<G, AddOp>(sxm);
            xa = group_all<G, AddOp>(xa);                  // at most one lane holds a nonzero value
            qsel = group_all<G, AddOp>(qsel);
            tsel = group_all<G, AddOp>(tsel);
            const float ls = logf(s);
            const float h = ls - sxm / s;
            const float la = xa - ls;                      // (x_a - m) - log s
            const float adv = qsel - bq / s;
            const float pterm = ai >= 0 ? la * adv : 0.f;
            const long row = bb + (long)k * GPB + gi;
            if (row < p.rows) {
                acc[0] = HW ? fmaf(wt[k], pterm, acc[0]) : acc[0] + pterm;
                acc[2] = HW ? fmaf(wt[k], h, acc[2]) : acc[2] + h;
                if (gl == 0) {
                    p.qa[row] = qsel;
                    p.tqa[row] = tsel;
                    p.lse[row] = m + ls;
                    p.ent[row] = h;
                    p.pc[row] = ai >= 0 ? (HW ? wt[k] * adv : adv) * p.scale_pe : 0.f;
                }
            }
        }
    }
    // every lane of a group holds the same row terms: lane 0 of each group counts
    if (gl != 0) { acc[0] = 0.f; acc[2] = 0.f; }
    publish_block_sums<kComaSums, 256>(acc, partials, fold);
}

// The dispatch records of the heads and the backward (hpc_rll_coma_last_config): {launches so far, G, VEC, E, R, flags, grid}
constexpr int kLaunchInts = 7;
LaunchRecord<kLaunchInts> g_coma_heads, g_coma_bwd;

template <bool HW>
int coma_heads(const ComaHeadArgs& p, float* partials, float* loss, hipStream_t st) {
    const RowCfg cfg = row_cfg(p.N, aligned(p.logit, 16) && aligned(p.q, 16) && aligned(p.tq, 16), kRow4Pieces);
    const float sc[kComaSums] = {-p.scale_pe, 0.f, p.scale_pe};
    return with_row4(cfg, [&](auto G_, auto V_, auto E_) {
        constexpr int G = G_, V = V_, E = E_, R = RowsPerIter<V, E>::value;
        long grid = 0;
        const int rc = launch_rows_folded(p.rows, (256 / G) * R, kComaSums, sc, loss, partials, st, &grid,
                                          [&](unsigned blocks, const ScanFold& fold) {
            hipLaunchKernelGGL((coma_heads_fwd_kernel<G, V, E, HW>), dim3(blocks), dim3(256), 0, st, p, partials, fold);
        });
        if (grid) g_coma_heads.note({G, V, E, R, HW ? 1 : 0, (int)grid});
        return rc;
    });
}

// ================================================================================================
// the scan over T-1 steps and C = B*A columns.  MT: mask element type; HAS_DONE / HW: done / weight given
// ================================================================================================
template <int MT, bool HAS_DONE, bool HW>
struct ComaOp {
    static constexpr int NACC = 1, DIAG_OP = kScanOpComa, DIAG_MT = MT, DIAG_MM = HAS_DONE ? MM_DONE : MM_NONE,
                         DIAG_NVF = HW ? 1 : 0;
    const float* reward; const void* done; const float* weight; const int64_t* action; const float* qa; const float* tqa;
    float* delta; int T1, C, B, A, N; float disc, rest, scale_q;   // T1 = T-1 steps; reward and done have B columns
    template <int V> struct Row { float r, tq1, qa0; MaskRow<1, MT> k; long a; };

    template <int V> __device__ void init(long col, bool ok, float (&carry)[V]) const {   // s_{T-1} = tqa_{T-1}
        static_assert(V == 1, "one column per lane");
        carry[0] = tqa[row_off(T1, col, ok, C, 1)];
    }
    template <int V> __device__ void load(Row<V>& row, int t, long col, bool ok, bool) const {
        // every load is unconditional and in bounds: columns past C load the row's last one
        const int cc = ok ? (int)col : C - 1;
        const size_t o = (size_t)t * C + cc;
        const size_t ob = (size_t)t * B + (size_t)(cc / A);   // up to A neighbouring lanes share this address
        row.r = reward[ob];
        if (HAS_DONE) row.k.template load<false>(done, ob);
        row.qa0 = qa[o];
        row.tq1 = tqa[o + C];                                  // t <= T-2: row t+1 exists
        row.a = action[o];
    }
    template <int V> __device__ void link(Row<V>&, const Row<V>&) const {}
    template <int V> __device__ void coeffs(const Row<V>& row, int, float (&a)[V], float (&b)[V]) const {
        if (HAS_DONE) {
            const float k = row.k.keep(0);
            a[0] = k * disc;
            b[0] = fmaf(k * rest, row.tq1, row.r);
        } else {
            a[0] = disc;
            b[0] = fmaf(rest, row.tq1, row.r);
        }
    }
    template <int V> __device__ void finish(const Row<V>& row, int t, long col, bool ok, const float (&s)[V],
                                            const float (&)[V], float (&acc)[1]) const {
        float w = 1.f;
        if (HW) w = weight[row_off(t, col, ok, C, 1)];
        if (!ok) return;
        const bool valid = row.a >= 0 && row.a < (long)N;
        const float d = row.qa0 - s[0];
        const float wd = HW ? w * d : d;
        if (valid) acc[0] = fmaf(wd, d, acc[0]);
        __builtin_nontemporal_store(valid ? (2.f * wd) * scale_q : 0.f, delta + (size_t)t * C + col);
    }
};

int coma_scan(const float* reward, const void* done, int mt, const float* weight, const int64_t* action, const float* qa,
              const float* tqa, float* delta, float* loss_q, float* partials, int T, int B, int A, int N, float gamma,
              float lambda, float scale_q, hipStream_t st) {
    const int T1 = T - 1, C = B * A;
    const ScanCfg cfg = scan_cfg(T1, C, false);   // V = 1
    const float disc = gamma * lambda, rest = gamma - disc;
    int rc = HPC_RLL_OK;
    auto run = [&](auto MT_, auto HD_, auto HW_) {
        using Op = ComaOp<decltype(MT_)::value, decltype(HD_)::value, decltype(HW_)::value>;
        const Op op{reward, done, weight, action, qa, tqa, delta, T1, C, B, A, N, disc, rest, scale_q};
        rc = scan_and_finalize<Op, false>(op, cfg, T1, C, partials, 1, &scale_q, loss_q, st);
    };
    using Yes = std::true_type;
    using No = std::false_type;
    auto with_w = [&](auto MT_, auto HD_) {
        if (weight) run(MT_, HD_, Yes{});
        else run(MT_, HD_, No{});
    };
    if (!done) with_w(I<0>{}, No{});
    else if (mt == HPC_RLL_MASK_F32) with_w(I<1>{}, Yes{});
    else with_w(I<0>{}, Yes{});
    return rc;
}

// ================================================================================================
// backward: rows = T*B*A rows of N floats per output, each float written once; no reduction, no atomics
// ================================================================================================
struct ComaBwdArgs {
    const float* g_p; const float* g_q; const float* g_e; const float* logit; const int64_t* action; const float* weight;
    const float* lse; const float* ent; const float* pc; const float* delta; float* grad_logit; float* grad_q;
    long rows, rows_q; int N; float scale_pe;   // rows_q = (T-1)*B*A: the rows that have a return
};

// GL / GQ: grad_logit / grad_q_value wanted; HW: weight given (it enters grad_logit only)
template <int G, int VEC, int E, bool GL, bool GQ, bool HW>
__global__ __launch_bounds__(256) void coma_bwd_kernel(const ComaBwdArgs p) {
    constexpr int GPB = 256 / G;
    constexpr int R = RowsPerIter<VEC, E>::value;
    const int gl = threadIdx.x % G;
    const int gi = threadIdx.x / G;
    const int N = p.N;
    const float gp = (GL && p.g_p) ? p.g_p[0] : 1.f;
    const float ge = (GL && p.g_e) ? p.g_e[0] : 1.f;
    const float gq = (GQ && p.g_q) ? p.g_q[0] : 1.f;
    const long last_q = p.rows_q > 0 ? p.rows_q - 1 : 0;   // (the delta region holds `rows` floats: index 0 is in bounds)
    const long stride = (long)gridDim.x * GPB * R;
    for (long bb = (long)blockIdx.x * GPB * R; bb < p.rows; bb += stride) {
        RowSlice<G, VEC, E> xs[R];
        long a[R];
        float lse[R], h[R], cp[R], ce[R], dq[R];
#pragma unroll
        for (int k = 0; k < R; ++k) {
            long row = bb + (long)k * GPB + gi;
            if (row >= p.rows) row = p.rows - 1;           // (re-reads the last row; the stores below are guarded)
            a[k] = p.action[row];
            if (GL) {
                xs[k].load(p.logit + row * (long)N, N, gl);
                lse[k] = p.lse[row];
                h[k] = p.ent[row];
                cp[k] = p.pc[row];
                ce[k] = HW ? p.weight[row] * p.scale_pe : p.scale_pe;
            }
            if (GQ) {
                const float d = p.delta[row < p.rows_q ? row : last_q];   // rows of t = T-1: in bounds, result unused
                dq[k] = row < p.rows_q ? gq * d : 0.f;
            }
        }
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const long row = bb + (long)k * GPB + gi;
            const bool live = row < p.rows;
            const int ai = action_index(a[k], N);
            const float cpk = GL ? gp * cp[k] : 0.f, cek = GL ? ge * ce[k] : 0.f;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const int c0 = (e * G + gl) * VEC;
                float ol[VEC], oq[VEC];
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    const int c = c0 + j;
                    if (GL) {
                        const float l = fmaxf(xs[k].x[e * VEC + j], -kFltMax) - lse[k];
                        const float pi = expf(l);
                        // -cp ([n = a] - pi) + ce (-pi (l + H)); a column of pi = 0 is selected out
                        const float v = fmaf(cek, -pi * (l + h[k]), cpk * pi);
                        ol[j] = pi > 0.f ? (c == ai ? v - cpk : v) : 0.f;
                    }
                    if (GQ) oq[j] = (c == ai) ? dq[k] : 0.f;
                }
                if (live && c0 < N) {
                    const long o = row * (long)N + c0;
                    if (GL) store_piece<VEC>(p.grad_logit + o, ol);
                    if (GQ) store_piece<VEC>(p.grad_q + o, oq);
                }
            }
        }
    }
}

template <bool GL, bool GQ, bool HW>
int coma_backward(const ComaBwdArgs& p, hipStream_t st) {
    // an absent operand restricts nothing; logit counts only when it is read
    const RowCfg cfg = row_cfg(p.N, aligned(GL ? p.logit : nullptr, 16) && aligned(p.grad_logit, 16) && aligned(p.grad_q, 16),
                               kRow4Pieces);
    return with_row4(cfg, [&](auto G_, auto V_, auto E_) {
        constexpr int G = G_, V = V_, E = E_, R = RowsPerIter<V, E>::value;
        const unsigned grid = row_grid(p.rows, (256 / G) * R, kUnfoldedGridCap);
        hipLaunchKernelGGL((coma_bwd_kernel<G, V, E, GL, GQ, HW>), dim3(grid), dim3(256), 0, st, p);
        const int rc = last_error();
        if (!rc) g_coma_bwd.note({G, V, E, R, (GL ? 1 : 0) | (GQ ? 2 : 0) | (HW ? 4 : 0), (int)grid});
        return rc;
    });
}

// B*A columns must fit an int
inline bool cols_fit(int B, int A) { return (int64_t)B * A <= (int64_t)INT32_MAX; }
// floats of the two partial-sum regions: the heads' (kComaSums per workgroup of at most kFoldMaxGrid) and the scan's (one
// per workgroup; its narrowest tile is 8 columns)
constexpr int64_t kHeadPartials = 8 * (kFoldMaxGrid + 1);
inline int64_t scan_partials(int64_t C) { return 8 * ((C + 7) / 8 + 1); }

}  // namespace
}  // namespace hpc_rll

using namespace hpc_rll;

// ws (floats), R = T*B*A: delta | qa | tqa | lse | H | w adv scale_pe (R each) | the heads' partial sums | the scan's
extern "C" int64_t hpc_rll_coma_workspace_floats(int T, int B, int A) {
    if (T < 0 || B < 0 || A < 0 || !cols_fit(B, A)) return HPC_RLL_EINVAL;
    const int64_t C = (int64_t)B * A;
    return 6 * (int64_t)T * C + kHeadPartials + scan_partials(C);
}

extern "C" int hpc_rll_coma_forward(const float* logit, const int64_t* action, const float* q_value,
                                    const float* target_q_value, const float* reward, const float* weight, const void* done,
                                    int mask_dtype, float* loss, float* ws, int T, int B, int A, int N, float gamma,
                                    float lambda, float scale_pe, float scale_q, void* stream) {
    const bool empty = T == 0 || B == 0 || A == 0;
    if (!loss) return HPC_RLL_EINVAL;
    if (!empty && (!logit || !action || !q_value || !target_q_value || !reward || !ws)) return HPC_RLL_EINVAL;
    if (T < 0 || B < 0 || A < 0 || N <= 0 || !cols_fit(B, A)) return HPC_RLL_EINVAL;
    if (mask_dtype != HPC_RLL_MASK_U8 && mask_dtype != HPC_RLL_MASK_F32) return HPC_RLL_EINVAL;
    if (!aligned(logit, 4) || !aligned(action, 8) || !aligned(q_value, 4) || !aligned(target_q_value, 4) ||
        !aligned(reward, 4) || !aligned(weight, 4) || !aligned(done, mask_dtype == HPC_RLL_MASK_F32 ? 4 : 1) ||
        !aligned(loss, 4) || !aligned(ws, 4))
        return HPC_RLL_EALIGN;
    if (N > kComaMaxN) return HPC_RLL_EUNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    if (empty) return (int)hipMemsetAsync(loss, 0, kComaSums * sizeof(float), st);
    const size_t C = (size_t)B * A, R = (size_t)T * C;
    float *delta = ws, *qa = ws + R, *tqa = ws + 2 * R, *lse = ws + 3 * R, *ent = ws + 4 * R, *pc = ws + 5 * R;
    float *head_partials = ws + 6 * R, *scan_part = head_partials + kHeadPartials;
    const ComaHeadArgs p{logit, q_value, target_q_value, action, weight, qa, tqa, lse, ent, pc, (long)R, N, scale_pe};
    int rc = weight ? coma_heads<true>(p, head_partials, loss, st) : coma_heads<false>(p, head_partials, loss, st);
    if (rc || T == 1) return rc;   // T = 1: no return, loss[1] = 0 is the heads'
    return coma_scan(reward, done, mask_dtype, weight, action, qa, tqa, delta, loss + 1, scan_part, T, B, A, N, gamma, lambda,
                     scale_q, st);
}

extern "C" int hpc_rll_coma_backward(const float* g_policy, const float* g_q, const float* g_entropy, const float* logit,
                                     const int64_t* action, const float* weight, const float* ws, float* grad_logit,
                                     float* grad_q_value, int T, int B, int A, int N, float scale_pe, void* stream) {
    const bool empty = T == 0 || B == 0 || A == 0 || (!grad_logit && !grad_q_value);
    if (!empty && (!action || !ws || (grad_logit && !logit))) return HPC_RLL_EINVAL;
    if (T < 0 || B < 0 || A < 0 || N <= 0 || !cols_fit(B, A)) return HPC_RLL_EINVAL;
    if (!aligned(g_policy, 4) || !aligned(g_q, 4) || !aligned(g_entropy, 4) || !aligned(logit, 4) || !aligned(action, 8) ||
        !aligned(weight, 4) || !aligned(ws, 4) || !aligned(grad_logit, 4) || !aligned(grad_q_value, 4))
        return HPC_RLL_EALIGN;
    if (N > kComaMaxN) return HPC_RLL_EUNSUPPORTED;
    if (empty) return HPC_RLL_OK;
    hipStream_t st = (hipStream_t)stream;
    const size_t C = (size_t)B * A, R = (size_t)T * C;
    const ComaBwdArgs p{g_policy, g_q, g_entropy, logit, action, weight, ws + 3 * R, ws + 4 * R, ws + 5 * R, ws,
                        grad_logit, grad_q_value, (long)R, (long)(R - C), N, scale_pe};
    if (!grad_logit) return coma_backward<false, true, false>(p, st);
    if (grad_q_value) return weight ? coma_backward<true, true, true>(p, st) : coma_backward<true, true, false>(p, st);
    return weight ? coma_backward<true, false, true>(p, st) : coma_backward<true, false, false>(p, st);
}

extern "C" int hpc_rll_coma_last_config(int* out) {
    if (!out) return HPC_RLL_EINVAL;
    const int rc = scan_read_record(kScanOpComa, out);
    if (rc) return rc;
    g_coma_heads.read(out + HPC_RLL_SCAN_CONFIG_INTS);
    g_coma_bwd.read(out + HPC_RLL_SCAN_CONFIG_INTS + kLaunchInts);
    return HPC_RLL_OK;
}
static_assert(HPC_RLL_COMA_CONFIG_INTS == HPC_RLL_SCAN_CONFIG_INTS + 2 * 7, "the layout documented in hpc_rll_hip.h");
