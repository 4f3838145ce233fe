// retrace.hip -- Retrace(lambda): off-policy multi-step Q targets for discrete actions and ACER's critic loss on gfx950.
//
// No reference counterpart; the semantics are DI-engine's compute_q_retraces and acer_value_error.  With a_t = action[t,b],
// qa_t = q_values[t,b,a_t], v_t the state value (t = 0..T), w_t the continuation weight and c_t = lambda*min(1, ratio_t):
//   Q_T = v_T,   Q_t = r_t + gamma*w_t*(c_{t+1}*(Q_{t+1} - qa_{t+1}) + v_{t+1}),  the c*(Q - qa) term := 0 at t+1 = T
// which is a first-order affine recurrence s_t = b_t + a_t*s_{t+1} walked backwards in time (colscan.hpp) with
//   a_t = (gamma*w_t)*c_{t+1}   (0 at t = T-1),      b_t = fmaf(gamma*w_t, fmaf(-c_{t+1}, qa_{t+1}, v_{t+1}), r_t).
// A zero weight gives a_t = 0 and b_t = r_t, so Q_t = r_t exactly; weights == NULL multiplies nothing (gamma*1.0f is gamma:
// the same bits as all-ones weights).  Critic loss = scale * 0.5 * sum_{t<T,b} lw (Q_t - qa_t)^2 with Q a constant, so
//   grad_q_values[t,b,n] = g * lw*(qa_t - Q_t)*scale * [n == a_t]   (t < T; row T is zero).
//
// Three stages, every array read or written once:
//   * per (t,b) streams v (T+1,B), qa (T,B), c (T,B).  The drop-in form (v_pred and a (T,B,N) ratio are given) gathers qa and c
//     with one thread per sample (retrace_gather_kernel).  The fused form computes them from the logits in
//     retrace_heads_fwd_kernel on the mapping of rowgroup.hpp: a row of N values is owned by a group of G lanes, lane gl
//     holds a RowSlice of the q_values, target_output and behaviour_output rows (3 inputs x R rows x E*VEC floats per lane); pi = softmax(target), v = sum pi q,
//     log ratio = ((x_a - max_t) - (y_a - max_b)) - (log s_t - log s_b) in ONE expression from the two rows' statistics (no
//     two separately rounded log-probabilities).  Rows of N % 4 != 0 (or a base off 16 bytes) take 4-byte loads.  Rows of
//     t = T have no behaviour row and no action: they re-read behaviour row (T-1,b) (every load stays unconditional and in
//     bounds) and store v only.
//   * RetraceOp on the shared reverse column scan, V = 1, the configuration rule of V-trace and UPGO (scan_cfg(T, B, false)).
//     A row holds r, w and its own v, c, qa; the step-(t+1) fields come from row t+1 when the same wave holds it (link) and
//     are loaded at +B by a chunk's last row (at t = T-1: v_T, c = 0, and the row's own address for c and qa).  The own v and
//     c of a chunk's first row feed nothing and their loads are dropped by the compiler.  finish stores Q_t and, in the fused
//     form, accumulates the loss and stores delta = lw*(qa_t - Q_t)*scale.  init writes row T of q_retraces (= v_T).
//   * the backward (onehot_stream_kernel of stream_write.hpp) writes all (T+1)*B*N gradient floats once (16-byte nontemporal
//     stores, every workgroup's 256 stores one 4 KiB-aligned block): g*delta at column a_t, zeros elsewhere.  No atomics,
//     q_values is not read.
//
// Algorithmic HBM bytes: heads 4 N (3 T B + 2 B) read (+ 8 T B action), 12 T B + 4 B written; scan 24 B per sample (r, v, c,
// qa read, Q, delta written) + 4 each for weights and loss_weight; backward 4 N (T+1) B written, 12 T B read.
// An action outside [0,N) matches no column: qa = 0, the drop-in form's ratio is 0, the fused form takes x_a = y_a = 0, and
// the gradient row is all zeros.  Nothing is addressed with it.
#include <hip/hip_runtime.h>

#include "colscan.hpp"
#include "hostutil.hpp"
#include "hpc_rll_hip.h"
#include "rowgroup.hpp"
#include "stream_write.hpp"
#include "wave.hpp"

namespace hpc_rll {
namespace {

constexpr int kRetraceMaxN = kRowTableMaxN;   // 64 lanes x 16 floats per lane and input

// ================================================================================================
// drop-in form: qa = q_values[t,b,a], c = lambda*min(1, ratio[t,b,a]) as coalesced (T,B) streams
// ================================================================================================
__global__ __launch_bounds__(256) void retrace_gather_kernel(const float* __restrict__ q, const float* __restrict__ ratio,
                                                             const int64_t* __restrict__ action, float* __restrict__ qa,
                                                             float* __restrict__ c, long TB, int N, float lambda) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= TB) return;
    const long a = action[i];
    const bool ok = a >= 0 && a < (long)N;
    const size_t idx = (size_t)i * N + (ok ? (size_t)a : 0);
    const float qv = q[idx], rv = ratio[idx];
    qa[i] = ok ? qv : 0.f;
    c[i] = lambda * fminf(1.f, ok ? rv : 0.f);
}

// ================================================================================================
// fused form: the heads
// ================================================================================================
// maximum, partition sum (relative to the maximum) and the selected logit of a row, in every lane of the group; -inf logits
// (masked actions) are clamped to the most negative finite float as categorical.hip does, padding counts as that value
template <int G, int VEC, int E>
__device__ __forceinline__ void softmax_stats(const RowSlice<G, VEC, E>& r, int N, int gl, int ai, float (&ex)[E * VEC],
                                              float& m, float& s, float& xa) {
    m = row_max_finite<G, VEC, E>(r.x, N, gl);
    float sum = 0.f, sel = 0.f;
#pragma unroll
    for (int e = 0; e < E; ++e)
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const int i = e * VEC + k;
            const int c = (e * G + gl) * VEC + k;
            const float x = fmaxf(r.x[i], -kFltMax);
            ex[i] = (c < N) ? __expf(x - m) : 0.f;
            sum += ex[i];
            sel = (c == ai) ? x : sel;
        }
    s = group_all<G, AddOp>(sum);
    xa = group_all<G, AddOp>(sel);   // at most one lane holds a nonzero value
}

// rows = (T+1)*B rows of q_values and target_output, TB = T*B rows of behaviour_output and action
template <int G, int VEC, int E>
__global__ __launch_bounds__(256) void retrace_heads_fwd_kernel(const float* __restrict__ q, const float* __restrict__ tgt,
                                                                const float* __restrict__ beh,
                                                                const int64_t* __restrict__ action, float* __restrict__ v_out,
                                                                float* __restrict__ qa_out, float* __restrict__ c_out,
                                                                long rows, long TB, long B, int N, float lambda) {
    constexpr int GPB = 256 / G;
    constexpr int R = RowsPerIter<VEC, E>::value;
    const int gl = threadIdx.x % G;
    const int gi = threadIdx.x / G;
    const long stride = (long)gridDim.x * GPB * R;
    for (long bb = (long)blockIdx.x * GPB * R; bb < rows; bb += stride) {
        RowSlice<G, VEC, E> qs[R], ts[R], bs[R];
        long a[R];
#pragma unroll
        for (int k = 0; k < R; ++k) {
            long row = bb + (long)k * GPB + gi;
            if (row >= rows) row = rows - 1;               // (re-reads the last row; the stores below are guarded)
            const long brow = row < TB ? row : row - B;    // rows of t = T: behaviour row (T-1,b), in bounds, result unused
            qs[k].load(q + row * (long)N, N, gl);
            ts[k].load(tgt + row * (long)N, N, gl);
            bs[k].load(beh + brow * (long)N, N, gl);
            a[k] = action[brow];
        }
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const int ai = action_index(a[k], N);
            float ex[E * VEC], eb[E * VEC];
            float mt, st, xa, mb, sb, ya;
            softmax_stats<G, VEC, E>(ts[k], N, gl, ai, ex, mt, st, xa);
            softmax_stats<G, VEC, E>(bs[k], N, gl, ai, eb, mb, sb, ya);
            float vq = 0.f, qsel = 0.f;
#pragma unroll
            for (int e = 0; e < E; ++e)
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    const int i = e * VEC + j;
                    const int c = (e * G + gl) * VEC + j;
                    vq = (c < N) ? fmaf(ex[i], qs[k].x[i], vq) : vq;
                    qsel = (c == ai) ? qs[k].x[i] : qsel;
                }
            vq = group_all<G, AddOp>(vq);
            qsel = group_all<G, AddOp>(qsel);
            const long row = bb + (long)k * GPB + gi;
            if (gl == 0 && row < rows) {
                v_out[row] = vq / st;
                if (row < TB) {
                    // log pi(a) - log mu(a) from the two rows' statistics in one expression
                    const float d = ((xa - mt) - (ya - mb)) - (logf(st) - logf(sb));
                    qa_out[row] = qsel;
                    c_out[row] = lambda * fminf(1.f, expf(d));
                }
            }
        }
    }
}

int retrace_heads(const float* q, const float* tgt, const float* beh, const int64_t* action, float* v_out, float* qa_out,
                  float* c_out, int T, int B, int N, float lambda, hipStream_t st) {
    const long rows = ((long)T + 1) * B, TB = (long)T * B;
    return with_row4(row_cfg(N, aligned(q, 16) && aligned(tgt, 16) && aligned(beh, 16), kRow4Pieces), [&](auto G_, auto V_, auto E_) {
        constexpr int G = G_, V = V_, E = E_;
        const unsigned grid = row_grid(rows, (256 / G) * RowsPerIter<V, E>::value, kUnfoldedGridCap);
        hipLaunchKernelGGL((retrace_heads_fwd_kernel<G, V, E>), dim3(grid), dim3(256), 0, st, q, tgt, beh, action, v_out,
                           qa_out, c_out, rows, TB, (long)B, N, lambda);
        return last_error();
    });
}

// ================================================================================================
// the scan.  HW / HLW: weights / loss_weight given (the null case loads nothing); LOSS: the fused form (loss and delta)
// ================================================================================================
template <bool HW, bool HLW, bool LOSS>
struct RetraceOp {
    static constexpr int NACC = LOSS ? 1 : 0, DIAG_OP = kScanOpRetrace, DIAG_MT = 0, DIAG_MM = (HW ? 1 : 0) | (HLW ? 2 : 0),
                         DIAG_NVF = LOSS ? 0 : 1;
    const float* reward; const float* weights; const float* loss_weight; const float* v; const float* c; const float* qa;
    float* q_out; float* delta; int T, B; float gamma, scale;
    // r, w and the row's own v, c, qa (what row t-1 links to; qa is also finish's), then the step-(t+1) fields
    template <int V> struct Row { Pack<V> r, w, v0, c0, qa0, v1, c1, qa1; };

    template <int V> __device__ void init(long col, bool ok, float (&carry)[V]) const {   // Q_T = v_T, stored here
        const Pack<V> vt = load_pack<V>(v + row_off(T, col, ok, B, V));
#pragma unroll
        for (int k = 0; k < V; ++k) carry[k] = vt.v[k];
        if (ok) store_pack<V>(q_out + (size_t)T * B + col, vt);
    }
    template <int V> __device__ void load(Row<V>& row, int t, long col, bool ok, bool next_in_regs) const {
        const size_t o = row_off(t, col, ok, B, V);
        row.r = load_pack<V>(reward + o);
        if (HW) row.w = load_pack<V>(weights + o);
        row.v0 = load_pack<V>(v + o);
        row.c0 = load_pack<V>(c + o);
        row.qa0 = load_pack<V>(qa + o);
        if (next_in_regs) return;
        // A chunk's last row: step t+1 belongs to another wave (or t = T-1).  v has T+1 rows; c and qa have T, so at t = T-1
        // the row's own address stands in (every address stays inside the arrays) and c_{t+1} := 0.
        const bool inner = t < T - 1;
        const size_t o1 = inner ? o + B : o;
        row.v1 = load_pack<V>(v + o + B);
        const Pack<V> c1 = load_pack<V>(c + o1);
        row.qa1 = load_pack<V>(qa + o1);
#pragma unroll
        for (int k = 0; k < V; ++k) row.c1.v[k] = inner ? c1.v[k] : 0.f;
    }
    template <int V> __device__ void link(Row<V>& row, const Row<V>& nxt) const {
        row.v1 = nxt.v0;
        row.c1 = nxt.c0;
        row.qa1 = nxt.qa0;
    }
    template <int V> __device__ void coeffs(const Row<V>& row, int, float (&a)[V], float (&b)[V]) const {
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const float gw = HW ? gamma * row.w.v[k] : gamma;
            a[k] = gw * row.c1.v[k];
            b[k] = fmaf(gw, fmaf(-row.c1.v[k], row.qa1.v[k], row.v1.v[k]), row.r.v[k]);
        }
    }
    template <int V> __device__ void finish(const Row<V>& row, int t, long col, bool ok, const float (&s)[V],
                                            const float (&)[V], float (&acc)[NACC > 0 ? NACC : 1]) const {
        Pack<V> lw;
        if (LOSS && HLW) lw = load_pack<V>(loss_weight + row_off(t, col, ok, B, V));
        if (!ok) return;
        Pack<V> qo, dl;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            qo.v[k] = s[k];
            if (LOSS) {
                const float d = row.qa0.v[k] - s[k];
                const float wd = HLW ? lw.v[k] * d : d;
                acc[0] = fmaf(wd, d, acc[0]);
                dl.v[k] = wd * scale;
            }
        }
        store_pack<V, true>(q_out + (size_t)t * B + col, qo);
        if (LOSS) store_pack<V, true>(delta + (size_t)t * B + col, dl);
    }
};

// the scan of either form over filled v / qa / c streams; loss == nullptr: the drop-in form (no loss, no delta)
int retrace_scan(const float* reward, const float* weights, const float* loss_weight, const float* v, const float* c,
                 const float* qa, float* q_out, float* delta, float* loss, float* partials, int T, int B, float gamma,
                 float scale, hipStream_t st) {
    const ScanCfg cfg = scan_cfg(T, B, false);   // V = 1, the rule of hpc_rll_vtrace_forward and hpc_rll_upgo_forward
    int rc = HPC_RLL_OK;
    auto run = [&](auto HW_, auto HLW_) {
        constexpr bool HW = decltype(HW_)::value, HLW = decltype(HLW_)::value;
        if (loss) {
            using Op = RetraceOp<HW, HLW, true>;
            const Op op{reward, weights, loss_weight, v, c, qa, q_out, delta, T, B, gamma, scale};
            const float sc = 0.5f * scale;
            rc = scan_and_finalize<Op, false>(op, cfg, T, B, partials, 1, &sc, loss, st);
        } else {
            using Op = RetraceOp<HW, false, false>;
            const Op op{reward, weights, nullptr, v, c, qa, q_out, nullptr, T, B, gamma, 0.f};
            launch_colscan<Op, false>(op, cfg, T, B, nullptr, st);
            rc = last_error();
            if (!rc) scan_note_final(Op::DIAG_OP, 0);
        }
    };
    using Yes = std::true_type;
    using No = std::false_type;
    if (weights) {
        if (loss && loss_weight) run(Yes{}, Yes{});
        else run(Yes{}, No{});
    } else {
        if (loss && loss_weight) run(No{}, Yes{});
        else run(No{}, No{});
    }
    return rc;
}

// ================================================================================================
// backward: every float of grad (n = (T+1)*B*N) written once by the one-hot writer of stream_write.hpp
// ================================================================================================
struct RetraceGrad {
    const int64_t* action; const float* delta; long TB;
    __device__ __forceinline__ float operator()(float u, long r, int c) const {
        const long rr = r < TB ? r : TB - 1;            // rows of t = T: an in-bounds load whose result is unused
        const long a = action[rr];
        const float d = delta[rr];
        return (r < TB && a == (long)c) ? u * d : 0.f;
    }
};

int retrace_backward(const float* g, const int64_t* action, const float* delta, float* grad, int T, int B, int N,
                     hipStream_t st) {
    const long TB = (long)T * B;
    const int rc = launch_onehot_stream(RetraceGrad{action, delta, TB}, g, grad, (size_t)(TB + B) * N, N, st);
    return rc == (int)hipSuccess ? HPC_RLL_OK : rc;
}

}  // namespace
}  // namespace hpc_rll

using namespace hpc_rll;

// ws (floats): delta T*B | qa T*B | c T*B | partial sums, one per workgroup of the scan
extern "C" int64_t hpc_rll_retrace_workspace_floats(int T, int B) {
    if (T < 0 || B < 0) return HPC_RLL_EINVAL;
    return 3 * (int64_t)T * B + 8 * (((int64_t)B + 7) / 8 + 1);
}

extern "C" int hpc_rll_retrace_forward(const float* q_values, const float* v_pred, const float* rewards,
                                       const int64_t* actions, const float* weights, const float* ratio, float* q_retraces,
                                       float* ws, int T, int B, int N, float gamma, float lambda, void* stream) {
    const bool empty = T == 0 || B == 0;
    if (!empty && (!q_values || !v_pred || !rewards || !actions || !ratio || !q_retraces || !ws)) return HPC_RLL_EINVAL;
    if (T < 0 || B < 0 || N <= 0) return HPC_RLL_EINVAL;
    if (!aligned(q_values, 4) || !aligned(v_pred, 4) || !aligned(rewards, 4) || !aligned(actions, 8) || !aligned(weights, 4) ||
        !aligned(ratio, 4) || !aligned(q_retraces, 4) || !aligned(ws, 4))
        return HPC_RLL_EALIGN;
    if (N > kRetraceMaxN) return HPC_RLL_EUNSUPPORTED;
    if (empty) return HPC_RLL_OK;
    hipStream_t st = (hipStream_t)stream;
    const long TB = (long)T * B;
    float *qa = ws, *c = ws + TB;
    hipLaunchKernelGGL(retrace_gather_kernel, dim3((unsigned)((TB + 255) / 256)), dim3(256), 0, st, q_values, ratio, actions,
                       qa, c, TB, N, lambda);
    const int rc = last_error();
    if (rc) return rc;
    return retrace_scan(rewards, weights, nullptr, v_pred, c, qa, q_retraces, nullptr, nullptr, nullptr, T, B, gamma, 0.f, st);
}

extern "C" int hpc_rll_retrace_loss_forward(const float* q_values, const float* target_output,
                                            const float* behaviour_output, const int64_t* action, const float* reward,
                                            const float* weights, const float* loss_weight, float* loss, float* q_retraces,
                                            float* v_pred, float* ws, int T, int B, int N, float gamma, float lambda,
                                            float scale, void* stream) {
    const bool empty = T == 0 || B == 0;
    if (!loss) return HPC_RLL_EINVAL;
    if (!empty && (!q_values || !target_output || !behaviour_output || !action || !reward || !q_retraces || !v_pred || !ws))
        return HPC_RLL_EINVAL;
    if (T < 0 || B < 0 || N <= 0) return HPC_RLL_EINVAL;
    if (!aligned(q_values, 4) || !aligned(target_output, 4) || !aligned(behaviour_output, 4) || !aligned(action, 8) ||
        !aligned(reward, 4) || !aligned(weights, 4) || !aligned(loss_weight, 4) || !aligned(loss, 4) ||
        !aligned(q_retraces, 4) || !aligned(v_pred, 4) || !aligned(ws, 4))
        return HPC_RLL_EALIGN;
    if (N > kRetraceMaxN) return HPC_RLL_EUNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    if (empty) return (int)hipMemsetAsync(loss, 0, sizeof(float), st);
    const size_t TB = (size_t)T * B;
    float *delta = ws, *qa = ws + TB, *c = ws + 2 * TB, *partials = ws + 3 * TB;
    const int rc = retrace_heads(q_values, target_output, behaviour_output, action, v_pred, qa, c, T, B, N, lambda, st);
    if (rc) return rc;
    return retrace_scan(reward, weights, loss_weight, v_pred, c, qa, q_retraces, delta, loss, partials, T, B, gamma, scale, st);
}

extern "C" int hpc_rll_retrace_loss_backward(const float* g_loss, const int64_t* action, const float* ws,
                                             float* grad_q_values, int T, int B, int N, void* stream) {
    const bool empty = T == 0 || B == 0;
    if (!empty && (!action || !ws || !grad_q_values)) return HPC_RLL_EINVAL;
    if (T < 0 || B < 0 || N <= 0) return HPC_RLL_EINVAL;
    if (!aligned(g_loss, 4) || !aligned(action, 8) || !aligned(ws, 4) || !aligned(grad_q_values, 4)) return HPC_RLL_EALIGN;
    if (N > kRetraceMaxN) return HPC_RLL_EUNSUPPORTED;
    if (empty) return HPC_RLL_OK;   // T == 0: the caller zeroes the (1,B,N) gradient of the bootstrap row itself
    return retrace_backward(g_loss, action, ws, grad_q_values, T, B, N, (hipStream_t)stream);
}
