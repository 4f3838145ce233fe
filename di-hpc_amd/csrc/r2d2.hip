// r2d2.hip -- the R2D2 sequence loss on gfx950: the n-step double-Q TD error of every step of a whole unroll, its loss, the
// replay priority and the gradient, in a number of launches that does not depend on T.
//
// No reference counterpart; the semantics restate the loop of DI-engine's r2d2 policy over q_nstep_td_error(_with_rescale).
// q, target_q (T,B,N), action, reward, done (T,B); the valid steps are t = burnin .. T-nstep-1 (L = T - nstep - burnin):
//   a  = action[t,b],  qa = q[t,b,a],   a* = the lowest index of max_n sel[t+n,b,:]  (sel = q if double_q else target_q)
//   v  = target_q[t+n,b,a*]   (h_inverse(v) with value_rescale),   k_t = 1 - done[t,b],   p_0 = 1, p_{j+1} = (p_j gamma) k_{t+j}
//   G  = sum_{j<n} p_j reward[t+j,b] + p_n v   (h_transform(G) with value_rescale),   d = qa - G,   td_error[t-burnin,b] = d^2
//   loss = scale sum w d^2,   priority[b] = eta max_t td_error[.,b] + (1 - eta) mean_t td_error[.,b]
//   grad_q[t,b,n] = g 2 w d scale [n = a] on valid rows, 0 on every other row   (G is a constant)
//
// Four kernels, every array read or written once:
//   * r2d2_heads_kernel on the mapping of rowgroup.hpp over the rows (t,b), t >= burnin: a group of G lanes holds a RowSlice of
//     the q row and of the target_q row.  The maximum of the selecting row by a group all-reduce, the lowest index that
//     holds it by a second one (min over the matching columns), then q[a] and target_q[a*] by selection.  Stores qa[t,b] and
//     v[t,b] (h_inverse already applied).  Every row computes both: rows t < burnin+nstep need no v and rows t >= T-nstep no
//     qa, and what they store is never read.  8 N + 8 bytes read, 8 written per row.
//   * r2d2_window_kernel, one lane per valid (t,b), coalesced over b: the n rewards and masks of the window through
//     nstep_return_masked (nstep.hpp: eight steps' loads in flight), v[t+n], qa[t], the action and the weight; stores td_error
//     and delta = 2 w d scale; the loss leaves through publish_sums (at most kFoldMaxGrid looping workgroups).
//   * r2d2_priority_kernel over td_error: 64 columns per workgroup, its four waves take every fourth step, partial sums and
//     maxima meet in LDS in a fixed order.  No atomics: the same bits on every run.
//   * the backward is the one-hot writer of stream_write.hpp over all T*B*N floats; q is not read.
//
// An action outside [0,N) matches no column: the step is dropped (d = 0, delta = 0), nothing is addressed with it.  NaN in the
// selecting row is not supported (the maximum skips it, a row of NaN alone selects no column and v = 0).
#include <hip/hip_runtime.h>

#include "colscan.hpp"
#include "hostutil.hpp"
#include "hpc_rll_hip.h"
#include "masks.hpp"
#include "nstep.hpp"
#include "rowgroup.hpp"
#include "stream_write.hpp"
#include "value_rescale.hpp"
#include "wave.hpp"

namespace hpc_rll {
namespace {

constexpr int kR2d2MaxN = kRowTableMaxN;   // 64 lanes x 16 floats per lane and input
constexpr float kRescaleEps = 1e-2f;       // as QNStepTDRescale

// ================================================================================================
// the heads: rows [row0, rows) of q, target_q and action, row = t*B + b
// ================================================================================================
template <int G, int VEC, int E>
__global__ __launch_bounds__(256) void r2d2_heads_kernel(const float* __restrict__ q, const float* __restrict__ tq,
                                                         const int64_t* __restrict__ action, float* __restrict__ qa_out,
                                                         float* __restrict__ v_out, long row0, long rows, int N, int double_q,
                                                         int rescale) {
    constexpr int GPB = 256 / G;
    constexpr int R = RowsPerIter<VEC, E>::value;
    const int gl = threadIdx.x % G;
    const int gi = threadIdx.x / G;
    const long stride = (long)gridDim.x * GPB * R;
    for (long bb = row0 + (long)blockIdx.x * GPB * R; bb < rows; bb += stride) {
        RowSlice<G, VEC, E> qs[R], ts[R];
        long a[R];
#pragma unroll
        for (int k = 0; k < R; ++k) {
            long row = bb + (long)k * GPB + gi;
            if (row >= rows) row = rows - 1;               // (re-reads the last row; the stores below are guarded)
            qs[k].load(q + row * (long)N, N, gl);
            ts[k].load(tq + row * (long)N, N, gl);
            a[k] = action[row];                            // (every lane: the same address per group, one request)
        }
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const int ai = action_index(a[k], N);
            // ---- the maximum of the selecting row; padding counts as -inf
            float mx = -INFINITY;
#pragma unroll
            for (int e = 0; e < E; ++e)
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    const int i = e * VEC + j;
                    const int c = (e * G + gl) * VEC + j;
                    const float s = double_q ? qs[k].x[i] : ts[k].x[i];
                    mx = fmaxf(mx, c < N ? s : -INFINITY);
                }
            const float m = group_all<G, MaxOp>(mx);
            // ---- the lowest column that holds it (columns are below 2^24: exact as floats)
            float first = (float)kR2d2MaxN;
#pragma unroll
            for (int e = 0; e < E; ++e)
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    const int i = e * VEC + j;
                    const int c = (e * G + gl) * VEC + j;
                    const float s = double_q ? qs[k].x[i] : ts[k].x[i];
                    first = (c < N && s == m) ? fminf(first, (float)c) : first;
                }
            const int star = (int)group_all<G, MinOp>(first);
            // ---- q[a] and target_q[a*]
            float qsel = 0.f, vsel = 0.f;
#pragma unroll
            for (int e = 0; e < E; ++e)
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    const int i = e * VEC + j;
                    const int c = (e * G + gl) * VEC + j;
                    qsel = (c == ai) ? qs[k].x[i] : qsel;
                    vsel = (c == star) ? ts[k].x[i] : vsel;
                }
            qsel = group_all<G, AddOp>(qsel);              // at most one lane holds a nonzero value
            vsel = group_all<G, AddOp>(vsel);
            const long row = bb + (long)k * GPB + gi;
            if (gl == 0 && row < rows) {
                qa_out[row] = qsel;
                v_out[row] = rescale ? h_inverse(vsel, kRescaleEps) : vsel;
            }
        }
    }
}

// The dispatch records (hpc_rll_r2d2_last_config)
constexpr int kHeadInts = 7, kWindowInts = 5, kPrioInts = 2, kBwdInts = 3;
LaunchRecord<kHeadInts> g_r2d2_heads;
LaunchRecord<kWindowInts> g_r2d2_window;
LaunchRecord<kPrioInts> g_r2d2_prio;
LaunchRecord<kBwdInts> g_r2d2_bwd;

int r2d2_heads(const float* q, const float* tq, const int64_t* action, float* qa, float* v, long row0, long rows, int N,
               int double_q, int rescale, hipStream_t st) {
    return with_row4(row_cfg(N, aligned(q, 16) && aligned(tq, 16), kRow4Pieces), [&](auto G_, auto V_, auto E_) {
        constexpr int G = G_, V = V_, E = E_, R = RowsPerIter<V, E>::value;
        const unsigned grid = row_grid(rows - row0, (256 / G) * R, kUnfoldedGridCap);
        hipLaunchKernelGGL((r2d2_heads_kernel<G, V, E>), dim3(grid), dim3(256), 0, st, q, tq, action, qa, v, row0, rows, N,
                           double_q, rescale);
        const int rc = last_error();
        if (!rc) g_r2d2_heads.note({G, V, E, R, (double_q ? 1 : 0) | (rescale ? 2 : 0), (int)grid});
        return rc;
    });
}

// ================================================================================================
// the window: n = L*B samples, sample i is step burnin + i / B of column i % B, so its (T,B) offset is burnin*B + i
// ================================================================================================
struct R2d2WindowArgs {
    const float* reward; const void* done; const float* weight; const int64_t* action; const float* qa; const float* v;
    float* td; float* delta; long n; size_t first; int B, N, nstep; float gamma, scale; int rescale;
};

// MT: mask element type; HD: done given; WM: weight form (0 none, 1 (B,), 2 (T,B)); NT: threads per workgroup
template <int MT, bool HD, int WM, int NT>
__global__ __launch_bounds__(NT) void r2d2_window_kernel(const R2d2WindowArgs p, float* __restrict__ partials,
                                                         const ScanFold fold) {
    float acc[1] = {0.f};
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < p.n; i += (long)gridDim.x * NT) {
        const size_t o = p.first + (size_t)i;
        const long a = p.action[o];
        const float qa = p.qa[o];
        const float v = p.v[o + (size_t)p.nstep * p.B];
        float w = 1.f;
        if (WM == 2) w = p.weight[o];
        if (WM == 1) w = p.weight[i % p.B];
        float pn;
        const float R = nstep_return_masked<MT, HD>(p.reward, p.done, o, p.B, p.nstep, p.gamma, pn);
        float G = fmaf(pn, v, R);
        if (p.rescale) G = h_transform(G, kRescaleEps);
        const float d = (a >= 0 && a < (long)p.N) ? qa - G : 0.f;   // an action outside: the step is dropped
        const float wd = WM ? w * d : d;
        acc[0] = fmaf(wd, d, acc[0]);
        __builtin_nontemporal_store(d * d, p.td + i);
        __builtin_nontemporal_store((2.f * wd) * p.scale, p.delta + o);
    }
    publish_block_sums<1, NT>(acc, partials, fold);
}

template <int MT, bool HD, int WM>
int r2d2_window_launch(const R2d2WindowArgs& p, float* partials, float* loss, hipStream_t st) {
    // the grid stays within the fold's workgroups, as sample_ops.hip's launches: 1024 threads above 131072 samples, then loops
    const bool wide = (p.n + 255) / 256 > kFoldMaxGrid;
    const long nt = wide ? 1024 : 256;
    long grid = (p.n + nt - 1) / nt;
    if (grid > kFoldMaxGrid) grid = kFoldMaxGrid;
    const ScanFold fold = make_fold(st, 1, &p.scale, loss, grid);
    if (wide) hipLaunchKernelGGL((r2d2_window_kernel<MT, HD, WM, 1024>), dim3((unsigned)grid), dim3(1024), 0, st, p, partials, fold);
    else hipLaunchKernelGGL((r2d2_window_kernel<MT, HD, WM, 256>), dim3((unsigned)grid), dim3(256), 0, st, p, partials, fold);
    int rc = last_error();
    if (rc) return rc;
    if (!fold.out) rc = finalize_sums(partials, (int)grid, 1, &p.scale, loss, st);
    if (!rc) {
        const int flags = (HD ? 1 + MT : 0) | (WM << 2) | (p.rescale ? 16 : 0);
        g_r2d2_window.note({(int)nt, flags, (int)grid, fold.out ? 1 : 2});
    }
    return rc;
}

int r2d2_window(const R2d2WindowArgs& p, int mt, int wm, float* partials, float* loss, hipStream_t st) {
    auto with_w = [&](auto MT_, auto HD_) {
        constexpr int MT = decltype(MT_)::value;
        constexpr bool HD = decltype(HD_)::value;
        if (wm == 2) return r2d2_window_launch<MT, HD, 2>(p, partials, loss, st);
        if (wm == 1) return r2d2_window_launch<MT, HD, 1>(p, partials, loss, st);
        return r2d2_window_launch<MT, HD, 0>(p, partials, loss, st);
    };
    if (!p.done) return with_w(I<0>{}, std::false_type{});
    if (mt == HPC_RLL_MASK_F32) return with_w(I<1>{}, std::true_type{});
    return with_w(I<0>{}, std::true_type{});
}

// ================================================================================================
// the priority: per column the maximum and the mean of td_error (L,B) over L.  A workgroup owns 64 columns; wave w takes the
// steps w, w+4, ..., four loads in flight; the four partial results meet in LDS and are combined in a fixed order.
// Chosen over a reduction inside the window launch: that launch is parallel over (t,b), so a column's L values lie in L / 4
// different workgroups and would have to meet through float atomics (no fixed order) or a serial walk over T.
// ================================================================================================
__global__ __launch_bounds__(256) void r2d2_priority_kernel(const float* __restrict__ td, float* __restrict__ priority, int L,
                                                            int B, float eta) {
    __shared__ float s_sum[4][64], s_max[4][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long col = (long)blockIdx.x * 64 + lane;
    const long cc = col < B ? col : (long)B - 1;           // columns past B load the last one and store nothing
    float sum = 0.f, mx = 0.f;                              // td_error >= 0
    for (int t0 = wv; t0 < L; t0 += 16) {
        float x[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int t = t0 + 4 * k < L ? t0 + 4 * k : L - 1;   // clamped: the load is unconditional
            x[k] = td[(size_t)t * B + cc];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (t0 + 4 * k < L) {
                sum += x[k];
                mx = fmaxf(mx, x[k]);
            }
    }
    s_sum[wv][lane] = sum;
    s_max[wv][lane] = mx;
    __syncthreads();
    if (wv == 0 && col < B) {
        const float tot = (s_sum[0][lane] + s_sum[1][lane]) + (s_sum[2][lane] + s_sum[3][lane]);
        const float top = fmaxf(fmaxf(s_max[0][lane], s_max[1][lane]), fmaxf(s_max[2][lane], s_max[3][lane]));
        priority[col] = fmaf(eta, top, (1.f - eta) * (tot / (float)L));
    }
}

// ================================================================================================
// backward: all T*B*N floats once (stream_write.hpp); rows outside [lo, hi) are zero
// ================================================================================================
struct R2d2Grad {
    const int64_t* action; const float* delta; long lo, hi;
    __device__ __forceinline__ float operator()(float u, long r, int c) const {
        const long a = action[r];                           // every row of the T*B is in bounds; outside [lo, hi) the
        const float d = delta[r];                           // loaded delta is whatever the workspace holds and is not used
        return (r >= lo && r < hi && a == (long)c) ? u * d : 0.f;
    }
};

}  // namespace
}  // namespace hpc_rll

using namespace hpc_rll;

// ws (floats): delta T*B (rows burnin .. T-nstep-1 are written) | qa T*B | v T*B (rows burnin .. T-1 of both are written) |
// partial sums, one per workgroup of the window launch
extern "C" int64_t hpc_rll_r2d2_workspace_floats(int T, int B) {
    if (T < 0 || B < 0) return HPC_RLL_EINVAL;
    return 3 * (int64_t)T * B + 8 * (kFoldMaxGrid + 1);
}

extern "C" int hpc_rll_r2d2_forward(const float* q, const float* target_q, const int64_t* action, const float* reward,
                                    const void* done, int mask_dtype, const float* weight, int weight_mode, float* loss,
                                    float* td_error, float* priority, float* ws, int T, int B, int N, int nstep, int burnin,
                                    float gamma, int value_rescale, int double_q, float priority_eta, float scale,
                                    void* stream) {
    const long L = (long)T - nstep - burnin;
    const bool empty = T == 0 || B == 0 || L <= 0;
    if (!loss) return HPC_RLL_EINVAL;
    if (!empty && (!q || !target_q || !action || !reward || !td_error || !priority || !ws)) return HPC_RLL_EINVAL;
    if (T < 0 || B < 0 || N <= 0 || nstep < 1 || burnin < 0) return HPC_RLL_EINVAL;
    if (mask_dtype != HPC_RLL_MASK_U8 && mask_dtype != HPC_RLL_MASK_F32) return HPC_RLL_EINVAL;
    if (weight_mode < 0 || weight_mode > 2 || (!empty && (weight == nullptr) != (weight_mode == 0))) return HPC_RLL_EINVAL;
    if (!aligned(q, 4) || !aligned(target_q, 4) || !aligned(action, 8) || !aligned(reward, 4) ||
        !aligned(done, mask_dtype == HPC_RLL_MASK_F32 ? 4 : 1) || !aligned(weight, 4) || !aligned(loss, 4) ||
        !aligned(td_error, 4) || !aligned(priority, 4) || !aligned(ws, 4))
        return HPC_RLL_EALIGN;
    if (N > kR2d2MaxN) return HPC_RLL_EUNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    if (empty) {   // no valid step: a zero loss (and zero priorities, when there are columns), nothing launched
        int rc = (int)hipMemsetAsync(loss, 0, sizeof(float), st);
        if (!rc && priority && B > 0) rc = (int)hipMemsetAsync(priority, 0, (size_t)B * sizeof(float), st);
        return rc;
    }
    const size_t TB = (size_t)T * B;
    float *delta = ws, *qa = ws + TB, *v = ws + 2 * TB, *partials = ws + 3 * TB;
    int rc = r2d2_heads(q, target_q, action, qa, v, (long)burnin * B, (long)TB, N, double_q, value_rescale, st);
    if (rc) return rc;
    const R2d2WindowArgs p{reward, done, weight, action, qa, v, td_error, delta, L * B, (size_t)burnin * B, B, N, nstep, gamma,
                           scale, value_rescale};
    rc = r2d2_window(p, mask_dtype, weight_mode, partials, loss, st);
    if (rc) return rc;
    const unsigned grid = (unsigned)(((long)B + 63) / 64);
    hipLaunchKernelGGL(r2d2_priority_kernel, dim3(grid), dim3(256), 0, st, td_error, priority, (int)L, B, priority_eta);
    rc = last_error();
    if (!rc) g_r2d2_prio.note({(int)grid});
    return rc;
}

extern "C" int hpc_rll_r2d2_backward(const float* g_loss, const int64_t* action, const float* ws, float* grad_q, int T, int B,
                                     int N, int nstep, int burnin, void* stream) {
    const bool empty = T == 0 || B == 0;
    if (!empty && (!action || !ws || !grad_q)) return HPC_RLL_EINVAL;
    if (T < 0 || B < 0 || N <= 0 || nstep < 1 || burnin < 0) return HPC_RLL_EINVAL;
    if (!aligned(g_loss, 4) || !aligned(action, 8) || !aligned(ws, 4) || !aligned(grad_q, 4)) return HPC_RLL_EALIGN;
    if (N > kR2d2MaxN) return HPC_RLL_EUNSUPPORTED;
    if (empty) return HPC_RLL_OK;
    const long lo = (long)burnin * B, end = ((long)T - nstep) * B;
    const R2d2Grad value{action, ws, lo, end > lo ? end : lo};   // L <= 0: no valid row, all zeros
    int vec = 0;
    long grid = 0;
    const int rc = launch_onehot_stream(value, g_loss, grad_q, (size_t)T * B * N, N, (hipStream_t)stream, &vec, &grid);
    if (rc != (int)hipSuccess) return rc;
    g_r2d2_bwd.note({vec, (int)grid});
    return HPC_RLL_OK;
}

extern "C" int hpc_rll_r2d2_last_config(int* out) {
    if (!out) return HPC_RLL_EINVAL;
    g_r2d2_heads.read(out);
    g_r2d2_window.read(out + kHeadInts);
    g_r2d2_prio.read(out + kHeadInts + kWindowInts);
    g_r2d2_bwd.read(out + kHeadInts + kWindowInts + kPrioInts);
    return HPC_RLL_OK;
}
static_assert(HPC_RLL_R2D2_CONFIG_INTS == kHeadInts + kWindowInts + kPrioInts + kBwdInts, "the layout documented in hpc_rll_hip.h");
