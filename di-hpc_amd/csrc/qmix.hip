// qmix.hip -- QMIX's monotonic mixing network on gfx950, from the hypernetworks' outputs on: the mix in one launch, the mixed
// one-step TD loss of a learner (online and target mix, target, error and loss sum) in one launch, and one streaming backward.
//
// No reference counterpart; the semantics restate DI-engine's Mixer.forward (ding/model/template/qmix.py) and
// v_1step_td_error on the mixed values.  Per sample (row) with q (A) the agents' chosen-action values, w1 (A,E) row-major,
// b1 (E), w2 (E), b2 (1) the raw hypernetwork outputs:
//   pre_e = b1_e + sum_a q_a |w1[a,e]|      h_e = elu(pre_e) = pre_e > 0 ? pre_e : expm1(pre_e)      q_tot = b2 + sum_e h_e |w2_e|
// and, for the learner, with the same five operands of the target network, k = 1 - done (1 without), w = weight (1 without):
//   y = reward + gamma k target_q_tot (a constant)     d = q_tot - y     td_error = d^2 (unweighted)
//   loss = scale sum_rows w d^2                         delta = 2 scale w d
// Gradients from g = dL/dq_tot (delta times the upstream scalar of the loss, or a per-row upstream gradient of the plain mix):
//   dh_e = g |w2_e|   dpre_e = dh_e (pre_e > 0 ? 1 : exp(pre_e))   grad_b2 = g   grad_w2_e = g h_e sgn(w2_e)   grad_b1_e = dpre_e
//   grad_w1[a,e] = dpre_e q_a sgn(w1[a,e])   grad_q_a = sum_e dpre_e |w1[a,e]|                     sgn(0) = 0, as torch.abs
//
// Mapping (rowgroup.hpp): a row is owned by an aligned group of G lanes, 256 / G rows per workgroup and iteration (R = 1).
// Lane gl owns PL pieces of VEC consecutive hidden units, piece e at unit (e*G + gl)*VEC, and keeps pre_e of its units in
// registers while it walks a = 0..A-1: row a of w1 is a contiguous span of E floats read across the group's lanes, kUnroll
// agents' loads are issued before the first is used, and q_a is loaded by every lane of the group from one address (one request
// per group, its address known from the start: no load depends on another).  The accumulation over a needs no cross-lane
// traffic; the sum over e is one butterfly (in fp64, group_all_f64), grad_q_a one group_all butterfly per agent.  No LDS and
// no barrier in the row work; every load is unconditional and in bounds (padding lanes re-read unit 0, an unrolled agent past
// A re-reads agent A - 1 with q = 0, idle groups the last row) and every sum selects on e < E.
//
// The backward recomputes pre_e from the inputs (nothing of size E or A*E is saved by a forward) and, when grad_w1 or grad_q
// is wanted, reads w1 a SECOND time: dpre_e needs the finished pre_e.  The first read then uses plain loads so that the second
// may hit in the cache; what is read last is read nontemporally.  Holding the slice in registers instead (A*PL*VEC floats per
// lane, a compile-time bound on A) was not built; DESIGN.md 4.2.10 has the bytes per row both ways.
//
// Algorithmic HBM bytes per row, n = A*E:  mix forward 4 (n + A + 2E + 1) read, 4 written;  TD forward twice the read,
// + 4 reward (+ 4 weight, + 1 or 4 done), 16 written (td_error, q_tot, target_q_tot, delta);  backward with all five gradients
// 4 (n + A + 2E + 2) read + 4 n read again (from the cache where it holds), 4 (n + A + 2E + 1) written.
#include <hip/hip_runtime.h>

#include "colscan.hpp"
#include "hostutil.hpp"
#include "hpc_rll_hip.h"
#include "rowgroup.hpp"
#include "wave.hpp"

namespace hpc_rll {
namespace {

constexpr int kQmixMaxA = 64, kQmixMaxE = 256;
// Workgroups of the two kernels that end in no sums; above it they loop.  (Long-lived workgroups: a row is up to 64 KiB.)
constexpr long kQmixGridCap = 4096;

// agents whose loads are issued together: U * PL * VEC floats of w1 per lane in flight
template <int PL, int VEC> struct QmixUnroll { static constexpr int value = (PL * VEC <= 4) ? 8 : ((PL * VEC <= 8) ? 4 : 2); };

// the five operands of one network
struct QmixSide { const float* q; const float* w1; const float* b1; const float* w2; const float* b2; };

// a lane's piece of a row; NT: the data is not read again
template <int VEC, bool NT> __device__ __forceinline__ void load_piece(const float* __restrict__ src, float* dst) {
    if constexpr (VEC == 4) {
        const vfloat4* p = reinterpret_cast<const vfloat4*>(src);
        const vfloat4 t = NT ? __builtin_nontemporal_load(p) : *p;
        dst[0] = t.x; dst[1] = t.y; dst[2] = t.z; dst[3] = t.w;
    } else {
        dst[0] = NT ? __builtin_nontemporal_load(src) : *src;
    }
}

// the units of a lane: col[e] the first unit of piece e (0 for a padding piece, which `in` excludes from every sum and store)
template <int G, int VEC, int PL> struct QmixCols {
    int col[PL];
    bool in[PL];
    __device__ __forceinline__ QmixCols(int E, int gl) {
#pragma unroll
        for (int e = 0; e < PL; ++e) {
            const int c = (e * G + gl) * VEC;
            in[e] = c < E;
            col[e] = in[e] ? c : 0;
        }
    }
};

// pre_e = b1_e + sum_a q_a |w1[a,e]| of the lane's units, agents in ascending order
template <int G, int VEC, int PL, bool NT>
__device__ __forceinline__ void qmix_pre(const QmixSide& s, long row, int A, int E, const QmixCols<G, VEC, PL>& cols,
                                         float (&pre)[PL * VEC]) {
    constexpr int U = QmixUnroll<PL, VEC>::value;
    const float* __restrict__ w1 = s.w1 + row * ((long)A * E);
    const float* __restrict__ q = s.q + row * (long)A;
#pragma unroll
    for (int e = 0; e < PL; ++e) load_piece<VEC, NT>(s.b1 + row * (long)E + cols.col[e], pre + e * VEC);
    for (int a0 = 0; a0 < A; a0 += U) {
        float w[U][PL * VEC], qa[U];
#pragma unroll
        for (int j = 0; j < U; ++j) {
            const int a = (a0 + j < A) ? a0 + j : A - 1;
            qa[j] = q[a];
#pragma unroll
            for (int e = 0; e < PL; ++e) load_piece<VEC, NT>(w1 + a * E + cols.col[e], w[j] + e * VEC);
        }
#pragma unroll
        for (int j = 0; j < U; ++j) {
            const float qq = (a0 + j < A) ? qa[j] : 0.f;
#pragma unroll
            for (int i = 0; i < PL * VEC; ++i) pre[i] = fmaf(qq, fabsf(w[j][i]), pre[i]);
        }
    }
}

// The sum over the group is in fp64 (group_all_f64 of rowgroup.hpp).  q_tot is a sum of up to 256 terms of both signs and the TD error squares a DIFFERENCE of two
// such sums: carried in fp32, the rounding of the sums alone put td_error past the project's bar wherever q_tot and its target
// nearly cancel (measured: 1.4e-5 at A = 3, E = 100).  The stream over w1 stays fp32; this is E fp64 operations per row.
// q_tot of one row in every lane of its group, before it is rounded to fp32
template <int G, int VEC, int PL>
__device__ __forceinline__ double qmix_row(const QmixSide& s, long row, int A, int E, const QmixCols<G, VEC, PL>& cols) {
    float pre[PL * VEC], w2[PL * VEC];
#pragma unroll
    for (int e = 0; e < PL; ++e) load_piece<VEC, true>(s.w2 + row * (long)E + cols.col[e], w2 + e * VEC);
    const float b2 = s.b2[row];
    qmix_pre<G, VEC, PL, true>(s, row, A, E, cols, pre);
    double part = 0.0;
#pragma unroll
    for (int e = 0; e < PL; ++e)
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const float x = pre[e * VEC + j];
            const float h = x > 0.f ? x : expm1f(x);
            part = cols.in[e] ? fma((double)h, (double)fabsf(w2[e * VEC + j]), part) : part;
        }
    return (double)b2 + group_all_f64<G>(part);
}

template <int G, int VEC, int PL>
__global__ __launch_bounds__(256) void qmix_mix_fwd_kernel(const QmixSide s, float* __restrict__ q_tot, long rows, int A,
                                                           int E) {
    constexpr int GPB = 256 / G;
    const int gl = threadIdx.x % G;
    const int gi = threadIdx.x / G;
    const QmixCols<G, VEC, PL> cols(E, gl);
    const long stride = (long)gridDim.x * GPB;
    for (long bb = (long)blockIdx.x * GPB; bb < rows; bb += stride) {
        const long row = bb + gi;
        const bool live = row < rows;
        const float v = (float)qmix_row<G, VEC, PL>(s, live ? row : rows - 1, A, E, cols);   // (re-reads the last row; the store is guarded)
        if (live && gl == 0) __builtin_nontemporal_store(v, q_tot + row);
    }
}

struct QmixTdArgs {
    QmixSide on, tg;
    const float* reward; const void* done; int done_f32; const float* weight;
    float* td_error; float* q_tot; float* target_q_tot; float* delta; long rows; int A, E; float gamma, scale;
};

template <int G, int VEC, int PL>
__global__ __launch_bounds__(256) void qmix_td_fwd_kernel(const QmixTdArgs p, float* __restrict__ partials, const ScanFold fold) {
    constexpr int GPB = 256 / G;
    const int gl = threadIdx.x % G;
    const int gi = threadIdx.x / G;
    const QmixCols<G, VEC, PL> cols(p.E, gl);
    const long stride = (long)gridDim.x * GPB;
    float acc[1] = {0.f};
    for (long bb = (long)blockIdx.x * GPB; bb < p.rows; bb += stride) {
        const long row = bb + gi;
        const bool live = row < p.rows;
        const long r = live ? row : p.rows - 1;
        const float rew = p.reward[r];
        const float wt = p.weight ? p.weight[r] : 1.f;
        float keep = 1.f;
        if (p.done) {
            if (p.done_f32) keep = 1.f - static_cast<const float*>(p.done)[r];
            else keep = static_cast<const uint8_t*>(p.done)[r] ? 0.f : 1.f;
        }
        const double tq = qmix_row<G, VEC, PL>(p.tg, r, p.A, p.E, cols);
        const double qt = qmix_row<G, VEC, PL>(p.on, r, p.A, p.E, cols);
        const double y = fma((double)p.gamma * (double)keep, tq, (double)rew);
        const double d = qt - y;                                   // (the unrounded sums: see group_all_f64)
        const double wd = (double)wt * d;
        if (live && gl == 0) {
            acc[0] += (float)(wd * d);
            p.td_error[row] = (float)(d * d);
            p.q_tot[row] = (float)qt;
            p.target_q_tot[row] = (float)tq;
            p.delta[row] = (float)((2.0 * wd) * (double)p.scale);
        }
    }
    publish_block_sums<1, 256>(acc, partials, fold);   // (the only LDS and barriers of the kernel)
}

// ================================================================================================
// backward: every float of each wanted output written once; no atomics
// ================================================================================================
struct QmixBwdArgs {
    QmixSide s;
    const float* g_rows; const float* delta; const float* g_loss;
    float* grad_q; float* grad_w1; float* grad_b1; float* grad_w2; float* grad_b2; long rows; int A, E;
};

template <int G, int VEC, int PL>
__global__ __launch_bounds__(256) void qmix_bwd_kernel(const QmixBwdArgs p) {
    constexpr int GPB = 256 / G;
    constexpr int U = QmixUnroll<PL, VEC>::value;
    constexpr int GS = G < U ? G : U;   // agents whose grad_q one store instruction writes
    const int gl = threadIdx.x % G;
    const int gi = threadIdx.x / G;
    const int A = p.A, E = p.E;
    const QmixCols<G, VEC, PL> cols(E, gl);
    const bool second = p.grad_w1 != nullptr || p.grad_q != nullptr;   // w1 is read again
    const float gs = (!p.g_rows && p.g_loss) ? p.g_loss[0] : 1.f;
    const long stride = (long)gridDim.x * GPB;
    for (long bb = (long)blockIdx.x * GPB; bb < p.rows; bb += stride) {
        const long row = bb + gi;
        const bool live = row < p.rows;
        const long r = live ? row : p.rows - 1;   // (re-reads the last row; the stores below are guarded)
        const float g = p.g_rows ? p.g_rows[r] : p.delta[r] * gs;
        float pre[PL * VEC], w2[PL * VEC];
#pragma unroll
        for (int e = 0; e < PL; ++e) load_piece<VEC, true>(p.s.w2 + r * (long)E + cols.col[e], w2 + e * VEC);
        if (second) qmix_pre<G, VEC, PL, false>(p.s, r, A, E, cols, pre);
        else qmix_pre<G, VEC, PL, true>(p.s, r, A, E, cols, pre);
        // ---- dpre (kept in pre), grad_b1, grad_w2, grad_b2
#pragma unroll
        for (int e = 0; e < PL; ++e) {
            float o1[VEC], o2[VEC];
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                const int i = e * VEC + j;
                const float x = pre[i], v = w2[i];
                const bool pos = x > 0.f;
                const float gh = g * (pos ? x : expm1f(x));
                o2[j] = v > 0.f ? gh : (v < 0.f ? -gh : 0.f);
                pre[i] = (g * fabsf(v)) * (pos ? 1.f : expf(x));
                o1[j] = pre[i];
            }
            if (live && cols.in[e]) {
                if (p.grad_b1) store_piece<VEC>(p.grad_b1 + row * (long)E + cols.col[e], o1);
                if (p.grad_w2) store_piece<VEC>(p.grad_w2 + row * (long)E + cols.col[e], o2);
            }
        }
        if (p.grad_b2 && live && gl == 0) __builtin_nontemporal_store(g, p.grad_b2 + row);
        if (!second) continue;
        // ---- grad_w1 and grad_q: w1 a second time
        const float* __restrict__ w1 = p.s.w1 + r * ((long)A * E);
        const float* __restrict__ q = p.s.q + r * (long)A;
        for (int a0 = 0; a0 < A; a0 += U) {
            float w[U][PL * VEC], qa[U], sq[U];
#pragma unroll
            for (int j = 0; j < U; ++j) {
                const int a = (a0 + j < A) ? a0 + j : A - 1;
                qa[j] = q[a];
#pragma unroll
                for (int e = 0; e < PL; ++e) load_piece<VEC, true>(w1 + a * E + cols.col[e], w[j] + e * VEC);
            }
#pragma unroll
            for (int j = 0; j < U; ++j) {
                const bool aok = live && a0 + j < A;
                float part = 0.f;
#pragma unroll
                for (int e = 0; e < PL; ++e) {
                    float o[VEC];
#pragma unroll
                    for (int k = 0; k < VEC; ++k) {
                        const int i = e * VEC + k;
                        const float x = w[j][i], v = pre[i] * qa[j];
                        o[k] = x > 0.f ? v : (x < 0.f ? -v : 0.f);
                        part += cols.in[e] ? pre[i] * fabsf(x) : 0.f;
                    }
                    if (p.grad_w1 && aok && cols.in[e])
                        store_piece<VEC>(p.grad_w1 + row * ((long)A * E) + (a0 + j) * E + cols.col[e], o);
                }
                sq[j] = p.grad_q ? group_all<G, AddOp>(part) : 0.f;   // (uniform: every lane of the group takes it)
            }
            if (p.grad_q) {
                // lane t of the group stores agent j0 + t: GS consecutive floats per store instruction
#pragma unroll
                for (int j0 = 0; j0 < U; j0 += GS) {
                    float mine = sq[j0];
#pragma unroll
                    for (int t = 1; t < GS; ++t) mine = (gl == t) ? sq[j0 + t] : mine;
                    const int a = a0 + j0 + gl;
                    if (live && gl < GS && a < A) __builtin_nontemporal_store(mine, p.grad_q + row * (long)A + a);
                }
            }
        }
    }
}

// The (G, VEC, PL) of row_cfg(E, ., kRow4Pieces) for 1 <= E <= kQmixMaxE: the kernels this file instantiates
#define HPC_RLL_QMIX_TABLE(CASE)                                                                          \
    CASE(1, 4, 1) CASE(2, 4, 1) CASE(4, 4, 1) CASE(8, 4, 1) CASE(16, 4, 1) CASE(16, 4, 2) CASE(16, 4, 4) \
    CASE(1, 1, 1) CASE(2, 1, 1) CASE(4, 1, 1) CASE(8, 1, 1) CASE(16, 1, 1) CASE(16, 1, 2) CASE(16, 1, 4) \
    CASE(64, 1, 2) CASE(64, 1, 4)

constexpr bool qmix_table_complete() {
    for (int n = 1; n <= kQmixMaxE; ++n)
        for (int v4 = 0; v4 < 2; ++v4) {
            const RowCfg c = row_cfg(n, v4 != 0, kRow4Pieces);
            if (!(false HPC_RLL_QMIX_TABLE(HPC_RLL_ROW_MATCH))) return false;
        }
    return true;
}
static_assert(qmix_table_complete(), "HPC_RLL_QMIX_TABLE misses a configuration row_cfg(E, ., kRow4Pieces) returns for E <= kQmixMaxE");

template <class F> int with_qmix(const RowCfg& cfg, F&& f) {
#define HPC_RLL_QMIX_CASE(G_, V_, E_) \
    if (cfg.g == G_ && cfg.vec == V_ && cfg.e == E_) return f(RowInt<G_>{}, RowInt<V_>{}, RowInt<E_>{});
    HPC_RLL_QMIX_TABLE(HPC_RLL_QMIX_CASE)
#undef HPC_RLL_QMIX_CASE
    return HPC_RLL_EUNSUPPORTED;
}

// 16-byte loads of the E-float rows of one network: q and b2 are read a float at a time and restrict nothing
bool side_v4(const QmixSide& s) { return aligned(s.w1, 16) && aligned(s.b1, 16) && aligned(s.w2, 16); }

// The dispatch records of the forwards and the backward (hpc_rll_qmix_last_config):
// {launches so far, G, VEC, PL, R, flags, grid}
constexpr int kLaunchInts = 7;
LaunchRecord<kLaunchInts> g_qmix_fwd, g_qmix_bwd;

int qmix_mix_forward(const QmixSide& s, float* q_tot, long rows, int A, int E, hipStream_t st) {
    return with_qmix(row_cfg(E, side_v4(s), kRow4Pieces), [&](auto G_, auto V_, auto P_) {
        constexpr int G = G_, V = V_, PL = P_;
        const unsigned grid = row_grid(rows, 256 / G, kQmixGridCap);
        hipLaunchKernelGGL((qmix_mix_fwd_kernel<G, V, PL>), dim3(grid), dim3(256), 0, st, s, q_tot, rows, A, E);
        const int rc = last_error();
        if (!rc) g_qmix_fwd.note({G, V, PL, 1, 0, (int)grid});
        return rc;
    });
}

int qmix_td_forward(const QmixTdArgs& p, float* partials, float* loss, hipStream_t st) {
    const float sc[1] = {p.scale};
    const int flags = (p.weight ? 1 : 0) | (p.done ? (p.done_f32 ? 4 : 2) : 0) | 8;
    return with_qmix(row_cfg(p.E, side_v4(p.on) && side_v4(p.tg), kRow4Pieces), [&](auto G_, auto V_, auto P_) {
        constexpr int G = G_, V = V_, PL = P_;
        long grid = 0;
        const int rc = launch_rows_folded(p.rows, 256 / G, 1, sc, loss, partials, st, &grid,
                                          [&](unsigned blocks, const ScanFold& fold) {
            hipLaunchKernelGGL((qmix_td_fwd_kernel<G, V, PL>), dim3(blocks), dim3(256), 0, st, p, partials, fold);
        });
        if (grid) g_qmix_fwd.note({G, V, PL, 1, flags, (int)grid});
        return rc;
    });
}

int qmix_backward(const QmixBwdArgs& p, hipStream_t st) {
    const bool v4 = side_v4(p.s) && aligned(p.grad_w1, 16) && aligned(p.grad_b1, 16) && aligned(p.grad_w2, 16);
    const int flags = (p.grad_q ? 1 : 0) | (p.grad_w1 ? 2 : 0) | (p.grad_b1 ? 4 : 0) | (p.grad_w2 ? 8 : 0) |
                      (p.grad_b2 ? 16 : 0) | (p.g_rows ? 32 : 0);
    return with_qmix(row_cfg(p.E, v4, kRow4Pieces), [&](auto G_, auto V_, auto P_) {
        constexpr int G = G_, V = V_, PL = P_;
        const unsigned grid = row_grid(p.rows, 256 / G, kQmixGridCap);
        hipLaunchKernelGGL((qmix_bwd_kernel<G, V, PL>), dim3(grid), dim3(256), 0, st, p);
        const int rc = last_error();
        if (!rc) g_qmix_bwd.note({G, V, PL, 1, flags, (int)grid});
        return rc;
    });
}

// floats of the partial-sum region: one sum per workgroup of at most kFoldMaxGrid
constexpr int64_t kQmixPartials = kFoldMaxGrid + 1;

bool side_null(const float* q, const float* w1, const float* b1, const float* w2, const float* b2) {
    return !q || !w1 || !b1 || !w2 || !b2;
}
bool side_aligned4(const float* q, const float* w1, const float* b1, const float* w2, const float* b2) {
    return aligned(q, 4) && aligned(w1, 4) && aligned(b1, 4) && aligned(w2, 4) && aligned(b2, 4);
}

}  // namespace
}  // namespace hpc_rll

using namespace hpc_rll;

// ws (floats): delta (rows) | the partial sums
extern "C" int64_t hpc_rll_qmix_workspace_floats(int64_t rows) {
    if (rows < 0 || rows > INT64_MAX - kQmixPartials) return HPC_RLL_EINVAL;
    return rows + kQmixPartials;
}

extern "C" int hpc_rll_qmix_mix_forward(const float* agent_q, const float* w1, const float* b1, const float* w2,
                                        const float* b2, float* q_tot, int64_t rows, int A, int E, void* stream) {
    const bool empty = rows == 0;
    if (!empty && (side_null(agent_q, w1, b1, w2, b2) || !q_tot)) return HPC_RLL_EINVAL;
    if (rows < 0 || A <= 0 || E <= 0) return HPC_RLL_EINVAL;
    if (!side_aligned4(agent_q, w1, b1, w2, b2) || !aligned(q_tot, 4)) return HPC_RLL_EALIGN;
    if (A > kQmixMaxA || E > kQmixMaxE) return HPC_RLL_EUNSUPPORTED;
    if (empty) return HPC_RLL_OK;
    return qmix_mix_forward(QmixSide{agent_q, w1, b1, w2, b2}, q_tot, (long)rows, A, E, (hipStream_t)stream);
}

extern "C" int hpc_rll_qmix_td_forward(const float* agent_q, const float* w1, const float* b1, const float* w2,
                                       const float* b2, const float* target_agent_q, const float* target_w1,
                                       const float* target_b1, const float* target_w2, const float* target_b2,
                                       const float* reward, const void* done, int mask_dtype, const float* weight,
                                       float* loss, float* td_error, float* q_tot, float* target_q_tot, float* ws,
                                       int64_t rows, int A, int E, float gamma, float scale, void* stream) {
    const bool empty = rows == 0;
    if (!loss) return HPC_RLL_EINVAL;
    if (!empty && (side_null(agent_q, w1, b1, w2, b2) ||
                   side_null(target_agent_q, target_w1, target_b1, target_w2, target_b2) || !reward || !td_error ||
                   !q_tot || !target_q_tot || !ws))
        return HPC_RLL_EINVAL;
    if (rows < 0 || A <= 0 || E <= 0) return HPC_RLL_EINVAL;
    if (mask_dtype != HPC_RLL_MASK_U8 && mask_dtype != HPC_RLL_MASK_F32) return HPC_RLL_EINVAL;
    if (!side_aligned4(agent_q, w1, b1, w2, b2) ||
        !side_aligned4(target_agent_q, target_w1, target_b1, target_w2, target_b2) || !aligned(reward, 4) ||
        !aligned(done, mask_dtype == HPC_RLL_MASK_F32 ? 4 : 1) || !aligned(weight, 4) || !aligned(loss, 4) ||
        !aligned(td_error, 4) || !aligned(q_tot, 4) || !aligned(target_q_tot, 4) || !aligned(ws, 4))
        return HPC_RLL_EALIGN;
    if (A > kQmixMaxA || E > kQmixMaxE) return HPC_RLL_EUNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    if (empty) return (int)hipMemsetAsync(loss, 0, sizeof(float), st);
    const QmixTdArgs p{{agent_q, w1, b1, w2, b2}, {target_agent_q, target_w1, target_b1, target_w2, target_b2},
                       reward, done, mask_dtype == HPC_RLL_MASK_F32 ? 1 : 0, weight, td_error, q_tot, target_q_tot,
                       ws, (long)rows, A, E, gamma, scale};
    return qmix_td_forward(p, ws + rows, loss, st);
}

extern "C" int hpc_rll_qmix_backward(const float* g_loss, const float* g_rows, const float* ws, const float* agent_q,
                                     const float* w1, const float* b1, const float* w2, const float* b2, float* grad_q,
                                     float* grad_w1, float* grad_b1, float* grad_w2, float* grad_b2, int64_t rows, int A,
                                     int E, void* stream) {
    const bool empty = rows == 0 || (!grad_q && !grad_w1 && !grad_b1 && !grad_w2 && !grad_b2);
    if (!empty && (side_null(agent_q, w1, b1, w2, b2) || (!g_rows && !ws))) return HPC_RLL_EINVAL;
    if (rows < 0 || A <= 0 || E <= 0) return HPC_RLL_EINVAL;
    if (!aligned(g_loss, 4) || !aligned(g_rows, 4) || !aligned(ws, 4) || !side_aligned4(agent_q, w1, b1, w2, b2) ||
        !side_aligned4(grad_q, grad_w1, grad_b1, grad_w2, grad_b2))
        return HPC_RLL_EALIGN;
    if (A > kQmixMaxA || E > kQmixMaxE) return HPC_RLL_EUNSUPPORTED;
    if (empty) return HPC_RLL_OK;
    const QmixBwdArgs p{{agent_q, w1, b1, w2, b2}, g_rows, ws, g_loss, grad_q, grad_w1, grad_b1, grad_w2, grad_b2,
                        (long)rows, A, E};
    return qmix_backward(p, (hipStream_t)stream);
}

extern "C" int hpc_rll_qmix_last_config(int* out) {
    if (!out) return HPC_RLL_EINVAL;
    g_qmix_fwd.read(out);
    g_qmix_bwd.read(out + kLaunchInts);
    return HPC_RLL_OK;
}
static_assert(HPC_RLL_QMIX_CONFIG_INTS == 2 * 7, "the layout documented in hpc_rll_hip.h");
