// lm_kl.hip -- the exact divergence over the whole vocabulary between two rows of logits on gfx950: forward KL, reverse KL
// and the generalized Jensen-Shannon divergence of on-policy distillation (GKD), with the streaming gradient towards the
// first ("student") row.  No reference counterpart; hpc_rll_hip.h has the formulas.
//
// With a = x / T, b = y / T (clamped as in the other heads: -inf and NaN become -FLT_MAX), p = softmax(a), q = softmax(b):
//   forward  KL(q||p) = sum q (b - a) - ly + lx        reverse  KL(p||q) = sum p (a - b) - lx + ly
//   jsd      beta KL(q||m) + (1 - beta) KL(p||m),  m = beta q + (1 - beta) p
//
// Kernels:
//   * lm_kl_kernel<Elem, WIDE, NT, MODE>: the row mapping of the head (lm_head.hpp: a wave per row up to kWaveRowMaxV, four
//     rows per workgroup; a workgroup per row above; the looping grid).  A lane issues kInFlight 16-byte loads of EACH row
//     before it uses the first; both rows are indexed identically, so WIDE needs both bases and the pitch on 16 bytes and
//     everything else takes one element per access (the two rows need not share an offset: no peeling).  Per lane the plain
//     online statistic (m, s) of either row and ONE cross moment, weighted by the row the mode weights:
//         forward  u = sum e^(b - my) (b - a)        reverse  u = sum e^(a - mx) (a - b)
//     rescaled by the bare e^(m_old - m_new), once per batch of loaded vectors.  An element whose exponential is 0 is selected
//     away, so an entry that is -inf in both rows adds exactly nothing and inf - inf is never formed.  Lanes merge by a
//     butterfly, waves through LDS words double-buffered by row parity (one barrier per row and pass).
//     jsd has no cross moment: the mixture needs lx and ly first, so the same lanes walk the same two rows a SECOND time
//     right after the first (plain loads the first time, so that the lines may stay cached) and sum KL(q||m) and KL(p||m)
//     from  d = log p - log q = (a - b) - (lx - ly):  log q - log m = -log(beta + (1 - beta) e^d)  for d <= 0, and the
//     mirrored form for d > 0, which never subtracts two logarithms of size ln V.
//     Saved per row: the value, lx, ly and for jsd KL(p||m).  A dropped row (weight == 0) is not read: its outputs are 0.
//   * lm_kl_grad_kernel<Elem, WIDE, NT, MODE>: dx = c (p - q)                       forward
//                                                   c p ((a - b) - (lx - ly) - KL)   reverse
//                                                   c (1 - beta) p (log p - log m - KL(p||m))   jsd
//     with c = g[row] / T, through stream_row2 (lm_head.hpp); a row with c == 0 or weight == 0 is zero-filled without reading.
// No atomics; every sum has a fixed order, so two runs give the same bits.
#include <hip/hip_runtime.h>

#include "hostutil.hpp"
#include "hpc_rll_hip.h"
#include "lm_head.hpp"
#include "wave.hpp"

namespace hpc_rll {
namespace {

constexpr int kFwd = HPC_RLL_KL_FORWARD, kRev = HPC_RLL_KL_REVERSE, kJsd = HPC_RLL_KL_JSD;

// The dispatch records (hpc_rll_lm_kl_last_config):
// [element type, bytes per access, threads per row, rows per workgroup, workgroups, mode]
constexpr int kKlInts = 7;
LaunchRecord<kKlInts> g_kl_head;
LaunchRecord<kKlInts> g_kl_grad;

// ---- the statistic of a lane over the pair of rows; u is the cross moment of the mode (unused by jsd)
struct PairStat { float mx, sx, my, sy, u; };

// `a` moved to the maxima mx >= a.mx, my >= a.my: the cross moment takes the bare factor of the row that weights it
template <int MODE> __device__ __forceinline__ PairStat pair_shift(const PairStat& a, float mx, float my) {
    const float ex = ex2((a.mx - mx) * kLog2eG), ey = ex2((a.my - my) * kLog2eG);
    PairStat r{mx, a.sx * ex, my, a.sy * ey, 0.f};
    if constexpr (MODE != kJsd) {
        const float e = MODE == kFwd ? ey : ex;
        r.u = e == 0.f ? 0.f : a.u * e;
    }
    return r;
}
template <int MODE> __device__ __forceinline__ PairStat pair_merge(const PairStat& a, const PairStat& b) {
    const float mx = fmaxf(a.mx, b.mx), my = fmaxf(a.my, b.my);
    const PairStat sa = pair_shift<MODE>(a, mx, my), sb = pair_shift<MODE>(b, mx, my);
    return PairStat{mx, sa.sx + sb.sx, my, sa.sy + sb.sy, sa.u + sb.u};
}
template <int MODE> __device__ __forceinline__ PairStat pair_wave(PairStat a) {   // all 64 lanes end with the wave's
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) {
        PairStat o{__shfl_xor(a.mx, k, 64), __shfl_xor(a.sx, k, 64), __shfl_xor(a.my, k, 64), __shfl_xor(a.sy, k, 64), 0.f};
        if constexpr (MODE != kJsd) o.u = __shfl_xor(a.u, k, 64);
        a = pair_merge<MODE>(a, o);
    }
    return a;
}

// One batch of N element pairs: a single rescale of the running sums of either row, then the elements in order.
template <int MODE, int N>
__device__ __forceinline__ void pair_update(PairStat& a, const float (&xa)[N], const float (&yb)[N]) {
    float bx = -kFltMaxG, by = -kFltMaxG;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        bx = fmaxf(bx, xa[i]);
        by = fmaxf(by, yb[i]);
    }
    PairStat n = pair_shift<MODE>(a, fmaxf(a.mx, bx), fmaxf(a.my, by));
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const float e = ex2((xa[i] - n.mx) * kLog2eG), f = ex2((yb[i] - n.my) * kLog2eG);
        n.sx += e;
        n.sy += f;
        // a zero exponential selects the difference away: 0 * 0, exactly nothing
        if constexpr (MODE == kFwd) n.u = fmaf(f, f == 0.f ? 0.f : yb[i] - xa[i], n.u);
        if constexpr (MODE == kRev) n.u = fmaf(e, e == 0.f ? 0.f : xa[i] - yb[i], n.u);
    }
    a = n;
}

// log p - log m (lpm) and log q - log m (lqm) of the mixture m = beta q + (1 - beta) p from d = log p - log q.  d = -inf
// (p = 0) leaves lqm = -ln beta and lpm = -inf, d = +inf the mirror image; the caller selects a zero probability away.
__device__ __forceinline__ void jsd_logs(float d, float beta, float& lpm, float& lqm) {
    const float e = ex2(-fabsf(d) * kLog2eG);
    const bool q_big = d <= 0.f;
    const float t = q_big ? fmaf(1.f - beta, e, beta) : fmaf(beta, e, 1.f - beta);   // m over the larger of p and q
    const float lt = __builtin_amdgcn_logf(t) * kLn2G;                               // t in [min(beta, 1 - beta), 1]
    lpm = q_big ? d - lt : -lt;
    lqm = q_big ? -lt : -d - lt;
}

// The walk of lane `tid` of the NT that share the rows p[0, V) and q[0, V): f(xa, yb) per batch of scaled, clamped elements;
// positions past the end hold -FLT_MAX in both.  CACHED: plain loads (the rows are read again), else nontemporal ones.
template <class Elem, bool WIDE, int NT, bool CACHED, class F>
__device__ __forceinline__ void walk_pair(const Elem* __restrict__ p, const Elem* __restrict__ q, int V, int tid, float inv_t,
                                          F&& f) {
    using IO = ElemIO<Elem>;
    if constexpr (WIDE) {
        constexpr int P = IO::P;
        const int nvec = V / P;
        const vuint4* __restrict__ pv = reinterpret_cast<const vuint4*>(p);
        const vuint4* __restrict__ qv = reinterpret_cast<const vuint4*>(q);
        for (int v = tid; v < nvec; v += kInFlight * NT) {
            const bool full = v + (kInFlight - 1) * NT < nvec;   // only a lane's last batch can be partial
            vuint4 rp[kInFlight], rq[kInFlight];
            const vuint4 z = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int k = 0; k < kInFlight; ++k) {
                rp[k] = z;
                if (full || v + k * NT < nvec) rp[k] = ld<!CACHED>(pv + v + k * NT);
            }
#pragma unroll
            for (int k = 0; k < kInFlight; ++k) {
                rq[k] = z;
                if (full || v + k * NT < nvec) rq[k] = ld<!CACHED>(qv + v + k * NT);
            }
            float xa[kInFlight * P], yb[kInFlight * P];
#pragma unroll
            for (int k = 0; k < kInFlight; ++k) {
                IO::unpack(rp[k], xa + k * P);
                IO::unpack(rq[k], yb + k * P);
                const bool ok = full || v + k * NT < nvec;
#pragma unroll
                for (int j = 0; j < P; ++j) {
                    xa[k * P + j] = ok ? clampf(xa[k * P + j] * inv_t) : -kFltMaxG;
                    yb[k * P + j] = ok ? clampf(yb[k * P + j] * inv_t) : -kFltMaxG;
                }
            }
            f(xa, yb);
        }
    } else {
        for (int i = tid; i < V; i += kInFlight * NT) {
            float xa[kInFlight], yb[kInFlight];
#pragma unroll
            for (int k = 0; k < kInFlight; ++k) {
                const bool ok = i + k * NT < V;
                xa[k] = ok ? clampf(IO::get(p + i + k * NT) * inv_t) : -kFltMaxG;
                yb[k] = ok ? clampf(IO::get(q + i + k * NT) * inv_t) : -kFltMaxG;
            }
            f(xa, yb);
        }
    }
}

struct KlOut { float *kl, *lx, *ly, *klp; };

// ================================================================================================
// the forward: ONE launch.  NT = 256: a workgroup per row, the four waves meet through 4 x 5 LDS words (and 4 x 2 for the
// second pass of jsd), double-buffered by row parity; NT = 64: a wave per row, four rows per workgroup.
// ================================================================================================
template <class Elem, bool WIDE, int NT, int MODE>
__global__ __launch_bounds__(256) void lm_kl_kernel(const Elem* __restrict__ x, const Elem* __restrict__ y,
                                                    const float* __restrict__ weight, const KlOut out, long rows, int V,
                                                    float inv_t, float beta) {
    constexpr int RPW = 256 / NT;
    __shared__ float red[2][4][5];
    __shared__ float red2[2][4][2];
    const int tid = threadIdx.x % NT, sub = threadIdx.x / NT;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int par = 0;
    for (long r0 = (long)blockIdx.x * RPW; r0 < rows; r0 += (long)gridDim.x * RPW) {
        const long row = r0 + sub;
        const bool have = row < rows;
        const bool live = have && (weight ? weight[row] != 0.f : true);   // the same for all NT threads of the row
        float val = 0.f, vlx = 0.f, vly = 0.f, vkp = 0.f;
        if (live) {
            const Elem* p = x + (size_t)row * (size_t)V;
            const Elem* q = y + (size_t)row * (size_t)V;
            PairStat a{-kFltMaxG, 0.f, -kFltMaxG, 0.f, 0.f};
            walk_pair<Elem, WIDE, NT, MODE == kJsd>(p, q, V, tid, inv_t,
                                                    [&](const auto& xa, const auto& yb) { pair_update<MODE>(a, xa, yb); });
            PairStat st = pair_wave<MODE>(a);
            if (NT == 256) {   // a workgroup per row: `live` is uniform over it
                if (lane == 0) {
                    red[par][wv][0] = st.mx;
                    red[par][wv][1] = st.sx;
                    red[par][wv][2] = st.my;
                    red[par][wv][3] = st.sy;
                    red[par][wv][4] = st.u;
                }
                __syncthreads();
                if (MODE == kJsd || threadIdx.x == 0) {   // jsd: every thread needs lx and ly, and merges the same words
                    PairStat w4[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        w4[i] = PairStat{red[par][i][0], red[par][i][1], red[par][i][2], red[par][i][3], red[par][i][4]};
                    st = pair_merge<MODE>(pair_merge<MODE>(w4[0], w4[1]), pair_merge<MODE>(w4[2], w4[3]));
                }
            }
            // sx, sy are in [1, V]: the bare log2.  lx - ly is formed from the parts, not from the two sums of size ln V
            const float lsx = __builtin_amdgcn_logf(st.sx) * kLn2G, lsy = __builtin_amdgcn_logf(st.sy) * kLn2G;
            const float dl = (st.mx - st.my) + (lsx - lsy);
            vlx = st.mx + lsx;
            vly = st.my + lsy;
            if constexpr (MODE == kFwd) val = st.u / st.sy + dl;
            if constexpr (MODE == kRev) val = st.u / st.sx - dl;
            if constexpr (MODE == kJsd) {
                float kq = 0.f, kp = 0.f;
                walk_pair<Elem, WIDE, NT, false>(p, q, V, tid, inv_t, [&](const auto& xa, const auto& yb) {
                    constexpr int N = sizeof(xa) / sizeof(float);
#pragma unroll
                    for (int i = 0; i < N; ++i) {
                        const float pe = ex2((xa[i] - vlx) * kLog2eG), qe = ex2((yb[i] - vly) * kLog2eG);
                        float lpm, lqm;
                        jsd_logs((xa[i] - yb[i]) - dl, beta, lpm, lqm);
                        kp = fmaf(pe, pe == 0.f ? 0.f : lpm, kp);
                        kq = fmaf(qe, qe == 0.f ? 0.f : lqm, kq);
                    }
                });
                kq = wave_sum(kq);
                kp = wave_sum(kp);
                if (NT == 256) {
                    if (lane == 0) {
                        red2[par][wv][0] = kq;
                        red2[par][wv][1] = kp;
                    }
                    __syncthreads();
                    if (threadIdx.x == 0) {
                        kq = (red2[par][0][0] + red2[par][1][0]) + (red2[par][2][0] + red2[par][3][0]);
                        kp = (red2[par][0][1] + red2[par][1][1]) + (red2[par][2][1] + red2[par][3][1]);
                    }
                }
                val = fmaf(beta, kq, (1.f - beta) * kp);
                vkp = kp;
            }
            if (NT == 256) par ^= 1;   // the next row writes the other half: one barrier per row and pass
        }
        if (tid == 0 && have) {
            out.kl[row] = val;
            out.lx[row] = vlx;
            out.ly[row] = vly;
            if constexpr (MODE == kJsd) out.klp[row] = vkp;
        }
    }
}

// ================================================================================================
// the gradient towards x: one streaming launch
// ================================================================================================
struct KlSaved { const float *g, *weight, *kl, *lx, *ly, *klp; };

template <class Elem, bool WIDE, int NT, int MODE>
__global__ __launch_bounds__(256) void lm_kl_grad_kernel(const Elem* __restrict__ x, const Elem* __restrict__ y, const KlSaved s,
                                                         Elem* __restrict__ grad, long rows, int V, float inv_t, float beta) {
    constexpr int RPW = 256 / NT;
    const int tid = threadIdx.x % NT, sub = threadIdx.x / NT;
    for (long r0 = (long)blockIdx.x * RPW; r0 < rows; r0 += (long)gridDim.x * RPW) {
        const long row = r0 + sub;
        if (row >= rows) continue;
        const bool live = s.weight ? s.weight[row] != 0.f : true;
        const float c = live ? s.g[row] * inv_t : 0.f;
        const Elem* p = x + (size_t)row * (size_t)V;
        const Elem* q = y + (size_t)row * (size_t)V;
        Elem* o = grad + (size_t)row * (size_t)V;
        if (!live || c == 0.f) {   // NaN != 0: a NaN upstream gradient still reaches its row
            zero_row<Elem, WIDE, NT>(o, V, tid);
            continue;
        }
        const float lx = s.lx[row], ly = s.ly[row];
        if constexpr (MODE == kFwd) {
            stream_row2<Elem, WIDE, NT>(p, q, o, V, tid, [&](float xv, float yv) {
                const float pe = ex2((clampf(xv * inv_t) - lx) * kLog2eG), qe = ex2((clampf(yv * inv_t) - ly) * kLog2eG);
                return c * (pe - qe);
            });
        } else if constexpr (MODE == kRev) {
            const float k0 = (lx - ly) + s.kl[row];
            stream_row2<Elem, WIDE, NT>(p, q, o, V, tid, [&](float xv, float yv) {
                const float a = clampf(xv * inv_t), b = clampf(yv * inv_t);
                const float pe = ex2((a - lx) * kLog2eG);
                return pe == 0.f ? 0.f : c * pe * ((a - b) - k0);   // a masked entry: exactly 0, never 0 * huge
            });
        } else {
            const float dl = lx - ly, kp = s.klp[row], c1 = c * (1.f - beta);
            stream_row2<Elem, WIDE, NT>(p, q, o, V, tid, [&](float xv, float yv) {
                const float a = clampf(xv * inv_t), b = clampf(yv * inv_t);
                const float pe = ex2((a - lx) * kLog2eG);
                float lpm, lqm;
                jsd_logs((a - b) - dl, beta, lpm, lqm);
                return pe == 0.f ? 0.f : c1 * pe * (lpm - kp);
            });
        }
    }
}

// f(MODE) as a std::integral_constant
template <class F> void with_mode(int mode, F&& f) {
    if (mode == kFwd) f(std::integral_constant<int, kFwd>{});
    else if (mode == kRev) f(std::integral_constant<int, kRev>{});
    else f(std::integral_constant<int, kJsd>{});
}

int lm_kl_head_any(const void* xv, const void* yv, int elem, const float* weight, const KlOut& out, long rows, int V, int mode,
                   float beta, float inv_t, hipStream_t st) {
    return with_elem(elem, [&](auto e) {
        using Elem = decltype(e);
        const Elem *x = static_cast<const Elem*>(xv), *y = static_cast<const Elem*>(yv);
        const RowLaunch L = row_launch<Elem>(x, y, rows, V);
        with_row_kernel(L, [&](auto W, auto NT) {
            with_mode(mode, [&](auto M) {
                hipLaunchKernelGGL((lm_kl_kernel<Elem, decltype(W)::value, decltype(NT)::value, decltype(M)::value>),
                                   dim3((unsigned)L.grid), dim3(256), 0, st, x, y, weight, out, rows, V, inv_t, beta);
            });
        });
        const int rc = last_error();
        if (!rc) g_kl_head.note({ElemIO<Elem>::kCode, L.wide ? 16 : (int)sizeof(Elem), L.nt, L.rpw, (int)L.grid, mode});
        return rc;
    });
}

int lm_kl_grad_any(const void* xv, const void* yv, int elem, const KlSaved& s, void* gradv, long rows, int V, int mode, float beta,
                   float inv_t, hipStream_t st) {
    return with_elem(elem, [&](auto e) {
        using Elem = decltype(e);
        const Elem *x = static_cast<const Elem*>(xv), *y = static_cast<const Elem*>(yv);
        Elem* grad = static_cast<Elem*>(gradv);
        RowLaunch L = row_launch<Elem>(x, grad, rows, V);
        L.wide = L.wide && aligned(y, 16);
        with_row_kernel(L, [&](auto W, auto NT) {
            with_mode(mode, [&](auto M) {
                hipLaunchKernelGGL((lm_kl_grad_kernel<Elem, decltype(W)::value, decltype(NT)::value, decltype(M)::value>),
                                   dim3((unsigned)L.grid), dim3(256), 0, st, x, y, s, grad, rows, V, inv_t, beta);
            });
        });
        const int rc = last_error();
        if (!rc) g_kl_grad.note({ElemIO<Elem>::kCode, L.wide ? 16 : (int)sizeof(Elem), L.nt, L.rpw, (int)L.grid, mode});
        return rc;
    });
}

// mode, beta and the inverse temperature: what both entries refuse before anything else is looked at
bool kl_scalars_ok(int mode, float beta, float inv_t) {
    if (mode != kFwd && mode != kRev && mode != kJsd) return false;
    if (mode == kJsd && !(beta > 0.f && beta < 1.f)) return false;
    return inv_t > 0.f && inv_t <= kFltMaxG;
}

}  // namespace
}  // namespace hpc_rll

using namespace hpc_rll;

extern "C" int hpc_rll_lm_kl_forward(const void* logits, const void* teacher, int elem, const float* weight, float* kl,
                                     float* lse_x, float* lse_y, float* kl_pm, int64_t rows, int V, int mode, float beta,
                                     float inv_temperature, void* stream) {
    const bool empty = rows == 0 || V == 0;
    if (!kl_scalars_ok(mode, beta, inv_temperature)) return HPC_RLL_EINVAL;
    if (!empty && (!logits || !teacher || !kl || !lse_x || !lse_y || (mode == kJsd && !kl_pm))) return HPC_RLL_EINVAL;
    if (const int bad = lm_shape_status(rows, 1, V, elem, aligned(logits, elem_size(elem)) && aligned(teacher, elem_size(elem)) &&
                                        aligned(weight, 4) && aligned(kl, 4) && aligned(lse_x, 4) && aligned(lse_y, 4) &&
                                        aligned(kl_pm, 4)))
        return bad;
    hipStream_t st = (hipStream_t)stream;
    if (empty) {   // V == 0 with rows: nothing to diverge over; zeros
        for (float* o : {kl, lse_x, lse_y, kl_pm})
            if (rows > 0 && o) {
                const int rc = (int)hipMemsetAsync(o, 0, (size_t)rows * sizeof(float), st);
                if (rc) return rc;
            }
        return HPC_RLL_OK;
    }
    return lm_kl_head_any(logits, teacher, elem, weight, KlOut{kl, lse_x, lse_y, kl_pm}, (long)rows, V, mode, beta, inv_temperature,
                          st);
}

extern "C" int hpc_rll_lm_kl_backward(const float* g, const void* logits, const void* teacher, int elem, const float* weight,
                                      const float* kl, const float* lse_x, const float* lse_y, const float* kl_pm,
                                      void* grad_logits, int64_t rows, int V, int mode, float beta, float inv_temperature,
                                      void* stream) {
    const bool empty = rows == 0 || V == 0;
    if (!kl_scalars_ok(mode, beta, inv_temperature)) return HPC_RLL_EINVAL;
    if (!empty && (!g || !logits || !teacher || !kl || !lse_x || !lse_y || !grad_logits || (mode == kJsd && !kl_pm)))
        return HPC_RLL_EINVAL;
    if (const int bad = lm_shape_status(rows, 1, V, elem, aligned(logits, elem_size(elem)) && aligned(teacher, elem_size(elem)) &&
                                        aligned(grad_logits, elem_size(elem)) && aligned(g, 4) && aligned(weight, 4) &&
                                        aligned(kl, 4) && aligned(lse_x, 4) && aligned(lse_y, 4) && aligned(kl_pm, 4)))
        return bad;
    if (empty) return HPC_RLL_OK;
    return lm_kl_grad_any(logits, teacher, elem, KlSaved{g, weight, kl, lse_x, lse_y, kl_pm}, grad_logits, (long)rows, V, mode, beta,
                          inv_temperature, (hipStream_t)stream);
}

extern "C" int hpc_rll_lm_kl_last_config(int* out) {
    if (!out) return HPC_RLL_EINVAL;
    g_kl_head.read(out);
    g_kl_grad.read(out + kKlInts);
    return HPC_RLL_OK;
}
static_assert(HPC_RLL_LM_KL_CONFIG_INTS == 2 * kKlInts, "the layout documented in hpc_rll_hip.h");
