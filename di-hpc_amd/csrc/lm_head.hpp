// lm_head.hpp -- what the language-model units grpo.hip and lm_ppo.hip share.  Each delicate piece exists once:
//   * the limits of a row launch and the two element types of the logits (fp32, bf16) with their 16-byte pack / unpack;
//   * RowStat<ENT>: the online softmax statistic of a lane, with the entropy moment only when ENT, its merge, wave
//     butterfly and batch update, and row_stats, the walk of one row (unaligned peel, kInFlight loads in flight, guarded tail);
//   * lm_head_kernel<Elem, ALIGNED, NT, ENT> and its launcher: GRPO instantiates ENT = false, LM-PPO ENT = true;
//   * zero_row / stream_row: the row-streaming body of the two gradient kernels, around the unit's own element formula;
//   * seq_weight_sum: the first pass of the token-loss kernels over a sequence;
//   * with_elem / with_row_kernel: the element type and the two-by-two kernel choice of a row launch as types;
//   * lm_shape_status: the argument checks the C entry points repeat.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "hostutil.hpp"
#include "hpc_rll_hip.h"
#include "wave.hpp"

namespace hpc_rll {

constexpr int kGrpoMaxV = 262144;
constexpr int kWaveRowMaxV = 2048;   // up to here a wave per row, above a workgroup per row
constexpr int kInFlight = 4;         // 16-byte loads a lane issues before it uses the first
constexpr float kFltMaxG = 3.402823466e+38f;
constexpr float kLog2eG = 1.44269504088896340736f, kLn2G = 0.69314718055994530942f;
constexpr long kRowGridMax = 1L << 16;   // workgroups of a row launch; above it they loop (far more than the device holds at once)

typedef unsigned int vuint4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float clampf(float x) { return fmaxf(x, -kFltMaxG); }   // -inf (masked) and NaN -> finite
__device__ __forceinline__ float ex2(float y) { return __builtin_amdgcn_exp2f(y); }
__device__ __forceinline__ float as_f(unsigned u) { return __builtin_bit_cast(float, u); }
__device__ __forceinline__ unsigned as_u(float f) { return __builtin_bit_cast(unsigned, f); }

// ---- the two element types: P elements per 16 bytes
template <class Elem> struct ElemIO;
template <> struct ElemIO<float> {
    static constexpr int P = 4;
    static constexpr int kCode = 0;
    static __device__ __forceinline__ float get(const float* p) { return *p; }
    static __device__ __forceinline__ void put(float* p, float v) { __builtin_nontemporal_store(v, p); }
    static __device__ __forceinline__ void unpack(const vuint4& v, float* x) {
        x[0] = as_f(v.x); x[1] = as_f(v.y); x[2] = as_f(v.z); x[3] = as_f(v.w);
    }
    static __device__ __forceinline__ vuint4 pack(const float* x) {
        vuint4 v = {as_u(x[0]), as_u(x[1]), as_u(x[2]), as_u(x[3])};
        return v;
    }
};
__device__ __forceinline__ unsigned bf16_bits(float f) {   // round to nearest even
    return (unsigned)__builtin_bit_cast(unsigned short, static_cast<__bf16>(f));
}
template <> struct ElemIO<uint16_t> {
    static constexpr int P = 8;
    static constexpr int kCode = 1;
    static __device__ __forceinline__ float get(const uint16_t* p) { return as_f((unsigned)*p << 16); }
    static __device__ __forceinline__ void put(uint16_t* p, float v) { __builtin_nontemporal_store((uint16_t)bf16_bits(v), p); }
    static __device__ __forceinline__ void unpack(const vuint4& v, float* x) {
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            x[2 * i] = as_f(w[i] << 16);
            x[2 * i + 1] = as_f(w[i] & 0xffff0000u);
        }
    }
    static __device__ __forceinline__ vuint4 pack(const float* x) {
        unsigned w[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) w[i] = bf16_bits(x[2 * i]) | (bf16_bits(x[2 * i + 1]) << 16);
        vuint4 v = {w[0], w[1], w[2], w[3]};
        return v;
    }
};

// ---- online softmax statistics of what a lane has seen: m the maximum (never below -FLT_MAX), s = sum e^(x-m) and, with
// ENT, the entropy moment u = sum e^(x-m) (x-m).  An entry whose exponential is 0 (a clamped -inf or NaN, or anything 88
// below the maximum) adds exactly 0 to u BY SELECTION: 0 * (-huge) is never formed.  The plain statistic has no u at all.
template <bool ENT> struct RowStat;
template <> struct RowStat<false> { float m, s; };
template <> struct RowStat<true> { float m, s, u; };

// `a` moved from its maximum to m >= a.m
template <bool ENT> __device__ __forceinline__ RowStat<ENT> stat_shift(const RowStat<ENT>& a, float m) {
    const float d = a.m - m;
    const float e = ex2(d * kLog2eG);
    RowStat<ENT> r{m, a.s * e};
    if constexpr (ENT) r.u = e == 0.f ? 0.f : (a.u + d * a.s) * e;
    return r;
}
template <bool ENT> __device__ __forceinline__ RowStat<ENT> stat_merge(const RowStat<ENT>& a, const RowStat<ENT>& b) {
    const float m = fmaxf(a.m, b.m);
    const RowStat<ENT> sa = stat_shift(a, m), sb = stat_shift(b, m);
    RowStat<ENT> r{m, sa.s + sb.s};
    if constexpr (ENT) r.u = sa.u + sb.u;
    return r;
}
template <bool ENT> __device__ __forceinline__ RowStat<ENT> stat_wave(RowStat<ENT> a) {   // all 64 lanes end with the wave's
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) {
        RowStat<ENT> o{__shfl_xor(a.m, k, 64), __shfl_xor(a.s, k, 64)};
        if constexpr (ENT) o.u = __shfl_xor(a.u, k, 64);
        a = stat_merge(a, o);
    }
    return a;
}

// One batch of kInFlight vectors: a single rescale of the running sums, then the elements in order.  GUARD: vector k counts
// only when ok[k].
template <class Elem, bool GUARD, bool ENT>
__device__ __forceinline__ void stat_batch(RowStat<ENT>& a, const vuint4 (&r)[kInFlight], const bool (&ok)[kInFlight]) {
    constexpr int P = ElemIO<Elem>::P;
    float x[kInFlight * P];
    float bm = -kFltMaxG;
#pragma unroll
    for (int k = 0; k < kInFlight; ++k) {
        ElemIO<Elem>::unpack(r[k], x + k * P);
#pragma unroll
        for (int j = 0; j < P; ++j) {
            float v = clampf(x[k * P + j]);
            if (GUARD) v = ok[k] ? v : -kFltMaxG;
            x[k * P + j] = v;
            bm = fmaxf(bm, v);
        }
    }
    RowStat<ENT> n = stat_shift(a, fmaxf(a.m, bm));
#pragma unroll
    for (int i = 0; i < kInFlight * P; ++i) {
        const float t = x[i] - n.m;
        const float e = ex2(t * kLog2eG);
        n.s += e;
        if constexpr (ENT) n.u = fmaf(e, e == 0.f ? 0.f : t, n.u);   // a zero exponential selects t away: 0 * 0, exactly nothing
    }
    a = n;
}

// The statistic of lane `tid` of the NT that share the row p[0, V).  ALIGNED = false peels the elements in front of the first
// and behind the last 16-byte boundary of the row, so no wide load is misaligned or leaves the row.
template <class Elem, bool ALIGNED, int NT, bool ENT>
__device__ __forceinline__ RowStat<ENT> row_stats(const Elem* __restrict__ p, int V, int tid) {
    using IO = ElemIO<Elem>;
    constexpr int P = IO::P;
    int h = 0;
    if (!ALIGNED) {
        h = (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) / sizeof(Elem));
        h = h < V ? h : V;
    }
    const int nvec = (V - h) / P;
    RowStat<ENT> a{-kFltMaxG, 0.f};
    if (!ALIGNED) {   // the elements outside the 16-byte grid of the row: fewer than 2 P, one lane each
        const int tail = V - h - nvec * P;
        if (tid < h + tail) {
            const int i = tid < h ? tid : h + nvec * P + (tid - h);
            a.m = clampf(IO::get(p + i));
            a.s = 1.f;
        }
    }
    const vuint4* __restrict__ pv = reinterpret_cast<const vuint4*>(p + h);
    const bool all[kInFlight] = {true, true, true, true};
    int v = tid;
    for (; v + (kInFlight - 1) * NT < nvec; v += kInFlight * NT) {
        vuint4 r[kInFlight];
#pragma unroll
        for (int k = 0; k < kInFlight; ++k) r[k] = __builtin_nontemporal_load(pv + v + k * NT);
        stat_batch<Elem, false>(a, r, all);
    }
    if (v < nvec) {
        vuint4 r[kInFlight];
        bool ok[kInFlight];
#pragma unroll
        for (int k = 0; k < kInFlight; ++k) {
            ok[k] = v + k * NT < nvec;
            const vuint4 z = {0u, 0u, 0u, 0u};
            r[k] = z;
            if (ok[k]) r[k] = __builtin_nontemporal_load(pv + v + k * NT);
        }
        stat_batch<Elem, true>(a, r, ok);
    }
    return a;
}

// ================================================================================================
// the head: ONE read of the row.  logp[row] = x[a] - lse, lse[row] = m + ln s (lse may be NULL) and, with ENT,
// ent[row] = ln s - u/s.  NT = 256: a workgroup per row, the four waves meet through 4 (2 + ENT) LDS words, double-buffered
// so that a row costs one barrier; NT = 64: a wave per row, four rows per workgroup.  A dropped row (action outside [0,V), or
// weight 0) is not read: its outputs are 0.
// ================================================================================================
template <class Elem, bool ALIGNED, int NT, bool ENT>
static __global__ __launch_bounds__(256) void lm_head_kernel(const Elem* __restrict__ x, const int64_t* __restrict__ action,
                                                             const float* __restrict__ weight, float* __restrict__ logp,
                                                             float* __restrict__ lse, float* __restrict__ ent, long rows,
                                                             int V) {
    constexpr int RPW = 256 / NT, NS = ENT ? 3 : 2;
    __shared__ float red[2][4][NS];
    const int tid = threadIdx.x % NT, sub = threadIdx.x / NT;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int par = 0;
    for (long r0 = (long)blockIdx.x * RPW; r0 < rows; r0 += (long)gridDim.x * RPW) {
        const long row = r0 + sub;
        const bool have = row < rows;
        long a = -1;
        float w = 1.f;
        if (have) {
            a = action[row];
            if (weight) w = weight[row];
        }
        const bool live = have && a >= 0 && a < (long)V && w != 0.f;   // the same for all NT threads of the row
        RowStat<ENT> st{-kFltMaxG, 0.f};
        float xa = 0.f;
        if (live) {
            const Elem* p = x + (size_t)row * (size_t)V;
            if (tid == 0) xa = clampf(ElemIO<Elem>::get(p + a));
            st = stat_wave(row_stats<Elem, ALIGNED, NT, ENT>(p, V, tid));
            if (NT == 256) {   // a workgroup per row: `live` is uniform over it
                if (lane == 0) {
                    red[par][wv][0] = st.m;
                    red[par][wv][1] = st.s;
                    if constexpr (ENT) red[par][wv][2] = st.u;
                }
                __syncthreads();
                if (threadIdx.x == 0) {
                    RowStat<ENT> q[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        q[i].m = red[par][i][0];
                        q[i].s = red[par][i][1];
                        if constexpr (ENT) q[i].u = red[par][i][2];
                    }
                    st = stat_merge(stat_merge(q[0], q[1]), stat_merge(q[2], q[3]));
                }
                par ^= 1;   // the next row writes the other half: one barrier per row
            }
        }
        if (tid == 0 && have) {
            [[maybe_unused]] float h = 0.f;
            float l = 0.f, lp = 0.f;
            if (live) {
                const float ls = __builtin_amdgcn_logf(st.s) * kLn2G;   // s is in [1, V]: the bare log2
                l = st.m + ls;
                lp = xa - l;
                if constexpr (ENT) h = ls - st.u / st.s;
            }
            logp[row] = lp;
            if (lse) lse[row] = l;
            if constexpr (ENT) ent[row] = h;
        }
    }
}

// ================================================================================================
// the row-streaming body of the gradient kernels, for lane `tid` of the NT that share the row.  WIDE needs both bases and the
// row pitch on 16 bytes; otherwise one element per access (input and output rows do not share an alignment, so peeling cannot
// serve both).  Nontemporal stores in the logits' dtype (bf16: round to nearest even).
// ================================================================================================
// A row whose coefficients are all 0: zero-filled, its logits are not read.
template <class Elem, bool WIDE, int NT> __device__ __forceinline__ void zero_row(Elem* o, int V, int tid) {
    using IO = ElemIO<Elem>;
    if (WIDE) {
        const vuint4 z = {0u, 0u, 0u, 0u};
        vuint4* ov = reinterpret_cast<vuint4*>(o);
        for (int v = tid; v < V / IO::P; v += NT) __builtin_nontemporal_store(z, ov + v);
    } else {
        for (int i = tid; i < V; i += NT) IO::put(o + i, 0.f);
    }
}
// o[v] = f(p[v], v == ai), kInFlight loads in flight; ai = -1 chooses no column.
template <class Elem, bool WIDE, int NT, class F>
__device__ __forceinline__ void stream_row(const Elem* p, Elem* o, int V, int tid, int ai, F&& f) {
    using IO = ElemIO<Elem>;
    constexpr int P = IO::P;
    if (WIDE) {
        const int nvec = V / P;
        const vuint4* __restrict__ pv = reinterpret_cast<const vuint4*>(p);
        vuint4* ov = reinterpret_cast<vuint4*>(o);
        for (int v = tid; v < nvec; v += kInFlight * NT) {
            vuint4 r[kInFlight];
#pragma unroll
            for (int k = 0; k < kInFlight; ++k)
                if (v + k * NT < nvec) r[k] = __builtin_nontemporal_load(pv + v + k * NT);
#pragma unroll
            for (int k = 0; k < kInFlight; ++k)
                if (v + k * NT < nvec) {
                    float xx[P];
                    IO::unpack(r[k], xx);
                    const int da = ai - (v + k * NT) * P;
#pragma unroll
                    for (int j = 0; j < P; ++j) xx[j] = f(xx[j], da == j);
                    __builtin_nontemporal_store(IO::pack(xx), ov + v + k * NT);
                }
        }
    } else {
        for (int i = tid; i < V; i += kInFlight * NT) {
            float xx[kInFlight];
#pragma unroll
            for (int k = 0; k < kInFlight; ++k)
                if (i + k * NT < V) xx[k] = IO::get(p + i + k * NT);
#pragma unroll
            for (int k = 0; k < kInFlight; ++k)
                if (i + k * NT < V) IO::put(o + i + k * NT, f(xx[k], ai == i + k * NT));
        }
    }
}

// The first pass of a token-loss wave over its sequence [base, base + S): the weight of the live tokens (action in [0,V),
// w != 0), in every lane.
__device__ __forceinline__ float seq_weight_sum(const int64_t* __restrict__ action, const float* __restrict__ weight, size_t base,
                                                int S, int V, int lane) {
    float sw = 0.f;
    for (int s = lane; s < S; s += 64) {
        const long a = action[base + s];
        const float w = weight ? weight[base + s] : 1.f;
        sw += (a >= 0 && a < (long)V && w != 0.f) ? w : 0.f;
    }
    return wave_sum(sw);
}

// ---- host side -------------------------------------------------------------------------------------------------------------
inline bool elem_ok(int e) { return e == HPC_RLL_ELEM_F32 || e == HPC_RLL_ELEM_BF16; }
inline size_t elem_size(int e) { return e == HPC_RLL_ELEM_BF16 ? 2 : 4; }

// A row launch over (rows, V) logits: 256 threads, a wave (V <= kWaveRowMaxV) or the workgroup per row; `wide`: x, the output
// o when there is one, and the row pitch lie on 16 bytes.
struct RowLaunch { bool wide; int nt, rpw; long grid; };
template <class Elem> RowLaunch row_launch(const Elem* x, const Elem* o, long rows, int V) {
    RowLaunch L;
    L.wide = aligned(x, 16) && aligned(o, 16) && ((size_t)V * sizeof(Elem)) % 16 == 0;
    L.nt = V > kWaveRowMaxV ? 256 : 64;
    L.rpw = 256 / L.nt;
    const long grid = (rows + L.rpw - 1) / L.rpw;
    L.grid = grid < 1 ? 1 : (grid > kRowGridMax ? kRowGridMax : grid);
    return L;
}
// f(Elem{}) for the element type code of the C ABI
template <class F> int with_elem(int elem, F&& f) { return elem == HPC_RLL_ELEM_BF16 ? f(uint16_t{}) : f(float{}); }
// f(WIDE, NT) as std::integral_constants (WIDE is the head's ALIGNED): the kernel of the launch
template <class F> void with_row_kernel(const RowLaunch& L, F&& f) {
    using NT256 = std::integral_constant<int, 256>;
    using NT64 = std::integral_constant<int, 64>;
    if (L.wide && L.nt == 256) f(std::true_type{}, NT256{});
    else if (L.wide) f(std::true_type{}, NT64{});
    else if (L.nt == 256) f(std::false_type{}, NT256{});
    else f(std::false_type{}, NT64{});
}

// The head launch of either unit, noted in the unit's own record `rec`:
// [element type, bytes per load, peeled, threads per row, rows per workgroup, workgroups]
template <bool ENT>
int lm_head_launch(const void* xv, int elem, const int64_t* action, const float* weight, float* logp, float* lse, float* ent,
                   long rows, int V, hipStream_t st, LaunchRecord<7>& rec) {
    return with_elem(elem, [&](auto e) {
        using Elem = decltype(e);
        const Elem* x = static_cast<const Elem*>(xv);
        const RowLaunch L = row_launch<Elem>(x, nullptr, rows, V);
        with_row_kernel(L, [&](auto AL, auto NT) {
            hipLaunchKernelGGL((lm_head_kernel<Elem, decltype(AL)::value, decltype(NT)::value, ENT>), dim3((unsigned)L.grid), dim3(256), 0, st, x, action,
                               weight, logp, lse, ent, rows, V);
        });
        const int rc = last_error();
        if (!rc) rec.note({ElemIO<Elem>::kCode, 16, L.wide ? 0 : 1, L.nt, L.rpw, (int)L.grid});
        return rc;
    });
}

// What the C entry points check after their own required pointers, in the order all of them keep: sizes and element type,
// then `al` (every pointer of the entry is aligned), then the width.
inline int lm_shape_status(int64_t n0, int64_t n1, int V, int elem, bool al) {
    if (n0 < 0 || n1 < 0 || V < 0 || !elem_ok(elem)) return HPC_RLL_EINVAL;
    if (!al) return HPC_RLL_EALIGN;
    return V > kGrpoMaxV ? HPC_RLL_EUNSUPPORTED : HPC_RLL_OK;
}

}  // namespace hpc_rll
