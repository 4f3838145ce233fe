// lm_topk.hip -- distillation from a top-k teacher on gfx950: token_topk selects the k largest entries of a row of logits with
// their log-probabilities (the producer, on the teacher's side), token_topk_kl_div is the divergence of a student's full row
// against such a sparse teacher with its streaming gradient (the consumer).  No reference counterpart; hpc_rll_hip.h has the
// formulas and the order of the selection.
//
// Kernels:
//   * lm_topk_kernel<Elem, WIDE>: a workgroup per row at every V (the selection meets in LDS: a wave-per-row instance would
//     repeat all of it for rows of at most 2048 entries, where the launch is latency-bound either way), the looping grid.
//     Radix select on the order-preserving 32-bit key of clampf(x) + 0, 11 + 11 + 10 bits:
//       1. the only read from memory (plain loads: the lines stay cached).  Each lane updates its RowStat<false> of
//          a = clampf(x / T) and adds every element to a 2048-bin LDS histogram of the top 11 key bits (integer LDS atomics: the
//          counts do not depend on order).  After the first batch of a long row a scan of what is there gives a floor bin -- the
//          k-th largest of a part lies at or below the k-th largest of the whole -- and the rest of the row only counts
//          elements at or above it, which takes the same-address atomics of a bell-shaped row off the LDS pipeline;
//       2. pick_bin: a suffix scan over the bins (8 bins a thread, wave shuffles, four wave totals) finds the bin of the k-th
//          largest key and the count strictly above it;
//       3. only a bin that holds more than kCand entries (heavy ties, constant rows) takes a further histogram level over the
//          row, restricted to the prefix so far, until it fits or the key is exhausted;
//       4. the collecting read: entries above the prefix go straight to the selection, entries that match it to the LDS
//          candidate buffer (key and index in one 64-bit word), where rank counting -- as tqc.hip ranks its atoms -- takes the
//          `need` largest, equal keys by ascending index;
//       5. with the key exhausted and the bin still too large every match EQUALS the threshold key: each wave owns a contiguous
//          span of the row, the waves' counts are prefix-summed once, and each wave walks its span in index order with ballot /
//          popcount ranks, taking the lowest indices -- wave-synchronous, coalesced, no barrier per chunk;
//       6. the k selected words are ordered by rank counting and written with their log-probabilities (the raw element is
//          fetched again: a NaN or -inf element carries -inf).
//   * lm_topk_kl_kernel<Elem, WIDE, NT>: the row mapping of lm_kl_kernel.  The row's owners set the bits of the live teacher
//     indices in an LDS bitmap (V bits for a workgroup per row, 2048 for each wave's row) and keep (index, logp) in an LDS table;
//     the single read of the row carries one running maximum and TWO sums, inside and outside the set -- the student's tail
//     mass 1 - P is summed, never subtracted -- reading one bitmap word per 16-byte vector; a set bit (rare) looks its slot up
//     and leaves its scaled logit there.  One wave then sums the k entries in a fixed order.
//   * lm_topk_kl_grad_kernel<Elem, WIDE, NT>: one streaming launch; it rebuilds the bitmap and the table and writes every
//     gradient element exactly once, c (A p_v) outside the set and c (A' p_v - q_v) on a set bit.
// No float atomics; every float sum has a fixed order, so two runs give the same bits.
#include <hip/hip_runtime.h>

#include "hostutil.hpp"
#include "hpc_rll_hip.h"
#include "lm_head.hpp"
#include "wave.hpp"

namespace hpc_rll {
namespace {

constexpr int kMaxK = HPC_RLL_LM_TOPK_MAX_K;   // 256: one selected entry a thread
constexpr int kBins = 2048;                    // 11 key bits a level
constexpr int kCand = 1024;                    // candidates of the threshold bin kept in LDS (four a thread)
constexpr int kRenorm = HPC_RLL_TOPK_TAIL_RENORM, kBucket = HPC_RLL_TOPK_TAIL_BUCKET;
constexpr float kInfG = __builtin_huge_valf();

// [element type, bytes per access, threads per row, rows per workgroup, workgroups, k]
constexpr int kTopkInts = 7;
LaunchRecord<kTopkInts> g_topk_sel;
LaunchRecord<kTopkInts> g_topk_kl;
LaunchRecord<kTopkInts> g_topk_grad;

typedef unsigned long long u64;

// The walk of lane `tid` of the NT that share a row over its groups [g0, g1): a group is the P elements of a 16-byte vector
// (WIDE) or one element.  kInFlight loads are issued before the first is used.  f(x, at): x the raw elements as floats, at[k]
// the index of group k's first element, -1 when the group lies past the end (its x are 0).  CACHED: plain loads.
template <class Elem, bool WIDE, int NT, bool CACHED, class F>
__device__ __forceinline__ void walk_row(const Elem* __restrict__ p, int g0, int g1, int tid, F&& f) {
    using IO = ElemIO<Elem>;
    constexpr int W = WIDE ? IO::P : 1;
    for (int v = g0 + tid; v < g1; v += kInFlight * NT) {
        float x[kInFlight * W];
        int at[kInFlight];
        if constexpr (WIDE) {
            const vuint4* __restrict__ pv = reinterpret_cast<const vuint4*>(p);
            vuint4 r[kInFlight];
            const vuint4 z = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int k = 0; k < kInFlight; ++k) {
                const bool ok = v + k * NT < g1;
                r[k] = z;
                if (ok) r[k] = ld<!CACHED>(pv + v + k * NT);
                at[k] = ok ? (v + k * NT) * W : -1;
            }
#pragma unroll
            for (int k = 0; k < kInFlight; ++k) IO::unpack(r[k], x + k * W);
        } else {
#pragma unroll
            for (int k = 0; k < kInFlight; ++k) {
                const bool ok = v + k * NT < g1;
                x[k] = ok ? IO::get(p + v + k * NT) : 0.f;
                at[k] = ok ? v + k * NT : -1;
            }
        }
        f(x, at);
    }
}

// larger key <=> larger clampf(x) + 0: NaN and -inf share the key of -FLT_MAX, -0 that of +0
__device__ __forceinline__ unsigned order_key(float x) {
    const unsigned u = as_u(clampf(x) + 0.0f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// key and index in one word: a larger word comes earlier in the output (equal keys: the lower index)
__device__ __forceinline__ u64 sel_word(unsigned key, int idx) { return ((u64)key << 32) | (u64)(~(unsigned)idx); }

__device__ __forceinline__ int wave_sum_i(int x) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
    return x;
}

// The bin of the need-th largest counted entry: found = {bin, entries strictly above it, entries in it}, bin -1 when fewer
// than `need` entries are counted.  All 256 threads call it; it begins and ends with a barrier.  CLEAR zeroes the bins.
template <bool CLEAR> __device__ __forceinline__ void pick_bin(unsigned* hist, int* wsum, int* found, int need) {
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    __syncthreads();   // every count has landed; the previous result has been read
    uint4* h4 = reinterpret_cast<uint4*>(hist) + 2 * t;
    const uint4 a = h4[0], b = h4[1];
    const int c[8] = {(int)a.x, (int)a.y, (int)a.z, (int)a.w, (int)b.x, (int)b.y, (int)b.z, (int)b.w};
    int mine = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) mine += c[i];
    int s = mine;   // the sum over this lane and the higher lanes of the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_down(s, d, 64);
        if (lane + d < 64) s += o;
    }
    if (lane == 0) wsum[wv] = s;
    if (t == 0) found[0] = -1;
    if (CLEAR) {
        const uint4 z = {0u, 0u, 0u, 0u};
        h4[0] = z;
        h4[1] = z;
    }
    __syncthreads();
    int above = s - mine;
    for (int w = wv + 1; w < 4; ++w) above += wsum[w];
    if (above < need && need <= above + mine) {   // exactly one thread
        int bin = -1, ab = above, fa = 0, fc = 0;
#pragma unroll
        for (int i = 7; i >= 0; --i) {
            if (bin < 0 && ab + c[i] >= need) {
                bin = i;
                fa = ab;
                fc = c[i];
            }
            if (bin < 0) ab += c[i];
        }
        found[0] = 8 * t + bin;
        found[1] = fa;
        found[2] = fc;
    }
    __syncthreads();
}

// ================================================================================================
// the producer
// ================================================================================================
template <class Elem, bool WIDE>
__global__ __launch_bounds__(256) void lm_topk_kernel(const Elem* __restrict__ x, const float* __restrict__ weight,
                                                      float* __restrict__ out_logp, int* __restrict__ out_idx, long rows, int V,
                                                      int K, float inv_t) {
    using IO = ElemIO<Elem>;
    constexpr int W = WIDE ? IO::P : 1;
    __shared__ __attribute__((aligned(16))) unsigned hist[kBins];
    __shared__ u64 cand[kCand];
    __shared__ u64 sel[kMaxK];
    __shared__ float red[4][2];
    __shared__ int wsum[4], found[3], cnt[2];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int ngroups = V / W;   // WIDE: the pitch is a multiple of 16 bytes
    for (int i = tid; i < kBins; i += 256) hist[i] = 0u;
    for (long row = blockIdx.x; row < rows; row += gridDim.x) {
        float* olp = out_logp + (size_t)row * (size_t)K;
        int* oix = out_idx + (size_t)row * (size_t)K;
        if (weight && weight[row] == 0.f) {   // uniform over the workgroup: a dropped row is not read
            if (tid < K) {
                oix[tid] = -1;
                olp[tid] = -kInfG;
            }
            continue;
        }
        const Elem* p = x + (size_t)row * (size_t)V;
        __syncthreads();   // the previous row's selection has been written out
        if (tid == 0) cnt[0] = cnt[1] = 0;

        // ---- 1. the read from memory: the statistic and the histogram of the top 11 key bits
        RowStat<false> st{-kFltMaxG, 0.f};
        int floor_bin = 0;
        auto first = [&](const auto& xv, const auto& at) {
            constexpr int N = sizeof(xv) / sizeof(float);
            float a[N];
            float bm = -kFltMaxG;
#pragma unroll
            for (int i = 0; i < N; ++i) {
                a[i] = at[i / W] >= 0 ? clampf(xv[i] * inv_t) : -kFltMaxG;
                bm = fmaxf(bm, a[i]);
            }
            RowStat<false> n = stat_shift(st, fmaxf(st.m, bm));
#pragma unroll
            for (int i = 0; i < N; ++i) {
                const float e = ex2((a[i] - n.m) * kLog2eG);
                n.s += at[i / W] >= 0 ? e : 0.f;
                const int bin = (int)(order_key(xv[i]) >> 21);
                if (at[i / W] >= 0 && bin >= floor_bin) atomicAdd(&hist[bin], 1u);
            }
            st = n;
        };
        const int ghead = ngroups < kInFlight * 256 ? ngroups : kInFlight * 256;   // one batch a thread
        walk_row<Elem, WIDE, 256, true>(p, 0, ghead, tid, first);
        if (ghead < ngroups) {   // uniform
            pick_bin<false>(hist, wsum, found, K);
            floor_bin = found[0] < 0 ? 0 : found[0];
            walk_row<Elem, WIDE, 256, true>(p, ghead, ngroups, tid, first);
        }
        st = stat_wave(st);
        if (lane == 0) {
            red[wv][0] = st.m;
            red[wv][1] = st.s;
        }

        // ---- 2. / 3. the threshold bin, and further levels over the row while it does not fit the candidate buffer
        int need = K, sh = 21;
        pick_bin<true>(hist, wsum, found, need);   // (its first barrier publishes `red` as well)
        unsigned prefix = (unsigned)found[0] << 21;
        need -= found[1];
        int nb = found[2];
        while (nb > kCand && sh > 0) {   // uniform
            const int psh = sh;
            sh = sh == 21 ? 10 : 0;
            const unsigned mask = sh == 10 ? 2047u : 1023u;
            walk_row<Elem, WIDE, 256, true>(p, 0, ngroups, tid, [&](const auto& xv, const auto& at) {
                constexpr int N = sizeof(xv) / sizeof(float);
#pragma unroll
                for (int i = 0; i < N; ++i) {
                    const unsigned key = order_key(xv[i]);
                    if (at[i / W] >= 0 && (key >> psh) == (prefix >> psh)) atomicAdd(&hist[(key >> sh) & mask], 1u);
                }
            });
            pick_bin<true>(hist, wsum, found, need);
            prefix |= (unsigned)found[0] << sh;
            need -= found[1];
            nb = found[2];
        }
        const RowStat<false> all = stat_merge(stat_merge(RowStat<false>{red[0][0], red[0][1]}, RowStat<false>{red[1][0], red[1][1]}),
                                              stat_merge(RowStat<false>{red[2][0], red[2][1]}, RowStat<false>{red[3][0], red[3][1]}));

        // ---- 4. the collecting read: above the prefix -> selected, matching it -> candidates (unless all of them are equal)
        const bool tie = nb > kCand;   // then sh == 0: the prefix is the threshold key itself
        const unsigned kp = prefix >> sh;
        const int base = K - need;     // entries above the prefix
        walk_row<Elem, WIDE, 256, true>(p, 0, ngroups, tid, [&](const auto& xv, const auto& at) {
            constexpr int N = sizeof(xv) / sizeof(float);
#pragma unroll
            for (int i = 0; i < N; ++i) {
                const unsigned key = order_key(xv[i]);
                const unsigned kk = key >> sh;
                if (at[i / W] >= 0 && kk >= kp) {
                    const u64 w = sel_word(key, at[i / W] + i % W);
                    if (kk > kp) {
                        const int slot = atomicAdd(&cnt[0], 1);
                        if (slot < base) sel[slot] = w;
                    } else if (!tie) {
                        const int slot = atomicAdd(&cnt[1], 1);
                        if (slot < kCand) cand[slot] = w;
                    }
                }
            }
        });
        __syncthreads();
        if (!tie) {   // rank counting among the nb <= kCand candidates: the `need` largest words
            u64 mine[kCand / 256];
            int rk[kCand / 256];
#pragma unroll
            for (int r = 0; r < kCand / 256; ++r) {
                mine[r] = tid + 256 * r < nb ? cand[tid + 256 * r] : ~0ull;
                rk[r] = 0;
            }
            for (int j = 0; j < nb; ++j) {
                const u64 o = cand[j];
#pragma unroll
                for (int r = 0; r < kCand / 256; ++r) rk[r] += (int)(o > mine[r]);
            }
#pragma unroll
            for (int r = 0; r < kCand / 256; ++r)
                if (tid + 256 * r < nb && rk[r] < need) sel[base + rk[r]] = mine[r];
        } else {      // ---- 5. every match equals the key `prefix`: the lowest `need` indices, a span of the row a wave
            const int span = (V + 3) / 4, b = wv * span, e = b + span < V ? b + span : V;
            int c = 0;
            for (int i = b + lane; i < e; i += 64) c += (int)(order_key(IO::get(p + i)) == prefix);
            c = wave_sum_i(c);
            if (lane == 0) wsum[wv] = c;
            __syncthreads();
            int rank = 0;
            for (int w = 0; w < wv; ++w) rank += wsum[w];
            for (int i0 = b; i0 < e && rank < need; i0 += 64) {
                const int i = i0 + lane;
                const bool eq = i < e && order_key(IO::get(p + i)) == prefix;
                const u64 m = __ballot(eq);
                const int r = rank + __popcll(m & ((1ull << lane) - 1ull));
                if (eq && r < need) sel[base + r] = sel_word(prefix, i);
                rank += __popcll(m);
            }
        }
        __syncthreads();

        // ---- 6. order the K selected words, fetch their elements again and write
        const u64 me = tid < K ? sel[tid] : 0ull;
        int rk = 0;
        for (int j = 0; j < K; ++j) rk += (int)(sel[j] > me);
        if (tid < K) {
            const unsigned idx = ~(unsigned)me;
            float lp = -kInfG;
            int oi = -1;
            if (idx < (unsigned)V && rk < K) {
                const float raw = IO::get(p + idx);
                const float ls = __builtin_amdgcn_logf(all.s) * kLn2G;
                lp = raw > -kInfG ? (clampf(raw * inv_t) - all.m) - ls : -kInfG;   // NaN and -inf: masked entries
                oi = (int)idx;
            }
            if (rk < K) {
                oix[rk] = oi;
                olp[rk] = lp;
            }
        }
    }
}

// ================================================================================================
// the consumer: what its two kernels share
// ================================================================================================
template <int NT> __device__ __forceinline__ void row_sync() {   // between the owners of a row
    if (NT == 256) __syncthreads();
    else __builtin_amdgcn_wave_barrier();   // one wave: its LDS operations run in order
}
template <int NT> __device__ __forceinline__ bool row_any(bool v) {   // over the owners of a row; a row_sync as well
    if (NT == 256) return __syncthreads_or(v);
    const bool r = __ballot(v) != 0ull;
    __builtin_amdgcn_wave_barrier();
    return r;
}

struct TopkIn { const void* index; const float* logp; int idx64, K; };

// The owners of a row set the bits of its live entries and fill the table: tab_i the index (-1: padding, up to the next
// multiple of four), tab_v the teacher's log-probability.  Returns whether the row has a live entry.
template <int NT>
__device__ __forceinline__ bool table_build(const TopkIn& t, long row, int V, int tid, bool live, unsigned* bits, int* tab_i,
                                            float* tab_v) {
    bool mine = false;
    if (live) {
        const int kpad = (t.K + 3) & ~3;
        for (int j = tid; j < kpad; j += NT) {
            long idx = -1;
            float lp = -kInfG;
            if (j < t.K) {
                const size_t at = (size_t)row * (size_t)t.K + (size_t)j;
                idx = t.idx64 ? (long)static_cast<const int64_t*>(t.index)[at] : (long)static_cast<const int*>(t.index)[at];
                lp = t.logp[at];
            }
            const bool ok = idx >= 0 && idx < (long)V && lp > -kInfG;   // (a NaN log-probability is padding too)
            tab_i[j] = ok ? (int)idx : -1;
            tab_v[j] = lp;
            if (ok) atomicOr(&bits[idx >> 5], 1u << (idx & 31));
            mine = mine || ok;
        }
    }
    return row_any<NT>(mine);
}
// the words the row's entries set, back to zero
template <int NT> __device__ __forceinline__ void table_clear(int K, int tid, unsigned* bits, const int* tab_i) {
    for (int j = tid; j < K; j += NT)
        if (tab_i[j] >= 0) bits[tab_i[j] >> 5] = 0u;
}
// the slot of index `idx` in the table (the last one when the caller passed duplicates), -1 when absent
__device__ __forceinline__ int find_slot(const int* tab_i, int K, int idx) {
    int slot = -1;
    for (int j = 0; j < K; j += 4) {
        const int4 t = *reinterpret_cast<const int4*>(tab_i + j);
        slot = t.x == idx ? j : slot;
        slot = t.y == idx ? j + 1 : slot;
        slot = t.z == idx ? j + 2 : slot;
        slot = t.w == idx ? j + 3 : slot;
    }
    return slot;
}
// the W bits of the group that starts at element `at` (a multiple of W, W divides 32)
template <int W> __device__ __forceinline__ unsigned group_bits(const unsigned* bits, int at) {
    return at >= 0 ? (bits[at >> 5] >> (at & 31)) & ((1u << W) - 1u) : 0u;
}

struct InOut { float m, si, so; };   // the maximum and the sums e^(a - m) inside and outside the teacher's set
__device__ __forceinline__ InOut io_merge(const InOut& a, const InOut& b) {
    const float m = fmaxf(a.m, b.m);
    const float ea = ex2((a.m - m) * kLog2eG), eb = ex2((b.m - m) * kLog2eG);
    return InOut{m, a.si * ea + b.si * eb, a.so * ea + b.so * eb};
}

struct TopkKlOut { float *kl, *lse, *c0, *c1; };

// ================================================================================================
// the consumer's forward.  Dynamic LDS: the bitmap, (V + 31) / 32 words for NT = 256, 4 x 64 for NT = 64.
// Saved per row: lse and two coefficients -- renorm: c0 = S / Q (the factor of p everywhere), c1 = 1 / Q (the factor of q);
// bucket: c0 = S - r P (the factor of p outside the set), c1 = S + (1 - Q) (inside it).  S = sum q, Q = min(S, 1).
// ================================================================================================
template <class Elem, bool WIDE, int NT>
__global__ __launch_bounds__(256) void lm_topk_kl_kernel(const Elem* __restrict__ x, const TopkIn t,
                                                         const float* __restrict__ weight, const TopkKlOut out, long rows, int V,
                                                         int tail, float inv_t, int bit_words) {
    using IO = ElemIO<Elem>;
    constexpr int RPW = 256 / NT, W = WIDE ? IO::P : 1;
    extern __shared__ unsigned bits_all[];
    __shared__ __attribute__((aligned(16))) int tab_i_all[RPW][kMaxK];
    __shared__ float tab_v_all[RPW][kMaxK], tab_a_all[RPW][kMaxK];
    __shared__ float red[4][3];
    const int tid = threadIdx.x % NT, sub = threadIdx.x / NT;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    unsigned* bits = bits_all + (NT == 256 ? 0 : sub * 64);
    int* tab_i = tab_i_all[sub];
    float *tab_v = tab_v_all[sub], *tab_a = tab_a_all[sub];
    for (int i = threadIdx.x; i < bit_words; i += 256) bits_all[i] = 0u;
    __syncthreads();
    const int ngroups = V / W;
    for (long r0 = (long)blockIdx.x * RPW; r0 < rows; r0 += (long)gridDim.x * RPW) {
        const long row = r0 + sub;
        const bool have = row < rows;
        const bool live = have && (weight ? weight[row] != 0.f : true);   // the same for all NT threads of the row
        row_sync<NT>();   // the previous row's sums and clearing are done
        const bool any = table_build<NT>(t, row, V, tid, live, bits, tab_i, tab_v);
        InOut st{-kFltMaxG, 0.f, 0.f};
        if (any) {   // a row without a live entry is not read
            const Elem* p = x + (size_t)row * (size_t)V;
            walk_row<Elem, WIDE, NT, false>(p, 0, ngroups, tid, [&](const auto& xv, const auto& at) {
                constexpr int N = sizeof(xv) / sizeof(float);
                float a[N];
                unsigned mk[kInFlight];
                float bm = -kFltMaxG;
#pragma unroll
                for (int k = 0; k < kInFlight; ++k) mk[k] = group_bits<W>(bits, at[k]);
#pragma unroll
                for (int i = 0; i < N; ++i) {
                    a[i] = at[i / W] >= 0 ? clampf(xv[i] * inv_t) : -kFltMaxG;
                    bm = fmaxf(bm, a[i]);
                }
                const float m = fmaxf(st.m, bm), e0 = ex2((st.m - m) * kLog2eG);
                float si = st.si * e0, so = st.so * e0;
#pragma unroll
                for (int i = 0; i < N; ++i) {
                    const float e = at[i / W] >= 0 ? ex2((a[i] - m) * kLog2eG) : 0.f;
                    const bool in = (mk[i / W] >> (i % W)) & 1u;
                    si += in ? e : 0.f;
                    so += in ? 0.f : e;
                }
                st = InOut{m, si, so};
#pragma unroll
                for (int k = 0; k < kInFlight; ++k)
                    if (mk[k] != 0u) {   // rare: the chosen logits go to their slots
#pragma unroll
                        for (int j = 0; j < W; ++j)
                            if ((mk[k] >> j) & 1u) {
                                const int slot = find_slot(tab_i, t.K, at[k] + j);
                                if (slot >= 0) tab_a[slot] = a[k * W + j];
                            }
                    }
            });
#pragma unroll
            for (int k = 32; k >= 1; k >>= 1)
                st = io_merge(st, InOut{__shfl_xor(st.m, k, 64), __shfl_xor(st.si, k, 64), __shfl_xor(st.so, k, 64)});
            if (NT == 256 && lane == 0) {
                red[wv][0] = st.m;
                red[wv][1] = st.si;
                red[wv][2] = st.so;
            }
        }
        row_sync<NT>();   // the slots and, for a workgroup per row, the waves' statistics are written
        float val = 0.f, vlse = 0.f, c0 = 0.f, c1 = 0.f;
        if (any && (NT == 64 || wv == 0)) {   // one wave sums the K entries, four a lane, in a fixed order
            if (NT == 256)
                st = io_merge(io_merge(InOut{red[0][0], red[0][1], red[0][2]}, InOut{red[1][0], red[1][1], red[1][2]}),
                              io_merge(InOut{red[2][0], red[2][1], red[2][2]}, InOut{red[3][0], red[3][1], red[3][2]}));
            const float tot = st.si + st.so;                          // in [1, V]: the bare log2
            const float lns = __builtin_amdgcn_logf(tot) * kLn2G;
            float S = 0.f, U = 0.f;   // sum q and sum q (log q - log p), log p = (a - m) - ln tot
            for (int j = lane; j < t.K; j += 64)
                if (tab_i[j] >= 0) {
                    const float lp = tab_v[j], q = ex2(lp * kLog2eG);
                    S += q;
                    U = fmaf(q, lp - ((tab_a[j] - st.m) - lns), U);
                }
            S = wave_sum(S);
            U = wave_sum(U);
            vlse = st.m + lns;
            if (S > 0.f) {   // (every q underflowed: the row counts as one without entries)
                const float Q = fminf(S, 1.f);
                if (tail == kRenorm) {
                    c0 = S / Q;
                    c1 = 1.f / Q;
                    val = U / Q - c0 * (__builtin_amdgcn_logf(Q) * kLn2G);
                } else {
                    const float omq = 1.f - Q;
                    const bool rest = omq > 0.f && st.so > 0.f;   // the "everything else" outcome has mass on both sides
                    const float r = rest ? omq / (st.so / tot) : 0.f;
                    val = U + (rest ? omq * ((__builtin_amdgcn_logf(omq) - (__builtin_amdgcn_logf(st.so) - __builtin_amdgcn_logf(tot))) * kLn2G) : 0.f);
                    c0 = S - r * (st.si / tot);
                    c1 = S + (rest ? omq : 0.f);
                }
            }
        }
        if (have && lane == 0 && (NT == 64 || wv == 0)) {
            out.kl[row] = val;
            out.lse[row] = vlse;
            out.c0[row] = c0;
            out.c1[row] = c1;
        }
        if (any) table_clear<NT>(t.K, tid, bits, tab_i);
    }
}

// ================================================================================================
// the consumer's gradient: grad[r, v] = c (c0 p_v) outside the set, c (A' p_v - s q_v) inside, c = g[r] / T;
// renorm: A' = c0, s = c1; bucket: A' = c1, s = 1.  A row with weight == 0, c == 0 or no live entry is zero-filled unread.
// ================================================================================================
struct TopkSaved { const float *g, *weight, *lse, *c0, *c1; };

template <class Elem, bool WIDE, int NT>
__global__ __launch_bounds__(256) void lm_topk_kl_grad_kernel(const Elem* __restrict__ x, const TopkIn t, const TopkSaved s,
                                                              Elem* __restrict__ grad, long rows, int V, int tail, float inv_t,
                                                              int bit_words) {
    using IO = ElemIO<Elem>;
    constexpr int RPW = 256 / NT, W = WIDE ? IO::P : 1;
    extern __shared__ unsigned bits_all[];
    __shared__ __attribute__((aligned(16))) int tab_i_all[RPW][kMaxK];
    __shared__ float tab_v_all[RPW][kMaxK];
    const int tid = threadIdx.x % NT, sub = threadIdx.x / NT;
    unsigned* bits = bits_all + (NT == 256 ? 0 : sub * 64);
    int* tab_i = tab_i_all[sub];
    float* tab_v = tab_v_all[sub];
    for (int i = threadIdx.x; i < bit_words; i += 256) bits_all[i] = 0u;
    __syncthreads();
    const int ngroups = V / W;
    for (long r0 = (long)blockIdx.x * RPW; r0 < rows; r0 += (long)gridDim.x * RPW) {
        const long row = r0 + sub;
        const bool have = row < rows;
        const bool live = have && (s.weight ? s.weight[row] != 0.f : true);
        const float c = live ? s.g[row] * inv_t : 0.f;
        row_sync<NT>();   // the previous row's clearing is done
        const bool any = table_build<NT>(t, row, V, tid, live && c != 0.f, bits, tab_i, tab_v);   // NaN != 0: it reaches its row
        if (any) {
            const float lse = s.lse[row], c0 = s.c0[row], c1 = s.c1[row];
            const float a_out = c * c0, a_in = c * (tail == kRenorm ? c0 : c1), qs = c * (tail == kRenorm ? c1 : 1.f);
            for (int j = tid; j < t.K; j += NT) tab_v[j] = qs * ex2(tab_v[j] * kLog2eG);   // each owner its own slots
            row_sync<NT>();
            const Elem* p = x + (size_t)row * (size_t)V;
            Elem* o = grad + (size_t)row * (size_t)V;
            walk_row<Elem, WIDE, NT, false>(p, 0, ngroups, tid, [&](const auto& xv, const auto& at) {
                constexpr int N = sizeof(xv) / sizeof(float);
                float d[N];
#pragma unroll
                for (int k = 0; k < kInFlight; ++k) {
                    const unsigned mk = group_bits<W>(bits, at[k]);
#pragma unroll
                    for (int j = 0; j < W; ++j) {
                        const float pe = ex2((clampf(xv[k * W + j] * inv_t) - lse) * kLog2eG);
                        d[k * W + j] = a_out * pe;
                        if ((mk >> j) & 1u) {   // rare
                            const int slot = find_slot(tab_i, t.K, at[k] + j);
                            if (slot >= 0) d[k * W + j] = a_in * pe - tab_v[slot];
                        }
                    }
                    if (at[k] >= 0) {   // every element of the row is written here, once
                        if constexpr (WIDE) __builtin_nontemporal_store(IO::pack(d + k * W), reinterpret_cast<vuint4*>(o) + at[k] / W);
                        else IO::put(o + at[k], d[k]);
                    }
                }
            });
            row_sync<NT>();   // every owner has read the bitmap
            table_clear<NT>(t.K, tid, bits, tab_i);
        } else if (have) {
            zero_row<Elem, WIDE, NT>(grad + (size_t)row * (size_t)V, V, tid);
        }
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------
int bitmap_words(const RowLaunch& L, int V) { return L.nt == 256 ? (V + 31) / 32 : L.rpw * 64; }

bool topk_scalars_ok(int k, float inv_t) { return k >= 1 && k <= kMaxK && inv_t > 0.f && inv_t <= kFltMaxG; }
bool tail_ok(int tail) { return tail == kRenorm || tail == kBucket; }

}  // namespace
}  // namespace hpc_rll

using namespace hpc_rll;

extern "C" int hpc_rll_lm_topk_forward(const void* logits, int elem, const float* weight, float* topk_logp, int* topk_index,
                                       int64_t rows, int V, int k, float inv_temperature, void* stream) {
    if (!topk_scalars_ok(k, inv_temperature)) return HPC_RLL_EINVAL;
    if (rows != 0 && (!logits || !topk_logp || !topk_index)) return HPC_RLL_EINVAL;
    if (const int bad = lm_shape_status(rows, 1, V, elem, aligned(logits, elem_size(elem)) && aligned(weight, 4) &&
                                        aligned(topk_logp, 4) && aligned(topk_index, 4)))
        return bad;
    if (V < 1 || k > V) return HPC_RLL_EINVAL;
    if (rows == 0) return HPC_RLL_OK;
    return with_elem(elem, [&](auto e) {
        using Elem = decltype(e);
        const Elem* x = static_cast<const Elem*>(logits);
        RowLaunch L = row_launch<Elem>(x, nullptr, (long)rows, V);
        L.grid = rows > kRowGridMax ? kRowGridMax : (long)rows;   // a workgroup per row at every V
        auto launch = [&](auto W) {
            hipLaunchKernelGGL((lm_topk_kernel<Elem, decltype(W)::value>), dim3((unsigned)L.grid), dim3(256), 0, (hipStream_t)stream, x,
                               weight, topk_logp, topk_index, (long)rows, V, k, inv_temperature);
        };
        if (L.wide) launch(std::true_type{});
        else launch(std::false_type{});
        const int rc = last_error();
        if (!rc) g_topk_sel.note({ElemIO<Elem>::kCode, L.wide ? 16 : (int)sizeof(Elem), 256, 1, (int)L.grid, k});
        return rc;
    });
}

extern "C" int hpc_rll_lm_topk_kl_forward(const void* logits, int elem, const void* topk_index, int index64,
                                          const float* topk_logp, const float* weight, float* kl, float* lse, float* c0, float* c1,
                                          int64_t rows, int V, int k, int tail, float inv_temperature, void* stream) {
    if (!topk_scalars_ok(k, inv_temperature) || !tail_ok(tail) || (index64 != 0 && index64 != 1)) return HPC_RLL_EINVAL;
    if (rows != 0 && (!logits || !topk_index || !topk_logp || !kl || !lse || !c0 || !c1)) return HPC_RLL_EINVAL;
    if (const int bad = lm_shape_status(rows, 1, V, elem, aligned(logits, elem_size(elem)) && aligned(topk_index, index64 ? 8 : 4) &&
                                        aligned(topk_logp, 4) && aligned(weight, 4) && aligned(kl, 4) && aligned(lse, 4) &&
                                        aligned(c0, 4) && aligned(c1, 4)))
        return bad;
    if (V < 1) return HPC_RLL_EINVAL;
    if (rows == 0) return HPC_RLL_OK;
    return with_elem(elem, [&](auto e) {
        using Elem = decltype(e);
        const Elem* x = static_cast<const Elem*>(logits);
        const RowLaunch L = row_launch<Elem>(x, nullptr, (long)rows, V);
        const int words = bitmap_words(L, V);
        with_row_kernel(L, [&](auto W, auto NT) {
            hipLaunchKernelGGL((lm_topk_kl_kernel<Elem, decltype(W)::value, decltype(NT)::value>), dim3((unsigned)L.grid), dim3(256),
                               (size_t)words * 4, (hipStream_t)stream, x, TopkIn{topk_index, topk_logp, index64, k}, weight,
                               TopkKlOut{kl, lse, c0, c1}, (long)rows, V, tail, inv_temperature, words);
        });
        const int rc = last_error();
        if (!rc) g_topk_kl.note({ElemIO<Elem>::kCode, L.wide ? 16 : (int)sizeof(Elem), L.nt, L.rpw, (int)L.grid, k});
        return rc;
    });
}

extern "C" int hpc_rll_lm_topk_kl_backward(const float* g, const void* logits, int elem, const void* topk_index, int index64,
                                           const float* topk_logp, const float* weight, const float* lse, const float* c0,
                                           const float* c1, void* grad_logits, int64_t rows, int V, int k, int tail,
                                           float inv_temperature, void* stream) {
    if (!topk_scalars_ok(k, inv_temperature) || !tail_ok(tail) || (index64 != 0 && index64 != 1)) return HPC_RLL_EINVAL;
    if (rows != 0 && (!g || !logits || !topk_index || !topk_logp || !lse || !c0 || !c1 || !grad_logits)) return HPC_RLL_EINVAL;
    if (const int bad = lm_shape_status(rows, 1, V, elem, aligned(logits, elem_size(elem)) && aligned(grad_logits, elem_size(elem)) &&
                                        aligned(topk_index, index64 ? 8 : 4) && aligned(topk_logp, 4) && aligned(g, 4) &&
                                        aligned(weight, 4) && aligned(lse, 4) && aligned(c0, 4) && aligned(c1, 4)))
        return bad;
    if (V < 1) return HPC_RLL_EINVAL;
    if (rows == 0) return HPC_RLL_OK;
    return with_elem(elem, [&](auto e) {
        using Elem = decltype(e);
        const Elem* x = static_cast<const Elem*>(logits);
        Elem* grad = static_cast<Elem*>(grad_logits);
        const RowLaunch L = row_launch<Elem>(x, grad, (long)rows, V);
        const int words = bitmap_words(L, V);
        with_row_kernel(L, [&](auto W, auto NT) {
            hipLaunchKernelGGL((lm_topk_kl_grad_kernel<Elem, decltype(W)::value, decltype(NT)::value>), dim3((unsigned)L.grid), dim3(256),
                               (size_t)words * 4, (hipStream_t)stream, x, TopkIn{topk_index, topk_logp, index64, k},
                               TopkSaved{g, weight, lse, c0, c1}, grad, (long)rows, V, tail, inv_temperature, words);
        });
        const int rc = last_error();
        if (!rc) g_topk_grad.note({ElemIO<Elem>::kCode, L.wide ? 16 : (int)sizeof(Elem), L.nt, L.rpw, (int)L.grid, k});
        return rc;
    });
}

extern "C" int hpc_rll_lm_topk_last_config(int* out) {
    if (!out) return HPC_RLL_EINVAL;
    g_topk_sel.read(out);
    g_topk_kl.read(out + kTopkInts);
    g_topk_grad.read(out + 2 * kTopkInts);
    return HPC_RLL_OK;
}
static_assert(HPC_RLL_LM_TOPK_CONFIG_INTS == 3 * kTopkInts, "the layout documented in hpc_rll_hip.h");
