// lm_policy.hip -- the policy losses of language-model RL (PPO, DAPO's asymmetric clip, GSPO's sequence ratio, CISPO, Dr. GRPO's
// constant normaliser, the k1 / k2 / k3 estimators of the reference KL) on per-token LOG-PROBABILITIES (B,S), the output of the
// fused head (lm_linear.hip), with value loss and entropy.  No vocabulary axis, no reference counterpart; hpc_rll_hip.h has the
// formulas.
//
// Kernels:
//   * lm_policy_stats_kernel<WIDE>: chunk mapping only, and only when something per-sequence is needed.  A 256-thread workgroup
//     owns one (sequence, chunk of kChunk = 1024 tokens), a thread 4 consecutive tokens; it leaves (sum w, sum w d) of the chunk in
//     the workspace: thread sums -> butterfly -> (r0 + r1) + (r2 + r3) over the waves.
//   * lm_policy_chunk_kernel<WIDE>: the same mapping.  All operands of the thread's four tokens are requested first; then EVERY
//     wave sums the sequence's chunk partials itself, strided lanes then a butterfly: the same additions in the same order in
//     every wave of every workgroup of the sequence, so all of them hold bit-identical W_b and s_b without LDS, a barrier, an
//     atomic or a grid-wide wait.  Then the per-token terms, the saved coefficients, and eight sums per thread.
//   * lm_policy_wave_kernel<WIDE>: short sequences, a wave per sequence, four sequences per workgroup, both phases in one launch;
//     a lane owns 4 consecutive tokens of every 256, which stay in registers between the phases for S <= 256 and are read again
//     above that.
//   * lm_policy_final_kernel: 'token' aggregation divides by sum w on the device.
//   * lm_policy_grad_kernel<WIDE>: one streaming launch over (B,S), coefficient x upstream scalar read on the device.
// The eight sums leave through publish_block_sums (colscan.hpp): wave butterflies, (r0 + r1) + (r2 + r3), partials per workgroup
// added by the last workgroup in a fixed order.  No float atomics: two runs give the same bits.
#include <hip/hip_runtime.h>

#include <cmath>

#include "colscan.hpp"
#include "hostutil.hpp"
#include "hpc_rll_hip.h"
#include "wave.hpp"

namespace hpc_rll {
namespace {

constexpr int kPolSums = 8;      // policy, kl, value, entropy, approx_kl, ratio, clipfrac numerators, sum w
constexpr int kChunk = 1024;     // tokens of a (sequence, chunk): 256 threads x 4 tokens
constexpr int kWaveStep = 256;   // tokens a wave takes per step: 64 lanes x 4 tokens
// Sequences up to this length take the wave mapping when the caller leaves the choice to the rule.  NOT MEASURED: the value is
// lm_ppo_token_kernel's comfort zone (at most four steps of a wave), nothing more; DESIGN.md 4.2.16.
constexpr int kWaveSeqMax = 1024;
constexpr long kPolWsHead = 8 + 8 * (kFoldMaxGrid + 1);   // the sums, then the partials of the fold

constexpr int kFwdInts = 7, kBwdInts = 3;
LaunchRecord<kFwdInts> g_pol_fwd;
LaunchRecord<kBwdInts> g_pol_bwd;

struct PolArgs {
    const float *pn, *po, *adv, *w, *pr, *ent, *vn, *vo, *ret;
    float *cp, *ck, *ce, *cv;
    int B, S, nchunk, adv_seq, ratio_seq, cispo, kl, agg, use_vclip, need_seq;
    float lo, hi, dual, vclip, scale;
};

// four consecutive tokens of one operand: one 16-byte access (WIDE: every base and S are multiples of 16 bytes, so a thread's
// four tokens are inside the sequence together), or single elements, zeros past the end.  An absent operand reads as zeros.
template <bool WIDE> __device__ __forceinline__ void load4(const float* __restrict__ p, size_t base, int s, int S, float (&v)[4]) {
    if (WIDE) {
        const Pack<4> t = (p && s < S) ? load_pack<4>(p + base + s) : Pack<4>{{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = t.v[j];
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (p && s + j < S) ? p[base + s + j] : 0.f;
    }
}
template <bool WIDE> __device__ __forceinline__ void store4(float* __restrict__ p, size_t base, int s, int S, const float (&v)[4]) {
    if (!p) return;
    if (WIDE) {
        if (s < S) store_pack<4>(p + base + s, Pack<4>{{v[0], v[1], v[2], v[3]}});
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (s + j < S) p[base + s + j] = v[j];
    }
}
// the weight: absent = ones inside the sequence; always 0 past its end
template <bool WIDE> __device__ __forceinline__ void load_w(const float* __restrict__ w, size_t base, int s, int S, float (&v)[4]) {
    if (w) {
        load4<WIDE>(w, base, s, S, v);
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = s + j < S ? 1.f : 0.f;
}

struct Tok4 { float pn[4], po[4], A[4], w[4], pr[4], H[4], vn[4], vo[4], ret[4]; };

// what the per-sequence pass needs of a thread's tokens: (sum w, sum w d) over the live ones, by selection
__device__ __forceinline__ void stat4(const float (&w)[4], const float (&pn)[4], const float (&po)[4], bool with_d, float& a,
                                      float& d) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool live = w[j] != 0.f;
        a += live ? w[j] : 0.f;
        if (with_d) d = live ? fmaf(w[j], pn[j] - po[j], d) : d;
    }
}

template <bool WIDE> __device__ __forceinline__ void load_rest(const PolArgs& p, int b, size_t base, int s, Tok4& t) {
    if (p.adv_seq) {
        const float a = p.adv[b];
#pragma unroll
        for (int j = 0; j < 4; ++j) t.A[j] = a;
    } else {
        load4<WIDE>(p.adv, base, s, p.S, t.A);
    }
    load4<WIDE>(p.pr, base, s, p.S, t.pr);
    load4<WIDE>(p.ent, base, s, p.S, t.H);
    load4<WIDE>(p.vn, base, s, p.S, t.vn);
    load4<WIDE>(p.vo, base, s, p.S, t.vo);
    load4<WIDE>(p.ret, base, s, p.S, t.ret);
}
template <bool WIDE> __device__ __forceinline__ void load_stat(const PolArgs& p, size_t base, int s, Tok4& t) {
    load_w<WIDE>(p.w, base, s, p.S, t.w);
    load4<WIDE>(p.pn, base, s, p.S, t.pn);
    load4<WIDE>(p.po, base, s, p.S, t.po);
}

// The terms of a thread's four tokens of sequence b: adds the sequence's share into acc[8], stores the coefficients.
// Wb, D: the sequence's sum w and sum w d (used only with need_seq).
template <bool WIDE>
__device__ __forceinline__ void token_terms(const PolArgs& p, const Tok4& t, size_t base, int s, float Wb, float D,
                                            float (&acc)[kPolSums]) {
    const bool seq_agg = p.agg == HPC_RLL_POLICY_AGG_SEQUENCE;
    const float inv = seq_agg ? (Wb != 0.f ? 1.f / Wb : 0.f) : 1.f;
    const float cs = seq_agg ? p.scale * inv : (p.agg == HPC_RLL_POLICY_AGG_CONSTANT ? p.scale : 1.f);
    const float lr_seq = (p.ratio_seq && Wb != 0.f) ? D / Wb : 0.f;
    const bool dual_on = p.dual > 1.f;
    float sm[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, sw = 0.f;
    float cp[4], ck[4], ce[4], cv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool live = t.w[j] != 0.f;                    // a dropped token: selected away, whatever its values are
        const float w = live ? t.w[j] : 0.f;
        const float pn = live ? t.pn[j] : 0.f, po = live ? t.po[j] : 0.f, A = live ? t.A[j] : 0.f;
        const float d = pn - po;
        const float lr = p.ratio_seq ? lr_seq : d;
        const float r = expf(lr);
        const float rc = fminf(fmaxf(r, p.lo), p.hi);
        float l, dl;
        if (p.cispo) {                                      // the clipped weight is detached: it multiplies logp
            dl = -rc * A;
            l = dl * pn;
        } else {
            const float t1 = -A * r, t2 = -A * rc;
            l = t2 > t1 ? t2 : t1;
            dl = t2 > t1 ? 0.f : t1;                        // a tie counts as unclipped
            if (dual_on && A < 0.f) {
                const float t3 = -p.dual * A;
                if (t3 < l) {
                    l = t3;
                    dl = 0.f;
                }
            }
        }
        const float wc = w * cs;
        sm[0] = fmaf(w, l, sm[0]);
        sm[4] = fmaf(w, expm1f(lr) - lr, sm[4]);
        sm[5] = fmaf(w, r, sm[5]);
        sm[6] = fmaf(w, (r > p.hi || r < p.lo) ? 1.f : 0.f, sm[6]);
        sw += w;
        cp[j] = live ? wc * dl : 0.f;
        ce[j] = live ? wc : 0.f;
        ck[j] = 0.f;
        cv[j] = 0.f;
        if (p.pr) {
            const float e = live ? t.pr[j] - pn : 0.f;
            float k, dk;
            if (p.kl == HPC_RLL_POLICY_KL_K1) {
                k = -e;
                dk = 1.f;
            } else if (p.kl == HPC_RLL_POLICY_KL_K2) {
                k = 0.5f * e * e;
                dk = -e;
            } else {
                const float em = expm1f(e);
                k = em - e;
                dk = -em;
            }
            sm[1] = fmaf(w, k, sm[1]);
            ck[j] = live ? wc * dk : 0.f;
        }
        if (p.ent) sm[3] = fmaf(w, live ? t.H[j] : 0.f, sm[3]);
        if (p.vn) {
            const float v = live ? t.vn[j] : 0.f, vo = live ? t.vo[j] : 0.f, rt = live ? t.ret[j] : 0.f;
            const float e1 = v - rt;
            float lv = e1 * e1, dv = e1;
            if (p.use_vclip) {
                const float dd = v - vo;
                const bool out = dd > p.vclip || dd < -p.vclip;
                const float e2 = vo + fminf(fmaxf(dd, -p.vclip), p.vclip) - rt;
                if (out && e2 * e2 > lv) {                  // the clipped branch: no gradient
                    lv = e2 * e2;
                    dv = 0.f;
                }
            }
            sm[2] = fmaf(w, 0.5f * lv, sm[2]);
            cv[j] = live ? wc * dv : 0.f;
        }
    }
#pragma unroll
    for (int k = 0; k < 7; ++k) acc[k] = fmaf(sm[k], inv, acc[k]);
    acc[7] += sw;
    store4<WIDE>(p.cp, base, s, p.S, cp);
    store4<WIDE>(p.ck, base, s, p.S, ck);
    store4<WIDE>(p.ce, base, s, p.S, ce);
    store4<WIDE>(p.cv, base, s, p.S, cv);
}

// ================================================================================================ chunk mapping
template <bool WIDE>
__global__ __launch_bounds__(256) void lm_policy_stats_kernel(const PolArgs p, float* __restrict__ stats) {
    __shared__ float red[4][2];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long pairs = (long)p.B * p.nchunk;
    for (long q = blockIdx.x; q < pairs; q += gridDim.x) {
        const int b = (int)(q / p.nchunk), c = (int)(q - (long)b * p.nchunk);
        const size_t base = (size_t)b * (size_t)p.S;
        const int s = c * kChunk + (int)threadIdx.x * 4;
        float w[4], pn[4] = {0.f, 0.f, 0.f, 0.f}, po[4] = {0.f, 0.f, 0.f, 0.f};
        load_w<WIDE>(p.w, base, s, p.S, w);
        if (p.ratio_seq) {
            load4<WIDE>(p.pn, base, s, p.S, pn);
            load4<WIDE>(p.po, base, s, p.S, po);
        }
        float a = 0.f, d = 0.f;
        stat4(w, pn, po, p.ratio_seq != 0, a, d);
        a = wave_sum(a);
        d = wave_sum(d);
        if (lane == 0) {
            red[wv][0] = a;
            red[wv][1] = d;
        }
        __syncthreads();
        if (threadIdx.x < 2) stats[2 * q + threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
        __syncthreads();   // red is rewritten by the next pair
    }
}

template <bool WIDE>
__global__ __launch_bounds__(256) void lm_policy_chunk_kernel(const PolArgs p, const float* __restrict__ stats,
                                                              float* __restrict__ partials, const ScanFold fold) {
    const int lane = threadIdx.x & 63;
    float acc[kPolSums];
#pragma unroll
    for (int k = 0; k < kPolSums; ++k) acc[k] = 0.f;
    const long pairs = (long)p.B * p.nchunk;
    for (long q = blockIdx.x; q < pairs; q += gridDim.x) {
        const int b = (int)(q / p.nchunk), c = (int)(q - (long)b * p.nchunk);
        const size_t base = (size_t)b * (size_t)p.S;
        const int s = c * kChunk + (int)threadIdx.x * 4;
        Tok4 t;
        load_stat<WIDE>(p, base, s, t);
        load_rest<WIDE>(p, b, base, s, t);
        float Wb = 0.f, D = 0.f;
        if (p.need_seq) {   // every wave: lane i adds partials i, i + 64, ... in turn, then the butterfly
            const float* st = stats + 2 * (size_t)b * (size_t)p.nchunk;
            for (int i = lane; i < p.nchunk; i += 64) {
                Wb += st[2 * i];
                D += st[2 * i + 1];
            }
            Wb = wave_sum(Wb);
            D = wave_sum(D);
        }
        token_terms<WIDE>(p, t, base, s, Wb, D, acc);
    }
    publish_block_sums<kPolSums, 256>(acc, partials, fold);
}

// ================================================================================================ wave mapping
template <bool WIDE>
__global__ __launch_bounds__(256) void lm_policy_wave_kernel(const PolArgs p, float* __restrict__ partials, const ScanFold fold) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float acc[kPolSums];
#pragma unroll
    for (int k = 0; k < kPolSums; ++k) acc[k] = 0.f;
    const int steps = (p.S + kWaveStep - 1) / kWaveStep;
    for (long b = (long)blockIdx.x * 4 + wv; b < (long)p.B; b += (long)gridDim.x * 4) {
        const size_t base = (size_t)b * (size_t)p.S;
        Tok4 t;
        float Wb = 0.f, D = 0.f;
        if (p.need_seq) {
            for (int k = 0; k < steps; ++k) {
                const int s = k * kWaveStep + lane * 4;
                if (steps == 1 || p.ratio_seq) load_stat<WIDE>(p, base, s, t);
                else load_w<WIDE>(p.w, base, s, p.S, t.w);
                stat4(t.w, t.pn, t.po, p.ratio_seq != 0, Wb, D);
            }
            Wb = wave_sum(Wb);
            D = wave_sum(D);
        }
        const bool kept = p.need_seq && steps == 1;   // the sequence is in registers: one read serves both phases
        for (int k = 0; k < steps; ++k) {
            const int s = k * kWaveStep + lane * 4;
            if (!kept) load_stat<WIDE>(p, base, s, t);
            load_rest<WIDE>(p, (int)b, base, s, t);
            token_terms<WIDE>(p, t, base, s, Wb, D, acc);
        }
    }
    publish_block_sums<kPolSums, 256>(acc, partials, fold);
}

// 'token' aggregation: the seven numerators over sum w (0 when nothing has weight); out8[7] = sum w
__global__ __launch_bounds__(64) void lm_policy_final_kernel(const float* __restrict__ sums, float* __restrict__ out8) {
    const int k = threadIdx.x;
    if (k >= 8) return;
    const float den = sums[7];
    out8[k] = k == 7 ? den : (den != 0.f ? sums[k] / den : 0.f);
}

// ================================================================================================ backward
struct PolGradArgs {
    const float *gp, *gk, *gv, *ge, *den, *cp, *ck, *ce, *cv;
    float *dlogp, *dent, *dval;
    long n;
};

__device__ __forceinline__ float scaled(float c, float u) { return c == 0.f ? 0.f : c * u; }   // a dropped token: exactly 0

template <bool WIDE>
__global__ __launch_bounds__(256) void lm_policy_grad_kernel(const PolGradArgs q) {
    float up = q.gp ? q.gp[0] : 0.f, uk = q.gk ? q.gk[0] : 0.f, uv = q.gv ? q.gv[0] : 0.f, ue = q.ge ? q.ge[0] : 0.f;
    if (q.den) {
        const float d = q.den[0];
        const float inv = d != 0.f ? 1.f / d : 0.f;
        up = d != 0.f ? up * inv : 0.f;
        uk = d != 0.f ? uk * inv : 0.f;
        uv = d != 0.f ? uv * inv : 0.f;
        ue = d != 0.f ? ue * inv : 0.f;
    }
    for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4; i < q.n; i += (long)gridDim.x * 1024) {
        if (WIDE && i + 4 <= q.n) {
            if (q.dlogp) {
                const Pack<4> a = load_pack<4>(q.cp + i);
                Pack<4> o;
#pragma unroll
                for (int j = 0; j < 4; ++j) o.v[j] = scaled(a.v[j], up);
                if (q.ck) {
                    const Pack<4> k = load_pack<4>(q.ck + i);
#pragma unroll
                    for (int j = 0; j < 4; ++j) o.v[j] += scaled(k.v[j], uk);
                }
                store_pack<4, true>(q.dlogp + i, o);
            }
            if (q.dent) {
                Pack<4> o = load_pack<4>(q.ce + i);
#pragma unroll
                for (int j = 0; j < 4; ++j) o.v[j] = scaled(o.v[j], ue);
                store_pack<4, true>(q.dent + i, o);
            }
            if (q.dval) {
                Pack<4> o = load_pack<4>(q.cv + i);
#pragma unroll
                for (int j = 0; j < 4; ++j) o.v[j] = scaled(o.v[j], uv);
                store_pack<4, true>(q.dval + i, o);
            }
            continue;
        }
        for (long e = i; e < i + 4 && e < q.n; ++e) {
            if (q.dlogp) q.dlogp[e] = scaled(q.cp[e], up) + (q.ck ? scaled(q.ck[e], uk) : 0.f);
            if (q.dent) q.dent[e] = scaled(q.ce[e], ue);
            if (q.dval) q.dval[e] = scaled(q.cv[e], uv);
        }
    }
}

long round4(long n) { return (n + 3) & ~3L; }
int chunks_of(int S) { return (S + kChunk - 1) / kChunk; }
int popcount4(int want) { return (want & 1) + ((want >> 1) & 1) + ((want >> 2) & 1) + ((want >> 3) & 1); }

// the coefficient rows of the workspace, in the order cp, ck, ce, cv, each present only when wanted
struct PolWs { float *sums, *partials, *stats, *c[4]; };
PolWs ws_layout(float* ws, int B, int S, int want) {
    PolWs L;
    L.sums = ws;
    L.partials = ws + 8;
    L.stats = ws + kPolWsHead;
    float* next = L.stats + round4(2L * B * chunks_of(S));
    const long R4 = round4((long)B * S);
    for (int k = 0; k < 4; ++k) {
        L.c[k] = (want >> k) & 1 ? next : nullptr;
        if ((want >> k) & 1) next += R4;
    }
    return L;
}

bool all16(std::initializer_list<const void*> ps) {
    for (const void* q : ps)
        if (!aligned(q, 16)) return false;
    return true;
}
bool all4(std::initializer_list<const void*> ps) {
    for (const void* q : ps)
        if (!aligned(q, 4)) return false;
    return true;
}

}  // namespace
}  // namespace hpc_rll

using namespace hpc_rll;

extern "C" int64_t hpc_rll_lm_policy_workspace_floats(int B, int S, int want) {
    if (B < 0 || S < 0 || want < 0 || want > 15) return HPC_RLL_EINVAL;
    return kPolWsHead + round4(2L * B * chunks_of(S)) + popcount4(want) * round4((long)B * S);
}

extern "C" int hpc_rll_lm_policy_forward(const float* logp, const float* old_logp, const float* adv, int adv_per_sequence,
                                         const float* weight, const float* ref_logp, const float* entropy,
                                         const float* value_new, const float* value_old, const float* ret, float* out8, float* ws,
                                         int B, int S, int ratio, int objective, float clip_low, float clip_high, float dual_clip,
                                         int kl, int agg, float norm_len, int use_value_clip, float value_clip, int want,
                                         int mapping, void* stream) {
    if (!out8 || B < 0 || S < 0) return HPC_RLL_EINVAL;
    if (ratio < 0 || ratio > 1 || objective < 0 || objective > 1 || kl < 0 || kl > 2 || agg < 0 || agg > 2 || mapping < 0 ||
        mapping > 2 || want < 0 || want > 15)
        return HPC_RLL_EINVAL;
    if (!(clip_low >= 0.f && clip_high >= 0.f && std::isfinite(clip_low) && std::isfinite(clip_high))) return HPC_RLL_EINVAL;
    if (objective == HPC_RLL_POLICY_OBJ_CISPO && dual_clip > 1.f) return HPC_RLL_EINVAL;
    if (agg == HPC_RLL_POLICY_AGG_CONSTANT ? !(norm_len > 0.f && std::isfinite(norm_len)) : norm_len != 0.f) return HPC_RLL_EINVAL;
    if (use_value_clip && !(value_clip >= 0.f)) return HPC_RLL_EINVAL;
    const int nval = (value_new ? 1 : 0) + (value_old ? 1 : 0) + (ret ? 1 : 0);
    if (nval != 0 && nval != 3) return HPC_RLL_EINVAL;
    if (((want & 2) && !(ref_logp && (want & 1))) || ((want & 4) && !entropy) || ((want & 8) && !value_new)) return HPC_RLL_EINVAL;
    const bool empty = B == 0 || S == 0;
    if (!empty && (!logp || !old_logp || !adv || !ws)) return HPC_RLL_EINVAL;
    if (!all4({logp, old_logp, adv, weight, ref_logp, entropy, value_new, value_old, ret, out8, ws})) return HPC_RLL_EALIGN;
    hipStream_t st = (hipStream_t)stream;
    if (empty) return (int)hipMemsetAsync(out8, 0, 8 * sizeof(float), st);

    const int nchunk = chunks_of(S);
    const PolWs L = ws_layout(ws, B, S, want);
    const bool wave = mapping == HPC_RLL_POLICY_MAP_WAVE || (mapping == HPC_RLL_POLICY_MAP_RULE && S <= kWaveSeqMax);
    const bool need_seq = ratio == HPC_RLL_POLICY_RATIO_SEQUENCE || agg == HPC_RLL_POLICY_AGG_SEQUENCE;
    const bool wide = S % 4 == 0 && all16({logp, old_logp, adv_per_sequence ? nullptr : adv, weight, ref_logp, entropy, value_new,
                                           value_old, ret, ws});
    float sc = 1.f;
    if (agg == HPC_RLL_POLICY_AGG_SEQUENCE) sc = (float)(1.0 / (double)B);
    if (agg == HPC_RLL_POLICY_AGG_CONSTANT) sc = (float)(1.0 / ((double)B * (double)norm_len));
    const PolArgs p{logp, old_logp, adv, weight, ref_logp, entropy, value_new, value_old, ret, L.c[0], L.c[1], L.c[2], L.c[3],
                    B, S, nchunk, adv_per_sequence ? 1 : 0, ratio, objective, kl, agg, use_value_clip ? 1 : 0, need_seq ? 1 : 0,
                    1.f - clip_low, 1.f + clip_high, dual_clip, value_clip, sc};
    const long pairs = (long)B * nchunk;
    long sgrid = 0;
    if (!wave && need_seq) {
        sgrid = pairs < kFoldMaxGrid ? pairs : kFoldMaxGrid;
        if (wide) hipLaunchKernelGGL(lm_policy_stats_kernel<true>, dim3((unsigned)sgrid), dim3(256), 0, st, p, L.stats);
        else hipLaunchKernelGGL(lm_policy_stats_kernel<false>, dim3((unsigned)sgrid), dim3(256), 0, st, p, L.stats);
        const int rc = last_error();
        if (rc) return rc;
    }
    long grid = wave ? ((long)B + 3) / 4 : pairs;
    if (grid > kFoldMaxGrid) grid = kFoldMaxGrid;
    const bool token_agg = agg == HPC_RLL_POLICY_AGG_TOKEN;
    const float scales[kPolSums] = {sc, sc, sc, sc, sc, sc, sc, 1.f};
    int rc = launch_folded(grid, kPolSums, scales, token_agg ? L.sums : out8, L.partials, st, [&](unsigned blocks, const ScanFold& fold) {
        if (wave) {
            if (wide) hipLaunchKernelGGL(lm_policy_wave_kernel<true>, dim3(blocks), dim3(256), 0, st, p, L.partials, fold);
            else hipLaunchKernelGGL(lm_policy_wave_kernel<false>, dim3(blocks), dim3(256), 0, st, p, L.partials, fold);
        } else {
            if (wide) hipLaunchKernelGGL(lm_policy_chunk_kernel<true>, dim3(blocks), dim3(256), 0, st, p, L.stats, L.partials, fold);
            else hipLaunchKernelGGL(lm_policy_chunk_kernel<false>, dim3(blocks), dim3(256), 0, st, p, L.stats, L.partials, fold);
        }
        return last_error();
    });
    if (rc) return rc;
    if (token_agg) {
        hipLaunchKernelGGL(lm_policy_final_kernel, dim3(1), dim3(64), 0, st, L.sums, out8);
        rc = last_error();
        if (rc) return rc;
    }
    g_pol_fwd.note({wave ? HPC_RLL_POLICY_MAP_WAVE : HPC_RLL_POLICY_MAP_CHUNK, sgrid ? 1 : 0, (int)sgrid, (int)grid, wide ? 16 : 4,
                    wave ? 0 : nchunk});
    return HPC_RLL_OK;
}

extern "C" int hpc_rll_lm_policy_backward(const float* g_policy, const float* g_kl, const float* g_value, const float* g_entropy,
                                          const float* ws, float* grad_logp, float* grad_entropy, float* grad_value, int B, int S,
                                          int want, int agg, void* stream) {
    if (B < 0 || S < 0 || want < 0 || want > 15 || agg < 0 || agg > 2) return HPC_RLL_EINVAL;
    if ((grad_logp && !(want & 1)) || (grad_entropy && !(want & 4)) || (grad_value && !(want & 8))) return HPC_RLL_EINVAL;
    const bool empty = B == 0 || S == 0;
    if (!empty && !ws) return HPC_RLL_EINVAL;
    if (!all4({g_policy, g_kl, g_value, g_entropy, ws, grad_logp, grad_entropy, grad_value})) return HPC_RLL_EALIGN;
    if (empty || !(grad_logp || grad_entropy || grad_value)) return HPC_RLL_OK;
    const PolWs L = ws_layout(const_cast<float*>(ws), B, S, want);
    const long n = (long)B * S;
    // an output that was not differentiated (NULL) has the upstream gradient 0
    const PolGradArgs q{g_policy, g_kl, g_value, g_entropy, agg == HPC_RLL_POLICY_AGG_TOKEN ? L.sums + 7 : nullptr,
                        L.c[0], L.c[1], L.c[2], L.c[3], grad_logp, grad_entropy, grad_value, n};
    const bool wide = all16({ws, grad_logp, grad_entropy, grad_value});
    long grid = (n + 1023) / 1024;
    if (grid > 2048) grid = 2048;
    if (wide) hipLaunchKernelGGL(lm_policy_grad_kernel<true>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, q);
    else hipLaunchKernelGGL(lm_policy_grad_kernel<false>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, q);
    const int rc = last_error();
    if (!rc) g_pol_bwd.note({(int)grid, wide ? 16 : 4});
    return rc;
}

extern "C" int hpc_rll_lm_policy_last_config(int* out) {
    if (!out) return HPC_RLL_EINVAL;
    g_pol_fwd.read(out);
    g_pol_bwd.read(out + kFwdInts);
    return HPC_RLL_OK;
}
static_assert(HPC_RLL_LM_POLICY_CONFIG_INTS == kFwdInts + kBwdInts, "the layout documented in hpc_rll_hip.h");
static_assert(HPC_RLL_LM_POLICY_CHUNK == kChunk && HPC_RLL_LM_POLICY_WAVE_SEQ_MAX == kWaveSeqMax, "the constants of hpc_rll_hip.h");
