// lm_ppo.hip -- token-level PPO for language models on gfx950: the per-token log-probability AND entropy over a large
// vocabulary from one read of the logits, GAE on the (B,S) layout with a response mask, the clipped PPO token loss with
// value loss and entropy, and the streaming gradient of both head outputs.
//
// No reference counterpart; the semantics are those of TRL's / OpenRLHF's PPO trainers (see hpc_rll_hip.h for the formulas).
//
// Kernels:
//   * lm_head_kernel<Elem, ALIGNED, NT, true> (lm_head.hpp, the kernel grpo.hip instantiates without the entropy): one read
//     of the row, kInFlight 16-byte loads in flight, a wave or a workgroup per row, peeled ends, an online TRIPLE per lane
//         m = max x,   s = sum e^(x-m),   u = sum e^(x-m) (x-m)
//     so that lse = m + ln s, logp = x[a] - lse, H = ln s - u/s.
//   * lm_gae_kernel: a wave per sequence walks S from the back, 64 tokens (one per lane, coalesced) per step.  A live token
//     maps the carry (A, Vn) to (gl A + g Vn + (r - V), V), a dropped one is the identity; these maps are closed under
//     composition as A' = a A + b Vn + c, Vn' = d Vn + e, and a step is a 6-stage suffix scan of the five coefficients.
//     The whitening statistics (n, mean, M2) are formed from centred values per step and merged with Chan's update in a
//     fixed order: step -> wave -> workgroup -> one triple per workgroup in the workspace.
//   * lm_whiten_kernel: every workgroup merges the workgroup triples in the same fixed order, then adv = (A - mu) rsqrt(var + eps).
//   * lm_ppo_token_kernel: a wave per sequence (as grpo_token_kernel: seq_weight_sum, then everything); seven sums leave
//     through publish_wave_sums (colscan.hpp).
//   * lm_ppo_final_kernel: the six aggregates from the sums.
//   * lm_grad_kernel<Elem, WIDE, NT>: grad[r,v] = c1 ([v = a] - p_v) - c2 p_v (x_v - lse + H), nontemporal stores in the
//     logits' dtype through stream_row (lm_head.hpp); a row with c1 == c2 == 0 is zero-filled without reading its logits
//     (zero_row; decided on the device).  Unlike grpo.hip's gradient, liveness here reads `weight` too.
//   * lm_value_grad_kernel: grad_value = g cv / den, (B,S).
// No float atomics; every sum has a fixed order, so two runs give the same bits.
#include <hip/hip_runtime.h>

#include "colscan.hpp"
#include "hostutil.hpp"
#include "hpc_rll_hip.h"
#include "lm_head.hpp"
#include "wave.hpp"

namespace hpc_rll {
namespace {

constexpr int kLmSums = 7;        // policy, value, entropy, approx_kl, ratio, clipfrac numerators, sum w
constexpr int kGaeChunk = 64;     // tokens per step of a wave
constexpr float kWhitenEps = 1e-8f;

// The dispatch records (hpc_rll_lm_ppo_last_config)
constexpr int kHeadInts = 7, kGaeInts = 5, kWhitenInts = 3, kTokenInts = 3, kGradInts = 6;
LaunchRecord<kHeadInts> g_lm_head;
LaunchRecord<kGaeInts> g_lm_gae;
LaunchRecord<kWhitenInts> g_lm_whiten;
LaunchRecord<kTokenInts> g_lm_token;
LaunchRecord<kGradInts> g_lm_grad;

// the head with the entropy: logp[row] = x[a] - lse, lse[row], ent[row] = ln s - u/s
int lm_head_any(const void* x, int elem, const int64_t* action, const float* weight, float* logp, float* lse, float* ent,
                long rows, int V, hipStream_t st) {
    return lm_head_launch<true>(x, elem, action, weight, logp, lse, ent, rows, V, st, g_lm_head);
}

// ================================================================================================
// the gradient of both head outputs.  Per row: c1 = k1[row] g1 / den, c2 = k2[row] g2 / den with g1, g2 device scalars
// (NULL: `gdef`) and den a device scalar (NULL: 1; a zero den gives zero rows).  k1 or k2 NULL: that coefficient is 0.
// ================================================================================================
struct LmGradArgs {
    const int64_t* action; const float* weight; const float *lse, *ent, *k1, *k2, *g1, *g2, *den; float gdef;
};

template <class Elem, bool WIDE, int NT>
__global__ __launch_bounds__(256) void lm_grad_kernel(const Elem* __restrict__ x, const LmGradArgs q, Elem* __restrict__ grad,
                                                      long rows, int V) {
    constexpr int RPW = 256 / NT;
    const int tid = threadIdx.x % NT, sub = threadIdx.x / NT;
    float u1 = q.g1 ? q.g1[0] : q.gdef, u2 = q.g2 ? q.g2[0] : q.gdef;
    if (q.den) {
        const float d = q.den[0];
        const float inv = d != 0.f ? 1.f / d : 0.f;
        u1 = d != 0.f ? u1 * inv : 0.f;
        u2 = d != 0.f ? u2 * inv : 0.f;
    }
    for (long r0 = (long)blockIdx.x * RPW; r0 < rows; r0 += (long)gridDim.x * RPW) {
        const long row = r0 + sub;
        if (row >= rows) continue;
        const long a = q.action[row];
        const float w = q.weight ? q.weight[row] : 1.f;
        const bool live = a >= 0 && a < (long)V && w != 0.f;
        const float c1 = (live && q.k1) ? q.k1[row] * u1 : 0.f;
        const float c2 = (live && q.k2) ? q.k2[row] * u2 : 0.f;
        const int ai = live ? (int)a : -1;
        const Elem* p = x + (size_t)row * (size_t)V;
        Elem* o = grad + (size_t)row * (size_t)V;
        if (c1 == 0.f && c2 == 0.f) {
            zero_row<Elem, WIDE, NT>(o, V, tid);
            continue;
        }
        const float l = q.lse[row];
        const float c0 = fmaf(c2, q.ent[row], c1);   // grad = [v = a] c1 - (c0 + c2 t) e^t,  t = x - lse
        stream_row<Elem, WIDE, NT>(p, o, V, tid, ai, [&](float xv, bool chosen) {
            const float t = clampf(xv) - l;
            const float e = ex2(t * kLog2eG);
            const float pg = e == 0.f ? 0.f : fmaf(c2, t, c0) * e;   // a masked entry: exactly 0, never 0 * huge
            return (chosen ? c1 : 0.f) - pg;
        });
    }
}

int lm_grad_any(const void* xv, int elem, const LmGradArgs& q, void* gradv, long rows, int V, hipStream_t st) {
    return with_elem(elem, [&](auto e) {
        using Elem = decltype(e);
        const Elem* x = static_cast<const Elem*>(xv);
        Elem* grad = static_cast<Elem*>(gradv);
        const RowLaunch L = row_launch<Elem>(x, grad, rows, V);
        with_row_kernel(L, [&](auto W, auto NT) {
            hipLaunchKernelGGL((lm_grad_kernel<Elem, decltype(W)::value, decltype(NT)::value>), dim3((unsigned)L.grid), dim3(256),
                               0, st, x, q, grad, rows, V);
        });
        const int rc = last_error();
        if (!rc) g_lm_grad.note({ElemIO<Elem>::kCode, L.wide ? 16 : (int)sizeof(Elem), L.nt, L.rpw, (int)L.grid});
        return rc;
    });
}

// grad_value[i] = g cv[i] / den (g NULL: 0 everywhere)
__global__ __launch_bounds__(256) void lm_value_grad_kernel(const float* __restrict__ g, const float* __restrict__ den,
                                                            const float* __restrict__ cv, float* __restrict__ out, long n) {
    float u = g ? g[0] : 0.f;
    if (den) {
        const float d = den[0];
        u = d != 0.f ? u / d : 0.f;
    }
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const float c = cv[i];
        out[i] = c == 0.f ? 0.f : c * u;
    }
}

// ================================================================================================
// GAE over (B,S): a wave per sequence
// ================================================================================================
// Chan's update of (n, mean, M2) with a second set; sets without elements change nothing
struct Moments { float n, mean, m2; };
__device__ __forceinline__ Moments chan(const Moments& a, const Moments& b) {
    const float n = a.n + b.n;
    if (b.n == 0.f) return a;
    if (a.n == 0.f) return b;
    const float d = b.mean - a.mean;
    Moments r;
    r.n = n;
    r.mean = a.mean + d * (b.n / n);
    r.m2 = a.m2 + b.m2 + d * d * (a.n * (b.n / n));
    return r;
}

struct LmGaeArgs {
    const float *value, *weight, *reward, *kl; float *adv, *ret;
    int B, S, per_seq; float beta, gamma, gl;
};

__global__ __launch_bounds__(256) void lm_gae_kernel(const LmGaeArgs p, float* __restrict__ moments) {
    __shared__ float red[4][3];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    Moments acc{0.f, 0.f, 0.f};   // wave-uniform
    for (long b = (long)blockIdx.x * 4 + wv; b < (long)p.B; b += (long)gridDim.x * 4) {
        const size_t base = (size_t)b * (size_t)p.S;
        float cA = 0.f, cV = 0.f;   // the carry: A and V of the next live token
        bool seen = false;           // a live token lies behind this step (the terminal score has been credited)
        const float score = p.per_seq ? p.reward[b] : 0.f;
        const int steps = (p.S + kGaeChunk - 1) / kGaeChunk;
        for (int c = steps - 1; c >= 0; --c) {
            const int s = c * kGaeChunk + lane;
            const bool in = s < p.S;
            float w = 0.f, v = 0.f, r = 0.f, k = 0.f;
            if (in) {
                w = p.weight ? p.weight[base + s] : 1.f;
                v = p.value[base + s];
                if (!p.per_seq) r = p.reward[base + s];
                if (p.kl) k = p.kl[base + s];
            }
            const bool live = in && w != 0.f;
            const unsigned long long mask = __ballot(live);
            if (mask == 0ull) {   // nothing lives here: the carry passes unchanged (uniform over the wave)
                if (in) {
                    p.adv[base + s] = 0.f;
                    p.ret[base + s] = 0.f;
                }
                continue;
            }
            if (p.per_seq) {
                const int last = 63 - __clzll((long long)mask);
                r = (!seen && lane == last) ? score : 0.f;
            }
            seen = true;
            if (p.kl) r = fmaf(-p.beta, k, r);
            // this token's map; a dropped one is the identity, whatever its operands hold
            float fa = live ? p.gl : 1.f, fb = live ? p.gamma : 0.f, fc = live ? r - v : 0.f;
            float fd = live ? 0.f : 1.f, fe = live ? v : 0.f;
            // suffix scan: F_lane = f_lane o f_(lane+1) o ... o f_63 (the rightmost is applied first)
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const float oa = __shfl_down(fa, d, 64), ob = __shfl_down(fb, d, 64), oc = __shfl_down(fc, d, 64);
                const float od = __shfl_down(fd, d, 64), oe = __shfl_down(fe, d, 64);
                if (lane + d < 64) {
                    const float na = fa * oa;
                    const float nb = fmaf(fa, ob, fb * od);
                    const float nc = fmaf(fa, oc, fmaf(fb, oe, fc));
                    const float nd = fd * od;
                    const float ne = fmaf(fd, oe, fe);
                    fa = na; fb = nb; fc = nc; fd = nd; fe = ne;
                }
            }
            const float A = fmaf(fa, cA, fmaf(fb, cV, fc));
            if (in) {
                p.adv[base + s] = live ? A : 0.f;
                p.ret[base + s] = live ? A + v : 0.f;
            }
            const float nV = fmaf(fd, cV, fe);
            cA = __shfl(A, 0, 64);
            cV = __shfl(nV, 0, 64);
            // the step's moments from centred values, then Chan's update of the wave's
            const float cnt = (float)__popcll(mask);
            const float mu = wave_sum(live ? A : 0.f) / cnt;
            const float dv = live ? A - mu : 0.f;
            const float m2 = wave_sum(dv * dv);
            acc = chan(acc, Moments{cnt, mu, m2});
        }
    }
    if (lane == 0) {
        red[wv][0] = acc.n;
        red[wv][1] = acc.mean;
        red[wv][2] = acc.m2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        Moments m{red[0][0], red[0][1], red[0][2]};
        for (int i = 1; i < 4; ++i) m = chan(m, Moments{red[i][0], red[i][1], red[i][2]});
        moments[3 * blockIdx.x + 0] = m.n;
        moments[3 * blockIdx.x + 1] = m.mean;
        moments[3 * blockIdx.x + 2] = m.m2;
    }
}

// adv = (A - mu) rsqrt(var + eps) on the live tokens.  Every workgroup merges the `nm` workgroup triples of the GAE launch
// itself, in the same order: lane i of wave 0 merges triples i, i + 64, ... in turn, then the lanes merge pairwise.
__global__ __launch_bounds__(256) void lm_whiten_kernel(const float* __restrict__ moments, int nm,
                                                        const float* __restrict__ weight, float* __restrict__ adv, long n) {
    __shared__ float stat[2];
    if (threadIdx.x < 64) {
        Moments m{0.f, 0.f, 0.f};
        for (int i = threadIdx.x; i < nm; i += 64) m = chan(m, Moments{moments[3 * i], moments[3 * i + 1], moments[3 * i + 2]});
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {   // lane l (a multiple of 2d) takes lane l + d: a fixed tree
            Moments o;
            o.n = __shfl_down(m.n, d, 64);
            o.mean = __shfl_down(m.mean, d, 64);
            o.m2 = __shfl_down(m.m2, d, 64);
            m = chan(m, o);
        }
        if (threadIdx.x == 0) {
            const float var = m.n > 0.f ? m.m2 / m.n : 0.f;
            stat[0] = m.mean;
            stat[1] = 1.f / sqrtf(var + kWhitenEps);
        }
    }
    __syncthreads();
    const float mu = stat[0], rs = stat[1];
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const float w = weight ? weight[i] : 1.f;
        const float a = adv[i];
        adv[i] = w != 0.f ? (a - mu) * rs : 0.f;
    }
}

// ================================================================================================
// the token loss: a wave per sequence
// ================================================================================================
struct LmTokenArgs {
    const float *pn, *ent, *po, *adv, *weight, *vnew, *vold, *ret; const int64_t* action;
    float *cp, *ce, *cv;
    int B, S, V, seq_mean, use_vclip; float clip, dual, vclip, scale;
};

__global__ __launch_bounds__(256) void lm_ppo_token_kernel(const LmTokenArgs p, float* __restrict__ partials,
                                                           const ScanFold fold) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const float lo = 1.f - p.clip, hi = 1.f + p.clip;
    const bool dual_on = p.dual > 1.f;
    float acc[kLmSums];
#pragma unroll
    for (int k = 0; k < kLmSums; ++k) acc[k] = 0.f;
    for (long b = (long)blockIdx.x * 4 + wv; b < (long)p.B; b += (long)gridDim.x * 4) {
        const size_t base = (size_t)b * (size_t)p.S;
        const float sw = seq_weight_sum(p.action, p.weight, base, p.S, p.V, lane);
        // 'sequence': every sum of the sequence is divided by its weight (a sequence without weight contributes 0 and still
        // counts in B) and `scale` = 1/B is applied with the batch sums; 'token': plain sums, divided by sum w at the end
        const float inv = p.seq_mean ? (sw != 0.f ? 1.f / sw : 0.f) : 1.f;
        const float cs = p.seq_mean ? p.scale * inv : 1.f;
        float sm[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int s = lane; s < p.S; s += 64) {
            const size_t i = base + s;
            const long a = p.action[i];
            float w = p.weight ? p.weight[i] : 1.f;
            const bool live = a >= 0 && a < (long)p.V && w != 0.f;
            w = live ? w : 0.f;                          // a dropped token: selected away, whatever its values are
            const float pn = live ? p.pn[i] : 0.f, po = live ? p.po[i] : 0.f;
            const float A = live ? p.adv[i] : 0.f, H = live ? p.ent[i] : 0.f;
            const float d = pn - po;
            const float r = expf(d);
            const float rc = fminf(fmaxf(r, lo), hi);
            const float t1 = -A * r, t2 = -A * rc;
            float l = t2 > t1 ? t2 : t1;
            float dl = t2 > t1 ? 0.f : t1;               // a tie counts as unclipped
            if (dual_on && A < 0.f) {
                const float t3 = -p.dual * A;
                if (t3 < l) {
                    l = t3;
                    dl = 0.f;
                }
            }
            const float clipped = (r > hi || r < lo) ? 1.f : 0.f;
            const float k1 = expm1f(d) - d;
            const float wc = w * cs;
            sm[0] = fmaf(w, l, sm[0]);
            sm[2] = fmaf(w, H, sm[2]);
            sm[3] = fmaf(w, k1, sm[3]);
            sm[4] = fmaf(w, r, sm[4]);
            sm[5] = fmaf(w, clipped, sm[5]);
            p.cp[i] = live ? wc * dl : 0.f;
            p.ce[i] = live ? wc : 0.f;
            if (p.vnew) {
                const float v = live ? p.vnew[i] : 0.f, vo = live ? p.vold[i] : 0.f, rt = live ? p.ret[i] : 0.f;
                const float e1 = v - rt;
                float lv = e1 * e1, dv = e1;
                if (p.use_vclip) {
                    const float dd = v - vo;
                    const bool out = dd > p.vclip || dd < -p.vclip;
                    const float e2 = vo + fminf(fmaxf(dd, -p.vclip), p.vclip) - rt;
                    if (out && e2 * e2 > lv) {   // the clipped branch: no gradient
                        lv = e2 * e2;
                        dv = 0.f;
                    }
                }
                sm[1] = fmaf(w, 0.5f * lv, sm[1]);
                p.cv[i] = live ? wc * dv : 0.f;
            }
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) acc[k] += wave_sum(sm[k]) * inv;
        acc[6] += sw;
    }
    publish_wave_sums<kLmSums>(acc, partials, fold);
}

// sums (7) -> out8: the six aggregates, the denominator (sum w in 'token' mode, 1 in 'sequence' mode), 0.  raw: the
// numerators are left undivided (a sharded caller divides after its all-reduce).
__global__ __launch_bounds__(64) void lm_ppo_final_kernel(const float* __restrict__ sums, float* __restrict__ out8, int seq_mean,
                                                          int raw) {
    const int k = threadIdx.x;
    if (k >= 8) return;
    const float den = seq_mean ? 1.f : sums[6];
    float v = 0.f;
    if (k < 6) v = (raw || seq_mean) ? sums[k] : (den != 0.f ? sums[k] / den : 0.f);
    else if (k == 6) v = den;
    out8[k] = v;
}

constexpr long kLmWsHead = 6;   // per-token rows of the workspace: lse, ent, cp, ce, cv, logp

}  // namespace
}  // namespace hpc_rll

using namespace hpc_rll;

extern "C" int hpc_rll_lm_head_forward(const void* logits, int elem, const int64_t* action, const float* weight, float* logp,
                                       float* lse, float* entropy, int64_t rows, int V, void* stream) {
    const bool empty = rows == 0 || V == 0;
    if (!empty && (!logits || !action || !logp || !lse || !entropy)) return HPC_RLL_EINVAL;
    if (const int bad = lm_shape_status(rows, 1, V, elem, aligned(logits, elem_size(elem)) && aligned(action, 8) &&
                                        aligned(weight, 4) && aligned(logp, 4) && aligned(lse, 4) && aligned(entropy, 4)))
        return bad;
    hipStream_t st = (hipStream_t)stream;
    if (empty) {   // V == 0 with rows: no token has a probability; zeros
        for (float* o : {logp, lse, entropy})
            if (rows > 0 && o) {
                const int rc = (int)hipMemsetAsync(o, 0, (size_t)rows * sizeof(float), st);
                if (rc) return rc;
            }
        return HPC_RLL_OK;
    }
    return lm_head_any(logits, elem, action, weight, logp, lse, entropy, (long)rows, V, st);
}

extern "C" int hpc_rll_lm_head_backward(const float* g_logp, const float* g_entropy, const void* logits, int elem,
                                        const int64_t* action, const float* weight, const float* lse, const float* entropy,
                                        void* grad_logits, int64_t rows, int V, void* stream) {
    const bool empty = rows == 0 || V == 0;
    if (!empty && (!logits || !action || !lse || !entropy || !grad_logits)) return HPC_RLL_EINVAL;
    if (const int bad = lm_shape_status(rows, 1, V, elem, aligned(logits, elem_size(elem)) && aligned(grad_logits, elem_size(elem)) &&
                                        aligned(action, 8) && aligned(g_logp, 4) && aligned(g_entropy, 4) &&
                                        aligned(weight, 4) && aligned(lse, 4) && aligned(entropy, 4)))
        return bad;
    if (empty) return HPC_RLL_OK;
    const LmGradArgs q{action, weight, lse, entropy, g_logp, g_entropy, nullptr, nullptr, nullptr, 1.f};
    return lm_grad_any(logits, elem, q, grad_logits, (long)rows, V, (hipStream_t)stream);
}

extern "C" int64_t hpc_rll_lm_gae_workspace_floats(void) { return 3 * kFoldMaxGrid; }

extern "C" int hpc_rll_lm_gae(const float* value, const float* weight, const float* reward, int reward_per_sequence,
                              const float* kl, float* adv, float* ret, float* ws, int B, int S, float beta, float gamma,
                              float lam, int whiten, void* stream) {
    const bool empty = B == 0 || S == 0;
    if (!empty && (!value || !reward || !adv || !ret || !ws)) return HPC_RLL_EINVAL;
    if (B < 0 || S < 0) return HPC_RLL_EINVAL;
    if (!aligned(value, 4) || !aligned(weight, 4) || !aligned(reward, 4) || !aligned(kl, 4) || !aligned(adv, 4) ||
        !aligned(ret, 4) || !aligned(ws, 4))
        return HPC_RLL_EALIGN;
    if (empty) return HPC_RLL_OK;
    hipStream_t st = (hipStream_t)stream;
    long grid = ((long)B + 3) / 4;
    if (grid > kFoldMaxGrid) grid = kFoldMaxGrid;
    const LmGaeArgs p{value, weight, reward, kl, adv, ret, B, S, reward_per_sequence ? 1 : 0, kl ? beta : 0.f, gamma, gamma * lam};
    hipLaunchKernelGGL(lm_gae_kernel, dim3((unsigned)grid), dim3(256), 0, st, p, ws);
    int rc = last_error();
    if (rc) return rc;
    g_lm_gae.note({64, 4, kGaeChunk, (int)grid});
    if (!whiten) return rc;
    const long n = (long)B * S;
    long wgrid = (n + 1023) / 1024;   // four tokens per thread
    if (wgrid > 2048) wgrid = 2048;
    hipLaunchKernelGGL(lm_whiten_kernel, dim3((unsigned)wgrid), dim3(256), 0, st, ws, (int)grid, weight, adv, n);
    rc = last_error();
    if (!rc) g_lm_whiten.note({256, (int)wgrid});
    return rc;
}

// ws (floats), R = B*S: lse (R) | entropy (R) | cp (R) | ce (R) | cv (R) | logp (R) | the seven sums (8) | partial sums
extern "C" int64_t hpc_rll_lm_ppo_workspace_floats(int B, int S) {
    if (B < 0 || S < 0) return HPC_RLL_EINVAL;
    return kLmWsHead * (int64_t)B * S + 8 + 8 * (kFoldMaxGrid + 1);
}

extern "C" int hpc_rll_lm_ppo_forward(const void* logit_new, int elem, const float* old_logp, const int64_t* action,
                                      const float* adv, const float* weight, const float* value_new, const float* value_old,
                                      const float* ret, float* out8, float* ws, int B, int S, int V, float clip_ratio,
                                      float dual_clip, int use_value_clip, float value_clip, int seq_mean, int raw, float scale,
                                      void* stream) {
    const bool empty = B == 0 || S == 0 || V == 0;
    if (!out8) return HPC_RLL_EINVAL;
    if (!empty && (!logit_new || !old_logp || !action || !adv || !ws)) return HPC_RLL_EINVAL;
    const int nval = (value_new ? 1 : 0) + (value_old ? 1 : 0) + (ret ? 1 : 0);
    if (nval != 0 && nval != 3) return HPC_RLL_EINVAL;
    if (const int bad = lm_shape_status(B, S, V, elem, aligned(logit_new, elem_size(elem)) && aligned(old_logp, 4) &&
                                        aligned(action, 8) && aligned(adv, 4) && aligned(weight, 4) && aligned(value_new, 4) &&
                                        aligned(value_old, 4) && aligned(ret, 4) && aligned(out8, 4) && aligned(ws, 4)))
        return bad;
    hipStream_t st = (hipStream_t)stream;
    if (empty) return (int)hipMemsetAsync(out8, 0, 8 * sizeof(float), st);
    const long R = (long)B * S;
    float *lse = ws, *ent = ws + R, *cp = ws + 2 * R, *ce = ws + 3 * R, *cv = ws + 4 * R, *pn = ws + 5 * R,
          *sums = ws + kLmWsHead * R, *partials = ws + kLmWsHead * R + 8;
    int rc = lm_head_any(logit_new, elem, action, weight, pn, lse, ent, R, V, st);
    if (rc) return rc;
    const float sc = seq_mean ? (scale > 0.f ? scale : 1.f / (float)B) : 1.f;
    const LmTokenArgs p{pn, ent, old_logp, adv, weight, value_new, value_old, ret, action, cp, ce, cv,
                        B, S, V, seq_mean ? 1 : 0, use_value_clip ? 1 : 0, clip_ratio, dual_clip, value_clip, sc};
    long grid = ((long)B + 3) / 4;
    if (grid > kFoldMaxGrid) grid = kFoldMaxGrid;
    const float scales[kLmSums] = {sc, sc, sc, sc, sc, sc, 1.f};
    const ScanFold fold = make_fold(st, kLmSums, scales, sums, grid);
    hipLaunchKernelGGL(lm_ppo_token_kernel, dim3((unsigned)grid), dim3(256), 0, st, p, partials, fold);
    rc = last_error();
    if (rc) return rc;
    if (!fold.out) {
        rc = finalize_sums(partials, (int)grid, kLmSums, scales, sums, st);
        if (rc) return rc;
    }
    g_lm_token.note({256, (int)grid});
    hipLaunchKernelGGL(lm_ppo_final_kernel, dim3(1), dim3(64), 0, st, sums, out8, seq_mean ? 1 : 0, raw ? 1 : 0);
    return last_error();
}

extern "C" int hpc_rll_lm_ppo_backward(const float* g_policy, const float* g_entropy, const float* g_value,
                                       const void* logit_new, int elem, const int64_t* action, const float* weight,
                                       const float* ws, void* grad_logit, float* grad_value, int B, int S, int V, int use_den,
                                       void* stream) {
    const bool empty = B == 0 || S == 0 || V == 0;
    if (!empty && (!action || !ws || (grad_logit && !logit_new))) return HPC_RLL_EINVAL;
    if (const int bad = lm_shape_status(B, S, V, elem, aligned(logit_new, elem_size(elem)) && aligned(grad_logit, elem_size(elem)) &&
                                        aligned(action, 8) && aligned(g_policy, 4) && aligned(g_entropy, 4) &&
                                        aligned(g_value, 4) && aligned(weight, 4) && aligned(ws, 4) && aligned(grad_value, 4)))
        return bad;
    if (empty) return HPC_RLL_OK;
    hipStream_t st = (hipStream_t)stream;
    const long R = (long)B * S;
    const float* den = use_den ? ws + kLmWsHead * R + 6 : nullptr;
    int rc = HPC_RLL_OK;
    if (grad_logit) {
        // an output that was not differentiated (NULL) has the upstream gradient 0: its coefficient row is left out
        const LmGradArgs q{action, weight, ws, ws + R, g_policy ? ws + 2 * R : nullptr, g_entropy ? ws + 3 * R : nullptr,
                           g_policy, g_entropy, den, 0.f};
        rc = lm_grad_any(logit_new, elem, q, grad_logit, R, V, st);
        if (rc) return rc;
    }
    if (grad_value) {
        long grid = (R + 255) / 256;
        if (grid > 2048) grid = 2048;
        hipLaunchKernelGGL(lm_value_grad_kernel, dim3((unsigned)grid), dim3(256), 0, st, g_value, den, ws + 4 * R, grad_value, R);
        rc = last_error();
    }
    return rc;
}

extern "C" int hpc_rll_lm_ppo_last_config(int* out) {
    if (!out) return HPC_RLL_EINVAL;
    g_lm_head.read(out);
    g_lm_gae.read(out + kHeadInts);
    g_lm_whiten.read(out + kHeadInts + kGaeInts);
    g_lm_token.read(out + kHeadInts + kGaeInts + kWhitenInts);
    g_lm_grad.read(out + kHeadInts + kGaeInts + kWhitenInts + kTokenInts);
    return HPC_RLL_OK;
}
static_assert(HPC_RLL_LM_PPO_CONFIG_INTS == kHeadInts + kGaeInts + kWhitenInts + kTokenInts + kGradInts,
              "the layout documented in hpc_rll_hip.h");