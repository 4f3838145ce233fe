// fqf.hip -- FQF (Fully parameterized Quantile Function, Yang et al. 2019) for gfx950: the fraction proposal, the quantile TD
// loss on per-sample fractions, the fraction loss and the expected value with its greedy action.  No reference counterpart: the
// formulas restate DI-engine's ding/rl_utils/td.py (fqf_nstep_td_error, fqf_calculate_fraction_loss) and ding/model FQFHead.
//
//   * TD loss: IQN's packed pair loop (dist_shared.hpp) on q (B,K,N), next_n_q (B,K',N) and fractions (B,K): a sample per group
//     of G lanes for max(K,K') <= 64, a wave per sample above; one launch, the loss folded inside it; buf (B,K) is the unit
//     gradient.  The backward streams grad_q (B,K,N), every row one-hot at the sample's action.
//   * fraction loss: the same group mapping; the two strided gathers of a sample sit in its lanes, the neighbours come by lane
//     shuffles, g (B,K-1) is written once and is the gradient on quantiles[:,1:K].
//   * fractions: softmax, inclusive scan and entropy from one read of the row (a row per lane group, or a wave per row with a
//     carried scan for 64 < K <= 1024); the backward is a suffix scan and one group sum.
//   * expected value: lanes along N, a loop over K with the fraction widths staged in LDS; the argmax runs in the same launch.
// Nothing here synchronises with the host; every loss sum has a fixed fold order.
#include <hip/hip_runtime.h>

#include <limits.h>

#include "colscan.hpp"
#include "dist_shared.hpp"
#include "hostutil.hpp"
#include "hpc_rll_hip.h"
#include "nstep.hpp"

namespace hpc_rll {
namespace {

constexpr int kFractionsMaxK = 1024;   // 16 chunks of 64 per lane in the wave kernels
constexpr int kMaxChunks = kFractionsMaxK / 64;

// an action outside [0, N) never addresses memory: the value it would have selected reads as 0
__device__ __forceinline__ bool in_range(long a, int N) { return a >= 0 && a < (long)N; }

// ------------------------------------------------------------------------------------------------ TD loss
// q (B,K,N), next_q (B,K',N), qh (B,K).  buf[b,i] = unit gradient wrt q[b,i,a_b].
template <int G>
__global__ __launch_bounds__(256) void fqf_td_fwd_group_kernel(
    const float* __restrict__ q, const float* __restrict__ next_q, const int64_t* __restrict__ action,
    const int64_t* __restrict__ next_action, const float* __restrict__ reward, const float* __restrict__ done,
    const float* __restrict__ qh, const float* __restrict__ weight, const float* __restrict__ value_gamma,
    float* __restrict__ td_err, float* __restrict__ buf, float* __restrict__ partials, int K, int Kp, int nstep, int B, int N,
    float gamma, float gamma_n, float kappa, float scale, const ScanFold fold) {
    group_per_sample<G>(B, partials, fold, [&](long b, bool ok, int gl, int base) -> float {
        float R = 0.f, vg = 0.f, w = 0.f, qi = 0.f, rho = 0.f, tgt = 0.f;
        if (ok) {
            // every scalar of the sample is requested before the first use, in the order of iqn_fwd_group_kernel
            const long a = action[b], na = next_action[b];
            const float dn = done[b], vgm = value_gamma ? value_gamma[b] : gamma_n;
            w = weight ? weight[b] : 1.f;
            if (gl < K) rho = qh[(size_t)b * K + gl];
            R = nstep_return1(reward, B, nstep, gamma, b);
            vg = vgm * (1.f - dn);
            if (gl < K && in_range(a, N)) qi = q[((size_t)b * K + gl) * N + a];
            if (gl < Kp) tgt = fmaf(vg, in_range(na, N) ? next_q[((size_t)b * Kp + gl) * N + na] : 0.f, R);
        }
        return quantile_huber_group<G>(b, ok, gl, base, K, Kp, qi, rho, tgt, w, kappa, scale, td_err, buf);
    });
}

// any K, K': a wave per sample, the arithmetic of iqn_fwd_kernel term by term
__global__ __launch_bounds__(256) void fqf_td_fwd_wave_kernel(
    const float* __restrict__ q, const float* __restrict__ next_q, const int64_t* __restrict__ action,
    const int64_t* __restrict__ next_action, const float* __restrict__ reward, const float* __restrict__ done,
    const float* __restrict__ qh, const float* __restrict__ weight, const float* __restrict__ value_gamma,
    float* __restrict__ td_err, float* __restrict__ buf, float* __restrict__ partials, int K, int Kp, int nstep, int B, int N,
    float gamma, float gamma_n, float kappa, float scale, const ScanFold fold) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long b = (long)blockIdx.x * 4 + wv;
    float contrib[1] = {0.f};
    if (b < (long)B) {   // wave-uniform
        const float R = nstep_return1(reward, B, nstep, gamma, b);
        const float vg = (value_gamma ? value_gamma[b] : gamma_n) * (1.f - done[b]);
        const long a = action[b], na = next_action[b];
        const bool av = in_range(a, N), nav = in_range(na, N);
        const float w = weight ? weight[b] : 1.f;
        const float inv_tp = 1.f / (float)Kp;
        float loss = 0.f;
        for (int i = lane; i < K; i += 64) {
            const float qi = av ? q[((size_t)b * K + i) * N + a] : 0.f;
            const float rho = qh[(size_t)b * K + i];
            float li = 0.f, gi = 0.f;
            for (int j = 0; j < Kp; ++j) {
                const float tgt = fmaf(vg, nav ? next_q[((size_t)b * Kp + j) * N + na] : 0.f, R);
                const float e = tgt - qi;
                const float ae = fabsf(e);
                const float hub = (ae <= kappa) ? 0.5f * e * e : kappa * (ae - 0.5f * kappa);
                const float dh = (ae <= kappa) ? e : ((e > 0.f) ? kappa : -kappa);
                const float qw = fabsf(rho - ((e < 0.f) ? 1.f : 0.f)) / kappa;
                li = fmaf(qw, hub, li);
                gi = fmaf(qw, dh, gi);
            }
            loss += li;
            buf[(size_t)b * K + i] = -gi * inv_tp * w * scale;   // de/dq = -1
        }
        loss = wave_sum(loss) * inv_tp;
        if (lane == 0) td_err[b] = loss;
        contrib[0] = loss * w;
    }
    publish_wave_sums<1>(contrib, partials, fold);
}

// grad_q[b,i,n] = (n == a_b) ? g * buf[b,i] : 0: rows of N floats, V of them per store (V = 4: 16-byte nontemporal stores).
// A workgroup takes RPB = max(1, 256 / NC) rows at a time, NC = N / V stores each: a thread keeps its column, so the only
// division in the loop is row / K (32 bits: the host refuses B * K >= 2^31).
template <int V>
__global__ __launch_bounds__(256) void fqf_td_bwd_kernel(const float* __restrict__ g, const float* __restrict__ buf,
                                                         const int64_t* __restrict__ action, float* __restrict__ grad,
                                                         unsigned K, unsigned rows, int N, unsigned NC, unsigned RPB) {
    const float u = g[0];
    const unsigned r_in = threadIdx.x / NC, c0 = threadIdx.x - r_in * NC;
    if (r_in >= RPB) return;   // the lanes past the last whole row of the tile (NC > 256: one row, every thread strides over it)
    for (unsigned long row = (unsigned long)blockIdx.x * RPB + r_in; row < rows; row += (unsigned long)gridDim.x * RPB) {
        const unsigned r = (unsigned)row;
        const long a = action[r / K];
        const float v = u * buf[r];
        float* __restrict__ out = grad + (size_t)r * N;
        for (unsigned c = c0; c < NC; c += 256) {
            Pack<V> o;
#pragma unroll
            for (int k = 0; k < V; ++k) o.v[k] = ((long)c * V + k == a) ? v : 0.f;
            store_pack<V, true>(out + (size_t)c * V, o);
        }
    }
}

// ------------------------------------------------------------------------------------------------ fraction loss
// The two terms of one fraction: s its value, h / h_next the quantile values on its sides, lo / hi the neighbours it is
// compared with (raw inputs: the comparisons are exact).
__device__ __forceinline__ float fraction_term(float s, float h, float h_next, float lo, float hi) {
    const float v1 = s - h, v2 = s - h_next;
    return (s > lo ? v1 : -v1) + (s < hi ? v2 : -v2);
}

// q_tau_i (B,K-1,N), q_value (B,K,N), quantiles (B,K+1).  g (B,K-1) is the output and the gradient on quantiles[:,1:K].
template <int G>
__global__ __launch_bounds__(256) void fqf_fraction_loss_fwd_group_kernel(
    const float* __restrict__ qt, const float* __restrict__ qv, const float* __restrict__ quant,
    const int64_t* __restrict__ action, float* __restrict__ g, float* __restrict__ partials, int K, int B, int N,
    const ScanFold fold) {
    group_per_sample<G>(B, partials, fold, [&](long b, bool ok, int gl, int base) -> float {
        const int M = K - 1;
        float s = 0.f, h = 0.f, tau = 0.f;
        if (ok) {
            const long a = action[b];
            const bool av = in_range(a, N);
            if (gl < M) tau = quant[(size_t)b * (K + 1) + gl + 1];
            if (av && gl < M) s = qt[((size_t)b * M + gl) * N + a];
            if (av && gl < K) h = qv[((size_t)b * K + gl) * N + a];
        }
        const int l = base + gl, up = gl + 1 < G ? l + 1 : l;
        const float s_prev = __shfl(s, gl > 0 ? l - 1 : l, 64), s_next = __shfl(s, up, 64), h_next = __shfl(h, up, 64);
        const float gi = fraction_term(s, h, h_next, gl == 0 ? h : s_prev, gl == M - 1 ? h_next : s_next);
        if (ok && gl < M) g[(size_t)b * M + gl] = gi;
        return hpc_rll::group_sum<G>(gl < M ? gi * tau : 0.f);
    });
}

// K > 64: a wave per sample, the neighbours re-read (they are in cache)
__global__ __launch_bounds__(256) void fqf_fraction_loss_fwd_wave_kernel(
    const float* __restrict__ qt, const float* __restrict__ qv, const float* __restrict__ quant,
    const int64_t* __restrict__ action, float* __restrict__ g, float* __restrict__ partials, int K, int B, int N,
    const ScanFold fold) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long b = (long)blockIdx.x * 4 + wv;
    float contrib[1] = {0.f};
    if (b < (long)B) {   // wave-uniform
        const int M = K - 1;
        const long a = action[b];
        const bool av = in_range(a, N);
        const float* __restrict__ sp = qt + (size_t)b * M * N + (av ? a : 0);
        const float* __restrict__ hp = qv + (size_t)b * K * N + (av ? a : 0);
        float sum = 0.f;
        for (int i = lane; i < M; i += 64) {
            const float s = av ? sp[(size_t)i * N] : 0.f, h = av ? hp[(size_t)i * N] : 0.f;
            const float h_next = av ? hp[(size_t)(i + 1) * N] : 0.f;
            const float lo = i == 0 ? h : (av ? sp[(size_t)(i - 1) * N] : 0.f);
            const float hi = i == M - 1 ? h_next : (av ? sp[(size_t)(i + 1) * N] : 0.f);
            const float gi = fraction_term(s, h, h_next, lo, hi);
            g[(size_t)b * M + i] = gi;
            sum = fmaf(gi, quant[(size_t)b * (K + 1) + i + 1], sum);
        }
        contrib[0] = wave_sum(sum);
    }
    publish_wave_sums<1>(contrib, partials, fold);
}

// grad_quantiles[b,c] = g_loss * scale * g[b,c-1] for 1 <= c <= K-1, zero in columns 0 and K
__global__ __launch_bounds__(256) void fqf_fraction_loss_bwd_kernel(const float* __restrict__ gl, const float* __restrict__ g,
                                                                    float* __restrict__ grad, int K, long total, float scale) {
    const float u = gl[0] * scale;
    for (long x = (long)blockIdx.x * 256 + threadIdx.x; x < total; x += (long)gridDim.x * 256) {
        const long b = x / (K + 1);
        const int c = (int)(x - b * (K + 1));
        grad[x] = (c >= 1 && c <= K - 1) ? u * g[b * (K - 1) + c - 1] : 0.f;
    }
}

// ------------------------------------------------------------------------------------------------ fractions
// Inclusive / suffix sums over aligned groups of G lanes (Hillis-Steele: a fixed order).
template <int G> __device__ __forceinline__ float group_scan(float x, int gl) {
#pragma unroll
    for (int d = 1; d < G; d <<= 1) {
        const float t = __shfl_up(x, d, G);
        if (gl >= d) x += t;
    }
    return x;
}
// Running maximum over the group: the sums of a parallel scan are each within rounding of the exact prefix sum but need not be
// ordered among themselves (lane k and lane k + 1 add in different trees); the fractions must not decrease.
template <int G> __device__ __forceinline__ float group_scan_max(float x, int gl) {
#pragma unroll
    for (int d = 1; d < G; d <<= 1) {
        const float t = __shfl_up(x, d, G);
        if (gl >= d) x = fmaxf(x, t);
    }
    return x;
}
template <int G> __device__ __forceinline__ float group_suffix(float x, int gl) {
#pragma unroll
    for (int d = 1; d < G; d <<= 1) {
        const float t = __shfl_down(x, d, G);
        if (gl + d < G) x += t;
    }
    return x;
}

// K <= G: a row per group of G lanes.  p = softmax(x), logp = log_softmax(x); a logit of -inf has p = 0 and adds exactly 0 to H.
template <int G>
__global__ __launch_bounds__(256) void fqf_fractions_fwd_group_kernel(const float* __restrict__ logits, float* __restrict__ quant,
                                                                      float* __restrict__ hats, float* __restrict__ ent, int B,
                                                                      int K) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, gl = lane % G, gs = lane / G;
    const long b = ((long)blockIdx.x * 4 + w) * (64 / G) + gs;
    const bool ok = b < (long)B, live = ok && gl < K;
    const float x = live ? logits[(size_t)b * K + gl] : -INFINITY;
    const float m = group_max<G>(x);
    const float e = live ? expf(x - m) : 0.f;
    const float s = hpc_rll::group_sum<G>(e);
    const float p = e / s, logp = (x - m) - logf(s);
    const float h = hpc_rll::group_sum<G>(p > 0.f ? -logp * p : 0.f);
    const float inc = group_scan_max<G>(group_scan<G>(p, gl), gl);
    const float up = __shfl_up(inc, 1, G);
    const float exc = gl == 0 ? 0.f : up;
    if (live) {
        quant[(size_t)b * (K + 1) + gl + 1] = inc;
        hats[(size_t)b * K + gl] = 0.5f * (exc + inc);
    }
    if (ok && gl == 0) {
        quant[(size_t)b * (K + 1)] = 0.f;
        ent[b] = h;
    }
}

// 64 < K <= 1024: a wave per row, the row in registers (chunk c = elements 64 c + lane), the scan carried from chunk to chunk
__global__ __launch_bounds__(256) void fqf_fractions_fwd_wave_kernel(const float* __restrict__ logits, float* __restrict__ quant,
                                                                     float* __restrict__ hats, float* __restrict__ ent, int B,
                                                                     int K) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long b = (long)blockIdx.x * 4 + wv;
    if (b >= (long)B) return;   // wave-uniform; the kernel has no workgroup barrier
    const int nch = (K + 63) >> 6;
    float x[kMaxChunks], e[kMaxChunks];
    float m = -INFINITY;
#pragma unroll
    for (int c = 0; c < kMaxChunks; ++c) {
        const int i = c * 64 + lane;
        x[c] = (c < nch && i < K) ? logits[(size_t)b * K + i] : -INFINITY;
        m = fmaxf(m, x[c]);
    }
    m = wave_max(m);
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < kMaxChunks; ++c) {
        e[c] = (c * 64 + lane < K) ? expf(x[c] - m) : 0.f;
        s += e[c];
    }
    s = wave_sum(s);
    const float logs = logf(s);
    float carry = 0.f, h = 0.f;
#pragma unroll
    for (int c = 0; c < kMaxChunks; ++c) {
        if (c < nch) {   // wave-uniform
            const int i = c * 64 + lane;
            const float p = e[c] / s, logp = (x[c] - m) - logs;
            h += p > 0.f ? -logp * p : 0.f;
            const float inc = fmaxf(group_scan_max<64>(group_scan<64>(p, lane) + carry, lane), carry);
            const float up = __shfl_up(inc, 1, 64);
            const float exc = lane == 0 ? carry : up;
            if (i < K) {
                quant[(size_t)b * (K + 1) + i + 1] = inc;
                hats[(size_t)b * K + i] = 0.5f * (exc + inc);
            }
            carry = __shfl(inc, 63, 64);
        }
    }
    h = wave_sum(h);
    if (lane == 0) {
        quant[(size_t)b * (K + 1)] = 0.f;
        ent[b] = h;
    }
}

// glogit_k = p_k (gp_k - sum_j p_j gp_j) - gH p_k (logp_k + H), gp the suffix sum of the quantile gradients; an absent upstream
// gradient counts as zero, a column with p = 0 gets exactly 0 from the entropy term.  The callers pass gp CENTRED on its value at
// the largest logit: since sum_j p_j = 1 that changes nothing in exact arithmetic, but when one fraction holds nearly all the
// mass (p = 1 in fp32) the difference gp_k - sum_j p_j gp_j of the uncentred form cancels to 0 where the true value, the
// negative sum of the other columns, is the largest entry of the row.
__device__ __forceinline__ float fractions_grad(float p, float logp, float gp, float dot, float gH, float H) {
    return p * (gp - dot) - (p > 0.f ? gH * p * (logp + H) : 0.f);
}

template <int G>
__global__ __launch_bounds__(256) void fqf_fractions_bwd_group_kernel(const float* __restrict__ logits, const float* __restrict__ ent,
                                                                      const float* __restrict__ gq, const float* __restrict__ gh,
                                                                      float* __restrict__ grad, int B, int K) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, gl = lane % G, gs = lane / G;
    const long b = ((long)blockIdx.x * 4 + w) * (64 / G) + gs;
    const bool ok = b < (long)B, live = ok && gl < K;
    const float x = live ? logits[(size_t)b * K + gl] : -INFINITY;
    const float gt = (gq && live) ? gq[(size_t)b * (K + 1) + gl + 1] : 0.f;
    const float gH = (gh && ok) ? gh[b] : 0.f, H = ok ? ent[b] : 0.f;
    const float m = group_max<G>(x);
    const float e = live ? expf(x - m) : 0.f;
    const float s = hpc_rll::group_sum<G>(e);
    const float p = e / s, logp = (x - m) - logf(s);
    // centred on the suffix sum at the (first) largest logit: see fractions_grad
    int at = (live && x == m) ? gl : G;
#pragma unroll
    for (int d = G / 2; d >= 1; d >>= 1) at = min(at, __shfl_xor(at, d, 64));
    const float sfx = group_suffix<G>(gt, gl);
    const float gp = sfx - __shfl(sfx, (lane - gl) + (at < G ? at : 0), 64);
    const float dot = hpc_rll::group_sum<G>(p * gp);
    if (live) grad[(size_t)b * K + gl] = fractions_grad(p, logp, gp, dot, gH, H);
}

__global__ __launch_bounds__(256) void fqf_fractions_bwd_wave_kernel(const float* __restrict__ logits, const float* __restrict__ ent,
                                                                     const float* __restrict__ gq, const float* __restrict__ gh,
                                                                     float* __restrict__ grad, int B, int K) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long b = (long)blockIdx.x * 4 + wv;
    if (b >= (long)B) return;   // wave-uniform; the kernel has no workgroup barrier
    const int nch = (K + 63) >> 6;
    float x[kMaxChunks], e[kMaxChunks], gp[kMaxChunks];
    float m = -INFINITY;
#pragma unroll
    for (int c = 0; c < kMaxChunks; ++c) {
        const int i = c * 64 + lane;
        const bool in = c < nch && i < K;
        x[c] = in ? logits[(size_t)b * K + i] : -INFINITY;
        gp[c] = (gq && in) ? gq[(size_t)b * (K + 1) + i + 1] : 0.f;
        m = fmaxf(m, x[c]);
    }
    const float gH = gh ? gh[b] : 0.f, H = ent[b];
    m = wave_max(m);
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < kMaxChunks; ++c) {
        e[c] = (c * 64 + lane < K) ? expf(x[c] - m) : 0.f;
        s += e[c];
    }
    s = wave_sum(s);
    const float logs = logf(s);
    float carry = 0.f, dot = 0.f;
    int at = INT_MAX;
#pragma unroll
    for (int c = kMaxChunks - 1; c >= 0; --c) {
        if (c < nch) {   // wave-uniform: the suffix sums run from the last chunk down
            gp[c] = group_suffix<64>(gp[c], lane) + carry;
            carry = __shfl(gp[c], 0, 64);
            if (c * 64 + lane < K && x[c] == m) at = c * 64 + lane;   // descending c: the first index of the largest logit stays
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) at = min(at, __shfl_xor(at, d, 64));
    if (at == INT_MAX) at = 0;   // a row without a largest logit (NaN): nothing to centre on
    float centre = 0.f;
#pragma unroll
    for (int c = 0; c < kMaxChunks; ++c)
        if (c == (at >> 6)) centre = gp[c];   // wave-uniform
    centre = __shfl(centre, at & 63, 64);
#pragma unroll
    for (int c = 0; c < kMaxChunks; ++c) {
        gp[c] -= centre;
        dot = fmaf(e[c] / s, gp[c], dot);   // e = 0 past the row
    }
    dot = wave_sum(dot);
#pragma unroll
    for (int c = 0; c < kMaxChunks; ++c) {
        const int i = c * 64 + lane;
        if (c < nch && i < K) grad[(size_t)b * K + i] = fractions_grad(e[c] / s, (x[c] - m) - logs, gp[c], dot, gH, H);
    }
}

// ------------------------------------------------------------------------------------------------ expected value
// logit[b,n] = sum_i (quantiles[b,i+1] - quantiles[b,i]) q[b,i,n].  A sample on G lanes, lane gl owns the columns gl, gl + G, ..
// of V floats each (V = 4: 16-byte loads); the widths of 64 fractions at a time are staged in the wave's LDS slot and read back
// as broadcasts.  ARGMAX: the lanes keep their best column, the group reduces with ties to the lowest index.
template <int G, int V, bool ARGMAX>
__global__ __launch_bounds__(256) void fqf_q_value_kernel(const float* __restrict__ q, const float* __restrict__ quant,
                                                          float* __restrict__ logit, int64_t* __restrict__ act, int B, int K,
                                                          int N) {
    constexpr int SPW = 64 / G;
    __shared__ float wid[4][SPW][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, gl = lane % G, gs = lane / G;
    const long b = ((long)blockIdx.x * 4 + w) * SPW + gs;
    const bool ok = b < (long)B;
    const long bb = ok ? b : (long)B - 1;   // clamped: every load is unconditional, the stores are guarded
    const int NC = N / V;
    float best = -INFINITY;
    int besti = INT_MAX;
    for (int c0 = 0; c0 < NC; c0 += G) {   // wave-uniform trip count
        const int c = c0 + gl;
        const bool cok = c < NC;
        const float* __restrict__ qc = q + (size_t)bb * K * N + (size_t)(cok ? c : NC - 1) * V;
        Pack<V> acc;
#pragma unroll
        for (int k = 0; k < V; ++k) acc.v[k] = 0.f;
        for (int k0 = 0; k0 < K; k0 += 64) {
            const int kt = K - k0 < 64 ? K - k0 : 64;
            __builtin_amdgcn_wave_barrier();   // the slot's previous tile has been read (one wave: LDS operations run in order)
            for (int i = gl; i < kt; i += G) {
                const float* __restrict__ t = quant + (size_t)bb * (K + 1) + k0 + i;
                wid[w][gs][i] = t[1] - t[0];
            }
            __builtin_amdgcn_wave_barrier();
#pragma unroll 4
            for (int i = 0; i < kt; ++i) {
                const Pack<V> v = load_pack<V>(qc + (size_t)(k0 + i) * N);
                const float wi = wid[w][gs][i];
#pragma unroll
                for (int k = 0; k < V; ++k) acc.v[k] = fmaf(wi, v.v[k], acc.v[k]);
            }
        }
        if (ok && cok) store_pack<V>(logit + (size_t)b * N + (size_t)c * V, acc);
        if (ARGMAX && cok) {
#pragma unroll
            for (int k = 0; k < V; ++k)
                if (besti == INT_MAX || acc.v[k] > best) {
                    best = acc.v[k];
                    besti = c * V + k;
                }
        }
    }
    if (ARGMAX) {
#pragma unroll
        for (int m = G / 2; m >= 1; m >>= 1) {
            const float ob = __shfl_xor(best, m, 64);
            const int oi = __shfl_xor(besti, m, 64);
            if (oi != INT_MAX && (besti == INT_MAX || ob > best || (ob == best && oi < besti))) {
                best = ob;
                besti = oi;
            }
        }
        if (ok && gl == 0) act[b] = (int64_t)besti;
    }
}

// ------------------------------------------------------------------------------------------------ host side
// The launch record (hpc_rll_fqf_last_config): one part per launch kind, noted beside the launch with the template arguments OF
// THAT LAUNCH.
LaunchRecord<HPC_RLL_FQF_PART_INTS> g_fqf_last[HPC_RLL_FQF_LAUNCHES];
void fqf_note(int kind, int family, int g, long grid, bool folded, int vec) {
    g_fqf_last[kind].note({family, g, (int)grid, folded ? 1 : 0, vec});
}

inline bool f4(const void* p) { return aligned(p, 4); }
inline bool i8(const void* p) { return aligned(p, 8); }
inline bool vec16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline long stream_blocks(long threads) {
    long blocks = (threads + 255) / 256;
    return blocks > 8192 ? 8192 : blocks < 1 ? 1 : blocks;
}

}  // namespace
}  // namespace hpc_rll

using namespace hpc_rll;

extern "C" int hpc_rll_fqf_nstep_td_forward(const float* q, const float* next_n_q, const int64_t* action,
                                            const int64_t* next_n_action, const float* reward, const float* done,
                                            const float* quantiles_hats, const float* weight, const float* value_gamma,
                                            float* loss, float* td_err, float* buf, float* partials, int K, int K_prime,
                                            int nstep, int B, int N, float gamma, float kappa, float scale, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (K <= 0 || K_prime <= 0 || N <= 0 || B < 0 || nstep < 0 || !(kappa > 0.f) || !loss) return HPC_RLL_EINVAL;
    if (B > 0 && (!q || !next_n_q || !action || !next_n_action || (nstep && !reward) || !done || !quantiles_hats || !td_err ||
                  !buf || !partials))
        return HPC_RLL_EINVAL;
    if (!f4(q) || !f4(next_n_q) || !f4(reward) || !f4(done) || !f4(quantiles_hats) || !f4(weight) || !f4(value_gamma) ||
        !f4(loss) || !f4(td_err) || !f4(buf) || !f4(partials))
        return HPC_RLL_EALIGN;
    if (!i8(action) || !i8(next_n_action)) return HPC_RLL_EALIGN;
    if (B == 0) return (int)hipMemsetAsync(loss, 0, sizeof(float), st);
    const float gamma_n = gamma_pow(gamma, nstep);
    const int gmax = K > K_prime ? K : K_prime;
    const int G = group_lanes(gmax), spb = gmax <= 64 ? 4 * (64 / G) : 4;
    const long blocks = ((long)B + spb - 1) / spb;
    return launch_folded(blocks, 1, &scale, loss, partials, st, [&](unsigned grid, const ScanFold& fold) {
        if (gmax <= 64)
            return with_width(G, [&](auto G_) {
                constexpr int GG = G_;
                hipLaunchKernelGGL(fqf_td_fwd_group_kernel<GG>, dim3(grid), dim3(256), 0, st, q, next_n_q, action, next_n_action,
                                   reward, done, quantiles_hats, weight, value_gamma, td_err, buf, partials, K, K_prime, nstep, B,
                                   N, gamma, gamma_n, kappa, scale, fold);
                fqf_note(HPC_RLL_FQF_LAUNCH_TD_FORWARD, HPC_RLL_FQF_FAMILY_GROUP, GG, blocks, fold.out, 1);
                return last_error();
            });
        hipLaunchKernelGGL(fqf_td_fwd_wave_kernel, dim3(grid), dim3(256), 0, st, q, next_n_q, action, next_n_action, reward, done,
                           quantiles_hats, weight, value_gamma, td_err, buf, partials, K, K_prime, nstep, B, N, gamma, gamma_n,
                           kappa, scale, fold);
        fqf_note(HPC_RLL_FQF_LAUNCH_TD_FORWARD, HPC_RLL_FQF_FAMILY_WAVE, 64, blocks, fold.out, 1);
        return last_error();
    });
}

extern "C" int hpc_rll_fqf_nstep_td_backward(const float* grad_loss, const float* buf, const int64_t* action, float* grad_q,
                                             int K, int B, int N, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (K <= 0 || B < 0 || N <= 0) return HPC_RLL_EINVAL;
    if (B > 0 && (!grad_loss || !buf || !action || !grad_q)) return HPC_RLL_EINVAL;
    if (!f4(grad_loss) || !f4(buf) || !f4(grad_q) || !i8(action)) return HPC_RLL_EALIGN;
    if ((long)B * K >= (1L << 31)) return HPC_RLL_EUNSUPPORTED;   // rows are counted in 32 bits (buf alone would hold 8 GB)
    if (B == 0) return HPC_RLL_OK;
    const bool v4 = N % 4 == 0 && vec16(grad_q);
    const unsigned rows = (unsigned)((long)B * K), NC = (unsigned)(v4 ? N / 4 : N), RPB = NC >= 256 ? 1 : 256 / NC;
    long blocks = ((long)rows + RPB - 1) / RPB;
    if (blocks > 32768) blocks = 32768;   // the workgroups loop
    auto run = [&](auto kernel, int vec) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, st, grad_loss, buf, action, grad_q, (unsigned)K, rows, N,
                           NC, RPB);
        fqf_note(HPC_RLL_FQF_LAUNCH_TD_BACKWARD, HPC_RLL_FQF_FAMILY_STREAM, 0, blocks, false, vec);
        return last_error();
    };
    return v4 ? run(fqf_td_bwd_kernel<4>, 4) : run(fqf_td_bwd_kernel<1>, 1);
}

extern "C" int hpc_rll_fqf_fraction_loss_forward(const float* q_tau_i, const float* q_value, const float* quantiles,
                                                 const int64_t* action, float* loss, float* g, float* partials, int K, int B,
                                                 int N, float scale, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (K <= 0 || N <= 0 || B < 0 || !loss) return HPC_RLL_EINVAL;
    // K = 1 has no inner fraction: q_tau_i and g are empty and may be null
    if (B > 0 && (!q_value || !quantiles || !action || !partials || (K > 1 && (!q_tau_i || !g)))) return HPC_RLL_EINVAL;
    if (!f4(q_tau_i) || !f4(q_value) || !f4(quantiles) || !f4(loss) || !f4(g) || !f4(partials)) return HPC_RLL_EALIGN;
    if (!i8(action)) return HPC_RLL_EALIGN;
    if (B == 0) return (int)hipMemsetAsync(loss, 0, sizeof(float), st);
    const int G = group_lanes(K), spb = K <= 64 ? 4 * (64 / G) : 4;
    const long blocks = ((long)B + spb - 1) / spb;
    return launch_folded(blocks, 1, &scale, loss, partials, st, [&](unsigned grid, const ScanFold& fold) {
        if (K <= 64)
            return with_width(G, [&](auto G_) {
                constexpr int GG = G_;
                hipLaunchKernelGGL(fqf_fraction_loss_fwd_group_kernel<GG>, dim3(grid), dim3(256), 0, st, q_tau_i, q_value,
                                   quantiles, action, g, partials, K, B, N, fold);
                fqf_note(HPC_RLL_FQF_LAUNCH_FRACTION_LOSS_FORWARD, HPC_RLL_FQF_FAMILY_GROUP, GG, blocks, fold.out, 1);
                return last_error();
            });
        hipLaunchKernelGGL(fqf_fraction_loss_fwd_wave_kernel, dim3(grid), dim3(256), 0, st, q_tau_i, q_value, quantiles, action, g,
                           partials, K, B, N, fold);
        fqf_note(HPC_RLL_FQF_LAUNCH_FRACTION_LOSS_FORWARD, HPC_RLL_FQF_FAMILY_WAVE, 64, blocks, fold.out, 1);
        return last_error();
    });
}

extern "C" int hpc_rll_fqf_fraction_loss_backward(const float* grad_loss, const float* g, float* grad_quantiles, int K, int B,
                                                  float scale, void* stream) {
    if (K <= 0 || B < 0) return HPC_RLL_EINVAL;
    if (B > 0 && (!grad_loss || !grad_quantiles || (K > 1 && !g))) return HPC_RLL_EINVAL;
    if (!f4(grad_loss) || !f4(g) || !f4(grad_quantiles)) return HPC_RLL_EALIGN;
    if (B == 0) return HPC_RLL_OK;
    const long total = (long)B * (K + 1), blocks = stream_blocks(total);
    hipLaunchKernelGGL(fqf_fraction_loss_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, grad_loss, g,
                       grad_quantiles, K, total, scale);
    fqf_note(HPC_RLL_FQF_LAUNCH_FRACTION_LOSS_BACKWARD, HPC_RLL_FQF_FAMILY_STREAM, 0, blocks, false, 1);
    return last_error();
}

extern "C" int hpc_rll_fqf_fractions_forward(const float* logits, float* quantiles, float* quantiles_hats, float* entropies,
                                             int B, int K, void* stream) {
    if (K <= 0 || B < 0) return HPC_RLL_EINVAL;
    if (B > 0 && (!logits || !quantiles || !quantiles_hats || !entropies)) return HPC_RLL_EINVAL;
    if (!f4(logits) || !f4(quantiles) || !f4(quantiles_hats) || !f4(entropies)) return HPC_RLL_EALIGN;
    if (K > kFractionsMaxK) return HPC_RLL_EUNSUPPORTED;
    if (B == 0) return HPC_RLL_OK;
    hipStream_t st = (hipStream_t)stream;
    const int G = group_lanes(K), rpb = K <= 64 ? 4 * (64 / G) : 4;
    const long blocks = ((long)B + rpb - 1) / rpb;
    if (K <= 64)
        return with_width(G, [&](auto G_) {
            constexpr int GG = G_;
            hipLaunchKernelGGL(fqf_fractions_fwd_group_kernel<GG>, dim3((unsigned)blocks), dim3(256), 0, st, logits, quantiles,
                               quantiles_hats, entropies, B, K);
            fqf_note(HPC_RLL_FQF_LAUNCH_FRACTIONS_FORWARD, HPC_RLL_FQF_FAMILY_GROUP, GG, blocks, false, 1);
            return last_error();
        });
    hipLaunchKernelGGL(fqf_fractions_fwd_wave_kernel, dim3((unsigned)blocks), dim3(256), 0, st, logits, quantiles, quantiles_hats,
                       entropies, B, K);
    fqf_note(HPC_RLL_FQF_LAUNCH_FRACTIONS_FORWARD, HPC_RLL_FQF_FAMILY_WAVE, 64, blocks, false, 1);
    return last_error();
}

extern "C" int hpc_rll_fqf_fractions_backward(const float* logits, const float* entropies, const float* grad_quantiles,
                                              const float* grad_entropies, float* grad_logits, int B, int K, void* stream) {
    if (K <= 0 || B < 0) return HPC_RLL_EINVAL;
    if (B > 0 && (!logits || !entropies || !grad_logits)) return HPC_RLL_EINVAL;   // either upstream gradient may be absent
    if (!f4(logits) || !f4(entropies) || !f4(grad_quantiles) || !f4(grad_entropies) || !f4(grad_logits)) return HPC_RLL_EALIGN;
    if (K > kFractionsMaxK) return HPC_RLL_EUNSUPPORTED;
    if (B == 0) return HPC_RLL_OK;
    hipStream_t st = (hipStream_t)stream;
    const int G = group_lanes(K), rpb = K <= 64 ? 4 * (64 / G) : 4;
    const long blocks = ((long)B + rpb - 1) / rpb;
    if (K <= 64)
        return with_width(G, [&](auto G_) {
            constexpr int GG = G_;
            hipLaunchKernelGGL(fqf_fractions_bwd_group_kernel<GG>, dim3((unsigned)blocks), dim3(256), 0, st, logits, entropies,
                               grad_quantiles, grad_entropies, grad_logits, B, K);
            fqf_note(HPC_RLL_FQF_LAUNCH_FRACTIONS_BACKWARD, HPC_RLL_FQF_FAMILY_GROUP, GG, blocks, false, 1);
            return last_error();
        });
    hipLaunchKernelGGL(fqf_fractions_bwd_wave_kernel, dim3((unsigned)blocks), dim3(256), 0, st, logits, entropies, grad_quantiles,
                       grad_entropies, grad_logits, B, K);
    fqf_note(HPC_RLL_FQF_LAUNCH_FRACTIONS_BACKWARD, HPC_RLL_FQF_FAMILY_WAVE, 64, blocks, false, 1);
    return last_error();
}

extern "C" int hpc_rll_fqf_q_value(const float* q, const float* quantiles, float* logit, int64_t* action, int B, int K, int N,
                                   void* stream) {
    if (K <= 0 || N <= 0 || B < 0) return HPC_RLL_EINVAL;
    if (B > 0 && (!q || !quantiles || !logit)) return HPC_RLL_EINVAL;   // action == NULL: no argmax
    if (!f4(q) || !f4(quantiles) || !f4(logit) || !i8(action)) return HPC_RLL_EALIGN;
    if (B == 0) return HPC_RLL_OK;
    hipStream_t st = (hipStream_t)stream;
    const bool v4 = N % 4 == 0 && vec16(q) && vec16(logit);
    const int G = group_lanes(v4 ? N / 4 : N);
    const long blocks = ((long)B + 4 * (64 / G) - 1) / (4 * (64 / G));
    return with_width(G, [&](auto G_) { return with_bool(v4, [&](auto V4_) { return with_bool(action != nullptr, [&](auto AM_) {
        constexpr int GG = G_, V = decltype(V4_)::value ? 4 : 1;
        constexpr bool AM = AM_;
        hipLaunchKernelGGL((fqf_q_value_kernel<GG, V, AM>), dim3((unsigned)blocks), dim3(256), 0, st, q, quantiles, logit, action, B,
                           K, N);
        fqf_note(HPC_RLL_FQF_LAUNCH_Q_VALUE, AM ? HPC_RLL_FQF_FAMILY_STREAM_ARGMAX : HPC_RLL_FQF_FAMILY_STREAM, GG, blocks, false, V);
        return last_error();
    }); }); });
}

extern "C" int hpc_rll_fqf_last_config(int* out) {
    if (!out) return HPC_RLL_EINVAL;
    for (int k = 0; k < HPC_RLL_FQF_LAUNCHES; ++k) g_fqf_last[k].read(out + k * HPC_RLL_FQF_PART_INTS);
    return HPC_RLL_OK;
}
