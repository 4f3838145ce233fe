// tqc.hip -- Truncated Quantile Critics (Kuznetsov et al. 2020) on gfx950: the critic loss with the atom selection inside the
// kernel, and the actor loss over the critics' quantiles.  TQC is SAC whose critics are ensembles of quantile heads; the head
// (tanh_gaussian_rsample) and the temperature loss (sac_alpha_loss) are those of continuous SAC.
//
// No reference counterpart; the semantics restate the authors' implementation (the mean over all four axes).
//
// The critic loss.  z (B,M,N) the online critics' quantiles, target_z (B,M',N') the target critics', n = M' N' pooled atoms per
// sample, K = n - drop of them kept; k = 1 - done, w = weight.  Per sample b:
//   s_(0) <= ... <= s_(n-1)   the pooled atoms in the total order of their bits (-0 < +0, every NaN above +inf, ties by index)
//   y_j   = reward + gamma k (s_(j) - alpha next_log_prob)        j < K                       -> target_atoms (B,K)
//   tau_i = (2 i + 1) / (2 N),   e = y_j - z[m,i],   rho = |tau_i - 1{e < 0}| huber_kappa(e) / kappa
//   td_b  = sum_{m,i,j} rho / (M N K)                                                         -> td_error (B)
//   loss  = scale sum_b w_b td_b
//   grad_unit[b,m,i] = -scale w_b / (M N K) sum_j |tau_i - 1{e < 0}| clamp(e, -kappa, kappa) / kappa,   grad_z = g grad_unit
//
// One wave64 per sample, four samples per 256-thread workgroup, at most kFoldMaxGrid workgroups which loop.  A wave owns two
// LDS slices of R*64 words (R = ceil(n/64), a template argument): `keys` and `kept`.  Three phases per sample:
//   1. load and rank.  The wave loads the pooled row (16-byte loads when every float operand of the launch lies on 16 bytes and
//      n % 4 == 0, 4-byte loads otherwise), turns each atom into a sortable integer key (sign-magnitude bits -> unsigned order;
//      a NaN -> the largest key) and writes it to `keys`; the slots from n up to R*64 get the largest key.  Lane l then owns atoms
//      l, l + 64, ... (R of them, in registers) and counts, for each, the atoms that precede it: it walks `keys` with same-address
//      16-byte reads (a broadcast: no bank conflict) and compares (key, index) pairs as 64-bit integers.  The count is the atom's
//      rank and the ranks are a permutation of 0 .. n-1: n R compares per lane (250 at the defaults n = 125, R = 2).
//   2. counting-sort scatter.  An atom of rank < K writes y to kept[rank]; the others write nothing.  `kept` is now the sorted,
//      truncated target; the wave streams it out as target_atoms[b,:], coalesced.
//   3. pair loop.  Lane l owns the online quantiles l, l + 64, ... of the flattened (M,N) row, four at a time, each with its
//      tau and the hoisted weights |tau| / kappa and |tau - 1| / kappa.  It walks kept[0..K) with same-address 16-byte reads,
//      four targets per read, the K % 4 tail with 4-byte reads (nothing past K is read: those slots hold nothing).  Per pair,
//      as quantile_huber_group does: dh = med3(e, -kappa, kappa), hub = dh (e - dh/2), the weight picked by the sign of e, two
//      accumulators (even and odd targets) per quantile and sum.  About 6 vector instructions per pair: 2 x 115 pairs = 1 400
//      per lane at the defaults, against 250 compare steps of phase 1.  The lane stores grad_unit, the wave sums td_b with the
//      DPP butterfly of wave.hpp.
// The slices are private to their wave: a wave's LDS operations execute in order, so the phases are separated by
// __builtin_amdgcn_wave_barrier() (a compiler fence, no instruction) and there is no __syncthreads() before the sums' epilogue.
// The loss leaves through publish_wave_sums (per-workgroup partials, the last workgroup folds them in a fixed order: no float
// atomics, the same bits from run to run).  No matrix instructions: a pair is compare-select, it does not factor into a product.
// This file is compiled without packed-fp32 instructions (build.py): the two-wide form below is the source form only.
//
// The backward is reduce.hip's scale_rows: grad_z = g grad_unit, one streaming launch.
//
// The actor loss.  log_prob (B), new_z (B,M,N) the online critics at the freshly sampled action:
//   policy = scale sum_b (alpha log_prob_b - mean_{m,i} new_z[b,m,i]),   entropy = -scale sum_b log_prob_b
//   grad_log_prob = g alpha scale,   grad_new_z = -g scale / (M N)
// A wave per row, 16-byte loads of new_z where the rows allow, the DPP sum, the same fold; the backward fills both gradients.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "colscan.hpp"
#include "dist_shared.hpp"
#include "hostutil.hpp"
#include "hpc_rll_hip.h"
#include "rowgroup.hpp"
#include "wave.hpp"

namespace hpc_rll {
namespace {

constexpr int kTqcMaxAtoms = 1024;                          // of the pooled target row and of the online row alike
constexpr int64_t kTqcPartials = 2 * kFoldMaxGrid + 8;      // floats of ws ahead of grad_unit: the partial sums, two constants
constexpr int64_t kTqcConsts = 2 * kFoldMaxGrid;            // (alpha scale, scale / (M N)) of the actor loss
static_assert(kTqcPartials % 4 == 0, "grad_unit keeps the alignment of ws");
constexpr unsigned kTopKey = 0xFFFFFFFFu;

struct TqcArgs {
    const float* z; const float* tz; const float* nlp; const float* reward; const void* done; int done_f32;
    const float* weight; const float* alpha_dev; float alpha;
    float* td_error; float* target_atoms; float* grad_unit; long rows; int MN, N, n, K; float gamma, kappa, scale;
};

// the bits of a float in an order that unsigned integers share: negative values reversed below the positive ones (so that
// -0 < +0), every NaN on top; and back (the largest key reads as a NaN)
__device__ __forceinline__ unsigned sort_key(float x) {
    const unsigned u = __float_as_uint(x);
    return x != x ? kTopKey : (u & 0x80000000u) ? ~u : u | 0x80000000u;
}
__device__ __forceinline__ float key_value(unsigned k) { return __uint_as_float((k & 0x80000000u) ? k & 0x7FFFFFFFu : ~k); }

// Two targets (an even and an odd one: the two halves of the accumulators) against the NJ quantiles of a lane
template <int NJ>
__device__ __forceinline__ void pair2(const vfloat2 t, const float (&zq)[NJ], const float (&qneg)[NJ], const float (&qpos)[NJ],
                                      float kappa, vfloat2 (&li)[NJ], vfloat2 (&gi)[NJ]) {
    const vfloat2 mh2 = {-0.5f, -0.5f};
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const vfloat2 q2 = {zq[j], zq[j]};
        const vfloat2 e = t - q2;
        vfloat2 dh, qw;
        dh.x = __builtin_amdgcn_fmed3f(e.x, -kappa, kappa);
        dh.y = __builtin_amdgcn_fmed3f(e.y, -kappa, kappa);
        const vfloat2 hub = dh * __builtin_elementwise_fma(mh2, dh, e);
        qw.x = e.x < 0.f ? qneg[j] : qpos[j];
        qw.y = e.y < 0.f ? qneg[j] : qpos[j];
        li[j] = __builtin_elementwise_fma(qw, hub, li[j]);
        gi[j] = __builtin_elementwise_fma(qw, dh, gi[j]);
    }
}

// The pair loop of the online quantiles q0 + j*64 + lane, j < NJ, against kept[0..K): stores their grad_unit and returns the
// lane's part of sum rho.  A quantile past MN takes part with z = 0 and is left out of both.
template <int NJ>
__device__ __forceinline__ float pair_pass(const float* kept, int K, const float* __restrict__ zrow, float* __restrict__ gurow,
                                           int q0, int MN, int N, int lane, float kappa, float gscale) {
    float zq[NJ], qneg[NJ], qpos[NJ];
    vfloat2 li[NJ], gi[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int qi = q0 + j * 64 + lane;
        zq[j] = qi < MN ? zrow[qi] : 0.f;
        const float tau = (float)(2 * (qi % N) + 1) / (float)(2 * N);
        qneg[j] = fabsf(tau - 1.f) / kappa;
        qpos[j] = fabsf(tau) / kappa;
        li[j] = vfloat2{0.f, 0.f};
        gi[j] = vfloat2{0.f, 0.f};
    }
    const int K4 = K & ~3;
    for (int j0 = 0; j0 < K4; j0 += 4) {
        const vfloat4 t = *reinterpret_cast<const vfloat4*>(kept + j0);   // every lane reads the same 16 bytes: a broadcast
        pair2<NJ>(vfloat2{t.x, t.y}, zq, qneg, qpos, kappa, li, gi);
        pair2<NJ>(vfloat2{t.z, t.w}, zq, qneg, qpos, kappa, li, gi);
    }
    for (int jt = K4; jt < K; ++jt) {   // the K % 4 tail, one target at a time: the slots from K on hold nothing
        const float t = kept[jt];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const float e = t - zq[j];
            const float dh = __builtin_amdgcn_fmed3f(e, -kappa, kappa);
            const float qw = e < 0.f ? qneg[j] : qpos[j];
            li[j].x = fmaf(qw, dh * fmaf(-0.5f, dh, e), li[j].x);
            gi[j].x = fmaf(qw, dh, gi[j].x);
        }
    }
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int qi = q0 + j * 64 + lane;
        if (qi < MN) {
            sum += li[j].x + li[j].y;
            gurow[qi] = -(gi[j].x + gi[j].y) * gscale;   // de/dz = -1
        }
    }
    return sum;
}

// R: atoms per lane (R*64 >= n); V4: 16-byte loads of the pooled row (n % 4 == 0, the row on 16 bytes)
template <int R, bool V4>
__global__ __launch_bounds__(256) void tqc_critic_fwd_kernel(const TqcArgs p, float* __restrict__ partials,
                                                             const ScanFold fold) {
    constexpr int SLOTS = R * 64;
    __shared__ __attribute__((aligned(16))) unsigned s_keys[4][SLOTS];
    __shared__ __attribute__((aligned(16))) float s_kept[4][SLOTS];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    unsigned* keys = s_keys[wv];
    float* kept = s_kept[wv];
    const float alpha = p.alpha_dev ? p.alpha_dev[0] : p.alpha;
    const int n = p.n, K = p.K, MN = p.MN;
    const int n4 = (n + 3) & ~3;                 // <= SLOTS: the slots from n on hold the largest key
    const float inv_pairs = 1.f / ((float)MN * (float)K);
    float acc[1] = {0.f};
    for (long b = (long)blockIdx.x * 4 + wv; b < p.rows; b += (long)gridDim.x * 4) {
        // ---- 1. load the pooled row as keys
        const float* trow = p.tz + b * (long)n;
        if (V4) {
            constexpr int E = (SLOTS + 255) / 256;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const int i0 = (e * 64 + lane) * 4;
                if (i0 < SLOTS) {
                    uint4 k4 = {kTopKey, kTopKey, kTopKey, kTopKey};
                    if (i0 < n) {
                        const vfloat4 x = *reinterpret_cast<const vfloat4*>(trow + i0);
                        k4 = uint4{sort_key(x.x), sort_key(x.y), sort_key(x.z), sort_key(x.w)};
                    }
                    *reinterpret_cast<uint4*>(keys + i0) = k4;
                }
            }
        } else {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int i = r * 64 + lane;
                keys[i] = i < n ? sort_key(trow[i]) : kTopKey;
            }
        }
        __builtin_amdgcn_wave_barrier();   // one wave, its own slice: the LDS operations run in order, no __syncthreads()
        // ---- the rank of each of this lane's atoms: how many (key, index) pairs precede it
        unsigned long long mine[R];
        int rank[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = r * 64 + lane;
            mine[r] = ((unsigned long long)keys[i] << 32) | (unsigned)i;
            rank[r] = 0;
        }
        for (int k0 = 0; k0 < n4; k0 += 4) {
            const uint4 k4 = *reinterpret_cast<const uint4*>(keys + k0);   // the same 16 bytes in every lane: a broadcast
            const unsigned long long o0 = ((unsigned long long)k4.x << 32) | (unsigned)k0,
                                     o1 = ((unsigned long long)k4.y << 32) | (unsigned)(k0 + 1),
                                     o2 = ((unsigned long long)k4.z << 32) | (unsigned)(k0 + 2),
                                     o3 = ((unsigned long long)k4.w << 32) | (unsigned)(k0 + 3);
#pragma unroll
            for (int r = 0; r < R; ++r)
                rank[r] += (int)(o0 < mine[r]) + (int)(o1 < mine[r]) + (int)(o2 < mine[r]) + (int)(o3 < mine[r]);
        }
        // ---- 2. the kept atoms, as targets, to their places
        const float nl = p.nlp[b], rew = p.reward[b], wt = p.weight ? p.weight[b] : 1.f;
        float keep = 1.f;
        if (p.done) {
            if (p.done_f32) keep = 1.f - static_cast<const float*>(p.done)[b];
            else keep = static_cast<const uint8_t*>(p.done)[b] ? 0.f : 1.f;
        }
        const float gk = p.gamma * keep;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = r * 64 + lane;
            if (i < n && rank[r] < K) kept[rank[r]] = fmaf(gk, fmaf(-alpha, nl, key_value((unsigned)(mine[r] >> 32))), rew);
        }
        __builtin_amdgcn_wave_barrier();   // kept[0..K) is written (the same wave, in order)
        float* trg = p.target_atoms + b * (long)K;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = r * 64 + lane;
            if (i < K) trg[i] = kept[i];
        }
        // ---- 3. every online quantile against every kept target
        const float* zrow = p.z + b * (long)MN;
        float* gurow = p.grad_unit + b * (long)MN;
        const float gscale = p.scale * wt * inv_pairs;
        float li = 0.f;
        for (int q0 = 0; q0 < MN; q0 += 256) {
            const int left = MN - q0;            // uniform: how many 64-quantile strips this pass has
            if (left > 128) li += pair_pass<4>(kept, K, zrow, gurow, q0, MN, p.N, lane, p.kappa, gscale);
            else if (left > 64) li += pair_pass<2>(kept, K, zrow, gurow, q0, MN, p.N, lane, p.kappa, gscale);
            else li += pair_pass<1>(kept, K, zrow, gurow, q0, MN, p.N, lane, p.kappa, gscale);
        }
        li = group_sum_last<64>(li);             // the wave's total in lane 63
        const float td = __shfl(li, 63, 64) * inv_pairs;
        if (lane == 0) p.td_error[b] = td;
        acc[0] = fmaf(wt, td, acc[0]);
        __builtin_amdgcn_wave_barrier();         // both slices are rewritten by the wave's next sample
    }
    publish_wave_sums<1>(acc, partials, fold);
}

// ================================================================================================
// the actor loss
// ================================================================================================
template <bool V4>
__global__ __launch_bounds__(256) void tqc_policy_fwd_kernel(const float* __restrict__ lp, const float* __restrict__ nz,
                                                             const float* __restrict__ alpha_dev, float alpha_host,
                                                             float* __restrict__ consts, long rows, int MN, float scale,
                                                             float* __restrict__ partials, const ScanFold fold) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const float alpha = alpha_dev ? alpha_dev[0] : alpha_host;
    const float inv = 1.f / (float)MN;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        consts[0] = alpha * scale;
        consts[1] = scale * inv;
    }
    float acc[2] = {0.f, 0.f};
    for (long b = (long)blockIdx.x * 4 + wv; b < rows; b += (long)gridDim.x * 4) {
        const float* row = nz + b * (long)MN;
        float s = 0.f;
        if (V4) {
            for (int i = lane * 4; i < MN; i += 256) {
                const vfloat4 x = *reinterpret_cast<const vfloat4*>(row + i);
                s += (x.x + x.y) + (x.z + x.w);
            }
        } else {
            for (int i = lane; i < MN; i += 64) s += row[i];
        }
        s = __shfl(group_sum_last<64>(s), 63, 64);
        const float l = lp[b];
        acc[0] += fmaf(alpha, l, -s * inv);
        acc[1] -= l;
    }
    publish_wave_sums<2>(acc, partials, fold);
}

// grad_lp (rows) = g consts[0]; grad_nz (n_z floats) = -g consts[1]; either may be NULL.  V4: grad_nz in 16-byte stores
template <bool V4>
__global__ __launch_bounds__(256) void tqc_policy_bwd_kernel(const float* __restrict__ g_policy, const float* __restrict__ consts,
                                                             float* __restrict__ grad_lp, float* __restrict__ grad_nz, long rows,
                                                             long n_z) {
    const float g = g_policy ? g_policy[0] : 1.f;
    const float glp = g * consts[0], gz = -(g * consts[1]);
    const long t = (long)blockIdx.x * 256 + threadIdx.x, stride = (long)gridDim.x * 256;
    if (grad_lp)
        for (long i = t; i < rows; i += stride) grad_lp[i] = glp;
    if (grad_nz) {
        if (V4) {
            const vfloat4 v = {gz, gz, gz, gz};
            for (long i = t; i < n_z / 4; i += stride) __builtin_nontemporal_store(v, reinterpret_cast<vfloat4*>(grad_nz) + i);
        } else {
            for (long i = t; i < n_z; i += stride) __builtin_nontemporal_store(gz, grad_nz + i);
        }
    }
}

// The dispatch records (hpc_rll_tqc_last_config): {launches so far, kernel id, R, load width, grid, flags} of the critic
// forward, the critic backward, the actor forward and the actor backward
constexpr int kLaunchInts = 6;
LaunchRecord<kLaunchInts> g_critic_fwd, g_critic_bwd, g_policy_fwd, g_policy_bwd;

template <class F> int with_atoms_per_lane(int n, F&& f) {
    const int r = (n + 63) / 64;
    if (r <= 1) return f(std::integral_constant<int, 1>{});
    if (r <= 2) return f(std::integral_constant<int, 2>{});
    if (r <= 4) return f(std::integral_constant<int, 4>{});
    if (r <= 8) return f(std::integral_constant<int, 8>{});
    return f(std::integral_constant<int, 16>{});
}

}  // namespace
}  // namespace hpc_rll

using namespace hpc_rll;

// ws (floats): the partial sums and the actor loss's two constants (kTqcPartials) | grad_unit (rows * MN)
extern "C" int64_t hpc_rll_tqc_workspace_floats(int64_t rows, int MN) {
    if (rows < 0 || MN < 0 || (MN > 0 && rows > (INT64_MAX - kTqcPartials) / MN)) return HPC_RLL_EINVAL;
    return kTqcPartials + rows * MN;
}

extern "C" int hpc_rll_tqc_critic_forward(const float* z, const float* target_z, const float* next_log_prob,
                                          const float* reward, const void* done, int mask_dtype, const float* weight,
                                          const float* alpha_dev, float alpha, float* loss, float* td_error,
                                          float* target_atoms, float* ws, int64_t rows, int M, int N, int Mt, int Nt, int drop,
                                          float gamma, float kappa, float scale, void* stream) {
    if (!loss) return HPC_RLL_EINVAL;
    if (rows > 0 && (!z || !target_z || !next_log_prob || !reward || !td_error || !target_atoms || !ws)) return HPC_RLL_EINVAL;
    if (rows < 0 || M <= 0 || N <= 0 || Mt <= 0 || Nt <= 0 || !(kappa > 0.f)) return HPC_RLL_EINVAL;
    if (mask_dtype != HPC_RLL_MASK_U8 && mask_dtype != HPC_RLL_MASK_F32) return HPC_RLL_EINVAL;
    const bool done_f32 = mask_dtype == HPC_RLL_MASK_F32;
    if (!aligned(z, 4) || !aligned(target_z, 4) || !aligned(next_log_prob, 4) || !aligned(reward, 4) ||
        !aligned(done, done_f32 ? 4 : 1) || !aligned(weight, 4) || !aligned(alpha_dev, 4) || !aligned(loss, 4) ||
        !aligned(td_error, 4) || !aligned(target_atoms, 4) || !aligned(ws, 4))
        return HPC_RLL_EALIGN;
    const long MN = (long)M * N, n = (long)Mt * Nt;
    if (MN > kTqcMaxAtoms || n > kTqcMaxAtoms) return HPC_RLL_EUNSUPPORTED;
    if (drop < 0 || drop >= n) return HPC_RLL_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (rows == 0) return (int)hipMemsetAsync(loss, 0, sizeof(float), st);
    // the rule of the other row kernels: the 16-byte variant only when every float operand of the launch lies on 16 bytes
    const bool v4 = n % 4 == 0 && aligned(z, 16) && aligned(target_z, 16) && aligned(next_log_prob, 16) && aligned(reward, 16) &&
                    (!done_f32 || aligned(done, 16)) && aligned(weight, 16) && aligned(td_error, 16) &&
                    aligned(target_atoms, 16) && aligned(ws, 16);
    const TqcArgs p{z, target_z, next_log_prob, reward, done, done_f32 ? 1 : 0, weight, alpha_dev, alpha, td_error, target_atoms,
                    ws + kTqcPartials, (long)rows, (int)MN, N, (int)n, (int)n - drop, gamma, kappa, scale};
    const int flags = (weight ? 1 : 0) | (done ? (done_f32 ? 4 : 2) : 0) | (alpha_dev ? 64 : 0);
    const float sc[1] = {scale};
    return with_atoms_per_lane((int)n, [&](auto R_) {
        constexpr int R = R_;
        return with_bool(v4, [&](auto V_) {
            constexpr bool V4 = V_;
            long grid = 0;
            const int rc = launch_rows_folded(rows, 4, 1, sc, loss, ws, st, &grid, [&](unsigned blocks, const ScanFold& fold) {
                hipLaunchKernelGGL((tqc_critic_fwd_kernel<R, V4>), dim3(blocks), dim3(256), 0, st, p, ws, fold);
            });
            if (grid) g_critic_fwd.note({1, R, V4 ? 4 : 1, (int)grid, flags});
            return rc;
        });
    });
}

extern "C" int hpc_rll_tqc_critic_backward(const float* g_loss, const float* ws, float* grad_z, int64_t rows, int M, int N,
                                           void* stream) {
    const bool empty = rows == 0 || !grad_z;
    if (!empty && (!g_loss || !ws)) return HPC_RLL_EINVAL;
    if (rows < 0 || M <= 0 || N <= 0) return HPC_RLL_EINVAL;
    if (!aligned(g_loss, 4) || !aligned(ws, 4) || !aligned(grad_z, 4)) return HPC_RLL_EALIGN;
    if ((long)M * N > kTqcMaxAtoms) return HPC_RLL_EUNSUPPORTED;
    if (empty) return HPC_RLL_OK;
    const long nz = (long)rows * M * N;
    const bool v4 = nz % 4 == 0 && aligned(ws, 16) && aligned(grad_z, 16);   // scale_rows' own rule
    const int rc = scale_rows(g_loss, ws + kTqcPartials, grad_z, nz, nz, (hipStream_t)stream);
    if (!rc) g_critic_bwd.note({2, 0, v4 ? 4 : 1, (int)std::min<long>(((v4 ? nz / 4 : nz) + 255) / 256, 4096), 0});
    return rc;
}

extern "C" int hpc_rll_tqc_policy_forward(const float* log_prob, const float* new_z, const float* alpha_dev, float alpha,
                                          float* out2, float* ws, int64_t rows, int MN, float scale, void* stream) {
    if (!out2) return HPC_RLL_EINVAL;
    if (rows > 0 && (!log_prob || !new_z || !ws)) return HPC_RLL_EINVAL;
    if (rows < 0 || MN <= 0) return HPC_RLL_EINVAL;
    if (!aligned(log_prob, 4) || !aligned(new_z, 4) || !aligned(alpha_dev, 4) || !aligned(out2, 4) || !aligned(ws, 4))
        return HPC_RLL_EALIGN;
    if (MN > kTqcMaxAtoms) return HPC_RLL_EUNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    if (rows == 0) return (int)hipMemsetAsync(out2, 0, 2 * sizeof(float), st);
    const bool v4 = MN % 4 == 0 && aligned(new_z, 16) && aligned(log_prob, 16);
    const float sc[2] = {scale, scale};
    return with_bool(v4, [&](auto V_) {
        constexpr bool V4 = V_;
        long grid = 0;
        const int rc = launch_rows_folded(rows, 4, 2, sc, out2, ws, st, &grid, [&](unsigned blocks, const ScanFold& fold) {
            hipLaunchKernelGGL((tqc_policy_fwd_kernel<V4>), dim3(blocks), dim3(256), 0, st, log_prob, new_z, alpha_dev, alpha,
                               ws + kTqcConsts, (long)rows, MN, scale, ws, fold);
        });
        if (grid) g_policy_fwd.note({3, 0, V4 ? 4 : 1, (int)grid, alpha_dev ? 64 : 0});
        return rc;
    });
}

extern "C" int hpc_rll_tqc_policy_backward(const float* g_policy, const float* ws, float* grad_log_prob, float* grad_new_z,
                                           int64_t rows, int MN, void* stream) {
    const bool empty = rows == 0 || (!grad_log_prob && !grad_new_z);
    if (!empty && !ws) return HPC_RLL_EINVAL;
    if (rows < 0 || MN <= 0) return HPC_RLL_EINVAL;
    if (!aligned(g_policy, 4) || !aligned(ws, 4) || !aligned(grad_log_prob, 4) || !aligned(grad_new_z, 4)) return HPC_RLL_EALIGN;
    if (MN > kTqcMaxAtoms) return HPC_RLL_EUNSUPPORTED;
    if (empty) return HPC_RLL_OK;
    hipStream_t st = (hipStream_t)stream;
    const long nz = (long)rows * MN;
    const bool v4 = nz % 4 == 0 && aligned(grad_new_z, 16);
    const unsigned grid = row_grid(grad_new_z ? (v4 ? nz / 4 : nz) : (long)rows, 256, 4096);
    const int flags = (grad_log_prob ? 1 : 0) | (grad_new_z ? 2 : 0);
    return with_bool(v4, [&](auto V_) {
        constexpr bool V4 = V_;
        hipLaunchKernelGGL((tqc_policy_bwd_kernel<V4>), dim3(grid), dim3(256), 0, st, g_policy, ws + kTqcConsts, grad_log_prob,
                           grad_new_z, (long)rows, nz);
        const int rc = last_error();
        if (!rc) g_policy_bwd.note({4, 0, V4 ? 4 : 1, (int)grid, flags});
        return rc;
    });
}

extern "C" int hpc_rll_tqc_last_config(int* out) {
    if (!out) return HPC_RLL_EINVAL;
    g_critic_fwd.read(out);
    g_critic_bwd.read(out + kLaunchInts);
    g_policy_fwd.read(out + 2 * kLaunchInts);
    g_policy_bwd.read(out + 3 * kLaunchInts);
    return HPC_RLL_OK;
}
static_assert(HPC_RLL_TQC_CONFIG_INTS == 4 * 6, "the layout documented in hpc_rll_hip.h");
