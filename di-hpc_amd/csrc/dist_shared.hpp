// dist_shared.hpp -- the pieces the quantile learners share: the sample-per-lane-group mapping, the packed quantile-Huber pair
// loop of IQN and FQF, and the host helpers that turn a run-time width into a template argument (dist_ops.hip, fqf.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <type_traits>

#include "colscan.hpp"
#include "hpc_rll_hip.h"
#include "wave.hpp"

namespace hpc_rll {
namespace {

// 4 waves x 64/G samples per workgroup; workgroup partial = the per-sample contributions added in sample order.
template <int G, class F>
__device__ __forceinline__ void group_per_sample(int B, float* __restrict__ partials, const ScanFold& fold, F&& body) {
    constexpr int SPW = 64 / G;
    __shared__ float red[4 * SPW];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, gl = lane % G, gs = lane / G;
    const long b = ((long)blockIdx.x * 4 + w) * SPW + gs;
    const float contrib = body(b, b < (long)B, gl, gs * G);   // every lane runs the body (it shuffles): loads are guarded
    if (gl == 0) red[w * SPW + gs] = b < (long)B ? contrib : 0.f;
    __syncthreads();
    float s = 0.f;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < 4 * SPW; ++i) s += red[i];
    }
    publish_sums<1, 256>(s, partials, fold);
}

// The pair loops of the group kernels take two targets per iteration: targets j and j + 1 of the group whose first lane is
// `base`, lane l of it holding target l.  `two` (wave-uniform) is false at an odd tail, where .y repeats target j and the caller
// takes it out of the sums.
__device__ __forceinline__ vfloat2 fetch_two_targets(float tgt, int base, int j, bool two) {
    vfloat2 t2;
    t2.x = __shfl(tgt, base + j, 64);
    t2.y = __shfl(tgt, base + (two ? j + 1 : j), 64);
    return t2;
}

// The quantile-Huber pair loop of one sample on a group of G lanes (IQN and FQF): lane gl < tau holds quantile value `qi` with
// fraction `rho`, lane gl < tau_p holds target `tgt`.  Stores the unit gradient buf[b, gl] and td_err[b]; returns the sample's
// weighted loss.  Run by every lane of the group (it shuffles).
template <int G>
__device__ __forceinline__ float quantile_huber_group(long b, bool ok, int gl, int base, int tau, int tau_p, float qi, float rho,
                                                      float tgt, float w, float kappa, float scale, float* __restrict__ td_err,
                                                      float* __restrict__ buf) {
    const float inv_tp = 1.f / (float)tau_p;
    // The pair loop is VALU-bound (tau * tau' pairs per sample, a wave64 instruction costs 4 cycles): two targets per
    // iteration in packed fp32 (v_pk_add / v_pk_fma / v_pk_mul), and per pair only
    //   dh = med3(e, -kappa, kappa)            (the Huber derivative: e inside, +-kappa outside)
    //   hub = dh * (e - 0.5 * dh)              (= 0.5 e^2 inside, kappa (|e| - 0.5 kappa) outside: the same roundings
    //                                           as the two-branch form, element by element)
    //   qw = e < 0 ? |rho - 1| / kappa : |rho| / kappa      (both hoisted out of the loop)
    // -- 5.5 instructions per pair instead of ~13.  Even and odd targets accumulate separately (summation order).
    const float qneg = fabsf(rho - 1.f) / kappa, qpos = fabsf(rho) / kappa;
    const vfloat2 q2 = {qi, qi}, mh2 = {-0.5f, -0.5f};
    vfloat2 li2 = {0.f, 0.f}, gi2 = {0.f, 0.f};
    for (int j = 0; j < tau_p; j += 2) {
        const bool two = j + 1 < tau_p;
        const vfloat2 e = fetch_two_targets(tgt, base, j, two) - q2;
        vfloat2 dh, qw;
        dh.x = __builtin_amdgcn_fmed3f(e.x, -kappa, kappa);
        dh.y = __builtin_amdgcn_fmed3f(e.y, -kappa, kappa);
        const vfloat2 hub = dh * __builtin_elementwise_fma(mh2, dh, e);
        qw.x = e.x < 0.f ? qneg : qpos;
        qw.y = two ? (e.y < 0.f ? qneg : qpos) : 0.f;
        li2 = __builtin_elementwise_fma(qw, hub, li2);
        gi2 = __builtin_elementwise_fma(qw, dh, gi2);
    }
    const float li = li2.x + li2.y, gi = gi2.x + gi2.y;
    if (ok && gl < tau) buf[(size_t)b * tau + gl] = -gi * inv_tp * w * scale;   // de/dq = -1
    const float loss = hpc_rll::group_sum<G>(gl < tau ? li : 0.f) * inv_tp;
    if (ok && gl == 0) td_err[b] = loss;
    return loss * w;
}

inline int group_lanes(int n) { return n <= 8 ? 8 : n <= 16 ? 16 : n <= 32 ? 32 : 64; }

// The widths that have instantiations, of a lane group (G) and of the samples a wave walks (SW, tune key 24) alike: 8, 16, 32, 64.
// f(width as a std::integral_constant) for the listed width that equals x, and its status; HPC_RLL_EUNSUPPORTED for any other x
// (f is not called: nothing is launched).  with_bool: f(std::true_type / std::false_type) for a template flag (FULL, BNT).
template <class F> int with_width(int x, F&& f) {
    switch (x) {
        case 8: return f(std::integral_constant<int, 8>{});
        case 16: return f(std::integral_constant<int, 16>{});
        case 32: return f(std::integral_constant<int, 32>{});
        case 64: return f(std::integral_constant<int, 64>{});
    }
    return HPC_RLL_EUNSUPPORTED;
}
template <class F> int with_bool(bool x, F&& f) { return x ? f(std::true_type{}) : f(std::false_type{}); }

inline float gamma_pow(float gamma, int nstep) { return (float)pow((double)gamma, (double)nstep); }

}  // namespace
}  // namespace hpc_rll
