// nstep.hpp -- the n-step discounted reward sum shared by the per-sample TD kernels (dist_ops.hip, sample_ops.hip) and its
// form with episode ends inside the window (r2d2.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "masks.hpp"

namespace hpc_rll {
namespace {

// n-step discounted reward sum R = sum_t gamma^t r[t, b] for S samples at once, in the SAME order of operations as the
// plain loop `R = fmaf(f, r_t, R); f *= gamma` -- but the loads of four (one sample: eight) time steps x S samples are all issued before the
// first use.  In a loop with a run-time trip count the compiler waits for every load before the fma that consumes it: the
// plain form costs one dependent memory round trip PER STEP (nstep = 5: five round trips before the sample's rows can
// even be addressed), which is what these per-sample kernels were bound by at large batch.
template <int S>
__device__ __forceinline__ void nstep_returns(const float* __restrict__ reward, int B, int nstep, float gamma,
                                              const long (&bb)[S], float (&R)[S]) {
    constexpr int CH = S == 1 ? 8 : 4;          // time steps requested together (x S samples)
#pragma unroll
    for (int s = 0; s < S; ++s) R[s] = 0.f;
    float f = 1.f;
    for (int t0 = 0; t0 < nstep; t0 += CH) {
        float r[CH][S];
#pragma unroll
        for (int k = 0; k < CH; ++k) {
            const int t = t0 + k < nstep ? t0 + k : nstep - 1;     // clamped: the load is unconditional
#pragma unroll
            for (int s = 0; s < S; ++s) r[k][s] = reward[(size_t)t * B + bb[s]];
        }
#pragma unroll
        for (int k = 0; k < CH; ++k) {
            if (t0 + k < nstep) {
#pragma unroll
                for (int s = 0; s < S; ++s) R[s] = fmaf(f, r[k][s], R[s]);
                f *= gamma;
            }
        }
    }
}
__device__ __forceinline__ float nstep_return1(const float* __restrict__ reward, int B, int nstep, float gamma, long b) {
    const long bb[1] = {b};
    float R[1];
    nstep_returns<1>(reward, B, nstep, gamma, bb, R);
    return R[0];
}

// The window of one step of a whole unroll (r2d2.hip): rewards and masks are (T,B) arrays, `o` is the offset of the window's
// first step (t*B + b), step j lies at o + j*B and k_j = 1 - done_j (masks.hpp).  With p_0 = 1, p_{j+1} = (p_j gamma) k_j:
//   R = sum_{j<nstep} p_j r_j,   pn = p_nstep   (the coefficient gamma^n c_n of the bootstrap value)
// so a done at step j keeps r_j and cuts everything after it.  The order of operations is the plain loop's, and the loads of
// eight steps (rewards and masks) are issued before the first use, as above.  HAS_DONE false loads no mask and multiplies
// nothing: the bits of an all-zero mask (x * 1.0f is x).
template <int MT, bool HAS_DONE>
__device__ __forceinline__ float nstep_return_masked(const float* __restrict__ reward, const void* __restrict__ done, size_t o,
                                                     int B, int nstep, float gamma, float& pn) {
    constexpr int CH = 8;
    float R = 0.f, p = 1.f;
    for (int j0 = 0; j0 < nstep; j0 += CH) {
        float r[CH];
        MaskRow<1, MT> m[CH];
#pragma unroll
        for (int k = 0; k < CH; ++k) {
            const int j = j0 + k < nstep ? j0 + k : nstep - 1;     // clamped: the loads are unconditional
            const size_t idx = o + (size_t)j * B;
            r[k] = reward[idx];
            if (HAS_DONE) m[k].template load<false>(done, idx);
        }
#pragma unroll
        for (int k = 0; k < CH; ++k) {
            if (j0 + k < nstep) {
                R = fmaf(p, r[k], R);
                p *= gamma;
                if (HAS_DONE) p *= m[k].keep(0);
            }
        }
    }
    pn = p;
    return R;
}

}  // namespace
}  // namespace hpc_rll
