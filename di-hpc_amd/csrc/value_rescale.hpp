// value_rescale.hpp -- the invertible value rescaling of the n-step TD losses (sample_ops.hip, r2d2.hip):
//   h(x) = sign(x) (sqrt(|x| + 1) - 1) + eps x,   h^-1(x) = sign(x) (((sqrt(1 + 4 eps (|x| + 1 + eps)) - 1) / (2 eps))^2 - 1)
// (Pohlen et al. 2018; hpc_rll/origin/td.py:326-354).  One definition, so that every op that rescales rounds alike.
#pragma once
#include <hip/hip_runtime.h>

namespace hpc_rll {
namespace {

__device__ __forceinline__ float h_transform(float x, float eps) {
    const float s = (x > 0.f) ? 1.f : ((x < 0.f) ? -1.f : 0.f);
    return s * (sqrtf(fabsf(x) + 1.f) - 1.f) + eps * x;
}
__device__ __forceinline__ float h_inverse(float x, float eps) {
    const float s = (x > 0.f) ? 1.f : ((x < 0.f) ? -1.f : 0.f);
    const float t = (sqrtf(1.f + 4.f * eps * (fabsf(x) + 1.f + eps)) - 1.f) / (2.f * eps);
    return s * (t * t - 1.f);
}

}  // namespace
}  // namespace hpc_rll
