// value_rescale.hpp -- the invertible value rescaling of the n-step TD losses (sample_ops.hip, r2d2.hip):
//   h(x) = sign(x) (sqrt(|x| + 1) - 1) + eps x,   h^-1(x) = sign(x) (((sqrt(1 + 4 eps (|x| + 1 + eps)) - 1) / (2 eps))^2 - 1)
// (Pohlen et al. 2018; hpc_rll/origin/td.py:326-354).  One definition, so that every op that rescales rounds alike.
// The fp64 forms below serve the categorical value losses (twohot.hip), whose per-row scalar chain is fp64: there phi(y)
// reaches the hundreds, where an fp32 rounding moves a two-hot weight by 3e-5, and fp32 h^-1 is off by 2.6e-5 at 0 through
// the cancellation under its square root.  With them symlog(x) = sign(x) log(1 + |x|) and its inverse sign(x) (e^|x| - 1)
// (Hafner et al. 2023).
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

__device__ __forceinline__ double h_transform(double x, double eps) {
    const double s = (x > 0.0) ? 1.0 : ((x < 0.0) ? -1.0 : 0.0);
    return s * (sqrt(fabs(x) + 1.0) - 1.0) + eps * x;
}
__device__ __forceinline__ double h_inverse(double x, double eps) {
    const double s = (x > 0.0) ? 1.0 : ((x < 0.0) ? -1.0 : 0.0);
    const double t = (sqrt(1.0 + 4.0 * eps * (fabs(x) + 1.0 + eps)) - 1.0) / (2.0 * eps);
    return s * (t * t - 1.0);
}
__device__ __forceinline__ double symlog(double x) { return copysign(log1p(fabs(x)), x); }
__device__ __forceinline__ double symlog_inverse(double x) { return copysign(expm1(fabs(x)), x); }

}  // namespace
}  // namespace hpc_rll
