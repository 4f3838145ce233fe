// heads.hpp -- what the translation units of the library call in each other's policy-head kernels, declared ONCE.
// The defining units (categorical.hip, gaussian.hip) include it too, so a signature that drifts is a compile error.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hpc_rll {

struct PpoOp;   // ppo_op.hpp

// categorical.hip: log pi(action) and (ent != NULL) the entropy of `rows` rows of N logits
int categorical_forward(const float* logits, const int64_t* action, float* logp, float* ent, long rows, int N,
                        hipStream_t st);
// grad[row,i] = g1*c1[row]*(1[i==a] - p_i) + g2*c2[row]*(-p_i*(log p_i + H)); g1 / g2 device scalars (NULL = 1), c2 may be NULL
int categorical_backward(const float* logits, const int64_t* action, const float* c1, const float* g1,
                         const float* c2, const float* g2, float* grad, long rows, int N, hipStream_t st);
// categorical.hip: both policy heads and the per-sample loss in ONE launch; false = shape not covered (caller runs three)
bool ppo_forward_fused(const float* logits_new, const float* logits_old, const int64_t* action, const PpoOp& op, long rows,
                       int N, float* partials, const float* scales, float* out5, hipStream_t st, int* rc);
extern int g_ppo_fused;   // hpc_rll_tune_set key 32: 1 = try ppo_forward_fused first, 0 = always three launches

// gaussian.hip: the heads of two diagonal-Gaussian policies over one action; log_ratio: logp_b receives logp_t - logp_b
int gaussian_heads_forward(const float* mu_t, const float* sigma_t, const float* mu_b, const float* sigma_b,
                           const float* action, float* logp_t, float* ent, float* logp_b, bool log_ratio, long rows, int A,
                           hipStream_t st);

}  // namespace hpc_rll
