// lm_head.hpp -- what the language-model head kernels of grpo.hip and lm_ppo.hip share: the limits of a row launch, the two
// element types of the logits (fp32, bf16) with their 16-byte pack / unpack, the clamp of masked entries and the bare exp2.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hpc_rll_hip.h"

namespace hpc_rll {

constexpr int kGrpoMaxV = 262144;
constexpr int kWaveRowMaxV = 2048;   // up to here a wave per row, above a workgroup per row
constexpr int kInFlight = 4;         // 16-byte loads a lane issues before it uses the first
constexpr float kFltMaxG = 3.402823466e+38f;
constexpr float kLog2eG = 1.44269504088896340736f, kLn2G = 0.69314718055994530942f;
constexpr long kRowGridMax = 1L << 16;   // workgroups of a row launch; above it they loop (far more than the device holds at once)

typedef unsigned int vuint4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float clampf(float x) { return fmaxf(x, -kFltMaxG); }   // -inf (masked) and NaN -> finite
__device__ __forceinline__ float ex2(float y) { return __builtin_amdgcn_exp2f(y); }
__device__ __forceinline__ float as_f(unsigned u) { return __builtin_bit_cast(float, u); }
__device__ __forceinline__ unsigned as_u(float f) { return __builtin_bit_cast(unsigned, f); }

// ---- the two element types: P elements per 16 bytes
template <class Elem> struct ElemIO;
template <> struct ElemIO<float> {
    static constexpr int P = 4;
    static constexpr int kCode = 0;
    static __device__ __forceinline__ float get(const float* p) { return *p; }
    static __device__ __forceinline__ void put(float* p, float v) { __builtin_nontemporal_store(v, p); }
    static __device__ __forceinline__ void unpack(const vuint4& v, float* x) {
        x[0] = as_f(v.x); x[1] = as_f(v.y); x[2] = as_f(v.z); x[3] = as_f(v.w);
    }
    static __device__ __forceinline__ vuint4 pack(const float* x) {
        vuint4 v = {as_u(x[0]), as_u(x[1]), as_u(x[2]), as_u(x[3])};
        return v;
    }
};
__device__ __forceinline__ unsigned bf16_bits(float f) {   // round to nearest even
    return (unsigned)__builtin_bit_cast(unsigned short, static_cast<__bf16>(f));
}
template <> struct ElemIO<uint16_t> {
    static constexpr int P = 8;
    static constexpr int kCode = 1;
    static __device__ __forceinline__ float get(const uint16_t* p) { return as_f((unsigned)*p << 16); }
    static __device__ __forceinline__ void put(uint16_t* p, float v) { __builtin_nontemporal_store((uint16_t)bf16_bits(v), p); }
    static __device__ __forceinline__ void unpack(const vuint4& v, float* x) {
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            x[2 * i] = as_f(w[i] << 16);
            x[2 * i + 1] = as_f(w[i] & 0xffff0000u);
        }
    }
    static __device__ __forceinline__ vuint4 pack(const float* x) {
        unsigned w[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) w[i] = bf16_bits(x[2 * i]) | (bf16_bits(x[2 * i + 1]) << 16);
        vuint4 v = {w[0], w[1], w[2], w[3]};
        return v;
    }
};

inline long row_grid_of(long rows, int rpw) {
    long grid = (rows + rpw - 1) / rpw;
    return grid < 1 ? 1 : (grid > kRowGridMax ? kRowGridMax : grid);
}
inline bool elem_ok(int e) { return e == HPC_RLL_ELEM_F32 || e == HPC_RLL_ELEM_BF16; }
inline size_t elem_size(int e) { return e == HPC_RLL_ELEM_BF16 ? 2 : 4; }

}  // namespace hpc_rll
