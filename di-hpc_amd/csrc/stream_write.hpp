// stream_write.hpp -- the store pattern that reaches MI355X's pure-write rate.
//
// Measured (tests/tools/micro/writebw2.hip, writebw3.hip; profiles/r04_writebw.txt): a 4 GiB output is written at
//   6.3-6.5 TB/s  by ONE workgroup of 256 threads per CU walking the output grid-stride with 16-byte stores (every sweep of
//                 the grid covers one contiguous MiB; hipMemsetD32Async: 6.6),
//   4.5-5.9 TB/s  by the same loop with 2 ... 256 workgroups per CU, with 2 / 6 / 8 / 16 waves per workgroup, or with a
//                 contiguous chunk per workgroup or per wave -- what every write-heavy kernel of this library did.
// What decides it is that the 256 x 16 bytes a workgroup stores together are ONE 4 KiB-ALIGNED block (2 / 6 KiB per workgroup,
// or 4 KiB starting 512 bytes off a boundary: 4.7-5.8) and that few waves per CU store at a time.
// Kernels whose output is mostly zeros (the one-hot gradients of the n-step TD losses: 1 / N of the elements) therefore
// write in two launches: this fill, then the few values.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hostutil.hpp"
#include "wave.hpp"

namespace hpc_rll {

// `shift` = 16-byte elements between the 4 KiB boundary below y and y: the loop runs over indices from that boundary, so that
// every workgroup's 256 x 16 bytes are ONE 4 KiB-aligned block (the same loop on a base 512 bytes off such a boundary:
// 5.7 instead of 6.5 TB/s).
static __global__ __launch_bounds__(256) void stream_zero_kernel(vfloat4* __restrict__ y, size_t n4, unsigned shift,
                                                          float* __restrict__ tail, int ntail) {
    const vfloat4 z = {0.f, 0.f, 0.f, 0.f};
    const size_t nt = (size_t)gridDim.x * 256, end = n4 + shift;
    for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < end; v += nt)
        if (v >= shift) y[v - shift] = z;
    if (blockIdx.x == 0 && (int)threadIdx.x < ntail) tail[threadIdx.x] = 0.f;
}

// p[0, n) = 0.  p must be 16-byte aligned.
inline int launch_stream_zero(float* p, size_t n, hipStream_t st) {
    if (n == 0) return 0;
    int cus = device_cus();
    if (cus <= 0) cus = 256;
    const size_t n4 = n / 4;
    const unsigned shift = (unsigned)((reinterpret_cast<uintptr_t>(p) & 4095) / 16);
    hipLaunchKernelGGL(stream_zero_kernel, dim3((unsigned)cus), dim3(256), 0, st, reinterpret_cast<vfloat4*>(p), n4, shift,
                       p + n4 * 4, (int)(n - n4 * 4));
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

// One-hot rows of N floats, every float of grad[0, n) written once: value(u, row, col) is the float at (row, col), u the
// upstream scalar (*g, or 1 when g is NULL).  Vector v of the launch covers elements [(v - shift)*VEC, +VEC): the loop runs
// from the 4 KiB boundary below grad (above).  (row, col) of a thread's first element advance by (step_row, step_col) =
// divmod(threads * VEC, N) per sweep: one 64-bit division per thread, not per store.  Used by the backward launches of
// retrace.hip and r2d2.hip.
template <int VEC, class Value>
static __global__ __launch_bounds__(256) void onehot_stream_kernel(const Value value, const float* __restrict__ g,
                                                                   float* __restrict__ grad, size_t n, unsigned shift, int N,
                                                                   long step_row, int step_col) {
    const float u = g ? g[0] : 1.f;
    const size_t nv = n / VEC, nt = (size_t)gridDim.x * 256, end = nv + shift;
    size_t v = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (v < shift) v += nt;                             // shift < 256 <= nt: one step passes the boundary
    if (v < end) {
        const size_t pos = (v - shift) * VEC;
        long row = (long)(pos / (size_t)N);
        int col = (int)(pos % (size_t)N);
        for (; v < end; v += nt) {
            float out[VEC];
            long r = row;
            int c = col;
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                out[k] = value(u, r, c);
                if (++c == N) { c = 0; ++r; }
            }
            if (VEC == 4) {
                vfloat4 t;
                t.x = out[0]; t.y = out[1]; t.z = out[2]; t.w = out[3];
                __builtin_nontemporal_store(t, reinterpret_cast<vfloat4*>(grad) + (v - shift));
            } else {
                __builtin_nontemporal_store(out[0], grad + (v - shift));
            }
            row += step_row;
            col += step_col;
            if (col >= N) { col -= N; ++row; }
        }
    }
    if (VEC > 1 && blockIdx.x == 0 && threadIdx.x < n - nv * VEC) {   // the last n % VEC floats
        const size_t i = nv * VEC + threadIdx.x;
        grad[i] = value(u, (long)(i / (size_t)N), (int)(i % (size_t)N));
    }
}

// Grid: unlike a pure fill, every store here waits for two small loads (action, delta), so one workgroup per CU -- the
// fill's best shape -- leaves a single wave per SIMD walking load -> store round trips (measured 282 us for 302 MB at
// T=256, B=16384, N=18).  Short-lived workgroups of at most kOnehotVecPerThread vectors per thread keep many loads in flight.
// Returns the hipError_t of the launch; *vec_out / *grid_out (either may be NULL) receive what was launched.
constexpr size_t kOnehotVecPerThread = 4;
template <class Value>
inline int launch_onehot_stream(const Value& value, const float* g, float* grad, size_t n, int N, hipStream_t st,
                                int* vec_out = nullptr, long* grid_out = nullptr) {
    const bool vec4 = (reinterpret_cast<uintptr_t>(grad) & 15) == 0;
    const unsigned shift = vec4 ? (unsigned)((reinterpret_cast<uintptr_t>(grad) & 4095) / 16) : 0u;
    const size_t end = (vec4 ? n / 4 : n) + shift;
    size_t grid = (end + 256 * kOnehotVecPerThread - 1) / (256 * kOnehotVecPerThread);
    if (grid < 1) grid = 1;
    if (grid > 256 * 1024) grid = 256 * 1024;   // the threads loop
    const size_t nt = grid * 256;
    if (vec4) {
        hipLaunchKernelGGL((onehot_stream_kernel<4, Value>), dim3((unsigned)grid), dim3(256), 0, st, value, g, grad, n, shift, N,
                           (long)(nt * 4 / N), (int)(nt * 4 % N));
    } else {
        hipLaunchKernelGGL((onehot_stream_kernel<1, Value>), dim3((unsigned)grid), dim3(256), 0, st, value, g, grad, n, 0u, N,
                           (long)(nt / N), (int)(nt % N));
    }
    if (vec_out) *vec_out = vec4 ? 4 : 1;
    if (grid_out) *grid_out = (long)grid;
    return (int)hipGetLastError();
}

}  // namespace hpc_rll
