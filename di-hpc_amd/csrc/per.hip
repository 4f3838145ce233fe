// per.hip -- prioritized replay on the device: a sum tree and a min tree of fan-out 64 with a scattered update, a rebuild
// and a proportional sampler (hpc_rll_per_*; include/hpc_rll_hip.h has the semantics and the layout of the state).
//
// One node per wave-wide read: a wave loads the 64 children of a node with one 256-byte access, forms the inclusive prefixes
// with six shuffle steps (scan_incl below; the node's value is the last prefix, so parent and prefixes agree bit for bit) and
// either stores the parent (update, rebuild) or votes for the child to descend into (sample).  The launch boundary is the
// only synchronisation between levels: no kernel waits on another workgroup, and nothing uses a float atomic.
// Duplicates in an update: launch 1 raises stamp[idx[k]] to k + 1 with an integer atomicMax, launch 2 writes the leaf only
// where the stamp is its own k + 1 and clears it.  A loser reads either the winner's stamp or 0, never its own, so the stamps
// are 0 again after the call without an epoch.
#include <float.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "hostutil.hpp"
#include "hpc_rll_hip.h"
#include "wave.hpp"

namespace hpc_rll {
namespace {

constexpr int kFan = 64;
constexpr int kPerMaxDepth = 4;
constexpr int kPerLevels = kPerMaxDepth + 1;
constexpr int kPerHead = 64;                       // scalar words in front of the per-wave maxima
constexpr unsigned kSampleGridCap = 2048;          // workgroups of 4 waves: 8192 per-wave maxima, every wave slot of the part
constexpr unsigned kLeafGridCap = 1024;            // stamp / leaf launches: one entry per thread
constexpr unsigned kNodeGridCap = 2048;            // level launches: one node per wave
constexpr float kLeafMax = 1e30f;
constexpr int64_t kPerMaxCount = 2147483646;       // k + 1 is an int32 stamp
static_assert(HPC_RLL_PER_SCALAR_WORDS == kPerHead + 4 * (int)kSampleGridCap, "the layout documented in hpc_rll_hip.h");
static_assert(HPC_RLL_PER_MAX_CAPACITY == 1 << (6 * kPerMaxDepth), "four levels of 64");

struct Layout {
    int depth;
    int64_t n[kPerLevels], sum[kPerLevels], mn[kPerLevels], scal, stamp, words;
};

inline int64_t pad64(int64_t n) { return (n + kFan - 1) / kFan * kFan; }

// capacity in [1, 2^24]
Layout layout_of(int64_t capacity) {
    Layout L{};
    L.depth = 1;
    for (int64_t r = kFan; r < capacity; r *= kFan) ++L.depth;
    int64_t n = capacity;
    for (int l = L.depth; l >= 0; --l) {
        L.n[l] = n;
        n = (n + kFan - 1) / kFan;
    }
    int64_t off = 0;
    for (int l = 0; l < kPerLevels; ++l) {
        L.sum[l] = l <= L.depth ? off : -1;
        if (l <= L.depth) off += pad64(L.n[l]);
    }
    for (int l = 0; l < kPerLevels; ++l) {
        L.mn[l] = l <= L.depth ? off : -1;
        if (l <= L.depth) off += pad64(L.n[l]);
    }
    L.scal = off;
    off += HPC_RLL_PER_SCALAR_WORDS;
    L.stamp = off;
    L.words = off + capacity;
    return L;
}

// ---------------------------------------------------------------------------------------------------------------- device
// The inclusive prefixes of a node's children in the order the header states: x_j += x_{j-s} for s = 1, 2, .., 32.
__device__ __forceinline__ float scan_incl(float x, int lane) {
#pragma unroll
    for (int s = 1; s < kFan; s <<= 1) {
        const float y = __shfl_up(x, s, 64);
        if (lane >= s) x += y;
    }
    return x;
}
__device__ __forceinline__ float wave_min(float x) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x = fminf(x, __shfl_xor(x, m, 64));
    return x;
}

__device__ __forceinline__ bool usable(float p) { return p >= 0.f && p <= FLT_MAX; }   // finite and not negative (NaN fails)

__device__ __forceinline__ float leaf_of(float p, float alpha, float eps) {
    const double b = (double)p + (double)eps;
    const double v = alpha == 1.f ? b : (alpha == 0.f ? 1.0 : pow(b, (double)alpha));
    return fminf((float)v, kLeafMax);
}

__global__ __launch_bounds__(256) void per_init_kernel(float* w, int64_t min_lo, int64_t min_hi, int64_t scal, int64_t words) {
    for (int64_t i = blockIdx.x * 256L + threadIdx.x; i < words; i += gridDim.x * 256L) {
        float v = 0.f;
        if (i >= min_lo && i < min_hi) v = INFINITY;
        if (i == scal || i == scal + 1) v = 1.f;            // max_priority, and its next value as float bits
        w[i] = v;
    }
}

// launch 1 of an update: the highest k of every index, and the largest usable priority of the call
__global__ __launch_bounds__(256) void per_stamp_kernel(int* stamp, int* max_next, const int64_t* idx, const float* pri,
                                                        int64_t M, int64_t capacity) {
    float mx = 0.f;
    for (int64_t k = blockIdx.x * 256L + threadIdx.x; k < M; k += gridDim.x * 256L) {
        const int64_t i = idx[k];
        if (i < 0 || i >= capacity) continue;
        atomicMax(&stamp[i], (int)(k + 1));
        if (pri) {
            const float p = pri[k];
            if (usable(p)) mx = fmaxf(mx, p);
        }
    }
    if (pri) {
        mx = wave_max(mx);
        if ((threadIdx.x & 63) == 0 && mx > 0.f) atomicMax(max_next, __float_as_int(mx));   // non-negative floats order as ints
    }
}

// launch 2 of an update: the winner of every index writes its leaf and clears the stamp
__global__ __launch_bounds__(256) void per_leaf_kernel(float* sum_leaf, float* min_leaf, int* stamp, const float* max_cur,
                                                       const int64_t* idx, const float* pri, int64_t M, int64_t capacity,
                                                       float alpha, float eps) {
    const float pmax = *max_cur;
    for (int64_t k = blockIdx.x * 256L + threadIdx.x; k < M; k += gridDim.x * 256L) {
        const int64_t i = idx[k];
        if (i < 0 || i >= capacity) continue;
        if (stamp[i] != (int)(k + 1)) continue;
        stamp[i] = 0;
        float p = pri ? pri[k] : pmax;
        if (!usable(p)) p = pmax;
        const float v = leaf_of(p, alpha, eps);
        sum_leaf[i] = v;
        min_leaf[i] = v > 0.f ? v : INFINITY;
    }
}

// the leaves of a rebuild (after per_init_kernel): an unusable priority leaves its slot unwritten
__global__ __launch_bounds__(256) void per_dense_leaf_kernel(float* sum_leaf, float* min_leaf, int* max_next, const float* pri,
                                                             int64_t capacity, float alpha, float eps) {
    float mx = 0.f;
    for (int64_t i = blockIdx.x * 256L + threadIdx.x; i < capacity; i += gridDim.x * 256L) {
        const float p = pri[i];
        if (!usable(p)) continue;
        mx = fmaxf(mx, p);
        const float v = leaf_of(p, alpha, eps);
        sum_leaf[i] = v;
        min_leaf[i] = v > 0.f ? v : INFINITY;
    }
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0 && mx > 0.f) atomicMax(max_next, __float_as_int(mx));
}

// One level: a wave recomputes the sum and the min of one parent from its 64 children.  idx == NULL: every node below
// `items`; otherwise the parents (idx >> shift) of the `items` entries, an entry whose predecessor has the same parent
// leaving it to the predecessor.  `scal` != NULL in the first level launch of a call: max_priority takes its next value.
__global__ __launch_bounds__(256) void per_level_kernel(const float* child_sum, const float* child_min, float* node_sum,
                                                        float* node_min, const int64_t* idx, int64_t items, int shift,
                                                        int64_t capacity, float* scal) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = gridDim.x * 4L;
    if (scal && blockIdx.x == 0 && threadIdx.x == 0) scal[0] = scal[1];
    for (int64_t k = blockIdx.x * 4L + (threadIdx.x >> 6); k < items; k += waves) {   // k is the same in every lane of a wave
        int64_t node = k;
        if (idx) {
            const int64_t i = idx[k];
            if (i < 0 || i >= capacity) continue;
            node = i >> shift;
            if (k > 0) {
                const int64_t prev = idx[k - 1];
                if (prev >= 0 && prev < capacity && (prev >> shift) == node) continue;
            }
        }
        const float c = child_sum[node * kFan + lane];
        const float m = wave_min(child_min[node * kFan + lane]);
        const float s = scan_incl(c, lane);
        if (lane == kFan - 1) node_sum[node] = s;
        if (lane == 0) node_min[node] = m;
    }
}

struct SampleArgs {
    float* state;
    int64_t sum[kPerLevels], min_root, scal;
    int depth;
    const float* u;
    int64_t* idx;
    float* weight;
    float* prob;
    int64_t B;
    int stratified, normalize;
    float beta;
    int64_t size;
    const int64_t* size_dev;
};

__global__ __launch_bounds__(256) void per_sample_kernel(SampleArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = blockIdx.x * 4L + (threadIdx.x >> 6), waves = gridDim.x * 4L;
    const float total = a.state[a.sum[0]];
    const bool has_mass = total > 0.f && total <= FLT_MAX;
    float wmax = 0.f;
    for (int64_t k = wave; k < a.B; k += waves) {
        float uk = a.u[k];
        if (!(uk == uk)) uk = 0.f;
        int64_t node = 0;
        float leaf = 0.f;
        bool ok = has_mass;
        if (has_mass) {
            const double md = a.stratified ? ((double)k + (double)uk) / (double)a.B * (double)total : (double)uk * (double)total;
            float m = (float)md;
#pragma unroll
            for (int l = 0; l < kPerMaxDepth; ++l) {
                if (l < a.depth && ok) {
                    const float c = a.state[a.sum[l + 1] + node * kFan + lane];
                    const float P = scan_incl(c, lane);
                    const bool live = c > 0.f;
                    const unsigned long long any = __ballot(live);
                    const unsigned long long hit = __ballot(live && m < P);
                    if (any == 0ull) {
                        ok = false;                                // a state that was not built by these kernels
                    } else {
                        const int j = hit ? __ffsll(hit) - 1 : 63 - __clzll(any);
                        float below = __shfl(P, j > 0 ? j - 1 : 0, 64);
                        if (j == 0) below = 0.f;
                        const float cj = __shfl(c, j, 64);
                        m -= below;
                        if (!(m >= 0.f)) m = 0.f;
                        if (m >= cj) m = __int_as_float(__float_as_int(cj) - 1);   // the largest float below cj > 0
                        node = node * kFan + j;
                        leaf = cj;
                    }
                }
            }
        }
        if (lane == 0) {
            a.idx[k] = ok ? node : -1;
            const double pr = ok ? (double)leaf / (double)total : 0.0;
            if (a.prob) a.prob[k] = (float)pr;
            if (a.weight) {
                float w = 0.f;
                if (ok) {
                    // (size prob) / (size min_leaf / total) is leaf / min_leaf: at least 1, so the weight is at most 1
                    const float sz = a.size_dev ? (float)*a.size_dev : (float)a.size;
                    const float x = a.normalize == HPC_RLL_PER_NORM_BUFFER ? leaf / a.state[a.min_root] : (float)((double)sz * pr);
                    w = a.beta == 0.f ? 1.f : exp2f(-a.beta * log2f(x));
                }
                a.weight[k] = w;
                wmax = fmaxf(wmax, w);
            }
        }
    }
    if (a.weight && a.normalize == HPC_RLL_PER_NORM_BATCH && lane == 0) a.state[a.scal + kPerHead + wave] = wmax;
}

// weight / the batch's largest weight, which every workgroup folds from the per-wave maxima of the sample launch
__global__ __launch_bounds__(256) void per_batch_norm_kernel(float* weight, const float* partial, int n_partial, int64_t B) {
    __shared__ float s[4];
    float mx = 0.f;
    for (int i = threadIdx.x; i < n_partial; i += 256) mx = fmaxf(mx, partial[i]);
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(s[0], s[1]), fmaxf(s[2], s[3]));
    for (int64_t k = blockIdx.x * 256L + threadIdx.x; k < B; k += gridDim.x * 256L) weight[k] = mx > 0.f ? weight[k] / mx : 0.f;
}

// ------------------------------------------------------------------------------------------------------------------ host
constexpr int kPerRecord = 6;
LaunchRecord<kPerRecord> g_update, g_sample;

unsigned grid_for(int64_t items, int per_block, unsigned cap) {
    const int64_t g = (items + per_block - 1) / per_block;
    return (unsigned)(g < 1 ? 1 : (g > (int64_t)cap ? (int64_t)cap : g));
}

void launch_init(float* w, const Layout& L, hipStream_t st) {
    hipLaunchKernelGGL(per_init_kernel, dim3(grid_for(L.words, 256, 2048)), dim3(256), 0, st, w, L.mn[0], L.scal, L.scal, L.words);
}

// levels depth-1 .. 0 after the leaves were written; returns the mask of the levels recomputed in full
int launch_levels(float* w, const Layout& L, const int64_t* idx, int64_t M, int64_t capacity, hipStream_t st, unsigned* first_grid) {
    int full = 0;
    for (int l = L.depth - 1; l >= 0; --l) {
        const bool all = !idx || L.n[l] <= M;
        const int64_t items = all ? L.n[l] : M;
        const unsigned grid = grid_for(items, 4, kNodeGridCap);
        if (l == L.depth - 1) *first_grid = grid;
        if (all) full |= 1 << l;
        hipLaunchKernelGGL(per_level_kernel, dim3(grid), dim3(256), 0, st, w + L.sum[l + 1], w + L.mn[l + 1], w + L.sum[l],
                           w + L.mn[l], all ? nullptr : idx, items, 6 * (L.depth - l), capacity,
                           l == L.depth - 1 ? w + L.scal : nullptr);
    }
    return full;
}

// EINVAL / EUNSUPPORTED of a capacity, 0 when it is one the kernels implement
int bad_capacity(int64_t capacity) {
    if (capacity < 1) return HPC_RLL_EINVAL;
    return capacity > HPC_RLL_PER_MAX_CAPACITY ? HPC_RLL_EUNSUPPORTED : 0;
}
bool bad_exponent(float x) { return !(x >= 0.f) || x > FLT_MAX; }

}  // namespace
}  // namespace hpc_rll

using namespace hpc_rll;

extern "C" int64_t hpc_rll_per_state_bytes(int64_t capacity) {
    if (const int rc = bad_capacity(capacity)) return rc;
    return 4 * layout_of(capacity).words;
}

extern "C" int64_t hpc_rll_per_capacity_of(int64_t state_bytes) {
    int64_t lo = 1, hi = HPC_RLL_PER_MAX_CAPACITY;
    while (lo < hi) {                                   // the size is strictly increasing in the capacity
        const int64_t mid = (lo + hi) / 2;
        if (4 * layout_of(mid).words < state_bytes) lo = mid + 1;
        else hi = mid;
    }
    return 4 * layout_of(lo).words == state_bytes ? lo : HPC_RLL_EINVAL;
}

extern "C" int hpc_rll_per_layout(int64_t capacity, int64_t* out) {
    if (!out) return HPC_RLL_EINVAL;
    if (const int rc = bad_capacity(capacity)) return rc;
    const Layout L = layout_of(capacity);
    out[0] = L.depth;
    out[1] = L.words;
    for (int l = 0; l < kPerLevels; ++l) {
        out[2 + 2 * l] = L.sum[l];
        out[3 + 2 * l] = l <= L.depth ? L.n[l] : 0;
        out[12 + 2 * l] = L.mn[l];
        out[13 + 2 * l] = l <= L.depth ? L.n[l] : 0;
    }
    out[22] = L.scal;
    out[23] = HPC_RLL_PER_SCALAR_WORDS;
    out[24] = L.stamp;
    out[25] = capacity;
    return HPC_RLL_OK;
}
static_assert(HPC_RLL_PER_LAYOUT_INTS == 2 + 4 * kPerLevels + 4, "the layout documented in hpc_rll_hip.h");

extern "C" int hpc_rll_per_init(void* state, int64_t capacity, void* stream) {
    if (!state || capacity < 1) return HPC_RLL_EINVAL;
    if (!aligned(state, 4)) return HPC_RLL_EALIGN;
    if (capacity > HPC_RLL_PER_MAX_CAPACITY) return HPC_RLL_EUNSUPPORTED;
    launch_init((float*)state, layout_of(capacity), (hipStream_t)stream);
    return last_error();
}

extern "C" int hpc_rll_per_update(void* state, int64_t capacity, const int64_t* idx, const float* priority, int64_t M,
                                  float alpha, float eps, void* stream) {
    if (!state || (M != 0 && !idx)) return HPC_RLL_EINVAL;
    if (capacity < 1 || M < 0 || M > kPerMaxCount || bad_exponent(alpha) || bad_exponent(eps)) return HPC_RLL_EINVAL;
    if (!aligned(state, 4) || !aligned(idx, 8) || !aligned(priority, 4)) return HPC_RLL_EALIGN;
    if (capacity > HPC_RLL_PER_MAX_CAPACITY) return HPC_RLL_EUNSUPPORTED;
    if (M == 0) return HPC_RLL_OK;
    const Layout L = layout_of(capacity);
    hipStream_t st = (hipStream_t)stream;
    float* w = (float*)state;
    int* stamp = (int*)state + L.stamp;
    const unsigned grid = grid_for(M, 256, kLeafGridCap);
    hipLaunchKernelGGL(per_stamp_kernel, dim3(grid), dim3(256), 0, st, stamp, (int*)state + L.scal + 1, idx, priority, M, capacity);
    hipLaunchKernelGGL(per_leaf_kernel, dim3(grid), dim3(256), 0, st, w + L.sum[L.depth], w + L.mn[L.depth], stamp, w + L.scal,
                       idx, priority, M, capacity, alpha, eps);
    unsigned first = 0;
    const int full = launch_levels(w, L, idx, M, capacity, st, &first);
    const int rc = last_error();
    if (!rc) g_update.note({(full & ~1) ? 1 : 0, L.depth, (int)first, 2 + L.depth, full});
    return rc;
}

extern "C" int hpc_rll_per_rebuild(void* state, int64_t capacity, const float* priority, float alpha, float eps, void* stream) {
    if (!state || !priority) return HPC_RLL_EINVAL;
    if (capacity < 1 || bad_exponent(alpha) || bad_exponent(eps)) return HPC_RLL_EINVAL;
    if (!aligned(state, 4) || !aligned(priority, 4)) return HPC_RLL_EALIGN;
    if (capacity > HPC_RLL_PER_MAX_CAPACITY) return HPC_RLL_EUNSUPPORTED;
    const Layout L = layout_of(capacity);
    hipStream_t st = (hipStream_t)stream;
    float* w = (float*)state;
    launch_init(w, L, st);
    hipLaunchKernelGGL(per_dense_leaf_kernel, dim3(grid_for(capacity, 256, kLeafGridCap)), dim3(256), 0, st, w + L.sum[L.depth],
                       w + L.mn[L.depth], (int*)state + L.scal + 1, priority, capacity, alpha, eps);
    unsigned first = 0;
    const int full = launch_levels(w, L, nullptr, 0, capacity, st, &first);
    const int rc = last_error();
    if (!rc) g_update.note({2, L.depth, (int)first, 2 + L.depth, full});
    return rc;
}

extern "C" int hpc_rll_per_sample(void* state, int64_t capacity, const float* u, int64_t* idx, float* weight, float* prob,
                                  int64_t B, int stratified, int normalize, float beta, int64_t size, const int64_t* size_dev,
                                  void* stream) {
    if (!state || (B != 0 && (!u || !idx))) return HPC_RLL_EINVAL;
    if (capacity < 1 || B < 0 || B > kPerMaxCount || bad_exponent(beta) || (!size_dev && size < 1) ||
        normalize < HPC_RLL_PER_NORM_NONE || normalize > HPC_RLL_PER_NORM_BATCH)
        return HPC_RLL_EINVAL;
    if (!aligned(state, 4) || !aligned(u, 4) || !aligned(idx, 8) || !aligned(weight, 4) || !aligned(prob, 4) ||
        !aligned(size_dev, 8))
        return HPC_RLL_EALIGN;
    if (capacity > HPC_RLL_PER_MAX_CAPACITY) return HPC_RLL_EUNSUPPORTED;
    if (B == 0) return HPC_RLL_OK;
    const Layout L = layout_of(capacity);
    hipStream_t st = (hipStream_t)stream;
    SampleArgs a{};
    a.state = (float*)state;
    for (int l = 0; l < kPerLevels; ++l) a.sum[l] = L.sum[l];
    a.min_root = L.mn[0];
    a.scal = L.scal;
    a.depth = L.depth;
    a.u = u;
    a.idx = idx;
    a.weight = weight;
    a.prob = prob;
    a.B = B;
    a.stratified = stratified != 0;
    a.normalize = normalize;
    a.beta = beta;
    a.size = size;
    a.size_dev = size_dev;
    const unsigned grid = grid_for(B, 4, kSampleGridCap);
    hipLaunchKernelGGL(per_sample_kernel, dim3(grid), dim3(256), 0, st, a);
    int launches = 1;
    if (weight && normalize == HPC_RLL_PER_NORM_BATCH) {
        hipLaunchKernelGGL(per_batch_norm_kernel, dim3(grid_for(B, 256, 256)), dim3(256), 0, st, weight,
                           (const float*)state + L.scal + kPerHead, (int)(grid * 4), B);
        launches = 2;
    }
    const int rc = last_error();
    if (!rc)
        g_sample.note({normalize, L.depth, (int)grid, launches,
                       (stratified ? 1 : 0) | (weight ? 2 : 0) | (prob ? 4 : 0) | (size_dev ? 8 : 0)});
    return rc;
}

extern "C" int hpc_rll_per_last_config(int* out) {
    if (!out) return HPC_RLL_EINVAL;
    g_update.read(out);
    g_sample.read(out + kPerRecord);
    return HPC_RLL_OK;
}
static_assert(HPC_RLL_PER_CONFIG_INTS == 2 * kPerRecord, "the layout documented in hpc_rll_hip.h");
