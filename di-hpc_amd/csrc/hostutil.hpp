// hostutil.hpp -- the host-side one-liners every entry point of the library needs, and the dispatch record of a launch site.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hpc_rll_hip.h"

namespace hpc_rll {

// the status of the launch just issued, as the C ABI returns it
inline int last_error() {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? HPC_RLL_OK : (int)e;
}

// an absent (null) optional pointer restricts nothing: it counts as aligned
inline bool aligned(const void* p, size_t a) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) % a) == 0; }

inline int device_cus() {   // CU count of the current device (cached per device; 0 on error)
    constexpr int kMax = 64;
    static int cus[kMax] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMax) return 0;
    if (cus[dev] == 0) {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) v = 0;
        cus[dev] = v > 0 ? v : -1;
    }
    return cus[dev] > 0 ? cus[dev] : 0;
}

// The dispatch record behind a hpc_rll_*_last_config: K plain ints of the host process, zero at load, not synchronised.
// v[0] counts the launches so far, the rest describe the last one and read as -1 before the first.
template <int K> struct LaunchRecord {
    int v[K];
    void note(const int (&vals)[K - 1]) {
        ++v[0];
        for (int i = 1; i < K; ++i) v[i] = vals[i - 1];
    }
    void read(int* out) const {
        out[0] = v[0];
        for (int i = 1; i < K; ++i) out[i] = v[0] ? v[i] : -1;
    }
};

}  // namespace hpc_rll
