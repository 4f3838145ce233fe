// hostutil.hpp -- the two host-side one-liners every entry point of the library needs.
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

}  // namespace hpc_rll
