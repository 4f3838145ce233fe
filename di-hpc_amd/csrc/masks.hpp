// masks.hpp -- done / traj_flag mask loading and dispatch shared by the episode-aware ops on gfx950 (gae_masked.hip,
// scan_masked.hip).
//
// With k^d_t = 1 - done_t and k^f_t = 1 - f_t (f = traj_flag, defaulting to done), every masked op weights its bootstrap
// value with k^d and its continuation with k^f.  Masks are (T,B) and loaded as they are stored: V bytes per lane for
// bool / uint8 (one dword for V = 4), V floats for float32.  traj_flag == NULL reuses the `done` registers (no second
// mask stream).
//
// Everything here has internal linkage: one copy per translation unit, as when it lived inside gae_masked.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <initializer_list>
#include <type_traits>

#include "hostutil.hpp"
#include "wave.hpp"

namespace hpc_rll {
namespace {

// mask modes: which of done / traj_flag are present (MM_DONE: f = done, one stream)
enum { MM_NONE = 0, MM_DONE = 1, MM_BOTH = 2, MM_FLAG = 3 };
constexpr bool has_done(int mm) { return mm == MM_DONE || mm == MM_BOTH; }
constexpr bool has_flag(int mm) { return mm == MM_BOTH || mm == MM_FLAG; }

// One row of a mask as loaded: MT = 0 -> V bytes (bool / uint8; nonzero = 1), MT = 1 -> V floats (soft masks).
template <int V, int MT> struct MaskRow;
template <int V> struct MaskRow<V, 0> {
    using Raw = typename std::conditional<V == 1, uint8_t, typename std::conditional<V == 2, uint16_t, uint32_t>::type>::type;
    Raw x;
    template <bool NT> __device__ __forceinline__ void load(const void* base, size_t idx) {
        x = ld<NT>(reinterpret_cast<const Raw*>(static_cast<const uint8_t*>(base) + idx));
    }
    __device__ __forceinline__ float keep(int k) const { return ((x >> (8 * k)) & 0xffu) ? 0.f : 1.f; }
};
template <int V> struct MaskRow<V, 1> {
    Pack<V> x;
    template <bool NT> __device__ __forceinline__ void load(const void* base, size_t idx) {
        x = load_pack<V, NT>(static_cast<const float*>(base) + idx);
    }
    __device__ __forceinline__ float keep(int k) const { return 1.f - x.v[k]; }
};

template <int N> using I = std::integral_constant<int, N>;

// Calls f(I<MT>, I<MM>, I<NVF>) for the runtime mask dtype / mask mode / input form.
template <class F>
inline void with_mode(int mt, int mm, bool nvf, F&& f) {
    auto form = [&](auto MT_, auto MM_) {
        if (nvf) f(MT_, MM_, I<1>{});
        else f(MT_, MM_, I<0>{});
    };
    if (mm == MM_NONE) { form(I<0>{}, I<MM_NONE>{}); return; }
    auto mode = [&](auto MT_) {
        if (mm == MM_DONE) form(MT_, I<MM_DONE>{});
        else if (mm == MM_BOTH) form(MT_, I<MM_BOTH>{});
        else form(MT_, I<MM_FLAG>{});
    };
    if (mt == 1) mode(I<1>{});
    else mode(I<0>{});
}

inline int mask_mode(const void* done, const void* flag) {
    return done ? (flag ? MM_BOTH : MM_DONE) : (flag ? MM_FLAG : MM_NONE);
}

// Widest pack (2 or 1 columns per lane) the shape and every pointer allow; masks in their own element size.
inline int max_vec(int B, int mt, std::initializer_list<const void*> f32, std::initializer_list<const void*> masks) {
    if (B % 2) return 1;
    bool ok = true;
    for (const void* p : f32) ok = ok && aligned(p, 8);
    for (const void* p : masks) ok = ok && aligned(p, mt == 1 ? 8 : 2);
    return ok ? 2 : 1;
}

}  // namespace
}  // namespace hpc_rll
