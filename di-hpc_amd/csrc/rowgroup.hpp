// rowgroup.hpp -- the row-per-lane-group mapping of the head kernels: categorical.hip, gaussian.hip, retrace.hip, acer.hip,
// coma.hip, r2d2.hip and sac.hip (grpo.hip uses group_all alone).
//
// A row of N floats is owned by an aligned GROUP of G lanes (G = 1..64, a power of two), 256 / G groups per workgroup.  Lane
// gl of the group holds E pieces of VEC consecutive floats, piece e at column (e*G + gl)*VEC, of every (rows,N) input, in
// VGPRs: each input is read from HBM exactly once, 16 bytes per lane when N % 4 == 0 and the bases allow it.  R rows per
// group and iteration (RowsPerIter) give R independent load + reduction chains; reductions over the group are butterflies in
// registers (group_all here, group_sum_last of wave.hpp): no LDS, no barrier.  Row (iteration block bb, slot k, group gi) is
// bb + k*(256/G) + gi, so for a fixed k the groups of a workgroup read consecutive rows: one contiguous span per load
// instruction whatever G is.
//
// Device side: RowSlice, RowsPerIter, dpp_mov, group_all with its ops (AddOp, MaxOp, MinOp), group_all_f64; for the softmax heads
// row_max_finite (the clamped maximum), action_index (the column an action selects) and store_piece (a lane's piece of an
// output row).
// Host side: row_cfg (which G, VEC, E for an N), row_grid, the table of configurations the rule gives at kRow4Pieces pieces
// per lane, checked against the rule at compile time and its dispatcher with_row4 (launch_rows_folded, for the
// forwards that end in loss sums, is in colscan.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "hpc_rll_hip.h"
#include "wave.hpp"

namespace hpc_rll {

// ---- all-reduce butterflies over aligned groups of G lanes: DPP inside a 16-lane row, ds_bpermute above it.
template <int CTRL> __device__ __forceinline__ float dpp_mov(float x) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xF, 0xF, true));
}
// Op::f(a, b): AddOp, MaxOp or MinOp below, or the unit's own (categorical.hip's max assumes other things about NaNs)
template <int G, class Op> __device__ __forceinline__ float group_all(float x) {
    if (G >= 2) x = Op::f(x, dpp_mov<0xB1>(x));    // quad_perm [1,0,3,2]
    if (G >= 4) x = Op::f(x, dpp_mov<0x4E>(x));    // quad_perm [2,3,0,1]
    if (G >= 8) x = Op::f(x, dpp_mov<0x141>(x));   // row_half_mirror: lane i <-> 7-i
    if (G >= 16) x = Op::f(x, dpp_mov<0x140>(x));  // row_mirror: lane i <-> 15-i
    if (G >= 32) x = Op::f(x, __shfl_xor(x, 16, 64));
    if (G >= 64) x = Op::f(x, __shfl_xor(x, 32, 64));
    return x;
}

// the sum over the group in fp64, for the few per-row sums whose fp32 rounding would show (qmix.hip's q_tot, twohot.hip's
// expectation): two 32-bit exchanges per step
template <int G> __device__ __forceinline__ double group_all_f64(double x) {
#pragma unroll
    for (int m = 1; m < G; m <<= 1) x += __shfl_xor(x, m, 64);
    return x;
}

struct AddOp { static __device__ __forceinline__ float f(float a, float b) { return a + b; } };
struct MaxOp { static __device__ __forceinline__ float f(float a, float b) { return fmaxf(a, b); } };
struct MinOp { static __device__ __forceinline__ float f(float a, float b) { return fminf(a, b); } };

// Per-lane slice of one row: E pieces of VEC consecutive floats, piece e at column (e*G + gl)*VEC.
// load() only ISSUES the (nontemporal: a row is read exactly once) loads: every lane loads unconditionally -- padding
// lanes re-read column 0 -- so there is no divergent branch around a load and all E loads of all R rows of an iteration
// are in flight before the first use.  What padding lanes hold is the user's to discard: the categorical kernels clamp it
// with ONE v_med3_f32 per element after the loads (finish() in categorical.hip), the others select on c < N where they
// accumulate.  (The first version of the categorical kernels clamped inside `if (c < N)`, which compiled to a branch and
// s_waitcnt vmcnt(0) per load plus two v_max per element; in an in-process A/B the two builds time the same to 1 % at
// every N (tests/tools/cat_ab_probe.py: the kernels are VALU-bound and eight waves per SIMD hid the serialised loads) --
// this form is kept for being branch-free and 40 instructions shorter.)
template <int G, int VEC, int E>
struct RowSlice {
    float x[E * VEC];
    __device__ __forceinline__ void load(const float* __restrict__ row, int N, int gl) {
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int c = (e * G + gl) * VEC;
            const int cc = (c < N) ? c : 0;
            if (VEC == 4) {
                const vfloat4 t = __builtin_nontemporal_load(reinterpret_cast<const vfloat4*>(row + cc));
                x[e * 4 + 0] = t.x; x[e * 4 + 1] = t.y; x[e * 4 + 2] = t.z; x[e * 4 + 3] = t.w;
            } else {
                x[e] = __builtin_nontemporal_load(row + cc);
            }
        }
    }
};

// R rows per group per iteration: R independent load + reduction chains in flight, the inputs x R rows x E*VEC floats per
// lane within the register budget of 256-thread workgroups.
template <int VEC, int E> struct RowsPerIter { static constexpr int value = (E * VEC <= 4) ? 4 : ((E * VEC <= 8) ? 2 : 1); };

// ---- what the softmax heads share beyond the slice
constexpr float kFltMax = 3.402823466e38f;

// the maximum of a row of logits in every lane of the group; -inf (a masked action) counts as the most negative finite
// float, as does padding
template <int G, int VEC, int E> __device__ __forceinline__ float row_max_finite(const float* x, int N, int gl) {
    float mx = -kFltMax;
#pragma unroll
    for (int e = 0; e < E; ++e)
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const int c = (e * G + gl) * VEC + j;
            mx = fmaxf(mx, c < N ? fmaxf(x[e * VEC + j], -kFltMax) : -kFltMax);
        }
    return group_all<G, MaxOp>(mx);
}

// the column an action selects, -1 outside [0, N): it then matches no column
__device__ __forceinline__ int action_index(long a, int N) { return (a >= 0 && a < (long)N) ? (int)a : -1; }

// a lane's piece of an output row (written exactly once: nontemporal), 16 bytes when VEC == 4
template <int VEC> __device__ __forceinline__ void store_piece(float* dst, const float (&o)[VEC]) {
    if constexpr (VEC == 4) {
        vfloat4 t;
        t.x = o[0]; t.y = o[1]; t.z = o[2]; t.w = o[3];
        __builtin_nontemporal_store(t, reinterpret_cast<vfloat4*>(dst));
    } else {
        __builtin_nontemporal_store(o[0], dst);
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------
struct RowCfg { int g, vec, e; };

// The group is one DPP row (16 lanes) or less while `row_pieces` pieces per lane suffice (the reductions are then DPP steps
// with no exchange between DPP rows); longer rows take the whole wave.  E is rounded up to a power of two.
constexpr RowCfg row_cfg(int N, bool can_vec4, int row_pieces) {
    RowCfg c{1, (can_vec4 && (N % 4) == 0) ? 4 : 1, 1};
    const int pieces = (N + c.vec - 1) / c.vec;
    const int gmax = pieces <= 16 * row_pieces ? 16 : 64;
    while (c.g < gmax && c.g < pieces) c.g <<= 1;
    const int e = (pieces + c.g - 1) / c.g;
    while (c.e < e) c.e <<= 1;
    return c;
}

// workgroups for `rows` rows at `rows_per_block` rows per workgroup and iteration; above `cap` the workgroups loop
inline unsigned row_grid(long rows, long rows_per_block, long cap) {
    long g = (rows + rows_per_block - 1) / rows_per_block;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (unsigned)g;
}

// Pieces per lane of every head but the categorical one: a unit holds three to five slices of a row at once, and at 16
// floats per slice that is 48 to 80 VGPRs for ONE row (categorical.hip's 8 pieces would be twice that).
constexpr int kRow4Pieces = 4;
// The grid cap of a row kernel that ends in no sums: short-lived workgroups; above it they loop.
constexpr long kUnfoldedGridCap = 256L * 1024;
// The (G, VEC, E) of row_cfg(N, ., kRow4Pieces) for 1 <= N <= kRowTableMaxN (64 lanes x 16 floats per lane and input): the
// kernels these heads instantiate.
constexpr int kRowTableMaxN = 1024;
#define HPC_RLL_ROW4_TABLE(CASE)                                                                                      \
    CASE(1, 4, 1) CASE(2, 4, 1) CASE(4, 4, 1) CASE(8, 4, 1) CASE(16, 4, 1) CASE(16, 4, 2) CASE(16, 4, 4)             \
    CASE(64, 4, 2) CASE(64, 4, 4)                                                                                     \
    CASE(1, 1, 1) CASE(2, 1, 1) CASE(4, 1, 1) CASE(8, 1, 1) CASE(16, 1, 1) CASE(16, 1, 2) CASE(16, 1, 4)             \
    CASE(64, 1, 2) CASE(64, 1, 4) CASE(64, 1, 8) CASE(64, 1, 16)

// A table is complete when every configuration the rule returns is one of its entries; a rule edit that forgets the table
// then fails to compile instead of turning a valid N into HPC_RLL_EUNSUPPORTED at run time.
#define HPC_RLL_ROW_MATCH(G_, V_, E_, ...) || (c.g == G_ && c.vec == V_ && c.e == E_)
constexpr bool row4_table_complete() {
    for (int n = 1; n <= kRowTableMaxN; ++n)
        for (int v4 = 0; v4 < 2; ++v4) {
            const RowCfg c = row_cfg(n, v4 != 0, kRow4Pieces);
            if (!(false HPC_RLL_ROW4_TABLE(HPC_RLL_ROW_MATCH))) return false;
        }
    return true;
}
static_assert(row4_table_complete(), "HPC_RLL_ROW4_TABLE misses a configuration row_cfg(N, ., kRow4Pieces) returns for N <= kRowTableMaxN");

// f(G, V, E) as std::integral_constants for the table entry that equals cfg; its status, or HPC_RLL_EUNSUPPORTED
template <int N> using RowInt = std::integral_constant<int, N>;
template <class F> int with_row4(const RowCfg& cfg, F&& f) {
#define HPC_RLL_ROW4_CASE(G_, V_, E_) \
    if (cfg.g == G_ && cfg.vec == V_ && cfg.e == E_) return f(RowInt<G_>{}, RowInt<V_>{}, RowInt<E_>{});
    HPC_RLL_ROW4_TABLE(HPC_RLL_ROW4_CASE)
#undef HPC_RLL_ROW4_CASE
    return HPC_RLL_EUNSUPPORTED;
}

}  // namespace hpc_rll
