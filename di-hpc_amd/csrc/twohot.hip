// twohot.hip -- value regression as classification on gfx950: the cross-entropy of a row of N <= 1024 logits against the
// two-hot or the HL-Gauss encoding of a scalar target on a fixed support, or against a given row of probabilities, in one
// forward launch (per-row loss and the weighted loss sum) and one streaming backward; the decoded expectation; the dense
// target rows.
//
// No reference counterpart.  The formulas restate, in this project's words: the scalar transforms and the two-hot
// ("phi transform") of MuZero-style learners as LightZero writes them (scalar_transform, phi_transform,
// inverse_scalar_transform), DI-engine's symlog / inv_symlog, DreamerV3's two-hot critic targets (Hafner et al. 2023) and the
// histogram loss of "Stop Regressing" (Farebrother et al. 2024).
//
// Support: N atoms v_i = v_min + i D, D = (v_max - v_min) / (N - 1).  Transform phi: the identity, h (value_rescale.hpp) or
// symlog.  For a scalar target y: c = clamp(phi(y), v_min, v_max), and the target row t is
//   two-hot   pos = (c - v_min) / D, lo = min(floor(pos), N - 2), w = pos - lo:  t_lo = 1 - w, t_{lo+1} = w, else 0
//   HL-Gauss  edges e_i = v_i - D/2 (i = 0..N), F(e) = erf((e - c) / (sqrt(2) sigma)):
//             t_i = (F(e_{i+1}) - F(e_i)) / (F(e_N) - F(e_0))
//   dense     t is the given row.
// Per row, with p = softmax(x):  l = lse(x) - sum_i t_i x_i  (a column with t_i == 0 adds exactly 0, also where x_i = -inf: a
// masked action),  dl/dx_i = p_i - t_i;  loss = scale sum_r w_r l_r.  A row with w_r == 0 is dead: l_r is reported as 0, its
// gradient row is zeros and nothing of it -- a NaN included -- reaches anything.  A NaN scalar target of a live row gives a NaN
// l_r, loss and gradient ROW; a NaN in a dense target row gives a NaN l_r and loss and a NaN gradient at its column.
// Decode: E = sum_i p_i v_i, value = phi^-1(E).
//
// Precision.  The per-row SCALAR chain is fp64: phi(y), pos, w, the HL-Gauss centre and normaliser, sum_i t_i x_i, the
// expectation (numerator and denominator, group_all_f64 butterflies) and phi^-1.  phi(y) reaches the hundreds, where one fp32
// rounding moves w by 3e-5, and fp32 h^-1 is off by 2.6e-5 at E = 0 (value_rescale.hpp): both past the project's 1e-5.  The
// ROW stays fp32: the maximum, the exponentials, their sum, the logarithm, and erff on fp32 arguments formed from the fp64
// centre -- edge k has ONE argument whichever lane forms it, so the bin masses telescope.
//
// Mapping (rowgroup.hpp): a row is owned by an aligned group of G lanes, 256 / G rows per workgroup and iteration (R = 1);
// lane gl holds E pieces of VEC consecutive columns, piece e at column (e*G + gl)*VEC.  Each input is read once; every load is
// unconditional and in bounds (padding lanes re-read column 0, idle groups the last row) and every sum and store selects on
// column < N.  No LDS and no barrier in the row work.  The backward recomputes p = exp(x - lse) and the target from the
// scalar: a forward keeps 8 bytes per row (lse and the row's coefficient scale * w_r).
//
// Algorithmic HBM bytes per row: forward 4N + 4 read (4N more when dense, 4 more with weights), 12 written; backward
// 4N + 12 read (4N more when dense), 4N written; decode 4N read, 4 or 8 written; encode 4 read, 4N written.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "colscan.hpp"
#include "hostutil.hpp"
#include "hpc_rll_hip.h"
#include "rowgroup.hpp"
#include "value_rescale.hpp"
#include "wave.hpp"

namespace hpc_rll {
namespace {

// Workgroups of the kernels that end in no sums; above it they loop.
constexpr long kTwohotGridCap = 4096;

// what a launch knows of the support and the target kind (launch-uniform)
struct CeSupport {
    double v_min, v_max, delta, eps, inv_s;   // inv_s = 1 / (sqrt(2) sigma): HL-Gauss only
    int N, kind, transform;
};

__device__ __forceinline__ double phi(double y, int transform, double eps) {
    if (transform == HPC_RLL_TWOHOT_PHI_H) return h_transform(y, eps);
    if (transform == HPC_RLL_TWOHOT_PHI_SYMLOG) return symlog(y);
    return y;
}
__device__ __forceinline__ double phi_inverse(double x, int transform, double eps) {
    if (transform == HPC_RLL_TWOHOT_PHI_H) return h_inverse(x, eps);
    if (transform == HPC_RLL_TWOHOT_PHI_SYMLOG) return symlog_inverse(x);
    return x;
}

// What the columns of a row need of its scalar target: c, and (lo, w) of the two-hot or 1 / (F(e_N) - F(e_0)) of HL-Gauss.
// A NaN target gives a NaN c (the comparisons of the clamp are false), hence a NaN w or NaN bin masses.
struct RowTarget { double c, w, inv_z; int lo; };

__device__ __forceinline__ double edge_arg(const CeSupport& s, double c, int k) {   // (e_k - c) / (sqrt(2) sigma)
    return (s.v_min + ((double)k - 0.5) * s.delta - c) * s.inv_s;
}

__device__ __forceinline__ RowTarget row_target(const CeSupport& s, float y) {
    RowTarget t{0.0, 0.0, 0.0, 0};
    const double u = phi((double)y, s.transform, s.eps);
    t.c = u < s.v_min ? s.v_min : (u > s.v_max ? s.v_max : u);
    if (s.kind == HPC_RLL_TWOHOT_KIND_HLGAUSS) {
        t.inv_z = 1.0 / (erf(edge_arg(s, t.c, s.N)) - erf(edge_arg(s, t.c, 0)));
    } else {
        const double pos = (t.c - s.v_min) / s.delta;
        const double fl = floor(pos), top = (double)(s.N - 2);
        const double lo = fl > top ? top : fl;
        t.w = pos - lo;
        t.lo = (lo == lo) ? (int)lo : 0;
    }
    return t;
}

// t of the VEC columns from c0 on
template <int VEC>
__device__ __forceinline__ void piece_target(const CeSupport& s, const RowTarget& rt, int c0, double (&t)[VEC]) {
    if (s.kind == HPC_RLL_TWOHOT_KIND_HLGAUSS) {
        float f[VEC + 1];
#pragma unroll
        for (int k = 0; k <= VEC; ++k) f[k] = erff((float)edge_arg(s, rt.c, c0 + k));
#pragma unroll
        for (int j = 0; j < VEC; ++j) t[j] = (double)(f[j + 1] - f[j]) * rt.inv_z;
    } else {
#pragma unroll
        for (int j = 0; j < VEC; ++j) t[j] = (c0 + j == rt.lo) ? 1.0 - rt.w : ((c0 + j == rt.lo + 1) ? rt.w : 0.0);
    }
}

// a lane's targets of piece e: from the dense row it holds, or from the scalar
template <int G, int VEC, int E, bool DENSE>
__device__ __forceinline__ void lane_target(const CeSupport& s, const RowTarget& rt, const RowSlice<G, VEC, E>& dense, int e,
                                            int gl, double (&t)[VEC]) {
    if constexpr (DENSE) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) t[j] = (double)dense.x[e * VEC + j];
    } else {
        piece_target<VEC>(s, rt, (e * G + gl) * VEC, t);
    }
}

// ================================================================================================
// forward: l and lse per row, the row's coefficient, the loss sum
// ================================================================================================
struct CeFwdArgs {
    const float* logits; const float* target; const float* weight;
    float* ell; float* lse; float* coef; long rows; float scale; CeSupport s;
};

template <int G, int VEC, int E, bool DENSE>
__global__ __launch_bounds__(256) void ce_fwd_kernel(const CeFwdArgs p, float* __restrict__ partials, const ScanFold fold) {
    constexpr int GPB = 256 / G;
    const int gl = threadIdx.x % G;
    const int gi = threadIdx.x / G;
    const int N = p.s.N;
    const long stride = (long)gridDim.x * GPB;
    float acc[1] = {0.f};
    for (long bb = (long)blockIdx.x * GPB; bb < p.rows; bb += stride) {
        const long row = bb + gi;
        const bool live = row < p.rows;
        const long r = live ? row : p.rows - 1;   // (re-reads the last row; the stores below are guarded)
        RowSlice<G, VEC, E> x, td;
        x.load(p.logits + r * (long)N, N, gl);
        if constexpr (DENSE) td.load(p.target + r * (long)N, N, gl);
        const float wt = p.weight ? p.weight[r] : 1.f;
        RowTarget rt{0.0, 0.0, 0.0, 0};
        if constexpr (!DENSE) rt = row_target(p.s, p.target[r]);
        const float mx = row_max_finite<G, VEC, E>(x.x, N, gl);
        float sum = 0.f;
        double dot = 0.0;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            double t[VEC];
            lane_target<G, VEC, E, DENSE>(p.s, rt, td, e, gl, t);
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                const bool in = (e * G + gl) * VEC + j < N;
                const float v = x.x[e * VEC + j];
                sum += in ? __expf(v - mx) : 0.f;
                dot = (in && t[j] != 0.0) ? fma(t[j], (double)v, dot) : dot;   // (a NaN t is != 0: it poisons the row)
            }
        }
        sum = group_all<G, AddOp>(sum);
        dot = group_all_f64<G>(dot);
        const float lse = mx + logf(sum);
        const bool dead = wt == 0.f;
        const float l = dead ? 0.f : (float)((double)lse - dot);
        if (live && gl == 0) {
            acc[0] += dead ? 0.f : wt * l;
            p.ell[row] = l;
            p.lse[row] = lse;
            p.coef[row] = dead ? 0.f : wt * p.scale;
        }
    }
    publish_block_sums<1, 256>(acc, partials, fold);   // (the only LDS and barriers of the kernel)
}

// ================================================================================================
// backward: every float of grad_logits written once; no atomics
// ================================================================================================
struct CeBwdArgs {
    const float* logits; const float* target; const float* lse; const float* coef; const float* g_loss; const float* g_rows;
    float* grad; long rows; CeSupport s;
};

template <int G, int VEC, int E, bool DENSE>
__global__ __launch_bounds__(256) void ce_bwd_kernel(const CeBwdArgs p) {
    constexpr int GPB = 256 / G;
    const int gl = threadIdx.x % G;
    const int gi = threadIdx.x / G;
    const int N = p.s.N;
    const float gs = (!p.g_rows && p.g_loss) ? p.g_loss[0] : 1.f;
    const long stride = (long)gridDim.x * GPB;
    for (long bb = (long)blockIdx.x * GPB; bb < p.rows; bb += stride) {
        const long row = bb + gi;
        const bool live = row < p.rows;
        const long r = live ? row : p.rows - 1;
        RowSlice<G, VEC, E> x, td;
        x.load(p.logits + r * (long)N, N, gl);
        if constexpr (DENSE) td.load(p.target + r * (long)N, N, gl);
        const float lse = p.lse[r], cf = p.coef[r];
        const bool dead = cf == 0.f;
        float g = p.g_rows ? p.g_rows[r] : cf * gs;
        RowTarget rt{0.0, 0.0, 0.0, 0};
        if constexpr (!DENSE) {
            rt = row_target(p.s, p.target[r]);
            g = (rt.c == rt.c) ? g : __builtin_nanf("");   // a NaN target: the whole row
        }
#pragma unroll
        for (int e = 0; e < E; ++e) {
            double t[VEC];
            lane_target<G, VEC, E, DENSE>(p.s, rt, td, e, gl, t);
            float o[VEC];
#pragma unroll
            for (int j = 0; j < VEC; ++j) o[j] = dead ? 0.f : g * (expf(x.x[e * VEC + j] - lse) - (float)t[j]);
            const int c = (e * G + gl) * VEC;
            if (live && c < N) store_piece<VEC>(p.grad + row * (long)N + c, o);
        }
    }
}

// ================================================================================================
// decode: E = sum_i p_i v_i, value = phi^-1(E)
// ================================================================================================
template <int G, int VEC, int E>
__global__ __launch_bounds__(256) void decode_kernel(const float* __restrict__ logits, float* __restrict__ value,
                                                     float* __restrict__ expected, long rows, const CeSupport s) {
    constexpr int GPB = 256 / G;
    const int gl = threadIdx.x % G;
    const int gi = threadIdx.x / G;
    const int N = s.N;
    const long stride = (long)gridDim.x * GPB;
    for (long bb = (long)blockIdx.x * GPB; bb < rows; bb += stride) {
        const long row = bb + gi;
        const bool live = row < rows;
        const long r = live ? row : rows - 1;
        RowSlice<G, VEC, E> x;
        x.load(logits + r * (long)N, N, gl);
        const float mx = row_max_finite<G, VEC, E>(x.x, N, gl);
        double num = 0.0, den = 0.0;
#pragma unroll
        for (int e = 0; e < E; ++e)
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                const int c = (e * G + gl) * VEC + j;
                const double pe = (c < N) ? (double)__expf(x.x[e * VEC + j] - mx) : 0.0;
                den += pe;
                num = fma(pe, s.v_min + (double)c * s.delta, num);
            }
        num = group_all_f64<G>(num);
        den = group_all_f64<G>(den);
        const double ev = num / den;
        if (live && gl == 0) {
            __builtin_nontemporal_store((float)phi_inverse(ev, s.transform, s.eps), value + row);
            if (expected) __builtin_nontemporal_store((float)ev, expected + row);
        }
    }
}

// ================================================================================================
// encode: the dense target rows, a plain grid-stride writer (n = rows * N floats; VEC == 4 needs N % 4 == 0)
// ================================================================================================
template <int VEC>
__global__ __launch_bounds__(256) void encode_kernel(const float* __restrict__ target, float* __restrict__ probs, size_t n,
                                                     const CeSupport s) {
    const size_t nv = n / VEC, nt = (size_t)gridDim.x * 256;
    for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < nv; v += nt) {
        const size_t pos = v * VEC;
        const size_t row = pos / (size_t)s.N;
        const RowTarget rt = row_target(s, target[row]);
        double t[VEC];
        piece_target<VEC>(s, rt, (int)(pos - row * (size_t)s.N), t);
        float o[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) o[j] = (float)t[j];
        store_piece<VEC>(probs + pos, o);
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------
// the row-table entry of (N, load width), with DENSE as a fourth constant
template <class F> int with_ce(int N, bool v4, bool dense, F&& f) {
    return with_row4(row_cfg(N, v4, kRow4Pieces), [&](auto G_, auto V_, auto E_) {
        return dense ? f(G_, V_, E_, std::true_type{}) : f(G_, V_, E_, std::false_type{});
    });
}

// The dispatch records (hpc_rll_twohot_last_config): {launches so far, G, VEC, E, R, flags, grid} of the forward, the
// backward, the decode and the encode
constexpr int kLaunchInts = 7;
LaunchRecord<kLaunchInts> g_ce_fwd, g_ce_bwd, g_decode, g_encode;

int kind_flags(const CeSupport& s) { return (s.kind << 1) | (s.transform << 3); }

int ce_forward(const CeFwdArgs& p, float* partials, float* loss, hipStream_t st) {
    const bool dense = p.s.kind == HPC_RLL_TWOHOT_KIND_DENSE;
    const bool v4 = aligned(p.logits, 16) && (!dense || aligned(p.target, 16));
    const float sc[1] = {p.scale};
    const int flags = (p.weight ? 1 : 0) | kind_flags(p.s);
    return with_ce(p.s.N, v4, dense, [&](auto G_, auto V_, auto E_, auto D_) {
        constexpr int G = G_, V = V_, E = E_;
        constexpr bool D = D_;
        long grid = 0;
        const int rc = launch_rows_folded(p.rows, 256 / G, 1, sc, loss, partials, st, &grid,
                                          [&](unsigned blocks, const ScanFold& fold) {
            hipLaunchKernelGGL((ce_fwd_kernel<G, V, E, D>), dim3(blocks), dim3(256), 0, st, p, partials, fold);
        });
        if (grid) g_ce_fwd.note({G, V, E, 1, flags, (int)grid});
        return rc;
    });
}

int ce_backward(const CeBwdArgs& p, hipStream_t st) {
    const bool dense = p.s.kind == HPC_RLL_TWOHOT_KIND_DENSE;
    const bool v4 = aligned(p.logits, 16) && aligned(p.grad, 16) && (!dense || aligned(p.target, 16));
    const int flags = (p.g_rows ? 1 : 0) | kind_flags(p.s) | ((!p.g_rows && p.g_loss) ? 32 : 0);
    return with_ce(p.s.N, v4, dense, [&](auto G_, auto V_, auto E_, auto D_) {
        constexpr int G = G_, V = V_, E = E_;
        constexpr bool D = D_;
        const unsigned grid = row_grid(p.rows, 256 / G, kTwohotGridCap);
        hipLaunchKernelGGL((ce_bwd_kernel<G, V, E, D>), dim3(grid), dim3(256), 0, st, p);
        const int rc = last_error();
        if (!rc) g_ce_bwd.note({G, V, E, 1, flags, (int)grid});
        return rc;
    });
}

int decode(const float* logits, float* value, float* expected, long rows, const CeSupport& s, hipStream_t st) {
    return with_row4(row_cfg(s.N, aligned(logits, 16), kRow4Pieces), [&](auto G_, auto V_, auto E_) {
        constexpr int G = G_, V = V_, E = E_;
        const unsigned grid = row_grid(rows, 256 / G, kTwohotGridCap);
        hipLaunchKernelGGL((decode_kernel<G, V, E>), dim3(grid), dim3(256), 0, st, logits, value, expected, rows, s);
        const int rc = last_error();
        if (!rc) g_decode.note({G, V, E, 1, (expected ? 1 : 0) | kind_flags(s), (int)grid});
        return rc;
    });
}

int encode(const float* target, float* probs, long rows, const CeSupport& s, hipStream_t st) {
    const size_t n = (size_t)rows * (size_t)s.N;
    const int vec = (s.N % 4 == 0 && aligned(probs, 16)) ? 4 : 1;
    const unsigned grid = row_grid((long)(n / vec), 256, kTwohotGridCap);
    if (vec == 4) hipLaunchKernelGGL((encode_kernel<4>), dim3(grid), dim3(256), 0, st, target, probs, n, s);
    else hipLaunchKernelGGL((encode_kernel<1>), dim3(grid), dim3(256), 0, st, target, probs, n, s);
    const int rc = last_error();
    if (!rc) g_encode.note({0, vec, 0, 0, kind_flags(s), (int)grid});
    return rc;
}

// floats of the partial-sum region: one sum per workgroup of at most kFoldMaxGrid
constexpr int64_t kTwohotPartials = kFoldMaxGrid + 1;
constexpr int kTwohotMaxN = kRowTableMaxN;

// The checks every entry point makes of (N, kind, transform, eps, sigma, v_min, v_max), in the header's order of statuses:
// HPC_RLL_EINVAL here; the caller adds alignment, then N > kTwohotMaxN.  A dense target has no support: only N >= 1 is asked.
bool bad_support(int N, int kind, int transform, float eps, float sigma, float v_min, float v_max) {
    if (kind == HPC_RLL_TWOHOT_KIND_DENSE) return N < 1;
    if (kind != HPC_RLL_TWOHOT_KIND_TWOHOT && kind != HPC_RLL_TWOHOT_KIND_HLGAUSS) return true;
    if (transform != HPC_RLL_TWOHOT_PHI_IDENTITY && transform != HPC_RLL_TWOHOT_PHI_H && transform != HPC_RLL_TWOHOT_PHI_SYMLOG)
        return true;
    if (transform == HPC_RLL_TWOHOT_PHI_H && !(eps > 0.f)) return true;
    if (kind == HPC_RLL_TWOHOT_KIND_HLGAUSS && !(sigma > 0.f)) return true;
    return N < 2 || !(v_max > v_min);   // (a NaN bound is refused too)
}

CeSupport support_of(int N, int kind, int transform, float eps, float sigma, float v_min, float v_max) {
    CeSupport s{};
    s.N = N;
    s.kind = kind;
    if (kind == HPC_RLL_TWOHOT_KIND_DENSE) return s;
    s.transform = transform;
    s.v_min = (double)v_min;
    s.v_max = (double)v_max;
    s.delta = (s.v_max - s.v_min) / (double)(N - 1);
    s.eps = (double)eps;
    s.inv_s = kind == HPC_RLL_TWOHOT_KIND_HLGAUSS ? 1.0 / (1.4142135623730951 * (double)sigma) : 0.0;
    return s;
}

}  // namespace
}  // namespace hpc_rll

using namespace hpc_rll;

// ws (floats): lse (rows) | coef (rows) | the partial sums
extern "C" int64_t hpc_rll_twohot_workspace_floats(int64_t rows) {
    if (rows < 0 || rows > (INT64_MAX - kTwohotPartials) / 2) return HPC_RLL_EINVAL;
    return 2 * rows + kTwohotPartials;
}

extern "C" int hpc_rll_twohot_ce_forward(const float* logits, const float* target, const float* weight, float* loss,
                                         float* ell, float* ws, int64_t rows, int N, int target_kind, int transform,
                                         float eps, float sigma, float v_min, float v_max, float scale, void* stream) {
    const bool empty = rows == 0;
    if (!loss) return HPC_RLL_EINVAL;
    if (!empty && (!logits || !target || !ell || !ws)) return HPC_RLL_EINVAL;
    if (rows < 0 || bad_support(N, target_kind, transform, eps, sigma, v_min, v_max)) return HPC_RLL_EINVAL;
    if (!aligned(logits, 4) || !aligned(target, 4) || !aligned(weight, 4) || !aligned(loss, 4) || !aligned(ell, 4) ||
        !aligned(ws, 4))
        return HPC_RLL_EALIGN;
    if (N > kTwohotMaxN) return HPC_RLL_EUNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    if (empty) return (int)hipMemsetAsync(loss, 0, sizeof(float), st);
    const CeFwdArgs p{logits, target, weight, ell, ws, ws + rows, (long)rows, scale,
                      support_of(N, target_kind, transform, eps, sigma, v_min, v_max)};
    return ce_forward(p, ws + 2 * rows, loss, st);
}

extern "C" int hpc_rll_twohot_ce_backward(const float* g_loss, const float* g_rows, const float* ws, const float* logits,
                                          const float* target, float* grad_logits, int64_t rows, int N, int target_kind,
                                          int transform, float eps, float sigma, float v_min, float v_max, void* stream) {
    const bool empty = rows == 0;
    if (!empty && (!ws || !logits || !target || !grad_logits)) return HPC_RLL_EINVAL;
    if (rows < 0 || bad_support(N, target_kind, transform, eps, sigma, v_min, v_max)) return HPC_RLL_EINVAL;
    if (!aligned(g_loss, 4) || !aligned(g_rows, 4) || !aligned(ws, 4) || !aligned(logits, 4) || !aligned(target, 4) ||
        !aligned(grad_logits, 4))
        return HPC_RLL_EALIGN;
    if (N > kTwohotMaxN) return HPC_RLL_EUNSUPPORTED;
    if (empty) return HPC_RLL_OK;
    const CeBwdArgs p{logits, target, ws, ws + rows, g_loss, g_rows, grad_logits, (long)rows,
                      support_of(N, target_kind, transform, eps, sigma, v_min, v_max)};
    return ce_backward(p, (hipStream_t)stream);
}

extern "C" int hpc_rll_twohot_decode(const float* logits, float* value, float* expected, int64_t rows, int N, int transform,
                                     float eps, float v_min, float v_max, void* stream) {
    const bool empty = rows == 0;
    if (!empty && (!logits || !value)) return HPC_RLL_EINVAL;
    if (rows < 0 || bad_support(N, HPC_RLL_TWOHOT_KIND_TWOHOT, transform, eps, 1.f, v_min, v_max)) return HPC_RLL_EINVAL;
    if (!aligned(logits, 4) || !aligned(value, 4) || !aligned(expected, 4)) return HPC_RLL_EALIGN;
    if (N > kTwohotMaxN) return HPC_RLL_EUNSUPPORTED;
    if (empty) return HPC_RLL_OK;
    return decode(logits, value, expected, (long)rows,
                  support_of(N, HPC_RLL_TWOHOT_KIND_TWOHOT, transform, eps, 1.f, v_min, v_max), (hipStream_t)stream);
}

extern "C" int hpc_rll_twohot_encode(const float* target, float* probs, int64_t rows, int N, int target_kind, int transform,
                                     float eps, float sigma, float v_min, float v_max, void* stream) {
    const bool empty = rows == 0;
    if (!empty && (!target || !probs)) return HPC_RLL_EINVAL;
    if (rows < 0 || target_kind == HPC_RLL_TWOHOT_KIND_DENSE ||
        bad_support(N, target_kind, transform, eps, sigma, v_min, v_max))
        return HPC_RLL_EINVAL;
    if (!aligned(target, 4) || !aligned(probs, 4)) return HPC_RLL_EALIGN;
    if (N > kTwohotMaxN) return HPC_RLL_EUNSUPPORTED;
    if (empty) return HPC_RLL_OK;
    return encode(target, probs, (long)rows, support_of(N, target_kind, transform, eps, sigma, v_min, v_max),
                  (hipStream_t)stream);
}

extern "C" int hpc_rll_twohot_last_config(int* out) {
    if (!out) return HPC_RLL_EINVAL;
    g_ce_fwd.read(out);
    g_ce_bwd.read(out + kLaunchInts);
    g_decode.read(out + 2 * kLaunchInts);
    g_encode.read(out + 3 * kLaunchInts);
    return HPC_RLL_OK;
}
static_assert(HPC_RLL_TWOHOT_CONFIG_INTS == 4 * 7, "the layout documented in hpc_rll_hip.h");
