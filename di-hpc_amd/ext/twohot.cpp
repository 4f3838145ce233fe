// hpc_twohot -- the categorical value losses (no reference counterpart): the cross-entropy of a row of logits against the
// two-hot or HL-Gauss encoding of a scalar target, or against a row of probabilities, the decoded expectation and the dense
// target rows (hpc_rll_twohot_*; include/hpc_rll_hip.h has the formulas).  HOST-ONLY C++ like the other four modules
// (common.hpp): it validates tensors, takes outputs and scratch from torch's caching allocator and calls the C ABI on torch's
// current stream.  Nothing here synchronises with the host.
#include "rl_utils_ops.hpp"

namespace hpc_rll_ext {
namespace {

// the scalars of a support and a target kind as python passes them
struct CeKind { int64_t kind, transform; double eps, sigma, v_min, v_max; };

std::vector<int64_t> lead_of(const Tensor& logits) {
    TORCH_CHECK(logits.defined(), "logits: expected a tensor, got None");
    TORCH_CHECK(logits.dim() >= 1, "logits: expected (..., N), got ", logits.sizes());
    return std::vector<int64_t>(logits.sizes().begin(), logits.sizes().end() - 1);
}

int64_t rows_of(const std::vector<int64_t>& lead) {
    int64_t rows = 1;
    for (int64_t n : lead) rows *= n;
    return rows;
}

void check_kind(const char* op, const CeKind& k, int64_t N, bool dense_allowed) {
    const bool dense = k.kind == HPC_RLL_TWOHOT_KIND_DENSE;
    TORCH_CHECK(k.kind == HPC_RLL_TWOHOT_KIND_TWOHOT || k.kind == HPC_RLL_TWOHOT_KIND_HLGAUSS || (dense && dense_allowed), op,
                ": unknown target kind ", k.kind);
    TORCH_CHECK(N <= 1024, op, ": rows of at most 1024 logits are implemented, got ", N);
    if (dense) {
        TORCH_CHECK(N >= 1, op, ": expected at least one logit per row, got ", N);
        return;
    }
    TORCH_CHECK(N >= 2, op, ": a support has at least 2 atoms, got ", N);
    TORCH_CHECK(k.transform >= HPC_RLL_TWOHOT_PHI_IDENTITY && k.transform <= HPC_RLL_TWOHOT_PHI_SYMLOG, op,
                ": unknown transform ", k.transform);
    TORCH_CHECK(k.v_max > k.v_min, op, ": expected v_max > v_min, got [", k.v_min, ", ", k.v_max, "]");
    TORCH_CHECK(k.transform != HPC_RLL_TWOHOT_PHI_H || k.eps > 0.0, op, ": h needs eps > 0, got ", k.eps);
    TORCH_CHECK(k.kind != HPC_RLL_TWOHOT_KIND_HLGAUSS || k.sigma > 0.0, op, ": HL-Gauss needs sigma > 0, got ", k.sigma);
}

// ================================================================================================== the three losses
// (loss (1,), ell (...)) from logits (..., N), target (...) or, dense, (..., N), weight (...) or None.  `reduced`: loss
// carries the gradient and ell is detached; otherwise ell carries it and takes a per-row upstream gradient (loss is then
// the plain weighted sum, detached).  Differentiable wrt logits; saves logits, target and the workspace (8 bytes per row).
struct CatCeFn : public ag::Function<CatCeFn> {
    static ag::tensor_list forward(ag::AutogradContext* ctx, const Tensor& logits, const Tensor& target,
                                   const OptTensor& weight, int64_t kind, int64_t transform, double eps, double sigma,
                                   double v_min, double v_max, bool reduced, std::optional<double> scale) {
        const std::vector<int64_t> lead = lead_of(logits);
        const int64_t N = logits.sizes().back(), rows = rows_of(lead);
        const CeKind k{kind, transform, eps, sigma, v_min, v_max};
        Args args;
        args.add(logits, "logits", logits.sizes());
        if (kind == HPC_RLL_TWOHOT_KIND_DENSE) args.add(target, "target_probs", logits.sizes());
        else args.add(target, "target", lead);
        args.add(weight, "weight", lead);
        check_kind("categorical_ce", k, N, true);
        const at::Device dev = args.on_device_of(logits);
        c10::DeviceGuard g(dev);
        Tensor loss = new_f32({1}, dev), ell = new_f32(lead, dev);
        Tensor ws = new_f32({rows > 0 ? hpc_rll_twohot_workspace_floats(rows) : 0}, dev);
        check(hpc_rll_twohot_ce_forward(fptr(logits), fptr(target), fptr(weight), fmut(loss), fmut(ell), fmut(ws), rows,
                                        (int)N, (int)kind, (int)transform, (float)eps, (float)sigma, (float)v_min,
                                        (float)v_max, reduced ? loss_scale(scale, rows) : 1.f, stream_of(dev)),
              "hpc_rll_twohot_ce_forward");
        ctx->save_for_backward({logits, target, ws});
        ctx->saved_data["kind"] = kind;
        ctx->saved_data["transform"] = transform;
        ctx->saved_data["eps"] = eps;
        ctx->saved_data["sigma"] = sigma;
        ctx->saved_data["v_min"] = v_min;
        ctx->saved_data["v_max"] = v_max;
        ctx->saved_data["reduced"] = reduced;
        ctx->mark_non_differentiable({reduced ? ell : loss});
        return {loss, ell};
    }
    static ag::tensor_list backward(ag::AutogradContext* ctx, ag::tensor_list grads) {
        ag::tensor_list out(11);
        if (!ctx->needs_input_grad(0)) return out;
        const auto saved = ctx->get_saved_variables();
        const Tensor &logits = saved[0], &target = saved[1], &ws = saved[2];
        const at::Device dev = logits.device();
        c10::DeviceGuard g(dev);
        Tensor g_loss, g_rows;
        if (ctx->saved_data["reduced"].toBool()) {
            g_loss = grad1(grads[0], dev, "grad_loss");
        } else {
            g_rows = grads[1].contiguous();
            req(g_rows, "grad_ell", dev);
        }
        Tensor grad = new_f32(logits.sizes(), dev);
        check(hpc_rll_twohot_ce_backward(fptr(g_loss), fptr(g_rows), fptr(ws), fptr(logits), fptr(target), fmut(grad),
                                         logits.numel() / logits.sizes().back(),
                                         (int)logits.sizes().back(), (int)ctx->saved_data["kind"].toInt(),
                                         (int)ctx->saved_data["transform"].toInt(), (float)ctx->saved_data["eps"].toDouble(),
                                         (float)ctx->saved_data["sigma"].toDouble(), (float)ctx->saved_data["v_min"].toDouble(),
                                         (float)ctx->saved_data["v_max"].toDouble(), stream_of(dev)),
              "hpc_rll_twohot_ce_backward");
        out[0] = grad;
        return out;
    }
};

// value (...) = phi^-1(E) and, when asked for, E (...) of logits (..., N); forward only
std::vector<Tensor> categorical_decode(const Tensor& logits, int64_t transform, double eps, double v_min, double v_max,
                                       bool return_expected) {
    const std::vector<int64_t> lead = lead_of(logits);
    const int64_t N = logits.sizes().back();
    Args args;
    args.add(logits, "logits", logits.sizes());
    check_kind("categorical_decode", CeKind{HPC_RLL_TWOHOT_KIND_TWOHOT, transform, eps, 1.0, v_min, v_max}, N, false);
    const at::Device dev = args.on_device_of(logits);
    c10::DeviceGuard g(dev);
    Tensor value = new_f32(lead, dev), expected = return_expected ? new_f32(lead, dev) : undef();
    check(hpc_rll_twohot_decode(fptr(logits), fmut(value), fmut(expected), rows_of(lead), (int)N, (int)transform, (float)eps,
                                (float)v_min, (float)v_max, stream_of(dev)),
          "hpc_rll_twohot_decode");
    if (return_expected) return {value, expected};
    return {value};
}

// probs (..., n): the two-hot or HL-Gauss rows of target (...)
Tensor categorical_encode(const Tensor& target, int64_t n, int64_t kind, int64_t transform, double eps, double sigma,
                          double v_min, double v_max) {
    TORCH_CHECK(target.defined(), "target: expected a tensor, got None");
    Args args;
    args.add(target, "target", target.sizes());
    check_kind("categorical_encode", CeKind{kind, transform, eps, sigma, v_min, v_max}, n, false);
    const at::Device dev = args.on_device_of(target);
    c10::DeviceGuard g(dev);
    std::vector<int64_t> shape(target.sizes().begin(), target.sizes().end());
    shape.push_back(n);
    Tensor probs = new_f32(shape, dev);
    check(hpc_rll_twohot_encode(fptr(target), fmut(probs), target.numel(), (int)n, (int)kind, (int)transform, (float)eps,
                                (float)sigma, (float)v_min, (float)v_max, stream_of(dev)),
          "hpc_rll_twohot_encode");
    return probs;
}

}  // namespace
}  // namespace hpc_rll_ext

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    using namespace hpc_rll_ext;
    m.doc() = "hpc_twohot (ROCm/HIP): categorical value losses (two-hot, HL-Gauss, dense) over libhpc_rll_hip.so";
    bind_common(m);
    m.def("categorical_ce", applier<CatCeFn>(&CatCeFn::forward), py::arg("logits"), py::arg("target"),
          py::arg("weight") = py::none(), py::arg("kind") = 0, py::arg("transform") = 0, py::arg("eps") = 1e-3,
          py::arg("sigma") = 1.0, py::arg("v_min") = 0.0, py::arg("v_max") = 1.0, py::arg("reduced") = true,
          py::arg("scale") = py::none(),
          "(loss (1,), ell (...)) of logits (..., N) against target: kind 0 the two-hot and 1 the HL-Gauss encoding of scalars "
          "(...) on the support of N atoms in [v_min, v_max] under transform 0 identity, 1 h (eps), 2 symlog; kind 2 rows of "
          "probabilities (..., N).  ell = lse(x) - sum t x per row (0 where weight is 0), loss = scale sum weight ell with "
          "scale = 1/rows unless given.  reduced: the gradient flows from loss; otherwise from ell, per row, and scale is 1.  "
          "Differentiable wrt logits");
    m.def("categorical_decode", &categorical_decode, py::arg("logits"), py::arg("transform") = 0, py::arg("eps") = 1e-3,
          py::arg("v_min") = 0.0, py::arg("v_max") = 1.0, py::arg("return_expected") = false,
          "[value (...)] or [value, expected] of logits (..., N): expected = sum softmax(logits) v, value = phi^-1(expected); "
          "forward only");
    m.def("categorical_encode", &categorical_encode, py::arg("target"), py::arg("n"), py::arg("kind") = 0,
          py::arg("transform") = 0, py::arg("eps") = 1e-3, py::arg("sigma") = 1.0, py::arg("v_min") = 0.0,
          py::arg("v_max") = 1.0, "probs (..., n): the two-hot (kind 0) or HL-Gauss (kind 1) rows of the scalars target (...)");
    m.def("twohot_last_config", []() {
        std::vector<int> v(HPC_RLL_TWOHOT_CONFIG_INTS);
        check(hpc_rll_twohot_last_config(v.data()), "hpc_rll_twohot_last_config");
        return v;
    }, "hpc_rll_twohot_last_config: the dispatch record of the last forward, backward, decode and encode, as the header documents");
}
