// hpc_lm_kl -- the exact divergence over the whole vocabulary between two sets of logits (no reference counterpart): forward
// KL, reverse KL and the generalized Jensen-Shannon divergence of on-policy distillation, per token, with the gradient towards
// the student's logits (hpc_rll_lm_kl_*; include/hpc_rll_hip.h has the formulas).  HOST-ONLY C++ like the other modules
// (common.hpp): it validates tensors, takes the outputs from torch's caching allocator and calls the C ABI on torch's current
// stream.  Nothing here synchronises with the host.
#include "rl_utils_ops.hpp"

namespace hpc_rll_ext {
namespace {

// kl (...) fp32; saves both logits, the weight and 12 (jsd: 16) bytes per token.  The teacher has no gradient and says so.
struct TokenKlFn : public ag::Function<TokenKlFn> {
    static Tensor forward(ag::AutogradContext* ctx, const Tensor& logits, const Tensor& teacher, const OptTensor& weight,
                          int64_t mode, double beta, double temperature) {
        TORCH_CHECK(logits.defined(), "logits: expected a tensor, got None");
        TORCH_CHECK(teacher.defined(), "teacher_logits: expected a tensor, got None");
        const at::ScalarType st = logits.scalar_type();
        TORCH_CHECK(st == at::kFloat || st == at::kBFloat16, "logits: dtype ", st, ", expected ", at::kFloat, " or ", at::kBFloat16);
        TORCH_CHECK(teacher.scalar_type() == st, "teacher_logits: dtype ", teacher.scalar_type(), ", expected ", st,
                    ", the dtype of logits (mixed element types are not supported)");
        TORCH_CHECK(logits.dim() >= 1, "logits: expected (..., V), got ", logits.sizes());
        const int64_t V = logits.size(-1);
        const at::IntArrayRef lead = logits.sizes().slice(0, logits.dim() - 1);
        Args args;
        args.add(logits, "logits", logits.sizes(), st);
        args.add(teacher, "teacher_logits", logits.sizes(), st);
        args.add(weight, "weight", lead);
        grpo_check_v("token_kl_div", V);
        TORCH_CHECK(mode == HPC_RLL_KL_FORWARD || mode == HPC_RLL_KL_REVERSE || mode == HPC_RLL_KL_JSD, "mode: ", mode,
                    ", expected 0 (forward), 1 (reverse) or 2 (jsd)");
        TORCH_CHECK(mode != HPC_RLL_KL_JSD || (beta > 0.0 && beta < 1.0), "beta: ", beta, ", expected 0 < beta < 1 for jsd");
        TORCH_CHECK(temperature > 0.0 && 1.0 / temperature <= 3.0e38, "temperature: ", temperature, ", expected > 0");
        const at::Device dev = args.on_device_of(logits);
        c10::DeviceGuard g(dev);
        const bool jsd = mode == HPC_RLL_KL_JSD;
        Tensor kl = new_f32(lead, dev);
        const int64_t rows = kl.numel();   // V == 0 still has them: zeros
        Tensor saved = new_f32({jsd ? 3 : 2, rows}, dev);
        float* s = fmut(saved);
        check(hpc_rll_lm_kl_forward(vptr(logits), vptr(teacher), elem_of(st), fptr(weight), fmut(kl), s, s + rows,
                                    jsd ? s + 2 * rows : nullptr, rows, to_int(V, "V"), (int)mode, (float)beta,
                                    (float)(1.0 / temperature), stream_of(dev)),
              "hpc_rll_lm_kl_forward");
        ctx->save_for_backward({logits, teacher, has(weight) ? *weight : undef(), kl, saved});
        ctx->saved_data["mode"] = mode;
        ctx->saved_data["beta"] = beta;
        ctx->saved_data["inv_t"] = 1.0 / temperature;
        return kl;
    }
    static ag::tensor_list backward(ag::AutogradContext* ctx, ag::tensor_list grads) {
        ag::tensor_list out(6);
        if (!ctx->needs_input_grad(0)) return out;
        const auto saved = ctx->get_saved_variables();
        const Tensor &logits = saved[0], &teacher = saved[1], &weight = saved[2], &kl = saved[3], &sv = saved[4];
        const at::Device dev = logits.device();
        c10::DeviceGuard g(dev);
        Tensor gk = grads[0].contiguous();
        req(gk, "grad_kl", dev);
        const int64_t rows = kl.numel(), V = logits.size(-1);
        const int64_t mode = ctx->saved_data["mode"].toInt();
        const float* s = fptr(sv);
        Tensor grad = at::empty(logits.sizes(), logits.options());
        check(hpc_rll_lm_kl_backward(fptr(gk), vptr(logits), vptr(teacher), elem_of(logits.scalar_type()), fptr(weight), fptr(kl), s,
                                     s + rows, mode == HPC_RLL_KL_JSD ? s + 2 * rows : nullptr, grad.data_ptr(), rows, (int)V,
                                     (int)mode, (float)ctx->saved_data["beta"].toDouble(),
                                     (float)ctx->saved_data["inv_t"].toDouble(), stream_of(dev)),
              "hpc_rll_lm_kl_backward");
        out[0] = grad;
        return out;
    }
    static int elem_of(at::ScalarType st) { return st == at::kBFloat16 ? HPC_RLL_ELEM_BF16 : HPC_RLL_ELEM_F32; }
};

// The teacher's refusal stands in front of the node: inside a node's forward grad mode is off.
Tensor token_kl_div(const Tensor& logits, const Tensor& teacher, const OptTensor& weight, int64_t mode, double beta,
                    double temperature) {
    TORCH_CHECK(!(at::GradMode::is_enabled() && teacher.defined() && teacher.requires_grad()),
                "token_kl_div has no gradient towards teacher_logits, which requires grad; detach it or compute it under "
                "torch.no_grad()");
    return TokenKlFn::apply(logits, teacher, weight, mode, beta, temperature);
}

}  // namespace
}  // namespace hpc_rll_ext

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    using namespace hpc_rll_ext;
    m.doc() = "hpc_lm_kl (ROCm/HIP): full-vocabulary KL / JSD between two sets of logits over libhpc_rll_hip.so";
    bind_common(m);
    m.def("token_kl_div", &token_kl_div, py::arg("logits"), py::arg("teacher_logits"),
          py::arg("weight") = py::none(), py::arg("mode") = 0, py::arg("beta") = 0.5, py::arg("temperature") = 1.0,
          "kl (...) fp32 of logits and teacher_logits (..., V), both fp32 or both bf16: mode 0 KL(q||p), 1 KL(p||q), 2 the "
          "generalized JSD beta KL(q||m) + (1 - beta) KL(p||m), with p = softmax(logits / temperature), q = softmax(teacher_logits "
          "/ temperature), m = beta q + (1 - beta) p.  weight (...) fp32 or None: a token with weight 0 is not read, kl = 0.  "
          "The gradient flows to logits only, in their dtype");
    m.def("lm_kl_last_config", []() {
        std::vector<int> v(HPC_RLL_LM_KL_CONFIG_INTS);
        check(hpc_rll_lm_kl_last_config(v.data()), "hpc_rll_lm_kl_last_config");
        return v;
    }, "hpc_rll_lm_kl_last_config: the records of the last forward and backward launch, as the header documents");
}
