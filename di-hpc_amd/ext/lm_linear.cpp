// hpc_lm_linear -- the language-model head fused with its bf16 matrix product (no reference counterpart): the log-probability
// and the entropy of given tokens from hidden states and the head's weight (hpc_rll_lm_linear_*; include/hpc_rll_hip.h has the
// formulas).  HOST-ONLY C++ like the other modules (common.hpp): it validates tensors, takes the outputs and the workspace
// from torch's caching allocator and calls the C ABI on torch's current stream.  linear_token_log_prob is a plain function
// for the policies evaluated without gradient (it says so instead of dropping one); lm_head_log_prob is the autograd node for
// the policy being trained.  Nothing here synchronises with the host.
#include "rl_utils_ops.hpp"

namespace hpc_rll_ext {
namespace {

// what is checked on host tensors too, in this order: dtype, shape, the limits, the gradient, contiguity; then the device
void check_operand(const Tensor& t, const char* name, at::ScalarType dtype) {
    TORCH_CHECK(t.defined(), name, ": expected a tensor, got None");
    TORCH_CHECK(t.scalar_type() == dtype, name, ": dtype ", t.scalar_type(), ", expected ", dtype);
}
void check_on(const Tensor& t, const char* name, const at::Device& dev, size_t align) {
    TORCH_CHECK(t.is_cuda(), name, ": must live on a GPU (hpc_rll has no CPU path)");
    TORCH_CHECK(t.device() == dev, name, ": on ", t.device(), ", expected ", dev);
    TORCH_CHECK(t.numel() == 0 || reinterpret_cast<uintptr_t>(t.const_data_ptr()) % align == 0, name, ": its base must lie on ",
                align, " bytes");
}

// The checks both functions make on their operands; `refuse_grad`: the plain function's refusal, at its place in the order.
struct Dims { int64_t rows, H, V; at::Device dev; };
Dims check_all(const Tensor& hidden, const Tensor& lm_weight, const Tensor& action, const OptTensor& weight, double temperature,
               bool refuse_grad) {
    check_operand(hidden, "hidden", at::kBFloat16);
    check_operand(lm_weight, "lm_weight", at::kBFloat16);
    check_operand(action, "action", at::kLong);
    if (has(weight)) check_operand(*weight, "weight", at::kFloat);
    TORCH_CHECK(hidden.dim() >= 1, "hidden: expected (..., H), got ", hidden.sizes());
    TORCH_CHECK(lm_weight.dim() == 2, "lm_weight: expected (V, H), got ", lm_weight.sizes());
    const int64_t H = hidden.size(-1), V = lm_weight.size(0);
    const at::IntArrayRef lead = hidden.sizes().slice(0, hidden.dim() - 1);
    TORCH_CHECK(lm_weight.size(1) == H, "lm_weight: shape ", lm_weight.sizes(), ", expected (V, ", H, ") for hidden ", hidden.sizes());
    TORCH_CHECK(action.sizes() == lead, "action: shape ", action.sizes(), ", expected ", lead);
    if (has(weight)) TORCH_CHECK(weight->sizes() == lead, "weight: shape ", weight->sizes(), ", expected ", lead);
    TORCH_CHECK(H >= 32 && H <= 16384 && H % 32 == 0, "hidden: H = ", H, " is not supported (32 <= H <= 16384, H % 32 == 0)");
    TORCH_CHECK(V >= 1, "lm_weight: V = ", V, " is not supported (1 <= V <= 262144)");
    grpo_check_v("lm_weight", V);
    TORCH_CHECK(temperature > 0.0 && 1.0 / temperature <= 3.0e38, "temperature: ", temperature, ", expected > 0");
    TORCH_CHECK(!(refuse_grad && at::GradMode::is_enabled() && (hidden.requires_grad() || lm_weight.requires_grad())),
                "linear_token_log_prob has no gradient: ", hidden.requires_grad() ? "hidden" : "lm_weight",
                " requires grad; call it under torch.no_grad() (it serves the old and the reference policy), or detach the operand");
    TORCH_CHECK(hidden.is_contiguous(), "hidden: must be contiguous");
    TORCH_CHECK(lm_weight.is_contiguous(), "lm_weight: must be contiguous");
    TORCH_CHECK(action.is_contiguous(), "action: must be contiguous");
    if (has(weight)) TORCH_CHECK(weight->is_contiguous(), "weight: must be contiguous");
    const at::Device dev = hidden.device();
    check_on(hidden, "hidden", dev, 16);
    check_on(lm_weight, "lm_weight", dev, 16);
    check_on(action, "action", dev, 8);
    if (has(weight)) check_on(*weight, "weight", dev, 4);
    return {action.numel(), H, V, dev};
}

Tensor bytes(int64_t n, const at::Device& dev) { return at::empty({n}, at::TensorOptions().dtype(at::kByte).device(dev)); }

// logp, the entropy when asked for and lse when `want_lse`, each (...) fp32; no rows: empty tensors, nothing launched
std::array<Tensor, 3> forward_launch(const Dims& d, const Tensor& hidden, const Tensor& lm_weight, const Tensor& action,
                                     const OptTensor& weight, double temperature, bool return_entropy, bool want_lse) {
    const at::IntArrayRef lead = action.sizes();
    Tensor logp = new_f32(lead, d.dev), ent = return_entropy ? new_f32(lead, d.dev) : undef();
    Tensor lse = want_lse ? new_f32(lead, d.dev) : undef();
    if (d.rows > 0) {
        Tensor ws = bytes(hpc_rll_lm_linear_workspace_bytes(d.rows, 0), d.dev);
        check(hpc_rll_lm_linear_forward_lse(vptr(hidden), vptr(lm_weight), iptr(action), fptr(weight), d.rows, (int)d.H, (int)d.V,
                                            (float)(1.0 / temperature), 0, ws.data_ptr(), fmut(logp), fmut(ent), fmut(lse),
                                            stream_of(d.dev)),
              "hpc_rll_lm_linear_forward");
    }
    return {logp, ent, lse};
}

std::vector<Tensor> linear_token_log_prob(const Tensor& hidden, const Tensor& lm_weight, const Tensor& action,
                                          const OptTensor& weight, double temperature, bool return_entropy) {
    const Dims d = check_all(hidden, lm_weight, action, weight, temperature, true);
    c10::DeviceGuard g(d.dev);
    const auto out = forward_launch(d, hidden, lm_weight, action, weight, temperature, return_entropy, false);
    if (return_entropy) return {out[0], out[1]};
    return {out[0]};
}

// The differentiable head: saves the operands, lse and the entropy (8 bytes per row); the backward walks the vocabulary in
// chunks (hpc_rll_lm_linear_backward) and computes only the gradients that are needed.
struct LmHeadFn : public ag::Function<LmHeadFn> {
    static ag::tensor_list forward(ag::AutogradContext* ctx, const Tensor& hidden, const Tensor& lm_weight, const Tensor& action,
                                   const OptTensor& weight, double temperature, bool return_entropy, int64_t chunk) {
        const Dims d = check_all(hidden, lm_weight, action, weight, temperature, false);
        c10::DeviceGuard g(d.dev);
        const auto out = forward_launch(d, hidden, lm_weight, action, weight, temperature, return_entropy, true);
        ctx->save_for_backward({hidden, lm_weight, action, has(weight) ? *weight : undef(), out[2], out[1]});
        ctx->saved_data["inv_t"] = 1.0 / temperature;
        ctx->saved_data["chunk"] = chunk;
        ctx->set_materialize_grads(false);
        if (return_entropy) return {out[0], out[1]};
        return {out[0]};
    }
    static ag::tensor_list backward(ag::AutogradContext* ctx, ag::tensor_list grads) {
        ag::tensor_list out(7);
        const auto saved = ctx->get_saved_variables();
        const Tensor &hidden = saved[0], &lm_weight = saved[1], &action = saved[2], &weight = saved[3], &lse = saved[4], &ent = saved[5];
        const bool dh = ctx->needs_input_grad(0), dw = ctx->needs_input_grad(1);
        const at::Device dev = hidden.device();
        c10::DeviceGuard g(dev);
        const int64_t rows = action.numel(), H = hidden.size(-1), V = lm_weight.size(0);
        Tensor g_lp = grads[0].defined() ? grads[0].contiguous() : undef();
        Tensor g_h = grads.size() > 1 && grads[1].defined() ? grads[1].contiguous() : undef();
        if (g_lp.defined()) req(g_lp, "grad_logp", dev);
        if (g_h.defined()) req(g_h, "grad_entropy", dev);
        if (rows == 0 || (!g_lp.defined() && !g_h.defined())) {   // nothing to propagate: zeros, nothing launched
            if (dh) out[0] = at::zeros_like(hidden);
            if (dw) out[1] = at::zeros_like(lm_weight);
            return out;
        }
        const int chunk = (int)ctx->saved_data["chunk"].toInt();
        const int64_t nws = hpc_rll_lm_linear_backward_workspace_bytes(rows, (int)H, (int)V, chunk, dh, dw);
        check(nws < 0 ? (int)nws : 0, "hpc_rll_lm_linear_backward_workspace_bytes");
        Tensor ws = bytes(std::max<int64_t>(nws, 16), dev);
        if (dh) out[0] = at::empty_like(hidden);
        if (dw) out[1] = at::empty_like(lm_weight);
        check(hpc_rll_lm_linear_backward(fptr(g_lp), fptr(g_h), vptr(hidden), vptr(lm_weight), iptr(action), fptr(weight), fptr(lse),
                                         fptr(ent), rows, (int)H, (int)V, (float)ctx->saved_data["inv_t"].toDouble(), chunk,
                                         ws.data_ptr(), dh ? out[0].data_ptr() : nullptr, dw ? out[1].data_ptr() : nullptr,
                                         stream_of(dev)),
              "hpc_rll_lm_linear_backward");
        return out;
    }
};

std::vector<Tensor> lm_head_log_prob(const Tensor& hidden, const Tensor& lm_weight, const Tensor& action, const OptTensor& weight,
                                     double temperature, bool return_entropy, int64_t chunk) {
    TORCH_CHECK(chunk >= 0 && chunk % 128 == 0 && chunk <= INT32_MAX, "chunk: ", chunk, ", expected 0 (by rule) or a multiple of 128");
    if (!(at::GradMode::is_enabled() && hidden.defined() && lm_weight.defined() &&
          (hidden.requires_grad() || lm_weight.requires_grad()))) {   // no gradient to serve: the plain forward
        at::NoGradGuard ng;
        return linear_token_log_prob(hidden, lm_weight, action, weight, temperature, return_entropy);
    }
    return LmHeadFn::apply(hidden, lm_weight, action, weight, temperature, return_entropy, chunk);
}

}  // namespace
}  // namespace hpc_rll_ext

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    using namespace hpc_rll_ext;
    m.doc() = "hpc_lm_linear (ROCm/HIP): the language-model head fused with its bf16 matrix product over libhpc_rll_hip.so";
    bind_common(m);
    m.def("linear_token_log_prob", &linear_token_log_prob, py::arg("hidden"), py::arg("lm_weight"), py::arg("action"),
          py::arg("weight") = py::none(), py::arg("temperature") = 1.0, py::arg("return_entropy") = false,
          "[logp (...)] or [logp, entropy] of hidden (..., H) bf16, lm_weight (V, H) bf16 and action (...) int64: with x = (hidden "
          "lm_weight^T) / temperature held in fp32, logp = x[a] - logsumexp(x) and entropy = logsumexp(x) - sum p x.  No logits "
          "tensor is formed.  No gradient (lm_head_log_prob has it)");
    m.def("lm_head_log_prob", &lm_head_log_prob, py::arg("hidden"), py::arg("lm_weight"), py::arg("action"),
          py::arg("weight") = py::none(), py::arg("temperature") = 1.0, py::arg("return_entropy") = false, py::arg("chunk") = 0,
          "linear_token_log_prob with its gradient towards hidden and lm_weight (bf16, only for the operands that require grad): "
          "the backward recomputes the logits in vocabulary chunks of `chunk` columns (0 = by rule) and forms dhidden = G W and "
          "dW = G^T hidden with one bf16 product kernel.  The same kernels and bits as linear_token_log_prob in the forward");
    m.def("lm_linear_backward_last_config", []() {
        std::vector<int> v(HPC_RLL_LM_LINEAR_BACKWARD_CONFIG_INTS);
        check(hpc_rll_lm_linear_backward_last_config(v.data()), "hpc_rll_lm_linear_backward_last_config");
        return v;
    }, "hpc_rll_lm_linear_backward_last_config: the record of the last backward and of the last product, as the header documents");
    m.def("lm_linear_last_config", []() {
        std::vector<int> v(HPC_RLL_LM_LINEAR_CONFIG_INTS);
        check(hpc_rll_lm_linear_last_config(v.data()), "hpc_rll_lm_linear_last_config");
        return v;
    }, "hpc_rll_lm_linear_last_config: the record of the last launch, as the header documents");
}
