// hpc_lm_linear -- the language-model head fused with its bf16 matrix product (no reference counterpart): the log-probability
// and the entropy of given tokens from hidden states and the head's weight (hpc_rll_lm_linear_*; include/hpc_rll_hip.h has the
// formulas).  HOST-ONLY C++ like the other modules (common.hpp): it validates tensors, takes the outputs and the workspace
// from torch's caching allocator and calls the C ABI on torch's current stream.  A plain function, no autograd node: the op has
// no gradient and says so instead of dropping one.  Nothing here synchronises with the host.
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

std::vector<Tensor> linear_token_log_prob(const Tensor& hidden, const Tensor& lm_weight, const Tensor& action,
                                          const OptTensor& weight, double temperature, bool return_entropy) {
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
    TORCH_CHECK(!(at::GradMode::is_enabled() && (hidden.requires_grad() || lm_weight.requires_grad())),
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
    c10::DeviceGuard g(dev);
    const int64_t rows = action.numel();
    Tensor logp = new_f32(lead, dev), ent = return_entropy ? new_f32(lead, dev) : undef();
    if (rows > 0) {   // no rows: empty tensors, nothing launched
        Tensor ws = at::empty({hpc_rll_lm_linear_workspace_bytes(rows, 0)}, at::TensorOptions().dtype(at::kByte).device(dev));
        check(hpc_rll_lm_linear_forward(vptr(hidden), vptr(lm_weight), iptr(action), fptr(weight), rows, (int)H, (int)V,
                                        (float)(1.0 / temperature), 0, ws.data_ptr(), fmut(logp), fmut(ent), stream_of(dev)),
              "hpc_rll_lm_linear_forward");
    }
    if (return_entropy) return {logp, ent};
    return {logp};
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
          "tensor is formed.  No gradient");
    m.def("lm_linear_last_config", []() {
        std::vector<int> v(HPC_RLL_LM_LINEAR_CONFIG_INTS);
        check(hpc_rll_lm_linear_last_config(v.data()), "hpc_rll_lm_linear_last_config");
        return v;
    }, "hpc_rll_lm_linear_last_config: the record of the last launch, as the header documents");
}
