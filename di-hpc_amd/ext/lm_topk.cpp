// hpc_lm_topk -- distillation from a top-k teacher (no reference counterpart): token_topk, the k largest entries of every row
// of logits with their log-probabilities, and token_topk_kl_div, the divergence of a student's full row against such a sparse
// teacher with the gradient towards the student's logits (hpc_rll_lm_topk_*; include/hpc_rll_hip.h has the formulas).
// HOST-ONLY C++ like the other modules (common.hpp): it validates tensors, takes the outputs from torch's caching allocator and
// calls the C ABI on torch's current stream.  Nothing here synchronises with the host.
#include "rl_utils_ops.hpp"

namespace hpc_rll_ext {
namespace {

int elem_of(at::ScalarType st) { return st == at::kBFloat16 ? HPC_RLL_ELEM_BF16 : HPC_RLL_ELEM_F32; }

// what both ops ask of the logits and the temperature; returns V
int64_t check_logits(const char* op, const Tensor& logits, double temperature) {
    TORCH_CHECK(logits.defined(), "logits: expected a tensor, got None");
    const at::ScalarType st = logits.scalar_type();
    TORCH_CHECK(st == at::kFloat || st == at::kBFloat16, "logits: dtype ", st, ", expected ", at::kFloat, " or ", at::kBFloat16);
    TORCH_CHECK(logits.dim() >= 1, "logits: expected (..., V), got ", logits.sizes());
    const int64_t V = logits.size(-1);
    TORCH_CHECK(V >= 1, op, ": V = ", V, " is not supported (1 <= V <= 262144)");
    grpo_check_v(op, V);
    TORCH_CHECK(temperature > 0.0 && 1.0 / temperature <= 3.0e38, "temperature: ", temperature, ", expected > 0");
    return V;
}

std::vector<int64_t> with_last(at::IntArrayRef lead, int64_t k) {
    std::vector<int64_t> s(lead.begin(), lead.end());
    s.push_back(k);
    return s;
}

// (topk_logp (..., k) fp32, topk_index (..., k) int32); no gradient, and it says so
std::tuple<Tensor, Tensor> token_topk(const Tensor& logits, int64_t k, const OptTensor& weight, double temperature) {
    const int64_t V = check_logits("token_topk", logits, temperature);
    const at::IntArrayRef lead = logits.sizes().slice(0, logits.dim() - 1);
    Args args;
    args.add(logits, "logits", logits.sizes(), logits.scalar_type());
    args.add(weight, "weight", lead);
    TORCH_CHECK(k >= 1 && k <= std::min<int64_t>(V, HPC_RLL_LM_TOPK_MAX_K), "k: ", k, ", expected 1 <= k <= min(V, ",
                HPC_RLL_LM_TOPK_MAX_K, ") with V = ", V);
    TORCH_CHECK(!(at::GradMode::is_enabled() && (logits.requires_grad() || (has(weight) && weight->requires_grad()))),
                "token_topk has no gradient: ", logits.requires_grad() ? "logits" : "weight",
                " requires grad; call it under torch.no_grad() (it serves the teacher), or detach the operand");
    const at::Device dev = args.on_device_of(logits);
    c10::DeviceGuard g(dev);
    const std::vector<int64_t> shape = with_last(lead, k);
    Tensor logp = new_f32(shape, dev);
    Tensor index = at::empty(shape, at::TensorOptions().dtype(at::kInt).device(dev));
    check(hpc_rll_lm_topk_forward(vptr(logits), elem_of(logits.scalar_type()), fptr(weight), fmut(logp), index.data_ptr<int>(),
                                  logp.numel() / k, to_int(V, "V"), (int)k, (float)(1.0 / temperature), stream_of(dev)),
          "hpc_rll_lm_topk_forward");
    return {logp, index};
}

// kl (...) fp32; saves the logits, the teacher's entries, the weight and 12 bytes per token
struct TopkKlFn : public ag::Function<TopkKlFn> {
    static Tensor forward(ag::AutogradContext* ctx, const Tensor& logits, const Tensor& index, const Tensor& logp,
                          const OptTensor& weight, int64_t tail, double temperature) {
        const int64_t V = check_logits("token_topk_kl_div", logits, temperature);
        const at::IntArrayRef lead = logits.sizes().slice(0, logits.dim() - 1);
        TORCH_CHECK(index.defined(), "topk_index: expected a tensor, got None");
        TORCH_CHECK(logp.defined(), "topk_logp: expected a tensor, got None");
        const at::ScalarType it = index.scalar_type();
        TORCH_CHECK(it == at::kInt || it == at::kLong, "topk_index: dtype ", it, ", expected ", at::kInt, " or ", at::kLong);
        TORCH_CHECK(index.dim() == logits.dim() && index.sizes().slice(0, index.dim() - 1) == lead, "topk_index: shape ",
                    index.sizes(), ", expected ", lead, " and a last dimension k");
        const int64_t k = index.size(-1);
        TORCH_CHECK(k >= 1 && k <= HPC_RLL_LM_TOPK_MAX_K, "topk_index: k = ", k, ", expected 1 <= k <= ", HPC_RLL_LM_TOPK_MAX_K);
        Args args;
        args.add(logits, "logits", logits.sizes(), logits.scalar_type());
        args.add(index, "topk_index", index.sizes(), it);
        args.add(logp, "topk_logp", index.sizes());
        args.add(weight, "weight", lead);
        TORCH_CHECK(tail == HPC_RLL_TOPK_TAIL_RENORM || tail == HPC_RLL_TOPK_TAIL_BUCKET, "tail: ", tail,
                    ", expected 0 (renorm) or 1 (bucket)");
        const at::Device dev = args.on_device_of(logits);
        c10::DeviceGuard g(dev);
        Tensor kl = new_f32(lead, dev);
        const int64_t rows = kl.numel();
        Tensor saved = new_f32({3, rows}, dev);
        float* s = fmut(saved);
        check(hpc_rll_lm_topk_kl_forward(vptr(logits), elem_of(logits.scalar_type()), vptr(index), it == at::kLong, fptr(logp),
                                         fptr(weight), fmut(kl), s, s + rows, s + 2 * rows, rows, to_int(V, "V"), (int)k, (int)tail,
                                         (float)(1.0 / temperature), stream_of(dev)),
              "hpc_rll_lm_topk_kl_forward");
        ctx->save_for_backward({logits, index, logp, has(weight) ? *weight : undef(), saved});
        ctx->saved_data["tail"] = tail;
        ctx->saved_data["inv_t"] = 1.0 / temperature;
        return kl;
    }
    static ag::tensor_list backward(ag::AutogradContext* ctx, ag::tensor_list grads) {
        ag::tensor_list out(6);
        if (!ctx->needs_input_grad(0)) return out;
        const auto saved = ctx->get_saved_variables();
        const Tensor &logits = saved[0], &index = saved[1], &logp = saved[2], &weight = saved[3], &sv = saved[4];
        const at::Device dev = logits.device();
        c10::DeviceGuard g(dev);
        Tensor gk = grads[0].contiguous();
        req(gk, "grad_kl", dev);
        const int64_t rows = sv.size(1), V = logits.size(-1);
        const float* s = fptr(sv);
        Tensor grad = at::empty(logits.sizes(), logits.options());
        check(hpc_rll_lm_topk_kl_backward(fptr(gk), vptr(logits), elem_of(logits.scalar_type()), vptr(index),
                                          index.scalar_type() == at::kLong, fptr(logp), fptr(weight), s, s + rows, s + 2 * rows,
                                          grad.data_ptr(), rows, (int)V, (int)index.size(-1), (int)ctx->saved_data["tail"].toInt(),
                                          (float)ctx->saved_data["inv_t"].toDouble(), stream_of(dev)),
              "hpc_rll_lm_topk_kl_backward");
        out[0] = grad;
        return out;
    }
};

// The teacher's refusal stands in front of the node: inside a node's forward grad mode is off.
Tensor token_topk_kl_div(const Tensor& logits, const Tensor& index, const Tensor& logp, const OptTensor& weight, int64_t tail,
                         double temperature) {
    TORCH_CHECK(!(at::GradMode::is_enabled() && logp.defined() && logp.requires_grad()),
                "token_topk_kl_div has no gradient towards topk_logp, which requires grad; detach it or compute it under "
                "torch.no_grad()");
    return TopkKlFn::apply(logits, index, logp, weight, tail, temperature);
}

}  // namespace
}  // namespace hpc_rll_ext

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    using namespace hpc_rll_ext;
    m.doc() = "hpc_lm_topk (ROCm/HIP): top-k selection over a vocabulary row and the divergence against a top-k teacher over "
              "libhpc_rll_hip.so";
    bind_common(m);
    m.def("token_topk", &token_topk, py::arg("logits"), py::arg("k"), py::arg("weight") = py::none(), py::arg("temperature") = 1.0,
          "(topk_logp (..., k) fp32, topk_index (..., k) int32) of logits (..., V), fp32 or bf16: the k largest entries of every row, "
          "sorted descending, equal values by ascending index, with log_softmax(logits / temperature) at them.  weight (...) fp32 "
          "or None: a token with weight 0 is not read, index -1 and logp -inf.  No gradient");
    m.def("token_topk_kl_div", &token_topk_kl_div, py::arg("logits"), py::arg("topk_index"), py::arg("topk_logp"),
          py::arg("weight") = py::none(), py::arg("tail") = 0, py::arg("temperature") = 1.0,
          "kl (...) fp32 of softmax(logits / temperature), logits (..., V) fp32 or bf16, against a teacher given by topk_index "
          "(..., k) int32 or int64 and topk_logp (..., k) fp32: tail 0 renormalises the teacher over its entries, 1 adds the "
          "'everything else' outcome.  The gradient flows to logits only, in their dtype");
    m.def("lm_topk_last_config", []() {
        std::vector<int> v(HPC_RLL_LM_TOPK_CONFIG_INTS);
        check(hpc_rll_lm_topk_last_config(v.data()), "hpc_rll_lm_topk_last_config");
        return v;
    }, "hpc_rll_lm_topk_last_config: the records of the last producer, consumer-forward and consumer-backward launch");
}
