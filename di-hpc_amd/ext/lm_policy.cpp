// hpc_lm_policy -- the policy losses of language-model RL on per-token log-probabilities (no reference counterpart): the
// clipped / CISPO objective with a token or sequence ratio, the k1 / k2 / k3 reference KL, value loss and entropy over (B,S)
// operands, with the gradient towards logp, entropy and value_new (hpc_rll_lm_policy_*; include/hpc_rll_hip.h has the formulas).
// HOST-ONLY C++ like the other modules (common.hpp): it validates tensors, takes the outputs and the workspace from torch's
// caching allocator and calls the C ABI on torch's current stream.  Nothing here synchronises with the host.
#include "rl_utils_ops.hpp"

namespace hpc_rll_ext {
namespace {

constexpr int kWantP = 1, kWantK = 2, kWantE = 4, kWantV = 8;

// (policy_loss, kl_loss, value_loss, entropy, approx_kl, mean_ratio, clipfrac), (1,) each; the first four are differentiable.
// `want`: the coefficient rows the backward will need, decided by the caller below while grad mode is still on.
struct LmPolicyFn : public ag::Function<LmPolicyFn> {
    static ag::tensor_list forward(ag::AutogradContext* ctx, const Tensor& logp, const Tensor& old_logp, const Tensor& adv,
                                   const OptTensor& weight, const OptTensor& ref_logp, const OptTensor& entropy,
                                   const OptTensor& value_new, const OptTensor& value_old, const OptTensor& ret, int64_t ratio,
                                   int64_t objective, double clip_low, double clip_high, std::optional<double> dual_clip,
                                   int64_t kl, int64_t agg, std::optional<double> norm_len, std::optional<double> value_clip,
                                   int64_t mapping, int64_t want) {
        TORCH_CHECK(logp.defined(), "logp: expected a tensor, got None");
        TORCH_CHECK(logp.dim() == 2, "logp: expected (B,S), got ", logp.sizes());
        const int64_t B = logp.size(0), S = logp.size(1);
        TORCH_CHECK(adv.defined(), "adv: expected a tensor, got None");
        const bool per_seq = adv.dim() == 1;
        Args args;
        args.add(logp, "logp", {B, S});
        args.add(old_logp, "old_logp", {B, S});
        if (per_seq) args.add(adv, "adv", {B});
        else args.add(adv, "adv", {B, S});
        args.add(weight, "weight", {B, S});
        args.add(ref_logp, "ref_logp", {B, S});
        args.add(entropy, "entropy", {B, S});
        const int nval = (int)has(value_new) + (int)has(value_old) + (int)has(ret);
        TORCH_CHECK(nval == 0 || nval == 3, "lm_policy_loss: value_new, value_old and ret are given all three or none (got ", nval,
                    " of them)");
        args.add(value_new, "value_new", {B, S});
        args.add(value_old, "value_old", {B, S});
        args.add(ret, "ret", {B, S});
        TORCH_CHECK(ratio == HPC_RLL_POLICY_RATIO_TOKEN || ratio == HPC_RLL_POLICY_RATIO_SEQUENCE, "ratio: ", ratio,
                    ", expected 0 (token) or 1 (sequence)");
        TORCH_CHECK(objective == HPC_RLL_POLICY_OBJ_CLIP || objective == HPC_RLL_POLICY_OBJ_CISPO, "objective: ", objective,
                    ", expected 0 (clip) or 1 (cispo)");
        TORCH_CHECK(kl >= HPC_RLL_POLICY_KL_K1 && kl <= HPC_RLL_POLICY_KL_K3, "kl: ", kl, ", expected 0 (k1), 1 (k2) or 2 (k3)");
        TORCH_CHECK(agg >= HPC_RLL_POLICY_AGG_TOKEN && agg <= HPC_RLL_POLICY_AGG_CONSTANT, "agg: ", agg,
                    ", expected 0 (token), 1 (sequence) or 2 (constant)");
        TORCH_CHECK(mapping >= HPC_RLL_POLICY_MAP_RULE && mapping <= HPC_RLL_POLICY_MAP_CHUNK, "mapping: ", mapping,
                    ", expected 0 (by rule), 1 (wave) or 2 (chunk)");
        TORCH_CHECK(clip_low >= 0.0 && clip_low <= 3.0e38, "clip_low: ", clip_low, ", expected a finite value >= 0");
        TORCH_CHECK(clip_high >= 0.0 && clip_high <= 3.0e38, "clip_high: ", clip_high, ", expected a finite value >= 0");
        TORCH_CHECK(!dual_clip.has_value() || *dual_clip > 1.0, "dual_clip: expected None or a value above 1, got ", *dual_clip);
        TORCH_CHECK(!dual_clip.has_value() || objective == HPC_RLL_POLICY_OBJ_CLIP, "dual_clip: must be None with objective='cispo'");
        if (agg == HPC_RLL_POLICY_AGG_CONSTANT) {
            TORCH_CHECK(norm_len.has_value() && *norm_len > 0.0 && *norm_len <= 3.0e38, "norm_len: agg='constant' needs a positive value");
        } else {
            TORCH_CHECK(!norm_len.has_value(), "norm_len: only agg='constant' takes it, got ", *norm_len);
        }
        TORCH_CHECK(!value_clip.has_value() || *value_clip >= 0.0, "value_clip: expected None or a value >= 0, got ", *value_clip);
        const at::Device dev = args.on_device_of(logp);
        c10::DeviceGuard g(dev);
        const bool empty = B == 0 || S == 0;
        const int Bi = to_int(B, "B"), Si = to_int(S, "S");
        Tensor out8, ws;
        if (empty) {
            out8 = at::zeros({8}, at::TensorOptions().dtype(at::kFloat).device(dev));   // nothing is launched by this library
        } else {
            out8 = new_f32({8}, dev);
            ws = new_f32({hpc_rll_lm_policy_workspace_floats(Bi, Si, (int)want)}, dev);
            check(hpc_rll_lm_policy_forward(fptr(logp), fptr(old_logp), fptr(adv), per_seq ? 1 : 0, fptr(weight), fptr(ref_logp),
                                            fptr(entropy), fptr(value_new), fptr(value_old), fptr(ret), fmut(out8), fmut(ws), Bi,
                                            Si, (int)ratio, (int)objective, (float)clip_low, (float)clip_high,
                                            dual_clip.has_value() ? (float)*dual_clip : 0.f, (int)kl, (int)agg,
                                            norm_len.has_value() ? (float)*norm_len : 0.f, value_clip.has_value() ? 1 : 0,
                                            value_clip.has_value() ? (float)*value_clip : 0.f, (int)want, (int)mapping,
                                            stream_of(dev)),
                  "hpc_rll_lm_policy_forward");
            ctx->save_for_backward({ws});
        }
        ctx->saved_data["B"] = B;
        ctx->saved_data["S"] = S;
        ctx->saved_data["want"] = want;
        ctx->saved_data["agg"] = agg;
        ctx->saved_data["device"] = (int64_t)dev.index();
        ag::tensor_list out = split1(out8, 7);
        ctx->mark_non_differentiable({out[4], out[5], out[6]});
        return out;
    }
    static ag::tensor_list backward(ag::AutogradContext* ctx, ag::tensor_list grads) {
        ag::tensor_list out(20);
        const int64_t B = ctx->saved_data["B"].toInt(), S = ctx->saved_data["S"].toInt(), want = ctx->saved_data["want"].toInt();
        if (!want) return out;
        const at::Device dev(at::kCUDA, (c10::DeviceIndex)ctx->saved_data["device"].toInt());
        c10::DeviceGuard g(dev);
        const bool empty = B == 0 || S == 0;
        auto make = [&](int bit) {
            if (!(want & bit)) return undef();
            return empty ? at::zeros({B, S}, at::TensorOptions().dtype(at::kFloat).device(dev)) : new_f32({B, S}, dev);
        };
        Tensor grad_p = make(kWantP), grad_e = make(kWantE), grad_v = make(kWantV);
        out[0] = grad_p;
        out[5] = grad_e;
        out[6] = grad_v;
        if (empty) return out;
        const Tensor ws = ctx->get_saved_variables()[0];
        // an output that did not enter the caller's loss arrives undefined: the kernel takes NULL for a zero gradient
        Tensor g_p = grads[0].defined() ? grad1(grads[0], dev, "grad_policy_loss") : undef();
        Tensor g_k = grads[1].defined() ? grad1(grads[1], dev, "grad_kl_loss") : undef();
        Tensor g_v = grads[2].defined() ? grad1(grads[2], dev, "grad_value_loss") : undef();
        Tensor g_e = grads[3].defined() ? grad1(grads[3], dev, "grad_entropy") : undef();
        check(hpc_rll_lm_policy_backward(fptr(g_p), fptr(g_k), fptr(g_v), fptr(g_e), fptr(ws), fmut(grad_p), fmut(grad_e),
                                         fmut(grad_v), (int)B, (int)S, (int)want, (int)ctx->saved_data["agg"].toInt(),
                                         stream_of(dev)),
              "hpc_rll_lm_policy_backward");
        return out;
    }
};

// Which gradients can be wanted is read off the operands here: inside a node's forward grad mode is off.
ag::tensor_list lm_policy_loss(const Tensor& logp, const Tensor& old_logp, const Tensor& adv, const OptTensor& weight,
                               const OptTensor& ref_logp, const OptTensor& entropy, const OptTensor& value_new,
                               const OptTensor& value_old, const OptTensor& ret, int64_t ratio, int64_t objective, double clip_low,
                               double clip_high, std::optional<double> dual_clip, int64_t kl, int64_t agg,
                               std::optional<double> norm_len, std::optional<double> value_clip, int64_t mapping) {
    int64_t want = 0;
    if (at::GradMode::is_enabled()) {
        if (logp.defined() && logp.requires_grad()) want |= kWantP | (has(ref_logp) ? kWantK : 0);
        if (has(entropy) && entropy->requires_grad()) want |= kWantE;
        if (has(value_new) && value_new->requires_grad()) want |= kWantV;
    }
    return LmPolicyFn::apply(logp, old_logp, adv, weight, ref_logp, entropy, value_new, value_old, ret, ratio, objective, clip_low,
                             clip_high, dual_clip, kl, agg, norm_len, value_clip, mapping, want);
}

}  // namespace
}  // namespace hpc_rll_ext

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    using namespace hpc_rll_ext;
    m.doc() = "hpc_lm_policy (ROCm/HIP): GRPO / PPO / GSPO / CISPO losses on per-token log-probabilities over libhpc_rll_hip.so";
    bind_common(m);
    m.def("lm_policy_loss", &lm_policy_loss, py::arg("logp"), py::arg("old_logp"), py::arg("adv"), py::arg("weight") = py::none(),
          py::arg("ref_logp") = py::none(), py::arg("entropy") = py::none(), py::arg("value_new") = py::none(),
          py::arg("value_old") = py::none(), py::arg("ret") = py::none(), py::arg("ratio") = 0, py::arg("objective") = 0,
          py::arg("clip_low") = 0.2, py::arg("clip_high") = 0.2, py::arg("dual_clip") = py::none(), py::arg("kl") = 2,
          py::arg("agg") = 0, py::arg("norm_len") = py::none(), py::arg("value_clip") = 0.2, py::arg("mapping") = 0,
          "(policy_loss, kl_loss, value_loss, entropy, approx_kl, mean_ratio, clipfrac), (1,) each, from (B,S) fp32 operands; adv "
          "(B,) or (B,S).  ratio 0 token / 1 sequence, objective 0 clip / 1 cispo, kl 0 k1 / 1 k2 / 2 k3, agg 0 token / 1 sequence "
          "/ 2 constant (norm_len), mapping 0 by rule / 1 wave / 2 chunk.  The gradient flows to logp, entropy and value_new");
    m.def("lm_policy_last_config", []() {
        std::vector<int> v(HPC_RLL_LM_POLICY_CONFIG_INTS);
        check(hpc_rll_lm_policy_last_config(v.data()), "hpc_rll_lm_policy_last_config");
        return v;
    }, "hpc_rll_lm_policy_last_config: the records of the last forward and backward launch");
    m.attr("CHUNK") = HPC_RLL_LM_POLICY_CHUNK;
    m.attr("WAVE_SEQ_MAX") = HPC_RLL_LM_POLICY_WAVE_SEQ_MAX;
}
