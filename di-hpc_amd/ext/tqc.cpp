// hpc_tqc -- Truncated Quantile Critics (no reference counterpart): the critic loss with the atom selection in the kernel and
// the actor loss over the critics' quantiles (hpc_rll_tqc_*; include/hpc_rll_hip.h has the formulas).  HOST-ONLY C++ like the
// other modules (common.hpp): it validates tensors, takes outputs and scratch from torch's caching allocator and calls the C
// ABI on torch's current stream.  Nothing here synchronises with the host.
#include "rl_utils_ops.hpp"

namespace hpc_rll_ext {
namespace {

// alpha as a 1-element fp32 tensor: its own messages (dtype and count here, the device with the others)
void check_alpha(const OptTensor& alpha_t) {
    if (!has(alpha_t)) return;
    TORCH_CHECK(alpha_t->scalar_type() == at::kFloat, "alpha: dtype ", alpha_t->scalar_type(), ", expected ", at::kFloat);
    TORCH_CHECK(alpha_t->numel() == 1, "alpha: expected a float or a 1-element tensor, got shape ", alpha_t->sizes());
}

// ============================================================================================================ the critic
// (critic_loss (1,), td_error (B,), target_atoms (B, K)) of z (B, M, N), target_z (B, M', N') and per-sample vectors (B,).
// Shapes and dtypes are checked before the device so that a wrong argument is named even on host tensors.  The gradient flows
// to z alone and is formed only when z needs it.  Saves the workspace alone.
struct TqcCriticFn : public ag::Function<TqcCriticFn> {
    static ag::tensor_list forward(ag::AutogradContext* ctx, const Tensor& z, const Tensor& target_z, const Tensor& next_log_prob,
                                   const Tensor& reward, const OptTensor& done, const OptTensor& weight, double alpha,
                                   const OptTensor& alpha_t, double gamma, int64_t drop, double kappa,
                                   std::optional<double> scale) {
        TORCH_CHECK(z.defined(), "z: expected a tensor, got None");
        TORCH_CHECK(target_z.defined(), "target_z: expected a tensor, got None");
        TORCH_CHECK(z.dim() == 3, "z: expected (B, M, N), got ", z.sizes());
        TORCH_CHECK(target_z.dim() == 3, "target_z: expected (B, M', N'), got ", target_z.sizes());
        TORCH_CHECK(z.size(0) == target_z.size(0), "z: shape ", z.sizes(), " has ", z.size(0), " rows, target_z ", target_z.sizes(),
                    " has ", target_z.size(0));
        TORCH_CHECK(reward.defined(), "reward: expected a tensor, got None");
        TORCH_CHECK(reward.dim() != 2 || reward.size(1) != 1, "reward: shape ", reward.sizes(),
                    " has a trailing dimension of 1; the per-sample operands are (B,), squeeze(-1) it first");
        const int64_t B = z.size(0), M = z.size(1), N = z.size(2), Mt = target_z.size(1), Nt = target_z.size(2);
        const int64_t MN = M * N, n = Mt * Nt;
        const std::vector<int64_t> lead{B};
        Args args;
        args.add(z, "z", z.sizes());
        args.add(target_z, "target_z", target_z.sizes());
        args.add(next_log_prob, "next_log_prob", lead);
        args.add(reward, "reward", lead);
        const Args::Mask dm = args.add_mask(done, "done", lead);
        args.add(weight, "weight", lead);
        check_alpha(alpha_t);
        TORCH_CHECK(MN >= 1 && MN <= 1024 && n >= 1 && n <= 1024, "tqc_critic_loss: M*N = ", MN, " and M'*N' = ", n,
                    " must both lie in 1 .. 1024");
        TORCH_CHECK(drop >= 0 && drop < n, "drop: ", drop, " is out of range, expected 0 <= drop < M'*N' = ", n);
        TORCH_CHECK(kappa > 0.0, "kappa: ", kappa, ", expected > 0");
        const at::Device dev = args.on_device_of(z);
        if (has(alpha_t)) req(*alpha_t, "alpha", dev);
        c10::DeviceGuard g(dev);
        const int64_t K = n - drop;
        Tensor loss = B > 0 ? new_f32({1}, dev) : at::zeros({1}, z.options());
        Tensor td = new_f32({B}, dev), atoms = new_f32({B, K}, dev);
        ctx->saved_data["shape"] = std::vector<int64_t>{B, M, N};
        ctx->mark_non_differentiable({td, atoms});
        if (B == 0) return {loss, td, atoms};   // no rows: zero loss, nothing launched
        Tensor ws = new_f32({hpc_rll_tqc_workspace_floats(B, (int)MN)}, dev);
        check(hpc_rll_tqc_critic_forward(fptr(z), fptr(target_z), fptr(next_log_prob), fptr(reward), dm.ptr, dm.code, fptr(weight),
                                         fptr(alpha_t), (float)alpha, fmut(loss), fmut(td), fmut(atoms), fmut(ws), B, (int)M,
                                         (int)N, (int)Mt, (int)Nt, (int)drop, (float)gamma, (float)kappa, loss_scale(scale, B),
                                         stream_of(dev)),
              "hpc_rll_tqc_critic_forward");
        ctx->save_for_backward({ws});
        return {loss, td, atoms};
    }
    static ag::tensor_list backward(ag::AutogradContext* ctx, ag::tensor_list grads) {
        ag::tensor_list out(12);
        if (!ctx->needs_input_grad(0)) return out;
        const std::vector<int64_t> shape = ctx->saved_data["shape"].toIntVector();
        const auto saved = ctx->get_saved_variables();
        if (shape[0] == 0 || saved.empty()) {
            out[0] = at::zeros(shape, grads[0].options());
            return out;
        }
        const Tensor& ws = saved[0];
        const at::Device dev = ws.device();
        c10::DeviceGuard g(dev);
        Tensor g_loss = grad1(grads[0], dev, "grad_critic_loss");
        Tensor grad_z = new_f32(shape, dev);
        check(hpc_rll_tqc_critic_backward(fptr(g_loss), fptr(ws), fmut(grad_z), shape[0], (int)shape[1], (int)shape[2],
                                          stream_of(dev)),
              "hpc_rll_tqc_critic_backward");
        out[0] = grad_z;
        return out;
    }
};

// ============================================================================================================= the actor
// (policy_loss, entropy (1,) each) of log_prob (B,) and new_z (B, M, N).  The gradient flows to log_prob and new_z; each is
// formed only when its input needs it.
struct TqcPolicyFn : public ag::Function<TqcPolicyFn> {
    static ag::tensor_list forward(ag::AutogradContext* ctx, const Tensor& log_prob, const Tensor& new_z, double alpha,
                                   const OptTensor& alpha_t, std::optional<double> scale) {
        TORCH_CHECK(log_prob.defined(), "log_prob: expected a tensor, got None");
        TORCH_CHECK(new_z.defined(), "new_z: expected a tensor, got None");
        TORCH_CHECK(new_z.dim() == 3, "new_z: expected (B, M, N), got ", new_z.sizes());
        TORCH_CHECK(log_prob.dim() != 2 || log_prob.size(1) != 1, "log_prob: shape ", log_prob.sizes(),
                    " has a trailing dimension of 1; the per-sample operands are (B,), squeeze(-1) it first");
        const int64_t B = new_z.size(0), MN = new_z.size(1) * new_z.size(2);
        Args args;
        args.add(new_z, "new_z", new_z.sizes());
        args.add(log_prob, "log_prob", std::vector<int64_t>{B});
        check_alpha(alpha_t);
        TORCH_CHECK(MN >= 1 && MN <= 1024, "tqc_policy_loss: M*N = ", MN, " must lie in 1 .. 1024");
        const at::Device dev = args.on_device_of(new_z);
        if (has(alpha_t)) req(*alpha_t, "alpha", dev);
        c10::DeviceGuard g(dev);
        Tensor out2 = B > 0 ? new_f32({2}, dev) : at::zeros({2}, new_z.options());
        Tensor policy = alias_of(out2, 0, 1), ent = alias_of(out2, 1, 1);
        ctx->saved_data["shape"] = new_z.sizes().vec();
        ctx->mark_non_differentiable({ent});
        if (B == 0) return {policy, ent};
        Tensor ws = new_f32({hpc_rll_tqc_workspace_floats(0, 0)}, dev);
        check(hpc_rll_tqc_policy_forward(fptr(log_prob), fptr(new_z), fptr(alpha_t), (float)alpha, fmut(out2), fmut(ws), B, (int)MN,
                                         loss_scale(scale, B), stream_of(dev)),
              "hpc_rll_tqc_policy_forward");
        ctx->save_for_backward({ws});
        return {policy, ent};
    }
    static ag::tensor_list backward(ag::AutogradContext* ctx, ag::tensor_list grads) {
        ag::tensor_list out(5);
        const bool n_lp = ctx->needs_input_grad(0), n_z = ctx->needs_input_grad(1);
        if (!(n_lp || n_z)) return out;
        const std::vector<int64_t> shape = ctx->saved_data["shape"].toIntVector();
        const auto saved = ctx->get_saved_variables();
        if (shape[0] == 0 || saved.empty()) {
            if (n_lp) out[0] = at::zeros({shape[0]}, grads[0].options());
            if (n_z) out[1] = at::zeros(shape, grads[0].options());
            return out;
        }
        const Tensor& ws = saved[0];
        const at::Device dev = ws.device();
        c10::DeviceGuard g(dev);
        Tensor g_p = grad1(grads[0], dev, "grad_policy_loss");
        Tensor d_lp = n_lp ? new_f32({shape[0]}, dev) : undef(), d_z = n_z ? new_f32(shape, dev) : undef();
        check(hpc_rll_tqc_policy_backward(fptr(g_p), fptr(ws), fmut(d_lp), fmut(d_z), shape[0], (int)(shape[1] * shape[2]),
                                          stream_of(dev)),
              "hpc_rll_tqc_policy_backward");
        out[0] = d_lp;
        out[1] = d_z;
        return out;
    }
};

}  // namespace
}  // namespace hpc_rll_ext

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    using namespace hpc_rll_ext;
    m.doc() = "hpc_tqc (ROCm/HIP): Truncated Quantile Critics -- the critic loss with in-kernel atom selection and the actor "
              "loss over libhpc_rll_hip.so";
    bind_common(m);
    m.def("tqc_critic", applier<TqcCriticFn>(&TqcCriticFn::forward), py::arg("z"), py::arg("target_z"), py::arg("next_log_prob"),
          py::arg("reward"), py::arg("done") = py::none(), py::arg("weight") = py::none(), py::arg("alpha") = 0.2,
          py::arg("alpha_t") = py::none(), py::arg("gamma") = 0.99, py::arg("drop") = 0, py::arg("kappa") = 1.0,
          py::arg("scale") = py::none(),
          "[critic_loss (1,), td_error (B,), target_atoms (B, K)] of z (B, M, N) and target_z (B, M', N'): the M'*N' target atoms "
          "of a sample are ordered, the largest `drop` are cut, y_j = reward + gamma (1 - done) (s_(j) - alpha next_log_prob) for "
          "the K kept, td_error = mean_{m,i,j} |tau_i - 1{y_j < z_mi}| huber_kappa(y_j - z_mi) / kappa, critic_loss = scale sum "
          "weight td_error, scale = 1/B unless given.  Differentiable wrt z");
    m.def("tqc_policy", applier<TqcPolicyFn>(&TqcPolicyFn::forward), py::arg("log_prob"), py::arg("new_z"), py::arg("alpha") = 0.2,
          py::arg("alpha_t") = py::none(), py::arg("scale") = py::none(),
          "[policy_loss, entropy (1,) each] of log_prob (B,) and new_z (B, M, N): policy_loss = scale sum (alpha log_prob - "
          "mean_{m,i} new_z), entropy = -scale sum log_prob, scale = 1/B unless given.  Differentiable wrt log_prob and new_z");
    m.def("tqc_last_config", []() {
        std::vector<int> v(HPC_RLL_TQC_CONFIG_INTS);
        check(hpc_rll_tqc_last_config(v.data()), "hpc_rll_tqc_last_config");
        return v;
    }, "hpc_rll_tqc_last_config: the dispatch record of the last critic forward, critic backward, actor forward and actor "
       "backward, as the header documents");
}
