// hpc_sac -- Soft Actor-Critic for continuous actions (no reference counterpart): the tanh-squashed Gaussian head and the SAC
// losses (hpc_rll_tanh_gaussian_rsample_*, hpc_rll_sac_continuous_*; include/hpc_rll_hip.h has the formulas).  HOST-ONLY C++
// like the other modules (common.hpp): it validates tensors, takes outputs and scratch from torch's caching allocator and calls
// the C ABI on torch's current stream.  Nothing here synchronises with the host.
#include "rl_utils_ops.hpp"

namespace hpc_rll_ext {
namespace {

// ============================================================================================================ the head
// (action (..., A), log_prob (...)) from mu, sigma, eps (..., A); eps is a constant.  Differentiable wrt mu and sigma from
// either output; saves sigma, eps and action.  An upstream gradient that is absent is not read.
struct TanhGaussianFn : public ag::Function<TanhGaussianFn> {
    static ag::tensor_list forward(ag::AutogradContext* ctx, const Tensor& mu, const Tensor& sigma, const Tensor& eps) {
        TORCH_CHECK(mu.defined(), "mu: expected a tensor, got None");
        TORCH_CHECK(mu.dim() >= 1, "mu: expected (..., A), got ", mu.sizes());
        const at::IntArrayRef full = mu.sizes(), lead = full.slice(0, full.size() - 1);
        const int64_t A = full.back();
        Args args;
        args.add(mu, "mu", full);
        args.add(sigma, "sigma", full);
        args.add(eps, "eps", full);
        TORCH_CHECK(A >= 1 && A <= 1024, "tanh_gaussian_rsample: A = ", A, " is not supported (1 <= A <= 1024)");
        const at::Device dev = args.on_device_of(mu);
        c10::DeviceGuard g(dev);
        Tensor action = new_f32(full, dev), logp = new_f32(lead, dev);
        check(hpc_rll_tanh_gaussian_rsample_forward(fptr(mu), fptr(sigma), fptr(eps), fmut(action), fmut(logp), logp.numel(),
                                                    (int)A, stream_of(dev)),
              "hpc_rll_tanh_gaussian_rsample_forward");
        ctx->save_for_backward({sigma, eps, action});
        ctx->set_materialize_grads(false);
        return {action, logp};
    }
    static ag::tensor_list backward(ag::AutogradContext* ctx, ag::tensor_list grads) {
        ag::tensor_list out(3);
        const bool need_mu = ctx->needs_input_grad(0), need_sigma = ctx->needs_input_grad(1);
        if (!(need_mu || need_sigma) || !(grads[0].defined() || grads[1].defined())) return out;
        const auto saved = ctx->get_saved_variables();
        const Tensor &sigma = saved[0], &eps = saved[1], &action = saved[2];
        const at::Device dev = action.device();
        c10::DeviceGuard g(dev);
        Tensor g_a, g_l;
        if (grads[0].defined()) g_a = req(grads[0].contiguous(), "grad_action", dev);
        if (grads[1].defined()) g_l = req(grads[1].contiguous(), "grad_log_prob", dev);
        Tensor grad_mu = need_mu ? new_f32(action.sizes(), dev) : undef();
        Tensor grad_sigma = need_sigma ? new_f32(action.sizes(), dev) : undef();
        const int64_t A = action.sizes().back();
        check(hpc_rll_tanh_gaussian_rsample_backward(fptr(g_a), fptr(g_l), fptr(sigma), fptr(eps), fptr(action), fmut(grad_mu),
                                                     fmut(grad_sigma), action.numel() / A, (int)A, stream_of(dev)),
              "hpc_rll_tanh_gaussian_rsample_backward");
        out[0] = grad_mu;
        out[1] = grad_sigma;
        return out;
    }
};

// ========================================================================================================== the losses
// (policy, critic, twin critic, entropy (1,) each, td_error (...), target_q (...)) from per-sample tensors of one leading
// shape.  The critic half (q1 .. weight) is absent when q1 is None, the actor half (log_prob, new_q1, new_q2) when log_prob
// is; the python side maps the outputs of an absent half to None.  Shapes and dtypes are checked before the device so that a
// wrong argument is named even on host tensors.  The gradient flows to q1, q2, log_prob, new_q1 and new_q2; each is formed
// only when its input needs it.  Saves the workspace alone.
struct SacContinuousFn : public ag::Function<SacContinuousFn> {
    static ag::tensor_list forward(ag::AutogradContext* ctx, const OptTensor& q1, const OptTensor& q2,
                                   const OptTensor& target_q1, const OptTensor& target_q2, const OptTensor& next_log_prob,
                                   const OptTensor& reward, const OptTensor& done, const OptTensor& weight,
                                   const OptTensor& log_prob, const OptTensor& new_q1, const OptTensor& new_q2, double alpha,
                                   const OptTensor& alpha_t, double gamma, std::optional<double> scale) {
        const bool critic = has(q1), actor = has(log_prob);
        TORCH_CHECK(critic || actor, "sac_continuous: the critic half (q1, ...) and the actor half (log_prob, ...) are both absent");
        TORCH_CHECK(!critic || has(reward), "reward: expected a tensor, got None");
        const Tensor& leadt = critic ? *reward : *log_prob;
        TORCH_CHECK(!critic || has(q2) == has(target_q2), "sac_continuous: q2 and target_q2 are both given or both None (got ",
                    has(q2) ? "q2" : "target_q2", " alone)");
        TORCH_CHECK(critic || !(has(q2) || has(target_q2)), "sac_continuous: q2 / target_q2 given without q1");
        TORCH_CHECK(actor || !has(new_q2), "sac_continuous: new_q2 given without log_prob");
        TORCH_CHECK(!(critic && actor) || has(q2) == has(new_q2), "sac_continuous: q2, target_q2 and new_q2 are all given or all "
                    "None (got ", has(q2) ? "q2 and target_q2 without new_q2" : "new_q2 alone", ")");
        const at::IntArrayRef lead = leadt.sizes();
        TORCH_CHECK(lead.empty() || lead.back() != 1 || leadt.dim() < 2, critic ? "reward" : "log_prob", ": shape ", lead,
                    " has a trailing dimension of 1; every operand is one float per sample, squeeze(-1) it first");
        Args args;
        if (critic) {
            TORCH_CHECK(has(target_q1), "target_q1: expected a tensor, got None");
            TORCH_CHECK(has(next_log_prob), "next_log_prob: expected a tensor, got None");
            args.add(*reward, "reward", lead);
            args.add(*q1, "q1", lead);
            args.add(q2, "q2", lead);
            args.add(*target_q1, "target_q1", lead);
            args.add(target_q2, "target_q2", lead);
            args.add(*next_log_prob, "next_log_prob", lead);
        }
        const Args::Mask dm = critic ? args.add_mask(done, "done", lead) : Args::Mask{HPC_RLL_MASK_U8, nullptr};
        if (critic) args.add(weight, "weight", lead);
        if (actor) {
            TORCH_CHECK(has(new_q1), "new_q1: expected a tensor, got None");
            args.add(*log_prob, "log_prob", lead);
            args.add(*new_q1, "new_q1", lead);
            args.add(new_q2, "new_q2", lead);
        }
        if (has(alpha_t)) {   // one element of any shape: its own messages
            TORCH_CHECK(alpha_t->scalar_type() == at::kFloat, "alpha: dtype ", alpha_t->scalar_type(), ", expected ", at::kFloat);
            TORCH_CHECK(alpha_t->numel() == 1, "alpha: expected a float or a 1-element tensor, got shape ", alpha_t->sizes());
        }
        const at::Device dev = args.on_device_of(leadt);
        if (has(alpha_t)) req(*alpha_t, "alpha", dev);
        c10::DeviceGuard g(dev);
        const int64_t rows = leadt.numel();
        Tensor out4 = new_f32({4}, dev);
        Tensor td = critic ? new_f32(lead, dev) : undef(), tq = critic ? new_f32(lead, dev) : undef();
        Tensor ws = new_f32({rows > 0 ? hpc_rll_sac_continuous_workspace_floats(rows) : 0}, dev);
        check(hpc_rll_sac_continuous_forward(fptr(q1), fptr(q2), fptr(target_q1), fptr(target_q2), fptr(next_log_prob),
                                             fptr(reward), dm.ptr, dm.code, critic ? fptr(weight) : nullptr, fptr(log_prob),
                                             fptr(new_q1), fptr(new_q2), fptr(alpha_t), (float)alpha, fmut(out4), fmut(td),
                                             fmut(tq), fmut(ws), rows, (float)gamma, loss_scale(scale, rows), stream_of(dev)),
              "hpc_rll_sac_continuous_forward");
        ctx->save_for_backward({ws});
        ctx->saved_data["lead"] = lead.vec();
        // needs_input_grad() counts the tensors that were given, not the arguments: the position of each among them, -1 = None
        std::vector<int64_t> edge;
        int64_t given = 0;
        for (const OptTensor* t : {&q1, &q2, &target_q1, &target_q2, &next_log_prob, &reward, &done, &weight, &log_prob, &new_q1,
                                   &new_q2})
            edge.push_back(has(*t) ? given++ : -1);
        ctx->saved_data["edge"] = edge;
        Tensor policy = alias_of(out4, 0, 1), critic_l = alias_of(out4, 1, 1), twin = alias_of(out4, 2, 1),
               ent = alias_of(out4, 3, 1);
        if (!critic) {   // an autograd node returns tensors: zero-size stand-ins, python maps them to None
            td = new_f32({0}, dev);
            tq = new_f32({0}, dev);
        }
        ctx->mark_non_differentiable({ent, td, tq});
        return {policy, critic_l, twin, ent, td, tq};
    }
    static ag::tensor_list backward(ag::AutogradContext* ctx, ag::tensor_list grads) {
        ag::tensor_list out(15);
        const std::vector<int64_t> edge = ctx->saved_data["edge"].toIntVector();
        auto needs = [&](int arg) { return edge[arg] >= 0 && ctx->needs_input_grad((size_t)edge[arg]); };
        const bool n_q1 = needs(0), n_q2 = needs(1), n_lp = needs(8), n_n1 = needs(9), n_n2 = needs(10);
        if (!(n_q1 || n_q2 || n_lp || n_n1 || n_n2)) return out;
        const auto saved = ctx->get_saved_variables();
        const Tensor& ws = saved[0];
        const at::Device dev = ws.device();
        c10::DeviceGuard g(dev);
        const std::vector<int64_t> lead = ctx->saved_data["lead"].toIntVector();
        int64_t rows = 1;
        for (int64_t n : lead) rows *= n;
        Tensor g_p = grad1(grads[0], dev, "grad_policy_loss"), g_1 = grad1(grads[1], dev, "grad_critic_loss"),
               g_2 = grad1(grads[2], dev, "grad_twin_critic_loss");
        auto want = [&](bool need) { return need ? new_f32(lead, dev) : undef(); };
        Tensor d_q1 = want(n_q1), d_q2 = want(n_q2), d_lp = want(n_lp), d_n1 = want(n_n1), d_n2 = want(n_n2);
        check(hpc_rll_sac_continuous_backward(fptr(g_p), fptr(g_1), fptr(g_2), fptr(ws), fmut(d_q1), fmut(d_q2), fmut(d_lp),
                                              fmut(d_n1), fmut(d_n2), rows, stream_of(dev)),
              "hpc_rll_sac_continuous_backward");
        out[0] = d_q1;
        out[1] = d_q2;
        out[8] = d_lp;
        out[9] = d_n1;
        out[10] = d_n2;
        return out;
    }
};

}  // namespace
}  // namespace hpc_rll_ext

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    using namespace hpc_rll_ext;
    m.doc() = "hpc_sac (ROCm/HIP): continuous SAC -- the tanh-Gaussian rsample head and the SAC losses over libhpc_rll_hip.so";
    bind_common(m);
    m.def("tanh_gaussian_rsample", applier<TanhGaussianFn>(&TanhGaussianFn::forward), py::arg("mu"), py::arg("sigma"),
          py::arg("eps"),
          "(action (..., A), log_prob (...)) of mu, sigma, eps (..., A): u = mu + sigma eps, action = tanh(u), log_prob = "
          "sum_j [log N(u_j; mu_j, sigma_j) - log(1 - tanh^2 u_j)], the last term formed from u.  eps is a constant.  "
          "Differentiable wrt mu and sigma");
    m.def("sac_continuous", applier<SacContinuousFn>(&SacContinuousFn::forward), py::arg("q1") = py::none(),
          py::arg("q2") = py::none(), py::arg("target_q1") = py::none(), py::arg("target_q2") = py::none(),
          py::arg("next_log_prob") = py::none(), py::arg("reward") = py::none(), py::arg("done") = py::none(),
          py::arg("weight") = py::none(), py::arg("log_prob") = py::none(), py::arg("new_q1") = py::none(),
          py::arg("new_q2") = py::none(), py::arg("alpha") = 0.2, py::arg("alpha_t") = py::none(), py::arg("gamma") = 0.99,
          py::arg("scale") = py::none(),
          "[policy_loss, critic_loss, twin_critic_loss, entropy (1,) each, td_error (...), target_q (...)] of per-sample "
          "tensors (...): G = reward + gamma (1 - done) (min(target_q1, target_q2) - alpha next_log_prob), critic_loss_i = "
          "scale sum weight (q_i - G)^2, policy_loss = scale sum (alpha log_prob - min(new_q1, new_q2)), entropy = -scale sum "
          "log_prob, scale = 1/rows unless given.  The critic half is absent when q1 is None (td_error and target_q are then "
          "empty), the actor half when log_prob is.  Differentiable wrt q1, q2, log_prob, new_q1, new_q2");
    m.def("sac_continuous_last_config", []() {
        std::vector<int> v(HPC_RLL_SAC_CONTINUOUS_CONFIG_INTS);
        check(hpc_rll_sac_continuous_last_config(v.data()), "hpc_rll_sac_continuous_last_config");
        return v;
    }, "hpc_rll_sac_continuous_last_config: the dispatch record of the last head forward, head backward, loss forward and loss "
       "backward, as the header documents");
}
