// rl_utils.cpp -- the compiled `hpc_rl_utils` extension module (reference: src/rl_utils/entry.cpp:8-39).
//
// Two layers in one module:
//   * the reference's L2 functions `XxxForward(inputs, outputs, scalars...)` / `XxxBackward(inputs, outputs)`
//     (declared in include/hpc/rll/cuda/rl_utils/entry.h:10-165) -- validated, launched on torch's current stream;
//   * fused autograd ops (`gae`, `td_lambda`, `vtrace`, `upgo`, `upgo_masked`, `ppo`, `ppo_continuous`, `vtrace_continuous`, `retrace_loss`, `acer_policy_loss`, `coma`, `r2d2_td`, `sac_discrete`, `token_log_prob`, `grpo_policy_loss`, `token_log_prob_entropy`, `lm_ppo_loss`, `q_nstep_td`, `dist_nstep_td`, `iqn_nstep_td`,
//     `qrdqn_nstep_td`, `fqf_fractions`, `fqf_nstep_td`, `fqf_fraction_loss`; `fqf_q_value` is a plain function) -- torch::autograd::Function nodes that allocate outputs, launch and register backward in ONE
//     pybind call; these are what hpc_rll.rl_utils.* modules use.
// Host-only C++: every kernel lives behind the C ABI of libhpc_rll_hip.so (include/hpc_rll_hip.h).
#include "common.hpp"
#include "rl_utils_ops.hpp"

#include <map>
#include <mutex>
#include <tuple>

namespace hpc_rll_ext {

// =========================================================================================================== GAE
// coef table c_t = gamma*lambda*D_{t+1}/D_t: depends only on (T, gamma, lambda).  Cached per device and NEVER freed
// (a captured hipGraph or another stream may hold the pointer for the life of the process; the cache is capped, past
// the cap tables are per call).  While a stream is capturing, a miss fills a per-call table inside the capture and
// does not publish it: its contents only exist once the graph is replayed.
struct CoefCache {
    std::mutex mu;
    std::map<std::tuple<int, int, float, float>, Tensor> tab;
};
CoefCache& coef_cache() {
    static CoefCache* c = new CoefCache();   // leaked on purpose: tensors must not be destroyed after torch shuts down
    return *c;
}
constexpr size_t kCoefCacheCap = 256;

Tensor gae_coef(int64_t T, double gamma, double lambda, const at::Device& dev) {
    const auto key = std::make_tuple((int)dev.index(), (int)T, (float)gamma, (float)lambda);
    CoefCache& cc = coef_cache();
    {
        std::lock_guard<std::mutex> lk(cc.mu);
        auto it = cc.tab.find(key);
        if (it != cc.tab.end()) return it->second;
    }
    void* st = stream_of(dev);
    const int capturing = hpc_rll_stream_is_capturing(st);
    TORCH_CHECK(capturing >= 0, "gae_coef: hipStreamIsCapturing failed");
    Tensor c = new_f32({std::max<int64_t>(T, 1)}, dev);
    check(hpc_rll_gae_coef(c.data_ptr<float>(), to_int(T, "T"), (float)gamma, (float)lambda, st), "hpc_rll_gae_coef");
    if (!capturing) {
        // published to every stream: make the fill globally visible first (one ~20 us host wait per new key)
        check(hpc_rll_stream_synchronize(st), "gae_coef: stream synchronize");
        std::lock_guard<std::mutex> lk(cc.mu);
        if (cc.tab.size() < kCoefCacheCap) cc.tab.emplace(key, c);
    }
    return c;
}

void gae_forward_launch(const Tensor& value, const Tensor& reward, const Tensor& adv, const Tensor& coef, double gamma) {
    const int64_t T = reward.size(0), B = reward.size(1);
    check(hpc_rll_gae_forward(fptr(value), fptr(reward), fmut(adv), fptr(coef), to_int(T, "T"), to_int(B, "B"),
                              (float)gamma, stream_of(reward.device())),
          "hpc_rll_gae_forward");
}

void check_gae_inputs(const Tensor& value, const Tensor& reward) {
    req(reward, "reward");
    TORCH_CHECK(reward.dim() == 2, "reward: expected (T,B), got ", reward.sizes());
    req(value, "value", reward.device(), {reward.size(0) + 1, reward.size(1)});
}

// inputs = [value (T+1,B), reward (T,B)], outputs = [adv (T,B)].  Reference: src/rl_utils/gae.cu:8-28.
void GaeForward(const TensorList& inputs, const TensorList& outputs, double gamma, double lambda) {
    expect_len(inputs, 2, "GaeForward inputs");
    expect_len(outputs, 1, "GaeForward outputs");
    const Tensor &value = inputs[0], &reward = inputs[1], &adv = outputs[0];
    check_gae_inputs(value, reward);
    req(adv, "adv", reward.device(), {reward.size(0), reward.size(1)});
    c10::DeviceGuard g(reward.device());
    gae_forward_launch(value, reward, adv, gae_coef(reward.size(0), gamma, lambda, reward.device()), gamma);
}

void gae_backward_launch(const Tensor& grad_adv, const Tensor& gv, const Tensor& gr, const Tensor& coef, double gamma) {
    const int64_t T = grad_adv.size(0), B = grad_adv.size(1);
    check(hpc_rll_gae_backward(fptr(grad_adv), fmut(gv), fmut(gr), fptr(coef), to_int(T, "T"), to_int(B, "B"),
                               (float)gamma, stream_of(grad_adv.device())),
          "hpc_rll_gae_backward");
}

// inputs = [grad_adv (T,B)], outputs = [grad_value (T+1,B) | None, grad_reward (T,B) | None].  New entry (the
// reference registers no GaeBackward, entry.cpp:22): the analytic adjoint of hpc_rll.origin.gae.
void GaeBackward(const TensorList& inputs, const OptList& outputs, double gamma, double lambda) {
    expect_len(inputs, 1, "GaeBackward inputs");
    expect_len(outputs, 2, "GaeBackward outputs");
    const Tensor& ga = req(inputs[0], "grad_adv");
    TORCH_CHECK(ga.dim() == 2, "grad_adv: expected (T,B), got ", ga.sizes());
    const int64_t T = ga.size(0), B = ga.size(1);
    req_opt(outputs[0], "grad_value", ga.device(), {T + 1, B});
    req_opt(outputs[1], "grad_reward", ga.device(), {T, B});
    c10::DeviceGuard g(ga.device());
    gae_backward_launch(ga, has(outputs[0]) ? *outputs[0] : undef(), has(outputs[1]) ? *outputs[1] : undef(),
                        gae_coef(T, gamma, lambda, ga.device()), gamma);
}

struct GaeFn : public ag::Function<GaeFn> {
    static Tensor forward(ag::AutogradContext* ctx, const Tensor& value, const Tensor& reward, double gamma,
                          double lambda) {
        check_gae_inputs(value, reward);
        c10::DeviceGuard g(reward.device());
        Tensor coef = gae_coef(reward.size(0), gamma, lambda, reward.device());
        Tensor adv = at::empty_like(reward);
        gae_forward_launch(value, reward, adv, coef, gamma);
        ctx->saved_data["coef"] = coef;   // keeps a per-call (uncached) table alive until backward
        ctx->saved_data["gamma"] = gamma;
        return adv;
    }
    static ag::tensor_list backward(ag::AutogradContext* ctx, ag::tensor_list grads) {
        const bool need_v = ctx->needs_input_grad(0), need_r = ctx->needs_input_grad(1);
        if (!(need_v || need_r)) return {undef(), undef(), undef(), undef()};
        Tensor ga = grads[0].contiguous();
        req(ga, "grad_adv");
        const int64_t T = ga.size(0), B = ga.size(1);
        c10::DeviceGuard g(ga.device());
        Tensor gv = need_v ? new_f32({T + 1, B}, ga.device()) : undef();
        Tensor gr = need_r ? at::empty_like(ga) : undef();
        gae_backward_launch(ga, gv, gr, ctx->saved_data["coef"].toTensor(), ctx->saved_data["gamma"].toDouble());
        return {gv, gr, undef(), undef()};
    }
};

// ============================================================================================ GAE with done masks
// Textbook GAE with episode ends (hpc_rll_gae_masked_*): value (T+1,B) stacked, or value (T,B) + next_value (T,B);
// done / traj_flag (T,B) bool, uint8 or float32 (either may be None).  Dtypes and shapes are checked before the device
// so that a wrong argument is named even on host tensors.
// The masks as the kernels take them: one dtype code for both (a byte mask next to a float one becomes 0/1 floats).
struct Masks { Tensor done, flag; int code = HPC_RLL_MASK_U8; };

// Shared by gae_masked, td_lambda_masked and vtrace_masked (`op` names the caller in the first message).
Masks check_masked_inputs(const char* op, const Tensor& value, const Tensor& reward, const OptTensor& done,
                          const OptTensor& flag, const OptTensor& next_value) {
    TORCH_CHECK(reward.defined() && value.defined(), op, ": value and reward are required");
    TORCH_CHECK(reward.dim() == 2, "reward: expected (T,B), got ", reward.sizes());
    const int64_t T = reward.size(0), B = reward.size(1);
    const bool nv = has(next_value);
    TORCH_CHECK(value.dim() == 2 && value.size(0) == (nv ? T : T + 1) && value.size(1) == B, "value: shape ",
                value.sizes(), ", expected ", nv ? "(T,B)" : "(T+1,B)", " = (", nv ? T : T + 1, ", ", B,
                ") for reward ", reward.sizes(), nv ? " with next_value" : " (stacked form: row T is the bootstrap value)");
    Masks m;
    int codes[2] = {-1, -1};
    const OptTensor* in[2] = {&done, &flag};
    const char* names[2] = {"done", "traj_flag"};
    for (int i = 0; i < 2; ++i) {
        if (!has(*in[i])) continue;
        const Tensor& t = **in[i];
        codes[i] = mask_code(t, names[i]);
        TORCH_CHECK(t.sizes() == reward.sizes(), names[i], ": shape ", t.sizes(), ", expected ", reward.sizes(),
                    " (the shape of reward)");
    }
    if (nv) {
        TORCH_CHECK(next_value->scalar_type() == at::kFloat, "next_value: dtype ", next_value->scalar_type(),
                    ", expected float32");
        TORCH_CHECK(next_value->sizes() == reward.sizes(), "next_value: shape ", next_value->sizes(), ", expected ",
                    reward.sizes());
    }
    req(reward, "reward");
    req(value, "value", reward.device());
    if (nv) req(*next_value, "next_value", reward.device());
    const at::Device dev = reward.device();
    for (int i = 0; i < 2; ++i) {
        if (codes[i] < 0) continue;
        const Tensor& t = **in[i];
        req(t, names[i], dev, t.scalar_type());
        (i == 0 ? m.done : m.flag) = t;
    }
    if (codes[0] >= 0 && codes[1] >= 0 && codes[0] != codes[1]) {
        Tensor& byte = codes[0] == HPC_RLL_MASK_U8 ? m.done : m.flag;
        byte = byte.ne(0).to(at::kFloat);
    }
    m.code = (codes[0] == HPC_RLL_MASK_F32 || codes[1] == HPC_RLL_MASK_F32) ? HPC_RLL_MASK_F32 : HPC_RLL_MASK_U8;
    return m;
}

struct GaeMaskedFn : public ag::Function<GaeMaskedFn> {
    static Tensor forward(ag::AutogradContext* ctx, const Tensor& value, const Tensor& reward, const OptTensor& done,
                          const OptTensor& flag, const OptTensor& next_value, double gamma, double lambda) {
        const Masks m = check_masked_inputs("gae_masked", value, reward, done, flag, next_value);
        const int64_t T = reward.size(0), B = reward.size(1);
        c10::DeviceGuard g(reward.device());
        Tensor adv = at::empty_like(reward);
        check(hpc_rll_gae_masked_forward(fptr(value), fptr(next_value), fptr(reward), vptr(m.done), vptr(m.flag), m.code,
                                         fmut(adv), to_int(T, "T"), to_int(B, "B"), (float)gamma, (float)lambda,
                                         stream_of(reward.device())),
              "hpc_rll_gae_masked_forward");
        ctx->save_for_backward({m.done, m.flag});   // the masks, not the coefficients
        ctx->saved_data["code"] = (int64_t)m.code;
        ctx->saved_data["stacked"] = !has(next_value);
        // needs_input_grad counts the tensor arguments that were passed (a None mask is not one)
        ctx->saved_data["nv_input"] = (int64_t)(2 + has(done) + has(flag));
        ctx->saved_data["gamma"] = gamma;
        ctx->saved_data["lambda"] = lambda;
        return adv;
    }
    static ag::tensor_list backward(ag::AutogradContext* ctx, ag::tensor_list grads) {
        const bool stacked = ctx->saved_data["stacked"].toBool();
        const bool need_v = ctx->needs_input_grad(0), need_r = ctx->needs_input_grad(1);
        const bool need_n = !stacked && ctx->needs_input_grad((size_t)ctx->saved_data["nv_input"].toInt());
        const ag::tensor_list out_none = {undef(), undef(), undef(), undef(), undef(), undef(), undef()};
        if (!(need_v || need_r || need_n)) return out_none;
        const auto saved = ctx->get_saved_variables();
        Tensor ga = grads[0].contiguous();
        req(ga, "grad_adv");
        const int64_t T = ga.size(0), B = ga.size(1);
        c10::DeviceGuard g(ga.device());
        Tensor gv = need_v ? new_f32({stacked ? T + 1 : T, B}, ga.device()) : undef();
        Tensor gr = need_r ? at::empty_like(ga) : undef();
        Tensor gn = need_n ? at::empty_like(ga) : undef();
        check(hpc_rll_gae_masked_backward(fptr(ga), vptr(saved[0]), vptr(saved[1]), (int)ctx->saved_data["code"].toInt(),
                                          fmut(gv), fmut(gn), fmut(gr), stacked ? 1 : 0, to_int(T, "T"), to_int(B, "B"),
                                          (float)ctx->saved_data["gamma"].toDouble(),
                                          (float)ctx->saved_data["lambda"].toDouble(), stream_of(ga.device())),
              "hpc_rll_gae_masked_backward");
        return {gv, gr, undef(), undef(), gn, undef(), undef()};
    }
};

// ==================================================================================================== TD(lambda)
int td_weight_mode(const OptTensor& weight, int64_t T, int64_t B, const at::Device& dev) {
    if (!has(weight)) return 0;
    req(*weight, "weight", dev);
    if (weight->dim() == 2 && weight->size(0) == T && weight->size(1) == B) return 2;
    if (weight->dim() == 1 && weight->size(0) == B) return 1;
    TORCH_CHECK(false, "weight: shape ", weight->sizes(), ", expected (", T, ",", B, ") or (", B, ",)");
}

void td_lambda_forward_impl(const Tensor& value, const Tensor& reward, const OptTensor& weight, const Tensor& loss,
                            const Tensor& grad_buf, double gamma, double lambda, std::optional<double> scale) {
    req(reward, "reward");
    TORCH_CHECK(reward.dim() == 2, "reward: expected (T,B), got ", reward.sizes());
    const int64_t T = reward.size(0), B = reward.size(1);
    const at::Device dev = reward.device();
    req(value, "value", dev, {T + 1, B});
    req(loss, "loss", dev, {1});
    req(grad_buf, "grad_buf", dev, {T, B});
    const int mode = td_weight_mode(weight, T, B, dev);
    c10::DeviceGuard g(dev);
    Tensor partials = new_f32({hpc_rll_partials_floats(B)}, dev);
    check(hpc_rll_td_lambda_forward(fptr(value), fptr(reward), fptr(weight), mode, fmut(loss), fmut(grad_buf),
                                    fmut(partials), to_int(T, "T"), to_int(B, "B"), (float)gamma, (float)lambda,
                                    loss_scale(scale, T * B), stream_of(dev)),
          "hpc_rll_td_lambda_forward");
}

// inputs = [value (T+1,B), reward (T,B), weight (None | (B,) | (T,B))], outputs = [loss (1,), grad_buf (T,B)].
// Reference: src/rl_utils/td_lambda.cu:8-33 (which reads weight as (T,B) whatever its shape: SURVEY.md A.2).
void TdLambdaForward(const OptList& inputs, const TensorList& outputs, double gamma, double lambda,
                     std::optional<double> scale) {
    expect_len(inputs, 3, "TdLambdaForward inputs");
    expect_len(outputs, 2, "TdLambdaForward outputs");
    TORCH_CHECK(has(inputs[0]) && has(inputs[1]), "TdLambdaForward: value / reward must be tensors");
    td_lambda_forward_impl(*inputs[0], *inputs[1], inputs[2], outputs[0], outputs[1], gamma, lambda, scale);
}

// inputs = [grad_loss (scalar tensor), grad_buf (T,B)], outputs = [grad_value (T+1,B)].  td_lambda.cu:35-52.
void TdLambdaBackward(const TensorList& inputs, const TensorList& outputs) {
    expect_len(inputs, 2, "TdLambdaBackward inputs");
    expect_len(outputs, 1, "TdLambdaBackward outputs");
    const Tensor& gb = req(inputs[1], "grad_buf");
    TORCH_CHECK(gb.dim() == 2, "grad_buf: expected (T,B), got ", gb.sizes());
    const int64_t T = gb.size(0), B = gb.size(1);
    Tensor gl = grad1(inputs[0], gb.device(), "grad_loss");
    req(outputs[0], "grad_value", gb.device(), {T + 1, B});
    c10::DeviceGuard g(gb.device());
    check(hpc_rll_td_lambda_backward(fptr(gl), fptr(gb), fmut(outputs[0]), to_int(T, "T"), to_int(B, "B"),
                                     stream_of(gb.device())),
          "hpc_rll_td_lambda_backward");
}

struct TdLambdaFn : public ag::Function<TdLambdaFn> {
    static Tensor forward(ag::AutogradContext* ctx, const Tensor& value, const Tensor& reward, const OptTensor& weight,
                          double gamma, double lambda, std::optional<double> scale) {
        req(reward, "reward");
        TORCH_CHECK(reward.dim() == 2, "reward: expected (T,B), got ", reward.sizes());
        c10::DeviceGuard g(reward.device());
        Tensor loss = new_f32({1}, reward.device());
        Tensor grad_buf = at::empty_like(reward);
        td_lambda_forward_impl(value, reward, weight, loss, grad_buf, gamma, lambda, scale);
        ctx->save_for_backward({grad_buf});
        return loss;
    }
    static ag::tensor_list backward(ag::AutogradContext* ctx, ag::tensor_list grads) {
        const Tensor grad_buf = ctx->get_saved_variables()[0];
        const int64_t T = grad_buf.size(0), B = grad_buf.size(1);
        const at::Device dev = grad_buf.device();
        c10::DeviceGuard g(dev);
        Tensor gl = grad1(grads[0], dev, "grad_loss");
        Tensor gv = new_f32({T + 1, B}, dev);
        check(hpc_rll_td_lambda_backward(fptr(gl), fptr(grad_buf), fmut(gv), (int)T, (int)B, stream_of(dev)),
              "hpc_rll_td_lambda_backward");
        return {gv, undef(), undef(), undef(), undef(), undef()};
    }
};

// ======================================================================================================= V-trace

VtraceDims vtrace_check(const Tensor& target, const Tensor& behaviour, const Tensor& action, const Tensor& value,
                        const Tensor& reward, const OptTensor& weight) {
    req(target, "target_output");
    TORCH_CHECK(target.dim() == 3, "target_output: expected (T,B,N), got ", target.sizes());
    const int64_t T = target.size(0), B = target.size(1), N = target.size(2);
    const at::Device dev = target.device();
    req(behaviour, "behaviour_output", dev, {T, B, N});
    req(action, "action", dev, {T, B}, at::kLong);
    req(value, "value", dev, {T + 1, B});
    req(reward, "reward", dev, {T, B});
    req_opt(weight, "weight", dev, {T, B});
    return {T, B, N, dev};
}

void vtrace_forward_launch(const VtraceDims& d, const Tensor& target, const Tensor& behaviour, const Tensor& action,
                           const Tensor& value, const Tensor& reward, const OptTensor& weight, const Tensor& losses,
                           const Tensor& ws, double gamma, double lambda, double rho_clip, double c_clip,
                           double rho_pg_clip, std::optional<double> scale) {
    check(hpc_rll_vtrace_forward(fptr(target), fptr(behaviour), iptr(action), fptr(value), fptr(reward), fptr(weight),
                                 fmut(losses), fmut(ws), to_int(d.T, "T"), to_int(d.B, "B"), to_int(d.N, "N"),
                                 (float)gamma, (float)lambda, (float)rho_clip, (float)c_clip, (float)rho_pg_clip,
                                 loss_scale(scale, d.T * d.B), stream_of(d.dev)),
          "hpc_rll_vtrace_forward");
}

Tensor vtrace_workspace(int64_t T, int64_t B, const at::Device& dev) {
    return new_f32({hpc_rll_vtrace_workspace_floats(to_int(T, "T"), to_int(B, "B"))}, dev);
}

void vtrace_backward_launch(const Tensor& g_pg, const Tensor& g_v, const Tensor& g_ent, const Tensor& target,
                            const Tensor& action, const Tensor& ws, const Tensor& grad_target, const Tensor& grad_value) {
    const at::Device dev = target.device();
    check(hpc_rll_vtrace_backward(fptr(g_pg), fptr(g_v), fptr(g_ent), fptr(target), iptr(action), fptr(ws),
                                  fmut(grad_target), fmut(grad_value), (int)target.size(0), (int)target.size(1),
                                  (int)target.size(2), stream_of(dev)),
          "hpc_rll_vtrace_backward");
}

struct VtraceFn : public ag::Function<VtraceFn> {
    static ag::tensor_list forward(ag::AutogradContext* ctx, const Tensor& target, const Tensor& behaviour,
                                   const Tensor& action, const Tensor& value, const Tensor& reward,
                                   const OptTensor& weight, double gamma, double lambda, double rho_clip, double c_clip,
                                   double rho_pg_clip, std::optional<double> scale) {
        const VtraceDims d = vtrace_check(target, behaviour, action, value, reward, weight);
        c10::DeviceGuard g(d.dev);
        Tensor losses = new_f32({3}, d.dev);
        Tensor ws = vtrace_workspace(d.T, d.B, d.dev);
        vtrace_forward_launch(d, target, behaviour, action, value, reward, weight, losses, ws, gamma, lambda, rho_clip,
                              c_clip, rho_pg_clip, scale);
        ctx->save_for_backward({target, action, ws});
        return split1(losses, 3);
    }
    static ag::tensor_list backward(ag::AutogradContext* ctx, ag::tensor_list grads) {
        ag::tensor_list out(12);
        const bool need_t = ctx->needs_input_grad(0), need_v = ctx->needs_input_grad(3);
        if (!(need_t || need_v)) return out;
        const auto saved = ctx->get_saved_variables();
        const Tensor &target = saved[0], &action = saved[1], &ws = saved[2];
        const at::Device dev = target.device();
        c10::DeviceGuard g(dev);
        const int64_t T = target.size(0), B = target.size(1);
        const auto [g_pg, g_v, g_e] = grad3(grads, dev);
        Tensor grad_target = need_t ? at::empty_like(target) : undef();
        Tensor grad_value = need_v ? new_f32({T + 1, B}, dev) : undef();
        vtrace_backward_launch(g_pg, g_v, g_e, target, action, ws, grad_target, grad_value);
        out[0] = grad_target;
        out[3] = grad_value;
        return out;
    }
};

// ============================================================================ TD(lambda) and V-trace with done masks
// Episode-aware returns (hpc_rll_td_lambda_masked_forward / hpc_rll_vtrace_masked_forward): the masks, the two value forms
// and the checks of gae_masked; only the forward scans differ from td_lambda / vtrace, whose backward entry points consume
// the saved per-sample coefficients.  Shapes and dtypes are checked before the device, so that a wrong argument is named
// even on host tensors.
// weight None | (B,) | (T,B) -> weight_mode 0 / 1 / 2 (dtype and shape only; the device is checked by the caller)
int masked_td_weight_mode(const OptTensor& weight, int64_t T, int64_t B) {
    if (!has(weight)) return 0;
    const Tensor& w = *weight;
    TORCH_CHECK(w.scalar_type() == at::kFloat, "weight: dtype ", w.scalar_type(), ", expected float32");
    if (w.dim() == 2 && w.size(0) == T && w.size(1) == B) return 2;
    if (w.dim() == 1 && w.size(0) == B) return 1;
    TORCH_CHECK(false, "weight: shape ", w.sizes(), ", expected (", T, ",", B, ") or (", B, ",)");
}

struct TdLambdaMaskedFn : public ag::Function<TdLambdaMaskedFn> {
    static Tensor forward(ag::AutogradContext* ctx, const Tensor& value, const Tensor& reward, const OptTensor& done,
                          const OptTensor& flag, const OptTensor& next_value, const OptTensor& weight, double gamma,
                          double lambda, std::optional<double> scale) {
        TORCH_CHECK(reward.defined() && value.defined(), "td_lambda_masked: value and reward are required");
        TORCH_CHECK(reward.dim() == 2, "reward: expected (T,B), got ", reward.sizes());
        const int64_t T = reward.size(0), B = reward.size(1);
        const int mode = masked_td_weight_mode(weight, T, B);
        const Masks m = check_masked_inputs("td_lambda_masked", value, reward, done, flag, next_value);
        const at::Device dev = reward.device();
        if (mode) req(*weight, "weight", dev);
        c10::DeviceGuard g(dev);
        Tensor loss = new_f32({1}, dev);
        Tensor grad_buf = at::empty_like(reward);
        Tensor partials = new_f32({hpc_rll_partials_floats(B)}, dev);
        check(hpc_rll_td_lambda_masked_forward(fptr(value), fptr(next_value), fptr(reward), fptr(weight), mode,
                                               vptr(m.done), vptr(m.flag), m.code, fmut(loss), fmut(grad_buf),
                                               fmut(partials), to_int(T, "T"), to_int(B, "B"), (float)gamma,
                                               (float)lambda, loss_scale(scale, T * B), stream_of(dev)),
              "hpc_rll_td_lambda_masked_forward");
        ctx->save_for_backward({grad_buf});
        ctx->saved_data["stacked"] = !has(next_value);
        return loss;
    }
    static ag::tensor_list backward(ag::AutogradContext* ctx, ag::tensor_list grads) {
        const Tensor grad_buf = ctx->get_saved_variables()[0];
        const bool stacked = ctx->saved_data["stacked"].toBool();
        const int64_t T = grad_buf.size(0), B = grad_buf.size(1);
        const at::Device dev = grad_buf.device();
        c10::DeviceGuard g(dev);
        Tensor gl = grad1(grads[0], dev, "grad_loss");
        Tensor gv = new_f32({stacked ? T + 1 : T, B}, dev);
        if (stacked)
            check(hpc_rll_td_lambda_backward(fptr(gl), fptr(grad_buf), fmut(gv), (int)T, (int)B, stream_of(dev)),
                  "hpc_rll_td_lambda_backward");
        else
            check(hpc_rll_scale_rows(fptr(gl), fptr(grad_buf), fmut(gv), T * B, T * B, stream_of(dev)),
                  "hpc_rll_scale_rows");
        ag::tensor_list out(9);
        out[0] = gv;
        return out;
    }
};

struct VtraceMaskedFn : public ag::Function<VtraceMaskedFn> {
    static ag::tensor_list forward(ag::AutogradContext* ctx, const Tensor& target, const Tensor& behaviour,
                                   const Tensor& action, const Tensor& value, const Tensor& reward,
                                   const OptTensor& done, const OptTensor& flag, const OptTensor& next_value,
                                   const OptTensor& weight, double gamma, double lambda, double rho_clip,
                                   double c_clip, double rho_pg_clip, std::optional<double> scale) {
        TORCH_CHECK(target.defined(), "target_output: expected a tensor, got None");
        TORCH_CHECK(target.dim() == 3, "target_output: expected (T,B,N), got ", target.sizes());
        const int64_t T = target.size(0), B = target.size(1), N = target.size(2);
        Args args;
        args.add(target, "target_output", {T, B, N});
        args.add(behaviour, "behaviour_output", {T, B, N});
        args.add(action, "action", {T, B}, at::kLong);
        check_shape(reward, "reward", {T, B});   // its device is check_masked_inputs's
        args.add(weight, "weight", {T, B});
        const Masks m = check_masked_inputs("vtrace_masked", value, reward, done, flag, next_value);
        const at::Device dev = args.on_device_of(reward);
        c10::DeviceGuard g(dev);
        Tensor losses = new_f32({3}, dev);
        Tensor ws = vtrace_workspace(T, B, dev);
        check(hpc_rll_vtrace_masked_forward(fptr(target), fptr(behaviour), iptr(action), fptr(value), fptr(next_value),
                                            fptr(reward), fptr(weight), vptr(m.done), vptr(m.flag), m.code,
                                            fmut(losses), fmut(ws), to_int(T, "T"), to_int(B, "B"), to_int(N, "N"),
                                            (float)gamma, (float)lambda, (float)rho_clip, (float)c_clip,
                                            (float)rho_pg_clip, loss_scale(scale, T * B), stream_of(dev)),
              "hpc_rll_vtrace_masked_forward");
        ctx->save_for_backward({target, action, ws});
        ctx->saved_data["stacked"] = !has(next_value);
        return split1(losses, 3);
    }
    static ag::tensor_list backward(ag::AutogradContext* ctx, ag::tensor_list grads) {
        ag::tensor_list out(15);
        const bool need_t = ctx->needs_input_grad(0), need_v = ctx->needs_input_grad(3);
        if (!(need_t || need_v)) return out;
        const bool stacked = ctx->saved_data["stacked"].toBool();
        const auto saved = ctx->get_saved_variables();
        const Tensor &target = saved[0], &action = saved[1], &ws = saved[2];
        const at::Device dev = target.device();
        c10::DeviceGuard g(dev);
        const int64_t T = target.size(0), B = target.size(1);
        const auto [g_pg, g_v, g_e] = grad3(grads, dev);
        Tensor grad_target = need_t ? at::empty_like(target) : undef();
        Tensor grad_value = need_v ? new_f32({stacked ? T + 1 : T, B}, dev) : undef();
        // next-value form: the unit value gradient (ws rows 2T*B ...) has T rows and no bootstrap row to zero
        vtrace_backward_launch(g_pg, g_v, g_e, target, action, ws, grad_target, stacked ? grad_value : undef());
        if (need_v && !stacked)
            check(hpc_rll_scale_rows(fptr(g_v), fptr(ws) + 2 * T * B, fmut(grad_value), T * B, T * B, stream_of(dev)),
                  "hpc_rll_scale_rows");
        out[0] = grad_target;
        out[3] = grad_value;
        return out;
    }
};

// ========================================================================================================== UPGO
struct UpgoFn : public ag::Function<UpgoFn> {
    static Tensor forward(ag::AutogradContext* ctx, const Tensor& target, const Tensor& rho, const Tensor& action,
                          const Tensor& reward, const Tensor& value, std::optional<double> scale);
    static ag::tensor_list backward(ag::AutogradContext* ctx, ag::tensor_list grads);
};

UpgoDims upgo_check(const Tensor& target, const Tensor& rho, const Tensor& action, const Tensor& reward,
                    const Tensor& value) {
    req(target, "target_output");
    TORCH_CHECK(target.dim() == 3, "target_output: expected (T,B,N), got ", target.sizes());
    const int64_t T = target.size(0), B = target.size(1), N = target.size(2);
    const at::Device dev = target.device();
    req(rho, "rhos", dev, {T, B});
    req(action, "action", dev, {T, B}, at::kLong);
    req(reward, "rewards", dev, {T, B});
    req(value, "bootstrap_values", dev, {T + 1, B});
    return {T, B, N, dev};
}
Tensor upgo_workspace(int64_t T, int64_t B, const at::Device& dev) {
    return new_f32({hpc_rll_upgo_workspace_floats(to_int(T, "T"), to_int(B, "B"))}, dev);
}
void upgo_forward_launch(const UpgoDims& d, const Tensor& target, const Tensor& rho, const Tensor& action,
                         const Tensor& reward, const Tensor& value, const Tensor& loss, const Tensor& ws,
                         std::optional<double> scale) {
    check(hpc_rll_upgo_forward(fptr(target), fptr(rho), iptr(action), fptr(reward), fptr(value), fmut(loss), fmut(ws),
                               to_int(d.T, "T"), to_int(d.B, "B"), to_int(d.N, "N"), loss_scale(scale, d.T * d.B),
                               stream_of(d.dev)),
          "hpc_rll_upgo_forward");
}
void upgo_backward_launch(const Tensor& g, const Tensor& target, const Tensor& action, const Tensor& ws,
                          const Tensor& grad_target) {
    check(hpc_rll_upgo_backward(g.defined() ? fptr(g) : nullptr, fptr(target), iptr(action), fptr(ws),
                                fmut(grad_target), (int)target.size(0), (int)target.size(1), (int)target.size(2),
                                stream_of(target.device())),
          "hpc_rll_upgo_backward");
}

Tensor UpgoFn::forward(ag::AutogradContext* ctx, const Tensor& target, const Tensor& rho, const Tensor& action,
                       const Tensor& reward, const Tensor& value, std::optional<double> scale) {
    const UpgoDims d = upgo_check(target, rho, action, reward, value);
    c10::DeviceGuard g(d.dev);
    Tensor loss = new_f32({1}, d.dev);
    Tensor ws = upgo_workspace(d.T, d.B, d.dev);
    upgo_forward_launch(d, target, rho, action, reward, value, loss, ws, scale);
    ctx->save_for_backward({target, action, ws});
    return loss;
}
ag::tensor_list UpgoFn::backward(ag::AutogradContext* ctx, ag::tensor_list grads) {
    ag::tensor_list out(6);
    if (!ctx->needs_input_grad(0)) return out;
    const auto saved = ctx->get_saved_variables();
    const Tensor& target = saved[0];
    c10::DeviceGuard g(target.device());
    Tensor gl = grad1(grads[0], target.device(), "grad_loss");
    Tensor grad_target = at::empty_like(target);
    upgo_backward_launch(gl, target, saved[1], saved[2], grad_target);
    out[0] = grad_target;
    return out;
}

// UPGO with done masks (hpc_rll_upgo_masked_forward): the masks, the two value forms and the checks of the masked ops
// above; the workspace and the backward are UpgoFn's.  Shapes and dtypes are checked before the device.
struct UpgoMaskedFn : public ag::Function<UpgoMaskedFn> {
    static Tensor forward(ag::AutogradContext* ctx, const Tensor& target, const Tensor& rho, const Tensor& action,
                          const Tensor& reward, const Tensor& value, const OptTensor& done, const OptTensor& flag,
                          const OptTensor& next_value, double gamma, std::optional<double> scale) {
        TORCH_CHECK(target.defined(), "target_output: expected a tensor, got None");
        TORCH_CHECK(target.dim() == 3, "target_output: expected (T,B,N), got ", target.sizes());
        const int64_t T = target.size(0), B = target.size(1), N = target.size(2);
        Args args;
        args.add(target, "target_output", {T, B, N});
        args.add(rho, "rhos", {T, B});
        args.add(action, "action", {T, B}, at::kLong);
        check_shape(reward, "rewards", {T, B});   // its device is check_masked_inputs's
        const Masks m = check_masked_inputs("upgo_masked", value, reward, done, flag, next_value);
        const at::Device dev = args.on_device_of(reward);
        c10::DeviceGuard g(dev);
        Tensor loss = new_f32({1}, dev);
        Tensor ws = upgo_workspace(T, B, dev);
        check(hpc_rll_upgo_masked_forward(fptr(target), fptr(rho), iptr(action), fptr(reward), fptr(value),
                                          fptr(next_value), vptr(m.done), vptr(m.flag), m.code, fmut(loss), fmut(ws),
                                          to_int(T, "T"), to_int(B, "B"), to_int(N, "N"), (float)gamma,
                                          loss_scale(scale, T * B), stream_of(dev)),
              "hpc_rll_upgo_masked_forward");
        ctx->save_for_backward({target, action, ws});
        return loss;
    }
    static ag::tensor_list backward(ag::AutogradContext* ctx, ag::tensor_list grads) {
        ag::tensor_list out(10);
        if (!ctx->needs_input_grad(0)) return out;
        const auto saved = ctx->get_saved_variables();
        const Tensor& target = saved[0];
        c10::DeviceGuard g(target.device());
        Tensor gl = grad1(grads[0], target.device(), "grad_loss");
        Tensor grad_target = at::empty_like(target);
        upgo_backward_launch(gl, target, saved[1], saved[2], grad_target);
        out[0] = grad_target;
        return out;
    }
};

// =========================================================================================================== PPO
PpoDims ppo_check(const Tensor& ln, const Tensor& lo, const Tensor& action, const Tensor& vn, const Tensor& vo,
                  const Tensor& adv, const Tensor& ret, const OptTensor& weight) {
    req(ln, "logits_new");
    TORCH_CHECK(ln.dim() == 2, "logits_new: expected (B,N), got ", ln.sizes());
    const int64_t B = ln.size(0), N = ln.size(1);
    const at::Device dev = ln.device();
    req(lo, "logits_old", dev, {B, N});
    req(action, "action", dev, {B}, at::kLong);
    req(vn, "value_new", dev, {B});
    req(vo, "value_old", dev, {B});
    req(adv, "adv", dev, {B});
    req(ret, "return_", dev, {B});
    req_opt(weight, "weight", dev, {B});
    return {B, N, dev};
}
Tensor ppo_workspace(int64_t B, const at::Device& dev) {
    return new_f32({hpc_rll_ppo_workspace_floats(to_int(B, "B"))}, dev);
}
void ppo_forward_launch(const PpoDims& d, const Tensor& ln, const Tensor& lo, const Tensor& action, const Tensor& vn,
                        const Tensor& vo, const Tensor& adv, const Tensor& ret, const OptTensor& weight,
                        const Tensor& out5, const Tensor& ws, bool use_value_clip, double clip_ratio, double dual_clip,
                        std::optional<double> scale) {
    check(hpc_rll_ppo_forward(fptr(ln), fptr(lo), iptr(action), fptr(vn), fptr(vo), fptr(adv), fptr(ret), fptr(weight),
                              fmut(out5), fmut(ws), to_int(d.B, "B"), to_int(d.N, "N"), (float)clip_ratio,
                              use_value_clip ? 1 : 0, (float)dual_clip, loss_scale(scale, d.B), stream_of(d.dev)),
          "hpc_rll_ppo_forward");
}
void ppo_backward_launch(const Tensor& g_p, const Tensor& g_v, const Tensor& g_e, const Tensor& ln, const Tensor& action,
                         const Tensor& ws, const Tensor& grad_logits, const Tensor& grad_value) {
    check(hpc_rll_ppo_backward(fptr(g_p), fptr(g_v), fptr(g_e), fptr(ln), iptr(action), fptr(ws), fmut(grad_logits),
                               fmut(grad_value), (int)ln.size(0), (int)ln.size(1), stream_of(ln.device())),
          "hpc_rll_ppo_backward");
}

struct PpoFn : public ag::Function<PpoFn> {
    static ag::tensor_list forward(ag::AutogradContext* ctx, const Tensor& ln, const Tensor& lo, const Tensor& action,
                                   const Tensor& vn, const Tensor& vo, const Tensor& adv, const Tensor& ret,
                                   const OptTensor& weight, double clip_ratio, bool use_value_clip, double dual_clip,
                                   std::optional<double> scale) {
        const PpoDims d = ppo_check(ln, lo, action, vn, vo, adv, ret, weight);
        c10::DeviceGuard g(d.dev);
        Tensor out5 = new_f32({5}, d.dev);
        Tensor ws = ppo_workspace(d.B, d.dev);
        ppo_forward_launch(d, ln, lo, action, vn, vo, adv, ret, weight, out5, ws, use_value_clip, clip_ratio, dual_clip,
                           scale);
        ctx->save_for_backward({ln, action, ws});
        Tensor info = alias_of(out5, 3, 2);
        ctx->mark_non_differentiable({info});
        return {alias_of(out5, 0, 1), alias_of(out5, 1, 1), alias_of(out5, 2, 1), info};
    }
    static ag::tensor_list backward(ag::AutogradContext* ctx, ag::tensor_list grads) {
        ag::tensor_list out(12);
        const bool need_l = ctx->needs_input_grad(0), need_v = ctx->needs_input_grad(3);
        if (!(need_l || need_v)) return out;
        const auto saved = ctx->get_saved_variables();
        const Tensor &ln = saved[0], &action = saved[1], &ws = saved[2];
        const at::Device dev = ln.device();
        c10::DeviceGuard g(dev);
        const auto [g_p, g_v, g_e] = grad3(grads, dev);
        Tensor grad_logits = need_l ? at::empty_like(ln) : undef();
        Tensor grad_value = need_v ? new_f32({ln.size(0)}, dev) : undef();
        ppo_backward_launch(g_p, g_v, g_e, ln, action, ws, grad_logits, grad_value);
        out[0] = grad_logits;
        out[3] = grad_value;
        return out;
    }
};

// ============================================================================================ PPO, Gaussian head
PpoContinuousDims ppo_continuous_check(const Tensor& mu_new, const Tensor& sigma_new, const Tensor& mu_old,
                                       const Tensor& sigma_old, const Tensor& action, const Tensor& vn, const Tensor& vo,
                                       const Tensor& adv, const Tensor& ret, const OptTensor& weight) {
    req(mu_new, "mu_new");
    TORCH_CHECK(mu_new.dim() == 2, "mu_new: expected (B,A), got ", mu_new.sizes());
    const int64_t B = mu_new.size(0), A = mu_new.size(1);
    const at::Device dev = mu_new.device();
    req(sigma_new, "sigma_new", dev, {B, A});
    req(mu_old, "mu_old", dev, {B, A});
    req(sigma_old, "sigma_old", dev, {B, A});
    req(action, "action", dev, {B, A});
    req(vn, "value_new", dev, {B});
    req(vo, "value_old", dev, {B});
    req(adv, "adv", dev, {B});
    req(ret, "return_", dev, {B});
    req_opt(weight, "weight", dev, {B});
    TORCH_CHECK(A >= 1, "mu_new: the action dimension must be at least 1, got ", mu_new.sizes());
    return {B, A, dev};
}

struct PpoContinuousFn : public ag::Function<PpoContinuousFn> {
    static ag::tensor_list forward(ag::AutogradContext* ctx, const Tensor& mu_new, const Tensor& sigma_new,
                                   const Tensor& mu_old, const Tensor& sigma_old, const Tensor& action, const Tensor& vn,
                                   const Tensor& vo, const Tensor& adv, const Tensor& ret, const OptTensor& weight,
                                   double clip_ratio, bool use_value_clip, double dual_clip, std::optional<double> scale) {
        const PpoContinuousDims d = ppo_continuous_check(mu_new, sigma_new, mu_old, sigma_old, action, vn, vo, adv, ret, weight);
        c10::DeviceGuard g(d.dev);
        const int B = to_int(d.B, "B"), A = to_int(d.A, "A");
        Tensor out5 = new_f32({5}, d.dev);
        Tensor ws = new_f32({hpc_rll_ppo_continuous_workspace_floats(B)}, d.dev);
        const int rc = hpc_rll_ppo_continuous_forward(
            fptr(mu_new), fptr(sigma_new), fptr(mu_old), fptr(sigma_old), fptr(action), fptr(vn), fptr(vo), fptr(adv), fptr(ret),
            fptr(weight), fmut(out5), fmut(ws), B, A, (float)clip_ratio, use_value_clip ? 1 : 0, (float)dual_clip,
            loss_scale(scale, d.B), stream_of(d.dev));
        TORCH_CHECK(rc != HPC_RLL_EUNSUPPORTED, "ppo_continuous: an action dimension of ", A,
                    " is not supported by the gfx950 kernels (1 <= A <= 1024)");
        check(rc, "hpc_rll_ppo_continuous_forward");
        ctx->save_for_backward({mu_new, sigma_new, action, ws});
        Tensor info = alias_of(out5, 3, 2);
        ctx->mark_non_differentiable({info});
        return {alias_of(out5, 0, 1), alias_of(out5, 1, 1), alias_of(out5, 2, 1), info};
    }
    static ag::tensor_list backward(ag::AutogradContext* ctx, ag::tensor_list grads) {
        ag::tensor_list out(14);
        const bool need_m = ctx->needs_input_grad(0), need_s = ctx->needs_input_grad(1), need_v = ctx->needs_input_grad(5);
        if (!(need_m || need_s || need_v)) return out;
        const auto saved = ctx->get_saved_variables();
        const Tensor &mu_new = saved[0], &sigma_new = saved[1], &action = saved[2], &ws = saved[3];
        const at::Device dev = mu_new.device();
        c10::DeviceGuard g(dev);
        const auto [g_p, g_v, g_e] = grad3(grads, dev);
        Tensor grad_mu = need_m ? at::empty_like(mu_new) : undef();
        Tensor grad_sigma = need_s ? at::empty_like(sigma_new) : undef();
        Tensor grad_value = need_v ? new_f32({mu_new.size(0)}, dev) : undef();
        check(hpc_rll_ppo_continuous_backward(fptr(g_p), fptr(g_v), fptr(g_e), fptr(mu_new), fptr(sigma_new), fptr(action),
                                              fptr(ws), fmut(grad_mu), fmut(grad_sigma), fmut(grad_value),
                                              (int)mu_new.size(0), (int)mu_new.size(1), stream_of(dev)),
              "hpc_rll_ppo_continuous_backward");
        out[0] = grad_mu;
        out[1] = grad_sigma;
        out[5] = grad_value;
        return out;
    }
};

// V-trace with a diagonal-Gaussian head (hpc_rll_vtrace_continuous_*): the masks, value forms and checks of vtrace_masked;
// mu / sigma of the target and the behaviour policy and the action are (T,B,A) fp32.  Gradients flow to mu_target,
// sigma_target and value; backward allocates only the gradients autograd asks for.
struct VtraceContinuousFn : public ag::Function<VtraceContinuousFn> {
    static ag::tensor_list forward(ag::AutogradContext* ctx, const Tensor& mu_t, const Tensor& sigma_t, const Tensor& mu_b,
                                   const Tensor& sigma_b, const Tensor& action, const Tensor& value, const Tensor& reward,
                                   const OptTensor& done, const OptTensor& flag, const OptTensor& next_value,
                                   const OptTensor& weight, double gamma, double lambda, double rho_clip, double c_clip,
                                   double rho_pg_clip, std::optional<double> scale) {
        TORCH_CHECK(mu_t.defined(), "mu_target: expected a tensor, got None");
        TORCH_CHECK(mu_t.dim() == 3, "mu_target: expected (T,B,A), got ", mu_t.sizes());
        const int64_t T = mu_t.size(0), B = mu_t.size(1), A = mu_t.size(2);
        Args args;
        args.add(mu_t, "mu_target", {T, B, A});
        args.add(sigma_t, "sigma_target", {T, B, A});
        args.add(mu_b, "mu_behaviour", {T, B, A});
        args.add(sigma_b, "sigma_behaviour", {T, B, A});
        args.add(action, "action", {T, B, A});
        check_shape(reward, "reward", {T, B});   // its device is check_masked_inputs's
        args.add(weight, "weight", {T, B});
        TORCH_CHECK(A >= 1 && A <= 1024, "vtrace_continuous: an action dimension of ", A,
                    " is not supported by the gfx950 kernels (1 <= A <= 1024)");
        const Masks m = check_masked_inputs("vtrace_continuous", value, reward, done, flag, next_value);
        const at::Device dev = args.on_device_of(reward);
        c10::DeviceGuard g(dev);
        Tensor losses = new_f32({3}, dev);
        Tensor ws = vtrace_workspace(T, B, dev);
        check(hpc_rll_vtrace_continuous_forward(fptr(mu_t), fptr(sigma_t), fptr(mu_b), fptr(sigma_b), fptr(action),
                                                fptr(value), fptr(next_value), fptr(reward), fptr(weight), vptr(m.done),
                                                vptr(m.flag), m.code, fmut(losses), fmut(ws), to_int(T, "T"),
                                                to_int(B, "B"), to_int(A, "A"), (float)gamma, (float)lambda,
                                                (float)rho_clip, (float)c_clip, (float)rho_pg_clip,
                                                loss_scale(scale, T * B), stream_of(dev)),
              "hpc_rll_vtrace_continuous_forward");
        ctx->save_for_backward({mu_t, sigma_t, action, ws});
        ctx->saved_data["stacked"] = !has(next_value);
        return split1(losses, 3);
    }
    static ag::tensor_list backward(ag::AutogradContext* ctx, ag::tensor_list grads) {
        ag::tensor_list out(17);
        const bool need_m = ctx->needs_input_grad(0), need_s = ctx->needs_input_grad(1), need_v = ctx->needs_input_grad(5);
        if (!(need_m || need_s || need_v)) return out;
        const bool stacked = ctx->saved_data["stacked"].toBool();
        const auto saved = ctx->get_saved_variables();
        const Tensor &mu_t = saved[0], &sigma_t = saved[1], &action = saved[2], &ws = saved[3];
        const at::Device dev = mu_t.device();
        c10::DeviceGuard g(dev);
        const int64_t T = mu_t.size(0), B = mu_t.size(1), A = mu_t.size(2);
        const auto [g_pg, g_v, g_e] = grad3(grads, dev);
        Tensor grad_mu = need_m ? at::empty_like(mu_t) : undef();
        Tensor grad_sigma = need_s ? at::empty_like(sigma_t) : undef();
        Tensor grad_value = need_v ? new_f32({stacked ? T + 1 : T, B}, dev) : undef();
        // next-value form: the unit value gradient (ws rows 2T*B ...) has T rows and no bootstrap row to zero
        check(hpc_rll_vtrace_continuous_backward(fptr(g_pg), fptr(g_v), fptr(g_e), fptr(mu_t), fptr(sigma_t), fptr(action),
                                                 fptr(ws), fmut(grad_mu), fmut(grad_sigma),
                                                 fmut(stacked ? grad_value : undef()), (int)T, (int)B, (int)A,
                                                 stream_of(dev)),
              "hpc_rll_vtrace_continuous_backward");
        if (need_v && !stacked)
            check(hpc_rll_scale_rows(fptr(g_v), fptr(ws) + 2 * T * B, fmut(grad_value), T * B, T * B, stream_of(dev)),
                  "hpc_rll_scale_rows");
        out[0] = grad_mu;
        out[1] = grad_sigma;
        out[5] = grad_value;
        return out;
    }
};

// ======================================================================================================= Retrace
// Retrace(lambda) Q targets for discrete actions (hpc_rll_retrace_*; DI-engine's compute_q_retraces / acer_value_error).
// Shapes and dtypes are checked before the device so that a wrong argument is named even on host tensors.
Tensor retrace_workspace(int64_t T, int64_t B, const at::Device& dev) {
    return new_f32({hpc_rll_retrace_workspace_floats(to_int(T, "T"), to_int(B, "B"))}, dev);
}
void retrace_check_n(const char* op, int64_t N) {
    TORCH_CHECK(N >= 1 && N <= 1024, op, ": an action count of ", N, " is not supported by the gfx950 kernels (1 <= N <= 1024)");
}

// The drop-in form: v_pred (T+1,B,1) and ratio (T,B,N) are given; q_retraces (T+1,B,1), no gradient.
Tensor retrace_targets(const Tensor& q, const Tensor& v_pred, const Tensor& reward, const Tensor& action,
                       const OptTensor& weights, const Tensor& ratio, double gamma, double lambda) {
    TORCH_CHECK(q.defined(), "q_values: expected a tensor, got None");
    TORCH_CHECK(q.dim() == 3 && q.size(0) >= 1, "q_values: expected (T+1,B,N), got ", q.sizes());
    const int64_t T = q.size(0) - 1, B = q.size(1), N = q.size(2);
    Args args;
    args.add(q, "q_values", {T + 1, B, N});
    args.add(v_pred, "v_pred", {T + 1, B, 1});
    args.add(reward, "rewards", {T, B});
    args.add(action, "actions", {T, B}, at::kLong);
    args.add(weights, "weights", {T, B});
    args.add(ratio, "ratio", {T, B, N});
    retrace_check_n("retrace", N);
    const at::Device dev = args.on_device_of(q);
    c10::DeviceGuard g(dev);
    if (T == 0 || B == 0) return v_pred.detach().clone();   // no step: Q_T = v_T
    Tensor out = new_f32({T + 1, B, 1}, dev);
    Tensor ws = new_f32({2 * T * B}, dev);
    check(hpc_rll_retrace_forward(fptr(q), fptr(v_pred), fptr(reward), iptr(action), fptr(weights), fptr(ratio), fmut(out),
                                  fmut(ws), to_int(T, "T"), to_int(B, "B"), to_int(N, "N"), (float)gamma, (float)lambda,
                                  stream_of(dev)),
          "hpc_rll_retrace_forward");
    return out;
}

// The fused form: heads, scan and critic loss; the gradient flows to q_values only.  Saves action and the workspace (delta).
struct RetraceLossFn : public ag::Function<RetraceLossFn> {
    static ag::tensor_list forward(ag::AutogradContext* ctx, const Tensor& q, const Tensor& target, const Tensor& behaviour,
                                   const Tensor& action, const Tensor& reward, const OptTensor& weights,
                                   const OptTensor& loss_weight, double gamma, double lambda, std::optional<double> scale) {
        TORCH_CHECK(q.defined(), "q_values: expected a tensor, got None");
        TORCH_CHECK(q.dim() == 3 && q.size(0) >= 1, "q_values: expected (T+1,B,N), got ", q.sizes());
        const int64_t T = q.size(0) - 1, B = q.size(1), N = q.size(2);
        Args args;
        args.add(q, "q_values", {T + 1, B, N});
        args.add(target, "target_output", {T + 1, B, N});
        args.add(behaviour, "behaviour_output", {T, B, N});
        args.add(action, "action", {T, B}, at::kLong);
        args.add(reward, "reward", {T, B});
        args.add(weights, "weights", {T, B});
        args.add(loss_weight, "loss_weight", {T, B});
        retrace_check_n("retrace_loss", N);
        const at::Device dev = args.on_device_of(q);
        c10::DeviceGuard g(dev);
        const bool empty = T == 0 || B == 0;
        Tensor loss = new_f32({1}, dev);
        // no step: the loss is zero and nothing is launched; the outputs are then zeros
        Tensor q_ret = empty ? at::zeros({T + 1, B}, q.options()) : new_f32({T + 1, B}, dev);
        Tensor v = empty ? at::zeros({T + 1, B}, q.options()) : new_f32({T + 1, B}, dev);
        Tensor ws = retrace_workspace(T, B, dev);
        check(hpc_rll_retrace_loss_forward(fptr(q), fptr(target), fptr(behaviour), iptr(action), fptr(reward), fptr(weights),
                                           fptr(loss_weight), fmut(loss), fmut(q_ret), fmut(v), fmut(ws), to_int(T, "T"),
                                           to_int(B, "B"), to_int(N, "N"), (float)gamma, (float)lambda,
                                           loss_scale(scale, T * B), stream_of(dev)),
              "hpc_rll_retrace_loss_forward");
        ctx->save_for_backward({action, ws});
        ctx->saved_data["N"] = N;
        ctx->mark_non_differentiable({q_ret, v});
        return {loss, q_ret, v};
    }
    static ag::tensor_list backward(ag::AutogradContext* ctx, ag::tensor_list grads) {
        ag::tensor_list out(10);
        if (!ctx->needs_input_grad(0)) return out;
        const auto saved = ctx->get_saved_variables();
        const Tensor &action = saved[0], &ws = saved[1];
        const at::Device dev = action.device();
        c10::DeviceGuard g(dev);
        const int64_t T = action.size(0), B = action.size(1), N = ctx->saved_data["N"].toInt();
        Tensor gl = grad1(grads[0], dev, "grad_loss");
        if (T == 0 || B == 0) {
            out[0] = at::zeros({T + 1, B, N}, gl.options());
            return out;
        }
        Tensor grad_q = new_f32({T + 1, B, N}, dev);
        check(hpc_rll_retrace_loss_backward(fptr(gl), iptr(action), fptr(ws), fmut(grad_q), (int)T, (int)B, (int)N,
                                            stream_of(dev)),
              "hpc_rll_retrace_loss_backward");
        out[0] = grad_q;
        return out;
    }
};

// ========================================================================================================== ACER
// ACER's actor loss (hpc_rll_acer_*; DI-engine's acer_policy_error and acer_trust_region_update).  T is action's; the tensors
// retrace_loss takes and returns may keep their T+1 rows (only the first T are read).  Shapes and dtypes are checked before
// the device so that a wrong argument is named even on host tensors.
int64_t acer_check_rows(const Tensor& t, const char* name, int64_t T, std::initializer_list<int64_t> rest) {
    TORCH_CHECK(t.defined(), name, ": expected a tensor, got None");
    TORCH_CHECK(t.scalar_type() == at::kFloat, name, ": dtype ", t.scalar_type(), ", expected ", at::kFloat);
    std::vector<int64_t> want{T};
    want.insert(want.end(), rest.begin(), rest.end());
    bool ok = t.dim() == (int64_t)want.size() && (t.size(0) == T || t.size(0) == T + 1);
    for (size_t i = 1; ok && i < want.size(); ++i) ok = t.size(i) == want[i];
    TORCH_CHECK(ok, name, ": shape ", t.sizes(), ", expected ", at::IntArrayRef(want), " or one more leading row");
    return t.size(0);
}

// The gradient flows to target_output only.  Saves the unit gradient (T,B,N), which is allocated only when it is wanted.
struct AcerPolicyFn : public ag::Function<AcerPolicyFn> {
    static ag::tensor_list forward(ag::AutogradContext* ctx, const Tensor& target, const Tensor& behaviour, const Tensor& q,
                                   const Tensor& q_ret, const Tensor& v_pred, const Tensor& action, const OptTensor& weights,
                                   const OptTensor& avg, double c_clip, double entropy_weight, double trust_region,
                                   std::optional<double> scale, bool want_grad) {
        TORCH_CHECK(action.defined(), "action: expected a tensor, got None");
        TORCH_CHECK(action.dim() == 2, "action: expected (T,B), got ", action.sizes());
        TORCH_CHECK(target.defined(), "target_output: expected a tensor, got None");
        TORCH_CHECK(target.dim() == 3, "target_output: expected (T,B,N) or (T+1,B,N), got ", target.sizes());
        const int64_t T = action.size(0), B = action.size(1), N = target.size(2);
        check_shape(action, "action", {T, B}, at::kLong);
        const int64_t target_rows = acer_check_rows(target, "target_output", T, {B, N});
        check_shape(behaviour, "behaviour_output", {T, B, N});
        acer_check_rows(q, "q_values", T, {B, N});
        acer_check_rows(q_ret, "q_retraces", T, {B});
        acer_check_rows(v_pred, "v_pred", T, {B});
        if (has(weights)) check_shape(*weights, "weights", {T, B});
        if (has(avg)) check_shape(*avg, "avg_output", {T, B, N});
        retrace_check_n("acer_policy_loss", N);
        const at::Device dev = target.device();
        req(target, "target_output", dev);
        req(behaviour, "behaviour_output", dev);
        req(q, "q_values", dev);
        req(q_ret, "q_retraces", dev);
        req(v_pred, "v_pred", dev);
        req(action, "action", dev, at::kLong);
        if (has(weights)) req(*weights, "weights", dev);
        if (has(avg)) req(*avg, "avg_output", dev);
        c10::DeviceGuard g(dev);
        Tensor out4 = new_f32({4}, dev);
        Tensor unit = (want_grad && T * B > 0) ? new_f32({T, B, N}, dev) : undef();
        Tensor ws = new_f32({hpc_rll_acer_policy_workspace_floats(to_int(T, "T"), to_int(B, "B"))}, dev);
        check(hpc_rll_acer_policy_forward(fptr(target), fptr(behaviour), fptr(avg), fptr(q), fptr(q_ret), fptr(v_pred),
                                          iptr(action), fptr(weights), fmut(out4), fmut(unit), fmut(ws), to_int(T, "T"),
                                          to_int(B, "B"), to_int(N, "N"), (float)c_clip, (float)entropy_weight,
                                          (float)trust_region, loss_scale(scale, T * B), stream_of(dev)),
              "hpc_rll_acer_policy_forward");
        ctx->save_for_backward({unit});
        ctx->saved_data["dims"] = std::vector<int64_t>{T, B, N, target_rows};
        Tensor loss = alias_of(out4, 0, 1), actor = alias_of(out4, 1, 1), bc = alias_of(out4, 2, 1), ent = alias_of(out4, 3, 1);
        ctx->mark_non_differentiable({actor, bc, ent});
        return {loss, actor, bc, ent};
    }
    static ag::tensor_list backward(ag::AutogradContext* ctx, ag::tensor_list grads) {
        ag::tensor_list out(13);
        if (!ctx->needs_input_grad(0)) return out;
        const Tensor unit = ctx->get_saved_variables()[0];
        const std::vector<int64_t> d = ctx->saved_data["dims"].toIntVector();
        const int64_t T = d[0], B = d[1], N = d[2], rows = d[3];
        const at::Device dev = grads[0].device();
        c10::DeviceGuard g(dev);
        Tensor gl = grad1(grads[0], dev, "grad_loss");
        if (T == 0 || B == 0) {
            out[0] = at::zeros({rows, B, N}, gl.options());
            return out;
        }
        TORCH_CHECK(unit.defined(), "acer_policy_loss: the gradient was not stored by the forward");
        Tensor grad = new_f32({rows, B, N}, dev);
        check(hpc_rll_acer_policy_backward(fptr(gl), fptr(unit), fmut(grad), (int)T, (int)B, (int)N, (int)rows, stream_of(dev)),
              "hpc_rll_acer_policy_backward");
        out[0] = grad;
        return out;
    }
};

// DI-engine's acer_trust_region_update for one gradient: both (..., N), avg_logit holds log-probabilities; no gradient.
Tensor acer_trust_region(const Tensor& grad, const Tensor& avg_logit, double trust_region) {
    TORCH_CHECK(grad.defined(), "actor_gradients: expected a tensor, got None");
    TORCH_CHECK(grad.dim() >= 1, "actor_gradients: expected (..., N), got ", grad.sizes());
    Args args;
    args.add(grad, "actor_gradients", grad.sizes());
    args.add(avg_logit, "avg_logit", grad.sizes());
    const int64_t N = grad.size(-1);
    retrace_check_n("acer_trust_region_update", N);
    const at::Device dev = args.on_device_of(grad);
    c10::DeviceGuard g(dev);
    Tensor out = at::empty_like(grad);
    check(hpc_rll_acer_trust_region(fptr(grad), fptr(avg_logit), fmut(out), grad.numel() / N, to_int(N, "N"),
                                    (float)trust_region, stream_of(dev)),
          "hpc_rll_acer_trust_region");
    return out;
}

// ========================================================================================================== COMA
// The counterfactual multi-agent actor-critic loss (hpc_rll_coma_*; DI-engine's coma_error).  Shapes and dtypes are checked
// before the device so that a wrong argument is named even on host tensors.  The gradient flows to logit and q_value; each
// is formed only when its input needs it.  Saves logit, action, weight and the one workspace.
struct ComaFn : public ag::Function<ComaFn> {
    static ag::tensor_list forward(ag::AutogradContext* ctx, const Tensor& logit, const Tensor& action, const Tensor& q,
                                   const Tensor& target_q, const Tensor& reward, const OptTensor& weight,
                                   const OptTensor& done, double gamma, double lambda, std::optional<double> scale_pe,
                                   std::optional<double> scale_q) {
        TORCH_CHECK(logit.defined(), "logit: expected a tensor, got None");
        TORCH_CHECK(logit.dim() == 4, "logit: expected (T,B,A,N), got ", logit.sizes());
        const int64_t T = logit.size(0), B = logit.size(1), A = logit.size(2), N = logit.size(3);
        Args args;
        args.add(logit, "logit", {T, B, A, N});
        args.add(action, "action", {T, B, A}, at::kLong);
        args.add(q, "q_value", {T, B, A, N});
        args.add(target_q, "target_q_value", {T, B, A, N});
        args.add(reward, "reward", {T, B});
        args.add(weight, "weight", {T, B, A});
        const Args::Mask dm = args.add_mask(done, "done", reward.sizes(), " (the shape of reward)");
        retrace_check_n("coma", N);
        TORCH_CHECK(B * A <= INT32_MAX, "coma: B*A = ", B * A, " does not fit the kernels' 32-bit column count");
        const at::Device dev = args.on_device_of(logit);
        c10::DeviceGuard g(dev);
        Tensor losses = new_f32({3}, dev);
        const int64_t nws = hpc_rll_coma_workspace_floats(to_int(T, "T"), to_int(B, "B"), to_int(A, "A"));
        TORCH_CHECK(nws >= 0, "coma: the workspace size of (T,B,A) = (", T, ",", B, ",", A, ") is not representable");
        Tensor ws = new_f32({nws}, dev);
        const float s_pe = loss_scale(scale_pe, T * B * A), s_q = loss_scale(scale_q, (T - 1) * B * A);
        check(hpc_rll_coma_forward(fptr(logit), iptr(action), fptr(q), fptr(target_q), fptr(reward), fptr(weight),
                                   dm.ptr, dm.code, fmut(losses), fmut(ws), (int)T, (int)B, (int)A,
                                   to_int(N, "N"), (float)gamma, (float)lambda, s_pe, s_q, stream_of(dev)),
              "hpc_rll_coma_forward");
        ctx->save_for_backward({logit, action, has(weight) ? *weight : undef(), ws});
        ctx->saved_data["scale_pe"] = (double)s_pe;
        return split1(losses, 3);
    }
    static ag::tensor_list backward(ag::AutogradContext* ctx, ag::tensor_list grads) {
        ag::tensor_list out(11);
        const bool need_l = ctx->needs_input_grad(0), need_q = ctx->needs_input_grad(2);
        if (!(need_l || need_q)) return out;
        const auto saved = ctx->get_saved_variables();
        const Tensor &logit = saved[0], &action = saved[1], &weight = saved[2], &ws = saved[3];
        const at::Device dev = logit.device();
        c10::DeviceGuard g(dev);
        const int64_t T = logit.size(0), B = logit.size(1), A = logit.size(2), N = logit.size(3);
        Tensor g_p = grad1(grads[0], dev, "grad_policy_loss"), g_q = grad1(grads[1], dev, "grad_q_value_loss"),
               g_e = grad1(grads[2], dev, "grad_entropy_loss");
        Tensor grad_logit = need_l ? at::empty_like(logit) : undef();
        Tensor grad_q = need_q ? at::empty_like(logit) : undef();
        check(hpc_rll_coma_backward(fptr(g_p), fptr(g_q), fptr(g_e), fptr(logit), iptr(action), fptr(weight), fptr(ws),
                                    fmut(grad_logit), fmut(grad_q), (int)T, (int)B, (int)A, (int)N,
                                    (float)ctx->saved_data["scale_pe"].toDouble(), stream_of(dev)),
              "hpc_rll_coma_backward");
        out[0] = grad_logit;
        out[2] = grad_q;
        return out;
    }
};

// ========================================================================================================== R2D2
// The R2D2 sequence loss (hpc_rll_r2d2_*): the n-step (double-)Q TD error of every step of a (T,B,N) unroll, its loss and the
// replay priority.  Shapes and dtypes are checked before the device so that a wrong argument is named even on host tensors.
// The gradient flows to q only; saves action and the workspace (delta).
struct R2d2Fn : public ag::Function<R2d2Fn> {
    static ag::tensor_list forward(ag::AutogradContext* ctx, const Tensor& q, const Tensor& target_q, const Tensor& action,
                                   const Tensor& reward, const OptTensor& done, const OptTensor& weight, double gamma,
                                   int64_t nstep, int64_t burnin, bool value_rescale, bool double_q, double priority_eta,
                                   std::optional<double> scale) {
        TORCH_CHECK(q.defined(), "q: expected a tensor, got None");
        TORCH_CHECK(q.dim() == 3, "q: expected (T,B,N), got ", q.sizes());
        const int64_t T = q.size(0), B = q.size(1), N = q.size(2);
        Args args;
        args.add(q, "q", {T, B, N});
        args.add(target_q, "target_q", {T, B, N});
        args.add(action, "action", {T, B}, at::kLong);
        args.add(reward, "reward", {T, B});
        const Args::Mask dm = args.add_mask(done, "done", reward.sizes(), " (the shape of reward)");
        const int wm = masked_td_weight_mode(weight, T, B);   // (B,) or (T,B): its own dtype and shape messages
        TORCH_CHECK(nstep >= 1, "r2d2_td: nstep = ", nstep, ", expected nstep >= 1");
        TORCH_CHECK(burnin >= 0, "r2d2_td: burnin = ", burnin, ", expected burnin >= 0");
        retrace_check_n("r2d2_td", N);
        const at::Device dev = args.on_device_of(q);
        if (has(weight)) req(*weight, "weight", dev);
        c10::DeviceGuard g(dev);
        const int64_t L = std::max<int64_t>(T - std::min(nstep, T) - std::min(burnin, T), 0);
        const bool empty = B == 0 || L == 0;
        Tensor loss = new_f32({1}, dev);
        // no valid step: the loss is zero and nothing is launched; the outputs are then zeros
        Tensor td = new_f32({L, B}, dev);
        Tensor priority = empty ? at::zeros({B}, q.options()) : new_f32({B}, dev);
        Tensor ws = new_f32({empty ? 0 : hpc_rll_r2d2_workspace_floats(to_int(T, "T"), to_int(B, "B"))}, dev);
        const int n = empty ? 1 : to_int(nstep, "nstep"), bi = empty ? (int)T : to_int(burnin, "burnin");
        check(hpc_rll_r2d2_forward(fptr(q), fptr(target_q), iptr(action), fptr(reward), dm.ptr, dm.code, fptr(weight), wm,
                                   fmut(loss), fmut(td), fmut(priority), fmut(ws), to_int(T, "T"),
                                   to_int(B, "B"), to_int(N, "N"), n, bi, (float)gamma, value_rescale ? 1 : 0,
                                   double_q ? 1 : 0, (float)priority_eta, loss_scale(scale, L * B), stream_of(dev)),
              "hpc_rll_r2d2_forward");
        ctx->save_for_backward({action, ws});
        ctx->saved_data["N"] = N;
        ctx->saved_data["nstep"] = (int64_t)n;
        ctx->saved_data["burnin"] = (int64_t)bi;
        ctx->saved_data["empty"] = empty;
        ctx->mark_non_differentiable({td, priority});
        return {loss, td, priority};
    }
    static ag::tensor_list backward(ag::AutogradContext* ctx, ag::tensor_list grads) {
        ag::tensor_list out(13);
        if (!ctx->needs_input_grad(0)) return out;
        const auto saved = ctx->get_saved_variables();
        const Tensor &action = saved[0], &ws = saved[1];
        const at::Device dev = action.device();
        c10::DeviceGuard g(dev);
        const int64_t T = action.size(0), B = action.size(1), N = ctx->saved_data["N"].toInt();
        Tensor gl = grad1(grads[0], dev, "grad_loss");
        if (ctx->saved_data["empty"].toBool()) {
            out[0] = at::zeros({T, B, N}, gl.options());
            return out;
        }
        Tensor grad_q = new_f32({T, B, N}, dev);
        check(hpc_rll_r2d2_backward(fptr(gl), iptr(action), fptr(ws), fmut(grad_q), (int)T, (int)B, (int)N,
                                    (int)ctx->saved_data["nstep"].toInt(), (int)ctx->saved_data["burnin"].toInt(),
                                    stream_of(dev)),
              "hpc_rll_r2d2_backward");
        out[0] = grad_q;
        return out;
    }
};

// ========================================================================================================== SAC
// Soft Actor-Critic for discrete actions (hpc_rll_sac_discrete_*; DI-engine's DiscreteSACPolicy._forward_learn).  logit and its
// five siblings are (..., N), the per-sample tensors have the leading shape.  Shapes and dtypes are checked before the device
// so that a wrong argument is named even on host tensors.  The gradient flows to logit, q1 and q2; each is formed only when
// its input needs it.  Saves the unit gradient of logit (allocated only when it is wanted), action and the workspace.
struct SacDiscreteFn : public ag::Function<SacDiscreteFn> {
    static ag::tensor_list forward(ag::AutogradContext* ctx, const Tensor& logit, const Tensor& next_logit, const Tensor& q1,
                                   const OptTensor& q2, const Tensor& target_q1, const OptTensor& target_q2,
                                   const Tensor& action, const Tensor& reward, const OptTensor& done, const OptTensor& weight,
                                   double alpha, const OptTensor& alpha_t, double gamma, std::optional<double> scale,
                                   bool want_grad) {
        TORCH_CHECK(logit.defined(), "logit: expected a tensor, got None");
        TORCH_CHECK(logit.dim() >= 1, "logit: expected (..., N), got ", logit.sizes());
        TORCH_CHECK(has(q2) == has(target_q2), "sac_discrete: q2 and target_q2 are both given or both None (got ",
                    has(q2) ? "q2" : "target_q2", " alone)");
        const at::IntArrayRef full = logit.sizes(), lead = full.slice(0, full.size() - 1);
        const int64_t N = full.back();
        Args args;
        args.add(logit, "logit", full);
        args.add(next_logit, "next_logit", full);
        args.add(q1, "q1", full);
        args.add(q2, "q2", full);
        args.add(target_q1, "target_q1", full);
        args.add(target_q2, "target_q2", full);
        args.add(action, "action", lead, at::kLong);
        args.add(reward, "reward", lead);
        const Args::Mask dm = args.add_mask(done, "done", lead);
        args.add(weight, "weight", lead);
        if (has(alpha_t)) {   // one element of any shape: its own messages
            TORCH_CHECK(alpha_t->scalar_type() == at::kFloat, "alpha: dtype ", alpha_t->scalar_type(), ", expected ", at::kFloat);
            TORCH_CHECK(alpha_t->numel() == 1, "alpha: expected a float or a 1-element tensor, got shape ", alpha_t->sizes());
        }
        retrace_check_n("sac_discrete", N);
        const at::Device dev = args.on_device_of(logit);
        if (has(alpha_t)) req(*alpha_t, "alpha", dev);
        c10::DeviceGuard g(dev);
        const int64_t rows = action.numel();
        Tensor out4 = new_f32({4}, dev);
        Tensor td = new_f32(lead, dev), tq = new_f32(lead, dev);
        Tensor unit = (want_grad && rows > 0) ? new_f32(full, dev) : undef();
        Tensor ws = new_f32({rows > 0 ? hpc_rll_sac_discrete_workspace_floats(rows) : 0}, dev);
        check(hpc_rll_sac_discrete_forward(fptr(logit), fptr(next_logit), fptr(q1), fptr(q2), fptr(target_q1), fptr(target_q2),
                                           iptr(action), fptr(reward), dm.ptr, dm.code, fptr(weight),
                                           fptr(alpha_t), (float)alpha, fmut(out4), fmut(td), fmut(tq), fmut(unit), fmut(ws),
                                           rows, to_int(N, "N"), (float)gamma, loss_scale(scale, rows), stream_of(dev)),
              "hpc_rll_sac_discrete_forward");
        ctx->save_for_backward({unit, action, ws});
        ctx->saved_data["N"] = N;
        Tensor policy = alias_of(out4, 0, 1), critic = alias_of(out4, 1, 1), twin = alias_of(out4, 2, 1),
               ent = alias_of(out4, 3, 1);
        ctx->mark_non_differentiable({ent, td, tq});
        return {policy, critic, twin, ent, td, tq};
    }
    static ag::tensor_list backward(ag::AutogradContext* ctx, ag::tensor_list grads) {
        ag::tensor_list out(15);
        const bool need_l = ctx->needs_input_grad(0), need_1 = ctx->needs_input_grad(2), need_2 = ctx->needs_input_grad(3);
        if (!(need_l || need_1 || need_2)) return out;
        const auto saved = ctx->get_saved_variables();
        const Tensor &unit = saved[0], &action = saved[1], &ws = saved[2];
        const at::Device dev = action.device();
        c10::DeviceGuard g(dev);
        const int64_t N = ctx->saved_data["N"].toInt(), rows = action.numel();
        std::vector<int64_t> full(action.sizes().begin(), action.sizes().end());
        full.push_back(N);
        TORCH_CHECK(!need_l || rows == 0 || unit.defined(), "sac_discrete: the logit gradient was not stored by the forward");
        Tensor g_p = grad1(grads[0], dev, "grad_policy_loss"), g_1 = grad1(grads[1], dev, "grad_critic_loss"),
               g_2 = grad1(grads[2], dev, "grad_twin_critic_loss");
        Tensor grad_l = need_l ? new_f32(full, dev) : undef();
        Tensor grad_1 = need_1 ? new_f32(full, dev) : undef();
        Tensor grad_2 = need_2 ? new_f32(full, dev) : undef();
        check(hpc_rll_sac_discrete_backward(fptr(g_p), fptr(g_1), fptr(g_2), fptr(unit), iptr(action), fptr(ws), fmut(grad_l),
                                            fmut(grad_1), fmut(grad_2), rows, (int)N, stream_of(dev)),
              "hpc_rll_sac_discrete_backward");
        out[0] = grad_l;
        out[2] = grad_1;
        out[3] = grad_2;
        return out;
    }
};

// ========================================================================================================== GRPO
// The language-model policy losses (hpc_rll_token_logp_*, hpc_rll_grpo_*): logits may be fp32 or bf16.  Shapes and dtypes are
// checked before the device so that a wrong argument is named even on host tensors.
at::ScalarType logits_dtype(const Tensor& t, const char* name) {
    TORCH_CHECK(t.defined(), name, ": expected a tensor, got None");
    const at::ScalarType st = t.scalar_type();
    TORCH_CHECK(st == at::kFloat || st == at::kBFloat16, name, ": dtype ", st, ", expected ", at::kFloat, " or ", at::kBFloat16);
    return st;
}
int elem_code(at::ScalarType st) { return st == at::kBFloat16 ? HPC_RLL_ELEM_BF16 : HPC_RLL_ELEM_F32; }
void grpo_check_v(const char* op, int64_t V) {
    TORCH_CHECK(V <= 262144, op, ": V = ", V, " is not supported (1 <= V <= 262144)");
}

// logp = logits[..., a] - logsumexp(logits); saves the logits, action and lse (4 bytes per token)
struct TokenLogpFn : public ag::Function<TokenLogpFn> {
    static Tensor forward(ag::AutogradContext* ctx, const Tensor& logits, const Tensor& action) {
        const at::ScalarType st = logits_dtype(logits, "logits");
        TORCH_CHECK(logits.dim() >= 1, "logits: expected (..., V), got ", logits.sizes());
        const int64_t V = logits.size(-1);
        Args args;
        args.add(logits, "logits", logits.sizes(), st);
        args.add(action, "action", logits.sizes().slice(0, logits.dim() - 1), at::kLong);
        grpo_check_v("token_log_prob", V);
        const at::Device dev = args.on_device_of(logits);
        c10::DeviceGuard g(dev);
        const int64_t rows = action.numel();
        Tensor logp = new_f32(action.sizes(), dev), lse = new_f32({rows}, dev);
        check(hpc_rll_token_logp_forward(vptr(logits), elem_code(st), iptr(action), nullptr, fmut(logp), fmut(lse), rows,
                                         to_int(V, "V"), stream_of(dev)),
              "hpc_rll_token_logp_forward");
        ctx->save_for_backward({logits, action, lse});
        return logp;
    }
    static ag::tensor_list backward(ag::AutogradContext* ctx, ag::tensor_list grads) {
        ag::tensor_list out(2);
        if (!ctx->needs_input_grad(0)) return out;
        const auto saved = ctx->get_saved_variables();
        const Tensor &logits = saved[0], &action = saved[1], &lse = saved[2];
        const at::Device dev = logits.device();
        c10::DeviceGuard g(dev);
        Tensor gl = grads[0].contiguous();
        req(gl, "grad_logp", dev);
        Tensor grad = at::empty(logits.sizes(), logits.options());
        check(hpc_rll_token_logp_backward(fptr(gl), vptr(logits), elem_code(logits.scalar_type()), iptr(action), fptr(lse),
                                          grad.data_ptr(), action.numel(), (int)logits.size(-1), stream_of(dev)),
              "hpc_rll_token_logp_backward");
        out[0] = grad;
        return out;
    }
};

// (loss, mean_kl, mean_ratio, mean_clipped), (1,) each; the gradient flows to logit_new only.  Saves logit_new, action and the
// workspace (lse and coef are what the backward reads).
struct GrpoFn : public ag::Function<GrpoFn> {
    // logits (B,S,V) of either element type, or log-probs (B,S) fp32: the number of dimensions decides
    static int kind_of(Args& args, const Tensor& t, const char* name, int64_t B, int64_t S, int64_t V) {
        TORCH_CHECK(t.defined(), name, ": expected a tensor, got None");
        TORCH_CHECK(t.dim() == 2 || t.dim() == 3, name, ": expected logits (B,S,V) or log-probs (B,S), got ", t.sizes());
        if (t.dim() == 2) {
            args.add(t, name, {B, S});
            return HPC_RLL_GRPO_LOGP;
        }
        const at::ScalarType st = logits_dtype(t, name);
        args.add(t, name, {B, S, V}, st);
        return elem_code(st);
    }
    static ag::tensor_list forward(ag::AutogradContext* ctx, const Tensor& logit_new, const Tensor& old, const OptTensor& ref,
                                   const Tensor& action, const Tensor& adv, const OptTensor& weight, double clip_ratio,
                                   double beta, std::optional<double> scale) {
        const at::ScalarType st = logits_dtype(logit_new, "logit_new");
        TORCH_CHECK(logit_new.dim() == 3, "logit_new: expected (B,S,V), got ", logit_new.sizes());
        const int64_t B = logit_new.size(0), S = logit_new.size(1), V = logit_new.size(2);
        Args args;
        args.add(logit_new, "logit_new", {B, S, V}, st);
        const int old_kind = kind_of(args, old, "old", B, S, V);
        const int ref_kind = has(ref) ? kind_of(args, *ref, "ref", B, S, V) : HPC_RLL_GRPO_LOGP;
        args.add(action, "action", {B, S}, at::kLong);
        args.add(adv, "adv", {B});
        args.add(weight, "weight", {B, S});
        grpo_check_v("grpo_policy_loss", V);
        const at::Device dev = args.on_device_of(logit_new);
        c10::DeviceGuard g(dev);
        const bool empty = B == 0 || S == 0 || V == 0;
        Tensor out4 = new_f32({4}, dev);
        Tensor ws = new_f32({empty ? 0 : hpc_rll_grpo_workspace_floats(to_int(B, "B"), to_int(S, "S"))}, dev);
        const float sc = scale.has_value() && *scale > 0.0 ? (float)*scale : 0.f;   // 0: the kernels take 1/B
        check(hpc_rll_grpo_forward(vptr(logit_new), elem_code(st), vptr(old), old_kind, has(ref) ? vptr(*ref) : nullptr,
                                   ref_kind, iptr(action), fptr(adv), fptr(weight), fmut(out4), fmut(ws), to_int(B, "B"),
                                   to_int(S, "S"), to_int(V, "V"), (float)clip_ratio, (float)beta, sc, stream_of(dev)),
              "hpc_rll_grpo_forward");
        ctx->save_for_backward({logit_new, action, ws});
        ctx->saved_data["empty"] = empty;
        ag::tensor_list out = split1(out4, 4);
        ctx->mark_non_differentiable({out[1], out[2], out[3]});
        return out;
    }
    static ag::tensor_list backward(ag::AutogradContext* ctx, ag::tensor_list grads) {
        ag::tensor_list out(9);
        if (!ctx->needs_input_grad(0)) return out;
        const auto saved = ctx->get_saved_variables();
        const Tensor &logit_new = saved[0], &action = saved[1], &ws = saved[2];
        const at::Device dev = logit_new.device();
        c10::DeviceGuard g(dev);
        if (ctx->saved_data["empty"].toBool()) {
            out[0] = at::zeros(logit_new.sizes(), logit_new.options());
            return out;
        }
        Tensor gl = grad1(grads[0], dev, "grad_loss");
        Tensor grad = at::empty(logit_new.sizes(), logit_new.options());
        check(hpc_rll_grpo_backward(fptr(gl), vptr(logit_new), elem_code(logit_new.scalar_type()), iptr(action), fptr(ws),
                                    grad.data_ptr(), (int)logit_new.size(0), (int)logit_new.size(1), (int)logit_new.size(2),
                                    stream_of(dev)),
              "hpc_rll_grpo_backward");
        out[0] = grad;
        return out;
    }
};

// ======================================================================================================== LM PPO
// Token-level PPO for language models (hpc_rll_lm_*): the head with entropy, GAE over (B,S), the token loss.
// (logp, entropy) per token; saves the logits, action, weight, lse and the entropy (8 bytes per token)
struct TokenLpeFn : public ag::Function<TokenLpeFn> {
    static ag::tensor_list forward(ag::AutogradContext* ctx, const Tensor& logits, const Tensor& action,
                                   const OptTensor& weight) {
        const at::ScalarType st = logits_dtype(logits, "logits");
        TORCH_CHECK(logits.dim() >= 1, "logits: expected (..., V), got ", logits.sizes());
        const int64_t V = logits.size(-1);
        const at::IntArrayRef lead = logits.sizes().slice(0, logits.dim() - 1);
        Args args;
        args.add(logits, "logits", logits.sizes(), st);
        args.add(action, "action", lead, at::kLong);
        args.add(weight, "weight", lead);
        grpo_check_v("token_log_prob_entropy", V);
        const at::Device dev = args.on_device_of(logits);
        c10::DeviceGuard g(dev);
        const int64_t rows = action.numel();
        Tensor logp = new_f32(action.sizes(), dev), ent = new_f32(action.sizes(), dev), lse = new_f32({rows}, dev);
        check(hpc_rll_lm_head_forward(vptr(logits), elem_code(st), iptr(action), fptr(weight), fmut(logp), fmut(lse), fmut(ent),
                                      rows, to_int(V, "V"), stream_of(dev)),
              "hpc_rll_lm_head_forward");
        ctx->save_for_backward({logits, action, has(weight) ? *weight : undef(), lse, ent});
        return {logp, ent};
    }
    static ag::tensor_list backward(ag::AutogradContext* ctx, ag::tensor_list grads) {
        ag::tensor_list out(3);
        if (!ctx->needs_input_grad(0)) return out;
        const auto saved = ctx->get_saved_variables();
        const Tensor &logits = saved[0], &action = saved[1], &weight = saved[2], &lse = saved[3], &ent = saved[4];
        const at::Device dev = logits.device();
        c10::DeviceGuard g(dev);
        Tensor g_lp = grads[0].defined() ? grads[0].contiguous() : undef();
        Tensor g_h = grads[1].defined() ? grads[1].contiguous() : undef();
        if (g_lp.defined()) req(g_lp, "grad_logp", dev);
        if (g_h.defined()) req(g_h, "grad_entropy", dev);
        Tensor grad = at::empty(logits.sizes(), logits.options());
        check(hpc_rll_lm_head_backward(fptr(g_lp), fptr(g_h), vptr(logits), elem_code(logits.scalar_type()), iptr(action),
                                       fptr(weight), fptr(lse), fptr(ent), grad.data_ptr(), action.numel(),
                                       (int)logits.size(-1), stream_of(dev)),
              "hpc_rll_lm_head_backward");
        out[0] = grad;
        return out;
    }
};

// (adv, ret) over (B,S); no gradient
std::tuple<Tensor, Tensor> lm_gae(const Tensor& value, const OptTensor& weight, const Tensor& reward, const OptTensor& kl,
                                  double beta, double gamma, double lam, bool whiten) {
    TORCH_CHECK(value.defined(), "value: expected a tensor, got None");
    TORCH_CHECK(value.dim() == 2, "value: expected (B,S), got ", value.sizes());
    const int64_t B = value.size(0), S = value.size(1);
    Args args;
    args.add(value, "value", {B, S});
    args.add(weight, "weight", {B, S});
    TORCH_CHECK(reward.defined(), "reward: expected a tensor, got None");
    TORCH_CHECK(reward.dim() == 1 || reward.dim() == 2, "reward: expected per-token (B,S) or per-sequence (B,), got ",
                reward.sizes());
    const bool per_seq = reward.dim() == 1;
    if (per_seq) args.add(reward, "reward", {B});
    else args.add(reward, "reward", {B, S});
    args.add(kl, "kl", {B, S});
    const at::Device dev = args.on_device_of(value);
    c10::DeviceGuard g(dev);
    Tensor adv = new_f32({B, S}, dev), ret = new_f32({B, S}, dev);
    const bool empty = B == 0 || S == 0;
    Tensor ws = new_f32({empty ? 0 : hpc_rll_lm_gae_workspace_floats()}, dev);
    check(hpc_rll_lm_gae(fptr(value), fptr(weight), fptr(reward), per_seq ? 1 : 0, fptr(kl), fmut(adv), fmut(ret), fmut(ws),
                         to_int(B, "B"), to_int(S, "S"), (float)beta, (float)gamma, (float)lam, whiten ? 1 : 0, stream_of(dev)),
          "hpc_rll_lm_gae");
    return {adv, ret};
}

// (policy_loss, value_loss, entropy, approx_kl, mean_ratio, clipfrac, den), (1,) each; the first three are differentiable, the
// gradient flows to logit_new and value_new.  Saves logit_new, action, weight and the workspace.
struct LmPpoFn : public ag::Function<LmPpoFn> {
    static ag::tensor_list forward(ag::AutogradContext* ctx, const Tensor& logit_new, const Tensor& old_logp,
                                   const Tensor& action, const Tensor& adv, const OptTensor& weight, const OptTensor& value_new,
                                   const OptTensor& value_old, const OptTensor& ret, double clip_ratio,
                                   std::optional<double> dual_clip, std::optional<double> value_clip, bool seq_mean, bool raw,
                                   std::optional<double> scale) {
        const at::ScalarType st = logits_dtype(logit_new, "logit_new");
        TORCH_CHECK(logit_new.dim() == 3, "logit_new: expected (B,S,V), got ", logit_new.sizes());
        const int64_t B = logit_new.size(0), S = logit_new.size(1), V = logit_new.size(2);
        Args args;
        args.add(logit_new, "logit_new", {B, S, V}, st);
        args.add(old_logp, "old_logp", {B, S});
        args.add(action, "action", {B, S}, at::kLong);
        args.add(adv, "adv", {B, S});
        args.add(weight, "weight", {B, S});
        const int nval = (int)has(value_new) + (int)has(value_old) + (int)has(ret);
        TORCH_CHECK(nval == 0 || nval == 3, "lm_ppo_loss: value_new, value_old and ret are given all three or none (got ", nval,
                    " of them)");
        args.add(value_new, "value_new", {B, S});
        args.add(value_old, "value_old", {B, S});
        args.add(ret, "ret", {B, S});
        TORCH_CHECK(!dual_clip.has_value() || *dual_clip > 1.0, "dual_clip: expected None or a value above 1, got ", *dual_clip);
        grpo_check_v("lm_ppo_loss", V);
        const at::Device dev = args.on_device_of(logit_new);
        c10::DeviceGuard g(dev);
        const bool empty = B == 0 || S == 0 || V == 0;
        Tensor out8 = new_f32({8}, dev);
        Tensor ws = new_f32({empty ? 0 : hpc_rll_lm_ppo_workspace_floats(to_int(B, "B"), to_int(S, "S"))}, dev);
        const float sc = scale.has_value() && *scale > 0.0 ? (float)*scale : 0.f;   // 0: the kernels take 1/B
        check(hpc_rll_lm_ppo_forward(vptr(logit_new), elem_code(st), fptr(old_logp), iptr(action), fptr(adv), fptr(weight),
                                     fptr(value_new), fptr(value_old), fptr(ret), fmut(out8), fmut(ws), to_int(B, "B"),
                                     to_int(S, "S"), to_int(V, "V"), (float)clip_ratio, dual_clip.has_value() ? (float)*dual_clip : 0.f,
                                     value_clip.has_value() ? 1 : 0, value_clip.has_value() ? (float)*value_clip : 0.f,
                                     seq_mean ? 1 : 0, raw ? 1 : 0, sc, stream_of(dev)),
              "hpc_rll_lm_ppo_forward");
        ctx->save_for_backward({logit_new, action, has(weight) ? *weight : undef(), ws});
        ctx->saved_data["empty"] = empty;
        ctx->saved_data["has_value"] = nval == 3;
        ctx->saved_data["use_den"] = !seq_mean && !raw;
        // needs_input_grad counts the tensor inputs that are present: value_new follows the four required ones and weight
        ctx->saved_data["value_edge"] = (int64_t)(has(weight) ? 5 : 4);
        ag::tensor_list out = split1(out8, 7);
        ctx->mark_non_differentiable({out[3], out[4], out[5], out[6]});
        return out;
    }
    static ag::tensor_list backward(ag::AutogradContext* ctx, ag::tensor_list grads) {
        ag::tensor_list out(14);
        const auto saved = ctx->get_saved_variables();
        const Tensor &logit_new = saved[0], &action = saved[1], &weight = saved[2], &ws = saved[3];
        const bool need_l = ctx->needs_input_grad(0);
        const bool need_v = ctx->saved_data["has_value"].toBool() && ctx->needs_input_grad((size_t)ctx->saved_data["value_edge"].toInt());
        if (!(need_l || need_v)) return out;
        const at::Device dev = logit_new.device();
        c10::DeviceGuard g(dev);
        if (ctx->saved_data["empty"].toBool()) {
            if (need_l) out[0] = at::zeros(logit_new.sizes(), logit_new.options());
            if (need_v) out[5] = at::zeros(action.sizes(), logit_new.options().dtype(at::kFloat));
            return out;
        }
        // an output that did not enter the caller's loss arrives undefined: the kernels take NULL for a zero gradient
        Tensor g_p = grads[0].defined() ? grad1(grads[0], dev, "grad_policy_loss") : undef();
        Tensor g_v = grads[1].defined() ? grad1(grads[1], dev, "grad_value_loss") : undef();
        Tensor g_e = grads[2].defined() ? grad1(grads[2], dev, "grad_entropy") : undef();
        Tensor grad_l = need_l ? at::empty(logit_new.sizes(), logit_new.options()) : undef();
        Tensor grad_v = need_v ? new_f32(action.sizes(), dev) : undef();
        check(hpc_rll_lm_ppo_backward(fptr(g_p), fptr(g_e), fptr(g_v), vptr(logit_new), elem_code(logit_new.scalar_type()),
                                      iptr(action), fptr(weight), fptr(ws), grad_l.defined() ? grad_l.data_ptr() : nullptr,
                                      fmut(grad_v), (int)logit_new.size(0), (int)logit_new.size(1), (int)logit_new.size(2),
                                      ctx->saved_data["use_den"].toBool() ? 1 : 0, stream_of(dev)),
              "hpc_rll_lm_ppo_backward");
        out[0] = grad_l;
        out[5] = grad_v;
        return out;
    }
};

// ==================================================================================================== q n-step TD
// What the five one-hot n-step TD ops (q, C51, IQN, QR-DQN, FQF) share.  They check the device first, one req() per tensor.
// The per-sample arguments that follow an op's leading tensors: action, next_n_action (B,) int64, reward (nstep,B), done (B,);
// returns nstep.  (weight and value_gamma stay with the op: IQN and FQF check a tensor of their own before them.)
int64_t nstep_sample_check(const Tensor& action, const Tensor& naction, const Tensor& reward, const Tensor& done, int64_t B,
                           const at::Device& dev) {
    req(action, "action", dev, {B}, at::kLong);
    req(naction, "next_n_action", dev, {B}, at::kLong);
    req(reward, "reward", dev);
    TORCH_CHECK(reward.dim() == 2 && reward.size(1) == B, "reward: expected (nstep,", B, "), got ", reward.sizes());
    req(done, "done", dev, {B});
    return reward.size(0);
}
// loss (1,) and td_err (B,) of a list-form forward in the order of its list, then the buffer of the unit gradient, which may
// be larger than the `need` floats that are written.
void td_list_outputs(const Tensor& first, const Tensor& second, bool loss_first, const Tensor& buf, const char* buf_name,
                     int64_t need, const char* need_name, int64_t B, const at::Device& dev) {
    req(first, loss_first ? "loss" : "td_err", dev, {loss_first ? 1 : B});
    req(second, loss_first ? "td_err" : "loss", dev, {loss_first ? B : 1});
    req(buf, buf_name, dev);
    TORCH_CHECK(buf.numel() >= need, buf_name, ": ", buf.numel(), " floats, need at least ", need_name, " = ", need);
}
// The backward of all five: the forward saved {unit gradient, action} and N; the gradient flows to the first of the
// `n_inputs` arguments only.  `shape(unit, N)` is that gradient's, `launch(grad_loss, unit, action, grad)` fills it.
template <class Shape, class Launch>
ag::tensor_list onehot_td_backward(ag::AutogradContext* ctx, const ag::tensor_list& grads, size_t n_inputs, Shape shape,
                                   Launch launch) {
    ag::tensor_list out(n_inputs);
    if (!ctx->needs_input_grad(0)) return out;
    const auto saved = ctx->get_saved_variables();
    const Tensor &unit = saved[0], &action = saved[1];
    const at::Device dev = unit.device();
    c10::DeviceGuard g(dev);
    out[0] = new_f32(shape(unit, ctx->saved_data["N"].toInt()), dev);
    launch(grad1(grads[0], dev, "grad_loss"), unit, action, out[0]);
    return out;
}
at::DimVector shape_bnx(const Tensor& unit, int64_t N) { return {unit.size(0), N, unit.size(1)}; }   // unit (B,X): gradient (B,N,X)

struct QDims { int64_t B, N, nstep; at::Device dev; };
QDims q_check(const Tensor& q, const Tensor& nq, const Tensor& action, const Tensor& naction, const Tensor& reward,
              const Tensor& done, const OptTensor& weight) {
    req(q, "q");
    TORCH_CHECK(q.dim() == 2, "q: expected (B,N), got ", q.sizes());
    const int64_t B = q.size(0), N = q.size(1);
    const at::Device dev = q.device();
    req(nq, "next_n_q", dev, {B, N});
    const int64_t nstep = nstep_sample_check(action, naction, reward, done, B, dev);
    req_opt(weight, "weight", dev, {B});
    return {B, N, nstep, dev};
}
void q_forward_launch(const QDims& d, const Tensor& q, const Tensor& nq, const Tensor& action, const Tensor& naction,
                      const Tensor& reward, const Tensor& done, const OptTensor& weight, const Tensor& td_err,
                      const Tensor& loss, const Tensor& grad_buf, double gamma, int rescale, std::optional<double> scale) {
    Tensor partials = new_f32({hpc_rll_partials_floats(d.B)}, d.dev);
    check(hpc_rll_q_nstep_td_forward(fptr(q), fptr(nq), iptr(action), iptr(naction), fptr(reward), fptr(done),
                                     fptr(weight), fmut(loss), fmut(td_err), fmut(grad_buf), fmut(partials),
                                     to_int(d.nstep, "nstep"), to_int(d.B, "B"), to_int(d.N, "N"), (float)gamma, rescale,
                                     loss_scale(scale, d.B), stream_of(d.dev)),
          "hpc_rll_q_nstep_td_forward");
}

// inputs = [q, next_n_q (B,N), action, next_n_action (B,) int64, reward (nstep,B), done (B,), weight (B,)|None];
// outputs = [td_err (B,), loss (1,), grad_buf (B,)].  Reference: src/rl_utils/q_nstep_td.cu:8-39,
// q_nstep_td_rescale.cu:8-39.
void q_forward_l2(const OptList& in, const TensorList& out, double gamma, int rescale, std::optional<double> scale) {
    expect_len(in, 7, "QNStepTdForward inputs");
    expect_len(out, 3, "QNStepTdForward outputs");
    for (int i = 0; i < 6; ++i) TORCH_CHECK(has(in[i]), "QNStepTdForward: inputs[", i, "] is None");
    const QDims d = q_check(*in[0], *in[1], *in[2], *in[3], *in[4], *in[5], in[6]);
    req(out[0], "td_err", d.dev, {d.B});
    req(out[1], "loss", d.dev, {1});
    req(out[2], "grad_buf", d.dev, {d.B});
    c10::DeviceGuard g(d.dev);
    q_forward_launch(d, *in[0], *in[1], *in[2], *in[3], *in[4], *in[5], in[6], out[0], out[1], out[2], gamma, rescale,
                     scale);
}
void q_backward_launch(const Tensor& gl, const Tensor& grad_buf, const Tensor& action, const Tensor& grad_q) {
    check(hpc_rll_q_nstep_td_backward(fptr(gl), fptr(grad_buf), iptr(action), fmut(grad_q), (int)grad_q.size(0),
                                      (int)grad_q.size(1), stream_of(grad_q.device())),
          "hpc_rll_q_nstep_td_backward");
}
// inputs = [grad_loss, grad_buf (B,), action]; outputs = [grad_q (B,N)].  q_nstep_td.cu:41-63.
void q_backward_l2(const TensorList& in, const TensorList& out) {
    expect_len(in, 3, "QNStepTdBackward inputs");
    expect_len(out, 1, "QNStepTdBackward outputs");
    const Tensor& gq = req(out[0], "grad_q");
    TORCH_CHECK(gq.dim() == 2, "grad_q: expected (B,N), got ", gq.sizes());
    const at::Device dev = gq.device();
    req(in[1], "grad_buf", dev, {gq.size(0)});
    req(in[2], "action", dev, {gq.size(0)}, at::kLong);
    c10::DeviceGuard g(dev);
    q_backward_launch(grad1(in[0], dev, "grad_loss"), in[1], in[2], gq);
}

template <int RESCALE> struct QNStepFn : public ag::Function<QNStepFn<RESCALE>> {
    static ag::tensor_list forward(ag::AutogradContext* ctx, const Tensor& q, const Tensor& nq, const Tensor& action,
                                   const Tensor& naction, const Tensor& reward, const Tensor& done,
                                   const OptTensor& weight, double gamma, std::optional<double> scale) {
        const QDims d = q_check(q, nq, action, naction, reward, done, weight);
        c10::DeviceGuard g(d.dev);
        Tensor td_err = new_f32({d.B}, d.dev), loss = new_f32({1}, d.dev), grad_buf = new_f32({d.B}, d.dev);
        q_forward_launch(d, q, nq, action, naction, reward, done, weight, td_err, loss, grad_buf, gamma, RESCALE, scale);
        ctx->save_for_backward({grad_buf, action});
        ctx->saved_data["N"] = d.N;
        ctx->mark_non_differentiable({td_err});
        return {loss, td_err};
    }
    static ag::tensor_list backward(ag::AutogradContext* ctx, ag::tensor_list grads) {
        return onehot_td_backward(ctx, grads, 9, [](const Tensor& gb, int64_t N) { return at::DimVector{gb.size(0), N}; },
                                  q_backward_launch);
    }
};

// ===================================================================================================== dist (C51)
struct DistDims { int64_t B, N, A, nstep; at::Device dev; };
DistDims dist_check(const Tensor& dist, const Tensor& ndist, const Tensor& action, const Tensor& naction,
                    const Tensor& reward, const Tensor& done, const OptTensor& weight) {
    req(dist, "dist");
    TORCH_CHECK(dist.dim() == 3, "dist: expected (B,N,n_atom), got ", dist.sizes());
    const int64_t B = dist.size(0), N = dist.size(1), A = dist.size(2);
    const at::Device dev = dist.device();
    req(ndist, "next_n_dist", dev, {B, N, A});
    const int64_t nstep = nstep_sample_check(action, naction, reward, done, B, dev);
    req_opt(weight, "weight", dev, {B});
    return {B, N, A, nstep, dev};
}
void dist_forward_launch(const DistDims& d, const Tensor& dist, const Tensor& ndist, const Tensor& action,
                         const Tensor& naction, const Tensor& reward, const Tensor& done, const OptTensor& weight,
                         const Tensor& td_err, const Tensor& loss, const Tensor& buf, double gamma, double v_min,
                         double v_max, std::optional<double> scale) {
    Tensor partials = new_f32({hpc_rll_partials_floats(d.B)}, d.dev);
    check(hpc_rll_dist_nstep_td_forward(fptr(dist), fptr(ndist), iptr(action), iptr(naction), fptr(reward), fptr(done),
                                        fptr(weight), fmut(loss), fmut(td_err), fmut(buf), fmut(partials),
                                        to_int(d.nstep, "nstep"), to_int(d.B, "B"), to_int(d.N, "N"), to_int(d.A, "n_atom"),
                                        (float)gamma, (float)v_min, (float)v_max, loss_scale(scale, d.B),
                                        stream_of(d.dev)),
          "hpc_rll_dist_nstep_td_forward");
}
// inputs = [dist, next_n_dist (B,N,n_atom), action, next_n_action (B,), reward (nstep,B), done (B,), weight (B,)|None];
// outputs = [td_err (B,), loss (1,), buf].  Reference: src/rl_utils/dist_nstep_td.cu:8-72, whose buf is
// (B + B*n_atom,) (hpc_rll/rl_utils/td.py:60): any contiguous buf with >= B*n_atom floats is accepted and its first
// B*n_atom floats receive the unit gradient wrt dist[b,a_b,:].
void DistNStepTdForward(const OptList& in, const TensorList& out, double gamma, double v_min, double v_max,
                        std::optional<double> scale) {
    expect_len(in, 7, "DistNStepTdForward inputs");
    expect_len(out, 3, "DistNStepTdForward outputs");
    for (int i = 0; i < 6; ++i) TORCH_CHECK(has(in[i]), "DistNStepTdForward: inputs[", i, "] is None");
    const DistDims d = dist_check(*in[0], *in[1], *in[2], *in[3], *in[4], *in[5], in[6]);
    td_list_outputs(out[0], out[1], false, out[2], "buf", d.B * d.A, "B*n_atom", d.B, d.dev);
    c10::DeviceGuard g(d.dev);
    dist_forward_launch(d, *in[0], *in[1], *in[2], *in[3], *in[4], *in[5], in[6], out[0], out[1], out[2], gamma, v_min,
                        v_max, scale);
}
void dist_backward_launch(const Tensor& gl, const Tensor& buf, const Tensor& action, const Tensor& grad_dist) {
    check(hpc_rll_dist_nstep_td_backward(fptr(gl), fptr(buf), iptr(action), fmut(grad_dist), (int)grad_dist.size(0),
                                         (int)grad_dist.size(1), (int)grad_dist.size(2), stream_of(grad_dist.device())),
          "hpc_rll_dist_nstep_td_backward");
}
// inputs = [grad_loss, buf, action]; outputs = [grad_dist (B,N,n_atom)].  dist_nstep_td.cu:74-98.
void DistNStepTdBackward(const TensorList& in, const TensorList& out) {
    expect_len(in, 3, "DistNStepTdBackward inputs");
    expect_len(out, 1, "DistNStepTdBackward outputs");
    const Tensor& gd = req(out[0], "grad_dist");
    TORCH_CHECK(gd.dim() == 3, "grad_dist: expected (B,N,n_atom), got ", gd.sizes());
    const at::Device dev = gd.device();
    req(in[1], "buf", dev);
    TORCH_CHECK(in[1].numel() >= gd.size(0) * gd.size(2), "buf: too small");
    req(in[2], "action", dev, {gd.size(0)}, at::kLong);
    c10::DeviceGuard g(dev);
    dist_backward_launch(grad1(in[0], dev, "grad_loss"), in[1], in[2], gd);
}

struct DistFn : public ag::Function<DistFn> {
    static ag::tensor_list forward(ag::AutogradContext* ctx, const Tensor& dist, const Tensor& ndist,
                                   const Tensor& action, const Tensor& naction, const Tensor& reward, const Tensor& done,
                                   const OptTensor& weight, double gamma, double v_min, double v_max,
                                   std::optional<double> scale) {
        const DistDims d = dist_check(dist, ndist, action, naction, reward, done, weight);
        c10::DeviceGuard g(d.dev);
        Tensor td_err = new_f32({d.B}, d.dev), loss = new_f32({1}, d.dev), buf = new_f32({d.B, d.A}, d.dev);
        dist_forward_launch(d, dist, ndist, action, naction, reward, done, weight, td_err, loss, buf, gamma, v_min, v_max,
                            scale);
        ctx->save_for_backward({buf, action});
        ctx->saved_data["N"] = d.N;
        ctx->mark_non_differentiable({td_err});
        return {loss, td_err};
    }
    static ag::tensor_list backward(ag::AutogradContext* ctx, ag::tensor_list grads) {
        return onehot_td_backward(ctx, grads, 11, shape_bnx, dist_backward_launch);
    }
};

// =========================================================================================================== IQN
struct IqnDims { int64_t tau, tau_p, B, N, nstep; at::Device dev; };
// bnt (round 6, not in the reference): q (B,N,tau), next_n_q (B,N,tau') -- the quantile axis innermost, QR-DQN's layout
IqnDims iqn_check(const Tensor& q, const Tensor& nq, const Tensor& action, const Tensor& naction, const Tensor& reward,
                  const Tensor& done, const Tensor& rq, const OptTensor& weight, const OptTensor& vg, bool bnt = false) {
    req(q, "q");
    TORCH_CHECK(q.dim() == 3, "q: expected ", bnt ? "(B,N,tau)" : "(tau,B,N)", ", got ", q.sizes());
    const int64_t tau = bnt ? q.size(2) : q.size(0), B = bnt ? q.size(0) : q.size(1), N = bnt ? q.size(1) : q.size(2);
    const at::Device dev = q.device();
    req(nq, "next_n_q", dev);
    if (bnt) {
        TORCH_CHECK(nq.dim() == 3 && nq.size(0) == B && nq.size(1) == N, "next_n_q: shape ", nq.sizes(), ", expected (", B, ",",
                    N, ",tau')");
    } else {
        TORCH_CHECK(nq.dim() == 3 && nq.size(1) == B && nq.size(2) == N, "next_n_q: shape ", nq.sizes(), ", expected (tau',",
                    B, ",", N, ")");
    }
    const int64_t nstep = nstep_sample_check(action, naction, reward, done, B, dev);
    req(rq, "replay_quantiles", dev);
    TORCH_CHECK(rq.numel() == tau * B, "replay_quantiles: ", rq.sizes(), " does not hold tau*B = ", tau * B, " values");
    req_opt(weight, "weight", dev, {B});
    req_opt(vg, "value_gamma", dev, {B});
    return {tau, bnt ? nq.size(2) : nq.size(0), B, N, nstep, dev};
}
void iqn_forward_launch(const IqnDims& d, const Tensor& q, const Tensor& nq, const Tensor& action, const Tensor& naction,
                        const Tensor& reward, const Tensor& done, const Tensor& rq, const OptTensor& weight,
                        const OptTensor& vg, const Tensor& loss, const Tensor& td_err, const Tensor& grad_buf,
                        double gamma, double kappa, std::optional<double> scale, bool bnt = false) {
    Tensor partials = new_f32({hpc_rll_partials_floats(d.B)}, d.dev);
    check((bnt ? hpc_rll_iqn_nstep_td_forward_bnt : hpc_rll_iqn_nstep_td_forward)(fptr(q), fptr(nq), iptr(action), iptr(naction), fptr(reward), fptr(done), fptr(rq),
                                       fptr(weight), fptr(vg), fmut(loss), fmut(td_err), fmut(grad_buf), fmut(partials),
                                       to_int(d.tau, "tau"), to_int(d.tau_p, "tau'"), to_int(d.nstep, "nstep"),
                                       to_int(d.B, "B"), to_int(d.N, "N"), (float)gamma, (float)kappa,
                                       loss_scale(scale, d.B), stream_of(d.dev)),
          "hpc_rll_iqn_nstep_td_forward");
}
// inputs = [q (tau,B,N), next_n_q (tau',B,N), action, next_n_action (B,), reward (nstep,B), done (B,),
// replay_quantiles (tau,B), weight (B,)|None, value_gamma (B,)|None].
// outputs: native [loss (1,), td_err (B,), grad_buf (B,tau)], or the reference's five
// [loss, td_err, bellman_err_buf, quantile_huber_loss_buf, grad_buf (B,tau',tau)] (hpc_rll/rl_utils/td.py:378-379):
// the two (B,tau',tau) scratch outputs are ignored and the first B*tau floats of grad_buf receive the unit gradient
// wrt q[:,b,a_b].  Reference: src/rl_utils/iqn_nstep_td_error.cu:8-72.
void IQNNStepTDErrorForward(const OptList& in, const TensorList& out, double gamma, double kappa,
                            std::optional<double> scale) {
    expect_len(in, 9, "IQNNStepTDErrorForward inputs");
    TORCH_CHECK(out.size() == 3 || out.size() == 5, "IQNNStepTDErrorForward outputs: expected 3 or 5 tensors, got ",
                out.size());
    for (int i = 0; i < 7; ++i) TORCH_CHECK(has(in[i]), "IQNNStepTDErrorForward: inputs[", i, "] is None");
    const IqnDims d = iqn_check(*in[0], *in[1], *in[2], *in[3], *in[4], *in[5], *in[6], in[7], in[8]);
    td_list_outputs(out[0], out[1], true, out.back(), "grad_buf", d.B * d.tau, "B*tau", d.B, d.dev);
    c10::DeviceGuard g(d.dev);
    iqn_forward_launch(d, *in[0], *in[1], *in[2], *in[3], *in[4], *in[5], *in[6], in[7], in[8], out[0], out[1], out.back(),
                       gamma, kappa, scale);
}
void iqn_backward_launch(const Tensor& gl, const Tensor& grad_buf, const Tensor& action, const Tensor& grad_q) {
    check(hpc_rll_iqn_nstep_td_backward(fptr(gl), fptr(grad_buf), iptr(action), fmut(grad_q), (int)grad_q.size(0),
                                        (int)grad_q.size(1), (int)grad_q.size(2), stream_of(grad_q.device())),
          "hpc_rll_iqn_nstep_td_backward");
}
void iqn_backward_bnt_launch(const Tensor& gl, const Tensor& grad_buf, const Tensor& action, const Tensor& grad_q) {   // (B,N,tau)
    check(hpc_rll_iqn_nstep_td_backward_bnt(fptr(gl), fptr(grad_buf), iptr(action), fmut(grad_q), (int)grad_q.size(2),
                                            (int)grad_q.size(0), (int)grad_q.size(1), stream_of(grad_q.device())),
          "hpc_rll_iqn_nstep_td_backward_bnt");
}
// inputs = [grad_loss, grad_buf, action] or the reference's [grad_loss, grad_buf, weight, action] (td.py:382; the
// weight is already folded into grad_buf); outputs = [grad_q (tau,B,N)].  iqn_nstep_td_error.cu:74-104.
void IQNNStepTDErrorBackward(const OptList& in, const TensorList& out) {
    TORCH_CHECK(in.size() == 3 || in.size() == 4, "IQNNStepTDErrorBackward inputs: expected 3 or 4 tensors");
    expect_len(out, 1, "IQNNStepTDErrorBackward outputs");
    const Tensor& gq = req(out[0], "grad_q");
    TORCH_CHECK(gq.dim() == 3, "grad_q: expected (tau,B,N), got ", gq.sizes());
    const at::Device dev = gq.device();
    TORCH_CHECK(has(in[0]) && has(in[1]) && has(in.back()), "IQNNStepTDErrorBackward: None input");
    req(*in[1], "grad_buf", dev);
    TORCH_CHECK(in[1]->numel() >= gq.size(0) * gq.size(1), "grad_buf: too small");
    req(*in.back(), "action", dev, {gq.size(1)}, at::kLong);
    c10::DeviceGuard g(dev);
    iqn_backward_launch(grad1(*in[0], dev, "grad_loss"), *in[1], *in.back(), gq);
}

struct IqnFn : public ag::Function<IqnFn> {
    static ag::tensor_list forward(ag::AutogradContext* ctx, const Tensor& q, const Tensor& nq, const Tensor& action,
                                   const Tensor& naction, const Tensor& reward, const Tensor& done, const Tensor& rq,
                                   const OptTensor& weight, const OptTensor& vg, double gamma, double kappa,
                                   std::optional<double> scale, bool bnt) {
        const IqnDims d = iqn_check(q, nq, action, naction, reward, done, rq, weight, vg, bnt);
        c10::DeviceGuard g(d.dev);
        Tensor loss = new_f32({1}, d.dev), td_err = new_f32({d.B}, d.dev), grad_buf = new_f32({d.B, d.tau}, d.dev);
        iqn_forward_launch(d, q, nq, action, naction, reward, done, rq, weight, vg, loss, td_err, grad_buf, gamma, kappa,
                           scale, bnt);
        ctx->save_for_backward({grad_buf, action});
        ctx->saved_data["N"] = d.N;
        ctx->saved_data["bnt"] = bnt;
        ctx->mark_non_differentiable({td_err});
        return {loss, td_err};
    }
    static ag::tensor_list backward(ag::AutogradContext* ctx, ag::tensor_list grads) {
        if (ctx->saved_data["bnt"].toBool()) return onehot_td_backward(ctx, grads, 13, shape_bnx, iqn_backward_bnt_launch);
        return onehot_td_backward(ctx, grads, 13, [](const Tensor& gb, int64_t N) { return at::DimVector{gb.size(1), gb.size(0), N}; },
                                  iqn_backward_launch);
    }
};

// ======================================================================================================== QR-DQN
struct QrDims { int64_t B, N, tau, nstep; at::Device dev; };
QrDims qr_check(const Tensor& q, const Tensor& nq, const Tensor& action, const Tensor& naction, const Tensor& reward,
                const Tensor& done, const OptTensor& weight, const OptTensor& vg) {
    req(q, "q");
    TORCH_CHECK(q.dim() == 3, "q: expected (B,N,tau), got ", q.sizes());
    const int64_t B = q.size(0), N = q.size(1), tau = q.size(2);
    const at::Device dev = q.device();
    req(nq, "next_n_q", dev, {B, N, tau});
    const int64_t nstep = nstep_sample_check(action, naction, reward, done, B, dev);
    req_opt(weight, "weight", dev, {B});
    req_opt(vg, "value_gamma", dev, {B});
    return {B, N, tau, nstep, dev};
}
void qr_forward_launch(const QrDims& d, const Tensor& q, const Tensor& nq, const Tensor& action, const Tensor& naction,
                       const Tensor& reward, const Tensor& done, const OptTensor& weight, const OptTensor& vg,
                       const Tensor& loss, const Tensor& td_err, const Tensor& grad_buf, double gamma,
                       std::optional<double> tau_value, std::optional<double> scale) {
    Tensor partials = new_f32({hpc_rll_partials_floats(d.B)}, d.dev);
    check(hpc_rll_qrdqn_nstep_td_forward(fptr(q), fptr(nq), iptr(action), iptr(naction), fptr(reward), fptr(done),
                                         fptr(weight), fptr(vg), fmut(loss), fmut(td_err), fmut(grad_buf), fmut(partials),
                                         to_int(d.tau, "tau"), to_int(d.nstep, "nstep"), to_int(d.B, "B"), to_int(d.N, "N"),
                                         (float)gamma, (float)(tau_value.has_value() ? *tau_value : (double)d.tau),
                                         loss_scale(scale, d.B), stream_of(d.dev)),
          "hpc_rll_qrdqn_nstep_td_forward");
}
// inputs = [q, next_n_q (B,N,tau), action, next_n_action (B,), reward (nstep,B), done (B,), weight (B,)|None,
// value_gamma (B,)|None]; outputs: native [loss (1,), td_err (B,), grad_buf (B,tau)] or the reference's five
// [loss, td_err, bellman_err_buf, quantile_huber_loss_buf, grad_buf (B,tau)] (td.py:492-493; the two (B,tau,tau)
// scratch outputs are ignored).  `tau_value` = the `tau` the oracle is called with; default = the integer count the
// reference kernel hard-codes (qrdqn_nstep_td_error_kernel.h:60).  Reference: src/rl_utils/qrdqn_nstep_td_error.cu:8-68.
void QRDQNNStepTDErrorForward(const OptList& in, const TensorList& out, double gamma, std::optional<double> tau_value,
                              std::optional<double> scale) {
    expect_len(in, 8, "QRDQNNStepTDErrorForward inputs");
    TORCH_CHECK(out.size() == 3 || out.size() == 5, "QRDQNNStepTDErrorForward outputs: expected 3 or 5 tensors, got ",
                out.size());
    for (int i = 0; i < 6; ++i) TORCH_CHECK(has(in[i]), "QRDQNNStepTDErrorForward: inputs[", i, "] is None");
    const QrDims d = qr_check(*in[0], *in[1], *in[2], *in[3], *in[4], *in[5], in[6], in[7]);
    td_list_outputs(out[0], out[1], true, out.back(), "grad_buf", d.B * d.tau, "B*tau", d.B, d.dev);
    c10::DeviceGuard g(d.dev);
    qr_forward_launch(d, *in[0], *in[1], *in[2], *in[3], *in[4], *in[5], in[6], in[7], out[0], out[1], out.back(), gamma,
                      tau_value, scale);
}
void qr_backward_launch(const Tensor& gl, const Tensor& grad_buf, const Tensor& action, const Tensor& grad_q) {
    check(hpc_rll_qrdqn_nstep_td_backward(fptr(gl), fptr(grad_buf), iptr(action), fmut(grad_q), (int)grad_q.size(2),
                                          (int)grad_q.size(0), (int)grad_q.size(1), stream_of(grad_q.device())),
          "hpc_rll_qrdqn_nstep_td_backward");
}
// inputs = [grad_loss, grad_buf (B,tau), action] or the reference's [grad_loss, grad_buf, weight, action] (td.py:496);
// outputs = [grad_q (B,N,tau)].  qrdqn_nstep_td_error.cu:70-99.
void QRDQNNStepTDErrorBackward(const OptList& in, const TensorList& out) {
    TORCH_CHECK(in.size() == 3 || in.size() == 4, "QRDQNNStepTDErrorBackward inputs: expected 3 or 4 tensors");
    expect_len(out, 1, "QRDQNNStepTDErrorBackward outputs");
    const Tensor& gq = req(out[0], "grad_q");
    TORCH_CHECK(gq.dim() == 3, "grad_q: expected (B,N,tau), got ", gq.sizes());
    const at::Device dev = gq.device();
    TORCH_CHECK(has(in[0]) && has(in[1]) && has(in.back()), "QRDQNNStepTDErrorBackward: None input");
    req(*in[1], "grad_buf", dev);
    TORCH_CHECK(in[1]->numel() >= gq.size(0) * gq.size(2), "grad_buf: too small");
    req(*in.back(), "action", dev, {gq.size(0)}, at::kLong);
    c10::DeviceGuard g(dev);
    qr_backward_launch(grad1(*in[0], dev, "grad_loss"), *in[1], *in.back(), gq);
}

struct QrFn : public ag::Function<QrFn> {
    static ag::tensor_list forward(ag::AutogradContext* ctx, const Tensor& q, const Tensor& nq, const Tensor& action,
                                   const Tensor& naction, const Tensor& reward, const Tensor& done,
                                   const OptTensor& weight, const OptTensor& vg, double gamma,
                                   std::optional<double> tau_value, std::optional<double> scale) {
        const QrDims d = qr_check(q, nq, action, naction, reward, done, weight, vg);
        c10::DeviceGuard g(d.dev);
        Tensor loss = new_f32({1}, d.dev), td_err = new_f32({d.B}, d.dev), grad_buf = new_f32({d.B, d.tau}, d.dev);
        qr_forward_launch(d, q, nq, action, naction, reward, done, weight, vg, loss, td_err, grad_buf, gamma, tau_value,
                          scale);
        ctx->save_for_backward({grad_buf, action});
        ctx->saved_data["N"] = d.N;
        ctx->mark_non_differentiable({td_err});
        return {loss, td_err};
    }
    static ag::tensor_list backward(ag::AutogradContext* ctx, ag::tensor_list grads) {
        return onehot_td_backward(ctx, grads, 11, shape_bnx, qr_backward_launch);
    }
};

// =========================================================================================================== FQF
// (no reference counterpart; DI-engine's fqf_nstep_td_error / fqf_calculate_fraction_loss and the fraction proposal of FQFHead)
struct FqfFractionsFn : public ag::Function<FqfFractionsFn> {
    static ag::tensor_list forward(ag::AutogradContext* ctx, const Tensor& logits) {
        req(logits, "logits");
        TORCH_CHECK(logits.dim() == 2 && logits.size(1) >= 1, "logits: expected (B,K) with K >= 1, got ", logits.sizes());
        const int64_t B = logits.size(0), K = logits.size(1);
        const at::Device dev = logits.device();
        c10::DeviceGuard g(dev);
        Tensor quantiles = new_f32({B, K + 1}, dev), hats = new_f32({B, K}, dev), ent = new_f32({B, 1}, dev);
        check(hpc_rll_fqf_fractions_forward(fptr(logits), fmut(quantiles), fmut(hats), fmut(ent), to_int(B, "B"), to_int(K, "K"),
                                            stream_of(dev)),
              "hpc_rll_fqf_fractions_forward (1 <= K <= 1024)");
        ctx->save_for_backward({logits, ent});
        ctx->mark_non_differentiable({hats});
        return {quantiles, hats, ent};
    }
    static ag::tensor_list backward(ag::AutogradContext* ctx, ag::tensor_list grads) {
        ag::tensor_list out(1);
        if (!ctx->needs_input_grad(0)) return out;
        const auto saved = ctx->get_saved_variables();
        const Tensor &logits = saved[0], &ent = saved[1];
        const at::Device dev = logits.device();
        c10::DeviceGuard g(dev);
        const int64_t B = logits.size(0), K = logits.size(1);
        // either upstream gradient may be absent: it counts as zero
        Tensor gq = grads[0].defined() ? req(grads[0].contiguous(), "grad_quantiles", dev, {B, K + 1}) : Tensor();
        Tensor gh = grads[2].defined() ? req(grads[2].contiguous(), "grad_entropies", dev, {B, 1}) : Tensor();
        Tensor gl = new_f32({B, K}, dev);
        check(hpc_rll_fqf_fractions_backward(fptr(logits), fptr(ent), fptr(gq), fptr(gh), fmut(gl), (int)B, (int)K, stream_of(dev)),
              "hpc_rll_fqf_fractions_backward");
        out[0] = gl;
        return out;
    }
};

struct FqfDims { int64_t B, K, Kp, N, nstep; at::Device dev; };
FqfDims fqf_td_check(const Tensor& q, const Tensor& nq, const Tensor& action, const Tensor& naction, const Tensor& reward,
                     const Tensor& done, const Tensor& qh, const OptTensor& weight, const OptTensor& vg) {
    req(q, "q");
    TORCH_CHECK(q.dim() == 3 && q.size(1) >= 1 && q.size(2) >= 1, "q: expected (B,K,N), got ", q.sizes());
    const int64_t B = q.size(0), K = q.size(1), N = q.size(2);
    const at::Device dev = q.device();
    req(nq, "next_n_q", dev);
    TORCH_CHECK(nq.dim() == 3 && nq.size(0) == B && nq.size(1) >= 1 && nq.size(2) == N, "next_n_q: shape ", nq.sizes(),
                ", expected (", B, ",K',", N, ")");
    const int64_t nstep = nstep_sample_check(action, naction, reward, done, B, dev);
    req(qh, "quantiles_hats", dev, {B, K});
    req_opt(weight, "weight", dev, {B});
    req_opt(vg, "value_gamma", dev, {B});
    return {B, K, nq.size(1), N, nstep, dev};
}

struct FqfTdFn : public ag::Function<FqfTdFn> {
    static ag::tensor_list forward(ag::AutogradContext* ctx, const Tensor& q, const Tensor& nq, const Tensor& action,
                                   const Tensor& naction, const Tensor& reward, const Tensor& done, const Tensor& qh,
                                   const OptTensor& weight, const OptTensor& vg, double gamma, double kappa,
                                   std::optional<double> scale) {
        const FqfDims d = fqf_td_check(q, nq, action, naction, reward, done, qh, weight, vg);
        TORCH_CHECK(kappa > 0.0, "kappa: expected > 0, got ", kappa);
        c10::DeviceGuard g(d.dev);
        Tensor loss = new_f32({1}, d.dev), td_err = new_f32({d.B}, d.dev), grad_buf = new_f32({d.B, d.K}, d.dev);
        Tensor partials = new_f32({hpc_rll_partials_floats(d.B)}, d.dev);
        check(hpc_rll_fqf_nstep_td_forward(fptr(q), fptr(nq), iptr(action), iptr(naction), fptr(reward), fptr(done), fptr(qh),
                                           fptr(weight), fptr(vg), fmut(loss), fmut(td_err), fmut(grad_buf), fmut(partials),
                                           to_int(d.K, "K"), to_int(d.Kp, "K'"), to_int(d.nstep, "nstep"), to_int(d.B, "B"),
                                           to_int(d.N, "N"), (float)gamma, (float)kappa, loss_scale(scale, d.B), stream_of(d.dev)),
              "hpc_rll_fqf_nstep_td_forward");
        ctx->save_for_backward({grad_buf, action});
        ctx->saved_data["N"] = d.N;
        ctx->mark_non_differentiable({td_err});
        return {loss, td_err};
    }
    static ag::tensor_list backward(ag::AutogradContext* ctx, ag::tensor_list grads) {
        return onehot_td_backward(
            ctx, grads, 12, [](const Tensor& gb, int64_t N) { return at::DimVector{gb.size(0), gb.size(1), N}; },
            [](const Tensor& gl, const Tensor& gb, const Tensor& action, const Tensor& gq) {   // gq (B,K,N)
                check(hpc_rll_fqf_nstep_td_backward(fptr(gl), fptr(gb), iptr(action), fmut(gq), (int)gq.size(1), (int)gq.size(0),
                                                    (int)gq.size(2), stream_of(gq.device())),
                      "hpc_rll_fqf_nstep_td_backward");
            });
    }
};

struct FqfFractionLossFn : public ag::Function<FqfFractionLossFn> {
    static Tensor forward(ag::AutogradContext* ctx, const Tensor& q_tau_i, const Tensor& q_value, const Tensor& quantiles,
                          const Tensor& actions, std::optional<double> scale) {
        req(q_value, "q_value");
        TORCH_CHECK(q_value.dim() == 3 && q_value.size(1) >= 1 && q_value.size(2) >= 1, "q_value: expected (B,K,N), got ",
                    q_value.sizes());
        const int64_t B = q_value.size(0), K = q_value.size(1), N = q_value.size(2);
        const at::Device dev = q_value.device();
        req(q_tau_i, "q_tau_i", dev, {B, K - 1, N});
        req(quantiles, "quantiles", dev, {B, K + 1});
        req(actions, "actions", dev, {B}, at::kLong);
        c10::DeviceGuard gd(dev);
        Tensor loss = new_f32({1}, dev), g = new_f32({B, K - 1}, dev), partials = new_f32({hpc_rll_partials_floats(B)}, dev);
        const float sc = loss_scale(scale, B);
        check(hpc_rll_fqf_fraction_loss_forward(fptr(q_tau_i), fptr(q_value), fptr(quantiles), iptr(actions), fmut(loss), fmut(g),
                                                fmut(partials), to_int(K, "K"), to_int(B, "B"), to_int(N, "N"), sc, stream_of(dev)),
              "hpc_rll_fqf_fraction_loss_forward");
        ctx->save_for_backward({g});
        ctx->saved_data["K"] = K;
        ctx->saved_data["scale"] = (double)sc;
        return loss;
    }
    static ag::tensor_list backward(ag::AutogradContext* ctx, ag::tensor_list grads) {
        ag::tensor_list out(5);
        if (!ctx->needs_input_grad(2)) return out;   // q_tau_i and q_value enter through g, a constant
        const Tensor g = ctx->get_saved_variables()[0];
        const at::Device dev = g.device();
        c10::DeviceGuard gd(dev);
        const int64_t B = g.size(0), K = ctx->saved_data["K"].toInt();
        Tensor gq = new_f32({B, K + 1}, dev);
        check(hpc_rll_fqf_fraction_loss_backward(fptr(grad1(grads[0], dev, "grad_loss")), fptr(g), fmut(gq), (int)K, (int)B,
                                                 (float)ctx->saved_data["scale"].toDouble(), stream_of(dev)),
              "hpc_rll_fqf_fraction_loss_backward");
        out[2] = gq;
        return out;
    }
};

// logit (B,N) and, with return_action, its argmax (B,) int64 from the same launch; forward only
std::tuple<Tensor, OptTensor> fqf_q_value(const Tensor& q, const Tensor& quantiles, bool return_action) {
    req(q, "q");
    TORCH_CHECK(q.dim() == 3 && q.size(1) >= 1 && q.size(2) >= 1, "q: expected (B,K,N), got ", q.sizes());
    const int64_t B = q.size(0), K = q.size(1), N = q.size(2);
    const at::Device dev = q.device();
    req(quantiles, "quantiles", dev, {B, K + 1});
    c10::DeviceGuard g(dev);
    Tensor logit = new_f32({B, N}, dev);
    OptTensor action;
    if (return_action) action = at::empty({B}, at::TensorOptions().dtype(at::kLong).device(dev));
    check(hpc_rll_fqf_q_value(fptr(q), fptr(quantiles), fmut(logit), action ? action->data_ptr<int64_t>() : nullptr,
                              to_int(B, "B"), to_int(K, "K"), to_int(N, "N"), stream_of(dev)),
          "hpc_rll_fqf_q_value");
    return {logit, action};
}

// defined in rl_utils_lists.cpp (V-trace / UPGO / PPO L2 functions incl. the reference's long positional lists) and
// rl_utils_pad.cpp (Pad / Unpad / group policies)
void bind_loss_lists(pybind11::module_& m);
void bind_padding(pybind11::module_& m);

}  // namespace hpc_rll_ext

PYBIND11_MODULE(hpc_rl_utils, m) {
    using namespace hpc_rll_ext;
    namespace py = pybind11;
    m.doc() = "hpc_rl_utils: MI355X (gfx950) operator library behind hpc_rll.rl_utils -- compiled PyTorch-ROCm "
              "extension over the C ABI of libhpc_rll_hip.so (reference: src/rl_utils/entry.cpp:8-39)";
    bind_common(m);

    // ---- L2: the reference's function names and list convention
    m.def("GaeForward", &GaeForward, py::arg("inputs"), py::arg("outputs"), py::arg("gamma"), py::arg("lambda_"),
          "gae forward (HIP)");
    m.def("GaeBackward", &GaeBackward, py::arg("inputs"), py::arg("outputs"), py::arg("gamma"), py::arg("lambda_"),
          "gae backward (HIP)");
    m.def("TdLambdaForward", &TdLambdaForward, py::arg("inputs"), py::arg("outputs"), py::arg("gamma"),
          py::arg("lambda_"), py::arg("scale") = py::none(), "td_lambda forward (HIP)");
    m.def("TdLambdaBackward", &TdLambdaBackward, "td_lambda backward (HIP)");
    m.def("QNStepTdForward",
          [](const OptList& in, const TensorList& out, double gamma, std::optional<double> scale) {
              q_forward_l2(in, out, gamma, 0, scale);
          },
          py::arg("inputs"), py::arg("outputs"), py::arg("gamma"), py::arg("scale") = py::none(),
          "q_nstep_td forward (HIP)");
    m.def("QNStepTdBackward", &q_backward_l2, "q_nstep_td backward (HIP)");
    m.def("QNStepTdRescaleForward",
          [](const OptList& in, const TensorList& out, double gamma, std::optional<double> scale) {
              q_forward_l2(in, out, gamma, 1, scale);
          },
          py::arg("inputs"), py::arg("outputs"), py::arg("gamma"), py::arg("scale") = py::none(),
          "q_nstep_td_with_rescale forward (HIP)");
    m.def("QNStepTdRescaleBackward", &q_backward_l2, "q_nstep_td_with_rescale backward (HIP)");
    m.def("DistNStepTdForward", &DistNStepTdForward, py::arg("inputs"), py::arg("outputs"), py::arg("gamma"),
          py::arg("v_min"), py::arg("v_max"), py::arg("scale") = py::none(), "dist_nstep_td forward (HIP)");
    m.def("DistNStepTdBackward", &DistNStepTdBackward, "dist_nstep_td backward (HIP)");
    m.def("IQNNStepTDErrorForward", &IQNNStepTDErrorForward, py::arg("inputs"), py::arg("outputs"), py::arg("gamma"),
          py::arg("kappa"), py::arg("scale") = py::none(), "iqn_nstep_td_error forward (HIP)");
    m.def("IQNNStepTDErrorBackward", &IQNNStepTDErrorBackward, "iqn_nstep_td_error backward (HIP)");
    m.def("QRDQNNStepTDErrorForward", &QRDQNNStepTDErrorForward, py::arg("inputs"), py::arg("outputs"), py::arg("gamma"),
          py::arg("tau_value") = py::none(), py::arg("scale") = py::none(), "qrdqn_nstep_td_error forward (HIP)");
    m.def("QRDQNNStepTDErrorBackward", &QRDQNNStepTDErrorBackward, "qrdqn_nstep_td_error backward (HIP)");
    bind_loss_lists(m);   // VTrace / Upgo / PPO Forward+Backward
    bind_padding(m);      // Pad / GroupPad / Unpad {1,2,3}D, split policies, packed variants

    // ---- fused autograd ops (what hpc_rll.rl_utils.* calls)
    m.def("gae", applier<GaeFn>(&GaeFn::forward),
          py::arg("value"), py::arg("reward"), py::arg("gamma") = 0.99, py::arg("lambda_") = 0.97,
          "adv = GAE(value (T+1,B), reward (T,B)); differentiable wrt value and reward");
    m.def("gae_masked", applier<GaeMaskedFn>(&GaeMaskedFn::forward),
          py::arg("value"), py::arg("reward"), py::arg("done") = py::none(), py::arg("traj_flag") = py::none(),
          py::arg("next_value") = py::none(), py::arg("gamma") = 0.99, py::arg("lambda_") = 0.97,
          "adv = textbook GAE with done / traj_flag masks; value (T+1,B), or value (T,B) with next_value (T,B); "
          "differentiable wrt value, next_value and reward");
    m.def("gae_coef", [](int64_t T, double gamma, double lambda, const at::Device& dev) {
        TORCH_CHECK(dev.is_cuda(), "gae_coef: device must be a GPU");
        c10::DeviceGuard g(dev);
        return gae_coef(T, gamma, lambda, dev);
    });
    m.def("td_lambda_masked", applier<TdLambdaMaskedFn>(&TdLambdaMaskedFn::forward),
          py::arg("value"), py::arg("reward"), py::arg("done") = py::none(), py::arg("traj_flag") = py::none(),
          py::arg("next_value") = py::none(), py::arg("weight") = py::none(), py::arg("gamma") = 0.9,
          py::arg("lambda_") = 0.8, py::arg("scale") = py::none(),
          "episode-aware TD(lambda) loss (1,) with done / traj_flag masks; differentiable wrt value");
    m.def("vtrace_masked", applier<VtraceMaskedFn>(&VtraceMaskedFn::forward),
          py::arg("target_output"), py::arg("behaviour_output"), py::arg("action"), py::arg("value"), py::arg("reward"),
          py::arg("done") = py::none(), py::arg("traj_flag") = py::none(), py::arg("next_value") = py::none(),
          py::arg("weight") = py::none(), py::arg("gamma") = 0.99, py::arg("lambda_") = 0.95,
          py::arg("rho_clip_ratio") = 1.0, py::arg("c_clip_ratio") = 1.0, py::arg("rho_pg_clip_ratio") = 1.0,
          py::arg("scale") = py::none(),
          "episode-aware V-trace losses (policy, value, entropy) with done / traj_flag masks");
    m.def("td_lambda", applier<TdLambdaFn>(&TdLambdaFn::forward),
          py::arg("value"), py::arg("reward"), py::arg("weight") = py::none(), py::arg("gamma") = 0.9,
          py::arg("lambda_") = 0.8, py::arg("scale") = py::none());
    m.def("vtrace", applier<VtraceFn>(&VtraceFn::forward),
          py::arg("target_output"), py::arg("behaviour_output"), py::arg("action"), py::arg("value"), py::arg("reward"),
          py::arg("weight") = py::none(), py::arg("gamma") = 0.99, py::arg("lambda_") = 0.95,
          py::arg("rho_clip_ratio") = 1.0, py::arg("c_clip_ratio") = 1.0, py::arg("rho_pg_clip_ratio") = 1.0,
          py::arg("scale") = py::none());
    m.def("upgo", applier<UpgoFn>(&UpgoFn::forward),
          py::arg("target_output"), py::arg("rhos"), py::arg("action"), py::arg("rewards"), py::arg("bootstrap_values"),
          py::arg("scale") = py::none());
    m.def("upgo_masked", applier<UpgoMaskedFn>(&UpgoMaskedFn::forward),
          py::arg("target_output"), py::arg("rhos"), py::arg("action"), py::arg("rewards"), py::arg("bootstrap_values"),
          py::arg("done") = py::none(), py::arg("traj_flag") = py::none(), py::arg("next_value") = py::none(),
          py::arg("gamma") = 1.0, py::arg("scale") = py::none(),
          "episode-aware UPGO loss (1,) with done / traj_flag masks; differentiable wrt target_output");
    m.def("ppo", applier<PpoFn>(&PpoFn::forward),
          py::arg("logits_new"), py::arg("logits_old"), py::arg("action"), py::arg("value_new"), py::arg("value_old"),
          py::arg("adv"), py::arg("return_"), py::arg("weight") = py::none(), py::arg("clip_ratio") = 0.2,
          py::arg("use_value_clip") = true, py::arg("dual_clip") = 0.0, py::arg("scale") = py::none());
    m.def("ppo_continuous", applier<PpoContinuousFn>(&PpoContinuousFn::forward),
          py::arg("mu_new"), py::arg("sigma_new"), py::arg("mu_old"), py::arg("sigma_old"), py::arg("action"),
          py::arg("value_new"), py::arg("value_old"), py::arg("adv"), py::arg("return_"), py::arg("weight") = py::none(),
          py::arg("clip_ratio") = 0.2, py::arg("use_value_clip") = true, py::arg("dual_clip") = 0.0,
          py::arg("scale") = py::none(),
          "PPO losses (policy, value, entropy, info) for a diagonal-Gaussian policy: mu / sigma / action (B,A) fp32, "
          "sigma > 0; differentiable wrt mu_new, sigma_new and value_new");
    m.def("vtrace_continuous", applier<VtraceContinuousFn>(&VtraceContinuousFn::forward),
          py::arg("mu_target"), py::arg("sigma_target"), py::arg("mu_behaviour"), py::arg("sigma_behaviour"), py::arg("action"),
          py::arg("value"), py::arg("reward"), py::arg("done") = py::none(), py::arg("traj_flag") = py::none(),
          py::arg("next_value") = py::none(), py::arg("weight") = py::none(), py::arg("gamma") = 0.99,
          py::arg("lambda_") = 0.95, py::arg("rho_clip_ratio") = 1.0, py::arg("c_clip_ratio") = 1.0,
          py::arg("rho_pg_clip_ratio") = 1.0, py::arg("scale") = py::none(),
          "episode-aware V-trace losses (policy, value, entropy) for diagonal-Gaussian policies: mu / sigma / action (T,B,A) "
          "fp32, sigma > 0; differentiable wrt mu_target, sigma_target and value");
    m.def("retrace", &retrace_targets, py::arg("q_values"), py::arg("v_pred"), py::arg("rewards"), py::arg("actions"),
          py::arg("weights"), py::arg("ratio"), py::arg("gamma") = 0.9, py::arg("lambda_") = 1.0,
          "Retrace(lambda) Q targets (T+1,B,1) from given state values (T+1,B,1) and importance ratios (T,B,N); no gradient");
    m.def("retrace_loss", applier<RetraceLossFn>(&RetraceLossFn::forward),
          py::arg("q_values"), py::arg("target_output"), py::arg("behaviour_output"), py::arg("action"), py::arg("reward"),
          py::arg("weights") = py::none(), py::arg("loss_weight") = py::none(), py::arg("gamma") = 0.9,
          py::arg("lambda_") = 1.0, py::arg("scale") = py::none(),
          "Retrace(lambda) critic loss (1,), Q targets (T+1,B) and state values (T+1,B) from q_values and the two policies' "
          "logits; differentiable wrt q_values");
    m.def("acer_policy_loss", [](const Tensor& target, const Tensor& behaviour, const Tensor& q, const Tensor& q_ret,
                                 const Tensor& v_pred, const Tensor& action, const OptTensor& weights, const OptTensor& avg,
                                 double c_clip, double entropy_weight, double trust_region, std::optional<double> scale) {
        // (inside the node grad mode is off: whether the unit gradient is worth storing is decided here)
        const bool want_grad = at::GradMode::is_enabled() && target.defined() && target.requires_grad();
        return AcerPolicyFn::apply(target, behaviour, q, q_ret, v_pred, action, weights, avg, c_clip, entropy_weight,
                                   trust_region, scale, want_grad);
    }, py::arg("target_output"), py::arg("behaviour_output"), py::arg("q_values"), py::arg("q_retraces"), py::arg("v_pred"),
          py::arg("action"), py::arg("weights") = py::none(), py::arg("avg_output") = py::none(),
          py::arg("c_clip_ratio") = 10.0, py::arg("entropy_weight") = 0.0, py::arg("trust_region_value") = 1.0,
          py::arg("scale") = py::none(),
          "ACER actor loss (1,) and its three detached monitors (actor, bias correction, entropy) from the two policies' "
          "logits, the average policy's (optional: the trust region), q_values and Retrace's q_retraces / v_pred; "
          "differentiable wrt target_output");
    m.def("acer_trust_region_update", &acer_trust_region, py::arg("actor_gradient"), py::arg("avg_logit"),
          py::arg("trust_region_value"),
          "g - max(0, (sum k g - trust_region_value) / sum k^2) k with k = exp(avg_logit), per row of N; no gradient");
    m.def("coma", [](const Tensor& logit, const Tensor& action, const Tensor& q, const Tensor& target_q, const Tensor& reward,
                     const OptTensor& weight, const OptTensor& done, double gamma, double lambda,
                     std::optional<std::pair<double, double>> scales) {
        std::optional<double> s_pe, s_q;
        if (scales.has_value()) { s_pe = scales->first; s_q = scales->second; }
        return ComaFn::apply(logit, action, q, target_q, reward, weight, done, gamma, lambda, s_pe, s_q);
    }, py::arg("logit"), py::arg("action"), py::arg("q_value"), py::arg("target_q_value"), py::arg("reward"),
          py::arg("weight") = py::none(), py::arg("done") = py::none(), py::arg("gamma") = 0.99, py::arg("lambda_") = 0.8,
          py::arg("scales") = py::none(),
          "COMA losses (policy, q_value, entropy; (1,) each) from (T,B,A,N) logits and action values, (T,B,A) int64 actions "
          "and (T,B) rewards; differentiable wrt logit and q_value; scales = (scale_pe, scale_q) for a sharded caller");
    m.def("r2d2_td", applier<R2d2Fn>(&R2d2Fn::forward),
          py::arg("q"), py::arg("target_q"), py::arg("action"), py::arg("reward"), py::arg("done") = py::none(),
          py::arg("weight") = py::none(), py::arg("gamma") = 0.997, py::arg("nstep") = 5, py::arg("burnin") = 0,
          py::arg("value_rescale") = true, py::arg("double_q") = true, py::arg("priority_eta") = 0.9,
          py::arg("scale") = py::none(),
          "R2D2 sequence loss over a (T,B,N) unroll: (loss (1,), td_error (L,B), priority (B,)) with L = T - nstep - burnin; "
          "differentiable wrt q; scale = 1/(global count) for a sharded caller");
    m.def("sac_discrete", [](const Tensor& logit, const Tensor& next_logit, const Tensor& q1, const OptTensor& q2,
                             const Tensor& target_q1, const OptTensor& target_q2, const Tensor& action, const Tensor& reward,
                             const OptTensor& done, const OptTensor& weight, double alpha, const OptTensor& alpha_tensor,
                             double gamma, std::optional<double> scale) {
        // (inside the node grad mode is off: whether the unit gradient is worth storing is decided here)
        const bool want_grad = at::GradMode::is_enabled() && logit.defined() && logit.requires_grad();
        return SacDiscreteFn::apply(logit, next_logit, q1, q2, target_q1, target_q2, action, reward, done, weight, alpha,
                                    alpha_tensor, gamma, scale, want_grad);
    }, py::arg("logit"), py::arg("next_logit"), py::arg("q1"), py::arg("q2"), py::arg("target_q1"), py::arg("target_q2"),
          py::arg("action"), py::arg("reward"), py::arg("done") = py::none(), py::arg("weight") = py::none(),
          py::arg("alpha") = 0.2, py::arg("alpha_tensor") = py::none(), py::arg("gamma") = 0.99,
          py::arg("scale") = py::none(),
          "Discrete SAC over (..., N) logits and critics: (policy_loss, critic_loss, twin_critic_loss, entropy; (1,) each, "
          "td_error, target_q (...)); q2 / target_q2 both tensors or both None (twin_critic_loss is then 0); alpha_tensor, a "
          "1-element fp32 GPU tensor, replaces alpha and is read on the device; differentiable wrt logit, q1 and q2; "
          "scale = 1/(global rows) for a sharded caller");
    m.def("token_log_prob", applier<TokenLogpFn>(&TokenLogpFn::forward), py::arg("logits"), py::arg("action"),
          "logits[..., a] - logsumexp(logits) per token: (..., V) fp32 or bf16 logits, (...) int64 actions -> (...) fp32; "
          "differentiable wrt logits");
    m.def("grpo_policy_loss", applier<GrpoFn>(&GrpoFn::forward),
          py::arg("logit_new"), py::arg("old"), py::arg("ref"), py::arg("action"), py::arg("adv"),
          py::arg("weight") = py::none(), py::arg("clip_ratio") = 0.2, py::arg("beta") = 0.1, py::arg("scale") = py::none(),
          "GRPO token loss over (B,S,V) logits: (loss, mean_kl, mean_ratio, mean_clipped), (1,) each; old / ref are logits "
          "(B,S,V) or log-probs (B,S), ref may be None; differentiable wrt logit_new; scale = 1/(global B) for a sharded caller");
    m.def("token_log_prob_entropy", applier<TokenLpeFn>(&TokenLpeFn::forward),
          py::arg("logits"), py::arg("action"), py::arg("weight") = py::none(),
          "(logp, entropy) per token from one read of (..., V) fp32 or bf16 logits; both differentiable wrt logits");
    m.def("lm_gae", &lm_gae, py::arg("value"), py::arg("weight"), py::arg("reward"), py::arg("kl") = py::none(),
          py::arg("beta") = 0.0, py::arg("gamma") = 1.0, py::arg("lam") = 0.95, py::arg("whiten") = true,
          "Token-level GAE over (B,S) under a response mask: (adv, ret); reward is (B,S) or a terminal score (B,)");
    m.def("lm_ppo_loss", applier<LmPpoFn>(&LmPpoFn::forward),
          py::arg("logit_new"), py::arg("old_logp"), py::arg("action"), py::arg("adv"), py::arg("weight") = py::none(),
          py::arg("value_new") = py::none(), py::arg("value_old") = py::none(), py::arg("ret") = py::none(),
          py::arg("clip_ratio") = 0.2, py::arg("dual_clip") = py::none(), py::arg("value_clip") = 0.2,
          py::arg("seq_mean") = false, py::arg("raw") = false, py::arg("scale") = py::none(),
          "Token-level PPO over (B,S,V) logits: (policy_loss, value_loss, entropy, approx_kl, mean_ratio, clipfrac, den), (1,) "
          "each; the first three are differentiable wrt logit_new and value_new; raw leaves the six as numerators over den "
          "for a sharded caller; scale = 1/(global B) for a sharded caller in sequence mode");
    m.def("q_nstep_td", [](const Tensor& q, const Tensor& nq, const Tensor& action, const Tensor& naction,
                           const Tensor& reward, const Tensor& done, const OptTensor& weight, double gamma, bool rescale,
                           std::optional<double> scale) {
        return rescale ? QNStepFn<1>::apply(q, nq, action, naction, reward, done, weight, gamma, scale)
                       : QNStepFn<0>::apply(q, nq, action, naction, reward, done, weight, gamma, scale);
    }, py::arg("q"), py::arg("next_n_q"), py::arg("action"), py::arg("next_n_action"), py::arg("reward"), py::arg("done"),
          py::arg("weight"), py::arg("gamma"), py::arg("rescale") = false, py::arg("scale") = py::none());
    m.def("dist_nstep_td", applier<DistFn>(&DistFn::forward),
          py::arg("dist"), py::arg("next_n_dist"), py::arg("action"), py::arg("next_n_action"), py::arg("reward"),
          py::arg("done"), py::arg("weight"), py::arg("gamma"), py::arg("v_min"), py::arg("v_max"),
          py::arg("scale") = py::none());
    m.def("iqn_nstep_td", applier<IqnFn>(&IqnFn::forward),
          py::arg("q"), py::arg("next_n_q"), py::arg("action"), py::arg("next_n_action"), py::arg("reward"), py::arg("done"),
          py::arg("replay_quantiles"), py::arg("weight") = py::none(), py::arg("value_gamma") = py::none(),
          py::arg("gamma") = 0.99, py::arg("kappa") = 1.0, py::arg("scale") = py::none(), py::arg("bnt") = false);
    m.def("qrdqn_nstep_td", applier<QrFn>(&QrFn::forward),
          py::arg("q"), py::arg("next_n_q"), py::arg("action"), py::arg("next_n_action"), py::arg("reward"), py::arg("done"),
          py::arg("weight") = py::none(), py::arg("value_gamma") = py::none(), py::arg("gamma") = 0.99,
          py::arg("tau_value") = py::none(), py::arg("scale") = py::none());
    m.def("fqf_fractions", applier<FqfFractionsFn>(&FqfFractionsFn::forward), py::arg("logits"),
          "FQF fraction proposal from (B,K) logits: (quantiles (B,K+1), quantiles_hats (B,K), entropies (B,1)); quantiles and "
          "entropies are differentiable wrt logits, quantiles_hats is detached");
    m.def("fqf_nstep_td", applier<FqfTdFn>(&FqfTdFn::forward),
          py::arg("q"), py::arg("next_n_q"), py::arg("action"), py::arg("next_n_action"), py::arg("reward"), py::arg("done"),
          py::arg("quantiles_hats"), py::arg("weight") = py::none(), py::arg("value_gamma") = py::none(),
          py::arg("gamma") = 0.99, py::arg("kappa") = 1.0, py::arg("scale") = py::none(),
          "FQF n-step quantile TD loss on q (B,K,N), next_n_q (B,K',N), quantiles_hats (B,K): (loss (1,), td_err (B,)); "
          "differentiable wrt q; scale = 1/(global B) for a sharded caller");
    m.def("fqf_fraction_loss", applier<FqfFractionLossFn>(&FqfFractionLossFn::forward),
          py::arg("q_tau_i"), py::arg("q_value"), py::arg("quantiles"), py::arg("actions"), py::arg("scale") = py::none(),
          "FQF fraction loss on q_tau_i (B,K-1,N), q_value (B,K,N), quantiles (B,K+1): loss (1,); differentiable wrt "
          "quantiles[:,1:K] only");
    m.def("fqf_q_value", &fqf_q_value, py::arg("q"), py::arg("quantiles"), py::arg("return_action") = false,
          "FQF expected value (B,N) = sum_i (quantiles[:,i+1] - quantiles[:,i]) q[:,i,:] and, with return_action, its argmax "
          "(ties to the lowest index) from the same launch; forward only");
}
