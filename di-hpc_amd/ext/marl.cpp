// hpc_marl -- the fused ops of cooperative multi-agent value decomposition (no reference counterpart): QMIX's monotonic
// mixing network from the hypernetworks' outputs on (hpc_rll_qmix_*; DI-engine's ding/model/template/qmix.py Mixer.forward)
// and its mixed one-step TD loss.  HOST-ONLY C++ like the other three modules (common.hpp): it validates tensors, takes
// outputs and scratch from torch's caching allocator and calls the C ABI on torch's current stream.  Nothing here
// synchronises with the host.
#include "rl_utils_ops.hpp"

namespace hpc_rll_ext {
namespace {

// The five operands of one mixing network behind agent_q (..., A) and b1 (..., E): w1 (..., A, E), w2 (..., E), b2 (...).
// Every tensor is declared once, with the prefix of its network in its name.
struct QmixDims { int64_t rows, A, E; std::vector<int64_t> lead, w1, hid, qs; };

QmixDims qmix_dims(const Tensor& agent_q, const Tensor& b1) {
    TORCH_CHECK(agent_q.defined(), "agent_q: expected a tensor, got None");
    TORCH_CHECK(agent_q.dim() >= 1, "agent_q: expected (..., A), got ", agent_q.sizes());
    TORCH_CHECK(b1.defined(), "b1: expected a tensor, got None");
    TORCH_CHECK(b1.dim() >= 1, "b1: expected (..., E), got ", b1.sizes());
    QmixDims d;
    const at::IntArrayRef full = agent_q.sizes();
    d.A = full.back();
    d.E = b1.sizes().back();
    d.lead.assign(full.begin(), full.end() - 1);
    d.qs.assign(full.begin(), full.end());
    d.w1 = d.lead;
    d.w1.push_back(d.A);
    d.w1.push_back(d.E);
    d.hid = d.lead;
    d.hid.push_back(d.E);
    d.rows = 1;
    for (int64_t n : d.lead) d.rows *= n;
    return d;
}

void qmix_check_sizes(const char* op, const QmixDims& d) {
    TORCH_CHECK(d.A >= 1 && d.A <= 64, op, ": 1 <= A <= 64 agents are implemented, got ", d.A);
    TORCH_CHECK(d.E >= 1 && d.E <= 256, op, ": 1 <= E <= 256 hidden units are implemented, got ", d.E);
}

// grad_q, grad_w1, grad_b1, grad_w2, grad_b2 for the inputs 0..4 that need them, from the per-row g the C ABI describes
ag::tensor_list qmix_backward_launch(ag::AutogradContext* ctx, const Tensor& g_loss, const Tensor& g_rows, const Tensor& ws,
                                     const ag::tensor_list& saved, size_t n_inputs) {
    ag::tensor_list out(n_inputs);
    const Tensor &q = saved[0], &w1 = saved[1], &b1 = saved[2], &w2 = saved[3], &b2 = saved[4];
    const at::Device dev = q.device();
    const Tensor* in[5] = {&q, &w1, &b1, &w2, &b2};
    Tensor grad[5];
    for (int i = 0; i < 5; ++i)
        if (ctx->needs_input_grad(i)) grad[i] = new_f32(in[i]->sizes(), dev);
    check(hpc_rll_qmix_backward(fptr(g_loss), fptr(g_rows), fptr(ws), fptr(q), fptr(w1), fptr(b1), fptr(w2), fptr(b2),
                                fmut(grad[0]), fmut(grad[1]), fmut(grad[2]), fmut(grad[3]), fmut(grad[4]), b2.numel(),
                                (int)q.sizes().back(), (int)b1.sizes().back(), stream_of(dev)),
          "hpc_rll_qmix_backward");
    for (int i = 0; i < 5; ++i) out[i] = grad[i];
    return out;
}

bool qmix_needs_any(ag::AutogradContext* ctx) {
    for (int i = 0; i < 5; ++i)
        if (ctx->needs_input_grad(i)) return true;
    return false;
}

// =========================================================================================================== the mix
// q_tot (...) from agent_q (..., A), w1 (..., A, E), b1 (..., E), w2 (..., E), b2 (...); differentiable wrt all five, each
// gradient formed only when its input needs it.  Saves the five inputs: the backward recomputes the hidden layer.
struct QmixMixFn : public ag::Function<QmixMixFn> {
    static Tensor forward(ag::AutogradContext* ctx, const Tensor& agent_q, const Tensor& w1, const Tensor& b1,
                          const Tensor& w2, const Tensor& b2) {
        const QmixDims d = qmix_dims(agent_q, b1);
        Args args;
        args.add(agent_q, "agent_q", d.qs);
        args.add(w1, "w1", d.w1);
        args.add(b1, "b1", d.hid);
        args.add(w2, "w2", d.hid);
        args.add(b2, "b2", d.lead);
        qmix_check_sizes("qmix_mix", d);
        const at::Device dev = args.on_device_of(agent_q);
        c10::DeviceGuard g(dev);
        Tensor q_tot = new_f32(d.lead, dev);
        check(hpc_rll_qmix_mix_forward(fptr(agent_q), fptr(w1), fptr(b1), fptr(w2), fptr(b2), fmut(q_tot), d.rows,
                                       (int)d.A, (int)d.E, stream_of(dev)),
              "hpc_rll_qmix_mix_forward");
        ctx->save_for_backward({agent_q, w1, b1, w2, b2});
        return q_tot;
    }
    static ag::tensor_list backward(ag::AutogradContext* ctx, ag::tensor_list grads) {
        if (!qmix_needs_any(ctx)) return ag::tensor_list(5);
        const auto saved = ctx->get_saved_variables();
        const at::Device dev = saved[0].device();
        c10::DeviceGuard g(dev);
        Tensor g_rows = grads[0].contiguous();
        req(g_rows, "grad_q_tot", dev);
        return qmix_backward_launch(ctx, undef(), g_rows, undef(), saved, 5);
    }
};

// ====================================================================================================== the TD loss
// (loss (1,), td_error, total_q, target_total_q (...)) of a learner step; the gradient flows from loss to the five online
// operands.  Saves them and the workspace (delta per row).
struct QmixTdFn : public ag::Function<QmixTdFn> {
    static ag::tensor_list forward(ag::AutogradContext* ctx, const Tensor& agent_q, const Tensor& w1, const Tensor& b1,
                                   const Tensor& w2, const Tensor& b2, const Tensor& target_agent_q, const Tensor& target_w1,
                                   const Tensor& target_b1, const Tensor& target_w2, const Tensor& target_b2,
                                   const Tensor& reward, const OptTensor& done, const OptTensor& weight, double gamma,
                                   std::optional<double> scale) {
        const QmixDims d = qmix_dims(agent_q, b1);
        Args args;
        args.add(agent_q, "agent_q", d.qs);
        args.add(w1, "w1", d.w1);
        args.add(b1, "b1", d.hid);
        args.add(w2, "w2", d.hid);
        args.add(b2, "b2", d.lead);
        args.add(target_agent_q, "target_agent_q", d.qs);
        args.add(target_w1, "target_w1", d.w1);
        args.add(target_b1, "target_b1", d.hid);
        args.add(target_w2, "target_w2", d.hid);
        args.add(target_b2, "target_b2", d.lead);
        args.add(reward, "reward", d.lead);
        const Args::Mask dm = args.add_mask(done, "done", d.lead);
        args.add(weight, "weight", d.lead);
        qmix_check_sizes("qmix_td", d);
        const at::Device dev = args.on_device_of(agent_q);
        c10::DeviceGuard g(dev);
        Tensor loss = new_f32({1}, dev);
        Tensor td = new_f32(d.lead, dev), qt = new_f32(d.lead, dev), tq = new_f32(d.lead, dev);
        Tensor ws = new_f32({d.rows > 0 ? hpc_rll_qmix_workspace_floats(d.rows) : 0}, dev);
        check(hpc_rll_qmix_td_forward(fptr(agent_q), fptr(w1), fptr(b1), fptr(w2), fptr(b2), fptr(target_agent_q),
                                      fptr(target_w1), fptr(target_b1), fptr(target_w2), fptr(target_b2), fptr(reward),
                                      dm.ptr, dm.code, fptr(weight), fmut(loss), fmut(td),
                                      fmut(qt), fmut(tq), fmut(ws), d.rows, (int)d.A, (int)d.E, (float)gamma,
                                      loss_scale(scale, d.rows), stream_of(dev)),
              "hpc_rll_qmix_td_forward");
        ctx->save_for_backward({agent_q, w1, b1, w2, b2, ws});
        ctx->mark_non_differentiable({td, qt, tq});
        return {loss, td, qt, tq};
    }
    static ag::tensor_list backward(ag::AutogradContext* ctx, ag::tensor_list grads) {
        if (!qmix_needs_any(ctx)) return ag::tensor_list(15);
        const auto saved = ctx->get_saved_variables();
        const at::Device dev = saved[0].device();
        c10::DeviceGuard g(dev);
        Tensor g_loss = grad1(grads[0], dev, "grad_loss");
        return qmix_backward_launch(ctx, g_loss, undef(), saved[5], saved, 15);
    }
};

}  // namespace
}  // namespace hpc_rll_ext

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    using namespace hpc_rll_ext;
    m.doc() = "hpc_marl (ROCm/HIP): cooperative multi-agent value decomposition over libhpc_rll_hip.so";
    bind_common(m);
    m.def("qmix_mix", applier<QmixMixFn>(&QmixMixFn::forward), py::arg("agent_q"), py::arg("w1"), py::arg("b1"),
          py::arg("w2"), py::arg("b2"),
          "QMIX's monotonic mix q_tot (...) = b2 + sum_e elu(b1_e + sum_a agent_q_a |w1[a,e]|) |w2_e| from agent_q (..., A) and "
          "the raw hypernetwork outputs w1 (..., A, E), b1 (..., E), w2 (..., E), b2 (...); 1 <= A <= 64, 1 <= E <= 256; "
          "differentiable wrt all five");
    m.def("qmix_td", applier<QmixTdFn>(&QmixTdFn::forward), py::arg("agent_q"), py::arg("w1"), py::arg("b1"), py::arg("w2"),
          py::arg("b2"), py::arg("target_agent_q"), py::arg("target_w1"), py::arg("target_b1"), py::arg("target_w2"),
          py::arg("target_b2"), py::arg("reward"), py::arg("done") = py::none(), py::arg("weight") = py::none(),
          py::arg("gamma") = 0.99, py::arg("scale") = py::none(),
          "QMIX's mixed one-step TD loss: (loss (1,), td_error_per_sample, total_q, target_total_q (...)) with "
          "y = reward + gamma (1 - done) target_total_q and loss = scale sum weight (total_q - y)^2; the online and the target "
          "mix take the operands of qmix_mix; differentiable wrt the five online operands; scale = 1/(global rows) for a "
          "sharded caller");
    m.def("qmix_last_config", []() {
        std::vector<int> v(HPC_RLL_QMIX_CONFIG_INTS);
        check(hpc_rll_qmix_last_config(v.data()), "hpc_rll_qmix_last_config");
        return v;
    }, "hpc_rll_qmix_last_config: the dispatch record of the last forward and backward, as the header documents");
}
