// rl_utils_ops.hpp -- what the units of hpc_rl_utils share: the two-phase argument checker, and the launch helpers of
// the categorical-head losses used by rl_utils.cpp (fused autograd ops) and rl_utils_lists.cpp (the reference's L2 list
// functions).
#pragma once
#include "common.hpp"

namespace hpc_rll_ext {

inline const void* vptr(const Tensor& t) { return t.defined() ? t.const_data_ptr() : nullptr; }

inline void check_shape(const Tensor& t, const char* name, at::IntArrayRef shape, at::ScalarType dtype = at::kFloat) {
    TORCH_CHECK(t.defined(), name, ": expected a tensor, got None");
    TORCH_CHECK(t.scalar_type() == dtype, name, ": dtype ", t.scalar_type(), ", expected ", dtype);
    TORCH_CHECK(t.sizes() == shape, name, ": shape ", t.sizes(), ", expected ", shape);
}

inline int mask_code(const Tensor& m, const char* name) {
    const at::ScalarType s = m.scalar_type();
    if (s == at::kBool || s == at::kByte) return HPC_RLL_MASK_U8;
    if (s == at::kFloat) return HPC_RLL_MASK_F32;
    TORCH_CHECK(false, name, ": dtype ", s, " is not accepted; expected bool, uint8 or float32");
    return -1;
}

// The argument checks of the ops that name a wrong argument even on host tensors.  They run in two phases: dtype and
// shape of every tensor first, GPU / contiguous / device afterwards.  An op declares each tensor ONCE, with add(): the
// dtype and shape messages are raised there, in declaration order.  One later on_device_of(lead) raises req()'s
// messages for the same tensors in the same order, against the device of `lead`, and returns that device.  Checks of
// the op's own (a count, a range) stand between the two phases, where they are to be raised.  A fixed-size value on the
// stack, nothing is allocated; it keeps pointers, so the declared tensors outlive it.
class Args {
  public:
    void add(const Tensor& t, const char* name, at::IntArrayRef shape, at::ScalarType dtype = at::kFloat) {
        check_shape(t, name, shape, dtype);
        keep(t, name);
    }
    void add(const OptTensor& t, const char* name, at::IntArrayRef shape, at::ScalarType dtype = at::kFloat) {   // None passes
        if (has(t)) add(*t, name, shape, dtype);
    }
    // A done mask of `shape`: bool, uint8 or float32, None passes.  What the kernels take: the dtype code and the data
    // (NULL when absent).  `note` ends the shape message.
    struct Mask { int code; const void* ptr; };
    Mask add_mask(const OptTensor& m, const char* name, at::IntArrayRef shape, const char* note = "") {
        if (!has(m)) return {HPC_RLL_MASK_U8, nullptr};
        const int code = mask_code(*m, name);
        TORCH_CHECK(m->sizes() == shape, name, ": shape ", m->sizes(), ", expected ", shape, note);
        keep(*m, name);
        return {code, vptr(*m)};
    }
    at::Device on_device_of(const Tensor& lead) const {
        const at::Device dev = lead.device();
        for (int i = 0; i < n_; ++i) req(*items_[i].t, items_[i].name, dev, items_[i].t->scalar_type());
        return dev;
    }

  private:
    struct Item { const Tensor* t; const char* name; };
    void keep(const Tensor& t, const char* name) {
        TORCH_INTERNAL_ASSERT(n_ < (int)items_.size(), "Args: more tensors than it holds");
        items_[n_++] = {&t, name};
    }
    std::array<Item, 16> items_;   // (qmix_td declares thirteen)
    int n_ = 0;
};

struct VtraceDims { int64_t T, B, N; at::Device dev; };
VtraceDims vtrace_check(const Tensor& target, const Tensor& behaviour, const Tensor& action, const Tensor& value,
                        const Tensor& reward, const OptTensor& weight);
Tensor vtrace_workspace(int64_t T, int64_t B, const at::Device& dev);
void vtrace_forward_launch(const VtraceDims& d, const Tensor& target, const Tensor& behaviour, const Tensor& action,
                           const Tensor& value, const Tensor& reward, const OptTensor& weight, const Tensor& losses,
                           const Tensor& ws, double gamma, double lambda, double rho_clip, double c_clip,
                           double rho_pg_clip, std::optional<double> scale);
void vtrace_backward_launch(const Tensor& g_pg, const Tensor& g_v, const Tensor& g_ent, const Tensor& target,
                            const Tensor& action, const Tensor& ws, const Tensor& grad_target, const Tensor& grad_value);

struct UpgoDims { int64_t T, B, N; at::Device dev; };
UpgoDims upgo_check(const Tensor& target, const Tensor& rho, const Tensor& action, const Tensor& reward,
                    const Tensor& value);
Tensor upgo_workspace(int64_t T, int64_t B, const at::Device& dev);
void upgo_forward_launch(const UpgoDims& d, const Tensor& target, const Tensor& rho, const Tensor& action,
                         const Tensor& reward, const Tensor& value, const Tensor& loss, const Tensor& ws,
                         std::optional<double> scale);
void upgo_backward_launch(const Tensor& g, const Tensor& target, const Tensor& action, const Tensor& ws,
                          const Tensor& grad_target);

struct PpoDims { int64_t B, N; at::Device dev; };
PpoDims ppo_check(const Tensor& ln, const Tensor& lo, const Tensor& action, const Tensor& vn, const Tensor& vo,
                  const Tensor& adv, const Tensor& ret, const OptTensor& weight);
Tensor ppo_workspace(int64_t B, const at::Device& dev);
void ppo_forward_launch(const PpoDims& d, const Tensor& ln, const Tensor& lo, const Tensor& action, const Tensor& vn,
                        const Tensor& vo, const Tensor& adv, const Tensor& ret, const OptTensor& weight,
                        const Tensor& out5, const Tensor& ws, bool use_value_clip, double clip_ratio, double dual_clip,
                        std::optional<double> scale);
void ppo_backward_launch(const Tensor& g_p, const Tensor& g_v, const Tensor& g_e, const Tensor& ln, const Tensor& action,
                         const Tensor& ws, const Tensor& grad_logits, const Tensor& grad_value);

// PPO with a diagonal-Gaussian head (no reference counterpart, hence no list form)
struct PpoContinuousDims { int64_t B, A; at::Device dev; };
PpoContinuousDims ppo_continuous_check(const Tensor& mu_new, const Tensor& sigma_new, const Tensor& mu_old,
                                       const Tensor& sigma_old, const Tensor& action, const Tensor& vn, const Tensor& vo,
                                       const Tensor& adv, const Tensor& ret, const OptTensor& weight);

}  // namespace hpc_rll_ext
