// hpc_replay -- the prioritized-replay index (no reference counterpart): a sum tree and a min tree of fan-out 64 in one
// device buffer, with a scattered update, a rebuild and a proportional sampler (hpc_rll_per_*; include/hpc_rll_hip.h has the
// semantics).  HOST-ONLY C++ like the other five modules (common.hpp): it validates tensors, takes outputs from torch's caching
// allocator and calls the C ABI on torch's current stream.  Nothing here synchronises with the host and nothing is
// differentiable.  The state is an int32 tensor, so that Module.half() / .double() leave its bits alone; its length alone
// gives the capacity (hpc_rll_per_capacity_of).
#include "rl_utils_ops.hpp"

namespace hpc_rll_ext {
namespace {

Tensor new_of(at::IntArrayRef shape, const at::Device& dev, at::ScalarType dtype) {
    return at::empty(shape, at::TensorOptions().dtype(dtype).device(dev));
}

int64_t capacity_arg(int64_t capacity) {
    TORCH_CHECK(capacity >= 1, "capacity: expected at least 1, got ", capacity);
    TORCH_CHECK(capacity <= HPC_RLL_PER_MAX_CAPACITY, "capacity: at most ", (int64_t)HPC_RLL_PER_MAX_CAPACITY,
                " (four levels of 64) are implemented, got ", capacity);
    return capacity;
}

// dtype and shape of the state, and the capacity its length stands for
int64_t capacity_of(const Tensor& state) {
    TORCH_CHECK(state.defined(), "state: expected a tensor, got None");
    TORCH_CHECK(state.scalar_type() == at::kInt, "state: dtype ", state.scalar_type(), ", expected ", at::kInt);
    TORCH_CHECK(state.dim() == 1, "state: shape ", state.sizes(), ", expected (words,) as per_init returns it");
    const int64_t capacity = hpc_rll_per_capacity_of(4 * state.numel());
    TORCH_CHECK(capacity >= 1, "state: ", state.numel(), " words are the state of no capacity (per_state_words)");
    return capacity;
}

void* state_ptr(const Tensor& state) { return (void*)state.data_ptr<int32_t>(); }

void check_exponent(const char* name, double v) { TORCH_CHECK(v >= 0.0, name, ": expected a value >= 0, got ", v); }

int64_t per_state_words(int64_t capacity) { return hpc_rll_per_state_bytes(capacity_arg(capacity)) / 4; }

std::vector<int64_t> per_layout(int64_t capacity) {
    std::vector<int64_t> out(HPC_RLL_PER_LAYOUT_INTS);
    check(hpc_rll_per_layout(capacity_arg(capacity), out.data()), "hpc_rll_per_layout");
    return out;
}

int64_t per_capacity(const Tensor& state) { return capacity_of(state); }

void per_init(const Tensor& state) {
    const int64_t capacity = capacity_of(state);
    req(state, "state", at::kInt);
    c10::DeviceGuard g(state.device());
    check(hpc_rll_per_init(state_ptr(state), capacity, stream_of(state.device())), "hpc_rll_per_init");
}

void per_update(const Tensor& state, const Tensor& idx, const OptTensor& priority, double alpha, double eps) {
    const int64_t capacity = capacity_of(state);
    TORCH_CHECK(idx.defined(), "idx: expected a tensor, got None");
    TORCH_CHECK(idx.dim() == 1, "idx: shape ", idx.sizes(), ", expected (M,)");
    Args args;
    args.add(idx, "idx", idx.sizes(), at::kLong);
    args.add(priority, "priority", idx.sizes());
    check_exponent("alpha", alpha);
    check_exponent("eps", eps);
    req(state, "state", at::kInt);
    const at::Device dev = args.on_device_of(state);
    c10::DeviceGuard g(dev);
    check(hpc_rll_per_update(state_ptr(state), capacity, iptr(idx), fptr(priority), idx.numel(), (float)alpha, (float)eps,
                             stream_of(dev)),
          "hpc_rll_per_update");
}

void per_rebuild(const Tensor& state, const Tensor& priorities, double alpha, double eps) {
    const int64_t capacity = capacity_of(state);
    Args args;
    args.add(priorities, "priorities", {capacity});
    check_exponent("alpha", alpha);
    check_exponent("eps", eps);
    req(state, "state", at::kInt);
    const at::Device dev = args.on_device_of(state);
    c10::DeviceGuard g(dev);
    check(hpc_rll_per_rebuild(state_ptr(state), capacity, fptr(priorities), (float)alpha, (float)eps, stream_of(dev)),
          "hpc_rll_per_rebuild");
}

// [idx (B,) int64, weight (B,), prob (B,)] for the uniforms u (B,)
std::vector<Tensor> per_sample(const Tensor& state, const Tensor& u, double beta, int64_t size, const OptTensor& size_tensor,
                               bool stratified, int64_t normalize) {
    const int64_t capacity = capacity_of(state);
    TORCH_CHECK(u.defined(), "u: expected a tensor, got None");
    TORCH_CHECK(u.dim() == 1, "u: shape ", u.sizes(), ", expected (B,)");
    Args args;
    args.add(u, "u", u.sizes());
    args.add(size_tensor, "size", {1}, at::kLong);
    check_exponent("beta", beta);
    TORCH_CHECK(normalize >= HPC_RLL_PER_NORM_NONE && normalize <= HPC_RLL_PER_NORM_BATCH, "normalize: unknown mode ", normalize);
    TORCH_CHECK(has(size_tensor) || size >= 1, "size: expected at least 1 stored transition, got ", size);
    req(state, "state", at::kInt);
    const at::Device dev = args.on_device_of(state);
    c10::DeviceGuard g(dev);
    const int64_t B = u.numel();
    Tensor idx = new_of({B}, dev, at::kLong), weight = new_f32({B}, dev), prob = new_f32({B}, dev);
    check(hpc_rll_per_sample(state_ptr(state), capacity, fptr(u), idx.data_ptr<int64_t>(), fmut(weight), fmut(prob), B,
                             stratified ? 1 : 0, (int)normalize, (float)beta, has(size_tensor) ? 1 : size,
                             has(size_tensor) ? iptr(*size_tensor) : nullptr, stream_of(dev)),
          "hpc_rll_per_sample");
    return {idx, weight, prob};
}

}  // namespace
}  // namespace hpc_rll_ext

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    using namespace hpc_rll_ext;
    m.doc() = "hpc_replay (ROCm/HIP): the prioritized-replay index (sum tree and min tree of fan-out 64) over libhpc_rll_hip.so";
    bind_common(m);
    m.def("per_state_words", &per_state_words, py::arg("capacity"),
          "the length of the int32 state tensor of an index over capacity leaves, 1 <= capacity <= 2**24");
    m.def("per_layout", &per_layout, py::arg("capacity"),
          "hpc_rll_per_layout: depth, words, then (offset, length) in words of levels 0..4 of the sum tree, of the min tree, of "
          "the scalars and of the stamps, as the header documents");
    m.def("per_capacity", &per_capacity, py::arg("state"), "the capacity a state tensor was made for");
    m.def("per_init", &per_init, py::arg("state"), "every leaf unwritten, max_priority = 1; one launch");
    m.def("per_update", &per_update, py::arg("state"), py::arg("idx"), py::arg("priority") = py::none(), py::arg("alpha") = 0.6,
          py::arg("eps") = 1e-6,
          "leaf idx[k] = (priority[k] + eps)^alpha for idx (M,) int64 and priority (M,), or the leaf of max_priority for None.  "
          "The last of several equal indices wins, indices outside [0, capacity) are skipped, a negative, NaN or infinite "
          "priority counts as max_priority; in place, 2 + depth launches");
    m.def("per_rebuild", &per_rebuild, py::arg("state"), py::arg("priorities"), py::arg("alpha") = 0.6, py::arg("eps") = 1e-6,
          "the whole index from priorities (capacity,); a negative, NaN or infinite entry leaves its slot unwritten");
    m.def("per_sample", &per_sample, py::arg("state"), py::arg("u"), py::arg("beta"), py::arg("size") = 1,
          py::arg("size_tensor") = py::none(), py::arg("stratified") = true, py::arg("normalize") = 1,
          "[idx (B,) int64, weight (B,), prob (B,)] for the uniforms u (B,): mass ((k + u_k) / B) total when stratified, u_k "
          "total otherwise; prob = leaf / total, weight = (size prob)^-beta over 0 nothing, 1 the buffer's largest weight, 2 the "
          "batch's.  size_tensor (1,) int64 on the device replaces size.  idx = -1 and weight = 0 for an empty index");
    m.def("per_last_config", []() {
        std::vector<int> v(HPC_RLL_PER_CONFIG_INTS);
        check(hpc_rll_per_last_config(v.data()), "hpc_rll_per_last_config");
        return v;
    }, "hpc_rll_per_last_config: the dispatch record of the last update (or rebuild) and the last sample, as the header documents");
}
