#include "common.h"

namespace {

// --------------------------------------------------------------------------------- Adam --
// Builds the device descriptor table for a fixed list of tensors (done once).
std::vector<torch::Tensor> adam_build(std::vector<torch::Tensor> params, std::vector<torch::Tensor> grads,
                                      std::vector<torch::Tensor> m, std::vector<torch::Tensor> v,
                                      std::vector<c10::optional<torch::Tensor>> shadows) {
  const size_t n = params.size();
  TORCH_CHECK(grads.size() == n && m.size() == n && v.size() == n && shadows.size() == n, "adam_build: list sizes");
  const int db = dpfs_adam_desc_bytes();
  TORCH_CHECK(db == 48, "unexpected AdamTensor layout");
  std::vector<int64_t> desc(n * 6);
  std::vector<int32_t> chunks;
  const int64_t C = dpfs_adam_chunk();
  for (size_t i = 0; i < n; ++i) {
    auto chk = [&](const torch::Tensor& t, const char* nm) {
      TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kFloat32 && t.is_contiguous() &&
                      t.numel() == params[i].numel(),
                  "adam_build: ", nm, " must be contiguous fp32 matching the param");
    };
    chk(params[i], "param");
    chk(grads[i], "grad");
    chk(m[i], "exp_avg");
    chk(v[i], "exp_avg_sq");
    int64_t sh = 0;
    if (shadows[i].has_value() && shadows[i]->defined()) {
      TORCH_CHECK(shadows[i]->scalar_type() == torch::kBFloat16 && shadows[i]->is_contiguous() &&
                      shadows[i]->numel() == params[i].numel(),
                  "adam_build: shadow must be contiguous bf16");
      sh = (int64_t)shadows[i]->data_ptr();
    }
    desc[i * 6 + 0] = (int64_t)params[i].data_ptr();
    desc[i * 6 + 1] = (int64_t)grads[i].data_ptr();
    desc[i * 6 + 2] = (int64_t)m[i].data_ptr();
    desc[i * 6 + 3] = (int64_t)v[i].data_ptr();
    desc[i * 6 + 4] = sh;
    desc[i * 6 + 5] = params[i].numel();
    const int64_t nc = (params[i].numel() + C - 1) / C;
    for (int64_t c = 0; c < nc; ++c) {
      chunks.push_back((int32_t)i);
      chunks.push_back((int32_t)c);
    }
  }
  auto dev = params.empty() ? torch::Device(torch::kCUDA) : params[0].device();
  // Pinned staging + async copies: a pageable H2D copy would block the host until the GPU
  // has drained every queued kernel (the whole backward), idling the GPU while the host then
  // enqueues the optimizer and the next step.  The caching host allocator keeps the pinned
  // blocks alive until their copies have run.
  auto d = torch::from_blob(desc.data(), {(int64_t)desc.size()}, torch::kInt64).pin_memory().to(dev, true);
  auto c = torch::from_blob(chunks.data(), {(int64_t)chunks.size()}, torch::kInt32).pin_memory().to(dev, true);
  return {d, c};
}

// Rewrite the gradient pointers of a descriptor table built by adam_build (same params,
// same order; only the gradient tensors changed) without a host -> device copy.
void adam_patch_grads(torch::Tensor desc, std::vector<torch::Tensor> grads) {
  TORCH_CHECK(desc.is_cuda() && desc.scalar_type() == torch::kInt64 && desc.numel() == (int64_t)grads.size() * 6,
              "adam_patch_grads: descriptor table / grad list mismatch");
  std::vector<long long> ptrs(grads.size());
  for (size_t i = 0; i < grads.size(); ++i) {
    TORCH_CHECK(grads[i].is_cuda() && grads[i].scalar_type() == torch::kFloat32 && grads[i].is_contiguous(),
                "adam_patch_grads: grads must be contiguous fp32 on the device");
    ptrs[i] = (long long)grads[i].data_ptr();
  }
  const at::DeviceGuard g(desc.device());
  dpfs_adam_patch_grads(desc.data_ptr(), ptrs.data(), (int)ptrs.size(), stream());
}

void adam_step(torch::Tensor desc, torch::Tensor chunks, double lr, double b1, double b2, double eps, double wd,
               int64_t step, double gscale, c10::optional<torch::Tensor> dscale) {
  TORCH_CHECK(desc.is_cuda() && chunks.is_cuda(), "adam_step: tables must be on the device");
  const double bc1 = 1.0 - std::pow(b1, (double)step);
  const double bc2 = 1.0 - std::pow(b2, (double)step);
  const float* ds = nullptr;
  if (dscale.has_value() && dscale->defined()) {
    TORCH_CHECK(dscale->scalar_type() == torch::kFloat32 && dscale->numel() == 1, "adam_step: dscale fp32 scalar");
    ds = dscale->data_ptr<float>();
  }
  const at::DeviceGuard g(desc.device());
  dpfs_adam_step(desc.data_ptr(), chunks.data_ptr<int32_t>(), (int)(chunks.numel() / 2), (float)lr, (float)b1,
                 (float)b2, (float)eps, (float)wd, (float)bc1, (float)std::sqrt(bc2), (float)gscale, ds, stream());
}

torch::Tensor grad_sumsq(torch::Tensor desc, torch::Tensor chunks) {
  const at::DeviceGuard g(desc.device());
  const int n = (int)(chunks.numel() / 2);
  auto partial = torch::empty({n}, desc.options().dtype(torch::kFloat32));
  dpfs_grad_sumsq(desc.data_ptr(), chunks.data_ptr<int32_t>(), n, partial.data_ptr<float>(), stream());
  return partial.sum();
}

}  // namespace

void bind_optim(py::module_& m) {
  m.def("adam_build", &adam_build);
  m.def("adam_step", &adam_step, py::arg("desc"), py::arg("chunks"), py::arg("lr"), py::arg("beta1"),
        py::arg("beta2"), py::arg("eps"), py::arg("weight_decay"), py::arg("step"), py::arg("grad_scale") = 1.0,
        py::arg("dscale") = py::none());
  m.def("grad_sumsq", &grad_sumsq);
  m.def("adam_patch_grads", &adam_patch_grads, py::arg("desc"), py::arg("grads"));
}
