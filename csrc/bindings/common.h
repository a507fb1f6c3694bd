// Python bindings of the gfx950 kernels: torch tensors in, kernels launched on the current
// HIP stream (so they interleave correctly with RCCL collectives issued by
// torch.distributed on its own streams and with hipGraph capture).
//
// Every function validates device/dtype/shape/stride assumptions of its kernel on the host
// BEFORE launching (an out-of-bounds wave can reset the whole node), allocates outputs from
// the PyTorch caching allocator, and mirrors the signature of the pure-PyTorch oracle of
// the same name in distributed_pytorch_from_scratch_amd/ops/reference.py.
//
// One file per area (gemm, norm_elementwise, attention, embedding_ce, optim, decode, comm), each
// exporting bind_<area>(); module.cpp registers them.  This header: what they share.
#pragma once

#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <ATen/DeviceGuard.h>
#include <hip/hip_runtime.h>

#include <vector>

#include "../dpfs_api.h"

void bind_gemm(py::module_& m);
void bind_norm_elementwise(py::module_& m);
void bind_attention(py::module_& m);
void bind_embedding_ce(py::module_& m);
void bind_optim(py::module_& m);
void bind_decode(py::module_& m);
void bind_comm(py::module_& m);

// norm_elementwise.cpp (the NT GEMM runs it where the RoPE epilogue does not apply)
torch::Tensor rope_(torch::Tensor qkv, torch::Tensor positions, torch::Tensor table, int64_t n_rot_heads,
                    int64_t head_dim, bool inverse);

inline hipStream_t stream() { return c10::hip::getCurrentHIPStream().stream(); }

inline int dcode(const torch::Tensor& t) {
  if (t.scalar_type() == torch::kBFloat16) return 1;
  if (t.scalar_type() == torch::kFloat32) return 0;
  TORCH_CHECK(false, "unsupported dtype ", t.scalar_type(), " (bf16 / fp32 only)");
  return -1;
}

inline void check_cuda(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a HIP (cuda) tensor");
}

inline void check_rowmajor(const torch::Tensor& t, const char* name) {
  check_cuda(t, name);
  TORCH_CHECK(t.dim() == 2, name, " must be 2-D, got ", t.dim(), "-D");
  TORCH_CHECK(t.stride(1) == 1, name, " must have unit inner stride");
}

inline const float* opt_f32(const c10::optional<torch::Tensor>& t, int64_t n, const char* name) {
  if (!t.has_value() || !t->defined()) return nullptr;
  check_cuda(*t, name);
  TORCH_CHECK(t->scalar_type() == torch::kFloat32 && t->is_contiguous() && t->numel() == n, name,
              " must be a contiguous fp32 vector of length ", n);
  return t->data_ptr<float>();
}

// The optional bias-gradient output of a backward op: null when absent.
inline float* dbias_out(const c10::optional<torch::Tensor>& db, int64_t n, const char* what) {
  if (!db.has_value() || !db->defined()) return nullptr;
  TORCH_CHECK(db->is_cuda() && db->scalar_type() == torch::kFloat32 && db->is_contiguous() && db->numel() == n, what,
              ": dbias must be contiguous fp32 [", n, "]");
  return db->data_ptr<float>();
}
