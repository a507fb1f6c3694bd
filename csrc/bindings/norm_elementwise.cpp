#include "common.h"

namespace {

torch::Tensor bias_grad(torch::Tensor dy) {
  check_rowmajor(dy, "dy");
  TORCH_CHECK(dy.is_contiguous(), "bias_grad: dy must be contiguous");
  const int64_t M = dy.size(0), N = dy.size(1);
  const int vec = dcode(dy) == 1 ? 8 : 4;
  TORCH_CHECK(N % vec == 0, "bias_grad: N must be a multiple of ", vec);
  const at::DeviceGuard g(dy.device());
  auto out = torch::empty({N}, dy.options().dtype(torch::kFloat32));
  if (M == 0) return out.zero_();
  auto ws = torch::empty({(int64_t)dpfs_colsum_ws((int)M, (int)N)}, out.options());
  dpfs_bias_grad(dcode(dy), dy.data_ptr(), out.data_ptr<float>(), ws.data_ptr<float>(), (int)M, (int)N, stream());
  return out;
}

torch::Tensor add_bias_(torch::Tensor y, torch::Tensor bias) {
  check_rowmajor(y, "y");
  TORCH_CHECK(y.is_contiguous(), "add_bias_: y must be contiguous");
  const int64_t M = y.size(0), N = y.size(1);
  const int vec = dcode(y) == 1 ? 8 : 4;
  TORCH_CHECK(N % vec == 0, "add_bias_: N must be a multiple of ", vec);
  const float* bp = opt_f32(bias, N, "bias");
  const at::DeviceGuard g(y.device());
  if (M) dpfs_bias_residual(dcode(y), y.data_ptr(), bp, nullptr, y.data_ptr(), (int)M, (int)N, stream());
  return y;
}

// out = residual + y (+ bias)
torch::Tensor bias_residual(torch::Tensor y, c10::optional<torch::Tensor> bias, torch::Tensor residual) {
  check_rowmajor(y, "y");
  TORCH_CHECK(y.is_contiguous() && residual.is_contiguous() && residual.sizes() == y.sizes() &&
                  residual.scalar_type() == y.scalar_type(),
              "bias_residual: y and residual must be contiguous, same shape/dtype");
  const int64_t M = y.size(0), N = y.size(1);
  const int vec = dcode(y) == 1 ? 8 : 4;
  TORCH_CHECK(N % vec == 0, "bias_residual: N must be a multiple of ", vec);
  const at::DeviceGuard g(y.device());
  auto out = torch::empty_like(y);
  if (M) dpfs_bias_residual(dcode(y), y.data_ptr(), opt_f32(bias, N, "bias"), residual.data_ptr(), out.data_ptr(),
                            (int)M, (int)N, stream());
  return out;
}

// ------------------------------------------------------------------------------- norms --
int check_norm_x(const torch::Tensor& x, const torch::Tensor& w) {
  check_rowmajor(x, "x");
  TORCH_CHECK(x.is_contiguous(), "norm: x must be contiguous");
  const int dt = dcode(x);
  const int64_t D = x.size(1);
  TORCH_CHECK(D % (dt == 1 ? 8 : 4) == 0 && D <= 32 * 64 * (dt == 1 ? 8 : 4), "norm: unsupported hidden size ", D);
  TORCH_CHECK(w.is_cuda() && w.scalar_type() == torch::kFloat32 && w.is_contiguous() && w.numel() == D,
              "norm: weight must be contiguous fp32 [D]");
  return dt;
}

std::vector<torch::Tensor> rmsnorm_fwd(torch::Tensor x, torch::Tensor w, double eps) {
  const int dt = check_norm_x(x, w);
  const at::DeviceGuard g(x.device());
  const int64_t M = x.size(0), D = x.size(1);
  auto y = torch::empty_like(x);
  auto rstd = torch::empty({M}, x.options().dtype(torch::kFloat32));
  if (M) dpfs_rmsnorm_fwd(dt, x.data_ptr(), w.data_ptr<float>(), y.data_ptr(), rstd.data_ptr<float>(), (int)M, (int)D,
                          (float)eps, stream());
  return {y, rstd};
}

// (x = y + bias + res, RMSNorm(x), rstd) in one pass: the residual epilogue of a row-parallel
// projection fused into the next norm.
std::vector<torch::Tensor> add_rmsnorm_fwd(torch::Tensor y, c10::optional<torch::Tensor> bias, torch::Tensor res,
                                           torch::Tensor w, double eps) {
  const int dt = check_norm_x(res, w);
  TORCH_CHECK(y.sizes() == res.sizes() && y.is_contiguous() && y.scalar_type() == res.scalar_type(),
              "add_rmsnorm_fwd: y must match res");
  const at::DeviceGuard g(res.device());
  const int64_t M = res.size(0), D = res.size(1);
  const float* bp = opt_f32(bias, D, "bias");
  auto x = torch::empty_like(res);
  auto h = torch::empty_like(res);
  auto rstd = torch::empty({M}, res.options().dtype(torch::kFloat32));
  if (M)
    dpfs_add_rmsnorm_fwd(dt, y.data_ptr(), bp, res.data_ptr(), w.data_ptr<float>(), x.data_ptr(), h.data_ptr(),
                         rstd.data_ptr<float>(), (int)M, (int)D, (float)eps, stream());
  return {x, h, rstd};
}

// dx = RMSNorm'(dy) (+ dres); with `dbias` also the column sums of dx (the bias grad of the
// projection whose output gradient dx is), from the same pass.
std::vector<torch::Tensor> rmsnorm_bwd(torch::Tensor dy, torch::Tensor x, torch::Tensor w, torch::Tensor rstd,
                                       c10::optional<torch::Tensor> dres, c10::optional<torch::Tensor> dbias,
                                       c10::optional<torch::Tensor> dw_out) {
  const int dt = check_norm_x(x, w);
  TORCH_CHECK(dy.sizes() == x.sizes() && dy.is_contiguous() && dy.scalar_type() == x.scalar_type(), "rmsnorm_bwd: dy");
  const void* rp = nullptr;
  if (dres.has_value() && dres->defined()) {
    TORCH_CHECK(dres->sizes() == x.sizes() && dres->is_contiguous() && dres->scalar_type() == x.scalar_type(),
                "rmsnorm_bwd: dres must match x");
    rp = dres->data_ptr();
  }
  const at::DeviceGuard g(x.device());
  const int64_t M = x.size(0), D = x.size(1);
  float* db = dbias_out(dbias, x.size(1), "rmsnorm_bwd");
  auto dx = torch::empty_like(x);
  torch::Tensor dw;
  if (dw_out.has_value() && dw_out->defined()) {   // the weight gradient straight into its slot
    dw = *dw_out;
    TORCH_CHECK(dw.scalar_type() == torch::kFloat32 && dw.is_contiguous() && dw.numel() == D &&
                    dw.device() == x.device(),
                "rmsnorm_bwd: dw_out must be contiguous fp32 [D] on the device of x");
  } else {
    dw = torch::empty({D}, w.options());
  }
  if (M == 0) {
    if (db) dbias->zero_();
    return {dx, dw.zero_()};
  }
  const int mode = db ? 2 : 0;
  const int G = dpfs_norm_bwd_grid((int)M);
  auto ws = torch::empty({(int64_t)dpfs_norm_bwd_ws(mode, (int)M, (int)D)}, w.options());
  float* pw = ws.data_ptr<float>();
  dpfs_norm_bwd(mode, dt, dy.data_ptr(), x.data_ptr(), w.data_ptr<float>(), nullptr, rstd.data_ptr<float>(), rp,
                dx.data_ptr(), dw.data_ptr<float>(), db, pw, db ? pw + (int64_t)G * D : nullptr, (int)M, (int)D,
                stream());
  return {dx, dw};
}

std::vector<torch::Tensor> layernorm_fwd(torch::Tensor x, torch::Tensor w, torch::Tensor b, double eps) {
  const int dt = check_norm_x(x, w);
  TORCH_CHECK(b.is_cuda() && b.scalar_type() == torch::kFloat32 && b.numel() == x.size(1), "layernorm: bias");
  const at::DeviceGuard g(x.device());
  const int64_t M = x.size(0), D = x.size(1);
  auto y = torch::empty_like(x);
  auto mean = torch::empty({M}, x.options().dtype(torch::kFloat32));
  auto rstd = torch::empty({M}, x.options().dtype(torch::kFloat32));
  if (M) dpfs_layernorm_fwd(dt, x.data_ptr(), w.data_ptr<float>(), b.data_ptr<float>(), y.data_ptr(),
                            mean.data_ptr<float>(), rstd.data_ptr<float>(), (int)M, (int)D, (float)eps, stream());
  return {y, mean, rstd};
}

std::vector<torch::Tensor> layernorm_bwd(torch::Tensor dy, torch::Tensor x, torch::Tensor w, torch::Tensor mean,
                                         torch::Tensor rstd) {
  const int dt = check_norm_x(x, w);
  TORCH_CHECK(dy.sizes() == x.sizes() && dy.is_contiguous() && dy.scalar_type() == x.scalar_type(),
              "layernorm_bwd: dy");
  const at::DeviceGuard g(x.device());
  const int64_t M = x.size(0), D = x.size(1);
  auto dx = torch::empty_like(x);
  auto dw = torch::empty({D}, w.options());
  auto db = torch::empty({D}, w.options());
  if (M == 0) return {dx, dw.zero_(), db.zero_()};
  const int64_t G = dpfs_norm_bwd_grid((int)M);
  auto ws = torch::empty({(int64_t)dpfs_norm_bwd_ws(1, (int)M, (int)D)}, w.options());
  dpfs_norm_bwd(1, dt, dy.data_ptr(), x.data_ptr(), w.data_ptr<float>(), mean.data_ptr<float>(),
                rstd.data_ptr<float>(), nullptr, dx.data_ptr(), dw.data_ptr<float>(), db.data_ptr<float>(),
                ws.data_ptr<float>(), ws.data_ptr<float>() + G * D, (int)M, (int)D, stream());
  return {dx, dw, db};
}

// ------------------------------------------------------------------------ elementwise --
// h = silu(gate) * up; `perm`: gu in the interleaved layout of the fused gate|up epilogue.
torch::Tensor swiglu_fwd(torch::Tensor gu, bool perm) {
  check_rowmajor(gu, "gu");
  TORCH_CHECK(gu.is_contiguous(), "swiglu: gu must be contiguous");
  const int dt = dcode(gu);
  const int64_t M = gu.size(0), F = gu.size(1) / 2;
  TORCH_CHECK(gu.size(1) % 2 == 0 && F % (dt == 1 ? 8 : 4) == 0, "swiglu: F must be a multiple of the vector width");
  TORCH_CHECK(!perm || F % 64 == 0, "swiglu: the interleaved layout needs F % 64 == 0");
  const at::DeviceGuard g(gu.device());
  auto h = torch::empty({M, F}, gu.options());
  if (M) dpfs_swiglu_fwd(dt, gu.data_ptr(), h.data_ptr(), (int)M, (int)F, perm ? 1 : 0, stream());
  return h;
}

// dgu = SwiGLU'(gu) * dh; with `dbias` the gate|up bias gradient (column sums of dgu) is
// written there by the same pass.
torch::Tensor swiglu_bwd(torch::Tensor dh, torch::Tensor gu, c10::optional<torch::Tensor> dbias, bool perm) {
  check_rowmajor(gu, "gu");
  const int dt = dcode(gu);
  const int64_t M = gu.size(0), F = gu.size(1) / 2;
  TORCH_CHECK(dh.is_contiguous() && dh.size(0) == M && dh.size(1) == F && dh.scalar_type() == gu.scalar_type(),
              "swiglu_bwd: dh");
  TORCH_CHECK(F % (dt == 1 ? 8 : 4) == 0, "swiglu: F must be a multiple of the vector width");
  TORCH_CHECK(!perm || F % 64 == 0, "swiglu: the interleaved layout needs F % 64 == 0");
  const at::DeviceGuard g(gu.device());
  auto dgu = torch::empty_like(gu);
  float* db = dbias_out(dbias, 2 * F, "swiglu_bwd");
  if (db && M == 0) dbias->zero_();
  if (M == 0) return dgu;
  if (db) {
    TORCH_CHECK(gu.is_contiguous(), "swiglu_bwd: gu must be contiguous");
    const long long wsn = dpfs_swiglu_bwd_dbias_ws((int)M, (int)F);
    auto ws = torch::empty({std::max<long long>(wsn, 1)}, gu.options().dtype(torch::kFloat32));
    dpfs_swiglu_bwd_dbias(dt, dh.data_ptr(), gu.data_ptr(), dgu.data_ptr(), db, ws.data_ptr<float>(), (int)M, (int)F,
                          perm ? 1 : 0, stream());
  } else {
    dpfs_swiglu_bwd(dt, dh.data_ptr(), gu.data_ptr(), dgu.data_ptr(), (int)M, (int)F, perm ? 1 : 0, stream());
  }
  return dgu;
}

}  // namespace

torch::Tensor rope_(torch::Tensor qkv, torch::Tensor positions, torch::Tensor table, int64_t n_rot_heads,
                    int64_t head_dim, bool inverse) {
  check_rowmajor(qkv, "qkv");
  TORCH_CHECK(positions.is_cuda() && positions.scalar_type() == torch::kInt64 && positions.is_contiguous() &&
                  positions.numel() == qkv.size(0),
              "rope: positions must be contiguous int64 [M]");
  TORCH_CHECK(table.is_cuda() && table.scalar_type() == torch::kFloat32 && table.is_contiguous() &&
                  table.dim() == 2 && table.size(1) == head_dim,
              "rope: table must be fp32 [maxlen, head_dim]");
  TORCH_CHECK(head_dim % 8 == 0, "rope: head_dim must be a multiple of 8");
  TORCH_CHECK(n_rot_heads * head_dim <= qkv.size(1), "rope: too many heads for the row");
  const at::DeviceGuard g(qkv.device());
  const int64_t M = qkv.size(0);
  if (M) dpfs_rope(dcode(qkv), qkv.data_ptr(), positions.data_ptr<int64_t>(), table.data_ptr<float>(), (int)M,
                   (int)qkv.stride(0), (int)n_rot_heads, (int)head_dim, inverse ? 1 : 0, stream());
  return qkv;
}

void bind_norm_elementwise(py::module_& m) {
  m.def("bias_grad", &bias_grad);
  m.def("add_bias_", &add_bias_);
  m.def("bias_residual", &bias_residual);
  m.def("rmsnorm_fwd", &rmsnorm_fwd);
  m.def("add_rmsnorm_fwd", &add_rmsnorm_fwd, py::arg("y"), py::arg("bias"), py::arg("res"), py::arg("w"),
        py::arg("eps"));
  m.def("rmsnorm_bwd", &rmsnorm_bwd, py::arg("dy"), py::arg("x"), py::arg("w"), py::arg("rstd"),
        py::arg("dres") = py::none(), py::arg("dbias") = py::none(), py::arg("dw_out") = py::none());
  m.def("layernorm_fwd", &layernorm_fwd);
  m.def("layernorm_bwd", &layernorm_bwd);
  m.def("swiglu_fwd", &swiglu_fwd, py::arg("gu"), py::arg("perm") = false);
  m.def("swiglu_bwd", &swiglu_bwd, py::arg("dh"), py::arg("gu"), py::arg("dbias") = py::none(),
        py::arg("perm") = false);
  m.def("rope_", &rope_, py::arg("qkv"), py::arg("positions"), py::arg("table"), py::arg("n_rot_heads"),
        py::arg("head_dim"), py::arg("inverse") = false);
  m.def("occupy", [](int64_t blocks, double us) { dpfs_occupy((int)blocks, us, stream()); }, py::arg("blocks"),
        py::arg("us"),
        "collective stand-in on the current stream: `blocks` resident 1024-thread workgroups for `us` microseconds");
}
