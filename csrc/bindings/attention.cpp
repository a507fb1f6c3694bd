#include "common.h"

namespace {

// ---------------------------------------------------------------------------- attention --
// A (B, T, H, hd) operand of the bf16 (`f32` false) or fp32 flash attention as (B*T, ld) rows with
// packed heads; returns ld, the token stride.  16-byte row loads: ld % 8 bf16, or ld % 4 floats
// and an aligned base in fp32 (whose operands may be views at any offset).
long long check_bthd(const torch::Tensor& t, const char* name, int64_t B, int64_t T, int64_t H, int64_t hd, bool f32) {
  check_cuda(t, name);
  TORCH_CHECK(t.scalar_type() == (f32 ? torch::kFloat32 : torch::kBFloat16), name,
              f32 ? " must be fp32" : " must be bf16");
  TORCH_CHECK(t.dim() == 4 && t.size(0) == B && t.size(1) == T && t.size(2) == H && t.size(3) == hd, name,
              " must be (B, T, H, hd)");
  TORCH_CHECK(t.stride(3) == 1 && t.stride(2) == hd && (B == 1 || t.stride(0) == T * t.stride(1)), name,
              " must be a (B*T, ld) row view with packed heads");
  if (f32) {
    TORCH_CHECK(t.stride(1) % 4 == 0 && (reinterpret_cast<uintptr_t>(t.data_ptr()) % 16) == 0, name,
                " token stride must be a multiple of 4 floats (16-byte rows)");
  } else {
    TORCH_CHECK(t.stride(1) % 8 == 0, name, " token stride must be a multiple of 8");
  }
  return t.stride(1);
}

// What the bf16 and fp32 backward share beyond their eight (B, T, H, hd) operands: lse, the
// optional QKV bias gradient `db` (fp32 [3 * H * hd]) and the optional inverse-RoPE arguments
// `rp` / `rt`.  `done`: the input is empty, dbias (if any) is zeroed and nothing is to launch.
struct BwdArgs {
  float* db = nullptr;
  const int64_t* rp = nullptr;
  const float* rt = nullptr;
  bool done = false;
};

BwdArgs check_bwd_args(const char* op, const char* rope_tab_msg, const torch::Tensor& lse,
                       c10::optional<torch::Tensor>& dbias, const c10::optional<torch::Tensor>& rope_pos,
                       const c10::optional<torch::Tensor>& rope_tab, int64_t B, int64_t T, int64_t H, int64_t hd) {
  BwdArgs r;
  TORCH_CHECK(lse.is_cuda() && lse.scalar_type() == torch::kFloat32 && lse.is_contiguous() && lse.numel() == B * H * T,
              op, ": lse must be contiguous fp32 (B, H, T)");
  if (dbias.has_value() && dbias->defined()) {
    TORCH_CHECK(dbias->is_cuda() && dbias->scalar_type() == torch::kFloat32 && dbias->is_contiguous() &&
                    dbias->numel() == 3 * H * hd,
                op, ": dbias must be contiguous fp32 [3 * H * hd]");
    r.db = dbias->data_ptr<float>();
  }
  if (B * T * H == 0) {
    if (r.db) dbias->zero_();
    r.done = true;
    return r;
  }
  if (rope_pos.has_value() && rope_pos->defined()) {
    TORCH_CHECK(rope_pos->scalar_type() == torch::kInt64 && rope_pos->is_contiguous() && rope_pos->numel() == B * T,
                op, ": rope_pos must be contiguous int64 [B*T]");
    TORCH_CHECK(rope_tab.has_value() && rope_tab->scalar_type() == torch::kFloat32 && rope_tab->is_contiguous() &&
                    rope_tab->dim() == 2 && rope_tab->size(1) == hd,
                op, rope_tab_msg);
    r.rp = rope_pos->data_ptr<int64_t>();
    r.rt = rope_tab->data_ptr<float>();
  }
  return r;
}

std::vector<torch::Tensor> attn_fwd(torch::Tensor q, torch::Tensor k, torch::Tensor v, double scale, bool causal,
                                    int64_t impl) {
  const int64_t B = q.size(0), T = q.size(1), H = q.size(2), hd = q.size(3);
  TORCH_CHECK(dpfs_attn_supported_hd((int)hd), "attn: head_dim ", hd, " not supported (32/64/128)");
  const long long ldq = check_bthd(q, "q", B, T, H, hd, false), ldk = check_bthd(k, "k", B, T, H, hd, false),
                  ldv = check_bthd(v, "v", B, T, H, hd, false);
  const at::DeviceGuard g(q.device());
  auto o = torch::empty({B, T, H, hd}, q.options());
  auto lse = torch::empty({B, H, T}, q.options().dtype(torch::kFloat32));
  if (B * T * H)
    dpfs_attn_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr<float>(), (int)B, (int)T,
                  (int)H, (int)hd, ldq, ldk, ldv, H * hd, (float)scale, causal ? 1 : 0, (int)impl, stream());
  return {o, lse};
}

// With dbias (fp32 [3 * H * hd], the packed QKV projection's bias layout) the q / k / v bias
// gradient (column sums of the stored dq / dk / dv) comes out of the same kernels; returns
// whether it did (false: another dK/dV variant is selected, dbias untouched).
bool attn_bwd(torch::Tensor dout, torch::Tensor q, torch::Tensor k, torch::Tensor v, torch::Tensor o,
              torch::Tensor lse, double scale, bool causal, torch::Tensor dq, torch::Tensor dk, torch::Tensor dv,
              c10::optional<torch::Tensor> rope_pos, c10::optional<torch::Tensor> rope_tab,
              c10::optional<torch::Tensor> dbias, int64_t impl) {
  const int64_t B = q.size(0), T = q.size(1), H = q.size(2), hd = q.size(3);
  TORCH_CHECK(dpfs_attn_supported_hd((int)hd), "attn: head_dim not supported");
  const long long ldq = check_bthd(q, "q", B, T, H, hd, false), ldk = check_bthd(k, "k", B, T, H, hd, false),
                  ldv = check_bthd(v, "v", B, T, H, hd, false), lddo = check_bthd(dout, "dout", B, T, H, hd, false),
                  ldo = check_bthd(o, "o", B, T, H, hd, false), lddq = check_bthd(dq, "dq", B, T, H, hd, false),
                  lddk = check_bthd(dk, "dk", B, T, H, hd, false), lddv = check_bthd(dv, "dv", B, T, H, hd, false);
  const at::DeviceGuard g(q.device());
  const BwdArgs a = check_bwd_args("attn_bwd", ": rope_tab must be contiguous fp32 [maxlen, hd]", lse, dbias, rope_pos,
                                   rope_tab, B, T, H, hd);
  if (a.done) return a.db != nullptr;
  auto delta = torch::empty({2, B, H, T}, lse.options());   // -delta | -lse/scale
  if (impl == 6 && dpfs_attn_fused_ws((int)B, (int)T, (int)H, (int)hd) > 0) {
    // fused backward (head_dim 64): fp32 dQ partials per (b, h, 256-key block, 64-query tile)
    auto dqp = torch::empty({dpfs_attn_fused_ws((int)B, (int)T, (int)H, (int)hd)}, lse.options());
    torch::Tensor fb;
    if (a.db) fb = torch::empty({dpfs_attn_fused_bias_ws((int)B, (int)T, (int)H, (int)hd)}, lse.options());
    return dpfs_attn_bwd_fused(dout.data_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
                               lse.data_ptr<float>(), delta.data_ptr<float>(), dqp.data_ptr<float>(), dq.data_ptr(),
                               dk.data_ptr(), dv.data_ptr(), (int)B, (int)T, (int)H, (int)hd, lddo, ldq, ldk, ldv, ldo,
                               lddq, lddk, lddv, (float)scale, causal ? 1 : 0, a.rp, a.rt, stream(), a.db,
                               a.db ? fb.data_ptr<float>() : nullptr) > 0;
  }
  torch::Tensor bws;
  if (a.db) bws = torch::empty({dpfs_attn_bias_ws((int)B, (int)T, (int)H, (int)hd)}, lse.options());
  return dpfs_attn_bwd(dout.data_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr<float>(),
                       delta.data_ptr<float>(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), (int)B, (int)T, (int)H,
                       (int)hd, lddo, ldq, ldk, ldv, ldo, lddq, lddk, lddv, (float)scale, causal ? 1 : 0, a.rp, a.rt,
                       stream(), a.db, a.db ? bws.data_ptr<float>() : nullptr, (int)impl) != 0;
}

// ----------------------------------------------------------------------- fp32 path --
// The reference's default (fp32) training on the device: fp32 flash attention
// (csrc/kernels/fp32.hip; its GEMM is gemm_f32).
std::vector<torch::Tensor> attn_fwd_f32(torch::Tensor q, torch::Tensor k, torch::Tensor v, double scale, bool causal) {
  const int64_t B = q.size(0), T = q.size(1), H = q.size(2), hd = q.size(3);
  TORCH_CHECK(dpfs_attn_f32_supported_hd((int)hd), "attn_fwd_f32: head_dim ", hd, " not supported (32/64/128)");
  const long long ldq = check_bthd(q, "q", B, T, H, hd, true), ldk = check_bthd(k, "k", B, T, H, hd, true),
                  ldv = check_bthd(v, "v", B, T, H, hd, true);
  const at::DeviceGuard g(q.device());
  auto o = torch::empty({B, T, H, hd}, q.options());
  auto lse = torch::empty({B, H, T}, q.options());
  if (B * T * H)
    dpfs_attn_fwd_f32(q.data_ptr<float>(), k.data_ptr<float>(), v.data_ptr<float>(), o.data_ptr<float>(),
                      lse.data_ptr<float>(), (int)B, (int)T, (int)H, (int)hd, ldq, ldk, ldv, H * hd, (float)scale,
                      causal ? 1 : 0, stream());
  return {o, lse};
}

bool attn_bwd_f32(torch::Tensor dout, torch::Tensor q, torch::Tensor k, torch::Tensor v, torch::Tensor o,
                  torch::Tensor lse, double scale, bool causal, torch::Tensor dq, torch::Tensor dk, torch::Tensor dv,
                  c10::optional<torch::Tensor> rope_pos, c10::optional<torch::Tensor> rope_tab,
                  c10::optional<torch::Tensor> dbias) {
  const int64_t B = q.size(0), T = q.size(1), H = q.size(2), hd = q.size(3);
  TORCH_CHECK(dpfs_attn_f32_supported_hd((int)hd), "attn_bwd_f32: head_dim not supported");
  const long long ldq = check_bthd(q, "q", B, T, H, hd, true), ldk = check_bthd(k, "k", B, T, H, hd, true),
                  ldv = check_bthd(v, "v", B, T, H, hd, true), lddo = check_bthd(dout, "dout", B, T, H, hd, true),
                  ldo = check_bthd(o, "o", B, T, H, hd, true), lddq = check_bthd(dq, "dq", B, T, H, hd, true),
                  lddk = check_bthd(dk, "dk", B, T, H, hd, true), lddv = check_bthd(dv, "dv", B, T, H, hd, true);
  const at::DeviceGuard g(q.device());
  const BwdArgs a = check_bwd_args("attn_bwd_f32", ": rope_tab fp32 [maxlen, hd]", lse, dbias, rope_pos, rope_tab, B, T,
                                   H, hd);
  if (a.done) return a.db != nullptr;
  auto ws = torch::empty({dpfs_attn_bwd_f32_ws((int)B, (int)T, (int)H, (int)hd, a.db ? 1 : 0)}, lse.options());
  return dpfs_attn_bwd_f32(dout.data_ptr<float>(), q.data_ptr<float>(), k.data_ptr<float>(), v.data_ptr<float>(),
                           o.data_ptr<float>(), lse.data_ptr<float>(), ws.data_ptr<float>(), dq.data_ptr<float>(),
                           dk.data_ptr<float>(), dv.data_ptr<float>(), (int)B, (int)T, (int)H, (int)hd, lddo, ldq, ldk,
                           ldv, ldo, lddq, lddk, lddv, (float)scale, causal ? 1 : 0, a.rp, a.rt, a.db, stream()) != 0;
}

}  // namespace

void bind_attention(py::module_& m) {
  m.def("attn_diag", [](torch::Tensor t) { dpfs_attn_diag(t.defined() && t.numel() ? t.data_ptr() : nullptr); },
        "int64 buffer of the DIAG builds (attn_fwd / attn_bwd impl 5): per-wave s_memtime splits");
  m.def("attn_prefetch", [](int v) { dpfs_attn_prefetch(v); },
        "head_dim-64 attention backward, next block's operands fetched ahead: bit 0 = dK/dV, bit 1 = dQ (3 default; A/B)");
  m.def("attn_fwd", &attn_fwd, py::arg("q"), py::arg("k"), py::arg("v"), py::arg("scale"), py::arg("causal") = true,
        py::arg("impl") = 0,
        "flash attention forward; impl (per call): 0 = auto (32x32x16 LDS-DMA ring at hd 64 / 128, "
        "16x16x32 register-staged at hd 32), 1 = 16x16x32 register-staged, 4 = 32x32x16 ring, 5 = its DIAG build");
  m.def("attn_bwd", &attn_bwd, py::arg("dout"), py::arg("q"), py::arg("k"), py::arg("v"), py::arg("o"),
        py::arg("lse"), py::arg("scale"), py::arg("causal"), py::arg("dq"), py::arg("dk"), py::arg("dv"),
        py::arg("rope_pos") = py::none(), py::arg("rope_tab") = py::none(), py::arg("dbias") = py::none(),
        py::arg("impl") = 0,
        "flash attention backward; impl (per call): 0 = auto (dq3 + dkdv3 at hd 64 / 128, dq + dkdv2 at hd 32), "
        "2 = dq + dkdv2 (16x16x32), 4 = dq3 + dkdv3 (32x32x16), 5 = 4 with the dK/dV DIAG build, 6 = the fused "
        "head_dim-64 backward (delta pass, one dK/dV/dQ kernel, dQ partial reduction)");
  m.def("attn_fwd_f32", &attn_fwd_f32, "fp32 causal flash attention forward: (o, lse)");
  m.def("attn_bwd_f32", &attn_bwd_f32, py::arg("dout"), py::arg("q"), py::arg("k"), py::arg("v"), py::arg("o"),
        py::arg("lse"), py::arg("scale"), py::arg("causal"), py::arg("dq"), py::arg("dk"), py::arg("dv"),
        py::arg("rope_pos") = py::none(), py::arg("rope_tab") = py::none(), py::arg("dbias") = py::none(),
        "fp32 flash attention backward (dQ kernel, then dK/dV), optional inverse RoPE and QKV bias gradient");
  m.def("attn_stagger", [](int v) { dpfs_attn_stagger(v); },
        "A/B hook: odd workgroups of the v3 attention backward kernels start v x 8k cycles late (0 default)");
}
