#include "common.h"

namespace {

// Output buffer: `out` when given (contiguous [M, N] of a's dtype, e.g. a staging slot of the
// xGMI collectives), else a fresh tensor.
torch::Tensor gemm_out(const c10::optional<torch::Tensor>& out, const torch::Tensor& a, int64_t M, int64_t N) {
  if (!out.has_value() || !out->defined()) return torch::empty({M, N}, a.options());
  check_cuda(*out, "out");
  TORCH_CHECK(out->is_contiguous() && out->dim() == 2 && out->size(0) == M && out->size(1) == N &&
                  out->scalar_type() == a.scalar_type(),
              "gemm: out must be a contiguous [M, N] tensor of the operand dtype");
  return *out;
}

// NT output: `out` may also be a row-major column slice of a wider buffer (unit column stride,
// row stride >= N and a multiple of 8), e.g. the V columns of the packed QKV output.
torch::Tensor gemm_out_rows(const c10::optional<torch::Tensor>& out, const torch::Tensor& a, int64_t M, int64_t N) {
  if (!out.has_value() || !out->defined()) return torch::empty({M, N}, a.options());
  check_cuda(*out, "out");
  TORCH_CHECK(out->dim() == 2 && out->size(0) == M && out->size(1) == N && out->scalar_type() == a.scalar_type() &&
                  (N <= 1 || out->stride(1) == 1) && out->stride(0) >= N && out->stride(0) % 8 == 0,
              "gemm_nt: out must be a row-major [M, N] tensor (or column slice) of the operand dtype");
  return *out;
}

// Kernel variant of the bf16 NT / NN GEMMs (an argument of every call, csrc/kernels/gemm.hip).
void check_bf16_variant(int64_t variant) {
  TORCH_CHECK((variant >= 0 && variant <= 6) || variant == 8 || variant == 12,
              "gemm: variant 0 (v4), 1 (v4 256-wide), 2 (v4 192-wide), 3 (v3), 8 (v4 stream-K 256-wide); "
              "+4: v4 with non-temporal output stores");
}

// The fp32 workspace of one bf16 NT / NN GEMM call: the split-K slabs, or with variant & 8 the
// stream-K partials / flags where that kernel applies (it replaces the split-K slabs).  gemm.hip
// keeps the pointer in a thread-local for the launch; it is cleared on every way out of the
// call, a throwing check included, so it never outlives the tensor.
struct Bf16Workspace {
  torch::Tensor ws;
  Bf16Workspace(const torch::Tensor& a, int64_t M, int64_t N, int64_t K, int64_t variant) {
    long long wsn = dpfs_gemm_bf16_ws((int)M, (int)N, (int)K);
    if (variant & 8) {
      const long long skn = dpfs_gemm4_sk_ws((int)M, (int)N, (int)K);
      if (skn > 0) wsn = skn;
    }
    if (wsn > 0) ws = torch::empty({wsn}, a.options().dtype(torch::kFloat32));
    dpfs_gemm_set_workspace(wsn > 0 ? ws.data_ptr<float>() : nullptr, wsn);
  }
  ~Bf16Workspace() { dpfs_gemm_set_workspace(nullptr, 0); }
  Bf16Workspace(const Bf16Workspace&) = delete;
  Bf16Workspace& operator=(const Bf16Workspace&) = delete;
};

// `out` when given (it must satisfy `ok`, else `msg`), else a fresh [M, N] tensor, which there
// is nothing to accumulate into.
template <class Pred>
torch::Tensor out_or_new(const c10::optional<torch::Tensor>& out, Pred ok, const char* msg, int64_t M, int64_t N,
                         const torch::TensorOptions& opts, bool& accumulate) {
  if (out.has_value() && out->defined()) {
    TORCH_CHECK(ok(*out), msg);
    return *out;
  }
  accumulate = false;
  return torch::empty({M, N}, opts);
}

// Bytes from the first to one past the last element of a row-major bf16 matrix.
long long span_bytes(const torch::Tensor& t) {
  return t.size(0) > 0 ? ((t.size(0) - 1) * t.stride(0) + t.size(1)) * 2 : 0;
}

torch::Tensor gemm_nt(torch::Tensor a, torch::Tensor b, c10::optional<torch::Tensor> bias,
                      c10::optional<torch::Tensor> rope_pos, c10::optional<torch::Tensor> rope_tab,
                      int64_t rope_heads, int64_t rope_hd, c10::optional<torch::Tensor> out, int64_t variant) {
  check_rowmajor(a, "a");
  check_bf16_variant(variant);
  check_rowmajor(b, "b");
  TORCH_CHECK(a.scalar_type() == torch::kBFloat16 && b.scalar_type() == torch::kBFloat16, "gemm_nt: bf16 operands");
  const int64_t M = a.size(0), K = a.size(1), N = b.size(0);
  TORCH_CHECK(b.size(1) == K, "gemm_nt: K mismatch ", K, " vs ", b.size(1));
  TORCH_CHECK(K % 8 == 0, "gemm_nt: K must be a multiple of 8, got ", K);
  TORCH_CHECK(a.stride(0) % 8 == 0 && b.stride(0) % 8 == 0, "gemm_nt: row strides must be multiples of 8");
  const at::DeviceGuard g(a.device());
  auto c = gemm_out_rows(out, a, M, N);
  if (M == 0 || N == 0) return c;
  if (K == 0) return c.zero_();
  TORCH_CHECK(N % 4 == 0, "gemm_nt: N must be a multiple of 4, got ", N);
  const int ldc = (int)(M > 1 ? c.stride(0) : N);
  const Bf16Workspace ws(a, M, N, K, variant);
  const bool want_rope = rope_pos.has_value() && rope_pos->defined() && rope_heads > 0;
  if (want_rope && dpfs_gemm_rope_fusable((int)M, (int)N, (int)K, (int)rope_hd, (int)variant)) {
    TORCH_CHECK(rope_pos->scalar_type() == torch::kInt64 && rope_pos->is_contiguous() && rope_pos->numel() == M,
                "gemm_nt: rope_pos must be contiguous int64 [M]");
    TORCH_CHECK(rope_tab.has_value() && rope_tab->scalar_type() == torch::kFloat32 && rope_tab->is_contiguous() &&
                    rope_tab->size(1) == rope_hd,
                "gemm_nt: rope_tab must be fp32 [maxlen, hd]");
    dpfs_gemm_nt_rope(a.data_ptr(), b.data_ptr(), c.data_ptr(), opt_f32(bias, N, "bias"), (int)M, (int)N, (int)K,
                      (int)a.stride(0), (int)b.stride(0), ldc, rope_pos->data_ptr<int64_t>(),
                      rope_tab->data_ptr<float>(), (int)(rope_heads * rope_hd), (int)rope_hd, (int)variant, stream());
  } else {
    TORCH_CHECK(!want_rope || ldc == N, "gemm_nt: the separate RoPE pass needs a contiguous output");
    dpfs_gemm_nt(a.data_ptr(), b.data_ptr(), c.data_ptr(), opt_f32(bias, N, "bias"), (int)M, (int)N, (int)K,
                 (int)a.stride(0), (int)b.stride(0), ldc, (int)variant, stream());
    if (want_rope) rope_(c, *rope_pos, *rope_tab, rope_heads, rope_hd, false);
  }
  return c;
}

torch::Tensor gemm_nn(torch::Tensor a, torch::Tensor b, c10::optional<torch::Tensor> out, int64_t variant) {
  check_rowmajor(a, "a");
  check_bf16_variant(variant);
  check_rowmajor(b, "b");
  TORCH_CHECK(a.scalar_type() == torch::kBFloat16 && b.scalar_type() == torch::kBFloat16, "gemm_nn: bf16 operands");
  const int64_t M = a.size(0), K = a.size(1), N = b.size(1);
  TORCH_CHECK(b.size(0) == K, "gemm_nn: K mismatch");
  TORCH_CHECK(K % 8 == 0 && N % 8 == 0, "gemm_nn: K and N must be multiples of 8, got ", K, " ", N);
  TORCH_CHECK(a.stride(0) % 8 == 0 && b.stride(0) % 8 == 0, "gemm_nn: row strides must be multiples of 8");
  const at::DeviceGuard g(a.device());
  auto c = gemm_out(out, a, M, N);
  if (M == 0 || N == 0) return c;
  if (K == 0) return c.zero_();
  const Bf16Workspace ws(a, M, N, K, variant);
  dpfs_gemm_nn(a.data_ptr(), b.data_ptr(), c.data_ptr(), (int)M, (int)N, (int)K, (int)a.stride(0), (int)b.stride(0),
               (int)N, (int)variant, stream());
  return c;
}

// c[M,N] fp32 = a[K,M]^T b[K,N]
torch::Tensor gemm_tn(torch::Tensor a, torch::Tensor b, c10::optional<torch::Tensor> out, bool accumulate,
                      int64_t variant) {
  check_rowmajor(a, "a");
  TORCH_CHECK(variant == 0 || variant == 3, "gemm_tn: variant 0 (v4) or 3 (v3)");
  check_rowmajor(b, "b");
  TORCH_CHECK(a.scalar_type() == torch::kBFloat16 && b.scalar_type() == torch::kBFloat16, "gemm_tn: bf16 operands");
  const int64_t K = a.size(0), M = a.size(1), N = b.size(1);
  TORCH_CHECK(b.size(0) == K, "gemm_tn: K mismatch");
  TORCH_CHECK(M % 8 == 0 && N % 8 == 0, "gemm_tn: M and N must be multiples of 8, got ", M, " ", N);
  TORCH_CHECK(a.stride(0) % 8 == 0 && b.stride(0) % 8 == 0, "gemm_tn: row strides must be multiples of 8");
  const at::DeviceGuard g(a.device());
  auto c = out_or_new(out, [&](const torch::Tensor& o) {
    return o.scalar_type() == torch::kFloat32 && o.is_contiguous() && o.size(0) == M && o.size(1) == N;
  }, "gemm_tn: out must be contiguous fp32 [M,N]", M, N, a.options().dtype(torch::kFloat32), accumulate);
  if (M == 0 || N == 0) return c;
  if (K == 0) {
    if (!accumulate) c.zero_();
    return c;
  }
  const long long wsn = dpfs_gemm_tn_ws((int)M, (int)N, (int)K, accumulate ? 1 : 0);
  torch::Tensor ws;
  if (wsn > 0) ws = torch::empty({(int64_t)wsn}, c.options());
  dpfs_gemm_tn(a.data_ptr(), b.data_ptr(), c.data_ptr<float>(), ws.defined() ? ws.data_ptr<float>() : nullptr, (int)M,
               (int)N, (int)K, (int)a.stride(0), (int)b.stride(0), accumulate ? 1 : 0, (int)variant, stream());
  return c;
}

// outs[g] fp32 (+= when acc[g]) a[g][K, M_g]^T b[g][K, N_g] for up to 4 GEMMs over one K as
// one grouped launch (+ one reduction); with a2 / b2 the rows continue in second buffers
// (a chunked step's other ping-pong chunk, K1 rows each).  False (nothing written) where the
// group does not apply.
bool gemm_tn_group(std::vector<torch::Tensor> a, std::vector<torch::Tensor> b, std::vector<torch::Tensor> outs,
                   std::vector<int64_t> acc, c10::optional<std::vector<torch::Tensor>> a2,
                   c10::optional<std::vector<torch::Tensor>> b2) {
  const size_t n = a.size();
  TORCH_CHECK(n >= 1 && n <= 4 && b.size() == n && outs.size() == n && acc.size() == n, "gemm_tn_group: 1..4 GEMMs");
  const bool two = a2.has_value() && b2.has_value();
  TORCH_CHECK(!two || (a2->size() == n && b2->size() == n), "gemm_tn_group: a2 / b2 per GEMM");
  const int64_t K = a[0].size(0);
  const int64_t K1 = two ? (*a2)[0].size(0) : 0;
  const void* pa[4];
  const void* pb[4];
  const void* pa2[4] = {nullptr, nullptr, nullptr, nullptr};
  const void* pb2[4] = {nullptr, nullptr, nullptr, nullptr};
  float* pc[4];
  int M[4], N[4], lda[4], ldb[4], ac[4], lda2[4] = {0, 0, 0, 0}, ldb2[4] = {0, 0, 0, 0};
  for (size_t g = 0; g < n; ++g) {
    check_rowmajor(a[g], "gemm_tn_group a");
    check_rowmajor(b[g], "gemm_tn_group b");
    TORCH_CHECK(a[g].scalar_type() == torch::kBFloat16 && b[g].scalar_type() == torch::kBFloat16,
                "gemm_tn_group: bf16 operands");
    TORCH_CHECK(a[g].size(0) == K && b[g].size(0) == K, "gemm_tn_group: one K for the group");
    TORCH_CHECK(a[g].device() == a[0].device() && b[g].device() == a[0].device() && outs[g].device() == a[0].device(),
                "gemm_tn_group: one device");
    M[g] = (int)a[g].size(1);
    N[g] = (int)b[g].size(1);
    TORCH_CHECK(outs[g].scalar_type() == torch::kFloat32 && outs[g].is_contiguous() && outs[g].dim() == 2 &&
                    outs[g].size(0) == M[g] && outs[g].size(1) == N[g],
                "gemm_tn_group: out must be contiguous fp32 [M,N]");
    lda[g] = (int)a[g].stride(0);
    ldb[g] = (int)b[g].stride(0);
    ac[g] = acc[g] ? 1 : 0;
    pa[g] = a[g].data_ptr();
    pb[g] = b[g].data_ptr();
    pc[g] = outs[g].data_ptr<float>();
    if (two) {
      const torch::Tensor& x = (*a2)[g];
      const torch::Tensor& y = (*b2)[g];
      check_rowmajor(x, "gemm_tn_group a2");
      check_rowmajor(y, "gemm_tn_group b2");
      TORCH_CHECK(x.scalar_type() == torch::kBFloat16 && y.scalar_type() == torch::kBFloat16 && x.size(0) == K1 &&
                      y.size(0) == K1 && x.size(1) == M[g] && y.size(1) == N[g] && x.device() == a[0].device() &&
                      y.device() == a[0].device(),
                  "gemm_tn_group: a2 [K1, M] / b2 [K1, N] bf16 on the group's device");
      lda2[g] = (int)x.stride(0);
      ldb2[g] = (int)y.stride(0);
      pa2[g] = x.data_ptr();
      pb2[g] = y.data_ptr();
    }
  }
  if (K <= 0 || K + K1 >= (1ll << 31) || (two && K1 <= 0)) return false;
  const long long wsn = dpfs_gemm_tn_group_ws((int)n, M, N, lda, ldb, (int)K, ac, two ? lda2 : nullptr,
                                              two ? ldb2 : nullptr, (int)K1);
  if (wsn < 0) return false;
  const at::DeviceGuard dg(a[0].device());
  torch::Tensor ws;
  if (wsn > 0) ws = torch::empty({(int64_t)wsn}, outs[0].options());
  return dpfs_gemm_tn_group((int)n, pa, pb, pc, M, N, lda, ldb, ac, (int)K, ws.defined() ? ws.data_ptr<float>() : nullptr,
                            wsn, pa2, pb2, lda2, ldb2, (int)K1, stream()) != 0;
}

// c[M,N] fp32 (+)= a0[K0,M]^T b0[K0,N] + a1[K1,M]^T b1[K1,N] in one split-K launch; None
// (nothing written) when the K-split plan does not fit the two buffers.
c10::optional<torch::Tensor> gemm_tn2(torch::Tensor a0, torch::Tensor b0, torch::Tensor a1, torch::Tensor b1,
                                      c10::optional<torch::Tensor> out, bool accumulate, int64_t variant) {
  TORCH_CHECK(variant == 0 || variant == 3, "gemm_tn2: variant 0 (v4) or 3 (v3)");
  for (auto* t : {&a0, &b0, &a1, &b1}) {
    check_rowmajor(*t, "gemm_tn2 operand");
    TORCH_CHECK(t->scalar_type() == torch::kBFloat16 && t->stride(0) % 8 == 0, "gemm_tn2: bf16, row stride % 8");
  }
  const int64_t K0 = a0.size(0), K1 = a1.size(0), M = a0.size(1), N = b0.size(1);
  TORCH_CHECK(b0.size(0) == K0 && b1.size(0) == K1 && a1.size(1) == M && b1.size(1) == N, "gemm_tn2: shape mismatch");
  TORCH_CHECK(M % 8 == 0 && N % 8 == 0, "gemm_tn2: M and N must be multiples of 8");
  TORCH_CHECK(a1.device() == a0.device() && b0.device() == a0.device() && b1.device() == a0.device(),
              "gemm_tn2: one device");
  const at::DeviceGuard g(a0.device());
  auto c = out_or_new(out, [&](const torch::Tensor& o) {
    return o.scalar_type() == torch::kFloat32 && o.is_contiguous() && o.size(0) == M && o.size(1) == N;
  }, "gemm_tn2: out must be contiguous fp32 [M,N]", M, N, a0.options().dtype(torch::kFloat32), accumulate);
  if (M == 0 || N == 0 || K0 == 0 || K1 == 0) return c10::nullopt;
  const long long wsn = dpfs_gemm_tn2_ws((int)M, (int)N, (int)K0, (int)K1);
  if (wsn <= 0) return c10::nullopt;
  auto ws = torch::empty({wsn}, c.options());
  const int ok = dpfs_gemm_tn2(a0.data_ptr(), b0.data_ptr(), a1.data_ptr(), b1.data_ptr(), c.data_ptr<float>(),
                               ws.data_ptr<float>(), (int)M, (int)N, (int)K0, (int)K1, (int)a0.stride(0),
                               (int)b0.stride(0), (int)a1.stride(0), (int)b1.stride(0), accumulate ? 1 : 0,
                               (int)variant, stream());
  if (!ok) return c10::nullopt;
  return c;
}

// Gate|up projection with SwiGLU in the GEMM epilogue: w / bias in the natural [gate | up]
// layout, read with the rows interleaved in 64-row blocks (reference.gu_perm).  Returns
// [gu (interleaved), h] or [] where the fused kernel does not apply (the caller runs the GEMM
// on the interleaved weight + swiglu_fwd(perm)).
std::vector<torch::Tensor> gemm_nt_swiglu(torch::Tensor a, torch::Tensor b, c10::optional<torch::Tensor> bias) {
  check_rowmajor(a, "a");
  check_rowmajor(b, "b");
  TORCH_CHECK(a.scalar_type() == torch::kBFloat16 && b.scalar_type() == torch::kBFloat16,
              "gemm_nt_swiglu: bf16 operands");
  const int64_t M = a.size(0), K = a.size(1), N = b.size(0);
  TORCH_CHECK(b.size(1) == K, "gemm_nt_swiglu: K mismatch");
  const at::DeviceGuard g(a.device());
  if (M == 0 || N % 128 || K % 64 || a.stride(0) % 8 || b.stride(0) % 8 || span_bytes(a) >= (1ll << 32) - 16 ||
      span_bytes(b) >= (1ll << 32) - 16)
    return {};
  auto c = torch::empty({M, N}, a.options());
  auto h = torch::empty({M, N / 2}, a.options());
  if (!dpfs_gemm4_nt_swiglu(a.data_ptr(), b.data_ptr(), c.data_ptr(), opt_f32(bias, N, "bias"), h.data_ptr(), (int)M,
                            (int)N, (int)K, (int)a.stride(0), (int)b.stride(0), (int)N, (int)(N / 2),
                            (unsigned)span_bytes(a), (unsigned)span_bytes(b), stream()))
    return {};
  return {c, h};
}

// Down-projection data gradient with the SwiGLU backward in its epilogue: dgu = SwiGLU'(gu) *
// (dy w) in the natural [gate | up] layout without materialising dy w (gu interleaved when
// `perm`); with `dbias` also the gate|up bias gradient (column sums of dgu) from the same
// kernel's partials.  Returns [] where the fused kernel does not apply (the caller runs
// gemm_nn + swiglu_bwd).
std::vector<torch::Tensor> gemm_nn_swiglu_bwd(torch::Tensor dy, torch::Tensor w, torch::Tensor gu,
                                              c10::optional<torch::Tensor> dbias, bool perm) {
  check_rowmajor(dy, "dy");
  check_rowmajor(w, "w");
  check_rowmajor(gu, "gu");
  TORCH_CHECK(dy.scalar_type() == torch::kBFloat16 && w.scalar_type() == torch::kBFloat16 &&
                  gu.scalar_type() == torch::kBFloat16, "gemm_nn_swiglu_bwd: bf16 operands");
  const int64_t M = dy.size(0), K = dy.size(1), F = w.size(1);
  TORCH_CHECK(w.size(0) == K && gu.size(0) == M && gu.size(1) == 2 * F, "gemm_nn_swiglu_bwd: shapes");
  const at::DeviceGuard g(dy.device());
  if (M == 0 || F % 64 || K % 64 || dy.stride(0) % 8 || w.stride(0) % 8 || gu.stride(0) % 8 ||
      span_bytes(dy) >= (1ll << 32) - 16 || span_bytes(w) >= (1ll << 32) - 16)
    return {};
  float* db = dbias_out(dbias, 2 * F, "gemm_nn_swiglu_bwd");
  auto dgu = torch::empty({M, 2 * F}, gu.options());
  const int64_t prow = 2 * ((M + 255) / 256);
  torch::Tensor part;
  if (db) part = torch::empty({prow, 2 * F}, gu.options().dtype(torch::kFloat32));
  if (!dpfs_gemm4_nn_swiglu_bwd(dy.data_ptr(), w.data_ptr(), gu.data_ptr(), dgu.data_ptr(),
                                db ? part.data_ptr<float>() : nullptr, (int)M, (int)F, (int)K, (int)dy.stride(0),
                                (int)w.stride(0), (int)gu.stride(0), (int)(2 * F), perm ? 1 : 0,
                                (unsigned)span_bytes(dy), (unsigned)span_bytes(w), stream()))
    return {};
  if (db) dpfs_colsum_rows_small(part.data_ptr<float>(), db, (int)prow, (int)(2 * F), stream());
  return {dgu};
}

// ----------------------------------------------------------------------- fp32 path --
// The reference's default (fp32) training on the device: fp32-input MFMA GEMMs and flash
// attention (csrc/kernels/fp32.hip).  layout 0 = NT: c[M,N] = a[M,K] b[N,K]^T (+ bias);
// 1 = NN: a[M,K] b[K,N]; 2 = TN: a[K,M]^T b[K,N] (+= into out with accumulate).
torch::Tensor gemm_f32(torch::Tensor a, torch::Tensor b, int64_t layout, c10::optional<torch::Tensor> bias,
                       c10::optional<torch::Tensor> out, bool accumulate) {
  check_cuda(a, "a");
  check_cuda(b, "b");
  const bool in16 = a.scalar_type() == torch::kBFloat16;
  TORCH_CHECK((a.scalar_type() == torch::kFloat32 || in16) && b.scalar_type() == a.scalar_type(),
              "gemm_f32: fp32 or bf16 operands (both alike)");
  TORCH_CHECK(a.dim() == 2 && b.dim() == 2 && a.stride(1) == 1 && b.stride(1) == 1, "gemm_f32: row-major 2-D operands");
  TORCH_CHECK(layout >= 0 && layout <= 2, "gemm_f32: layout 0 / 1 / 2");
  const int64_t M = layout == 2 ? a.size(1) : a.size(0), K = layout == 2 ? a.size(0) : a.size(1);
  const int64_t N = layout == 0 ? b.size(0) : b.size(1);
  TORCH_CHECK((layout == 0 ? b.size(1) : b.size(0)) == K, "gemm_f32: inner dimensions differ");
  const at::DeviceGuard g(a.device());
  // a fresh output has the bf16 API's dtypes: a.dtype for NT / NN, fp32 for TN (weight gradients)
  auto c = out_or_new(out, [&](const torch::Tensor& o) {
    return (o.scalar_type() == torch::kFloat32 || o.scalar_type() == torch::kBFloat16) && o.dim() == 2 &&
           o.size(0) == M && o.size(1) == N && o.stride(1) == 1;
  }, "gemm_f32: out fp32 / bf16 [M, N] row-major", M, N,
                      a.options().dtype(layout == 2 ? torch::kFloat32 : a.scalar_type()), accumulate);
  TORCH_CHECK(in16 || c.scalar_type() == torch::kFloat32, "gemm_f32: fp32 operands give an fp32 output");
  const float* bp = nullptr;
  if (bias.has_value() && bias->defined()) {
    TORCH_CHECK(bias->scalar_type() == torch::kFloat32 && bias->is_contiguous() && bias->numel() == N,
                "gemm_f32: bias fp32 [N]");
    bp = bias->data_ptr<float>();
  }
  if (M && N) {
    if (K == 0) {
      if (!accumulate) c.zero_();
      if (bp) c.add_(*bias);
    } else {
      const int sp = dpfs_gemm_f32_splits((int)M, (int)N, (int)K);   // K-split slabs (weight gradients)
      torch::Tensor ws;
      if (sp > 1) ws = torch::empty({(int64_t)sp * M * N}, a.options().dtype(torch::kFloat32));
      dpfs_gemm_f32((int)layout, a.data_ptr(), b.data_ptr(), c.data_ptr(), bp, (int)M, (int)N, (int)K, a.stride(0),
                    b.stride(0), c.stride(0), accumulate ? 1 : 0, sp > 1 ? ws.data_ptr<float>() : nullptr,
                    in16 ? 1 : 0, c.scalar_type() == torch::kBFloat16 ? 1 : 0, stream());
    }
  }
  return c;
}

}  // namespace

void bind_gemm(py::module_& m) {
  m.def("gemm_nt", &gemm_nt, py::arg("a"), py::arg("b"), py::arg("bias") = py::none(),
        py::arg("rope_pos") = py::none(), py::arg("rope_tab") = py::none(), py::arg("rope_heads") = 0,
        py::arg("rope_hd") = 0, py::arg("out") = py::none(), py::arg("variant") = 0);
  m.def("gemm_nn", &gemm_nn, py::arg("a"), py::arg("b"), py::arg("out") = py::none(), py::arg("variant") = 0);
  m.def("gemm_force", [](int cfg, int splits) { dpfs_gemm_force(cfg, splits); },
        "force the v2 tile config (-1 auto, 0 = 256x256, 1 = 256x128) and K-splits (0 auto)");
  m.def("gemm4_ablate", [](int v) { dpfs_gemm4_ablate(v); }, "timing-only: 1 = drop stores, 2 = zero operands");
  m.def("gemm4_diag", [](torch::Tensor t) { dpfs_gemm4_diag(t.defined() && t.numel() ? t.data_ptr() : nullptr); },
        "int64 buffer [grid*4*4] for the DIAG build's per-wave cycle split (gemm4_ablate bit 16)");
  m.def("gemm_tn_group", &gemm_tn_group, py::arg("a"), py::arg("b"), py::arg("outs"), py::arg("acc"),
        py::arg("a2") = py::none(), py::arg("b2") = py::none());
  m.def("gemm_tn_splits", [](int M, int N, int K) { return dpfs_gemm_tn_splits(M, N, K); },
        "K-split count of the TN (weight-gradient) plan for an M x N output over K");
  m.def("gemm4_swb_depth", [](int v) { dpfs_gemm4_swb_depth(v); },
        "SwiGLU-backward epilogue of the down-projection dgrad: gate / up row blocks in flight (2 default, 1 = A/B)");
  m.def("gemm_sk_error", [](bool reset) { return dpfs_gemm4_sk_error(reset ? 1 : 0); }, py::arg("reset") = false,
        "sticky host-mapped word: 1 when a stream-K consumer's bounded wait for its producer's partial timed out "
        "(that GEMM's output is wrong); read without a device sync");
  m.def("gemm_sk_starve", [](bool on) { dpfs_gemm4_sk_starve(on ? 1 : 0); },
        "test hook: the next stream-K launch's producers never raise their flags, so every consumer wait times out");
  m.def("gemm_sk_applies", [](int64_t M, int64_t N, int64_t K) { return dpfs_gemm4_sk_ws((int)M, (int)N, (int)K) > 0; },
        "whether the stream-K bf16 kernel (variant 8 / 12) applies to an M x N x K NT / NN GEMM on this device");
  m.def("gemm4_m32k", [](int v) { dpfs_gemm4_m32k(v); },
        "NN / NT 256-wide main loop of the v4 GEMM: bit 0 = 32x32x16 MFMAs for the fp32 (split-K) output, bit 1 = for "
        "the bf16 (+ bias) output, 0 = 16x16x32 (default; measured faster in the step)");
  m.def("gemm4_m32", [](int v) { dpfs_gemm4_m32(v); },
        "TN main loop of the v4 GEMM: 1 = 32x32x16 MFMAs (default), 0 = 16x16x32 (A/B probes)");
  m.def("gemm4_br", [](int v) { dpfs_gemm4_br(v); },
        "rows of MFMAs before each step's barrier in the plain v4 kernels (0, 1, 2 = default; A/B runs)");
  m.def("gemm4_sched", [](int v) { dpfs_gemm4_sched(v); },
        "v4 main-loop variant: 0 = default (descriptor-advancing DMA where K ranges allow, one piece per MFMA "
        "row), 1 = two pieces per row in rows 4-7, 2 = per-lane K checks everywhere (the pre-FAST stream)");
  m.def("gemm4_br_tn", [](int v) { dpfs_gemm4_br_tn(v); },
        "blocks of 4 MFMAs before each step's barrier in the 32x32x16 (TN weight-gradient) main loop (0 default, 1, 2; A/B)");
  m.def("gemm4_group_m", [](int v) { dpfs_gemm4_group_m(v); }, "v4 tile-row group size of the item order (default 4)");
  m.def("gemm_v2_sched", [](int v) { dpfs_gemm_v2_sched(v); }, "v2 256x256 schedule (-1 per-layout default, 0..4 see gemm2_k SCHED)");
  m.def("gemm_set_impl", [](int v) { dpfs_gemm_set_impl(v); }, "1 = v1 (128x128 register-staged), 2 = v2 (LDS-DMA, one tile per workgroup), 3 = v3 (persistent v2, default)");
  m.def("gemm_tn2", &gemm_tn2, "fp32 c (+)= a0^T b0 + a1^T b1 (reduction dim over two buffers), one split-K launch; None if the plan does not fit",
        py::arg("a0"), py::arg("b0"), py::arg("a1"), py::arg("b1"), py::arg("out") = py::none(),
        py::arg("accumulate") = false, py::arg("variant") = 0);
  m.def("gemm_tn", &gemm_tn, py::arg("a"), py::arg("b"), py::arg("out") = py::none(), py::arg("accumulate") = false,
        py::arg("variant") = 0);
  m.def("gemm_nn_swiglu_bwd", &gemm_nn_swiglu_bwd, py::arg("dy"), py::arg("w"), py::arg("gu"),
        py::arg("dbias") = py::none(), py::arg("perm") = true);
  m.def("gemm_nt_swiglu", &gemm_nt_swiglu,
        "gate|up NT GEMM (rows interleaved in 64-row blocks) with SwiGLU in the epilogue: [gu, h] or []",
        py::arg("a"), py::arg("b"), py::arg("bias") = py::none());
  m.def("gemm_f32", &gemm_f32, py::arg("a"), py::arg("b"), py::arg("layout"), py::arg("bias") = py::none(),
        py::arg("out") = py::none(), py::arg("accumulate") = false,
        "fp32-input MFMA GEMM (v_mfma_f32_32x32x2_f32, exact products): layout 0 = a b^T (+ bias), 1 = a b, 2 = a^T b "
        "(+=); fp32 or bf16 operands of any alignment (bf16: the shapes the bf16 MFMA kernels decline)");
}
