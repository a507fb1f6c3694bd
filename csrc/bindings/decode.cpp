#include "common.h"

namespace {

// ----------------------------------------------------------------------------- decode --
void check_cache(const torch::Tensor& c, const char* name) {
  check_cuda(c, name);
  TORCH_CHECK(c.dim() == 4 && c.is_contiguous() && c.scalar_type() == torch::kBFloat16, name,
              " must be a contiguous bf16 (B, T_max, H, hd) cache");
}

// The cache length: one int32 for the whole batch (false: the uniform kernels), or one per
// sequence, B of them (true: the per-row kernels; at B == 1 the two coincide).
bool check_len(const torch::Tensor& len, int64_t B) {
  check_cuda(len, "len");
  TORCH_CHECK(len.scalar_type() == torch::kInt32 && len.is_contiguous() && (len.numel() == 1 || len.numel() == B),
              "len must be a contiguous device int32 tensor of 1 or B = ", B, " elements, got ", len.numel(), " of ",
              len.scalar_type());
  return len.numel() != 1;
}

// o[B, H*hd] = softmax(q k^T * scale) v over keys [0, *len] of the cache (one query per
// sequence and head).  q: [B, >= H*hd] rows (e.g. the q part of the packed qkv row).
torch::Tensor attn_decode(torch::Tensor q, torch::Tensor kc, torch::Tensor vc, torch::Tensor len, double scale) {
  check_rowmajor(q, "q");
  check_cache(kc, "k_cache");
  check_cache(vc, "v_cache");
  TORCH_CHECK(kc.sizes() == vc.sizes(), "k / v cache shapes differ");
  const int64_t B = kc.size(0), Tmax = kc.size(1), H = kc.size(2), hd = kc.size(3);
  const bool rows = check_len(len, B);
  TORCH_CHECK(hd == 32 || hd == 64 || hd == 128, "attn_decode: head_dim 32, 64 or 128");
  TORCH_CHECK(q.size(0) == B && q.size(1) >= H * hd && q.stride(0) % 8 == 0 && q.scalar_type() == torch::kBFloat16,
              "attn_decode: q rows");
  const at::DeviceGuard g(q.device());
  auto o = torch::empty({B, H * hd}, q.options());
  const int ns = dpfs_decode_nsplit((int)Tmax);
  auto part = torch::empty({B * H * ns * (hd + 2)}, q.options().dtype(torch::kFloat32));
  (rows ? dpfs_attn_decode_rows : dpfs_attn_decode)(q.data_ptr(), q.stride(0), kc.data_ptr(), vc.data_ptr(),
                                                    len.data_ptr<int>(), o.data_ptr(), H * hd, part.data_ptr<float>(),
                                                    (int)B, (int)H, (int)hd, (int)Tmax, (float)scale, stream());
  return o;
}

// Write the k / v parts of the packed qkv rows [B, 3*H*hd] into the caches at row *len.
void kv_append(torch::Tensor qkv, torch::Tensor kc, torch::Tensor vc, torch::Tensor len) {
  check_rowmajor(qkv, "qkv");
  check_cache(kc, "k_cache");
  check_cache(vc, "v_cache");
  TORCH_CHECK(kc.sizes() == vc.sizes(), "k / v cache shapes differ");
  const int64_t B = kc.size(0), Tmax = kc.size(1), H = kc.size(2), hd = kc.size(3);
  const bool rows = check_len(len, B);
  TORCH_CHECK(qkv.size(0) == B && qkv.size(1) == 3 * H * hd && qkv.stride(0) % 8 == 0 &&
                  qkv.scalar_type() == torch::kBFloat16,
              "kv_append: qkv must be [B, 3*H*hd] bf16");
  const at::DeviceGuard g(qkv.device());
  const char* p = static_cast<const char*>(qkv.data_ptr());
  (rows ? dpfs_kv_append_rows : dpfs_kv_append)(p + H * hd * 2, p + 2 * H * hd * 2, qkv.stride(0), kc.data_ptr(),
                                                vc.data_ptr(), len.data_ptr<int>(), (int)B, (int)H, (int)hd, (int)Tmax,
                                                stream());
}

// The real new tokens of every sequence of a chunk: B device int32, or none (T for every row).
const int* check_chunk_n(const c10::optional<torch::Tensor>& n, int64_t B, const torch::Tensor& like) {
  if (!n.has_value()) return nullptr;
  check_cuda(*n, "n");
  TORCH_CHECK(n->scalar_type() == torch::kInt32 && n->is_contiguous() && n->numel() == B && n->device() == like.device(),
              "n must be a contiguous device int32 tensor of B = ", B, " elements");
  return n->data_ptr<int>();
}

// o[B*T, H*hd]: query (b, t) (row b*T + t of q, the q part of the packed qkv rows) attends keys
// [0, len[b] + t] of the cache, which already holds the chunk's rows (_kv_append_chunk).  A
// query with t >= n[b] or len[b] + t >= T_max gives zeros.  Bound with a leading underscore:
// the module's recorded public surface (tests/golden/ext_api.txt) is left as it is.
torch::Tensor attn_extend(torch::Tensor q, torch::Tensor kc, torch::Tensor vc, torch::Tensor len,
                          c10::optional<torch::Tensor> n, double scale) {
  check_rowmajor(q, "q");
  check_cache(kc, "k_cache");
  check_cache(vc, "v_cache");
  TORCH_CHECK(kc.sizes() == vc.sizes(), "k / v cache shapes differ");
  const int64_t B = kc.size(0), Tmax = kc.size(1), H = kc.size(2), hd = kc.size(3);
  const bool rows = check_len(len, B);
  TORCH_CHECK(hd == 32 || hd == 64 || hd == 128, "attn_extend: head_dim 32, 64 or 128");
  TORCH_CHECK(q.size(0) % B == 0 && q.size(0) >= B && q.size(1) >= H * hd && q.stride(0) % 8 == 0 &&
                  q.scalar_type() == torch::kBFloat16 && reinterpret_cast<uintptr_t>(q.data_ptr()) % 16 == 0,
              "attn_extend: q must be bf16 rows [B*T, >= H*hd], row stride % 8 == 0, 16-byte aligned");
  const int64_t T = q.size(0) / B;
  TORCH_CHECK(B * H <= 65535 && B * T * H * hd < (1LL << 31) && Tmax < (1LL << 30), "attn_extend: shape too large");
  const int* np = check_chunk_n(n, B, q);
  const at::DeviceGuard g(q.device());
  auto o = torch::empty({B * T, H * hd}, q.options());
  dpfs_attn_extend(q.data_ptr(), q.stride(0), kc.data_ptr(), vc.data_ptr(), len.data_ptr<int>(), rows ? 1 : 0, np,
                   o.data_ptr(), (int)B, (int)T, (int)H, (int)hd, (int)Tmax, (float)scale, stream());
  return o;
}

// The k / v parts of packed qkv row b*T + t ([B*T, 3*H*hd]) go to cache row len[b] + t, for
// t < n[b] (n none: T) and len[b] + t < T_max; nothing else is written.
void kv_append_chunk(torch::Tensor qkv, torch::Tensor kc, torch::Tensor vc, torch::Tensor len,
                     c10::optional<torch::Tensor> n) {
  check_rowmajor(qkv, "qkv");
  check_cache(kc, "k_cache");
  check_cache(vc, "v_cache");
  TORCH_CHECK(kc.sizes() == vc.sizes(), "k / v cache shapes differ");
  const int64_t B = kc.size(0), Tmax = kc.size(1), H = kc.size(2), hd = kc.size(3);
  const bool rows = check_len(len, B);
  TORCH_CHECK(qkv.size(0) % B == 0 && qkv.size(0) >= B && qkv.size(1) == 3 * H * hd && qkv.stride(0) % 8 == 0 &&
                  (H * hd) % 8 == 0 && qkv.scalar_type() == torch::kBFloat16 &&
                  reinterpret_cast<uintptr_t>(qkv.data_ptr()) % 16 == 0,
              "kv_append_chunk: qkv must be [B*T, 3*H*hd] bf16, H*hd % 8 == 0, 16-byte aligned");
  const int64_t T = qkv.size(0) / B;
  TORCH_CHECK(B * T < (1LL << 31) && Tmax < (1LL << 30), "kv_append_chunk: shape too large");
  const int* np = check_chunk_n(n, B, qkv);
  const at::DeviceGuard g(qkv.device());
  const char* p = static_cast<const char*>(qkv.data_ptr());
  dpfs_kv_append_chunk(p + H * hd * 2, p + 2 * H * hd * 2, qkv.stride(0), kc.data_ptr(), vc.data_ptr(),
                       len.data_ptr<int>(), rows ? 1 : 0, np, (int)B, (int)T, (int)H, (int)hd, (int)Tmax, stream());
}

// y[M, N] = x[M, K] w[N, K]^T (+ bias) for M <= 16 (decode-step projections); with swiglu,
// x is the packed [M, 2K] gate|up output and the operand is silu(gate) * up.
bool gemv_nt_ok(torch::Tensor x, torch::Tensor w, bool swiglu) {
  if (!x.is_cuda() || x.dim() != 2 || w.dim() != 2 || x.scalar_type() != torch::kBFloat16 ||
      w.scalar_type() != torch::kBFloat16 || x.stride(1) != 1 || w.stride(1) != 1)
    return false;
  const int64_t K = w.size(1);
  if (x.size(1) != (swiglu ? 2 * K : K)) return false;
  if (reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 || reinterpret_cast<uintptr_t>(w.data_ptr()) % 16)
    return false;   // 16-byte operand loads
  return dpfs_gemv16_ok((int)x.size(0), (int)w.size(0), (int)K, x.stride(0), w.stride(0)) != 0;
}

torch::Tensor gemv_nt(torch::Tensor x, torch::Tensor w, c10::optional<torch::Tensor> bias, bool swiglu) {
  TORCH_CHECK(gemv_nt_ok(x, w, swiglu), "gemv_nt: needs bf16 row-major x [M <= 16, K or 2K], w [N, K], K % 32 == 0");
  const int64_t M = x.size(0), N = w.size(0), K = w.size(1);
  const at::DeviceGuard g(x.device());
  auto y = torch::empty({M, N}, x.options());
  dpfs_gemv16(x.data_ptr(), x.stride(0), w.data_ptr(), w.stride(0), opt_f32(bias, N, "bias"), y.data_ptr(), N, (int)M,
              (int)N, (int)K, swiglu ? 1 : 0, stream());
  return y;
}

// rope_ on the q and k heads of the packed qkv rows + kv_append of the rotated k and v rows
// at *len, one kernel (decode step).
void rope_append(torch::Tensor qkv, torch::Tensor pos, torch::Tensor table, torch::Tensor kc, torch::Tensor vc,
                 torch::Tensor len) {
  check_rowmajor(qkv, "qkv");
  check_cache(kc, "k_cache");
  check_cache(vc, "v_cache");
  TORCH_CHECK(kc.sizes() == vc.sizes(), "k / v cache shapes differ");
  const int64_t B = kc.size(0), Tmax = kc.size(1), H = kc.size(2), hd = kc.size(3);
  const bool rows = check_len(len, B);
  TORCH_CHECK(qkv.size(0) == B && qkv.size(1) == 3 * H * hd && qkv.stride(0) % 8 == 0 &&
                  qkv.scalar_type() == torch::kBFloat16 && hd % 16 == 0,
              "rope_append: qkv must be [B, 3*H*hd] bf16, hd % 16 == 0");
  TORCH_CHECK(pos.is_cuda() && pos.scalar_type() == torch::kInt64 && pos.is_contiguous() && pos.numel() == B,
              "rope_append: pos must be contiguous int64 [B]");
  TORCH_CHECK(table.is_cuda() && table.scalar_type() == torch::kFloat32 && table.is_contiguous() &&
                  table.size(1) == hd,
              "rope_append: table must be fp32 [maxlen, hd]");
  const at::DeviceGuard g(qkv.device());
  (rows ? dpfs_rope_append_rows : dpfs_rope_append)(qkv.data_ptr(), qkv.stride(0), pos.data_ptr<int64_t>(),
                                                    table.data_ptr<float>(), kc.data_ptr(), vc.data_ptr(),
                                                    len.data_ptr<int>(), (int)B, (int)H, (int)hd, (int)Tmax, stream());
}

// ---------------------------------------------------------------------- fp8 KV cache --
// e4m3 codes (B, T_max, H, hd) with one fp32 scale per (b, t, h) row (kernels/kv8.h).  Bound with
// a leading underscore: the module's recorded public surface (tests/golden/ext_api.txt) is left
// as it is.
struct Q8Shape {
  int64_t B, Tmax, H, hd;
};

Q8Shape check_cache_q8(const torch::Tensor& k8, const torch::Tensor& v8, const torch::Tensor& ks,
                       const torch::Tensor& vs, const char* op) {
  for (const torch::Tensor* c : {&k8, &v8}) {
    check_cuda(*c, "fp8 cache");
    TORCH_CHECK(c->dim() == 4 && c->is_contiguous() && c->scalar_type() == at::kFloat8_e4m3fn, op,
                ": k8 / v8 must be contiguous float8_e4m3fn (B, T_max, H, hd) caches");
  }
  TORCH_CHECK(k8.sizes() == v8.sizes(), op, ": k8 / v8 shapes differ");
  const Q8Shape s{k8.size(0), k8.size(1), k8.size(2), k8.size(3)};
  for (const torch::Tensor* c : {&ks, &vs}) {
    check_cuda(*c, "cache scales");
    TORCH_CHECK(c->dim() == 3 && c->is_contiguous() && c->scalar_type() == torch::kFloat32 && c->size(0) == s.B &&
                    c->size(1) == s.Tmax && c->size(2) == s.H && c->device() == k8.device(),
                op, ": ks / vs must be contiguous fp32 (B, T_max, H) scales of the caches");
  }
  TORCH_CHECK(s.hd == 32 || s.hd == 64 || s.hd == 128, op, ": head_dim 32, 64 or 128");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(k8.data_ptr()) % 16 == 0 && reinterpret_cast<uintptr_t>(v8.data_ptr()) % 16 == 0,
              op, ": caches must be 16-byte aligned");
  TORCH_CHECK(s.Tmax < (1LL << 30), op, ": shape too large");
  return s;
}

// attn_decode over an fp8 cache.
torch::Tensor attn_decode_q8(torch::Tensor q, torch::Tensor k8, torch::Tensor v8, torch::Tensor ks, torch::Tensor vs,
                             torch::Tensor len, double scale) {
  check_rowmajor(q, "q");
  const Q8Shape c = check_cache_q8(k8, v8, ks, vs, "attn_decode_q8");
  const bool rows = check_len(len, c.B);
  TORCH_CHECK(q.size(0) == c.B && q.size(1) >= c.H * c.hd && q.stride(0) % 8 == 0 &&
                  q.scalar_type() == torch::kBFloat16 && reinterpret_cast<uintptr_t>(q.data_ptr()) % 16 == 0,
              "attn_decode_q8: q rows");
  const at::DeviceGuard g(q.device());
  auto o = torch::empty({c.B, c.H * c.hd}, q.options());
  const int ns = dpfs_decode_nsplit((int)c.Tmax);
  auto part = torch::empty({c.B * c.H * ns * (c.hd + 2)}, q.options().dtype(torch::kFloat32));
  dpfs_attn_decode_q8(q.data_ptr(), q.stride(0), k8.data_ptr(), v8.data_ptr(), ks.data_ptr<float>(),
                      vs.data_ptr<float>(), len.data_ptr<int>(), rows ? 1 : 0, o.data_ptr(), c.H * c.hd,
                      part.data_ptr<float>(), (int)c.B, (int)c.H, (int)c.hd, (int)c.Tmax, (float)scale, stream());
  return o;
}

// attn_extend over an fp8 cache (which already holds the chunk's rows, _kv_append_chunk_q8).
torch::Tensor attn_extend_q8(torch::Tensor q, torch::Tensor k8, torch::Tensor v8, torch::Tensor ks, torch::Tensor vs,
                             torch::Tensor len, c10::optional<torch::Tensor> n, double scale) {
  check_rowmajor(q, "q");
  const Q8Shape c = check_cache_q8(k8, v8, ks, vs, "attn_extend_q8");
  const bool rows = check_len(len, c.B);
  TORCH_CHECK(q.size(0) % c.B == 0 && q.size(0) >= c.B && q.size(1) >= c.H * c.hd && q.stride(0) % 8 == 0 &&
                  q.scalar_type() == torch::kBFloat16 && reinterpret_cast<uintptr_t>(q.data_ptr()) % 16 == 0,
              "attn_extend_q8: q must be bf16 rows [B*T, >= H*hd], row stride % 8 == 0, 16-byte aligned");
  const int64_t T = q.size(0) / c.B;
  TORCH_CHECK(c.B * c.H <= 65535 && c.B * T * c.H * c.hd < (1LL << 31), "attn_extend_q8: shape too large");
  const int* np = check_chunk_n(n, c.B, q);
  const at::DeviceGuard g(q.device());
  auto o = torch::empty({c.B * T, c.H * c.hd}, q.options());
  dpfs_attn_extend_q8(q.data_ptr(), q.stride(0), k8.data_ptr(), v8.data_ptr(), ks.data_ptr<float>(),
                      vs.data_ptr<float>(), len.data_ptr<int>(), rows ? 1 : 0, np, o.data_ptr(), (int)c.B, (int)T,
                      (int)c.H, (int)c.hd, (int)c.Tmax, (float)scale, stream());
  return o;
}

// The quantising _kv_append_chunk: the k / v parts of packed qkv row b*T + t become codes and a
// scale at cache row len[b] + t, for t < n[b] (n none: T) and len[b] + t < T_max; nothing else is
// written.
void kv_append_chunk_q8(torch::Tensor qkv, torch::Tensor k8, torch::Tensor v8, torch::Tensor ks, torch::Tensor vs,
                        torch::Tensor len, c10::optional<torch::Tensor> n) {
  check_rowmajor(qkv, "qkv");
  const Q8Shape c = check_cache_q8(k8, v8, ks, vs, "kv_append_chunk_q8");
  const bool rows = check_len(len, c.B);
  TORCH_CHECK(qkv.size(0) % c.B == 0 && qkv.size(0) >= c.B && qkv.size(1) == 3 * c.H * c.hd && qkv.stride(0) % 8 == 0 &&
                  qkv.scalar_type() == torch::kBFloat16 && reinterpret_cast<uintptr_t>(qkv.data_ptr()) % 16 == 0,
              "kv_append_chunk_q8: qkv must be [B*T, 3*H*hd] bf16, row stride % 8 == 0, 16-byte aligned");
  const int64_t T = qkv.size(0) / c.B;
  TORCH_CHECK(c.B * T * c.H * (c.hd / 8) < (1LL << 40), "kv_append_chunk_q8: shape too large");
  const int* np = check_chunk_n(n, c.B, qkv);
  const at::DeviceGuard g(qkv.device());
  const char* p = static_cast<const char*>(qkv.data_ptr());
  dpfs_kv_append_chunk_q8(p + c.H * c.hd * 2, p + 2 * c.H * c.hd * 2, qkv.stride(0), k8.data_ptr(), v8.data_ptr(),
                          ks.data_ptr<float>(), vs.data_ptr<float>(), len.data_ptr<int>(), rows ? 1 : 0, np, (int)c.B,
                          (int)T, (int)c.H, (int)c.hd, (int)c.Tmax, stream());
}

// rope_append into an fp8 cache: the rotation of rope_append, the rotated k row and the v row
// quantised at *len / len[b].
void rope_append_q8(torch::Tensor qkv, torch::Tensor pos, torch::Tensor table, torch::Tensor k8, torch::Tensor v8,
                    torch::Tensor ks, torch::Tensor vs, torch::Tensor len) {
  check_rowmajor(qkv, "qkv");
  const Q8Shape c = check_cache_q8(k8, v8, ks, vs, "rope_append_q8");
  const bool rows = check_len(len, c.B);
  TORCH_CHECK(qkv.size(0) == c.B && qkv.size(1) == 3 * c.H * c.hd && qkv.stride(0) % 8 == 0 &&
                  qkv.scalar_type() == torch::kBFloat16 && reinterpret_cast<uintptr_t>(qkv.data_ptr()) % 16 == 0,
              "rope_append_q8: qkv must be [B, 3*H*hd] bf16, row stride % 8 == 0, 16-byte aligned");
  TORCH_CHECK(pos.is_cuda() && pos.scalar_type() == torch::kInt64 && pos.is_contiguous() && pos.numel() == c.B,
              "rope_append_q8: pos must be contiguous int64 [B]");
  TORCH_CHECK(table.is_cuda() && table.scalar_type() == torch::kFloat32 && table.is_contiguous() &&
                  table.dim() == 2 && table.size(1) == c.hd,
              "rope_append_q8: table must be fp32 [maxlen, hd]");
  TORCH_CHECK(c.B * c.H * c.hd < (1LL << 27), "rope_append_q8: shape too large");
  const at::DeviceGuard g(qkv.device());
  dpfs_rope_append_q8(qkv.data_ptr(), qkv.stride(0), pos.data_ptr<int64_t>(), table.data_ptr<float>(), k8.data_ptr(),
                      v8.data_ptr(), ks.data_ptr<float>(), vs.data_ptr<float>(), len.data_ptr<int>(), rows ? 1 : 0,
                      (int)c.B, (int)c.H, (int)c.hd, (int)c.Tmax, stream());
}

// -------------------------------------------------------------------- paged KV cache --
// The layout of kernels/kv_page.h: pools (P, page, H, hd) per side, bf16 (ks / vs none) or
// float8_e4m3fn with fp32 scale pools ks / vs (P, page, H); tbl int32 (B, MP), MP = ceil(t_max /
// page), entry -1 = unmapped; len int32 [B] (a paged cache is per-row).  Shapes, dtypes and the page
// size are checked here; the table's content is device data that the kernels are safe against
// (a store through an entry outside [0, P) is dropped, a load is redirected inside the pool), so
// nothing here reads it and nothing synchronises.  Bound with leading underscores and recorded in
// tests/golden/ext_api_paged.txt (tests/test_ext_api_paged.py).
struct PagedShape {
  int64_t B, MP, P, PS, H, hd;
  int lg;
  float *ks, *vs;   // null: bf16 pools
};

PagedShape check_paged(const torch::Tensor& kp, const torch::Tensor& vp, const c10::optional<torch::Tensor>& ks,
                       const c10::optional<torch::Tensor>& vs, const torch::Tensor& tbl, const torch::Tensor& len,
                       int64_t t_max, int64_t page, const char* op) {
  TORCH_CHECK(page >= 16 && page <= 256 && (page & (page - 1)) == 0, op,
              ": the page size must be a power of two in [16, 256], got ", page);
  TORCH_CHECK(ks.has_value() == vs.has_value(), op, ": ks and vs are given together (fp8 pools) or not at all");
  const bool q8 = ks.has_value();
  const auto want = q8 ? at::kFloat8_e4m3fn : at::kBFloat16;
  for (const torch::Tensor* c : {&kp, &vp}) {
    check_cuda(*c, "pool");
    TORCH_CHECK(c->dim() == 4 && c->is_contiguous() && c->scalar_type() == want && c->size(1) == page, op,
                ": k_pool / v_pool must be contiguous ", want, " (P, page = ", page, ", H, hd) pools, got ", c->sizes(),
                " of ", c->scalar_type());
    TORCH_CHECK(reinterpret_cast<uintptr_t>(c->data_ptr()) % 16 == 0, op, ": pools must be 16-byte aligned");
  }
  TORCH_CHECK(kp.sizes() == vp.sizes() && kp.device() == vp.device(), op, ": k_pool / v_pool differ");
  PagedShape s{0, 0, kp.size(0), page, kp.size(2), kp.size(3), 0, nullptr, nullptr};
  while ((1LL << s.lg) < page) ++s.lg;
  TORCH_CHECK(s.hd == 32 || s.hd == 64 || s.hd == 128, op, ": head_dim 32, 64 or 128");
  TORCH_CHECK(s.P >= 1 && s.P * s.PS < (1LL << 31), op, ": the pool needs 1 <= P and P * page < 2^31 rows");
  if (q8) {
    for (const torch::Tensor* c : {&*ks, &*vs}) {
      check_cuda(*c, "pool scales");
      TORCH_CHECK(c->dim() == 3 && c->is_contiguous() && c->scalar_type() == torch::kFloat32 && c->size(0) == s.P &&
                      c->size(1) == s.PS && c->size(2) == s.H && c->device() == kp.device(),
                  op, ": ks / vs must be contiguous fp32 (P, page, H) scale pools");
    }
    s.ks = ks->data_ptr<float>();
    s.vs = vs->data_ptr<float>();
  }
  TORCH_CHECK(t_max >= 1 && t_max < (1LL << 30), op, ": t_max must be in [1, 2^30), got ", t_max);
  check_cuda(tbl, "tbl");
  TORCH_CHECK(tbl.scalar_type() == torch::kInt32 && tbl.dim() == 2 && tbl.is_contiguous() && tbl.size(0) >= 1 &&
                  tbl.size(1) == (t_max + page - 1) / page && tbl.device() == kp.device(),
              op, ": tbl must be a contiguous device int32 (B, MP = ceil(t_max / page) = ", (t_max + page - 1) / page,
              ") table, got ", tbl.sizes(), " of ", tbl.scalar_type());
  s.B = tbl.size(0);
  s.MP = tbl.size(1);
  check_cuda(len, "len");
  TORCH_CHECK(len.scalar_type() == torch::kInt32 && len.is_contiguous() && len.numel() == s.B &&
                  len.device() == kp.device(),
              op, ": len must be a contiguous device int32 tensor of B = ", s.B, " elements (a paged cache is per-row)");
  return s;
}

// attn_decode (per-row form) / _attn_decode_q8 through a block table: same grid, splits and math
// over the logical key index, so the output equals the contiguous launch on the same cache
// content bit for bit.
torch::Tensor attn_decode_paged(torch::Tensor q, torch::Tensor kp, torch::Tensor vp, c10::optional<torch::Tensor> ks,
                                c10::optional<torch::Tensor> vs, torch::Tensor tbl, torch::Tensor len, int64_t t_max,
                                int64_t page, double scale) {
  check_rowmajor(q, "q");
  const PagedShape c = check_paged(kp, vp, ks, vs, tbl, len, t_max, page, "attn_decode_paged");
  TORCH_CHECK(q.size(0) == c.B && q.size(1) >= c.H * c.hd && q.stride(0) % 8 == 0 &&
                  q.scalar_type() == torch::kBFloat16 && reinterpret_cast<uintptr_t>(q.data_ptr()) % 16 == 0,
              "attn_decode_paged: q rows");
  TORCH_CHECK(c.B * c.H <= 65535, "attn_decode_paged: shape too large");
  const at::DeviceGuard g(q.device());
  auto o = torch::empty({c.B, c.H * c.hd}, q.options());
  const int ns = dpfs_decode_nsplit((int)t_max);
  auto part = torch::empty({c.B * c.H * ns * (c.hd + 2)}, q.options().dtype(torch::kFloat32));
  dpfs_attn_decode_paged(q.data_ptr(), q.stride(0), kp.data_ptr(), vp.data_ptr(), c.ks, c.vs, tbl.data_ptr<int>(),
                         (int)c.MP, (int)c.P, c.lg, len.data_ptr<int>(), o.data_ptr(), c.H * c.hd,
                         part.data_ptr<float>(), (int)c.B, (int)c.H, (int)c.hd, (int)t_max, (float)scale, stream());
  return o;
}

// rope_append (per-row form) / _rope_append_q8 through a block table.
void rope_append_paged(torch::Tensor qkv, torch::Tensor pos, torch::Tensor table, torch::Tensor kp, torch::Tensor vp,
                       c10::optional<torch::Tensor> ks, c10::optional<torch::Tensor> vs, torch::Tensor tbl,
                       torch::Tensor len, int64_t t_max, int64_t page) {
  check_rowmajor(qkv, "qkv");
  const PagedShape c = check_paged(kp, vp, ks, vs, tbl, len, t_max, page, "rope_append_paged");
  TORCH_CHECK(qkv.size(0) == c.B && qkv.size(1) == 3 * c.H * c.hd && qkv.stride(0) % 8 == 0 &&
                  qkv.scalar_type() == torch::kBFloat16 && reinterpret_cast<uintptr_t>(qkv.data_ptr()) % 16 == 0,
              "rope_append_paged: qkv must be [B, 3*H*hd] bf16, row stride % 8 == 0, 16-byte aligned");
  TORCH_CHECK(pos.is_cuda() && pos.scalar_type() == torch::kInt64 && pos.is_contiguous() && pos.numel() == c.B,
              "rope_append_paged: pos must be contiguous int64 [B]");
  TORCH_CHECK(table.is_cuda() && table.scalar_type() == torch::kFloat32 && table.is_contiguous() &&
                  table.dim() == 2 && table.size(1) == c.hd,
              "rope_append_paged: table must be fp32 [maxlen, hd]");
  TORCH_CHECK(c.B * c.H * c.hd < (1LL << 27), "rope_append_paged: shape too large");
  const at::DeviceGuard g(qkv.device());
  if (c.ks)
    dpfs_rope_append_q8_paged(qkv.data_ptr(), qkv.stride(0), pos.data_ptr<int64_t>(), table.data_ptr<float>(),
                              kp.data_ptr(), vp.data_ptr(), c.ks, c.vs, tbl.data_ptr<int>(), (int)c.MP, (int)c.P, c.lg,
                              len.data_ptr<int>(), (int)c.B, (int)c.H, (int)c.hd, (int)t_max, stream());
  else
    dpfs_rope_append_paged(qkv.data_ptr(), qkv.stride(0), pos.data_ptr<int64_t>(), table.data_ptr<float>(),
                           kp.data_ptr(), vp.data_ptr(), tbl.data_ptr<int>(), (int)c.MP, (int)c.P, c.lg,
                           len.data_ptr<int>(), (int)c.B, (int)c.H, (int)c.hd, (int)t_max, stream());
}

// _kv_append_chunk / _kv_append_chunk_q8 through a block table.
void kv_append_chunk_paged(torch::Tensor qkv, torch::Tensor kp, torch::Tensor vp, c10::optional<torch::Tensor> ks,
                           c10::optional<torch::Tensor> vs, torch::Tensor tbl, torch::Tensor len,
                           c10::optional<torch::Tensor> n, int64_t t_max, int64_t page) {
  check_rowmajor(qkv, "qkv");
  const PagedShape c = check_paged(kp, vp, ks, vs, tbl, len, t_max, page, "kv_append_chunk_paged");
  TORCH_CHECK(qkv.size(0) % c.B == 0 && qkv.size(0) >= c.B && qkv.size(1) == 3 * c.H * c.hd && qkv.stride(0) % 8 == 0 &&
                  qkv.scalar_type() == torch::kBFloat16 && reinterpret_cast<uintptr_t>(qkv.data_ptr()) % 16 == 0,
              "kv_append_chunk_paged: qkv must be [B*T, 3*H*hd] bf16, row stride % 8 == 0, 16-byte aligned");
  const int64_t T = qkv.size(0) / c.B;
  TORCH_CHECK(c.B * T < (1LL << 31) && c.B * T * c.H * (c.hd / 8) < (1LL << 40), "kv_append_chunk_paged: shape too large");
  const int* np = check_chunk_n(n, c.B, qkv);
  const at::DeviceGuard g(qkv.device());
  const char* p = static_cast<const char*>(qkv.data_ptr());
  if (c.ks)
    dpfs_kv_append_chunk_q8_paged(p + c.H * c.hd * 2, p + 2 * c.H * c.hd * 2, qkv.stride(0), kp.data_ptr(),
                                  vp.data_ptr(), c.ks, c.vs, tbl.data_ptr<int>(), (int)c.MP, (int)c.P, c.lg,
                                  len.data_ptr<int>(), np, (int)c.B, (int)T, (int)c.H, (int)c.hd, (int)t_max, stream());
  else
    dpfs_kv_append_chunk_paged(p + c.H * c.hd * 2, p + 2 * c.H * c.hd * 2, qkv.stride(0), kp.data_ptr(), vp.data_ptr(),
                               tbl.data_ptr<int>(), (int)c.MP, (int)c.P, c.lg, len.data_ptr<int>(), np, (int)c.B,
                               (int)T, (int)c.H, (int)c.hd, (int)t_max, stream());
}

// _attn_extend / _attn_extend_q8 through a block table (the pools already hold the chunk's rows):
// the same tiles over the logical key index, bit-identical to the contiguous launch.
torch::Tensor attn_extend_paged(torch::Tensor q, torch::Tensor kp, torch::Tensor vp, c10::optional<torch::Tensor> ks,
                                c10::optional<torch::Tensor> vs, torch::Tensor tbl, torch::Tensor len,
                                c10::optional<torch::Tensor> n, int64_t t_max, int64_t page, double scale) {
  check_rowmajor(q, "q");
  const PagedShape c = check_paged(kp, vp, ks, vs, tbl, len, t_max, page, "attn_extend_paged");
  TORCH_CHECK(q.size(0) % c.B == 0 && q.size(0) >= c.B && q.size(1) >= c.H * c.hd && q.stride(0) % 8 == 0 &&
                  q.scalar_type() == torch::kBFloat16 && reinterpret_cast<uintptr_t>(q.data_ptr()) % 16 == 0,
              "attn_extend_paged: q must be bf16 rows [B*T, >= H*hd], row stride % 8 == 0, 16-byte aligned");
  const int64_t T = q.size(0) / c.B;
  TORCH_CHECK(c.B * c.H <= 65535 && c.B * T * c.H * c.hd < (1LL << 31), "attn_extend_paged: shape too large");
  const int* np = check_chunk_n(n, c.B, q);
  const at::DeviceGuard g(q.device());
  auto o = torch::empty({c.B * T, c.H * c.hd}, q.options());
  dpfs_attn_extend_paged(q.data_ptr(), q.stride(0), kp.data_ptr(), vp.data_ptr(), c.ks, c.vs, tbl.data_ptr<int>(),
                         (int)c.MP, (int)c.P, c.lg, len.data_ptr<int>(), np, o.data_ptr(), (int)c.B, (int)T, (int)c.H,
                         (int)c.hd, (int)t_max, (float)scale, stream());
  return o;
}

// Per-tensor fp8 quantisation with current scaling: (q, inv) with q = sat(x * FMAX / amax)
// in float8_e4m3fn (fmt 0) or float8_e5m2 (fmt 1), inv = amax / FMAX as an fp32 0-d tensor
// (the scale torch._scaled_mm multiplies back).  No host synchronisation.
std::vector<torch::Tensor> fp8_quant(torch::Tensor x, int64_t fmt) {
  check_cuda(x, "x");
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16 && x.is_contiguous() && x.numel() % 8 == 0 &&
                  reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0,
              "fp8_quant: x must be contiguous bf16 with numel % 8 == 0");
  TORCH_CHECK(fmt == 0 || fmt == 1, "fp8_quant: fmt 0 (e4m3) or 1 (e5m2)");
  const at::DeviceGuard g(x.device());
  auto q = torch::empty(x.sizes(), x.options().dtype(fmt == 0 ? at::kFloat8_e4m3fn : at::kFloat8_e5m2));
  auto inv = torch::empty({}, x.options().dtype(torch::kFloat32));
  auto work = torch::empty({dpfs_fp8_work_floats()}, x.options().dtype(torch::kFloat32));
  if (x.numel())
    dpfs_fp8_quant(x.data_ptr(), x.numel(), (int)fmt, q.data_ptr(), inv.data_ptr<float>(), work.data_ptr<float>(),
                   stream());
  else
    inv.fill_(1.0);
  return {q, inv};
}

// *len += 1 and pos[:] = *len on the device (end of a decode step; graph-replayable).  The
// uniform form only: a per-row len goes through step_advance_rows, which needs the capacity.
void step_advance(torch::Tensor len, torch::Tensor pos) {
  check_cuda(len, "len");
  TORCH_CHECK(len.scalar_type() == torch::kInt32 && len.numel() == 1,
              "step_advance: len must be a device int32 scalar (per-row lengths: _step_advance_rows(len, pos, t_max))");
  check_cuda(pos, "pos");
  TORCH_CHECK(pos.scalar_type() == torch::kInt64 && pos.is_contiguous(), "pos must be contiguous int64");
  const at::DeviceGuard g(len.device());
  dpfs_step_advance(len.data_ptr<int>(), pos.data_ptr<int64_t>(), (int)pos.numel(), stream());
}

// Per-row end of a decode step: len[b] = min(len[b] + 1, t_max) and pos[b] = min(len[b],
// t_max - 1) for each of the B sequences, so a row that fills its cache (capacity t_max) is
// frozen there.  Bound as _step_advance_rows: the module's recorded public surface
// (tests/golden/ext_api.txt) is left as it is.
void step_advance_rows(torch::Tensor len, torch::Tensor pos, int64_t t_max) {
  check_cuda(pos, "pos");
  TORCH_CHECK(pos.scalar_type() == torch::kInt64 && pos.is_contiguous(), "pos must be contiguous int64");
  const int64_t B = pos.numel();
  check_len(len, B);
  TORCH_CHECK(len.numel() == B, "step_advance_rows: len must have one element per pos entry, got ", len.numel(),
              " for ", B);
  TORCH_CHECK(len.device() == pos.device(), "len and pos must be on the same device");
  TORCH_CHECK(t_max >= 1 && t_max < (1LL << 31), "step_advance_rows: t_max must be in [1, 2^31), got ", t_max);
  const at::DeviceGuard g(len.device());
  dpfs_step_advance_rows(len.data_ptr<int>(), pos.data_ptr<int64_t>(), (int)B, (int)t_max, stream());
}

// Temperature / top-k / top-p sampling of one token per row (kernels/sample.hip): logits
// [B, >= vocab] bf16 / fp32 with unit column stride, columns >= vocab are padding.  What the
// scalar and the per-row launch share, in two steps so that the scalar call checks its arguments
// in the order it always has: the logits / vocab checks, then the pos / u checks and the outputs.
struct SampleCall {
  int dt;
  int64_t B, ld;
  bool vec_ok;
  const float* u;
  torch::Tensor ids, kept, thresh, uo;
};

SampleCall sample_rows(const torch::Tensor& logits, int64_t vocab, const char* op) {
  check_rowmajor(logits, "logits");
  SampleCall c;
  c.dt = dcode(logits);
  c.B = logits.size(0);
  c.ld = logits.stride(0);
  const int64_t vec = c.dt == 1 ? 8 : 4;
  TORCH_CHECK(vocab >= 1 && vocab <= logits.size(1) && vocab < (1LL << 31) && (c.B <= 1 || c.ld >= logits.size(1)), op,
              ": 1 <= vocab <= ld, got vocab ", vocab, " for rows of ", logits.size(1));
  // 16-byte row loads need aligned rows whose last vector lies inside the row
  const int64_t esz = c.dt == 1 ? 2 : 4;
  c.vec_ok = reinterpret_cast<uintptr_t>(logits.data_ptr()) % 16 == 0 && (c.B <= 1 || c.ld * esz % 16 == 0) &&
             (vocab + vec - 1) / vec * vec <= logits.size(1);
  return c;
}

// (the caller holds a DeviceGuard of the logits' device)
void sample_outputs(SampleCall& c, const torch::Tensor& pos, const c10::optional<torch::Tensor>& u, const char* op) {
  TORCH_CHECK(pos.is_cuda() && pos.scalar_type() == torch::kInt64 && pos.is_contiguous() && pos.numel() == c.B, op,
              ": pos must be contiguous int64 [B]");
  c.u = opt_f32(u, c.B, "u");
  c.ids = torch::empty({c.B}, pos.options());
  c.kept = torch::empty({c.B}, pos.options().dtype(torch::kInt32));
  c.thresh = torch::empty({c.B}, pos.options().dtype(torch::kFloat32));
  c.uo = torch::empty({c.B}, pos.options().dtype(torch::kFloat32));
}

// One (temperature, top_k, top_p, seed) for every row.  top_k 0 or >= vocab and top_p 1 are
// off.  The uniform of row b is Philox4x32-10(key seed, counter (pos[b], b, 0)) unless `u` [B]
// supplies it (tests).  Returns (ids int64, kept int32, thresh fp32, u fp32), each [B].  No host
// synchronisation: graph-capturable.
py::tuple sample_logits(torch::Tensor logits, int64_t vocab, double temperature, int64_t top_k, double top_p,
                        int64_t seed, torch::Tensor pos, c10::optional<torch::Tensor> u) {
  SampleCall c = sample_rows(logits, vocab, "sample_logits");
  TORCH_CHECK(temperature > 0.0, "sample_logits: temperature must be > 0, got ", temperature);
  TORCH_CHECK(top_p > 0.0 && top_p <= 1.0, "sample_logits: top_p must be in (0, 1], got ", top_p);
  TORCH_CHECK(top_k >= 0, "sample_logits: top_k must be >= 0, got ", top_k);
  const at::DeviceGuard g(logits.device());
  sample_outputs(c, pos, u, "sample_logits");
  const int k = (int)std::min<int64_t>(top_k, vocab);
  dpfs_sample_logits(logits.data_ptr(), c.dt, c.ld, (int)c.B, (int)vocab, c.vec_ok ? 1 : 0,
                     (float)(1.0 / temperature), k, top_p, (unsigned long long)seed, pos.data_ptr<int64_t>(), c.u,
                     c.ids.data_ptr<int64_t>(), c.kept.data_ptr<int>(), c.thresh.data_ptr<float>(),
                     c.uo.data_ptr<float>(), stream());
  return py::make_tuple(c.ids, c.kept, c.thresh, c.uo);
}

// One setting of a per-row launch: B values of `type` in the logits' device memory.
const void* row_setting(const torch::Tensor& t, at::ScalarType type, const torch::Tensor& logits, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.device() == logits.device() && t.scalar_type() == type && t.dim() == 1 &&
                  t.is_contiguous() && t.numel() == logits.size(0),
              "sample_logits_rows: ", name, " must be a contiguous ", type, " tensor of B = ", logits.size(0),
              " elements on the device of logits, got ", t.sizes(), " of ", t.scalar_type(), " on ", t.device());
  return t.data_ptr();
}

// sample_logits with the settings of every row in device memory: inv_t fp32 = fp32(1 / T), 0
// marks a greedy row (ids = the first maximum, kept = the number of maxima, thresh = the
// maximum, u = 0); top_k int32, <= 0 or >= vocab is off; top_p fp64, >= 1 is off; seed int64, the
// Philox key; rid int32, the counter word where the scalar form puts the row index.  The device
// values are not read here (their range is the caller's to check where the lists come from): no
// host synchronisation, graph-capturable, and one captured launch serves every setting.  Bound as
// _sample_logits_rows: tests/golden/ext_api.txt, which records the public names, cannot change
// with this function, so its signature and docstring are recorded in
// tests/golden/ext_api_sample_rows.txt instead (tests/test_ext_api_sample_rows.py).
py::tuple sample_logits_rows(torch::Tensor logits, int64_t vocab, torch::Tensor inv_t, torch::Tensor top_k,
                             torch::Tensor top_p, torch::Tensor seed, torch::Tensor rid, torch::Tensor pos,
                             c10::optional<torch::Tensor> u) {
  SampleCall c = sample_rows(logits, vocab, "sample_logits_rows");
  const at::DeviceGuard g(logits.device());
  sample_outputs(c, pos, u, "sample_logits_rows");
  TORCH_CHECK(pos.device() == logits.device() && (c.u == nullptr || u->device() == logits.device()),
              "sample_logits_rows: pos and u must be on the device of logits");
  const auto* it = static_cast<const float*>(row_setting(inv_t, torch::kFloat32, logits, "inv_t"));
  const auto* tk = static_cast<const int*>(row_setting(top_k, torch::kInt32, logits, "top_k"));
  const auto* tp = static_cast<const double*>(row_setting(top_p, torch::kFloat64, logits, "top_p"));
  const auto* sd = static_cast<const int64_t*>(row_setting(seed, torch::kInt64, logits, "seed"));
  const auto* ri = static_cast<const int*>(row_setting(rid, torch::kInt32, logits, "rid"));
  dpfs_sample_logits_rows(logits.data_ptr(), c.dt, c.ld, (int)c.B, (int)vocab, c.vec_ok ? 1 : 0, it, tk, tp, sd, ri,
                          pos.data_ptr<int64_t>(), c.u, c.ids.data_ptr<int64_t>(), c.kept.data_ptr<int>(),
                          c.thresh.data_ptr<float>(), c.uo.data_ptr<float>(), stream());
  return py::make_tuple(c.ids, c.kept, c.thresh, c.uo);
}

// One setting of the penalised launch: as row_setting, under that launch's name.
const void* pen_setting(const torch::Tensor& t, at::ScalarType type, const torch::Tensor& logits, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.device() == logits.device() && t.scalar_type() == type && t.dim() == 1 &&
                  t.is_contiguous() && t.numel() == logits.size(0),
              "sample_logits_pen: ", name, " must be a contiguous ", type, " tensor of B = ", logits.size(0),
              " elements on the device of logits, got ", t.sizes(), " of ", t.scalar_type(), " on ", t.device());
  return t.data_ptr();
}

// _sample_logits_rows on penalised logits, with the token history of every row as device state
// and two log-probabilities per row (ops/reference.py:sample_logits_pen is the contract).  rep,
// inv_rep = fp32(1 / rep), pres, freq: fp32 [B].  hist: int32 [B, >= vocab], unit column stride;
// bit 31 of hist[b, i] says that id i occurs in row b's prompt, bits 0..30 count c, the times this
// launch has drawn i for the row.  Column i of row b is sampled as
//   x = fp32(logit); if hist != 0: x = x > 0 ? x * inv_rep : x * rep; x = x - freq * fp32(c);
//   if c > 0: x = x - pres
// (every operation rounded to fp32), and kept / thresh are in units of x.  With update the launch
// then adds 1 to hist[b, ids[b]] in place.  Returns (ids int64 [B], kept int32 [B], thresh fp32 [B],
// u fp32 [B], logp fp32 [B, 2]): logp[b, 0] is the log-probability of ids[b] under the softmax of
// the raw logits (temperature 1, no penalty, no filter), logp[b, 1] under the distribution the
// draw used (-log(number of maxima) on a greedy row).  The device values are not read here: no
// host synchronisation, graph-capturable.  Recorded in tests/golden/ext_api_sample_pen.txt
// (tests/test_ext_api_sample_pen.py).
py::tuple sample_logits_pen(torch::Tensor logits, int64_t vocab, torch::Tensor inv_t, torch::Tensor top_k,
                            torch::Tensor top_p, torch::Tensor seed, torch::Tensor rid, torch::Tensor rep,
                            torch::Tensor inv_rep, torch::Tensor pres, torch::Tensor freq, torch::Tensor hist,
                            torch::Tensor pos, c10::optional<torch::Tensor> u, bool update) {
  SampleCall c = sample_rows(logits, vocab, "sample_logits_pen");
  const at::DeviceGuard g(logits.device());
  sample_outputs(c, pos, u, "sample_logits_pen");
  TORCH_CHECK(pos.device() == logits.device() && (c.u == nullptr || u->device() == logits.device()),
              "sample_logits_pen: pos and u must be on the device of logits");
  const auto* it = static_cast<const float*>(pen_setting(inv_t, torch::kFloat32, logits, "inv_t"));
  const auto* tk = static_cast<const int*>(pen_setting(top_k, torch::kInt32, logits, "top_k"));
  const auto* tp = static_cast<const double*>(pen_setting(top_p, torch::kFloat64, logits, "top_p"));
  const auto* sd = static_cast<const int64_t*>(pen_setting(seed, torch::kInt64, logits, "seed"));
  const auto* ri = static_cast<const int*>(pen_setting(rid, torch::kInt32, logits, "rid"));
  const auto* rp = static_cast<const float*>(pen_setting(rep, torch::kFloat32, logits, "rep"));
  const auto* ir = static_cast<const float*>(pen_setting(inv_rep, torch::kFloat32, logits, "inv_rep"));
  const auto* pr = static_cast<const float*>(pen_setting(pres, torch::kFloat32, logits, "pres"));
  const auto* fr = static_cast<const float*>(pen_setting(freq, torch::kFloat32, logits, "freq"));
  TORCH_CHECK(hist.is_cuda() && hist.device() == logits.device() && hist.scalar_type() == torch::kInt32 &&
                  hist.dim() == 2 && hist.size(0) == c.B && hist.stride(1) == 1,
              "sample_logits_pen: hist must be an int32 [B = ", c.B, ", >= vocab] tensor with unit column stride on "
              "the device of logits, got ", hist.sizes(), " of ", hist.scalar_type(), " on ", hist.device());
  const int64_t ld_h = hist.stride(0);
  TORCH_CHECK(hist.size(1) >= vocab && (c.B <= 1 || ld_h >= hist.size(1)),
              "sample_logits_pen: hist needs vocab = ", vocab, " <= columns <= row stride, got rows of ", hist.size(1),
              " with stride ", ld_h);
  // 16-byte history loads: aligned rows that hold the last vector of the logits' layout
  const int64_t vec = c.dt == 1 ? 8 : 4;
  const bool hvec_ok = reinterpret_cast<uintptr_t>(hist.data_ptr()) % 16 == 0 && (c.B <= 1 || ld_h % 4 == 0) &&
                       (vocab + vec - 1) / vec * vec <= hist.size(1);
  auto logp = torch::empty({c.B, 2}, c.thresh.options());
  dpfs_sample_logits_pen(logits.data_ptr(), c.dt, c.ld, (int)c.B, (int)vocab, c.vec_ok ? 1 : 0, it, tk, tp, sd, ri, rp,
                         ir, pr, fr, hist.data_ptr<int>(), ld_h, hvec_ok ? 1 : 0, update ? 1 : 0,
                         pos.data_ptr<int64_t>(), c.u, c.ids.data_ptr<int64_t>(), c.kept.data_ptr<int>(),
                         c.thresh.data_ptr<float>(), c.uo.data_ptr<float>(), logp.data_ptr<float>(), stream());
  return py::make_tuple(c.ids, c.kept, c.thresh, c.uo, logp);
}

}  // namespace

void bind_decode(py::module_& m) {
  m.def("attn_decode", &attn_decode, py::arg("q"), py::arg("k_cache"), py::arg("v_cache"), py::arg("len"),
        py::arg("scale"));
  m.def("kv_append", &kv_append, py::arg("qkv"), py::arg("k_cache"), py::arg("v_cache"), py::arg("len"));
  m.def("step_advance", &step_advance, py::arg("len"), py::arg("pos"));
  m.def("_step_advance_rows", &step_advance_rows, py::arg("len"), py::arg("pos"), py::arg("t_max"));
  m.def("_attn_extend", &attn_extend, py::arg("q"), py::arg("k_cache"), py::arg("v_cache"), py::arg("len"),
        py::arg("n"), py::arg("scale"));
  m.def("_kv_append_chunk", &kv_append_chunk, py::arg("qkv"), py::arg("k_cache"), py::arg("v_cache"), py::arg("len"),
        py::arg("n") = py::none());
  m.def("_attn_decode_q8", &attn_decode_q8, py::arg("q"), py::arg("k8"), py::arg("v8"), py::arg("ks"), py::arg("vs"),
        py::arg("len"), py::arg("scale"));
  m.def("_attn_extend_q8", &attn_extend_q8, py::arg("q"), py::arg("k8"), py::arg("v8"), py::arg("ks"), py::arg("vs"),
        py::arg("len"), py::arg("n"), py::arg("scale"));
  m.def("_kv_append_chunk_q8", &kv_append_chunk_q8, py::arg("qkv"), py::arg("k8"), py::arg("v8"), py::arg("ks"),
        py::arg("vs"), py::arg("len"), py::arg("n") = py::none());
  m.def("_rope_append_q8", &rope_append_q8, py::arg("qkv"), py::arg("pos"), py::arg("table"), py::arg("k8"),
        py::arg("v8"), py::arg("ks"), py::arg("vs"), py::arg("len"));
  m.def("_attn_decode_paged", &attn_decode_paged, py::arg("q"), py::arg("k_pool"), py::arg("v_pool"), py::arg("ks"),
        py::arg("vs"), py::arg("tbl"), py::arg("len"), py::arg("t_max"), py::arg("page"), py::arg("scale"));
  m.def("_rope_append_paged", &rope_append_paged, py::arg("qkv"), py::arg("pos"), py::arg("table"), py::arg("k_pool"),
        py::arg("v_pool"), py::arg("ks"), py::arg("vs"), py::arg("tbl"), py::arg("len"), py::arg("t_max"),
        py::arg("page"));
  m.def("_kv_append_chunk_paged", &kv_append_chunk_paged, py::arg("qkv"), py::arg("k_pool"), py::arg("v_pool"),
        py::arg("ks"), py::arg("vs"), py::arg("tbl"), py::arg("len"), py::arg("n"), py::arg("t_max"), py::arg("page"));
  m.def("_attn_extend_paged", &attn_extend_paged, py::arg("q"), py::arg("k_pool"), py::arg("v_pool"), py::arg("ks"),
        py::arg("vs"), py::arg("tbl"), py::arg("len"), py::arg("n"), py::arg("t_max"), py::arg("page"),
        py::arg("scale"));
  m.def("fp8_quant", &fp8_quant, py::arg("x"), py::arg("fmt") = 0);
  m.def("gemv_nt_ok", &gemv_nt_ok, py::arg("x"), py::arg("w"), py::arg("swiglu") = false);
  m.def("gemv_nt", &gemv_nt, py::arg("x"), py::arg("w"), py::arg("bias") = py::none(), py::arg("swiglu") = false);
  m.def("rope_append", &rope_append, py::arg("qkv"), py::arg("pos"), py::arg("table"), py::arg("k_cache"),
        py::arg("v_cache"), py::arg("len"));
  m.def("sample_logits", &sample_logits, py::arg("logits"), py::arg("vocab"), py::arg("temperature"), py::arg("top_k"),
        py::arg("top_p"), py::arg("seed"), py::arg("pos"), py::arg("u") = py::none());
  m.def("_sample_logits_rows", &sample_logits_rows, py::arg("logits"), py::arg("vocab"), py::arg("inv_t"),
        py::arg("top_k"), py::arg("top_p"), py::arg("seed"), py::arg("rid"), py::arg("pos"), py::arg("u") = py::none());
  m.def("_sample_logits_pen", &sample_logits_pen, py::arg("logits"), py::arg("vocab"), py::arg("inv_t"),
        py::arg("top_k"), py::arg("top_p"), py::arg("seed"), py::arg("rid"), py::arg("rep"), py::arg("inv_rep"),
        py::arg("pres"), py::arg("freq"), py::arg("hist"), py::arg("pos"), py::arg("u") = py::none(),
        py::arg("update") = true);
}
