#include "common.h"

namespace {

// ------------------------------------------------------------------- embedding / CE --
torch::Tensor embedding_fwd(torch::Tensor ids, torch::Tensor weight, int64_t vocab_start, py::object out_dtype) {
  check_cuda(ids, "ids");
  check_cuda(weight, "weight");
  TORCH_CHECK(ids.scalar_type() == torch::kInt64 && ids.is_contiguous() && ids.dim() == 1, "embedding: ids int64 [M]");
  TORCH_CHECK(weight.scalar_type() == torch::kFloat32 && weight.is_contiguous() && weight.dim() == 2 &&
                  weight.size(1) % 4 == 0,
              "embedding: weight must be contiguous fp32 [V_local, D], D % 4 == 0");
  const auto odt = torch::python::detail::py_object_to_dtype(out_dtype);
  TORCH_CHECK(odt == torch::kBFloat16 || odt == torch::kFloat32, "embedding: out dtype bf16/fp32");
  const at::DeviceGuard g(ids.device());
  const int64_t M = ids.numel(), D = weight.size(1);
  auto out = torch::empty({M, D}, weight.options().dtype(odt));
  if (M) dpfs_embedding_fwd(odt == torch::kBFloat16 ? 1 : 0, ids.data_ptr<int64_t>(), weight.data_ptr<float>(),
                            out.data_ptr(), (int)M, (int)D, vocab_start, (int)weight.size(0), stream());
  return out;
}

void check_emb_out(const torch::Tensor& dw, const char* op, int64_t v_local, int64_t D, const torch::Tensor& dout) {
  TORCH_CHECK(dw.scalar_type() == torch::kFloat32 && dw.is_contiguous() && dw.dim() == 2 && dw.size(0) == v_local &&
                  dw.size(1) == D && dw.device() == dout.device(),
              op, ": out must be contiguous fp32 [v_local, D] on the device of dout");
}

// fp32 dW[v_local, D] of the masked embedding; with ``out`` the rows are ADDED to it (the
// engines' gradient arena: zeroed once per step, every chunk accumulates).
torch::Tensor embedding_bwd(torch::Tensor dout, torch::Tensor ids, int64_t v_local, int64_t vocab_start,
                            c10::optional<torch::Tensor> out) {
  check_rowmajor(dout, "dout");
  TORCH_CHECK(dout.is_contiguous(), "embedding_bwd: dout contiguous");
  TORCH_CHECK(ids.scalar_type() == torch::kInt64 && ids.is_contiguous() && ids.numel() == dout.size(0),
              "embedding_bwd: ids");
  const at::DeviceGuard g(dout.device());
  const int64_t M = dout.size(0), D = dout.size(1);
  torch::Tensor dw;
  if (out.has_value()) {
    dw = *out;
    check_emb_out(dw, "embedding_bwd", v_local, D, dout);
  } else {
    dw = torch::zeros({v_local, D}, dout.options().dtype(torch::kFloat32));
  }
  if (M) dpfs_embedding_bwd(dcode(dout), dout.data_ptr(), ids.data_ptr<int64_t>(), dw.data_ptr<float>(), (int)M,
                            (int)D, vocab_start, (int)v_local, stream());
  return dw;
}

// Deterministic embedding gradient (no atomics): the ids sorted (stable), each local vocab row's
// segment found by binary search, one wave per vocab row sums its rows in row order and WRITES
// dw (every row: no zero pass), or adds to it (`accumulate`).  D % 4 == 0 (else the atomic form).
// Stable order of the ids by local vocab row (ids outside [vocab_start, vocab_start + v_local)
// last) and each row's segment start: the deterministic embedding backward's index
// (embedding_bwd_sorted); a two-pass radix sort on our kernels (embedding_ce.hip).
std::vector<torch::Tensor> emb_sort(torch::Tensor ids, int64_t vocab_start, int64_t v_local) {
  check_cuda(ids, "ids");
  TORCH_CHECK(ids.scalar_type() == torch::kInt64 && ids.is_contiguous(), "emb_sort: ids int64 contiguous");
  TORCH_CHECK(v_local >= 0 && v_local < 65535, "emb_sort: the local vocab must be below 65535 rows");
  TORCH_CHECK(ids.numel() < (1LL << 31), "emb_sort: too many ids");
  const at::DeviceGuard g(ids.device());
  const int M = (int)ids.numel();
  auto ws = torch::empty({dpfs_emb_sort_ws(M)}, ids.options().dtype(torch::kInt32));
  auto perm = torch::empty({M}, ids.options());
  auto seg = torch::empty({v_local + 1}, ids.options());
  dpfs_emb_sort(ids.data_ptr<int64_t>(), M, vocab_start, (int)v_local, ws.data_ptr<int>(), perm.data_ptr<int64_t>(),
                seg.data_ptr<int64_t>(), stream());
  return {perm, seg};
}

torch::Tensor embedding_bwd_sorted(torch::Tensor dout, torch::Tensor ids, int64_t v_local, int64_t vocab_start,
                                   c10::optional<torch::Tensor> out, bool accumulate,
                                   c10::optional<torch::Tensor> perm_in, c10::optional<torch::Tensor> seg_in) {
  check_rowmajor(dout, "dout");
  TORCH_CHECK(dout.is_contiguous(), "embedding_bwd_sorted: dout contiguous");
  TORCH_CHECK(ids.scalar_type() == torch::kInt64 && ids.is_contiguous() && ids.numel() == dout.size(0),
              "embedding_bwd_sorted: ids");
  const at::DeviceGuard g(dout.device());
  const int64_t D = dout.size(1);
  torch::Tensor dw;
  if (out.has_value()) {
    dw = *out;
    check_emb_out(dw, "embedding_bwd_sorted", v_local, D, dout);
  } else {
    dw = torch::empty({v_local, D}, dout.options().dtype(torch::kFloat32));
    accumulate = false;
  }
  if (v_local == 0) return dw;
  if (D % 4) {   // (the atomic form needs a zeroed / accumulating output)
    if (!accumulate) dw.zero_();
    return embedding_bwd(dout, ids, v_local, vocab_start, dw);
  }
  torch::Tensor perm, seg;
  if (perm_in.has_value() && seg_in.has_value()) {   // sorted ahead (e.g. on a side stream in the forward)
    perm = *perm_in;
    seg = *seg_in;
    TORCH_CHECK(perm.scalar_type() == torch::kInt64 && perm.is_contiguous() && perm.numel() == ids.numel() &&
                    seg.scalar_type() == torch::kInt64 && seg.is_contiguous() && seg.numel() == v_local + 1,
                "embedding_bwd_sorted: perm [M] / seg [v_local + 1] int64");
  } else {
    auto ps = emb_sort(ids, vocab_start, v_local);
    perm = ps[0];
    seg = ps[1];
  }
  dpfs_embedding_bwd_seg(dcode(dout), dout.data_ptr(), perm.data_ptr<int64_t>(), seg.data_ptr<int64_t>(),
                         dw.data_ptr<float>(), (int)D, (int)v_local, accumulate ? 1 : 0, stream());
  return dw;
}

// Loss bookkeeping of the vocab-parallel CE from the gathered statistics (nsh, M, 3): per-row
// lse and validity (1.0 / 0.0), the running (loss sum, valid count) in acc[2] (overwritten when
// `first`), and with `last` the mean loss into `loss` (0-d) and max(count, 1) into acc[1].
std::vector<torch::Tensor> ce_finalize(torch::Tensor stats, torch::Tensor targets, int64_t ignore_index,
                                       torch::Tensor acc, torch::Tensor loss, bool first, bool last) {
  check_cuda(stats, "stats");
  TORCH_CHECK(stats.scalar_type() == torch::kFloat32 && stats.is_contiguous() && stats.dim() == 3 &&
                  stats.size(2) == 3, "ce_finalize: stats fp32 contiguous (nsh, M, 3)");
  const int64_t M = stats.size(1);
  TORCH_CHECK(targets.scalar_type() == torch::kInt64 && targets.is_contiguous() && targets.numel() == M,
              "ce_finalize: targets int64 [M]");
  TORCH_CHECK(acc.scalar_type() == torch::kFloat32 && acc.is_contiguous() && acc.numel() >= 2 &&
                  loss.scalar_type() == torch::kFloat32 && loss.numel() == 1 && loss.is_contiguous(),
              "ce_finalize: acc fp32 [>=2], loss fp32 scalar");
  const at::DeviceGuard g(stats.device());
  auto lse = torch::empty({M}, stats.options());
  auto valid = torch::empty({M}, stats.options());
  auto part = torch::empty({dpfs_ce_part_floats()}, stats.options());
  dpfs_ce_finalize(stats.data_ptr<float>(), targets.data_ptr<int64_t>(), ignore_index, lse.data_ptr<float>(),
                   valid.data_ptr<float>(), acc.data_ptr<float>(), loss.data_ptr<float>(), part.data_ptr<float>(),
                   (int)M, (int)stats.size(0), first ? 1 : 0, last ? 1 : 0, stream());
  return {lse, valid};
}

std::vector<torch::Tensor> ce_valid_scale(torch::Tensor targets, int64_t ignore_index) {
  check_cuda(targets, "targets");
  TORCH_CHECK(targets.scalar_type() == torch::kInt64 && targets.is_contiguous(), "ce_valid_scale: int64 targets");
  const at::DeviceGuard g(targets.device());
  const int64_t M = targets.numel();
  auto gs = torch::empty({M}, targets.options().dtype(torch::kFloat32));
  auto n = torch::empty({}, targets.options().dtype(torch::kFloat32));
  auto part = torch::empty({dpfs_ce_part_floats()}, targets.options().dtype(torch::kFloat32));
  dpfs_ce_valid_scale(targets.data_ptr<int64_t>(), ignore_index, gs.data_ptr<float>(), n.data_ptr<float>(),
                      part.data_ptr<float>(), (int)M, stream());
  return {gs, n};
}

torch::Tensor ce_grad_scale(torch::Tensor valid, torch::Tensor gloss, torch::Tensor n_valid) {
  check_cuda(valid, "valid");
  TORCH_CHECK(valid.scalar_type() == torch::kFloat32 && valid.is_contiguous(), "ce_grad_scale: fp32 valid [M]");
  TORCH_CHECK((gloss.scalar_type() == torch::kFloat32 || gloss.scalar_type() == torch::kBFloat16) && gloss.numel() == 1 &&
                  gloss.is_cuda(), "ce_grad_scale: gloss fp32 / bf16 scalar on the device");
  TORCH_CHECK(n_valid.scalar_type() == torch::kFloat32 && n_valid.numel() == 1 && n_valid.is_cuda(),
              "ce_grad_scale: n_valid fp32 scalar on the device");
  const at::DeviceGuard g(valid.device());
  auto gs = torch::empty_like(valid);
  auto gl = gloss.contiguous();
  auto nv = n_valid.contiguous();
  dpfs_ce_grad_scale(valid.data_ptr<float>(), gl.data_ptr(), gl.scalar_type() == torch::kBFloat16 ? 1 : 0,
                     nv.data_ptr<float>(), gs.data_ptr<float>(), (int)valid.numel(), stream());
  return gs;
}

torch::Tensor ce_fwd_stats(torch::Tensor logits, torch::Tensor targets, int64_t vocab_start, int64_t vocab_valid) {
  check_rowmajor(logits, "logits");
  TORCH_CHECK(logits.is_contiguous(), "ce: logits contiguous");
  TORCH_CHECK(targets.scalar_type() == torch::kInt64 && targets.is_contiguous() && targets.numel() == logits.size(0),
              "ce: targets int64 [M]");
  TORCH_CHECK(vocab_valid >= 0 && vocab_valid <= logits.size(1), "ce: vocab_valid out of range");
  const at::DeviceGuard g(logits.device());
  const int64_t M = logits.size(0), V = logits.size(1);
  auto stats = torch::empty({M, 3}, logits.options().dtype(torch::kFloat32));
  if (M) dpfs_ce_stats(dcode(logits), logits.data_ptr(), targets.data_ptr<int64_t>(), stats.data_ptr<float>(), (int)M,
                       (int)V, vocab_start, (int)vocab_valid, stream());
  return stats;
}

// Single-shard CE forward + backward in one pass (TP 1): returns the ce_fwd_stats rows and
// overwrites logits with (softmax - onehot) * gscale[row] (+ the bias gradient into dbias);
// None (nothing launched) where the one-pass kernel does not apply.
c10::optional<torch::Tensor> ce_fused(torch::Tensor logits, torch::Tensor targets, torch::Tensor gscale,
                                      int64_t vocab_start, int64_t vocab_valid, c10::optional<torch::Tensor> dbias) {
  check_rowmajor(logits, "logits");
  TORCH_CHECK(logits.is_contiguous(), "ce_fused: logits contiguous");
  const int64_t M = logits.size(0), V = logits.size(1);
  TORCH_CHECK(targets.scalar_type() == torch::kInt64 && targets.is_contiguous() && targets.numel() == M,
              "ce_fused: targets int64 [M]");
  TORCH_CHECK(gscale.scalar_type() == torch::kFloat32 && gscale.is_contiguous() && gscale.numel() == M,
              "ce_fused: gscale fp32 [M]");
  TORCH_CHECK(vocab_valid >= 0 && vocab_valid <= V, "ce_fused: vocab_valid out of range");
  TORCH_CHECK(M < (1ll << 31) / 3, "ce_fused: too many rows");
  const at::DeviceGuard g(logits.device());
  float* db = dbias_out(dbias, V, "ce_fused");
  auto stats = torch::empty({M, 3}, logits.options().dtype(torch::kFloat32));
  torch::Tensor ws;
  if (db) ws = torch::empty({std::max<long long>(dpfs_ce_fused_ws((int)M, (int)V), 1)}, stats.options());
  if (db && M == 0) dbias->zero_();
  const int ok = dpfs_ce_fused(dcode(logits), logits.data_ptr(), targets.data_ptr<int64_t>(), gscale.data_ptr<float>(),
                               stats.data_ptr<float>(), db, db ? ws.data_ptr<float>() : nullptr, (int)M, (int)V,
                               vocab_start, (int)vocab_valid, stream());
  if (!ok) return c10::nullopt;
  return stats;
}

torch::Tensor ce_bwd(torch::Tensor logits, torch::Tensor targets, torch::Tensor lse, torch::Tensor gscale,
                     int64_t vocab_start, int64_t vocab_valid, torch::Tensor out,
                     c10::optional<torch::Tensor> dbias) {
  check_rowmajor(logits, "logits");
  TORCH_CHECK(logits.is_contiguous() && out.is_contiguous() && out.sizes() == logits.sizes() &&
                  out.scalar_type() == logits.scalar_type(),
              "ce_bwd: out must match logits");
  const int64_t M = logits.size(0), V = logits.size(1);
  TORCH_CHECK(lse.scalar_type() == torch::kFloat32 && lse.numel() == M && gscale.scalar_type() == torch::kFloat32 &&
                  gscale.numel() == M && lse.is_contiguous() && gscale.is_contiguous(),
              "ce_bwd: lse/gscale fp32 [M]");
  const at::DeviceGuard g(logits.device());
  float* db = dbias_out(dbias, V, "ce_bwd");
  if (db && M == 0) dbias->zero_();
  if (M == 0) return out;
  if (db) {
    const long long wsn = dpfs_ce_bwd_dbias_ws(dcode(logits), (int)M, (int)V);
    auto ws = torch::empty({std::max<long long>(wsn, 1)}, lse.options());
    dpfs_ce_bwd_dbias(dcode(logits), logits.data_ptr(), targets.data_ptr<int64_t>(), lse.data_ptr<float>(),
                      gscale.data_ptr<float>(), out.data_ptr(), db, ws.data_ptr<float>(), (int)M, (int)V, vocab_start,
                      (int)vocab_valid, stream());
  } else {
    dpfs_ce_bwd(dcode(logits), logits.data_ptr(), targets.data_ptr<int64_t>(), lse.data_ptr<float>(),
                gscale.data_ptr<float>(), out.data_ptr(), (int)M, (int)V, vocab_start, (int)vocab_valid, stream());
  }
  return out;
}

}  // namespace

void bind_embedding_ce(py::module_& m) {
  m.def("ce_finalize", &ce_finalize, py::arg("stats"), py::arg("targets"), py::arg("ignore_index"), py::arg("acc"),
        py::arg("loss"), py::arg("first"), py::arg("last"),
        "CE loss bookkeeping from gathered (nsh, M, 3) statistics: returns (lse, valid); running sums in acc");
  m.def("ce_valid_scale", &ce_valid_scale, py::arg("targets"), py::arg("ignore_index"),
        "(gs, n_valid): per-row 1 / max(#valid, 1) on valid rows (0 on ignored), and max(#valid, 1)");
  m.def("emb_sort", &emb_sort, py::arg("ids"), py::arg("vocab_start"), py::arg("v_local"),
        "(perm, seg): the ids' stable order by local vocab row (out-of-shard ids last) and each row's segment "
        "start, int64 (deterministic radix sort on HIP kernels)");
  m.def("ce_grad_scale", &ce_grad_scale, py::arg("valid"), py::arg("gloss"), py::arg("n_valid"),
        "gs = valid * gloss / n_valid (the CE backward's per-row loss gradient; device scalars, one launch)");
  m.def("embedding_fwd", &embedding_fwd);
  m.def("embedding_bwd_sorted", &embedding_bwd_sorted, py::arg("dout"), py::arg("ids"), py::arg("v_local"),
        py::arg("vocab_start"), py::arg("out") = py::none(), py::arg("accumulate") = false,
        py::arg("perm") = py::none(), py::arg("seg") = py::none(),
        "deterministic embedding gradient (sorted ids, one wave per vocab row; writes or adds every row)");
  m.def("embedding_bwd", &embedding_bwd, py::arg("dout"), py::arg("ids"), py::arg("v_local"), py::arg("vocab_start"),
        py::arg("out") = py::none());
  m.def("ce_fwd_stats", &ce_fwd_stats);
  m.def("ce_fused", &ce_fused, py::arg("logits"), py::arg("targets"), py::arg("gscale"), py::arg("vocab_start"),
        py::arg("vocab_valid"), py::arg("dbias") = py::none());
  m.def("ce_bwd", &ce_bwd, py::arg("logits"), py::arg("targets"), py::arg("lse"), py::arg("gscale"),
        py::arg("vocab_start"), py::arg("vocab_valid"), py::arg("out"), py::arg("dbias") = py::none());
}
