#include "common.h"

namespace {

// ------------------------------------------------------------- xGMI collectives (comm/) --
void* xgmi_ptr(int64_t h) {
  TORCH_CHECK(h != 0, "xgmi: null communicator");
  return reinterpret_cast<void*>(h);
}

py::tuple xgmi_create(int64_t rank, int64_t world, int64_t cap_bytes, int64_t nslots) {
  std::string hb((size_t)dpfs_xgmi_handle_bytes(), '\0');
  void* h = dpfs_xgmi_create((int)rank, (int)world, cap_bytes, (int)nslots, &hb[0]);
  TORCH_CHECK(h != nullptr, "xgmi_create failed: ", dpfs_xgmi_last_error());
  return py::make_tuple(reinterpret_cast<int64_t>(h), py::bytes(hb));
}

void xgmi_open(int64_t h, py::bytes all_handles) {
  std::string s = all_handles;
  TORCH_CHECK(s.size() % dpfs_xgmi_handle_bytes() == 0, "xgmi_open: handle blob size");
  TORCH_CHECK(dpfs_xgmi_open(xgmi_ptr(h), s.data()) == 0, "xgmi_open failed: ", dpfs_xgmi_last_error());
}

// op 0 all-reduce (out may be x), 1 reduce-scatter (out = x.numel()/W elements),
// 2 all-gather (out = W * x.numel() elements), 3 one-shot all-reduce (out may be x; up to the
// one-shot capacity, unstaged); launched on the current stream.
// A staging slot as a non-owning uint8 tensor of `cap` bytes on `device` (the communicator
// owns the memory; the Python side keeps the communicator alive as long as the views).
torch::Tensor xgmi_slot_tensor(int64_t h, int64_t slot, int64_t cap, torch::Device device) {
  void* p = dpfs_xgmi_slot(xgmi_ptr(h), (int)slot);
  TORCH_CHECK(p != nullptr, "xgmi: no staging slot ", slot);
  return torch::from_blob(p, {cap}, torch::TensorOptions().dtype(torch::kUInt8).device(device));
}

void xgmi_run(int64_t h, int64_t op, torch::Tensor x, torch::Tensor out, int64_t world, double timeout_s,
              int64_t slot) {
  TORCH_CHECK(op >= 0 && op <= 3, "xgmi_run: op");
  check_cuda(x, "x");
  check_cuda(out, "out");
  TORCH_CHECK(x.is_contiguous() && out.is_contiguous(), "xgmi_run: contiguous tensors");
  TORCH_CHECK(x.scalar_type() == out.scalar_type(), "xgmi_run: dtype mismatch");
  const int dt = dcode(x);
  const int64_t vec = dt == 1 ? 8 : 4;
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(out.data_ptr()) % 16 == 0,
              "xgmi_run: 16-byte aligned buffers");
  const int64_t n = x.numel();
  TORCH_CHECK(n > 0 && n % vec == 0, "xgmi_run: numel must be a positive multiple of ", vec);
  int64_t total, part;
  if (op == 3) {
    TORCH_CHECK(out.numel() == n && slot < 0, "xgmi one-shot all_reduce: out numel, no staging");
    total = n;
    part = n;
  } else if (op == 0) {
    TORCH_CHECK(out.numel() == n, "xgmi all_reduce: out numel");
    total = n;
    part = ((n + world * vec - 1) / (world * vec)) * vec;
  } else if (op == 1) {
    TORCH_CHECK(n % (world * vec) == 0 && out.numel() * world == n, "xgmi reduce_scatter: sizes");
    total = n;
    part = n / world;
  } else {
    TORCH_CHECK(out.numel() == n * world, "xgmi all_gather: out numel");
    total = n * world;
    part = n;
  }
  const at::DeviceGuard g(x.device());
  TORCH_CHECK(dpfs_xgmi_run(xgmi_ptr(h), (int)op, dt, x.data_ptr(), out.data_ptr(), total, part, timeout_s,
                            (int)slot, stream()) == 0,
              "xgmi_run failed: ", dpfs_xgmi_last_error());
}

// ------------------------------------------------------- native RCCL communicator (comm/) --
void* rccl_ptr(int64_t h) {
  TORCH_CHECK(h != 0, "rccl: null communicator");
  return reinterpret_cast<void*>(h);
}

int rccl_dtype(const torch::Tensor& t) {   // ncclDataType_t values (rccl.h)
  switch (t.scalar_type()) {
    case torch::kBFloat16: return 9;
    case torch::kFloat32: return 7;
    case torch::kFloat16: return 6;
    case torch::kFloat64: return 8;
    case torch::kInt64: return 4;
    case torch::kInt32: return 2;
    case torch::kUInt8: return 1;
    default: TORCH_CHECK(false, "rccl: unsupported dtype ", t.scalar_type());
  }
  return -1;
}

void rccl_check(int rc, const char* what) { TORCH_CHECK(rc == 0, what, " failed: ", dpfs_rccl_last_error()); }

py::bytes rccl_unique_id() {
  std::string b((size_t)dpfs_rccl_id_bytes(), '\0');
  rccl_check(dpfs_rccl_unique_id(&b[0]), "ncclGetUniqueId");
  return py::bytes(b);
}

int64_t rccl_init(py::bytes id, int64_t nranks, int64_t rank) {
  std::string b = id;
  TORCH_CHECK((int)b.size() == dpfs_rccl_id_bytes(), "rccl_init: unique id size");
  void* c = nullptr;
  {
    py::gil_scoped_release nogil;   // blocks until every rank has joined
    rccl_check(dpfs_rccl_init(b.data(), (int)nranks, (int)rank, &c), "ncclCommInitRank");
  }
  return reinterpret_cast<int64_t>(c);
}

// Input and output of a collective: on the device, contiguous, one dtype, sizes as `sizes_ok`.
void rccl_check_pair(const torch::Tensor& x, const torch::Tensor& out, bool sizes_ok, const char* msg) {
  check_cuda(x, "x");
  check_cuda(out, "out");
  TORCH_CHECK(x.is_contiguous() && out.is_contiguous() && sizes_ok && x.scalar_type() == out.scalar_type(), msg);
}

// Collectives on the CURRENT HIP stream (the Python side selects its side stream).
void rccl_all_reduce(int64_t h, torch::Tensor x, torch::Tensor out, int64_t op) {
  rccl_check_pair(x, out, x.numel() == out.numel(), "rccl all_reduce: contiguous, same size and dtype");
  const at::DeviceGuard g(x.device());
  rccl_check(dpfs_rccl_all_reduce(rccl_ptr(h), x.data_ptr(), out.data_ptr(), (size_t)x.numel(), rccl_dtype(x),
                                  (int)op, stream()), "ncclAllReduce");
}

void rccl_reduce_scatter(int64_t h, torch::Tensor out, torch::Tensor x, int64_t world, int64_t op) {
  rccl_check_pair(x, out, out.numel() * world == x.numel(), "rccl reduce_scatter: out = in / world elements");
  const at::DeviceGuard g(x.device());
  rccl_check(dpfs_rccl_reduce_scatter(rccl_ptr(h), x.data_ptr(), out.data_ptr(), (size_t)out.numel(), rccl_dtype(x),
                                      (int)op, stream()), "ncclReduceScatter");
}

void rccl_all_gather(int64_t h, torch::Tensor out, torch::Tensor x, int64_t world) {
  rccl_check_pair(x, out, x.numel() * world == out.numel(), "rccl all_gather: out = world x in elements");
  const at::DeviceGuard g(x.device());
  rccl_check(dpfs_rccl_all_gather(rccl_ptr(h), x.data_ptr(), out.data_ptr(), (size_t)x.numel(), rccl_dtype(x),
                                  stream()), "ncclAllGather");
}

void rccl_broadcast(int64_t h, torch::Tensor t, int64_t root) {
  check_cuda(t, "t");
  TORCH_CHECK(t.is_contiguous(), "rccl broadcast: contiguous tensor");
  const at::DeviceGuard g(t.device());
  rccl_check(dpfs_rccl_broadcast(rccl_ptr(h), t.data_ptr(), t.data_ptr(), (size_t)t.numel(), rccl_dtype(t),
                                 (int)root, stream()), "ncclBroadcast");
}

// ---- hipBLASLt, driven directly (blas/blaslt.hip) ----
// layout 0 NT: out[M,N] bf16 = a[M,K] b[N,K]^T (+ bias fp32[N]);  1 NN: out = a[M,K] b[K,N];
// 2 TN: out[M,N] fp32 (+)= a[K,M]^T b[K,N].  Operands contiguous bf16.
int64_t lt_algos(int64_t layout, int64_t M, int64_t N, int64_t K, bool bias) {
  return dpfs_lt_algos((int)layout, M, N, K, bias ? 1 : 0);
}

void lt_run(int64_t layout, torch::Tensor a, torch::Tensor b, torch::Tensor out, c10::optional<torch::Tensor> bias,
            int64_t algo, bool accumulate) {
  TORCH_CHECK(layout >= 0 && layout <= 2, "lt_run: layout 0 (NT), 1 (NN) or 2 (TN)");
  for (const torch::Tensor* t : {&a, &b, &out}) {
    check_cuda(*t, "lt_run operand");
    TORCH_CHECK(t->dim() == 2 && t->is_contiguous(), "lt_run: 2-D contiguous operands");
  }
  TORCH_CHECK(a.scalar_type() == torch::kBFloat16 && b.scalar_type() == torch::kBFloat16, "lt_run: bf16 operands");
  int64_t M, N, K;
  if (layout == 0) {
    M = a.size(0), K = a.size(1), N = b.size(0);
    TORCH_CHECK(b.size(1) == K, "lt_run NT: a [M,K], b [N,K]");
  } else if (layout == 1) {
    M = a.size(0), K = a.size(1), N = b.size(1);
    TORCH_CHECK(b.size(0) == K, "lt_run NN: a [M,K], b [K,N]");
  } else {
    K = a.size(0), M = a.size(1), N = b.size(1);
    TORCH_CHECK(b.size(0) == K, "lt_run TN: a [K,M], b [K,N]");
  }
  TORCH_CHECK(out.size(0) == M && out.size(1) == N, "lt_run: out must be [M, N]");
  TORCH_CHECK(out.scalar_type() == (layout == 2 ? torch::kFloat32 : torch::kBFloat16),
              "lt_run: out fp32 for TN, bf16 otherwise");
  TORCH_CHECK(!accumulate || layout == 2, "lt_run: accumulate is TN only");
  const float* bp = nullptr;
  if (bias.has_value()) {
    TORCH_CHECK(layout == 0, "lt_run: bias is NT only");
    check_cuda(*bias, "bias");
    TORCH_CHECK(bias->scalar_type() == torch::kFloat32 && bias->is_contiguous() && bias->numel() == N,
                "lt_run: bias fp32 [N] contiguous");
    bp = bias->data_ptr<float>();
  }
  TORCH_CHECK(a.device() == b.device() && a.device() == out.device(), "lt_run: operands on one device");
  const at::DeviceGuard g(a.device());
  const int n = dpfs_lt_algos((int)layout, M, N, K, bp ? 1 : 0);
  TORCH_CHECK(algo >= 0 && algo < n, "lt_run: algorithm ", algo, " of ", n, " (", dpfs_lt_last_error(), ")");
  const long long wsb = dpfs_lt_workspace((int)layout, M, N, K, bp ? 1 : 0, (int)algo);
  torch::Tensor ws;
  if (wsb > 0) ws = torch::empty({wsb}, a.options().dtype(torch::kUInt8));
  const int st = dpfs_lt_run((int)layout, M, N, K, bp, (int)algo, a.data_ptr(), b.data_ptr(), out.data_ptr(),
                             accumulate ? 1.f : 0.f, wsb > 0 ? ws.data_ptr() : nullptr, wsb > 0 ? wsb : 0, stream());
  TORCH_CHECK(st == 0, "hipBLASLt: ", dpfs_lt_last_error());
}

}  // namespace

void bind_comm(py::module_& m) {
  m.def("lt_algos", &lt_algos, py::arg("layout"), py::arg("M"), py::arg("N"), py::arg("K"), py::arg("bias") = false,
        "hipBLASLt heuristic algorithms for a problem (0 NT, 1 NN, 2 TN)");
  m.def("lt_run", &lt_run, py::arg("layout"), py::arg("a"), py::arg("b"), py::arg("out"), py::arg("bias") = py::none(),
        py::arg("algo") = 0, py::arg("accumulate") = false);
  m.def("xgmi_create", &xgmi_create, "allocate IPC buffers: -> (handle, ipc handle bytes)");
  m.def("xgmi_open", &xgmi_open, "map every peer's buffers (rank-ordered concatenated handle bytes)");
  m.def("xgmi_run", &xgmi_run, py::arg("h"), py::arg("op"), py::arg("x"), py::arg("out"), py::arg("world"),
        py::arg("timeout_s") = 120.0, py::arg("slot") = -1);
  m.def("xgmi_one_shot_capacity", [](int64_t h) { return dpfs_xgmi_one_shot_capacity(xgmi_ptr(h)); });
  m.def("xgmi_slot_tensor", &xgmi_slot_tensor, py::arg("h"), py::arg("slot"), py::arg("cap"), py::arg("device"));
  m.def("xgmi_set_blocks", [](int64_t h, int b) { dpfs_xgmi_set_blocks(xgmi_ptr(h), b); });
  m.def("xgmi_capacity", [](int64_t h) { return dpfs_xgmi_capacity(xgmi_ptr(h)); });
  m.def("xgmi_error", [](int64_t h) { return dpfs_xgmi_error(xgmi_ptr(h)); });
  m.def("xgmi_clear_error", [](int64_t h) { dpfs_xgmi_clear_error(xgmi_ptr(h)); });
  m.def("xgmi_destroy", [](int64_t h) { dpfs_xgmi_destroy(xgmi_ptr(h)); });
  m.def("rccl_unique_id", &rccl_unique_id, "ncclGetUniqueId -> bytes");
  m.def("rccl_init", &rccl_init, py::arg("id"), py::arg("nranks"), py::arg("rank"),
        "ncclCommInitRank on the current device -> communicator handle");
  m.def("rccl_all_reduce", &rccl_all_reduce, py::arg("h"), py::arg("x"), py::arg("out"), py::arg("op") = 0);
  m.def("rccl_reduce_scatter", &rccl_reduce_scatter, py::arg("h"), py::arg("out"), py::arg("x"), py::arg("world"),
        py::arg("op") = 0);
  m.def("rccl_all_gather", &rccl_all_gather, py::arg("h"), py::arg("out"), py::arg("x"), py::arg("world"));
  m.def("rccl_broadcast", &rccl_broadcast, py::arg("h"), py::arg("t"), py::arg("root"));
  m.def("rccl_group_start", []() { TORCH_CHECK(dpfs_rccl_group_start() == 0, "ncclGroupStart"); });
  m.def("rccl_group_end", []() { rccl_check(dpfs_rccl_group_end(), "ncclGroupEnd"); });
  m.def("rccl_async_error", [](int64_t h) {
    return dpfs_rccl_async_error(rccl_ptr(h)) == 0 ? std::string() : std::string(dpfs_rccl_last_error());
  });
  m.def("rccl_destroy", [](int64_t h) { rccl_check(dpfs_rccl_destroy(rccl_ptr(h)), "ncclCommDestroy"); });
}
