#include "common.h"

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "gfx950 (MI355X) HIP kernels of distributed_pytorch_from_scratch_amd";
  bind_gemm(m);
  bind_norm_elementwise(m);
  bind_attention(m);
  bind_embedding_ce(m);
  bind_optim(m);
  bind_decode(m);
  bind_comm(m);
}
