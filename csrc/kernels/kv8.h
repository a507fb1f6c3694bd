// The fp8 KV cache row format (gfx950: OCP e4m3fn, the format of v_cvt_pk_fp8_f32 /
// v_cvt_pk_f32_fp8), shared by the quantising appends (kv8.hip) and the fp8 forms of the decode
// and extend attention (decode.hip, attn_extend.hip).
//
// A row is the hd bf16 values of one (sequence, cache row, head):
//   amax  = max(max_j |x_j|, 1e-12f)
//   scale = 448.f / amax                         (IEEE fp32 division)
//   code_j = e4m3fn(clamp(x_j * scale, +-448))   (fp32 product, round to nearest even)
//   inv   = 1.f / scale                          (IEEE fp32 division; the stored fp32 scale)
//   value_j = f32(code_j) * inv
// the arithmetic of fp8_cast_k (fp8.hip) per row instead of per tensor, operation for operation
// that of the PyTorch oracle (ops/reference.py _kv_quant_rows), so codes and scales are identical
// bit for bit.  x * scale reaches 448.00003 for some amax, hence the clamp in front of the
// convert; with it no NaN code (0x7f / 0xff) is produced from finite input.
#pragma once

#include "common.h"

namespace dpfs {

typedef float f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float kv8_scale(float amax) { return 448.f / fmaxf(amax, 1e-12f); }

// max over an aligned group of GRP lanes (a power of two <= 64); every lane of the group active
template <int GRP>
__device__ __forceinline__ float kv8_group_max(float m) {
#pragma unroll
  for (int x = 1; x < GRP; x <<= 1) m = fmaxf(m, __shfl_xor(m, x, 64));
  return m;
}

__device__ __forceinline__ float kv8_amax8(const bf16x8& v, float m) {
#pragma unroll
  for (int j = 0; j < 8; ++j) m = fmaxf(m, fabsf((float)v[j]));
  return m;
}

// 8 bf16 -> 8 codes (byte j = element j)
__device__ __forceinline__ u32x2 kv8_enc8(const bf16x8& v, float scale) {
  float f[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = __builtin_amdgcn_fmed3f((float)v[j] * scale, 448.f, -448.f);
  u32x2 r;
#pragma unroll
  for (int w = 0; w < 2; ++w) {
    int p = __builtin_amdgcn_cvt_pk_fp8_f32(f[4 * w], f[4 * w + 1], 0, false);
    p = __builtin_amdgcn_cvt_pk_fp8_f32(f[4 * w + 2], f[4 * w + 3], p, true);
    r[w] = (uint32_t)p;
  }
  return r;
}

// the 4 codes of one 32-bit word -> fp32 (exact)
__device__ __forceinline__ void kv8_dec4(uint32_t w, float* out) {
  const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
  const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
  out[0] = lo[0];
  out[1] = lo[1];
  out[2] = hi[0];
  out[3] = hi[1];
}

// 8 codes -> the 8 bf16 values bf16_rn(f32(code) * inv)
__device__ __forceinline__ bf16x8 kv8_dec8_bf16(u32x2 c, float inv) {
  float f[8];
  kv8_dec4(c[0], f);
  kv8_dec4(c[1], f + 4);
  bf16x8 r;
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = (bf16)(f[j] * inv);
  return r;
}

}  // namespace dpfs
