// Weight-only fp8 decode projections (gfx950): e4m3 weight codes with one fp32 scale per output
// channel, for the one-token steps whose time is the weight bytes they stream.
//
// Format (the row format of kv8.h applied to one weight row = the K input features of output
// channel n): codes uint8 [N, K] row-major, inv fp32 [N], value = f32(code) * inv[n].
//
//   quant_w8_rows_k  one workgroup per weight row: an amax pass over the bf16 row, then the encode
//                    pass (kv8_scale / kv8_amax8 / kv8_enc8: the bytes of the PyTorch oracle).
//   swiglu_quant_w8_rows_k  the same on the rows of bf16(silu(g) * u) of a packed [g | u]: the per-token
//                    activation codes of the W8A8 down projection (gemm_w8a8.hip).
//   gemv_w8_k        y[M, N] = bf16( fp32(sum_k a[m,k] f32(code[n,k])) * inv[n] + bias[n] ),
//                    1 <= M <= 64, K % 64 == 0.
//
// gemv_w8_k.  Every e4m3 value is a bf16 value, so the codes enter v_mfma_f32_16x16x32_bf16 exactly
// and the scale multiplies the finished fp32 sum once per output column in the epilogue: no
// multiply and no rounding per weight element.  A lane's weight load is 16 bytes = 16 codes.  The
// order of k inside a dot product is free as long as both operands agree, so the 4 lanes (g = 0..3)
// that share weight row n own 64 consecutive k: lane g holds k = 64c + 16g .. + 16, and the wave's
// "pair-step" c is two MFMA k-steps, the first over codes 0..7 of every lane (k = 64c + 16g + 0..7
// for g = 0..3: 32 distinct k), the second over codes 8..15.  The lane reads its A fragments for
// both from the same 16 k as two 16-byte loads.  v_cvt_scalef32_pk_bf16_fp8 (scale 1.0) turns two
// codes into two packed bf16 in one VALU: 8 per pair-step.
//
// A wave is one 16-column B tile against MT = ceil(M / 16) A tiles (rows >= M read as zeros): a
// converted weight fragment is used by MT MFMAs, MT f32x4 accumulators.  All weight loads of a
// batch of CH pair-steps are issued ahead of the batch's A loads, conversions and MFMAs; CH shrinks
// with MT so that the A fragments of a batch stay in registers.  A workgroup is KS x CW waves: KS
// waves split K (merged through LDS in wave order: no atomics, bit-reproducible), CW waves take
// neighbouring 16-column tiles of the same K slice, so their A reads hit the same L1 lines.
// A (a few KB up to ~1 MB) stays in L2; W is streamed once.
// SW: A = bf16(silu(g) * u) of a packed [M, 2K] gate|up input, the formula and rounding of
// gemv16_k / swiglu_fwd_k: the SwiGLU fused into the down projection's operand load.
#include "common.h"
#include "kv8.h"
#include "../dpfs_api.h"

namespace dpfs {

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

__global__ __launch_bounds__(256) void quant_w8_rows_k(const bf16* __restrict__ W, long long ldw,
                                                        uint8_t* __restrict__ codes, long long ldc,
                                                        float* __restrict__ inv, int K) {
  __shared__ float red[4];
  const long long n = blockIdx.x;
  const bf16* wr = W + n * ldw;
  const int nv = K / 8;
  float m = 0.f;
  for (int j = threadIdx.x; j < nv; j += 256) m = kv8_amax8(*reinterpret_cast<const bf16x8*>(wr + 8 * j), m);
  m = wave_max(m);
  if (lane_id() == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  const float scale = kv8_scale(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])));
  for (int j = threadIdx.x; j < nv; j += 256)
    *reinterpret_cast<u32x2*>(codes + n * ldc + 8 * j) = kv8_enc8(*reinterpret_cast<const bf16x8*>(wr + 8 * j), scale);
  if (threadIdx.x == 0) inv[n] = 1.f / scale;
}

__device__ __forceinline__ float silu_w8(float g) { return g * __builtin_amdgcn_rcpf(1.f + __expf(-g)); }   // = silu_f

// 8 elements of h = bf16(silu(g) * u): swiglu_fwd_k's formula and rounding
__device__ __forceinline__ bf16x8 swiglu8_w8(const bf16* g, const bf16* u) {
  const bf16x8 gv = *reinterpret_cast<const bf16x8*>(g), uv = *reinterpret_cast<const bf16x8*>(u);
  bf16x8 r;
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = (bf16)(silu_w8((float)gv[j]) * (float)uv[j]);
  return r;
}

// quant_w8_rows_k on the rows of h = bf16(silu(g) * u) of a packed gu = [g | u] [M, 2F]: the per-token
// activation codes of the W8A8 down projection (gemm_w8a8.hip).  h is recomputed from gu in the encode
// pass (the row's second read comes from L2) and never written: the bytes of quant_w8_rows(swiglu_fwd(gu)).
__global__ __launch_bounds__(256) void swiglu_quant_w8_rows_k(const bf16* __restrict__ GU, long long ldg,
                                                               uint8_t* __restrict__ codes, long long ldc,
                                                               float* __restrict__ inv, int F) {
  __shared__ float red[4];
  const long long m = blockIdx.x;
  const bf16* gr = GU + m * ldg;
  const int nv = F / 8;
  float a = 0.f;
  for (int j = threadIdx.x; j < nv; j += 256) a = kv8_amax8(swiglu8_w8(gr + 8 * j, gr + F + 8 * j), a);
  a = wave_max(a);
  if (lane_id() == 0) red[threadIdx.x >> 6] = a;
  __syncthreads();
  const float scale = kv8_scale(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])));
  for (int j = threadIdx.x; j < nv; j += 256)
    *reinterpret_cast<u32x2*>(codes + m * ldc + 8 * j) = kv8_enc8(swiglu8_w8(gr + 8 * j, gr + F + 8 * j), scale);
  if (threadIdx.x == 0) inv[m] = 1.f / scale;
}

// codes 8h .. 8h + 7 of a 16-code load (words 2h, 2h + 1) -> 8 bf16, exact
__device__ __forceinline__ bf16x8 w8_cvt8(uint32_t w0, uint32_t w1) {
  const bf16x2 p0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, 1.0f, false);
  const bf16x2 p1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, 1.0f, true);
  const bf16x2 p2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, 1.0f, false);
  const bf16x2 p3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, 1.0f, true);
  return bf16x8{p0[0], p0[1], p1[0], p1[1], p2[0], p2[1], p3[0], p3[1]};
}

// pair-steps per batch of weight loads: 4 VGPRs of codes and 8 MT VGPRs of A fragments each
template <int MT> struct W8Batch { static constexpr int CH = MT == 1 ? 8 : MT == 2 ? 4 : 2; };

template <int MT, int KS, int CW, bool SW>
__global__ __launch_bounds__(64 * KS * CW) void gemv_w8_k(const bf16* __restrict__ A, long long lda,
                                                          const uint8_t* __restrict__ C8, long long ldc,
                                                          const float* __restrict__ inv,
                                                          const float* __restrict__ bias, bf16* __restrict__ Y,
                                                          long long ldy, int M, int N, int K) {
  constexpr int CH = W8Batch<MT>::CH;
  __shared__ f32x4 red[CW][KS][MT][64];
  const int wave = threadIdx.x >> 6, kw = wave % KS, cw = wave / KS;
  const int l = lane_id(), g = l >> 4, i = l & 15;
  const int n0 = (blockIdx.x * CW + cw) * 16;
  const int nk = K / 64;                       // pair-steps
  const int per = (nk + KS - 1) / KS;
  const int c0 = kw * per, c1 = min(nk, c0 + per);   // (c0 >= nk: a wave with no k-steps adds zeros)
  const uint8_t* wp = C8 + (long long)min(n0 + i, N - 1) * ldc + 16 * g;
  const bf16* ap[MT];
  bool mv[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    mv[t] = 16 * t + i < M;
    ap[t] = A + (long long)(mv[t] ? 16 * t + i : 0) * lda + 16 * g;
  }
  f32x4 acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int cb = c0; cb < c1; cb += CH) {
    u32x4 wq[CH];
#pragma unroll
    for (int u = 0; u < CH; ++u)
      if (cb + u < c1) wq[u] = *reinterpret_cast<const u32x4*>(wp + 64 * (cb + u));
#pragma unroll
    for (int u = 0; u < CH; ++u) {
      if (cb + u < c1) {
        const int k = 64 * (cb + u);
        bf16x8 a0[MT], a1[MT];
#pragma unroll
        for (int t = 0; t < MT; ++t) {
          if (SW) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              const bf16x8 gv = *reinterpret_cast<const bf16x8*>(ap[t] + k + 8 * h);
              const bf16x8 uv = *reinterpret_cast<const bf16x8*>(ap[t] + K + k + 8 * h);
              bf16x8 r;
#pragma unroll
              for (int j = 0; j < 8; ++j) r[j] = (bf16)(silu_w8((float)gv[j]) * (float)uv[j]);
              (h ? a1[t] : a0[t]) = r;
            }
          } else {
            a0[t] = *reinterpret_cast<const bf16x8*>(ap[t] + k);
            a1[t] = *reinterpret_cast<const bf16x8*>(ap[t] + k + 8);
          }
        }
        const bf16x8 b0 = w8_cvt8(wq[u][0], wq[u][1]), b1 = w8_cvt8(wq[u][2], wq[u][3]);
        const bf16x8 z = {};
#pragma unroll
        for (int t = 0; t < MT; ++t) {
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(mv[t] ? a0[t] : z, b0, acc[t], 0, 0, 0);
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(mv[t] ? a1[t] : z, b1, acc[t], 0, 0, 0);
        }
      }
    }
  }
#pragma unroll
  for (int t = 0; t < MT; ++t) red[cw][kw][t][l] = acc[t];
  __syncthreads();
  if (kw == 0) {
    const int n = n0 + i;                      // D[row = 4g + j][col = lane & 15]
#pragma unroll
    for (int t = 0; t < MT; ++t) {
#pragma unroll
      for (int w = 1; w < KS; ++w) acc[t] += red[cw][w][t][l];
    }
    if (n < N) {
      const float sc = inv[n], bv = bias ? bias[n] : 0.f;
#pragma unroll
      for (int t = 0; t < MT; ++t) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int m = 16 * t + 4 * g + j;
          if (m < M) Y[(long long)m * ldy + n] = (bf16)(acc[t][j] * sc + bv);
        }
      }
    }
  }
}

template <int MT, int KS, int CW>
static void launch_w8(const void* A, long long lda, const void* C8, long long ldc, const float* inv, const float* bias,
                      void* Y, long long ldy, int M, int N, int K, int swiglu, hipStream_t s) {
  const int nb = (N + 16 * CW - 1) / (16 * CW);
  if (swiglu)
    gemv_w8_k<MT, KS, CW, true><<<nb, 64 * KS * CW, 0, s>>>((const bf16*)A, lda, (const uint8_t*)C8, ldc, inv, bias,
                                                           (bf16*)Y, ldy, M, N, K);
  else
    gemv_w8_k<MT, KS, CW, false><<<nb, 64 * KS * CW, 0, s>>>((const bf16*)A, lda, (const uint8_t*)C8, ldc, inv, bias,
                                                            (bf16*)Y, ldy, M, N, K);
}

template <int MT>
static void launch_w8_mt(const void* A, long long lda, const void* C8, long long ldc, const float* inv,
                         const float* bias, void* Y, long long ldy, int M, int N, int K, int swiglu, hipStream_t s) {
  // The launch rule, from N and K (as dpfs_gemv16): a workgroup is 8 waves.  While the grid of
  // 16-column tiles is small (<= 512 tiles: about two per CU) and K leaves every wave >= 2
  // pair-steps, all 8 waves split K over one tile (KS 8, CW 1: the narrow projections need the
  // waves for bytes in flight).  Wide N (QKV, gate|up, the lm_head: thousands of tiles) and short K
  // take 4 K-waves x 2 neighbouring tiles (KS 4, CW 2), half the LDS merges per column, and the two
  // tiles' A reads share L1 lines.
  const int tiles = (N + 15) / 16;
  if (tiles <= 512 && K / 64 >= 16) launch_w8<MT, 8, 1>(A, lda, C8, ldc, inv, bias, Y, ldy, M, N, K, swiglu, s);
  else launch_w8<MT, 4, 2>(A, lda, C8, ldc, inv, bias, Y, ldy, M, N, K, swiglu, s);
}

}  // namespace dpfs

using namespace dpfs;

// lda: A's row stride (bf16 elements), ldc: the codes' row stride (bytes)
extern "C" int dpfs_gemv_w8_ok(int M, int N, int K, long long lda, long long ldc) {
  return M >= 1 && M <= 64 && N >= 1 && K > 0 && K % 64 == 0 && lda % 8 == 0 && ldc % 16 == 0 && ldc >= K;
}

// Y[M, N] bf16 (row stride ldy) = (A or silu(g) u of A = [g | u]) codes^T * inv (+ bias; null: none).
// A and the codes 16-byte aligned.  No host state: graph-capturable.
extern "C" void dpfs_gemv_w8(const void* A, long long lda, const void* codes, long long ldc, const float* inv,
                             const float* bias, void* Y, long long ldy, int M, int N, int K, int swiglu,
                             hipStream_t s) {
  switch ((M + 15) / 16) {
    case 1: launch_w8_mt<1>(A, lda, codes, ldc, inv, bias, Y, ldy, M, N, K, swiglu, s); break;
    case 2: launch_w8_mt<2>(A, lda, codes, ldc, inv, bias, Y, ldy, M, N, K, swiglu, s); break;
    case 3: launch_w8_mt<3>(A, lda, codes, ldc, inv, bias, Y, ldy, M, N, K, swiglu, s); break;
    default: launch_w8_mt<4>(A, lda, codes, ldc, inv, bias, Y, ldy, M, N, K, swiglu, s); break;
  }
}

// W bf16 [N, K] (row stride ldw elements, ldw % 8 == 0, K % 8 == 0, 16-byte aligned) -> codes
// uint8 [N, K] (row stride ldc bytes, ldc % 8 == 0) and inv fp32 [N].
extern "C" void dpfs_quant_w8_rows(const void* W, long long ldw, void* codes, long long ldc, float* inv, int N, int K,
                                   hipStream_t s) {
  if (N > 0) quant_w8_rows_k<<<N, 256, 0, s>>>((const bf16*)W, ldw, (uint8_t*)codes, ldc, inv, K);
}

// gu bf16 [M, 2F] = [gate | up] (row stride ldg elements, ldg % 8 == 0, F % 8 == 0, 16-byte aligned) ->
// codes uint8 [M, F] (row stride ldc bytes, ldc % 8 == 0) and inv fp32 [M] of the rows bf16(silu(gate) * up).
extern "C" void dpfs_swiglu_quant_w8_rows(const void* gu, long long ldg, void* codes, long long ldc, float* inv, int M,
                                          int F, hipStream_t s) {
  if (M > 0) swiglu_quant_w8_rows_k<<<M, 256, 0, s>>>((const bf16*)gu, ldg, (uint8_t*)codes, ldc, inv, F);
}
