// Weight-only MXFP4 decode projections (gfx950): OCP MX e2m1 weight codes with one e8m0 scale per
// block of 32 consecutive k, for the one-token steps whose time is the weight bytes they stream.
//
// Format: codes uint8 [N, K / 2] row-major, element k of row n in bits 4 (k % 2) .. + 3 of byte k / 2
// (low nibble first), a code = sign bit + e2m1 (magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6); scales uint8
// [N, K / 32], byte s of block k / 32 = 2^(s - 127); value = e2m1(code) * 2^(s - 127).  K % 128 == 0.
//
//   quant_w4_rows_k  four lanes per block: the OCP MX v1.0 conversion in integer operations (the
//                    bytes of ops/reference.py:_quant_w4_rows).
//   gemv_w4_k        y[M, N] = bf16( fp32(sum_k a[m,k] wq[n,k]) + bias[n] ), 1 <= M <= 64.
//
// gemv_w4_k.  Every e2m1 x 2^e with s >= 2 is a bf16 value, so v_cvt_scalef32_pk_bf16_fp4 (two codes
// and the block scale -> two packed bf16, one VALU) feeds v_mfma_f32_16x16x32_bf16 exactly: no
// rounding per weight and no scale multiply in the epilogue.  A lane's 16-byte weight load is 32
// codes = one scale block of one weight row, and the order of k inside a dot product is free as long
// as both operands agree, so the 4 lanes (g = 0..3) that share weight row n own whole blocks: a
// "block-step" is four MFMA k-steps, step j over word j (codes 8j .. 8j + 7) of every lane's block,
// with the lane's A fragment read from the same 8 k.  The four lanes of a row own the four blocks of
// a "quad" (128 k): lane g block 4q + g.  So one weight load instruction reads 64 contiguous bytes
// per weight row and one A load touches two cache lines per A row (with a run of consecutive blocks
// per lane group it is four and eight: measured, the launch was then bound by those line touches at
// M >= 8), and the quad's four scales are one aligned dword, the same for the four lanes, of which
// lane g takes byte g.  A K-wave's slice is a whole number of quads (K % 128 == 0) and a batch is
// R = min(CH, quads left) of them, so the last batch shrinks and covers the slice exactly: no lane
// ever reads a block past its slice, and none idles.
//
// A wave is one 16-column B tile against MT = ceil(M / 16) A tiles (rows >= M read as zeros): a
// converted fragment is used by MT MFMAs, MT f32x4 accumulators.  All weight and scale loads of a
// batch are issued ahead of the batch's A loads, conversions and MFMAs.  A workgroup is KS x CW
// waves: KS waves split K (merged through LDS in wave order: no atomics, bit-reproducible), CW waves
// take neighbouring 16-column tiles of the same K slice.  SW: A = bf16(silu(g) * u) of a packed
// [M, 2K] gate|up input, the formula and rounding of gemv16_k / swiglu_fwd_k.
#include "common.h"
#include "../dpfs_api.h"

namespace dpfs {

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

// ---------------------------------------------------------------------------- quantiser ----
// One bf16 (its 16 bits) against the block scale s -> sign + e2m1 code.  |w| = mant 2^(e' - 134)
// (e' = max(e, 1), mant = the 7 mantissa bits plus the hidden one of a normal), so in units of 0.25
// q = mant 2^-t with t = s + 5 - e' >= 3 (s >= E - 2 >= e - 2).  Q is q with 24 fraction bits; the
// code counts the midpoints of the e2m1 grid (1, 3, 5, 7, 10, 14, 20 quarter units) below Q, a tie
// going to the even code; >= 6 saturates.  t > 24 only where q < 2^-16: code 0 either way.
__device__ __forceinline__ uint32_t w4_enc(uint32_t b, int s) {
  const int e = (b >> 7) & 0xFF;
  const uint32_t mant = (b & 0x7F) | (e ? 0x80u : 0u);
  const int t = min(s + 5 - max(e, 1), 24);
  const uint32_t Q = mant << (24 - t), f = 1u << 24;
  const uint32_t c = (Q > f) + (Q >= 3 * f) + (Q > 5 * f) + (Q >= 7 * f) + (Q > 10 * f) + (Q >= 14 * f) + (Q > 20 * f);
  return c | ((b >> 12) & 8);
}

// thread = 8 consecutive k of one row; the 4 lanes of a block are neighbours inside a wave
__global__ __launch_bounds__(256) void quant_w4_rows_k(const bf16* __restrict__ W, long long ldw,
                                                        uint8_t* __restrict__ codes, long long ldc,
                                                        uint8_t* __restrict__ scales, long long lds,
                                                        long long total, int K8) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const bool live = idx < total;                 // total % 4 == 0: a block's four lanes live or die together
  const long long n = live ? idx / K8 : 0;
  const int j = live ? (int)(idx % K8) : 0;
  const u32x4 v = *reinterpret_cast<const u32x4*>(W + n * ldw + 8 * j);
  uint32_t m = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) m = max(m, max(v[q] & 0x7FFF, (v[q] >> 16) & 0x7FFF));
  m = max(m, (uint32_t)__shfl_xor((int)m, 1));
  m = max(m, (uint32_t)__shfl_xor((int)m, 2));
  const int s = max((int)(m >> 7) - 2, 2);       // E - 2, floor 2: every dequantised value a normal bf16
  uint32_t out = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q)
    out |= (w4_enc(v[q] & 0xFFFF, s) | (w4_enc(v[q] >> 16, s) << 4)) << (8 * q);
  if (live) {
    *reinterpret_cast<uint32_t*>(codes + n * ldc + 4 * j) = out;
    if ((j & 3) == 0) scales[n * lds + (j >> 2)] = (uint8_t)s;
  }
}

// --------------------------------------------------------------------------- projection ----
__device__ __forceinline__ float silu_w4(float g) { return g * __builtin_amdgcn_rcpf(1.f + __expf(-g)); }   // = silu_f

// one word of a block (8 codes) and the block scale -> 8 bf16, exact
__device__ __forceinline__ bf16x8 w4_cvt8(uint32_t w, float scale) {
  const bf16x2 p0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 0);
  const bf16x2 p1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 1);
  const bf16x2 p2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 2);
  const bf16x2 p3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 3);
  return bf16x8{p0[0], p0[1], p1[0], p1[1], p2[0], p2[1], p3[0], p3[1]};
}

// quads (blocks per lane) per batch of weight loads: 4 VGPRs of codes and one of scales each
template <int MT> struct W4Batch { static constexpr int CH = MT == 1 ? 8 : 4; };

template <int MT, int KS, int CW, bool SW>
__global__ __launch_bounds__(64 * KS * CW) void gemv_w4_k(const bf16* __restrict__ A, long long lda,
                                                          const uint8_t* __restrict__ C4, long long ldc,
                                                          const uint8_t* __restrict__ S8, long long lds,
                                                          const float* __restrict__ bias, bf16* __restrict__ Y,
                                                          long long ldy, int M, int N, int K) {
  constexpr int CH = W4Batch<MT>::CH;
  __shared__ f32x4 red[CW][KS][MT][64];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), kw = wave % KS, cw = wave / KS;
  const int l = lane_id(), g = l >> 4, i = l & 15;
  const int n0 = (blockIdx.x * CW + cw) * 16;
  const int nq = K / 128;                      // quads of blocks
  const int per = (nq + KS - 1) / KS;
  const int b0 = 4 * min(nq, kw * per), b1 = 4 * min(nq, kw * per + per);   // (b0 == b1: a wave with no blocks adds zeros)
  const long long row = min(n0 + i, N - 1);
  const uint8_t* wp = C4 + row * ldc;
  const uint8_t* sp = S8 + row * lds;
  const bf16* ap[MT];
  bool mv[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    mv[t] = 16 * t + i < M;
    ap[t] = A + (long long)(mv[t] ? 16 * t + i : 0) * lda;
  }
  f32x4 acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int bb = b0; bb < b1;) {
    const int R = min(CH, (b1 - bb) >> 2);     // quads of this batch: bb + 4 R <= b1
    u32x4 wq[CH];
    uint32_t sc[CH];
#pragma unroll
    for (int u = 0; u < CH; ++u) {
      if (u < R) {
        wq[u] = *reinterpret_cast<const u32x4*>(wp + 16 * (bb + 4 * u + g));
        sc[u] = *reinterpret_cast<const uint32_t*>(sp + bb + 4 * u);     // bb % 4 == 0: aligned
      }
    }
#pragma unroll
    for (int u = 0; u < CH; ++u) {
      if (u < R) {
        const int k = 32 * (bb + 4 * u + g);
        const float scale = __uint_as_float(((sc[u] >> (8 * g)) & 0xFF) << 23);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          bf16x8 a[MT];
#pragma unroll
          for (int t = 0; t < MT; ++t) {
            if (SW) {
              const bf16x8 gv = *reinterpret_cast<const bf16x8*>(ap[t] + k + 8 * j);
              const bf16x8 uv = *reinterpret_cast<const bf16x8*>(ap[t] + K + k + 8 * j);
#pragma unroll
              for (int e = 0; e < 8; ++e) a[t][e] = (bf16)(silu_w4((float)gv[e]) * (float)uv[e]);
            } else {
              a[t] = *reinterpret_cast<const bf16x8*>(ap[t] + k + 8 * j);
            }
          }
          const bf16x8 b = w4_cvt8(wq[u][j], scale);
          const bf16x8 z = {};
#pragma unroll
          for (int t = 0; t < MT; ++t)
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(mv[t] ? a[t] : z, b, acc[t], 0, 0, 0);
        }
      }
    }
    bb += 4 * R;
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
      const float bv = bias ? bias[n] : 0.f;
#pragma unroll
      for (int t = 0; t < MT; ++t) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int m = 16 * t + 4 * g + j;
          if (m < M) Y[(long long)m * ldy + n] = (bf16)(acc[t][j] + bv);
        }
      }
    }
  }
}

template <int MT, int KS, int CW>
static void launch_w4(const void* A, long long lda, const void* C4, long long ldc, const void* S8, long long lds,
                      const float* bias, void* Y, long long ldy, int M, int N, int K, int swiglu, hipStream_t s) {
  const int nb = (N + 16 * CW - 1) / (16 * CW);
  if (swiglu)
    gemv_w4_k<MT, KS, CW, true><<<nb, 64 * KS * CW, 0, s>>>((const bf16*)A, lda, (const uint8_t*)C4, ldc,
                                                           (const uint8_t*)S8, lds, bias, (bf16*)Y, ldy, M, N, K);
  else
    gemv_w4_k<MT, KS, CW, false><<<nb, 64 * KS * CW, 0, s>>>((const bf16*)A, lda, (const uint8_t*)C4, ldc,
                                                            (const uint8_t*)S8, lds, bias, (bf16*)Y, ldy, M, N, K);
}

template <int MT>
static void launch_w4_mt(const void* A, long long lda, const void* C4, long long ldc, const void* S8, long long lds,
                         const float* bias, void* Y, long long ldy, int M, int N, int K, int swiglu, hipStream_t s) {
  // The launch rule, from N and K (that of dpfs_gemv_w8): a workgroup is 8 waves.  While the grid of
  // 16-column tiles is small (<= 512 tiles) and K gives every wave a quad of blocks (K >= 1024), all 8
  // waves split K over one tile (KS 8, CW 1); wide N and short K take 4 K-waves x 2 neighbouring
  // tiles (KS 4, CW 2): half the LDS merges per column, and the two tiles' A reads share L1 lines.
  const int tiles = (N + 15) / 16;
  if (tiles <= 512 && K / 128 >= 8) launch_w4<MT, 8, 1>(A, lda, C4, ldc, S8, lds, bias, Y, ldy, M, N, K, swiglu, s);
  else launch_w4<MT, 4, 2>(A, lda, C4, ldc, S8, lds, bias, Y, ldy, M, N, K, swiglu, s);
}

}  // namespace dpfs

using namespace dpfs;

// lda: A's row stride (bf16 elements); ldc, lds: the codes' and the scales' row strides (bytes)
extern "C" int dpfs_gemv_w4_ok(int M, int N, int K, long long lda, long long ldc, long long lds) {
  return M >= 1 && M <= 64 && N >= 1 && K > 0 && K % 128 == 0 && lda % 8 == 0 && ldc % 16 == 0 && ldc >= K / 2 &&
         lds % 4 == 0 && lds >= K / 32;
}

// Y[M, N] bf16 (row stride ldy) = (A or silu(g) u of A = [g | u]) wq^T (+ bias; null: none).  A and
// the codes 16-byte aligned, the scales 4-byte aligned.  No host state: graph-capturable.
extern "C" void dpfs_gemv_w4(const void* A, long long lda, const void* codes, long long ldc, const void* scales,
                             long long lds, const float* bias, void* Y, long long ldy, int M, int N, int K, int swiglu,
                             hipStream_t s) {
  switch ((M + 15) / 16) {
    case 1: launch_w4_mt<1>(A, lda, codes, ldc, scales, lds, bias, Y, ldy, M, N, K, swiglu, s); break;
    case 2: launch_w4_mt<2>(A, lda, codes, ldc, scales, lds, bias, Y, ldy, M, N, K, swiglu, s); break;
    case 3: launch_w4_mt<3>(A, lda, codes, ldc, scales, lds, bias, Y, ldy, M, N, K, swiglu, s); break;
    default: launch_w4_mt<4>(A, lda, codes, ldc, scales, lds, bias, Y, ldy, M, N, K, swiglu, s); break;
  }
}

// W bf16 [N, K] (row stride ldw elements, ldw % 8 == 0, K % 32 == 0, 16-byte aligned) -> codes uint8
// [N, K / 2] (row stride ldc bytes, ldc % 4 == 0) and scales uint8 [N, K / 32] (row stride lds bytes).
extern "C" void dpfs_quant_w4_rows(const void* W, long long ldw, void* codes, long long ldc, void* scales,
                                   long long lds, int N, int K, hipStream_t s) {
  const long long total = (long long)N * (K / 8);
  if (total > 0)
    quant_w4_rows_k<<<(unsigned)((total + 255) / 256), 256, 0, s>>>((const bf16*)W, ldw, (uint8_t*)codes, ldc,
                                                                    (uint8_t*)scales, lds, total, K / 8);
}
