// Quantised-weight prefill GEMM (gfx950): y[M, N] = a[M, K] wq[N, K]^T for any M, on the weight codes
// of the decode kernels (gemv_w8.hip, gemv_w4.hip) and with their formulas and rounding points:
//
//   W8  codes uint8 [N, K] e4m3, inv fp32 [N], K % 64 == 0:
//       y = bf16( fp32(sum_k a[m,k] f32(code[n,k])) * inv[n] + bias[n] )    (the scale once, in the epilogue)
//   W4  codes uint8 [N, K / 2] e2m1 (low nibble first), scales uint8 [N, K / 32] e8m0, K % 128 == 0:
//       y = bf16( fp32(sum_k a[m,k] wq[n,k]) + bias[n] )                    (the block scale inside wq)
//
// The M <= 64 kernels convert a weight fragment in registers in every wave that uses it; past four row
// tiles that work, not the weight bytes, is their time.  Here a workgroup converts each code of its B tile
// once, into LDS, and every wave reads bf16 fragments from there.
//
// Tile.  256 threads = 2 x 2 waves on a BM x 128 x 64 stage, BM = 32 TM (TM = 4, 2, 1: 128, 64 or 32 rows);
// a wave owns 16 TM rows x 64 columns = TM x 4 tiles of v_mfma_f32_16x16x32_bf16, its fp32 accumulators
// (TM x 4 f32x4) in registers for the whole K loop.  The MFMA runs transposed (B fragment as the first
// operand), so a lane ends with 4 consecutive columns of one row: an 8-byte bf16 store.  At TM = 4 a stage
// is 32 MFMAs per wave against, per lane, 16 packed converts and 4 ds_write_b128 (W8: two 16-byte code
// loads of 16 codes; W4: one of 32 codes) plus 4 A chunks: the conversion fits under the matrix time.  The
// launcher takes the largest BM that still gives every CU a workgroup (256 CUs), else 32.
//
// Data path.  B: codes travel HBM -> registers in 16-byte loads, issued for stage s + 1 before the MFMAs
// of stage s; after them they are converted with v_cvt_scalef32_pk_bf16_fp8 / _fp4 (exact: every e4m3
// value and every e2m1 x 2^e, s >= 2, is a bf16 value) and written to the other LDS buffer as bf16.  A
// W4 load is one 32-k scale block of one weight row, so a lane's conversion group never straddles a block
// and its scale byte is loaded once, with the codes.  A: bf16, staged through registers the same way (not
// re-read from L2 per column tile: every wave reads its A fragments from LDS).  Two stages are in flight:
// one in LDS under the MFMAs, the next in registers; one barrier per stage (a stage's writes go to the
// buffer whose last reads ended at the previous barrier).
//
// LDS image.  Both tiles are [rows][64 k] bf16 = 128-byte rows of eight 16-byte chunks, chunk c of row r at
// r * 128 + 16 (c ^ ((r >> 1) & 7)).  A fragment read (ds_read_b128) is lane (i = l & 15, g = l >> 4) ->
// row i, chunk 4 step + g: the 16 lanes of a group read rows 0 .. 15 of one chunk, whose sixteen 16-byte
// slots ((r & 1) * 8 + (c ^ (r >> 1))) are all distinct in the 256 bytes the banks span: no conflict.  The
// order of k is the same natural one in both tiles, so the operands agree by construction.
//
// Edges.  Rows >= M and columns >= N read the clamped last row of A / the codes (in bounds; their sums
// land in accumulators that are never stored); stores are guarded per row and per column.  No K split, no
// atomics, no host state: a call is run-to-run bit-identical and graph-capturable.
#include "common.h"
#include "../dpfs_api.h"

namespace dpfs {

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ bf16x8 wq_pack8(bf16x2 p0, bf16x2 p1, bf16x2 p2, bf16x2 p3) {
  return bf16x8{p0[0], p0[1], p1[0], p1[1], p2[0], p2[1], p3[0], p3[1]};
}

// 8 e4m3 codes (two words) -> 8 bf16, exact
__device__ __forceinline__ bf16x8 wq_cvt8_fp8(uint32_t w0, uint32_t w1) {
  return wq_pack8(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, 1.0f, false),
                  __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, 1.0f, true),
                  __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, 1.0f, false),
                  __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, 1.0f, true));
}

// 8 e2m1 codes (one word) and their block scale -> 8 bf16, exact
__device__ __forceinline__ bf16x8 wq_cvt8_fp4(uint32_t w, float scale) {
  return wq_pack8(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 0),
                  __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 1),
                  __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 2),
                  __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 3));
}

// byte offset of 16-byte chunk c (8 k) of row r in a [rows][64] bf16 tile
__device__ __forceinline__ int wq_lds(int r, int c) { return r * 128 + ((c ^ ((r >> 1) & 7)) << 4); }

constexpr int WQ_BN = 128, WQ_BK = 64;

template <bool W4, int TM>
__global__ __launch_bounds__(256) void gemm_wq_k(const bf16* __restrict__ A, long long lda,
                                                 const uint8_t* __restrict__ C, long long ldc,
                                                 const uint8_t* __restrict__ S, long long lds,
                                                 const float* __restrict__ inv, const float* __restrict__ bias,
                                                 bf16* __restrict__ Y, long long ldy, int M, int N, int K, int row_tiles,
                                                 int vec_store) {
  constexpr int BM = 32 * TM;
  constexpr int NB = W4 ? 1 : 2;        // 16-byte code loads per lane and stage
  constexpr int RL = W4 ? 2 : 4;        // code loads per weight row and stage
  constexpr int CL = W4 ? 4 : 2;        // 8-k chunks per code load
  __shared__ __attribute__((aligned(16))) char sA[2][BM * 128];
  __shared__ __attribute__((aligned(16))) char sB[2][WQ_BN * 128];
  const int t = threadIdx.x, wave = t >> 6, l = t & 63, g = l >> 4, i = l & 15;
  const int wm = wave & 1, wn = wave >> 1;
  // consecutive ids share an XCD's L2; the row tiles of one column tile are neighbours: its codes leave HBM once
  const int id = xcd_remap(blockIdx.x, gridDim.x);
  const int m0 = (id % row_tiles) * BM, n0 = (id / row_tiles) * WQ_BN;

  const bf16* ag[TM];
  int ao[TM];
#pragma unroll
  for (int p = 0; p < TM; ++p) {
    const int idx = t + 256 * p, r = idx >> 3, c = idx & 7;
    ag[p] = A + (long long)min(m0 + r, M - 1) * lda + 8 * c;
    ao[p] = wq_lds(r, c);
  }
  const uint8_t* bg[NB];
  const uint8_t* sg = nullptr;
  int bo[NB];                            // (row, first chunk) of the load: its CL chunks follow in k order
#pragma unroll
  for (int p = 0; p < NB; ++p) {
    const int idx = t + 256 * p, r = idx / RL, j = idx % RL;
    const long long row = min(n0 + r, N - 1);
    bg[p] = C + row * ldc + 16 * j;
    if (W4) sg = S + row * lds + j;
    bo[p] = (r << 8) | (CL * j);
  }

  bf16x8 ra[TM];
  u32x4 rb[NB];
  uint32_t rs = 0;
  auto fetch = [&](int kt) {             // stage kt: HBM / L2 -> registers
#pragma unroll
    for (int p = 0; p < TM; ++p) ra[p] = *reinterpret_cast<const bf16x8*>(ag[p] + WQ_BK * kt);
#pragma unroll
    for (int p = 0; p < NB; ++p) rb[p] = *reinterpret_cast<const u32x4*>(bg[p] + (W4 ? WQ_BK / 2 : WQ_BK) * kt);
    if (W4) rs = sg[2 * kt];
  };
  auto stash = [&](int buf) {            // registers -> bf16 LDS image (the one conversion of every code)
#pragma unroll
    for (int p = 0; p < TM; ++p) *reinterpret_cast<bf16x8*>(sA[buf] + ao[p]) = ra[p];
#pragma unroll
    for (int p = 0; p < NB; ++p) {
      const int r = bo[p] >> 8, c = bo[p] & 255;
      if (W4) {
        const float scale = __uint_as_float(rs << 23);
#pragma unroll
        for (int q = 0; q < 4; ++q)
          *reinterpret_cast<bf16x8*>(sB[buf] + wq_lds(r, c + q)) = wq_cvt8_fp4(rb[p][q], scale);
      } else {
#pragma unroll
        for (int q = 0; q < 2; ++q)
          *reinterpret_cast<bf16x8*>(sB[buf] + wq_lds(r, c + q)) = wq_cvt8_fp8(rb[p][2 * q], rb[p][2 * q + 1]);
      }
    }
  };

  f32x4 acc[TM][4];
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = K / WQ_BK;
  fetch(0);
  stash(0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    const bool more = kt + 1 < nk;
    if (more) fetch(kt + 1);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      bf16x8 fa[TM], fb[4];
#pragma unroll
      for (int a = 0; a < TM; ++a)
        fa[a] = *reinterpret_cast<const bf16x8*>(sA[buf] + wq_lds(16 * (TM * wm + a) + i, 4 * s + g));
#pragma unroll
      for (int b = 0; b < 4; ++b)
        fb[b] = *reinterpret_cast<const bf16x8*>(sB[buf] + wq_lds(16 * (4 * wn + b) + i, 4 * s + g));
#pragma unroll
      for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)     // D[4g + j = column][i = row]
          acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[b], fa[a], acc[a][b], 0, 0, 0);
    }
    if (more) stash(buf ^ 1);
    __syncthreads();
  }

  // epilogue: the lane's 16 columns' inv / bias once into registers, then guarded bf16 stores
  float sc[4][4], bv[4][4];
#pragma unroll
  for (int b = 0; b < 4; ++b)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = min(n0 + 16 * (4 * wn + b) + 4 * g + j, N - 1);
      sc[b][j] = W4 ? 1.f : inv[n];
      bv[b][j] = bias ? bias[n] : 0.f;
    }
#pragma unroll
  for (int a = 0; a < TM; ++a) {
    const int m = m0 + 16 * (TM * wm + a) + i;
    if (m >= M) continue;
    bf16* yr = Y + (long long)m * ldy;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int n = n0 + 16 * (4 * wn + b) + 4 * g;
      bf16x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = (bf16)(W4 ? acc[a][b][j] + bv[b][j] : acc[a][b][j] * sc[b][j] + bv[b][j]);
      if (vec_store && n + 3 < N) {
        *reinterpret_cast<bf16x4*>(yr + n) = o;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (n + j < N) yr[n + j] = o[j];
      }
    }
  }
}

template <bool W4, int TM>
static void launch_wq(const void* A, long long lda, const void* C, long long ldc, const void* S, long long lds,
                      const float* inv, const float* bias, void* Y, long long ldy, int M, int N, int K, hipStream_t s) {
  const int rt = (M + 32 * TM - 1) / (32 * TM), ct = (N + WQ_BN - 1) / WQ_BN;
  const int vec = reinterpret_cast<uintptr_t>(Y) % 8 == 0 && ldy % 4 == 0;
  gemm_wq_k<W4, TM><<<rt * ct, 256, 0, s>>>((const bf16*)A, lda, (const uint8_t*)C, ldc, (const uint8_t*)S, lds, inv,
                                            bias, (bf16*)Y, ldy, M, N, K, rt, vec);
}

// The launch rule: the largest row tile (128, 64, 32) whose grid still has a workgroup for every CU
// (256), else 32 rows: below that the launch is short of workgroups, not of MFMA rate.
template <bool W4>
static void launch_wq_tm(const void* A, long long lda, const void* C, long long ldc, const void* S, long long lds,
                         const float* inv, const float* bias, void* Y, long long ldy, int M, int N, int K,
                         hipStream_t s) {
  const long long ct = (N + WQ_BN - 1) / WQ_BN;
  if ((M + 127) / 128 * ct >= 256) launch_wq<W4, 4>(A, lda, C, ldc, S, lds, inv, bias, Y, ldy, M, N, K, s);
  else if ((M + 63) / 64 * ct >= 256) launch_wq<W4, 2>(A, lda, C, ldc, S, lds, inv, bias, Y, ldy, M, N, K, s);
  else launch_wq<W4, 1>(A, lda, C, ldc, S, lds, inv, bias, Y, ldy, M, N, K, s);
}

static bool wq_grid_ok(int M, int N) {
  return ((long long)(M + 31) / 32) * ((N + WQ_BN - 1) / WQ_BN) < (1LL << 31);
}

}  // namespace dpfs

using namespace dpfs;

// lda: A's row stride (bf16 elements); ldc, lds: the codes' and the scales' row strides (bytes)
extern "C" int dpfs_gemm_wq8_ok(int M, int N, int K, long long lda, long long ldc) {
  return M >= 1 && N >= 1 && K > 0 && K % 64 == 0 && lda % 8 == 0 && lda >= K && ldc % 16 == 0 && ldc >= K &&
         wq_grid_ok(M, N);
}

extern "C" int dpfs_gemm_wq4_ok(int M, int N, int K, long long lda, long long ldc, long long lds) {
  return M >= 1 && N >= 1 && K > 0 && K % 128 == 0 && lda % 8 == 0 && lda >= K && ldc % 16 == 0 && ldc >= K / 2 &&
         lds % 4 == 0 && lds >= K / 32 && wq_grid_ok(M, N);
}

// Y[M, N] bf16 (row stride ldy) = (A codes^T) * inv (+ bias; null: none).  A and the codes 16-byte
// aligned.  No host state: graph-capturable.
extern "C" void dpfs_gemm_wq8(const void* A, long long lda, const void* codes, long long ldc, const float* inv,
                              const float* bias, void* Y, long long ldy, int M, int N, int K, hipStream_t s) {
  launch_wq_tm<false>(A, lda, codes, ldc, nullptr, 0, inv, bias, Y, ldy, M, N, K, s);
}

// Y[M, N] bf16 (row stride ldy) = A wq^T (+ bias; null: none), wq = e2m1(code) * 2^(scale - 127).
extern "C" void dpfs_gemm_wq4(const void* A, long long lda, const void* codes, long long ldc, const void* scales,
                              long long lds, const float* bias, void* Y, long long ldy, int M, int N, int K,
                              hipStream_t s) {
  launch_wq_tm<true>(A, lda, codes, ldc, scales, lds, nullptr, bias, Y, ldy, M, N, K, s);
}
