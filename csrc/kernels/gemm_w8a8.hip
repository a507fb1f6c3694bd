// W8A8 prefill GEMM (gfx950): per-token e4m3 activation codes on the session's e4m3 weight codes, on the
// fp8 MFMA, both scales applied once in the epilogue:
//
//   y[m, n] = bf16( fp32(sum_k f32(ac[m,k]) f32(wc[n,k])) * sa[m] * inv[n] + bias[n] )
//
// ac uint8 [M, K] e4m3 with sa fp32 [M] (the per-row quantiser of gemv_w8.hip applied to the activation
// rows), wc uint8 [N, K] with inv fp32 [N] as the decode kernels read them: no second weight copy, no
// repacking.  Any M >= 1, N >= 1; K % 128 == 0.
//
// Main loop.  v_mfma_f32_16x16x128_f8f6f4 with both operands e4m3 (cbsz = blgp = 0, no scale operands): one
// MFMA per 128-k stage per 16 x 16 tile, and nothing else on the operand path: the codes are the MFMA's
// input as they lie in memory.  gemm_wq_k converts every weight code to bf16 by VALU between the MFMAs;
// here no VALU instruction touches an operand.
//
// Tile.  256 threads = 2 x 2 waves on a BM x 128 x 128 stage, BM = 32 TM (TM = 8, 4, 2, 1: 256, 128, 64 or
// 32 rows); a wave owns 16 TM rows x 64 columns = TM x 4 MFMA tiles, its TM x 4 f32x4 accumulators in
// registers for the whole K loop.  The wave tile is chosen from LDS traffic: a stage of a 128 x 64 wave
// tile is 32 MFMAs against (8 + 4) fragments x 2 KB = 24 KB of LDS reads, 0.75 KB per MFMA; the 64 x 64
// tile of gemm_wq_k would be 16 MFMAs against 16 KB, 1 KB per MFMA, at twice the matrix rate of bf16.  The
// MFMA runs transposed (weight fragment as the first operand), so a lane ends with 4 consecutive columns
// of one row: an 8-byte bf16 store.  The launcher takes the largest BM that still gives every CU a
// workgroup (256 CUs), else 32; tiles in the XCD-contiguous order of gemm_wq_k (the row tiles of one
// column tile are neighbours on one L2: its codes leave HBM once).
//
// Data path.  Both tiles go HBM / L2 -> LDS by LDS-DMA (buffer_load_dwordx4 ... lds), never through
// VGPRs.  A stage is [BM + 128 rows][128 B] = (BM + 128) / 8 pieces of 1 KiB (8 rows), one DMA instruction
// of one wave each, (BM + 128) / 32 per wave.  The DMA writes its 64 lanes' 16 bytes lane-linear, so the
// image's swizzle is applied to the SOURCE address: lane l of a piece fetches row 8 piece + (l >> 3),
// chunk (l & 7) ^ ((row >> 1) & 7), which lands in physical chunk l & 7: chunk c of row r sits at
// r * 128 + 16 (c ^ ((r >> 1) & 7)), the image of gemm_wq_k.  A lane's fragment is 32 consecutive k of one
// row: lane (i = l & 15, g = l >> 4) reads chunks 2g and 2g + 1 of row i as two ds_read_b128; the 16 lanes
// of a group read one chunk of rows 0 .. 15, sixteen distinct 16-byte slots of the 256 bytes the banks
// span.  A and B fragments follow the same rule, so the operands agree in k by construction whatever
// order the MFMA gives the 32 bytes.  Three LDS stages: while stage s is under the MFMAs, stages s + 1
// and s + 2 are in flight; one barrier per stage (the DMA of stage s + 2 is issued after the barrier that
// ends the reads of stage s - 1, whose slot it takes).  The wait in front of the barrier is s_waitcnt
// vmcnt(pieces of one stage): the wave's own pieces of stage s have landed, the barrier extends that to
// every wave's.
//
// Edges.  Rows >= M and columns >= N fetch the clamped last row (in bounds, and inside the buffer
// descriptors, whose records end with the last row's K bytes); their sums land in accumulators that are
// never stored.  Stores are guarded per row and per column, scalar where N % 4 != 0 or Y is unaligned.
// Epilogue: sa[m] and inv[n] (and bias[n]) are loaded once per tile into registers; two fp32 multiplies,
// one add, one bf16 rounding, none contracted.  No K split, no atomics, no host state: a call is
// run-to-run bit-identical and graph-capturable.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; no scratch, no spills):
//   TM  BM   VGPRs  AGPRs  SGPRs  LDS bytes  waves/SIMD
//    8  256   183    128     37    147456        1
//    4  128   119     64     37     98304        1
//    2   64    87     32     37     73728        2
//    1   32    70     16     37     61440        2
// (the accumulators are the AGPRs; LDS, three stages of (BM + 128) x 128 bytes, sets the waves of TM 4 and 2.)
//
// Precision.  The products of two e4m3 values are exact in fp32, but the instruction's sum of a 128-product
// step is not an fp32 sum in some order: against an fp64 reference the accumulator error reaches 1.84 x the
// bound (K + 2) 2^-24 sum|products| of such a sum at K = 128 (tests/test_gemm_w8a8_gpu.py, measured).
#include "common.h"
#include "../dpfs_api.h"

namespace dpfs {

typedef int i32x8 __attribute__((ext_vector_type(8)));

constexpr int A8_BN = 128, A8_BK = 128, A8_STAGES = 3;

// byte offset of 16-byte chunk c (16 k) of row r in a [rows][128 B] tile of codes
__device__ __forceinline__ int a8_lds(int r, int c) { return r * 128 + ((c ^ ((r >> 1) & 7)) << 4); }

// One LDS-DMA piece: 16 bytes per lane from r at byte (voff, per lane) + (soff, uniform) to lds_wave_base + 16 lane.
// (dma16 of common.h with the stage's uniform offset as the instruction's scalar offset)
__device__ __forceinline__ void a8_dma16(__amdgpu_buffer_rsrc_t r, char* lds_wave_base, unsigned voff, unsigned soff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (__attribute__((address_space(3))) void*)lds_wave_base, 16, voff, soff, 0,
                                           0);
}

template <int TM>
__global__ __launch_bounds__(256) void gemm_w8a8_k(const uint8_t* __restrict__ A, long long lda,
                                                   const float* __restrict__ sa, const uint8_t* __restrict__ C,
                                                   long long ldc, const float* __restrict__ inv,
                                                   const float* __restrict__ bias, bf16* __restrict__ Y, long long ldy,
                                                   int M, int N, int K, int row_tiles, int vec_store) {
  constexpr int BM = 32 * TM;
  constexpr int STAGE = (BM + A8_BN) * 128;   // bytes: the A tile, then the B tile
  constexpr int PA = BM / 32;                 // DMA pieces per wave and stage: of A,
  constexpr int P = PA + A8_BN / 32;          // and in all
  __shared__ __attribute__((aligned(1024))) char smem[A8_STAGES * STAGE];
  const int t = threadIdx.x, wave = t >> 6, l = t & 63, g = l >> 4, i = l & 15;
  const int wm = wave & 1, wn = wave >> 1;
  const int id = xcd_remap(blockIdx.x, gridDim.x);
  const int m0 = (id % row_tiles) * BM, n0 = (id / row_tiles) * A8_BN;

  // descriptors of the tile's rows: the records end with the K bytes of the operand's last row
  const long long ra_rows = M - 1 - m0, rb_rows = N - 1 - n0;
  const long long a_rec = min(ra_rows * lda + K, 0xFFFFFFFFLL), b_rec = min(rb_rows * ldc + K, 0xFFFFFFFFLL);
  const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint8_t*>(A + (long long)m0 * lda), (short)0, (int)(unsigned)a_rec, 0x00020000);
  const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint8_t*>(C + (long long)n0 * ldc), (short)0, (int)(unsigned)b_rec, 0x00020000);
  unsigned pbase[P];                           // the lane's source offset of piece q at stage 0
#pragma unroll
  for (int q = 0; q < P; ++q) {
    const bool isA = q < PA;
    const int r = 8 * (wave + 4 * (isA ? q : q - PA)) + (l >> 3);      // row in its tile
    const int c = (l & 7) ^ ((r >> 1) & 7);
    const long long row = isA ? min((long long)r, ra_rows) : min((long long)r, rb_rows);
    pbase[q] = (unsigned)(row * (isA ? lda : ldc) + 16 * c);
  }
  auto issue = [&](int kt, int slot) {         // stage kt: HBM / L2 -> LDS slot
#pragma unroll
    for (int q = 0; q < P; ++q)
      a8_dma16(q < PA ? ra : rb, smem + slot * STAGE + (wave + 4 * q) * 1024, pbase[q], kt * A8_BK);
  };

  f32x4 acc[TM][4];
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  // the lane's fragment offsets in a stage: row 16 tile + i, chunks 2g and 2g + 1 (rows 16 apart keep the swizzle)
  const int fo0 = a8_lds(i, 2 * g), fo1 = a8_lds(i, 2 * g + 1);
  auto frag = [&](const char* tile, int tile16) -> i32x8 {
    const u32x4 lo = *reinterpret_cast<const u32x4*>(tile + tile16 * 2048 + fo0);
    const u32x4 hi = *reinterpret_cast<const u32x4*>(tile + tile16 * 2048 + fo1);
    return i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
  };

  const int nk = K / A8_BK;
  issue(0, 0);
  if (nk > 1) issue(1, 1);
  int slot = 0;
  for (int kt = 0; kt < nk; ++kt) {
    if (kt + 1 < nk) wait_vmcnt<P>();          // stage kt landed; stage kt + 1 may be in flight
    else wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();
    if (kt + 2 < nk) issue(kt + 2, slot == 0 ? 2 : slot - 1);
    const char* sA = smem + slot * STAGE;
    const char* sB = sA + BM * 128;
    i32x8 fb[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) fb[b] = frag(sB, 4 * wn + b);
#pragma unroll
    for (int a = 0; a < TM; ++a) {
      const i32x8 fa = frag(sA, TM * wm + a);
#pragma unroll
      for (int b = 0; b < 4; ++b)              // D[4g + j = column][i = row]
        acc[a][b] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fb[b], fa, acc[a][b], 0, 0, 0, 0, 0, 0);
    }
    slot = slot == 2 ? 0 : slot + 1;
  }

  // epilogue: the lane's 16 columns' inv / bias and its TM rows' sa once into registers, guarded stores
  float sc[4][4], bv[4][4];
#pragma unroll
  for (int b = 0; b < 4; ++b)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = min(n0 + 16 * (4 * wn + b) + 4 * g + j, N - 1);
      sc[b][j] = inv[n];
      bv[b][j] = bias ? bias[n] : 0.f;
    }
#pragma unroll
  for (int a = 0; a < TM; ++a) {
    const int m = m0 + 16 * (TM * wm + a) + i;
    if (m >= M) continue;
    const float sm = sa[m];
    bf16* yr = Y + (long long)m * ldy;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int n = n0 + 16 * (4 * wn + b) + 4 * g;
      bf16x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = (bf16)__fadd_rn(__fmul_rn(__fmul_rn(acc[a][b][j], sm), sc[b][j]), bv[b][j]);
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

template <int TM>
static void launch_w8a8(const void* A, long long lda, const float* sa, const void* C, long long ldc, const float* inv,
                        const float* bias, void* Y, long long ldy, int M, int N, int K, hipStream_t s) {
  const int rt = (M + 32 * TM - 1) / (32 * TM), ct = (N + A8_BN - 1) / A8_BN;
  const int vec = reinterpret_cast<uintptr_t>(Y) % 8 == 0 && ldy % 4 == 0;
  gemm_w8a8_k<TM><<<rt * ct, 256, 0, s>>>((const uint8_t*)A, lda, sa, (const uint8_t*)C, ldc, inv, bias, (bf16*)Y, ldy,
                                          M, N, K, rt, vec);
}

}  // namespace dpfs

using namespace dpfs;

// lda, ldc: the row strides of the activation and the weight codes (bytes).  A tile's source offsets are
// 32-bit: 256 rows of either operand stay below 2^31 bytes.
extern "C" int dpfs_gemm_w8a8_ok(int M, int N, int K, long long lda, long long ldc) {
  return M >= 1 && N >= 1 && K > 0 && K % A8_BK == 0 && lda % 16 == 0 && lda >= K && ldc % 16 == 0 && ldc >= K &&
         lda < (1LL << 23) && ldc < (1LL << 23) &&
         ((long long)(M + 31) / 32) * ((N + A8_BN - 1) / A8_BN) < (1LL << 31);
}

// Y[M, N] bf16 (row stride ldy) = (acodes codes^T) * sa[m] * inv[n] (+ bias; null: none).  Both code
// matrices 16-byte aligned.  The launch rule: the largest row tile (256, 128, 64) whose grid still has a
// workgroup for every CU (256), else 32 rows.  No host state: graph-capturable.
extern "C" void dpfs_gemm_w8a8(const void* acodes, long long lda, const float* sa, const void* codes, long long ldc,
                               const float* inv, const float* bias, void* Y, long long ldy, int M, int N, int K,
                               hipStream_t s) {
  const long long ct = (N + A8_BN - 1) / A8_BN;
  if ((M + 255) / 256 * ct >= 256) launch_w8a8<8>(acodes, lda, sa, codes, ldc, inv, bias, Y, ldy, M, N, K, s);
  else if ((M + 127) / 128 * ct >= 256) launch_w8a8<4>(acodes, lda, sa, codes, ldc, inv, bias, Y, ldy, M, N, K, s);
  else if ((M + 63) / 64 * ct >= 256) launch_w8a8<2>(acodes, lda, sa, codes, ldc, inv, bias, Y, ldy, M, N, K, s);
  else launch_w8a8<1>(acodes, lda, sa, codes, ldc, inv, bias, Y, ldy, M, N, K, s);
}
