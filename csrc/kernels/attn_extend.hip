// Prefill against a KV cache (gfx950): T > 1 new tokens of every sequence attend the keys the
// cache already holds plus the causal part of their own chunk.  This is the case between the
// causal flash prefill (attention.hip: empty cache) and the single-query attn_decode
// (decode.hip: one new token); generation.py uses it for chunked prompts and for multi-token
// continuations of uniform and ragged caches.
//
//   kv_append_chunk_k  the k / v parts of packed qkv row (b, t) go to cache row len[b] + t,
//                      for t < n[b] and len[b] + t < Tmax; every other cache byte is untouched.
//   attn_extend_k      grid (ceil(T / 32), B * H): one workgroup per (32-query tile, b, h).
//
// attn_extend_k follows the 32x32x16 forward of attention.hip (attn_fwd3_k): S^T = K Q^T with
// the query on the lane (C/D column) and the keys in the 16 registers, so the online softmax is
// lane-local plus one exchange between lanes l and l ^ 32 (same query, other keys), and P^T
// rounded to bf16 in registers is directly the B operand of O^T += V^T P^T; V^T comes from LDS
// by ds_read_b64_tr_b16 with the matching k order.  What differs:
//  * query (b, t) sees keys [0, len[b] + t]: the diagonal sits at the per-row offset len[b],
//    read from DEVICE memory (no host synchronisation; len has 1 or B elements, as in decode);
//  * query (b, t) is live iff t < n[b] (n null: T) and len[b] + t < Tmax; a query that is not
//    live loads nothing and stores zeros.  Q rows of queries that are not live are replaced by
//    zeros, masked scores are selected (not multiplied) away, and V rows past the tile's last
//    attended key are staged as zeros, so NaN in padded q rows or in cache rows nobody attends
//    cannot reach a live output;
//  * the 4 waves of a workgroup share the 32 queries and take the 32-key tiles w, w + 4, ...
//    (a short chunk over a long prefix still spreads its keys over the waves); key tiles wholly
//    above the tile's diagonal are never visited.  Each wave stages its own V tile in its own
//    LDS region (wave-local ordering only), and at the end the waves' (m, l, O) partials meet
//    in LDS and are merged in wave order: deterministic, no atomics, no waiting between
//    workgroups.
//
// fp8 KV cache (Q8 = true; the row format is in kv8.h): the cache operands are e4m3 codes with
// one fp32 scale per (b, key, h) row, converted where they are used and nothing else changed:
// the K fragment becomes bf16_rn(f32(code) * ks[row]) (one scale per lane per tile: the lane's
// A-operand row) and the V chunks staged to LDS bf16_rn(f32(code) * vs[row]), so the kernel
// equals, bit for bit, the bf16 form run on caches dequantised to bf16 by that expression.  The
// prefetched tile is held as codes (half the registers of the bf16 prefetch).
//
// Paged KV cache (PAGED = true; the layout and its safety contract are in kv_page.h): the caches
// are pools addressed through a block table.  Tiles, waves and the merge stay on the logical key
// index; only the K-row and V-chunk fetches differ, each lane looking up the pool row of the key
// it loads, so the output equals the contiguous launch on the same cache content bit for bit.
#include "common.h"
#include "kv8.h"
#include "kv_page.h"
#include "../dpfs_api.h"
#include "attn_common.h"

namespace dpfs {

constexpr int kExtQ = 32;    // queries per workgroup
constexpr int kExtK = 32;    // keys per wave tile

// 16-byte chunk swizzle of a wave's [32][HD] V tile: conflict-free for the transposed reads
// (32 lanes = 4 rows x 64 B); hd 32 rows are one 64-B span, left as they are.
template <int HD>
__device__ __forceinline__ int ext_swz(int r, int ch) {
  if (HD == 32) return ch;
  return HD == 64 ? (ch ^ (((r >> 1) & 1) << 2)) : (ch ^ ((r & 3) << 2));
}

template <int HD, bool Q8 = false, bool PAGED = false, typename... PG>
__global__ __launch_bounds__(256) void attn_extend_k(const bf16* __restrict__ q, long long ldq,
                                                     const void* __restrict__ kcv, const void* __restrict__ vcv,
                                                     const float* __restrict__ ksc, const float* __restrict__ vsc,
                                                     const int* __restrict__ len_ptr, int len_rows,
                                                     const int* __restrict__ n_ptr, bf16* __restrict__ o, int T,
                                                     int H, int Tmax, float scale, PG... pgv) {
  const KvPageArgs<PAGED> pg = kv_page_args<PAGED>(pgv...);
  constexpr int KS = HD / 16, DTN = HD / 32, RB = HD * 2, CPR = HD / 8;
  constexpr int VT = kExtK * RB;             // a wave's V tile
  constexpr int NVC = kExtK * CPR / 64;      // 16-byte V chunks per lane per tile
  constexpr int OLD = HD + 4;                // padded fp32 row of the merge image
  constexpr int MERGE = 4 * kExtQ * OLD * 4;
  static_assert(4 * VT <= MERGE, "the V tiles alias the merge image");
  __shared__ __attribute__((aligned(16))) char smem[MERGE];
  __shared__ float ml_lds[4][kExtQ][2];

  const int bh = blockIdx.y, b = bh / H, h = bh % H;
  const int q0 = blockIdx.x * kExtQ;
  const int wave = threadIdx.x >> 6, l = lane_id(), r32 = l & 31, hf = l >> 5, g16 = l >> 4, i16 = l & 15;
  KASSERT(len_ptr[len_rows ? b : 0] >= 0, "cache length %d of sequence %d", len_ptr[len_rows ? b : 0], b);
  const int len = len_ptr[len_rows ? b : 0];
  const int nb = n_ptr ? min(max(n_ptr[b], 0), T) : T;
  // live queries of this sequence: t < nlive
  const int nlive = len < 0 ? 0 : min(nb, Tmax - len);
  bf16* obase = o + ((long long)b * T) * ((long long)H * HD) + (long long)h * HD;

  if (q0 >= nlive) {   // block-uniform: nothing to attend, the tile's rows are zeros
    const int qq = threadIdx.x >> 3, part = threadIdx.x & 7;
    if (q0 + qq < T) {
      bf16* orow = obase + (long long)(q0 + qq) * H * HD + part * (HD / 8);
      const bf16x4 z = {};
#pragma unroll
      for (int c = 0; c < HD / 32; ++c) *reinterpret_cast<bf16x4*>(orow + 4 * c) = z;
    }
    return;
  }
  const int kmax = len + min(q0 + kExtQ, nlive) - 1;   // last key any query of the tile attends (< Tmax)
  const int nkt = kmax / kExtK + 1;
  const float c2 = scale * kLog2e;

  // Q^T operand: lane holds Q[q0 + r32][16 ks + 8 hf + j]; zeros for a query that is not live
  const int tq = q0 + r32;
  const bool live = tq < nlive;
  bf16x8 qf[KS];
  {
    const bf16* qrow = q + ((long long)b * T + tq) * ldq + (long long)h * HD + 8 * hf;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      bf16x8 v = {};
      if (live) v = *reinterpret_cast<const bf16x8*>(qrow + 16 * ks);
      qf[ks] = v;
    }
  }
  // the last key of this lane's query, relative to its first key row of a tile (4 hf)
  const int qlim = (live ? len + tq : -1) - 4 * hf;

  // PAGED: the bases are the pools' (head h of pool row 0) and krow() maps a key of this sequence
  // to its pool row, one table lookup per lane and fetch (a 32-key tile may span two pages)
  const long long seq0 = PAGED ? 0 : (long long)b * Tmax * H;
  const bf16* kbase = (const bf16*)kcv + (seq0 + h) * HD;
  const bf16* vbase = (const bf16*)vcv + (seq0 + h) * HD;
  const uint8_t* k8base = (const uint8_t*)kcv + (seq0 + h) * HD;
  const uint8_t* v8base = (const uint8_t*)vcv + (seq0 + h) * HD;
  const long long sbase = seq0 + h;   // scale of key row k: sbase + k * H
  const long long ldkv = (long long)H * HD;
  auto krow = [&](int k) __attribute__((always_inline)) -> long long {
    if constexpr (PAGED) return kv_page_row(pg, b, k);
    else return (long long)k;
  };
  char* lv = smem + wave * VT;
  // V^T fragment reads (as attn_fwd3_k): rows 16 s + 4 hf + (i16 >> 2) [+ 8], d columns
  // 32 dt + 16 (g16 & 1) + 4 (i16 & 3); the swizzle ignores the row bits the 16 s / + 8 steps move
  int voff[DTN];
#pragma unroll
  for (int dt = 0; dt < DTN; ++dt) {
    const int row = 4 * hf + (i16 >> 2);
    const int col = 32 * dt + 16 * (g16 & 1) + 4 * (i16 & 3);
    voff[dt] = row * RB + (ext_swz<HD>(row, col >> 3) << 4) + (col & 7) * 2;
  }

  // the prefetched tile: bf16 values, or with Q8 codes (8 per register pair) and their row scales
  bf16x8 kreg[Q8 ? 1 : KS];
  u32x4 vreg[Q8 ? 1 : NVC];
  u32x2 kreg8[Q8 ? KS : 1], vreg8[Q8 ? NVC : 1];
  float ksreg = 0.f, vsreg[Q8 ? NVC : 1];
  // K fragment (A operand): lane holds K[k0 + r32][16 ks + 8 hf + j]; rows past kmax are masked
  // after the product, so they may hold anything, but the address stays inside the cache.
  // V rows past kmax are zeros: their P is 0, and 0 x NaN would not be.
  auto fetch = [&](int kt) __attribute__((always_inline)) {
    const int k0 = kt * kExtK;
    if constexpr (Q8) {
      const long long kr = krow(min(k0 + r32, kmax));
      const uint8_t* kptr = k8base + kr * ldkv + 8 * hf;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) kreg8[ks] = *reinterpret_cast<const u32x2*>(kptr + 16 * ks);
      ksreg = ksc[sbase + kr * H];
#pragma unroll
      for (int i = 0; i < NVC; ++i) {
        const int c = l + 64 * i, r = c / CPR, ch = c % CPR;
        u32x2 v = {0u, 0u};
        float sc = 0.f;                      // rows past kmax: code 0 x scale 0 = the staged zero
        if (k0 + r <= kmax) {
          const long long vr = krow(k0 + r);
          v = *reinterpret_cast<const u32x2*>(v8base + vr * ldkv + ch * 8);
          sc = vsc[sbase + vr * H];
        }
        vreg8[i] = v;
        vsreg[i] = sc;
      }
    } else {
      const bf16* kptr = kbase + krow(min(k0 + r32, kmax)) * ldkv + 8 * hf;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) kreg[ks] = *reinterpret_cast<const bf16x8*>(kptr + 16 * ks);
#pragma unroll
      for (int i = 0; i < NVC; ++i) {
        const int c = l + 64 * i, r = c / CPR, ch = c % CPR;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (k0 + r <= kmax) v = *reinterpret_cast<const u32x4*>(vbase + krow(k0 + r) * ldkv + ch * 8);
        vreg[i] = v;
      }
    }
  };

  f32x16 oacc[DTN];
#pragma unroll
  for (int d = 0; d < DTN; ++d)
#pragma unroll
    for (int i = 0; i < 16; ++i) oacc[d][i] = 0.f;
  float m = -INFINITY, lsum = 0.f;

  if (wave < nkt) fetch(wave);
  for (int kt = wave; kt < nkt; kt += 4) {
    const int k0 = kt * kExtK;
    // this tile's V into the wave's LDS region (the wave's earlier reads of it have returned:
    // their values fed the MFMAs above); LDS serves a wave's operations in order
    asm volatile("" ::: "memory");
#pragma unroll
    for (int i = 0; i < NVC; ++i) {
      const int c = l + 64 * i, r = c / CPR, ch = c % CPR;
      if constexpr (Q8)
        *reinterpret_cast<bf16x8*>(lv + r * RB + (ext_swz<HD>(r, ch) << 4)) = kv8_dec8_bf16(vreg8[i], vsreg[i]);
      else
        *reinterpret_cast<u32x4*>(lv + r * RB + (ext_swz<HD>(r, ch) << 4)) = vreg[i];
    }
    bf16x8 kcur[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      if constexpr (Q8) kcur[ks] = kv8_dec8_bf16(kreg8[ks], ksreg);
      else kcur[ks] = kreg[ks];
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    if (kt + 4 < nkt) fetch(kt + 4);   // the next tile's loads fly under this tile's math

    f32x16 s;
#pragma unroll
    for (int i = 0; i < 16; ++i) s[i] = 0.f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) s = MFMA32(kcur[ks], qf[ks], s);
    // key k0 + 8 (i >> 2) + 4 hf + (i & 3) is attended iff it is <= len + tq
    const bool need_mask = k0 + kExtK - 1 > len + q0 || q0 + kExtQ > nlive;   // wave-uniform
    if (need_mask) {
      const int lim = qlim - k0;
#pragma unroll
      for (int i = 0; i < 16; ++i) s[i] = (8 * (i >> 2) + (i & 3) > lim) ? -INFINITY : s[i];
    }
    float mx = s[0];
#pragma unroll
    for (int i = 1; i < 16; ++i) mx = fmaxf(mx, s[i]);
    mx = pair_max(mx) * c2;                     // both lanes of a query move m together
    const float mnew = fmaxf(m, mx);
    const float ms = mnew == -INFINITY ? 0.f : mnew;   // no key yet: p = exp2(-inf) = 0
    const float alpha = __builtin_amdgcn_exp2f(m - ms);
    m = mnew;
    lsum *= alpha;
#pragma unroll
    for (int d = 0; d < DTN; ++d) oacc[d] *= alpha;
    float ps = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      s[i] = __builtin_amdgcn_exp2f(fmaf(s[i], c2, -ms));
      ps += s[i];
    }
    lsum += ps;
    bf16x8 pk[2];
#pragma unroll
    for (int k2 = 0; k2 < 2; ++k2)
#pragma unroll
      for (int j = 0; j < 8; ++j) pk[k2][j] = (bf16)s[8 * k2 + j];
    // O^T[d][q] += V^T[d][k] P^T[k][q]
#pragma unroll
    for (int dt = 0; dt < DTN; ++dt)
#pragma unroll
      for (int k2 = 0; k2 < 2; ++k2) {
        const char* vb = lv + voff[dt] + 16 * k2 * RB;
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)vb);
        const s16x4 hi =
            __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(vb + 8 * RB));
        oacc[dt] = MFMA32(tr_join(lo, hi), pk[k2], oacc[dt]);
      }
  }

  // the waves' partials meet in LDS (the V tiles are dead once every wave is past its loop)
  __syncthreads();
  {
    const float ls = pair_sum(lsum);
    float* orow = reinterpret_cast<float*>(smem) + ((long long)wave * kExtQ + r32) * OLD;
#pragma unroll
    for (int dt = 0; dt < DTN; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 v = {oacc[dt][4 * g], oacc[dt][4 * g + 1], oacc[dt][4 * g + 2], oacc[dt][4 * g + 3]};
        *reinterpret_cast<f32x4*>(orow + 32 * dt + 8 * g + 4 * hf) = v;
      }
    if (hf == 0) {
      ml_lds[wave][r32][0] = m;
      ml_lds[wave][r32][1] = ls;
    }
  }
  __syncthreads();
  // merge in wave order; thread = (query, HD / 8 output columns)
  {
    const int qq = threadIdx.x >> 3, part = threadIdx.x & 7;
    const int t = q0 + qq;
    if (t >= T) return;
    float M = -INFINITY;
#pragma unroll
    for (int w = 0; w < 4; ++w) M = fmaxf(M, ml_lds[w][qq][0]);
    float f[4], ls = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float mw = ml_lds[w][qq][0];
      f[w] = mw == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(mw - M);
      ls += f[w] * ml_lds[w][qq][1];
    }
    const bool lq = t < nlive;
    const float inv = lq ? 1.f / ls : 0.f;
    bf16* orow = obase + (long long)t * H * HD + part * (HD / 8);
#pragma unroll
    for (int c = 0; c < HD / 32; ++c) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(smem) +
                                                        ((long long)w * kExtQ + qq) * OLD + part * (HD / 8) + 4 * c);
        acc += f[w] * v;
      }
      bf16x4 r = {};
      if (lq) r = (bf16x4){(bf16)(acc[0] * inv), (bf16)(acc[1] * inv), (bf16)(acc[2] * inv), (bf16)(acc[3] * inv)};
      *reinterpret_cast<bf16x4*>(orow + 4 * c) = r;
    }
  }
}

// cache[b, len[b] + t, h, :] = the k / v parts of packed row b * T + t, for t < n[b] (n null: T)
// and len[b] + t < Tmax.  One 16-byte vector per thread step.
template <bool PAGED = false, typename... PG>
__global__ __launch_bounds__(256) void kv_append_chunk_k(const bf16* __restrict__ ksrc, const bf16* __restrict__ vsrc,
                                                         long long ld, bf16* __restrict__ kc, bf16* __restrict__ vc,
                                                         const int* __restrict__ len_ptr, int len_rows,
                                                         const int* __restrict__ n_ptr, int B, int T, int H, int HD,
                                                         int Tmax, PG... pgv) {
  const KvPageArgs<PAGED> pg = kv_page_args<PAGED>(pgv...);
  const int nv = H * HD / 8;               // 16-byte vectors per token row
  const long long per = (long long)B * T * nv;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < 2 * per;
       i += (long long)gridDim.x * blockDim.x) {
    const int isv = i >= per;
    const long long j = isv ? i - per : i;
    const int c = (int)(j % nv);
    const long long row = j / nv;          // b * T + t
    const int b = (int)(row / T), t = (int)(row % T);
    const int len = len_ptr[len_rows ? b : 0];
    KASSERT(len >= 0, "cache length %d of sequence %d", len, b);
    const int nb = n_ptr ? n_ptr[b] : T;
    if (len < 0 || t >= nb || len + t >= Tmax) continue;
    const bf16* src = (isv ? vsrc : ksrc) + row * ld + 8 * c;
    if constexpr (PAGED) {   // an entry that maps no page: the append is dropped
      bool mapped;
      const long long prow = kv_page_row(pg, b, len + t, mapped);
      if (mapped) *reinterpret_cast<u32x4*>((isv ? vc : kc) + prow * H * HD + 8 * c) = *reinterpret_cast<const u32x4*>(src);
    } else {
      bf16* dst = (isv ? vc : kc) + ((long long)b * Tmax + len + t) * H * HD + 8 * c;
      *reinterpret_cast<u32x4*>(dst) = *reinterpret_cast<const u32x4*>(src);
    }
  }
}

}  // namespace dpfs

using namespace dpfs;

// q: bf16 rows (B * T, >= H * HD) with row stride ldq (a multiple of 8); kc / vc: contiguous
// (B, Tmax, H, HD) caches that already hold the chunk's rows; len: 1 (len_rows 0) or B
// (len_rows 1) device int32, the cache length before the chunk; n: B device int32 or null (T
// for every row); o: (B * T, H * HD) contiguous.  HD is 32, 64 or 128.
extern "C" void dpfs_attn_extend(const void* q, long long ldq, const void* kc, const void* vc, const int* len,
                                 int len_rows, const int* n, void* o, int B, int T, int H, int HD, int Tmax,
                                 float scale, hipStream_t s) {
  const dim3 grid((T + kExtQ - 1) / kExtQ, B * H);
#define EXT_LAUNCH(HD_)                                                                                     \
  attn_extend_k<HD_><<<grid, 256, 0, s>>>((const bf16*)q, ldq, kc, vc, nullptr, nullptr, len, len_rows, n, \
                                          (bf16*)o, T, H, Tmax, scale)
  if (HD == 32) EXT_LAUNCH(32);
  else if (HD == 64) EXT_LAUNCH(64);
  else EXT_LAUNCH(128);
#undef EXT_LAUNCH
}

// The fp8-cache form: k8 / v8 contiguous (B, Tmax, H, HD) e4m3 codes that already hold the
// chunk's rows (dpfs_kv_append_chunk_q8), ks / vs contiguous (B, Tmax, H) fp32 scales.
extern "C" void dpfs_attn_extend_q8(const void* q, long long ldq, const void* k8, const void* v8, const float* ks,
                                    const float* vs, const int* len, int len_rows, const int* n, void* o, int B, int T,
                                    int H, int HD, int Tmax, float scale, hipStream_t s) {
  const dim3 grid((T + kExtQ - 1) / kExtQ, B * H);
#define EXT_LAUNCH(HD_)                                                                                         \
  attn_extend_k<HD_, true><<<grid, 256, 0, s>>>((const bf16*)q, ldq, k8, v8, ks, vs, len, len_rows, n, (bf16*)o, T, H, \
                                                Tmax, scale)
  if (HD == 32) EXT_LAUNCH(32);
  else if (HD == 64) EXT_LAUNCH(64);
  else EXT_LAUNCH(128);
#undef EXT_LAUNCH
}

// ksrc / vsrc: the k / v parts of the packed rows (B * T rows of stride ld); len, len_rows, n as
// in dpfs_attn_extend.
extern "C" void dpfs_kv_append_chunk(const void* ksrc, const void* vsrc, long long ld, void* kc, void* vc,
                                     const int* len, int len_rows, const int* n, int B, int T, int H, int HD,
                                     int Tmax, hipStream_t s) {
  const long long total = 2LL * B * T * (H * HD / 8);
  const int grid = (int)((total + 255) / 256 < 65535 ? (total + 255) / 256 : 65535);
  if (total > 0)
    kv_append_chunk_k<<<grid, 256, 0, s>>>((const bf16*)ksrc, (const bf16*)vsrc, ld, (bf16*)kc, (bf16*)vc, len,
                                           len_rows, n, B, T, H, HD, Tmax);
}

// ------------------------------------------------------------------------ paged KV cache --
// The layout is in kv_page.h: kp / vp pools (P, PS, H, HD) of bf16, or with ks / vs non-null of
// e4m3 codes with fp32 scale pools (P, PS, H); tbl (B, MP) device int32, PS = 1 << lg; len: B
// device int32 (a paged cache is per-row); Tmax: the logical capacity of a sequence,
// MP = ceil(Tmax / PS).  Grid and tiles are those of the contiguous form: the tiles are taken
// over the logical key index.
extern "C" void dpfs_attn_extend_paged(const void* q, long long ldq, const void* kp, const void* vp, const float* ks,
                                       const float* vs, const int* tbl, int MP, int P, int lg, const int* len,
                                       const int* n, void* o, int B, int T, int H, int HD, int Tmax, float scale,
                                       hipStream_t s) {
  const dim3 grid((T + kExtQ - 1) / kExtQ, B * H);
  const KvPageArgs<true> pg{tbl, MP, P, lg};
#define EXT_LAUNCH(HD_, Q8_)                                                                                      \
  attn_extend_k<HD_, Q8_, true><<<grid, 256, 0, s>>>((const bf16*)q, ldq, kp, vp, ks, vs, len, 1, n, (bf16*)o, T, H, \
                                                     Tmax, scale, pg)
  if (ks) {
    if (HD == 32) EXT_LAUNCH(32, true);
    else if (HD == 64) EXT_LAUNCH(64, true);
    else EXT_LAUNCH(128, true);
  } else {
    if (HD == 32) EXT_LAUNCH(32, false);
    else if (HD == 64) EXT_LAUNCH(64, false);
    else EXT_LAUNCH(128, false);
  }
#undef EXT_LAUNCH
}

// dpfs_kv_append_chunk into bf16 pools (the fp8 form is dpfs_kv_append_chunk_q8_paged, kv8.hip).
extern "C" void dpfs_kv_append_chunk_paged(const void* ksrc, const void* vsrc, long long ld, void* kp, void* vp,
                                           const int* tbl, int MP, int P, int lg, const int* len, const int* n, int B,
                                           int T, int H, int HD, int Tmax, hipStream_t s) {
  const long long total = 2LL * B * T * (H * HD / 8);
  const int grid = (int)((total + 255) / 256 < 65535 ? (total + 255) / 256 : 65535);
  if (total > 0)
    kv_append_chunk_k<true><<<grid, 256, 0, s>>>((const bf16*)ksrc, (const bf16*)vsrc, ld, (bf16*)kp, (bf16*)vp, len, 1,
                                                 n, B, T, H, HD, Tmax, KvPageArgs<true>{tbl, MP, P, lg});
}
