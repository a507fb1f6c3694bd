// Quantising appends of the fp8 KV cache (gfx950; the row format is in kv8.h): the k / v parts
// of packed bf16 qkv rows become e4m3 codes (k8 / v8: (B, Tmax, H, HD) bytes) and one fp32 scale
// per cached (token, head) row (ks / vs: (B, Tmax, H)).
//
//   kv_append_chunk_q8_k  the quantising form of kv_append_chunk_k (attn_extend.hip): packed row
//                         (b, t) goes to cache row len[b] + t, for t < n[b] and len[b] + t < Tmax;
//                         nothing else is written, neither codes nor scales.  With T = 1 it is the
//                         un-fused single-token append.
//   rope_append_q8_k      the decode step's fused kernel: rope_append_k (decode.hip) with the
//                         rotated bf16 k row and the v row quantised on their way into the cache.
//
// A row is spread over a group of lanes (8 values per lane in the chunk kernel and for v, the 16
// values of 8 frequency pairs for a rotated k head); the row's amax comes from xor exchanges
// inside the group, so a group never straddles a wave, the k / v (or rotate / v) boundary or the
// end of the index space: every index space below is a whole number of groups, groups start at
// multiples of their size, and the sizes divide 64.  Rows that are not written still take part in
// the exchange (on zeros) so that no lane of a group leaves it early.
//
// Paged KV cache (PAGED = true; kv_page.h): k8 / v8 / ks / vs are pools and the written row is the
// one the block table gives (b, len[b] + t); an entry that maps no page drops the write.
#include "kv8.h"
#include "kv_page.h"
#include "../dpfs_api.h"

namespace dpfs {

template <int HD, bool PAGED = false, typename... PG>
__global__ __launch_bounds__(256) void kv_append_chunk_q8_k(const bf16* __restrict__ ksrc,
                                                            const bf16* __restrict__ vsrc, long long ld,
                                                            uint8_t* __restrict__ k8, uint8_t* __restrict__ v8,
                                                            float* __restrict__ ks, float* __restrict__ vs,
                                                            const int* __restrict__ len_ptr, int len_rows,
                                                            const int* __restrict__ n_ptr, int B, int T, int H,
                                                            int Tmax, PG... pgv) {
  const KvPageArgs<PAGED> pg = kv_page_args<PAGED>(pgv...);
  constexpr int G = HD / 8;                  // lanes per row, 8 values (16 bytes in, 8 out) each
  const long long per = (long long)B * T * H * G;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < 2 * per;
       i += (long long)gridDim.x * blockDim.x) {
    const int isv = i >= per;
    const long long j = isv ? i - per : i;
    const int c = (int)(j % G);
    const long long rh = j / G;              // (b * T + t) * H + h
    const int h = (int)(rh % H);
    const long long row = rh / H;            // b * T + t
    const int b = (int)(row / T), t = (int)(row % T);
    const int len = len_ptr[len_rows ? b : 0];
    KASSERT(len >= 0, "cache length %d of sequence %d", len, b);
    const int nb = n_ptr ? n_ptr[b] : T;
    const bool live = len >= 0 && t < nb && len + t < Tmax;
    bf16x8 x = {};
    if (live) x = *reinterpret_cast<const bf16x8*>((isv ? vsrc : ksrc) + row * ld + (long long)h * HD + 8 * c);
    const float scale = kv8_scale(kv8_group_max<G>(kv8_amax8(x, 0.f)));
    if constexpr (PAGED) {
      if (live) {   // an entry that maps no page: the append is dropped, codes and scale
        bool mapped;
        const long long crow = (long long)kv_page_row(pg, b, len + t, mapped) * H + h;
        if (mapped) {
          *reinterpret_cast<u32x2*>((isv ? v8 : k8) + crow * HD + 8 * c) = kv8_enc8(x, scale);
          if (c == 0) (isv ? vs : ks)[crow] = 1.f / scale;
        }
      }
    } else if (live) {
      const long long crow = ((long long)b * Tmax + len + t) * H + h;
      *reinterpret_cast<u32x2*>((isv ? v8 : k8) + crow * HD + 8 * c) = kv8_enc8(x, scale);
      if (c == 0) (isv ? vs : ks)[crow] = 1.f / scale;
    }
  }
}

// Same index space, arithmetic and bf16 rounding as rope_append_k (8 frequency pairs per thread
// for the q and k heads, then one 16-byte vector of v per thread); a rotated k head is the
// HD / 16 consecutive threads of its pairs.
template <int HD, bool ROWS, bool PAGED = false, typename... PG>
__global__ __launch_bounds__(256) void rope_append_q8_k(bf16* __restrict__ qkv, long long ld,
                                                        const int64_t* __restrict__ pos,
                                                        const float* __restrict__ tab, uint8_t* __restrict__ k8,
                                                        uint8_t* __restrict__ v8, float* __restrict__ ks,
                                                        float* __restrict__ vs, const int* __restrict__ len_ptr,
                                                        int B, int H, int Tmax, PG... pgv) {
  const KvPageArgs<PAGED> pg = kv_page_args<PAGED>(pgv...);
  static_assert(ROWS || !PAGED, "a paged cache is per-row");
  constexpr int h2 = HD / 2, q8 = h2 / 8, G = HD / 8;
  const int t0 = ROWS ? 0 : *len_ptr;
  const bool app0 = ROWS || (t0 >= 0 && t0 < Tmax);   // full cache: rotate, append nothing
  const int rot_per_b = 2 * H * q8;
  const int nrot = B * rot_per_b;
  const int vpr = H * G;                   // 16-byte v vectors per sequence
  const int total = nrot + B * vpr;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    if (i < nrot) {
      const int b = i / rot_per_b, r = i - b * rot_per_b;
      const int head = r / q8, f0 = (r - head * q8) * 8;
      const int t = ROWS ? len_ptr[b] : t0;
      KASSERT(!ROWS || t >= 0, "cache length %d of sequence %d", t, b);
      const bool app = ROWS ? (t >= 0 && t < Tmax) : app0;
      bf16* base = qkv + (long long)b * ld + head * HD;
      KASSERT(pos[b] >= 0, "decode position %lld of sequence %d", (long long)pos[b], b);
      const float* tr = tab + pos[b] * (long long)HD;
      const bf16x8 xa = *reinterpret_cast<const bf16x8*>(base + f0);
      const bf16x8 xb = *reinterpret_cast<const bf16x8*>(base + h2 + f0);
      bf16x8 oa, ob;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float c = tr[f0 + j], sn = tr[h2 + f0 + j];
        const float x1 = (float)xa[j], x2 = (float)xb[j];
        oa[j] = (bf16)(x1 * c - x2 * sn);
        ob[j] = (bf16)(x2 * c + x1 * sn);
      }
      *reinterpret_cast<bf16x8*>(base + f0) = oa;
      *reinterpret_cast<bf16x8*>(base + h2 + f0) = ob;
      // the head's amax over its q8 threads (the q heads take part: their groups are whole too)
      const float scale = kv8_scale(kv8_group_max<q8>(kv8_amax8(ob, kv8_amax8(oa, 0.f))));
      if constexpr (PAGED) {
        if (head >= H && app) {   // an entry that maps no page: the append is dropped
          bool mapped;
          const long long crow = (long long)kv_page_row(pg, b, t, mapped) * H + (head - H);
          uint8_t* dst = k8 + crow * HD;
          if (mapped) {
            *reinterpret_cast<u32x2*>(dst + f0) = kv8_enc8(oa, scale);
            *reinterpret_cast<u32x2*>(dst + h2 + f0) = kv8_enc8(ob, scale);
            if (f0 == 0) ks[crow] = 1.f / scale;
          }
        }
      } else if (head >= H && app) {
        const long long crow = ((long long)b * Tmax + t) * H + (head - H);
        uint8_t* dst = k8 + crow * HD;
        *reinterpret_cast<u32x2*>(dst + f0) = kv8_enc8(oa, scale);
        *reinterpret_cast<u32x2*>(dst + h2 + f0) = kv8_enc8(ob, scale);
        if (f0 == 0) ks[crow] = 1.f / scale;
      }
    } else if (app0) {
      const int j = i - nrot, b = j / vpr, r = j - b * vpr;
      const int h = r / G, c = r - h * G;
      const int t = ROWS ? len_ptr[b] : t0;
      const bool app = !ROWS || (t >= 0 && t < Tmax);   // ROWS: this row may be full
      const bf16x8 x = *reinterpret_cast<const bf16x8*>(qkv + (long long)b * ld + 2 * H * HD + h * HD + 8 * c);
      const float scale = kv8_scale(kv8_group_max<G>(kv8_amax8(x, 0.f)));
      if constexpr (PAGED) {
        if (app) {
          bool mapped;
          const long long crow = (long long)kv_page_row(pg, b, t, mapped) * H + h;
          if (mapped) {
            *reinterpret_cast<u32x2*>(v8 + crow * HD + 8 * c) = kv8_enc8(x, scale);
            if (c == 0) vs[crow] = 1.f / scale;
          }
        }
      } else if (app) {
        const long long crow = ((long long)b * Tmax + t) * H + h;
        *reinterpret_cast<u32x2*>(v8 + crow * HD + 8 * c) = kv8_enc8(x, scale);
        if (c == 0) vs[crow] = 1.f / scale;
      }
    }
  }
}

}  // namespace dpfs

using namespace dpfs;

// ksrc / vsrc: the k / v parts of the packed bf16 rows (B * T rows of stride ld, 16-byte aligned);
// k8 / v8: contiguous (B, Tmax, H, HD) e4m3 codes; ks / vs: contiguous (B, Tmax, H) fp32; len,
// len_rows, n as in dpfs_kv_append_chunk.  HD is 32, 64 or 128.
extern "C" void dpfs_kv_append_chunk_q8(const void* ksrc, const void* vsrc, long long ld, void* k8, void* v8,
                                        float* ks, float* vs, const int* len, int len_rows, const int* n, int B,
                                        int T, int H, int HD, int Tmax, hipStream_t s) {
  const long long total = 2LL * B * T * H * (HD / 8);
  const int grid = (int)((total + 255) / 256 < 65535 ? (total + 255) / 256 : 65535);
  if (total <= 0) return;
#define Q8_LAUNCH(HD_)                                                                                           \
  kv_append_chunk_q8_k<HD_><<<grid, 256, 0, s>>>((const bf16*)ksrc, (const bf16*)vsrc, ld, (uint8_t*)k8, (uint8_t*)v8, \
                                                 ks, vs, len, len_rows, n, B, T, H, Tmax)
  if (HD == 32) Q8_LAUNCH(32);
  else if (HD == 64) Q8_LAUNCH(64);
  else Q8_LAUNCH(128);
#undef Q8_LAUNCH
}

// qkv: B packed bf16 rows [3 * H * HD] of stride ld, rotated in place; caches as above; len: one
// device int32 (len_rows 0) or B of them (len_rows 1).  HD is 32, 64 or 128.
extern "C" void dpfs_rope_append_q8(void* qkv, long long ld, const int64_t* pos, const float* tab, void* k8, void* v8,
                                    float* ks, float* vs, const int* len, int len_rows, int B, int H, int HD,
                                    int Tmax, hipStream_t s) {
  const int total = B * 2 * H * (HD / 16) + B * H * (HD / 8);
  const int grid = (total + 255) / 256;
#define Q8_LAUNCH(HD_, ROWS_)                                                                                  \
  rope_append_q8_k<HD_, ROWS_><<<grid, 256, 0, s>>>((bf16*)qkv, ld, pos, tab, (uint8_t*)k8, (uint8_t*)v8, ks, vs, len, \
                                                    B, H, Tmax)
  if (len_rows) {
    if (HD == 32) Q8_LAUNCH(32, true);
    else if (HD == 64) Q8_LAUNCH(64, true);
    else Q8_LAUNCH(128, true);
  } else {
    if (HD == 32) Q8_LAUNCH(32, false);
    else if (HD == 64) Q8_LAUNCH(64, false);
    else Q8_LAUNCH(128, false);
  }
#undef Q8_LAUNCH
}

// ------------------------------------------------------------------------ paged KV cache --
// The quantising appends into fp8 pools (the layout is in kv_page.h): kp / vp (P, PS, H, HD) e4m3
// codes, ks / vs (P, PS, H) fp32 scales, tbl (B, MP) device int32, PS = 1 << lg; len: B device
// int32 (a paged cache is per-row); Tmax: the logical capacity of a sequence.
extern "C" void dpfs_kv_append_chunk_q8_paged(const void* ksrc, const void* vsrc, long long ld, void* kp, void* vp,
                                              float* ks, float* vs, const int* tbl, int MP, int P, int lg,
                                              const int* len, const int* n, int B, int T, int H, int HD, int Tmax,
                                              hipStream_t s) {
  const long long total = 2LL * B * T * H * (HD / 8);
  const int grid = (int)((total + 255) / 256 < 65535 ? (total + 255) / 256 : 65535);
  if (total <= 0) return;
  const KvPageArgs<true> pg{tbl, MP, P, lg};
#define Q8_LAUNCH(HD_)                                                                                          \
  kv_append_chunk_q8_k<HD_, true><<<grid, 256, 0, s>>>((const bf16*)ksrc, (const bf16*)vsrc, ld, (uint8_t*)kp, \
                                                       (uint8_t*)vp, ks, vs, len, 1, n, B, T, H, Tmax, pg)
  if (HD == 32) Q8_LAUNCH(32);
  else if (HD == 64) Q8_LAUNCH(64);
  else Q8_LAUNCH(128);
#undef Q8_LAUNCH
}

extern "C" void dpfs_rope_append_q8_paged(void* qkv, long long ld, const int64_t* pos, const float* tab, void* kp,
                                          void* vp, float* ks, float* vs, const int* tbl, int MP, int P, int lg,
                                          const int* len, int B, int H, int HD, int Tmax, hipStream_t s) {
  const int total = B * 2 * H * (HD / 16) + B * H * (HD / 8);
  const int grid = (total + 255) / 256;
  const KvPageArgs<true> pg{tbl, MP, P, lg};
#define Q8_LAUNCH(HD_)                                                                                            \
  rope_append_q8_k<HD_, true, true><<<grid, 256, 0, s>>>((bf16*)qkv, ld, pos, tab, (uint8_t*)kp, (uint8_t*)vp, ks, vs, \
                                                         len, B, H, Tmax, pg)
  if (HD == 32) Q8_LAUNCH(32);
  else if (HD == 64) Q8_LAUNCH(64);
  else Q8_LAUNCH(128);
#undef Q8_LAUNCH
}
