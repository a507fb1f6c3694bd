// The paged KV cache layout (gfx950), shared by the PAGED forms of the cache-addressing kernels
// (decode.hip, attn_extend.hip, kv8.hip).
//
//   * page size PS: a power of two, 16 <= PS <= 256, passed to the kernels as lg = log2(PS);
//   * per layer and side one pool (P, PS, H, hd): bf16, or e4m3 codes with fp32 scale pools
//     (P, PS, H) for the fp8 form (the row format of kv8.h, unchanged); hd is 32, 64 or 128;
//   * one block table for the whole model: tbl int32 (B, MP) on the device, MP = ceil(t_max / PS);
//     every layer's pool is indexed by the same page number;
//   * key t of sequence b lives in pool row tbl[b, t >> lg] * PS + (t & (PS - 1)); an entry that
//     maps nothing is -1;
//   * paged caches are always per-row: len[B], the ROWS forms of the kernels.
//
// Device safety ("safe for any table content"): P and MP are kernel arguments.  The kernels index
// the table only with t < t_max <= MP * PS, so the table read itself is in bounds.  A STORE whose
// entry is outside [0, P) is dropped, like an append to a full row.  A LOAD whose entry is outside
// [0, P) is redirected to page 0: the address stays inside the pool, that sequence's output is
// then unspecified, and no other sequence is affected.  Range checks proper (is every live key
// mapped?) are the host's; nothing here synchronises.
#pragma once

#include "common.h"

namespace dpfs {

// The page arguments of a kernel: nothing for the contiguous forms.
template <bool PAGED>
struct KvPageArgs {};

template <>
struct KvPageArgs<true> {
  const int* tbl;   // (B, MP) page numbers, -1 = unmapped
  int MP, P, lg;    // table columns, pool pages, log2(page size)
};

// A kernel with a PAGED form ends its parameter list with a pack `PG... pgv`: one
// KvPageArgs<true> when PAGED, no parameter at all otherwise (an empty struct would still take a
// kernel-argument slot and move the hidden arguments behind it), so the contiguous instantiations
// keep the parameter list, the argument offsets and the code they had.
template <bool PAGED, typename... PG>
__device__ __forceinline__ KvPageArgs<PAGED> kv_page_args(PG... pgv) {
  static_assert(sizeof...(PG) == (PAGED ? 1 : 0), "one KvPageArgs<true> iff PAGED");
  if constexpr (PAGED) return (pgv, ...);
  else return {};
}

// Pool row of key t (0 <= t < MP * PS) of sequence b; P * PS < 2^31 (checked by the bindings), so
// a row fits an int, and the callers widen it where they scale it to elements.  The row is always
// inside the pool (an entry outside [0, P) gives a row of page 0); `mapped` says whether the entry
// names a page: a load uses the row as it is, a store is made only when `mapped`.
__device__ __forceinline__ int kv_page_row(const KvPageArgs<true>& pg, int b, int t, bool& mapped) {
  const int e = pg.tbl[(long long)b * pg.MP + (t >> pg.lg)];
  mapped = (unsigned)e < (unsigned)pg.P;
  return ((mapped ? e : 0) << pg.lg) + (t & ((1 << pg.lg) - 1));
}

__device__ __forceinline__ int kv_page_row(const KvPageArgs<true>& pg, int b, int t) {
  bool mapped;
  return kv_page_row(pg, b, t, mapped);
}

}  // namespace dpfs
