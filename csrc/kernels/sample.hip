// Temperature / top-k / top-p token sampling for the KV-cached decode step (gfx950).
//
// One launch per decode step, one workgroup per sequence row, no host state: the launch is
// captured in the decode graph like every other kernel of the step.  Per row:
//
//   z_i = fp32(logit_i) * fp32(1/T) (one fp32 multiply), w_i = exp(z_i - max z);
//   top-k : keep {logit >= v_k}, v_k the k-th largest logit (ties at v_k all kept);
//   top-p : of the survivors keep {logit >= t*}, t* the largest logit value present whose
//           upper set holds a share >= p of the survivors' mass (ties kept whole);
//   draw  : C_j = kept mass at indices <= j in vocabulary order, M = C_last; the token is
//           the smallest kept j with C_j > u M, u = (x0 >> 8) 2^-24 of Philox4x32-10 with key
//           (seed lo, seed hi) and counter (pos lo, pos hi, row, 0) -- a pure function of
//           (seed, row, position), so eager steps, graph replays and every TP rank agree.
//
// Per-row settings (ROWS = true): workgroup b reads (1/T, top_k, top_p, seed, row id) from five
// device arrays instead of the launch arguments, so a batch mixes requests and a captured
// launch serves every setting; the row id takes the place of b in the Philox counter (a request
// keyed on (seed, position) alone draws the same in any slot).  1/T == 0 marks a greedy row:
// no radix select, the threshold is the row maximum and u = 0, so the draw below returns the
// smallest index of the maximum (every maximum weighs 2^40).  The settings are uniform within
// the workgroup: control flow stays wave-uniform.  Any array content is safe: the values only
// steer comparisons and arithmetic, every loop is bounded by the row, and ids[b] is preset to 0
// (settings out of range, which the host rejects, may leave no crossing to write it).
//
// Selection never sorts: a logit's raw bits map to an order-preserving integer key (the order
// is unchanged by the positive scale 1/T) and both thresholds are found by an 8-bit radix
// descent over that key, most significant digit first (2 rounds for bf16, 4 for fp32) --
// top-k on per-digit counts, top-p on per-digit masses of the survivors (a weighted radix
// select).  Masses are 2^40 fixed point in 64-bit integers (the row maximum weighs exactly
// 2^40, so V 2^40 fits) and every accumulation is an integer LDS atomic or an integer wave
// scan: sums do not depend on arrival order, the outputs are bit-reproducible.
//
// Layout: the row is cut into one contiguous range of 16-byte vectors per wave (vector
// wave * WV + it * 64 + lane), so the final draw is an index-ordered prefix scan: per-wave
// kept totals go through LDS once, and only the wave whose range holds the crossing
// rescans it.  The row is re-read from L2 by every pass (a 50,304-column bf16 row is
// 100 KB); it is never staged in LDS.
#include "common.h"
#include "../dpfs_api.h"

namespace dpfs {
namespace {

constexpr int kSampleMaxWaves = 16;
constexpr float kFix = 1099511627776.f;   // 2^40

typedef unsigned long long u64;

template <typename T> struct KeyBits;
template <> struct KeyBits<bf16> { static constexpr int BITS = 16; };
template <> struct KeyBits<float> { static constexpr int BITS = 32; };

// raw storage bits -> unsigned key with the order of the values (-0 == +0)
template <typename T>
__device__ __forceinline__ uint32_t raw_to_key(uint32_t r) {
  constexpr int BITS = KeyBits<T>::BITS;
  constexpr uint32_t MASK = BITS == 32 ? 0xFFFFFFFFu : 0xFFFFu, SIGN = 1u << (BITS - 1);
  if ((r & (MASK >> 1)) == 0) r = 0;
  return (r & SIGN) ? (~r & MASK) : (r | SIGN);
}

template <typename T>
__device__ __forceinline__ float key_to_float(uint32_t k) {
  constexpr int BITS = KeyBits<T>::BITS;
  constexpr uint32_t MASK = BITS == 32 ? 0xFFFFFFFFu : 0xFFFFu, SIGN = 1u << (BITS - 1);
  const uint32_t r = (k & SIGN) ? (k & ~SIGN) : (~k & MASK);
  return __uint_as_float(BITS == 32 ? r : r << 16);
}

// 2^40 fixed-point weight exp(z - zmax); the product is rounded to fp32 before the subtract
// (no fused multiply-add), so the row maximum weighs exactly 2^40.
__device__ __forceinline__ u64 weight_fx(float val, float inv_t, float zmax) {
#pragma clang fp contract(off)
  const float z = val * inv_t;
  const float w = __expf(z - zmax);
  return (u64)(w * kFix);
}

// One row as seen by one lane: vectors [wave * wv, (wave + 1) * wv) of the nv the row has.
template <typename T>
struct Row {
  static constexpr int N = Vec<T>::N;
  const T* p;
  int vocab, nv, wv, wave, lane;
  bool vec_ok;

  __device__ __forceinline__ int iters() const { return wv >> 6; }
  __device__ __forceinline__ int vec_at(int it) const { return wave * wv + it * 64 + lane; }

  // raw bits of the N elements of vector v (v < nv); elements at index >= vocab are not valid
  __device__ __forceinline__ void load(int v, uint32_t (&raw)[N]) const {
    KASSERT(v >= 0 && v < nv, "vector %d of %d", v, nv);
    if (vec_ok) {
      const u32x4 x = *reinterpret_cast<const u32x4*>(p + (long long)v * N);
      if constexpr (N == 8) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          raw[2 * j] = x[j] & 0xFFFFu;
          raw[2 * j + 1] = x[j] >> 16;
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) raw[j] = x[j];
      }
    } else {
#pragma unroll
      for (int j = 0; j < N; ++j) {
        const int i = v * N + j;
        uint32_t r = 0;
        if (i < vocab) {
          if constexpr (N == 8) r = reinterpret_cast<const uint16_t*>(p)[i];
          else r = reinterpret_cast<const uint32_t*>(p)[i];
        }
        raw[j] = r;
      }
    }
  }

  // f(index, key, value) for every valid element of this lane
  template <typename F>
  __device__ __forceinline__ void for_each(F f) const {
    for (int it = 0; it < iters(); ++it) {
      const int v = vec_at(it);
      if (v >= nv) break;
      uint32_t raw[N];
      load(v, raw);
#pragma unroll
      for (int j = 0; j < N; ++j) {
        const int i = v * N + j;
        if (i < vocab) {
          const uint32_t k = raw_to_key<T>(raw[j]);
          f(i, k, key_to_float<T>(k));
        }
      }
    }
  }
};

__device__ __forceinline__ u64 shfl_u64(u64 v, int src) { return __shfl(v, src, 64); }

struct Shared {
  u64 hist[256];
  u64 wave_tot[kSampleMaxWaves];
  u64 above, target;
  uint32_t wave_a[kSampleMaxWaves], wave_b[kSampleMaxWaves];
  uint32_t prefix;
};

// Radix descent for the largest key t with  (count | mass){key >= t} >= target, over the
// elements with key >= floor_key.  MASS = false: counts, target = k.  MASS = true: 2^40
// fixed-point masses, target = ceil(p * their total).  Every thread of the block calls it.
// ROWS is not used in the body; it only names the calling kernel.  Keep it: with it every
// instantiation has one caller, and the uniform kernel compiles to the instructions it had
// before the per-row kernel existed.  Shared between the two kernels, the function is inlined
// with other register and scheduling choices, and the uniform kernel's code changes silently
// (diff the disassembly of sample_logits_k<T, false> against the previous build to check).
template <typename T, bool MASS, bool ROWS>
__device__ uint32_t radix_select(const Row<T>& row, Shared& sh, uint32_t floor_key, u64 k_target, double p,
                                 float inv_t, float zmax) {
  constexpr int BITS = KeyBits<T>::BITS, ND = BITS / 8;
  uint32_t prefix = 0;
  for (int r = 0; r < ND; ++r) {
    const int shift = BITS - 8 * (r + 1);
    for (int i = threadIdx.x; i < 256; i += blockDim.x) sh.hist[i] = 0;
    __syncthreads();
    row.for_each([&](int, uint32_t key, float val) {
      if (key < floor_key) return;
      if (r > 0 && (key >> (shift + 8)) != prefix) return;
      const int d = (key >> shift) & 255;
      if constexpr (MASS) {
        const u64 w = weight_fx(val, inv_t, zmax);
        if (w) atomicAdd(&sh.hist[d], w);
      } else {
        atomicAdd(reinterpret_cast<unsigned int*>(&sh.hist[d]), 1u);   // low word: counts < 2^32
      }
    });
    __syncthreads();
    if (row.wave == 0) {
      // lane l owns digits 4 l .. 4 l + 3; suf = sum over the digits of lanes >= l
      const int l = row.lane;
      u64 h[4], s = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        h[j] = sh.hist[4 * l + j];
        s += h[j];
      }
      u64 suf = s;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const u64 t = __shfl_down(suf, d, 64);
        if (l + d < 64) suf += t;
      }
      u64 above = r == 0 ? 0 : sh.above, target = r == 0 ? k_target : sh.target;
      if (MASS && r == 0) {
        const u64 total = shfl_u64(suf, 0);
        const double t = ceil(p * (double)total);
        target = t >= (double)total ? total : (u64)t;
        if (target < 1) target = 1;
      }
      unsigned long long m = __ballot(above + suf >= target);
      if (m == 0) m = 1;   // cannot happen: the digits of this prefix hold the crossing
      const int src = 63 - __clzll(m);
      if (l == src) {
        u64 acc = above + suf - s;
        int d = 0;
#pragma unroll
        for (int j = 3; j >= 0; --j) {
          if (acc + h[j] >= target) {
            d = j;
            break;
          }
          if (j > 0) acc += h[j];
        }
        sh.prefix = (prefix << 8) | (uint32_t)(4 * l + d);
        sh.above = acc;
        sh.target = target;
      }
    }
    __syncthreads();
    prefix = sh.prefix;
  }
  return prefix;
}

// Philox4x32-10 (Salmon et al., Random123), word 0 of the output block.
__device__ __forceinline__ uint32_t philox4x32_10_x0(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                     uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0;
    c1 = lo1;
    c2 = n2;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c0;
}

// ROWS = false: the settings are the launch arguments inv_t .. seed and the *_r arrays are not
// read (trailing arguments, so the uniform kernel's code is what it was without them).
// ROWS = true: workgroup b takes them from inv_t_r[b] .. rid_r[b].
template <typename T, bool ROWS>
__global__ __launch_bounds__(1024) void sample_logits_k(const T* __restrict__ logits, long long ld, int vocab,
                                                        bool vec_ok, float inv_t, int top_k, double top_p,
                                                        u64 seed, const int64_t* __restrict__ pos,
                                                        const float* __restrict__ u_in, int64_t* __restrict__ ids,
                                                        int* __restrict__ kept, float* __restrict__ thresh,
                                                        float* __restrict__ u_out, const float* __restrict__ inv_t_r,
                                                        const int* __restrict__ top_k_r,
                                                        const double* __restrict__ top_p_r,
                                                        const int64_t* __restrict__ seed_r,
                                                        const int* __restrict__ rid_r) {
  constexpr int N = Vec<T>::N;
  __shared__ Shared sh;
  const int b = blockIdx.x, nw = blockDim.x >> 6;
  uint32_t rid = (uint32_t)b;
  if constexpr (ROWS) {
    inv_t = inv_t_r[b];
    top_k = top_k_r[b];
    top_p = top_p_r[b];
    seed = (u64)seed_r[b];
    rid = (uint32_t)rid_r[b];
    if (threadIdx.x == 0) ids[b] = 0;   // ordered before the draw's store by the barriers below
  }
  const bool greedy = ROWS && inv_t == 0.f;
  Row<T> row;
  row.p = logits + (long long)b * ld;
  row.vocab = vocab;
  row.nv = (vocab + N - 1) / N;
  row.wv = ((row.nv + nw - 1) / nw + 63) & ~63;
  row.wave = threadIdx.x >> 6;
  row.lane = lane_id();
  row.vec_ok = vec_ok;

  // row maximum / minimum key
  uint32_t kmax = 0, kmin = 0xFFFFFFFFu;
  row.for_each([&](int, uint32_t key, float) {
    kmax = max(kmax, key);
    kmin = min(kmin, key);
  });
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    kmax = max(kmax, (uint32_t)__shfl_xor(kmax, o, 64));
    kmin = min(kmin, (uint32_t)__shfl_xor(kmin, o, 64));
  }
  if (row.lane == 0) {
    sh.wave_a[row.wave] = kmax;
    sh.wave_b[row.wave] = kmin;
  }
  __syncthreads();
  for (int w = 0; w < nw; ++w) {
    kmax = max(kmax, sh.wave_a[w]);
    kmin = min(kmin, sh.wave_b[w]);
  }
  const float zmax = key_to_float<T>(kmax) * inv_t;

  uint32_t thr = kmin;
  if (greedy) {
    thr = kmax;
  } else {
    if (top_k > 0 && top_k < vocab) thr = radix_select<T, false, ROWS>(row, sh, 0u, (u64)top_k, 1.0, inv_t, zmax);
    if (top_p < 1.0) thr = radix_select<T, true, ROWS>(row, sh, thr, 0, top_p, inv_t, zmax);
  }

  // kept mass and count per wave, in index order
  u64 tot = 0;
  uint32_t cnt = 0;
  row.for_each([&](int, uint32_t key, float val) {
    if (key >= thr) {
      tot += weight_fx(val, inv_t, zmax);
      ++cnt;
    }
  });
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    tot += (u64)__shfl_xor(tot, o, 64);
    cnt += (uint32_t)__shfl_xor(cnt, o, 64);
  }
  __syncthreads();   // wave_a / wave_b of the max pass have been read
  if (row.lane == 0) {
    sh.wave_tot[row.wave] = tot;
    sh.wave_a[row.wave] = cnt;
  }
  __syncthreads();
  u64 M = 0, base = 0;
  uint32_t nkept = 0;
  for (int w = 0; w < nw; ++w) {
    if (w < row.wave) base += sh.wave_tot[w];
    M += sh.wave_tot[w];
    nkept += sh.wave_a[w];
  }

  float u;
  if (greedy) {
    u = 0.f;   // need = 1: the first index of the maximum
  } else if (u_in != nullptr) {
    u = u_in[b];
  } else {
    const u64 ps = (u64)pos[b];
    const uint32_t x0 = philox4x32_10_x0((uint32_t)ps, (uint32_t)(ps >> 32), rid, 0u, (uint32_t)seed,
                                         (uint32_t)(seed >> 32));
    u = (float)(x0 >> 8) * 5.9604644775390625e-8f;   // 2^-24
  }
  // the token is the first kept index whose inclusive mass reaches floor(u M) + 1
  const double um = (double)u * (double)M;
  u64 need = um <= 0.0 ? 0 : (u64)um;
  if (need >= M) need = M - 1;
  need += 1;
  if (threadIdx.x == 0) {
    kept[b] = (int)nkept;
    thresh[b] = key_to_float<T>(thr);
    u_out[b] = u;
  }
  if (!(base < need && need <= base + tot)) return;   // one wave owns the crossing
  u64 running = base;
  for (int it = 0; it < row.iters(); ++it) {
    const int v = row.vec_at(it);
    u64 m[N], s = 0;
#pragma unroll
    for (int j = 0; j < N; ++j) m[j] = 0;
    if (v < row.nv) {
      uint32_t raw[N];
      row.load(v, raw);
#pragma unroll
      for (int j = 0; j < N; ++j) {
        const uint32_t key = raw_to_key<T>(raw[j]);
        if (v * N + j < vocab && key >= thr) m[j] = weight_fx(key_to_float<T>(key), inv_t, zmax);
        s += m[j];
      }
    }
    u64 incl = s;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const u64 t = __shfl_up(incl, d, 64);
      if (row.lane >= d) incl += t;
    }
    const unsigned long long hit = __ballot(running + incl >= need);
    if (hit) {
      if (row.lane == __ffsll(hit) - 1) {
        u64 acc = running + incl - s;
        int id = -1;
#pragma unroll
        for (int j = 0; j < N; ++j) {
          acc += m[j];
          if (id < 0 && acc >= need) id = v * N + j;
        }
        KASSERT(id >= 0 && id < vocab, "id %d, vocab %d", id, vocab);
        ids[b] = id;
      }
      return;
    }
    running += shfl_u64(incl, 63);
  }
}

}  // namespace
}  // namespace dpfs

using namespace dpfs;

// threads of a workgroup: one per 16-byte vector of the row, whole waves, at most 16 of them
static int sample_threads(int dtype, int vocab) {
  const int n = dtype == kBF16 ? 8 : 4;
  const int nv = (vocab + n - 1) / n;
  const int nt = (nv + 63) & ~63;
  return nt < 64 ? 64 : (nt > 64 * kSampleMaxWaves ? 64 * kSampleMaxWaves : nt);
}

// logits [B, >= vocab] (dtype kBF16 / kF32, unit column stride, row stride ld elements);
// vec_ok: rows are 16-byte aligned and padded to whole 16-byte vectors past vocab.
extern "C" void dpfs_sample_logits(const void* logits, int dtype, long long ld, int B, int vocab, int vec_ok,
                                   float inv_t, int top_k, double top_p, unsigned long long seed, const int64_t* pos,
                                   const float* u_in, int64_t* ids, int* kept, float* thresh, float* u_out,
                                   hipStream_t s) {
  if (B <= 0) return;
  const int nt = sample_threads(dtype, vocab);
  if (dtype == kBF16)
    sample_logits_k<bf16, false><<<B, nt, 0, s>>>((const bf16*)logits, ld, vocab, vec_ok != 0, inv_t, top_k, top_p,
                                                  seed, pos, u_in, ids, kept, thresh, u_out, nullptr, nullptr, nullptr,
                                                  nullptr, nullptr);
  else
    sample_logits_k<float, false><<<B, nt, 0, s>>>((const float*)logits, ld, vocab, vec_ok != 0, inv_t, top_k, top_p,
                                                   seed, pos, u_in, ids, kept, thresh, u_out, nullptr, nullptr,
                                                   nullptr, nullptr, nullptr);
  LAUNCH_CHECK();
}

// The per-row form: inv_t (fp32; 0 marks a greedy row), top_k (int32; <= 0 or >= vocab: off),
// top_p (fp64; >= 1: off), seed (int64, the Philox key) and rid (int32, counter word 2) hold
// B values each in device memory.
extern "C" void dpfs_sample_logits_rows(const void* logits, int dtype, long long ld, int B, int vocab, int vec_ok,
                                        const float* inv_t, const int* top_k, const double* top_p,
                                        const int64_t* seed, const int* rid, const int64_t* pos, const float* u_in,
                                        int64_t* ids, int* kept, float* thresh, float* u_out, hipStream_t s) {
  if (B <= 0) return;
  const int nt = sample_threads(dtype, vocab);
  if (dtype == kBF16)   // (the scalar settings are not read)
    sample_logits_k<bf16, true><<<B, nt, 0, s>>>((const bf16*)logits, ld, vocab, vec_ok != 0, 0.f, 0, 1.0, 0ull, pos,
                                                 u_in, ids, kept, thresh, u_out, inv_t, top_k, top_p, seed, rid);
  else
    sample_logits_k<float, true><<<B, nt, 0, s>>>((const float*)logits, ld, vocab, vec_ok != 0, 0.f, 0, 1.0, 0ull, pos,
                                                  u_in, ids, kept, thresh, u_out, inv_t, top_k, top_p, seed, rid);
  LAUNCH_CHECK();
}
