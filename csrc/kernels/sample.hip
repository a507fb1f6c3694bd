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
// Penalties and log-probabilities (sample_logits_pen_k, below): the per-row kernel on logits
// penalised by a device-resident token history (repetition / presence / frequency), which the
// launch itself updates with the id it draws, plus the id's log-probability under the raw softmax
// and under the distribution drawn from.  It has a row type and a kernel of its own, so the two
// forms above compile to the instructions they had before it existed.
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

// The penalised logit of one column (the PEN form; ops/reference.py:sample_logits_pen is the
// contract): h is the column's history word, bit 31 = "occurs in the prompt", bits 0..30 = c, the
// draws of this id so far.  Repetition over prompt and output, frequency and presence over the
// output only; every operation is one rounded fp32 operation (no fused multiply-add).
//
// The pragma alone does not give that: this file is built with -ffp-contract=fast, under which
// the backend fuses a multiply into the subtract that consumes it whatever the source says
// (weight_fx above is compiled to one v_fma_f32 in every kernel of this file, the same one in
// each, which is what keeps the forms bit-identical to one another).  So both products pass
// through rounded(): an identity DPP move (quad_perm [0,1,2,3], all rows and banks), which the
// instruction selector cannot look through.  It costs nothing: the move folds into the DPP form
// of the consuming subtract, after selection, when the multiply is already an instruction of
// its own (v_mul_f32, then v_sub*_f32; tests/test_sampling_penalties_gpu.py reads every
// penalised value back and compares it with the oracle's exactly).
__device__ __forceinline__ float rounded(float v) {
  return __uint_as_float((uint32_t)__builtin_amdgcn_update_dpp(0, (int)__float_as_uint(v), 0xE4, 0xF, 0xF, true));
}

__device__ __forceinline__ float penalise(float x, int h, float rep, float inv_rep, float pres, float freq) {
#pragma clang fp contract(off)
  const int c = h & 0x7FFFFFFF;
  if (h != 0) x = rounded(x > 0.f ? x * inv_rep : x * rep);
  x = x - rounded(freq * (float)c);
  if (c > 0) x = x - pres;
  return x;
}

// One row of the PEN form as seen by one lane: the layout of Row<T> (vectors of N stored logits),
// each logit with its history word.  The keys are those of the penalised fp32 value whatever T
// is: a penalised bf16 logit is no bf16 value any more.  A row of its own, not a mode of Row<T>:
// the two kernels on stored logits keep the loader, and so the code, they had.
template <typename T>
struct PenRow {
  static constexpr int N = Vec<T>::N;
  const T* p;
  const int* h;
  float rep, inv_rep, pres, freq;
  int vocab, nv, wv, wave, lane;
  bool vec_ok, hvec_ok;

  __device__ __forceinline__ int iters() const { return wv >> 6; }
  __device__ __forceinline__ int vec_at(int it) const { return wave * wv + it * 64 + lane; }

  // the N logits (fp32) and history words of vector v (v < nv); elements at index >= vocab are
  // not valid.  16-byte loads where the row allows them (logits and history independently).
  __device__ __forceinline__ void load(int v, float (&lg)[N], int (&hw)[N]) const {
    KASSERT(v >= 0 && v < nv, "vector %d of %d", v, nv);
    if (vec_ok) {
      const u32x4 x = *reinterpret_cast<const u32x4*>(p + (long long)v * N);
      if constexpr (N == 8) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          lg[2 * j] = __uint_as_float(x[j] << 16);
          lg[2 * j + 1] = __uint_as_float(x[j] & 0xFFFF0000u);
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) lg[j] = __uint_as_float(x[j]);
      }
    } else {
#pragma unroll
      for (int j = 0; j < N; ++j) {
        const int i = v * N + j;
        uint32_t r = 0;
        if (i < vocab) {
          if constexpr (N == 8) r = (uint32_t)reinterpret_cast<const uint16_t*>(p)[i] << 16;
          else r = reinterpret_cast<const uint32_t*>(p)[i];
        }
        lg[j] = __uint_as_float(r);
      }
    }
    if (hvec_ok) {
#pragma unroll
      for (int q = 0; q < N / 4; ++q) {
        const u32x4 x = *reinterpret_cast<const u32x4*>(h + (long long)v * N + 4 * q);
#pragma unroll
        for (int j = 0; j < 4; ++j) hw[4 * q + j] = (int)x[j];
      }
    } else {
#pragma unroll
      for (int j = 0; j < N; ++j) {
        const int i = v * N + j;
        hw[j] = i < vocab ? h[i] : 0;
      }
    }
  }

  __device__ __forceinline__ float pen(float lg, int hw) const { return penalise(lg, hw, rep, inv_rep, pres, freq); }

  // f(index, key, value, raw logit) for every valid element of this lane; key and value are
  // those of the penalised logit
  template <typename F>
  __device__ __forceinline__ void for_each(F f) const {
    for (int it = 0; it < iters(); ++it) {
      const int v = vec_at(it);
      if (v >= nv) break;
      float lg[N];
      int hw[N];
      load(v, lg, hw);
#pragma unroll
      for (int j = 0; j < N; ++j) {
        const int i = v * N + j;
        if (i < vocab) {
          const uint32_t k = raw_to_key<float>(__float_as_uint(pen(lg[j], hw[j])));
          f(i, k, key_to_float<float>(k), lg[j]);
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
// RowT is the row the caller scans, T its key type: Row<T> for the two kernels on stored logits,
// PenRow<.> with fp32 keys for the penalised form (its for_each passes the raw logit as a
// fourth argument, which the descent does not use).
template <typename T, bool MASS, bool ROWS, typename RowT = Row<T>>
__device__ uint32_t radix_select(const RowT& row, Shared& sh, uint32_t floor_key, u64 k_target, double p,
                                 float inv_t, float zmax) {
  constexpr int BITS = KeyBits<T>::BITS, ND = BITS / 8;
  uint32_t prefix = 0;
  for (int r = 0; r < ND; ++r) {
    const int shift = BITS - 8 * (r + 1);
    for (int i = threadIdx.x; i < 256; i += blockDim.x) sh.hist[i] = 0;
    __syncthreads();
    row.for_each([&](int, uint32_t key, float val, auto...) {
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
//
// sample_logits_pen_k below repeats this body (max pass, thresholds, mass pass, the uniform and
// `need`, the crossing scan) on its own row type.  The copy is deliberate: this kernel's code
// object stays what it was.  A change to the draw, the tie rules or the safety presets here has
// to be made there too; the bit-for-bit tests between the two forms fail if only one moves.
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

struct SharedPen {
  u64 wave_s1[kSampleMaxWaves];
  uint32_t wave_c[kSampleMaxWaves];
};

// The PEN form: the per-row kernel above on penalised logits, with the history of every row as
// device state and two log-probabilities per row.
//
//   x_i     = penalise(fp32(logit_i), hist[b, i]); the selection, the draw and kept / thresh / u
//             are those of the ROWS form on the fp32 row x (fp32 keys: 4 radix rounds also for
//             bf16 storage);
//   logp[b] = (log-probability of the id under softmax(raw logits): (l_id - l_max) - log S1 with
//              S1 = sum_i exp(l_i - l_max), summed like M as 2^40 fixed-point integers in the
//              kept-mass pass;  log-probability under the distribution drawn from: log(m_id / M));
//   update  : hist[b, id] += 1.
//
// The update is a plain store by the lane that found the crossing, of the word that lane loaded
// plus one.  It races with nothing: every other wave has finished its last read of the row when
// it passes the barrier in front of the sum M (the waves that do not own the crossing return
// right after it), only the owning wave still reads the row, and within that wave the store
// follows the loads of the iteration that found the crossing, the last one it runs.  Workgroup b
// touches row b of hist alone.
// Any table or history content is safe: the values only steer comparisons and arithmetic, every
// loop is bounded by the row, and ids[b] and logp[b, :] are preset to 0.
//
// The body is sample_logits_k<T, true>'s, copied (see the note there), and PenRow::load repeats
// Row::load: a fix to the draw, the tie rules or the loaders belongs in both.
template <typename T>
__global__ __launch_bounds__(1024) void sample_logits_pen_k(
    const T* __restrict__ logits, long long ld, int vocab, bool vec_ok, const int64_t* __restrict__ pos,
    const float* __restrict__ u_in, int64_t* __restrict__ ids, int* __restrict__ kept, float* __restrict__ thresh,
    float* __restrict__ u_out, float* __restrict__ logp, const float* __restrict__ inv_t_r,
    const int* __restrict__ top_k_r, const double* __restrict__ top_p_r, const int64_t* __restrict__ seed_r,
    const int* __restrict__ rid_r, const float* __restrict__ rep_r, const float* __restrict__ inv_rep_r,
    const float* __restrict__ pres_r, const float* __restrict__ freq_r, int* hist, long long ld_h, bool hvec_ok,
    bool update) {
  constexpr int N = Vec<T>::N;
  __shared__ Shared sh;
  __shared__ SharedPen shp;
  const int b = blockIdx.x, nw = blockDim.x >> 6;
  const float inv_t = inv_t_r[b];
  const int top_k = top_k_r[b];
  const double top_p = top_p_r[b];
  const u64 seed = (u64)seed_r[b];
  const uint32_t rid = (uint32_t)rid_r[b];
  if (threadIdx.x == 0) {   // ordered before the draw's stores by the barriers below
    ids[b] = 0;
    logp[2 * b] = 0.f;
    logp[2 * b + 1] = 0.f;
  }
  const bool greedy = inv_t == 0.f;
  int* const hrow = hist + (long long)b * ld_h;
  PenRow<T> row;
  row.p = logits + (long long)b * ld;
  row.h = hrow;
  row.rep = rep_r[b];
  row.inv_rep = inv_rep_r[b];
  row.pres = pres_r[b];
  row.freq = freq_r[b];
  row.vocab = vocab;
  row.nv = (vocab + N - 1) / N;
  row.wv = ((row.nv + nw - 1) / nw + 63) & ~63;
  row.wave = threadIdx.x >> 6;
  row.lane = lane_id();
  row.vec_ok = vec_ok;
  row.hvec_ok = hvec_ok;

  // maximum / minimum key of the penalised row, maximum key of the raw row
  uint32_t kmax = 0, kmin = 0xFFFFFFFFu, lkmax = 0;
  row.for_each([&](int, uint32_t key, float, float lg) {
    kmax = max(kmax, key);
    kmin = min(kmin, key);
    lkmax = max(lkmax, raw_to_key<float>(__float_as_uint(lg)));
  });
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    kmax = max(kmax, (uint32_t)__shfl_xor(kmax, o, 64));
    kmin = min(kmin, (uint32_t)__shfl_xor(kmin, o, 64));
    lkmax = max(lkmax, (uint32_t)__shfl_xor(lkmax, o, 64));
  }
  if (row.lane == 0) {
    sh.wave_a[row.wave] = kmax;
    sh.wave_b[row.wave] = kmin;
    shp.wave_c[row.wave] = lkmax;
  }
  __syncthreads();
  for (int w = 0; w < nw; ++w) {
    kmax = max(kmax, sh.wave_a[w]);
    kmin = min(kmin, sh.wave_b[w]);
    lkmax = max(lkmax, shp.wave_c[w]);
  }
  const float zmax = key_to_float<float>(kmax) * inv_t;
  const float lmax = key_to_float<float>(lkmax);

  uint32_t thr = kmin;
  if (greedy) {
    thr = kmax;
  } else {
    if (top_k > 0 && top_k < vocab)
      thr = radix_select<float, false, true, PenRow<T>>(row, sh, 0u, (u64)top_k, 1.0, inv_t, zmax);
    if (top_p < 1.0) thr = radix_select<float, true, true, PenRow<T>>(row, sh, thr, 0, top_p, inv_t, zmax);
  }

  // kept mass and count per wave, in index order; the raw row's mass S1 beside them
  u64 tot = 0, s1 = 0;
  uint32_t cnt = 0;
  row.for_each([&](int, uint32_t key, float val, float lg) {
    s1 += weight_fx(lg, 1.0f, lmax);
    if (key >= thr) {
      tot += weight_fx(val, inv_t, zmax);
      ++cnt;
    }
  });
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    tot += (u64)__shfl_xor(tot, o, 64);
    s1 += (u64)__shfl_xor(s1, o, 64);
    cnt += (uint32_t)__shfl_xor(cnt, o, 64);
  }
  __syncthreads();   // wave_a / wave_b of the max pass have been read
  if (row.lane == 0) {
    sh.wave_tot[row.wave] = tot;
    shp.wave_s1[row.wave] = s1;
    sh.wave_a[row.wave] = cnt;
  }
  __syncthreads();   // every wave's last read of the row (logits and history) lies before this
  u64 M = 0, S1 = 0, base = 0;
  uint32_t nkept = 0;
  for (int w = 0; w < nw; ++w) {
    if (w < row.wave) base += sh.wave_tot[w];
    M += sh.wave_tot[w];
    S1 += shp.wave_s1[w];
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
    thresh[b] = key_to_float<float>(thr);
    u_out[b] = u;
  }
  if (!(base < need && need <= base + tot)) return;   // one wave owns the crossing
  u64 running = base;
  for (int it = 0; it < row.iters(); ++it) {
    const int v = row.vec_at(it);
    u64 m[N], s = 0;
    float lg[N];
    int hw[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
      m[j] = 0;
      lg[j] = 0.f;
      hw[j] = 0;
    }
    if (v < row.nv) {
      row.load(v, lg, hw);
#pragma unroll
      for (int j = 0; j < N; ++j) {
        const uint32_t key = raw_to_key<float>(__float_as_uint(row.pen(lg[j], hw[j])));
        if (v * N + j < vocab && key >= thr) m[j] = weight_fx(key_to_float<float>(key), inv_t, zmax);
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
        u64 acc = running + incl - s, m_id = 0;
        int id = -1, h_id = 0;
        float l_id = 0.f;
#pragma unroll
        for (int j = 0; j < N; ++j) {
          acc += m[j];
          if (id < 0 && acc >= need) {
            id = v * N + j;
            m_id = m[j];
            l_id = lg[j];
            h_id = hw[j];
          }
        }
        KASSERT(id >= 0 && id < vocab, "id %d, vocab %d", id, vocab);
        if (id >= 0 && id < vocab) {   // (always: m[j] > 0 only at valid columns)
          ids[b] = id;
          const float dl = l_id - lmax;   // one fp32 subtract, as in weight_fx
          logp[2 * b] = (float)((double)dl - log((double)S1 * 9.094947017729282379150390625e-13));   // 2^-40
          logp[2 * b + 1] = (float)(log((double)m_id) - log((double)M));
          if (update) hrow[id] = h_id + 1;
        }
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

// The penalised form (sample_logits_pen_k): the five per-row settings of the form above, the
// penalties rep / inv_rep = fp32(1 / rep) / pres / freq (fp32, B values each) and the history
// hist [B, >= vocab] int32 with row stride ld_h (bit 31: the id occurs in the prompt; bits 0..30:
// draws so far), in device memory.  hist_vec_ok: its rows are 16-byte aligned and hold whole
// vectors of the logits' layout past vocab.  update != 0: hist[b, ids[b]] += 1.  logp [B, 2].
extern "C" void dpfs_sample_logits_pen(const void* logits, int dtype, long long ld, int B, int vocab, int vec_ok,
                                       const float* inv_t, const int* top_k, const double* top_p,
                                       const int64_t* seed, const int* rid, const float* rep, const float* inv_rep,
                                       const float* pres, const float* freq, int* hist, long long ld_h,
                                       int hist_vec_ok, int update, const int64_t* pos, const float* u_in,
                                       int64_t* ids, int* kept, float* thresh, float* u_out, float* logp,
                                       hipStream_t s) {
  if (B <= 0) return;
  const int nt = sample_threads(dtype, vocab);
  if (dtype == kBF16)
    sample_logits_pen_k<bf16><<<B, nt, 0, s>>>((const bf16*)logits, ld, vocab, vec_ok != 0, pos, u_in, ids, kept,
                                               thresh, u_out, logp, inv_t, top_k, top_p, seed, rid, rep, inv_rep, pres,
                                               freq, hist, ld_h, hist_vec_ok != 0, update != 0);
  else
    sample_logits_pen_k<float><<<B, nt, 0, s>>>((const float*)logits, ld, vocab, vec_ok != 0, pos, u_in, ids, kept,
                                                thresh, u_out, logp, inv_t, top_k, top_p, seed, rid, rep, inv_rep, pres,
                                                freq, hist, ld_h, hist_vec_ok != 0, update != 0);
  LAUNCH_CHECK();
}
