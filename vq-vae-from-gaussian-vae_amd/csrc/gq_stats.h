// gq_stats.h -- order-independent accumulation of the GroupNorm statistics.
//
// The conv-stack kernels leave the statistics of the NEXT GroupNorm (sum and sum of squares per (image, group)) with
// their output, accumulated across threads and blocks by atomics.  A floating-point atomic sum depends on the order
// in which the adds land, so the statistics -- and with them the encoder's z and, at a near-tie, a token -- could
// differ between two runs of the same input (the reference's CPU path is deterministic: pit/quantization/
// gaussian.py:136-150 sees one z per image).  Here every addend (one thread's partial sums: StatPartial below) is converted EXACTLY
// to a 120-bit fixed-point number held in three signed 64-bit limbs of 40 payload bits each, and the limbs are summed
// with integer atomics: integer addition is associative, so the total is the exact sum of the addends whatever the
// order, and the statistics are bit-reproducible by construction.
//
//   value = q[0] * 2^-56 + q[1] * 2^-16 + q[2] * 2^24,   |q[k]| < 2^40 per addend
//
// Range: |addend| < 2^64 (a sum of squares of fp32 activations up to ~4e9 per element at 1 element per thread);
// bits below 2^-56 of an addend are truncated toward zero (a function of the addend alone, so still order-independent;
// 2^-56 is 36 binary orders below the eps = 1e-6 of every GroupNorm of this UNet).  24 spare bits per limb allow 2^23
// addends per statistic.  An addend that is not finite or not below 2^64 poisons the record (q[6] != 0) and every
// reader then sees NaN -- loud, like the fp64 sum it replaces.
//
// Record per (image, group): 8 x int64 = {sum: q0 q1 q2, sum of squares: q0 q1 q2, poison, unused} (64 bytes).
#pragma once
#ifndef GQ_STATS_HOST_TEST          // tests/stats_host_test.cpp compiles the arithmetic for the host with its own shims
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

namespace gqhip {

constexpr int kStatWords = 8;   // int64 words per (image, group) record

// the three limbs of one addend
__device__ __forceinline__ void stat_split(double v, int64_t (&q)[3], bool &poison) {
  const double a = __builtin_fabs(v);
  poison = !(a < 18446744073709551616.0);                 // NaN, inf, >= 2^64
  const double a2 = __builtin_trunc(a * 5.9604644775390625e-08);             // a / 2^24
  double r = a - a2 * 16777216.0;                                           // exact: < 2^24
  const double a1 = __builtin_trunc(r * 65536.0);                           // r / 2^-16
  r = r * 65536.0 - a1;                                                     // exact: < 1 (in units of 2^-16)
  const double a0 = __builtin_trunc(r * 1099511627776.0);                   // units of 2^-56
  const bool neg = v < 0.0;
  q[2] = poison ? 0 : (neg ? -(int64_t)a2 : (int64_t)a2);
  q[1] = poison ? 0 : (neg ? -(int64_t)a1 : (int64_t)a1);
  q[0] = poison ? 0 : (neg ? -(int64_t)a0 : (int64_t)a0);
}

__device__ __forceinline__ void stat_atomic_add(int64_t *dst, int64_t v) {
  if (v != 0) atomicAdd(reinterpret_cast<unsigned long long *>(dst), (unsigned long long)v);
}

// Add one addend pair (a thread's fp32 partial sums, or a fixed-order combination of them) to a record in LDS or
// global memory.
__device__ __forceinline__ void stat_add(int64_t *rec, double s, double ss) {
  int64_t q[3];
  bool bad, bad2;
  stat_split(s, q, bad);
  stat_atomic_add(rec + 0, q[0]);
  stat_atomic_add(rec + 1, q[1]);
  stat_atomic_add(rec + 2, q[2]);
  stat_split(ss, q, bad2);
  stat_atomic_add(rec + 3, q[0]);
  stat_atomic_add(rec + 4, q[1]);
  stat_atomic_add(rec + 5, q[2]);
  if (bad) atomicAdd(reinterpret_cast<unsigned long long *>(rec + 6), 1ull);
  if (bad2) atomicAdd(reinterpret_cast<unsigned long long *>(rec + 6), 1ull);
}

// The same for a thread's fp32 partial sums (the common case), by integer arithmetic on the fp32 bits: the 24-bit
// significand m of v = m 2^(e - 150) lands at bit (e - 94) of the fixed-point number, i.e. in limb k = (e - 94) / 40 and,
// when it straddles, limb k + 1 -- two shifts and at most two atomics instead of ~80 fp64 instructions.  Bit-identical
// to stat_split((double)v) (tests/stats_host_test.cpp).  The conv-stack producers no longer add raw fp32 partials (see
// StatPartial: their variance error grew like (mean / std)^2); the split itself is what the host test pins.
__device__ __forceinline__ void stat_add_one_f32(int64_t *limbs, int64_t *poison, float v) {
  const unsigned bits = __float_as_uint(v);
  const int e = (int)((bits >> 23) & 0xffu);
  if (e >= 191) {                                     // |v| >= 2^64, inf, NaN
    atomicAdd(reinterpret_cast<unsigned long long *>(poison), 1ull);
    return;
  }
  const unsigned long long m = (unsigned long long)((bits & 0x7fffffu) | (e ? 0x800000u : 0u));
  const int shift = (e ? e : 1) - 94;                 // v = +- m 2^(shift - 56)
  if (shift <= -24) return;                           // entirely below 2^-56
  unsigned long long lo, hi = 0ull;
  int k = 0;
  if (shift < 0) {
    lo = m >> (-shift);                               // truncation toward zero, as stat_split
  } else {
    k = shift >= 80 ? 2 : (shift >= 40 ? 1 : 0);
    const unsigned long long t = m << (shift - 40 * k);          // < 2^64: the in-limb offset is < 40 and m < 2^24
    lo = t & 0xffffffffffull;
    hi = t >> 40;                                     // 0 when k == 2 (offset <= 16)
  }
  const bool neg = (bits >> 31) != 0u;
  stat_atomic_add(limbs + k, neg ? -(int64_t)lo : (int64_t)lo);
  if (hi) stat_atomic_add(limbs + k + 1, neg ? -(int64_t)hi : (int64_t)hi);
}
__device__ __forceinline__ void stat_add_f32(int64_t *rec, float s, float ss) {
#ifdef GQHIP_STATS_SPLIT_F64   // diagnostic build (A/B timing): the fp64 split for fp32 addends too
  stat_add(rec, (double)s, (double)ss);
#else
  stat_add_one_f32(rec, rec + 6, s);
  stat_add_one_f32(rec + 3, rec + 6, ss);
#endif
}

// A thread's partial moments of its values v of one group, SHIFTED by the thread's first value v0: d = v - v0 is exact in
// fp64 (two fp32 values), sum d and sum d^2 accumulate in fp64, and the flush rebuilds sum v = s + n v0 and
// sum v^2 = ss + v0 (2 s + n v0) in fp64 before the exact limb split.  Why: consumers form var = SS / n - mean^2, so an
// absolute error e of SS costs e / (n var) of var.  fp32 partials of raw v and v^2 make e ~ 2^-24 n_t SS, i.e. a relative
// error of var ~ 2^-24 n_t (mean / std)^2 -- 0.3 % at mean / std = 1000 (tests/test_gpu_groupnorm_offsets.py).  Shifted
// fp64 partials leave ~2^-53 n_t (spread of the thread's d / std)^2 plus 2^-53 (mean / std)^2 for the fp64 rebuild:
// below 2^-30 of var up to mean / std = 1e4 (tests/stats_host_test.cpp).  fp64 rather than fp32 for d: a thread whose first
// value is an outlier has d ~ the outlier for all its values, and an fp32 sum of those would cost ~n_t 2^-24 outlier^2 of SS.
// Every addend is still a function of the thread's own values alone, so the record stays order-independent.
struct StatPartial {
  double v0 = 0.0, s = 0.0, ss = 0.0;
  int n = 0;
};
__device__ __forceinline__ void stat_partial_add(StatPartial &p, float v) {
  if (p.n == 0) p.v0 = (double)v;      // non-finite v0: d = NaN, the record is poisoned as before
  const double d = (double)v - p.v0;
  p.s += d;
  p.ss = __builtin_fma(d, d, p.ss);
  ++p.n;
}
template <typename VEC>
__device__ __forceinline__ void stat_partial_add_vec(StatPartial &p, VEC v) {
#pragma unroll
  for (int e = 0; e < (int)(sizeof(VEC) / sizeof(float)); ++e) stat_partial_add(p, v[e]);
}
// (sum v, sum v^2) of the partial, as stat_add takes them
__device__ __forceinline__ void stat_partial_moments(const StatPartial &p, double &s, double &ss) {
  const double n = (double)p.n;
  s = __builtin_fma(n, p.v0, p.s);
  ss = __builtin_fma(p.v0, __builtin_fma(n, p.v0, 2.0 * p.s), p.ss);
}
__device__ __forceinline__ void stat_partial_flush(int64_t *rec, const StatPartial &p) {
  double s, ss;
  stat_partial_moments(p, s, ss);
  stat_add(rec, s, ss);
}

// word `w` of a block's LDS records -> the same word of the global records (one thread per word)
__device__ __forceinline__ void stat_flush_word(int64_t *global_word, int64_t local_word) {
  stat_atomic_add(global_word, local_word);
}

// (sum, sum of squares) of a finished record, as doubles; a fixed evaluation order, the same for every reader
__device__ __forceinline__ void stat_load(const int64_t *rec, double &s, double &ss) {
  s = ((double)rec[2] * 16777216.0 + (double)rec[1] * 1.52587890625e-05) + (double)rec[0] * 1.3877787807814457e-17;
  ss = ((double)rec[5] * 16777216.0 + (double)rec[4] * 1.52587890625e-05) + (double)rec[3] * 1.3877787807814457e-17;
  if (rec[6] != 0) {
    s = __builtin_nan("");
    ss = __builtin_nan("");
  }
}

// ---- the GroupNorm fold: THE definition every consumer of a record calls, so the fused consumers (Winograd input
// transforms, direct convolutions) and gn_apply + their plain twins see the same bits of a and sh by construction.
// Record -> (mean, rstd) of the group's n values: fp64, the variance clamped at zero, eps inside the root.
struct GnGroup {
  double mean, rstd;
};
__device__ __forceinline__ GnGroup gn_group(const int64_t *rec, double n, double eps) {
  double s, ss;
  stat_load(rec, s, ss);
  const double mean = s / n;
  double var = ss / n - mean * mean;
  var = var > 0.0 ? var : 0.0;
  return {mean, 1.0 / sqrt(var + eps)};
}
// Channel c: y = a x + sh is gamma (x + pre_bias - mean) rstd + beta (pre_bias nullable: a bias still pending on x).  Every
// operation in fp64 (-ffp-contract=off: no fused multiply-add), one rounding to fp32 each; the order is load pre_bias, a, sh.
struct GnAffine {
  float a, sh;
};
__device__ __forceinline__ GnAffine gn_channel(const GnGroup g, const float *gamma, const float *beta, const float *pre_bias,
                                               int c) {
  const double pbk = pre_bias ? (double)pre_bias[c] : 0.0;
  GnAffine f;
  f.a = (float)(g.rstd * (double)gamma[c]);
  f.sh = (float)((double)beta[c] + (pbk - g.mean) * g.rstd * (double)gamma[c]);
  return f;
}

}  // namespace gqhip
