// Host-side check of csrc/gq_stats.h (CPU suite, no GPU): the integer split of an fp32 addend (stat_add_f32) is
// bit-identical to the fp64 split (stat_add), sums are order-independent, the value read back is the exact sum of the
// addends down to 2^-56, out-of-range addends poison the record, and the shifted per-thread partials (StatPartial) give
// the mean and variance of an fp64 two-pass for mean / std up to 1e4, whatever the thread partition.  Built and run by tests/test_host.py.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#define GQ_STATS_HOST_TEST 1
#define __device__
#define __forceinline__ inline
static inline unsigned __float_as_uint(float f) { unsigned u; std::memcpy(&u, &f, 4); return u; }
static inline unsigned long long atomicAdd(unsigned long long *p, unsigned long long v) { const unsigned long long o = *p; *p = o + v; return o; }
#include "gq_stats.h"

using namespace gqhip;

int main() {
  std::mt19937_64 rng(12345);
  std::vector<float> vals;
  const float edges[] = {0.f, -0.f, 1.f, -1.f, 1e-30f, 1.17549435e-38f, 1e-45f, 5.4210109e-20f /* 2^-64 */, 1.3877788e-17f /* 2^-56 */,
                         2.7755576e-17f, 1.52587890625e-05f, 0.99999994f, 16777216.f, 16777217.f, 1.09951163e12f /* 2^40 */, 1.8446743e19f /* ~2^64- */,
                         9.223372e18f, -9.223372e18f, 3.4e38f, INFINITY, -INFINITY, NAN};
  for (float e : edges) vals.push_back(e);
  for (int i = 0; i < 200000; ++i) {
    const unsigned bits = (unsigned)rng();
    float f; std::memcpy(&f, &bits, 4);
    vals.push_back(f);
  }
  std::uniform_real_distribution<float> uni(-8.f, 8.f);
  for (int i = 0; i < 100000; ++i) vals.push_back(uni(rng) * uni(rng));
  // 1. per addend: integer split == fp64 split
  long bad = 0;
  for (float v : vals) {
    int64_t a[kStatWords] = {0}, b[kStatWords] = {0};
    stat_add(a, (double)v, (double)v);
    stat_add_f32(b, v, v);
    if (std::memcmp(a, b, sizeof(a)) != 0) {
      if (bad < 5) std::printf("mismatch at %a: f64 {%lld %lld %lld | p %lld} int {%lld %lld %lld | p %lld}\n", (double)v, (long long)a[0], (long long)a[1],
                               (long long)a[2], (long long)a[6], (long long)b[0], (long long)b[1], (long long)b[2], (long long)b[6]);
      ++bad;
    }
  }
  if (bad) { std::printf("FAIL: %ld addends split differently\n", bad); return 1; }
  // 2. order independence + exactness: finite moderate values, forward vs reversed vs shuffled; value == long double sum of truncated addends
  std::vector<float> fin;
  for (float v : vals) if (std::isfinite(v) && std::fabs(v) < 1e15f) fin.push_back(v);
  int64_t r0[kStatWords] = {0}, r1[kStatWords] = {0};
  for (size_t i = 0; i < fin.size(); ++i) stat_add_f32(r0, fin[i], fin[i] * fin[i] < 1e18f ? fin[i] * fin[i] : 0.f);
  for (size_t i = fin.size(); i-- > 0;) stat_add_f32(r1, fin[i], fin[i] * fin[i] < 1e18f ? fin[i] * fin[i] : 0.f);
  if (std::memcmp(r0, r1, sizeof(r0)) != 0) { std::printf("FAIL: order dependence\n"); return 1; }
  __int128 exact = 0;                                 // in units of 2^-56; |v| < 2^50 -> each addend < 2^106
  for (float v : fin) {
    int ex;
    const double fr = std::frexp((double)v, &ex);     // v = fr 2^ex, |fr| in [0.5, 1): 24 significant bits
    const long long m = (long long)std::ldexp(fr, 24);          // exact integer significand
    const int sh = ex - 24 + 56;
    if (sh >= 0) exact += (__int128)m << sh;
    else if (sh > -63) exact += (__int128)(m < 0 ? -((-m) >> -sh) : m >> -sh);   // truncation toward zero
  }
  const __int128 back = ((__int128)r0[2] << 80) + ((__int128)r0[1] << 40) + (__int128)r0[0];
  if (back != exact) { std::printf("FAIL: limbs != exact integer sum (diff %g units of 2^-56)\n", (double)(back - exact)); return 1; }
  double s, ss;
  stat_load(r0, s, ss);
  const double want = (double)exact * 0x1p-56;
  if (std::fabs(s - want) > std::fabs(want) * 0x1p-50 + 0x1p-56) { std::printf("FAIL: stat_load %.17g vs %.17g\n", s, want); return 1; }
  // 3. poison
  int64_t p[kStatWords] = {0};
  stat_add_f32(p, 1.0f, INFINITY);
  stat_load(p, s, ss);
  if (!(s != s) || !(ss != ss)) { std::printf("FAIL: poison not reported\n"); return 1; }
  // 4. shifted partials (StatPartial): groups x = c + sigma N(0, 1) in fp32, c / sigma up to 1e4, plus an outlier that is the
  //    first value of its thread.  The record read back by the consumers' formula var = SS / n - mean^2 must match an fp64
  //    two-pass over the same fp32 values to 2^-40 of var + 2^-50 mean^2 (the fp64 floor of that formula; 2^-40 leaves 2^16
  //    below the 8 x 2^-24 the GPU tests allow), and the same data cut into threads two different ways gives the same sums
  //    up to the fp64 arithmetic inside a thread and the per-addend truncation at 2^-56.
  std::normal_distribution<double> gauss(0.0, 1.0);
  const double ratios[] = {0.0, 1.0, 10.0, 100.0, 1000.0, 1e4};
  const double sigmas[] = {0x1p-10, 1.0, 0x1p10};
  const int n = 4096;
  int cases = 0;
  for (int outlier = 0; outlier < 2; ++outlier)
    for (double r : ratios)
      for (double sg : sigmas) {
        std::vector<float> x(n);
        for (int i = 0; i < n; ++i) x[i] = (float)(r * sg + sg * gauss(rng));
        if (outlier) x[0] = (float)(r * sg + 1000.0 * sg);
        long double m = 0.0L;
        for (float v : x) m += v;
        m /= n;
        long double v2 = 0.0L;
        for (float v : x) v2 += ((long double)v - m) * ((long double)v - m);
        const double mean64 = (double)m, var64 = (double)(v2 / n);
        int64_t rec[2][kStatWords] = {{0}, {0}};
        const int per[2] = {64, 16};                     // two thread partitions of the same data
        for (int k = 0; k < 2; ++k)
          for (int t0 = 0; t0 < n; t0 += per[k]) {
            StatPartial p;
            for (int i = t0; i < t0 + per[k]; ++i) stat_partial_add(p, x[i]);
            stat_partial_flush(rec[k], p);
          }
        for (int k = 0; k < 2; ++k) {
          double s2, ss2;
          stat_load(rec[k], s2, ss2);
          const double mean = s2 / n;
          double var = ss2 / n - mean * mean;
          var = var > 0.0 ? var : 0.0;
          const double dm = std::fabs(mean - mean64), dv = std::fabs(var - var64);
          if (dm > 0x1p-40 * (std::fabs(mean64) + std::sqrt(var64)) || dv > 0x1p-40 * var64 + 0x1p-50 * mean64 * mean64) {
            std::printf("FAIL: shifted partials, c/sigma %g sigma %g outlier %d partition %d: mean %.17g vs %.17g, var %.17g vs %.17g\n",
                        r, sg, outlier, per[k], mean, mean64, var, var64);
            return 1;
          }
        }
        // the two partitions: the same sums up to the fp64 arithmetic inside a thread ((64 + 2) 2^-53 < 2^-46 of the sum of
        // squares, charged 2^-44) and the truncation of the addends (n / 16 addends of < 2^-56 each per statistic)
        double sa, ssa, sb, ssb;
        stat_load(rec[0], sa, ssa);
        stat_load(rec[1], sb, ssb);
        if (std::fabs(sa - sb) > (n / 16) * 0x1p-56 + 0x1p-44 * std::sqrt(n * ssa) ||      // sum |v| <= sqrt(n sum v^2)
            std::fabs(ssa - ssb) > (n / 16) * 0x1p-56 + 0x1p-44 * std::fabs(ssa)) {
          std::printf("FAIL: partitions disagree: %.17g %.17g / %.17g %.17g\n", sa, sb, ssa, ssb);
          return 1;
        }
        ++cases;
      }
  // order independence of the shifted record: the same threads flushed in reverse order give identical limbs
  {
    std::vector<float> x(2048);
    for (auto &v : x) v = (float)(300.0 + gauss(rng));
    int64_t a[kStatWords] = {0}, b[kStatWords] = {0};
    for (int t = 0; t < 32; ++t) { StatPartial p; for (int i = 0; i < 64; ++i) stat_partial_add(p, x[64 * t + i]); stat_partial_flush(a, p); }
    for (int t = 32; t-- > 0;) { StatPartial p; for (int i = 0; i < 64; ++i) stat_partial_add(p, x[64 * t + i]); stat_partial_flush(b, p); }
    if (std::memcmp(a, b, sizeof(a)) != 0) { std::printf("FAIL: shifted partials order dependence\n"); return 1; }
    StatPartial p;                                    // a non-finite value poisons, also as the shift
    stat_partial_add(p, INFINITY);
    stat_partial_add(p, 1.0f);
    int64_t q[kStatWords] = {0};
    stat_partial_flush(q, p);
    stat_load(q, s, ss);
    if (!(s != s)) { std::printf("FAIL: shifted partials: poison not reported\n"); return 1; }
  }
  std::printf("ok: %zu addends, %zu in the order test, %d shifted-partial groups\n", vals.size(), fin.size(), cases);
  return 0;
}
