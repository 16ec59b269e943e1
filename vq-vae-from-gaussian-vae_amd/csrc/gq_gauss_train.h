// gq_gauss_train.h -- the train-mode step of the Gaussian regularizers (pit/quantization/gaussian.py:77-119 GQ1, :211-271 GQ2):
// one elementwise forward (GQ1: sample + per-row KL bits; GQ2's forward is gq_quantize_z_gauss_f32) and one elementwise backward
// for both, which writes the whole grad_z -- the mu half and the logvar half.
//
// Forward (gq_gauss_train_f32): zhat = mu + noise * sd, optionally sd, and kl2row[row] (row = (b L + l) K + k, the eval path's
// indexing) = the fp64 sum, in ascending g, of kl_bits_term(mu, lv) rounded once -- the same function and the same order as
// gq_prep.h, so the statistics block (gq_gauss.h: gauss_stats_finalize_kernel, the SECOND launch on the stream; nothing is handed
// between workgroups inside a launch) sees the bits the eval call would have produced.
//
// Backward (gq_gauss_backward_f32): per row the kernel recomputes kl2 exactly as the forward did, so the row's class -- and with it
// its weight -- is the forward's and nothing per row is saved:
//     w(row) = (float)lam_max if kl2 > thr_hi, (float)lam_min if kl2 < thr_lo, 1 otherwise   (lambdas as they were BEFORE the update)
//     coef   = g_kl * (float)lam * w(row) / divisor
//     grad_mu     = g_zhat + coef * 1.4426 * mu
//     grad_logvar = inside ? g_zhat * noise * 0.5 * sd + g_sd * 0.5 * sd + coef * 1.4426 * 0.5 * (var - 1) : 0
// with inside = (lv_min <= logvar <= lv_max) on the unclamped value (torch.clamp's gradient mask; NaN is outside), 1.4426 * 0.5 =
// float(0.7213) as in the forward, sd / var = fp64 exp rounded once.  Two passes over the row's channels (one for kl2, one for
// the gradients; the second is served from cache): a thread cannot hold a row of up to 64 elements in registers.
//
// Work split: a thread owns a SLAB of V elements along the contiguous axis, so that every access is V * 4 bytes:
//   rows-wide  V consecutive rows of the same g:  BCHW (V positions l; needs L % V == 0), BLC with strided grouping (V
//              sub-codebooks k; needs K % V == 0); V = 1 is the form that serves every shape;
//   g-wide     V consecutive g of ONE row: BLC with contiguous channels (contiguous grouping, or K == 1), dim % V == 0.
// Grid: at most 2048 blocks of 256 threads, grid-stride over the slabs.  No atomics, no LDS, no cross-block traffic.
#pragma once
#include "gq_common.h"
#include "gq_prep.h"

namespace gqhip {

constexpr int kTrainMaxBlocks = 2048;

struct GaussTrainParams {
  const float *z;            // [B, 2c, L] (BCHW) or [B, L, 2c] (BLC)
  const float *noise;        // layout of zhat
  float *zhat, *sd_out;      // forward: [B, c, L] / [B, L, c]; sd_out may be NULL
  float *kl2row;             // forward: [rows]
  const float *g_zhat, *g_sd, *g_kl;   // backward: upstream gradients (layout of zhat; one float), each may be NULL = zero
  const double *lam_before;  // backward: { lam, lam_min, lam_max } before the forward's update
  float *grad_z;             // backward: layout of z
  double divisor;            // backward: the loss divisor (GaussStatsParams::loss_divisor of the forward)
  float thr_hi, thr_lo;      // backward: float(n + tol), float(n - tol)
  float lv_min, lv_max;
  long items;                // slabs
  int dim, K, L, c;
  int layout;                // 1 BCHW, 2 BLC (OutMap::mode)
  int grouping;              // 0 strided, 1 contiguous
};

template <int V>
struct alignas(4 * V) FV {
  float v[V];
};
template <int V>
__device__ __forceinline__ FV<V> ldv(const float *p) { return *reinterpret_cast<const FV<V> *>(p); }
template <int V>
__device__ __forceinline__ void stv(float *p, const FV<V> &x) { *reinterpret_cast<FV<V> *>(p) = x; }

// slab i -> offset of its first mu in z (zo), of its first element in the layout of zhat (oo), the stride between consecutive g
// (gs; the same in both tensors), its first row and the stride between its rows (rs)
template <int V, bool GW>
__device__ __forceinline__ void train_slab(const GaussTrainParams &p, long i, long &zo, long &oo, long &gs, long &row0, long &rs) {
  if constexpr (GW) {          // BLC, the row's channels contiguous: slab = row
    const long pos = i / p.K;
    const int k = (int)(i % p.K);
    zo = pos * 2 * p.c + (long)k * p.dim;
    oo = pos * p.c + (long)k * p.dim;
    gs = 1; row0 = i; rs = 1;
    return;
  }
  if (p.layout == 1) {
    const long nl = p.L / V;
    const long l = (i % nl) * V;
    const int k = (int)((i / nl) % p.K);
    const long b = i / (nl * p.K);
    const long ch0 = p.grouping == 0 ? k : (long)k * p.dim;
    zo = (b * 2 * p.c + ch0) * p.L + l;
    oo = (b * p.c + ch0) * p.L + l;
    gs = (p.grouping == 0 ? (long)p.K : 1L) * p.L;
    row0 = (b * p.L + l) * p.K + k;
    rs = p.K;
  } else {
    const long nk = p.K / V;
    const int k = (int)(i % nk) * V;
    const long pos = i / nk;
    const long ch0 = p.grouping == 0 ? k : (long)k * p.dim;     // (V > 1: strided only)
    zo = pos * 2 * p.c + ch0;
    oo = pos * p.c + ch0;
    gs = p.grouping == 0 ? (long)p.K : 1L;
    row0 = pos * p.K + k;
    rs = 1;
  }
}

// torch.clamp propagates NaN; min / max with explicit compares keeps that (gq_prep.h)
__device__ __forceinline__ float train_clamp(float lv, float lo, float hi) {
  lv = lv < lo ? lo : lv;
  lv = lv > hi ? hi : lv;
  return lv;
}

// the slab's KL bits: per row the fp64 sum of kl_bits_term in ascending g (the forward and the backward both call this)
template <int V, bool GW>
__device__ __forceinline__ void train_row_bits(const GaussTrainParams &p, long zo, long lvo, long gs, double (&acc)[GW ? 1 : V]) {
#pragma unroll
  for (int j = 0; j < (GW ? 1 : V); ++j) acc[j] = 0.0;
  if constexpr (GW) {
    for (int g = 0; g < p.dim; g += V) {
      const FV<V> m = ldv<V>(p.z + zo + g), lv = ldv<V>(p.z + zo + lvo + g);
#pragma unroll
      for (int j = 0; j < V; ++j) acc[0] += (double)kl_bits_term(m.v[j], train_clamp(lv.v[j], p.lv_min, p.lv_max));
    }
  } else {
    for (int g = 0; g < p.dim; ++g) {
      const FV<V> m = ldv<V>(p.z + zo + g * gs), lv = ldv<V>(p.z + zo + lvo + g * gs);
#pragma unroll
      for (int j = 0; j < V; ++j) acc[j] += (double)kl_bits_term(m.v[j], train_clamp(lv.v[j], p.lv_min, p.lv_max));
    }
  }
}

template <int V, bool GW>
__global__ __launch_bounds__(256) void gauss_train_fwd_kernel(const GaussTrainParams p) {
#pragma clang fp contract(off)
  constexpr int NR = GW ? 1 : V;
  const long lvo = p.layout == 1 ? (long)p.c * p.L : (long)p.c;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < p.items; i += (long)gridDim.x * 256) {
    long zo, oo, gs, row0, rs;
    train_slab<V, GW>(p, i, zo, oo, gs, row0, rs);
    double acc[NR];
#pragma unroll
    for (int j = 0; j < NR; ++j) acc[j] = 0.0;
    const int steps = GW ? p.dim / V : p.dim;
    for (int s = 0; s < steps; ++s) {
      const long d = GW ? (long)s * V : (long)s * gs;
      const FV<V> m = ldv<V>(p.z + zo + d), lvr = ldv<V>(p.z + zo + lvo + d), nz = ldv<V>(p.noise + oo + d);
      FV<V> zh, sd;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float lv = train_clamp(lvr.v[j], p.lv_min, p.lv_max);
        const float half = 0.5f * lv;
        sd.v[j] = (float)exp((double)half);
        const float e = nz.v[j] * sd.v[j];
        zh.v[j] = m.v[j] + e;
        acc[GW ? 0 : j] += (double)kl_bits_term(m.v[j], lv);
      }
      stv<V>(p.zhat + oo + d, zh);
      if (p.sd_out) stv<V>(p.sd_out + oo + d, sd);
    }
#pragma unroll
    for (int j = 0; j < NR; ++j) p.kl2row[row0 + j * rs] = (float)acc[j];
  }
}

template <int V, bool GW>
__global__ __launch_bounds__(256) void gauss_train_bwd_kernel(const GaussTrainParams p) {
#pragma clang fp contract(off)
  constexpr int NR = GW ? 1 : V;
  const long lvo = p.layout == 1 ? (long)p.c * p.L : (long)p.c;
  const float w_lam = (float)p.lam_before[0], w_lo = (float)p.lam_before[1], w_hi = (float)p.lam_before[2];
  const float gk = p.g_kl ? *p.g_kl : 0.0f;
  const double base = (double)gk * (double)w_lam / p.divisor * (double)(float)0.7213;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < p.items; i += (long)gridDim.x * 256) {
    long zo, oo, gs, row0, rs;
    train_slab<V, GW>(p, i, zo, oo, gs, row0, rs);
    double acc[NR];
    train_row_bits<V, GW>(p, zo, lvo, gs, acc);
    float t[NR];                           // coef * 0.7213, rounded once
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      const float k = (float)acc[j];
      // ge / eq / le of gaussian.py:91-95: a NaN row is in none of the three classes
      const float w = k > p.thr_hi ? w_hi : (k < p.thr_lo ? w_lo : ((k <= p.thr_hi && k >= p.thr_lo) ? 1.0f : 0.0f));
      t[j] = (float)(base * (double)w);
    }
    const int steps = GW ? p.dim / V : p.dim;
    for (int s = 0; s < steps; ++s) {
      const long d = GW ? (long)s * V : (long)s * gs;
      const FV<V> m = ldv<V>(p.z + zo + d), lvr = ldv<V>(p.z + zo + lvo + d);
      FV<V> gz, gsd, nz;
#pragma unroll
      for (int j = 0; j < V; ++j) { gz.v[j] = 0.0f; gsd.v[j] = 0.0f; nz.v[j] = 0.0f; }
      if (p.g_zhat) { gz = ldv<V>(p.g_zhat + oo + d); nz = ldv<V>(p.noise + oo + d); }
      if (p.g_sd) gsd = ldv<V>(p.g_sd + oo + d);
      FV<V> gm, gl;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float tj = t[GW ? 0 : j];
        const float lvraw = lvr.v[j];
        const bool inside = lvraw >= p.lv_min && lvraw <= p.lv_max;
        const float lv = train_clamp(lvraw, p.lv_min, p.lv_max);
        const float half = 0.5f * lv;
        const float hsd = 0.5f * (float)exp((double)half);
        const float var = (float)exp((double)lv);
        const float km = (tj + tj) * m.v[j];
        gm.v[j] = gz.v[j] + km;
        float a = gz.v[j] * nz.v[j];
        a = a * hsd;
        const float b = gsd.v[j] * hsd;
        const float c = tj * (var - 1.0f);
        a = a + b;
        a = a + c;
        gl.v[j] = inside ? a : 0.0f;
      }
      stv<V>(p.grad_z + zo + d, gm);
      stv<V>(p.grad_z + zo + lvo + d, gl);
    }
  }
}

}  // namespace gqhip
