// bsq_fsq_train.h -- the train steps of BSQQuantizer (pit/quantization/bsq.py:14-37, 64-133) and FSQQuantizer
// (pit/quantization/fsq.py:6-9, 29-68), each as one forward and one backward call on either module layout in place.
//
// BSQ.  A position (b, l) holds C = 16 d channels; channel i d + j is codebook i, bit plane j.  With n = ||x||_2 over the channels
// (summed in fp64), u = fl32(x / max(n, 1e-12)), q = u > 0 ? 1 : -1, q_scale = 1 / sqrt(C):
//     quantized = fl(fl(u + fl(q - u)) q_scale)          idx[j] = sum_i bit(i, j) << (15 - i)
//     s = -400 u / sqrt(C),  p = sigma(s),  e = exp(-|s|): larger of (p, 1 - p) = 1 / (1 + e), smaller = e / (1 + e)
//     h(p) = -p log(p + eps) - (1 - p) log(1 - p + eps),  eps = 1e-5 (inside a plain log: it does not cancel)
//     per_sample_entropy = (1 / M) sum h,  M = B L 16;   avg[j] = (mean of p, mean of 1 - p) over bit plane j, each summed on its own
//     codebook_entropy = -sum_j (a log(a + eps) + b log(b + eps)) at (a, b) = avg[j]
// Backward, recomputing u, p, q from x:
//     g_u = q_scale g_q + g_aux (-400 / sqrt(C)) p (1 - p) ((w_s / M) h'(p) - (w_b / M) A'_j)
//     h'(p) = -log(p + eps) - p / (p + eps) + log(1 - p + eps) + (1 - p) / (1 - p + eps),  A'_j = the same at avg[j]
//     grad_x = (g_u - u (u . g_u)) / n   when n >= 1e-12,   g_u / 1e-12 otherwise (clamp_min's backward)
// Every entropy term, sum and the projection are fp64, rounded once.  No float atomics: a block's sums are a fixed tree, the
// blocks' partials (2 d + 1 doubles each) are added by bsq_finish_kernel in an order that depends on the shape alone.
//
// Kernels:
//   bsq_fwd_blc_kernel<G, NS>   [B, L, C]: G lanes share a row, lane k holds the 16-byte chunks k, k + G, .. (NS of them) in
//                               registers; the row sums go round the group with shuffles.  A lane meets the same channels in every
//                               row, so its running sums are per channel; they are folded to bit planes once, at the block's end.
//                               The sign bits pass through LDS to the threads that pack the d indices of a row.
//   bsq_fwd_bchw_kernel         [B, C, L]: one thread per position in blocks of one wave, coalesced along L; a first pass for n,
//                               then bit plane by bit plane (x is re-read: it is cache-resident), each plane's two sums reduced
//                               over the block.
//   bsq_finish_kernel           one block: the partials -> avg and the three scalars.
//   bsq_bwd_blc_kernel<G, NS>, bsq_bwd_bchw_kernel   the same two mappings; one launch.
//
// FSQ.  Per channel with L levels: half_l = (L - 1)(1 + 1e-3) / 2, offset = L even ? 0.5 : 0, shift = atanh(offset / half_l),
// b = tanh(z + shift) half_l - offset (fsq_quantize_kernel's arithmetic: tanh / atanh in fp64, rounded once), r = rint(b),
//     zhat = fl(fl(b + fl(r - b)) / half_width)   (round_ste's value),   idx = mixed-radix pack of r + half_width
//     grad_z = g_zhat (half_l / half_width) sech^2(z + shift),  sech^2 t = 4 e / (1 + e)^2 with e = exp(-2 |t|), in fp64.
#pragma once
#include "gq_aux.h"
#include "gq_common.h"

namespace gqhip {

constexpr int kBsqMaxD = 16;
constexpr int kBsqMaxBlocks = 1024;   // partial records of a forward (the finish kernel reads them all)
constexpr double kBsqEps = 1e-5;
constexpr double kBsqNormMin = 1e-12;
constexpr int kBsqBchwThreads = 64;   // one position per thread: small blocks, so that 16 384 positions already fill the CUs

struct BsqGeom {
  long P, L;        // positions B L, positions per image
  int d, C;
  int mode;         // 1: [B, C, L]; 2: [B, L, C]
  int iters;        // row groups (blc) / position tiles (bchw) a block walks
  int blocks;
  float q_scale;    // fl32(1 / sqrt(C)): the forward's factor
  double cs;        // -400 / sqrt(C)
  double M;         // B L 16
};

// (p, 1 - p) = (sigma(s), sigma(-s)) without cancellation
__device__ __forceinline__ void bsq_prob(double s, double &p, double &om) {
  const double e = exp(-fabs(s));
  const double big = 1.0 / (1.0 + e), small = e / (1.0 + e);
  p = s > 0.0 ? big : small;
  om = s > 0.0 ? small : big;
}

__device__ __forceinline__ double bsq_h(double p, double om) { return -p * log(p + kBsqEps) - om * log(om + kBsqEps); }

__device__ __forceinline__ double bsq_dh(double p, double om) {
  return -log(p + kBsqEps) - p / (p + kBsqEps) + log(om + kBsqEps) + om / (om + kBsqEps);
}

// sum over the block's WAVES * 64 threads in a fixed tree (wave butterfly, then the waves in order); every thread gets the result
template <int WAVES>
__device__ __forceinline__ double bsq_block_sum(double v, double *shw) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if (WAVES == 1) return v;
  if ((threadIdx.x & 63) == 0) shw[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = shw[0];
#pragma unroll
  for (int w = 1; w < WAVES; ++w) r += shw[w];
  __syncthreads();
  return r;
}

struct BsqFwdParams {
  const float *x;
  float *quant;
  int64_t *idx;
  double *part;      // [blocks][2 d + 1]: per bit plane (sum p, sum 1 - p), then sum h
  float *avg;        // [d][2]
  float *scalars;    // entropy_aux_loss, per_sample_entropy, codebook_entropy
  BsqGeom g;
  float ws, wb;
};

template <int G, int NS>
__global__ __launch_bounds__(256) void bsq_fwd_blc_kernel(const BsqFwdParams p) {
  constexpr int RPB = 256 / G;
  __shared__ unsigned char sbit[RPB][G * NS];       // the four sign bits of each 16-byte chunk
  __shared__ double sacc[4][2][64 * NS];            // per wave, per channel: sum p, sum 1 - p
  __shared__ double sh4[4];
  const BsqGeom &g = p.g;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, k = tid % G, rloc = tid / G;
  const int C4 = g.C >> 2;
  double ap[NS][4], aq[NS][4], ent = 0.0;
#pragma unroll
  for (int s = 0; s < NS; ++s)
#pragma unroll
    for (int e = 0; e < 4; ++e) ap[s][e] = aq[s][e] = 0.0;
  for (int it = 0; it < g.iters; ++it) {
    const long row0 = ((long)blockIdx.x * g.iters + it) * RPB;
    const long row = row0 + rloc;
    const bool live = row < g.P;
    f32x4 xv[NS];
    double ss = 0.0;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const int c = k + G * s;
      xv[s] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (live && c < C4) xv[s] = *reinterpret_cast<const f32x4 *>(p.x + row * g.C + 4 * c);
#pragma unroll
      for (int e = 0; e < 4; ++e) ss += (double)xv[s][e] * (double)xv[s][e];
    }
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
    const double den = fmax(sqrt(ss), kBsqNormMin);
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const int c = k + G * s;
      const bool ok = live && c < C4;
      unsigned nib = 0;
      f32x4 qv;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float u = (float)((double)xv[s][e] / den);
        const bool bit = u > 0.0f;
        const float q = bit ? 1.0f : -1.0f;
        const float t = q - u;
        qv[e] = (u + t) * g.q_scale;
        nib |= (bit ? 1u : 0u) << e;
        double pp, om;
        bsq_prob(g.cs * (double)u, pp, om);
        if (ok) {
          ap[s][e] += pp;
          aq[s][e] += om;
          ent += bsq_h(pp, om);
        }
      }
      if (ok) {
        *reinterpret_cast<f32x4 *>(p.quant + row * g.C + 4 * c) = qv;
        sbit[rloc][c] = (unsigned char)nib;
      }
    }
    __syncthreads();
    for (int o = tid; o < RPB * g.d; o += 256) {
      const int r = o / g.d, j = o % g.d;
      if (row0 + r < g.P) {
        int64_t v = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int ch = i * g.d + j;
          v = v * 2 + ((sbit[r][ch >> 2] >> (ch & 3)) & 1);
        }
        p.idx[(row0 + r) * g.d + j] = v;
      }
    }
    __syncthreads();
  }
  // lanes k, k + G, .. of a wave hold the same channels
#pragma unroll
  for (int s = 0; s < NS; ++s)
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int o = G; o < 64; o <<= 1) {
        ap[s][e] += __shfl_xor(ap[s][e], o);
        aq[s][e] += __shfl_xor(aq[s][e], o);
      }
  if (lane < G) {
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const int c = k + G * s;
      if (c < C4) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          sacc[wave][0][4 * c + e] = ap[s][e];
          sacc[wave][1][4 * c + e] = aq[s][e];
        }
      }
    }
  }
  ent = bsq_block_sum<4>(ent, sh4);                 // its barriers also publish sacc
  double *dst = p.part + (long)blockIdx.x * (2 * g.d + 1);
  if (tid < 2 * g.d) {
    const int j = tid >> 1, which = tid & 1;
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int ch = i * g.d + j;
      s += (sacc[0][which][ch] + sacc[1][which][ch]) + (sacc[2][which][ch] + sacc[3][which][ch]);
    }
    dst[tid] = s;
  }
  if (tid == 0) dst[2 * g.d] = ent;
}

__global__ __launch_bounds__(kBsqBchwThreads) void bsq_fwd_bchw_kernel(const BsqFwdParams p) {
  constexpr int WAVES = kBsqBchwThreads / 64;
  __shared__ double sh4[WAVES];
  __shared__ double stot[2 * kBsqMaxD + 1];
  const BsqGeom &g = p.g;
  const int tid = threadIdx.x;
  if (tid < 2 * g.d + 1) stot[tid] = 0.0;
  __syncthreads();
  double ent = 0.0;
  for (int it = 0; it < g.iters; ++it) {
    const long pos = ((long)blockIdx.x * g.iters + it) * kBsqBchwThreads + tid;
    const bool live = pos < g.P;
    const long b = live ? pos / g.L : 0, l = live ? pos % g.L : 0;
    const float *xb = p.x + b * g.C * g.L + l;
    float *qb = p.quant + b * g.C * g.L + l;
    double ss = 0.0;
    if (live)
      for (int ch = 0; ch < g.C; ++ch) {
        const double x = (double)xb[(long)ch * g.L];
        ss += x * x;
      }
    const double den = fmax(sqrt(ss), kBsqNormMin);
    for (int j = 0; j < g.d; ++j) {
      double sp = 0.0, sq = 0.0;
      if (live) {
        int64_t v = 0;
#pragma unroll 4
        for (int i = 0; i < 16; ++i) {
          const long o = (long)(i * g.d + j) * g.L;
          const float u = (float)((double)xb[o] / den);
          const bool bit = u > 0.0f;
          const float q = bit ? 1.0f : -1.0f;
          const float t = q - u;
          qb[o] = (u + t) * g.q_scale;
          v = v * 2 + (bit ? 1 : 0);
          double pp, om;
          bsq_prob(g.cs * (double)u, pp, om);
          sp += pp;
          sq += om;
          ent += bsq_h(pp, om);
        }
        p.idx[(b * g.d + j) * g.L + l] = v;
      }
      sp = bsq_block_sum<WAVES>(sp, sh4);
      sq = bsq_block_sum<WAVES>(sq, sh4);
      if (tid == 0) {
        stot[2 * j] += sp;
        stot[2 * j + 1] += sq;
      }
    }
  }
  ent = bsq_block_sum<WAVES>(ent, sh4);
  if (tid == 0) stot[2 * g.d] = ent;
  __syncthreads();
  if (tid < 2 * g.d + 1) p.part[(long)blockIdx.x * (2 * g.d + 1) + tid] = stot[tid];
}

// one block of 256 threads: sum s of the 2 d + 1 is added over the blocks in `slices` interleaved runs, then the runs in order
__global__ __launch_bounds__(256) void bsq_finish_kernel(const BsqFwdParams p) {
  __shared__ double sh[256];
  __shared__ double tot[64];
  const BsqGeom &g = p.g;
  const int tid = threadIdx.x, nsum = 2 * g.d + 1;
  int pad = 4;
  while (pad < nsum) pad <<= 1;
  const int slices = 256 / pad, s = tid % pad, sl = tid / pad;
  double a = 0.0;
  if (s < nsum)
    for (int b = sl; b < g.blocks; b += slices) a += p.part[(long)b * nsum + s];
  sh[tid] = a;
  __syncthreads();
  if (tid < nsum) {
    double t = 0.0;
    for (int i = 0; i < slices; ++i) t += sh[i * pad + tid];
    tot[tid] = t;
  }
  __syncthreads();
  if (tid == 0) {
    double ce = 0.0;
    for (int i = 0; i < 2 * g.d; ++i) {
      const double m = tot[i] / g.M;
      p.avg[i] = (float)m;
      ce -= m * log(m + kBsqEps);
    }
    const double se = tot[2 * g.d] / g.M;
    p.scalars[0] = (float)((double)p.ws * se - (double)p.wb * ce);
    p.scalars[1] = (float)se;
    p.scalars[2] = (float)ce;
  }
}

// ---- backward ------------------------------------------------------------------------------------------------------------------
struct BsqBwdParams {
  const float *x, *avg;
  const float *g_q, *g_aux;   // each may be null (zero)
  float *grad_x;
  BsqGeom g;
  float ws, wb;
};

// A'_j of every bit plane into LDS (the caller synchronises)
__device__ __forceinline__ void bsq_plane_terms(const BsqBwdParams &p, double *sA) {
  if ((int)threadIdx.x < p.g.d) sA[threadIdx.x] = bsq_dh((double)p.avg[2 * threadIdx.x], (double)p.avg[2 * threadIdx.x + 1]);
}

// g_u of one element; ca = g_aux (-400 / sqrt(C)) / M or 0
__device__ __forceinline__ double bsq_gu(const BsqBwdParams &p, float u, float gq, double ca, double Aj) {
  double v = (1.0 / sqrt((double)p.g.C)) * (double)gq;
  if (p.g_aux) {
    double pp, om;
    bsq_prob(p.g.cs * (double)u, pp, om);
    v += ca * (pp * om) * ((double)p.ws * bsq_dh(pp, om) - (double)p.wb * Aj);
  }
  return v;
}

template <int G, int NS>
__global__ __launch_bounds__(256) void bsq_bwd_blc_kernel(const BsqBwdParams p) {
  constexpr int RPB = 256 / G;
  __shared__ double sA[kBsqMaxD];
  const BsqGeom &g = p.g;
  const int tid = threadIdx.x, k = tid % G, rloc = tid / G;
  const int C4 = g.C >> 2;
  bsq_plane_terms(p, sA);
  __syncthreads();
  const double ca = p.g_aux ? (double)*p.g_aux * g.cs / g.M : 0.0;
  for (int it = 0; it < g.iters; ++it) {
    const long row = ((long)blockIdx.x * g.iters + it) * RPB + rloc;
    const bool live = row < g.P;
    f32x4 xv[NS];
    double ss = 0.0;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const int c = k + G * s;
      xv[s] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (live && c < C4) xv[s] = *reinterpret_cast<const f32x4 *>(p.x + row * g.C + 4 * c);
#pragma unroll
      for (int e = 0; e < 4; ++e) ss += (double)xv[s][e] * (double)xv[s][e];
    }
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
    const double nrm = sqrt(ss), den = fmax(nrm, kBsqNormMin);
    double gu[NS][4], dot = 0.0;
    float uu[NS][4];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const int c = k + G * s;
      const bool ok = live && c < C4;
      f32x4 gq = f32x4{0.f, 0.f, 0.f, 0.f};
      if (ok && p.g_q) gq = *reinterpret_cast<const f32x4 *>(p.g_q + row * g.C + 4 * c);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float u = (float)((double)xv[s][e] / den);
        const int j = ok ? (4 * c + e) % g.d : 0;
        const double v = ok ? bsq_gu(p, u, gq[e], ca, sA[j]) : 0.0;
        uu[s][e] = u;
        gu[s][e] = v;
        dot += (double)u * v;
      }
    }
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) dot += __shfl_xor(dot, o);
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const int c = k + G * s;
      if (!(live && c < C4)) continue;
      f32x4 out;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        out[e] = (float)(nrm >= kBsqNormMin ? (gu[s][e] - (double)uu[s][e] * dot) / nrm : gu[s][e] / kBsqNormMin);
      *reinterpret_cast<f32x4 *>(p.grad_x + row * g.C + 4 * c) = out;
    }
  }
}

__global__ __launch_bounds__(kBsqBchwThreads) void bsq_bwd_bchw_kernel(const BsqBwdParams p) {
  __shared__ double sA[kBsqMaxD];
  const BsqGeom &g = p.g;
  bsq_plane_terms(p, sA);
  __syncthreads();
  const long pos = (long)blockIdx.x * kBsqBchwThreads + threadIdx.x;
  if (pos >= g.P) return;
  const double ca = p.g_aux ? (double)*p.g_aux * g.cs / g.M : 0.0;
  const long base = (pos / g.L) * g.C * g.L + pos % g.L;
  const float *xb = p.x + base;
  const float *gb = p.g_q ? p.g_q + base : nullptr;
  double ss = 0.0;
  for (int ch = 0; ch < g.C; ++ch) {
    const double x = (double)xb[(long)ch * g.L];
    ss += x * x;
  }
  const double nrm = sqrt(ss), den = fmax(nrm, kBsqNormMin);
  double dot = 0.0;
  for (int i = 0; i < 16; ++i)
    for (int j = 0; j < g.d; ++j) {
      const long o = (long)(i * g.d + j) * g.L;
      const float u = (float)((double)xb[o] / den);
      dot += (double)u * bsq_gu(p, u, gb ? gb[o] : 0.0f, ca, sA[j]);
    }
  for (int i = 0; i < 16; ++i)
    for (int j = 0; j < g.d; ++j) {
      const long o = (long)(i * g.d + j) * g.L;
      const float u = (float)((double)xb[o] / den);
      const double v = bsq_gu(p, u, gb ? gb[o] : 0.0f, ca, sA[j]);
      p.grad_x[base + o] = (float)(nrm >= kBsqNormMin ? (v - (double)u * dot) / nrm : v / kBsqNormMin);
    }
}

// ---- FSQ -----------------------------------------------------------------------------------------------------------------------
struct FsqTrainParams {
  const float *z, *g_zhat;
  float *out;          // zhat (forward) / grad_z (backward)
  int32_t *idx;
  long P, L;           // positions B L, positions per image
  int mode;            // 1: [B, n, L]; 2: [B, L, n]
  FsqLevels lv;
};

__device__ __forceinline__ void fsq_level_consts(int lv, float &half_l, float &offset, float &shift) {
#pragma clang fp contract(off)
  half_l = (float)(lv - 1) * (1.0f + 1e-3f) / 2.0f;
  offset = (lv % 2 == 0) ? 0.5f : 0.0f;
  shift = (float)atanh((double)(offset / half_l));
}

// one thread per position
__global__ __launch_bounds__(256) void fsq_train_kernel(const FsqTrainParams p) {
#pragma clang fp contract(off)
  const long pos = (long)blockIdx.x * 256 + threadIdx.x;
  if (pos >= p.P) return;
  const int n = p.lv.n;
  const long base = p.mode == 1 ? (pos / p.L) * n * p.L + pos % p.L : pos * n;
  const long stride = p.mode == 1 ? p.L : 1;
  int packed = 0;
  for (int l = 0; l < n; ++l) {
    const int lv = p.lv.lev[l];
    float half_l, offset, shift;
    fsq_level_consts(lv, half_l, offset, shift);
    const float x = p.z[base + l * stride] + shift;
    const float b = (float)tanh((double)x) * half_l - offset;
    const float r = rintf(b);
    const int hw = lv / 2;
    const float t = r - b;
    p.out[base + l * stride] = (b + t) / (float)hw;
    packed = packed * lv + (int)(r + (float)hw);
  }
  p.idx[pos] = packed;
}

// one thread per element
__global__ __launch_bounds__(256) void fsq_backward_kernel(const FsqTrainParams p) {
  const int n = p.lv.n;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= p.P * n) return;
  const int l = p.mode == 1 ? (int)((e / p.L) % n) : (int)(e % n);
  const int lv = p.lv.lev[l];
  float half_l, offset, shift;
  fsq_level_consts(lv, half_l, offset, shift);
  const double t = (double)p.z[e] + (double)shift;
  const double ex = exp(-2.0 * fabs(t));
  const double sech2 = 4.0 * ex / ((1.0 + ex) * (1.0 + ex));
  p.out[e] = (float)((double)p.g_zhat[e] * ((double)half_l / (double)(lv / 2)) * sech2);
}

}  // namespace gqhip
