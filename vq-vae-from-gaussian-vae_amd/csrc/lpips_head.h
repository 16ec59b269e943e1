// lpips_head.h -- the comparison head of LPIPS (pit/modules/lpips/loss/lpips.py: normalize_tensor, the squared difference, the
// `lin` layer's dropout and 1x1 convolution, spatial_average) for one VGG level, as one forward and one backward call on either
// module layout in place.
//
// Per pixel p of image b, over the C channels, with weights w[C], an optional keep mask m (one byte per element, layout of the
// features) and its scale s (m_c s = 1 without a mask):
//     n0 = sqrt(sum f0_c^2),  n1 = sqrt(sum f1_c^2),  r0 = 1 / (n0 + 1e-10),  r1 = 1 / (n1 + 1e-10)
//     u_c = f0_c r0 - f1_c r1,   d_p = sum_c w_c (m_c s) u_c^2,   out[b] = (1 / HW) sum_p d_p
//     t_c = -2 w_c (m_c s) u_c,  dot = sum_c t_c f1_c
//     grad_f1_j = (g[b] / HW) (r1 t_j - f1_j dot r1^2 / n1)
// At n1 = 0 the second term is 0: that is its limit (every f1_c is 0 there, so dot is 0 too), where torch's autograd gives NaN
// (sqrt's backward at 0 is 0 / 0).  The head is symmetric in (f0, f1): the gradient for f0 is the same call with the two swapped.
// Every sum, r0, r1, u, dot and the spatial sum are fp64, rounded once.  No float atomics: a tile's per-image sums go to the
// workspace, lpips_finish_kernel adds an image's tiles in an order that depends on the shape alone.
//
// A tile is T consecutive pixels of the flat [B HW] range (T = 16 or 64, by kernel); it may span several images (HW < T), so a tile
// owns `slots` partial sums, one per image it can touch.
//
// Kernels.  A feature element is loaded once per call; the second (and the backward's third) pass over a pixel's channels is
// served from registers at every C <= 512.
//   lpips_bchw_kernel<BWD, VEC, NH>   [B, C, HW]: a wave is 16 pixel lanes x 4 channel lanes, a lane holds VEC consecutive pixels
//                                     (VEC = 4: 16-byte loads, 256 contiguous bytes per channel row and wave) of the channels
//                                     q, q + 16, .. (q = 4 wave + channel lane; at most NH of them, in registers: 2 NH VEC floats).
//                                     Per-pixel sums: shuffles over the channel lanes, then the four waves through LDS.
//                                     <4, 4> C <= 64, <4, 8> C <= 128, <4, 16> C <= 256, <1, 32> every other case (T = 16: 256 blocks at 4096 pixels).
//   lpips_blc_kernel<BWD, G, NS, VEC> [B, HW, C]: G lanes share a pixel, lane k holds the chunks k, k + G, .. (NS of them, VEC floats
//                                     each) in registers; the sums go round the group with shuffles.  T = 64 (G <= 16) or 16.
//   lpips_finish_kernel               one block per image: its tiles' partial sums -> out[b].
#pragma once
#include "gq_common.h"

namespace gqhip {

constexpr int kLpipsMaxC = 512;
constexpr double kLpipsEps = 1e-10;

struct LpipsGeom {
  long P, L;        // pixels B HW, pixels per image
  int mode;         // 1: [B, C, HW]; 2: [B, HW, C]
  int C;
  int T, slots;     // pixels per tile, partial sums per tile
};

struct LpipsParams {
  const float *f0, *f1, *w;
  const unsigned char *keep;   // null: every element kept, scale 1
  float keep_scale;
  double *part;                // forward: [tiles][slots]
  float *out;                  // forward: [B]
  const float *g;              // backward: [B]
  float *grad;                 // backward: layout of f1
  LpipsGeom g_;
};

// images a tile of T pixels can touch
__host__ __device__ inline long lpips_slots(long B, long HW, long T) {
  const long s = (T + HW - 2) / HW + 1;
  return s < B ? s : B;
}

// sd[0 .. T) hold the tile's per-pixel d (published by a barrier): wave 0 writes the tile's per-image sums, a fixed butterfly each
__device__ __forceinline__ void lpips_tile_partials(const LpipsParams &p, const double *sd) {
  const LpipsGeom &g = p.g_;
  if (threadIdx.x >= 64) return;
  const int lane = threadIdx.x;
  const long p0 = (long)blockIdx.x * g.T, pix = p0 + lane;
  const long pend = p0 + g.T < g.P ? p0 + g.T : g.P;
  const long bf = p0 / g.L, bl = (pend - 1) / g.L;
  const bool live = lane < g.T && pix < pend;
  const long mine = live ? pix / g.L : -1;
  const double v = live ? sd[lane] : 0.0;
  for (long b = bf; b <= bl; ++b) {
    double s = mine == b ? v : 0.0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) p.part[(long)blockIdx.x * g.slots + (b - bf)] = s;
  }
}

template <int VEC>
struct LpipsVec;
template <>
struct LpipsVec<1> {
  static __device__ __forceinline__ void load(const float *a, float *v) { v[0] = *a; }
  static __device__ __forceinline__ void store(float *a, const float *v) { *a = v[0]; }
  static __device__ __forceinline__ void keep(const unsigned char *a, float *m) { m[0] = *a ? 1.f : 0.f; }
};
template <>
struct LpipsVec<4> {
  static __device__ __forceinline__ void load(const float *a, float *v) {
    const f32x4 x = *reinterpret_cast<const f32x4 *>(a);
    v[0] = x[0]; v[1] = x[1]; v[2] = x[2]; v[3] = x[3];
  }
  static __device__ __forceinline__ void store(float *a, const float *v) { *reinterpret_cast<f32x4 *>(a) = f32x4{v[0], v[1], v[2], v[3]}; }
  static __device__ __forceinline__ void keep(const unsigned char *a, float *m) {
    const unsigned x = *reinterpret_cast<const unsigned *>(a);
#pragma unroll
    for (int e = 0; e < 4; ++e) m[e] = ((x >> (8 * e)) & 0xffu) ? 1.f : 0.f;
  }
};

// ---- [B, C, HW] ----------------------------------------------------------------------------------------------------------------
// v[e] summed over the wave's four channel lanes, then over the four waves in order; every lane gets its pixels' totals.
// `sw`: [4][64] doubles.  Two barriers: the second frees `sw` for the next call.
template <int VEC>
__device__ __forceinline__ void lpips_bchw_combine(double *v, double *sw, int wave, int pl) {
#pragma unroll
  for (int e = 0; e < VEC; ++e) {
    v[e] += __shfl_xor(v[e], 16);
    v[e] += __shfl_xor(v[e], 32);
  }
  if ((threadIdx.x & 63) < 16) {
#pragma unroll
    for (int e = 0; e < VEC; ++e) sw[wave * 64 + pl * VEC + e] = v[e];
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < VEC; ++e) {
    const int i = pl * VEC + e;
    v[e] = (sw[i] + sw[64 + i]) + (sw[128 + i] + sw[192 + i]);
  }
  __syncthreads();
}

template <bool BWD, int VEC, int NH>
__global__ __launch_bounds__(256) void lpips_bchw_kernel(const LpipsParams p) {
  __shared__ double sw[4 * 64];
  __shared__ double sd[64];
  const LpipsGeom &g = p.g_;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, pl = lane & 15, q = wave * 4 + (lane >> 4);
  const long pix = (long)blockIdx.x * g.T + pl * VEC;   // VEC = 4: HW % 4 == 0, so the four pixels share an image and P % 4 == 0
  const bool live = pix < g.P;
  const long b = live ? pix / g.L : 0, l = live ? pix % g.L : 0;
  const long base = b * g.C * g.L + l;
  float a0[NH][VEC], a1[NH][VEC];
  double s0[VEC], s1[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) s0[e] = s1[e] = 0.0;
#pragma unroll
  for (int i = 0; i < NH; ++i) {
    const int c = q + 16 * i;
#pragma unroll
    for (int e = 0; e < VEC; ++e) a0[i][e] = a1[i][e] = 0.f;
    if (live && c < g.C) {
      LpipsVec<VEC>::load(p.f0 + base + (long)c * g.L, a0[i]);
      LpipsVec<VEC>::load(p.f1 + base + (long)c * g.L, a1[i]);
    }
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      s0[e] += (double)a0[i][e] * (double)a0[i][e];
      s1[e] += (double)a1[i][e] * (double)a1[i][e];
    }
  }
  lpips_bchw_combine<VEC>(s0, sw, wave, pl);
  lpips_bchw_combine<VEC>(s1, sw, wave, pl);
  double r0[VEC], r1[VEC], n1[VEC], acc[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) {
    n1[e] = sqrt(s1[e]);
    r0[e] = 1.0 / (sqrt(s0[e]) + kLpipsEps);
    r1[e] = 1.0 / (n1[e] + kLpipsEps);
    acc[e] = 0.0;
  }
  // second pass, from registers: d (forward) or dot (backward)
#pragma unroll
  for (int i = 0; i < NH; ++i) {
    const int c = q + 16 * i;
    if (live && c < g.C) {
      float m[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) m[e] = 1.f;
      if (p.keep) LpipsVec<VEC>::keep(p.keep + base + (long)c * g.L, m);
      const double wc = (double)p.w[c] * (p.keep ? (double)p.keep_scale : 1.0);
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const double u = (double)a0[i][e] * r0[e] - (double)a1[i][e] * r1[e];
        const double wm = wc * (double)m[e];
        acc[e] += BWD ? (-2.0 * wm * u) * (double)a1[i][e] : wm * u * u;
      }
    }
  }
  lpips_bchw_combine<VEC>(acc, sw, wave, pl);
  if (!BWD) {
    if (lane < 16 && wave == 0) {
#pragma unroll
      for (int e = 0; e < VEC; ++e) sd[pl * VEC + e] = live ? acc[e] : 0.0;
    }
    __syncthreads();
    lpips_tile_partials(p, sd);
    return;
  }
  if (!live) return;
  const double gs = (double)p.g[b] / (double)g.L;
  double k[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) k[e] = n1[e] > 0.0 ? acc[e] * r1[e] * r1[e] / n1[e] : 0.0;
#pragma unroll
  for (int i = 0; i < NH; ++i) {
    const int c = q + 16 * i;
    if (c < g.C) {
      float m[VEC], o[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) m[e] = 1.f;
      if (p.keep) LpipsVec<VEC>::keep(p.keep + base + (long)c * g.L, m);
      const double wc = (double)p.w[c] * (p.keep ? (double)p.keep_scale : 1.0);
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const double u = (double)a0[i][e] * r0[e] - (double)a1[i][e] * r1[e];
        const double t = -2.0 * (wc * (double)m[e]) * u;
        o[e] = (float)(gs * (r1[e] * t - (double)a1[i][e] * k[e]));
      }
      LpipsVec<VEC>::store(p.grad + base + (long)c * g.L, o);
    }
  }
}

// ---- [B, HW, C] ----------------------------------------------------------------------------------------------------------------
template <bool BWD, int G, int NS, int VEC>
__global__ __launch_bounds__(256) void lpips_blc_kernel(const LpipsParams p) {
  constexpr int RPB = 256 / G;
  __shared__ double sd[64];
  const LpipsGeom &g = p.g_;
  const int tid = threadIdx.x, k = tid % G, rloc = tid / G;
  const int units = g.C / VEC;                       // VEC = 4: C % 4 == 0
  const double ks = p.keep ? (double)p.keep_scale : 1.0;
  float wv[NS][VEC];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int c = k + G * s;
#pragma unroll
    for (int e = 0; e < VEC; ++e) wv[s][e] = 0.f;
    if (c < units) LpipsVec<VEC>::load(p.w + c * VEC, wv[s]);
  }
  const long p0 = (long)blockIdx.x * g.T;
  for (int r0i = 0; r0i < g.T; r0i += RPB) {
    const int pin = r0i + rloc;                      // pixel of the tile
    const long pix = p0 + pin;
    const bool live = pin < g.T && pix < g.P;
    const long base = pix * g.C;
    float a0[NS][VEC], a1[NS][VEC];
    double s0 = 0.0, s1 = 0.0;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const int c = k + G * s;
#pragma unroll
      for (int e = 0; e < VEC; ++e) a0[s][e] = a1[s][e] = 0.f;
      if (live && c < units) {
        LpipsVec<VEC>::load(p.f0 + base + c * VEC, a0[s]);
        LpipsVec<VEC>::load(p.f1 + base + c * VEC, a1[s]);
      }
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        s0 += (double)a0[s][e] * (double)a0[s][e];
        s1 += (double)a1[s][e] * (double)a1[s][e];
      }
    }
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) {
      s0 += __shfl_xor(s0, o);
      s1 += __shfl_xor(s1, o);
    }
    const double n1 = sqrt(s1), r0 = 1.0 / (sqrt(s0) + kLpipsEps), r1 = 1.0 / (n1 + kLpipsEps);
    float m[NS][VEC];
    double acc = 0.0;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const int c = k + G * s;
#pragma unroll
      for (int e = 0; e < VEC; ++e) m[s][e] = 1.f;
      if (p.keep && live && c < units) LpipsVec<VEC>::keep(p.keep + base + c * VEC, m[s]);
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const double u = (double)a0[s][e] * r0 - (double)a1[s][e] * r1;
        const double wm = (double)wv[s][e] * ks * (double)m[s][e];
        acc += BWD ? (-2.0 * wm * u) * (double)a1[s][e] : wm * u * u;
      }
    }
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (!BWD) {
      if (k == 0 && pin < g.T) sd[pin] = live ? acc : 0.0;
      continue;
    }
    if (!live) continue;
    const double gs = (double)p.g[pix / g.L] / (double)g.L;
    const double kk = n1 > 0.0 ? acc * r1 * r1 / n1 : 0.0;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const int c = k + G * s;
      if (c < units) {
        float o[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          const double u = (double)a0[s][e] * r0 - (double)a1[s][e] * r1;
          const double t = -2.0 * ((double)wv[s][e] * ks * (double)m[s][e]) * u;
          o[e] = (float)(gs * (r1 * t - (double)a1[s][e] * kk));
        }
        LpipsVec<VEC>::store(p.grad + base + c * VEC, o);
      }
    }
  }
  if (!BWD) {
    __syncthreads();
    lpips_tile_partials(p, sd);
  }
}

// one block of 256 threads per image: thread i adds the image's tiles i, i + 256, .. in order, then a fixed tree over the block
__global__ __launch_bounds__(256) void lpips_finish_kernel(const LpipsParams p) {
  __shared__ double sh[4];
  const LpipsGeom &g = p.g_;
  const long b = blockIdx.x;
  const long t0 = b * g.L / g.T, t1 = ((b + 1) * g.L - 1) / g.T;
  double v = 0.0;
  for (long t = t0 + threadIdx.x; t <= t1; t += 256) v += p.part[t * g.slots + (b - t * g.T / g.L)];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) p.out[b] = (float)(((sh[0] + sh[1]) + (sh[2] + sh[3])) / (double)g.L);
}

}  // namespace gqhip
