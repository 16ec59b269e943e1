// lfq_train.h -- the train step of LFQQuantizer (pit/quantization/lfq.py:56-76, 160-208) without the [rows, 2^d] logits matrix.
//
// Row r = (b L + l) nc + ci holds the d channels ci d + i of position (b, l).  The codebook is the whole product set {-1,+1}^d
// (code j has value +1 in dimension i when bit i of j is set), so the row's softmax over the 2^d codes at temperature T = 0.01 is
// a product of d independent Bernoullis: with s_i = 4 x_i / T = 400 x_i,
//     P_r[j] = prod_i (bit_i(j) ? p_i : q_i),   p_i = sigma(s_i),   q_i = sigma(-s_i)
// computed as e = exp(-|s|), larger = 1 / (1 + e), smaller = e / (1 + e).
//   sample entropy of a row  = sum_i H_b(i),  H_b = log1p(e) + |s| e / (1 + e)        (no 0 log 0: e underflows to 0, H_b to 0)
//   Split the bits: the low dl = d / 2 bits index v, the high dh = d - dl bits index u, j = u 2^dl + v.  With the per-row tables
//   A_r[u] = prod over the high bits, B_r[v] = prod over the low bits:  P_r[u, v] = A_r[u] B_r[v], so
//     avg[u, v] = (1 / R) sum_r A_r[u] B_r[v]          a 2^dh x R x 2^dl GEMM on v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32
//                                                       accumulation in program order)
//   codebook entropy = -sum avg log(avg + eps)          (the eps inside log_softmax shifts every logit alike and cancels)
// Backward, G[u, v] = -(log(avg + eps) + avg / (avg + eps)):
//   d codebook_entropy / d s_i = (1 / R) sum_u (G B_r)[u] A_r[u] (bit_i(u) ? q_i : -p_i)     for a high bit (low bits: G^T A_r, B_r)
//   d H_b / d s = -s p q
//   grad_x = g_q + g_commit 2 (x - q) / numel + g_aux 400 (w_s / R (-s p q) - w_b d codebook_entropy / d s)
//
// Kernels (no float atomics; the order of every sum depends on the shape alone, so results are bit-identical from run to run):
//   lfq_elem_kernel      one thread per position: quantized = x + (q - x), the big-endian index of all nc d sign bits, and the
//                        block's partial sums (fp64 terms, fixed tree) of H_b and (x - q)^2.
//   lfq_avg_gemm_kernel  grid (chunks of kLfqChunk rows, output tiles): builds the A and B tiles of kLfqKStep rows in LDS from the
//                        rows' probabilities (doubling: one multiply per entry and level) and accumulates A^T B, a step in the
//                        matrix core's fp32, the chunk's steps in fp64; the chunk's partial tile goes to the workspace as fp32.
//   lfq_avg_reduce_kernel adds the chunks' partials in chunk order (fp64), writes avg and per-block partial sums of -avg log(avg+eps).
//   lfq_finish_kernel    one block: the four scalars.
//   lfq_g_kernel         G and its transpose into the workspace.
//   lfq_bwd_kernel       a wave owns 32 rows: two passes of Out[m][row] = sum_k Mat[k][m] Tab_row[k] on the same MFMA, with
//                        (Mat, Tab) = (G^T, B) then (G, A); Mat is streamed through LDS in slabs of 32 k (16-byte copies where a slab is whole rows); the wave contracts Out
//                        with the other table and the per-bit factors in registers, then writes grad_x.
// Tables are padded to the tile sizes with "bits" whose factors are (set: 0, clear: 1): padded entries are exact zeros.
#pragma once
#include "gq_common.h"

namespace gqhip {

constexpr int kLfqChunk = 256;       // rows per partial avg tile (part of the value contract: the order of the sum over rows)
constexpr int kLfqKStep = 32;        // rows per table step of the forward GEMM
constexpr int kLfqMaxD = 16;
constexpr int kLfqBwdWaves = 2;      // waves (of 32 rows each) per block of lfq_bwd_kernel
constexpr float kLfqScale = 400.0f;  // 4 / T
constexpr double kLfqEps = 1e-5;

struct LfqGeom {
  long P, R, L;        // positions B L, rows P nc, positions per image
  int nc, d, dh, dl, C;
  int mode;            // 1: x is [B, C, L]; 2: [B, L, C]
};

__device__ __forceinline__ long lfq_off(const LfqGeom &g, long p, int ch) {
  if (g.mode == 1) return ((p / g.L) * g.C + ch) * g.L + p % g.L;
  return p * g.C + ch;
}

// (P(bit set), P(bit clear)) of one value
__device__ __forceinline__ void lfq_prob(float x, float &p1, float &p0) {
  const float s = kLfqScale * x;
  const float e = expf(-fabsf(s));
  const float ope = 1.0f + e;
  const float big = 1.0f / ope, small = e / ope;
  p1 = s > 0.0f ? big : small;
  p0 = s > 0.0f ? small : big;
}

// block-wide sum of one double per thread in a fixed tree; the result is valid in thread 0
template <int THREADS>
__device__ __forceinline__ double lfq_block_sum(double v, double *sh) {
  const int tid = threadIdx.x;
  sh[tid] = v;
  __syncthreads();
#pragma unroll
  for (int o = THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) sh[tid] += sh[tid + o];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}

struct LfqFwdParams {
  const float *x;
  float *quant;
  int64_t *idx;
  double *elem_part;   // [elem_blocks][2]: sum of H_b, sum of (x - q)^2
  float *part;         // [chunks][Mpad][Npad]
  float *avg;          // [2^d]
  double *ent_part;    // [avg_blocks]
  float *scalars;      // entropy_aux_loss, per_sample_entropy, codebook_entropy, commit_loss
  LfqGeom g;
  float ws, wb;
  int chunks, Mpad, Npad, elem_blocks, avg_blocks;
};

__global__ __launch_bounds__(256) void lfq_elem_kernel(const LfqFwdParams p) {
  __shared__ double sh[256];
  const LfqGeom &g = p.g;
  const long pos = (long)blockIdx.x * 256 + threadIdx.x;
  double ent = 0.0, com = 0.0;
  if (pos < g.P) {
    int64_t v = 0;
    for (int ch = 0; ch < g.C; ++ch) {
      const long o = lfq_off(g, pos, ch);
      const float x = p.x[o];
      const bool bit = x > 0.0f;
      const float q = bit ? 1.0f : -1.0f;
      v = v * 2 + (bit ? 1 : 0);
      const float t = q - x;
      p.quant[o] = x + t;
      const double a = fabs(400.0 * (double)x);                  // fp64: the two sums are rounded once, in lfq_finish_kernel
      const double e = exp(-a);
      ent += log1p(e) + a * e / (1.0 + e);
      const double diff = (double)x - (double)q;
      com += diff * diff;
    }
    p.idx[pos] = v;
  }
  ent = lfq_block_sum<256>(ent, sh);
  com = lfq_block_sum<256>(com, sh);
  if (threadIdx.x == 0) {
    p.elem_part[2 * blockIdx.x] = ent;
    p.elem_part[2 * blockIdx.x + 1] = com;
  }
}

// Padded factor slots of one row: slot b < nb is bit `first + b` of the row (channel ci d + first + b), the others are (set 0,
// clear 1).  A row >= R gets (0, 0) in slot 0: its whole table is zero.
__device__ __forceinline__ void lfq_slot(const float *x, const LfqGeom &g, long row, int first, int nb, int b, float &f1, float &f0) {
  f1 = 0.0f;
  f0 = 1.0f;
  if (row >= g.R) {
    if (b == 0) f0 = 0.0f;
    return;
  }
  if (b < nb) lfq_prob(x[lfq_off(g, row / g.nc, (int)(row % g.nc) * g.d + first + b)], f1, f0);
}

// the 2^NB table entries of NB consecutive slots, times `base`: out[e] = base prod_b (bit_b(e) ? f1[b] : f0[b])
template <int NB>
__device__ __forceinline__ void lfq_double(float base, const float *f1, const float *f0, float (&out)[1 << NB]) {
  out[0] = base;
#pragma unroll
  for (int b = 0; b < NB; ++b) {
#pragma unroll
    for (int e = 0; e < (1 << b); ++e) {
      out[e + (1 << b)] = out[e] * f1[b];
      out[e] = out[e] * f0[b];
    }
  }
}

// grid (chunks, tiles_m * tiles_n), 256 threads: waves 2 x 2, each W x W MFMA tiles; block tile T x T, T = 64 W
template <int W>
__global__ __launch_bounds__(256) void lfq_avg_gemm_kernel(const LfqFwdParams p) {
  constexpr int T = 64 * W, SEG = T / 8, NB = W == 2 ? 4 : 3;       // a thread builds SEG = 2^NB consecutive entries of a row
  __shared__ float sA[kLfqKStep][T], sB[kLfqKStep][T];
  __shared__ float fA1[kLfqKStep][8], fA0[kLfqKStep][8], fB1[kLfqKStep][8], fB0[kLfqKStep][8];
  const LfqGeom &g = p.g;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hi = lane >> 5, r = lane & 31;
  const int wm = wave >> 1, wn = wave & 1;
  const int tiles_n = p.Npad / T;
  const int m0 = (blockIdx.y / tiles_n) * T, n0 = (blockIdx.y % tiles_n) * T;
  const long row0 = (long)blockIdx.x * kLfqChunk;
  f32x16 acc[W][W];            // one step's kLfqKStep rows, in the matrix core's fp32 ...
  double sum[W][W][16];        // ... the steps of the chunk in fp64: the fp32 running sum never gets longer than kLfqKStep rows
#pragma unroll
  for (int i = 0; i < W; ++i)
#pragma unroll
    for (int j = 0; j < W; ++j)
#pragma unroll
      for (int c = 0; c < 16; ++c) {
        acc[i][j][c] = 0.f;
        sum[i][j][c] = 0.0;
      }
  const int trow = tid >> 3, seg = tid & 7;
  for (int step = 0; step < kLfqChunk / kLfqKStep; ++step) {
    {  // thread (row, slot): one slot of the high table and one of the low table
      const long row = row0 + step * kLfqKStep + trow;
      float f1, f0;
      lfq_slot(p.x, g, row, g.dl, g.dh, seg, f1, f0);
      fA1[trow][seg] = f1; fA0[trow][seg] = f0;
      lfq_slot(p.x, g, row, 0, g.dl, seg, f1, f0);
      fB1[trow][seg] = f1; fB0[trow][seg] = f0;
    }
    __syncthreads();
    {  // thread (row, segment): entries [m0 + seg SEG, + SEG) of A and [n0 + seg SEG, + SEG) of B
      float out[SEG];
      float base = 1.0f;
      const int ua = m0 + seg * SEG, ub = n0 + seg * SEG;
#pragma unroll
      for (int b = NB; b < 8; ++b) base *= ((ua >> b) & 1) ? fA1[trow][b] : fA0[trow][b];
      lfq_double<NB>(base, fA1[trow], fA0[trow], out);
#pragma unroll
      for (int e = 0; e < SEG; ++e) sA[trow][seg * SEG + e] = out[e];
      base = 1.0f;
#pragma unroll
      for (int b = NB; b < 8; ++b) base *= ((ub >> b) & 1) ? fB1[trow][b] : fB0[trow][b];
      lfq_double<NB>(base, fB1[trow], fB0[trow], out);
#pragma unroll
      for (int e = 0; e < SEG; ++e) sB[trow][seg * SEG + e] = out[e];
    }
    __syncthreads();
#pragma unroll 4
    for (int kk = 0; kk < kLfqKStep; kk += 2) {
      float a[W], b[W];
#pragma unroll
      for (int i = 0; i < W; ++i) a[i] = sA[kk + hi][wm * 32 * W + i * 32 + r];
#pragma unroll
      for (int j = 0; j < W; ++j) b[j] = sB[kk + hi][wn * 32 * W + j * 32 + r];
#pragma unroll
      for (int i = 0; i < W; ++i)
#pragma unroll
        for (int j = 0; j < W; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < W; ++i)
#pragma unroll
      for (int j = 0; j < W; ++j)
#pragma unroll
        for (int c = 0; c < 16; ++c) {
          sum[i][j][c] += (double)acc[i][j][c];
          acc[i][j][c] = 0.f;
        }
    __syncthreads();
  }
  float *dst = p.part + (long)blockIdx.x * p.Mpad * p.Npad;
#pragma unroll
  for (int i = 0; i < W; ++i)
#pragma unroll
    for (int j = 0; j < W; ++j)
#pragma unroll
      for (int c = 0; c < 16; ++c) {
        const int m = m0 + wm * 32 * W + i * 32 + (c & 3) + 8 * (c >> 2) + 4 * hi;
        const int n = n0 + wn * 32 * W + j * 32 + r;
        dst[(long)m * p.Npad + n] = (float)sum[i][j][c];
      }
}

// one thread per code j = u 2^dl + v
__global__ __launch_bounds__(256) void lfq_avg_reduce_kernel(const LfqFwdParams p) {
  __shared__ double sh[256];
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  const long n = 1L << p.g.d;
  double term = 0.0;
  if (j < n) {
    const long u = j >> p.g.dl, v = j & ((1L << p.g.dl) - 1);
    const float *src = p.part + u * p.Npad + v;
    const long stride = (long)p.Mpad * p.Npad;
    double s = 0.0;
    for (int c = 0; c < p.chunks; ++c) s += (double)src[c * stride];
    const float a = (float)(s / (double)p.g.R);
    p.avg[j] = a;
    term = -(double)a * log((double)a + kLfqEps);
  }
  term = lfq_block_sum<256>(term, sh);
  if (threadIdx.x == 0) p.ent_part[blockIdx.x] = term;
}

__global__ __launch_bounds__(256) void lfq_finish_kernel(const LfqFwdParams p) {
  __shared__ double sh[256];
  double ent = 0.0, com = 0.0, ce = 0.0;
  for (int i = threadIdx.x; i < p.elem_blocks; i += 256) {
    ent += p.elem_part[2 * i];
    com += p.elem_part[2 * i + 1];
  }
  for (int i = threadIdx.x; i < p.avg_blocks; i += 256) ce += p.ent_part[i];
  ent = lfq_block_sum<256>(ent, sh);
  com = lfq_block_sum<256>(com, sh);
  ce = lfq_block_sum<256>(ce, sh);
  if (threadIdx.x == 0) {
    const double se = ent / (double)p.g.R;
    p.scalars[0] = (float)((double)p.ws * se - (double)p.wb * ce);
    p.scalars[1] = (float)se;
    p.scalars[2] = (float)ce;
    p.scalars[3] = (float)(com / ((double)p.g.P * p.g.C));
  }
}

// ---- backward ------------------------------------------------------------------------------------------------------------------
struct LfqBwdParams {
  const float *x, *avg;
  const float *g_q, *g_aux, *g_commit;   // each may be null (zero)
  float *grad_x;
  float *G, *GT;                          // [2^dh][2^dl] and its transpose
  LfqGeom g;
  float ws, wb;
};

__global__ __launch_bounds__(256) void lfq_g_kernel(const LfqBwdParams p) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= (1L << p.g.d)) return;
  const long u = j >> p.g.dl, v = j & ((1L << p.g.dl) - 1);
  const double a = (double)p.avg[j];
  const float gv = (float)(-(log(a + kLfqEps) + a / (a + kLfqEps)));
  p.G[j] = gv;
  p.GT[(v << p.g.dh) + u] = gv;
}

// One pass of the backward for the wave's 32 rows: Out[m][row] = sum_k mat[k][m] Tk_row[k] (mat is [kdim][mdim], row-major), then
// dm[b] = sum_m Out[m] Tm_row[m] (bit_b(m) ? m0f[b] : -m1f[b]), summed over the wave's two lane halves.  (k1f, k0f) / (m1f, m0f):
// the padded factor slots of the lane's row for the table along k / along m.
template <int MT>
__device__ __forceinline__ void lfq_bwd_pass(const float *__restrict__ mat, int kdim, int mdim, const float (&k1f)[8],
                                             const float (&k0f)[8], const float (&m1f)[8], const float (&m0f)[8], float (&dm)[8],
                                             float *sM, float *sT, int hi, int r) {
  constexpr int MP = 32 * MT;
  f32x16 acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int c = 0; c < 16; ++c) acc[t][c] = 0.f;
  float ck[16];                                                  // entries kk = 16 hi + e of a slab, without the slab's own bits
  lfq_double<4>(hi ? k1f[4] : k0f[4], k1f, k0f, ck);
  const int slabs = kdim > 32 ? kdim / 32 : 1;
  for (int s = 0; s < slabs; ++s) {
    float sf = 1.0f;
#pragma unroll
    for (int b = 5; b < 8; ++b) sf *= ((s >> (b - 5)) & 1) ? k1f[b] : k0f[b];
#pragma unroll
    for (int e = 0; e < 16; ++e) sT[(16 * hi + e) * 32 + r] = ck[e] * sf;
    if (mdim == MP && kdim >= 32) {                               // the slab is 32 whole rows of mat: one run of 16-byte copies
      const f32x4 *src = reinterpret_cast<const f32x4 *>(mat + (long)s * 32 * MP);
      f32x4 *dst = reinterpret_cast<f32x4 *>(sM);
#pragma unroll
      for (int j = 0; j < (8 * MP) / (64 * kLfqBwdWaves); ++j) dst[threadIdx.x + j * 64 * kLfqBwdWaves] = src[threadIdx.x + j * 64 * kLfqBwdWaves];
    } else {
      for (int i = threadIdx.x; i < 32 * MP; i += 64 * kLfqBwdWaves) {
        const int kk = i / MP, m = i % MP, k = s * 32 + kk;
        sM[i] = (k < kdim && m < mdim) ? mat[(long)k * mdim + m] : 0.0f;
      }
    }
    __syncthreads();
#pragma unroll 4
    for (int kk = 0; kk < 32; kk += 2) {
      const float b = sT[(kk + hi) * 32 + r];
#pragma unroll
      for (int t = 0; t < MT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(sM[(kk + hi) * MP + t * 32 + r], b, acc[t], 0, 0, 0);
    }
    __syncthreads();
  }
  // register c of tile t is m = 32 t + (c & 3) + 8 (c >> 2) + 4 hi: bits 0-1 = c & 3, bit 2 = hi, bits 3-4 = c >> 2, bits 5-7 = t
  float t01[4], t34[4], t567[8];
  lfq_double<2>(hi ? m1f[2] : m0f[2], m1f, m0f, t01);
  lfq_double<2>(1.0f, &m1f[3], &m0f[3], t34);
  lfq_double<3>(1.0f, &m1f[5], &m0f[5], t567);
#pragma unroll
  for (int b = 0; b < 8; ++b) dm[b] = 0.f;
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      const int m = 32 * t + (c & 3) + 8 * (c >> 2);                // without bit 2
      const float w = acc[t][c] * ((t01[c & 3] * t34[c >> 2]) * t567[t]);
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        const bool set = b == 2 ? hi != 0 : ((m >> b) & 1) != 0;
        dm[b] += w * (set ? m0f[b] : -m1f[b]);
      }
    }
#pragma unroll
  for (int b = 0; b < 8; ++b) dm[b] += __shfl_xor(dm[b], 32);
}

// grid ceil(R / (32 kLfqBwdWaves)), 64 kLfqBwdWaves threads.  MT = max(1, 2^dh / 32) tiles of table entries.
template <int MT>
__global__ __launch_bounds__(64 * kLfqBwdWaves) void lfq_bwd_kernel(const LfqBwdParams p) {
  __shared__ __attribute__((aligned(16))) float sM[32 * 32 * MT];
  __shared__ float sT[kLfqBwdWaves][32 * 32];
  const LfqGeom &g = p.g;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hi = lane >> 5, r = lane & 31;
  const long row = ((long)blockIdx.x * kLfqBwdWaves + wave) * 32 + r;
  const bool live = row < g.R;
  const long pos = live ? row / g.nc : 0;
  const int ch0 = live ? (int)(row % g.nc) * g.d : 0;
  float xh[8], xl[8], h1[8], h0[8], l1[8], l0[8], dh_[8], dl_[8];
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    xh[b] = xl[b] = 0.f;
    h1[b] = l1[b] = 0.f;
    h0[b] = l0[b] = 1.f;
    dh_[b] = dl_[b] = 0.f;
    if (live && b < g.dh) { xh[b] = p.x[lfq_off(g, pos, ch0 + g.dl + b)]; lfq_prob(xh[b], h1[b], h0[b]); }
    if (live && b < g.dl) { xl[b] = p.x[lfq_off(g, pos, ch0 + b)]; lfq_prob(xl[b], l1[b], l0[b]); }
  }
  if (p.g_aux) {
    lfq_bwd_pass<MT>(p.GT, 1 << g.dl, 1 << g.dh, l1, l0, h1, h0, dh_, sM, sT[wave], hi, r);
    lfq_bwd_pass<MT>(p.G, 1 << g.dh, 1 << g.dl, h1, h0, l1, l0, dl_, sM, sT[wave], hi, r);
  }
  if (!live) return;
  const double ga = p.g_aux ? (double)*p.g_aux : 0.0, gc = p.g_commit ? (double)*p.g_commit : 0.0;
  const double invR = 1.0 / (double)g.R, cc = 2.0 / ((double)g.P * g.C);
  // lane half 0 writes the high bits, half 1 the low bits
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    if (b >= (hi ? g.dl : g.dh)) continue;
    const float x = hi ? xl[b] : xh[b];
    const float p1 = hi ? l1[b] : h1[b], p0 = hi ? l0[b] : h0[b];
    const float dce = hi ? dl_[b] : dh_[b];
    const long o = lfq_off(g, pos, ch0 + (hi ? b : g.dl + b));
    const float q = x > 0.0f ? 1.0f : -1.0f;
    const float s = kLfqScale * x;
    const double dsample = -(double)s * ((double)p1 * (double)p0);
    double v = p.g_q ? (double)p.g_q[o] : 0.0;
    v += gc * cc * (double)(x - q);
    v += ga * 400.0 * (invR * ((double)p.ws * dsample - (double)p.wb * (double)dce));
    p.grad_x[o] = (float)v;
  }
}

}  // namespace gqhip
