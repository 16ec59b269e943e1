// gq_moments.h -- the raw first and second moments of a feature block, accumulated in fp64 on the device: what the reference's FID
// needs of its Inception features (eval.py:186-203 keeps every feature row on the host, :241-257 runs np.mean / np.cov over them).
//
// state (fp64 words) = [ outer: D D, row-major | sum: D | count: 1 ].  One call, x [rows, D] fp32 with row r at x + r row_stride:
//     outer[i][j] <- fma((double)x[r][i], (double)x[r][j], outer[i][j])   r = 0 .. rows - 1 in ascending r, j >= i
//     sum[i]      <- sum[i] + (double)x[r][i]                             in the same order
//     count       <- count + rows
// The product of two fp32 values has at most 48 significant bits and an exponent far inside fp64's range, so it is exact in fp64
// and every step is ONE rounding, that of outer + product: a sequential fp64 loop on the host gives the same bits, splitting the
// rows over several calls changes none, and a * b + c equals fma(a, b, c) here whatever -ffp-contract says.
//
// Tile map.  The D x D matrix is cut into 64 x 64 tiles; the grid is the T (T + 1) / 2 tile pairs (ti, tj) with tj >= ti
// (T = ceil(D / 64)), row by row of the upper triangle.  A block of 256 threads owns one tile; thread (ty = tid / 16,
// tx = tid % 16) owns its rows 4 ty .. 4 ty + 3 and columns {2 tx, 2 tx + 1, 32 + 2 tx, 33 + 2 tx}: 16 doubles, loaded once, run
// through their FMA chains in registers, stored once.  No atomics: every output element has one owner, and calls on a stream are
// ordered.  A diagonal tile also writes its elements below the diagonal (the same chain with i and j swapped: unspecified by
// the contract, bit-symmetric in fact) and its 64 entries of `sum`; thread 0 of block 0 advances `count`.
//   x:     the block stages the two column strips it needs through LDS, 16 rows at a time (2 x 16 x 64 floats), the next chunk's
//          loads in flight under the FMAs; 16-byte loads where x and row_stride are 16-byte multiples and the four columns lie
//          inside D, 4-byte loads otherwise (the same values either way).
//   state: 16 lanes x 16 bytes = 256 contiguous bytes per tile row when the state is 16-byte aligned and D is even, 8-byte
//          accesses (16 lanes x 8 bytes, twice) otherwise.
#pragma once
#include "gq_common.h"

namespace gqhip {

constexpr int kMomTile = 64;      // outputs per tile side
constexpr int kMomChunk = 16;     // rows of x staged at a time
constexpr int kMomMaxD = 8192;

typedef double f64x2 __attribute__((ext_vector_type(2)));

struct MomentsParams {
  const float *x;
  double *state;
  int rows, D, stride;
  int T;            // tiles per side
  int vec_x;        // x and row_stride allow 16-byte loads
  int wide_state;   // state is 16-byte aligned and D is even
};

// four columns c .. c + 3 of row r of x; columns from D on and rows from `rows` on read as 0 and are never dereferenced
__device__ __forceinline__ f32x4 moments_quad(const MomentsParams &p, int r, int c) {
  f32x4 v{0.f, 0.f, 0.f, 0.f};
  if (r < p.rows && c < p.D) {
    const float *s = p.x + (long)r * p.stride + c;
    if (p.vec_x && c + 3 < p.D) {
      v = *reinterpret_cast<const f32x4 *>(s);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (c + e < p.D) v[e] = s[e];
    }
  }
  return v;
}

__global__ __launch_bounds__(256) void moments_update_kernel(const MomentsParams p) {
  __shared__ __attribute__((aligned(16))) float sa[kMomChunk][kMomTile];   // columns of tile row ti
  __shared__ __attribute__((aligned(16))) float sb[kMomChunk][kMomTile];   // columns of tile column tj
  const int T = p.T, D = p.D, blk = blockIdx.x;
  // blk -> (ti, tj): row ti of the upper triangle starts at off(ti) = ti (2 T - ti + 1) / 2
  const double w = 2.0 * T + 1.0;
  int ti = (int)((w - sqrt(w * w - 8.0 * blk)) * 0.5);
  ti = ti < 0 ? 0 : ti > T - 1 ? T - 1 : ti;
  while (ti > 0 && ti * (2 * T - ti + 1) / 2 > blk) --ti;
  while (ti < T - 1 && (ti + 1) * (2 * T - ti) / 2 <= blk) ++ti;
  const int tj = ti + (blk - ti * (2 * T - ti + 1) / 2);
  const int i0 = ti * kMomTile, j0 = tj * kMomTile;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  double *outer = p.state, *sum = p.state + (long)D * D;

  // this thread's 4 x 4 outputs: rows i0 + 4 ty + a, columns j0 + 2 tx + (e & 1) + 32 (e >> 1)
  double acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int i = i0 + 4 * ty + a;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int j = j0 + 2 * tx + 32 * h;
      acc[a][2 * h] = acc[a][2 * h + 1] = 0.0;
      if (i < D && j < D) {
        const double *s = outer + (long)i * D + j;
        if (p.wide_state) {       // D even, j even: j + 1 < D
          const f64x2 v = *reinterpret_cast<const f64x2 *>(s);
          acc[a][2 * h] = v[0]; acc[a][2 * h + 1] = v[1];
        } else {
          acc[a][2 * h] = s[0];
          if (j + 1 < D) acc[a][2 * h + 1] = s[1];
        }
      }
    }
  }
  const bool sums = ti == tj && tid < kMomTile && i0 + tid < D;
  double colsum = sums ? sum[i0 + tid] : 0.0;

  const int qr = tid >> 4, qc = (tid & 15) * 4;     // the quad of a chunk this thread stages, for both strips
  f32x4 qa = moments_quad(p, qr, i0 + qc), qb = moments_quad(p, qr, j0 + qc);
  for (int r0 = 0; r0 < p.rows; r0 += kMomChunk) {
    __syncthreads();                                // the previous chunk has been consumed
    *reinterpret_cast<f32x4 *>(&sa[qr][qc]) = qa;
    *reinterpret_cast<f32x4 *>(&sb[qr][qc]) = qb;
    __syncthreads();
    if (r0 + kMomChunk < p.rows) {
      qa = moments_quad(p, r0 + kMomChunk + qr, i0 + qc);
      qb = moments_quad(p, r0 + kMomChunk + qr, j0 + qc);
    }
    // rows past the last are not run through the chains: fma(0, 0, -0.0) is +0.0
    const int nr = p.rows - r0 < kMomChunk ? p.rows - r0 : kMomChunk;
#pragma unroll 4
    for (int r = 0; r < nr; ++r) {
      const f32x4 av = *reinterpret_cast<const f32x4 *>(&sa[r][4 * ty]);
      const f32x2 b0 = *reinterpret_cast<const f32x2 *>(&sb[r][2 * tx]);
      const f32x2 b1 = *reinterpret_cast<const f32x2 *>(&sb[r][32 + 2 * tx]);
      const double bd[4] = {(double)b0[0], (double)b0[1], (double)b1[0], (double)b1[1]};
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        const double ad = (double)av[a];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[a][e] = fma(ad, bd[e], acc[a][e]);
      }
      if (sums) colsum += (double)sa[r][tid];
    }
  }

#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int i = i0 + 4 * ty + a;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int j = j0 + 2 * tx + 32 * h;
      if (i < D && j < D) {
        double *s = outer + (long)i * D + j;
        if (p.wide_state) {
          *reinterpret_cast<f64x2 *>(s) = f64x2{acc[a][2 * h], acc[a][2 * h + 1]};
        } else {
          s[0] = acc[a][2 * h];
          if (j + 1 < D) s[1] = acc[a][2 * h + 1];
        }
      }
    }
  }
  if (sums) sum[i0 + tid] = colsum;
  if (blk == 0 && tid == 0) sum[D] += (double)p.rows;
}

}  // namespace gqhip
