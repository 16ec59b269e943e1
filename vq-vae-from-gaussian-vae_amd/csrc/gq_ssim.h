// gq_ssim.h -- per-image SSIM and MS-SSIM on the device (pit/evaluations/ssim.py:5-63, i.e. pytorch_msssim's ssim / ms_ssim
// with data_range 255, size_average False, an 11-tap Gaussian window of sigma 1.5, K = (0.01, 0.03)).
//
// One launch per scale level.  A block owns one kTH x kTW tile of the level's "valid" output positions of one (image, channel)
// plane: it stages the (kTH + 10) x (kTW + 10) input halo of X and Y in LDS as fp64, runs the separable window along W for the
// five moments (X, Y, XX, YY, XY) into LDS and along H in registers, forms ssim_map / cs_map and leaves the tile's two sums in the
// workspace.  A side shorter than 11 is not filtered (pytorch_msssim skips it): template flags FH / FW.  The blocks after those
// write the next level's 2 x 2 average pool of X and Y (zero padding on the leading edge of an odd side, divided by 4).  In the
// level that finishes the call the LAST block of each image (a per-image ticket, left zero for the next call) adds the tile sums
// of every level in a fixed order, so the values are bit-reproducible, zeroes them and writes SSIM and MS-SSIM as fp32.  A call
// that pooled (MS-SSIM) ends with one launch of ssim_zero_kernel over the pooled planes: the workspace is ALL zero between calls,
// so the next call may lay it out for any other shape that fits (its tickets must find zeros wherever they land).
//
// Numerics: the scaled inputs are formed in fp32 as the reference does ((x + 1) 127.5 or x 255); from there on everything is
// fp64 -- at the 0..255 scale G(XX) - mu^2 cancels up to ~16 bits in flat regions, which fp32 (the reference) cannot carry.
#pragma once
#include <hip/hip_runtime.h>

namespace gqssim {

constexpr int kTW = 32, kTH = 16, kWin = 11, kLevels = 5;

struct Level {
  int H, W;              // plane size at this level
  int Ho, Wo;            // valid output positions (a side under 11 is left unfiltered: Ho = H)
  int tiles_x, tiles_y;  // output tiles per plane
  long part;             // first tile record of this level: records [B * C * tiles] of two doubles (sum ssim_map, sum cs_map)
};

struct Params {
  const float *x, *y;        // level 0: B images, NCHW (layout 0) or NHWC (layout 1), fp32, unscaled
  const double *px, *py;     // level >= 1: this level's planes [B * C, H, W] (workspace)
  double *qx, *qy;           // next level's pooled planes (workspace), NULL: no pooling in this launch
  double *partial;           // tile sums of every level (workspace; zeroed again by the block that adds them)
  int *ticket;               // [B], zero between calls (workspace)
  float *ssim_out, *ms_out;  // NULL or per-image values at [b * out_stride]
  long out_stride;
  float win[kWin];           // the fp32 Gaussian window
  Level lv[kLevels];
  int B, C, layout, zero_mean;
  int level, final_level;    // this launch's level; the level whose launch combines the sums
  int nan_ms;                // 1: MS-SSIM is undefined for this size (a side < 256): write NaN
  int ssim_blocks;           // blocks [0, ssim_blocks) compute tiles, the rest pool
};

// Both images' values at (i, j) (out of range: 0).
__device__ inline void load_xy(const Params &p, int plane, int i, int j, double &a, double &b) {
  const Level &L = p.lv[p.level];
  if (i < 0 || j < 0 || i >= L.H || j >= L.W) { a = 0.0; b = 0.0; return; }
  if (p.level == 0) {
#pragma clang fp contract(off)
    long off;
    if (p.layout == 0) {
      off = ((long)plane * L.H + i) * L.W + j;
    } else {
      const int bi = plane / p.C, c = plane - bi * p.C;
      off = (((long)bi * L.H + i) * L.W + j) * p.C + c;
    }
    const float u = p.x[off], v = p.y[off];
    a = (double)(p.zero_mean ? (u + 1.0f) * 127.5f : u * 255.0f);
    b = (double)(p.zero_mean ? (v + 1.0f) * 127.5f : v * 255.0f);
    return;
  }
  const long off = ((long)plane * L.H + i) * L.W + j;
  a = p.px[off];
  b = p.py[off];
}

// torch.relu: negative -> 0, NaN stays NaN
__device__ inline double relu(double v) { return v < 0.0 ? 0.0 : v; }

// Deterministic sum of one double over the block's 256 threads (fixed shuffle tree, waves added in order).
__device__ inline double block_sum(double v, double *sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

template <bool FH, bool FW>
__global__ __launch_bounds__(256) void ssim_level_kernel(const Params p) {
  constexpr int KH = FH ? kWin : 1, KW = FW ? kWin : 1;
  constexpr int HH = kTH + KH - 1, HW = kTW + KW - 1;
  const int tid = threadIdx.x;
  const Level &L = p.lv[p.level];

  if ((int)blockIdx.x >= p.ssim_blocks) {       // next level's 2 x 2 average pool (avg_pool2d, padding = side % 2, /4)
    const Level &N = p.lv[p.level + 1];
    const long e = (long)(blockIdx.x - p.ssim_blocks) * 256 + tid;
    const long per = (long)N.H * N.W;
    if (e >= (long)p.B * p.C * per) return;
    const int plane = (int)(e / per), rem = (int)(e - (long)plane * per);
    const int i = rem / N.W, j = rem - (rem / N.W) * N.W;
    const int r0 = 2 * i - (L.H & 1), c0 = 2 * j - (L.W & 1);
    double a00, b00, a01, b01, a10, b10, a11, b11;
    load_xy(p, plane, r0, c0, a00, b00);
    load_xy(p, plane, r0, c0 + 1, a01, b01);
    load_xy(p, plane, r0 + 1, c0, a10, b10);
    load_xy(p, plane, r0 + 1, c0 + 1, a11, b11);
    p.qx[e] = (((a00 + a01) + a10) + a11) * 0.25;
    p.qy[e] = (((b00 + b01) + b10) + b11) * 0.25;
    return;
  }

  __shared__ double sx[HH][HW], sy[HH][HW];
  __shared__ double sm[5][HH][kTW];
  __shared__ double sh[4];
  __shared__ int sh_last;

  const int tiles = L.tiles_x * L.tiles_y;
  const int plane = blockIdx.x / tiles, t = blockIdx.x - plane * tiles;
  const int oy0 = (t / L.tiles_x) * kTH, ox0 = (t - (t / L.tiles_x) * L.tiles_x) * kTW;

  double w[kWin];
#pragma unroll
  for (int k = 0; k < kWin; ++k) w[k] = (double)p.win[k];

  for (int e = tid; e < HH * HW; e += 256) {
    const int r = e / HW, q = e - r * HW;
    double a, b;
    load_xy(p, plane, oy0 + r, ox0 + q, a, b);
    sx[r][q] = a;
    sy[r][q] = b;
  }
  __syncthreads();

  // along W: the five moments of every halo row at the tile's kTW output columns
  for (int e = tid; e < HH * kTW; e += 256) {
    const int r = e / kTW, j = e - r * kTW;
    double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0, m4 = 0.0;
#pragma unroll
    for (int k = 0; k < KW; ++k) {
      const double wk = FW ? w[k] : 1.0;
      const double a = sx[r][j + k], b = sy[r][j + k];
      m0 += wk * a;
      m1 += wk * b;
      m2 += wk * (a * a);
      m3 += wk * (b * b);
      m4 += wk * (a * b);
    }
    sm[0][r][j] = m0; sm[1][r][j] = m1; sm[2][r][j] = m2; sm[3][r][j] = m3; sm[4][r][j] = m4;
  }
  __syncthreads();

  // along H: thread (column j, row pair rp) forms two outputs
  const int j = tid & (kTW - 1), rp = tid / kTW;          // rp in [0, 8): rows 2 rp, 2 rp + 1
  double v0[5] = {0, 0, 0, 0, 0}, v1[5] = {0, 0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < KH + 1; ++k) {
    const int r = 2 * rp + k;
#pragma unroll
    for (int m = 0; m < 5; ++m) {
      const double s = sm[m][r < HH ? r : HH - 1][j];
      if (k < KH) v0[m] += (FH ? w[k] : 1.0) * s;
      if (k >= 1) v1[m] += (FH ? w[k - 1] : 1.0) * s;
    }
  }
  const double C1 = (0.01 * 255.0) * (0.01 * 255.0), C2 = (0.03 * 255.0) * (0.03 * 255.0);
  double s_acc = 0.0, c_acc = 0.0;
  auto tally = [&](const double (&v)[5], int oy) {
    if (oy >= L.Ho || ox0 + j >= L.Wo) return;
    const double mu1 = v[0], mu2 = v[1];
    const double mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
    const double s11 = v[2] - mu1_sq, s22 = v[3] - mu2_sq, s12 = v[4] - mu12;
    const double cs = (2.0 * s12 + C2) / (s11 + s22 + C2);
    const double ss = ((2.0 * mu12 + C1) / (mu1_sq + mu2_sq + C1)) * cs;
    s_acc += ss;
    c_acc += cs;
  };
  tally(v0, oy0 + 2 * rp);
  tally(v1, oy0 + 2 * rp + 1);
  const double bs = block_sum(s_acc, sh);
  const double bc = block_sum(c_acc, sh);

  const int b = plane / p.C;
  if (tid == 0) {
    double *dst = p.partial + (L.part + (long)plane * tiles + t) * 2;
    dst[0] = bs;
    dst[1] = bc;
  }
  if (p.level != p.final_level) return;
  if (tid == 0) {
    __threadfence();
    sh_last = atomicAdd(&p.ticket[b], 1) == p.C * tiles - 1;
  }
  __syncthreads();
  if (!sh_last || tid >= 64) return;
  __threadfence();

  // the image's last block: wave 0 adds every level's tile sums (lanes stride the tiles, a fixed shuffle tree combines them)
  const float wts[kLevels] = {0.0448f, 0.2856f, 0.3001f, 0.2363f, 0.1333f};
  const int nl = p.final_level + 1;
  double ssim_img = 0.0, ms_img = 0.0;
  for (int c = 0; c < p.C; ++c) {
    const int pl = b * p.C + c;
    double ms_c = 1.0, ssim_c = 0.0;
    for (int l = 0; l < nl; ++l) {
      const Level &M = p.lv[l];
      const int nt = M.tiles_x * M.tiles_y;
      double *src = p.partial + (M.part + (long)pl * nt) * 2;
      double s = 0.0, cs = 0.0;
      for (int k = tid; k < nt; k += 64) {
        s += __hip_atomic_load(src + 2 * k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        cs += __hip_atomic_load(src + 2 * k + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        src[2 * k] = 0.0;                      // zero behind the call, like the ticket: a later call with another B puts its
        src[2 * k + 1] = 0.0;                  // tickets where these records were
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        s += __shfl_xor(s, o);
        cs += __shfl_xor(cs, o);
      }
      const double n = (double)M.Ho * (double)M.Wo;
      if (l == 0) ssim_c = s / n;
      if (l < kLevels - 1) {
        ms_c *= pow(relu(cs / n), (double)wts[l]);            // relu(cs) ** w
      } else {
        ms_c *= pow(relu(s / n), (double)wts[l]);             // relu(ssim) ** w at the last level
      }
    }
    ssim_img += ssim_c;
    ms_img += ms_c;
  }
  if (tid != 0) return;
  if (p.ssim_out) p.ssim_out[(long)b * p.out_stride] = (float)(ssim_img / p.C);
  if (p.ms_out) p.ms_out[(long)b * p.out_stride] = p.nan_ms ? __int_as_float(0x7fc00000) : (float)(ms_img / p.C);
  p.ticket[b] = 0;                             // ready for the next call on this workspace
}

// The pooled planes of a call that ran more than one level, back to zero (grid-stride, 16-byte stores; n2 = pairs of doubles).
__global__ __launch_bounds__(256) void ssim_zero_kernel(double2 *dst, long n2) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n2; i += (long)gridDim.x * 256) dst[i] = double2{0.0, 0.0};
}

}  // namespace gqssim
