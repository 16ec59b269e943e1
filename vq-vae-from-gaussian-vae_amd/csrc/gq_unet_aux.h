// gq_unet_aux.h -- the kernels of the conv stack around the matrix-core kernels: fused GroupNorm (+ SiLU),
// residual adds that leave the next GroupNorm's statistics behind, the Winograd F(2x2,3x3) / F(4x4,3x3) data transforms,
// the sub-pixel upsample glue and the operand splits of the attention GEMMs (pit/modules/unet.py:49-206).  One pass over
// memory each; the GroupNorm-fused Winograd input transforms are nevertheless bound by vector issue, not by HBM (their VALU is
// busy 57-64 % of the kernel's time, 68-73 % before their index arithmetic was taken out of the tile loops: profiles/r20).
#pragma once
#include "gq_common.h"
#include "gq_stats.h"

namespace gqhip {

typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));

// x * sigmoid(x) = x / (1 + e^-x), the quotient by one Newton step on v_rcp_f32 (q = x r; q += (x - d q) r: within
// half an ulp of the IEEE quotient up to a few units of 2^-24 of an ulp, at a third of the IEEE divide's instructions).
// EVERY SiLU of libgqhip goes through this function, so the GroupNorm applied as its own pass and the one fused into
// the Winograd input transforms produce identical bits.  d > 1e37 (x < -85.2; d = inf below -88.7): 1 / d is subnormal,
// the result (|.| < 1e-35) is returned as x * 0 = -0 -- the divide gives -0 for d = inf too -- and never a NaN.
__device__ __forceinline__ float silu_f32(float x) {
  const float d = 1.0f + __expf(-x);
  const float r = __builtin_amdgcn_rcpf(d);
  const float q = x * r;
  const float q1 = __builtin_fmaf(__builtin_fmaf(-d, q, x), r, q);
  return d > 1e37f ? q : q1;
}

// SiLU(GroupNorm(x)) of a thread's channels: a, sh = the folded per-channel scale and shift (gq_stats.h: gn_channel).  EVERY
// consumer of a GroupNorm applies them through this function -- gn_apply as its own pass and every kernel with the producer
// fused in -- so the fused transforms write bit-for-bit the V of the two-pass route.
template <int SILU, typename VEC>
__device__ __forceinline__ VEC gn_act(VEC v, VEC a, VEC sh) {
  v = v * a + sh;
  if (SILU) {
#pragma unroll
    for (int e = 0; e < (int)(sizeof(VEC) / sizeof(float)); ++e) v[e] = silu_f32(v[e]);
  }
  return v;
}
// ---- NHWC (channels_last) variants: x[b][hw][c], the layout MIOpen's fp32 igemm kernels want ----
// A block owns a slab of pixels of one image and ALL channels: thread -> channel quad q = tid % (C/4)
// (4 consecutive channels of ONE group since cpg % 4 == 0), pixel lane = tid / (C/4).
__global__ __launch_bounds__(256) void gn_stats_nhwc_kernel(const float *__restrict__ x,
                                                            const float *__restrict__ pre_bias,
                                                            int64_t *__restrict__ stats, int C, long HW, int cpg,
                                                            int slabs) {
  __shared__ int64_t red[kStatWords * 64];   // per-group statistics records (gq_stats.h), groups <= 64
  const int groups = C / cpg, quads = C / 4, lanes = 256 / quads;
  const long b = blockIdx.x / slabs;
  const int slab = blockIdx.x % slabs;
  const long per = (HW + slabs - 1) / slabs;
  const long lo = slab * per, hi = lo + per < HW ? lo + per : HW;
  const int q = threadIdx.x % quads, pl = threadIdx.x / quads;
  for (int w = threadIdx.x; w < kStatWords * groups; w += 256) red[w] = 0;
  __syncthreads();
  f32x4 pb = {0.f, 0.f, 0.f, 0.f};
  if (pre_bias) pb = *reinterpret_cast<const f32x4 *>(pre_bias + 4 * q);
  const float *base = x + (b * HW) * C + 4 * q;
  StatPartial st;
  for (long p = lo + pl; p < hi; p += lanes) stat_partial_add_vec(st, *reinterpret_cast<const f32x4 *>(base + p * C) + pb);
  const int g = (4 * q) / cpg;
  stat_partial_flush(red + kStatWords * g, st);
  __syncthreads();
  for (int w = threadIdx.x; w < kStatWords * groups; w += 256) stat_flush_word(stats + kStatWords * (b * groups) + w, red[w]);
}

template <int SILU>
__global__ __launch_bounds__(256) void gn_apply_nhwc_kernel(const float *__restrict__ x, const float *__restrict__ gamma,
                                                            const float *__restrict__ beta, float *__restrict__ y,
                                                            const int64_t *__restrict__ stats,
                                                            const float *__restrict__ pre_bias, int C, long HW,
                                                            int cpg, double eps, int slabs) {
  const int groups = C / cpg, quads = C / 4, lanes = 256 / quads;
  const long b = blockIdx.x / slabs;
  const int slab = blockIdx.x % slabs;
  const long per = (HW + slabs - 1) / slabs;
  const long lo = slab * per, hi = lo + per < HW ? lo + per : HW;
  const int q = threadIdx.x % quads, pl = threadIdx.x / quads;
  const int g = (4 * q) / cpg;
  const GnGroup gg = gn_group(stats + kStatWords * (b * groups + g), (double)cpg * (double)HW, eps);
  f32x4 a, sh;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const GnAffine f = gn_channel(gg, gamma, beta, pre_bias, 4 * q + k);
    a[k] = f.a;
    sh[k] = f.sh;
  }
  const float *xi = x + (b * HW) * C + 4 * q;
  float *yo = y + (b * HW) * C + 4 * q;
  for (long p = lo + pl; p < hi; p += lanes)
    *reinterpret_cast<f32x4 *>(yo + p * C) = gn_act<SILU>(*reinterpret_cast<const f32x4 *>(xi + p * C), a, sh);
}

__global__ __launch_bounds__(256) void add_bias_nhwc_kernel(const float *__restrict__ a, const float *__restrict__ b,
                                                            const float *__restrict__ bias, float *__restrict__ y,
                                                            int C, long total4) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total4; i += (long)gridDim.x * 256) {
    f32x4 v = reinterpret_cast<const f32x4 *>(a)[i] + reinterpret_cast<const f32x4 *>(b)[i];
    if (bias) v = v + *reinterpret_cast<const f32x4 *>(bias + (int)((i * 4) % C));
    reinterpret_cast<f32x4 *>(y)[i] = v;
  }
}

// Residual add that also leaves the GroupNorm statistics of its OUTPUT behind (the next op of the UNet is a
// GroupNorm over exactly this tensor: unet.py:160 -> :140): same block/thread mapping as gn_stats_nhwc_kernel, so
// the consumer's statistics pass (one full read of the tensor) disappears.
__global__ __launch_bounds__(256) void add_bias_stats_nhwc_kernel(const float *__restrict__ a, const float *__restrict__ b,
                                                                  const float *__restrict__ bias, float *__restrict__ y,
                                                                  int64_t *__restrict__ stats, int C, long HW, int cpg,
                                                                  int slabs) {
  __shared__ int64_t red[kStatWords * 64];   // per-group statistics records (gq_stats.h), groups <= 64
  const int groups = C / cpg, quads = C / 4, lanes = 256 / quads;
  const long bi = blockIdx.x / slabs;
  const int slab = blockIdx.x % slabs;
  const long per = (HW + slabs - 1) / slabs;
  const long lo = slab * per, hi = lo + per < HW ? lo + per : HW;
  const int q = threadIdx.x % quads, pl = threadIdx.x / quads;
  for (int w = threadIdx.x; w < kStatWords * groups; w += 256) red[w] = 0;
  __syncthreads();
  f32x4 pb = {0.f, 0.f, 0.f, 0.f};
  if (bias) pb = *reinterpret_cast<const f32x4 *>(bias + 4 * q);
  const long off = (bi * HW) * C + 4 * q;
  StatPartial st;
  for (long p = lo + pl; p < hi; p += lanes) {
    const f32x4 v = *reinterpret_cast<const f32x4 *>(a + off + p * C) + *reinterpret_cast<const f32x4 *>(b + off + p * C) + pb;
    *reinterpret_cast<f32x4 *>(y + off + p * C) = v;
    stat_partial_add_vec(st, v);
  }
  const int g = (4 * q) / cpg;
  stat_partial_flush(red + kStatWords * g, st);
  __syncthreads();
  for (int w = threadIdx.x; w < kStatWords * groups; w += 256) stat_flush_word(stats + kStatWords * (bi * groups) + w, red[w]);
}

// Nearest-neighbour x2 upsample, NHWC (unet.py:69-73 `interpolate(scale_factor=2, mode="nearest")`):
// one thread per (input pixel, channel quad); the 16-byte value is written to the 2x2 output pixels.
__global__ __launch_bounds__(256) void upsample2x_nhwc_kernel(const float *__restrict__ x, float *__restrict__ y,
                                                              int H, int W, int C4, long total) {
  for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
    const int q = (int)(t % C4);
    long p = t / C4;
    const int w = (int)(p % W);
    p /= W;
    const int h = (int)(p % H);
    const long b = p / H;
    const f32x4 v = reinterpret_cast<const f32x4 *>(x)[t];
    f32x4 *o = reinterpret_cast<f32x4 *>(y) + ((b * 2 * H + 2 * h) * (2L * W) + 2 * w) * C4 + q;
    o[0] = v;
    o[C4] = v;
    o[2L * W * C4] = v;
    o[2L * W * C4 + C4] = v;
  }
}

// ---- Winograd F(2x2, 3x3), NHWC, stride 1, padding 1 (used for the decoder's wide 3x3 convolutions) -------------
// Y = A^T [ (G g G^T) . (B^T d B) ] A per 4x4 input tile d (stride 2) and 2x2 output tile: 16 multiplies per 4 outputs
// instead of 36.  The element-wise products over the channels are 16 independent GEMMs [tiles, Cin] x [Cin, Cout]
// (torch.bmm -> hipBLASLt); these two kernels are the data transforms around them.
//   V[k][tile][c] = (B^T d B)[k]     B^T = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1]
//   y[2x2]        = A^T m A          A^T = [1 1 1 0; 0 1 -1 -1]
// One thread per (tile, channel quad); tiles = B * (H/2) * (W/2), H and W even.
// Where a transformed value goes.  F16X3 = false: V [k][tile][C] fp32.  F16X3 = true: the operand of ONE fp16 GEMM with
// fp32 accumulation whose K axis carries the three split products (v = h + l, two-term fp16 split of v * scale):
// V3 [k][tile][3C] fp16 = [ h | h | l ], to be multiplied by U3 [k][3C][Cout] = [ U_h ; U_l ; U_h ] (unet._wino_weights_f16):
// V3 U3 = h U_h + h U_l + l U_h, error ~3 * 2^-22 per product -- the level of hipBLASLt's own fp32 (split-bf16) GEMM, at
// 2-2.5x its speed (tools/bmm_bf16x3.py).  `scale` is a power of two chosen by the caller so that |v * scale| < 65504.
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
// F16X3 = 2 ("f16x2"): V2 [k][tile][2C] = [ h | l ] only -- the operand of wino_gemm_f16x2_kernel / wino_gemm_f16x2_k64_kernel (gq_wino_gemm.h), which form the
// three products itself (4 instead of 6 bytes per element).
//
// ---- Addressing of the transform kernels.  Every address is a base plus a BYTE offset of type OFF, and the offsets of an item
// are formed once per item, not once per access (hipcc does not strength-reduce `x[((b * H + y) * W + x) * CV + q]` in `long`: it
// multiplies again for each of the 36 loads and 72 stores of an F(4x4,3x3) item -- profiles/r20):
//   x / y / res   the tensor's base (the kernel argument: wave-uniform) + row offset + column offset: N offsets per axis, clamps
//                 included; the row offsets carry the item's image and channel vector
//   V / M         the plane's base (wave-uniform, advanced plane by plane on the scalar side) + the item's offset in a plane
// so an access is `global_load / global_store v_offset, s[base]` with at most one 32-bit add in front.
// OFF = uint32_t in the kernels proper: the host launches them only where every such offset is below 2^32
// (gq_wino_range.h: wino_offsets_fit_u32).  OFF = uint64_t in their *_wide_kernel twins, which take every other shape.
// Four kernels keep the per-access 64-bit indexing, each for the reason given where it stands: wino_in_nhwc_kernel<0>,
// wino4_in_gn_nhwc_kernel<*, 0, 4>, wino4_out_nhwc_kernel and wino_out_res_nhwc_kernel<4, *>.
// amdgpu_waves_per_eu on the two fused input kernels: with the cheaper addresses hipcc aims at one wave per SIMD more than it can
// use and pays with the load schedule (wino_in_gn: three loads in flight instead of 16; wino4_in_gn: 163 registers = three waves).
// The ranges name the occupancy each kernel has anyway (98-108 registers: four waves) and leave the loads as written.
template <int F16X3, typename VEC>
struct WinoVRow {   // one item's vector in a row of V: VB bytes in each of the row's PARTS parts of CV vectors ([v], [h | h | l], [h | l])
  static constexpr int VB = F16X3 ? sizeof(VEC) / 2 : sizeof(VEC), PARTS = F16X3 == 1 ? 3 : F16X3 == 2 ? 2 : 1;
};
// Plane 0 of V / M for one item.  The plane bases do not depend on the item, so hipcc would form all N * N of them ahead of the item
// loop (72 scalar registers for F(4x4,3x3): it spills them); through this the planes are walked by scalar additions item by item.
template <typename P>
__device__ __forceinline__ P *wino_plane0(P *p) {
  uint64_t zero = 0;   // (the pointer itself stays the kernel argument: a global address)
  asm volatile("" : "+s"(zero));
  return p + zero;
}
// plane = base of the value's plane k, at = byte offset of the item's vector in part 0 of its row, part = bytes per part
template <int F16X3, typename VEC, typename OFF>
__device__ __forceinline__ void wino_store_v(char *plane, OFF at, OFF part, VEC v, float scale) {
  constexpr int VW = sizeof(VEC) / sizeof(float);          // channels per thread (4, or 2 in the two-channel kernels)
  typedef _Float16 hvec __attribute__((ext_vector_type(VW)));
  if constexpr (F16X3 != 0) {
    v = v * scale;
    hvec h, l;
#pragma unroll
    for (int e = 0; e < VW; ++e) {
      h[e] = (_Float16)v[e];
      l[e] = (_Float16)(v[e] - (float)h[e]);
    }
    *reinterpret_cast<hvec *>(plane + at) = h;
    if constexpr (F16X3 == 2) {
      *reinterpret_cast<hvec *>(plane + (OFF)(at + part)) = l;
    } else {
      *reinterpret_cast<hvec *>(plane + (OFF)(at + part)) = h;
      *reinterpret_cast<hvec *>(plane + (OFF)(at + 2 * part)) = l;
    }
  } else {
    *reinterpret_cast<VEC *>(plane + at) = v;
  }
}

// ---- Winograd F(4x4, 3x3): 6x6 input tiles (stride 4), 36 GEMMs, 4x4 output tiles: 36 multiplies per 16 outputs (4x
// fewer than direct, 1.78x fewer than F(2x2,3x3)) and V / M are 2.25x the activation instead of 4x.  Larger transform
// constants (up to 8) cost ~10x the rounding error of F(2x2,3x3): used in the decoder only.
//   B^T = [4 0 -5 0 1 0; 0 -4 -4 1 1 0; 0 4 -4 -1 1 0; 0 -2 -1 2 1 0; 0 2 -1 -2 1 0; 0 4 0 -5 0 1]
//   A^T = [1 1 1 1 1 0; 0 1 -1 2 -2 0; 0 1 1 4 4 0; 0 1 -1 8 -8 1]
//
// ---- The pieces the seven transform kernels share.  T = 2: F(2x2,3x3), 4: F(4x4,3x3); N = T + 2 = the transform size.
// The 1-D transforms of one column or row: A^T m of both sizes (wino_at<T>) and F(4x4,3x3)'s B^T d; F(2x2,3x3)'s B^T d is
// written out in its two input kernels, each value formed in its store's argument (fewer registers: profiles/r17).
template <typename V>
__device__ __forceinline__ void wino2_at(const V (&m)[4], V (&o)[2]) {
  o[0] = m[0] + m[1] + m[2];
  o[1] = m[1] - m[2] - m[3];
}
template <typename V>
__device__ __forceinline__ void wino4_bt(const V (&d)[6], V (&o)[6]) {
  o[0] = 4.f * d[0] - 5.f * d[2] + d[4];
  o[1] = -4.f * (d[1] + d[2]) + d[3] + d[4];
  o[2] = 4.f * (d[1] - d[2]) - d[3] + d[4];
  o[3] = 2.f * (d[3] - d[1]) - d[2] + d[4];
  o[4] = 2.f * (d[1] - d[3]) - d[2] + d[4];
  o[5] = 4.f * d[1] - 5.f * d[3] + d[5];
}
template <typename V>
__device__ __forceinline__ void wino4_at(const V (&m)[6], V (&o)[4]) {
  const V s12 = m[1] + m[2], d12 = m[1] - m[2], s34 = m[3] + m[4], d34 = m[3] - m[4];
  o[0] = m[0] + s12 + s34;
  o[1] = d12 + 2.f * d34;
  o[2] = s12 + 4.f * s34;
  o[3] = d12 + 8.f * d34 + m[5];
}
template <int T, typename V>
__device__ __forceinline__ void wino_at(const V (&m)[T + 2], V (&o)[T]) {
  if constexpr (T == 4) wino4_at(m, o); else wino2_at(m, o);
}

// Item t of a grid-stride transform -> channel vector q (of CV per pixel) of tile (b, th, tw); `tile` counts over all images.
// IDX = the type the item counts in: OFF (an item count is below the byte count of a plane).
template <typename IDX>
struct WinoTile {
  int q, th, tw;
  IDX tile, b;
};
template <int T, typename IDX>
__device__ __forceinline__ WinoTile<IDX> wino_tile(IDX t, int CV, int H, int W) {
  WinoTile<IDX> w;
  w.q = (int)(t % (IDX)CV);
  w.tile = t / (IDX)CV;
  w.tw = (int)(w.tile % (IDX)(W / T));
  const IDX r = w.tile / (IDX)(W / T);
  w.th = (int)(r % (IDX)(H / T));
  w.b = r / (IDX)(H / T);
  return w;
}
// The N taps of one axis of an input tile whose first tap is `first` (-1 in the first tile: the padding), once per item: the byte
// offset of each tap's CLAMPED index (`stride` bytes per step along the axis) and whether the tap lies inside the image (MASK =
// float: 1.f / 0.f, the factor of the fused kernels, where the product of a row's and a column's factor is exact; bool: the plain
// kernels' branch).
template <int N, typename OFF, typename MASK>
__device__ __forceinline__ void wino_taps(int first, int extent, OFF stride, OFF origin, OFF (&off)[N], MASK (&in)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const int s = first + i;
    off[i] = origin + (OFF)clamp_index(s, extent) * stride;
    in[i] = (MASK)(s >= 0 && s < extent);
  }
}
// The T output positions of one axis of output tile `t`
template <int T, typename OFF>
__device__ __forceinline__ void wino_outs(int t, OFF stride, OFF origin, OFF (&off)[T]) {
#pragma unroll
  for (int i = 0; i < T; ++i) off[i] = origin + (OFF)(T * t + i) * stride;
}
// The four input transforms keep a loop body each, so that hipcc keeps all loads of a tile (F(4x4,3x3): of all columns) in
// flight: do not wrap the gather in a function shared by the plain and the fused kernels (profiles/r17).  Each body is a
// function of OFF, called by the kernel (uint32_t) and by its wide twin (uint64_t).
template <int F16X3, typename OFF>
__device__ __forceinline__ void wino_in_items(const float *__restrict__ x, void *__restrict__ V, int H, int W, int C4, long tiles,
                                              long total, float scale) {
  typedef WinoVRow<F16X3, f32x4> VR;
  const OFF px = (OFF)C4 * sizeof(f32x4), row = (OFF)W * px;          // bytes per pixel, per image row
  const OFF part = (OFF)C4 * VR::VB;
  const uint64_t plane = (uint64_t)tiles * VR::PARTS * part;
  const char *xb = reinterpret_cast<const char *>(x);
  for (OFF t = (OFF)blockIdx.x * 256 + threadIdx.x; t < (OFF)total; t += (OFF)gridDim.x * 256) {
    const WinoTile<OFF> wt = wino_tile<2>(t, C4, H, W);
    char *vk = wino_plane0(static_cast<char *>(V));
    const OFF xq = wt.b * ((OFF)H * row) + (OFF)wt.q * sizeof(f32x4);   // the item's image and channel vector
    OFF ro[4], co[4];
    bool rin[4], cin[4];
    wino_taps<4>(2 * wt.th - 1, H, row, xq, ro, rin);
    wino_taps<4>(2 * wt.tw - 1, W, px, (OFF)0, co, cin);
    f32x4 d[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        d[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (rin[i] && cin[j]) d[i][j] = *reinterpret_cast<const f32x4 *>(xb + (OFF)(ro[i] + co[j]));
      }
    f32x4 w[4][4];   // B^T d
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      w[0][j] = d[0][j] - d[2][j];
      w[1][j] = d[1][j] + d[2][j];
      w[2][j] = d[2][j] - d[1][j];
      w[3][j] = d[1][j] - d[3][j];
    }
    const OFF at = wt.tile * (VR::PARTS * part) + (OFF)wt.q * VR::VB;
#pragma unroll
    for (int i = 0; i < 4; ++i) {   // (B^T d) B, each value stored as it is formed; vk walks the planes 4 i + j
      wino_store_v<F16X3>(vk, at, part, w[i][0] - w[i][2], scale);
      vk += plane;
      wino_store_v<F16X3>(vk, at, part, w[i][1] + w[i][2], scale);
      vk += plane;
      wino_store_v<F16X3>(vk, at, part, w[i][2] - w[i][1], scale);
      vk += plane;
      wino_store_v<F16X3>(vk, at, part, w[i][1] - w[i][3], scale);
      vk += plane;
    }
  }
}
// fp32 V (F16X3 = 0) keeps the per-access 64-bit indexing at every shape, in the kernel and in its wide twin: with the offsets of an item formed once hipcc takes 81
// instead of 79 registers for this kernel, a wave per SIMD fewer (profiles/r20).
__device__ __forceinline__ void wino_in_items_f32(const float *__restrict__ x, float *__restrict__ V, int H, int W, int C4,
                                                  long tiles, long total) {
  for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
    const WinoTile<long> wt = wino_tile<2>(t, C4, H, W);
    f32x4 d[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int sy = 2 * wt.th - 1 + i, sx = 2 * wt.tw - 1 + j;
        d[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (sy >= 0 && sy < H && sx >= 0 && sx < W)
          d[i][j] = reinterpret_cast<const f32x4 *>(x)[((wt.b * H + sy) * W + sx) * C4 + wt.q];
      }
    f32x4 w[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      w[0][j] = d[0][j] - d[2][j];
      w[1][j] = d[1][j] + d[2][j];
      w[2][j] = d[2][j] - d[1][j];
      w[3][j] = d[1][j] - d[3][j];
    }
    f32x4 *v = reinterpret_cast<f32x4 *>(V);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[((long)(4 * i + 0) * tiles + wt.tile) * C4 + wt.q] = w[i][0] - w[i][2];
      v[((long)(4 * i + 1) * tiles + wt.tile) * C4 + wt.q] = w[i][1] + w[i][2];
      v[((long)(4 * i + 2) * tiles + wt.tile) * C4 + wt.q] = w[i][2] - w[i][1];
      v[((long)(4 * i + 3) * tiles + wt.tile) * C4 + wt.q] = w[i][1] - w[i][3];
    }
  }
}
template <int F16X3>
__global__ __launch_bounds__(256) void wino_in_nhwc_kernel(const float *__restrict__ x, void *__restrict__ V, int H, int W,
                                                           int C4, long tiles, long total, float scale) {
  if constexpr (F16X3 == 0) wino_in_items_f32(x, static_cast<float *>(V), H, W, C4, tiles, total);
  else wino_in_items<F16X3, uint32_t>(x, V, H, W, C4, tiles, total, scale);
}
template <int F16X3>
__global__ __launch_bounds__(256) void wino_in_nhwc_wide_kernel(const float *__restrict__ x, void *__restrict__ V, int H, int W,
                                                                int C4, long tiles, long total, float scale) {
  if constexpr (F16X3 == 0) wino_in_items_f32(x, static_cast<float *>(V), H, W, C4, tiles, total);
  else wino_in_items<F16X3, uint64_t>(x, V, H, W, C4, tiles, total, scale);
}

// Input transform with the producer fused in: the conv input is GroupNorm(+SiLU) of x (unet.py:140-142, :146-149), so
// the normalisation is applied to the 16 loaded values on the fly (statistics from gn_stats / add_bias_stats) and the
// normalised tensor is never written: saves gn_apply's write and this kernel's read of it.  Zero padding applies to the
// ACTIVATED tensor, so out-of-bounds taps stay exactly 0.
template <int SILU, int F16X3, typename OFF>
__device__ __forceinline__ void wino_in_gn_items(const float *__restrict__ x, const float *__restrict__ gamma,
                                                 const float *__restrict__ beta, const float *__restrict__ pre_bias,
                                                 const int64_t *__restrict__ stats, void *__restrict__ V, int H, int W, int C4,
                                                 int cpg, double eps, long tiles, long total, float scale) {
  typedef WinoVRow<F16X3, f32x4> VR;
  const int groups = 4 * C4 / cpg;
  const OFF px = (OFF)C4 * sizeof(f32x4), row = (OFF)W * px;
  const OFF part = (OFF)C4 * VR::VB;
  const uint64_t plane = (uint64_t)tiles * VR::PARTS * part;
  const char *xb = reinterpret_cast<const char *>(x);
  for (OFF t = (OFF)blockIdx.x * 256 + threadIdx.x; t < (OFF)total; t += (OFF)gridDim.x * 256) {
    const WinoTile<OFF> wt = wino_tile<2>(t, C4, H, W);
    char *vk = wino_plane0(static_cast<char *>(V));
    const int g = (4 * wt.q) / cpg;
    const GnGroup gg = gn_group(stats + kStatWords * ((long)wt.b * groups + g), (double)cpg * (double)H * (double)W, eps);
    f32x4 a, sh;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const GnAffine f = gn_channel(gg, gamma, beta, pre_bias, 4 * wt.q + k);
      a[k] = f.a;
      sh[k] = f.sh;
    }
    const OFF xq = wt.b * ((OFF)H * row) + (OFF)wt.q * sizeof(f32x4);   // the item's image and channel vector
    OFF ro[4], co[4];
    float rin[4], cin[4];
    wino_taps<4>(2 * wt.th - 1, H, row, xq, ro, rin);
    wino_taps<4>(2 * wt.tw - 1, W, px, (OFF)0, co, cin);
    f32x4 d[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        // no branch around the load: the 16 loads must all be in flight before the first activation (with the
        // activation inside an `if` hipcc keeps 16 load -> wait -> compute rounds: measured 965 vs 765 us); taps outside
        // the image read a clamped address and are zeroed afterwards
        d[i][j] = *reinterpret_cast<const f32x4 *>(xb + (OFF)(ro[i] + co[j]));
      }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float inb = rin[i] * cin[j];   // 1.f or 0.f, exactly
        d[i][j] = gn_act<SILU>(d[i][j], a, sh) * inb;
      }
    f32x4 w[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      w[0][j] = d[0][j] - d[2][j];
      w[1][j] = d[1][j] + d[2][j];
      w[2][j] = d[2][j] - d[1][j];
      w[3][j] = d[1][j] - d[3][j];
    }
    const OFF at = wt.tile * (VR::PARTS * part) + (OFF)wt.q * VR::VB;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      wino_store_v<F16X3>(vk, at, part, w[i][0] - w[i][2], scale);
      vk += plane;
      wino_store_v<F16X3>(vk, at, part, w[i][1] + w[i][2], scale);
      vk += plane;
      wino_store_v<F16X3>(vk, at, part, w[i][2] - w[i][1], scale);
      vk += plane;
      wino_store_v<F16X3>(vk, at, part, w[i][1] - w[i][3], scale);
      vk += plane;
    }
  }
}
#define GQ_WINO_GN_ARGS                                                                                                        \
  const float *__restrict__ x, const float *__restrict__ gamma, const float *__restrict__ beta,                               \
      const float *__restrict__ pre_bias, const int64_t *__restrict__ stats, void *__restrict__ V, int H, int W, int CV, int cpg, \
      double eps, long tiles, long total, float scale
template <int SILU, int F16X3>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 4))) void wino_in_gn_nhwc_kernel(GQ_WINO_GN_ARGS) {
  wino_in_gn_items<SILU, F16X3, uint32_t>(x, gamma, beta, pre_bias, stats, V, H, W, CV, cpg, eps, tiles, total, scale);
}
template <int SILU, int F16X3>
__global__ __launch_bounds__(256) void wino_in_gn_nhwc_wide_kernel(GQ_WINO_GN_ARGS) {
  wino_in_gn_items<SILU, F16X3, uint64_t>(x, gamma, beta, pre_bias, stats, V, H, W, CV, cpg, eps, tiles, total, scale);
}

template <int F16X3, typename OFF>
__device__ __forceinline__ void wino4_in_items(const float *__restrict__ x, void *__restrict__ V, int H, int W, int C4, long tiles,
                                               long total, float scale) {
  typedef WinoVRow<F16X3, f32x4> VR;
  const OFF px = (OFF)C4 * sizeof(f32x4), row = (OFF)W * px;
  const OFF part = (OFF)C4 * VR::VB;
  const uint64_t plane = (uint64_t)tiles * VR::PARTS * part;
  const char *xb = reinterpret_cast<const char *>(x);
  for (OFF t = (OFF)blockIdx.x * 256 + threadIdx.x; t < (OFF)total; t += (OFF)gridDim.x * 256) {
    const WinoTile<OFF> wt = wino_tile<4>(t, C4, H, W);
    char *vk = wino_plane0(static_cast<char *>(V));
    const OFF xq = wt.b * ((OFF)H * row) + (OFF)wt.q * sizeof(f32x4);   // the item's image and channel vector
    OFF ro[6], co[6];
    bool rin[6], cin[6];
    wino_taps<6>(4 * wt.th - 1, H, row, xq, ro, rin);
    wino_taps<6>(4 * wt.tw - 1, W, px, (OFF)0, co, cin);
    f32x4 w[6][6];   // B^T d, column by column
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      f32x4 col[6], o[6];
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        col[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (rin[i] && cin[j]) col[i] = *reinterpret_cast<const f32x4 *>(xb + (OFF)(ro[i] + co[j]));
      }
      wino4_bt(col, o);
#pragma unroll
      for (int i = 0; i < 6; ++i) w[i][j] = o[i];
    }
    const OFF at = wt.tile * (VR::PARTS * part) + (OFF)wt.q * VR::VB;
#pragma unroll
    for (int i = 0; i < 6; ++i) {   // (B^T d) B, row by row; vk walks the planes 6 i + j
      f32x4 o[6];
      wino4_bt(w[i], o);
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        wino_store_v<F16X3>(vk, at, part, o[j], scale);
        vk += plane;
      }
    }
  }
}
template <int F16X3>
__global__ __launch_bounds__(256) void wino4_in_nhwc_kernel(const float *__restrict__ x, void *__restrict__ V, int H, int W,
                                                            int C4, long tiles, long total, float scale) {
  wino4_in_items<F16X3, uint32_t>(x, V, H, W, C4, tiles, total, scale);
}
template <int F16X3>
__global__ __launch_bounds__(256) void wino4_in_nhwc_wide_kernel(const float *__restrict__ x, void *__restrict__ V, int H, int W,
                                                                 int C4, long tiles, long total, float scale) {
  wino4_in_items<F16X3, uint64_t>(x, V, H, W, C4, tiles, total, scale);
}

// wino4_in_nhwc_kernel with the producer fused in (see wino_in_gn_nhwc_kernel): every pixel is activated by the 2.25 tiles
// that overlap it.  VW = channels per thread: with 4 the 36 x 4 values of a tile plus the activation's temporaries take
// ~250 registers (two waves per SIMD, the activations' VALU time shows: 399 vs 304 us for the plain transform); with 2
// (whenever a 256-thread block still spans whole pixels) twice the waves hide it.
template <int SILU, int F16X3, int VW, typename OFF>
__device__ __forceinline__ void wino4_in_gn_items(const float *__restrict__ x, const float *__restrict__ gamma,
                                                  const float *__restrict__ beta, const float *__restrict__ pre_bias,
                                                  const int64_t *__restrict__ stats, void *__restrict__ V, int H, int W, int CV,
                                                  int cpg, double eps, long tiles, long total, float scale) {
  typedef float vec __attribute__((ext_vector_type(VW)));
  typedef WinoVRow<F16X3, vec> VR;
  const int groups = VW * CV / cpg;
  const OFF px = (OFF)CV * sizeof(vec), row = (OFF)W * px;
  const OFF part = (OFF)CV * VR::VB;
  const uint64_t plane = (uint64_t)tiles * VR::PARTS * part;
  const char *xb = reinterpret_cast<const char *>(x);
  for (OFF t = (OFF)blockIdx.x * 256 + threadIdx.x; t < (OFF)total; t += (OFF)gridDim.x * 256) {
    const WinoTile<OFF> wt = wino_tile<4>(t, CV, H, W);
    char *vk = wino_plane0(static_cast<char *>(V));
    const int g = (VW * wt.q) / cpg;
    const GnGroup gg = gn_group(stats + kStatWords * ((long)wt.b * groups + g), (double)cpg * (double)H * (double)W, eps);
    vec a, sh;
#pragma unroll
    for (int k = 0; k < VW; ++k) {
      const GnAffine f = gn_channel(gg, gamma, beta, pre_bias, VW * wt.q + k);
      a[k] = f.a;
      sh[k] = f.sh;
    }
    const OFF xq = wt.b * ((OFF)H * row) + (OFF)wt.q * sizeof(vec);   // the item's image and channel vector
    OFF ro[6], co[6];
    float rin[6], cin[6];
    wino_taps<6>(4 * wt.th - 1, H, row, xq, ro, rin);
    wino_taps<6>(4 * wt.tw - 1, W, px, (OFF)0, co, cin);
    vec w[6][6];
    vec nxt[6];   // column j + 1 is loaded before column j is activated: six loads in flight under every activation
#pragma unroll
    for (int i = 0; i < 6; ++i) nxt[i] = *reinterpret_cast<const vec *>(xb + (OFF)(ro[i] + co[0]));   // branch-free: see wino_in_gn_nhwc_kernel
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      vec col[6], o[6];
#pragma unroll
      for (int i = 0; i < 6; ++i) col[i] = nxt[i];
      if (j + 1 < 6) {
#pragma unroll
        for (int i = 0; i < 6; ++i) nxt[i] = *reinterpret_cast<const vec *>(xb + (OFF)(ro[i] + co[j + 1]));
      }
      __builtin_amdgcn_sched_barrier(0);   // (hipcc otherwise sinks the loads into the activation: two or three in flight)
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        const float inb = rin[i] * cin[j];   // 1.f or 0.f, exactly
        col[i] = gn_act<SILU>(col[i], a, sh) * inb;
      }
      wino4_bt(col, o);
#pragma unroll
      for (int i = 0; i < 6; ++i) w[i][j] = o[i];
    }
    const OFF at = wt.tile * (VR::PARTS * part) + (OFF)wt.q * VR::VB;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      vec o[6];
      wino4_bt(w[i], o);
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        wino_store_v<F16X3>(vk, at, part, o[j], scale);
        vk += plane;
      }
    }
  }
}
// fp32 V (F16X3 = 0, four channels per thread) keeps the per-access 64-bit indexing at every shape, in the kernel and in its wide twin: with the offsets of an item
// formed once hipcc takes 235-251 instead of 173 registers for this kernel (profiles/r20).
template <int SILU>
__device__ __forceinline__ void wino4_in_gn_items_f32(const float *__restrict__ x, const float *__restrict__ gamma,
                                                      const float *__restrict__ beta, const float *__restrict__ pre_bias,
                                                      const int64_t *__restrict__ stats, float *__restrict__ V, int H, int W,
                                                      int CV, int cpg, double eps, long tiles, long total) {
  const int groups = 4 * CV / cpg;
  for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
    const WinoTile<long> wt = wino_tile<4>(t, CV, H, W);
    const int g = (4 * wt.q) / cpg;
    const GnGroup gg = gn_group(stats + kStatWords * (wt.b * groups + g), (double)cpg * (double)H * (double)W, eps);
    f32x4 a, sh;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const GnAffine f = gn_channel(gg, gamma, beta, pre_bias, 4 * wt.q + k);
      a[k] = f.a;
      sh[k] = f.sh;
    }
    f32x4 w[6][6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      f32x4 col[6], o[6];
      const int sx = 4 * wt.tw - 1 + j;
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        const int sy = 4 * wt.th - 1 + i;
        const int cy = clamp_index(sy, H), cx = clamp_index(sx, W);
        col[i] = reinterpret_cast<const f32x4 *>(x)[((wt.b * H + cy) * W + cx) * CV + wt.q];
      }
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        const int sy = 4 * wt.th - 1 + i;
        const float inb = (sy >= 0 && sy < H && sx >= 0 && sx < W) ? 1.f : 0.f;
        col[i] = gn_act<SILU>(col[i], a, sh) * inb;
      }
      wino4_bt(col, o);
#pragma unroll
      for (int i = 0; i < 6; ++i) w[i][j] = o[i];
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      f32x4 o[6];
      wino4_bt(w[i], o);
#pragma unroll
      for (int j = 0; j < 6; ++j) reinterpret_cast<f32x4 *>(V)[((long)(6 * i + j) * tiles + wt.tile) * CV + wt.q] = o[j];
    }
  }
}
template <int SILU, int F16X3, int VW>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(VW == 2 ? (SILU ? 3 : 4) : 1, VW == 2 ? 4 : 8))) void wino4_in_gn_nhwc_kernel(GQ_WINO_GN_ARGS) {
  if constexpr (F16X3 == 0)
    wino4_in_gn_items_f32<SILU>(x, gamma, beta, pre_bias, stats, static_cast<float *>(V), H, W, CV, cpg, eps, tiles, total);
  else
    wino4_in_gn_items<SILU, F16X3, VW, uint32_t>(x, gamma, beta, pre_bias, stats, V, H, W, CV, cpg, eps, tiles, total, scale);
}
template <int SILU, int F16X3, int VW>
__global__ __launch_bounds__(256) void wino4_in_gn_nhwc_wide_kernel(GQ_WINO_GN_ARGS) {
  if constexpr (F16X3 == 0)
    wino4_in_gn_items_f32<SILU>(x, gamma, beta, pre_bias, stats, static_cast<float *>(V), H, W, CV, cpg, eps, tiles, total);
  else
    wino4_in_gn_items<SILU, F16X3, VW, uint64_t>(x, gamma, beta, pre_bias, stats, V, H, W, CV, cpg, eps, tiles, total, scale);
}
#undef GQ_WINO_GN_ARGS

// "Load M, A^T M" of one output tile, shared by the three output transforms: the N x N values M of the tile (mi = its channel
// vector in plane 0, `plane` vectors per plane) -> u = A^T M; the caller finishes y = u A row by row (wino_at on u[i]) as it
// stores.  NJ = columns of M loaded before they are transformed: all N in the plain F(2x2,3x3) kernel, 1 (column by column)
// elsewhere -- the order each kernel had, which is the order hipcc schedules by.
// Addressing: m0 = plane 0 of M, at = the item's byte offset in a plane, plane = bytes per plane; the plane pointers cj (plane
// j0), pi (plane N i + j0) and pk are wave-uniform and advance by additions.
template <int T, int NJ, typename VEC, typename OFF>
__device__ __forceinline__ void wino_out_cols(const char *m0, OFF at, uint64_t plane, VEC (&u)[T][T + 2]) {
  constexpr int N = T + 2;
  const char *cj = m0;
#pragma unroll
  for (int j0 = 0; j0 < N; j0 += NJ) {
    VEC m[NJ][N];   // NJ columns
    const char *pi = cj;
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const char *pk = pi;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        m[j][i] = *reinterpret_cast<const VEC *>(pk + at);
        pk += plane;
      }
      pi += N * plane;
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      VEC o[T];
      wino_at<T>(m[j], o);
#pragma unroll
      for (int i = 0; i < T; ++i) u[i][j0 + j] = o[i];
    }
    cj += NJ * plane;
  }
}
// The same with per-access 64-bit indexing (mi = the item's channel vector in plane 0, `plane` vectors per plane), for the output
// kernels that keep it: wino4_out_nhwc_kernel and wino_out_res_nhwc_kernel<4, *>.
template <int T, int NJ, typename VEC>
__device__ __forceinline__ void wino_out_cols(const VEC *mi, long plane, VEC (&u)[T][T + 2]) {
  constexpr int N = T + 2;
#pragma unroll
  for (int j0 = 0; j0 < N; j0 += NJ) {
    VEC m[NJ][N];   // NJ columns
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j) m[j][i] = mi[(N * i + j0 + j) * plane];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      VEC o[T];
      wino_at<T>(m[j], o);
#pragma unroll
      for (int i = 0; i < T; ++i) u[i][j0 + j] = o[i];
    }
  }
}

// The plain output transforms.  `mscale`: M came out of a GEMM on scaled operands (the f16x3 path): y = mscale * (A^T M A);
// 1 otherwise (a power of two).
template <int T, int NJ, typename OFF>
__device__ __forceinline__ void wino_out_items(const float *__restrict__ M, float *__restrict__ y, int H, int W, int C4, long tiles,
                                               long total, float mscale) {
  const OFF px = (OFF)C4 * sizeof(f32x4), row = (OFF)W * px;
  const uint64_t plane = (uint64_t)tiles * px;
  char *yb = reinterpret_cast<char *>(y);
  for (OFF t = (OFF)blockIdx.x * 256 + threadIdx.x; t < (OFF)total; t += (OFF)gridDim.x * 256) {
    const WinoTile<OFF> wt = wino_tile<T>(t, C4, H, W);
    f32x4 u[T][T + 2];   // A^T m
    wino_out_cols<T, NJ>(wino_plane0(reinterpret_cast<const char *>(M)), (OFF)(wt.tile * px + (OFF)wt.q * sizeof(f32x4)), plane, u);
    OFF ro[T], co[T];
    wino_outs<T>(wt.th, row, (OFF)(wt.b * ((OFF)H * row) + (OFF)wt.q * sizeof(f32x4)), ro);
    wino_outs<T>(wt.tw, px, (OFF)0, co);
#pragma unroll
    for (int i = 0; i < T; ++i) {
      f32x4 o[T];
      wino_at<T>(u[i], o);
#pragma unroll
      for (int j = 0; j < T; ++j) *reinterpret_cast<f32x4 *>(yb + (OFF)(ro[i] + co[j])) = o[j] * mscale;
    }
  }
}
#define GQ_WINO_OUT_ARGS const float *__restrict__ M, float *__restrict__ y, int H, int W, int C4, long tiles, long total, float mscale
__global__ __launch_bounds__(256) void wino_out_nhwc_kernel(GQ_WINO_OUT_ARGS) {
  wino_out_items<2, 4, uint32_t>(M, y, H, W, C4, tiles, total, mscale);
}
__global__ __launch_bounds__(256) void wino_out_nhwc_wide_kernel(GQ_WINO_OUT_ARGS) {
  wino_out_items<2, 4, uint64_t>(M, y, H, W, C4, tiles, total, mscale);
}
#undef GQ_WINO_OUT_ARGS
// F(4x4,3x3) keeps the per-access 64-bit indexing at every shape (no wide twin): re-addressed, hipcc ran it at 161 registers with
// 16 + 6 loads in flight where this form has 31 at 254 -- fewer loads in flight per SIMD, and bench.py has no call of it to time.
// (decode written out: wino_tile costs this kernel, at 254 VGPRs, a scalar register -- profiles/r17)
__global__ __launch_bounds__(256) void wino4_out_nhwc_kernel(const float *__restrict__ M, float *__restrict__ y, int H, int W,
                                                             int C4, long tiles, long total, float mscale) {
  for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
    const int q = (int)(t % C4);
    const long tile = t / C4;
    const int tw = (int)(tile % (W / 4));
    const long r = tile / (W / 4);
    const int th = (int)(r % (H / 4));
    const long b = r / (H / 4);
    const f32x4 *mi = reinterpret_cast<const f32x4 *>(M) + tile * C4 + q;
    const long plane = tiles * C4;
    f32x4 u[4][6];   // A^T m
    wino_out_cols<4, 1>(mi, plane, u);
    f32x4 *out = reinterpret_cast<f32x4 *>(y) + ((b * H + 4 * th) * W + 4 * tw) * C4 + q;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      f32x4 o[4];
      wino4_at(u[i], o);
#pragma unroll
      for (int j = 0; j < 4; ++j) out[((long)i * W + j) * C4] = o[j] * mscale;
    }
  }
}

// Output transform with the ResnetBlock's tail fused in (unet.py:149-153): y = A^T M A + bias[c] (+ res), and the GroupNorm
// statistics of y for the block that follows (as add_bias_stats_nhwc_kernel).  A block owns a range of tiles of ONE
// image; thread -> channel quad q = tid % C4 (one GroupNorm group), tile lane = tid / C4.  T = 2: F(2x2,3x3), 4: F(4x4,3x3).
// VW = channels per thread: 4 (16-byte accesses), or 2 for F(4x4,3x3) -- with 4 the 36 loads of M, the 24 intermediate
// values and the 16 residual loads of a tile do not fit 256 registers, the residual is loaded late, one wave per SIMD
// waits for it 16 times (585 us at 16 x 256 x 256 x 128, 3.9 TB/s); with 2 everything is in flight at once at two waves
// per SIMD and an access of a wave is still whole 128-byte lines (64 lanes x 8 bytes = the 128 channels of a pixel).
// Addressing: the image is the block's, so the image bases of res and y are wave-uniform like the planes of M and advance row by
// row on the scalar side; a thread keeps the offset of its tile in a plane of M and T column offsets (its channel vector included).
template <int T, int VW, typename OFF>
__device__ __forceinline__ void wino_out_res_items(const float *__restrict__ M, const float *__restrict__ res,
                                                   const float *__restrict__ bias, float *__restrict__ y,
                                                   int64_t *__restrict__ stats, int H, int W, int CV, int cpg, long tiles, int slabs,
                                                   float mscale) {
  typedef float vec __attribute__((ext_vector_type(VW)));
  __shared__ int64_t red[kStatWords * 64];   // per-group statistics records (gq_stats.h)
  const int groups = VW * CV / cpg, lanes = 256 / CV;
  const long b = blockIdx.x / slabs;
  const int slab = blockIdx.x % slabs;
  const long tpi = (long)(H / T) * (W / T);           // tiles per image
  const long per = (tpi + slabs - 1) / slabs;
  const long lo = slab * per, hi = lo + per < tpi ? lo + per : tpi;
  const int q = threadIdx.x % CV, tl = threadIdx.x / CV;
  for (int w = threadIdx.x; w < kStatWords * groups; w += 256) red[w] = 0;
  __syncthreads();
  vec pb = (vec)(0.f);
  if (bias) pb = reinterpret_cast<const vec *>(bias)[q];
  const OFF px = (OFF)CV * sizeof(vec), row = (OFF)W * px;
  const uint64_t plane = (uint64_t)tiles * px, image = (uint64_t)H * row;
  const char *resb = reinterpret_cast<const char *>(res) + (uint64_t)b * image;
  char *yb = reinterpret_cast<char *>(y) + (uint64_t)b * image;
  const OFF qb = (OFF)q * sizeof(vec), mrow = (OFF)(b * tpi) * px + qb;   // tile 0 of the image in a plane of M
  StatPartial st;
  for (OFF ti = (OFF)(lo + tl); ti < (OFF)hi; ti += (OFF)lanes) {
    const int tw = (int)(ti % (OFF)(W / T)), th = (int)(ti / (OFF)(W / T));
    const char *m0 = wino_plane0(reinterpret_cast<const char *>(M));
    OFF pj[T];   // the tile's first row, its column j, the thread's channel vector
#pragma unroll
    for (int j = 0; j < T; ++j) pj[j] = (OFF)(T * th) * row + (OFF)(T * tw + j) * px + qb;
    vec r[T][T];
    if (res) {   // wave-uniform; issued ahead of M so that nothing waits for it at the end
#pragma unroll
      for (int i = 0; i < T; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j)
          r[i][j] = *reinterpret_cast<const vec *>(resb + (uint64_t)i * row + pj[j]);
    } else {
#pragma unroll
      for (int i = 0; i < T; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j) r[i][j] = (vec)(0.f);
    }
    vec u[T][T + 2];
    wino_out_cols<T, 1>(m0, (OFF)(mrow + ti * px), plane, u);
#pragma unroll
    for (int i = 0; i < T; ++i) {
      vec o[T];
      wino_at<T>(u[i], o);
#pragma unroll
      for (int j = 0; j < T; ++j) {
        vec v = o[j] * mscale + pb;
        if (res) v = v + r[i][j];
        *reinterpret_cast<vec *>(yb + (uint64_t)i * row + pj[j]) = v;
        stat_partial_add_vec(st, v);
      }
    }
  }
  const int g = (VW * q) / cpg;
  stat_partial_flush(red + kStatWords * g, st);
  __syncthreads();
  for (int w = threadIdx.x; w < kStatWords * groups; w += 256) stat_flush_word(stats + kStatWords * (b * groups) + w, red[w]);
}
#define GQ_WINO_RES_ARGS                                                                                                        \
  const float *__restrict__ M, const float *__restrict__ res, const float *__restrict__ bias, float *__restrict__ y,          \
      int64_t *__restrict__ stats, int H, int W, int CV, int cpg, long tiles, int slabs, float mscale
// F(4x4,3x3) keeps the per-access 64-bit indexing -- the kernel template below, as it was; it has no wide twin: with the offsets
// formed once wino_out_res_nhwc_kernel<4, 2> was not faster on MI355X (98.2 against 98.0-100.2 us per call, whether its 52 loads
// were all in flight at three waves per SIMD or column by column at four: profiles/r20/kernel_times.txt) -- its VALU is idle 85 %
// of the time (profiles/r20/pmc_before.txt) -- and <4, 4> is not run by the step.  (The body stands in the kernel, not in a
// function the kernel calls: called, hipcc gives <4, 4> 306 instead of 276 registers and 14 spills.)
template <int T, int VW>
__global__ __launch_bounds__(256) void wino_out_res_nhwc_kernel(const float *__restrict__ M, const float *__restrict__ res,
                                                                const float *__restrict__ bias, float *__restrict__ y,
                                                                int64_t *__restrict__ stats, int H, int W, int CV,
                                                                int cpg, long tiles, int slabs, float mscale) {
  typedef float vec __attribute__((ext_vector_type(VW)));
  __shared__ int64_t red[kStatWords * 64];   // per-group statistics records (gq_stats.h)
  const int groups = VW * CV / cpg, lanes = 256 / CV;
  const long b = blockIdx.x / slabs;
  const int slab = blockIdx.x % slabs;
  const long tpi = (long)(H / T) * (W / T);           // tiles per image
  const long per = (tpi + slabs - 1) / slabs;
  const long lo = slab * per, hi = lo + per < tpi ? lo + per : tpi;
  const int q = threadIdx.x % CV, tl = threadIdx.x / CV;
  for (int w = threadIdx.x; w < kStatWords * groups; w += 256) red[w] = 0;
  __syncthreads();
  vec pb = (vec)(0.f);
  if (bias) pb = reinterpret_cast<const vec *>(bias)[q];
  const long plane = tiles * CV;
  StatPartial st;
  for (long ti = lo + tl; ti < hi; ti += lanes) {
    const int tw = (int)(ti % (W / T)), th = (int)(ti / (W / T));
    const vec *mi = reinterpret_cast<const vec *>(M) + (b * tpi + ti) * CV + q;
    const long pix0 = ((b * H + (long)T * th) * W + (long)T * tw) * CV + q;
    vec r[T][T];
    if (res) {   // wave-uniform; issued ahead of M so that nothing waits for it at the end
#pragma unroll
      for (int i = 0; i < T; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j) r[i][j] = reinterpret_cast<const vec *>(res)[pix0 + ((long)i * W + j) * CV];
    } else {
#pragma unroll
      for (int i = 0; i < T; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j) r[i][j] = (vec)(0.f);
    }
    vec u[T][T + 2];
    wino_out_cols<T, 1>(mi, plane, u);
#pragma unroll
    for (int i = 0; i < T; ++i) {
      vec o[T];
      wino_at<T>(u[i], o);
#pragma unroll
      for (int j = 0; j < T; ++j) {
        const long off = pix0 + ((long)i * W + j) * CV;
        vec v = o[j] * mscale + pb;
        if (res) v = v + r[i][j];
        reinterpret_cast<vec *>(y)[off] = v;
        stat_partial_add_vec(st, v);
      }
    }
  }
  const int g = (VW * q) / cpg;
  stat_partial_flush(red + kStatWords * g, st);
  __syncthreads();
  for (int w = threadIdx.x; w < kStatWords * groups; w += 256) stat_flush_word(stats + kStatWords * (b * groups) + w, red[w]);
}
// F(2x2,3x3): the strength-reduced form
template <>
__global__ __launch_bounds__(256) void wino_out_res_nhwc_kernel<2, 4>(GQ_WINO_RES_ARGS) {
  wino_out_res_items<2, 4, uint32_t>(M, res, bias, y, stats, H, W, CV, cpg, tiles, slabs, mscale);
}
template <int T, int VW>
__global__ __launch_bounds__(256) void wino_out_res_nhwc_wide_kernel(GQ_WINO_RES_ARGS) {
  static_assert(T == 2, "F(4x4,3x3) has one kernel");
  wino_out_res_items<T, VW, uint64_t>(M, res, bias, y, stats, H, W, CV, cpg, tiles, slabs, mscale);
}
#undef GQ_WINO_RES_ARGS

// scales[0] = v_scale = the largest power of two with amp * bound * v_scale <= 32768, bound = sqrt(max over (image,
// group) of the sum of squares) >= max|x| (rigorous: the L2 norm of a group bounds its largest element), from the
// GroupNorm statistics [2 * n_bg] (sum, sum of squares) the producer of x left behind; scales[1] = 1 / (v_scale * u_scale),
// the factor that takes the GEMM result back.  One wave.
__global__ __launch_bounds__(64) void f16_scales_from_stats_kernel(const int64_t *__restrict__ stats, int n_bg, float amp,
                                                                   float u_scale, float *__restrict__ scales) {
  double m = 0.0;
  for (int i = threadIdx.x; i < n_bg; i += 64) {
    double sum_unused, ss;
    stat_load(stats + kStatWords * i, sum_unused, ss);
    m = (ss != ss) ? __builtin_inf() : (ss > m ? ss : m);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double other = __shfl_xor(m, o);
    m = other > m ? other : m;
  }
  if (threadIdx.x == 0) {
    const double bound = sqrt(m) * (double)amp;
    int e = 14;                                        // never scale UP by more than 2^14
    if (bound > 0.0 && bound < 1e300) {
      int eb;
      (void)frexp(32768.0 / bound, &eb);               // 32768 / bound = f * 2^eb, f in [0.5, 1)
      e = eb - 1 < 14 ? eb - 1 : 14;
    }
    const float vs = (float)ldexp(1.0, e);
    scales[0] = vs;
    scales[1] = (float)(1.0 / ((double)vs * (double)u_scale));
  }
}

// y = a + b (+ bias[c]): the residual add of a ResnetBlock with the pending conv biases folded in.
__global__ __launch_bounds__(256) void add_bias_kernel(const float *__restrict__ a, const float *__restrict__ b,
                                                       const float *__restrict__ bias, float *__restrict__ y, int C,
                                                       long HW, long total4) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total4; i += (long)gridDim.x * 256) {
    f32x4 v = reinterpret_cast<const f32x4 *>(a)[i] + reinterpret_cast<const f32x4 *>(b)[i];
    if (bias) v = v + bias[(int)(((i * 4) / HW) % C)];
    reinterpret_cast<f32x4 *>(y)[i] = v;
  }
}

// ---- fused GroupNorm (+SiLU), NCHW fp32 --------------------------------------------
// stats: each block reduces a contiguous slice of one (b, g) chunk; shifted fp64 per-thread partials (gq_stats.h:
// StatPartial), fp64 across the block's threads in a fixed order, the exact limb sum across blocks.
// pre_bias (nullable, [C]): a per-channel bias still pending on x (the producing conv ran without
// its bias); it is added on the fly so the separate bias pass disappears.
__global__ __launch_bounds__(256) void gn_stats_kernel(const float *__restrict__ x, const float *__restrict__ pre_bias,
                                                       int64_t *__restrict__ stats, long chunk, int slices, long HW,
                                                       int cpg, int groups) {
  const long bg = blockIdx.x / slices;
  const int sl = blockIdx.x % slices;
  const long per = ((chunk / 4 + slices - 1) / slices) * 4;      // floats per slice (multiple of 4)
  const long lo = sl * per, hi = lo + per < chunk ? lo + per : chunk;
  const float *base = x + bg * chunk;
  const int c0 = (int)(bg % groups) * cpg;
  StatPartial st;
  for (long i = lo + threadIdx.x * 4; i + 3 < hi; i += 256 * 4) {
    f32x4 v = *reinterpret_cast<const f32x4 *>(base + i);
    if (pre_bias) v = v + pre_bias[c0 + (int)(i / HW)];
    stat_partial_add_vec(st, v);
  }
  double ds, dq;
  stat_partial_moments(st, ds, dq);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    ds += __shfl_xor(ds, o);
    dq += __shfl_xor(dq, o);
  }
  __shared__ double sh[8];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sh[wave] = ds; sh[4 + wave] = dq; }
  __syncthreads();
  if (threadIdx.x == 0)   // the block's sums in a fixed order, then order-independent across blocks (gq_stats.h)
    stat_add(stats + kStatWords * bg, (sh[0] + sh[1]) + (sh[2] + sh[3]), (sh[4] + sh[5]) + (sh[6] + sh[7]));
}

template <int SILU>
__global__ __launch_bounds__(256) void gn_apply_kernel(const float *__restrict__ x, const float *__restrict__ gamma,
                                                       const float *__restrict__ beta, float *__restrict__ y,
                                                       const int64_t *__restrict__ stats,
                                                       const float *__restrict__ pre_bias, int C, long HW, int cpg,
                                                       double eps, int segs) {
  const long row = blockIdx.x / segs;          // (b, c)
  const int seg = blockIdx.x % segs;
  const int c = (int)(row % C);
  const long b = row / C;
  const long bg = b * (C / cpg) + c / cpg;
  const GnAffine f = gn_channel(gn_group(stats + kStatWords * bg, (double)cpg * (double)HW, eps), gamma, beta, pre_bias, c);
  const long per = ((HW / 4 + segs - 1) / segs) * 4;
  const long lo = seg * per, hi = lo + per < HW ? lo + per : HW;
  const float *xi = x + row * HW;
  float *yo = y + row * HW;
  for (long i = lo + threadIdx.x * 4; i + 3 < hi; i += 256 * 4)
    *reinterpret_cast<f32x4 *>(yo + i) = gn_act<SILU>(*reinterpret_cast<const f32x4 *>(xi + i), (f32x4)(f.a), (f32x4)(f.sh));
}

// ---- single-head attention of the deepest level (pit/modules/unet.py:185-206) on the fp16 matrix cores, fp32 results:
// softmax(q k^T c^-1/2) v as TWO library fp16 GEMMs with fp32 accumulation whose K axes carry the three products of
// two-term fp16 splits (the scheme of the Winograd GEMMs) instead of two fp32 GEMMs (a split-bf16 emulation on gfx950 at
// ~120 TFLOP/s).  attn_split_qkv_kernel prepares the operands of both GEMMs from the fused q|k|v projection; the softmax
// between them writes its result directly as the split operand of the second GEMM.
//   qkv [B][L][3C] fp32 (q | k | v per token)  ->  Q3 [B][L][3C] = [q_h | q_h | q_l] of q * sq
//                                                   K3 [B][L][3C] = [k_h | k_l | k_h] of k * sq     (S' = Q3 K3^T = sq^2 q k^T)
//                                                   V3 [B][3L][C] = [v_h ; v_l ; v_h] of v * sv     (rows stacked along K)
// thread = 4 channels of one token.
__global__ __launch_bounds__(256) void attn_split_qkv_kernel(const float *__restrict__ qkv, _Float16 *__restrict__ Q3,
                                                             _Float16 *__restrict__ K3, _Float16 *__restrict__ V3, long L,
                                                             int C4, float sq, float sv, long total) {
  const int C = 4 * C4;
  for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
    const int q4 = (int)(t % C4);
    const long tok = t / C4;            // b * L + l
    const long b = tok / L, l = tok % L;
    const float *src = qkv + tok * 3 * C + 4 * q4;
    f32x4 q = *reinterpret_cast<const f32x4 *>(src) * sq;
    f32x4 k = *reinterpret_cast<const f32x4 *>(src + C) * sq;
    f32x4 v = *reinterpret_cast<const f32x4 *>(src + 2 * C) * sv;
    f16x4 qh, ql, kh, kl, vh, vl;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      qh[e] = (_Float16)q[e]; ql[e] = (_Float16)(q[e] - (float)qh[e]);
      kh[e] = (_Float16)k[e]; kl[e] = (_Float16)(k[e] - (float)kh[e]);
      vh[e] = (_Float16)v[e]; vl[e] = (_Float16)(v[e] - (float)vh[e]);
    }
    f16x4 *qo = reinterpret_cast<f16x4 *>(Q3 + tok * 3 * C) + q4;
    qo[0] = qh; qo[C4] = qh; qo[2 * C4] = ql;
    f16x4 *ko = reinterpret_cast<f16x4 *>(K3 + tok * 3 * C) + q4;
    ko[0] = kh; ko[C4] = kl; ko[2 * C4] = kh;
    f16x4 *vo = reinterpret_cast<f16x4 *>(V3 + (b * 3 * L + l) * C) + q4;
    vo[0] = vh; vo[L * C4] = vl; vo[2 * L * C4] = vh;
  }
}

// Row softmax of S' * factor (factor = c^-1/2 / sq^2) written as the split operand of the second GEMM:
// P3 [rows][3L] = [p_h | p_h | p_l] of p * 2^14 (p <= 1).  One wave per row, the row in registers (L = 64 * NPL <= 4096).
template <int NPL>
__global__ __launch_bounds__(256) void attn_softmax_split_kernel(const float *__restrict__ S, _Float16 *__restrict__ P3,
                                                                 long rows, float factor) {
  constexpr int L = 64 * NPL;
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float *s = S + row * L;
  float v[NPL];
  float m = -__builtin_inff();
  if constexpr (NPL % 4 == 0) {      // lane owns runs of 4 consecutive elements: 16-byte loads, 8-byte stores
#pragma unroll
    for (int i = 0; i < NPL / 4; ++i) {
      const f32x4 x = *reinterpret_cast<const f32x4 *>(s + (i * 64 + lane) * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) { v[4 * i + e] = x[e] * factor; m = fmaxf(m, v[4 * i + e]); }
    }
  } else {
#pragma unroll
    for (int i = 0; i < NPL; ++i) { v[i] = s[i * 64 + lane] * factor; m = fmaxf(m, v[i]); }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < NPL; ++i) { v[i] = expf(v[i] - m); sum += v[i]; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
  const float inv = 16384.0f / sum;
  _Float16 *p = P3 + row * 3 * L;
  if constexpr (NPL % 4 == 0) {
#pragma unroll
    for (int i = 0; i < NPL / 4; ++i) {
      f16x4 h, l;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float x = v[4 * i + e] * inv;
        // opaque: hipcc otherwise forms h as v_fma_mixlo_f16(v, inv) -- ONE rounding of the exact product -- for the residual
        // while the stored h is the conversion of the fp32 product: at double-rounding ties h + l was one fp16 ulp off
        asm volatile("" : "+v"(x));
        h[e] = (_Float16)x; l[e] = (_Float16)(x - (float)h[e]);
      }
      f16x4 *o = reinterpret_cast<f16x4 *>(p) + i * 64 + lane;
      o[0] = h; o[L / 4] = h; o[2 * (L / 4)] = l;
    }
  } else {
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
      float x = v[i] * inv;
      asm volatile("" : "+v"(x));
      const _Float16 h = (_Float16)x;
      p[i * 64 + lane] = h; p[L + i * 64 + lane] = h; p[2 * L + i * 64 + lane] = (_Float16)(x - (float)h);
    }
  }
}

// ---- content checksums of a module's parameters (the guard of the weight-derived caches, pit_hip/modules/unet.py) ----------
// The conv stack caches data derived from the weights (Winograd U matrices, fp16 splits in MFMA operand order, rigorous
// operand bounds), keyed on (data_ptr, _version).  A write through `param.data` changes neither, so the ONLY way to notice it
// is to look at the bytes: one launch per forward sums a position-salted hash of every 32-bit word of every parameter into one
// 64-bit word per tensor (integer atomics: order-independent); the module compares the sums with those its caches were built
// from and, on a difference, rebuilds the caches and runs the forward again.  Reads every parameter once: ~0.3 GB per step at
// config 2, ~0.2 % of the step.
//   table[t] = {pointer, 32-bit words}; grid = (tensors, kChecksumSlices); sums[t] zeroed by the caller.
struct ChecksumEntry {
  const unsigned *ptr;
  long words;
};
constexpr int kChecksumSlices = 32;
__global__ __launch_bounds__(256) void checksum_tensors_kernel(const ChecksumEntry *__restrict__ table,
                                                               unsigned long long *__restrict__ sums) {
  const ChecksumEntry e = table[blockIdx.x];
  unsigned long long acc = 0ull;
  const long n4 = e.words / 4;
  const u32x4_t *p4 = reinterpret_cast<const u32x4_t *>(e.ptr);
  for (long i = (long)blockIdx.y * 256 + threadIdx.x; i < n4; i += (long)kChecksumSlices * 256) {
    const u32x4_t v = p4[i];
    const unsigned long long salt = (unsigned long long)i * 0x9E3779B97F4A7C15ull;
    acc += ((unsigned long long)v.x ^ salt) * 0x85EBCA77C2B2AE63ull + ((unsigned long long)v.y ^ (salt >> 7)) * 0xC2B2AE3D27D4EB4Full;
    acc += ((unsigned long long)v.z ^ (salt >> 13)) * 0x165667B19E3779F9ull + ((unsigned long long)v.w ^ (salt >> 29)) * 0x27D4EB2F165667C5ull;
  }
  if (blockIdx.y == 0) {   // the tail (words % 4) and nothing else
    for (long i = 4 * n4 + threadIdx.x; i < e.words; i += 256)
      acc += ((unsigned long long)e.ptr[i] ^ ((unsigned long long)i * 0x9E3779B97F4A7C15ull)) * 0xFF51AFD7ED558CCDull;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if ((threadIdx.x & 63) == 0 && acc != 0ull) atomicAdd(&sums[blockIdx.x], acc);
}

}  // namespace gqhip
