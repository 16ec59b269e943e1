// gq_epilogue.h -- the store phase of the direct v_mfma_f32_32x32x16_f16 convolutions (gq_conv3.h: conv3x3_gn, conv1x1,
// conv3x3s2, upconv2x), staged through LDS.
//
// A wave of those kernels ends with four 32-row x 64-column fp32 slices in accumulator order: register r of lane (c, h)
// (c = lane & 31, h = lane >> 5) of acc[rr][j] = row (r & 3) + 8 (r >> 2) + 4 h of slice rr, column 32 j + c.  Stored as
// they stand, every value is one global dword access (128 stores and, with a residual, 128 loads per lane, each with an
// address of its own): the r03 ablation put that epilogue at 15 % of conv3x3_gn's time.  Here each slice goes through
// the wave's own 8 KiB of LDS: 32 ds_write_b32 into a row-major [32][64] image, then lane l reads columns 4 (l & 15) .. + 3
// of rows (l >> 4) + 4 i (i < 8) with 8 ds_read_b128 and the global traffic is 8 dwordx4 accesses per slice; the 16
// lanes of one row cover its 256 bytes.  Conflict-free without padding: the ds_write_b32 of a half-wave (one bank group
// of 32) is 32 consecutive dwords, and each 16-lane group of ds_read_b128 ({0-3, 12-15, 20-27}, ...) reads 16 distinct
// 16-byte slots of the 256-byte bank row.  Only the wave itself touches its image, and a wave's LDS operations execute
// in order, so a wave-level fence (no block barrier, no wait) orders the slices.  The lane's column quad is fixed, so
// with GroupNorm groups of a multiple of 4 channels all its values fall into one group.
// Not used by the Winograd GEMMs (gq_wino_gemm.h): their M store has no residual and no statistics, and the 8-wave GEMM
// (one block per CU, every CU storing at once) measured no faster through LDS (profiles/r09).
#pragma once
#include "gq_common.h"
#include "gq_stats.h"

namespace gqhip {

constexpr int kEpiWaveBytes = 32 * 64 * 4;   // LDS image of one wave

__device__ __forceinline__ void epi_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One slice (a = acc[rr]) through the wave's image `stage`: out[i] = columns 4 (lane & 15) .. + 3 of row (lane >> 4) + 4 i.
__device__ __forceinline__ void epi_transpose(const f32x16 (&a)[2], float *stage, int lane, f32x4 (&out)[8]) {
  const int c = lane & 31, h = lane >> 5;
  epi_wave_sync();   // the reads of the previous slice come first
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) stage[((r & 3) + 8 * (r >> 2) + 4 * h) * 64 + 32 * j + c] = a[j][r];
  epi_wave_sync();
  const f32x4 *s = reinterpret_cast<const f32x4 *>(stage) + (lane >> 4) * 16 + (lane & 15);
#pragma unroll
  for (int i = 0; i < 8; ++i) out[i] = s[64 * i];
}

// The RR (four; two in the 128-pixel tiling of the 1x1 kernel) slices of a wave to y: row (lane >> 4) + 4 i of slice rr, columns 4 (lane & 15) .. + 3 go to
// y[o + rr * slice + i * step .. + 3] (element offsets; o holds the lane's first row and its column quad), as
//   MODE 1: acc * mscale + bias                  (upconv)
//   MODE 2: acc * mscale + bias + 0              (the direct convolutions without a residual: their "+ 0" kept, it turns -0 into +0)
//   MODE 3: acc * mscale + bias + res            (the direct convolutions with one, read at the same offsets as y)
// -- per element the fp32 operations of the accumulator-order epilogues, in their order.  STATS: every stored value is
// also added to st.
template <int MODE, bool STATS, int RR>
__device__ __forceinline__ void epi_store(const f32x16 (&acc)[RR][2], float *stage, int lane, float *y, const float *res,
                                          long o, long slice, long step, float mscale, f32x4 bias, StatPartial &st) {
#pragma unroll
  for (int rr = 0; rr < RR; ++rr) {
    __builtin_amdgcn_sched_barrier(0);   // one slice at a time: hoisting the residual loads of later slices spills
    const long orr = o + rr * slice;
    f32x4 rv[8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
      rv[i] = MODE == 3 ? *reinterpret_cast<const f32x4 *>(res + orr + i * step) : f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 v[8];
    epi_transpose(acc[rr], stage, lane, v);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      f32x4 w = v[i];
      w = w * mscale + bias;
      if (MODE >= 2) w = w + rv[i];
      *reinterpret_cast<f32x4 *>(y + orr + i * step) = w;
      if (STATS) stat_partial_add_vec(st, w);
    }
  }
}

// The slices of a wave of the attention block's q | k | v projection, written as the operands of the two attention GEMMs
// (what attn_split_qkv_kernel makes of the fp32 projection, which is then never stored): the fp32 value of MODE 2 above,
// times the power of two `s`, as a two-term fp16 split h + l.  h goes to dst[o ..], the second and third copies one and
// two `plane` elements further: (h, h, l) for q (`second_h`), (h, l, h) for k and v.  A lane's four values are 8 bytes
// and the 16 lanes of a row cover one 128-byte run of each copy.  h is the conversion of the fp32 product as it stands
// (kept opaque: see attn_softmax_split_kernel), so h + l is the split the separate pass computes, bit for bit.
template <int RR>
__device__ __forceinline__ void epi_store_split(const f32x16 (&acc)[RR][2], float *stage, int lane, _Float16 *dst, long o,
                                                long slice, long step, long plane, bool second_h, float mscale,
                                                f32x4 bias, float s) {
  typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
#pragma unroll
  for (int rr = 0; rr < RR; ++rr) {
    __builtin_amdgcn_sched_barrier(0);
    const long orr = o + rr * slice;
    f32x4 v[8];
    epi_transpose(acc[rr], stage, lane, v);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      f32x4 w = v[i];
      w = w * mscale + bias;
      w = w + f32x4{0.f, 0.f, 0.f, 0.f};
      f16x4 h, l;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float x = w[e] * s;
        asm volatile("" : "+v"(x));
        h[e] = (_Float16)x;
        l[e] = (_Float16)(x - (float)h[e]);
      }
      _Float16 *d = dst + orr + i * step;
      *reinterpret_cast<f16x4 *>(d) = h;
      *reinterpret_cast<f16x4 *>(d + plane) = second_h ? h : l;
      *reinterpret_cast<f16x4 *>(d + 2 * plane) = second_h ? l : h;
    }
  }
}

}  // namespace gqhip
