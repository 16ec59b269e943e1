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

// The four slices of a wave to y: row (lane >> 4) + 4 i of slice rr, columns 4 (lane & 15) .. + 3 go to
// y[o + rr * slice + i * step .. + 3] (element offsets; o holds the lane's first row and its column quad), as
//   MODE 1: acc * mscale + bias                  (upconv)
//   MODE 2: acc * mscale + bias + 0              (the direct convolutions without a residual: their "+ 0" kept, it turns -0 into +0)
//   MODE 3: acc * mscale + bias + res            (the direct convolutions with one, read at the same offsets as y)
// -- per element the fp32 operations of the accumulator-order epilogues, in their order.  STATS: every stored value is
// also added to st.
template <int MODE, bool STATS>
__device__ __forceinline__ void epi_store(const f32x16 (&acc)[4][2], float *stage, int lane, float *y, const float *res,
                                          long o, long slice, long step, float mscale, f32x4 bias, StatPartial &st) {
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
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

}  // namespace gqhip
