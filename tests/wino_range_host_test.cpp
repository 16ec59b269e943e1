// Host-side check of csrc/gq_wino_range.h (CPU suite, no GPU): wino_offsets_fit_u32 -- the predicate by which the conv stack's
// entry points choose the Winograd transform kernels with 32-bit byte offsets or their wide twins -- at its boundaries, against
// a 128-bit evaluation of the same sizes: the largest shapes it accepts, one step past them, the three operand widths (4 bytes
// per channel for fp32 V and M, 4 for [h | l], 6 for [h | h | l]), both tile sizes, and arguments whose products overflow 64 bits.
// Built and run by tests/test_wino_range_host.py.
#include <cstdint>
#include <cstdio>

#include "gq_wino_range.h"

using gqhip::wino_offsets_fit_u32;

static bool reference(int64_t B, int64_t H, int64_t W, int64_t C, int64_t tile, int64_t pb) {
  const unsigned __int128 limit = (unsigned __int128)1 << 32;
  const unsigned __int128 tensor = (unsigned __int128)B * H * W * C * 4;
  const unsigned __int128 plane = (unsigned __int128)B * (H / tile) * (W / tile) * C * pb;
  return tensor <= limit && plane <= limit;
}

static int failures = 0;
static void expect(bool got, bool want, const char *what) {
  if (got != want) {
    std::printf("FAIL: %s: got %d, want %d\n", what, (int)got, (int)want);
    ++failures;
  }
}

int main() {
  const int64_t widths[] = {4, 4, 6};   // fp32 V / M, [h | l], [h | h | l]
  for (int64_t pb : widths)
    for (int64_t tile : {2, 4}) {
      // the tensor's size at exactly 2^32 bytes: the largest accepted shape; one more tile row, column, image or channel quad: wide
      expect(wino_offsets_fit_u32(16, 256, 256, 1024, tile, pb), true, "16 x 256 x 256 x 1024 = 2^32 bytes");
      expect(wino_offsets_fit_u32(16, 256 + tile, 256, 1024, tile, pb), false, "one tile row past 2^32 bytes");
      expect(wino_offsets_fit_u32(16, 256, 256 + tile, 1024, tile, pb), false, "one tile column past 2^32 bytes");
      expect(wino_offsets_fit_u32(17, 256, 256, 1024, tile, pb), false, "one image past 2^32 bytes");
      expect(wino_offsets_fit_u32(16, 256, 256, 1028, tile, pb), false, "one channel quad past 2^32 bytes");
      expect(wino_offsets_fit_u32(1, 32768, 32768, 4, tile, pb), false, "one image of 2^34 bytes");
      expect(wino_offsets_fit_u32(1, 16384, 16384, 4, tile, pb), true, "one image of 2^32 bytes");
      // the flagship step and an empty batch
      expect(wino_offsets_fit_u32(16, 256, 256, 128, tile, pb), true, "16 x 256 x 256 x 128");
      expect(wino_offsets_fit_u32(0, 256, 256, 128, tile, pb), true, "B = 0");
      // products beyond 64 bits must not wrap into range
      expect(wino_offsets_fit_u32(INT64_MAX / 2, 4, 4, 4, tile, pb), false, "B near 2^62");
      expect(wino_offsets_fit_u32((int64_t)1 << 32, (int64_t)1 << 32, 4, 4, tile, pb), false, "B * H = 2^64");
      expect(wino_offsets_fit_u32(4, (int64_t)1 << 31, (int64_t)1 << 31, (int64_t)1 << 2, tile, pb), false, "2^68 bytes");
      // a sweep across the boundary, against the 128-bit evaluation
      for (int64_t B = 1; B <= 33; B += 4)
        for (int64_t H = tile; H <= 4096; H *= 2)
          for (int64_t dW = -tile; dW <= tile; dW += tile)
            for (int64_t C : {4, 128, 1024, 4096}) {
              const int64_t W = (((int64_t)1 << 32) / (4 * B * H * C) / tile) * tile + dW;   // around tensor = 2^32
              if (W < tile) continue;
              if (wino_offsets_fit_u32(B, H, W, C, tile, pb) != reference(B, H, W, C, tile, pb)) {
                std::printf("FAIL: B %lld H %lld W %lld C %lld tile %lld width %lld\n", (long long)B, (long long)H, (long long)W,
                            (long long)C, (long long)tile, (long long)pb);
                ++failures;
              }
            }
    }
  // the plane of V / M alone: a width so large that the plane passes 2^32 bytes while the tensor does not (no operand of the
  // library has it -- 4 t^2 bytes of x stand behind every channel of a tile -- but the predicate checks the plane on its own)
  expect(wino_offsets_fit_u32(16, 256, 256, 512, 2, 64), false, "plane of 2^33 bytes under a tensor of 2^31");
  expect(wino_offsets_fit_u32(16, 256, 256, 512, 2, 32), true, "plane of 2^32 bytes under a tensor of 2^31");
  if (failures) return 1;
  std::printf("ok: wino_offsets_fit_u32 agrees with the 128-bit sizes at its boundaries\n");
  return 0;
}
