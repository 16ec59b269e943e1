// gq_wino_range.h -- host side: which calls of the Winograd transforms fit the kernels' 32-bit byte offsets (gq_unet_aux.h:
// "Addressing of the transform kernels").  Plain C++, no HIP: tests/wino_range_host_test.cpp compiles it on its own.
#pragma once
#include <stdint.h>

#include <initializer_list>

namespace gqhip {

// a * b <= limit for non-negative factors, without overflow
inline bool wino_product_le(uint64_t a, uint64_t b, uint64_t limit) { return a == 0 || b <= limit / a; }

// The kernels with OFF = uint32_t form, per access, base + a byte offset computed in 32 bits.  Derived from their expressions:
//   x / y / res [B][H][W][C] fp32   offset = b * (H * W * C * 4) + row * (W * C * 4) + column * (C * 4) + channel bytes, all terms and
//                                   every partial sum below the tensor's size B * H * W * C * 4;
//   V / M [planes][tiles][row]      offset in a plane = tile * row bytes + channel bytes (+ 1 or 2 parts of an fp16 row), below the
//                                   plane's size tiles * C * plane_bytes_per_channel: 4 for fp32 V and for M, 2 * 2 for the [h | l]
//                                   operand, 3 * 2 for [h | h | l]; tiles = B * (H / tile) * (W / tile);
//   the item counter                below tiles * C / 2 + 2^23 (a grid stride), itself below the plane's size.
// An access ends at most at the size, so sizes up to 2^32 fit.  Every other shape runs the *_wide_kernel twins (64-bit offsets).
inline bool wino_offsets_fit_u32(int64_t B, int64_t H, int64_t W, int64_t C, int64_t tile, int64_t plane_bytes_per_channel) {
  if (B < 0 || H < 1 || W < 1 || C < 1 || tile < 1 || plane_bytes_per_channel < 1) return false;
  const uint64_t limit = 1ull << 32;
  uint64_t tensor = 4, plane = (uint64_t)plane_bytes_per_channel;
  for (uint64_t f : {(uint64_t)B, (uint64_t)H, (uint64_t)W, (uint64_t)C}) {
    if (!wino_product_le(tensor, f, limit)) return false;
    tensor *= f;
  }
  for (uint64_t f : {(uint64_t)B, (uint64_t)(H / tile), (uint64_t)(W / tile), (uint64_t)C}) {
    if (!wino_product_le(plane, f, limit)) return false;
    plane *= f;
  }
  return true;
}

}  // namespace gqhip
