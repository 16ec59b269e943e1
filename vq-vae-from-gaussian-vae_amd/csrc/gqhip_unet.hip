// gqhip_unet.hip -- C-ABI entry points of libgqhip.so for the conv stack (include/gqhip.h): fused GroupNorm, residual adds,
// Winograd transforms and GEMMs, the direct fp16 x 3 convolutions, attention operand splits.
// gfx950 only; built by `make -C vq-vae-from-gaussian-vae_amd/csrc` (its own translation unit: the two halves compile in parallel).
#include "gqhip.h"

#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <initializer_list>
#include <cstring>

#include "gqhip_internal.h"
#include "gq_unet_aux.h"
#include "gq_wino_range.h"
#include "gq_wino_gemm.h"
#include "gq_conv3.h"
#include "gq_conv_f32.h"
#include "gq_attn.h"
#include "gq_attn_bwd.h"

using namespace gqhip;

namespace {
// Statistics records are zeroed by the entry point that fills them -- unless the caller has said that they already are
// (gqhip_stats_prezeroed: the conv stack's modules carve all records of a forward out of one arena zeroed by ONE fill, instead of
// ~60 separate 32-KB memset launches per step).  Thread-local: the flag belongs to the calling thread's sequence of calls.
thread_local int g_stats_prezeroed = 0;
inline hipError_t stats_zero(void *p, size_t bytes, hipStream_t st) {
  return g_stats_prezeroed ? hipSuccess : hipMemsetAsync(p, 0, bytes, st);
}

// What a check helper returns when the arguments are fine and there is something to do; any other value is the entry point's status.
constexpr int kGo = -1;

// 256-thread blocks over `total` items, `cap` at the most (the kernels stride over the rest)
dim3 grid1d(long total, long cap) {
  const long blocks = (total + 255) / 256;
  return dim3((unsigned)(blocks > cap ? cap : blocks));
}

// slabs of ~16 pixels per thread for the NHWC GroupNorm kernels (256 / (C / 4) pixel lanes per block)
int nhwc_slabs(int64_t C, int64_t HW) {
  const int lanes = (int)(256 / (C / 4));
  int slabs = (int)((HW + (int64_t)lanes * 16 - 1) / ((int64_t)lanes * 16));
  if (slabs > 1024) slabs = 1024;
  return slabs < 1 ? 1 : slabs;
}

// The checks of the GroupNorm entry points, in this order: sizes, nothing to do, pointers, and for NHWC the kernels' thread <->
// channel-quad mapping: cpg % 4 == 0, (C/4) | 256, <= 64 groups.
int gn_check(int64_t B, int64_t C, int64_t HW, int64_t groups, bool ptrs_ok, bool nhwc) {
  if (B < 0 || C < 1 || HW < 1 || groups < 1 || C % groups != 0) return GQHIP_ERR_INVALID_ARG;
  if (B == 0) return GQHIP_OK;
  if (!ptrs_ok) return GQHIP_ERR_INVALID_ARG;
  if (nhwc && ((C / groups) % 4 != 0 || 256 % (C / 4) != 0 || groups > 64)) return GQHIP_ERR_INVALID_ARG;
  return kGo;
}

// Winograd F(tile x tile, 3x3) on NHWC: whole tiles, channel quads
bool wino_shape_ok(int64_t B, int64_t H, int64_t W, int64_t C, int64_t tile) {
  return (tile == 2 || tile == 4) && B >= 0 && H >= tile && W >= tile && H % tile == 0 && W % tile == 0 && C >= 4 && C % 4 == 0;
}
// Beside it: wino_offsets_fit_u32 (gq_wino_range.h) -- a shape it accepts runs the transform kernels with 32-bit offsets, any other
// their *_wide_kernel twins; no accepted shape is refused for its size.  GQHIP_WINO_WIDE=1 forces the wide twins at every shape
// (tests: no test tensor passes 4 GiB); read per call, so one process can run both.
bool wino_u32(int64_t B, int64_t H, int64_t W, int64_t C, int64_t tile, int64_t plane_bytes_per_channel) {
  const char *knob = getenv("GQHIP_WINO_WIDE");
  return !(knob && !strcmp(knob, "1")) && wino_offsets_fit_u32(B, H, W, C, tile, plane_bytes_per_channel);
}

bool one_of(int64_t v, std::initializer_list<int64_t> values) {
  for (int64_t w : values)
    if (v == w) return true;
  return false;
}
}  // namespace

extern "C" {

int gqhip_stats_prezeroed(int on) {
  g_stats_prezeroed = on != 0;
  return GQHIP_OK;
}

int gn_silu_f32(const float *x, const float *gamma, const float *beta, const float *pre_bias_or_null, float *y,
                int64_t B, int64_t C, int64_t HW, int64_t groups, double eps, int apply_silu, int layout,
                int64_t *stats_ws, void *stream) {
  const bool nhwc = layout == GQHIP_LAYOUT_NHWC;
  if (int rc = gn_check(B, C, HW, groups, x && gamma && beta && y && stats_ws, nhwc); rc != kGo) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t bg = B * groups, cpg = C / groups, chunk = cpg * HW;
  if (nhwc) {
    if (stats_zero(stats_ws, sizeof(int64_t) * kStatWords * bg, st) != hipSuccess) return check_launch();
    const int slabs = nhwc_slabs(C, HW);
    hipLaunchKernelGGL(gn_stats_nhwc_kernel, dim3((unsigned)(B * slabs)), dim3(256), 0, st, x, pre_bias_or_null,
                       stats_ws, (int)C, (long)HW, (int)cpg, slabs);
    int rc = check_launch();
    if (rc != GQHIP_OK) return rc;
    return launch(apply_silu ? gn_apply_nhwc_kernel<1> : gn_apply_nhwc_kernel<0>, dim3((unsigned)(B * slabs)), dim3(256), 0, st, x,
                  gamma, beta, y, stats_ws, pre_bias_or_null, (int)C, (long)HW, (int)cpg, eps, slabs);
  }
  if (layout != GQHIP_LAYOUT_NCHW || HW % 4 != 0) return GQHIP_ERR_INVALID_ARG;   // callers fall back to torch
  if (stats_zero(stats_ws, sizeof(int64_t) * kStatWords * bg, st) != hipSuccess) return check_launch();
  // ~16 KiB of input per block keeps >= 2k blocks in flight at the big resolutions
  int slices = (int)((chunk + 4095) / 4096);
  if (slices > 256) slices = 256;
  if (slices < 1) slices = 1;
  hipLaunchKernelGGL(gn_stats_kernel, dim3((unsigned)(bg * slices)), dim3(256), 0, st, x, pre_bias_or_null, stats_ws,
                     (long)chunk, slices, (long)HW, (int)cpg, (int)groups);
  int rc = check_launch();
  if (rc != GQHIP_OK) return rc;
  int segs = (int)((HW + 8191) / 8192);
  if (segs < 1) segs = 1;
  const dim3 grid((unsigned)(B * C * segs));
  return launch(apply_silu ? gn_apply_kernel<1> : gn_apply_kernel<0>, grid, dim3(256), 0, st, x, gamma, beta, y, stats_ws,
                pre_bias_or_null, (int)C, (long)HW, (int)cpg, eps, segs);
}

int add_bias_f32(const float *a, const float *b, const float *bias_or_null, float *y, int64_t B, int64_t C,
                 int64_t HW, int layout, void *stream) {
  if (B < 0 || C < 1 || HW < 1) return GQHIP_ERR_INVALID_ARG;
  if (B == 0) return GQHIP_OK;
  if (!a || !b || !y) return GQHIP_ERR_INVALID_ARG;
  const long total4 = (long)(B * C * HW / 4);
  const dim3 grid = grid1d(total4, 8192);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (layout == GQHIP_LAYOUT_NHWC) {
    if (C % 4 != 0) return GQHIP_ERR_INVALID_ARG;
    hipLaunchKernelGGL(add_bias_nhwc_kernel, grid, dim3(256), 0, st, a, b, bias_or_null, y, (int)C,
                       total4);
  } else {
    if (layout != GQHIP_LAYOUT_NCHW || HW % 4 != 0) return GQHIP_ERR_INVALID_ARG;
    hipLaunchKernelGGL(add_bias_kernel, grid, dim3(256), 0, st, a, b, bias_or_null, y, (int)C,
                       (long)HW, total4);
  }
  return check_launch();
}

int add_bias_stats_f32(const float *a, const float *b, const float *bias_or_null, float *y, int64_t B, int64_t C,
                       int64_t HW, int64_t groups, int64_t *stats_out, void *stream) {
  if (int rc = gn_check(B, C, HW, groups, a && b && y && stats_out, true); rc != kGo) return rc;
  const int64_t cpg = C / groups;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (stats_zero(stats_out, sizeof(int64_t) * kStatWords * B * groups, st) != hipSuccess) return check_launch();
  const int slabs = nhwc_slabs(C, HW);
  return launch(add_bias_stats_nhwc_kernel, dim3((unsigned)(B * slabs)), dim3(256), 0, st, a, b, bias_or_null, y,
                stats_out, (int)C, (long)HW, (int)cpg, slabs);
}

int gn_apply_f32(const float *x, const float *gamma, const float *beta, float *y, int64_t B, int64_t C, int64_t HW,
                 int64_t groups, double eps, int apply_silu, const int64_t *stats, void *stream) {
  if (int rc = gn_check(B, C, HW, groups, x && gamma && beta && y && stats, true); rc != kGo) return rc;
  const int64_t cpg = C / groups;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int slabs = nhwc_slabs(C, HW);
  return launch(apply_silu ? gn_apply_nhwc_kernel<1> : gn_apply_nhwc_kernel<0>, dim3((unsigned)(B * slabs)), dim3(256), 0, st, x,
                gamma, beta, y, stats, nullptr, (int)C, (long)HW, (int)cpg, eps, slabs);
}

// The plain input transforms: vm = 0 fp32 V, 1 the three-plane fp16 operand, 2 the [h | l] operand (gq_unet_aux.h)
static int wino_in_impl(int vm, const float *x, void *V, int64_t B, int64_t H, int64_t W, int64_t C, int tile, float scale,
                        void *stream) {
  if (!wino_shape_ok(B, H, W, C, tile) || !(scale > 0.f)) return GQHIP_ERR_INVALID_ARG;
  if (B == 0) return GQHIP_OK;
  if (!x || !V) return GQHIP_ERR_INVALID_ARG;
  const long tiles = (long)(B * (H / tile) * (W / tile)), total = tiles * (C / 4);
  const bool u32 = wino_u32(B, H, W, C, tile, vm == 1 ? 6 : 4);
  const auto kernel =
      u32 ? (tile == 4 ? (vm == 2 ? wino4_in_nhwc_kernel<2> : vm == 1 ? wino4_in_nhwc_kernel<1> : wino4_in_nhwc_kernel<0>)
                       : (vm == 2 ? wino_in_nhwc_kernel<2> : vm == 1 ? wino_in_nhwc_kernel<1> : wino_in_nhwc_kernel<0>))
          : (tile == 4 ? (vm == 2 ? wino4_in_nhwc_wide_kernel<2> : vm == 1 ? wino4_in_nhwc_wide_kernel<1> : wino4_in_nhwc_wide_kernel<0>)
                       : (vm == 2 ? wino_in_nhwc_wide_kernel<2> : vm == 1 ? wino_in_nhwc_wide_kernel<1> : wino_in_nhwc_wide_kernel<0>));
  return launch(kernel, grid1d(total, 16384), dim3(256), 0, static_cast<hipStream_t>(stream), x, V, (int)H, (int)W, (int)(C / 4),
                tiles, total, scale);
}

int wino_in_nhwc_f32(const float *x, float *V, int64_t B, int64_t H, int64_t W, int64_t C, void *stream) {
  return wino_in_impl(0, x, V, B, H, W, C, 2, 1.0f, stream);
}

int wino4_in_nhwc_f32(const float *x, float *V, int64_t B, int64_t H, int64_t W, int64_t C, void *stream) {
  return wino_in_impl(0, x, V, B, H, W, C, 4, 1.0f, stream);
}

int wino_in_nhwc_f16x3(const float *x, void *V3, int64_t B, int64_t H, int64_t W, int64_t C, int tile, float scale,
                       void *stream) {
  return wino_in_impl(1, x, V3, B, H, W, C, tile, scale, stream);
}

int wino_in_nhwc_f16x2(const float *x, void *V2, int64_t B, int64_t H, int64_t W, int64_t C, int tile, float scale,
                       void *stream) {
  return wino_in_impl(2, x, V2, B, H, W, C, tile, scale, stream);
}

// The tiling of wino_gemm_f16x2 (gq_wino_gemm.h).  The 256-column tilings need Cin % 64 == 0 and Cout % 256 == 0; every other
// shape runs 256 x 128.  Among the two, 128 x 256 (two 4-wave blocks per CU) everywhere: alternating with 256 x 256 (one 8-wave
// block per CU) in one process on MI355X it was the faster of each adjacent pair of windows at all six shapes of the step, by
// 4-16 % in the median, at Cin = 256 as much as at Cin = 512 (profiles/r12/gemm_ab.txt -- one session with short windows; its
// caveats are stated there).
// GQHIP_WGEMM forces one (A/B, tests): 128 = 256 x 128, w8 = 256 x 256, anything else (w4) = 128 x 256; read per call, so one process can
// compare them.  A forced 256-column tiling still yields to 256 x 128 where the shape does not allow it.
enum class WinoGemmTiling { k256x128, k256x256, k128x256 };
static WinoGemmTiling wino_gemm_tiling(int64_t Cin, int64_t Cout) {
  const char *knob = getenv("GQHIP_WGEMM");
  if (Cin % 64 != 0 || Cout % 256 != 0 || (knob && !strcmp(knob, "128"))) return WinoGemmTiling::k256x128;
  if (knob && !strcmp(knob, "w8")) return WinoGemmTiling::k256x256;
  return WinoGemmTiling::k128x256;
}

int wino_gemm_f16x2(const void *V2, const void *Wf, float *M, int64_t P, int64_t tiles, int64_t Cin, int64_t Cout,
                    void *stream) {
  if (P < 1 || tiles < 0 || tiles > 0x3fffffff || tiles % 256 != 0 || Cin < 32 || Cin % 32 != 0 || Cin > 4096 || Cout < 128 ||
      Cout % 128 != 0 || Cout > 4096)
    return GQHIP_ERR_INVALID_ARG;
  if (tiles == 0) return GQHIP_OK;
  if (!V2 || !Wf || !M) return GQHIP_ERR_INVALID_ARG;
  WinoGemm2Params wp{};
  wp.V2 = static_cast<const _Float16 *>(V2); wp.Wf = static_cast<const _Float16 *>(Wf); wp.M = M; wp.tiles = tiles;
  wp.cin = (int)Cin; wp.cout = (int)Cout;
  const WinoGemmTiling tiling = wino_gemm_tiling(Cin, Cout);
  const long rows = tiling == WinoGemmTiling::k128x256 ? 128 : 256, cols = tiling == WinoGemmTiling::k256x128 ? 128 : 256;
  wp.nnb = (int)(Cout / cols);
  wp.mtiles = tiles / rows; wp.ntile_total = P * wp.mtiles; wp.tiles_per_xcd = (wp.ntile_total + 7) / 8;
  const long blocks = 8 * wp.tiles_per_xcd * wp.nnb;
  if (blocks > 0x7fffffffL) return GQHIP_ERR_INVALID_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (tiling) {
    case WinoGemmTiling::k128x256: hipLaunchKernelGGL(wino_gemm_f16x2_k64_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, st, wp); break;
    case WinoGemmTiling::k256x256: hipLaunchKernelGGL(wino_gemm_f16x2_k64_kernel<2>, dim3((unsigned)blocks), dim3(512), 0, st, wp); break;
    case WinoGemmTiling::k256x128: hipLaunchKernelGGL(wino_gemm_f16x2_kernel, dim3((unsigned)blocks), dim3(256), 0, st, wp); break;
  }
  return check_launch();
}

int gn_stats_f32(const float *x, const float *pre_bias_or_null, int64_t B, int64_t C, int64_t HW, int64_t groups,
                 int64_t *stats_out, void *stream) {
  if (int rc = gn_check(B, C, HW, groups, x && stats_out, true); rc != kGo) return rc;
  const int64_t cpg = C / groups;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (stats_zero(stats_out, sizeof(int64_t) * kStatWords * B * groups, st) != hipSuccess) return check_launch();
  const int slabs = nhwc_slabs(C, HW);
  return launch(gn_stats_nhwc_kernel, dim3((unsigned)(B * slabs)), dim3(256), 0, st, x, pre_bias_or_null, stats_out,
                (int)C, (long)HW, (int)cpg, slabs);
}

static int wino_in_gn_impl(int tile, int f16, const float *x, const float *gamma, const float *beta,
                           const float *pre_bias_or_null, const int64_t *stats, void *V, int64_t B, int64_t H, int64_t W,
                           int64_t C, int64_t groups, double eps, int apply_silu, float scale, void *stream) {
  if (!wino_shape_ok(B, H, W, C, tile) || groups < 1 || C % groups != 0 || (C / groups) % 4 != 0 || !(scale > 0.f))
    return GQHIP_ERR_INVALID_ARG;
  if (B == 0) return GQHIP_OK;
  if (!x || !gamma || !beta || !stats || !V) return GQHIP_ERR_INVALID_ARG;
  // F(4x4,3x3) on an fp16 operand: two channels per thread (register pressure: see the kernel); 4 otherwise
  const int vw = (tile == 4 && f16 != 0) ? 2 : 4;
  const long tiles = (long)(B * (H / tile) * (W / tile)), total = tiles * (C / vw);
  const dim3 grid = grid1d(total, 32768);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool u32 = wino_u32(B, H, W, C, tile, f16 == 1 ? 6 : 4);
#define GQ_WGN(K, ...)                                                                                                       \
  hipLaunchKernelGGL((u32 ? K##_kernel<__VA_ARGS__> : K##_wide_kernel<__VA_ARGS__>), grid, dim3(256), 0, st, x, gamma, beta, \
                     pre_bias_or_null, stats, V, (int)H, (int)W, (int)(C / vw), (int)(C / groups), eps, tiles, total, scale)
  if (tile == 4) {
    if (apply_silu) {
      if (f16 == 2) GQ_WGN(wino4_in_gn_nhwc, 1, 2, 2); else if (f16 == 1) GQ_WGN(wino4_in_gn_nhwc, 1, 1, 2);
      else GQ_WGN(wino4_in_gn_nhwc, 1, 0, 4);
    } else {
      if (f16 == 2) GQ_WGN(wino4_in_gn_nhwc, 0, 2, 2); else if (f16 == 1) GQ_WGN(wino4_in_gn_nhwc, 0, 1, 2);
      else GQ_WGN(wino4_in_gn_nhwc, 0, 0, 4);
    }
  } else {
    if (apply_silu) {
      if (f16 == 2) GQ_WGN(wino_in_gn_nhwc, 1, 2); else if (f16 == 1) GQ_WGN(wino_in_gn_nhwc, 1, 1);
      else GQ_WGN(wino_in_gn_nhwc, 1, 0);
    } else {
      if (f16 == 2) GQ_WGN(wino_in_gn_nhwc, 0, 2); else if (f16 == 1) GQ_WGN(wino_in_gn_nhwc, 0, 1);
      else GQ_WGN(wino_in_gn_nhwc, 0, 0);
    }
  }
#undef GQ_WGN
  return check_launch();
}

int wino_in_gn_nhwc_f32(const float *x, const float *gamma, const float *beta, const float *pre_bias_or_null,
                        const int64_t *stats, float *V, int64_t B, int64_t H, int64_t W, int64_t C, int64_t groups,
                        double eps, int apply_silu, void *stream) {
  return wino_in_gn_impl(2, 0, x, gamma, beta, pre_bias_or_null, stats, V, B, H, W, C, groups, eps, apply_silu, 1.0f, stream);
}

int wino4_in_gn_nhwc_f32(const float *x, const float *gamma, const float *beta, const float *pre_bias_or_null,
                         const int64_t *stats, float *V, int64_t B, int64_t H, int64_t W, int64_t C, int64_t groups,
                         double eps, int apply_silu, void *stream) {
  return wino_in_gn_impl(4, 0, x, gamma, beta, pre_bias_or_null, stats, V, B, H, W, C, groups, eps, apply_silu, 1.0f, stream);
}

int wino_in_gn_nhwc_f16x3(const float *x, const float *gamma, const float *beta, const float *pre_bias_or_null,
                          const int64_t *stats, void *V3, int64_t B, int64_t H, int64_t W, int64_t C, int64_t groups,
                          double eps, int apply_silu, int tile, float scale, void *stream) {
  return wino_in_gn_impl(tile, 1, x, gamma, beta, pre_bias_or_null, stats, V3, B, H, W, C, groups, eps, apply_silu, scale,
                         stream);
}

int wino_in_gn_nhwc_f16x2(const float *x, const float *gamma, const float *beta, const float *pre_bias_or_null,
                          const int64_t *stats, void *V2, int64_t B, int64_t H, int64_t W, int64_t C, int64_t groups,
                          double eps, int apply_silu, int tile, float scale, void *stream) {
  return wino_in_gn_impl(tile, 2, x, gamma, beta, pre_bias_or_null, stats, V2, B, H, W, C, groups, eps, apply_silu, scale,
                         stream);
}

static bool conv3_groups_ok(int64_t Cout, int64_t groups_out) {
  if (groups_out < 1 || Cout % groups_out != 0) return false;
  const int64_t cpg = Cout / groups_out;
  return cpg % 4 == 0 && 128 % cpg == 0;
}

// an operand scale from the host, or the device's (scales_dev: f16_scales_from_gn_stats)
static bool scale_ok(const float *scales_dev_or_null, float scale) { return scales_dev_or_null || scale > 0.f; }

// What every direct convolution does between its shape checks and its launch, in this order: the groups of the statistics it
// is to leave (groups_ok only counts when there are statistics; the caller evaluates it either way, so it must be safe for any
// groups_out: conv3_groups_ok refuses groups_out < 1 before it divides), nothing to do, pointers -- conv_checks -- and then
// the records are zeroed.  conv1_launch settles its tiling between the two.
static int conv_checks(int64_t B, bool ptrs_ok, const int64_t *stats_out, bool groups_ok) {
  if (stats_out && !groups_ok) return GQHIP_ERR_INVALID_ARG;
  if (B == 0) return GQHIP_OK;
  return ptrs_ok ? kGo : GQHIP_ERR_INVALID_ARG;
}

static int conv_stats_zero(int64_t *stats_out, int64_t records, hipStream_t st) {
  if (stats_out && stats_zero(stats_out, sizeof(int64_t) * kStatWords * records, st) != hipSuccess) return check_launch();
  return kGo;
}

static int conv_prologue(int64_t B, bool ptrs_ok, int64_t *stats_out, bool groups_ok, int64_t groups_out, hipStream_t st) {
  const int rc = conv_checks(B, ptrs_ok, stats_out, groups_ok);
  return rc != kGo ? rc : conv_stats_zero(stats_out, B * groups_out, st);
}

// Fills cp for output tiles of tile_h x kC3TW pixels and returns the grid: every XCD walks its share of the tiles per column block.
static dim3 conv3_fill(Conv3Params &cp, const void *Wf, const float *bias, const float *res, float *y, int64_t *stats, int64_t B,
                       int64_t H, int64_t W, int64_t Cin, int64_t Cout, int64_t groups_out, float mscale, int tile_h = kC3TH) {
  cp.Wf = static_cast<const _Float16 *>(Wf);
  cp.bias = bias; cp.res = res; cp.y = y; cp.stats = stats;
  cp.H = (int)H; cp.W = (int)W; cp.nch = (int)(Cin / 16); cp.cpg = stats ? (int)(Cout / groups_out) : 4;
  cp.cout = (int)Cout; cp.nnb = (int)(Cout / 128);
  cp.tiles_x = (int)(W / kC3TW); cp.tiles_y = (int)(H / tile_h);
  cp.ntiles = (long)B * cp.tiles_x * cp.tiles_y;
  cp.tiles_per_xcd = (cp.ntiles + 7) / 8;
  cp.mscale = mscale;
  return dim3((unsigned)(8 * cp.tiles_per_xcd * cp.nnb));
}

int conv3x3_gn_f16x3(const float *x, const float *gamma, const float *beta, const float *pre_bias_or_null,
                     const int64_t *stats_in, int64_t groups_in, double eps, int apply_silu, float scale, const void *Wf,
                     const float *bias_or_null, const float *res_or_null, float *y, int64_t *stats_out_or_null, int64_t B,
                     int64_t H, int64_t W, int64_t Cin, int64_t Cout, int64_t groups_out, float mscale, void *stream) {
  if (B < 0 || H < kC3TH || W < kC3TW || H % kC3TH || W % kC3TW || Cin < 32 || Cin % 32 != 0 || Cin > 512 || !one_of(Cout, {128, 256}) ||
      H * W > (1 << 22) || groups_in < 1 || Cin % groups_in != 0 || !(scale > 0.f))
    return GQHIP_ERR_INVALID_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (int rc = conv_prologue(B, x && gamma && beta && stats_in && Wf && y, stats_out_or_null, conv3_groups_ok(Cout, groups_out),
                             groups_out, st);
      rc != kGo)
    return rc;
  Conv3GnParams gp{};
  gp.c.Xs = nullptr;
  const dim3 grid = conv3_fill(gp.c, Wf, bias_or_null, res_or_null, y, stats_out_or_null, B, H, W, Cin, Cout, groups_out, mscale);
  gp.x = x; gp.gamma = gamma; gp.beta = beta; gp.pre_bias = pre_bias_or_null; gp.stats_in = stats_in;
  gp.cin = (int)Cin; gp.cpg_in = (int)(Cin / groups_in); gp.eps = eps; gp.scale = scale;
  static const int env_dyn = getenv("GQHIP_C3_DYNLDS") ? atoi(getenv("GQHIP_C3_DYNLDS")) : 0;   // diagnostic: extra LDS -> one block per CU
  if (Cout == 128) {
    if (apply_silu) hipLaunchKernelGGL((conv3x3_gn_f16x3_kernel<1, 128>), grid, dim3(256), env_dyn, st, gp);
    else hipLaunchKernelGGL((conv3x3_gn_f16x3_kernel<0, 128>), grid, dim3(256), 0, st, gp);
  } else {
    if (apply_silu) hipLaunchKernelGGL((conv3x3_gn_f16x3_kernel<1, 256>), grid, dim3(256), 0, st, gp);
    else hipLaunchKernelGGL((conv3x3_gn_f16x3_kernel<0, 256>), grid, dim3(256), 0, st, gp);
  }
  return check_launch();
}

#ifdef GQHIP_CLOCK_STAMPS
extern "C" int gqhip_debug_c3_stamps(unsigned long long *out, int64_t words) {   // diagnostic build only
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_c3_stamps), sizeof(unsigned long long) * words) == hipSuccess ? 0 : 1;
}
#endif

// ---- the 1x1 convolutions (gq_conv3.h: conv1x1_f16x3_kernel) ----
// Tiling: 256 pixels x 128 columns per block, two blocks per CU = 2 CUs slots.  Where that grid leaves the chip under-filled --
// fewer blocks than slots, or a last round less than 85 % full (the attention block at 16 x 32 x 32 pixels: q | k | v 768 blocks =
// 1.5 rounds of 512 slots, proj_out 256 = half a round) -- the 128-pixel tiling doubles the block count instead (1536 = three
// full rounds, 512 = one); every output bit and statistics record is the same (tests/test_gpu_attn_fused_proj.py).  HW % 256 != 0
// can only run with 128-pixel tiles.  GQHIP_CONV1_TILE = 128 | 256 forces one (A/B, tests); read per call, as GQHIP_WGEMM is.
// A forced 256 at HW % 256 != 0 is an invalid argument.  Returns rows of 32 pixels per wave (4 | 2), 0 = invalid.
// The rule is a heuristic, not a model of the schedule: it counts two slots per CU although some 128-pixel instantiations
// (the SPLIT ones, which the attention block launches, and <128, 2, 0, 0>) need few enough registers for three (profiles/r13/
// resource_usage.txt), and it was reasoned through and measured at the benchmark's batch of 16 only, where every nin_shortcut
// grid is a multiple of 512 blocks and keeps the 256-pixel tiling; at other batch sizes those calls may take 128-pixel tiles too
// (same results, speed not measured).
static int conv1_tile_rows(int64_t B, int64_t HW, int64_t Cout) {
  const char *knob = getenv("GQHIP_CONV1_TILE");
  if (knob && !strcmp(knob, "128")) return 2;
  if (knob && !strcmp(knob, "256")) return HW % 256 == 0 ? 4 : 0;
  if (HW % 256 != 0) return 2;
  static thread_local int cus_of[64];   // per device; 0 = not asked yet
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 4;
  if (cus_of[dev] == 0) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) return 4;
    cus_of[dev] = n;
  }
  const int64_t slots = 2 * (int64_t)cus_of[dev], blocks = B * (HW / 256) * (Cout / 128);
  if (blocks < slots) return 2;
  const int64_t last = blocks % slots;
  return (last != 0 && last * 100 < slots * 85) ? 2 : 4;
}

#define GQ_C1_LAUNCH(RR, GN)                                                                                             \
  do {                                                                                                                   \
    if (split) hipLaunchKernelGGL((conv1x1_f16x3_kernel<0, RR, GN, 1>), grid, dim3(256), 0, st, gp);                     \
    else if (Cout == 128) hipLaunchKernelGGL((conv1x1_f16x3_kernel<128, RR, GN, 0>), grid, dim3(256), 0, st, gp);        \
    else if (Cout == 256) hipLaunchKernelGGL((conv1x1_f16x3_kernel<256, RR, GN, 0>), grid, dim3(256), 0, st, gp);        \
    else if (Cout == 512) hipLaunchKernelGGL((conv1x1_f16x3_kernel<512, RR, GN, 0>), grid, dim3(256), 0, st, gp);        \
    else hipLaunchKernelGGL((conv1x1_f16x3_kernel<1536, RR, GN, 0>), grid, dim3(256), 0, st, gp);                        \
  } while (0)

// One launch path for the three entry points below.  gp: x, pre_bias, scales, and -- for the GroupNorm variant -- gamma, beta,
// stats_in, cpg_in, eps, and -- for the split epilogue -- Q3, K3, V3, sq, sv already filled in; gp.c filled here.  ptrs_ok: the entry
// point's required pointers are there (checked here, after the groups of the statistics and "nothing to do": conv_checks).
static int conv1_launch(Conv1Params &gp, bool ptrs_ok, const void *Wf, float mscale, const float *bias, const float *res, float *y,
                        int64_t *stats_out, int64_t B, int64_t HW, int64_t Cin, int64_t Cout, int64_t groups_out, void *stream) {
  const bool split = gp.Q3 != nullptr, gn = gp.gamma != nullptr;
  if (int rc = conv_checks(B, ptrs_ok, stats_out, conv3_groups_ok(Cout, groups_out)); rc != kGo) return rc;
  const int rows = conv1_tile_rows(B, HW, Cout);
  if (rows == 0) return GQHIP_ERR_INVALID_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (int rc = conv_stats_zero(stats_out, B * groups_out, st); rc != kGo) return rc;
  // the pixels as an image of HW / 32 rows of 32: a tile of 64 * rows pixels is 2 * rows of them
  const dim3 grid = conv3_fill(gp.c, Wf, bias, res, y, stats_out, B, HW / 32, 32, Cin, Cout, groups_out, mscale, 2 * rows);
  gp.cin = (int)Cin;
  if (rows == 4) {
    if (gn) GQ_C1_LAUNCH(4, 1); else GQ_C1_LAUNCH(4, 0);
  } else {
    if (gn) GQ_C1_LAUNCH(2, 1); else GQ_C1_LAUNCH(2, 0);
  }
#undef GQ_C1_LAUNCH
  return check_launch();
}

static bool conv1_shape_ok(int64_t B, int64_t HW, int64_t Cin) {
  return B >= 0 && HW >= 128 && HW % 128 == 0 && Cin >= 32 && Cin % 32 == 0 && HW <= (1 << 24);
}

static bool conv1_gn_ok(int64_t Cin, int64_t groups_in) {
  return Cin <= 512 && groups_in >= 1 && Cin % groups_in == 0 && (Cin / groups_in) % 4 == 0;
}

int conv1x1_f16x3(const float *x, const float *pre_bias_or_null, const void *Wf, const float *scales_dev_or_null, float scale,
                  float mscale, const float *bias_or_null, const float *res_or_null, float *y, int64_t *stats_out_or_null, int64_t B, int64_t HW,
                  int64_t Cin, int64_t Cout, int64_t groups_out, void *stream) {
  if (!conv1_shape_ok(B, HW, Cin) || !one_of(Cout, {128, 256, 512, 1536}) || !scale_ok(scales_dev_or_null, scale))
    return GQHIP_ERR_INVALID_ARG;
  Conv1Params gp{};
  gp.x = x; gp.pre_bias = pre_bias_or_null; gp.scales_dev = scales_dev_or_null; gp.scale = scale;
  return conv1_launch(gp, x && Wf && y, Wf, mscale, bias_or_null, res_or_null, y, stats_out_or_null, B, HW, Cin, Cout, groups_out,
                      stream);
}

int conv1x1_gn_f16x3(const float *x, const float *gamma, const float *beta, const float *pre_bias_or_null,
                     const int64_t *stats_in, int64_t groups_in, double eps, const void *Wf, float scale, float mscale,
                     const float *bias_or_null, const float *res_or_null, float *y, int64_t *stats_out_or_null, int64_t B,
                     int64_t HW, int64_t Cin, int64_t Cout, int64_t groups_out, void *stream) {
  if (!conv1_shape_ok(B, HW, Cin) || !conv1_gn_ok(Cin, groups_in) || !one_of(Cout, {128, 256, 512, 1536}) || !(scale > 0.f))
    return GQHIP_ERR_INVALID_ARG;
  Conv1Params gp{};
  gp.x = x; gp.pre_bias = pre_bias_or_null; gp.scale = scale;
  gp.gamma = gamma; gp.beta = beta; gp.stats_in = stats_in; gp.cpg_in = (int)(Cin / groups_in); gp.eps = eps;
  return conv1_launch(gp, x && gamma && beta && stats_in && Wf && y, Wf, mscale, bias_or_null, res_or_null, y, stats_out_or_null, B,
                      HW, Cin, Cout, groups_out, stream);
}

int conv1x1_qkv_split_f16x3(const float *x, const float *gamma_or_null, const float *beta_or_null, const float *pre_bias_or_null,
                            const int64_t *stats_in_or_null, int64_t groups_in, double eps, const void *Wf, float scale,
                            float mscale, const float *bias_or_null, void *Q3, void *K3, void *V3, float sq, float sv, int64_t B,
                            int64_t L, int64_t C, void *stream) {
  if (!conv1_shape_ok(B, L, C) || C % 128 != 0 || !(scale > 0.f) || !(sq > 0.f) || !(sv > 0.f))
    return GQHIP_ERR_INVALID_ARG;
  if (gamma_or_null && !conv1_gn_ok(C, groups_in)) return GQHIP_ERR_INVALID_ARG;
  const bool ptrs_ok = x && Wf && Q3 && K3 && V3 && (!gamma_or_null || (beta_or_null && stats_in_or_null));
  Conv1Params gp{};
  gp.x = x; gp.pre_bias = pre_bias_or_null; gp.scale = scale;
  if (gamma_or_null) {
    gp.gamma = gamma_or_null; gp.beta = beta_or_null; gp.stats_in = stats_in_or_null; gp.cpg_in = (int)(C / groups_in); gp.eps = eps;
  }
  gp.Q3 = static_cast<_Float16 *>(Q3); gp.K3 = static_cast<_Float16 *>(K3); gp.V3 = static_cast<_Float16 *>(V3);
  gp.sq = sq; gp.sv = sv;
  return conv1_launch(gp, ptrs_ok, Wf, mscale, bias_or_null, nullptr, nullptr, nullptr, B, L, C, 3 * C, 1, stream);
}

// the kernels instantiated for 128 | 256 | 512 output channels (conv3x3s2_f16x3, upconv2x_f16x3)
#define GQ_COUT3_LAUNCH(K)                                                                  \
  do {                                                                                      \
    if (Cout == 128) hipLaunchKernelGGL(K<128>, grid, dim3(256), 0, st, gp);                \
    else if (Cout == 256) hipLaunchKernelGGL(K<256>, grid, dim3(256), 0, st, gp);           \
    else hipLaunchKernelGGL(K<512>, grid, dim3(256), 0, st, gp);                            \
  } while (0)

int conv3x3s2_f16x3(const float *x, const void *Wf, const float *scales_dev_or_null, float scale, float mscale,
                    const float *bias_or_null, float *y, int64_t *stats_out_or_null, int64_t B, int64_t Hin, int64_t Win,
                    int64_t Cin, int64_t Cout, int64_t groups_out, void *stream) {
  // output H = Hin / 2, W = Win / 2 (the reference pads one zero row / column at the bottom / right: unet.py:92-95)
  if (B < 0 || Hin < 2 * kC3TH || Win < 2 * kC3TW || Hin % (2 * kC3TH) || Win % (2 * kC3TW) || Cin < 16 || Cin % 16 != 0 ||
      !one_of(Cout, {128, 256, 512}) || Hin * Win > (1 << 24) || !scale_ok(scales_dev_or_null, scale))
    return GQHIP_ERR_INVALID_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (int rc = conv_prologue(B, x && Wf && y, stats_out_or_null, conv3_groups_ok(Cout, groups_out), groups_out, st); rc != kGo)
    return rc;
  Conv3S2Params gp{};
  const dim3 grid = conv3_fill(gp.c, Wf, bias_or_null, nullptr, y, stats_out_or_null, B, Hin / 2, Win / 2, Cin, Cout, groups_out,
                               mscale);
  gp.x = x; gp.scales_dev = scales_dev_or_null; gp.scale = scale; gp.cin = (int)Cin; gp.Hin = (int)Hin; gp.Win = (int)Win;
  GQ_COUT3_LAUNCH(conv3x3s2_f16x3_kernel);
  return check_launch();
}

int upconv2x_f16x3(const float *x, const void *Wf, const float *scales_dev_or_null, float scale, float mscale,
                   const float *bias_or_null, float *y, int64_t *stats_out_or_null, int64_t B, int64_t H, int64_t W,
                   int64_t Cin, int64_t Cout, int64_t groups_out, void *stream) {
  if (B < 0 || H < kC3TH || W < kC3TW || H % kC3TH || W % kC3TW || Cin < 16 || Cin % 16 != 0 ||
      !one_of(Cout, {128, 256, 512}) || H * W > (1 << 22) || !scale_ok(scales_dev_or_null, scale))
    return GQHIP_ERR_INVALID_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (int rc = conv_prologue(B, x && Wf && y, stats_out_or_null, conv3_groups_ok(Cout, groups_out), groups_out, st); rc != kGo)
    return rc;
  Upconv2Params gp{};
  dim3 grid = conv3_fill(gp.c, Wf, bias_or_null, nullptr, y, stats_out_or_null, B, H, W, Cin, Cout, groups_out, mscale);
  grid.y = 4;   // the four sub-pixel phases
  gp.x = x; gp.scales_dev = scales_dev_or_null; gp.scale = scale; gp.cin = (int)Cin;
  GQ_COUT3_LAUNCH(upconv2x_f16x3_kernel);
  return check_launch();
}

#undef GQ_COUT3_LAUNCH

int conv3x3_gn_small_f32(const float *x, const float *gamma, const float *beta, const float *pre_bias_or_null,
                         const int64_t *stats_in, int64_t groups_in, double eps, int apply_silu, const float *w_ohwi,
                         const float *bias_or_null, float *y, int64_t B, int64_t H, int64_t W, int64_t Cin, int64_t Cout,
                         void *stream) {
  if (B < 0 || H < 16 || W < 16 || H % 16 || W % 16 || Cin < 32 || Cin % 32 != 0 || Cin > 512 || Cout < 1 || Cout > 4 ||
      groups_in < 1 || Cin % groups_in != 0 || B * (H / 16) * (W / 16) > 0x7fffffffL)
    return GQHIP_ERR_INVALID_ARG;
  if (B == 0) return GQHIP_OK;
  if (!x || !gamma || !beta || !stats_in || !w_ohwi || !y) return GQHIP_ERR_INVALID_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)(B * (H / 16) * (W / 16)));
  const int cpg = (int)(Cin / groups_in);
#define GQ_CS(S, CO)                                                                                                      \
  hipLaunchKernelGGL((conv3x3_gn_small_kernel<S, CO>), grid, dim3(256), 0, st, x, gamma, beta, pre_bias_or_null, stats_in, \
                     w_ohwi, bias_or_null, y, (int)H, (int)W, (int)Cin, cpg, eps)
#define GQ_CS2(CO) do { if (apply_silu) GQ_CS(1, CO); else GQ_CS(0, CO); } while (0)
  switch (Cout) {
    case 1: GQ_CS2(1); break;
    case 2: GQ_CS2(2); break;
    case 3: GQ_CS2(3); break;
    default: GQ_CS2(4); break;
  }
#undef GQ_CS2
#undef GQ_CS
  return check_launch();
}

int conv3x3_cin_small_f32(const float *x, const float *wk, const float *bias_or_null, float *y, int64_t *stats_out_or_null,
                          int64_t B, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int64_t groups_out, void *stream) {
  if (B < 0 || H < 8 || W < 32 || H % 8 || W % 32 || Cin < 1 || Cin > 4 || Cout != 128 || B * (H / 8) * (W / 32) > 0x7fffffffL)
    return GQHIP_ERR_INVALID_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (int rc = conv_prologue(B, x && wk && y, stats_out_or_null, groups_out == 32, 32, st); rc != kGo) return rc;
  ConvInParams cp{};
  cp.x = x; cp.wk = wk; cp.bias = bias_or_null; cp.y = y; cp.stats = stats_out_or_null; cp.H = (int)H; cp.W = (int)W;
  const dim3 grid((unsigned)(B * (H / 8) * (W / 32)));
  switch (Cin) {
    case 1: hipLaunchKernelGGL(conv3x3_cin_small_kernel<1>, grid, dim3(256), 0, st, cp); break;
    case 2: hipLaunchKernelGGL(conv3x3_cin_small_kernel<2>, grid, dim3(256), 0, st, cp); break;
    case 3: hipLaunchKernelGGL(conv3x3_cin_small_kernel<3>, grid, dim3(256), 0, st, cp); break;
    default: hipLaunchKernelGGL(conv3x3_cin_small_kernel<4>, grid, dim3(256), 0, st, cp); break;
  }
  return check_launch();
}

int conv3x3_f32(const float *x, const float *gamma_or_null, const float *beta_or_null, const float *pre_bias_or_null,
                const int64_t *stats_or_null, int64_t groups_in, double eps, int apply_silu, const float *wk,
                const float *bias_or_null, float *y, int64_t B, int64_t H, int64_t W, int64_t Cin, int64_t Cout, void *stream) {
  if (B < 0 || H < 1 || W < 1 || Cin < 8 || Cout < 4 || Cout % 4 != 0 || B * H * ((W + 31) / 32) > 0x7fffffffL)
    return GQHIP_ERR_INVALID_ARG;
  if (B == 0) return GQHIP_OK;
  if (!x || !wk || !y) return GQHIP_ERR_INVALID_ARG;
  const bool gn = stats_or_null != nullptr;
  if (gn && (!gamma_or_null || !beta_or_null || groups_in < 1 || Cin % groups_in != 0 || Cin > 1024)) return GQHIP_ERR_INVALID_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  ConvF32Params cp{};
  cp.x = x; cp.gamma = gamma_or_null; cp.beta = beta_or_null; cp.pre_bias = pre_bias_or_null; cp.stats = stats_or_null;
  cp.wk = wk; cp.bias = bias_or_null; cp.y = y;
  cp.H = (int)H; cp.W = (int)W; cp.Cin = (int)Cin; cp.Cout = (int)Cout; cp.cpg = gn ? (int)(Cin / groups_in) : 1; cp.eps = eps;
  const unsigned segs = (unsigned)(B * H * ((W + 31) / 32));
  if (Cin % 64 == 0) {
    // many input channels: K split over the waves of a block, partial tiles added in wave order
    const dim3 grid(segs, (unsigned)((Cout + 31) / 32));
    if (gn && apply_silu) hipLaunchKernelGGL((conv3x3_f32_ksplit_kernel<true, 1>), grid, dim3(256), 0, st, cp);
    else if (gn) hipLaunchKernelGGL((conv3x3_f32_ksplit_kernel<true, 0>), grid, dim3(256), 0, st, cp);
    else hipLaunchKernelGGL((conv3x3_f32_ksplit_kernel<false, 0>), grid, dim3(256), 0, st, cp);
    return check_launch();
  }
  if (gn) return GQHIP_ERR_INVALID_ARG;
  switch (Cin) {
    case 8: hipLaunchKernelGGL((conv3x3_f32_nsplit_kernel<8>), dim3(segs), dim3(256), 0, st, cp); break;
    case 16: hipLaunchKernelGGL((conv3x3_f32_nsplit_kernel<16>), dim3(segs), dim3(256), 0, st, cp); break;
    case 32: hipLaunchKernelGGL((conv3x3_f32_nsplit_kernel<32>), dim3(segs), dim3(256), 0, st, cp); break;
    default: return GQHIP_ERR_INVALID_ARG;
  }
  return check_launch();
}

static int wino_out_impl(int tile, const float *M, float *y, int64_t B, int64_t H, int64_t W, int64_t C, float mscale,
                         void *stream) {
  if (!wino_shape_ok(B, H, W, C, tile)) return GQHIP_ERR_INVALID_ARG;
  if (B == 0) return GQHIP_OK;
  if (!M || !y) return GQHIP_ERR_INVALID_ARG;
  const long tiles = (long)(B * (H / tile) * (W / tile)), total = tiles * (C / 4);
  // F(4x4,3x3) indexes in 64 bits at every shape (gq_unet_aux.h); F(2x2,3x3) has a wide twin
  const auto kernel = tile == 4 ? wino4_out_nhwc_kernel : wino_u32(B, H, W, C, tile, 4) ? wino_out_nhwc_kernel : wino_out_nhwc_wide_kernel;
  return launch(kernel, grid1d(total, 16384), dim3(256), 0, static_cast<hipStream_t>(stream), M, y, (int)H, (int)W, (int)(C / 4),
                tiles, total, mscale);
}

int wino_out_nhwc_f32(const float *M, float *y, int64_t B, int64_t H, int64_t W, int64_t C, float mscale, void *stream) {
  return wino_out_impl(2, M, y, B, H, W, C, mscale, stream);
}

int wino4_out_nhwc_f32(const float *M, float *y, int64_t B, int64_t H, int64_t W, int64_t C, float mscale, void *stream) {
  return wino_out_impl(4, M, y, B, H, W, C, mscale, stream);
}

int wino_out_res_nhwc_f32(const float *M, const float *res, const float *bias_or_null, float *y, int64_t *stats_out,
                          int64_t B, int64_t H, int64_t W, int64_t C, int64_t groups, int tile, float mscale,
                          void *stream) {
  if (!wino_shape_ok(B, H, W, C, tile)) return GQHIP_ERR_INVALID_ARG;
  // res may be NULL: bias + statistics only
  if (int rc = gn_check(B, C, H * W, groups, M && y && stats_out, true); rc != kGo) return rc;
  const int64_t cpg = C / groups;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (stats_zero(stats_out, sizeof(int64_t) * kStatWords * B * groups, st) != hipSuccess) return check_launch();
  const long tpi = (long)((H / tile) * (W / tile)), tiles = (long)B * tpi;
  // F(4x4,3x3): two channels per thread (see the kernel) wherever a block still spans whole pixels
  const int vw = (tile == 4 && 256 % (C / 2) == 0) ? 2 : 4;
  const int lanes = (int)(256 / (C / vw));
  long slabs = (tpi + (long)lanes * 4 - 1) / ((long)lanes * 4);    // ~4 tiles per thread
  if (slabs > 1024) slabs = 1024;
  if (slabs < 1) slabs = 1;
  const dim3 grid((unsigned)(B * slabs));
  // F(4x4,3x3) indexes in 64 bits at every shape (gq_unet_aux.h); F(2x2,3x3) has a wide twin
  const auto kernel = tile == 4 ? (vw == 2 ? wino_out_res_nhwc_kernel<4, 2> : wino_out_res_nhwc_kernel<4, 4>)
                                : wino_u32(B, H, W, C, tile, 4) ? wino_out_res_nhwc_kernel<2, 4>
                                                                            : wino_out_res_nhwc_wide_kernel<2, 4>;
  return launch(kernel, grid, dim3(256), 0, st, M, res, bias_or_null, y, stats_out, (int)H, (int)W, (int)(C / vw), (int)cpg, tiles,
                (int)slabs, mscale);
}

int attn_split_qkv_f16x3(const float *qkv, void *Q3, void *K3, void *V3, int64_t B, int64_t L, int64_t C, float sq, float sv,
                         void *stream) {
  if (B < 0 || L < 1 || C < 4 || C % 4 != 0 || !(sq > 0.f) || !(sv > 0.f)) return GQHIP_ERR_INVALID_ARG;
  if (B == 0) return GQHIP_OK;
  if (!qkv || !Q3 || !K3 || !V3) return GQHIP_ERR_INVALID_ARG;
  const long total = (long)(B * L * (C / 4));
  return launch(attn_split_qkv_kernel, grid1d(total, 16384), dim3(256), 0, static_cast<hipStream_t>(stream), qkv,
                static_cast<_Float16 *>(Q3), static_cast<_Float16 *>(K3), static_cast<_Float16 *>(V3), (long)L,
                (int)(C / 4), sq, sv, total);
}

int attn_softmax_split_f16x3(const float *S, void *P3, int64_t rows, int64_t L, float factor, void *stream) {
  if (rows < 0 || L < 64 || L % 64 != 0 || L > 4096 || !(factor > 0.f)) return GQHIP_ERR_INVALID_ARG;
  if (rows == 0) return GQHIP_OK;
  if (!S || !P3) return GQHIP_ERR_INVALID_ARG;
  const dim3 grid((unsigned)((rows + 3) / 4));
  hipStream_t st = static_cast<hipStream_t>(stream);
  _Float16 *p = static_cast<_Float16 *>(P3);
#define GQ_SM(N) hipLaunchKernelGGL(attn_softmax_split_kernel<N>, grid, dim3(256), 0, st, S, p, (long)rows, factor)
  switch (L / 64) {
    case 1: GQ_SM(1); break;
    case 4: GQ_SM(4); break;
    case 16: GQ_SM(16); break;
    case 36: GQ_SM(36); break;
    case 64: GQ_SM(64); break;
    default: return GQHIP_ERR_INVALID_ARG;
  }
#undef GQ_SM
  return check_launch();
}

int f16_scales_from_gn_stats(const int64_t *stats, int64_t n_bg, double amp, double u_scale, float *scales_out,
                             void *stream) {
  if (!stats || !scales_out || n_bg < 1 || n_bg > 0x7fffffff || !(amp > 0.0) || !(u_scale > 0.0)) return GQHIP_ERR_INVALID_ARG;
  return launch(f16_scales_from_stats_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), stats, (int)n_bg,
                (float)amp, (float)u_scale, scales_out);
}

int upsample2x_nhwc_f32(const float *x, float *y, int64_t B, int64_t H, int64_t W, int64_t C, void *stream) {
  if (B < 0 || H < 1 || W < 1 || C < 4 || C % 4 != 0) return GQHIP_ERR_INVALID_ARG;
  if (B == 0) return GQHIP_OK;
  if (!x || !y) return GQHIP_ERR_INVALID_ARG;
  const long total = (long)(B * H * W * (C / 4));
  return launch(upsample2x_nhwc_kernel, grid1d(total, 16384), dim3(256), 0, static_cast<hipStream_t>(stream), x,
                y, (int)H, (int)W, (int)(C / 4), total);
}

int gqhip_checksum_tensors(const void *table_dev, int64_t count, uint64_t *sums_dev, void *stream) {
  if (count < 0 || count > 65535) return GQHIP_ERR_INVALID_ARG;
  if (count == 0) return GQHIP_OK;
  if (!table_dev || !sums_dev) return GQHIP_ERR_INVALID_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(sums_dev, 0, sizeof(uint64_t) * count, st) != hipSuccess) return check_launch();
  return launch(checksum_tensors_kernel, dim3((unsigned)count, kChecksumSlices), dim3(256), 0, st,
                static_cast<const ChecksumEntry *>(table_dev), reinterpret_cast<unsigned long long *>(sums_dev));
}

int64_t gq_mha_workspace_bytes(int64_t B, int64_t L, int64_t E, int64_t H) {
  (void)B; (void)L; (void)E; (void)H;
  return 0;   // the fp32 route keeps everything on chip: no scratch
}

// the argument checks shared by the attention entry points: 0 = launch, 1 = nothing to do, -1 = invalid
static int mha_check(int64_t B, int64_t L, int64_t E, int64_t H, std::initializer_list<const void *> rows16,
                     std::initializer_list<const void *> words4) {
  if (B < 0 || L < 0 || H < 1 || E != H * kAttnD || B * H > 65535 || L > (int64_t)0x7fffffff / 3 / E) return -1;
  if (B == 0 || L == 0) return 1;
  for (const void *p : rows16)
    if (!p || ((uintptr_t)p & 15)) return -1;
  for (const void *p : words4)
    if (!p || ((uintptr_t)p & 3)) return -1;
  return 0;
}

int gq_mha_fwd_f32(const float *qkv, float *out, int64_t B, int64_t L, int64_t E, int64_t H, void *workspace, void *stream) {
  (void)workspace;
  const int c = mha_check(B, L, E, H, {qkv, out}, {});
  if (c) return c < 0 ? GQHIP_ERR_INVALID_ARG : GQHIP_OK;
  const dim3 grid((unsigned)((L + kAttnQRows - 1) / kAttnQRows), (unsigned)(B * H));
  return launch(mha_fwd_f32_kernel<false>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), qkv, out, nullptr, (int)L, (int)E,
                (int)H);
}

int gq_mha_fwd_lse_f32(const float *qkv, float *out, float *lse, int64_t B, int64_t L, int64_t E, int64_t H, void *workspace,
                       void *stream) {
  (void)workspace;
  const int c = mha_check(B, L, E, H, {qkv, out}, {lse});
  if (c) return c < 0 ? GQHIP_ERR_INVALID_ARG : GQHIP_OK;
  const dim3 grid((unsigned)((L + kAttnQRows - 1) / kAttnQRows), (unsigned)(B * H));
  return launch(mha_fwd_f32_kernel<true>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), qkv, out, lse, (int)L, (int)E, (int)H);
}

int64_t gq_mha_bwd_workspace_bytes(int64_t B, int64_t L, int64_t E, int64_t H) {
  (void)E;
  if (B < 0 || L < 0 || H < 0) return 0;
  return (2 * B * H * L * (int64_t)sizeof(float) + 255) / 256 * 256;   // n [B][H][L], then D [B][H][L] (gq_attn_bwd.h)
}

int gq_mha_bwd_f32(const float *qkv, const float *out, const float *lse, const float *dout, float *dqkv, int64_t B, int64_t L,
                   int64_t E, int64_t H, void *workspace, void *stream) {
  const int c = mha_check(B, L, E, H, {qkv, out, dout, dqkv}, {lse, workspace});
  if (c) return c < 0 ? GQHIP_ERR_INVALID_ARG : GQHIP_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((L + kAttnQRows - 1) / kAttnQRows), (unsigned)(B * H));
  float *rown = static_cast<float *>(workspace), *rowd = rown + B * H * L;
  // `out` is checked like the other tensors and not read: delta comes from P and dP (gq_attn_bwd.h)
  const int rc = launch(mha_bwd_dq_f32_kernel, grid, dim3(256), 0, st, qkv, lse, dout, dqkv, rown, rowd, (int)L, (int)E, (int)H);
  if (rc != GQHIP_OK) return rc;
  return launch(mha_bwd_dkdv_f32_kernel, grid, dim3(256), 0, st, qkv, lse, dout, rown, rowd, dqkv, (int)L, (int)E, (int)H);
}

}  // extern "C"
