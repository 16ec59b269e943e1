// gqhip.hip -- C-ABI entry points of libgqhip.so (see include/gqhip.h): the quantiser path (fused arg-max, compat score
// op, dequant, LFQ / FSQ, wire format) and the library-wide services.  The conv-stack entry points are in gqhip_unet.hip.
// gfx950 only; built by `make -C vq-vae-from-gaussian-vae_amd/csrc`.
#include "gqhip.h"

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdlib>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

#include "gqhip_internal.h"
#include "gq_aux.h"
#include "gq_common.h"
#include "gq_filter.h"
#include "gq_filter_bf16.h"
#include "gq_gauss_train.h"
#include "gq_grid.h"
#include "gq_lowdim.h"
#include "gq_prep.h"
#include "gq_rerank.h"
#include "gq_scores.h"
#include "gq_scores_f16.h"
#include "gq_ssim.h"
#include "vq_train.h"
#include "lfq_train.h"
#include "bsq_fsq_train.h"
#include "lpips_head.h"
#include "gq_moments.h"

using namespace gqhip;

namespace gqhip {
thread_local int g_last_hip_error = 0;

int check_launch() {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    g_last_hip_error = (int)e;
    return GQHIP_ERR_LAUNCH;
  }
  return GQHIP_OK;
}
}  // namespace gqhip

namespace {

// ---- diagnostic environment knobs ------------------------------------------
const char *env_str(const char *name) { return getenv(name); }
int env_int(const char *name, int dflt) {
  const char *e = env_str(name);
  return e ? atoi(e) : dflt;
}
double env_f64(const char *name, double dflt) {
  const char *e = env_str(name);
  return e ? atof(e) : dflt;
}
// GQHIP_FILTER=fp32|bf16|mixed, by their first letters in either case -> the kinds of gqhip_set_filter(); anything else: auto
int filter_kind_from(const char *e) {
  if (e && (e[0] == 'f' || e[0] == 'F') && (e[1] == 'p' || e[1] == 'P') && e[2] == '3') return GQHIP_FILTER_FP32;
  if (e && (e[0] == 'b' || e[0] == 'B')) return GQHIP_FILTER_BF16;
  if (e && (e[0] == 'm' || e[0] == 'M')) return GQHIP_FILTER_MIXED;   // fp16 + fp8
  return GQHIP_FILTER_AUTO;
}
// GQHIP_ODD_DIMS=padded, by its first letter in either case -> GQHIP_ODD_DIMS_PADDED; anything else: the exhaustive kernel
int odd_dims_kind_from(const char *e) { return e && (e[0] == 'p' || e[0] == 'P') ? GQHIP_ODD_DIMS_PADDED : GQHIP_ODD_DIMS_EXHAUSTIVE; }

// GQHIP_LOW_DIMS=search, by its first letter in either case -> GQHIP_LOW_DIMS_SEARCH; anything else: the exhaustive kernel
int low_dims_kind_from(const char *e) { return e && (e[0] == 's' || e[0] == 'S') ? GQHIP_LOW_DIMS_SEARCH : GQHIP_LOW_DIMS_EXHAUSTIVE; }

// GQHIP_WIDE_DIMS=filter, by its first letter in either case -> GQHIP_WIDE_DIMS_FILTER; anything else: the exhaustive kernel
int wide_dims_kind_from(const char *e) { return e && (e[0] == 'f' || e[0] == 'F') ? GQHIP_WIDE_DIMS_FILTER : GQHIP_WIDE_DIMS_EXHAUSTIVE; }

// Every GQHIP_* variable this translation unit reads: diagnostics and A/B timing, never needed in production.  Read once per
// process, when the library is loaded (g_filter_kind's initialiser is the first user).
struct Env {
  int filter = filter_kind_from(env_str("GQHIP_FILTER"));   // initial filter selection (gqhip_set_filter() changes it at run time)
  int odd_dims = odd_dims_kind_from(env_str("GQHIP_ODD_DIMS"));   // initial route of dims 5-7, 9-15, 17-31 (gqhip_set_odd_dims() changes it at run time)
  int low_dims = low_dims_kind_from(env_str("GQHIP_LOW_DIMS"));   // initial route of dims 1-3 (gqhip_set_low_dims() changes it at run time)
  int wide_dims = wide_dims_kind_from(env_str("GQHIP_WIDE_DIMS"));   // initial route of dims 33-64 (gqhip_set_wide_dims() changes it at run time)
  int rt = env_int("GQHIP_RT", 0);                           // 1 | 2: row tiles per wave of the filter (default: 2 from 8192 rows)
  int target_blocks = env_int("GQHIP_TARGET_BLOCKS", 0);     // > 0: filter blocks the code splits aim at (default: 256 / 512, make_plan)
  int nsplit = env_int("GQHIP_NSPLIT", 0);                   // > 0: code splits of the filter, before make_plan's caps
  int bf16_waves = env_int("GQHIP_BF16_WAVES", 0);           // 4: two 4-wave blocks per CU instead of one 8-wave block
  int bf16_ct = env_int("GQHIP_BF16_CT", 0);                 // 8: 8-tile LDS chunks at dim 16 too
  double ef_coeff = env_f64("GQHIP_EF_COEFF", 0.0);          // > 0: replaces the re-rank's error-bound coefficient in the launch
  int grid = env_int("GQHIP_GRID", 4);                       // dims of the pruned search: 0 none, 4, 8, 48 = both (dim 8 is slower than the dense path today)
  int grid_cap = env_int("GQHIP_GRID_CAP", 0);               // > 0: leaves a row may visit before it is handed to the scan (default 256)
  int grid_inwave = env_int("GQHIP_GRID_INWAVE", 0);         // > 0: listed leaves a row's lanes go through themselves (default kGridLeafCap)
  int grid_abl = env_int("GQHIP_GRID_ABL", 0);               // ablations of the search kernel (diagnostic builds, make abl, only)
  int grid_blocks = env_int("GQHIP_GRID_BLOCKS", 0);         // > 0: most blocks of the search launch (default 512)
  int finish_blocks = env_int("GQHIP_FINISH_BLOCKS", 0);     // > 0: blocks of the finish launch (default 256)
  int img_cache = env_int("GQHIP_IMG_CACHE", 1);             // 0: no codebook image in the cache, rebuilt in the workspace on every call
  char scores = env_str("GQHIP_SCORES") ? env_str("GQHIP_SCORES")[0] : 0;   // compat op: d(irect) per-pair kernel, f(32) MFMA kernel at dims 16 / 32 too
  int scores_nsplit = env_int("GQHIP_SCORES_NSPLIT", 0);     // > 0: code splits per row block of the compat op (tools/scores_sweep.sh)
  int scores_rot = env_int("GQHIP_SCORES_ROT", 3);           // bit 0 / 1 of its write rotation (gq_scores.h)
};
const Env &env() {
  static const Env e;
  return e;
}

// Filter selection: 0 = auto (the fp16 main-product filter at every MFMA dim, GQ and VQ), 1 = always the fp32 MFMA filter,
// 2 = split-bf16 wherever it applies, 3 = fp16 + fp8 (round 2's default: dim 16 / Gaussian score, split-bf16 elsewhere).
// Initial value from GQHIP_FILTER, changed at run time by gqhip_set_filter().  Every filter feeds the same exact re-rank, so the
// choice never changes an index.
std::atomic<int> g_filter_kind{env().filter};
int filter_kind() { return g_filter_kind.load(std::memory_order_relaxed); }

// Route of the dims between the filter dims (gqhip.h: gqhip_set_odd_dims).  The filter only nominates candidates and the re-rank
// scores with the true dim, so the choice never changes an index either.
std::atomic<int> g_odd_dims{env().odd_dims};
// the filter dim an odd dim is zero-padded to under PADDED (5-7 -> 8, 9-15 -> 16, 17-31 -> 32); 0: no such route for this dim
// (dims 1-3: 65 536 codes are dense in so few dimensions, the rows would live in the finish scan; 33-64: wide_dim below)
int64_t padded_dim(int64_t dim) {
  if (g_odd_dims.load(std::memory_order_relaxed) != GQHIP_ODD_DIMS_PADDED) return 0;
  if (dim > 4 && dim < 8) return 8;
  if (dim > 8 && dim < 16) return 16;
  if (dim > 16 && dim < 32) return 32;
  return 0;
}

// Route of dims 33-64 (gqhip.h: gqhip_set_wide_dims).  Under FILTER, with the fp16 main-product filter selected (AUTO), they run the
// filter and the re-rank at dim 64 -- 33-63 zero-padded as the odd dims are, 64 as it is.  The re-rank decides with the true dim, so the
// choice never changes an index.  Returns the filter dim, 0: no such route for this dim under the current selections.
std::atomic<int> g_wide_dims{env().wide_dims};
constexpr int64_t kWideDim = 64;
int64_t wide_dim(int64_t dim) {
  if (g_wide_dims.load(std::memory_order_relaxed) != GQHIP_WIDE_DIMS_FILTER || filter_kind() != GQHIP_FILTER_AUTO) return 0;
  return dim > 32 && dim <= kWideDim ? kWideDim : 0;
}

// Route of the Gaussian arg-max at dims 1-3 (gqhip.h: gqhip_set_low_dims): under SEARCH a call with a codebook cache runs the pruned
// exact search of gq_lowdim.h, whose winner is decided by the reference's arithmetic as on the exhaustive route: never another index.
std::atomic<int> g_low_dims{env().low_dims};

// ---- launch plan: identical on the sizing and the launching side -----------
struct Plan {
  bool mfma;            // filter kernel applies (dim in {4,8,16,32}, or 64 on the wide route; n >= 1)
  int rt;               // row tiles per wave
  int rows_per_block;   // 128 * rt
  int row_blocks;
  int nsplit;           // code splits
  int tiles_total;
  int tiles_per_split;
  int gt;               // tiles per candidate group: 4 for dim <= 8 and for the split-bf16 filter, else 2
  bool bf16;            // split-bf16 filter (gq_filter_bf16.h) instead of the fp32 MFMA one
  int ct;               // tiles per LDS chunk of the split-bf16 filter
  int waves;            // waves per block: 8 (one block per CU) for the split-bf16 filter, else 4
  bool mixed;           // dim 16, Gaussian score: fp16 main product + fp8 corrections instead of three bf16 products
  bool f16;             // fp16 main product only + the data-dependent bound of the re-rank (round 3: the default filter)
  int fdim;             // the dim the filter and the re-rank's templates run at: dim itself, the next filter dim on the padded route, 0 without a filter
  bool padded;          // fdim > dim: rows and codebook are zero-padded in the workspace first (run_padded)
  bool wide;            // the dim-64 filter of gqhip_set_wide_dims(FILTER): dims 33-63 padded to it, dim 64 itself

  // The fp16 + fp8 filter scores Gaussians only: under that selection a VQ call runs the split-bf16 kernels.  The sizing side does
  // not know the mode and sizes for the Gaussian score (mode defaulted), which needs no less.
  bool mixed_in(int mode) const { return mixed && mode == kModeGQ; }
  // The fp16 filters leave one record per lane half: two record sets per code split for the re-rank (<= kMaxSplit in all).
  int rec_halves(int mode = kModeGQ) const { return (mixed_in(mode) || f16) ? 2 : 1; }
  int rec_sets(int mode = kModeGQ) const { return nsplit * rec_halves(mode); }   // record sets per row the re-rank is told of
  int stored_rec_sets() const { return mfma ? rec_sets() : 0; }                   // ... and how many the workspace holds
};

// gq_filter_bf16.h / DESIGN.md section 3: 2 x 1057 (the two fp8 correction types: (2^-3 + 2^-8) relative on a term of at most
// 2^-11 (1 + 2^-11) |A s|) + 4 (dropped A_l s_l) + 1 (fp32 square) + 42 (operands in the fp8 / fp16 subnormal ranges: absolute
// errors, bounded against T for 1 <= max|cb| <= 16) + 4 * 32 + 2 * 64 (accumulation steps of the main product / of the
// corrections) = 2417, rounded up
constexpr float kMixedEfCoeff = 2450.0f;
constexpr float kMixedN1Limit = 16.0f;   // ... and max|cb| >= 1 (gq_rerank.h)
// fp16 main-product filter (gq_filter_bf16.h, F16): per product the two fp16 roundings, (1 + 2^-11)^2 - 1 = 16384 u + 4 u, the fp32
// roundings of A / B, of n^2 and of the row normalisation's inputs (3 u), 4 u per accumulation step of up to 2 x 64 slots
// ... charged for the widest layout of the default routes (dim 32: 64 products): 16384 + 4 + 3 + 4 * 64 = 16647, rounded up.  Operands
// in fp16's subnormal range are charged separately, as an absolute term (gq_rerank.h:f16_bound).
constexpr float kF16EfCoeff = 16700.0f;
// The dim-64 filter (wide route): 128 products per value, accumulated by eight chained v_mfma_f32_32x32x16_f16 (each adds its 16
// products to the fp32 accumulator the previous one left).  Whatever order the matrix core adds its 16 products in, a product takes
// part in at most 16 additions inside its MFMA and the accumulator in one more per later MFMA: at most 128 roundings on any path,
// each charged 4 u of the running magnitude (<= T) as above: 16384 + 4 + 3 + 4 * 128 = 16903, rounded up.
constexpr float kF16EfCoeffWide = 17000.0f;
constexpr float kF16N1Limit = 255.0f;    // n^2 must stay a finite fp16

// The re-rank's bound on the filter's error: its coefficient, and the range of max|cb| (n1) inside which it holds.
// The one place that knows them: the launch and gqhip_debug_plan (what the tests read) both ask here.
struct RerankBound {
  float ef_coeff, n1_limit, n1_min;
};
RerankBound rerank_bound(const Plan &pl, int mode, int64_t dim) {
  if (pl.f16) return {dim > 32 ? kF16EfCoeffWide : kF16EfCoeff, kF16N1Limit, 0.0f};   // `dim`: the filter dim
  if (pl.mixed_in(mode)) return {kMixedEfCoeff, kMixedN1Limit, 1.0f};
  return {pl.bf16 ? (float)(dim == 4 ? 332 : 220 + 24 * dim) : (float)(2 * dim + 4), 0.0f, 0.0f};
}

// Grid search (gq_grid.h) instead of filter + re-rank: dims 4 / 8 as GQHIP_GRID allows, filter selection AUTO, 2^14 <= n <= 2^20
// codes, and the caller passed a codebook cache of gqhip_cb_cache_bytes().
bool grid_dim_enabled(int64_t dim) {
  const int g = env().grid;
  return g == 48 ? (dim == 4 || dim == 8) : (g != 0 && dim == g);
}

// `wide`: dim is kWideDim and the caller is the wide route (without it dim 64 has no filter, as every dim outside the four has none)
Plan plan_at(int64_t rows, int64_t n, int64_t dim, bool wide = false) {
  const Env &e = env();
  Plan pl{};
  pl.wide = wide && dim == kWideDim;
  pl.mfma = (dim == 4 || dim == 8 || dim == 16 || dim == 32 || pl.wide) && n >= 1 && rows >= 1;
  pl.tiles_total = (int)((n + kTileCodes - 1) / kTileCodes);
  pl.rt = rows >= 8192 ? 2 : 1;
  if (e.rt == 1 || e.rt == 2) pl.rt = e.rt;
  pl.bf16 = pl.mfma && filter_kind() != GQHIP_FILTER_FP32;
  pl.waves = pl.bf16 ? (e.bf16_waves == 4 ? 4 : 8) : 4;
  pl.rows_per_block = 32 * pl.waves * pl.rt;
  pl.row_blocks = (int)((rows + pl.rows_per_block - 1) / pl.rows_per_block);
  // 4-wave blocks: ~2 blocks per CU on 256 CUs; 8-wave blocks: one per CU.  Splits in multiples of 8 so that
  // blockIdx % 8 (XCD) == split % 8.
  const int target = e.target_blocks > 0 ? e.target_blocks : (pl.waves == 8 ? 256 : 512);
  int s = (target + pl.row_blocks - 1) / (pl.row_blocks > 0 ? pl.row_blocks : 1);
  s = ((s + 7) / 8) * 8;
  if (e.nsplit > 0) s = e.nsplit;
  if (s > kMaxSplit) s = kMaxSplit;
  if (s > pl.tiles_total) s = pl.tiles_total;
  if (s < 1) s = 1;
  pl.tiles_per_split = (pl.tiles_total + s - 1) / s;
  // tiles per LDS chunk: 16 at dim 16 with one block per CU (2 x 64 KiB of LDS, half the chunk barriers: +1-2 %)
  pl.ct = dim == 32 ? 4 : ((dim == 16 && pl.waves == 8 && e.bf16_ct != 8) ? 16 : 8);

  // Candidate granularity: GT tiles per half-group.  Behind the bf16 / fp16 filters 4 (64-code candidates): the tracker's top-4
  // insert (12 VALU) runs once per GT tiles, and VALU issue is what those loops are short of (measured at config 2 with the
  // split-bf16 filter: GT 1 162 us, 2 157, 4 153; GT 8: filter -2 us, re-rank +14 us); the re-rank's fp32 pre-filter makes their
  // 16 GT codes cheap to go through.
  // dim 4 keeps the packed split-bf16 filter: 65 536 codes are dense in 4-d -- 3.5 candidate groups per row inside the fp16
  // margin and a quarter of the rows undecided (measured, profiles/r03) -- and its kernel is not MFMA-bound in the first place
  pl.f16 = pl.bf16 && filter_kind() == GQHIP_FILTER_AUTO && pl.waves == 8 && dim != 4;
  pl.gt = pl.bf16 ? 4 : (dim <= 8 ? 4 : 2);
  // (Measured in round 4 and not kept: groups of 8 tiles at dim 8, where the tracker's 12 VALU per group weigh twice what they do at
  // dim 16 -- filter 78.9 -> 75.1 us, but the re-rank's 128-code candidates give it back: whole call 128.4 -> 130.2 us.)
  pl.tiles_per_split = (pl.tiles_per_split + pl.gt - 1) / pl.gt * pl.gt;   // a tile group never straddles two splits
  pl.nsplit = (pl.tiles_total + pl.tiles_per_split - 1) / pl.tiles_per_split;
  pl.mixed = pl.bf16 && filter_kind() == GQHIP_FILTER_MIXED && dim == 16 && pl.waves == 8 && pl.ct == 16 && pl.gt == 4;
  if (pl.f16) pl.ct = dim == 32 ? 8 : 16;   // one 16-byte vector per MFMA, lane and tile: 16-tile chunks are 16 / 32 KiB
  if (pl.wide) pl.ct = 4;                   // dim 64: 8 KiB per tile, 4-tile chunks of 32 KiB as at dim 32
  const int split_cap = kMaxSplit / pl.rec_halves();   // the re-rank takes at most kMaxSplit record sets
  if (pl.nsplit > split_cap) {
    pl.tiles_per_split = ((pl.tiles_total + split_cap - 1) / split_cap + pl.gt - 1) / pl.gt * pl.gt;
    pl.nsplit = (pl.tiles_total + pl.tiles_per_split - 1) / pl.tiles_per_split;
  }
  // The records carry half-group ids RELATIVE to their split in 16 bits (gq_common.h:Rec): 2 * tiles_per_split / GT <= 65536, i.e.
  // at most 2^20 GT codes per split.  More splits where that is not so (n > 2^22 at the bench's 8..16 splits); codebooks beyond what
  // the split cap allows (n > 2^26 GT / 2: 134 M codes at GT 4) leave the MFMA path for the exhaustive kernel.
  const int64_t max_tps = 32768LL * pl.gt;
  if (pl.mfma && pl.tiles_per_split > max_tps) {
    const int64_t need = (pl.tiles_total + max_tps - 1) / max_tps;
    if (need > split_cap) {
      pl.mfma = pl.bf16 = pl.f16 = pl.mixed = false;
    } else {
      pl.tiles_per_split = (int)(((pl.tiles_total + need - 1) / need + pl.gt - 1) / pl.gt * pl.gt);
      pl.nsplit = (pl.tiles_total + pl.tiles_per_split - 1) / pl.tiles_per_split;
    }
  }
  pl.fdim = pl.mfma ? (int)dim : 0;
  return pl;
}

// The one place that decides the route: the plan of `dim`, or -- under GQHIP_ODD_DIMS_PADDED, for a dim between two filter dims --
// the plan of the filter dim it is padded to, marked `padded`; or -- under GQHIP_WIDE_DIMS_FILTER, for dims 33-64 -- the plan of the
// dim-64 filter, `padded` below 64.
Plan make_plan(int64_t rows, int64_t n, int64_t dim) {
  if (const int64_t dw = wide_dim(dim)) {
    Plan pl = plan_at(rows, n, dw, true);
    if (pl.mfma && pl.f16) {      // (only the fp16 main-product filter has a dim-64 kernel; beyond the split cap: exhaustive, as below)
      pl.padded = dim < dw;
      return pl;
    }
  }
  if (const int64_t dp = padded_dim(dim)) {
    Plan pl = plan_at(rows, n, dp);
    if (pl.mfma) {      // (a codebook beyond the split cap runs the exhaustive kernel, at its true dim)
      pl.padded = true;
      return pl;
    }
  }
  return plan_at(rows, n, dim);
}

inline int64_t align256(int64_t v) { return (v + 255) / 256 * 256; }

// Dims 8 / 16 / 32 (the fp16 main-product filter): the codebook's fp16 operand image is kept in the cache, every 1/256 slice of it
// validated against -- and, when stale, rebuilt and restamped by -- the code block of the first launch that owns it (gq_prep.h).
// GQHIP_IMG_CACHE=0 disables it (A/B timing): the image is then rebuilt in the workspace on every call, as before round 5.
// (What the image depends on -- tiles, chunk padding, vectors -- does not depend on rows: any plan of (n, dim) serves.)
int64_t image_cache_bytes(const Plan &pl, int64_t dim) {
  if (env().img_cache == 0 || (dim != 8 && dim != 16 && dim != 32) || filter_kind() != GQHIP_FILTER_AUTO || !pl.f16) return 0;
  return (int64_t)sizeof(GridHdr) + align256((int64_t)(pl.tiles_total + pl.ct) * (dim / 8) * 64 * 16);
}

// The one answer to "which codebook cache does (n, dim) keep, and how many bytes": the index of the dim-4 / 8 search first, then the
// index of the dims 1-3 search, then the fp16 image.  An index also names its stamp and the bucket size beyond which it is degenerate.
// (Whether a search RUNS is the caller's to add: run_argmax wants the caller's buffer, the dim-4 / 8 search the AUTO filter besides.)
struct CacheUse {
  enum Kind { kNone, kImage, kGrid, kLow } kind;
  int64_t bytes;
  unsigned magic;
  int degenerate_above;
  bool fits(const void *cache, int64_t cache_bytes) const { return kind != kNone && cache && cache_bytes >= bytes; }
};
// `pl`: a plan of (n, dim) the caller already has (any serves: what the image depends on does not depend on rows)
CacheUse cache_use(int64_t n, int64_t dim, const Plan *pl = nullptr) {
  if (grid_dim_enabled(dim) && n >= 16384 && n <= (1 << 20)) return {CacheUse::kGrid, grid_layout(n, dim).total, kGridMagic, 255};
  if (g_low_dims.load(std::memory_order_relaxed) == GQHIP_LOW_DIMS_SEARCH && dim >= 1 && dim <= 3 && n >= 4096 && n <= (1 << 20))
    return {CacheUse::kLow, low_layout(n, dim).total, kLowMagic, low_cell_cap(n)};
  if (n < 1 || dim < 1 || dim > kMaxDim) return {CacheUse::kNone, 0, 0u, 0};
  const int64_t img = image_cache_bytes(pl ? *pl : make_plan(65536, n, dim), dim);
  return {img > 0 ? CacheUse::kImage : CacheUse::kNone, img, 0u, 0};
}
bool grid_applies(int64_t n, int64_t dim, const void *cache, int64_t cache_bytes, const Plan &pl) {
  const CacheUse u = cache_use(n, dim, &pl);
  return u.kind == CacheUse::kGrid && u.fits(cache, cache_bytes) && filter_kind() == GQHIP_FILTER_AUTO;
}
bool low_applies(int64_t n, int64_t dim, const void *cache, int64_t cache_bytes, const Plan &pl) {
  const CacheUse u = cache_use(n, dim, &pl);
  return u.kind == CacheUse::kLow && u.fits(cache, cache_bytes);
}

struct WsLayout {
  int64_t hdr, rec, fb, dbg, mu, sd, lsd, rowsum, coef, cbimg, rowimg, rowscale, rowaux, kl2, pmu, psd, plsd, pcb, total;
};

// `dim`: the caller's; on the padded route everything the filter and the re-rank read is sized at pl.fdim, and the padded rows and the
// zero-padded fp32 codebook they gather from follow the regions of every other route
WsLayout ws_layout(const Plan &pl, int64_t rows, int64_t dim_true) {
  WsLayout w{};
  const int64_t dim = pl.padded ? pl.fdim : dim_true;     // (the wide route at dim 64 itself: fdim == dim_true, no padded copies)
  int64_t off = 0;
  w.hdr = off; off += (int64_t)sizeof(WsHeader);
  w.rec = off; off += align256((int64_t)sizeof(Rec) * rows * pl.stored_rec_sets());
  w.fb = off;  off += align256(4 * rows);
  w.dbg = off; off += 128 * 1024;     // diagnostic builds only (GQHIP_CLOCK_STAMPS: per-block timeline records of the filter | of the re-rank)
  w.mu = off;  off += align256(4 * rows * dim_true);
  w.sd = off;  off += align256(4 * rows * dim_true);
  w.lsd = off; off += align256(4 * rows * dim_true);
  w.rowsum = off; off += pl.mfma ? align256(8 * 4 * rows) : 0;
  w.coef = off; off += pl.mfma ? align256(4 * 2 * rows * dim) : 0;
  // split-bf16 operand images: 2*NV vectors of 16 B per (code, half) / (row, half), NV = dim / 8
  const int64_t nvec = pl.f16 ? (dim == 4 ? 1 : dim / 8) : (dim == 4 ? 2 : dim / 4);
  w.cbimg = off;  off += pl.bf16 ? align256((int64_t)(pl.tiles_total + pl.ct) * nvec * 64 * 16) : 0;
  w.rowimg = off; off += pl.bf16 ? align256(rows * nvec * 2 * 16) : 0;
  w.rowscale = off; off += (pl.mixed || pl.f16) ? align256(4 * rows) : 0;
  w.rowaux = off; off += pl.f16 ? align256(32 * rows) : 0;
  w.kl2 = off; off += align256(4 * rows);       // per-row KL bits of gq_quantize_z_gauss_f32
  if (pl.padded) {
    w.pmu = off;  off += align256(4 * rows * dim);
    w.psd = off;  off += align256(4 * rows * dim);
    w.plsd = off; off += align256(4 * rows * dim);
    w.pcb = off;  off += align256(4 * (int64_t)pl.tiles_total * kTileCodes * dim);
  }
  w.total = off;
  return w;
}

// ---- profiling recorder ------------------------------------------------------
std::mutex g_prof_mu;
bool g_prof_on = false;
int g_debug_stats = 0;
std::vector<std::pair<hipEvent_t, hipEvent_t>> g_prof_events;   // attached to a dispatch, not yet collected
std::vector<std::pair<hipEvent_t, hipEvent_t>> g_prof_pool;     // created ahead of time (gqhip_profile_reserve)

}  // namespace

// When profiling is on, the filter is launched with a start and a stop event attached to the dispatch itself (gqhip_internal.h:
// launch), so the elapsed time is the kernel's own duration on its stream (what rocprofv3 --kernel-trace reports), not a
// marker-to-marker bracket.  The event pairs come from a pool filled by gqhip_profile_reserve(): nothing is created on the launch
// path, and a launch that finds the pool empty simply is not recorded.
gqhip::ProfScope::ProfScope(bool enable) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  if (g_prof_on && enable && !g_prof_pool.empty()) {
    a = g_prof_pool.back().first;
    b = g_prof_pool.back().second;
    g_prof_pool.pop_back();
    on = true;
  }
}
gqhip::ProfScope::~ProfScope() {
  if (on) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof_events.emplace_back(a, b);
  }
}

namespace {

// ---- which kernel serves a plan: one function per family, nullptr = no instantiation for that shape (GQHIP_ERR_INVALID_ARG) ------
using FilterKernel = void (*)(FilterParams);
using FilterBfKernel = void (*)(FilterBfParams);
using PrepKernel = void (*)(PrepParams);
using RerankKernel = void (*)(RerankParams);

template <int MODE>
FilterKernel filter_kernel(const Plan &pl, int64_t dim) {
  switch (dim * 10 + pl.rt) {
    case 41: return gq_filter_kernel<4, 1, 8, MODE, 4>;
    case 42: return gq_filter_kernel<4, 2, 8, MODE, 4>;
    case 81: return gq_filter_kernel<8, 1, 8, MODE, 4>;
    case 82: return gq_filter_kernel<8, 2, 8, MODE, 4>;
    case 161: return gq_filter_kernel<16, 1, 8, MODE, 2>;
    case 162: return gq_filter_kernel<16, 2, 8, MODE, 2>;
    case 321: return gq_filter_kernel<32, 1, 4, MODE, 2>;
    case 322: return gq_filter_kernel<32, 2, 4, MODE, 2>;
    default: return nullptr;
  }
}

// the split-bf16 kernel <NV, RT, CT> of either block size
template <int NV, int RT, int CT>
FilterBfKernel bf16_kernel(int waves) {
  return waves == 8 ? gq_filter_bf16_kernel<NV, RT, CT, 4, 8> : gq_filter_bf16_kernel<NV, RT, CT, 4, 4>;
}
// fp16 main product (FK 2) | fp16 + fp8 (FK 1, dim 16) | split-bf16: template arguments <NV = dim / 8, RT, CT, GT, WAVES, FK>
FilterBfKernel filter_bf16_kernel(const Plan &pl, int64_t dim, bool mixed) {
  const int key = (int)dim * 10 + pl.rt;
  if (pl.f16) {
    switch (key) {
      case 81: return gq_filter_bf16_kernel<1, 1, 16, 4, 8, 2>;
      case 82: return gq_filter_bf16_kernel<1, 2, 16, 4, 8, 2>;
      case 161: return gq_filter_bf16_kernel<2, 1, 16, 4, 8, 2>;
      case 162: return gq_filter_bf16_kernel<2, 2, 16, 4, 8, 2>;
      case 321: return gq_filter_bf16_kernel<4, 1, 8, 4, 8, 2>;
      case 322: return gq_filter_bf16_kernel<4, 2, 8, 4, 8, 2>;
      case 641: return gq_filter_bf16_kernel<8, 1, 4, 4, 8, 2>;     // the wide route: eight MFMAs per tile and row tile
      case 642: return gq_filter_bf16_kernel<8, 2, 4, 4, 8, 2>;
      default: return nullptr;
    }
  }
  switch (key) {
    case 41: return bf16_kernel<0, 1, 8>(pl.waves);
    case 42: return bf16_kernel<0, 2, 8>(pl.waves);
    case 81: return bf16_kernel<1, 1, 8>(pl.waves);
    case 82: return bf16_kernel<1, 2, 8>(pl.waves);
    // dim 16: the 16-tile chunks of the plan (pl.ct == 16: one 8-wave block per CU) have a split-bf16 kernel at two row tiles only;
    // one row tile runs 8-tile chunks over the same image (its padding covers either)
    case 161: return mixed ? gq_filter_bf16_kernel<2, 1, 16, 4, 8, 1> : bf16_kernel<2, 1, 8>(pl.waves);
    case 162:
      if (mixed) return gq_filter_bf16_kernel<2, 2, 16, 4, 8, 1>;
      return pl.ct == 16 ? gq_filter_bf16_kernel<2, 2, 16, 4, 8> : bf16_kernel<2, 2, 8>(pl.waves);
    case 321: return bf16_kernel<4, 1, 4>(pl.waves);
    case 322: return bf16_kernel<4, 2, 4>(pl.waves);
    default: return nullptr;
  }
}

// images: 0 none or split-bf16 (the same kernel writes them when the parameters name them), 1 fp16 + fp8, 2 fp16 main product
template <int MODE, bool FROM_Z>
PrepKernel prep_kernel_z(int64_t dim, bool mixed, bool f16) {
  if constexpr (MODE == kModeGQ) {
    if (mixed && dim == 16) return gq_prep_kernel<MODE, 16, FROM_Z, 1>;
  }
  switch ((int)dim * 10 + (f16 ? 2 : 0)) {
    case 40: return gq_prep_kernel<MODE, 4, FROM_Z>;
    case 80: return gq_prep_kernel<MODE, 8, FROM_Z>;
    case 160: return gq_prep_kernel<MODE, 16, FROM_Z>;
    case 320: return gq_prep_kernel<MODE, 32, FROM_Z>;
    case 82: return gq_prep_kernel<MODE, 8, FROM_Z, 2>;
    case 162: return gq_prep_kernel<MODE, 16, FROM_Z, 2>;
    case 322: return gq_prep_kernel<MODE, 32, FROM_Z, 2>;
    case 642: return gq_prep_kernel<MODE, 64, FROM_Z, 2>;     // the wide route
    default: return nullptr;
  }
}
template <int MODE>
PrepKernel prep_kernel(bool from_z, int64_t dim, bool mixed, bool f16) {
  return from_z ? prep_kernel_z<MODE, true>(dim, mixed, f16) : prep_kernel_z<MODE, false>(dim, mixed, f16);
}

// re-rank: 16 lanes per row, 16 rows per block; NSI = record passes per lane (1 covers up to 16 record sets: every BASELINE shape)
template <int MODE, int DIM, int GT>
RerankKernel rerank_kernel_nsi(int rec_sets) {
  return rec_sets <= 16 ? gq_rerank_kernel<MODE, DIM, GT, 1> : gq_rerank_kernel<MODE, DIM, GT, 4>;
}
// ... and of a padded call: the same block with the scorer, the output and nothing else at the true dim (gq_rerank.h)
template <int MODE, int DIM, int GT>
RerankKernel rerank_pad_kernel_nsi(int rec_sets) {
  return rec_sets <= 16 ? gq_rerank_pad_kernel<MODE, DIM, GT, 1> : gq_rerank_pad_kernel<MODE, DIM, GT, 4>;
}
template <int MODE>
RerankKernel rerank_pad_kernel(int64_t dim, int gt, int rec_sets) {
  switch (dim * 100 + gt) {
    case 804: return rerank_pad_kernel_nsi<MODE, 8, 4>(rec_sets);
    case 1602: return rerank_pad_kernel_nsi<MODE, 16, 2>(rec_sets);
    case 1604: return rerank_pad_kernel_nsi<MODE, 16, 4>(rec_sets);
    case 3202: return rerank_pad_kernel_nsi<MODE, 32, 2>(rec_sets);
    case 3204: return rerank_pad_kernel_nsi<MODE, 32, 4>(rec_sets);
    case 6404: return rerank_pad_kernel_nsi<MODE, 64, 4>(rec_sets);     // dims 33-63 on the wide route
    default: return nullptr;
  }
}
template <int MODE>
RerankKernel rerank_kernel(int64_t dim, int gt, int rec_sets) {
  switch (dim * 100 + gt) {
    case 404: return rerank_kernel_nsi<MODE, 4, 4>(rec_sets);
    case 804: return rerank_kernel_nsi<MODE, 8, 4>(rec_sets);
    case 1602: return rerank_kernel_nsi<MODE, 16, 2>(rec_sets);
    case 1604: return rerank_kernel_nsi<MODE, 16, 4>(rec_sets);
    case 3202: return rerank_kernel_nsi<MODE, 32, 2>(rec_sets);
    case 3204: return rerank_kernel_nsi<MODE, 32, 4>(rec_sets);
    case 6404: return rerank_kernel_nsi<MODE, 64, 4>(rec_sets);         // dim 64 on the wide route
    default: return nullptr;
  }
}

struct GridKernels {
  void (*build)(IndexBuildParams);
  void (*search)(GridParams);
  void (*finish)(GridParams);
};
template <int MODE>
GridKernels grid_kernels(int64_t dim) {   // (grid_applies() has let dims 4 / 8 through)
  if (dim == 4) return {gq_grid_build_kernel<4>, gq_grid_kernel<MODE, 4>, gq_grid_finish_kernel<MODE, 4>};
  return {gq_grid_build_kernel<8>, gq_grid_kernel<MODE, 8>, gq_grid_finish_kernel<MODE, 8>};
}

// What the first launch reads: either z in the module layout (FROM_Z) or ready-made rows.
struct PrepInput {
  const float *z = nullptr, *noise = nullptr;
  float *zhat_noquant = nullptr;
  float lv_min = 0.f, lv_max = 0.f;
  float *mu_out = nullptr, *sd_out = nullptr;   // FROM_Z: optional copies of the row operands for the caller
  float *sd_layout = nullptr;                   // FROM_Z: optional sd in the layout of zhat
  bool want_kl2 = false;                        // FROM_Z: leave the per-row KL bits in the workspace (WsLayout::kl2)
  int ste_kind = 0;                             // straight-through mix where zhat is stored (gq_common.h:WsHeader)
  const float *ste = nullptr;
  float *pure = nullptr;
  GaussStatsParams gs{};                        // want_kl2: the statistics block's parameters (kl2row is filled in by prep_params)
  bool *stats_done = nullptr;                   // out: the statistics block ran inside the re-rank launch (no launch of its own needed)
  WsLayout *layout = nullptr;                   // out: where this call put things in the workspace, for the kernels the caller appends
};

// One arg-max call after its checks: what the three paths below share.
struct Call {
  const PrepInput &in;
  const float *lsd;                             // the caller's log sd rows, or NULL
  const float *cb;
  int64_t *idx;
  float *zhat;
  int64_t dim, rows, n;
  double beta;
  void *cb_cache;
  int64_t cb_cache_bytes;
  const OutMap &omap;
  hipStream_t st;
  Plan pl;
  WsLayout w;
  char *ws;
  WsHeader *hdr;
  float *ws_lsd;
  const float *r_mu, *r_sd, *r_lsd;             // the rows every later kernel reads
  int64_t dim_true = 0;                         // > 0: `dim` is the filter dim of a padded call, rows and `cb` its padded copies (run_padded)
  bool from_z() const { return in.z != nullptr; }
  template <class T>
  T *at(int64_t off) const { return reinterpret_cast<T *>(ws + off); }
};

template <int MODE>
RerankParams rerank_params(const Call &c) {
  const Plan &pl = c.pl;
  RerankParams rp{};
  rp.mu = c.r_mu; rp.sd = MODE == kModeGQ ? c.r_sd : nullptr; rp.lsd = c.r_lsd; rp.cb = c.cb;
  rp.rowsum = c.at<const double>(c.w.rowsum);
  rp.coef = c.at<const float>(c.w.coef);
  rp.rec = c.at<const Rec>(c.w.rec);
  rp.idx = c.idx; rp.zhat = c.zhat; rp.hdr = c.hdr;
  rp.fb_list = c.at<int>(c.w.fb);
  rp.rows = (int)c.rows; rp.n = (int)c.n; rp.dim = (int)(c.dim_true ? c.dim_true : c.dim);
  const RerankBound b = rerank_bound(pl, MODE, c.dim);
  rp.ef_coeff = env().ef_coeff > 0.0 ? (float)env().ef_coeff : b.ef_coeff;
  rp.n1_limit = b.n1_limit; rp.n1_min = b.n1_min;
  if (pl.f16) rp.rowaux = c.at<const float>(c.w.rowaux);
  rp.beta = (float)c.beta; rp.nsplit = pl.rec_sets(MODE); rp.gt = pl.gt; rp.all_rows = pl.mfma ? 0 : 1; rp.stats = g_debug_stats;
  rp.omap = c.omap;
  rp.dbg = c.ws + c.w.dbg + 64 * 1024;
  rp.rec_halves = pl.rec_halves(MODE);
  rp.tiles_per_split = pl.tiles_per_split; rp.tiles_total = pl.tiles_total;
  return rp;
}

// The first launch of the MFMA dims: rows (+ zhat_noquant), bound sums, max|cb| partials, header -- and, on the dense path, the
// operand images of the plan's filter.  The grid search reads no image; the cache it validates is its spatial index
// (`cache_stale`: the builder that follows rebuilds it), where the dense path may keep the codebook's fp16 image in the cache.
template <int MODE>
PrepParams prep_params(const Call &c, bool grid, bool stats_in_rerank) {
  const PrepInput &in = c.in;
  const Plan &pl = c.pl;
  const bool scaled = !grid && (pl.mixed_in(MODE) || pl.f16);
  PrepParams pp{};
  pp.z = in.z; pp.noise = in.noise; pp.zhat_noquant = in.zhat_noquant; pp.lv_min = in.lv_min; pp.lv_max = in.lv_max;
  pp.sd_layout = in.sd_layout; pp.kl2row = in.want_kl2 ? c.at<float>(c.w.kl2) : nullptr;
  pp.ste_kind = in.ste_kind; pp.ste = in.ste; pp.pure = in.pure;
  if (stats_in_rerank) {
    pp.gs = in.gs;
    pp.gs.kl2row = pp.kl2row;
  }
  pp.mu = const_cast<float *>(c.r_mu); pp.sd = const_cast<float *>(c.r_sd);
  pp.lsd = const_cast<float *>(c.from_z() ? c.ws_lsd : c.lsd);
  pp.lsd_out = (!c.from_z() && MODE == kModeGQ && !c.lsd) ? c.ws_lsd : nullptr;
  pp.rowsum = c.at<double>(c.w.rowsum);
  pp.coef = c.at<float>(c.w.coef);
  pp.cb = c.cb;
  pp.hdr = c.hdr; pp.rows = c.rows; pp.n = (int)c.n; pp.tiles_total = pl.tiles_total;
  pp.row_blocks = (int)((c.rows * c.dim + 255) / 256);
  pp.beta = (float)c.beta; pp.omap = c.omap;
  pp.rowimg = (!grid && pl.bf16) ? c.at<u32x4>(c.w.rowimg) : nullptr;
  pp.cbimg = (!grid && pl.bf16) ? c.at<u32x4>(c.w.cbimg) : nullptr;
  pp.rowscale = scaled ? c.at<float>(c.w.rowscale) : nullptr;
  pp.rowaux = (!grid && pl.f16) ? c.at<float>(c.w.rowaux) : nullptr;
  GridHdr *ch = reinterpret_cast<GridHdr *>(c.cb_cache);
  const int64_t img = grid ? 0 : image_cache_bytes(pl, c.dim);
  if (grid) {
    pp.cache_sums = ch->blk_sum; pp.cache_stale = &ch->stale;
  } else if (ch && img > 0 && c.cb_cache_bytes >= img) {
    pp.cbimg = reinterpret_cast<u32x4 *>(static_cast<char *>(c.cb_cache) + sizeof(GridHdr));
    pp.cache_sums = ch->blk_sum;     // (of the header only the slice hashes are used: a slice is current iff its hash matches)
  }
  return pp;
}

// dims outside {4, 8, 16, 32}: prep -> exact score of every code (gq_exhaustive_kernel)
// the rows of a call without a gq_prep_kernel at its dim: header zeroed, then (module entry points) z -> rows at the true dim with
// zhat_noquant, sd_out, the per-row KL bits and the straight-through words
template <int MODE>
int run_prep_plain(const Call &c) {
  const PrepInput &in = c.in;
  if (hipMemsetAsync(c.hdr, 0, sizeof(WsHeader), c.st) != hipSuccess) return check_launch();
  if (c.from_z()) {
    PrepPlainParams pq{};
    pq.z = in.z; pq.noise = in.noise; pq.zhat_noquant = in.zhat_noquant;
    pq.sd_layout = in.sd_layout; pq.kl2row = in.want_kl2 ? c.at<float>(c.w.kl2) : nullptr;
    pq.vq = MODE == kModeVQ ? 1 : 0;
    pq.hdr = c.hdr; pq.ste_kind = in.ste_kind; pq.ste = in.ste; pq.pure = in.pure;
    pq.mu = const_cast<float *>(c.r_mu); pq.sd = const_cast<float *>(c.r_sd); pq.lsd = c.ws_lsd;
    pq.rows = c.rows; pq.dim = (int)c.dim; pq.lv_min = in.lv_min; pq.lv_max = in.lv_max; pq.omap = c.omap;
    return launch(prep_plain_kernel, dim3((unsigned)((c.rows * c.dim + 255) / 256)), dim3(256), 0, c.st, pq);
  }
  return GQHIP_OK;
}

template <int MODE>
int run_exhaustive(const Call &c) {
  const int rc = run_prep_plain<MODE>(c);
  if (rc != GQHIP_OK) return rc;
  const int ex_blocks = (int)(c.rows < 4096 ? c.rows : 4096);
  return launch(gq_exhaustive_kernel<MODE>, dim3((unsigned)ex_blocks), dim3(256), 0, c.st, rerank_params<MODE>(c));
}

// Dims 1-3 under GQHIP_LOW_DIMS_SEARCH with a codebook cache (GQ): rows as on the exhaustive path -> codebook hash and max|cb| ->
// index builder (exits unless the hash or the stamp says the cache is stale) -> pruned exact search (gq_lowdim.h) -> the rows it
// listed, through gq_exhaustive_kernel itself (exits at once when there are none).
// the second launch of both searches: one block that exits unless the hash or the stamp says the index is not current
int launch_index_builder(const Call &c, void (*build)(IndexBuildParams), int threads) {
  IndexBuildParams bp{};
  bp.cb = c.cb; bp.cache = static_cast<char *>(c.cb_cache); bp.hdr = c.hdr; bp.n = (int)c.n;
  return launch(build, dim3(1), dim3((unsigned)threads), 0, c.st, bp);
}

int run_low(const Call &c) {
  int rc = run_prep_plain<kModeGQ>(c);
  if (rc != GQHIP_OK) return rc;
  LowHashParams hp{};
  hp.cb = c.cb; hp.hdr = c.hdr; hp.cache = static_cast<GridHdr *>(c.cb_cache); hp.count = (long)(c.n * c.dim);
  rc = launch(gq_low_hash_kernel, dim3(kLowHashBlocks), dim3(256), 0, c.st, hp);
  if (rc != GQHIP_OK) return rc;
  const auto build = c.dim == 1 ? gq_low_build_kernel<1> : (c.dim == 2 ? gq_low_build_kernel<2> : gq_low_build_kernel<3>);
  rc = launch_index_builder(c, build, kLowBuildThreads);
  if (rc != GQHIP_OK) return rc;
  RerankParams rp = rerank_params<kModeGQ>(c);
  rp.all_rows = 0;                                  // the finish launch: the listed rows only
  LowParams lp{};
  lp.mu = c.r_mu; lp.sd = c.r_sd; lp.lsd = c.r_lsd; lp.cb = c.cb; lp.cache = static_cast<const char *>(c.cb_cache);
  lp.idx = c.idx; lp.zhat = c.zhat; lp.hdr = c.hdr; lp.fb_list = rp.fb_list;
  lp.rows = (int)c.rows; lp.n = (int)c.n; lp.beta = (float)c.beta; lp.stats = g_debug_stats; lp.omap = c.omap;
  const auto search = c.dim == 1 ? gq_low_search_kernel<1> : (c.dim == 2 ? gq_low_search_kernel<2> : gq_low_search_kernel<3>);
  const int64_t nsets = (c.rows + 15) / 16;
  rc = launch(ProfScope(), search, dim3((unsigned)(nsets < 4096 ? nsets : 4096)), dim3(kLowThreads), 0, c.st, lp);
  if (rc != GQHIP_OK) return rc;
  const int fin_blocks = (int)(c.rows < 1024 ? c.rows : 1024);
  return launch(gq_exhaustive_kernel<kModeGQ>, dim3((unsigned)fin_blocks), dim3(256), 0, c.st, rp);
}

// dims 4 / 8 with a codebook cache: prep (rows, bound sums, max|cb|, codebook hash) -> index builder (exits unless the hash says the
// cache is stale) -> pruned exact search (gq_grid.h) -> the rows it left undecided.  Four launches, no filter, no re-rank.
template <int MODE>
int run_grid(const Call &c) {
  const Env &e = env();
  const GridKernels k = grid_kernels<MODE>(c.dim);
  const PrepParams pp = prep_params<MODE>(c, true, false);
  const dim3 pgrid((unsigned)(pp.row_blocks + kPrepCodeBlocks));
  int rc = launch(prep_kernel<MODE>(c.from_z(), c.dim, false, false), pgrid, dim3(256), 0, c.st, pp);
  if (rc != GQHIP_OK) return rc;
  rc = launch_index_builder(c, k.build, kGridBuildThreads);
  if (rc != GQHIP_OK) return rc;
  GridParams gp{};
  gp.mu = c.r_mu; gp.sd = c.r_sd; gp.lsd = c.r_lsd; gp.rowsum = pp.rowsum; gp.coef = pp.coef; gp.cb = c.cb;
  gp.cache = static_cast<const char *>(c.cb_cache);
  gp.idx = c.idx; gp.zhat = c.zhat; gp.hdr = c.hdr; gp.rows = (int)c.rows; gp.n = (int)c.n; gp.beta = (float)c.beta;
  gp.leaf_cap = e.grid_cap > 0 ? e.grid_cap : 256;     // leaves a row may visit before it is handed to the scan (a flat score)
  gp.inwave_cap = e.grid_inwave > 0 ? e.grid_inwave : kGridLeafCap;
  gp.stats = g_debug_stats; gp.omap = c.omap;
  gp.abl = e.grid_abl;
  // the list of undecided rows lives in the (otherwise unused) candidate-record region: 16 B x rows x record sets >= 12 B x rows
  gp.und_row = c.at<int>(c.w.rec);
  gp.und_thr = c.at<float>(c.w.rec) + c.rows;
  gp.und_margin = c.at<float>(c.w.rec) + 2 * c.rows;
  const int64_t nsets = (c.rows + 31) / 32;                        // (a block's eight waves fetch four rows at a time from a counter)
  const int64_t max_blocks = e.grid_blocks > 0 ? e.grid_blocks : 512;
  const dim3 ggrid((unsigned)(nsets < max_blocks ? nsets : max_blocks));   // two 512-thread blocks per CU: one wave of blocks
  rc = launch(ProfScope(), k.search, ggrid, dim3(kGridThreads), 0, c.st, gp);
  if (rc != GQHIP_OK) return rc;
  // launch 4: the rows the search left undecided, a block per row (exits at once when there are none)
  const dim3 fgrid((unsigned)(e.finish_blocks > 0 ? e.finish_blocks : 256));
  return launch(k.finish, fgrid, dim3(kGridThreads), 0, c.st, gp);
}

// prep -> filter -> re-rank.  Three launches per call (round 4: the rows the candidates cannot decide are finished inside the
// re-rank, gq_rerank.h); `stats_in_rerank`: one more block of the re-rank launch runs GQ2's statistics (gq_gauss.h).
template <int MODE>
int run_dense(const Call &c, bool stats_in_rerank) {
  const Plan &pl = c.pl;
  const bool mixed = pl.mixed_in(MODE);
  // ---- launch 1 ----
  const PrepParams pp = prep_params<MODE>(c, false, stats_in_rerank);
  const dim3 pgrid((unsigned)(pp.row_blocks + kPrepCodeBlocks));
  int rc = launch(prep_kernel<MODE>(c.from_z(), c.dim, mixed, pl.f16), pgrid, dim3(256), 0, c.st, pp);
  if (rc != GQHIP_OK) return rc;

  // ---- launch 2: the filter ----
  const dim3 fgrid((unsigned)(pl.row_blocks * pl.nsplit));
  if (pl.bf16) {
    FilterBfParams fp{};
    fp.cbimg = pp.cbimg; fp.rowimg = pp.rowimg;
    fp.rec = c.at<Rec>(c.w.rec);
    fp.rows = (int)c.rows; fp.n = (int)c.n;
    fp.nsplit = pl.nsplit; fp.tiles_total = pl.tiles_total; fp.tiles_per_split = pl.tiles_per_split;
    fp.hdr = c.hdr;
    fp.dbg = c.ws + c.w.dbg;    // diagnostic builds only
    fp.rowscale = pp.rowscale;
    rc = launch(ProfScope(), filter_bf16_kernel(pl, c.dim, mixed), fgrid, dim3((unsigned)(64 * pl.waves)), 0, c.st, fp);
  } else {
    FilterParams fp{};
    fp.mu = c.r_mu; fp.sd = c.r_sd; fp.cb = c.cb;
    fp.rec = c.at<Rec>(c.w.rec);
    fp.rows = (int)c.rows; fp.n = (int)c.n; fp.beta = (float)c.beta;
    fp.nsplit = pl.nsplit; fp.tiles_total = pl.tiles_total; fp.tiles_per_split = pl.tiles_per_split;
    fp.hdr = c.hdr;
    fp.dbg = c.ws + c.w.dbg;      // diagnostic builds only
    rc = launch(ProfScope(), filter_kernel<MODE>(pl, c.dim), fgrid, dim3(256), 0, c.st, fp);
  }
  if (rc != GQHIP_OK) return rc;

  // ---- launch 3: exact re-rank of the candidates; rows they cannot decide are finished by their own block ----
  const RerankParams rp = rerank_params<MODE>(c);
  const dim3 rgrid((unsigned)((c.rows + 15) / 16 + (stats_in_rerank ? 1 : 0)));
  const RerankKernel rk = c.dim_true ? rerank_pad_kernel<MODE>(c.dim, rp.gt, rp.nsplit) : rerank_kernel<MODE>(c.dim, rp.gt, rp.nsplit);
  return launch(rk, rgrid, dim3(256), 0, c.st, rp);
}

// Dims 5-7, 9-15, 17-31 under GQHIP_ODD_DIMS_PADDED, dims 33-63 under GQHIP_WIDE_DIMS_FILTER: rows at the true dim as on the exhaustive path (so zhat_noquant, sd_out, the KL
// bits and the VQ loss's rows are what they are there), gq_pad_kernel -> rows and codebook zero-padded to the plan's filter dim, then
// the dense path on the padded copies: its from-rows prep, the selected filter and the re-rank, which scores and stores at the true dim.
// No codebook cache: the padded operand image is rebuilt in the workspace on every call.
template <int MODE>
int run_padded(const Call &c) {
  int rc = run_prep_plain<MODE>(c);
  if (rc != GQHIP_OK) return rc;
  const int64_t dp = c.pl.fdim;
  PadParams pd{};
  pd.mu = c.r_mu; pd.sd = MODE == kModeGQ ? c.r_sd : nullptr;
  pd.lsd = MODE == kModeGQ ? (c.from_z() ? c.ws_lsd : c.lsd) : nullptr;
  pd.cb = c.cb;
  pd.pmu = c.at<float>(c.w.pmu); pd.psd = c.at<float>(c.w.psd); pd.plsd = c.at<float>(c.w.plsd); pd.pcb = c.at<float>(c.w.pcb);
  pd.rows = (long)c.rows; pd.n = (long)c.n; pd.dim = (int)c.dim; pd.dp = (int)dp;
  const int64_t pblocks = ((c.rows + c.n) * dp + 255) / 256;
  rc = launch(gq_pad_kernel, dim3((unsigned)(pblocks < kPadMaxBlocks ? pblocks : kPadMaxBlocks)), dim3(256), 0, c.st, pd);
  if (rc != GQHIP_OK) return rc;
  PrepInput pin;
  pin.ste_kind = c.in.ste_kind; pin.ste = c.in.ste; pin.pure = c.in.pure;
  Call cp{pin, MODE == kModeGQ ? pd.plsd : nullptr, pd.pcb, c.idx, c.zhat, dp, c.rows, c.n, c.beta, nullptr, 0, c.omap, c.st, c.pl, c.w, c.ws};
  cp.hdr = c.hdr; cp.ws_lsd = pd.plsd;
  cp.r_mu = pd.pmu; cp.r_sd = pd.psd; cp.r_lsd = MODE == kModeGQ ? pd.plsd : nullptr;
  cp.dim_true = c.dim;
  return run_dense<MODE>(cp, false);
}

// The fused arg-max, shared by GQ and VQ: checks, plan and workspace layout (once per call), the rows every kernel reads, then one
// of the three paths above.  Nothing derived from the codebook or the rows survives the call outside the caller's codebook cache.
template <int MODE>
int run_argmax(const PrepInput &in, const float *mu, const float *sd, const float *lsd, const float *cb, int64_t *idx,
               float *zhat, int64_t dim, int64_t rows, int64_t n, double beta, void *workspace,
               int64_t workspace_bytes, void *cb_cache, int64_t cb_cache_bytes, const OutMap &omap, hipStream_t st) {
  if (dim < 1 || dim > kMaxDim || rows < 0 || n < 1 || n > 0x3fffffff || rows > 0x3fffffff)
    return GQHIP_ERR_INVALID_ARG;
  if (rows == 0) return GQHIP_OK;   // empty batch: nothing to do (pointers may be NULL)
  const bool from_z = in.z != nullptr;
  if (!cb || !idx || (!from_z && (!mu || (MODE == kModeGQ && !sd)))) return GQHIP_ERR_INVALID_ARG;
  const Plan pl = make_plan(rows, n, dim);
  const WsLayout w = ws_layout(pl, rows, dim);
  if (!workspace || workspace_bytes < w.total) return GQHIP_ERR_WORKSPACE;
  if (in.layout) *in.layout = w;
  Call c{in, lsd, cb, idx, zhat, dim, rows, n, beta, cb_cache, cb_cache_bytes, omap, st, pl, w, static_cast<char *>(workspace)};
  c.hdr = c.at<WsHeader>(w.hdr);
  c.ws_lsd = c.at<float>(w.lsd);
  c.r_mu = from_z ? (in.mu_out ? in.mu_out : c.at<float>(w.mu)) : mu;
  c.r_sd = from_z ? (in.sd_out ? in.sd_out : c.at<float>(w.sd)) : sd;
  c.r_lsd = from_z ? c.ws_lsd : (MODE == kModeGQ ? (lsd ? lsd : (pl.mfma ? c.ws_lsd : nullptr)) : nullptr);
  if (!pl.mfma) {     // the one place that chooses between the exhaustive kernel and the low-dim search
    if constexpr (MODE == kModeGQ)
      if (low_applies(n, dim, cb_cache, cb_cache_bytes, pl)) return run_low(c);
    return run_exhaustive<MODE>(c);
  }
  if (pl.padded) {
    if (in.stats_done) *in.stats_done = false;     // GQ2's statistics: the launch of their own the exhaustive path has
    return run_padded<MODE>(c);
  }
  const bool grid = grid_applies(n, dim, cb_cache, cb_cache_bytes, pl);
  const bool stats_in_rerank = MODE == kModeGQ && in.want_kl2 && !grid;
  if (in.stats_done) *in.stats_done = stats_in_rerank;
  return grid ? run_grid<MODE>(c) : run_dense<MODE>(c, stats_in_rerank);
}

// ---- the module-level entry points: (B, L, c, dim, layout, grouping) -> groups per position, rows, and where a row's outputs go ----
struct ZGeom {
  int64_t K = 0, rows = 0;
  OutMap om{};
};
// `strict` off (gq_dequant_f32 only): that entry point has never bounded dim by kMaxDim -- its kernel takes any -- nor rejected
// layout / grouping values outside the enums (read as BLC / as the kernel reads them), and callers may rely on either.
bool z_geometry(int64_t B, int64_t L, int64_t c, int64_t dim, int layout, int grouping, ZGeom *g, bool strict = true) {
  if (B < 0 || L < 1 || c < 1 || dim < 1 || c % dim != 0) return false;
  if (strict && (dim > kMaxDim || (layout != GQHIP_LAYOUT_BCHW && layout != GQHIP_LAYOUT_BLC) ||
                 (grouping != GQHIP_GROUP_STRIDED && grouping != GQHIP_GROUP_CONTIGUOUS)))
    return false;
  g->K = c / dim;
  g->rows = B * L * g->K;
  g->om.mode = layout == GQHIP_LAYOUT_BCHW ? 1 : 2;
  g->om.K = (int)g->K; g->om.L = (int)L; g->om.c = (int)c; g->om.grouping = grouping;
  return true;
}
// ---- the host vocabulary of the train steps: alignment, geometry, workspace rule, workspace carving, launch chain ----
// every pointer given is NULL or aligned to `mask` + 1 bytes
template <class... P>
bool aligned(unsigned mask, const P *...p) { return ((reinterpret_cast<uintptr_t>(p) | ... | (uintptr_t)0) & mask) == 0; }
// g->P positions, g->L of them per image, g->mode 1 = "bchw" / 2 = "blc"; false: a negative size, an unknown layout, or B, L, B L or B L
// `per_position` beyond 2^30 - 1.  (Not under z_geometry: that wants L >= 1 and leaves the bound to its callers, behind their "nothing to do".)
template <class G>
bool train_geometry(int64_t B, int64_t L, int layout, int64_t per_position, G *g) {
  const int64_t lim = 0x3fffffff;
  if (B < 0 || L < 0 || B > lim || L > lim || B * L > lim || B * L * per_position > lim) return false;
  if (layout != GQHIP_LAYOUT_BCHW && layout != GQHIP_LAYOUT_BLC) return false;
  g->P = (long)(B * L); g->L = (long)L; g->mode = layout == GQHIP_LAYOUT_BCHW ? 1 : 2;
  return true;
}
// the one workspace rule: there, 16-byte aligned, and of at least `need` bytes
int workspace_status(const void *ws, int64_t bytes, int64_t need) {
  return ws && aligned(15u, ws) && bytes >= need ? GQHIP_OK : GQHIP_ERR_WORKSPACE;
}
struct Carve {   // a workspace handed out front to back in 256-byte steps: take() is where the next block starts, `off` the bytes taken so far
  int64_t off = 0;
  int64_t take(int64_t bytes) { const int64_t at = off; off += align256(bytes); return at; }
};
template <class T>
T *at(void *workspace, int64_t off) { return reinterpret_cast<T *>(static_cast<char *>(workspace) + off); }   // ... and the block taken at `off`
struct Chain {   // launches on one stream, in order, through launch() (gqhip_internal.h): `rc` is the first failing status, nothing is launched after it
  hipStream_t st;
  int rc = GQHIP_OK;
  explicit Chain(void *stream) : st(static_cast<hipStream_t>(stream)) {}
  template <class... P, class... A>
  Chain &run(void (*kernel)(P...), dim3 grid, dim3 block, A &&...args) {
    if (rc == GQHIP_OK) rc = launch(kernel, grid, block, 0, st, static_cast<A &&>(args)...);
    return *this;
  }
};

// the statistics block's parameters (gq_gauss.h); `kl2row` may be filled in later
GaussStatsParams gauss_stats_params(const float *kl2row, int64_t rows, double *lam_state, void *scalars, double log2n, double tolerance,
                                    double lam_factor, double lam_lo, double lam_hi, int lam_max_decreases, double loss_divisor) {
  GaussStatsParams gp{};
  gp.kl2row = kl2row; gp.rows = (long)rows; gp.lam_state = lam_state; gp.scalars = scalars;
  gp.thr_hi = (float)(log2n + tolerance); gp.thr_lo = (float)(log2n - tolerance); gp.log2n = (float)log2n;
  gp.lam_factor = lam_factor; gp.lam_lo = lam_lo; gp.lam_hi = lam_hi; gp.lam_max_decreases = lam_max_decreases;
  gp.loss_divisor = loss_divisor;
  return gp;
}

}  // namespace

extern "C" {

int gqhip_abi_version(void) { return GQHIP_ABI_VERSION; }

const char *gqhip_status_string(int s) {
  switch (s) {
    case GQHIP_OK: return "ok";
    case GQHIP_ERR_INVALID_ARG: return "invalid argument";
    case GQHIP_ERR_WORKSPACE: return "workspace missing or too small";
    case GQHIP_ERR_LAUNCH: return "kernel launch failed";
    case GQHIP_ERR_NO_DEVICE: return "no HIP device";
    default: return "unknown status";
  }
}

int gqhip_last_hip_error(void) { return g_last_hip_error; }

int gqhip_set_filter(int kind) {
  if (kind != GQHIP_FILTER_AUTO && kind != GQHIP_FILTER_FP32 && kind != GQHIP_FILTER_BF16 && kind != GQHIP_FILTER_MIXED)
    return GQHIP_ERR_INVALID_ARG;
  g_filter_kind.store(kind, std::memory_order_relaxed);
  return GQHIP_OK;
}

int gqhip_get_filter(void) { return g_filter_kind.load(std::memory_order_relaxed); }

int gqhip_set_odd_dims(int kind) {
  if (kind != GQHIP_ODD_DIMS_EXHAUSTIVE && kind != GQHIP_ODD_DIMS_PADDED) return GQHIP_ERR_INVALID_ARG;
  g_odd_dims.store(kind, std::memory_order_relaxed);
  return GQHIP_OK;
}

int gqhip_get_odd_dims(void) { return g_odd_dims.load(std::memory_order_relaxed); }

int gqhip_set_low_dims(int kind) {
  if (kind != GQHIP_LOW_DIMS_EXHAUSTIVE && kind != GQHIP_LOW_DIMS_SEARCH) return GQHIP_ERR_INVALID_ARG;
  g_low_dims.store(kind, std::memory_order_relaxed);
  return GQHIP_OK;
}

int gqhip_get_low_dims(void) { return g_low_dims.load(std::memory_order_relaxed); }

int gqhip_set_wide_dims(int kind) {
  if (kind != GQHIP_WIDE_DIMS_EXHAUSTIVE && kind != GQHIP_WIDE_DIMS_FILTER) return GQHIP_ERR_INVALID_ARG;
  g_wide_dims.store(kind, std::memory_order_relaxed);
  return GQHIP_OK;
}

int gqhip_get_wide_dims(void) { return g_wide_dims.load(std::memory_order_relaxed); }

int gqhip_low_dim_search_applies(int64_t n, int64_t dim) { return cache_use(n, dim).kind == CacheUse::kLow; }

int64_t gqhip_filter_dim(int64_t n, int64_t dim) {
  if (n < 1 || dim < 1 || dim > kMaxDim) return -1;
  return make_plan(65536, n, dim).fdim;
}

int gqhip_debug_plan(int64_t rows, int64_t n, int64_t dim, int64_t *out8_host) {
  if (!out8_host || rows < 1 || n < 1 || dim < 1 || dim > kMaxDim) return GQHIP_ERR_INVALID_ARG;
  const Plan pl = make_plan(rows, n, dim);
  out8_host[0] = ws_layout(pl, rows, dim).rec; out8_host[1] = pl.stored_rec_sets();
  out8_host[2] = pl.gt; out8_host[3] = pl.tiles_per_split;
  out8_host[4] = pl.f16 ? 3 : (pl.mixed ? 2 : (pl.bf16 ? 1 : 0));   // 0 fp32 MFMA filter, 1 split-bf16, 2 fp16 + fp8 (Gaussian score), 3 fp16 main product
  out8_host[5] = (int64_t)rerank_bound(pl, kModeGQ, pl.mfma ? pl.fdim : dim).ef_coeff;
  out8_host[6] = pl.rt; out8_host[7] = pl.waves;
  return GQHIP_OK;
}

int gqhip_grid_search_applies(int64_t n, int64_t dim) {
  return cache_use(n, dim).kind == CacheUse::kGrid && filter_kind() == GQHIP_FILTER_AUTO;
}

int gqhip_cb_cache_degenerate(const void *cb_cache, int64_t n, int64_t dim) {
  const CacheUse use = cache_use(n, dim);
  if (!cb_cache || (use.kind != CacheUse::kGrid && use.kind != CacheUse::kLow)) return -1;
  GridHdr g;
  if (hipMemcpy(&g, cb_cache, sizeof(g), hipMemcpyDeviceToHost) != hipSuccess) { (void)check_launch(); return -1; }
  if (!index_current(&g, use.magic, (int)n, (int)dim)) return -1;
  return g.max_sub > use.degenerate_above ? 1 : 0;
}

int64_t gqhip_cb_cache_bytes(int64_t n, int64_t dim) {
  if (n < 1 || dim < 1 || dim > kMaxDim) return -1;
  return cache_use(n, dim).bytes;
}

int64_t gqhip_workspace_bytes(int64_t rows, int64_t n, int64_t dim) {
  if (rows < 0 || n < 1 || dim < 1 || dim > kMaxDim) return -1;
  if (rows < 1) rows = 1;
  return ws_layout(make_plan(rows, n, dim), rows, dim).total;
}

// the per-pair kernel of the compat op at the MFMA dims (gq_aux.h), 16 rows per block; nullptr: any other dim
static auto scores_pair_kernel(int64_t dim, bool beta1) -> decltype(&gq_scores_kernel<4, 16, true>) {
  switch (dim * 2 + (beta1 ? 1 : 0)) {
    case 8: return gq_scores_kernel<4, 16, false>;
    case 9: return gq_scores_kernel<4, 16, true>;
    case 16: return gq_scores_kernel<8, 16, false>;
    case 17: return gq_scores_kernel<8, 16, true>;
    case 32: return gq_scores_kernel<16, 16, false>;
    case 33: return gq_scores_kernel<16, 16, true>;
    case 64: return gq_scores_kernel<32, 16, false>;
    case 65: return gq_scores_kernel<32, 16, true>;
    default: return nullptr;
  }
}

int gq_scores_f32(const float *mu, const float *sd, const float *cb, float *out, int64_t dim,
                  int64_t rows, int64_t n, double beta, void *stream) {
  if (dim < 1 || rows < 0 || n < 1 || n > 0x7fffffff || rows > 0x7fffffff) return GQHIP_ERR_INVALID_ARG;
  if (rows == 0) return GQHIP_OK;
  if (!mu || !sd || !cb || !out) return GQHIP_ERR_INVALID_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const Env &e = env();
  // Default: the score matrix on the matrix cores, HBM-write bound -- dims 16 / 32 as three fp16 products of two-term splits
  // (gq_scores_f16.h), dims 4 / 8 on the fp32 matrix cores (gq_scores.h; GQHIP_SCORES=f32: at every dim).  GQHIP_SCORES=direct:
  // the per-pair restatement of the CUDA kernel's formula (VALU bound, ~3x slower).  Non-finite beta, dims outside
  // {4, 8, 16, 32}: per-pair kernels.
  if (e.scores != 'd' && (dim == 4 || dim == 8 || dim == 16 || dim == 32) && beta == beta && n >= 32) {
    ScoresParams sp{};
    sp.mu = mu; sp.sd = sd; sp.cb = cb; sp.out = out; sp.rows = (int)rows; sp.n = (int)n; sp.beta = beta;
    sp.tiles_total = (int)((n + kTileCodes - 1) / kTileCodes);
    sp.rot = e.scores_rot;
    constexpr int RT = 2;
    const int row_blocks = (int)((rows + 128 * RT - 1) / (128 * RT));
    int s = (512 + row_blocks - 1) / row_blocks;      // ~2 blocks per CU; splits in multiples of 8 (XCD = blockIdx % 8)
    s = ((s + 7) / 8) * 8;
    if (e.scores_nsplit > 0) s = e.scores_nsplit;
    if (s > sp.tiles_total) s = sp.tiles_total;
    if (s < 1) s = 1;
    sp.tiles_per_split = (sp.tiles_total + s - 1) / s;
    sp.nsplit = (sp.tiles_total + sp.tiles_per_split - 1) / sp.tiles_per_split;
    const dim3 grid((unsigned)(row_blocks * sp.nsplit));
    const bool f16x3 = e.scores != 'f';
    if (f16x3 && dim == 16) return launch(gq_scores_f16x3_kernel<16, RT, 8>, grid, dim3(256), 0, st, sp);
    if (f16x3 && dim == 32) return launch(gq_scores_f16x3_kernel<32, RT, 4>, grid, dim3(256), 0, st, sp);
    switch (dim) {
      case 4: return launch(gq_scores_mfma_kernel<4, RT, 8>, grid, dim3(256), 0, st, sp);
      case 8: return launch(gq_scores_mfma_kernel<8, RT, 8>, grid, dim3(256), 0, st, sp);
      case 16: return launch(gq_scores_mfma_kernel<16, RT, 8>, grid, dim3(256), 0, st, sp);
      default: return launch(gq_scores_mfma_kernel<32, RT, 4>, grid, dim3(256), 0, st, sp);
    }
  }
  const int cpt = 1;   // codes per thread of gq_scores_kernel (CPT there)
  const unsigned gx = (unsigned)((n + 256 * cpt - 1) / (256 * cpt));
  const unsigned gy = (unsigned)((rows + 16 - 1) / 16);
  if (gy > 65535u * 32u) return GQHIP_ERR_INVALID_ARG;
  if (const auto pair = scores_pair_kernel(dim, beta == 1.0))
    return launch(pair, dim3(gx, gy), dim3(256), 0, st, mu, sd, cb, out, (int)rows, (int)n, beta);
  return launch(gq_scores_generic_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)rows), dim3(256), 0, st, mu, sd, cb, out,
                (int)dim, (int)rows, (int)n, beta);
}

int gq_argmax_f32(const float *mu, const float *sd, const float *logsd_or_null, const float *cb,
                  int64_t *idx, float *zhat_or_null, int64_t dim, int64_t rows, int64_t n, double beta,
                  void *workspace, int64_t workspace_bytes, void *cb_cache_or_null, int64_t cb_cache_bytes, void *stream) {
  OutMap om{};
  om.mode = 0; om.K = 1; om.L = 1; om.c = (int)dim;
  return run_argmax<kModeGQ>(PrepInput{}, mu, sd, logsd_or_null, cb, idx, zhat_or_null, dim, rows, n, beta,
                             workspace, workspace_bytes, cb_cache_or_null, cb_cache_bytes, om, static_cast<hipStream_t>(stream));
}

int gq_quantize_z_f32(const float *z, const float *noise_or_null, const float *cb, int64_t *idx,
                      float *zhat_or_null, float *zhat_noquant_or_null, float *mu_out_or_null,
                      float *sd_out_or_null, int64_t B, int64_t L, int64_t c, int64_t dim, int64_t n, int layout,
                      int grouping, double lv_min, double lv_max, double beta, void *workspace,
                      int64_t workspace_bytes, void *cb_cache_or_null, int64_t cb_cache_bytes, void *stream) {
  ZGeom g;
  if (!z || !cb || !idx || !z_geometry(B, L, c, dim, layout, grouping, &g)) return GQHIP_ERR_INVALID_ARG;
  if (zhat_noquant_or_null && !noise_or_null) return GQHIP_ERR_INVALID_ARG;
  if (g.rows == 0) return GQHIP_OK;
  if (g.rows > 0x3fffffff) return GQHIP_ERR_INVALID_ARG;
  PrepInput in;
  in.z = z; in.noise = noise_or_null; in.zhat_noquant = zhat_noquant_or_null;
  in.lv_min = (float)lv_min; in.lv_max = (float)lv_max;
  in.mu_out = mu_out_or_null; in.sd_out = sd_out_or_null;
  return run_argmax<kModeGQ>(in, nullptr, nullptr, nullptr, cb, idx, zhat_or_null, dim, g.rows, n, beta, workspace,
                             workspace_bytes, cb_cache_or_null, cb_cache_bytes, g.om, static_cast<hipStream_t>(stream));
}

int gq_quantize_z_gauss_f32(const float *z, const float *noise, const float *cb, int64_t *idx, float *zhat,
                            float *zhat_quant_or_null, float *zhat_noquant, float *sd_out_or_null, void *scalars_out, double *lam_state, int64_t B,
                            int64_t L, int64_t c, int64_t dim, int64_t n, int layout, int grouping, double lv_min,
                            double lv_max, double beta, int use_ste, double log2n, double tolerance, double lam_factor,
                            double lam_lo, double lam_hi, int lam_max_decreases, void *workspace, int64_t workspace_bytes,
                            void *cb_cache_or_null, int64_t cb_cache_bytes, void *stream) {
  ZGeom g;
  if (!z || !noise || !cb || !idx || !zhat || !zhat_noquant || !scalars_out || !lam_state ||
      !z_geometry(B, L, c, dim, layout, grouping, &g))
    return GQHIP_ERR_INVALID_ARG;
  if (!aligned(7u, scalars_out, lam_state)) return GQHIP_ERR_INVALID_ARG;
  if (g.rows == 0) return GQHIP_OK;      // (the reference's means of an empty tensor are NaN; nothing is written here)
  if (g.rows > 0x3fffffff) return GQHIP_ERR_INVALID_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  PrepInput in;
  in.z = z; in.noise = noise; in.zhat_noquant = zhat_noquant;
  in.lv_min = (float)lv_min; in.lv_max = (float)lv_max;
  in.sd_layout = sd_out_or_null; in.want_kl2 = true;
  if (use_ste) { in.ste_kind = 1; in.ste = zhat_noquant; in.pure = zhat_quant_or_null; }
  in.gs = gauss_stats_params(nullptr, g.rows, lam_state, scalars_out, log2n, tolerance, lam_factor, lam_lo, lam_hi, lam_max_decreases,
                             (double)g.rows);        // the mean of gaussian.py:241
  bool stats_done = false;
  WsLayout w{};
  in.stats_done = &stats_done; in.layout = &w;
  const int rc = run_argmax<kModeGQ>(in, nullptr, nullptr, nullptr, cb, idx, zhat, dim, g.rows, n, beta, workspace, workspace_bytes,
                                     cb_cache_or_null, cb_cache_bytes, g.om, st);
  if (rc != GQHIP_OK || stats_done) return rc;       // dims 8 / 16 / 32: the statistics block ran as one extra block of the re-rank launch
  in.gs.kl2row = reinterpret_cast<const float *>(static_cast<char *>(workspace) + w.kl2);
  return launch(gauss_stats_finalize_kernel, dim3(1), dim3(256), 0, st, in.gs);
}

// ---- the train-mode step of the Gaussian regularizers (gq_gauss_train.h) ----
namespace {
// which slab form serves this shape with 16-byte accesses (gq_gauss_train.h): 0 = one element per thread step (every shape),
// 1 = four rows wide, 2 = four g wide; `ptr_bits` = the OR of every pointer the kernel vectorises
int train_variant(int layout, int grouping, int64_t dim, int64_t K, int64_t L, uintptr_t ptr_bits, long rows, long *items) {
  const bool al = (ptr_bits & 15u) == 0;
  if (layout == GQHIP_LAYOUT_BCHW) {
    if (al && L % 4 == 0) { *items = rows / 4; return 1; }
  } else {
    if (al && (grouping == GQHIP_GROUP_CONTIGUOUS || K == 1) && dim % 4 == 0) { *items = rows; return 2; }
    if (al && grouping == GQHIP_GROUP_STRIDED && K % 4 == 0) { *items = rows / 4; return 1; }
  }
  *items = rows;
  return 0;
}
unsigned train_grid(long items) {
  const long blocks = (items + 255) / 256;
  return (unsigned)(blocks < kTrainMaxBlocks ? blocks : kTrainMaxBlocks);
}
uintptr_t bits(const void *p) { return reinterpret_cast<uintptr_t>(p); }
}  // namespace

int gq_gauss_train_f32(const float *z, const float *noise, float *zhat, float *sd_out_or_null, float *kl2row, void *scalars_out,
                       double *lam_state, int64_t B, int64_t L, int64_t c, int64_t dim, int layout, int grouping, double lv_min,
                       double lv_max, double log2n, double tolerance, double lam_factor, double lam_lo, double lam_hi,
                       int lam_max_decreases, double loss_divisor, void *stream) {
  ZGeom g;
  if (!z || !noise || !zhat || !kl2row || !scalars_out || !lam_state || !aligned(7u, scalars_out, lam_state) ||
      !z_geometry(B, L, c, dim, layout, grouping, &g))
    return GQHIP_ERR_INVALID_ARG;
  if (g.rows == 0) return GQHIP_OK;      // (the reference's means of an empty tensor are NaN; nothing is written here)
  if (g.rows > 0x3fffffff || !(loss_divisor > 0.0)) return GQHIP_ERR_INVALID_ARG;
  GaussTrainParams p{};
  p.z = z; p.noise = noise; p.zhat = zhat; p.sd_out = sd_out_or_null; p.kl2row = kl2row;
  p.lv_min = (float)lv_min; p.lv_max = (float)lv_max;
  p.dim = (int)dim; p.K = (int)g.K; p.L = (int)L; p.c = (int)c;
  p.layout = g.om.mode; p.grouping = grouping;
  const int variant = train_variant(layout, grouping, dim, g.K, L, bits(z) | bits(noise) | bits(zhat) | bits(sd_out_or_null),
                                    (long)g.rows, &p.items);
  const auto fwd = variant == 1 ? gauss_train_fwd_kernel<4, false> : variant == 2 ? gauss_train_fwd_kernel<4, true> : gauss_train_fwd_kernel<1, false>;
  return Chain(stream).run(fwd, dim3(train_grid(p.items)), dim3(256), p)       // then, on the same stream, the statistics block
      .run(gauss_stats_finalize_kernel, dim3(1), dim3(256), gauss_stats_params(kl2row, g.rows, lam_state, scalars_out, log2n, tolerance,
                                                                              lam_factor, lam_lo, lam_hi, lam_max_decreases, loss_divisor)).rc;
}

int gq_gauss_backward_f32(const float *z, const float *noise, const float *g_zhat_or_null, const float *g_sd_or_null,
                          const float *g_kl_or_null, const double *lam_before, float *grad_z, int64_t B, int64_t L, int64_t c,
                          int64_t dim, int layout, int grouping, double lv_min, double lv_max, double log2n, double tolerance,
                          double loss_divisor, void *stream) {
  ZGeom g;
  if (!z || !noise || !lam_before || !grad_z || !aligned(7u, lam_before) || !aligned(3u, g_kl_or_null) ||
      !z_geometry(B, L, c, dim, layout, grouping, &g))
    return GQHIP_ERR_INVALID_ARG;
  if (g.rows == 0) return GQHIP_OK;
  if (g.rows > 0x3fffffff || !(loss_divisor > 0.0)) return GQHIP_ERR_INVALID_ARG;
  GaussTrainParams p{};
  p.z = z; p.noise = noise; p.g_zhat = g_zhat_or_null; p.g_sd = g_sd_or_null; p.g_kl = g_kl_or_null;
  p.lam_before = lam_before; p.grad_z = grad_z; p.divisor = loss_divisor;
  p.thr_hi = (float)(log2n + tolerance); p.thr_lo = (float)(log2n - tolerance);
  p.lv_min = (float)lv_min; p.lv_max = (float)lv_max;
  p.dim = (int)dim; p.K = (int)g.K; p.L = (int)L; p.c = (int)c;
  p.layout = g.om.mode; p.grouping = grouping;
  const int variant = train_variant(layout, grouping, dim, g.K, L,
                                    bits(z) | bits(noise) | bits(g_zhat_or_null) | bits(g_sd_or_null) | bits(grad_z), (long)g.rows, &p.items);
  const auto bwd = variant == 1 ? gauss_train_bwd_kernel<4, false> : variant == 2 ? gauss_train_bwd_kernel<4, true> : gauss_train_bwd_kernel<1, false>;
  return launch(bwd, dim3(train_grid(p.items)), dim3(256), 0, static_cast<hipStream_t>(stream), p);
}

int vq_quantize_z_f32(const float *z, const float *emb, int64_t *idx, float *zq, float *loss2_or_null, int64_t B, int64_t L,
                      int64_t c, int64_t dim, int64_t n, int layout, double beta, int legacy, void *workspace,
                      int64_t workspace_bytes, void *cb_cache_or_null, int64_t cb_cache_bytes, void *stream) {
  ZGeom g;                                                                            // channel = d * K + k (vq.py:53): strided
  if (!z || !emb || !idx || !zq || !z_geometry(B, L, c, dim, layout, GQHIP_GROUP_STRIDED, &g)) return GQHIP_ERR_INVALID_ARG;
  if (g.rows == 0) return GQHIP_OK;
  if (g.rows > 0x3fffffff) return GQHIP_ERR_INVALID_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  PrepInput in;
  WsLayout w{};
  in.z = z; in.layout = &w;
  in.ste_kind = 2; in.ste = z;                                                        // z_q = z + (z_q - z) (vq.py:89)
  const int rc = run_argmax<kModeVQ>(in, nullptr, nullptr, nullptr, emb, idx, zq, dim, g.rows, n, 0.0, workspace, workspace_bytes,
                                     cb_cache_or_null, cb_cache_bytes, g.om, st);
  if (rc != GQHIP_OK || !loss2_or_null) return rc;
  VqLossParams lp{};
  lp.zrows = reinterpret_cast<const float *>(static_cast<char *>(workspace) + w.mu);
  lp.idx = idx; lp.emb = emb; lp.loss = loss2_or_null;
  lp.hdr = reinterpret_cast<WsHeader *>(static_cast<char *>(workspace) + w.hdr);
  lp.rows = (long)g.rows; lp.dim = (int)dim; lp.n = (int)n; lp.beta = (float)beta; lp.legacy = legacy; lp.omap = g.om;
  int64_t blocks = (g.rows * dim + 256 * 16 - 1) / (256 * 16);
  blocks = blocks < 1 ? 1 : (blocks > 256 ? 256 : blocks);
  return launch(vq_loss_kernel, dim3((unsigned)blocks), dim3(256), 0, st, lp);
}

// ---- the backward of VQQuantizer's train step (vq_train.h) ----
namespace {
struct VqBwdLayout {
  int64_t keys[2], vals[2], table, partial, flag, total;
  int tiles, passes;
};
static bool vq_backward_layout(int64_t items, int64_t n, int64_t dim, VqBwdLayout *w) {
  if (items < 0 || items > 0x3fffffff || n < 1 || n > 0x7fffffff || dim < 1 || dim > kMaxDim) return false;
  int bits = 0;
  while (((int64_t)1 << bits) < n) ++bits;
  w->passes = bits <= 8 ? 1 : (bits + 7) / 8;
  w->tiles = (int)((items + kVqSortTile - 1) / kVqSortTile);
  Carve ws;
  for (int i = 0; i < 2; ++i) {
    w->keys[i] = ws.take(items * 4);
    w->vals[i] = ws.take(items * 4);
  }
  w->table = ws.take((int64_t)256 * w->tiles * 4);
  w->partial = ws.take(2 * ((items + kVqChunk - 1) / kVqChunk) * dim * 8);
  w->flag = ws.take(256);
  w->total = ws.off;
  return true;
}
}  // namespace

int64_t vq_backward_workspace_bytes(int64_t items, int64_t n, int64_t dim) {
  VqBwdLayout w;
  return vq_backward_layout(items, n, dim, &w) ? w.total : -1;
}

int vq_backward_f32(const float *z, const float *emb, const int64_t *idx, const float *g_zq_or_null, const float *g_loss_or_null,
                    float *grad_z_or_null, float *grad_emb_or_null, int64_t B, int64_t L, int64_t c, int64_t dim, int64_t n,
                    int layout, double beta, int legacy, void *workspace, int64_t workspace_bytes, void *stream) {
  ZGeom g;
  VqBwdLayout w;
  if (!z || !emb || !idx || !z_geometry(B, L, c, dim, layout, GQHIP_GROUP_STRIDED, &g)) return GQHIP_ERR_INVALID_ARG;
  // the odd one among the train steps: a misaligned workspace is an invalid argument here, and is looked at before the workspace's size
  if (!vq_backward_layout(g.rows, n, dim, &w) || !aligned(3u, g_loss_or_null) || !aligned(15u, workspace)) return GQHIP_ERR_INVALID_ARG;
  Chain ch(stream);
  if (g.rows > 0 && workspace_status(workspace, workspace_bytes, w.total) != GQHIP_OK) return GQHIP_ERR_WORKSPACE;
  if (grad_emb_or_null && hipMemsetAsync(grad_emb_or_null, 0, sizeof(float) * n * dim, ch.st) != hipSuccess) return check_launch();
  if (g.rows == 0) return GQHIP_OK;
  const int last = (w.passes - 1) & 1;                           // pass i writes buffer pair i & 1
  VqBwdParams p{};
  p.z = z; p.emb = emb; p.idx = idx; p.g_zq = g_zq_or_null; p.g_loss = g_loss_or_null;
  p.grad_z = grad_z_or_null; p.grad_emb = grad_emb_or_null;
  p.keys = at<const unsigned>(workspace, w.keys[last]); p.vals = at<const unsigned>(workspace, w.vals[last]);
  p.partial = at<double>(workspace, w.partial); p.flag = at<int>(workspace, w.flag);
  p.items = (long)g.rows; p.total = (long)(B * L * c);
  p.cz = (legacy ? 1.0 : beta) * 2.0 / (double)p.total; p.ce = (legacy ? beta : 1.0) * 2.0 / (double)p.total;
  p.dim = (int)dim; p.n = (int)n; p.omap = g.om;
  if (grad_z_or_null) {
    const bool wide = ((bits(z) | bits(g_zq_or_null) | bits(grad_z_or_null)) & 15u) == 0 && (layout == GQHIP_LAYOUT_BCHW ? L : c) % 4 == 0;
    const long threads = wide ? p.total / 4 : p.total;
    ch.run(wide ? vq_grad_z_kernel<4> : vq_grad_z_kernel<1>, dim3((unsigned)((threads + 255) / 256)), dim3(256), p);
  }
  if (!grad_emb_or_null || !g_loss_or_null) return ch.rc;       // no gradient arrives at the loss: grad_emb stays the zeros above
  VqSortParams sp{};
  sp.idx = idx; sp.table = at<int>(workspace, w.table); sp.flag = p.flag;
  sp.items = p.items; sp.tiles = w.tiles; sp.n = p.n; sp.omap = g.om;
  for (int pass = 0; pass < w.passes; ++pass) {
    sp.first = pass == 0; sp.shift = 8 * pass;
    sp.keys_in = at<const unsigned>(workspace, w.keys[(pass + 1) & 1]); sp.vals_in = at<const unsigned>(workspace, w.vals[(pass + 1) & 1]);
    sp.keys_out = at<unsigned>(workspace, w.keys[pass & 1]); sp.vals_out = at<unsigned>(workspace, w.vals[pass & 1]);
    ch.run(vq_sort_count_kernel, dim3((unsigned)w.tiles), dim3(64), sp)
        .run(vq_sort_scan_kernel, dim3(1), dim3(1024), sp.table, (long)256 * w.tiles)
        .run(vq_sort_place_kernel, dim3((unsigned)w.tiles), dim3(64), sp);
  }
  const dim3 blocks((unsigned)((g.rows * dim + 255) / 256));      // rows < 2^30 and dim <= 64: at most 2^28
  return ch.run(vq_emb_sum_kernel, blocks, dim3(256), p).run(vq_emb_combine_kernel, blocks, dim3(256), p).rc;
}

// ---- LFQQuantizer's train step (lfq_train.h) ----
namespace {
struct LfqLayout {
  int64_t elem_part, part, ent_part, G, GT, total;
  int chunks, Mpad, Npad, elem_blocks, avg_blocks, wide;
};
static bool lfq_layout(int64_t rows, int64_t d, LfqLayout *w) {
  if (rows < 0 || rows > 0x3fffffff || d < 1 || d > kLfqMaxD) return false;
  const int dl = (int)d / 2, dh = (int)d - dl;
  w->wide = (1 << dl) >= 128;                                    // 128 x 128 block tiles from d = 14 on, 64 x 64 below
  const int T = w->wide ? 128 : 64;
  w->Mpad = (1 << dh) > T ? (1 << dh) : T;
  w->Npad = (1 << dl) > T ? (1 << dl) : T;
  w->chunks = (int)((rows + kLfqChunk - 1) / kLfqChunk);
  w->elem_blocks = (int)((rows + 255) / 256);                    // positions <= rows
  w->avg_blocks = (int)((((int64_t)1 << d) + 255) / 256);
  Carve ws;
  w->elem_part = ws.take((int64_t)w->elem_blocks * 16);
  w->part = ws.take((int64_t)w->chunks * w->Mpad * w->Npad * 4);
  w->ent_part = ws.take((int64_t)w->avg_blocks * 8);
  w->G = ws.take(((int64_t)4) << d);
  w->GT = ws.take(((int64_t)4) << d);
  w->total = ws.off;
  return true;
}
static bool lfq_geometry(int64_t B, int64_t L, int64_t C, int64_t nc, int64_t d, int layout, LfqGeom *g, LfqLayout *w) {
  if (nc < 1 || d < 1 || d > kLfqMaxD || nc * d > 62 || C != nc * d || !train_geometry(B, L, layout, nc, g)) return false;
  g->R = g->P * (long)nc;
  g->nc = (int)nc; g->d = (int)d; g->dl = (int)d / 2; g->dh = (int)d - g->dl; g->C = (int)C;
  return lfq_layout(g->R, d, w);
}
}  // namespace

int64_t lfq_train_workspace_bytes(int64_t rows, int64_t d) {
  LfqLayout w;
  return lfq_layout(rows, d, &w) ? w.total : -1;
}

int lfq_train_f32(const float *x, float *quantized, int64_t *idx, float *avg, float *scalars, int64_t B, int64_t L, int64_t C,
                  int64_t nc, int64_t d, int layout, float w_s, float w_b, void *workspace, int64_t workspace_bytes, void *stream) {
  LfqGeom g;
  LfqLayout w;
  if (!x || !quantized || !idx || !avg || !scalars || !lfq_geometry(B, L, C, nc, d, layout, &g, &w) || !aligned(3u, avg, scalars))
    return GQHIP_ERR_INVALID_ARG;
  if (g.R == 0) return GQHIP_OK;
  if (const int rc = workspace_status(workspace, workspace_bytes, w.total)) return rc;
  LfqFwdParams p{};
  p.x = x; p.quant = quantized; p.idx = idx; p.avg = avg; p.scalars = scalars;
  p.elem_part = at<double>(workspace, w.elem_part); p.part = at<float>(workspace, w.part); p.ent_part = at<double>(workspace, w.ent_part);
  p.g = g; p.ws = w_s; p.wb = w_b;
  p.chunks = w.chunks; p.Mpad = w.Mpad; p.Npad = w.Npad; p.avg_blocks = w.avg_blocks;
  p.elem_blocks = (int)((g.P + 255) / 256);
  const int T = w.wide ? 128 : 64;
  const dim3 grid((unsigned)w.chunks, (unsigned)((w.Mpad / T) * (w.Npad / T)));
  return Chain(stream).run(lfq_elem_kernel, dim3((unsigned)p.elem_blocks), dim3(256), p)
      .run(w.wide ? lfq_avg_gemm_kernel<2> : lfq_avg_gemm_kernel<1>, grid, dim3(256), p)
      .run(lfq_avg_reduce_kernel, dim3((unsigned)w.avg_blocks), dim3(256), p)
      .run(lfq_finish_kernel, dim3(1), dim3(256), p).rc;
}

namespace {
using LfqBwdKernel = void (*)(const LfqBwdParams);
static LfqBwdKernel lfq_bwd_choice(int dh) {
  switch (dh <= 5 ? 1 : 1 << (dh - 5)) {
    case 1: return lfq_bwd_kernel<1>;
    case 2: return lfq_bwd_kernel<2>;
    case 4: return lfq_bwd_kernel<4>;
    case 8: return lfq_bwd_kernel<8>;
  }
  return nullptr;
}
}  // namespace

int lfq_backward_f32(const float *x, const float *avg, const float *g_q_or_null, const float *g_aux_or_null,
                     const float *g_commit_or_null, float *grad_x, int64_t B, int64_t L, int64_t C, int64_t nc, int64_t d, int layout,
                     float w_s, float w_b, void *workspace, int64_t workspace_bytes, void *stream) {
  LfqGeom g;
  LfqLayout w;
  if (!x || !avg || !grad_x || !lfq_geometry(B, L, C, nc, d, layout, &g, &w) || !aligned(3u, avg, g_aux_or_null, g_commit_or_null))
    return GQHIP_ERR_INVALID_ARG;
  if (g.R == 0) return GQHIP_OK;
  if (const int rc = workspace_status(workspace, workspace_bytes, w.total)) return rc;
  LfqBwdParams p{};
  p.x = x; p.avg = avg; p.g_q = g_q_or_null; p.g_aux = g_aux_or_null; p.g_commit = g_commit_or_null; p.grad_x = grad_x;
  p.G = at<float>(workspace, w.G); p.GT = at<float>(workspace, w.GT);
  p.g = g; p.ws = w_s; p.wb = w_b;
  Chain ch(stream);
  if (g_aux_or_null) ch.run(lfq_g_kernel, dim3((unsigned)w.avg_blocks), dim3(256), p);
  const int64_t blocks = (g.R + 32 * kLfqBwdWaves - 1) / (32 * kLfqBwdWaves);
  return ch.run(lfq_bwd_choice(g.dh), dim3((unsigned)blocks), dim3(64 * kLfqBwdWaves), p).rc;
}

// ---- BSQQuantizer's train step (bsq_fsq_train.h) ----
namespace {
static int64_t bsq_part_blocks(int64_t rows) {                     // an upper bound of the forward's blocks for either layout
  const int64_t b = (rows + 15) / 16;
  return b < 1 ? 1 : (b > kBsqMaxBlocks ? kBsqMaxBlocks : b);
}
static bool bsq_geometry(int64_t B, int64_t L, int64_t C, int64_t d, int layout, BsqGeom *g) {
  if (d < 1 || d > kBsqMaxD || C != 16 * d || !train_geometry(B, L, layout, 1, g)) return false;
  g->d = (int)d; g->C = (int)C;
  const int64_t rpb = g->mode == 1 ? kBsqBchwThreads : (d == 1 ? 64 : d == 2 ? 32 : 16);      // positions a block covers per step
  const int64_t tiles = (g->P + rpb - 1) / rpb;
  g->iters = (int)((tiles + kBsqMaxBlocks - 1) / kBsqMaxBlocks);
  if (g->iters < 1) g->iters = 1;
  g->blocks = (int)((tiles + g->iters - 1) / g->iters);
  g->q_scale = (float)(1.0 / sqrt((double)C));
  g->cs = -400.0 / sqrt((double)C);
  g->M = (double)g->P * 16.0;
  return true;
}
using BsqFwdKernel = void (*)(const BsqFwdParams);
using BsqBwdKernel = void (*)(const BsqBwdParams);
// "blc": lanes per row and 16-byte chunks per lane for C = 16 d floats
static int bsq_blc_slot(int d) { return d == 1 ? 0 : d == 2 ? 1 : d <= 4 ? 2 : d <= 8 ? 3 : d <= 12 ? 4 : 5; }
static BsqFwdKernel bsq_fwd_choice(const BsqGeom &g) {
  static const BsqFwdKernel blc[6] = {bsq_fwd_blc_kernel<4, 1>,  bsq_fwd_blc_kernel<8, 1>,  bsq_fwd_blc_kernel<16, 1>,
                                      bsq_fwd_blc_kernel<16, 2>, bsq_fwd_blc_kernel<16, 3>, bsq_fwd_blc_kernel<16, 4>};
  return g.mode == 1 ? bsq_fwd_bchw_kernel : blc[bsq_blc_slot(g.d)];
}
static BsqBwdKernel bsq_bwd_choice(const BsqGeom &g) {
  static const BsqBwdKernel blc[6] = {bsq_bwd_blc_kernel<4, 1>,  bsq_bwd_blc_kernel<8, 1>,  bsq_bwd_blc_kernel<16, 1>,
                                      bsq_bwd_blc_kernel<16, 2>, bsq_bwd_blc_kernel<16, 3>, bsq_bwd_blc_kernel<16, 4>};
  return g.mode == 1 ? bsq_bwd_bchw_kernel : blc[bsq_blc_slot(g.d)];
}
}  // namespace

int64_t bsq_train_workspace_bytes(int64_t rows, int64_t d) {
  if (rows < 0 || rows > 0x3fffffff || d < 1 || d > kBsqMaxD) return -1;
  return align256(bsq_part_blocks(rows) * (2 * d + 1) * 8);       // one block (BsqFwdParams::part): nothing to carve
}

int bsq_train_f32(const float *x, float *quantized, int64_t *idx, float *avg, float *scalars, int64_t B, int64_t L, int64_t C,
                  int64_t d, int layout, float w_s, float w_b, void *workspace, int64_t workspace_bytes, void *stream) {
  BsqGeom g;
  if (!x || !quantized || !idx || !avg || !scalars || !bsq_geometry(B, L, C, d, layout, &g)) return GQHIP_ERR_INVALID_ARG;
  const unsigned amask = g.mode == 2 ? 15u : 3u;                   // "blc" rows are read and written 16 bytes at a time
  if (!aligned(amask, x, quantized) || !aligned(3u, avg, scalars) || !aligned(7u, idx)) return GQHIP_ERR_INVALID_ARG;
  if (g.P == 0) return GQHIP_OK;
  if (const int rc = workspace_status(workspace, workspace_bytes, bsq_train_workspace_bytes(g.P, d))) return rc;
  BsqFwdParams p{};
  p.x = x; p.quant = quantized; p.idx = idx; p.avg = avg; p.scalars = scalars; p.part = static_cast<double *>(workspace);
  p.g = g; p.ws = w_s; p.wb = w_b;
  return Chain(stream).run(bsq_fwd_choice(g), dim3((unsigned)g.blocks), dim3(g.mode == 1 ? kBsqBchwThreads : 256), p)
      .run(bsq_finish_kernel, dim3(1), dim3(256), p).rc;
}

int bsq_backward_f32(const float *x, const float *avg, const float *g_q_or_null, const float *g_aux_or_null, float *grad_x,
                     int64_t B, int64_t L, int64_t C, int64_t d, int layout, float w_s, float w_b, void *workspace,
                     int64_t workspace_bytes, void *stream) {
  BsqGeom g;
  if (!x || !avg || !grad_x || !bsq_geometry(B, L, C, d, layout, &g)) return GQHIP_ERR_INVALID_ARG;
  const unsigned amask = g.mode == 2 ? 15u : 3u;
  if (!aligned(amask, x, grad_x, g_q_or_null) || !aligned(3u, avg, g_aux_or_null)) return GQHIP_ERR_INVALID_ARG;
  if (g.P == 0) return GQHIP_OK;
  if (const int rc = workspace_status(workspace, workspace_bytes, bsq_train_workspace_bytes(g.P, d))) return rc;
  BsqBwdParams p{};
  p.x = x; p.avg = avg; p.g_q = g_q_or_null; p.g_aux = g_aux_or_null; p.grad_x = grad_x;
  p.g = g; p.ws = w_s; p.wb = w_b;
  const int64_t blocks = g.mode == 1 ? (g.P + kBsqBchwThreads - 1) / kBsqBchwThreads : g.blocks;
  return launch(bsq_bwd_choice(g), dim3((unsigned)blocks), dim3(g.mode == 1 ? kBsqBchwThreads : 256), 0, static_cast<hipStream_t>(stream), p);
}

// ---- the LPIPS comparison head (lpips_head.h) ----
namespace {
using LpipsKernel = void (*)(const LpipsParams);
// the kernel of a call and its tile: `wide` = every feature pointer (and w, for "blc") is 16-byte aligned and the keep mask 4-byte
extern "C++" template <bool BWD>
LpipsKernel lpips_choice(LpipsGeom *g, bool wide) {
  if (g->mode == 1) {
    const bool v4 = wide && g->L % 4 == 0 && g->C <= 256;
    g->T = v4 ? 64 : 16;
    return !v4           ? lpips_bchw_kernel<BWD, 1, 32>
           : g->C <= 64  ? lpips_bchw_kernel<BWD, 4, 4>
           : g->C <= 128 ? lpips_bchw_kernel<BWD, 4, 8>
                         : lpips_bchw_kernel<BWD, 4, 16>;
  }
  if (wide && g->C % 4 == 0) {
    const int u = g->C / 4;
    g->T = u <= 16 ? 64 : 16;
    return u <= 4    ? lpips_blc_kernel<BWD, 4, 1, 4>
           : u <= 8  ? lpips_blc_kernel<BWD, 8, 1, 4>
           : u <= 16 ? lpips_blc_kernel<BWD, 16, 1, 4>
           : u <= 32 ? lpips_blc_kernel<BWD, 32, 1, 4>
           : u <= 64 ? lpips_blc_kernel<BWD, 64, 1, 4>
                     : lpips_blc_kernel<BWD, 64, 2, 4>;
  }
  g->T = 16;
  return g->C <= 64    ? lpips_blc_kernel<BWD, 64, 1, 1>
         : g->C <= 128 ? lpips_blc_kernel<BWD, 64, 2, 1>
         : g->C <= 256 ? lpips_blc_kernel<BWD, 64, 4, 1>
                       : lpips_blc_kernel<BWD, 64, 8, 1>;
}
bool lpips_geometry(int64_t B, int64_t C, int64_t HW, int layout, LpipsGeom *g) {
  if (C < 1 || C > kLpipsMaxC || HW < 1 || !train_geometry(B, HW, layout, 1, g)) return false;
  g->C = (int)C;
  return true;
}
int64_t lpips_part_bytes(int64_t B, int64_t HW, int64_t T) { return ((B * HW + T - 1) / T) * lpips_slots(B, HW, T) * 8; }
}  // namespace

// either tile size a call may pick (16, 64): the larger of the two partial-sum tables
int64_t lpips_head_workspace_bytes(int64_t B, int64_t C, int64_t HW) {
  LpipsGeom g;
  if (!lpips_geometry(B, C, HW, GQHIP_LAYOUT_BCHW, &g)) return -1;
  const int64_t a = lpips_part_bytes(B, HW, 16), b = lpips_part_bytes(B, HW, 64);
  return align256(a > b ? a : b);
}

int lpips_head_f32(const float *f0, const float *f1, const float *w, const uint8_t *keep_or_null, float keep_scale, float *out,
                   int64_t B, int64_t C, int64_t HW, int layout, void *workspace, int64_t workspace_bytes, void *stream) {
  LpipsParams p{};
  LpipsGeom &g = p.g_;
  if (!f0 || !f1 || !w || !out || !lpips_geometry(B, C, HW, layout, &g) || !aligned(3u, f0, f1, w, out)) return GQHIP_ERR_INVALID_ARG;
  if (g.P == 0) return GQHIP_OK;
  if (const int rc = workspace_status(workspace, workspace_bytes, lpips_head_workspace_bytes(B, C, HW))) return rc;
  const LpipsKernel kernel = lpips_choice<false>(&g, aligned(15u, f0, f1) && aligned(g.mode == 2 ? 15u : 3u, w) && aligned(3u, keep_or_null));
  g.slots = (int)lpips_slots(B, HW, g.T);
  p.f0 = f0; p.f1 = f1; p.w = w; p.keep = keep_or_null; p.keep_scale = keep_scale;
  p.part = static_cast<double *>(workspace); p.out = out;
  return Chain(stream).run(kernel, dim3((unsigned)((g.P + g.T - 1) / g.T)), dim3(256), p)
      .run(lpips_finish_kernel, dim3((unsigned)B), dim3(256), p).rc;
}

int lpips_head_backward_f32(const float *f0, const float *f1, const float *w, const uint8_t *keep_or_null, float keep_scale,
                            const float *g_out, float *grad_f1, int64_t B, int64_t C, int64_t HW, int layout, void *stream) {
  LpipsParams p{};
  LpipsGeom &g = p.g_;
  if (!f0 || !f1 || !w || !g_out || !grad_f1 || !lpips_geometry(B, C, HW, layout, &g) || !aligned(3u, f0, f1, w, g_out, grad_f1))
    return GQHIP_ERR_INVALID_ARG;
  if (g.P == 0) return GQHIP_OK;
  const LpipsKernel kernel =
      lpips_choice<true>(&g, aligned(15u, f0, f1, grad_f1) && aligned(g.mode == 2 ? 15u : 3u, w) && aligned(3u, keep_or_null));
  g.slots = (int)lpips_slots(B, HW, g.T);
  p.f0 = f0; p.f1 = f1; p.w = w; p.keep = keep_or_null; p.keep_scale = keep_scale; p.g = g_out; p.grad = grad_f1;
  return launch(kernel, dim3((unsigned)((g.P + g.T - 1) / g.T)), dim3(256), 0, static_cast<hipStream_t>(stream), p);
}

// ---- raw feature moments in fp64 (gq_moments.h) ----
int64_t gq_moments_state_bytes(int64_t D) { return D < 1 || D > kMomMaxD ? -1 : (D * D + D + 1) * 8; }

int gq_moments_update_f32(const float *x, int64_t rows, int64_t D, int64_t row_stride, double *state, void *stream) {
  if (!x || !state || D < 1 || D > kMomMaxD || rows < 0 || row_stride < D || !aligned(3u, x) || !aligned(7u, state))
    return GQHIP_ERR_INVALID_ARG;
  if (row_stride > 0x7fffffffL || rows * row_stride > 0x7fffffffL) return GQHIP_ERR_INVALID_ARG;   // each factor < 2^31: no overflow
  if (rows == 0) return GQHIP_OK;
  MomentsParams p{};
  p.x = x; p.state = state; p.rows = (int)rows; p.D = (int)D; p.stride = (int)row_stride;
  p.T = (int)((D + kMomTile - 1) / kMomTile);
  p.vec_x = aligned(15u, x) && row_stride % 4 == 0;
  p.wide_state = aligned(15u, state) && D % 2 == 0;
  return launch(moments_update_kernel, dim3((unsigned)(p.T * (p.T + 1) / 2)), dim3(256), 0, static_cast<hipStream_t>(stream), p);
}

int gq_dequant_f32(const int64_t *idx, const float *cb, float *zhat, int64_t B, int64_t L, int64_t K,
                   int64_t dim, int64_t n, int layout, int grouping, void *stream) {
  ZGeom g;
  if (!idx || !cb || !zhat || K < 1 || n < 1 || !z_geometry(B, L, K * dim, dim, layout, grouping, &g, /*strict=*/false))
    return GQHIP_ERR_INVALID_ARG;
  if (g.rows == 0) return GQHIP_OK;
  DequantParams dp{};
  dp.idx = idx; dp.cb = cb; dp.zhat = zhat; dp.rows = g.rows; dp.dim = (int)dim; dp.n = (int)n; dp.omap = g.om;
  return launch(dequant_kernel, dim3((unsigned)((g.rows * dim + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), dp);
}

int vq_argmin_f32(const float *z, const float *emb, int64_t *idx, float *zq_or_null, int64_t dim,
                  int64_t rows, int64_t n, void *workspace, int64_t workspace_bytes, void *cb_cache_or_null,
                  int64_t cb_cache_bytes, void *stream) {
  OutMap om{};
  om.mode = 0; om.K = 1; om.L = 1; om.c = (int)dim;
  return run_argmax<kModeVQ>(PrepInput{}, z, nullptr, nullptr, emb, idx, zq_or_null, dim, rows, n, 0.0, workspace,
                             workspace_bytes, cb_cache_or_null, cb_cache_bytes, om, static_cast<hipStream_t>(stream));
}

int lfq_pack_f32(const float *x, int64_t *idx, float *q_or_null, int64_t rows, int64_t nbits,
                 void *stream) {
  if (!x || !idx || rows < 0 || nbits < 1 || nbits > 62) return GQHIP_ERR_INVALID_ARG;
  if (rows == 0) return GQHIP_OK;
  return launch(lfq_pack_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0,
                static_cast<hipStream_t>(stream), x, idx, q_or_null, (long)rows, (int)nbits);
}

int lfq_unpack_f32(const int64_t *idx, float *q, int64_t rows, int64_t nbits, void *stream) {
  if (!idx || !q || rows < 0 || nbits < 1 || nbits > 62) return GQHIP_ERR_INVALID_ARG;
  if (rows == 0) return GQHIP_OK;
  return launch(lfq_unpack_kernel, dim3((unsigned)((rows * nbits + 255) / 256)), dim3(256), 0,
                static_cast<hipStream_t>(stream), idx, q, (long)rows, (int)nbits);
}

static int fsq_levels(const int32_t *levels_host, int64_t nlev, FsqLevels *L) {
  if (!levels_host || nlev < 1 || nlev > 16) return GQHIP_ERR_INVALID_ARG;
  L->n = (int)nlev;
  long prod = 1;
  for (int i = 0; i < 16; ++i) L->lev[i] = 1;
  for (int i = 0; i < nlev; ++i) {
    if (levels_host[i] < 2) return GQHIP_ERR_INVALID_ARG;
    L->lev[i] = levels_host[i];
    prod *= levels_host[i];
    if (prod > 0x7fffffffL) return GQHIP_ERR_INVALID_ARG;   // the packed index is an int32
  }
  return GQHIP_OK;
}

int fsq_quantize_f32(const float *z, const int32_t *levels_host, int64_t nlev, float *zhat, int32_t *idx,
                     int64_t rows, void *stream) {
  FsqLevels L;
  if (!z || !idx || rows < 0 || fsq_levels(levels_host, nlev, &L) != GQHIP_OK) return GQHIP_ERR_INVALID_ARG;
  if (rows == 0) return GQHIP_OK;
  return launch(fsq_quantize_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0,
                static_cast<hipStream_t>(stream), z, L, zhat, idx, (long)rows);
}

int fsq_dequant_f32(const int32_t *idx, const int32_t *levels_host, int64_t nlev, float *zhat, int64_t rows,
                    void *stream) {
  FsqLevels L;
  if (!idx || !zhat || rows < 0 || fsq_levels(levels_host, nlev, &L) != GQHIP_OK) return GQHIP_ERR_INVALID_ARG;
  if (rows == 0) return GQHIP_OK;
  return launch(fsq_dequant_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0,
                static_cast<hipStream_t>(stream), idx, L, zhat, (long)rows);
}

// ---- FSQQuantizer's train step (bsq_fsq_train.h) ----
int fsq_train_f32(const float *z, const int32_t *levels_host, int64_t nlev, float *zhat, int32_t *idx, int64_t B, int64_t L,
                  int layout, void *stream) {
  FsqTrainParams p{};
  if (!z || !zhat || !idx || !aligned(3u, z, zhat, idx) || !train_geometry(B, L, layout, 1, &p) || fsq_levels(levels_host, nlev, &p.lv) != GQHIP_OK)
    return GQHIP_ERR_INVALID_ARG;
  if (p.P == 0) return GQHIP_OK;
  p.z = z; p.out = zhat; p.idx = idx;
  return launch(fsq_train_kernel, dim3((unsigned)((p.P + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), p);
}

int fsq_backward_f32(const float *z, const float *g_zhat, const int32_t *levels_host, int64_t nlev, float *grad_z, int64_t B,
                     int64_t L, int layout, void *stream) {
  FsqTrainParams p{};
  if (!z || !g_zhat || !grad_z || !aligned(3u, z, g_zhat, grad_z) || !train_geometry(B, L, layout, 1, &p) || fsq_levels(levels_host, nlev, &p.lv) != GQHIP_OK)
    return GQHIP_ERR_INVALID_ARG;
  if (p.P == 0) return GQHIP_OK;
  p.z = z; p.g_zhat = g_zhat; p.out = grad_z;
  const int64_t blocks = (p.P * p.lv.n + 255) / 256;              // P < 2^30 and at most 16 levels: at most 2^26
  return launch(fsq_backward_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), p);
}

int gq_index_histogram(const int64_t *idx, int64_t count, int64_t n, int32_t *hist, void *stream) {
  if (!idx || !hist || count < 0 || n < 1) return GQHIP_ERR_INVALID_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(hist, 0, sizeof(int32_t) * n, st) != hipSuccess) return check_launch();
  if (count == 0) return GQHIP_OK;
  int blocks = (int)((count + 255) / 256);
  blocks = blocks > 2048 ? 2048 : blocks;
  return launch(hist_kernel, dim3(blocks), dim3(256), 0, st, idx, (long)count, (int)n, hist);
}

int gq_indices_to_u16(const int64_t *idx, uint16_t *out, int64_t count, void *stream) {
  if (!idx || !out || count < 0) return GQHIP_ERR_INVALID_ARG;
  if (count == 0) return GQHIP_OK;
  return launch(to_u16_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0,
                static_cast<hipStream_t>(stream), idx, out, (long)count);
}

int gq_indices_from_u16(const uint16_t *in, int64_t *idx, int64_t count, void *stream) {
  if (!in || !idx || count < 0) return GQHIP_ERR_INVALID_ARG;
  if (count == 0) return GQHIP_OK;
  return launch(from_u16_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0,
                static_cast<hipStream_t>(stream), in, idx, (long)count);
}

// ---- the bit-packed index wire format (csrc/gq_aux.h) ----------------------------------------------------------------------------
namespace {
// 1 <= index_bits <= 32 and 1 <= n_codes <= 2^index_bits: every in-range index survives the packing
bool bits_args_ok(int index_bits, int64_t n_codes) {
  return index_bits >= 1 && index_bits <= 32 && n_codes >= 1 && n_codes <= ((int64_t)1 << index_bits);
}
// the stream of `count` indices in words; -1 when the bit count leaves int64 or the block count leaves the grid
int64_t bits_words(int64_t count, int index_bits) {
  if (count < 0 || count > (INT64_MAX - 8192) / 32) return -1;
  const int64_t words = (count * index_bits + 31) / 32;
  return (words + 255) / 256 > 0x3fffffff ? -1 : words;
}
PackBitsParams pack_bits_params(const int64_t *idx, int32_t *words, int64_t count, int64_t n_words, int index_bits, int64_t n_codes) {
  PackBitsParams k{};
  k.idx = idx; k.words = words; k.n_idx = (long)count; k.n_words = (long)n_words; k.n_codes = n_codes; k.w = index_bits;
  return k;
}
// the records argument of the unpack / histogram entry points: n_records fields of `count` indices at records + r stride + offset
bool packed_fields_ok(const void *records, int64_t n_records, int64_t stride_words, int64_t offset_words, int64_t count,
                      int index_bits) {
  if (!records || n_records < 0 || count < 0 || index_bits < 1 || index_bits > 32 || offset_words < 0) return false;
  const int64_t words = bits_words(count, index_bits);
  if (words < 0 || stride_words < 0 || stride_words - offset_words < words) return false;
  return n_records == 0 || count == 0 || n_records <= INT64_MAX / count;
}
}  // namespace

int gq_indices_pack_bits(const int64_t *idx, int32_t *words, int64_t count, int index_bits, int64_t n_codes,
                         int32_t *violations_or_null, void *stream) {
  const int64_t n_words = bits_words(count, index_bits);
  if (!bits_args_ok(index_bits, n_codes) || n_words < 0 || (count > 0 && (!idx || !words))) return GQHIP_ERR_INVALID_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (violations_or_null && hipMemsetAsync(violations_or_null, 0, sizeof(int32_t), st) != hipSuccess) return check_launch();
  if (count == 0) return GQHIP_OK;
  return launch(pack_bits_kernel, dim3((unsigned)((n_words + 255) / 256)), dim3(256), 0, st,
                pack_bits_params(idx, words, count, n_words, index_bits, n_codes), violations_or_null);
}

int gq_indices_unpack_bits(const int32_t *records, int64_t *idx, int64_t n_records, int64_t stride_words, int64_t offset_words,
                           int64_t count, int index_bits, void *stream) {
  if (!packed_fields_ok(records, n_records, stride_words, offset_words, count, index_bits) || !idx) return GQHIP_ERR_INVALID_ARG;
  const int64_t total = n_records * count;
  if (total == 0) return GQHIP_OK;
  const int64_t blocks = (total + 255) / 256;
  return launch(unpack_bits_kernel, dim3((unsigned)(blocks > 2048 ? 2048 : blocks)), dim3(256), 0, static_cast<hipStream_t>(stream),
                records, idx, (long)n_records, (long)stride_words, (long)offset_words, (long)count, index_bits);
}

int gq_index_histogram_packed(const int32_t *records, int64_t n_records, int64_t stride_words, int64_t offset_words, int64_t count,
                              int index_bits, int64_t n, int64_t *hist, void *stream) {
  if (!packed_fields_ok(records, n_records, stride_words, offset_words, count, index_bits) || !hist || n < 1)
    return GQHIP_ERR_INVALID_ARG;
  const int64_t total = n_records * count;
  if (total == 0) return GQHIP_OK;
  const int64_t blocks = (total + 255) / 256;
  return launch(hist_packed_kernel, dim3((unsigned)(blocks > 2048 ? 2048 : blocks)), dim3(256), 0, static_cast<hipStream_t>(stream),
                records, (long)n_records, (long)stride_words, (long)offset_words, (long)count, index_bits, n,
                reinterpret_cast<unsigned long long *>(hist));
}

// ---- SSIM / MS-SSIM (csrc/gq_ssim.h) ---------------------------------------------------------------------------------------------
namespace {
constexpr int64_t kSsimMsMin = 256;          // pit/evaluations/ssim.py:31-34: MS-SSIM only when both sides are >= 256

struct SsimPlan {
  gqssim::Level lv[gqssim::kLevels];
  int levels;                                // 5 when MS-SSIM is defined for the size, else 1
  int64_t part_doubles, p1_doubles, p2_doubles, ticket_bytes, bytes;
};

bool ssim_plan(int64_t B, int64_t C, int64_t H, int64_t W, SsimPlan &pl) {
  if (B < 1 || C < 1 || H < 1 || W < 1 || B > 0x3fffffff || H > 0x3fffffff || W > 0x3fffffff) return false;
  pl = SsimPlan{};
  pl.levels = (H >= kSsimMsMin && W >= kSsimMsMin) ? gqssim::kLevels : 1;
  int64_t h = H, w = W, part = 0;
  for (int l = 0; l < pl.levels; ++l) {
    gqssim::Level &L = pl.lv[l];
    L.H = (int)h; L.W = (int)w;
    L.Ho = (int)(h >= gqssim::kWin ? h - gqssim::kWin + 1 : h);
    L.Wo = (int)(w >= gqssim::kWin ? w - gqssim::kWin + 1 : w);
    L.tiles_y = (L.Ho + gqssim::kTH - 1) / gqssim::kTH;
    L.tiles_x = (L.Wo + gqssim::kTW - 1) / gqssim::kTW;
    L.part = (long)part;
    const int64_t blocks = B * C * L.tiles_x * L.tiles_y;
    if (blocks > 0x3fffffff) return false;
    part += blocks;                            // tile records of two doubles
    h = (h + 1) / 2;                           // avg_pool2d(2, 2, padding = side % 2): floor(s / 2) + s % 2
    w = (w + 1) / 2;
  }
  pl.part_doubles = 2 * part;
  pl.p1_doubles = pl.levels > 1 ? 2 * B * C * (int64_t)pl.lv[1].H * pl.lv[1].W : 0;
  pl.p2_doubles = pl.levels > 2 ? 2 * B * C * (int64_t)pl.lv[2].H * pl.lv[2].W : 0;
  pl.ticket_bytes = ((B * 4 + 255) / 256) * 256;
  pl.bytes = pl.ticket_bytes + 8 * (pl.part_doubles + pl.p1_doubles + pl.p2_doubles);
  return true;
}

// pytorch_msssim's window: exp(-(k - 5)^2 / (2 sigma^2)) in fp32, divided by its (fp32, left-to-right) sum.
void ssim_window(float *g) {
  float sum = 0.0f;
  for (int k = 0; k < gqssim::kWin; ++k) {
    const float d = (float)(k - gqssim::kWin / 2);
    g[k] = expf(-(d * d) / 4.5f);
    sum += g[k];
  }
  for (int k = 0; k < gqssim::kWin; ++k) g[k] /= sum;
}

int ssim_launch(const float *x, const float *y, int64_t B, int64_t C, int layout, int zero_mean, float *ssim_out, float *ms_out,
                long out_stride, const SsimPlan &pl, void *ws, hipStream_t st) {
  gqssim::Params p{};
  p.x = x; p.y = y;
  p.ssim_out = ssim_out; p.ms_out = ms_out; p.out_stride = out_stride;
  ssim_window(p.win);
  for (int l = 0; l < pl.levels; ++l) p.lv[l] = pl.lv[l];
  p.B = (int)B; p.C = (int)C; p.layout = layout; p.zero_mean = zero_mean ? 1 : 0;
  const int levels = ms_out ? pl.levels : 1;
  p.final_level = levels - 1;
  p.nan_ms = ms_out && pl.levels == 1;
  char *base = static_cast<char *>(ws);
  p.ticket = reinterpret_cast<int *>(base);
  p.partial = reinterpret_cast<double *>(base + pl.ticket_bytes);
  double *p1 = p.partial + pl.part_doubles, *p2 = p1 + pl.p1_doubles;
  const int64_t n1 = pl.p1_doubles / 2, n2 = pl.p2_doubles / 2;
  for (int l = 0; l < levels; ++l) {
    const gqssim::Level &L = pl.lv[l];
    p.level = l;
    // level 1 / 3 read P1, level 2 / 4 read P2; each level pools into the other buffer
    p.px = l == 0 ? nullptr : (l & 1) ? p1 : p2;
    p.py = l == 0 ? nullptr : (l & 1) ? p1 + n1 : p2 + n2;
    p.qx = l + 1 < levels ? ((l & 1) ? p2 : p1) : nullptr;
    p.qy = l + 1 < levels ? ((l & 1) ? p2 + n2 : p1 + n1) : nullptr;
    p.ssim_blocks = (int)(B * C * L.tiles_x * L.tiles_y);
    int64_t blocks = p.ssim_blocks;
    if (p.qx) blocks += (B * C * (int64_t)pl.lv[l + 1].H * pl.lv[l + 1].W + 255) / 256;
    if (blocks > 0x7fffffff) return GQHIP_ERR_INVALID_ARG;
    const bool fh = L.H >= gqssim::kWin, fw = L.W >= gqssim::kWin;
    const dim3 grid((unsigned)blocks);
    const auto level = fh ? (fw ? gqssim::ssim_level_kernel<true, true> : gqssim::ssim_level_kernel<true, false>)
                          : (fw ? gqssim::ssim_level_kernel<false, true> : gqssim::ssim_level_kernel<false, false>);
    const int rc = launch(level, grid, dim3(256), 0, st, p);
    if (rc != GQHIP_OK) return rc;
  }
  if (levels > 1) {
    // the pooled planes are the only words still set (tickets and tile records are zeroed by the block that finishes an image): one
    // fill, and the workspace is all zero for whatever shape the next call lays out in it (p1 | p2 are adjacent, an even count)
    const int64_t pairs = (pl.p1_doubles + pl.p2_doubles) / 2;
    const int64_t blocks = (pairs + 255) / 256;
    return launch(gqssim::ssim_zero_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, st,
                  reinterpret_cast<double2 *>(p1), (long)pairs);
  }
  return GQHIP_OK;
}
}  // namespace

int64_t gq_ssim_workspace_bytes(int64_t B, int64_t C, int64_t H, int64_t W) {
  SsimPlan pl;
  return ssim_plan(B, C, H, W, pl) ? pl.bytes : -1;
}

int gq_ssim_f32(const float *x, const float *x_rec, int64_t B, int64_t C, int64_t H, int64_t W, int layout, int zero_mean,
                float *ssim_out_or_null, float *msssim_out_or_null, void *workspace_zeroed, int64_t workspace_bytes, void *stream) {
  SsimPlan pl;
  if (!ssim_plan(B, C, H, W, pl) || (layout != 0 && layout != 1) || !x || !x_rec) return GQHIP_ERR_INVALID_ARG;
  if (!ssim_out_or_null && !msssim_out_or_null) return GQHIP_OK;
  if (!workspace_zeroed || workspace_bytes < pl.bytes) return GQHIP_ERR_WORKSPACE;
  return ssim_launch(x, x_rec, B, C, layout, zero_mean, ssim_out_or_null, msssim_out_or_null, 1, pl, workspace_zeroed,
                     static_cast<hipStream_t>(stream));
}

// ---- one rank's per-step record (csrc/gq_aux.h: step_record_kernel / step_record_bits_kernel; csrc/gq_ssim.h) -------------------
namespace {
// One description of a record call.  rec = [ B x stride metric words | index words | bits: 1 violations word ]: stride 1 (PSNR) or 3
// (PSNR, SSIM, MS-SSIM), the index words uint16 pairs or (`bits`) the index_bits-wide stream.
struct RecordPlan {
  int status;                 // of the checks that come before the pointers are looked at
  bool nothing;               // the call returns OK before it looks at a pointer
  bool need_ws;               // the call wants `bytes` of zeroed workspace
  bool grid_ok;               // the block counts fit the kernels' fields (checked after the workspace, as it always was)
  bool bits;
  int stride, index_bits, layout, chunks, psnr_blocks, pack_blocks;
  int64_t B, C, per_image, n_idx, n_codes, n_words;
  // the workspace, all zero between calls: B x chunks fp64 PSNR partials at 0, B int32 tickets (padded to 8 bytes) at off_ticket,
  // bits only: the 64-bit violations count | ticket at off_viol, stride 3 only: the SSIM workspace at off_ssim (a multiple of 256)
  int64_t off_ticket, off_viol, off_ssim, bytes;          // bytes: -1 for a shape the size functions refuse
  SsimPlan ssim;              // stride 3
};

// Stride 1 takes the image as (C, H, W) = (per_image, 1, 1).  The size functions pass n_idx = 0 and any valid index format: `bytes`
// depends on neither, nor on anything checked after it is set.
RecordPlan record_plan(int stride, bool bits, int64_t B, int64_t C, int64_t H, int64_t W, int layout, int64_t n_idx, int index_bits,
                       int64_t n_codes) {
  RecordPlan pl{};
  pl.status = GQHIP_ERR_INVALID_ARG; pl.bytes = -1;
  pl.stride = stride; pl.bits = bits; pl.index_bits = index_bits; pl.layout = layout;
  pl.B = B; pl.C = C; pl.n_idx = n_idx; pl.n_codes = n_codes;
  // the shape; three metrics refuse B < 1 (and sides or block counts beyond 2^30) through ssim_plan
  if (stride == 3 ? !ssim_plan(B, C, H, W, pl.ssim) : (B < 0 || C < 1)) return pl;
  pl.per_image = C * H * W;
  const int64_t chunks = (pl.per_image + kPsnrChunk - 1) / kPsnrChunk;
  pl.off_ticket = B * chunks * 8;
  pl.off_viol = pl.off_ticket + ((B * 4 + 7) / 8) * 8;
  pl.off_ssim = ((pl.off_viol + (bits ? 8 : 0) + 255) / 256) * 256;
  pl.bytes = stride == 3 ? pl.off_ssim + pl.ssim.bytes : pl.off_viol + (bits ? 8 : 0);
  // the arguments
  if (B > 0x3fffffff || n_idx < 0 || (stride == 3 && layout != 0 && layout != 1) || (bits && !bits_args_ok(index_bits, n_codes))) return pl;
  pl.status = GQHIP_OK;
  pl.nothing = !bits && stride == 1 && B == 0 && n_idx == 0;     // the bit-packed record still writes its violations word ...
  pl.need_ws = bits || B > 0;                                    // ... through the workspace; the uint16 one needs it for PSNR only
  // the grid: B x chunks PSNR blocks and the packing blocks of 256 words; bits_words bounds the stream (-1)
  pl.n_words = bits ? bits_words(n_idx, index_bits) : (n_idx + 1) / 2;
  if (B * chunks > 0x3fffffff || pl.n_words < 0) return pl;
  pl.chunks = (int)chunks; pl.psnr_blocks = (int)(B * chunks);
  pl.pack_blocks = bits && pl.n_words == 0 ? 1 : (int)((pl.n_words + 255) / 256);
  // the ticket field of the violations word: pack_blocks < 2^24
  pl.grid_ok = !bits || (pl.n_words <= ((int64_t)1 << 31) && (int64_t)pl.pack_blocks + pl.psnr_blocks <= 0x7fffffff);
  return pl;
}

// The pointer and workspace checks of every record entry point, then step_record_kernel or step_record_bits_kernel and, for three
// metrics, the SSIM launches into rec + 1 / rec + 2 at stride 3.
int record_launch(const RecordPlan &pl, const float *x, const float *x_rec, const int64_t *idx, int32_t *rec, void *ws, int64_t ws_bytes,
                  void *stream) {
  if (pl.status != GQHIP_OK || pl.nothing) return pl.status;
  if (!rec || (pl.B > 0 && (!x || !x_rec)) || (pl.n_idx > 0 && !idx)) return GQHIP_ERR_INVALID_ARG;
  if (pl.need_ws && (!ws || ws_bytes < pl.bytes)) return GQHIP_ERR_WORKSPACE;
  if (!pl.grid_ok) return GQHIP_ERR_INVALID_ARG;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  char *base = static_cast<char *>(ws);
  StepRecordBitsParams p{};
  StepRecordParams &r = p.r;
  r.x = x; r.x_rec = x_rec; r.idx = idx; r.rec = rec;
  r.per_image = (long)pl.per_image; r.n_idx = (long)pl.n_idx; r.B = (int)pl.B; r.stride = pl.stride;
  r.chunks = pl.chunks; r.psnr_blocks = pl.psnr_blocks;
  r.partial = reinterpret_cast<double *>(base);
  r.ticket = reinterpret_cast<int *>(base + pl.off_ticket);
  p.viol = reinterpret_cast<unsigned long long *>(base + pl.off_viol);         // p.viol, p.k, p.pack_blocks: the bit-packed kernel's
  p.k = pack_bits_params(idx, rec + pl.B * pl.stride, pl.n_idx, pl.n_words, pl.index_bits, pl.n_codes);
  p.pack_blocks = pl.pack_blocks;
  const dim3 grid((unsigned)((int64_t)pl.psnr_blocks + pl.pack_blocks));
  const int rc = pl.bits ? launch(step_record_bits_kernel, grid, dim3(256), 0, st, p) : launch(step_record_kernel, grid, dim3(256), 0, st, r);
  if (rc != GQHIP_OK || pl.stride != 3) return rc;
  return ssim_launch(x, x_rec, pl.B, pl.C, pl.layout, 1, reinterpret_cast<float *>(rec + 1), reinterpret_cast<float *>(rec + 2), 3,
                     pl.ssim, base + pl.off_ssim, st);
}
}  // namespace

int64_t gq_step_record_workspace_bytes(int64_t B, int64_t per_image) { return record_plan(1, false, B, per_image, 1, 1, 0, 0, 0, 0).bytes; }
int64_t gq_step_record_bits_workspace_bytes(int64_t B, int64_t per_image) { return record_plan(1, true, B, per_image, 1, 1, 0, 0, 1, 1).bytes; }
int64_t gq_step_record_ssim_workspace_bytes(int64_t B, int64_t C, int64_t H, int64_t W) { return record_plan(3, false, B, C, H, W, 0, 0, 0, 0).bytes; }
int64_t gq_step_record_ssim_bits_workspace_bytes(int64_t B, int64_t C, int64_t H, int64_t W) { return record_plan(3, true, B, C, H, W, 0, 0, 1, 1).bytes; }

int gq_step_record_f32(const float *x, const float *x_rec, const int64_t *idx, int32_t *rec, int64_t B, int64_t per_image,
                       int64_t n_idx, void *workspace_zeroed, int64_t workspace_bytes, void *stream) {
  return record_launch(record_plan(1, false, B, per_image, 1, 1, 0, n_idx, 0, 0), x, x_rec, idx, rec, workspace_zeroed, workspace_bytes, stream);
}

int gq_step_record_bits_f32(const float *x, const float *x_rec, const int64_t *idx, int32_t *rec, int64_t B, int64_t per_image,
                            int64_t n_idx, int index_bits, int64_t n_codes, void *workspace_zeroed, int64_t workspace_bytes,
                            void *stream) {
  return record_launch(record_plan(1, true, B, per_image, 1, 1, 0, n_idx, index_bits, n_codes), x, x_rec, idx, rec, workspace_zeroed, workspace_bytes, stream);
}

int gq_step_record_ssim_f32(const float *x, const float *x_rec, const int64_t *idx, int32_t *rec, int64_t B, int64_t C, int64_t H,
                            int64_t W, int layout, int64_t n_idx, void *workspace_zeroed, int64_t workspace_bytes, void *stream) {
  return record_launch(record_plan(3, false, B, C, H, W, layout, n_idx, 0, 0), x, x_rec, idx, rec, workspace_zeroed, workspace_bytes, stream);
}

int gq_step_record_ssim_bits_f32(const float *x, const float *x_rec, const int64_t *idx, int32_t *rec, int64_t B, int64_t C, int64_t H,
                                 int64_t W, int layout, int64_t n_idx, int index_bits, int64_t n_codes, void *workspace_zeroed,
                                 int64_t workspace_bytes, void *stream) {
  return record_launch(record_plan(3, true, B, C, H, W, layout, n_idx, index_bits, n_codes), x, x_rec, idx, rec, workspace_zeroed, workspace_bytes, stream);
}

int gqhip_profile_enable(int on) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  g_prof_on = on != 0;
  if (g_prof_on && g_prof_pool.empty()) {   // callers that never reserve still get a (small) pool
    for (int i = 0; i < 64; ++i) {
      hipEvent_t a, b;
      if (hipEventCreate(&a) != hipSuccess) break;
      if (hipEventCreate(&b) != hipSuccess) { (void)hipEventDestroy(a); break; }
      g_prof_pool.emplace_back(a, b);
    }
  }
  return GQHIP_OK;
}

int gqhip_profile_reserve(int pairs) {
  if (pairs < 0) return GQHIP_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  while ((int)g_prof_pool.size() < pairs) {
    hipEvent_t a, b;
    if (hipEventCreate(&a) != hipSuccess) return check_launch();
    if (hipEventCreate(&b) != hipSuccess) { (void)hipEventDestroy(a); return check_launch(); }
    g_prof_pool.emplace_back(a, b);
  }
  return GQHIP_OK;
}

int gqhip_debug_enable(int on) {
  g_debug_stats = on != 0;
  return GQHIP_OK;
}

int gqhip_profile_collect(int *launches_host, double *total_ms_host) {
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
  {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    ev.swap(g_prof_events);
  }
  double total = 0.0;
  int cnt = 0;
  for (auto &pr : ev) {
    float ms = 0.f;
    if (hipEventSynchronize(pr.second) == hipSuccess &&
        hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) {
      total += ms;
      ++cnt;
    }
  }
  {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    for (auto &pr : ev) g_prof_pool.push_back(pr);   // recycled: the next profiled region creates nothing
  }
  if (launches_host) *launches_host = cnt;
  if (total_ms_host) *total_ms_host = total;
  return GQHIP_OK;
}

int gqhip_debug_counters(const void *workspace, int64_t *fallback_rows_host,
                         int64_t *reranked_halftiles_host) {
  if (!workspace) return GQHIP_ERR_INVALID_ARG;
  WsHeader h;
  if (hipMemcpy(&h, workspace, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return check_launch();
  if (fallback_rows_host) *fallback_rows_host = h.fb_count;
  if (reranked_halftiles_host) *reranked_halftiles_host = (int64_t)h.reranked;
  return GQHIP_OK;
}

int gqhip_debug_grid(const void *workspace, const void *cb_cache, int64_t *out4_host) {
  if (!workspace || !out4_host) return GQHIP_ERR_INVALID_ARG;
  WsHeader h;
  if (hipMemcpy(&h, workspace, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return check_launch();
  out4_host[0] = (int64_t)h.grid_leaves;
  out4_host[1] = (int64_t)h.reranked;
  out4_host[2] = h.fb_count;
  out4_host[3] = -1;
  if (cb_cache) {
    GridHdr g;
    if (hipMemcpy(&g, cb_cache, sizeof(g), hipMemcpyDeviceToHost) != hipSuccess) return check_launch();
    out4_host[3] = index_current(&g, kGridMagic, g.n, g.dim) ? 1 : 0;   // (this query knows neither n nor dim: the stamp and `stale` decide)
  }
  return GQHIP_OK;
}

}  // extern "C"
