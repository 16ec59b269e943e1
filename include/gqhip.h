/*
 * gqhip.h -- C ABI of libgqhip.so, the MI355X (gfx950) implementation of the
 * reference's Gaussian-quantiser inference hot path.
 *
 * Plain pointers and sizes only: every pointer is a DEVICE pointer (hipMalloc /
 * torch CUDA tensor .data_ptr()) unless its name ends in _host; `stream` is a
 * hipStream_t passed as void* (NULL = the default stream).  All entry points
 * are asynchronous on `stream`, never synchronise, never allocate, and return
 * a gqhip_status (0 = success) instead of throwing.  They are re-entrant and
 * hold no global state except the optional profiling recorder.
 *
 * The _host suffix is load-bearing: the Python package reads this header when
 * it loads the library and types a parameter `T *name_host` as a pointer to T
 * that the library dereferences on the host, every other pointer as an opaque
 * address (pit_hip/_lib.py:_parse_header), so a new prototype keeps to the
 * forms used below: `[const] type [*]name` with int, int64_t, float or double
 * scalars.
 *
 * Reference interface each entry point replaces (paths under /root/reference):
 *
 *   gq_scores_f32    gq_cuda_extension/gq_cuda/csrc/cuda/gq_cuda.cu:77-118
 *                    (host launcher `gq_cuda`, schema csrc/gq_cuda.cpp:29-31,
 *                    python gq_cuda/ops.py:7-8) -- fills out[b, n].
 *   gq_argmax_f32    pit/quantization/gaussian.py:124-150 -- the whole
 *                    "score matrix -> argmax -> index_select" block (K1+K2+K3 /
 *                    K4 of SURVEY.md 2.3), fused; indices are those of the
 *                    reference's torch CPU backend (gaussian.py:134-150).
 *   gq_quantize_z_f32 pit/quantization/gaussian.py:61-81,120-160 (GQ1) and
 *                    :273-331 (GQ2.quant_vq) -- also folds the chunk/clamp/exp
 *                    and the group permutes into the kernels.
 *   gq_dequant_f32   pit/quantization/gaussian.py:162-178, :347-362.
 *   gq_quantize_z_gauss_f32  pit/quantization/gaussian.py:211-271,273-345 (GaussianQuantRegularizer2.forward, eval).
 *   gq_gauss_train_f32 / gq_gauss_backward_f32  pit/quantization/gaussian.py:77-119 (GaussianQuantRegularizer.forward in
 *                    train()) and the autograd backward of it and of GaussianQuantRegularizer2.forward.
 *   vq_argmin_f32    pit/quantization/vq.py:58-73.
 *   vq_quantize_z_f32 pit/quantization/vq.py:39-96 (VQQuantizer.forward, eval).
 *   vq_backward_f32  the autograd backward of pit/quantization/vq.py:39-96 (VQQuantizer.forward in train()).
 *   lfq_pack_f32     pit/quantization/lfq.py:147-158.
 *   lfq_train_f32 / lfq_backward_f32  pit/quantization/lfq.py:56-76, 160-208 (LFQQuantizer.forward in train()) and its autograd backward.
 *   lfq_unpack_f32   pit/quantization/lfq.py:210-228 (also BSQ: pit/quantization/bsq.py:85-156).
 *   bsq_train_f32 / bsq_backward_f32  pit/quantization/bsq.py:14-37, 64-133 (BSQQuantizer.forward in train()) and its autograd backward.
 *   fsq_quantize_f32 / fsq_dequant_f32  pit/quantization/fsq.py:29-89.
 *   fsq_train_f32 / fsq_backward_f32  pit/quantization/fsq.py:6-9, 29-68 (FSQQuantizer.forward with round_ste's value) and its autograd backward.
 *   lpips_head_f32 / lpips_head_backward_f32  pit/modules/lpips/loss/lpips.py:46-66, 136-148 (the five comparison heads of LPIPS.forward) and their autograd backward.
 *   gn_silu_f32      pit/modules/unet.py:49-57 (Normalize + nonlinearity pairs).
 *   gq_index_histogram eval.py:127,137-141,152-154 (stubbed-out histogram).
 *   gq_ssim_f32      pit/evaluations/ssim.py:5-63 (get_ssim / get_ssim_and_msssim via pytorch_msssim), eval.py:170-178.
 *   gq_moments_update_f32  eval.py:186-203, 241-257 (the Inception feature blocks kept on the host, np.mean / np.cov over them).
 */
#ifndef GQHIP_H_
#define GQHIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GQHIP_ABI_VERSION 8   /* 2: filter selection, debug plan, NHWC upsample; 3: Winograd / sub-pixel conv transforms, gn_stats, add_bias_stats;
                               * 4: four-launch fused arg-max (no caller-cached max|cb|; noise / zhat_noquant in gq_quantize_z_f32), profile_reserve;
                               * 5: GroupNorm statistics as order-independent fixed-point records (gqhip_gnstat_t), conv3x3_f32 (fp32 matrix
                               *    cores: conv_in / conv_out of the encoder and decoder), gqhip_debug_barrier / gqhip_debug_tail;
                               * 6: three-launch fused arg-max -- undecided rows are finished inside the re-rank, the tail kernel with its grid
                               *    barriers is gone and gqhip_debug_barrier / gqhip_debug_tail with it; gq_step_record_f32, conv3x3_cin_small_f32;
                               * 7: codebook cache (gqhip_cb_cache_bytes; cb_cache arguments of gq_argmax_f32 / gq_quantize_z_f32 / vq_argmin_f32):
                               *    dim 4 runs a pruned exact search over a cached spatial index of the codebook (csrc/gq_grid.h), dims 8 / 16 /
                               *    32 keep the filter's fp16 codebook image there;
                               * 8: module-level eval forwards of GaussianQuantRegularizer2 (gq_quantize_z_gauss_f32: the Gaussian branch's
                               *    statistics and lambda state on the device) and VQQuantizer (vq_quantize_z_f32: layouts, straight-through
                               *    value and codebook loss inside the launches); additive since, the version unchanged: per-image SSIM /
                               *    MS-SSIM (gq_ssim_f32), the three-metric step record (gq_step_record_ssim_f32), the train-mode step of the Gaussian
                               *    regularizers (gq_gauss_train_f32, gq_gauss_backward_f32), the backward of VQQuantizer's train step
                               *    (vq_backward_f32, vq_backward_workspace_bytes), LFQQuantizer's train step
                               *    (lfq_train_f32, lfq_backward_f32, lfq_train_workspace_bytes), the bit-packed index wire format for any
                               *    codebook size (gq_indices_pack_bits, gq_indices_unpack_bits, gq_index_histogram_packed,
                               *    gq_step_record_bits_f32, gq_step_record_ssim_bits_f32 and their two _workspace_bytes functions), the train steps of
                               *    BSQQuantizer (bsq_train_f32, bsq_backward_f32, bsq_train_workspace_bytes) and FSQQuantizer (fsq_train_f32,
                               *    fsq_backward_f32), the LPIPS comparison head (lpips_head_f32, lpips_head_backward_f32,
                               *    lpips_head_workspace_bytes), the fp64 feature moments of the Frechet statistics (gq_moments_update_f32,
                               *    gq_moments_state_bytes) */

/* GroupNorm statistics of one (image, group): GQHIP_GNSTAT_WORDS int64 words = {sum: 3 limbs, sum of squares: 3 limbs, poison,
 * unused}; value = q0 2^-56 + q1 2^-16 + q2 2^24.  Every kernel that leaves statistics behind adds its threads' fp32 partial
 * sums to these records with INTEGER atomics (exact, associative), so the statistics -- and everything normalised with them --
 * are bit-identical from run to run whatever order the adds land in (csrc/gq_stats.h).  A `stats` argument below is an
 * array of B * groups such records (64 bytes each), zeroed by the producing call. */
typedef int64_t gqhip_gnstat_t;
#define GQHIP_GNSTAT_WORDS 8

typedef enum gqhip_status {
  GQHIP_OK = 0,
  GQHIP_ERR_INVALID_ARG = 1,   /* NULL pointer, negative size, unsupported dim */
  GQHIP_ERR_WORKSPACE = 2,     /* workspace too small / NULL                  */
  GQHIP_ERR_LAUNCH = 3,        /* hipGetLastError() != hipSuccess after launch */
  GQHIP_ERR_NO_DEVICE = 4
} gqhip_status;

int gqhip_abi_version(void);
const char *gqhip_status_string(int status);
/* last hipError_t observed by a failing call on this thread (0 if none). */
int gqhip_last_hip_error(void);

/* Filter kernel of the fused arg-max (gq_argmax_f32 / gq_quantize_z_f32 / vq_argmin_f32).  AUTO: the fp16 main-product
 * filter (ONE fp16 MFMA product per fp32 product, no correction terms; its rounding error is covered by a bound the re-rank
 * derives from the row's own data) at every MFMA dim (4/8/16/32), Gaussian score and VQ; rows whose candidate records are incomplete
 * are finished inside the re-rank kernel by a complete scan of the record sets in question (csrc/gq_rerank.h).  FP32: always the fp32 MFMA filter.  BF16: the split-bf16 filter (three
 * bf16 products per fp32 product).  MIXED: round 2's fp16 + fp8 filter (one fp16 product + block-scaled fp8 corrections) at
 * dim 16 with the Gaussian score, split-bf16 elsewhere.  All feed the same exact re-rank: the indices are identical.
 * Process-wide; initial value from the environment (GQHIP_FILTER=fp32|bf16|mixed).  The workspace size depends on it:
 * query gqhip_workspace_bytes after changing it.  (No reference counterpart.) */
#define GQHIP_FILTER_AUTO 0
#define GQHIP_FILTER_FP32 1
#define GQHIP_FILTER_BF16 2
#define GQHIP_FILTER_MIXED 3
int gqhip_set_filter(int kind);
int gqhip_get_filter(void);

/* Route of the codebook dims between the filter dims -- 5..7, 9..15, 17..31 -- in gq_argmax_f32 / gq_quantize_z_f32 /
 * gq_quantize_z_gauss_f32 / vq_argmin_f32 / vq_quantize_z_f32.  EXHAUSTIVE (default): one block per row scores every code with the
 * reference's arithmetic.  PADDED: the rows and the codebook are zero-padded in the workspace to the next filter dim (8, 16, 32:
 * mu 0, sd 1, log sd 0, code 0 in the pad columns), the selected filter runs there unchanged, and the exact re-rank -- which alone
 * decides an index -- scores with the TRUE dim, so the indices, zhat and every other output are the same bits either way
 * (DESIGN.md section 3.1).  Such a call keeps nothing in the codebook cache (gqhip_cb_cache_bytes stays 0 at these dims): the padded
 * operand image is rebuilt in the workspace on every call.  Dims 1..3 and 33..64 stay on the exhaustive kernel under either value
 * (they have switches of their own: gqhip_set_low_dims and gqhip_set_wide_dims below).
 * Process-wide; initial value from the environment (GQHIP_ODD_DIMS=padded).  The workspace size depends on it: query
 * gqhip_workspace_bytes after changing it.  An unknown kind: GQHIP_ERR_INVALID_ARG, the selection stays.  (No reference counterpart.) */
#define GQHIP_ODD_DIMS_EXHAUSTIVE 0
#define GQHIP_ODD_DIMS_PADDED 1
int gqhip_set_odd_dims(int kind);
int gqhip_get_odd_dims(void);
/* Diagnostic: the dim the filter of the fused arg-max runs at for (n, dim) under the current selections -- `dim` itself at 4, 8,
 * 16, 32; 8, 16 or 32 for a dim the PADDED route serves; 64 for dims 33..64 where the wide route (gqhip_set_wide_dims below) runs;
 * 0 where the exhaustive kernel runs; -1: n < 1 or dim outside 1..64. */
int64_t gqhip_filter_dim(int64_t n, int64_t dim);

/* Route of the codebook dims 33..64 in gq_argmax_f32 / gq_quantize_z_f32 / gq_quantize_z_gauss_f32 / vq_argmin_f32 /
 * vq_quantize_z_f32 (and the train forwards that call the last two).  EXHAUSTIVE (default): one block per row scores every code with
 * the reference's arithmetic.  FILTER: with the filter selection AUTO (the fp16 main product) the filter and the exact re-rank run at
 * dim 64 -- 128 fp16 products per value, eight v_mfma_f32_32x32x16_f16 per tile.  Dim 64 itself: prep -> filter -> re-rank, as at
 * dims 8 / 16 / 32.  Dims 33..63: rows and codebook are zero-padded to 64 in the workspace first (mu 0, sd 1, log sd 0, code 0 in the
 * pad columns), exactly as gqhip_set_odd_dims(PADDED) does below 32, and the re-rank -- which alone decides an index -- scores, scans
 * and stores with the TRUE dim: the indices, zhat and every other output are the same bits either way.
 * What keeps the exhaustive kernel under either value: the filter selections FP32 / BF16 / MIXED (no dim-64 kernel of theirs:
 * gqhip_filter_dim says 0), a codebook beyond the split cap, gq_scores_f32's own route.  Nothing is kept in the codebook cache at these
 * dims (gqhip_cb_cache_bytes and gqhip_grid_search_applies stay 0): the operand image is rebuilt in the workspace on every call.
 * Process-wide; initial value from the environment (GQHIP_WIDE_DIMS=filter).  The workspace size depends on it: query
 * gqhip_workspace_bytes after changing it.  An unknown kind: GQHIP_ERR_INVALID_ARG, the selection stays.  (No reference counterpart.) */
#define GQHIP_WIDE_DIMS_EXHAUSTIVE 0   /* default */
#define GQHIP_WIDE_DIMS_FILTER 1
int gqhip_set_wide_dims(int kind);
int gqhip_get_wide_dims(void);

/* Route of the codebook dims 1..3 in gq_argmax_f32 / gq_quantize_z_f32 / gq_quantize_z_gauss_f32 (the Gaussian score only).
 * EXHAUSTIVE (default): one block per row scores every code with the reference's arithmetic.  SEARCH: a call with 4096 <= n <= 2^20
 * codes and a codebook cache of gqhip_cb_cache_bytes runs a pruned exact search (csrc/gq_lowdim.h): rows as on the exhaustive
 * route -> codebook hash -> index builder (exits unless the cache is stale) -> search -> finish of the rows it listed.  The index
 * buckets the codes into 4096 cells with tight bounding boxes (4096 / 64 x 64 / 16 x 16 x 16 quantile cells) under 256 coarse
 * nodes; a row gives the reference's arithmetic to the codes of the cells whose closed-form bound is within the rounding margin of
 * its best code, and the (score, lowest index) order decides: the indices, zhat and every other output are the same bits either way
 * (DESIGN.md section 3.2b).  Rows with a non-finite operand, bound or codebook, with sd <= 0, or that reach an overfull cell get
 * the exhaustive kernel itself in the finish launch.  There is no filter: gqhip_filter_dim stays 0, and gqhip_set_filter /
 * gqhip_set_odd_dims do not matter here.  What keeps today's route under either value: the VQ entry points, gq_scores_f32, the train
 * steps, n outside the range, a NULL or short cache, every other dim.  Process-wide; initial value from the environment
 * (GQHIP_LOW_DIMS=search).  gqhip_cb_cache_bytes depends on it, and gqhip_workspace_bytes may: query them after changing it.  An
 * unknown kind: GQHIP_ERR_INVALID_ARG, the selection stays.  (No reference counterpart.) */
#define GQHIP_LOW_DIMS_EXHAUSTIVE 0   /* default */
#define GQHIP_LOW_DIMS_SEARCH 1
int gqhip_set_low_dims(int kind);
int gqhip_get_low_dims(void);
/* 1: a GQ call of this codebook shape with a cache runs the search (SEARCH selected, dim 1..3, 4096 <= n <= 2^20); 0 otherwise. */
int gqhip_low_dim_search_applies(int64_t n, int64_t dim);

/* Diagnostics: launch plan and workspace layout of the fused arg-max for a shape.  out8_host = { byte offset of the
 * candidate records, code splits, tiles per candidate group, tiles per split, filter kernel the plan selects (0 fp32 MFMA, 1 split-bf16, 2 fp16 + fp8, 3 fp16 main product: the default at dims 8 / 16 / 32), coefficient of the
 * filter error bound (E_f = coeff * 2^-24 * T; fp16 main product: 16700 at filter dims 8 / 16 / 32 -- up to 64 products per value --,
 * 17000 at the wide route's filter dim 64 -- 128 products), row tiles per wave, waves per filter block }.
 * The records are 16 bytes per (row, record set): { fp32 m1; fp16 gaps m1 - m2..m4, rounded towards zero; three 16-bit
 * half-group ids relative to the set's split } (csrc/gq_common.h:Rec); "code splits" counts record sets. */
int gqhip_debug_plan(int64_t rows, int64_t n, int64_t dim, int64_t *out8_host);


/* ---- workspace ------------------------------------------------------------
 * Bytes of scratch gq_argmax_f32 / gq_quantize_z_f32 / vq_argmin_f32 need for
 * `rows` rows against `n` codes of width `dim`.  The caller allocates once
 * (device memory, 256-B aligned) and reuses it; contents are don't-care: every call
 * rebuilds what it keeps there (row operands, bound sums, candidate records, max|cb|,
 * counters) from its arguments.  What is derived from the CODEBOOK and worth keeping
 * across calls lives in the separate codebook cache below, which the library validates
 * against the codebook's content on every call. */
int64_t gqhip_workspace_bytes(int64_t rows, int64_t n, int64_t dim);

/* ---- codebook cache ---------------------------------------------------------
 * Bytes of PERSISTENT device memory (256-B aligned) in which the fused arg-max keeps what it derives from a codebook of `n` codes
 * of width `dim` across calls; 0 when this shape keeps nothing (then pass NULL / 0).  Today: dim 4 with 2^14 <= n <= 2^20
 * -- the codes sorted into 4096 sub-leaves under a tree of bounding boxes (16 -> 256 -> 1024 -> 4096), which lets dim 4 run a pruned
 * exact search (~8 sub-leaves of ~16 codes per row instead of all n codes; csrc/gq_grid.h) in place of filter + re-rank --; dims
 * 8 / 16 / 32: the fp16 operand image of the codebook that the MFMA filter reads (each 1/256 slice stamped with its content hash);
 * dims 1 / 2 / 3 with 4096 <= n <= 2^20, only under gqhip_set_low_dims(GQHIP_LOW_DIMS_SEARCH): the cell index of csrc/gq_lowdim.h
 * (same header, hashes and rebuild protocol; every offset and index read from its body is bounded by the codebook size as well).
 * Contract: the caller owns the buffer, hands the SAME buffer to every call that uses the same codebook, and never writes it;
 * its initial contents are don't-care.  The library validates it on EVERY call -- the first launch hashes the codebook it is
 * given (it reads it anyway) and compares with the hashes the cache was stamped with -- and rebuilds it in-stream (one extra
 * one-block kernel that otherwise exits at once) when they differ: a codebook edited in place by any route, a different
 * codebook, a fresh buffer or one overwritten as a whole all cost one rebuild and never a wrong index.  What the validation does NOT
 * cover is a write into the BODY of a cache whose 4-KiB header (the stamps) is left intact -- the "never writes it" above is the
 * caller's half of the contract; the dim-4 search still bounds every offset and index it reads from the body by the codebook size,
 * so such a write can cost a wrong index but never an out-of-range access (csrc/gq_grid.h); the fp16 image of dims 8 / 16 / 32 is only
 * ever multiplied -- no address is derived from it.  One cache serves one stream at a time.
 * Without a cache (NULL) every shape runs the filter + re-rank path.  (No reference counterpart: the reference recomputes
 * everything per call, pit/quantization/gaussian.py:136-150.) */
int64_t gqhip_cb_cache_bytes(int64_t n, int64_t dim);
/* 1 when a call with this codebook shape and a cache runs the pruned search (today: dim 4, 2^14 <= n <= 2^20, filter selection
 * AUTO), 0 when it runs filter + re-rank (dims 8 / 16 / 32 then keep the filter's fp16 codebook image in the cache). */
int gqhip_grid_search_applies(int64_t n, int64_t dim);
/* Synchronous (a 4-KiB device-to-host copy; never needed for correctness): what the index builder found when it sorted this codebook.
 * 1: a DEGENERATE book for the search -- some sub-leaf holds more than 255 codes (most of the book in one cell: clustered or collapsed
 * codebooks), so every row that lists it is handed to gq_grid_finish_kernel, a block per row: a multi-millisecond call where the dense
 * filter + re-rank takes ~100 us; a host that sees 1 should stop passing the cache for this codebook (NULL / 0: the dense path).
 * 0: fine.  -1: no current index in `cb_cache` (never built, stale, another shape) or a shape without a search.  pit_hip's Workspace
 * asks once, at the call after the one that built the index.  Dims 1..3 under GQHIP_LOW_DIMS_SEARCH: the same answers for the cell
 * index of csrc/gq_lowdim.h -- 1: some cell holds more than max(256, n / 256) codes, and every row that reaches it is finished by the
 * exhaustive kernel.  (No reference counterpart.) */
int gqhip_cb_cache_degenerate(const void *cb_cache, int64_t n, int64_t dim);

/* ---- compat op: the reference's native boundary ---------------------------
 * out[r, j] = sum_i -((cb[j,i]-mu[r,i])/sd[r,i])^2 + cb[j,i]^2 * beta
 * mu, sd [rows, dim]; cb [n, dim]; out [rows, n]; all fp32 contiguous.
 * dims 4 / 8 / 16 / 32: the expanded form [beta - 1/sd^2 | 2 mu/sd^2] x [cb^2 | cb] + const on the matrix cores (fp32 MFMA at
 * dims 4 / 8; three fp16 products of two-term splits with fp32 accumulation at dims 16 / 32 -- error vs an fp64 evaluation
 * <= ~4e-7 of sum_i |terms| per element in either form, the level of the per-pair formula in fp32); other dims, n < 32 or a
 * NaN beta: the per-pair formula.  Environment: GQHIP_SCORES=f32 (fp32 MFMA at dims 16 / 32 too), =direct (per-pair always). */
int gq_scores_f32(const float *mu, const float *sd, const float *cb, float *out,
                  int64_t dim, int64_t rows, int64_t n, double beta,
                  void *stream);

/* ---- fused score + argmax + gather ----------------------------------------
 * idx[r]  = argmax_j of the reference torch-backend score (first max wins,
 *           NaN counts as max), bit-identical to the CPU reference given the
 *           same (mu, sd, logsd).
 * zhat[r] = cb[idx[r]]  (optional, may be NULL).
 * logsd_or_null: log(sd) as the caller computed it; NULL -> the kernel uses
 *           float(log(double(sd))) (correctly rounded).
 * dim: any 1..64 (4, 8, 16, 32 run on the MFMA filter; 5..7, 9..15, 17..31 too, zero-padded to the next of them, once
 *           gqhip_set_odd_dims(GQHIP_ODD_DIMS_PADDED) selects that -- prep of the padded operands, filter, re-rank, the same
 *           indices; 1..3 with a codebook cache run the pruned search of csrc/gq_lowdim.h once
 *           gqhip_set_low_dims(GQHIP_LOW_DIMS_SEARCH) selects that -- five launches, the builder and the finish exit at once in
 *           the common case, the same indices; 33..64 run the dim-64 filter + re-rank once
 *           gqhip_set_wide_dims(GQHIP_WIDE_DIMS_FILTER) selects that, the same indices; every other case exhaustive).
 * Dim 4 with a codebook cache: prep -> index check -> pruned exact search -> finish of the rows it left undecided
 * (csrc/gq_grid.h; four launches, the second and fourth exit at once in the common case).
 * Three launches on `stream` for the other MFMA dims: prep (operand images, bound sums,
 * max|cb|) -> filter -> exact re-rank (rows the filter leaves undecided are
 * finished inside it by a block-wide scan of their record sets). */
int gq_argmax_f32(const float *mu, const float *sd, const float *logsd_or_null,
                  const float *cb, int64_t *idx, float *zhat_or_null,
                  int64_t dim, int64_t rows, int64_t n, double beta,
                  void *workspace, int64_t workspace_bytes,
                  void *cb_cache_or_null, int64_t cb_cache_bytes, void *stream);

/* ---- module-level fused quantiser -----------------------------------------
 * z is the encoder output holding [mu | logvar] along its channel axis.
 * layout: GQHIP_LAYOUT_BCHW  z [B, 2c, L] (L = h*w)   -> idx [B, K, L], zhat [B, c, L]
 *         GQHIP_LAYOUT_BLC   z [B, L, 2c]             -> idx [B, L, K], zhat [B, L, c]
 * grouping: GQHIP_GROUP_STRIDED    (GaussianQuantRegularizer : column g of
 *                                   sub-codebook k <- channel g*K + k)
 *           GQHIP_GROUP_CONTIGUOUS (GaussianQuantRegularizer2: channel k*dim + g)
 * K = c / dim.  logvar is clamped to [lv_min, lv_max]; sd = exp(0.5*logvar) and
 * log(sd) are evaluated in fp64 and rounded once (numerics).
 * mu_out/sd_out (optional, [rows, dim], row = (b*L + l)*K + k) receive the
 * permuted operands so callers/tests can replay them through the oracle.
 * noise_or_null / zhat_noquant_or_null (both in the layout of zhat): when given,
 * zhat_noquant = mu + noise * sd (gaussian.py:121; the caller draws `noise` with
 * its own generator, e.g. torch.randn) is written by the same first launch. */
#define GQHIP_LAYOUT_BCHW 0
#define GQHIP_LAYOUT_BLC 1
#define GQHIP_GROUP_STRIDED 0
#define GQHIP_GROUP_CONTIGUOUS 1
int gq_quantize_z_f32(const float *z, const float *noise_or_null, const float *cb,
                      int64_t *idx, float *zhat_or_null, float *zhat_noquant_or_null,
                      float *mu_out_or_null, float *sd_out_or_null, int64_t B,
                      int64_t L, int64_t c, int64_t dim, int64_t n, int layout,
                      int grouping, double lv_min, double lv_max, double beta,
                      void *workspace, int64_t workspace_bytes,
                      void *cb_cache_or_null, int64_t cb_cache_bytes, void *stream);

/* ---- GaussianQuantRegularizer2.forward in eval (pit/quantization/gaussian.py:211-271 quant_gaussian, :273-331 quant_vq,
 * :333-345 forward) as ONE call: gq_quantize_z_f32's launches, the re-rank launch carrying one extra block for the statistics (behind the
 * dim-4 search and at dims without a filter: one extra one-block launch).  On top of gq_quantize_z_f32:
 *   zhat_noquant = mu + noise * sd (required here: it is the Gaussian branch's sample), sd_out_or_null = sd in the layout of zhat
 *   (info["std"]); use_ste != 0: zhat = (zhat_noquant - zhat_noquant) + code, the value of `zhat_g - zhat_g.detach() + zhat_v`
 *   (gaussian.py:337-338) in the reference's fp32 op order (a non-finite zhat_noquant makes it NaN there too), and
 *   zhat_quant_or_null (layout of zhat) then receives the codewords themselves (info["zhat_quant"]); without use_ste zhat holds them;
 *   per row (= per group) kl2 = sum_i 1.4426 * 0.5 * (mu^2 + var - 1 - logvar) (gaussian.py:225-229; the element in the
 *   reference's fp32 op order with var = float(exp(double(logvar))), the row sum in fp64 rounded once), reduced in a fixed order
 *   (bit-reproducible) to
 *   scalars_out (64 bytes of device memory, 8-byte aligned): float[0..3] = { kl_loss, bits-mean, bits-min, bits-max }
 *       (kl_loss = mean(ge kl2 + eq kl2 + le kl2) * lam with lam / lam_min / lam_max as they were BEFORE this call, gaussian.py:233-241);
 *       double[0..2] at byte 32 = { lam, lam_min, lam_max } AFTER this call's update (what info["lam"], ["lam-min"], ["lam-max"] report).
 *   lam_state (device, double[3] = { lam, lam_min, lam_max }, in / out): the adaptive lambda state machine of gaussian.py:243-257
 *       advanced on the device in fp64 (the same IEEE operations as the reference's Python floats), so the forward reads nothing
 *       back -- the reference pays three host syncs per forward for it.  log2n = int(log2(n_samples)); thresholds are compared as
 *       torch does (the scalar cast to fp32); lam_max_decreases: 1 = gaussian.py:109-112 (GQ1's train branch), 0 = GQ2, whose
 *       decrease at gaussian.py:251 is an expression without effect; clamps: lam_max to [1, lam_hi], lam_min to [lam_lo, 1].
 * Workspace / codebook cache / stream: as gq_quantize_z_f32. */
int gq_quantize_z_gauss_f32(const float *z, const float *noise, const float *cb, int64_t *idx, float *zhat,
                            float *zhat_quant_or_null, float *zhat_noquant, float *sd_out_or_null, void *scalars_out, double *lam_state, int64_t B,
                            int64_t L, int64_t c, int64_t dim, int64_t n, int layout, int grouping, double lv_min,
                            double lv_max, double beta, int use_ste, double log2n, double tolerance, double lam_factor,
                            double lam_lo, double lam_hi, int lam_max_decreases, void *workspace, int64_t workspace_bytes,
                            void *cb_cache_or_null, int64_t cb_cache_bytes, void *stream);

/* ---- the train-mode step of the Gaussian regularizers: GaussianQuantRegularizer.forward in train()
 * (pit/quantization/gaussian.py:77-119) as ONE call -- an elementwise launch + the one-block statistics launch of
 * gq_quantize_z_gauss_f32 -- with no codebook and no workspace (csrc/gq_gauss_train.h).  Layouts and groupings as above:
 *   zhat (layout of zhat above) = mu + noise * sd, sd = float(exp(double(0.5f * logvar))), logvar clamped to [lv_min, lv_max] (NaN
 *       propagates), every fp32 op rounded separately; sd_out_or_null receives sd in the same layout;
 *   kl2row (caller-owned, rows = B L K floats, row = (b L + l) K + k): per row the fp64 sum, in ascending g, of
 *       1.4426 * 0.5 * (mu^2 + var - 1 - logvar) (the element in the reference's fp32 op order), rounded once -- the values
 *       gq_quantize_z_gauss_f32 reduces;
 *   scalars_out / lam_state / log2n / tolerance / lam_factor / lam_lo / lam_hi / lam_max_decreases: as gq_quantize_z_gauss_f32
 *       (same 64 bytes, same fixed-order reduction, same fp64 state machine; GQ1's train branch passes lam_max_decreases = 1);
 *   loss_divisor (> 0): kl_loss = sum(ge kl2 + eq kl2 + le kl2) / loss_divisor * lam -- B for GQ1 (gaussian.py:96-98:
 *       sum over [1, 2], sum / B), rows for a mean (gaussian.py:241; then scalars_out and lam_state are bit-identical to
 *       gq_quantize_z_gauss_f32's on the same z and state).
 * Accesses are 16 bytes wide along the contiguous axis (L for BCHW, c for BLC) when the shape and the pointers allow (L % 4 == 0;
 * K % 4 == 0 or dim % 4 == 0; 16-byte aligned tensors), 4 bytes otherwise.  rows == 0: GQHIP_OK, nothing is launched. */
int gq_gauss_train_f32(const float *z, const float *noise, float *zhat, float *sd_out_or_null, float *kl2row, void *scalars_out,
                       double *lam_state, int64_t B, int64_t L, int64_t c, int64_t dim, int layout, int grouping, double lv_min,
                       double lv_max, double log2n, double tolerance, double lam_factor, double lam_lo, double lam_hi,
                       int lam_max_decreases, double loss_divisor, void *stream);

/* ---- the backward of both train-mode forwards (gq_gauss_train_f32; gq_quantize_z_gauss_f32 under autograd) in ONE elementwise
 * launch that writes the whole grad_z (layout of z: the mu half and the logvar half).
 *   z, noise: the forward's; g_zhat_or_null / g_sd_or_null (layout of zhat): gradients arriving at zhat (for GQ2 with the straight-
 *   through mix: at zhat plus at zhat_noquant, summed by the caller) and at sd; g_kl_or_null: ONE float on the device, the gradient
 *   arriving at kl_loss; NULL = zero.  lam_before (device double[3], 8-byte aligned): { lam, lam_min, lam_max } as they were BEFORE
 *   the forward's update (a device copy taken ahead of the forward call); thresholds, clamp, layout, grouping and loss_divisor as
 *   the forward's.  Per row the kernel recomputes kl2 with the forward's function and order, so its class is the forward's:
 *       w(row) = (float)lam_max if kl2 > float(log2n + tol), (float)lam_min if kl2 < float(log2n - tol), 1 otherwise
 *       coef   = g_kl * (float)lam * w(row) / loss_divisor
 *       grad_mu     = g_zhat + coef * 1.4426 * mu
 *       grad_logvar = inside ? g_zhat * noise * 0.5 * sd + g_sd * 0.5 * sd + coef * 1.4426 * 0.5 * (var - 1) : 0
 *   inside = (lv_min <= logvar <= lv_max) on the unclamped value (torch.clamp's gradient mask); sd / var = fp64 exp rounded once,
 *   1.4426 * 0.5 = float(0.7213) as in the forward.  Error against an fp64 evaluation: a few 2^-24 of the sum of |terms|
 *   (tests/test_gpu_train_step.py).  Reads nothing from the host, no atomics: graph-capturable like the forward. */
int gq_gauss_backward_f32(const float *z, const float *noise, const float *g_zhat_or_null, const float *g_sd_or_null,
                          const float *g_kl_or_null, const double *lam_before, float *grad_z, int64_t B, int64_t L, int64_t c,
                          int64_t dim, int layout, int grouping, double lv_min, double lv_max, double log2n, double tolerance,
                          double loss_divisor, void *stream);

/* zhat from indices (same layouts as above). */
int gq_dequant_f32(const int64_t *idx, const float *cb, float *zhat, int64_t B,
                   int64_t L, int64_t K, int64_t dim, int64_t n, int layout,
                   int grouping, void *stream);

/* ---- VQ: argmin_j |z_r - e_j|^2 (fp64 arbiter, first min wins) ------------- */
int vq_argmin_f32(const float *z, const float *emb, int64_t *idx,
                  float *zq_or_null, int64_t dim, int64_t rows, int64_t n,
                  void *workspace, int64_t workspace_bytes,
                  void *cb_cache_or_null, int64_t cb_cache_bytes, void *stream);

/* ---- VQQuantizer.forward in eval (pit/quantization/vq.py:39-96) as ONE call: the permutes, the per-sub-codebook slices, the
 * embedding lookup, the straight-through value and the two MSE means are inside vq_argmin_f32's launches + one small launch.
 *   z [B, c, L] (GQHIP_LAYOUT_BCHW) or [B, L, c] (GQHIP_LAYOUT_BLC), c = dim * K; sub-codebook k, column d <- channel d * K + k
 *   (vq.py:53), every sub-codebook against the same `emb` [n, dim];
 *   idx [B, K, L] / [B, L, K];  zq (layout of z) = z + (e - z), e = emb[idx], in the reference's fp32 op order (vq.py:89);
 *   loss2_or_null (device float[2]): [0] = codebook_loss = mean + beta * mean (legacy != 0) | beta * mean + mean (vq.py:78-86) in
 *   fp32, [1] = mean = sum((e - z)^2) / (rows * dim): squared differences formed in fp32, summed in fp64 in a fixed order
 *   (bit-reproducible; torch's fp32 mean agrees to rounding).  Arg-min: vq_argmin_f32's (fp64 arbiter, first minimum wins). */
int vq_quantize_z_f32(const float *z, const float *emb, int64_t *idx, float *zq, float *loss2_or_null, int64_t B, int64_t L,
                      int64_t c, int64_t dim, int64_t n, int layout, double beta, int legacy, void *workspace,
                      int64_t workspace_bytes, void *cb_cache_or_null, int64_t cb_cache_bytes, void *stream);

/* ---- the backward of VQQuantizer.forward's train step (vq.py:78-89; the forward is vq_quantize_z_f32 without a cache) in ONE call.
 *   z, emb, idx, layouts and the channel rule: vq_quantize_z_f32's.  Item p = (b L + l) K + k, e_p = emb[idx_p], N = B L c;
 *   (a, b) = (1, beta) when legacy != 0, (beta, 1) otherwise.
 *   g_zq_or_null (layout of z): the gradient arriving at zq; g_loss_or_null: ONE float on the device (4-byte aligned), the gradient
 *   arriving at codebook_loss; NULL = zero.
 *   grad_z_or_null (layout of z) = g_zq + (g_loss a 2 / N) (z - e): the difference in fp32, the rest in fp64, rounded once (the
 *   straight-through value hands g_zq to z and nothing to e).  16-byte accesses when z, g_zq and grad_z are 16-byte aligned and
 *   L % 4 == 0 (BCHW) / c % 4 == 0 (BLC), 4-byte accesses otherwise.
 *   grad_emb_or_null [n, dim], written WHOLE (exact +0.0 for a code no item chose):
 *       grad_emb[j][d] = (float)((g_loss b 2 / N) * sum over p with idx_p = j, ascending p, of (double)fl32(e_p[d] - z_p[d]))
 *   with the sum and the product in fp64.  A code chosen by more than 128 items (kVqChunk, csrc/vq_train.h) is summed as partials
 *   of 128 consecutive items of its ascending list each, added in chunk order.  The order of every sum depends on idx and the
 *   shape alone: no float atomics, results are bit-identical from run to run.  (Built from a stable radix sort of the items by
 *   code in the workspace; integer atomics only where their result is order-free.)
 *   An idx value outside [0, n) is checked before it addresses anything: that item adds nothing to grad_emb, and its elements of
 *   grad_z are g_zq alone.
 *   workspace: vq_backward_workspace_bytes(B L K, n, dim) bytes (-1: unsupported shape), 16-byte aligned, contents don't-care on entry -- the call
 *   rebuilds all of it; NULL or short -> GQHIP_ERR_WORKSPACE.  No items: GQHIP_OK after zeroing grad_emb.  Reads nothing back to
 *   the host: graph-capturable. */
int64_t vq_backward_workspace_bytes(int64_t items, int64_t n, int64_t dim);
int vq_backward_f32(const float *z, const float *emb, const int64_t *idx, const float *g_zq_or_null, const float *g_loss_or_null,
                    float *grad_z_or_null, float *grad_emb_or_null, int64_t B, int64_t L, int64_t c, int64_t dim, int64_t n,
                    int layout, double beta, int legacy, void *workspace, int64_t workspace_bytes, void *stream);

/* ---- LFQ: sign quantisation + big-endian bit pack -------------------------- */
int lfq_pack_f32(const float *x, int64_t *idx, float *q_or_null, int64_t rows,
                 int64_t nbits, void *stream);
int lfq_unpack_f32(const int64_t *idx, float *q, int64_t rows, int64_t nbits,
                   void *stream);

/* ---- LFQQuantizer's train step (lfq.py:56-76, 160-208) in ONE forward and ONE backward call, without the [rows, 2^d] logits.
 *   x: [B, C, L] (layout 0, BCHW) or [B, L, C] (layout 1, BLC; also channels_last memory), C = nc d, d in 1..16, nc d <= 62.
 *   Row r = (b L + l) nc + ci holds channels ci d + i; R = B L nc rows.  T = 0.01, eps = 1e-5, s = 400 x, p = sigma(s), q = 1 - p:
 *   the row's softmax over {-1,+1}^d is the product of d Bernoullis, so with the low dl = d / 2 bits as v, the high dh = d - dl
 *   bits as u and the per-row tables A_r[u], B_r[v] of those products, avg[u 2^dl + v] = (1 / R) sum_r A_r[u] B_r[v] (code j has
 *   +1 in dimension i when bit i of j is set: the order of the reference's avg_probs).
 * lfq_train_f32 writes
 *   quantized (layout of x) = x + (q - x), q = x > 0 ? 1 : -1, two rounded fp32 operations;
 *   idx [B L] = the big-endian pack of the C sign bits of a position (lfq_pack_f32's value);
 *   avg [2^d] floats, kept by the caller for the backward;
 *   scalars [4] floats ON THE DEVICE = {entropy_aux_loss = w_s per_sample_entropy - w_b codebook_entropy, per_sample_entropy =
 *     mean_r sum_i (log1p(e) + |s| e / (1 + e)) with e = exp(-|s|), codebook_entropy = -sum avg log(avg + eps), commit_loss =
 *     mean((x - q)^2)}.
 * lfq_backward_f32, with the gradients arriving at quantized (g_q, layout of x) and at entropy_aux_loss / commit_loss (ONE float
 * each ON THE DEVICE), NULL = zero, writes grad_x (layout of x) =
 *     g_q + g_commit 2 (x - q) / (B L C) + g_aux 400 (w_s / R (-s p q) - w_b d codebook_entropy / d s)
 *   from x and avg alone (G = -(log(avg + eps) + avg / (avg + eps)); for a high bit i,
 *   d codebook_entropy / d s_i = (1 / R) sum_u (G B_r)[u] A_r[u] (bit_i(u) ? q_i : -p_i); low bits: G^T A_r and B_r).
 * The GEMMs run on v_mfma_f32_32x32x2_f32.  Rows are summed in chunks of 256 (csrc/lfq_train.h: kLfqChunk) added in chunk
 * order: no float atomics, bit-identical from run to run.  Neither call reads the host or synchronises; both are ordered on
 * `stream`.  workspace: lfq_train_workspace_bytes(R, d) bytes (-1: rows < 0 or too many, d outside 1..16), 16-byte aligned, contents
 * don't-care on entry, nothing in it is kept between calls; NULL, misaligned or short -> GQHIP_ERR_WORKSPACE.  B L = 0: GQHIP_OK. */
int64_t lfq_train_workspace_bytes(int64_t rows, int64_t d);
int lfq_train_f32(const float *x, float *quantized, int64_t *idx, float *avg, float *scalars, int64_t B, int64_t L, int64_t C,
                  int64_t nc, int64_t d, int layout, float w_s, float w_b, void *workspace, int64_t workspace_bytes, void *stream);
int lfq_backward_f32(const float *x, const float *avg, const float *g_q_or_null, const float *g_aux_or_null,
                     const float *g_commit_or_null, float *grad_x, int64_t B, int64_t L, int64_t C, int64_t nc, int64_t d, int layout,
                     float w_s, float w_b, void *workspace, int64_t workspace_bytes, void *stream);

/* ---- FSQ: tanh-bounded rounding + mixed-radix pack (pit/quantization/fsq.py:29-89) ----
 * z, zhat [rows, nlev] fp32; idx [rows] int32 (the reference's dtype); levels_host: nlev (<= 16)
 * positive ints on the HOST.  tanh/atanh are evaluated in fp64 and rounded once. */
int fsq_quantize_f32(const float *z, const int32_t *levels_host, int64_t nlev, float *zhat,
                     int32_t *idx, int64_t rows, void *stream);
int fsq_dequant_f32(const int32_t *idx, const int32_t *levels_host, int64_t nlev, float *zhat,
                    int64_t rows, void *stream);

/* ---- BSQQuantizer's train step (bsq.py:14-37, 64-133) in ONE forward and ONE backward call.
 *   x: [B, C, L] (layout 0, BCHW) or [B, L, C] (layout 1, BLC; also channels_last memory; there x, quantized, g_q and grad_x are
 *   16-byte aligned), C = 16 d, d = log2(codebook_size) in 1..16 (the reference packs exactly 16 codebooks); channel i d + j is
 *   codebook i, bit plane j.  Per position: n = ||x||_2 summed in fp64, u = fl32(x / max(n, 1e-12)), q = u > 0 ? 1 : -1 (the sign
 *   of the fp32 quotient), q_scale = fl32(1 / sqrt(C)), s = -400 u / sqrt(C), p = sigma(s) with e = exp(-|s|): the larger of
 *   (p, 1 - p) is 1 / (1 + e), the smaller e / (1 + e); eps = 1e-5; M = B L 16.
 * bsq_train_f32 writes
 *   quantized (layout of x) = fl(fl(u + fl(q - u)) q_scale);
 *   idx int64 [B, L, d] (BLC) / [B, d, L] (BCHW): idx[j] = sum_i bit(i, j) << (15 - i);
 *   avg [d][2] floats = the reference's avg_probs: (mean of p, mean of 1 - p) over the M entries of bit plane j, each summed on its
 *     own in fp64 and rounded once; kept by the caller for the backward;
 *   scalars [3] floats ON THE DEVICE = {entropy_aux_loss = w_s per_sample_entropy - w_b codebook_entropy, per_sample_entropy =
 *     (1 / M) sum (-p log(p + eps) - (1 - p) log(1 - p + eps)), codebook_entropy = -sum over avg of a log(a + eps)}.
 * bsq_backward_f32, with the gradients arriving at quantized (g_q, layout of x) and at entropy_aux_loss (ONE float ON THE DEVICE),
 * NULL = zero, writes grad_x (layout of x) from x and avg alone, in one launch:
 *     g_u = q_scale g_q + g_aux (-400 / sqrt(C)) p (1 - p) ((w_s / M) h'(p) - (w_b / M) A'_j),
 *     h'(p) = -log(p + eps) - p / (p + eps) + log(1 - p + eps) + (1 - p) / (1 - p + eps), A'_j the same at avg[j];
 *     grad_x = (g_u - u (u . g_u)) / n when n >= 1e-12, g_u / 1e-12 otherwise; fp64, rounded once.
 * The forward is two launches (per-block fp64 partial sums, one finishing block); no float atomics, every sum's order depends on the
 * shape alone: bit-identical from run to run.  Neither call reads the host or synchronises; both are ordered on `stream`.
 * workspace: bsq_train_workspace_bytes(B L, d) bytes (-1: rows < 0 or too many, d outside 1..16), 16-byte aligned, contents
 * don't-care on entry, nothing in it is kept between calls; NULL, misaligned or short -> GQHIP_ERR_WORKSPACE.  B L = 0: GQHIP_OK. */
int64_t bsq_train_workspace_bytes(int64_t rows, int64_t d);
int bsq_train_f32(const float *x, float *quantized, int64_t *idx, float *avg, float *scalars, int64_t B, int64_t L, int64_t C,
                  int64_t d, int layout, float w_s, float w_b, void *workspace, int64_t workspace_bytes, void *stream);
int bsq_backward_f32(const float *x, const float *avg, const float *g_q_or_null, const float *g_aux_or_null, float *grad_x,
                     int64_t B, int64_t L, int64_t C, int64_t d, int layout, float w_s, float w_b, void *workspace,
                     int64_t workspace_bytes, void *stream);

/* ---- FSQQuantizer's train step (fsq.py:6-9, 29-68) on a module layout in place: z, zhat, g_zhat, grad_z are [B, nlev, L] (layout 0)
 * or [B, L, nlev] (layout 1); idx int32 [B L] (one packed index per position).  levels_host as in fsq_quantize_f32 (every level >= 2).
 * fsq_train_f32: b as in fsq_quantize_f32, r = rint(b), zhat = fl(fl(b + fl(r - b)) / half_width) (round_ste's value), idx = the
 * pack of r + half_width.  fsq_backward_f32: grad_z = g_zhat (half_l / half_width) sech^2(z + shift), sech^2 t = 4 e / (1 + e)^2 with
 * e = exp(-2 |t|), in fp64, rounded once.  One launch each, no workspace.  B L = 0: GQHIP_OK. */
int fsq_train_f32(const float *z, const int32_t *levels_host, int64_t nlev, float *zhat, int32_t *idx, int64_t B, int64_t L,
                  int layout, void *stream);
int fsq_backward_f32(const float *z, const float *g_zhat, const int32_t *levels_host, int64_t nlev, float *grad_z, int64_t B,
                     int64_t L, int layout, void *stream);

/* ---- the LPIPS comparison head (pit/modules/lpips/loss/lpips.py:46-66: normalize_tensor, squared difference, the `lin` layer's
 * dropout and 1x1 convolution, spatial_average) of one VGG level, forward and backward, on a module layout in place (csrc/lpips_head.h).
 *   f0, f1, grad_f1: [B, C, HW] (layout 0, BCHW) or [B, HW, C] (layout 1, BLC; also channels_last memory), 1 <= C <= 512, HW >= 1,
 *   B HW < 2^30; w [C]; keep: NULL, or one byte (0 / 1) per feature element in the features' layout, with keep_scale = 1 / (1 - p)
 *   (m_c s below; 1 without a mask).  Per pixel, over the channels, in fp64 and rounded once:
 *     n0 = sqrt(sum f0_c^2), n1 = sqrt(sum f1_c^2), r0 = 1 / (n0 + 1e-10), r1 = 1 / (n1 + 1e-10), u_c = f0_c r0 - f1_c r1,
 *     out[b] = (1 / HW) sum_p sum_c w_c (m_c s) u_c^2;
 *     t_c = -2 w_c (m_c s) u_c, dot = sum_c t_c f1_c, grad_f1_j = (g_out[b] / HW) (r1 t_j - f1_j dot r1^2 / n1);
 *   at n1 = 0 the second term is 0 (its limit; torch's autograd gives NaN there).  The head is symmetric: the gradient for f0 is the
 *   same call with f0 and f1 swapped.  16-byte aligned pointers (keep: 4-byte) take 16-byte accesses; 4-byte alignment is required.
 * The forward is two launches (per-tile fp64 partial sums, one finishing block per image), the backward one; no float atomics, every
 * sum's order depends on the shape alone: bit-identical from run to run.  Neither reads the host or synchronises.
 * workspace (forward): lpips_head_workspace_bytes(B, C, HW) bytes (-1: a size outside the limits above), 16-byte aligned, contents
 * don't-care on entry, nothing kept between calls; NULL, misaligned or short -> GQHIP_ERR_WORKSPACE.  B = 0: GQHIP_OK. */
int64_t lpips_head_workspace_bytes(int64_t B, int64_t C, int64_t HW);
int lpips_head_f32(const float *f0, const float *f1, const float *w, const uint8_t *keep_or_null, float keep_scale, float *out,
                   int64_t B, int64_t C, int64_t HW, int layout, void *workspace, int64_t workspace_bytes, void *stream);
int lpips_head_backward_f32(const float *f0, const float *f1, const float *w, const uint8_t *keep_or_null, float keep_scale,
                            const float *g_out, float *grad_f1, int64_t B, int64_t C, int64_t HW, int layout, void *stream);

/* ---- raw first and second moments of a feature block, accumulated in fp64 (csrc/gq_moments.h): what the Frechet statistics of
 * eval.py:186-203, 241-257 need, without a feature row leaving the device.
 *   state: (D D + D + 1) fp64 words = [ outer: D D, row-major | sum: D | count: 1 ]; gq_moments_state_bytes(D) bytes (-1 for a D
 *   outside 1 .. 8192).  The caller zeroes it once; each call adds to it.
 *   x: [rows, D] fp32, row r at x + r row_stride, row_stride >= D.  For r = 0 .. rows - 1, IN ASCENDING r:
 *     outer[i][j] <- fma((double)x[r][i], (double)x[r][j], outer[i][j])   for j >= i
 *     sum[i]      <- sum[i] + (double)x[r][i]
 *   and count <- count + rows (a double: exact to 2^53).  Only the upper triangle (j >= i) of outer is defined; what it holds
 *   below the diagonal is unspecified.
 *   The product of two fp32 values has at most 48 significant bits and its exponent lies far inside fp64's range even for two fp32
 *   subnormals, so it is exact in fp64 and every step is one rounding of outer + product.  Hence: a plain sequential fp64 loop on
 *   the host reproduces every bit; splitting the rows over several calls changes no bit; a * b + c and fma(a, b, c) agree.
 *   Limits: 1 <= D <= 8192, rows >= 0, rows row_stride < 2^31; x 4-byte and state 8-byte aligned, neither NULL; anything else is
 *   GQHIP_ERR_INVALID_ARG.  rows == 0: GQHIP_OK, nothing is launched.  x 16-byte aligned with row_stride % 4 == 0 takes 16-byte
 *   loads, a 16-byte aligned state with an even D 16-byte accesses; the bits are the same either way.
 * One launch over the tile pairs of the upper triangle; every output element has one owning thread, no atomics of any kind, no
 * workspace, no host read: asynchronous and graph-capturable. */
int64_t gq_moments_state_bytes(int64_t D);
int gq_moments_update_f32(const float *x, int64_t rows, int64_t D, int64_t row_stride, double *state, void *stream);

/* ---- fused GroupNorm (+ SiLU) for the conv stack -----------------------------------
 * y = act( (x - mean_g) * rstd_g * gamma_c + beta_c ), act = SiLU when apply_silu != 0.
 * Replaces the GroupNorm -> swish pairs of pit/modules/unet.py:54-57,49-51,137-153,432-435
 * (three PyTorch kernels, five HBM passes) by a stats pass + one apply pass (three passes).
 * x, y [B, C, HW] fp32 contiguous (NCHW), groups | C; stats_ws: B*groups statistics records
 * (GQHIP_GNSTAT_WORDS int64 each) of caller scratch.  x and y may alias.  pre_bias_or_null [C]: a per-channel bias still pending
 * on x (the producing conv was run without its bias) -- normalises x + pre_bias[c] without a
 * separate bias pass. */
#define GQHIP_LAYOUT_NCHW 0   /* x[b][c][hw] */
#define GQHIP_LAYOUT_NHWC 1   /* x[b][hw][c] (torch channels_last): needs (C/groups) % 4 == 0, (C/4) | 256 */
int gn_silu_f32(const float *x, const float *gamma, const float *beta,
                const float *pre_bias_or_null, float *y, int64_t B, int64_t C, int64_t HW,
                int64_t groups, double eps, int apply_silu, int layout, gqhip_gnstat_t *stats_ws,
                void *stream);
/* y = a + b (+ bias[c]): residual add with the pending conv biases folded in (unet.py:153). */
int add_bias_f32(const float *a, const float *b, const float *bias_or_null, float *y, int64_t B,
                 int64_t C, int64_t HW, int layout, void *stream);

/* NHWC only.  y = a + b (+ bias[c]) AND the GroupNorm statistics of y: record b*groups+g of stats_out = sum and sum of
 * squares over the group (gqhip_gnstat_t records; zeroed here).  The residual add of a ResnetBlock / AttnBlock (unet.py:160, :205) is
 * always followed by a GroupNorm over the same tensor (unet.py:140, :190, :581): gn_apply_f32 then normalises from
 * these statistics without its own statistics pass.  Needs (C/groups) % 4 == 0, 256 % (C/4) == 0, groups <= 64. */
int add_bias_stats_f32(const float *a, const float *b, const float *bias_or_null, float *y, int64_t B,
                       int64_t C, int64_t HW, int64_t groups, gqhip_gnstat_t *stats_out, void *stream);

/* NHWC only.  The apply pass of gn_silu_f32 with statistics computed earlier (by add_bias_stats_f32). */
int gn_apply_f32(const float *x, const float *gamma, const float *beta, float *y, int64_t B, int64_t C,
                 int64_t HW, int64_t groups, double eps, int apply_silu, const gqhip_gnstat_t *stats, void *stream);

/* Content checksums of `count` device tensors in ONE launch: table_dev = count entries {const void *ptr; int64_t words}
 * (32-bit words; 16-byte aligned pointers), sums_dev[t] = a 64-bit position-salted hash sum of tensor t (zeroed here; integer
 * atomics: independent of the order of the adds).  The conv-stack modules use it to notice parameter writes that bump no
 * version counter (`param.data`): their weight-derived caches are rebuilt when a sum differs (pit_hip/modules/unet.py). */
int gqhip_checksum_tensors(const void *table_dev, int64_t count, uint64_t *sums_dev, void *stream);

/* Every entry point that FILLS GroupNorm statistics records zeroes them first (one small memset launch each).  A caller that hands
 * out records which are already zero -- e.g. slices of one arena cleared by a single fill per forward, as pit_hip/modules/unet.py
 * does -- says so with gqhip_stats_prezeroed(1) around those calls; (0) restores the default.  Thread-local.  (ABI 6; no reference
 * counterpart.) */
int gqhip_stats_prezeroed(int on);

/* The encoder's conv_in (pit/modules/unet.py:411-413: 3 -> ch channels): a 3x3 / stride 1 / pad 1 convolution of a channels_last
 * image with Cin <= 4 input channels into Cout = 128 channels as fp32 FMAs in a FIXED order (tap-major, then input channel), + bias,
 * + the statistics of the result for the GroupNorm that follows (stats_out: B * 32 records, zeroed here; groups_out must be 32).
 * wk [9 Cin, 128]: wk[(tap * Cin + ci) * 128 + co] = weight[co][ci][tap / 3][tap % 3].  H % 8 == 0, W % 32 == 0.  Bit-reproducible;
 * replaces the last library convolution of the bench shapes (ABI 6). */
int conv3x3_cin_small_f32(const float *x, const float *wk, const float *bias_or_null, float *y, int64_t *stats_out_or_null,
                          int64_t B, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int64_t groups_out, void *stream);

/* 3x3 convolution, stride 1, zero padding 1, NHWC fp32, on the fp32 matrix cores (v_mfma_f32_32x32x2_f32: an exact fp32 FMA
 * chain) with a FIXED summation order, so the result is bit-identical from run to run -- for the narrow ends of the conv
 * stack, where the library's pick is a split-K kernel with floating-point atomics: the encoder's conv_out
 * (pit/modules/unet.py:425-436: norm_out -> swish -> conv 512 -> 2 z_channels, the layer that produces z) and the decoder's
 * conv_in (unet.py:487-489: z_channels -> 512).  stats != NULL: the input is act(GroupNorm(x + pre_bias)) applied while the
 * patch is staged (gamma, beta [Cin]; stats = B * groups_in records; Cin <= 1024); act = SiLU when apply_silu != 0.
 * wk: the weights in operand order [ceil(Cout/32)][9 taps][Cin/8][64 lanes][4]: element (t, tap, g, 32 h + j, m) =
 * w[32 t + j][8 g + 4 h + m][tap / 3][tap % 3], zero for output channels >= Cout.  Any H, W (a block owns 32 pixels of a row); Cout % 4 == 0;
 * Cin % 64 == 0 (K split over the four waves of a block, partial sums added in wave order) or, without GroupNorm,
 * Cin in {8, 16, 32} (output channels split over the waves). */
int conv3x3_f32(const float *x, const float *gamma_or_null, const float *beta_or_null, const float *pre_bias_or_null,
                const gqhip_gnstat_t *stats_or_null, int64_t groups_in, double eps, int apply_silu, const float *wk,
                const float *bias_or_null, float *y, int64_t B, int64_t H, int64_t W, int64_t Cin, int64_t Cout, void *stream);

/* Nearest-neighbour x2 upsample of an NHWC fp32 tensor: x [B, H, W, C] -> y [B, 2H, 2W, C], C % 4 == 0
 * (pit/modules/unet.py:69-73, `F.interpolate(scale_factor=2.0, mode="nearest")` in channels_last). */
int upsample2x_nhwc_f32(const float *x, float *y, int64_t B, int64_t H, int64_t W, int64_t C,
                        void *stream);

/* Winograd F(2x2, 3x3) data transforms for a stride-1, padding-1 3x3 convolution of an NHWC tensor (the decoder's wide
 * ResnetBlock convolutions, pit/modules/unet.py:142, :149): V [16, tiles, C] = B^T d B of every 4x4 input tile
 * (tiles = B * H/2 * W/2, H and W even); after the 16 GEMMs M[k] = V[k] x U[k] (U = G g G^T, [16, Cin, Cout]) the
 * output transform writes y [B, H, W, Cout] = A^T M A.  16 instead of 36 multiplies per 2x2 outputs. */
int wino_in_nhwc_f32(const float *x, float *V, int64_t B, int64_t H, int64_t W, int64_t C, void *stream);
/* `mscale` (all three output transforms): y = mscale * (A^T M A) (+ bias, + res): 1 for fp32 operands, the inverse of
 * the operands' power-of-two scales behind wino_in_nhwc_f16x3. */
int wino_out_nhwc_f32(const float *M, float *y, int64_t B, int64_t H, int64_t W, int64_t C, float mscale, void *stream);

/* The input transforms (tile = 2: F(2x2,3x3), 4: F(4x4,3x3)) writing the operand of ONE fp16 GEMM with fp32 accumulation
 * whose K axis carries the three products of two-term fp16 splits: V3 [16|36, tiles, 3C] fp16 = [h | h | l] of
 * (B^T d B) * scale, to be multiplied by U3 [16|36, 3C, Cout] fp16 = [U_h ; U_l ; U_h]: the products h U_h + h U_l + l U_h
 * carry 22-bit operands (error 2.5-2.9e-7 of sum |a||b| measured -- the level of hipBLASLt's own fp32 GEMM, which is a
 * split-bf16 emulation on gfx950 -- at 1.2-2.5x its speed).  `scale`: a power of two with |V| * scale < 65504 (the
 * caller derives it from the GroupNorm that feeds the convolution: |SiLU(GN(x))| <= sqrt(n - 1) max|gamma| + max|beta|). */
int wino_in_nhwc_f16x3(const float *x, void *V3, int64_t B, int64_t H, int64_t W, int64_t C, int tile, float scale,
                       void *stream);
/* ... as V2 [16|36, tiles, 2C] fp16 = [h | l] only (4 instead of 6 bytes per element): the operand of wino_gemm_f16x2, which
 * forms the three products itself. */
int wino_in_nhwc_f16x2(const float *x, void *V2, int64_t B, int64_t H, int64_t W, int64_t C, int tile, float scale,
                       void *stream);
/* The wider levels (Cin % 32 == 0, Cout % 128 == 0, tiles % 256 == 0; the SD3-UNet's 256- and 512-channel convolutions,
 * reference pit/modules/unet.py:142, :149): M [P, tiles, Cout] fp32 = V2 (x) U with Wf [P, Cin/16, Cout/32, 2, 64, 8] fp16 =
 * (U_h, U_l) of U * u_scale in MFMA operand order (lane (c, h) of column tile nt holds k = 16 chunk + 8 h .. + 7 of column
 * 32 nt + c).  Replaces the hipBLASLt GEMM over K' = 3 Cin of V3 = [h | h | l]: same splits, same three products, fp32
 * accumulation; a third less traffic on V. */
int wino_gemm_f16x2(const void *V2, const void *Wf, float *M, int64_t P, int64_t tiles, int64_t Cin, int64_t Cout,
                    void *stream);
/* Direct 3x3 convolution (stride 1, zero padding 1) Cin -> Cout (128 or 256) channels, channels_last, as an implicit
 * GEMM on the fp16 matrix cores with the fp16 x 3 scheme above (two-term splits of both operands, three products, fp32
 * accumulation): the convolutions of the 256 x 256 level and the encoder's 128 x 128 level (reference pit/modules/unet.py:142,
 * :149), where the Winograd routes are HBM-bound on V and M.  Replaces F.conv2d(swish(norm(x)), w, None, 1, 1) + bias +
 * residual (unet.py:140-153).
 *   conv3x3_gn_f16x3     y [B, H, W, Cout] = (SiLU(GroupNorm(x + pre_bias)) (*) w) + bias (+ res) in ONE kernel: x [B, H, W, Cin]
 *                        fp32 is normalised, activated, scaled and split on its way into LDS.  stats_in [B, groups_in, 2] as
 *                        gn_stats_f32 / the statistics outputs of this library; stats_out (optional): GroupNorm statistics of
 *                        y, [B, groups_out] statistics records (4 | Cout / groups_out | 128).  H % 8 == 0, W % 32 == 0, Cin % 32 == 0,
 *                        Cin <= 512.  `scale`: a power of two with |activation| * scale <= 32768; mscale = 1 / (scale * u_scale).
 *                        Wf [Cin/16, 9, Cout/32, 2, 64, 8] fp16: operand-order weights -- chunk, tap ky*3+kx, column tile,
 *                        plane (h, l of w * u_scale), lane (n = 32 tile + lane%32, k-half lane/32), 8 input channels
 *                        16 chunk + 8 (lane/32) + e.
 */
int conv3x3_gn_f16x3(const float *x, const float *gamma, const float *beta, const float *pre_bias_or_null,
                     const gqhip_gnstat_t *stats_in, int64_t groups_in, double eps, int apply_silu, float scale, const void *Wf,
                     const float *bias_or_null, const float *res_or_null, float *y, gqhip_gnstat_t *stats_out_or_null, int64_t B,
                     int64_t H, int64_t W, int64_t Cin, int64_t Cout, int64_t groups_out, float mscale, void *stream);
/* 1x1 convolution Cin -> Cout (128, 256, 512 or 1536 = the attention block's q | k | v) of a channels_last tensor = a GEMM over its B * HW pixels, fp16 x 3 as above
 * with the split of x done inside the kernel: the ResnetBlocks' nin_shortcut (reference pit/modules/unet.py:151-152) and the
 * attention block's proj_out (:203).  x [B * HW, Cin] fp32 (NOT normalised; + pre_bias[c], a bias still pending on it); the
 * power-of-two scale of x + pre_bias comes from
 * scales_dev = {scale, 1 / (scale * u_scale)} in device memory (f16_scales_from_gn_stats) or, when that is NULL, from the
 * `scale` / `mscale` arguments.  Wf [Cin/16, 1, Cout/32, 2, 64, 8] as for conv3x3_gn_f16x3; y = x W * mscale + bias (+ res);
 * stats_out optional.  HW % 128 == 0, Cin % 32 == 0.  Blocks are 256 pixels x 128 columns, or 128 x 128 where the 256-pixel
 * grid would leave the chip under-filled (fewer than two blocks per CU, or a last round less than 85 % full) or HW % 256 != 0;
 * the result does not depend on the tiling.  GQHIP_CONV1_TILE = 128 | 256 in the environment forces one (read per call; a
 * forced 256 at HW % 256 != 0 is GQHIP_ERR_INVALID_ARG). */
int conv1x1_f16x3(const float *x, const float *pre_bias_or_null, const void *Wf, const float *scales_dev_or_null, float scale,
                  float mscale, const float *bias_or_null, const float *res_or_null, float *y, gqhip_gnstat_t *stats_out_or_null, int64_t B, int64_t HW,
                  int64_t Cin, int64_t Cout, int64_t groups_out, void *stream);
/* conv1x1_f16x3 of GroupNorm(x + pre_bias) (no SiLU: the attention block's norm, reference pit/modules/unet.py:185-190) with
 * the normalisation applied while x is staged, as conv3x3_gn_f16x3 does: the normalised tensor is never written, and the
 * result is bit for bit that of gn_silu_f32(apply_silu = 0) followed by conv1x1_f16x3.  stats_in: the statistics of
 * x + pre_bias (gn_stats_f32 / a producer's stats_out); `scale` >= 1 / max|normalised tensor| as a power of two, host side
 * only.  Cin <= 512, (Cin / groups_in) % 4 == 0. */
int conv1x1_gn_f16x3(const float *x, const float *gamma, const float *beta, const float *pre_bias_or_null,
                     const gqhip_gnstat_t *stats_in, int64_t groups_in, double eps, const void *Wf, float scale, float mscale,
                     const float *bias_or_null, const float *res_or_null, float *y, gqhip_gnstat_t *stats_out_or_null, int64_t B,
                     int64_t HW, int64_t Cin, int64_t Cout, int64_t groups_out, void *stream);
/* The attention block's q | k | v projection C -> 3C (Wf [C/16, 1, 3C/32, 2, 64, 8]) writing the operands of the attention
 * GEMMs itself: Q3, K3, V3 are byte for byte what attn_split_qkv_f16x3(sq, sv) makes of the projection conv1x1_f16x3 (or,
 * with gamma / beta / stats_in given, conv1x1_gn_f16x3) would have stored, and that fp32 tensor is never written.
 * x [B * L, C]; C % 128 == 0 (a block's 128 columns lie inside q, k or v), L % 128 == 0; with GroupNorm C <= 512. */
int conv1x1_qkv_split_f16x3(const float *x, const float *gamma_or_null, const float *beta_or_null, const float *pre_bias_or_null,
                            const gqhip_gnstat_t *stats_in_or_null, int64_t groups_in, double eps, const void *Wf, float scale,
                            float mscale, const float *bias_or_null, void *Q3, void *K3, void *V3, float sq, float sv, int64_t B,
                            int64_t L, int64_t C, void *stream);
/* 3x3 convolution with stride 2 over x padded by one zero row / column at the bottom / right -- the reference's Downsample
 * (pit/modules/unet.py:76-97: F.pad(x, (0,1,0,1)) + conv stride 2) -- Cin -> Cout (128, 256 or 512), fp16 x 3 on the four
 * phase images of x (nine k-steps per 16 input channels).  x [B, Hin, Win, Cin] fp32 (not normalised; scale as for
 * conv1x1_f16x3), y [B, Hin/2, Win/2, Cout] = conv * mscale + bias; stats_out optional.  Hin % 16 == 0, Win % 64 == 0,
 * Cin % 16 == 0.  Wf [9 Cin/16, Cout/32, 2, 64, 8]: operand-order weights, k-steps in the order (phase (a, b) = (0,0), (0,1),
 * (1,0), (1,1); chunk; tap (dy, dx) of the phase, ky = 2 dy + a, kx = 2 dx + b). */
int conv3x3s2_f16x3(const float *x, const void *Wf, const float *scales_dev_or_null, float scale, float mscale,
                    const float *bias_or_null, float *y, gqhip_gnstat_t *stats_out_or_null, int64_t B, int64_t Hin, int64_t Win,
                    int64_t Cin, int64_t Cout, int64_t groups_out, void *stream);
/* The reference's Upsample (pit/modules/unet.py:60-73: nearest x2, then conv 3x3) Cin -> Cout (128, 256 or 512) as its sub-pixel
 * form computed directly: output phase (a, b) = a 2x2 convolution of the low-resolution input with the phase weights (sums of
 * the 3x3 taps landing on the same source pixel), fp16 x 3, one kernel: no patch matrix, no pixel-shuffle pass.
 * x [B, H, W, Cin] fp32 (not normalised; scale as for conv1x1_f16x3), y [B, 2H, 2W, Cout] = conv * mscale + bias; stats_out
 * optional (GroupNorm statistics of y).  H % 8 == 0, W % 32 == 0, Cin % 16 == 0.  Wf [4, 4 Cin/16, Cout/32, 2, 64, 8]:
 * operand-order phase weights, [phase 2a + b][chunk][tap 2u + v], tap (u, v) reading x[i - 1 + a + u][j - 1 + b + v]. */
int upconv2x_f16x3(const float *x, const void *Wf, const float *scales_dev_or_null, float scale, float mscale,
                   const float *bias_or_null, float *y, gqhip_gnstat_t *stats_out_or_null, int64_t B, int64_t H, int64_t W,
                   int64_t Cin, int64_t Cout, int64_t groups_out, void *stream);
/* 3x3 convolution (stride 1, zero padding 1) into 1..4 channels with GroupNorm (+ SiLU) of the input fused in, fp32 FMAs:
 * the decoder's conv_out(swish(norm_out(h))) (reference pit/modules/unet.py:585-587).  x [B, H, W, Cin] fp32, w_ohwi
 * [Cout, 3, 3, Cin] fp32, y [B, H, W, Cout].  H % 16 == 0, W % 16 == 0, Cin % 32 == 0, Cin <= 512. */
int conv3x3_gn_small_f32(const float *x, const float *gamma, const float *beta, const float *pre_bias_or_null,
                         const gqhip_gnstat_t *stats_in, int64_t groups_in, double eps, int apply_silu, const float *w_ohwi,
                         const float *bias_or_null, float *y, int64_t B, int64_t H, int64_t W, int64_t Cin, int64_t Cout,
                         void *stream);
/* ... with the producer fused in (as wino_in_gn_nhwc_f32 / wino4_in_gn_nhwc_f32): the convolution's input is
 * SiLU(GroupNorm(x + pre_bias)), never written. */
int wino_in_gn_nhwc_f16x3(const float *x, const float *gamma, const float *beta, const float *pre_bias_or_null,
                          const gqhip_gnstat_t *stats, void *V3, int64_t B, int64_t H, int64_t W, int64_t C, int64_t groups,
                          double eps, int apply_silu, int tile, float scale, void *stream);
/* ... writing the [h | l] operand of wino_gemm_f16x2. */
int wino_in_gn_nhwc_f16x2(const float *x, const float *gamma, const float *beta, const float *pre_bias_or_null,
                          const gqhip_gnstat_t *stats, void *V2, int64_t B, int64_t H, int64_t W, int64_t C, int64_t groups,
                          double eps, int apply_silu, int tile, float scale, void *stream);

/* Winograd F(4x4, 3x3): V [36, tiles, C] of the 6x6 input tiles (tiles = B * H/4 * W/4, H and W multiples of 4) and
 * y [B, H, W, Cout] from M [36, tiles, Cout]; U = G g G^T is [36, Cin, Cout].  36 multiplies per 16 outputs and 2.25x
 * (instead of 4x) the activation in V / M, at ~10x the rounding error of F(2x2,3x3): the decoder's convolutions. */
int wino4_in_nhwc_f32(const float *x, float *V, int64_t B, int64_t H, int64_t W, int64_t C, void *stream);
int wino4_out_nhwc_f32(const float *M, float *y, int64_t B, int64_t H, int64_t W, int64_t C, float mscale, void *stream);

/* Output transform (tile = 2: F(2x2,3x3), M [16, tiles, C]; tile = 4: F(4x4,3x3), M [36, tiles, C]) with the ResnetBlock's
 * tail fused in (pit/modules/unet.py:149-153): y = A^T M A + bias[c] (+ res, may be NULL), plus the GroupNorm statistics of y
 * (stats_out as add_bias_stats_f32) for the block that follows.  Needs (C/groups) % 4 == 0, 256 % (C/4) == 0. */
int wino_out_res_nhwc_f32(const float *M, const float *res, const float *bias_or_null, float *y, gqhip_gnstat_t *stats_out,
                          int64_t B, int64_t H, int64_t W, int64_t C, int64_t groups, int tile, float mscale,
                          void *stream);

/* NHWC only.  GroupNorm statistics alone (the first pass of gn_silu_f32): stats_out[2*(b*groups+g)] = sum, [+1] = sum of
 * squares of x (+ pre_bias[c]) over the group (gqhip_gnstat_t records), zeroed here. */
int gn_stats_f32(const float *x, const float *pre_bias_or_null, int64_t B, int64_t C, int64_t HW, int64_t groups,
                 gqhip_gnstat_t *stats_out, void *stream);

/* wino_in_nhwc_f32 with the producer fused in: the convolution's input is SiLU(GroupNorm(x + pre_bias)) (the
 * `Normalize` -> `nonlinearity` -> conv chains of pit/modules/unet.py:140-142, :146-149); the normalised tensor is
 * never written.  `stats` as produced by gn_stats_f32 / add_bias_stats_f32. */
int wino_in_gn_nhwc_f32(const float *x, const float *gamma, const float *beta, const float *pre_bias_or_null,
                        const gqhip_gnstat_t *stats, float *V, int64_t B, int64_t H, int64_t W, int64_t C,
                        int64_t groups, double eps, int apply_silu, void *stream);
/* the same for F(4x4,3x3) (V [36, tiles, C], H and W multiples of 4) */
int wino4_in_gn_nhwc_f32(const float *x, const float *gamma, const float *beta, const float *pre_bias_or_null,
                         const gqhip_gnstat_t *stats, float *V, int64_t B, int64_t H, int64_t W, int64_t C,
                         int64_t groups, double eps, int apply_silu, void *stream);

/* Single-head attention softmax(q k^T C^-1/2) v (reference pit/modules/unet.py:185-206: F.scaled_dot_product_attention on
 * [B, 1, L, C]) as two fp16 GEMMs with fp32 accumulation over K axes of two-term fp16 splits, fp32 results:
 *   attn_split_qkv_f16x3   qkv [B, L, 3C] fp32 (q | k | v per token) -> Q3 [B, L, 3C] = [q_h | q_h | q_l] of q * sq,
 *                          K3 [B, L, 3C] = [k_h | k_l | k_h] of k * sq, V3 [B, 3L, C] = [v_h ; v_l ; v_h] of v * sv
 *                          (sq, sv: powers of two keeping the operands inside fp16's range; C % 4 == 0);
 *   attn_softmax_split_f16x3  S' [rows, L] fp32 (= Q3 K3^T = sq^2 q k^T) -> P3 [rows, 3L] = [p_h | p_h | p_l] of
 *                          softmax(S' * factor) * 2^14, factor = C^-1/2 / sq^2; L % 64 == 0, L <= 4096.
 * The caller multiplies Q3 K3^T and P3 V3 (library fp16 GEMMs, fp32 out) and scales the result by 1 / (2^14 sv). */
int attn_split_qkv_f16x3(const float *qkv, void *Q3, void *K3, void *V3, int64_t B, int64_t L, int64_t C, float sq, float sv,
                         void *stream);
int attn_softmax_split_f16x3(const float *S, void *P3, int64_t rows, int64_t L, float factor, void *stream);
int f16_scales_from_gn_stats(const gqhip_gnstat_t *stats, int64_t n_bg, double amp, double u_scale, float *scales_out,
                             void *stream);

/* ---- index wire format / usage histogram ----------------------------------- */
int gq_index_histogram(const int64_t *idx, int64_t count, int64_t n,
                       int32_t *hist, void *stream);
int gq_indices_to_u16(const int64_t *idx, uint16_t *out, int64_t count,
                      void *stream);
int gq_indices_from_u16(const uint16_t *in, int64_t *idx, int64_t count,
                        void *stream);

/* One rank's per-step record in ONE launch -- what eval.py:165-169 (per-image PSNR: pit/evaluations/psnr.py:17-28 with
 * zero_mean = True, images in [-1, 1]) and eval.py:152-154 (the batch's code indices) publish per batch, in the packed wire
 * format of pit_hip/eval_dist.py:StepRecord with one metric:
 *     rec [B + (n_idx + 1) / 2] int32 = [ B PSNRs as fp32 bits | indices as uint16 pairs, low half first (odd count: zero pad) ].
 * x, x_rec: B images of `per_image` floats each in the SAME dense layout (NCHW or channels_last: the metric is elementwise);
 * idx: n_idx values in [0, 65536) (not checked; a wider value is truncated to its low 16 bits).  The squared differences are
 * formed in the reference's fp32 op order and summed in fp64 in a fixed order (bit-reproducible; within 2e-6 of torch's fp32
 * mean).  workspace: gq_step_record_workspace_bytes(B, per_image) bytes, ZERO when first used; every call leaves it zero
 * again -- every byte of it: the thread that finishes an image stores zeros over the partial sums it has added and over the
 * image's ticket --, so one allocation serves a stream of calls (one stream at a time) of ANY (B, per_image) whose byte count it
 * holds: the short last batch of an epoch runs in the buffer that was sized for the full one.  Bytes beyond the call's own
 * gq_step_record_workspace_bytes are neither read nor written.  Asynchronous on `stream`, no allocation. */
int64_t gq_step_record_workspace_bytes(int64_t B, int64_t per_image);
int gq_step_record_f32(const float *x, const float *x_rec, const int64_t *idx, int32_t *rec, int64_t B, int64_t per_image,
                       int64_t n_idx, void *workspace_zeroed, int64_t workspace_bytes, void *stream);

/* Per-image SSIM and MS-SSIM -- pit/evaluations/ssim.py:5-63 (get_ssim / get_ssim_and_msssim: pytorch_msssim's ssim / ms_ssim
 * with data_range 255, size_average False, the 11-tap sigma-1.5 Gaussian window, K = (0.01, 0.03), MS-SSIM weights
 * (0.0448, 0.2856, 0.3001, 0.2363, 0.1333) over five scales joined by avg_pool2d(2, 2, padding = side % 2)).
 * x, x_rec: B images [B, C, H, W], fp32, NCHW (layout 0) or NHWC / channels_last (layout 1), both the same layout; zero_mean != 0:
 * images in [-1, 1] scaled by (x + 1) 127.5, else by x 255, in fp32 like the reference; the window and the maps in fp64 from there
 * (csrc/gq_ssim.h).  A side under 11 is left unfiltered, as pytorch_msssim does.  ssim_out_or_null / msssim_out_or_null: B fp32
 * values each; a NULL msssim_out skips levels 1-4; when H < 256 or W < 256 MS-SSIM is NaN (ssim.py:31-34).  One launch per level,
 * sums in a fixed order: bit-reproducible.  workspace: gq_ssim_workspace_bytes(B, C, H, W) bytes, ZERO when first used; every
 * call leaves it zero again -- every byte of it: tickets and tile sums are zeroed by the block that finishes an image, and a call
 * that ran levels 1-4 ends with one more launch that clears the pooled planes --, so one allocation serves a stream of calls (one
 * stream at a time) of ANY (B, C, H, W) whose byte count it holds.  Bytes beyond the call's own gq_ssim_workspace_bytes are neither
 * read nor written.  Asynchronous on `stream`, no allocation: graph-capturable. */
int64_t gq_ssim_workspace_bytes(int64_t B, int64_t C, int64_t H, int64_t W);
int gq_ssim_f32(const float *x, const float *x_rec, int64_t B, int64_t C, int64_t H, int64_t W, int layout, int zero_mean,
                float *ssim_out_or_null, float *msssim_out_or_null, void *workspace_zeroed, int64_t workspace_bytes, void *stream);
/* The three-metric step record -- eval.py:152-154,165-178 (indices, PSNR, SSIM, MS-SSIM with zero_mean = True) in the wire
 * format of pit_hip/eval_dist.py:StepRecord with n_metrics = 3:
 *     rec [3 B + (n_idx + 1) / 2] int32 = [ B x (psnr, ssim, ms_ssim) as fp32 bits, image-major | indices as uint16 pairs ].
 * The PSNR words and the index words come from the kernel of gq_step_record_f32 (bit-identical to it), SSIM / MS-SSIM from that
 * of gq_ssim_f32.  workspace: gq_step_record_ssim_workspace_bytes(B, C, H, W) bytes, ZERO when first used, left zero: every byte, as
 * by the two calls it is made of, so one allocation serves any stream of shapes that fit. */
int64_t gq_step_record_ssim_workspace_bytes(int64_t B, int64_t C, int64_t H, int64_t W);
int gq_step_record_ssim_f32(const float *x, const float *x_rec, const int64_t *idx, int32_t *rec, int64_t B, int64_t C, int64_t H,
                            int64_t W, int layout, int64_t n_idx, void *workspace_zeroed, int64_t workspace_bytes, void *stream);

/* ---- the bit-packed index wire format: any codebook size up to 2^32 ---------
 * Index k -- its low w = index_bits bits (1 <= w <= 32), the value taken as unsigned 32-bit -- occupies bits [k w, (k + 1) w) of a
 * little-endian bit stream laid over int32 words: stream bit p is bit p mod 32 of word p div 32, and the stream is zero-padded to
 * a whole word, ceil(count w / 32) words.  An index straddles two words when 32 % w != 0.  w = 16 is exactly the "uint16 pairs,
 * low half first" format above.  n_codes (1 <= n_codes <= 2^w, else GQHIP_ERR_INVALID_ARG) is the codebook size: an index outside
 * [0, n_codes) is a VIOLATION -- it is packed as its low w bits and counted.  Every word is written by one thread with a plain
 * store, from indices read with coalesced loads through LDS (csrc/gq_aux.h); the counts are summed per block and added with one
 * integer atomic per block.  All calls here are asynchronous on `stream`, allocate nothing and are graph-capturable.
 *
 * gq_indices_pack_bits: words[ceil(count w / 32)] <- idx[count]; violations_or_null: one int32 that receives the number of
 *   violations, saturated at 2^31 - 1 (zeroed in-stream by the call, then added to).
 * gq_indices_unpack_bits: n_records packed fields of `count` indices each, field r at records + r stride_words + offset_words
 *   (stride_words - offset_words >= ceil(count w / 32)) -> idx[n_records, count], each value in [0, 2^w).  One field: n_records 1.
 * gq_index_histogram_packed: hist[v] += 1 (int64 hist[n]; it ADDS: a running histogram over many calls, zeroed by the caller)
 *   for every value v < n of the same fields, read from the packed words -- no int64 indices are formed; values >= n are skipped.
 *   Integer atomics only: the result is exact whatever the order. */
int gq_indices_pack_bits(const int64_t *idx, int32_t *words, int64_t count, int index_bits, int64_t n_codes,
                         int32_t *violations_or_null, void *stream);
int gq_indices_unpack_bits(const int32_t *records, int64_t *idx, int64_t n_records, int64_t stride_words, int64_t offset_words,
                           int64_t count, int index_bits, void *stream);
int gq_index_histogram_packed(const int32_t *records, int64_t n_records, int64_t stride_words, int64_t offset_words, int64_t count,
                              int index_bits, int64_t n, int64_t *hist, void *stream);
/* The step records with bit-packed indices -- pit_hip/eval_dist.py:StepRecord(n_codes=...):
 *     rec [B m + ceil(n_idx w / 32) + 1] int32 = [ the metric words of gq_step_record_f32 (m = 1) / gq_step_record_ssim_f32 (m = 3),
 *                                                  from the same code, bit-identical | the packed index words | 1 violations word ].
 * The violations word is this record's number of indices outside [0, n_codes), saturated at 2^31 - 1, written with a plain store
 * by the last packing block (the per-block counts meet in the workspace: no atomics on the record); it is written when n_idx = 0
 * too.  workspace: gq_step_record_bits_workspace_bytes(B, per_image) / gq_step_record_ssim_bits_workspace_bytes(B, C, H, W) bytes
 * (8 more than the uint16 records need: the violations count and its ticket; required for every call), under the contract of
 * gq_step_record_f32: ZERO when first used, every byte left zero, any later shape whose byte count it holds. */
int64_t gq_step_record_bits_workspace_bytes(int64_t B, int64_t per_image);
int gq_step_record_bits_f32(const float *x, const float *x_rec, const int64_t *idx, int32_t *rec, int64_t B, int64_t per_image,
                            int64_t n_idx, int index_bits, int64_t n_codes, void *workspace_zeroed, int64_t workspace_bytes,
                            void *stream);
int64_t gq_step_record_ssim_bits_workspace_bytes(int64_t B, int64_t C, int64_t H, int64_t W);
int gq_step_record_ssim_bits_f32(const float *x, const float *x_rec, const int64_t *idx, int32_t *rec, int64_t B, int64_t C, int64_t H,
                                 int64_t W, int layout, int64_t n_idx, int index_bits, int64_t n_codes, void *workspace_zeroed,
                                 int64_t workspace_bytes, void *stream);

/* Fused multi-head self-attention forward -- pit/modules/vit.py:142-151 (nn.MultiheadAttention(x, x, x, need_weights=False):
 * softmax(q k^T / sqrt(d)) v per (batch, head), no mask, no dropout; csrc/gq_attn.h).
 * qkv: [B, L, 3E] fp32, contiguous, 16-byte aligned: the in-projection output F.linear(x, in_proj_weight, in_proj_bias), read in
 * place -- q, k, v are its three E-wide column blocks, head h is columns h d .. h d + d - 1 of each.  out: [B, L, E] fp32 with the
 * heads concatenated (the operand of out_proj).  Head dim d = E / H: 64 is built (any other -> GQHIP_ERR_INVALID_ARG); any L >= 1;
 * B H <= 65535.  Precision: exact fp32 products on the fp32 matrix cores, fp32 online softmax; S and P never reach memory.
 * Fixed-order sums: bit-reproducible.  workspace: gq_mha_workspace_bytes(B, L, E, H) bytes (0 today: NULL is fine).
 * Asynchronous on `stream`, no allocation: graph-capturable. */
int64_t gq_mha_workspace_bytes(int64_t B, int64_t L, int64_t E, int64_t H);
int gq_mha_fwd_f32(const float *qkv, float *out, int64_t B, int64_t L, int64_t E, int64_t H, void *workspace, void *stream);
/* The same forward for training: it also stores lse [B, H, L] fp32 (4-byte aligned), per (batch, head, query row) the
 * log-sum-exp of the row's scores in the kernel's own units, lse2 = log2 sum_j exp2(s_ij log2(e)) with s = q k^T / sqrt(d)
 * (lse2 ln 2 is the natural log-sum-exp of s).  `out` is that of gq_mha_fwd_f32 bit for bit. */
int gq_mha_fwd_lse_f32(const float *qkv, float *out, float *lse, int64_t B, int64_t L, int64_t E, int64_t H, void *workspace,
                       void *stream);
/* Fused attention backward (csrc/gq_attn_bwd.h): from qkv, the forward's out and lse, and dout [B, L, E] (the gradient of out)
 * to dqkv [B, L, 3E], the gradient of qkv in qkv's layout (dq | dk | dv column blocks: what F.linear's backward takes as is).
 * P = exp2(s2 - lse2) is recomputed and divided by its own row sum (which takes out the rounding of lse2), dV = P^T dout,
 * dP = dout V^T, delta_i = sum_j P_ij dP_ij (in exact arithmetic sum_d dout_id out_id; taken from the kernels' own P and dP so that
 * dP - delta cancels on a peaked softmax as an explicit softmax backward does -- `out` is checked like the other tensors and not
 * read), dS = P o (dP - delta), dQ = dS K / sqrt(d), dK = dS^T Q / sqrt(d).  Same limits and checks as the forward: qkv, out, dout,
 * dqkv 16-byte aligned, lse and workspace 4-byte aligned, all non-NULL unless B == 0 or L == 0 (GQHIP_OK, nothing launched).
 * Every element of dqkv is written.  Exact fp32 products on the fp32 matrix cores, fixed-order fp32 sums, no atomics:
 * bit-reproducible.  workspace: gq_mha_bwd_workspace_bytes(B, L, E, H) bytes (two row sums: 2 B H L floats, rounded up), contents
 * irrelevant.  Two kernels on `stream`, asynchronous, no allocation: graph-capturable. */
int64_t gq_mha_bwd_workspace_bytes(int64_t B, int64_t L, int64_t E, int64_t H);
int gq_mha_bwd_f32(const float *qkv, const float *out, const float *lse, const float *dout, float *dqkv, int64_t B, int64_t L,
                   int64_t E, int64_t H, void *workspace, void *stream);

/* ---- profiling recorder ------------------------------------------------------
 * When enabled, every launch of the MFMA filter kernel is bracketed with
 * hipEvents on its own stream.  gqhip_profile_collect synchronises those
 * events and returns the number of launches and their total/avg milliseconds;
 * it resets the recorder.  Disabled by default (zero overhead). */
int gqhip_profile_enable(int on);
/* Pre-create `pairs` event pairs (outside any timed region): profiled launches only take events from this pool, a
 * launch that finds it empty is not recorded; collected events return to the pool. */
int gqhip_profile_reserve(int pairs);
int gqhip_profile_collect(int *launches_host, double *total_ms_host);

/* Diagnostics of the last fused call on `workspace` (device-side counters,
 * copied out synchronously): rows sent to the exhaustive fallback and total
 * half-tiles re-ranked.  For tests / DESIGN.md statistics only.  After a dims 1..3 search call (gqhip_set_low_dims) the first
 * word is the number of rows its finish launch took, the second (with gqhip_debug_enable(1)) the codes scored exactly. */
/* on != 0: the re-rank kernel also counts re-ranked half-tiles (adds one
 * contended atomic per row -- keep off when timing). */
int gqhip_debug_enable(int on);
int gqhip_debug_counters(const void *workspace, int64_t *fallback_rows_host,
                         int64_t *reranked_halftiles_host);
/* Grid search (dim 4 with a codebook cache), last call on `workspace`, synchronous copy: out4 = { sub-leaves visited summed
 * over the rows (counted only after gqhip_debug_enable(1); a sub-leaf is ~n / 4096 codes, a whole leaf counts four), codes that
 * received the reference's arithmetic (likewise; a row with ONE code within the margin needs none), rows handed to
 * gq_grid_finish_kernel, 1 if `cb_cache_or_null` holds a current index / 0 if not / -1 without a cache }. */
int gqhip_debug_grid(const void *workspace, const void *cb_cache_or_null, int64_t *out4_host);
#ifdef __cplusplus
}
#endif
#endif /* GQHIP_H_ */
