// gq_index.h -- what the pruned searches (gq_grid.h: dims 4 / 8; gq_lowdim.h: dims 1-3) share around their search loops: the header
// and the validation protocol of the codebook cache, the one-block builder of a 4096-bucket codebook index, and the DPP row
// reduction of both searches.
//
// Cache protocol.  The index lives in a caller-owned, persistent buffer (gqhip_cb_cache_bytes) and is validated on EVERY call:
//   * the call's first launch hashes the codebook the caller passes, slice by slice, while it reduces max|cb| (cb_hash_block), and
//     marks the cache `stale` when a slice's hash is not the one the index was built from;
//   * the builder, the next launch, exits when the index is current (index_current: magic, n, dim, not stale) and otherwise rebuilds
//     it from that very codebook and stamps it (index_stamp) -- the hashes first, a fence, then the words index_current reads, so a
//     stamp never becomes visible before the body it vouches for.
// A codebook edited in place by any route is seen by the very next call; a fresh or clobbered buffer costs one rebuild.
//
// Builder.  One block of NT threads, six steps: (1) index_moments: per-axis fp64 sums -> the owner's thresholds (any ascending
// thresholds are valid; the owners put them at normal quantiles of the book's own mean and deviation); (2) index_histogram_census:
// bucket sizes in LDS and the fullest bucket into GridHdr::max_sub; (3) index_scan4096: bucket starts; (4) index_scatter: codes and
// their original indices into bucket order; (5) index_tight_boxes, index_merge_boxes: [lo | hi] per bucket, parents as the union of
// their children; (6) index_stamp.  The owners keep their layouts, thresholds and the function that maps a code to its bucket.
#pragma once
#include "gq_common.h"
#include "gq_rerank.h"

namespace gqhip {

constexpr int kIndexBuckets = 4096;                // buckets of either index (gq_grid.h: sub-leaves; gq_lowdim.h: cells)

struct GridHdr {                                   // first 4 KiB of the codebook cache
  unsigned magic;
  int n, dim;
  int stale;                                       // set by the first launch when the codebook's hash differs; cleared by the builder
  int max_sub;                                     // the builder's census: codes in the fullest bucket (beyond the route's cap the search hands every row
                                                   // that lists it to its finish launch -- a degenerate book; hosts read it through gqhip_cb_cache_degenerate)
  int pad0[11];
  float thr[8][8];                                 // gq_grid.h, per axis: the (cells - 1) ascending thresholds of its coordinate, rest +inf
  unsigned long long blk_sum[kAbsmaxParts];        // hash of the codebook slice of code block k when the index was built
  int pad1[432];
};
static_assert(sizeof(GridHdr) == 4096, "cache header is 4 KiB");

__host__ __device__ inline int64_t grid_align(int64_t v) { return (v + 255) / 256 * 256; }

// the index in this cache was built for (n, dim) by the route of `magic`, from the bytes the codebook still has
__host__ __device__ inline bool index_current(const GridHdr *h, unsigned magic, int n, int dim) {
  return h->magic == magic && h->n == n && h->dim == dim && h->stale == 0;
}

// ---------------------------------------------------------------------------------------------------- codebook hash (256-thread blocks)
// The end of a code block: max |cb| and the content hash of the block's slice, reduced over its four waves, into the workspace header,
// and the cache's `stale` word set when the slice's hash differs from the one the index was built from.
__device__ __forceinline__ void cb_hash_store(float amax, unsigned long long hsum, int block, int tid, WsHeader *hdr,
                                              const unsigned long long *cache_sums, int *cache_stale) {
  __shared__ float s_amax[4];
  __shared__ unsigned long long s_hsum[4];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    amax = __builtin_fmaxf(amax, __shfl_xor(amax, o));
    hsum += __shfl_xor(hsum, o);
  }
  if ((tid & 63) == 0) { s_amax[tid >> 6] = amax; s_hsum[tid >> 6] = hsum; }
  __syncthreads();
  if (tid == 0) {
    hdr->absmax_part[block] = __builtin_fmaxf(__builtin_fmaxf(s_amax[0], s_amax[1]), __builtin_fmaxf(s_amax[2], s_amax[3]));
    const unsigned long long h = s_hsum[0] + s_hsum[1] + s_hsum[2] + s_hsum[3];
    hdr->cbsum[block] = h;
    // built from other bytes -> rebuilt, by the one-block kernel that follows, before its use
    if (cache_sums && cache_stale && cache_sums[block] != h) *cache_stale = 1;
  }
}
// A code block of a call that builds no operand image: slice `block` of `nblocks` of the codebook's `count` words (NaN reads as +inf)
__device__ __forceinline__ void cb_hash_block(const float *cb, long count, int block, int nblocks, int tid, WsHeader *hdr,
                                              const unsigned long long *cache_sums, int *cache_stale) {
  float amax = 0.0f;
  unsigned long long hsum = 0ull;
  for (long i = (long)block * 256 + tid; i < count; i += (long)nblocks * 256) {
    const float x = cb[i];
    const float a = fabsf(x);
    amax = (a != a) ? __builtin_inff() : __builtin_fmaxf(amax, a);
    hsum += cb_hash_term(x, i);
  }
  cb_hash_store(amax, hsum, block, tid, hdr, cache_sums, cache_stale);
}

// ---------------------------------------------------------------------------------------------------- builder (one block of NT threads)
struct IndexBuildParams {
  const float *cb;
  char *cache;            // the codebook cache (grid_layout / low_layout)
  const WsHeader *hdr;    // this call's workspace header: cbsum[] = the hashes the call's first launch just computed
  int n;
};

// what a step wrote to the cache, visible to the whole block
__device__ __forceinline__ void index_publish() {
  __threadfence();
  __syncthreads();
}

template <int DIM>
__device__ __forceinline__ void index_load_code(const float *cb, int j, float (&x)[DIM]) {
#pragma unroll
  for (int i = 0; i < DIM; ++i) x[i] = cb[(long)j * DIM + i];
}

// ---- 1. per-axis sums of v | v^2 in fp64: strided over the threads, then over a wave; s_red[wave] (the caller's barrier follows)
template <int DIM, int NT>
__device__ __forceinline__ void index_moments(const float *cb, int n, int tid, double (*s_red)[2 * DIM]) {
  double acc[2 * DIM];
#pragma unroll
  for (int i = 0; i < 2 * DIM; ++i) acc[i] = 0.0;
  for (int j = tid; j < n; j += NT) {
#pragma unroll
    for (int i = 0; i < DIM; ++i) {
      const double v = (double)cb[(long)j * DIM + i];
      acc[i] += v;
      acc[DIM + i] += v * v;
    }
  }
#pragma unroll
  for (int i = 0; i < 2 * DIM; ++i) {
    double v = acc[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((tid & 63) == 0) s_red[tid >> 6][i] = v;
  }
}
// ... and axis i's mean and deviation from them (the waves in ascending order)
template <int DIM, int NT>
__device__ __forceinline__ void index_mean_sd(const double (*s_red)[2 * DIM], int i, int n, double &mean, double &sd) {
  double s = 0.0, q = 0.0;
  for (int w = 0; w < NT / 64; ++w) { s += s_red[w][i]; q += s_red[w][DIM + i]; }
  mean = s / n;
  const double var = q / n - mean * mean;
  sd = sqrt(var > 0.0 ? var : 0.0);
}

// ---- 2. bucket histogram in s_cnt, and the census of the fullest bucket (one wave-reduced atomicMax per wave into LDS).  Its first
// barrier also publishes the thresholds the caller has just left in LDS for bucket_of.
template <int DIM, int NT, class BucketOf>
__device__ __forceinline__ void index_histogram_census(const float *cb, int n, int tid, int *s_cnt, const BucketOf &bucket_of, int *max_sub) {
  __shared__ int s_max;
  for (int c = tid; c < kIndexBuckets; c += NT) s_cnt[c] = 0;
  if (tid == 0) s_max = 0;
  __syncthreads();
  for (int j = tid; j < n; j += NT) {
    float x[DIM];
    index_load_code<DIM>(cb, j, x);
    atomicAdd(&s_cnt[bucket_of(x)], 1);
  }
  __syncthreads();
  int mx = 0;
  for (int c = tid; c < kIndexBuckets; c += NT) mx = max(mx, s_cnt[c]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = max(mx, __shfl_xor(mx, o));
  if ((tid & 63) == 0) atomicMax(&s_max, mx);
  __syncthreads();
  if (tid == 0) *max_sub = s_max;
}

// ---- 3. exclusive scan of the bucket counters (consecutive ones per thread) -> start[] with its 16 entries of padding (= n: the end
// of the last bucket, and what a 16-byte copy may read behind it), cursors in s_cnt.  LEAVES (gq_grid.h): a thread's four buckets
// are one leaf, whose start goes to leaf_start[], padded alike.
template <int NT, bool LEAVES>
__device__ __forceinline__ void index_scan4096(int tid, int *s_cnt, int *s_wsum, int *start, int *leaf_start) {
  constexpr int PER = kIndexBuckets / NT;
  static_assert(kIndexBuckets % NT == 0 && (!LEAVES || PER == 4), "a thread scans whole buckets; with leaves, those of one leaf");
  const int lane = tid & 63, wave = tid >> 6;
  int loc[PER], sum = 0;
#pragma unroll
  for (int k = 0; k < PER; ++k) { loc[k] = s_cnt[tid * PER + k]; sum += loc[k]; }
  int inc = sum;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(inc, o);
    if (lane >= o) inc += v;
  }
  if (lane == 63) s_wsum[wave] = inc;
  __syncthreads();
  int base = 0;
  for (int w = 0; w < wave; ++w) base += s_wsum[w];
  int run = base + inc - sum;
  if constexpr (LEAVES) leaf_start[tid] = run;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    start[tid * PER + k] = run;
    s_cnt[tid * PER + k] = run;
    run += loc[k];
  }
  if (tid == NT - 1)
    for (int k = 0; k < 16; ++k) {
      start[kIndexBuckets + k] = run;
      if constexpr (LEAVES) leaf_start[NT + k] = run;
    }
  __syncthreads();
}

// ---- 4. scatter the codes into bucket order (order inside a bucket: arbitrary -- no result depends on it)
template <int DIM, int NT, class BucketOf>
__device__ __forceinline__ void index_scatter(const float *cb, int n, int tid, int *s_cnt, const BucketOf &bucket_of, float *scb, int *sidx) {
  for (int j = tid; j < n; j += NT) {
    float x[DIM];
    index_load_code<DIM>(cb, j, x);
    const int pos = atomicAdd(&s_cnt[bucket_of(x)], 1);
#pragma unroll
    for (int i = 0; i < DIM; ++i) scb[(long)pos * DIM + i] = x[i];
    sidx[pos] = j;
  }
  index_publish();
}

// ---- 5. tight bounding boxes of the buckets ([lo | hi]; an empty one: lo = +inf, hi = -inf) ...
template <int DIM, int NT>
__device__ __forceinline__ void index_tight_boxes(const int *start, const float *scb, float *box, int tid) {
  const float INF = __builtin_inff();
  for (int c = tid; c < kIndexBuckets; c += NT) {
    float lo[DIM], hi[DIM];
#pragma unroll
    for (int i = 0; i < DIM; ++i) { lo[i] = INF; hi[i] = -INF; }
    const int s = start[c], e = start[c + 1];
    for (int j = s; j < e; ++j) {
#pragma unroll
      for (int i = 0; i < DIM; ++i) {
        const float v = scb[(long)j * DIM + i];
        lo[i] = __builtin_fminf(lo[i], v);
        hi[i] = __builtin_fmaxf(hi[i], v);
      }
    }
#pragma unroll
    for (int i = 0; i < DIM; ++i) { box[(long)c * 2 * DIM + i] = lo[i]; box[(long)c * 2 * DIM + DIM + i] = hi[i]; }
  }
  index_publish();
}
// ... and one level up: each of `nodes` parents is the union of its `fan` consecutive children (index_publish between two levels)
template <int DIM>
__device__ __forceinline__ void index_merge_boxes(const float *child, float *parent, int nodes, int fan, int tid) {
  if (tid >= nodes) return;
  const float INF = __builtin_inff();
  float lo[DIM], hi[DIM];
#pragma unroll
  for (int i = 0; i < DIM; ++i) { lo[i] = INF; hi[i] = -INF; }
  for (int k = 0; k < fan; ++k) {
    const float *b = child + (long)(tid * fan + k) * 2 * DIM;
#pragma unroll
    for (int i = 0; i < DIM; ++i) { lo[i] = __builtin_fminf(lo[i], b[i]); hi[i] = __builtin_fmaxf(hi[i], b[DIM + i]); }
  }
#pragma unroll
  for (int i = 0; i < DIM; ++i) { parent[(long)tid * 2 * DIM + i] = lo[i]; parent[(long)tid * 2 * DIM + DIM + i] = hi[i]; }
}

// ---- 6. stamp: the hashes this call's first launch computed of the very codebook that was just indexed; then, behind a fence, the
// words index_current reads
__device__ __forceinline__ void index_stamp(GridHdr *gh, const WsHeader *hdr, int n, int dim, unsigned magic, int tid) {
  if (tid < kAbsmaxParts) gh->blk_sum[tid] = hdr->cbsum[tid];
  __threadfence();
  __syncthreads();
  if (tid == 0) {
    gh->n = n;
    gh->dim = dim;
    gh->stale = 0;
    gh->magic = magic;
  }
}

// ---------------------------------------------------------------------------------------------------- row reduction of both searches
// Max over the 16 lanes of a DPP row (= one search group) without an LDS round trip: quad_perm [1,0,3,2], [2,3,0,1],
// row_half_mirror, row_mirror -- afterwards every lane of the row holds the result.
// (Written out: from the builtins the compiler makes v_mov_b32_dpp + a canonicalising v_max + the v_max itself per step, twelve
//  VALU instructions per reduction of kernels that are VALU-issue bound; the fused form is four.  s_nop 1: the two wait states a
//  DPP read needs after a VALU write of its source.  Every lane of a row is active or none is, and no source lane is invalid for
//  these four patterns.)  PINNED (volatile): it stays where the row's lanes have converged.
#define GQ_ROW16_MAX_DPP                                                              \
  "s_nop 1\n\t"                                                                       \
  "v_max_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"       \
  "s_nop 1\n\t"                                                                       \
  "v_max_f32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"       \
  "s_nop 1\n\t"                                                                       \
  "v_max_f32_dpp %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf\n\t"           \
  "s_nop 1\n\t"                                                                       \
  "v_max_f32_dpp %0, %0, %0 row_mirror row_mask:0xf bank_mask:0xf"
template <bool PINNED = false>
__device__ __forceinline__ float row16_max(float v) {
  if constexpr (PINNED) asm volatile(GQ_ROW16_MAX_DPP : "+v"(v));
  else asm(GQ_ROW16_MAX_DPP : "+v"(v));
  return v;
}
#undef GQ_ROW16_MAX_DPP

}  // namespace gqhip
