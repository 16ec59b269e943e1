// vq_train.h -- the backward of VQQuantizer's train step (pit/quantization/vq.py:78-89): grad_z elementwise, and grad_emb as a
// BIT-REPRODUCIBLE scatter-reduce of per-item rows into the codebook, without float atomics.
//
// Item p = (b L + l) K + k chose code idx_p; e_p = emb[idx_p].  With N = B L c and (a, b) = (1, beta) legacy | (beta, 1):
//   grad_z   = g_zq + (g_loss a 2 / N) (z - e)          difference in fp32, the rest in fp64, rounded once
//   grad_emb[j][d] = fl32( (g_loss b 2 / N) * sum_{p: idx_p = j} fl32(e_p[d] - z_p[d]) )     sum and product in fp64
//
// grad_emb, store-then-sum without the store (nothing per item is kept: the sum pass RECOMPUTES e - z from z and emb):
//   1. inverted index: a stable LSD radix sort of (code, p) by code, 8 bits per pass, max(1, ceil(log2 n / 8)) passes, starting
//      from ascending p -- so every code's list ends up contiguous and in ascending p.  Per pass three launches: one wave per tile
//      of kVqSortTile items counts its digits (LDS integer adds: a count does not depend on arrival order), one block turns the
//      [digit][tile] table into exclusive offsets, one wave per tile places its items in tile order (ballot ranks, no cursor that
//      arrival order could move).
//   2. sum pass, one thread per (sorted position, column): the thread at the head of a list walks it in ascending p.  A list
//      LONGER THAN kVqChunk = 128 items is summed as partials of kVqChunk consecutive list entries each (the last one shorter), by
//      the threads at those entries, and a further launch adds the partials of a list in chunk order.  So the order of every sum
//      depends on idx and the shape alone, and a collapsed codebook (every item on one code) spreads over items / kVqChunk chunks.
//   grad_emb is zeroed whole first, so a code no item chose holds exact +0.0.
// An idx value outside [0, n) is checked before it addresses anything: the item contributes nothing to grad_emb and its elements
// of grad_z get g_zq alone.  (Inside the sort it rides on code 0 with a flag bit, and the sum pass skips it.)
//
// Workspace (vq_backward_workspace_bytes; contents don't-care on entry, all of it rebuilt by the call): two (key, item) buffer
// pairs, the [256][tiles] digit table, two partial slots of `dim` doubles per kVqChunk-aligned block of sorted positions (such a
// block meets at most two long lists: one that began before it -- its chunk there starts at a non-head entry -- and one that begins
// inside it), and a flag word.
#pragma once
#include "gq_common.h"
#include "gq_rerank.h"

namespace gqhip {

constexpr int kVqChunk = 128;        // list entries per partial sum of grad_emb (part of the value contract: see above)
constexpr int kVqSortTile = 512;     // items per wave and sort pass
constexpr int kVqSortSteps = kVqSortTile / 64;
constexpr unsigned kVqBadItem = 0x80000000u;   // flag on an item whose idx is out of range

struct VqBwdParams {
  const float *z, *emb;
  const int64_t *idx;
  const float *g_zq, *g_loss;          // either may be null (zero)
  float *grad_z, *grad_emb;
  const unsigned *keys, *vals;         // the sorted (code, item) pairs
  double *partial;                     // [2 * ceil(items / kVqChunk)][dim]
  int *flag;                           // set when some list is longer than kVqChunk
  long items, total;                   // B L K;  B L c
  double cz, ce;                       // a 2 / N,  b 2 / N
  int dim, n;
  OutMap omap;
};

struct VqSortParams {
  const int64_t *idx;                  // pass 0 reads the indices themselves ...
  const unsigned *keys_in, *vals_in;   // ... later passes the previous pass's output
  unsigned *keys_out, *vals_out;
  int *table;                          // [256][tiles]
  int *flag;                           // zeroed by pass 0's count launch
  long items;
  int tiles, n, shift, first;
  OutMap omap;
};

__device__ __forceinline__ void vq_sort_load(const VqSortParams &p, long i, unsigned &key, unsigned &val) {
  if (p.first) {
    const long j = p.idx[out_idx_offset(p.omap, i)];
    const bool ok = j >= 0 && j < p.n;
    key = ok ? (unsigned)j : 0u;
    val = (unsigned)i | (ok ? 0u : kVqBadItem);
  } else {
    key = p.keys_in[i];
    val = p.vals_in[i];
  }
}

// one wave per tile: table[digit][tile] = how many of the tile's items carry the digit
__global__ __launch_bounds__(64) void vq_sort_count_kernel(const VqSortParams p) {
  __shared__ int cnt[256];
  const int lane = threadIdx.x, tile = blockIdx.x;
  for (int b = lane; b < 256; b += 64) cnt[b] = 0;
  if (p.first && tile == 0 && lane == 0) *p.flag = 0;
  __syncthreads();
  for (int s = 0; s < kVqSortSteps; ++s) {
    const long i = (long)tile * kVqSortTile + s * 64 + lane;
    if (i < p.items) {
      unsigned key, val;
      vq_sort_load(p, i, key, val);
      atomicAdd(&cnt[(key >> p.shift) & 255u], 1);
    }
  }
  __syncthreads();
  for (int b = lane; b < 256; b += 64) p.table[(long)b * p.tiles + tile] = cnt[b];
}

// one block: the table, read digit-major, becomes its own exclusive prefix sum.  A thread owns kVqScanPer consecutive entries per
// round, loaded up front as 16-byte vectors (the table has 256 * tiles entries and is 256-byte aligned, so a thread's slab is whole or
// empty and aligned); a first cut that walked its slab entry by entry took 30-50 us at 128 tiles, all of it load latency.
constexpr int kVqScanPer = 32;
typedef int vq_i32x4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(1024) void vq_sort_scan_kernel(int *table, long entries) {
  __shared__ int sh[1024];
  const int tid = threadIdx.x;
  int carry = 0;
  for (long base = 0; base < entries; base += 1024L * kVqScanPer) {
    const long lo = base + (long)tid * kVqScanPer;
    const bool in = lo + kVqScanPer <= entries;
    vq_i32x4 v[kVqScanPer / 4];
#pragma unroll
    for (int k = 0; k < kVqScanPer / 4; ++k) v[k] = in ? *reinterpret_cast<const vq_i32x4 *>(table + lo + 4 * k) : vq_i32x4{0, 0, 0, 0};
    int sum = 0;
#pragma unroll
    for (int k = 0; k < kVqScanPer / 4; ++k) sum += (v[k].x + v[k].y) + (v[k].z + v[k].w);
    sh[tid] = sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
      const int add = tid >= o ? sh[tid - o] : 0;
      __syncthreads();
      sh[tid] += add;
      __syncthreads();
    }
    int run = carry + sh[tid] - sum;
    carry += sh[1023];
#pragma unroll
    for (int k = 0; k < kVqScanPer / 4; ++k) {
      const vq_i32x4 t = v[k];
      v[k].x = run; run += t.x;
      v[k].y = run; run += t.y;
      v[k].z = run; run += t.z;
      v[k].w = run; run += t.w;
      if (in) *reinterpret_cast<vq_i32x4 *>(table + lo + 4 * k) = v[k];
    }
    __syncthreads();                                             // sh is reused by the next round
  }
}

// one wave per tile: every item goes to (offset of its digit and tile) + (items of that digit earlier in the tile) -- stable
__global__ __launch_bounds__(64) void vq_sort_place_kernel(const VqSortParams p) {
  __shared__ int base[256];
  const int lane = threadIdx.x, tile = blockIdx.x;
  for (int b = lane; b < 256; b += 64) base[b] = p.table[(long)b * p.tiles + tile];
  unsigned key[kVqSortSteps], val[kVqSortSteps];
#pragma unroll
  for (int s = 0; s < kVqSortSteps; ++s) {
    const long i = (long)tile * kVqSortTile + s * 64 + lane;
    key[s] = val[s] = 0;
    if (i < p.items) vq_sort_load(p, i, key[s], val[s]);
  }
  __syncthreads();
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (int s = 0; s < kVqSortSteps; ++s) {
    const bool live = (long)tile * kVqSortTile + s * 64 + lane < p.items;
    const unsigned digit = (key[s] >> p.shift) & 255u;
    unsigned long long peers = __ballot(live);                 // the live lanes of this step that carry my digit
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const unsigned long long has = __ballot((digit >> b) & 1u);
      peers &= ((digit >> b) & 1u) ? has : ~has;
    }
    const int rank = __popcll(peers & below);
    const long pos = live ? (long)base[digit] + rank : -1;
    __syncthreads();
    if (live && rank == 0) base[digit] += __popcll(peers);      // one lane per digit
    __syncthreads();
    if (pos >= 0 && pos < p.items) {                            // (always, when the table was counted from these items)
      p.keys_out[pos] = key[s];
      p.vals_out[pos] = val[s];
    }
  }
}

// ---- grad_emb: the sum pass over the sorted pairs ------------------------------------------------------------------------------
// fl32(e[d] - z_p[d]) of list entries [q, end) of code `key`, at most kVqChunk of them, added in entry order in fp64
__device__ __forceinline__ double vq_chunk_sum(const VqBwdParams &p, long q, unsigned key, float e, int d) {
#pragma clang fp contract(off)
  double acc = 0.0;
  const long end = q + kVqChunk < p.items ? q + kVqChunk : p.items;
  for (; q < end && p.keys[q] == key; ++q) {
    const unsigned v = p.vals[q];
    if ((v & kVqBadItem) || (long)v >= p.items) continue;
    acc += (double)(e - p.z[out_zhat_offset(p.omap, (long)v, d, p.dim)]);
  }
  return acc;
}
__device__ __forceinline__ long vq_partial_slot(long pos, bool list_head) { return 2 * (pos / kVqChunk) + (list_head ? 1 : 0); }

__global__ __launch_bounds__(256) void vq_emb_sum_kernel(const VqBwdParams p) {
#pragma clang fp contract(off)
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  const long i = t / p.dim;
  const int d = (int)(t % p.dim);
  if (i >= p.items) return;
  const unsigned key = p.keys[i];
  if (key >= (unsigned)p.n) return;
  const bool head = i == 0 || p.keys[i - 1] != key;
  const float e = p.emb[(long)key * p.dim + d];
  if (head) {
    const bool is_long = i + kVqChunk < p.items && p.keys[i + kVqChunk] == key;
    const double acc = vq_chunk_sum(p, i, key, e, d);
    if (!is_long) {
      p.grad_emb[(long)key * p.dim + d] = (float)(((double)*p.g_loss * p.ce) * acc);
    } else {
      p.partial[vq_partial_slot(i, true) * p.dim + d] = acc;
      *p.flag = 1;
    }
    return;
  }
  if (i < kVqChunk || p.keys[i - kVqChunk] != key) return;      // less than a chunk into its list
  long lo = 0, hi = i - kVqChunk;                               // the list's first entry: the first position with this key
  while (lo < hi) {
    const long mid = (lo + hi) >> 1;
    if (p.keys[mid] < key) lo = mid + 1; else hi = mid;
  }
  if ((i - lo) % kVqChunk != 0) return;
  p.partial[vq_partial_slot(i, false) * p.dim + d] = vq_chunk_sum(p, i, key, e, d);
}

// the lists longer than kVqChunk: their partials, added in chunk order
__global__ __launch_bounds__(256) void vq_emb_combine_kernel(const VqBwdParams p) {
#pragma clang fp contract(off)
  if (*p.flag == 0) return;
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  const long i = t / p.dim;
  const int d = (int)(t % p.dim);
  if (i >= p.items) return;
  const unsigned key = p.keys[i];
  if (key >= (unsigned)p.n || !(i == 0 || p.keys[i - 1] != key)) return;
  if (!(i + kVqChunk < p.items && p.keys[i + kVqChunk] == key)) return;
  double acc = p.partial[vq_partial_slot(i, true) * p.dim + d];
  for (long q = i + kVqChunk; q < p.items && p.keys[q] == key; q += kVqChunk) acc += p.partial[vq_partial_slot(q, false) * p.dim + d];
  p.grad_emb[(long)key * p.dim + d] = (float)(((double)*p.g_loss * p.ce) * acc);
}

// ---- grad_z: elementwise over the layout of z, V consecutive elements per thread (V = 4: 16-byte accesses) ---------------------
template <int V>
__global__ __launch_bounds__(256) void vq_grad_z_kernel(const VqBwdParams p) {
#pragma clang fp contract(off)
  const long t = ((long)blockIdx.x * 256 + threadIdx.x) * V;
  if (t >= p.total) return;
  const OutMap &m = p.omap;
  alignas(16) float zv[V], gv[V];
  if (V == 4) {
    *reinterpret_cast<f32x4 *>(zv) = *reinterpret_cast<const f32x4 *>(p.z + t);
    if (p.g_zq) *reinterpret_cast<f32x4 *>(gv) = *reinterpret_cast<const f32x4 *>(p.g_zq + t);
  } else {
    zv[0] = p.z[t];
    if (p.g_zq) gv[0] = p.g_zq[t];
  }
  const double coef = p.g_loss ? (double)*p.g_loss * p.cz : 0.0;
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const long o = t + v;
    long b, l;
    int ch;
    if (m.mode == 1) { l = o % m.L; ch = (int)((o / m.L) % m.c); b = o / ((long)m.L * m.c); }
    else             { ch = (int)(o % m.c); l = (o / m.c) % m.L; b = o / ((long)m.L * m.c); }
    const int d = ch / m.K, k = ch % m.K;                        // channel = d K + k (vq.py:53)
    const long j = p.idx[out_idx_offset(m, (b * m.L + l) * m.K + k)];
    const double g = p.g_zq ? (double)gv[v] : 0.0;
    float diff = 0.0f;
    if (p.g_loss && j >= 0 && j < p.n) diff = zv[v] - p.emb[j * p.dim + d];
    gv[v] = (float)(g + coef * (double)diff);
  }
  if (V == 4) *reinterpret_cast<f32x4 *>(p.grad_z + t) = *reinterpret_cast<const f32x4 *>(gv);
  else p.grad_z[t] = gv[0];
}

}  // namespace gqhip
