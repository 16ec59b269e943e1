// gq_aux.h -- the small HBM-bound kernels around the filter: codebook abs-max,
// workspace header init, operand prep from the encoder output, dequant gather,
// the reference-compatible score-matrix op, LFQ bit pack/unpack, index
// histogram, the u16 wire format and the bit-packed one for any codebook size.
#pragma once
#include "gq_common.h"
#include "gq_rerank.h"
#include "gq_gauss.h"

namespace gqhip {

// ---- dequant: zhat <- cb[idx] in the module layout -------------------------
struct DequantParams {
  const int64_t *idx;
  const float *cb;
  float *zhat;
  long rows;
  int dim, n;
  OutMap omap;
};

__global__ __launch_bounds__(256) void dequant_kernel(const DequantParams p) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= p.rows * p.dim) return;
  long row;
  int g;
  if (p.omap.mode == 1) {
    // walk the output [B, c, L] linearly so stores coalesce
    const long l = t % p.omap.L;
    const int ch = (int)((t / p.omap.L) % p.omap.c);
    const long b = t / ((long)p.omap.L * p.omap.c);
    int k;
    if (p.omap.grouping == 0) { g = ch / p.omap.K; k = ch % p.omap.K; } else { k = ch / p.dim; g = ch % p.dim; }
    row = (b * p.omap.L + l) * p.omap.K + k;
  } else {
    row = t / p.dim;
    g = (int)(t % p.dim);
  }
  long j = p.idx[out_idx_offset(p.omap, row)];
  j = j < 0 ? 0 : (j >= p.n ? p.n - 1 : j);
  p.zhat[out_zhat_offset(p.omap, row, g, p.dim)] = p.cb[j * p.dim + g];
}

// ---- compat op: the reference's score matrix --------------------------------
// gq_cuda.cu:12-40.  One thread per code column, ROWS rows per block; the code
// row lives in registers, mu / sd are wave-uniform (scalar loads), stores are
// 1 KiB coalesced runs along n.  The running sum is a float; `iv*iv` is
// contracted into the subtraction (nvcc's default -fmad), and the beta term is
// accumulated through double exactly as the CUDA source spells it.
// Division: iv = (n - mu) / sd is an IEEE fp32 divide in the CUDA source.  A hardware divide costs
// ~10 VALU instructions per (row, code, dim); instead the correctly rounded reciprocal y = RN(1/sd)
// is formed once per (row, dim) and each quotient is q = a*y, r = fma(-sd, q, a), q' = fma(r, y, q)
// (Markstein: with y correctly rounded and no over/underflow, q' = RN(a/sd)).  Rows whose sd (or
// whose numerators) could leave the safe exponent range take the hardware divide instead.
// BETA1: beta == 1.0 -- (float)((double)acc + (double)co2) equals the fp32 add acc + co2 exactly
// (double rounding is innocuous for the sum of two floats), so the fp64 detour is dropped.
template <int DIM, int ROWS, bool BETA1>
__global__ __launch_bounds__(256) void gq_scores_kernel(const float *__restrict__ mu,
                                                        const float *__restrict__ sd,
                                                        const float *__restrict__ cb,
                                                        float *__restrict__ out, int rows, int n,
                                                        double beta) {
#pragma clang fp contract(off)
  // codes per thread.  2 was measured slower, and so was 2 held as one f32x2 (v_pk_add/mul/fma_f32): on gfx950 a scalar
  // fp32 VALU op issues every ~2.7-3.2 cycles per SIMD and a packed one every ~4.7-5 (tools/valu_pk_peak.hip), so packing
  // buys < 15 % before the splat moves it needs; the kernel is bound by its 6 VALU ops per (row, code, dim).
  constexpr int CPT = 1;
  __shared__ float s_mu[ROWS][DIM], s_sd[ROWS][DIM], s_y[ROWS][DIM];
  __shared__ int s_fast[ROWS];
  const int j0 = blockIdx.x * (256 * CPT) + threadIdx.x;
  const int r0 = blockIdx.y * ROWS;
  if (threadIdx.x < ROWS) s_fast[threadIdx.x] = 1;
  __syncthreads();
  for (int t = threadIdx.x; t < ROWS * DIM; t += 256) {
    const int r = t / DIM, i = t % DIM;
    const int rr = r0 + r < rows ? r0 + r : rows - 1;
    const float m = mu[(long)rr * DIM + i], s = sd[(long)rr * DIM + i];
    s_mu[r][i] = m;
    s_sd[r][i] = s;
    s_y[r][i] = __fdiv_rn(1.0f, s);
    const float as = fabsf(s), am = fabsf(m);
    if (!(as > 1e-18f && as < 1e18f && am < 1e18f)) s_fast[r] = 0;   // also catches NaN
  }
  float nv[CPT][DIM], n2[CPT][DIM];
  float amax = 0.f;
#pragma unroll
  for (int k = 0; k < CPT; ++k) {
    const int j = j0 + 256 * k;
    const int jc = j < n ? j : n - 1;
#pragma unroll
    for (int i = 0; i < DIM; ++i) {
      nv[k][i] = cb[(long)jc * DIM + i];
      n2[k][i] = nv[k][i] * nv[k][i];
      amax = __builtin_fmaxf(amax, fabsf(nv[k][i]));
    }
  }
  const bool code_ok = amax < 1e18f;   // false for inf / NaN codes too
  __syncthreads();
  for (int r = 0; r < ROWS && r0 + r < rows; ++r) {
    float acc[CPT];
#pragma unroll
    for (int k = 0; k < CPT; ++k) acc[k] = 0.0f;
    if (s_fast[r] && __all(code_ok)) {
#pragma unroll
      for (int i = 0; i < DIM; ++i) {
        const float m = s_mu[r][i], sg = s_sd[r][i], y = s_y[r][i];
#pragma unroll
        for (int k = 0; k < CPT; ++k) {
          const float a = nv[k][i] - m;
          const float q = a * y;
          const float rem = __builtin_fmaf(-sg, q, a);
          const float iv = __builtin_fmaf(rem, y, q);
          acc[k] = __builtin_fmaf(-iv, iv, acc[k]);
          if constexpr (BETA1) acc[k] = acc[k] + n2[k][i];
          else acc[k] = (float)((double)acc[k] + (double)n2[k][i] * beta);
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < DIM; ++i) {
#pragma unroll
        for (int k = 0; k < CPT; ++k) {
          const float iv = __fdiv_rn(nv[k][i] - s_mu[r][i], s_sd[r][i]);
          acc[k] = __builtin_fmaf(-iv, iv, acc[k]);
          acc[k] = (float)((double)acc[k] + (double)n2[k][i] * beta);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
      const int j = j0 + 256 * k;
      if (j < n) out[(long)(r0 + r) * n + j] = acc[k];
    }
  }
}

__global__ __launch_bounds__(256) void gq_scores_generic_kernel(const float *__restrict__ mu,
                                                                const float *__restrict__ sd,
                                                                const float *__restrict__ cb,
                                                                float *__restrict__ out, int dim,
                                                                int rows, int n, double beta) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  const int r = blockIdx.y;
  if (j >= n || r >= rows) return;
  float acc = 0.0f;
  for (int i = 0; i < dim; ++i) {
    const float co = cb[(long)j * dim + i];
    const float iv = __fdiv_rn(co - mu[(long)r * dim + i], sd[(long)r * dim + i]);
    acc = __builtin_fmaf(-iv, iv, acc);
    acc = (float)((double)acc + (double)(co * co) * beta);
  }
  out[(long)r * n + j] = acc;
}

// ---- LFQ (lfq.py:147-158, 210-228) ------------------------------------------
__global__ __launch_bounds__(256) void lfq_pack_kernel(const float *__restrict__ x,
                                                       int64_t *__restrict__ idx,
                                                       float *__restrict__ q, long rows, int nbits) {
  const long r = (long)blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  int64_t v = 0;
  for (int i = 0; i < nbits; ++i) {
    const bool bit = x[r * nbits + i] > 0.0f;
    v = v * 2 + (bit ? 1 : 0);
    if (q) q[r * nbits + i] = bit ? 1.0f : -1.0f;
  }
  idx[r] = v;
}

__global__ __launch_bounds__(256) void lfq_unpack_kernel(const int64_t *__restrict__ idx,
                                                         float *__restrict__ q, long rows, int nbits) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= rows * nbits) return;
  const long r = t / nbits;
  const int i = (int)(t % nbits);
  const int64_t v = idx[r];
  q[t] = ((v >> (nbits - 1 - i)) & 1) ? 1.0f : -1.0f;
}

// ---- FSQ (fsq.py:29-89) ------------------------------------------------------
struct FsqLevels {
  int n;
  int lev[16];
};

__global__ __launch_bounds__(256) void fsq_quantize_kernel(const float *__restrict__ z, FsqLevels L,
                                                           float *__restrict__ zhat,
                                                           int32_t *__restrict__ idx, long rows) {
#pragma clang fp contract(off)
  const long r = (long)blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  int packed = 0;
  for (int l = 0; l < L.n; ++l) {
    const int lv = L.lev[l];
    const float half_l = (float)(lv - 1) * (1.0f + 1e-3f) / 2.0f;          // (levels-1)*(1+eps)/2
    const float offset = (lv % 2 == 0) ? 0.5f : 0.0f;
    const float shift = (float)atanh((double)(offset / half_l));
    const float x = z[r * L.n + l] + shift;
    const float b = (float)tanh((double)x) * half_l - offset;
    const float q = rintf(b);                                              // torch.round: half to even
    const int hw = lv / 2;
    if (zhat) zhat[r * L.n + l] = q / (float)hw;
    packed = packed * lv + (int)(q + (float)hw);
  }
  idx[r] = packed;
}

__global__ __launch_bounds__(256) void fsq_dequant_kernel(const int32_t *__restrict__ idx, FsqLevels L,
                                                          float *__restrict__ zhat, long rows) {
  const long r = (long)blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  int v = idx[r];
  for (int l = L.n - 1; l >= 0; --l) {
    const int lv = L.lev[l];
    const int d = v % lv;
    v /= lv;
    const int hw = lv / 2;
    zhat[r * L.n + l] = (float)(d - hw) / (float)hw;
  }
}

// ---- index histogram + u16 wire format (eval.py:127,137-141,152-154) --------
__global__ __launch_bounds__(256) void hist_kernel(const int64_t *__restrict__ idx, long count, int n,
                                                   int *__restrict__ hist) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < count; i += (long)gridDim.x * 256) {
    const int64_t v = idx[i];
    if (v >= 0 && v < n) atomicAdd(&hist[v], 1);
  }
}
__global__ __launch_bounds__(256) void to_u16_kernel(const int64_t *__restrict__ idx,
                                                     uint16_t *__restrict__ out, long count) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < count) out[i] = (uint16_t)idx[i];
}
__global__ __launch_bounds__(256) void from_u16_kernel(const uint16_t *__restrict__ in,
                                                       int64_t *__restrict__ idx, long count) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < count) idx[i] = (int64_t)in[i];
}


// ---- one rank's per-step record in ONE launch (round 4): per-image PSNR + the uint16 index wire format -----------------------
// rec (int32 words) = [ B per-image PSNRs as fp32 bits | indices as uint16 pairs, low half first ] -- pit_hip/eval_dist.py:StepRecord
// with n_metrics = 1, i.e. what eval.py:165-169 (get_psnr(zero_mean=True), pit/evaluations/psnr.py:17-28) and the index gather
// of eval.py:152-154 publish per batch.  Blocks [0, B * chunks): one contiguous chunk of one image, the squared differences in
// the reference's fp32 op order ((x + 1) 127.5 - (x_rec + 1) 127.5, squared), summed in fp64; the LAST block of an image (a ticket
// per image, reset for the next call) adds the chunk sums in chunk order -- a fixed order: the value is bit-reproducible --, stores
// zeros over them (one thread per image, `chunks` stores: the workspace is all zero between calls whatever B the next one has) and
// writes 20 log10(255 / sqrt(mse)).  The blocks after those pack the indices.  The three-metric record (gq_step_record_ssim_f32)
// runs the same kernel with stride 3: [ B x (psnr, ssim, ms_ssim) | indices ], its PSNR words those of stride 1 bit for bit.
struct StepRecordParams {
  const float *x, *x_rec;     // [B, per_image] in the SAME dense layout
  const int64_t *idx;         // [n_idx]
  int *rec;                   // [B + (n_idx + 1) / 2]
  double *partial;            // [B, chunks]      (workspace; zero between calls, like the tickets)
  int *ticket;                // [B], all zero between calls (workspace)
  long per_image, n_idx;
  int B, chunks, psnr_blocks;
  int stride;                 // int32 words per image in the metric block: PSNR of image b at rec[b * stride], indices at rec[B * stride]
};
constexpr int kPsnrChunk = 256 * 4 * 8;      // floats per block: eight 16-byte loads per thread

// PSNR block `blk` of [0, B * chunks): shared by the uint16 record and the bit-packed one, so their metric words are the same code.
__device__ __forceinline__ void step_record_psnr_block(const StepRecordParams &p, const int blk) {
  const int tid = threadIdx.x;
  const int b = blk / p.chunks, ch = blk % p.chunks;
  const long e0 = (long)ch * kPsnrChunk, e1 = e0 + kPsnrChunk < p.per_image ? e0 + kPsnrChunk : p.per_image;
  const float *xa = p.x + (long)b * p.per_image, *xb = p.x_rec + (long)b * p.per_image;
  double acc = 0.0;
  auto term = [&](float u, float v) {
#pragma clang fp contract(off)
    const float a = (u + 1.0f) * 127.5f, c = (v + 1.0f) * 127.5f;
    const float d = a - c;
    acc += (double)(d * d);
  };
  if ((p.per_image & 3) == 0) {
    for (long e = e0 + 4 * tid; e < e1; e += 1024) {
      const f32x4 u = *reinterpret_cast<const f32x4 *>(xa + e), v = *reinterpret_cast<const f32x4 *>(xb + e);
      term(u.x, v.x); term(u.y, v.y); term(u.z, v.z); term(u.w, v.w);
    }
  } else {
    for (long e = e0 + tid; e < e1; e += 256) term(xa[e], xb[e]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  __shared__ double sh[4];
  __shared__ int sh_last;
  if ((tid & 63) == 0) sh[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    p.partial[(long)b * p.chunks + ch] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
    __threadfence();
    sh_last = atomicAdd(&p.ticket[b], 1) == p.chunks - 1;
  }
  __syncthreads();
  if (!sh_last || tid != 0) return;
  __threadfence();
  double sum = 0.0;
  for (int k = 0; k < p.chunks; ++k) {
    double *part = &p.partial[(long)b * p.chunks + k];
    sum += __hip_atomic_load(part, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *part = 0.0;                               // the whole workspace is zero again behind the call: a later call may lay it out
  }                                            // for another B (its tickets then sit where these sums were)
  const float mse = (float)(sum / (double)p.per_image);
  const float psnr = (float)(20.0 * log10(255.0 / sqrt((double)mse)));      // identical images: +inf, like the reference
  p.rec[(long)b * p.stride] = __float_as_int(psnr);
  p.ticket[b] = 0;                             // ready for the next call on this workspace
}

__global__ __launch_bounds__(256) void step_record_kernel(const StepRecordParams p) {
  if ((int)blockIdx.x >= p.psnr_blocks) {
    const long w = (long)(blockIdx.x - p.psnr_blocks) * 256 + threadIdx.x;        // one packed word per thread
    if (2 * w < p.n_idx) {
      const unsigned lo = (unsigned)p.idx[2 * w] & 0xffffu;
      const unsigned hi = 2 * w + 1 < p.n_idx ? (unsigned)p.idx[2 * w + 1] & 0xffffu : 0u;
      p.rec[(long)p.B * p.stride + w] = (int)(lo | (hi << 16));
    }
    return;
  }
  step_record_psnr_block(p, (int)blockIdx.x);
}

// ---- the bit-packed index wire format: any codebook size up to 2^32 ----------------------------------------------------------------
// Index k -- its low w bits, the value taken as unsigned 32-bit -- occupies bits [k w, (k + 1) w) of a little-endian bit stream over
// int32 words (stream bit p = bit p mod 32 of word p div 32), zero-padded to a whole word; w = 16 is the uint16 pair format above.
// A block owns 256 consecutive words = stream bits [8192 blk, 8192 (blk + 1)).  It reads the indices that touch those bits with
// coalesced 8-byte loads (lane i takes index base + i), kBitsTile at a time, leaves their masked values in LDS, and every thread
// ORs its own word together from the at most ceil(32 / w) + 1 of them that touch it: one plain store per word, no atomics on the
// stream.  An index outside [0, n_codes) is counted by the block that owns its FIRST bit (so once), the counts are summed per
// block, and the sum is returned to thread 0.
constexpr int kBitsTile = 2048 + 64;          // indices per LDS pass: w >= 4 needs one pass (8192 / 4 + 2)
struct PackBitsParams {
  const int64_t *idx;         // [n_idx]
  int *words;                 // [n_words]
  long n_idx, n_words;        // n_words = ceil(n_idx w / 32)
  int64_t n_codes;
  int w;                      // 1..32
};

__device__ __forceinline__ int pack_bits_block(const PackBitsParams &p, const long blk) {
  __shared__ unsigned s_val[kBitsTile];
  __shared__ int s_viol[4];
  const int tid = threadIdx.x;
  const unsigned mask = p.w == 32 ? 0xffffffffu : (1u << p.w) - 1u;
  const long bit0 = blk * 8192;                                     // the block's first stream bit
  const long k_lo = bit0 / p.w;                                     // first index with a bit in the block
  long k_hi = (bit0 + 8191) / p.w;                                  // last one
  k_hi = k_hi < p.n_idx ? k_hi : p.n_idx - 1;
  const long word = blk * 256 + tid, p0 = word * 32;                // this thread's word, its first stream bit
  const long k0 = p0 / p.w;
  long k1 = (p0 + 31) / p.w;
  k1 = k1 < p.n_idx ? k1 : p.n_idx - 1;
  unsigned out = 0u;
  int viol = 0;
  for (long base = k_lo; base <= k_hi; base += kBitsTile) {
    if (base != k_lo) __syncthreads();                              // the previous pass has been read
    for (int i = tid; i < kBitsTile && base + i <= k_hi; i += 256) {
      const int64_t v = p.idx[base + i];
      s_val[i] = (unsigned)v & mask;
      viol += ((v < 0 || v >= p.n_codes) && (base + i) * p.w >= bit0) ? 1 : 0;
    }
    __syncthreads();
    const long lo = k0 > base ? k0 : base, hi = k1 < base + kBitsTile - 1 ? k1 : base + kBitsTile - 1;
    for (long k = lo; k <= hi; ++k) {
      const int sh = (int)(k * p.w - p0);                           // in (-w, 32)
      const unsigned v = s_val[k - base];
      out |= sh >= 0 ? v << sh : v >> -sh;
    }
  }
  if (word < p.n_words) p.words[word] = (int)out;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) viol += __shfl_xor(viol, o);
  if ((tid & 63) == 0) s_viol[tid >> 6] = viol;
  __syncthreads();
  return (s_viol[0] + s_viol[1]) + (s_viol[2] + s_viol[3]);
}

// *p = min(*p + v, 2^31 - 1) for v >= 0: the one integer atomic a block spends on its violations
__device__ __forceinline__ void saturating_add(int *p, const int v) {
  int old = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), seen;
  do {
    seen = old;
    old = atomicCAS(p, seen, seen > 0x7fffffff - v ? 0x7fffffff : seen + v);
  } while (old != seen);
}

// gq_indices_pack_bits: violations (or NULL) was zeroed in-stream by the entry point
__global__ __launch_bounds__(256) void pack_bits_kernel(const PackBitsParams p, int *__restrict__ violations) {
  const int viol = pack_bits_block(p, (long)blockIdx.x);
  if (threadIdx.x == 0 && violations && viol) saturating_add(violations, viol);
}

// value k of a bit-packed field (the inverse of the above)
__device__ __forceinline__ unsigned unpack_bits_at(const int *__restrict__ field, const long k, const int w) {
  const long p = k * w;
  const long wd = p >> 5;
  const int off = (int)(p & 31);
  unsigned v = (unsigned)field[wd] >> off;
  if (off + w > 32) v |= (unsigned)field[wd + 1] << (32 - off);      // the index straddles two words (then off > 0)
  return w == 32 ? v : v & ((1u << w) - 1u);
}

// n_records fields of `count` indices each, field r at records + r * stride + offset (words): one index per thread, 8-byte
// coalesced stores; neighbouring lanes read the same or neighbouring words.
__global__ __launch_bounds__(256) void unpack_bits_kernel(const int *__restrict__ records, int64_t *__restrict__ idx, long n_records,
                                                          long stride, long offset, long count, int w) {
  const long total = n_records * count;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long r = i / count, k = i - r * count;
    idx[i] = (int64_t)unpack_bits_at(records + r * stride + offset, k, w);
  }
}

// hist[v] += 1 for every packed value v < n of the same fields: integer atomics only, so the sums are exact whatever the order
__global__ __launch_bounds__(256) void hist_packed_kernel(const int *__restrict__ records, long n_records, long stride, long offset,
                                                          long count, int w, int64_t n, unsigned long long *__restrict__ hist) {
  const long total = n_records * count;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long r = i / count, k = i - r * count;
    const unsigned v = unpack_bits_at(records + r * stride + offset, k, w);
    if ((int64_t)v < n) atomicAdd(&hist[v], 1ull);
  }
}

// ---- the step record with bit-packed indices: [ metrics as in step_record_kernel | n_words index words | 1 violations word ] -------
// Blocks [0, pack_blocks) pack (first, so the short ones are not the kernel's tail), the rest are step_record_psnr_block.  The
// violations count goes through ONE 64-bit workspace word behind the PSNR workspace, zero between calls like the rest: bits 0..39
// the running count, bits 40..63 a ticket.  A packing block adds (1 << 40) + its count with one integer atomic; the block whose
// add returns ticket pack_blocks - 1 has the other blocks' total in the same returned value, stores the sum (saturated) into the
// record with a plain store and zeroes the word.  pack_blocks < 2^24 (the host checks), so the count stays below 2^37.
constexpr int kViolTicketShift = 40;
struct StepRecordBitsParams {
  StepRecordParams r;         // r.rec, r.B, r.stride: the metric block; r.idx / r.n_idx: the indices
  PackBitsParams k;           // k.words = r.rec + B * stride
  unsigned long long *viol;   // workspace: count | ticket << 40
  int pack_blocks;            // >= 1: the violations word is written even when there are no indices
};

__global__ __launch_bounds__(256) void step_record_bits_kernel(const StepRecordBitsParams p) {
  if ((int)blockIdx.x >= p.pack_blocks) {
    step_record_psnr_block(p.r, (int)blockIdx.x - p.pack_blocks);
    return;
  }
  const int viol = pack_bits_block(p.k, (long)blockIdx.x);
  if (threadIdx.x != 0) return;
  const unsigned long long old = atomicAdd(p.viol, (1ull << kViolTicketShift) + (unsigned long long)viol);
  if ((int)(old >> kViolTicketShift) != p.pack_blocks - 1) return;
  const unsigned long long total = (old & ((1ull << kViolTicketShift) - 1)) + (unsigned long long)viol;
  p.k.words[p.k.n_words] = total > 0x7fffffffull ? 0x7fffffff : (int)total;
  *p.viol = 0ull;                               // ready for the next call on this workspace
}

// ---- VQ's codebook loss in eval (pit/quantization/vq.py:78-86): mean((z_q - z)^2) over every element --------------------------
// After the arg-min has left its indices: element (row, g) contributes (emb[idx[row]][g] - z[row][g])^2 formed in fp32 like the
// reference, summed in fp64 -- per thread in a fixed assignment, per block by a fixed tree, and the LAST block (a ticket in the
// workspace header, reset by the call's first launch) adds the block sums in block order: bit-reproducible.
//   loss[0] = mean + beta * mean (legacy) | beta * mean + mean, in fp32 like the reference;  loss[1] = mean.
struct VqLossParams {
  const float *zrows;       // [rows, dim] the row operands gq_prep_kernel left in the workspace
  const int64_t *idx;       // module layout
  const float *emb;         // [n, dim]
  float *loss;              // [2]
  WsHeader *hdr;
  long rows;
  int dim, n;
  float beta;
  int legacy;
  OutMap omap;
};

__global__ __launch_bounds__(256) void vq_loss_kernel(const VqLossParams p) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x;
  double acc = 0.0;
  // one row per thread and pass: ONE index load, then the row's codeword and operands as 16-byte loads (dim % 4 == 0) -- the first cut
  // walked elements (an index load and an integer division per element: 47 us at 65 536 rows, latency-bound)
  const bool vec = (p.dim & 3) == 0;
  for (long row = (long)blockIdx.x * 256 + tid; row < p.rows; row += (long)gridDim.x * 256) {
    const long j = p.idx[out_idx_offset(p.omap, row)];
    const bool ok = j >= 0 && j < p.n;
    const float *e = p.emb + (ok ? j : 0) * p.dim, *z = p.zrows + row * p.dim;
    if (vec) {
      for (int g = 0; g < p.dim; g += 4) {
        const f32x4 ev = *reinterpret_cast<const f32x4 *>(e + g), zv = *reinterpret_cast<const f32x4 *>(z + g);
        const float d0 = ev.x - zv.x, d1 = ev.y - zv.y, d2 = ev.z - zv.z, d3 = ev.w - zv.w;
        acc += (double)(d0 * d0);
        acc += (double)(d1 * d1);
        acc += (double)(d2 * d2);
        acc += (double)(d3 * d3);
      }
    } else {
      for (int g = 0; g < p.dim; ++g) {
        const float d = e[g] - z[g];
        acc += (double)(d * d);
      }
    }
    if (!ok) acc = __builtin_nan("");
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  __shared__ double sh[4];
  __shared__ int sh_last;
  if ((tid & 63) == 0) sh[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    p.hdr->loss_part[blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
    __threadfence();
    sh_last = atomicAdd(&p.hdr->loss_ticket, 1) == (int)gridDim.x - 1;
  }
  __syncthreads();
  if (!sh_last || tid >= 64) return;
  __threadfence();
  // the last block: the block sums in block order per lane (lane l: l, l + 64, ...), then a fixed shuffle tree
  double sum = 0.0;
  for (int k = tid; k < (int)gridDim.x; k += 64) sum += __hip_atomic_load(&p.hdr->loss_part[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
  if (tid != 0) return;
  const float m = (float)(sum / (double)(p.rows * p.dim));
  p.loss[0] = p.legacy ? m + p.beta * m : p.beta * m + m;
  p.loss[1] = m;
}

}  // namespace gqhip
