// gq_attn.h -- fused multi-head attention forward, softmax(q k^T / sqrt(d)) v, for the ViT backbone (pit/modules/vit.py:142-151:
// nn.MultiheadAttention(x, x, x, need_weights=False), no mask, no dropout).  Flash-style: S = q k^T and P never leave the chip.
//
// Operands are read IN PLACE from the in-projection output qkv [B][L][3E] fp32 (F.linear(x, in_proj_weight, in_proj_bias)):
// q, k, v are the three E-wide column blocks, head h is columns h d .. h d + d - 1 of each (MHA's view(L, B H, d)).  The result
// is written as [B][L][E] fp32 with the heads concatenated (the operand of out_proj).  d = 64.
//
// Precision: every product on v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 accumulation in program order), softmax in fp32
// registers.  q is pre-multiplied by log2(e) / sqrt(d) (one rounding per element) so that p = exp2(s - m) needs no further
// multiply.  No data-dependent operand scaling is needed: fp32 covers the range of the products.  Deterministic: fixed-order
// sums, no atomics.
//
// Tiling: a block = 4 waves = 128 query rows of one (batch, head); a wave owns 32 query rows.  Keys stream in tiles of 32 rows,
// double-buffered in LDS (one barrier per tile; the next tile's global loads are in flight while the current one is multiplied).
//   S^T = K Q^T : A = K[key][dim] from LDS (row stride 68 floats: a ds_read_b128 phase of 16 keys covers all 64 banks),
//                 B = Q^T from registers (lane: query row lane % 32, dims 32 (lane / 32) + s).  The accumulator leaves each
//                 lane with 16 of the 32 scores of ITS query row (keys crow(i, lane / 32)), the other 16 in lane ^ 32: row max
//                 and row sum are 15 in-lane ops + one cross-half exchange.
//   O^T += V^T P^T : A = V^T[dim][key] from LDS (V stored transposed, row stride 36 floats, conflict-free b128 reads),
//                 B = P^T straight from the score registers (MFMA step i takes key crow(i, lane / 32), the accumulator layout).
//                 Two 32 x 32 accumulators (dims 0-31, 32-63), again one query row per lane.
// Tails: query rows >= L compute on zeros and are not stored; key rows >= L are zero in LDS and their scores are -inf.
#pragma once
#include "gq_common.h"

namespace gqhip {

constexpr int kAttnD = 64;          // head dim built
constexpr int kAttnQRows = 128;     // query rows per block (4 waves x 32)
constexpr int kAttnKT = 32;         // keys per tile
constexpr int kAttnKS = kAttnD + 4;     // K row stride in LDS (floats)
constexpr int kAttnVS = kAttnKT + 4;    // V^T row stride in LDS (floats)

// accumulator register i of lane half hi holds row crow(i, hi) of a 32 x 32 MFMA tile (column = lane % 32)
__device__ __forceinline__ int attn_crow(int i, int hi) { return (i & 3) + 8 * (i >> 2) + 4 * hi; }

struct AttnTileRegs {
  f32x4 k[2], v[2];
};

// global -> registers: thread t moves float4 number t and t + 256 of the 32 x 64 K and V tiles (zeros beyond L)
__device__ __forceinline__ void attn_load_tile(AttnTileRegs &r, const float *kbase, const float *vbase, long row_stride, int k0,
                                               int L, int tid) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int idx = tid + 256 * j, key = idx >> 4, d4 = idx & 15;
    if (k0 + key < L) {
      const long off = (long)(k0 + key) * row_stride + 4 * d4;
      r.k[j] = *reinterpret_cast<const f32x4 *>(kbase + off);
      r.v[j] = *reinterpret_cast<const f32x4 *>(vbase + off);
    } else {
      r.k[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      r.v[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }
}

__device__ __forceinline__ void attn_store_tile(const AttnTileRegs &r, float *sK, float *sV, int tid) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int idx = tid + 256 * j, key = idx >> 4, d4 = idx & 15;
    *reinterpret_cast<f32x4 *>(sK + key * kAttnKS + 4 * d4) = r.k[j];
    sV[(4 * d4 + 0) * kAttnVS + key] = r.v[j].x;
    sV[(4 * d4 + 1) * kAttnVS + key] = r.v[j].y;
    sV[(4 * d4 + 2) * kAttnVS + key] = r.v[j].z;
    sV[(4 * d4 + 3) * kAttnVS + key] = r.v[j].w;
  }
}

// grid = (ceil(L / 128), B * H), block = 256.  kLse: also store lse[B][H][L] = m + log2(l), the log-sum-exp of the row's scores in
// the kernel's own units (scores times log2(e) / sqrt(d)) -- what the backward (gq_attn_bwd.h) recomputes P from.  One more store;
// the arithmetic and `out` are those of the `false` instantiation bit for bit.
template <bool kLse>
__global__ __launch_bounds__(256, 2) void mha_fwd_f32_kernel(const float *__restrict__ qkv, float *__restrict__ out,
                                                              float *__restrict__ lse, int L, int E, int H) {
  __shared__ __attribute__((aligned(16))) float sK[2][kAttnKT * kAttnKS];
  __shared__ __attribute__((aligned(16))) float sV[2][kAttnD * kAttnVS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hi = lane >> 5, r = lane & 31;
  const int bh = blockIdx.y, b = bh / H, h = bh - b * H;
  const long rs = 3L * E;                                        // qkv row stride
  const float *qbase = qkv + (long)b * L * rs + (long)h * kAttnD;
  const float *kbase = qbase + E;
  const float *vbase = qbase + 2 * E;
  const int qrow = blockIdx.x * kAttnQRows + wave * 32 + r;

  // Q^T operand: lane holds q[qrow][32 hi + s] * log2(e) / sqrt(d), s = 0..31
  constexpr float kQScale = 0.18033688011112042f;                // log2(e) / 8
  float q[32];
  if (qrow < L) {
    const float *qp = qbase + (long)qrow * rs + 32 * hi;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const f32x4 t = *reinterpret_cast<const f32x4 *>(qp + 4 * j);
      q[4 * j + 0] = t.x * kQScale; q[4 * j + 1] = t.y * kQScale; q[4 * j + 2] = t.z * kQScale; q[4 * j + 3] = t.w * kQScale;
    }
  } else {
#pragma unroll
    for (int s = 0; s < 32; ++s) q[s] = 0.f;
  }

  f32x16 o0, o1;
#pragma unroll
  for (int i = 0; i < 16; ++i) { o0[i] = 0.f; o1[i] = 0.f; }
  float m = -__builtin_inff(), l = 0.f;                          // running max (both halves agree), this half's running sum

  const int ntiles = (L + kAttnKT - 1) / kAttnKT;
  AttnTileRegs pre;
  attn_load_tile(pre, kbase, vbase, rs, 0, L, tid);
  attn_store_tile(pre, sK[0], sV[0], tid);
  __syncthreads();

  for (int t = 0; t < ntiles; ++t) {
    const int buf = t & 1, k0 = t * kAttnKT;
    if (t + 1 < ntiles) attn_load_tile(pre, kbase, vbase, rs, k0 + kAttnKT, L, tid);

    // S^T[key][qrow] over the 64 dims: MFMA step s multiplies dims (s, 32 + s) -- lane half hi supplies dim 32 hi + s
    f32x16 sacc;
#pragma unroll
    for (int i = 0; i < 16; ++i) sacc[i] = 0.f;
    const float *kp = sK[buf] + r * kAttnKS + 32 * hi;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const f32x4 kv = *reinterpret_cast<const f32x4 *>(kp + 4 * j);
      sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(kv.x, q[4 * j + 0], sacc, 0, 0, 0);
      sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(kv.y, q[4 * j + 1], sacc, 0, 0, 0);
      sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(kv.z, q[4 * j + 2], sacc, 0, 0, 0);
      sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(kv.w, q[4 * j + 3], sacc, 0, 0, 0);
    }
    if (k0 + kAttnKT > L) {                                      // the last, partial tile: keys >= L do not exist
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (k0 + attn_crow(i, hi) >= L) sacc[i] = -__builtin_inff();
    }

    // online softmax for query row r: this half's 16 scores, the other 16 in lane ^ 32
    float mt = sacc[0];
#pragma unroll
    for (int i = 1; i < 16; ++i) mt = fmaxf(mt, sacc[i]);
    mt = fmaxf(mt, __shfl_xor(mt, 32));
    const float mn = fmaxf(m, mt);                               // finite: every tile holds a key < L
    const float alpha = exp2f(m - mn);                           // 0 on the first tile
    m = mn;
    float ls = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      sacc[i] = exp2f(sacc[i] - mn);
      ls += sacc[i];
    }
    l = l * alpha + ls;
#pragma unroll
    for (int i = 0; i < 16; ++i) { o0[i] *= alpha; o1[i] *= alpha; }

    // O^T[dim][qrow] += V^T[dim][key] P^T[key][qrow]: step i takes key attn_crow(i, hi), the key of score register i
    const float *vp0 = sV[buf] + r * kAttnVS + 4 * hi;
    const float *vp1 = vp0 + 32 * kAttnVS;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const f32x4 va = *reinterpret_cast<const f32x4 *>(vp0 + 8 * j);   // keys 8 j + 4 hi + 0..3 = attn_crow(4 j + c, hi)
      const f32x4 vb = *reinterpret_cast<const f32x4 *>(vp1 + 8 * j);
      o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(va.x, sacc[4 * j + 0], o0, 0, 0, 0);
      o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(vb.x, sacc[4 * j + 0], o1, 0, 0, 0);
      o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(va.y, sacc[4 * j + 1], o0, 0, 0, 0);
      o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(vb.y, sacc[4 * j + 1], o1, 0, 0, 0);
      o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(va.z, sacc[4 * j + 2], o0, 0, 0, 0);
      o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(vb.z, sacc[4 * j + 2], o1, 0, 0, 0);
      o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(va.w, sacc[4 * j + 3], o0, 0, 0, 0);
      o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(vb.w, sacc[4 * j + 3], o1, 0, 0, 0);
    }

    // the buffer written here was last read in tile t - 1, which every wave finished before the previous barrier
    if (t + 1 < ntiles) attn_store_tile(pre, sK[buf ^ 1], sV[buf ^ 1], tid);
    __syncthreads();
  }

  if (qrow >= L) return;
  const float ll = l + __shfl_xor(l, 32);
  if (kLse && hi == 0) lse[(long)bh * L + qrow] = m + log2f(ll);
  // lane holds dims attn_crow(i, hi) (+ 32): runs of four consecutive dims -> float4 stores
  float *op = out + ((long)b * L + qrow) * E + (long)h * kAttnD;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int d = 8 * j + 4 * hi;
    *reinterpret_cast<f32x4 *>(op + d) = f32x4{o0[4 * j] / ll, o0[4 * j + 1] / ll, o0[4 * j + 2] / ll, o0[4 * j + 3] / ll};
    *reinterpret_cast<f32x4 *>(op + 32 + d) = f32x4{o1[4 * j] / ll, o1[4 * j + 1] / ll, o1[4 * j + 2] / ll, o1[4 * j + 3] / ll};
  }
}

}  // namespace gqhip
