// gq_attn_bwd.h -- backward of the fused multi-head attention of gq_attn.h: from qkv [B][L][3E], out [B][L][E], the forward's
// lse [B][H][L] (log-sum-exp of the scores in the forward's units, scores times log2(e) / sqrt(d)) and dout [B][L][E] to
// dqkv [B][L][3E] in the layout of qkv (the gradient F.linear's backward takes as is).  Flash-style: P is recomputed, S, P, dP and
// dS never leave the chip.  With s = q k^T / sqrt(d) and s2 = s log2(e):
//   P = exp2(s2 - lse2),  dV = P^T dout,  dP = dout V^T,  delta_i = sum_j P_ij dP_ij,  dS = P o (dP - delta),
//   dQ = dS K / sqrt(d),  dK = dS^T Q / sqrt(d).
// The q operand of the score product carries log2(e) / 8 exactly as in the forward (same products in the same order: the scores
// are the forward's bit for bit); the gradient scale is 1 / 8.
//
// delta and the row sum.  In exact arithmetic delta_i = sum_d dout[i][d] out[i][d]; the kernels take it as sum_j P_ij dP_ij from the
// very P and dP they multiply with, and `out` is not read.  Where one key holds a row's weight (a peaked softmax), dS of that key
// is the small difference dP - delta of two numbers of size |dout . v|: with delta = dout . out the two are separately rounded
// 64-term dot products and the difference carries ~sqrt(64) roundings of that size; with delta = sum_j P_ij dP_ij the key's own
// rounded dP is the leading term of delta and drops out up to the rounding of the sum -- what an explicit softmax backward does.
// One float of lse2 resolves exp2's argument to ulp(lse2) / 2 only (at |lse2| ~ 100 every P of a row is off by a common factor of up
// to 1 +- 2.6e-6), so the row sum n_i = sum_j p_ij of the recomputed p = exp2(s2 - lse2) is taken too, P = p / n, and
//   dS_ij = (p_ij / n_i) (fma(dP_ij, n_i, -D_i) / n_i),  D_i = sum_j p_ij dP_ij:
// the fused multiply-add forms dP n - D exactly and rounds once.  n and D are summed with one partial per score register (a key's
// term meets L / 32 + 5 additions, not L) and combined in a fixed tree.  The dQ kernel makes a first pass over the keys for n and D
// (S and dP only: 4 of its 10 L^2 d products), writes them to the workspace and makes the second pass for dQ; the dK/dV kernel
// reads them.
//
// Precision and order: every product on v_mfma_f32_32x32x2_f32 (fp32 products, fp32 accumulation in program order), no atomics:
// each dqkv element is summed by one wave in a fixed order, bit-reproducible from call to call.
//
// Two kernels on one stream, both with the forward's block shape (4 waves, a wave owns 32 rows of one (batch, head)):
//   mha_bwd_dq_f32_kernel     a lane owns one QUERY row: q and dout rows in registers, K and V tiles (32 keys) double-buffered in
//       LDS.  S^T = K Q^T and dP^T = V dout^T leave each lane with the scores of its query (keys attn_crow(i, lane / 32), the
//       forward's layout); dS^T stays in those registers and is the A operand of dQ += dS K (MFMA step i: keys attn_crow(i, 0 / 1);
//       B = K[key][dim] read from the same LDS image with ds_read_b32, conflict-free: 32 consecutive floats per half).  Two passes
//       over the keys (above); n and D go to the workspace.
//   mha_bwd_dkdv_f32_kernel   a lane owns one KEY row: k and v rows in registers; Q (scaled and plain), dout, lse, n and D tiles
//       (32 query rows) double-buffered in LDS.  S = Q K^T and dP = dout V^T have the query rows as accumulator rows, so lse, n and
//       D of row attn_crow(i, lane / 32) are LDS broadcasts; P and dS are the A operands of dV += P^T dout and dK += dS^T Q
//       (B = dout / Q [query][dim] from LDS as above).
// The dQ / dK / dV accumulators hold [row attn_crow(i, hi)][dim lane % 32]: a store instruction writes two rows of 32 consecutive
// floats.
// Tails: rows >= L are zeros in registers / LDS and are not stored.  dQ kernel: keys >= L get s = -inf, P = 0.  dK/dV kernel: query
// rows >= L get lse = +inf (p = exp2(0 - inf) = 0), n = 1 / n = D = 0 and dout = 0: dS = 0 (0 0 - 0) 0 = 0, they contribute exactly
// nothing.
#pragma once
#include "gq_attn.h"

namespace gqhip {

constexpr float kAttnQScale = 0.18033688011112042f;   // log2(e) / 8, the forward's
constexpr float kAttnGScale = 0.125f;                 // 1 / sqrt(d)

// 16 MFMA steps: acc0/acc1 [row][dim r (+32)] += sum over the 32 tile rows c of a[c -> register i] * tile[c][dim], tile row stride
// kAttnKS; register i of lane half hi is tile row attn_crow(i, hi)
__device__ __forceinline__ void attn_bwd_accumulate(f32x16 &acc0, f32x16 &acc1, const f32x16 &a, const float *tile, int r, int hi) {
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const float *p = tile + attn_crow(i, hi) * kAttnKS + r;
    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], p[0], acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], p[32], acc1, 0, 0, 0);
  }
}

// acc [tile row][lane's row] = sum over the 64 dims of tile[row][dim] * x[dim] (the forward's S^T = K Q^T with x = the lane's 32
// dims 32 hi + s): MFMA step s multiplies dims (s, 32 + s)
__device__ __forceinline__ f32x16 attn_bwd_scores(const float *tile, const float (&x)[32], int r, int hi) {
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  const float *tp = tile + r * kAttnKS + 32 * hi;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const f32x4 t = *reinterpret_cast<const f32x4 *>(tp + 4 * j);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(t.x, x[4 * j + 0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(t.y, x[4 * j + 1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(t.z, x[4 * j + 2], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(t.w, x[4 * j + 3], acc, 0, 0, 0);
  }
  return acc;
}

// the lane's half row (32 floats at p) into registers, times `scale`
__device__ __forceinline__ void attn_bwd_load_row(float (&x)[32], const float *p, bool valid, float scale) {
  if (valid) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const f32x4 t = *reinterpret_cast<const f32x4 *>(p + 4 * j);
      x[4 * j + 0] = t.x * scale; x[4 * j + 1] = t.y * scale; x[4 * j + 2] = t.z * scale; x[4 * j + 3] = t.w * scale;
    }
  } else {
#pragma unroll
    for (int s = 0; s < 32; ++s) x[s] = 0.f;
  }
}

// rows [row0 + attn_crow(i, hi)] < L of a wave's two accumulators to dst (row stride rs; dst points at row row0, dim 0 of the
// head's column block)
__device__ __forceinline__ void attn_bwd_store(float *dst, long rs, const f32x16 &a0, const f32x16 &a1, int row0, int L, int r,
                                               int hi) {
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int c = attn_crow(i, hi);
    if (row0 + c < L) {
      float *p = dst + (long)c * rs + r;
      p[0] = a0[i];
      p[32] = a1[i];
    }
  }
}

struct AttnBwdKVRegs {
  f32x4 k[2], v[2];
};

// thread t moves float4 number t and t + 256 of the two 32 x 64 tiles at a / b (row strides rsa / rsb; zeros beyond L)
__device__ __forceinline__ void attn_bwd_load_tiles(AttnBwdKVRegs &g, const float *a, long rsa, const float *b, long rsb, int row0,
                                                    int L, int tid) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int idx = tid + 256 * j, row = idx >> 4, d4 = idx & 15;
    if (row0 + row < L) {
      g.k[j] = *reinterpret_cast<const f32x4 *>(a + (long)(row0 + row) * rsa + 4 * d4);
      g.v[j] = *reinterpret_cast<const f32x4 *>(b + (long)(row0 + row) * rsb + 4 * d4);
    } else {
      g.k[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      g.v[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }
}

// sum of the 16 partials in a fixed tree
__device__ __forceinline__ float attn_bwd_tree16(const f32x16 &x) {
  return (((x[0] + x[1]) + (x[2] + x[3])) + ((x[4] + x[5]) + (x[6] + x[7]))) +
         (((x[8] + x[9]) + (x[10] + x[11])) + ((x[12] + x[13]) + (x[14] + x[15])));
}

// grid = (ceil(L / 128), B * H), block = 256.  Writes the q block of dqkv, rown[B][H][L] = n and rowd[B][H][L] = D (header).
__global__ __launch_bounds__(256, 2) void mha_bwd_dq_f32_kernel(const float *__restrict__ qkv, const float *__restrict__ lse,
                                                                 const float *__restrict__ dout, float *__restrict__ dqkv,
                                                                 float *__restrict__ rown, float *__restrict__ rowd, int L, int E,
                                                                 int H) {
  __shared__ __attribute__((aligned(16))) float sK[2][kAttnKT * kAttnKS];
  __shared__ __attribute__((aligned(16))) float sV[2][kAttnKT * kAttnKS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hi = lane >> 5, r = lane & 31;
  const int bh = blockIdx.y, b = bh / H, h = bh - b * H;
  const long rs = 3L * E;
  const float *qbase = qkv + (long)b * L * rs + (long)h * kAttnD;
  const float *kbase = qbase + E;
  const float *vbase = qbase + 2 * E;
  const int wrow0 = blockIdx.x * kAttnQRows + wave * 32, qrow = wrow0 + r;
  const bool valid = qrow < L;

  float q[32], dO[32];
  attn_bwd_load_row(q, qbase + (long)qrow * rs + 32 * hi, valid, kAttnQScale);
  attn_bwd_load_row(dO, dout + ((long)b * L + qrow) * E + (long)h * kAttnD + 32 * hi, valid, 1.f);
  const float lse2 = valid ? lse[(long)bh * L + qrow] : 0.f;

  f32x16 a0, a1;                                                 // pass 0: the partials of n and D; pass 1: dQ, dims 0-31 / 32-63
#pragma unroll
  for (int i = 0; i < 16; ++i) { a0[i] = 0.f; a1[i] = 0.f; }
  float n = 0.f, D = 0.f;

  const int ntiles = (L + kAttnKT - 1) / kAttnKT;
  AttnBwdKVRegs pre;
  auto stage = [&](int buf) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int idx = tid + 256 * j, key = idx >> 4, d4 = idx & 15;
      *reinterpret_cast<f32x4 *>(sK[buf] + key * kAttnKS + 4 * d4) = pre.k[j];
      *reinterpret_cast<f32x4 *>(sV[buf] + key * kAttnKS + 4 * d4) = pre.v[j];
    }
  };
  attn_bwd_load_tiles(pre, kbase, rs, vbase, rs, 0, L, tid);
  stage(0);
  __syncthreads();

  // the tiles stream twice through the same two buffers: iteration it is tile it (pass 0) or it - ntiles (pass 1)
  for (int it = 0; it < 2 * ntiles; ++it) {
    const bool second = it >= ntiles;
    const int buf = it & 1, k0 = (second ? it - ntiles : it) * kAttnKT;
    if (it + 1 < 2 * ntiles) {
      const int tn = it + 1 >= ntiles ? it + 1 - ntiles : it + 1;
      attn_bwd_load_tiles(pre, kbase, rs, vbase, rs, tn * kAttnKT, L, tid);
    }
    if (it == ntiles) {                                          // between the passes: the row's n and D, both halves alike
      n = attn_bwd_tree16(a0);
      D = attn_bwd_tree16(a1);
      const float n1 = __shfl_xor(n, 32), D1 = __shfl_xor(D, 32);
      n = hi ? n1 + n : n + n1;                                  // (lower half) + (upper half) in both halves
      D = hi ? D1 + D : D + D1;
      if (valid && hi == 0) {
        rown[(long)bh * L + qrow] = n;
        rowd[(long)bh * L + qrow] = D;
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) { a0[i] = 0.f; a1[i] = 0.f; }
    }

    f32x16 s = attn_bwd_scores(sK[buf], q, r, hi);               // S^T[key][query], the forward's bits
    const f32x16 dp = attn_bwd_scores(sV[buf], dO, r, hi);       // dP^T[key][query]
    if (k0 + kAttnKT > L) {
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (k0 + attn_crow(i, hi) >= L) s[i] = -__builtin_inff();
    }
    if (!second) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float p = exp2f(s[i] - lse2);
        a0[i] += p;
        a1[i] = __builtin_fmaf(p, dp[i], a1[i]);
      }
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i) s[i] = exp2f(s[i] - lse2) * __builtin_fmaf(dp[i], n, -D);   // dS^T n^2
      attn_bwd_accumulate(a0, a1, s, sK[buf], r, hi);            // dQ[query][dim] += dS[query][key] K[key][dim]
    }

    // the buffer written here was last read in iteration it - 1, which every wave finished before the previous barrier
    if (it + 1 < 2 * ntiles) stage(buf ^ 1);
    __syncthreads();
  }
  const float inv = valid ? 1.f / n : 0.f;                       // a row < L has a key whose p is ~ its share of 1: n > 0
  // the accumulators hold query rows attn_crow(i, hi), not the lane's own: their 1 / n comes from lane attn_crow(i, hi)
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const float iv = __shfl(inv, attn_crow(i, hi));
    a0[i] = a0[i] * iv * iv * kAttnGScale;
    a1[i] = a1[i] * iv * iv * kAttnGScale;
  }
  attn_bwd_store(dqkv + ((long)b * L + wrow0) * rs + (long)h * kAttnD, rs, a0, a1, wrow0, L, r, hi);
}

// grid = (ceil(L / 128), B * H), block = 256, after mha_bwd_dq_f32_kernel on the same stream (it reads n and D).  Writes the k and
// v blocks of dqkv.
__global__ __launch_bounds__(256, 2) void mha_bwd_dkdv_f32_kernel(const float *__restrict__ qkv, const float *__restrict__ lse,
                                                                   const float *__restrict__ dout, const float *__restrict__ rown,
                                                                   const float *__restrict__ rowd, float *__restrict__ dqkv,
                                                                   int L, int E, int H) {
  __shared__ __attribute__((aligned(16))) float sQs[2][kAttnKT * kAttnKS];   // q log2(e) / 8: the A operand of S
  __shared__ __attribute__((aligned(16))) float sQ[2][kAttnKT * kAttnKS];    // q: the B operand of dK
  __shared__ __attribute__((aligned(16))) float sO[2][kAttnKT * kAttnKS];    // dout
  __shared__ float sLse[2][kAttnKT], sN[2][kAttnKT], sD[2][kAttnKT], sInv[2][kAttnKT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hi = lane >> 5, r = lane & 31;
  const int bh = blockIdx.y, b = bh / H, h = bh - b * H;
  const long rs = 3L * E;
  const float *qbase = qkv + (long)b * L * rs + (long)h * kAttnD;
  const float *obase = dout + (long)b * L * E + (long)h * kAttnD;
  const float *lbase = lse + (long)bh * L, *nbase = rown + (long)bh * L, *dbase = rowd + (long)bh * L;
  const int wrow0 = blockIdx.x * kAttnQRows + wave * 32, krow = wrow0 + r;

  float k[32], v[32];
  attn_bwd_load_row(k, qbase + E + (long)krow * rs + 32 * hi, krow < L, 1.f);
  attn_bwd_load_row(v, qbase + 2 * E + (long)krow * rs + 32 * hi, krow < L, 1.f);

  f32x16 k0a, k1a, v0a, v1a;
#pragma unroll
  for (int i = 0; i < 16; ++i) { k0a[i] = 0.f; k1a[i] = 0.f; v0a[i] = 0.f; v1a[i] = 0.f; }

  const int ntiles = (L + kAttnKT - 1) / kAttnKT;
  AttnBwdKVRegs pre;                                             // .k: the Q tile, .v: the dout tile
  float pl = 0.f, pd = 0.f, pn = 0.f;
  auto load = [&](int q0) {
    attn_bwd_load_tiles(pre, qbase, rs, obase, E, q0, L, tid);
    if (tid < kAttnKT) {
      const bool in = q0 + tid < L;
      pl = in ? lbase[q0 + tid] : __builtin_inff();
      pn = in ? nbase[q0 + tid] : 0.f;
      pd = in ? dbase[q0 + tid] : 0.f;
    }
  };
  auto stage = [&](int buf) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int idx = tid + 256 * j, row = idx >> 4, d4 = idx & 15;
      const f32x4 t = pre.k[j];
      *reinterpret_cast<f32x4 *>(sQ[buf] + row * kAttnKS + 4 * d4) = t;
      *reinterpret_cast<f32x4 *>(sQs[buf] + row * kAttnKS + 4 * d4) =
          f32x4{t.x * kAttnQScale, t.y * kAttnQScale, t.z * kAttnQScale, t.w * kAttnQScale};
      *reinterpret_cast<f32x4 *>(sO[buf] + row * kAttnKS + 4 * d4) = pre.v[j];
    }
    if (tid < kAttnKT) {
      sLse[buf][tid] = pl;
      sN[buf][tid] = pn;
      sD[buf][tid] = pd;
      sInv[buf][tid] = pn > 0.f ? 1.f / pn : 0.f;
    }
  };
  load(0);
  stage(0);
  __syncthreads();

  for (int t = 0; t < ntiles; ++t) {
    const int buf = t & 1;
    if (t + 1 < ntiles) load((t + 1) * kAttnKT);

    f32x16 p = attn_bwd_scores(sQs[buf], k, r, hi);              // S[query][key], the forward's bits
    f32x16 ds = attn_bwd_scores(sO[buf], v, r, hi);              // dP[query][key]
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int c = attn_crow(i, hi);
      const float iv = sInv[buf][c];
      p[i] = exp2f(p[i] - sLse[buf][c]) * iv;
      ds[i] = p[i] * (__builtin_fmaf(ds[i], sN[buf][c], -sD[buf][c]) * iv);
    }
    attn_bwd_accumulate(v0a, v1a, p, sO[buf], r, hi);            // dV[key][dim] += P[query][key] dout[query][dim]
    attn_bwd_accumulate(k0a, k1a, ds, sQ[buf], r, hi);           // dK[key][dim] += dS[query][key] Q[query][dim]

    if (t + 1 < ntiles) stage(buf ^ 1);
    __syncthreads();
  }
  float *dst = dqkv + ((long)b * L + wrow0) * rs + (long)h * kAttnD;
#pragma unroll
  for (int i = 0; i < 16; ++i) { k0a[i] *= kAttnGScale; k1a[i] *= kAttnGScale; }
  attn_bwd_store(dst + E, rs, k0a, k1a, wrow0, L, r, hi);
  attn_bwd_store(dst + 2 * E, rs, v0a, v1a, wrow0, L, r, hi);
}

}  // namespace gqhip
