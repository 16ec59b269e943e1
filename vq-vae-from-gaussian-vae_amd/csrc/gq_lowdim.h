// gq_lowdim.h -- the fused Gaussian arg-max at codebook dims 1, 2 and 3 (gqhip.h: gqhip_set_low_dims): an exact, PRUNED search over
// a cell index of the codebook instead of gq_exhaustive_kernel's score of every code.
//
// Why: 65 536 codes are so dense in one to three dimensions that zero-padding to dim 4 would leave every row in the dim-4 search's
// finish scan.  The same density makes a direct search cheap: the codes whose score lies within the rounding
// margin of a row's best are a few hundred at dim 1 and a handful at dims 2 and 3, so the reference's arithmetic
// is needed for those, not for 65 536.
//
// Index (the caller's codebook cache; its protocol and the builder's steps: gq_index.h): the codes bucketed into 4096 CELLS by per-axis
// thresholds at the normal quantiles of the book's own mean and deviation -- 4096 at dim 1, 64 x 64 at dim 2, 16 x 16 x 16 at dim 3 --
// each cell with the TIGHT bounding box of its members (at dim 1: the interval [min, max] of a run of the value-ordered book) and
// their original indices; 256 COARSE nodes of 16 neighbouring cells each (16 consecutive cells, 4 x 4, 2 x 2 x 4), whose boxes
// (at most 6 KiB) the search holds in LDS.  A NaN coordinate sorts into cell 0 of its axis, as in grid_sub_of.
//
// Search, 16 lanes (one DPP row) per row:
//   (1) A_i, B_i and the four bound sums from mu, sd, log sd -- the definitions of gq_prep_kernel -- and T, G from row_bound;
//   (2) every lane bounds 16 coarse nodes (closed form of a separable quadratic over a box: grid_box_ub_v); the best node's best
//       cell is scored with the fp32 FMA expansion f^ -> a first F;
//   (3) the coarse nodes, then their cells, whose bound is >= F - margin32; in such a cell the codes with f^ >= F - margin32 receive
//       the reference's arithmetic (ref_score_lds<DIM>: operation for operation ref_score_ops(n, ro, DIM, beta)), F tightening
//       after every cell;
//   (4) the winner in torch.argmax order (score, then lowest ORIGINAL index; NaN first), stored with ordinary vector stores.
// At dim 1 the passing cells are one contiguous run of the value-ordered book around the parabola's vertex (A < 0), or a run at
// either end (A >= 0): {n : A n^2 + B n >= t} is an interval or the complement of one.  The run is found by the same box test as
// at dims 2 and 3 and not by solving the quadratic, so no square root or division enters the argument and there is no extra term;
// a node's run is then scored in ONE pass from its first to its last passing cell (a superset of the passing cells).
//
// Exactness (the argument of gq_grid.h, with its margin):  f^ = the fp32 FMA expansion, |f^ - f| <= E32 = (2 dim + 4) u T;  E_r
// bounds the reference score's own rounding (gq_rerank.h:row_bound);  margin32 = 2.5 (E32 + E_r).
//   * The reference's arg-max j* has f(j*) >= f(j^) - 2 E_r for every code j^, in particular the one that set F:
//     f(j*) >= F - E32 - 2 E_r.
//   * A box (cell or coarse node; at dim 1 an interval) that holds j* has a true upper bound >= f(j*), and its computed bound is
//     below the true one by at most (dim + 1) u T <= E32: it passes  F - margin32  whatever F was at the time (F only grows).
//   * In its cell, f^(j*) >= F - 2 E32 - 2 E_r >= F - margin32: j* receives the reference's arithmetic, as does every code that
//     could tie with it, and the (score, index) order names the winner.  The global margin is kept; no local bound is used.
// Rows that get gq_exhaustive_kernel's semantics instead -- appended to the call's row list and finished by that very kernel, the
// launch after the search, a block per row over ALL codes (it exits at once when the list is empty): a non-finite operand, bound
// or codebook; sigma <= 0; a row whose candidates include an overfull cell (more than low_cell_cap(n) codes: a clustered or
// collapsed book; gqhip_cb_cache_degenerate reports it).  There are no candidate lists, so nothing overflows.
#pragma once
#include "gq_common.h"
#include "gq_grid.h"
#include "gq_index.h"
#include "gq_rerank.h"

namespace gqhip {

constexpr unsigned kLowMagic = 0x47514c31u;
constexpr int kLowCells = 4096, kLowCoarse = 256, kLowFan = kLowCells / kLowCoarse;
constexpr int kLowBuildThreads = 1024;
constexpr int kLowThreads = 256;                   // 16 rows per block pass
constexpr int kLowHashBlocks = kAbsmaxParts;

// cells per axis
__host__ __device__ constexpr int low_axis_cells(int dim) { return dim == 1 ? 4096 : (dim == 2 ? 64 : 16); }
// codes in a cell beyond which a row that lists it is handed to the finish launch: 16 times the mean cell
__host__ __device__ inline int low_cell_cap(int64_t n) { return (int)(n / 256 > 256 ? n / 256 : 256); }

struct LowLayout {
  int64_t hdr, cbox, box, start, scb, sidx, total;
};
__host__ __device__ inline LowLayout low_layout(int64_t n, int64_t dim) {
  LowLayout g{};
  int64_t off = 0;
  g.hdr = off;   off += (int64_t)sizeof(GridHdr);
  g.cbox = off;  off += grid_align((int64_t)kLowCoarse * 2 * dim * 4);
  g.box = off;   off += grid_align((int64_t)kLowCells * 2 * dim * 4);
  g.start = off; off += grid_align((kLowCells + 16) * 4);
  g.scb = off;   off += grid_align(n * dim * 4);
  g.sidx = off;  off += grid_align(n * 4);
  g.total = off;
  return g;
}

// ---------------------------------------------------------------------------------------------------- codebook hash (256 blocks)
// What gq_prep_kernel's code blocks do on the dim-4 route, for a call whose rows are prepared by prep_plain_kernel (gq_index.h:
// cb_hash_block).
struct LowHashParams {
  const float *cb;
  WsHeader *hdr;
  GridHdr *cache;
  long count;             // n * dim
};
__global__ __launch_bounds__(256) void gq_low_hash_kernel(const LowHashParams p) {
  cb_hash_block(p.cb, p.count, blockIdx.x, kLowHashBlocks, threadIdx.x, p.hdr, p.cache->blk_sum, &p.cache->stale);
}

// ---------------------------------------------------------------------------------------------------- builder (one block; gq_index.h)
// N(0, 1) quantile (P. J. Acklam's rational approximation, relative error 1e-9): any ascending thresholds are valid, these balance a
// Gaussian book.
__device__ inline double low_norm_quantile(double pr) {
  const double a[6] = {-3.969683028665376e+01, 2.209460984245205e+02, -2.759285104469687e+02,
                       1.383577518672690e+02, -3.066479806614716e+01, 2.506628277459239e+00};
  const double b[5] = {-5.447609879822406e+01, 1.615858368580409e+02, -1.556989798598866e+02, 6.680131188771972e+01,
                       -1.328068155288572e+01};
  const double c[6] = {-7.784894002430293e-03, -3.223964580411365e-01, -2.400758277161838e+00,
                       -2.549732539343734e+00, 4.374664141464968e+00, 2.938163982698783e+00};
  const double d[4] = {7.784695709041462e-03, 3.224671290700398e-01, 2.445134137142996e+00, 3.754408661907416e+00};
  const double plow = 0.02425;
  if (pr < plow || pr > 1.0 - plow) {
    const double q = sqrt(-2.0 * log(pr < plow ? pr : 1.0 - pr));
    const double v = (((((c[0] * q + c[1]) * q + c[2]) * q + c[3]) * q + c[4]) * q + c[5]) /
                     ((((d[0] * q + d[1]) * q + d[2]) * q + d[3]) * q + 1.0);
    return pr < plow ? v : -v;
  }
  const double q = pr - 0.5, r = q * q;
  return (((((a[0] * r + a[1]) * r + a[2]) * r + a[3]) * r + a[4]) * r + a[5]) * q /
         (((((b[0] * r + b[1]) * r + b[2]) * r + b[3]) * r + b[4]) * r + 1.0);
}

// thresholds t[0 .. cells - 2] ascending: the number of them that are <= x (NaN: 0)
__device__ __forceinline__ int low_axis_cell(float x, const float *t, int cells) {
  int lo = 0, hi = cells - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (x >= t[mid]) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// cell id: coarse node * 16 + cell of the node; a node is 16 consecutive cells (dim 1), 4 x 4 (dim 2), 2 x 2 x 4 (dim 3)
template <int DIM>
__device__ __forceinline__ int low_cell_of(const float (&x)[DIM], const float *thr) {
  constexpr int C = low_axis_cells(DIM);
  int c[DIM];
#pragma unroll
  for (int i = 0; i < DIM; ++i) c[i] = low_axis_cell(x[i], thr + i * C, C);
  if constexpr (DIM == 1) return c[0];
  else if constexpr (DIM == 2) return (((c[0] >> 2) * 16 + (c[1] >> 2)) * 16) + (c[0] & 3) * 4 + (c[1] & 3);
  else return ((((c[0] >> 1) * 8 + (c[1] >> 1)) * 4 + (c[2] >> 2)) * 16) + (c[0] & 1) * 8 + (c[1] & 1) * 4 + (c[2] & 3);
}

template <int DIM>
__global__ __launch_bounds__(kLowBuildThreads) void gq_low_build_kernel(const IndexBuildParams p) {
  GridHdr *gh = reinterpret_cast<GridHdr *>(p.cache);
  if (index_current(gh, kLowMagic, p.n, DIM)) return;   // (block-uniform)
  const LowLayout L = low_layout(p.n, DIM);
  float *cbox = reinterpret_cast<float *>(p.cache + L.cbox), *box = reinterpret_cast<float *>(p.cache + L.box);
  int *start = reinterpret_cast<int *>(p.cache + L.start);
  float *scb = reinterpret_cast<float *>(p.cache + L.scb);
  int *sidx = reinterpret_cast<int *>(p.cache + L.sidx);
  constexpr int NT = kLowBuildThreads, C = low_axis_cells(DIM);
  const int tid = threadIdx.x;
  __shared__ double s_red[NT / 64][2 * DIM];
  __shared__ double s_ms[2 * DIM];
  __shared__ float s_thr[DIM * C];
  __shared__ int s_cnt[kLowCells];
  __shared__ int s_wsum[NT / 64];

  // thresholds at the normal quantiles k / C of each axis' own mean and deviation
  index_moments<DIM, NT>(p.cb, p.n, tid, s_red);
  __syncthreads();
  if (tid < DIM) index_mean_sd<DIM, NT>(s_red, tid, p.n, s_ms[tid], s_ms[DIM + tid]);
  __syncthreads();
  for (int k = tid; k < DIM * C; k += NT) {
    const int i = k / C, t = k % C;
    s_thr[k] = t < C - 1 ? (float)(s_ms[i] + s_ms[DIM + i] * low_norm_quantile((double)(t + 1) / C)) : __builtin_inff();
  }
  const auto cell_of = [&](const float (&x)[DIM]) { return low_cell_of<DIM>(x, s_thr); };
  index_histogram_census<DIM, NT>(p.cb, p.n, tid, s_cnt, cell_of, &gh->max_sub);
  static_assert(kLowCells == kIndexBuckets, "the builder's bucket count");
  index_scan4096<NT, false>(tid, s_cnt, s_wsum, start, nullptr);
  index_scatter<DIM, NT>(p.cb, p.n, tid, s_cnt, cell_of, scb, sidx);
  index_tight_boxes<DIM, NT>(start, scb, box, tid);
  index_merge_boxes<DIM>(box, cbox, kLowCoarse, kLowFan, tid);
  index_stamp(gh, p.hdr, p.n, DIM, kLowMagic, tid);
}

// ---------------------------------------------------------------------------------------------------- the search
struct LowParams {
  const float *mu, *sd, *lsd;      // [rows, dim]; lsd may be NULL (fp64 log of sd, as load_row_ops)
  const float *cb;                 // [n, dim] the caller's codebook (the stored code word)
  const char *cache;               // the codebook cache (low_layout)
  int64_t *idx;
  float *zhat;                     // may be NULL
  WsHeader *hdr;
  int *fb_list;                    // [rows] rows handed to the finish launch (hdr->fb_count of them)
  int rows, n;
  float beta;
  int stats;
  OutMap omap;
};

template <int DIM>
__global__ __launch_bounds__(kLowThreads) void gq_low_search_kernel(const LowParams p) {
  constexpr int GROUP = 16, RPB = kLowThreads / GROUP, BOXF = 2 * DIM, CPL = kLowCoarse / GROUP;
  __shared__ float s_cbox[kLowCoarse * BOXF];
  const LowLayout L = low_layout(p.n, DIM);
  const float *gbox = reinterpret_cast<const float *>(p.cache + L.box);
  const int *gstart = reinterpret_cast<const int *>(p.cache + L.start);
  const float *scb = reinterpret_cast<const float *>(p.cache + L.scb);
  const int *sidx = reinterpret_cast<const int *>(p.cache + L.sidx);
  const int tid = threadIdx.x, lane = tid & 63;
  const int sub = lane % GROUP, gshift = (lane / GROUP) * GROUP;
  auto group_bits = [&](bool c) { return (unsigned)((__builtin_amdgcn_ballot_w64(c) >> gshift) & 0xffffull); };
  {
    const float *src = reinterpret_cast<const float *>(p.cache + L.cbox);
    for (int k = tid; k < kLowCoarse * BOXF; k += kLowThreads) s_cbox[k] = src[k];
  }
  const float N1f = wave_absmax(p.hdr->absmax_part, lane);
  const int cap = low_cell_cap(p.n);
  const float NEG_INF = -__builtin_inff();
  __syncthreads();

  const int nsets = (p.rows + RPB - 1) / RPB;
  for (int set = (int)blockIdx.x; set < nsets; set += (int)gridDim.x) {
    const long pos_raw = (long)set * RPB + tid / GROUP;
    const bool live = pos_raw < p.rows;
    const long row = live ? pos_raw : p.rows - 1;
    // ---- (1) row operands, coefficients and bound sums: gq_prep_kernel's definitions
    float ops[3 * DIM], cA[DIM], cB[DIM], cM[DIM];
    double rs[4] = {0.0, 0.0, 0.0, 0.0};
    bool concave = true;
#pragma unroll
    for (int i = 0; i < DIM; ++i) {
      const float m = p.mu[row * DIM + i], s = p.sd[row * DIM + i];
      const float ls = p.lsd ? p.lsd[row * DIM + i] : (float)log((double)s);
      ops[i] = m;
      {
#pragma clang fp contract(off)
        ops[DIM + i] = 2.0f * (s * s);
      }
      ops[2 * DIM + i] = ls;
      const double sg = (double)s;
      double inv = 1.0 / (sg * sg);
      cA[i] = (float)(0.5 * (double)p.beta - 0.5 * inv);
      cB[i] = (float)((double)m * inv);
      if (!(sg > 0.0)) inv = __builtin_nan("");   // sd <= 0 or NaN: the row's bound is NaN -> exhaustive semantics
      const double am = fabs((double)m);
      rs[0] += inv; rs[1] += am * inv; rs[2] += am * am * inv; rs[3] += fabs((double)ls);
      // the parabola's vertex to within an ulp or two: a bound evaluated a relative 1e-7 beside it is below the true one by
      // ~|A| mu'^2 1e-14, nothing against E32 (gq_grid.h)
      cM[i] = cA[i] < 0.0f ? -0.5f * cB[i] * __builtin_amdgcn_rcpf(cA[i]) : 0.0f;
      concave = concave && cA[i] < 0.0f;
    }
    const double u = 5.9604644775390625e-08;  // 2^-24
    const double N1 = (double)N1f;
    double T, G;
    row_bound<kModeGQ>(rs, N1, DIM, p.beta, T, G);
    const double Er = (DIM + 16.0) * u * G;
    const float margin32 = (float)(2.5 * ((2.0 * DIM + 4.0) * u * T + Er) * 1.0000002 + 1e-30);
    const bool bad = !(N1 == N1) || N1 > 1e18 || !(T < 1e30) || !(G < 1e30) || !(margin32 < 1e30f);

    auto expansion = [&](const float (&n)[DIM]) {
      float f = 0.0f;
#pragma unroll
      for (int i = 0; i < DIM; ++i) f = __builtin_fmaf(__builtin_fmaf(cA[i], n[i], cB[i]), n[i], f);
      return f;
    };
    // thr: what a box / a code must reach (rounded down: the subtraction and F's own last bit)
    auto thr_of = [&](float Fv) { return Fv > NEG_INF ? (Fv - margin32) - 2.4e-7f * __builtin_fabsf(Fv) : NEG_INF; };
    auto cell_range = [&](int cell, int &s, int &e) {      // clamped: a cache body written behind the library's back costs a wrong
      s = min(max(gstart[cell], 0), p.n);                  // index at worst, never an out-of-range read (gqhip.h, codebook cache)
      e = min(max(gstart[cell + 1], s), p.n);
    };
    auto load_code = [&](int j, float (&n)[DIM]) {
#pragma unroll
      for (int i = 0; i < DIM; ++i) n[i] = scb[(long)j * DIM + i];
    };
    float F = NEG_INF, thr = NEG_INF;
    double best_s = 0.0;
    int best_i = 0x7fffffff;
    bool have = false, hand = bad;
    unsigned exact_n = 0u;
    // the codes [s, e) of the cell-ordered book: f^ for all, the reference's arithmetic for those within the margin; F and thr tighten
    // afterwards
    auto visit_codes = [&](int s, int e, bool exact) {
      float fl = NEG_INF;
      for (int j = s + sub; j < e; j += GROUP) {
        float nn[DIM];
        load_code(j, nn);
        const float f = expansion(nn);
        fl = fmax_nn(fl, f);
        if (exact && !(f < thr)) {
          const int code = (int)min((unsigned)sidx[j], (unsigned)(p.n - 1));
          const double sc = (double)ref_score_lds<DIM>(nn, ops, p.beta);
          if (!have || better_d(sc, code, best_s, best_i)) { best_s = sc; best_i = code; have = true; }
          ++exact_n;
        }
      }
      F = fmax_nn(F, row16_max<true>(fl));
      thr = thr_of(F);
    };
    auto visit_cell = [&](int cell, bool exact) {
      int s, e;
      cell_range(cell, s, e);
      if (e - s > cap) hand = true;                  // (group-uniform)
      else visit_codes(s, e, exact);
    };

    if (!hand) {
      // ---- (2) coarse bounds (16 per lane), a first F from the best node's best cell
      float ubl = NEG_INF;
      int kb = 0;
      auto node_ub = [&](int k) {
        const float *b = s_cbox + (k * GROUP + sub) * BOXF;
        float lo[DIM], hi[DIM];
#pragma unroll
        for (int i = 0; i < DIM; ++i) { lo[i] = b[i]; hi[i] = b[DIM + i]; }
        return grid_box_ub_v<DIM>(cA, cB, cM, lo, hi, concave);
      };
#pragma unroll
      for (int k = 0; k < CPL; ++k) {
        const float v = node_ub(k);
        if (v > ubl) { ubl = v; kb = k; }
      }
      auto cell_ub = [&](int cell) {
        const float *b = gbox + (long)cell * BOXF;
        float lo[DIM], hi[DIM];
#pragma unroll
        for (int i = 0; i < DIM; ++i) { lo[i] = b[i]; hi[i] = b[DIM + i]; }
        return grid_box_ub_v<DIM>(cA, cB, cM, lo, hi, concave);
      };
      {
        const float ubg = row16_max<true>(ubl);
        const unsigned who = group_bits(ubl == ubg && ubg > NEG_INF);
        if (who == 0u) {
          hand = true;                                  // no node with a bound (cannot happen behind a finite book): all codes
        } else {
          const int l = __builtin_ctz(who);
          const int node = __shfl(kb, gshift + l) * GROUP + l;
          const float cu = cell_ub(node * kLowFan + sub);
          const float cg = row16_max<true>(cu);
          const unsigned cw = group_bits(cu == cg && cg > NEG_INF);
          if (cw == 0u) hand = true;
          else visit_cell(node * kLowFan + __builtin_ctz(cw), false);
        }
      }
      // ---- (3) every coarse node, then cell, within the margin; the reference's arithmetic inside the cells
      if (!hand && !(F > NEG_INF)) hand = true;
      for (int k = 0; k < CPL; ++k) {
        unsigned bits = hand ? 0u : group_bits(!(node_ub(k) < thr));
        while (bits != 0u && !hand) {
          const int l = __builtin_ctz(bits);
          bits &= bits - 1u;
          const int node = k * GROUP + l;
          const float cu = cell_ub(node * kLowFan + sub);
          unsigned cbits = group_bits(!(cu < thr));
          if constexpr (DIM == 1) {
            // the node's passing cells are neighbours in the value-ordered book (one run around the vertex, or one at an end of the
            // book): one pass over the codes from the first to the last of them, whatever lies between included
            if (cbits != 0u) {
              const int first = __builtin_ctz(cbits), last = 31 - __builtin_clz(cbits);
              int cs, ce;
              cell_range(node * kLowFan + sub, cs, ce);
              if (group_bits(sub >= first && sub <= last && ce - cs > cap) != 0u) hand = true;
              else visit_codes(__shfl(cs, gshift + first), __shfl(ce, gshift + last), true);
            }
            cbits = 0u;
          }
          while (cbits != 0u && !hand) {
            const int c = __builtin_ctz(cbits);
            cbits &= cbits - 1u;
            if (!(__shfl(cu, gshift + c) < thr)) visit_cell(node * kLowFan + c, true);   // (thr may have tightened since the ballot)
          }
        }
      }
      if (!hand) {
        // ---- (4) the winner of the row's 16 lanes, torch.argmax order
#pragma unroll
        for (int o = GROUP / 2; o > 0; o >>= 1) {
          const double os = __shfl_xor(best_s, o);
          const int oi = __shfl_xor(best_i, o);
          const bool oh = __shfl_xor(have ? 1 : 0, o) != 0;
          if (oh && (!have || better_d(os, oi, best_s, best_i))) { best_s = os; best_i = oi; have = true; }
        }
        if (!have) hand = true;
      }
    }
    if (live) {
      if (hand) {
        if (sub == 0) p.fb_list[atomicAdd(&p.hdr->fb_count, 1)] = (int)row;
      } else {
        if (sub == 0) p.idx[out_idx_offset(p.omap, row)] = (int64_t)best_i;
        if (p.zhat && sub < DIM) {
          const long o = out_zhat_offset(p.omap, row, sub, DIM);
          p.zhat[o] = ste_mix(p.hdr, o, p.cb[(long)best_i * DIM + sub]);
        }
        if (p.stats && exact_n != 0u) atomicAdd(&p.hdr->reranked, (unsigned long long)exact_n);   // debug: codes scored exactly
      }
    }
  }
}

}  // namespace gqhip
