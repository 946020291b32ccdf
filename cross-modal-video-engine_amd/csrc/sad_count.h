// The count kernel of the integer SAD filters, written once (K22: l1_filter.hip under CMVE_PW_L1; K24:
// jaccard_filter.hip under CMVE_PW_JACCARD): l1f_sad_tile's 128 x 128 tile on 256 threads of 8 x 8 u32 accumulators,
// then the fp64 epilogue -- the two-pass round loop over the tile's lists, the valid / band bit masks, the shuffle /
// LDS count reduction, one integer atomic per (item, tile), the band append with decided + band = pairs -- and the
// host pieces the two count entries share.  A filter supplies a policy P with only what differs:
//   P::Args                       the kernel's flat argument block: SadArgs (the common prefix) plus the filter's own
//                                 scalars and pointers
//   P::NS                         the doubles a side carries per row
//   P::Iv                         the interval of a pair
//   P::side<B>(a, v, i, lo, s, t) the terms of A row i (B: of B row i); v: the row is in the set
//   P::thresholds(a, w, t0, t1)   an item word -> the round's two thresholds
//   P::interval(a, sad, s, ta, tb)  SAD and two sides -> the pair's interval
//   P::has(iv)                    the pair has an interval
//   P::below / P::not_below(iv, pos, t0, t1)   the pair is decided below / not below the item (pos: alpha > 0)
// l2f_main_kernel keeps an epilogue of its own (another thread layout, at 256 VGPRs: DESIGN s4, "One host mechanism").
#ifndef CMVE_SAD_COUNT_H
#define CMVE_SAD_COUNT_H
#include "filter_count.h"
#include "l1_filter_tile.h"

namespace cmve {

// the common prefix of a SAD count kernel's flat argument block (a policy's Args derives from it and adds its own
// fields: one block, no nesting -- embedding FltArgs moved l1f_main_kernel's scalar loads and cost it 1.2%)
struct SadArgs {
  const uint32_t* a_codes;  // tiled (l1_filter_tile.h)
  const uint32_t* b_codes;
  const double* a_err;
  const double* b_err;
  const double* grid;
  int64_t na, nb;
  int nkt;  // K tiles
  double alpha, beta;
  const int64_t* row_off;
  const double* row_sc;
  int32_t* row_pos;
  const int64_t* col_off;
  const double* col_sc;
  int32_t* col_pos;
  int2* band;
  int64_t cap;
  l2f_u64* stats;  // {decided, band found, band re-scored, overflow}
  int tiles_a, tiles_b;
};

// the epilogue's LDS, laid over the staging buffers once the K loop is done
template <int NS>
struct SadEpi {
  double sa[NS][L1F_BM], sb[NS][L1F_BN];  // the sides' terms of the tile's rows / columns
  double rt[2][L1F_BM], ct[2][L1F_BN];    // one round's two thresholds per row / column
  int64_t ro[L1F_BM], co[L1F_BN];
  int mr[L1F_BM], mc[L1F_BN];
  int rc[L1F_BM], cc[L1F_BN];
  int s_m[2];
  int band_cnt;
  long long band_base;
  double s;  // the grid's step, re-read per row of a round (see the epilogue)
};

// one side's setup: thread t of the 128 loads the terms and the list of row i of its set
template <typename P, bool B>
__device__ __forceinline__ void sad_count_side(const typename P::Args& a, int t, int64_t i, int64_t n, double lo,
                                               double s, const int64_t* off, const int32_t* pos,
                                               double (&terms)[P::NS][L1F_BM], int64_t* eo, int* em, int* ec,
                                               int* s_m) {
  const bool v = i < n;
  double x[P::NS];
  P::template side<B>(a, v, i, lo, s, x);
#pragma unroll
  for (int k = 0; k < P::NS; ++k) terms[k][t] = x[k];
  const int64_t o = (v && pos) ? off[i] : 0;
  const int m = (v && pos) ? (int)(off[i + 1] - o) : 0;
  eo[t] = o;
  em[t] = m;
  ec[t] = 0;
  if (m) atomicMax(s_m, m);
}

template <typename P>
__device__ __forceinline__ void sad_count_body(const typename P::Args& a) {
  using Epi = SadEpi<P::NS>;
  static_assert(sizeof(Epi) <= L1F_SMEM, "the epilogue's LDS fits the staging buffers");
  __shared__ __attribute__((aligned(16))) char smem[L1F_SMEM];
  const int tid = threadIdx.x, lane = tid & 63, tx = tid & 15, ty = tid >> 4;
  int ta, tb_;
  l2f_tile_of_block(blockIdx.x, a.tiles_a, a.tiles_b, ta, tb_);
  const int64_t i0 = (int64_t)ta * L1F_BM, j0 = (int64_t)tb_ * L1F_BN;

  // ---- the SADs: acc[u][v] of the pair (A row i0 + l1f_row(ty, u), B row j0 + l1f_row(tx, v)); the tiles' blocks lie
  // below the sets' n_pad (a multiple of 128) and d_pad: in bounds
  uint32_t acc[8][8];
  l1f_sad_tile(a.a_codes + (int64_t)ta * a.nkt * L1F_TILE_DW, a.b_codes + (int64_t)tb_ * a.nkt * L1F_TILE_DW, a.nkt,
               smem, acc);

  // ---- epilogue (every wave has passed the loop's last barrier: smem is free) ------------------------------------------
  Epi& E = *(Epi*)smem;
  double lo, s;
  l1f_grid_of(a.grid, lo, s);
  if (tid < 2) E.s_m[tid] = 0;
  if (tid == 2) E.band_cnt = 0;
  if (tid == 3) E.s = s;
  __syncthreads();
  if (tid < L1F_BM)
    sad_count_side<P, false>(a, tid, i0 + tid, a.na, lo, s, a.row_off, a.row_pos, E.sa, E.ro, E.mr, E.rc, &E.s_m[0]);
  else
    sad_count_side<P, true>(a, tid - L1F_BM, j0 + tid - L1F_BM, a.nb, lo, s, a.col_off, a.col_pos, E.sb, E.co, E.mc,
                            E.cc, &E.s_m[1]);
  __syncthreads();
  const int rounds = max(E.s_m[0], E.s_m[1]);  // block-uniform
  // bit u * 8 + v of `valid`: the pair exists
  uint64_t valid = 0, band = 0;
#pragma unroll
  for (int u = 0; u < 8; ++u)
#pragma unroll
    for (int v = 0; v < 8; ++v)
      if (i0 + l1f_row(ty, u) < a.na && j0 + l1f_row(tx, v) < a.nb) valid |= 1ull << (u * 8 + v);

  // one round: item `it` of every row and column list.  PASS 0 marks the pairs some item cannot decide, PASS 1
  // counts the decided ones.
  for (int pass = 0; pass < 2; ++pass) {
    for (int it = 0; it < rounds; ++it) {
      // the item's word becomes the round's two thresholds here, once per (item, round)
      if (tid < L1F_BM) {
        double t0 = (double)NAN, t1 = (double)NAN;
        if (it < E.mr[tid]) P::thresholds(a, a.row_sc[E.ro[tid] + it], t0, t1);
        E.rt[0][tid] = t0;
        E.rt[1][tid] = t1;
      } else {
        const int t = tid - L1F_BM;
        double t0 = (double)NAN, t1 = (double)NAN;
        if (it < E.mc[t]) P::thresholds(a, a.col_sc[E.co[t] + it], t0, t1);
        E.ct[0][t] = t0;
        E.ct[1][t] = t1;
      }
      __syncthreads();
      const bool pos = a.alpha > 0.0;
      int ccnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      int rpack[2] = {0, 0};  // four rows' counts each, a byte a row (<= 8 per thread, <= 128 over the row's 16 lanes)
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int row = l1f_row(ty, u);
        // a volatile read: the 64 intervals are formed again in every round, eight at a time, instead of being
        // hoisted out of the rounds as 128 (two bounds) or 256 (four) live doubles per thread
        const double sv = *(const volatile double*)&E.s;
        double xa[P::NS];
#pragma unroll
        for (int k = 0; k < P::NS; ++k) xa[k] = E.sa[k][row];
        const double rt0 = E.rt[0][row], rt1 = E.rt[1][row];
        const bool rhas = it < E.mr[row];
        int rcnt = 0;
#pragma unroll
        for (int v = 0; v < 8; ++v) {
          const int col = l1f_row(tx, v);
          const int bit = u * 8 + v;
          double xb[P::NS];
#pragma unroll
          for (int k = 0; k < P::NS; ++k) xb[k] = E.sb[k][col];
          const typename P::Iv iv = P::interval(a, acc[u][v], sv, xa, xb);
          const bool chas = it < E.mc[col];
          const double ct0 = E.ct[0][col], ct1 = E.ct[1][col];
          const bool rb = P::below(iv, pos, rt0, rt1), rn = P::not_below(iv, pos, rt0, rt1);
          const bool cb = P::below(iv, pos, ct0, ct1), cn = P::not_below(iv, pos, ct0, ct1);
          if (pass == 0) {
            // also a pair with no item to compare against must have an interval, so that decided + band = pairs
            const bool okr = rhas ? (rb || rn) : P::has(iv);
            const bool okc = chas ? (cb || cn) : P::has(iv);
            if (!(okr && okc)) band |= 1ull << bit;
          } else {
            const bool live = ((valid & ~band) >> bit) & 1;
            rcnt += (live && rhas && rb) ? 1 : 0;
            ccnt[v] += (live && chas && cb) ? 1 : 0;
          }
        }
        rpack[u >> 2] += rcnt << (8 * (u & 3));
      }
      if (pass == 1) {
        // rows: the 16 lanes tx = 0..15 of this wave share them
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          int p = rpack[h];
          p += __shfl_xor(p, 1, 64);
          p += __shfl_xor(p, 2, 64);
          p += __shfl_xor(p, 4, 64);
          p += __shfl_xor(p, 8, 64);
          if (tx == 0 && p) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int c = (p >> (8 * r)) & 255;
              if (c) atomicAdd(&E.rc[l1f_row(ty, 4 * h + r)], c);
            }
          }
        }
        // columns: the 4 lane groups of each of the 4 waves share them (<= 8 per thread, <= 32 per wave)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          int p = ccnt[4 * h] | (ccnt[4 * h + 1] << 8) | (ccnt[4 * h + 2] << 16) | (ccnt[4 * h + 3] << 24);
          p += __shfl_xor(p, 16, 64);
          p += __shfl_xor(p, 32, 64);
          if ((lane >> 4) == 0 && p) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int c = (p >> (8 * r)) & 255;
              if (c) atomicAdd(&E.cc[l1f_row(tx, 4 * h + r)], c);
            }
          }
        }
      }
      __syncthreads();
      if (pass == 1) {  // one integer atomic per (item, tile)
        if (tid < L1F_BM) {
          const int c = E.rc[tid];
          if (c && it < E.mr[tid]) gadd(a.row_pos + E.ro[tid] + it, (int32_t)c);
          E.rc[tid] = 0;
        } else {
          const int t = tid - L1F_BM;
          const int c = E.cc[t];
          if (c && it < E.mc[t]) gadd(a.col_pos + E.co[t] + it, (int32_t)c);
          E.cc[t] = 0;
        }
        // (the next round's threshold writes and this read touch different words; its barrier orders the counters)
      }
    }
    if (pass == 0) {
      if (rounds == 0) {  // no list in this tile: nothing to decide, but the pairs without an interval are band
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
          for (int v = 0; v < 8; ++v) {
            const int row = l1f_row(ty, u), col = l1f_row(tx, v);
            double xa[P::NS], xb[P::NS];
#pragma unroll
            for (int k = 0; k < P::NS; ++k) xa[k] = E.sa[k][row], xb[k] = E.sb[k][col];
            if (!P::has(P::interval(a, acc[u][v], E.s, xa, xb))) band |= 1ull << (u * 8 + v);
          }
      }
      // the band pairs, once each, into the caller's list
      band &= valid;
      const int nband = __popcll(band);
      int my = 0;
      if (nband) my = atomicAdd(&E.band_cnt, nband);
      __syncthreads();
      if (tid == 0) {
        const int total = E.band_cnt;
        const int nv = (int)(min<int64_t>(L1F_BM, a.na - i0) * min<int64_t>(L1F_BN, a.nb - j0));
        long long base = 0;
        if (total) {
          base = (long long)gadd(a.stats + 1, (l2f_u64)total);
          if (base + total > a.cap) gmax(a.stats + 3, (l2f_u64)1);
        }
        if (nv - total) gadd(a.stats + 0, (l2f_u64)(nv - total));
        E.band_base = base;
      }
      __syncthreads();
      if (nband) {
        long long p = E.band_base + my;
        uint64_t b = band;
        while (b) {
          const int bit = __ffsll((long long)b) - 1;
          b &= b - 1;
          if (p < a.cap) a.band[p] = make_int2((int)(i0 + l1f_row(ty, bit >> 3)), (int)(j0 + l1f_row(tx, bit & 7)));
          ++p;
        }
      }
    }
  }
}

// ---- the host side ------------------------------------------------------------------------------------------------------
// the common prefix of a kernel's argument block from what flt_count_run hands a main launch
static inline SadArgs sad_count_args(const FltArgs& f, const void* a_codes, const double* a_err, const void* b_codes,
                                     const double* b_err, const double* grid, int64_t d) {
  int64_t n_pad = 0, d_pad = 0;
  l1f_pads(f.na, d, n_pad, d_pad);
  const FltLists& l = f.lists;
  return SadArgs{(const uint32_t*)a_codes, (const uint32_t*)b_codes, a_err, b_err, grid, f.na, f.nb,
                 (int)(d_pad / L1F_BK), f.alpha, f.beta, l.row_off, l.row_sc, l.row_pos, l.col_off, l.col_sc,
                 l.col_pos, f.band.band, f.band.cap, f.band.stats, f.tiles_a, f.tiles_b};
}

// the workspace of a count entry (`name`: the *_count_workspace entry)
static inline int sad_count_workspace(const char* name, int64_t band_cap, int64_t* bytes) {
  CMVE_REQUIRE(bytes, "%s: NULL argument", name);
  CMVE_REQUIRE(band_cap >= 0 && band_cap <= INT64_MAX / 8, "%s: bad band capacity (%lld)", name, (long long)band_cap);
  *bytes = band_cap * (int64_t)sizeof(int2);  // the band list and nothing else: (i, j) per slot
  return CMVE_OK;
}

}  // namespace cmve
#endif
