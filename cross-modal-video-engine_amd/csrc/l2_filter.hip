// K19: the count pass of K18 under the Euclidean measures (euclidean / l2 / l2_norm: CMVE_PW_L2, fp64 score words)
// at the MFMA rate -- what
//   LINAS-engine/evaluation.py:22-35 + util/metrics.py:61-157   cal_error(measure) -> eval_q2m's argsort loop /
//                                                               t2v_map / v2t_map
// decide per pair.  ||a - b||^2 = ||a||^2 + ||b||^2 - 2 ||a|| ||b|| cos(a, b): the cosine comes from an fp16
// v_mfma_f32_16x16x32_f16 GEMM over the packed unit-vector planes (h16), its error from the rows' err_h16 and the
// accumulation model of DESIGN s4, and every comparison  e(i, j) < item score  whose two sides are further apart
// than that error (and than every rounding of the canonical chain, DESIGN s4 "K19") is decided from the MFMA
// value.  The pairs that are not -- the band -- are appended to a caller-owned list and re-scored by the second
// kernel on the canonical chain of pairwise_tile.h (one accumulator, k ascending, from zero), so the counts are,
// word for word, cmve_pairwise_count's.
//   l2f_main_kernel   128 x 128 tile, 4 waves of 64 x 64, 64-deep K-tiles double-buffered in LDS (register staged,
//                     XOR-swizzled 16-B chunks); fp64 epilogue: interval test against each item, band append, counts
//                     (shuffle / LDS partial sums, one integer atomic per (item, tile): bit-reproducible)
//   l2f_fixup_kernel  a wave takes 64 band pairs: the (a - b) chunks go through LDS transposed (coalesced loads), each
//                     lane runs its own pair's chain
//   l2f_nan_kernel    the NaN items' words (cmve_pairwise_count's rule with the caller's n)
// K21 (cmve_l2_count_resolved): the same launches, then two that read the overflow word and do nothing when it is 0 --
//   l2f_gated_zero_kernel zeroes the words, pairwise_rank.hip's gated pwr_count_kernel counts every pair on the
//   canonical chain -- so the words are cmve_pairwise_count's whatever the band did, with no host read in between.
#include "filter_count.h"

namespace cmve {
namespace {

struct L2fArgs {
  const uint16_t* a16;  // [na_pad, d_pad] fp16 unit rows
  const uint16_t* b16;
  const double* a_inv;  // 1 / ||row||
  const double* b_inv;
  const float* a_err;   // >= || x_hat - h16 ||
  const float* b_err;
  int64_t d_pad;
  L2fConsts c;   // gamma, theta, kappa, rho (l2_filter_tile.h)
  FltArgs f;
};

// the epilogue's LDS, laid over the staging buffers once the K loop is done
struct L2fEpi {
  double an[L2F_BM], ae[L2F_BM], bn[L2F_BN], be[L2F_BN];      // norms and row errors of the tile's rows / columns
  double rtb[L2F_BM], rtn[L2F_BM], ctb[L2F_BN], ctn[L2F_BN];  // one round's thresholds (below / not-below)
  int64_t ro[L2F_BM], co[L2F_BN];
  int mr[L2F_BM], mc[L2F_BN];
  int rc[L2F_BM], cc[L2F_BN];
  int s_m[2];
  int band_cnt;
  long long band_base;
};
static_assert(sizeof(L2fEpi) <= L2F_SMEM, "the epilogue's LDS fits the staging buffers");

__global__ __launch_bounds__(256, 2) void l2f_main_kernel(L2fArgs a) {
  __shared__ __attribute__((aligned(16))) char smem[L2F_SMEM];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, fr = lane & 15, fq = lane >> 4;
  int ta, tb_;
  l2f_tile_of_block(blockIdx.x, a.f.tiles_a, a.f.tiles_b, ta, tb_);
  const int64_t i0 = (int64_t)ta * L2F_BM, j0 = (int64_t)tb_ * L2F_BN;

  // ---- the GEMM: c[tm][tn] = 16 x 16 blocks of the wave's 64 x 64 (rows below n_pad, a multiple of 256: in bounds)
  l2f_f32x4 acc[4][4];
  l2f_gemm_tile(a.a16, a.b16, a.d_pad, i0, j0, smem, acc);

  // ---- epilogue ------------------------------------------------------------------------------------------------------
  // acc[m][n][r] is the pair (A row wm 64 + 16 m + 4 fq + r, B row wn 64 + 16 n + fr) of the tile
  L2fEpi& E = *(L2fEpi*)smem;
  if (tid < 2) E.s_m[tid] = 0;
  if (tid == 2) E.band_cnt = 0;
  __syncthreads();
  if (tid < L2F_BM) {
    const int64_t i = i0 + tid;
    const bool v = i < a.f.na;
    E.an[tid] = l2f_side_norm(i, v, a.a_inv);
    E.ae[tid] = l2f_side_err(i, v, a.a_err, a.c.theta);
    const int64_t o = (v && a.f.lists.row_pos) ? a.f.lists.row_off[i] : 0;
    const int m = (v && a.f.lists.row_pos) ? (int)(a.f.lists.row_off[i + 1] - o) : 0;
    E.ro[tid] = o;
    E.mr[tid] = m;
    E.rc[tid] = 0;
    if (m) atomicMax(&E.s_m[0], m);
  } else {
    const int t = tid - L2F_BM;
    const int64_t j = j0 + t;
    const bool v = j < a.f.nb;
    E.bn[t] = l2f_side_norm(j, v, a.b_inv);
    E.be[t] = l2f_side_err(j, v, a.b_err, a.c.theta);
    const int64_t o = (v && a.f.lists.col_pos) ? a.f.lists.col_off[j] : 0;
    const int m = (v && a.f.lists.col_pos) ? (int)(a.f.lists.col_off[j + 1] - o) : 0;
    E.co[t] = o;
    E.mc[t] = m;
    E.cc[t] = 0;
    if (m) atomicMax(&E.s_m[1], m);
  }
  __syncthreads();
  const int rounds = max(E.s_m[0], E.s_m[1]);  // block-uniform
  const int rbase = wm * 64 + 4 * fq, cbase = wn * 64 + fr;
  // bit (m * 4 + r) * 4 + n of `valid`: the pair exists
  uint64_t valid = 0, band = 0;
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int n = 0; n < 4; ++n)
        if (i0 + rbase + 16 * m + r < a.f.na && j0 + cbase + 16 * n < a.f.nb) valid |= 1ull << ((m * 4 + r) * 4 + n);

  // one round: item `it` of every row and column list.  PASS 0 marks the pairs some item cannot decide, PASS 1
  // counts the decided ones.
  for (int pass = 0; pass < 2; ++pass) {
    for (int it = 0; it < rounds; ++it) {
      if (tid < L2F_BM) {
        double tb = (double)NAN, tn = (double)NAN;
        const bool has = it < E.mr[tid];
        if (has) l2f_thresholds(a.f.lists.row_sc[E.ro[tid] + it], a.f.alpha, a.f.beta, a.c.rho, tb, tn);
        E.rtb[tid] = tb;
        E.rtn[tid] = tn;
      } else {
        const int t = tid - L2F_BM;
        double tb = (double)NAN, tn = (double)NAN;
        const bool has = it < E.mc[t];
        if (has) l2f_thresholds(a.f.lists.col_sc[E.co[t] + it], a.f.alpha, a.f.beta, a.c.rho, tb, tn);
        E.ctb[t] = tb;
        E.ctn[t] = tn;
      }
      __syncthreads();
      const bool pos = a.f.alpha > 0.0;
      int ccnt[4] = {0, 0, 0, 0};
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        int rpack = 0;  // the four rows' counts, a byte each (<= 4 per thread, <= 64 over the row's 16 lanes)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = rbase + 16 * m + r;
          const double an = E.an[row], ae = E.ae[row], rtb = E.rtb[row], rtn = E.rtn[row];
          const bool rhas = it < E.mr[row];
#pragma unroll
          for (int n = 0; n < 4; ++n) {
            const int col = cbase + 16 * n;
            const int bit = (m * 4 + r) * 4 + n;
            double dlo, dhi;
            l2f_interval(acc[m][n][r], an, ae, E.bn[col], E.be[col], a.c.gamma, a.c.kappa, dlo, dhi);
            const bool chas = it < E.mc[col];
            const double ctb = E.ctb[col], ctn = E.ctn[col];
            const bool rb = pos ? dhi < rtb : dlo > rtb, rn = pos ? dlo > rtn : dhi < rtn;
            const bool cb = pos ? dhi < ctb : dlo > ctb, cn = pos ? dlo > ctn : dhi < ctn;
            if (pass == 0) {
              // also a pair with no item to compare against must have an interval, so that decided + band = pairs
              const bool okr = rhas ? (rb || rn) : (dlo == dlo);
              const bool okc = chas ? (cb || cn) : (dlo == dlo);
              if (!(okr && okc)) band |= 1ull << bit;
            } else {
              const bool live = ((valid & ~band) >> bit) & 1;
              rpack += (live && rhas && rb) ? (1 << (8 * r)) : 0;
              ccnt[n] += (live && chas && cb) ? 1 : 0;
            }
          }
        }
        if (pass == 1) {  // rows: the 16 lanes fr = 0..15 of this wave share them
          rpack += __shfl_xor(rpack, 1, 64);
          rpack += __shfl_xor(rpack, 2, 64);
          rpack += __shfl_xor(rpack, 4, 64);
          rpack += __shfl_xor(rpack, 8, 64);
          if (fr == 0 && rpack) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int c = (rpack >> (8 * r)) & 255;
              if (c) atomicAdd(&E.rc[rbase + 16 * m + r], c);
            }
          }
        }
      }
      if (pass == 1) {  // columns: the 4 lane groups fq = 0..3 share them (<= 16 per thread, <= 64 per wave)
        int cpack = ccnt[0] | (ccnt[1] << 8) | (ccnt[2] << 16) | (ccnt[3] << 24);
        cpack += __shfl_xor(cpack, 16, 64);
        cpack += __shfl_xor(cpack, 32, 64);
        if (fq == 0 && cpack) {
#pragma unroll
          for (int n = 0; n < 4; ++n) {
            const int c = (cpack >> (8 * n)) & 255;
            if (c) atomicAdd(&E.cc[cbase + 16 * n], c);
          }
        }
      }
      __syncthreads();
      if (pass == 1) {  // one integer atomic per (item, tile)
        if (tid < L2F_BM) {
          const int c = E.rc[tid];
          if (c && it < E.mr[tid]) gadd(a.f.lists.row_pos + E.ro[tid] + it, (int32_t)c);
          E.rc[tid] = 0;
        } else {
          const int t = tid - L2F_BM;
          const int c = E.cc[t];
          if (c && it < E.mc[t]) gadd(a.f.lists.col_pos + E.co[t] + it, (int32_t)c);
          E.cc[t] = 0;
        }
        // (the next round's threshold writes and this read touch different words; its barrier orders the counters)
      }
    }
    if (pass == 0) {
      if (rounds == 0) {  // no list in this tile: nothing to decide, but the pairs without an interval are band
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
          for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int n = 0; n < 4; ++n) {
              const int row = rbase + 16 * m + r, col = cbase + 16 * n;
              double dlo, dhi;
              l2f_interval(acc[m][n][r], E.an[row], E.ae[row], E.bn[col], E.be[col], a.c.gamma, a.c.kappa, dlo, dhi);
              if (!(dlo == dlo)) band |= 1ull << ((m * 4 + r) * 4 + n);
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
        const int nv = (int)(min<int64_t>(L2F_BM, a.f.na - i0) * min<int64_t>(L2F_BN, a.f.nb - j0));
        long long base = 0;
        if (total) {
          base = (long long)gadd(a.f.band.stats + 1, (l2f_u64)total);
          if (base + total > a.f.band.cap) gmax(a.f.band.stats + 3, (l2f_u64)1);
        }
        if (nv - total) gadd(a.f.band.stats + 0, (l2f_u64)(nv - total));
        E.band_base = base;
      }
      __syncthreads();
      if (nband) {
        long long p = E.band_base + my;
        uint64_t b = band;
        while (b) {
          const int bit = __ffsll((long long)b) - 1;
          b &= b - 1;
          const int n = bit & 3, r = (bit >> 2) & 3, m = bit >> 4;
          if (p < a.f.band.cap) a.f.band.band[p] = make_int2((int)(i0 + rbase + 16 * m + r), (int)(j0 + cbase + 16 * n));
          ++p;
        }
      }
    }
  }
}

// ---- the band pairs on the canonical chain -----------------------------------------------------------------------------
// (METRIC: CMVE_PW_L2, CMVE_PW_L1 for the SAD filter of l1_filter.hip, or CMVE_PW_JACCARD for jaccard_filter.hip's --
// the list, the lists' words and the counters are the same, the chain is the metric's; jaccard's words are float32)
template <int METRIC, typename TA, typename TB>
__global__ __launch_bounds__(256) void l2f_fixup_kernel(const TA* __restrict__ A, int64_t lda,
                                                        const TB* __restrict__ B, int64_t ldb, int64_t d, double alpha,
                                                        double beta, const int64_t* __restrict__ row_off,
                                                        const double* __restrict__ row_sc, int32_t* __restrict__ row_pos,
                                                        const int64_t* __restrict__ col_off,
                                                        const double* __restrict__ col_sc, int32_t* __restrict__ col_pos,
                                                        const int2* __restrict__ band, int64_t cap,
                                                        l2f_u64* __restrict__ stats) {
  __shared__ double sd[4][64][L2F_KC + 1];  // [wave][pair][k]: lane p reads row p (17-double stride: conflict-free)
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t n = (int64_t)stats[1];
  if (n > cap) return;  // the list overflowed: the caller redoes the call with the reported need
  for (int64_t b0 = (int64_t)blockIdx.x * 256; b0 < n; b0 += (int64_t)gridDim.x * 256) {  // block-uniform
    const int64_t p = b0 + w * 64 + lane;
    const bool live = p < n;
    const int2 ij = band[live ? p : b0];  // an idle lane repeats a pair of the list: its loads stay in bounds
    double s1 = 0.0;
    const double s = l2f_chain64<METRIC>(A, lda, B, ldb, d, ij.x, ij.y, sd[w], lane, &s1);
    // (jaccard's words are float32: K24)
    const double e = pw_round(pw_score<METRIC>(s, s1, alpha, beta), METRIC == CMVE_PW_JACCARD);
    if (live) {
      if (row_pos) {
        const int64_t o = row_off[ij.x], m = row_off[ij.x + 1];
        for (int64_t q = o; q < m; ++q)
          if (e < row_sc[q]) gadd(row_pos + q, (int32_t)1);
      }
      if (col_pos) {
        const int64_t o = col_off[ij.y], m = col_off[ij.y + 1];
        for (int64_t q = o; q < m; ++q)
          if (e < col_sc[q]) gadd(col_pos + q, (int32_t)1);
      }
    }
    const int nl = (int)min<int64_t>(64, max<int64_t>(0, n - (b0 + w * 64)));
    if (lane == 0 && nl) gadd(stats + 2, (l2f_u64)nl);
  }
}

// ---- NaN items: n - (NaN items of the list) + (the item's place among them), in list order -----------------------------
__global__ __launch_bounds__(256) void l2f_nan_kernel(const int64_t* __restrict__ off, const double* __restrict__ sc,
                                                      int64_t n_lists, int64_t n, int32_t* __restrict__ pos) {
  const int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (l >= n_lists) return;
  const int64_t lo = off[l], hi = off[l + 1];
  int64_t n_nan = 0, run = 0;
  for (int64_t p = lo; p < hi; ++p) {
    const double t = sc[p];
    n_nan += (t != t);
  }
  for (int64_t p = lo; p < hi && n_nan; ++p) {
    const double t = sc[p];
    if (t != t) pos[p] = (int32_t)(n - n_nan + run++);
  }
}

// ---- K21: the band list overflowed -> drop the words counted so far (the canonical count that follows needs zeros) ----
__global__ __launch_bounds__(256) void l2f_gated_zero_kernel(int32_t* __restrict__ row_pos, int64_t row_items,
                                                             int32_t* __restrict__ col_pos, int64_t col_items,
                                                             const l2f_u64* __restrict__ gate) {
  if (gld(gate) == 0ull) return;
  const int64_t step = (int64_t)gridDim.x * 256;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < row_items; p += step) row_pos[p] = 0;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < col_items; p += step) col_pos[p] = 0;
}

}  // namespace

// ---- the launches every filtered count shares (filter_count.h) -------------------------------------------------------------
void l2f_nan_launch(hipStream_t st, const int64_t* off, const double* sc, int64_t n_lists, int64_t n, int32_t* pos) {
  hipLaunchKernelGGL(l2f_nan_kernel, dim3((unsigned)((n_lists + 255) / 256)), dim3(256), 0, st, off, sc, n_lists, n,
                     pos);
}

void l2f_fixup_launch(hipStream_t st, int32_t metric, const FltRows& r, double alpha, double beta, const FltLists& l,
                      const FltBand& b) {
  const int fix_blocks = (int)std::max<int64_t>(1, std::min<int64_t>(8 * device_cus(), (b.cap + 255) / 256));
#define L2F_FIXUP(M)                                                                                                  \
  PWR_TYPES(r.a_dtype, r.b_dtype, TA, TB, {                                                                           \
    hipLaunchKernelGGL((l2f_fixup_kernel<M, TA, TB>), dim3((unsigned)fix_blocks), dim3(256), 0, st, (const TA*)r.A,   \
                       r.lda, (const TB*)r.B, r.ldb, r.d, alpha, beta, l.row_off, l.row_sc, l.row_pos, l.col_off,     \
                       l.col_sc, l.col_pos, (const int2*)b.band, b.cap, b.stats);                                     \
  })
  if (metric == CMVE_PW_L1) { L2F_FIXUP(CMVE_PW_L1) }
  else if (metric == CMVE_PW_JACCARD) { L2F_FIXUP(CMVE_PW_JACCARD) }
  else { L2F_FIXUP(CMVE_PW_L2) }
#undef L2F_FIXUP
}

void l2f_resolve_launch(hipStream_t st, int32_t metric, const FltRows& r, double alpha, double beta, const FltLists& l,
                        const l2f_u64* stats) {
  // the list overflowed (decided on the device: both launches do nothing otherwise): the words so far are
  // dropped and cmve_pairwise_count's kernel counts every pair on the canonical chain, NaN items included
  const int64_t items = std::max(l.row_items, l.col_items);
  const int zero_blocks = (int)std::max<int64_t>(1, std::min<int64_t>(8 * device_cus(), (items + 255) / 256));
  hipLaunchKernelGGL(l2f_gated_zero_kernel, dim3((unsigned)zero_blocks), dim3(256), 0, st, l.row_pos, l.row_items,
                     l.col_pos, l.col_items, stats + 3);
  pwr_count_gated_launch(st, metric, r, alpha, beta, l, stats + 3);
}

}  // namespace cmve

using namespace cmve;

extern "C" int cmve_l2_count_workspace(const cmve_rows_t* a, const cmve_rows_t* b, int64_t band_cap, int64_t* bytes) {
  CMVE_REQUIRE(a && b && bytes, "cmve_l2_count_workspace: NULL argument");
  CMVE_REQUIRE(band_cap >= 0 && band_cap <= INT64_MAX / 8, "cmve_l2_count_workspace: bad band capacity (%lld)",
               (long long)band_cap);
  CMVE_REQUIRE(a->n >= 0 && b->n >= 0 && a->d > 0 && a->d == b->d,
               "cmve_l2_count_workspace: bad shape (%lld x %lld, %lld x %lld)", (long long)a->n, (long long)a->d,
               (long long)b->n, (long long)b->d);
  *bytes = band_cap * (int64_t)sizeof(int2);  // the band list and nothing else: (i, j) per slot
  return CMVE_OK;
}

// cmve_l2_count and cmve_l2_count_resolved: the sets' own checks and the main launch of flt_count_run; `resolved` adds
// the two launches gated on the overflow word
static int l2_count_run(const char* name, bool resolved, cmve_handle_t h, const cmve_rows_t* a, const cmve_rows_t* b,
                        double alpha, double beta, const FltLists& lists, void* ws, int64_t ws_bytes, int64_t* stats) {
  CMVE_REQUIRE(h && a && b && stats, "%s: NULL argument", name);
  const FltRows rows{a->raw, a->raw_dtype, a->raw_ld, a->n, b->raw, b->raw_dtype, b->raw_ld, b->n, a->d};
  return flt_count_run(
      name, resolved ? "l2_count_resolved" : "l2_count", h, CMVE_PW_L2, rows, alpha, beta, lists, ws, ws_bytes, stats,
      resolved, [&] { return l2f_check_sets(name, a, b); },
      [&](hipStream_t st, const FltArgs& f) {
        const L2fArgs g{a->h16,     b->h16,   a->inv_norm, b->inv_norm,
                        a->err_h16, b->err_h16, a->d_pad,  l2f_consts(a->d, a->d_pad), f};  // DESIGN s4 (K19)
        hipLaunchKernelGGL(l2f_main_kernel, dim3((unsigned)(f.tiles_a * f.tiles_b)), dim3(256), 0, st, g);
      });
}

extern "C" int cmve_l2_count(cmve_handle_t h, const cmve_rows_t* a, const cmve_rows_t* b, double alpha, double beta,
                             const int64_t* row_off, const double* row_sc, int64_t row_items, int64_t row_n,
                             int32_t* row_pos, const int64_t* col_off, const double* col_sc, int64_t col_items,
                             int64_t col_n, int32_t* col_pos, void* ws, int64_t ws_bytes, int64_t* stats) {
  return l2_count_run("cmve_l2_count", false, h, a, b, alpha, beta,
                      {row_off, row_sc, row_items, row_n, row_pos, col_off, col_sc, col_items, col_n, col_pos}, ws,
                      ws_bytes, stats);
}

extern "C" int cmve_l2_count_resolved(cmve_handle_t h, const cmve_rows_t* a, const cmve_rows_t* b, double alpha,
                                      double beta, const int64_t* row_off, const double* row_sc, int64_t row_items,
                                      int64_t row_n, int32_t* row_pos, const int64_t* col_off, const double* col_sc,
                                      int64_t col_items, int64_t col_n, int32_t* col_pos, void* ws, int64_t ws_bytes,
                                      int64_t* stats) {
  return l2_count_run("cmve_l2_count_resolved", true, h, a, b, alpha, beta,
                      {row_off, row_sc, row_items, row_n, row_pos, col_off, col_sc, col_items, col_n, col_pos}, ws,
                      ws_bytes, stats);
}
