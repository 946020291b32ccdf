// K24: the count pass of K18 under jaccard (CMVE_PW_JACCARD, float32 score words) from the integer SAD filter of K22
// -- what
//   LINAS-engine/evaluation.py:32-35,56-72 + util/metrics.py:61-157   cal_error / cal_error_batch('jaccard') ->
//                                                                     eval_q2m's argsort loop / t2v_map / v2t_map
// decide per pair.  Both sets are K22's uint16 codes on one grid (cmve_l1_grid, cmve_l1_pack: unchanged); on that
// grid sum_k min and sum_k max of the decoded rows are (P -+ s SAD) / 2 with P from the rows' exact code sums, the SAD
// is l1f_sad_tile's (the one K loop of l1_filter_tile.h), and the true sums lie within the two rows' quantisation
// errors of those.  Every comparison  e(i, j) < item word  that the interval of the quotient (jaccard_filter_tile.h,
// DESIGN s4 "K24") puts out of reach of every rounding -- the float32 one included -- is decided from the integers;
// the other pairs -- the band -- are re-scored on the canonical two-accumulator chain by K19's fix-up kernel, and a
// list that overflows is resolved on the device by K21's gated launches with float32 words: the counts are, word for
// word, cmve_pairwise_count's.
//   jacf_rowsums_kernel  a row's exact code sum (the pack's own quantisation, so the integers are the stored codes')
//                        and S >= sum_k |x_k|
//   jacf_main_kernel     l1f_main_kernel's tile, block order, two-pass epilogue and thread layout; the interval is of
//                        two sums, the tests are products against thresholds moved to quotient space once per
//                        (item, round): no division per pair
#include "filter_count.h"
#include "jaccard_filter_tile.h"

namespace cmve {
namespace {

// ---- the per-row extras: a wave per row ------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void jacf_rowsums_kernel(const T* __restrict__ X, int64_t ld, int64_t n, int64_t d,
                                                           const double* __restrict__ grid,
                                                           int64_t* __restrict__ qsum, double* __restrict__ asum) {
  double lo, s;
  l1f_grid_of(grid, lo, s);
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;  // wave-uniform
  const T* row = X + i * ld;
  unsigned long long q = 0;
  double a = 0.0;
  for (int64_t k = lane; k < d; k += 64) {
    const double x = (double)row[k];
    q += (uint32_t)fmin(fmax(rint((x - lo) / s), 0.0), 65535.0);  // l1f_pack_kernel's expression (NaN -> 0)
    a += fabs(x) <= L1F_X_MAX ? fabs(x) : __builtin_huge_val();   // NaN, inf, huge: where err is +inf
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    q += __shfl_xor(q, o, 64);
    a += __shfl_xor(a, o, 64);
  }
  // rounded up past every rounding of a sum of d terms
  if (lane == 0) {
    qsum[i] = (int64_t)q;
    asum[i] = a * (1.0 + 4.0 * ((double)d + 8.0) * L2F_U) + 1e-300;
  }
}

// ---- the count -----------------------------------------------------------------------------------------------------------
struct JacfArgs {
  const uint32_t* a_codes;  // tiled (l1_filter_tile.h)
  const uint32_t* b_codes;
  const double* a_err;
  const double* b_err;
  const int64_t* a_qsum;  // exact code sums
  const int64_t* b_qsum;
  const double* a_asum;   // >= sum |x|
  const double* b_asum;
  const double* grid;
  int64_t na, nb;
  int nkt;  // K tiles
  double d, alpha, beta;
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
struct JacfEpi {
  double ap[L1F_BM], aw[L1F_BM], bp[L1F_BN], bw[L1F_BN];      // jacf_side's terms of the tile's rows / columns
  double rtl[L1F_BM], rtu[L1F_BM], ctl[L1F_BN], ctu[L1F_BN];  // one round's thresholds in quotient space
  int64_t ro[L1F_BM], co[L1F_BN];
  int mr[L1F_BM], mc[L1F_BN];
  int rc[L1F_BM], cc[L1F_BN];
  int s_m[2];
  int band_cnt;
  long long band_base;
  double s;  // the grid's step, re-read per row of a round (see the epilogue)
};
static_assert(sizeof(JacfEpi) <= L1F_SMEM, "the epilogue's LDS fits the staging buffers");

__global__ __launch_bounds__(256, 4) void jacf_main_kernel(JacfArgs a) {
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
  JacfEpi& E = *(JacfEpi*)smem;
  double lo, s;
  l1f_grid_of(a.grid, lo, s);
  if (tid < 2) E.s_m[tid] = 0;
  if (tid == 2) E.band_cnt = 0;
  if (tid == 3) E.s = s;
  __syncthreads();
  if (tid < L1F_BM) {
    const int64_t i = i0 + tid;
    const bool v = i < a.na;
    jacf_side(v, v ? a.a_err[i] : 0.0, v ? a.a_asum[i] : 0.0, v ? (double)a.a_qsum[i] : 0.0, a.d, lo, s, E.ap[tid],
              E.aw[tid]);
    const int64_t o = (v && a.row_pos) ? a.row_off[i] : 0;
    const int m = (v && a.row_pos) ? (int)(a.row_off[i + 1] - o) : 0;
    E.ro[tid] = o;
    E.mr[tid] = m;
    E.rc[tid] = 0;
    if (m) atomicMax(&E.s_m[0], m);
  } else {
    const int t = tid - L1F_BM;
    const int64_t j = j0 + t;
    const bool v = j < a.nb;
    jacf_side(v, v ? a.b_err[j] : 0.0, v ? a.b_asum[j] : 0.0, v ? (double)a.b_qsum[j] : 0.0, a.d, lo, s, E.bp[t],
              E.bw[t]);
    const int64_t o = (v && a.col_pos) ? a.col_off[j] : 0;
    const int m = (v && a.col_pos) ? (int)(a.col_off[j + 1] - o) : 0;
    E.co[t] = o;
    E.mc[t] = m;
    E.cc[t] = 0;
    if (m) atomicMax(&E.s_m[1], m);
  }
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
      // the item's edge moves to quotient space here, once per (item, round): the only divisions of the epilogue
      if (tid < L1F_BM) {
        double tl = (double)NAN, tu = (double)NAN;
        const bool has = it < E.mr[tid];
        if (has) jacf_thresholds(a.row_sc[E.ro[tid] + it], a.alpha, a.beta, tl, tu);
        E.rtl[tid] = tl;
        E.rtu[tid] = tu;
      } else {
        const int t = tid - L1F_BM;
        double tl = (double)NAN, tu = (double)NAN;
        const bool has = it < E.mc[t];
        if (has) jacf_thresholds(a.col_sc[E.co[t] + it], a.alpha, a.beta, tl, tu);
        E.ctl[t] = tl;
        E.ctu[t] = tu;
      }
      __syncthreads();
      const bool pos = a.alpha > 0.0;
      int ccnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      int rpack[2] = {0, 0};  // four rows' counts each, a byte a row (<= 8 per thread, <= 128 over the row's 16 lanes)
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int row = l1f_row(ty, u);
        // a volatile read: the 64 intervals are formed again in every round, eight at a time, instead of being
        // hoisted out of the rounds as 256 live doubles per thread
        const double sv = *(const volatile double*)&E.s;
        const double ap = E.ap[row], aw = E.aw[row], rtl = E.rtl[row], rtu = E.rtu[row];
        const bool rhas = it < E.mr[row];
        int rcnt = 0;
#pragma unroll
        for (int v = 0; v < 8; ++v) {
          const int col = l1f_row(tx, v);
          const int bit = u * 8 + v;
          double ilo, ihi, ulo, uhi;
          jacf_interval(acc[u][v], sv, ap, aw, E.bp[col], E.bw[col], ilo, ihi, ulo, uhi);
          const bool chas = it < E.mc[col];
          const double ctl = E.ctl[col], ctu = E.ctu[col];
          const bool rlt = jacf_lt(ihi, ulo, uhi, rtl), rgt = jacf_gt(ilo, ulo, uhi, rtu);
          const bool clt = jacf_lt(ihi, ulo, uhi, ctl), cgt = jacf_gt(ilo, ulo, uhi, ctu);
          const bool rb = pos ? rlt : rgt, cb = pos ? clt : cgt;  // below
          if (pass == 0) {
            // also a pair with no item to compare against must have an interval, so that decided + band = pairs
            const bool okr = rhas ? (rlt || rgt) : (ilo == ilo);
            const bool okc = chas ? (clt || cgt) : (ilo == ilo);
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
            double ilo, ihi, ulo, uhi;
            jacf_interval(acc[u][v], E.s, E.ap[row], E.aw[row], E.bp[col], E.bw[col], ilo, ihi, ulo, uhi);
            if (!(ilo == ilo)) band |= 1ull << (u * 8 + v);
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

}  // namespace
}  // namespace cmve

using namespace cmve;

extern "C" int cmve_jaccard_rowsums(cmve_handle_t h, const void* X, int32_t dtype, int64_t ld, int64_t n, int64_t d,
                                    const double* grid, int64_t n_pad, int64_t d_pad, int64_t* qsum, double* asum) {
  CMVE_REQUIRE(h && grid && (X || !n) && ((qsum && asum) || !n), "cmve_jaccard_rowsums: NULL argument");
  CMVE_REQUIRE(n >= 0 && n < (1ll << 31) && d > 0 && d <= L1F_D_MAX && ld >= d, "cmve_jaccard_rowsums: bad shape");
  CMVE_REQUIRE(l1f_dtype_ok(dtype), "cmve_jaccard_rowsums: rows must be CMVE_F32/CMVE_F64");
  int64_t np = 0, dp = 0;
  l1f_pads(n, d, np, dp);
  CMVE_REQUIRE(n_pad >= np && n_pad % L1F_BM == 0 && d_pad == dp,
               "cmve_jaccard_rowsums: short pad (%lld x %lld given, cmve_l1_pack_size says %lld x %lld)",
               (long long)n_pad, (long long)d_pad, (long long)np, (long long)dp);
  if (n == 0) return CMVE_OK;
  const dim3 blocks((unsigned)((n + 3) / 4));
  if (dtype == CMVE_F64)
    hipLaunchKernelGGL((jacf_rowsums_kernel<double>), blocks, dim3(256), 0, h->stream, (const double*)X, ld, n, d, grid,
                       qsum, asum);
  else
    hipLaunchKernelGGL((jacf_rowsums_kernel<float>), blocks, dim3(256), 0, h->stream, (const float*)X, ld, n, d, grid,
                       qsum, asum);
  return check_launch("jaccard_rowsums");
}

extern "C" int cmve_jaccard_count_workspace(int64_t band_cap, int64_t* bytes) {
  CMVE_REQUIRE(bytes, "cmve_jaccard_count_workspace: NULL argument");
  CMVE_REQUIRE(band_cap >= 0 && band_cap <= INT64_MAX / 8, "cmve_jaccard_count_workspace: bad band capacity (%lld)",
               (long long)band_cap);
  *bytes = band_cap * (int64_t)sizeof(int2);  // the band list and nothing else: (i, j) per slot
  return CMVE_OK;
}

extern "C" int cmve_jaccard_count(cmve_handle_t h, const void* A, int32_t a_dtype, int64_t lda, int64_t na,
                                  const void* a_codes, const double* a_err, const int64_t* a_qsum,
                                  const double* a_asum, const void* B, int32_t b_dtype, int64_t ldb, int64_t nb,
                                  const void* b_codes, const double* b_err, const int64_t* b_qsum,
                                  const double* b_asum, int64_t d, const double* grid, double alpha, double beta,
                                  const int64_t* row_off, const double* row_sc, int64_t row_items, int64_t row_n,
                                  int32_t* row_pos, const int64_t* col_off, const double* col_sc, int64_t col_items,
                                  int64_t col_n, int32_t* col_pos, void* ws, int64_t ws_bytes, int64_t* stats) {
  const char* name = "cmve_jaccard_count";
  CMVE_REQUIRE(h && stats && (A || !na) && (B || !nb), "%s: NULL argument", name);
  auto own_checks = [&]() -> int {
    CMVE_REQUIRE(d > 0 && d <= L1F_D_MAX, "%s: d must be in [1, %lld] (%lld): the u32 SAD is exact up to there", name,
                 (long long)L1F_D_MAX, (long long)d);
    CMVE_REQUIRE(na >= 0 && nb >= 0 && na < (1ll << 31) && nb < (1ll << 31) && lda >= d && ldb >= d, "%s: bad shape",
                 name);
    CMVE_REQUIRE(l1f_dtype_ok(a_dtype) && l1f_dtype_ok(b_dtype), "%s: rows must be CMVE_F32/CMVE_F64", name);
    CMVE_REQUIRE(grid && ((a_codes && a_err && a_qsum && a_asum) || !na) &&
                     ((b_codes && b_err && b_qsum && b_asum) || !nb),
                 "%s: the codes, the row errors, the row sums or the grid are missing (cmve_l1_grid, cmve_l1_pack, "
                 "cmve_jaccard_rowsums)",
                 name);
    CMVE_REQUIRE(((((uintptr_t)a_codes) | ((uintptr_t)b_codes)) & 15) == 0, "%s: codes must be 16-byte aligned", name);
    return CMVE_OK;
  };
  auto main_launch = [&](hipStream_t st, const FltArgs& f) {
    int64_t n_pad = 0, d_pad = 0;
    l1f_pads(na, d, n_pad, d_pad);
    // (a flat argument block, as l1f_main_kernel's)
    const FltLists& l = f.lists;
    const JacfArgs g{(const uint32_t*)a_codes, (const uint32_t*)b_codes, a_err, b_err, a_qsum, b_qsum, a_asum, b_asum,
                     grid, f.na, f.nb, (int)(d_pad / L1F_BK), (double)d, f.alpha, f.beta,
                     l.row_off, l.row_sc, l.row_pos, l.col_off, l.col_sc, l.col_pos, f.band.band, f.band.cap,
                     f.band.stats, f.tiles_a, f.tiles_b};
    hipLaunchKernelGGL(jacf_main_kernel, dim3((unsigned)(f.tiles_a * f.tiles_b)), dim3(256), 0, st, g);
  };
  // (resolve: an overflowing list is resolved on the device, from the start -- no entry leaves it to the host)
  return flt_count_run(name, "jaccard_count", h, CMVE_PW_JACCARD, FltRows{A, a_dtype, lda, na, B, b_dtype, ldb, nb, d},
                       alpha, beta,
                       {row_off, row_sc, row_items, row_n, row_pos, col_off, col_sc, col_items, col_n, col_pos}, ws,
                       ws_bytes, stats, true, own_checks, main_launch);
}
