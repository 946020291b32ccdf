// K26: the exact position of EVERY listed item under cosine, both directions, from ONE pass over the pairs at the MFMA
// rate -- what
//   LINAS-engine/evaluation.py:17-21 + util/metrics.py:61-102,124-157   cal_error (cosine) -> t2v_map / v2t_map /
//                                                                       eval_q2m's argsort loop (validate.py:15-54)
// decide per pair.  The item words and every re-score are the canonical cos64 of rank.hip's gt_thr_kernel /
// fixup_kernel (wave_cos64, cmve_internal.h: ONE device function); the fp16 MFMA cosine of l2f_gemm_tile decides every
// comparison  cos64(i, j) > item word  whose two sides lie further apart than score_error_bound's model allows
// (DESIGN s4, "K26"); the pairs it cannot decide -- the band -- go to the caller's list and are re-scored.
//   cosf_item_kernel    a wave per listed item: its cos64 word
//   cosf_main_kernel    128 x 128 tile on l2f_gemm_tile, K19's block order and round structure; the epilogue compares
//                       the fp32 accumulators with directed-rounded fp32 threshold pairs (no fp64 per pair), made
//                       16 rounds at a time into LDS; a round past the tile's longest row (column) list compares
//                       against the other side's items alone
//   cosf_fixup_kernel   a wave per band pair: cos64, then every item of row i's and column j's list
// K27, for a gallery sharded by rows (the same reference lines, one shard's pairs per call): cosf_item_kernel scores an
// item where its row lives (cmve_cos_item_scores_sharded), and cmve_cos_count_resolved resolves a band list that
// overflowed on the device -- cosf_gated_zero_kernel, then cosf_fixup_kernel's body over every pair.
// The lists, the band list, the counters, the NaN items and the host body are filter_count.h's.
#include "filter_count.h"

namespace cmve {
namespace {

struct CosfArgs {
  const uint16_t* a16;  // [na_pad, d_pad] fp16 unit rows
  const uint16_t* b16;
  const double* a_inv;  // 1 / ||row||
  const double* b_inv;
  const float* a_err;   // >= || x_hat - h16 ||
  const float* b_err;
  const float* a_emax;  // the sets' err_max words {hi, hilo, h16}
  const float* b_emax;
  int64_t d_pad;
  double theta, rho;  // DESIGN s4 (K26)
  FltArgs f;
};

// The bound of one side's items (the per-row form of score_error_bound: this row's err_h16 against the other set's
// err_max), NaN when the row has none: a row beyond the set, a zero-norm or NaN row (inv_norm inf / NaN, err NaN), or
// a norm outside [1e-140, 1e140] (beyond it the products of cos64's dot may under- or overflow, which the model does
// not charge).  theta: the pack's x_hat against the true unit vector; rho: cos64 against the true cosine.
__device__ __forceinline__ double cosf_row_bound(int64_t row, int64_t n, const double* inv, const float* err,
                                                 const float* other_emax, int64_t d_pad, double theta, double rho) {
  if (row >= n) return (double)NAN;
  const double v = inv[row];
  if (!(v > 1e-140 && v < 1e140)) return (double)NAN;
  const double E = score_error_bound((double)err[row] + theta, (double)other_emax[mode_slot(CMVE_SIM_F16)] + theta,
                                     d_pad, CMVE_SIM_F16);
  return (E + rho) * (1.0 + 1e-9) + 1e-15;  // (the roundings of this expression and of t +- E below)
}

// The item word t as an fp32 pair: an MFMA value above hi has cos64 > t, one below lo has not.  A NaN item is never
// counted (x > NaN is false): every pair with a value is decided, not counted (hi = lo = +inf).  A row without a
// bound (E NaN) gives NaN thresholds, but its pairs are band already.
__device__ __forceinline__ void cosf_thresholds(double t, double E, float& hi, float& lo) {
  if (t != t) {
    hi = lo = INFINITY;
    return;
  }
  hi = f32_round_up(t + E);
  lo = f32_round_down(t - E);
}

// The epilogue's LDS, laid over the staging buffers once the K loop is done.  Line t of the tile is A row t for
// t < 128 and B row t - 128 above: thread t owns it.  The thresholds of COSF_R rounds (item `it` of every line's list
// is round `it`) are made at once -- one round trip to the item words per chunk, not per round -- and a call whose
// longest list fits one chunk makes them once for both passes.
constexpr int COSF_R = 16, COSF_LINES = L2F_BM + L2F_BN;
struct CosfEpi {
  float2 thr[COSF_R][COSF_LINES];  // {hi, lo} of the chunk's rounds (cosf_thresholds; +inf, +inf: no item)
  int cnt[COSF_R][COSF_LINES];     // PASS 1: the tile's count of each item of the chunk
  double e[COSF_LINES];            // the bound of the line's items (cosf_row_bound)
  int64_t o[COSF_LINES];           // the line's list: first item, items
  int m[COSF_LINES];
  int s_m[2];  // the longest row / column list of the tile
  int band_cnt;
  long long band_base;
};
static_assert(sizeof(CosfEpi) <= L2F_SMEM, "the epilogue's LDS fits the staging buffers");

__global__ __launch_bounds__(256, 2) void cosf_main_kernel(CosfArgs a) {
  __shared__ __attribute__((aligned(16))) char smem[L2F_SMEM];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, fr = lane & 15, fq = lane >> 4;
  int ta, tb_;
  l2f_tile_of_block(blockIdx.x, a.f.tiles_a, a.f.tiles_b, ta, tb_);
  const int64_t i0 = (int64_t)ta * L2F_BM, j0 = (int64_t)tb_ * L2F_BN;

  // ---- the GEMM (rows below n_pad, a multiple of 256: in bounds)
  l2f_f32x4 acc[4][4];
  l2f_gemm_tile(a.a16, a.b16, a.d_pad, i0, j0, smem, acc);

  // ---- epilogue ------------------------------------------------------------------------------------------------------
  // acc[m][n][r] is the pair (A row wm 64 + 16 m + 4 fq + r, B row wn 64 + 16 n + fr) of the tile
  CosfEpi& E = *(CosfEpi*)smem;
  if (tid < 2) E.s_m[tid] = 0;
  if (tid == 2) E.band_cnt = 0;
  __syncthreads();
  // this thread's line: its list and its items' words and positions
  const bool is_row = tid < L2F_BM;
  const int64_t line = is_row ? i0 + tid : j0 + (tid - L2F_BM);
  const int64_t line_n = is_row ? a.f.na : a.f.nb;
  const int64_t* line_off = is_row ? a.f.lists.row_off : a.f.lists.col_off;
  const double* line_sc = is_row ? a.f.lists.row_sc : a.f.lists.col_sc;
  int32_t* line_pos = is_row ? a.f.lists.row_pos : a.f.lists.col_pos;
  const double my_e = is_row ? cosf_row_bound(line, line_n, a.a_inv, a.a_err, a.b_emax, a.d_pad, a.theta, a.rho)
                             : cosf_row_bound(line, line_n, a.b_inv, a.b_err, a.a_emax, a.d_pad, a.theta, a.rho);
  const bool listed = line < line_n && line_pos;
  const int64_t my_o = listed ? line_off[line] : 0;
  const int my_m = listed ? (int)(line_off[line + 1] - my_o) : 0;
  E.e[tid] = my_e;
  E.o[tid] = my_o;
  E.m[tid] = my_m;
  if (my_m) atomicMax(&E.s_m[is_row ? 0 : 1], my_m);
  __syncthreads();
  const int rmax = E.s_m[0], cmax = E.s_m[1], rounds = max(rmax, cmax);  // block-uniform
  const int rbase = wm * 64 + 4 * fq, cbase = wn * 64 + fr;
  // bit (m * 4 + r) * 4 + n of `valid`: the pair exists; of `band`: some comparison of the pair is not decided.  A
  // pair without a value or without a bound on either side is band whatever the lists say: decided + band = pairs.
  uint64_t valid = 0, band = 0;
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const double re = E.e[rbase + 16 * m + r];
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        const int bit = (m * 4 + r) * 4 + n;
        const float c = acc[m][n][r];
        const double ce = E.e[L2F_BM + cbase + 16 * n];
        if (i0 + rbase + 16 * m + r < a.f.na && j0 + cbase + 16 * n < a.f.nb) valid |= 1ull << bit;
        if (!(c == c && re == re && ce == ce)) band |= 1ull << bit;
      }
    }

  // One round over the thread's 64 pairs: item k of the chunk of every line's list.  PASS 0 marks the pairs some item
  // cannot decide, PASS 1 counts the decided ones; ROWS / COLS: the round has row / column items at all.
  constexpr std::integral_constant<int, 0> kPass0{};
  constexpr std::integral_constant<int, 1> kPass1{};
  constexpr std::true_type kYes{};
  constexpr std::false_type kNo{};
  auto round = [&](int k, auto PASS, auto ROWS, auto COLS) {
    constexpr int pass = decltype(PASS)::value;
    constexpr bool rows = decltype(ROWS)::value, cols = decltype(COLS)::value;
    float2 ct[4];
    if constexpr (cols) {
#pragma unroll
      for (int n = 0; n < 4; ++n) ct[n] = E.thr[k][L2F_BM + cbase + 16 * n];
    }
    int ccnt[4] = {0, 0, 0, 0};
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      int rpack = 0;  // the four rows' counts, a byte each (<= 4 per thread, <= 64 over the row's 16 lanes)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float2 rt = make_float2(0.f, 0.f);
        if constexpr (rows) rt = E.thr[k][rbase + 16 * m + r];
#pragma unroll
        for (int n = 0; n < 4; ++n) {
          const int bit = (m * 4 + r) * 4 + n;
          const float c = acc[m][n][r];
          if constexpr (pass == 0) {
            bool ok = true;
            if constexpr (rows) ok = ok && (c > rt.x || c < rt.y);
            if constexpr (cols) ok = ok && (c > ct[n].x || c < ct[n].y);
            if (!ok) band |= 1ull << bit;
          } else {
            const bool live = ((valid & ~band) >> bit) & 1;
            if constexpr (rows) rpack += (live && c > rt.x) ? (1 << (8 * r)) : 0;
            if constexpr (cols) ccnt[n] += (live && c > ct[n].x) ? 1 : 0;
          }
        }
      }
      if constexpr (pass == 1 && rows) {  // rows: the 16 lanes fr = 0..15 of this wave share them
        rpack += __shfl_xor(rpack, 1, 64);
        rpack += __shfl_xor(rpack, 2, 64);
        rpack += __shfl_xor(rpack, 4, 64);
        rpack += __shfl_xor(rpack, 8, 64);
        if (fr == 0 && rpack) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int c = (rpack >> (8 * r)) & 255;
            if (c) atomicAdd(&E.cnt[k][rbase + 16 * m + r], c);
          }
        }
      }
    }
    if constexpr (pass == 1 && cols) {  // columns: the 4 lane groups fq = 0..3 share them (<= 16 per thread, <= 64 per wave)
      int cpack = ccnt[0] | (ccnt[1] << 8) | (ccnt[2] << 16) | (ccnt[3] << 24);
      cpack += __shfl_xor(cpack, 16, 64);
      cpack += __shfl_xor(cpack, 32, 64);
      if (fq == 0 && cpack) {
#pragma unroll
        for (int n = 0; n < 4; ++n) {
          const int c = (cpack >> (8 * n)) & 255;
          if (c) atomicAdd(&E.cnt[k][L2F_BM + cbase + 16 * n], c);
        }
      }
    }
  };

  for (int pass = 0; pass < 2; ++pass) {
    for (int c0 = 0; c0 < rounds; c0 += COSF_R) {  // block-uniform
      if (pass == 0 || rounds > COSF_R) {  // (one chunk: PASS 1 reads the table PASS 0 made)
        __syncthreads();  // the last chunk's readers are done
        double t[COSF_R];
#pragma unroll
        for (int k = 0; k < COSF_R; ++k) t[k] = (c0 + k < my_m) ? gld(line_sc + my_o + c0 + k) : 0.0;
#pragma unroll
        for (int k = 0; k < COSF_R; ++k) {
          float hi = INFINITY, lo = INFINITY;  // no item this round: as a NaN item, decided and not counted
          if (c0 + k < my_m) cosf_thresholds(t[k], my_e, hi, lo);
          E.thr[k][tid] = make_float2(hi, lo);
        }
      }
      if (pass == 1) {
#pragma unroll
        for (int k = 0; k < COSF_R; ++k) E.cnt[k][tid] = 0;
      }
      __syncthreads();
      const int nr = min(COSF_R, rounds - c0);
      for (int k = 0; k < nr; ++k) {
        // (block-uniform: past the longest row list a round compares against the column items alone, and the mirror)
        const bool dr = c0 + k < rmax, dc = c0 + k < cmax;
        if (pass == 0) {
          if (dr && dc) round(k, kPass0, kYes, kYes);
          else if (dc) round(k, kPass0, kNo, kYes);
          else round(k, kPass0, kYes, kNo);
        } else {
          if (dr && dc) round(k, kPass1, kYes, kYes);
          else if (dc) round(k, kPass1, kNo, kYes);
          else round(k, kPass1, kYes, kNo);
        }
      }
      if (pass == 1) {  // one integer atomic per (item, tile)
        __syncthreads();
        for (int k = 0; k < nr; ++k) {
          const int c = E.cnt[k][tid];
          if (c && c0 + k < my_m) gadd(line_pos + my_o + c0 + k, (int32_t)c);
        }
      }
    }
    if (pass == 0) {
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

// ---- the band pairs on the canonical chain: a wave per pair -------------------------------------------------------------
// DENSE = false: the pairs of the band list (nothing when it overflowed: stats[1] > cap).  DENSE = true (K27, the
// overflow resolved on the device): nothing unless stats[3] is set, then EVERY pair p -> (p / nb, p % nb) of the
// cap = na * nb pairs through the same body -- the words of a list large enough, by construction; the re-score
// counter stays as the overflow left it.
template <bool DENSE, typename TA, typename TB>
__global__ __launch_bounds__(256) void cosf_fixup_kernel(const TA* __restrict__ A, int64_t lda,
                                                         const double* __restrict__ ainv, const TB* __restrict__ B,
                                                         int64_t ldb, const double* __restrict__ binv, int64_t d,
                                                         const int64_t* __restrict__ row_off,
                                                         const double* __restrict__ row_sc, int32_t* __restrict__ row_pos,
                                                         const int64_t* __restrict__ col_off,
                                                         const double* __restrict__ col_sc, int32_t* __restrict__ col_pos,
                                                         const int2* __restrict__ band, int64_t cap, int64_t nb,
                                                         l2f_u64* __restrict__ stats) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int64_t n;
  if constexpr (DENSE) {
    if (gld(stats + 3) == 0ull) return;  // the list held the band: the words stand
    n = cap;
  } else {
    n = (int64_t)gld(stats + 1);
    if (n > cap) return;  // the list overflowed: the caller redoes the call with the reported need, or resolves it
  }
  const int64_t step = (int64_t)gridDim.x * 4;
  int64_t done = 0;
  for (int64_t p = (int64_t)blockIdx.x * 4 + w; p < n; p += step, ++done) {  // wave-uniform
    int64_t i, j;
    if constexpr (DENSE) {
      i = p / nb;
      j = p - i * nb;
    } else {
      const int2 ij = band[p];
      i = ij.x;
      j = ij.y;
    }
    const double s = wave_cos64(A + i * lda, B + j * ldb, gld(ainv + i), gld(binv + j), d, lane);
    if (row_pos) {
      const int64_t m = row_off[i + 1];
      for (int64_t q = row_off[i] + lane; q < m; q += 64)
        if (s > row_sc[q]) gadd(row_pos + q, (int32_t)1);
    }
    if (col_pos) {
      const int64_t m = col_off[j + 1];
      for (int64_t q = col_off[j] + lane; q < m; q += 64)
        if (s > col_sc[q]) gadd(col_pos + q, (int32_t)1);
    }
  }
  if (!DENSE && lane == 0 && done) gadd(stats + 2, (l2f_u64)done);
}

// K27: the band list overflowed -> drop the partial counts before the dense pass.  A NaN item's word is
// l2f_nan_launch's and no pair ever counts into it (x > NaN is false): it is spared.
__global__ __launch_bounds__(256) void cosf_gated_zero_kernel(const double* __restrict__ row_sc,
                                                              int32_t* __restrict__ row_pos, int64_t row_items,
                                                              const double* __restrict__ col_sc,
                                                              int32_t* __restrict__ col_pos, int64_t col_items,
                                                              const l2f_u64* __restrict__ gate) {
  if (gld(gate) == 0ull) return;
  const int64_t step = (int64_t)gridDim.x * 256;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < row_items; p += step) {
    const double t = row_sc[p];
    if (t == t) row_pos[p] = 0;
  }
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < col_items; p += step) {
    const double t = col_sc[p];
    if (t == t) col_pos[p] = 0;
  }
}

// ---- the items' words: a wave per item ----------------------------------------------------------------------------------
// item p of list `owner` names row idx[p] of the other side (col_dir: the lists belong to B rows and name A rows); an
// index outside it scores NaN and reads nothing.  idx_base >= 0 (K27, a gallery sharded by rows): idx holds GLOBAL
// rows of the other side, of which this call's operand is [idx_base, idx_base + n_other); an item outside it is
// another shard's and gets the all-zero word, so that the int64 SUM of the shards' words is the owner's.
template <typename TA, typename TB>
__global__ __launch_bounds__(256) void cosf_item_kernel(const TA* __restrict__ A, int64_t lda,
                                                        const double* __restrict__ ainv, int64_t na,
                                                        const TB* __restrict__ B, int64_t ldb,
                                                        const double* __restrict__ binv, int64_t nb, int64_t d,
                                                        const int64_t* __restrict__ off, const int32_t* __restrict__ idx,
                                                        int64_t n_lists, int64_t n_items, int col_dir,
                                                        int64_t idx_base, double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= n_items) return;  // wave-uniform
  int64_t lo = 0, hi = n_lists;  // first list whose offset exceeds p, minus one
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (off[mid + 1] > p) hi = mid; else lo = mid + 1;
  }
  const bool sharded = idx_base >= 0;
  const int64_t owner = lo, other = (int64_t)idx[p] - (sharded ? idx_base : 0);
  const int64_t i = col_dir ? other : owner, j = col_dir ? owner : other;
  double s = sharded ? 0.0 : (double)NAN;
  if (owner < n_lists && i >= 0 && i < na && j >= 0 && j < nb)
    s = wave_cos64(A + i * lda, B + j * ldb, gld(ainv + i), gld(binv + j), d, lane);
  if (lane == 0) out[p] = s;
}

}  // namespace
}  // namespace cmve

using namespace cmve;

// cmve_cos_item_scores (idx_base < 0: an index outside the other set scores NaN) and cmve_cos_item_scores_sharded
// (idx_base >= 0: global indices, the zero word outside this call's operand): one argument list, one launch
static int cos_item_scores_run(const char* name, cmve_handle_t h, const cmve_rows_t* a, const cmve_rows_t* b,
                               const int64_t* off, const int32_t* idx, int64_t n_lists, int64_t n_items,
                               int32_t col_dir, int64_t idx_base, double* out) {
  CMVE_REQUIRE(h && a && b && off, "%s: NULL argument", name);
  if (int rc = l2f_check_sets(name, a, b)) return rc;
  CMVE_REQUIRE(n_items >= 0 && n_items < (1ll << 31) * 4, "%s: bad item count (%lld)", name, (long long)n_items);
  CMVE_REQUIRE(col_dir == 0 || col_dir == 1, "%s: col_dir must be 0 or 1", name);
  CMVE_REQUIRE(n_lists == (col_dir ? b->n : a->n), "%s: %lld lists for the %lld rows that own them", name,
               (long long)n_lists, (long long)(col_dir ? b->n : a->n));
  CMVE_REQUIRE(n_items == 0 || (idx && out), "%s: NULL argument", name);
  if (n_items == 0) return CMVE_OK;
  PWR_TYPES(a->raw_dtype, b->raw_dtype, TA, TB, {
    hipLaunchKernelGGL((cosf_item_kernel<TA, TB>), dim3((unsigned)((n_items + 3) / 4)), dim3(256), 0, h->stream,
                       (const TA*)a->raw, a->raw_ld, a->inv_norm, a->n, (const TB*)b->raw, b->raw_ld, b->inv_norm,
                       b->n, a->d, off, idx, n_lists, n_items, (int)col_dir, idx_base, out);
  })
  return check_launch(name + 5);  // (without "cmve_")
}

extern "C" int cmve_cos_item_scores(cmve_handle_t h, const cmve_rows_t* a, const cmve_rows_t* b, const int64_t* off,
                                    const int32_t* idx, int64_t n_lists, int64_t n_items, int32_t col_dir,
                                    double* out) {
  return cos_item_scores_run("cmve_cos_item_scores", h, a, b, off, idx, n_lists, n_items, col_dir, -1, out);
}

extern "C" int cmve_cos_item_scores_sharded(cmve_handle_t h, const cmve_rows_t* a, const cmve_rows_t* b,
                                            const int64_t* off, const int32_t* idx, int64_t n_lists, int64_t n_items,
                                            int32_t col_dir, int64_t idx_base, double* out) {
  CMVE_REQUIRE(idx_base >= 0, "cmve_cos_item_scores_sharded: idx_base must not be negative (%lld)",
               (long long)idx_base);
  return cos_item_scores_run("cmve_cos_item_scores_sharded", h, a, b, off, idx, n_lists, n_items, col_dir, idx_base,
                             out);
}

extern "C" int cmve_cos_count_workspace(const cmve_rows_t* a, const cmve_rows_t* b, int64_t band_cap, int64_t* bytes) {
  CMVE_REQUIRE(a && b && bytes, "cmve_cos_count_workspace: NULL argument");
  CMVE_REQUIRE(band_cap >= 0 && band_cap <= INT64_MAX / 8, "cmve_cos_count_workspace: bad band capacity (%lld)",
               (long long)band_cap);
  CMVE_REQUIRE(a->n >= 0 && b->n >= 0 && a->d > 0 && a->d == b->d,
               "cmve_cos_count_workspace: bad shape (%lld x %lld, %lld x %lld)", (long long)a->n, (long long)a->d,
               (long long)b->n, (long long)b->d);
  *bytes = band_cap * (int64_t)sizeof(int2);  // the band list and nothing else: (i, j) per slot
  return CMVE_OK;
}

// cmve_cos_count and cmve_cos_count_resolved: the sets' own checks, the main launch and K26's fix-up launch of
// flt_count_run; `resolved` adds K27's two launches gated on the overflow word
static int cos_count_run(const char* name, bool resolved, cmve_handle_t h, const cmve_rows_t* a, const cmve_rows_t* b,
                         const FltLists& lists, void* ws, int64_t ws_bytes, int64_t* stats) {
  CMVE_REQUIRE(h && a && b && stats, "%s: NULL argument", name);
  const FltRows rows{a->raw, a->raw_dtype, a->raw_ld, a->n, b->raw, b->raw_dtype, b->raw_ld, b->n, a->d};
  // the canonical chain over a pair source: the band list, or (DENSE) every pair once the overflow word is set
#define COSF_FIXUP(DENSE, blocks, l, band_, cap_)                                                                     \
  PWR_TYPES(a->raw_dtype, b->raw_dtype, TA, TB, {                                                                     \
    hipLaunchKernelGGL((cosf_fixup_kernel<DENSE, TA, TB>), dim3((unsigned)(blocks)), dim3(256), 0, st,                \
                       (const TA*)a->raw, a->raw_ld, a->inv_norm, (const TB*)b->raw, b->raw_ld, b->inv_norm, a->d,    \
                       (l).row_off, (l).row_sc, (l).row_pos, (l).col_off, (l).col_sc, (l).col_pos, band_, cap_,       \
                       (int64_t)b->n, bd.stats);                                                                      \
  })
  return flt_count_run(
      name, resolved ? "cos_count_resolved" : "cos_count", h, CMVE_PW_DOT, rows, 1.0, 0.0, lists, ws, ws_bytes, stats,
      resolved,
      [&]() -> int {
        if (int rc = l2f_check_sets(name, a, b)) return rc;
        CMVE_REQUIRE(a->err_max && b->err_max, "%s: a set was packed without its err_max words", name);
        return CMVE_OK;
      },
      [&](hipStream_t st, const FltArgs& f) {
        const L2fConsts c = l2f_consts(a->d, a->d_pad);
        // rho: cos64 against the true cosine -- the dot's chains and tree, two norms, three products (DESIGN s4, K26)
        const CosfArgs g{a->h16,     b->h16,     a->inv_norm, b->inv_norm, a->err_h16,
                         b->err_h16, a->err_max, b->err_max,  a->d_pad,    c.theta,
                         4.0 * ((double)a->d + 16.0) * L2F_U, f};
        hipLaunchKernelGGL(cosf_main_kernel, dim3((unsigned)(f.tiles_a * f.tiles_b)), dim3(256), 0, st, g);
      },
      [&](hipStream_t st, const FltLists& l, const FltBand& bd) {
        const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(16 * device_cus(), (bd.cap + 3) / 4));
        COSF_FIXUP(false, blocks, l, (const int2*)bd.band, bd.cap)
      },
      [&](hipStream_t st, const FltLists& l, const FltBand& bd) {
        // the list overflowed (decided on the device: both launches do nothing otherwise): the partial counts are
        // dropped -- not the NaN items' words -- and every pair goes through the fix-up's body
        const int64_t items = std::max(l.row_items, l.col_items), pairs = a->n * b->n;
        const int zero_blocks = (int)std::max<int64_t>(1, std::min<int64_t>(8 * device_cus(), (items + 255) / 256));
        hipLaunchKernelGGL(cosf_gated_zero_kernel, dim3((unsigned)zero_blocks), dim3(256), 0, st, l.row_sc, l.row_pos,
                           l.row_items, l.col_sc, l.col_pos, l.col_items, bd.stats + 3);
        const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(16 * device_cus(), (pairs + 3) / 4));
        COSF_FIXUP(true, blocks, l, (const int2*)nullptr, pairs)
      });
#undef COSF_FIXUP
}

extern "C" int cmve_cos_count(cmve_handle_t h, const cmve_rows_t* a, const cmve_rows_t* b, const int64_t* row_off,
                              const double* row_sc, int64_t row_items, int64_t row_n, int32_t* row_pos,
                              const int64_t* col_off, const double* col_sc, int64_t col_items, int64_t col_n,
                              int32_t* col_pos, void* ws, int64_t ws_bytes, int64_t* stats) {
  return cos_count_run("cmve_cos_count", false, h, a, b,
                       {row_off, row_sc, row_items, row_n, row_pos, col_off, col_sc, col_items, col_n, col_pos}, ws,
                       ws_bytes, stats);
}

extern "C" int cmve_cos_count_resolved(cmve_handle_t h, const cmve_rows_t* a, const cmve_rows_t* b,
                                       const int64_t* row_off, const double* row_sc, int64_t row_items, int64_t row_n,
                                       int32_t* row_pos, const int64_t* col_off, const double* col_sc,
                                       int64_t col_items, int64_t col_n, int32_t* col_pos, void* ws, int64_t ws_bytes,
                                       int64_t* stats) {
  return cos_count_run("cmve_cos_count_resolved", true, h, a, b,
                       {row_off, row_sc, row_items, row_n, row_pos, col_off, col_sc, col_items, col_n, col_pos}, ws,
                       ws_bytes, stats);
}
