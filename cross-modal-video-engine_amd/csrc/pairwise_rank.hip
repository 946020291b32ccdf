// K18: retrieval under the non-cosine measures WITHOUT the n_q x n_g error matrix -- what
//   LINAS-engine/evaluation.py:22-35,46-71 + util/metrics.py:61-102,124-157   cal_error(measure) -> eval_q2m's argsort
//                                            loop / t2v_map / v2t_map (validate.py:15-54 cal_perf, tester.py:137)
//   LINAS-engine/inference.py:78-80          cal_error(measure) -> np.argsort(errors[0])[:topK]
// compute from the matrix.  Every score here is K10's (pairwise.hip) for the same (metric, alpha, beta, score
// dtype): the shared chain of pairwise_tile.h, so ranks, positions and top-k order are, word for word, those of
// cmve_rank_from_matrix / cmve_gt_positions_from_matrix / a stable argsort on cmve_pairwise's output.
//   positions: launch 1 scores the listed items (one thread each, O(N_c) of them); launch 2 is K10's 64 x 128
//              tile loop whose epilogue, instead of storing, counts the tile's outputs below each item score of
//              the rows and columns it holds: both directions from one pass over the pairs, one integer
//              atomicAdd per (item, tile) -- bit-reproducible.  The two launches are entries of their own as well
//              (cmve_pairwise_item_scores with shard ownership, cmve_pairwise_count with the caller's scores) for a
//              gallery sharded by rows: a position is the plain sum of the shards' counts against one item score,
//              and cmve_pairwise_list_ranks turns the summed positions into best-GT ranks on the device.
//   top-k:     gallery chunks scored into the caller's workspace (-error: K12f orders by score descending) and
//              merged into the running best by K12f (cmve_topk_dense_merge); a small-row geometry of the tile
//              loop serves n_q <= 8 (inference.py's single caption).  With few queries the chunk is cut into
//              column segments so that K12f has a block per (segment, query), and C3's k-way merge joins them.
#include "filter_count.h"  // (pairwise_tile.h; the lists of a count, and the gated launch the filters use)

namespace cmve {

// ---- launch 1: the score of every listed item -------------------------------------------------------------
// item p of list `owner` (off[owner] <= p < off[owner + 1]) names row idx[p] - idx_base of the other side; col_dir:
// the lists belong to B rows and name A rows.  An index outside the other side (nothing is read) scores NaN, or --
// `shard`: idx holds global rows, this call owns [idx_base, idx_base + n_other) of them -- the all-zero word, so
// that an integer SUM of the shards' outputs is the owner's word.
template <int METRIC, typename TA, typename TB>
__global__ __launch_bounds__(256) void pwr_item_kernel(const TA* __restrict__ A, int64_t lda, int64_t na,
                                                       const TB* __restrict__ B, int64_t ldb, int64_t nb, int64_t d,
                                                       double alpha, double beta, int f32,
                                                       const int64_t* __restrict__ off,
                                                       const int32_t* __restrict__ idx, int64_t n_lists,
                                                       int64_t n_items, int col_dir, int64_t idx_base, int shard,
                                                       double* __restrict__ sc) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= n_items) return;
  int64_t lo = 0, hi = n_lists;  // first list whose offset exceeds p, minus one
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (off[mid + 1] > p) hi = mid; else lo = mid + 1;
  }
  const int64_t owner = lo, other = (int64_t)idx[p] - idx_base;
  const int64_t i = col_dir ? other : owner, j = col_dir ? owner : other;
  double s = shard ? 0.0 : (double)NAN;
  if (owner < n_lists && i >= 0 && i < na && j >= 0 && j < nb)
    s = pw_round(pw_pair_score<METRIC>(A + i * lda, B + j * ldb, d, alpha, beta), f32);
  sc[p] = s;
}

// ---- launch 2: K10's tile loop with a counting epilogue -----------------------------------------------------
// row_pos[p] += #{ j in the tile's columns, j < nb : e(i, j) < row_sc[p] } for every item p of every A row i of the
// tile (col_pos: the mirror over i < na).  The item scores are the caller's.  A NaN item is never counted (x < NaN
// is false): with row_n > 0 the tile of its list in the first block column / row stores
// cmve_gt_positions_from_matrix's value for it instead, row_n - (NaN items of the list) + (its place among them)
// (row_n == 0: its word stays 0 -- another shard of the gallery stores it).  The grid has at least one block row and
// column, so the rule also runs when na or nb is 0.  pos must be zero on entry.
// GATED (K21 / K22 / K24, cmve_l2_count_resolved, cmve_l1_count and cmve_jaccard_count; gate / tiles_x / tiles are read by this instantiation alone): every thread reads
// *gate first and the block returns at once when it is 0; otherwise the blocks of a BOUNDED 1-d grid loop over the
// tiles_x x tiles_y tiles, block b taking b, b + gridDim.x, ... in the plain grid's own order -- a call whose gate stays
// shut dispatches a few thousand blocks, not one per tile.
template <int METRIC, typename TA, typename TB, bool GATED = false>
__global__ __launch_bounds__(256) void pwr_count_kernel(const TA* __restrict__ A, int64_t lda, int64_t na,
                                                        const TB* __restrict__ B, int64_t ldb, int64_t nb, int64_t d,
                                                        double alpha, double beta, int f32,
                                                        const int64_t* __restrict__ row_off,
                                                        const double* __restrict__ row_sc, int64_t row_n,
                                                        int32_t* __restrict__ row_pos,
                                                        const int64_t* __restrict__ col_off,
                                                        const double* __restrict__ col_sc, int64_t col_n,
                                                        int32_t* __restrict__ col_pos,
                                                        const unsigned long long* __restrict__ gate, unsigned tiles_x,
                                                        int64_t tiles) {
  using G = PwWide;
  if constexpr (GATED) {
    if (gld(gate) == 0ull) return;  // block-uniform, before the first barrier and before any LDS write
  }
  __shared__ __attribute__((aligned(16))) double sa[G::KS][G::PA];
  __shared__ __attribute__((aligned(16))) double sb[G::KS][G::PB];
  __shared__ int s_m[2];     // the longest row / column list of the tile: the rounds are block-uniform
  __shared__ int lc[G::TB];  // one round's column counts
  constexpr bool JAC = METRIC == CMVE_PW_JACCARD;
  const int tid = threadIdx.x;
  const int tx = tid % G::TX, ty = tid / G::TX;
  int64_t t = blockIdx.x;  // GATED: this block's tile, then every gridDim.x-th after it
  do {
    const unsigned bx = GATED ? (unsigned)(t % tiles_x) : blockIdx.x;
    const unsigned by = GATED ? (unsigned)(t / tiles_x) : blockIdx.y;
    const int64_t i0 = (int64_t)by * G::TA, j0 = (int64_t)bx * G::TB;
    if (tid < 2) s_m[tid] = 0;
    if (tid < G::TB) lc[tid] = 0;
    double e[G::NA][G::NB] = {}, s1[JAC ? G::NA : 1][JAC ? G::NB : 1] = {};
    pw_tile_loop<G, METRIC>(A, lda, na, B, ldb, nb, d, i0, j0, sa, sb, e, s1);
#pragma unroll
    for (int u = 0; u < G::NA; ++u)
#pragma unroll
      for (int v = 0; v < G::NB; ++v)
        e[u][v] = pw_round(pw_score<METRIC>(e[u][v], JAC ? s1[JAC ? u : 0][JAC ? v : 0] : 0.0, alpha, beta), f32);
    // rows and columns of a partial tile beyond na / nb were staged as zeros: they never count and own no list
    bool va[G::NA], vb[G::NB];
    int64_t ro[G::NA], co[G::NB];
    int mr[G::NA], mc[G::NB], mr_max = 0, mc_max = 0;
#pragma unroll
    for (int u = 0; u < G::NA; ++u) {
      const int64_t i = i0 + G::arow(ty, u);
      va[u] = i < na;
      ro[u] = (va[u] && row_pos) ? row_off[i] : 0;
      mr[u] = (va[u] && row_pos) ? (int)(row_off[i + 1] - ro[u]) : 0;
      mr_max = max(mr_max, mr[u]);
    }
#pragma unroll
    for (int v = 0; v < G::NB; ++v) {
      const int64_t j = j0 + G::brow(tx, v);
      vb[v] = j < nb;
      co[v] = (vb[v] && col_pos) ? col_off[j] : 0;
      mc[v] = (vb[v] && col_pos) ? (int)(col_off[j + 1] - co[v]) : 0;
      mc_max = max(mc_max, mc[v]);
    }
    if (tx == 0 && mr_max) atomicMax(&s_m[0], mr_max);
    if (ty == 0 && mc_max) atomicMax(&s_m[1], mc_max);
    // NaN items: the last positions of the row / column, in list order (as gtpos_rows_kernel / gtpos_cols_kernel)
    if (bx == 0 && tx == 0 && row_n > 0) {
#pragma unroll
      for (int u = 0; u < G::NA; ++u) {
        int n_nan = 0, run = 0;
        for (int a = 0; a < mr[u]; ++a) {
          const double t = row_sc[ro[u] + a];
          n_nan += (t != t);
        }
        for (int a = 0; a < mr[u] && n_nan; ++a) {
          const double t = row_sc[ro[u] + a];
          if (t != t) row_pos[ro[u] + a] = (int32_t)(row_n - n_nan + run++);
        }
      }
    }
    if (by == 0 && ty == 0 && col_n > 0) {
#pragma unroll
      for (int v = 0; v < G::NB; ++v) {
        int n_nan = 0, run = 0;
        for (int a = 0; a < mc[v]; ++a) {
          const double t = col_sc[co[v] + a];
          n_nan += (t != t);
        }
        for (int a = 0; a < mc[v] && n_nan; ++a) {
          const double t = col_sc[co[v] + a];
          if (t != t) col_pos[co[v] + a] = (int32_t)(col_n - n_nan + run++);
        }
      }
    }
    __syncthreads();
    const int rounds_r = s_m[0], rounds_c = s_m[1];
    // rows: the 16 threads that share a row (tx = 0..15, consecutive lanes) sum by xor shuffles; every lane of the
    // block runs every shuffle (the loop bounds are block-uniform, the list test is inside)
    for (int a = 0; a < rounds_r; ++a) {
#pragma unroll
      for (int u = 0; u < G::NA; ++u) {
        int c = 0;
        if (a < mr[u]) {
          const double t = row_sc[ro[u] + a];
#pragma unroll
          for (int v = 0; v < G::NB; ++v) c += (vb[v] && e[u][v] < t);
        }
        c += __shfl_xor(c, 8, 64);
        c += __shfl_xor(c, 4, 64);
        c += __shfl_xor(c, 2, 64);
        c += __shfl_xor(c, 1, 64);
        if (tx == 0 && c) gadd(row_pos + ro[u] + a, (int32_t)c);
      }
    }
    // columns: the 16 threads that share a column are 4 lanes (ty & 3) of each of the 4 waves: shuffles within the
    // wave, LDS across the waves, then one atomic per column
    const int64_t jc = j0 + tid;
    const bool cown = tid < G::TB && jc < nb && col_pos != nullptr;
    const int64_t co_t = cown ? col_off[jc] : 0;
    const int mc_t = cown ? (int)(col_off[jc + 1] - co_t) : 0;
    for (int a = 0; a < rounds_c; ++a) {
#pragma unroll
      for (int v = 0; v < G::NB; ++v) {
        int c = 0;
        if (a < mc[v]) {
          const double t = col_sc[co[v] + a];
#pragma unroll
          for (int u = 0; u < G::NA; ++u) c += (va[u] && e[u][v] < t);
        }
        c += __shfl_xor(c, 16, 64);
        c += __shfl_xor(c, 32, 64);
        if ((ty & 3) == 0 && c) atomicAdd(&lc[G::brow(tx, v)], c);
      }
      __syncthreads();
      if (tid < G::TB) {
        const int c = lc[tid];
        if (a < mc_t && c) gadd(col_pos + co_t + a, (int32_t)c);
        lc[tid] = 0;
      }
      __syncthreads();
    }
    if constexpr (GATED) __syncthreads();  // the tile's last LDS reads before the next tile's first writes
    t += gridDim.x;
  } while (GATED && t < tiles);
}

// ---- top-k: one gallery chunk's scores into the workspace (fp64, already rounded to the score dtype) ----------
template <typename G, int METRIC, typename TA, typename TB>
__global__ __launch_bounds__(256) void pwr_chunk_kernel(const TA* __restrict__ A, int64_t lda, int64_t na,
                                                        const TB* __restrict__ B, int64_t ldb, int64_t nb, int64_t d,
                                                        double alpha, double beta, int f32, double* __restrict__ out,
                                                        int64_t seg, int64_t ncols) {
  // out is [segment][row][seg]: column j of row i at ((j / seg) * na + i) * seg + j % seg -- each segment's rows are
  // contiguous score rows for K12f (one segment: the plain [na, seg] layout); columns nb <= j < ncols pad the last
  // segment with NaN (K12f ranks NaN last, after every real column of the segment)
  __shared__ __attribute__((aligned(16))) double sa[G::KS][G::PA];
  __shared__ __attribute__((aligned(16))) double sb[G::KS][G::PB];
  constexpr bool JAC = METRIC == CMVE_PW_JACCARD;
  const int tid = threadIdx.x;
  const int tx = tid % G::TX, ty = tid / G::TX;
  const int64_t i0 = (int64_t)blockIdx.y * G::TA, j0 = (int64_t)blockIdx.x * G::TB;
  double s0[G::NA][G::NB] = {}, s1[JAC ? G::NA : 1][JAC ? G::NB : 1] = {};
  pw_tile_loop<G, METRIC>(A, lda, na, B, ldb, nb, d, i0, j0, sa, sb, s0, s1);
#pragma unroll
  for (int u = 0; u < G::NA; ++u) {
    const int64_t i = i0 + G::arow(ty, u);
    if (i >= na) continue;
#pragma unroll
    for (int v = 0; v < G::NB; ++v) {
      const int64_t j = j0 + G::brow(tx, v);
      if (j < ncols)
        out[((j / seg) * na + i) * seg + j % seg] =
            j < nb ? pw_round(pw_score<METRIC>(s0[u][v], JAC ? s1[JAC ? u : 0][JAC ? v : 0] : 0.0, alpha, beta), f32)
                   : (double)NAN;
    }
  }
}

// segment-local ids of K12f's per-segment lists -> global gallery ids; a padding column becomes an empty slot (-1)
__global__ __launch_bounds__(256) void pwr_segment_ids_kernel(int64_t* __restrict__ ids, int64_t n, int64_t per_seg,
                                                              int64_t seg, int64_t j0, int64_t n_g) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const int64_t c = ids[p], j = j0 + (p / per_seg) * seg + c;
  ids[p] = (c >= 0 && j < n_g) ? j : -1;
}

// the winners' ids and their errors (the chain again with the caller's alpha / beta: NaN stays NaN); slots past the
// kf merged entries, and empty ones, hold id -1 / NaN
template <int METRIC, typename TA, typename TB>
__global__ __launch_bounds__(256) void pwr_finish_kernel(const TA* __restrict__ A, int64_t lda, int64_t na,
                                                         const TB* __restrict__ B, int64_t ldb, int64_t nb, int64_t d,
                                                         double alpha, double beta, int f32,
                                                         const int64_t* __restrict__ best_i, int64_t kf, int64_t k,
                                                         int64_t* __restrict__ out_idx, double* __restrict__ out_err) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= na * k) return;
  const int64_t i = p / k, t = p % k;
  const int64_t j = t < kf ? best_i[i * kf + t] : -1;
  const bool ok = j >= 0 && j < nb;
  out_idx[p] = ok ? j : -1;
  out_err[p] = ok ? pw_round(pw_pair_score<METRIC>(A + i * lda, B + j * ldb, d, alpha, beta), f32) : (double)NAN;
}

static bool pwr_dtypes_ok(int32_t a, int32_t b, int32_t s) {
  return (a == CMVE_F32 || a == CMVE_F64) && (b == CMVE_F32 || b == CMVE_F64) && (s == CMVE_F32 || s == CMVE_F64);
}
static int64_t round_up128(int64_t n) { return (n + 127) / 128 * 128; }
// K12f gives a query ONE block; with few queries the gallery chunk is cut into S column segments, each (query,
// segment) a K12f row of its own, and C3's k-way merge joins the segments' lists with the running best (<= 64 lists)
// (<= 63 segments, each at least round_up128(k) columns so that K12f fills every slot of a segment's list)
static int64_t pwr_segments(int64_t n_q, int64_t n_g, int64_t k) {
  if (n_q >= 256) return 1;
  const int64_t by_q = std::min<int64_t>(63, 512 / std::max<int64_t>(n_q, 1));
  return std::max<int64_t>(1, std::min(by_q, round_up128(std::max<int64_t>(n_g, 1)) / round_up128(k)));
}
// bytes of the lists in the segmented layout: S + 1 slabs (running best + S segment lists) and the merge's output
static int64_t pwr_seg_lists_bytes(int64_t nk, int64_t S) { return (2 * S + 4) * nk * 8; }
constexpr int PWR_KMAX = 2048;  // K12f's limit (TD_KMAX, topk.hip): TOPK_MAX of the Python binding

// ---- the best-GT rank of every list from its items' scores and positions (one thread per list) ------------------
// 1 + the least position over the non-NaN items; an empty list ranks n_m + 1, a list whose items all score NaN n_m
// (cmve_rank_from_matrix's rules, metrics.py:137-147)
__global__ __launch_bounds__(256) void pwr_list_ranks_kernel(const int64_t* __restrict__ off,
                                                             const double* __restrict__ sc,
                                                             const int32_t* __restrict__ pos, int64_t n_lists,
                                                             int64_t n_m, int64_t* __restrict__ ranks) {
  const int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (l >= n_lists) return;
  const int64_t lo = off[l], hi = off[l + 1];
  int64_t best = n_m - 1;  // every item NaN
  bool any = false;
  for (int64_t p = lo; p < hi; ++p) {
    const double t = sc[p];
    if (t != t) continue;
    const int64_t q = pos[p];
    best = (any && best < q) ? best : q;
    any = true;
  }
  ranks[l] = hi > lo ? best + 1 : n_m + 1;
}

// launch 1 of one CSR side on the stream (n_items > 0)
static void pwr_item_launch(hipStream_t st, const void* A, int32_t a_dtype, int64_t lda, int64_t na, const void* B,
                            int32_t b_dtype, int64_t ldb, int64_t nb, int64_t d, int32_t metric, double alpha,
                            double beta, int f32, const int64_t* off, const int32_t* idx, int64_t n_items, int col_dir,
                            int64_t idx_base, int shard, double* sc) {
  PW_DISPATCH_METRIC(metric, M, PWR_TYPES(a_dtype, b_dtype, TA, TB, {
    hipLaunchKernelGGL((pwr_item_kernel<M, TA, TB>), dim3((unsigned)((n_items + 255) / 256)), dim3(256), 0, st,
                       (const TA*)A, lda, na, (const TB*)B, ldb, nb, d, alpha, beta, f32, off, idx, col_dir ? nb : na,
                       n_items, col_dir, idx_base, shard, sc);
  }))
}

// launch 2 on the stream: THE counting kernel, over at least one block row and column (a direction whose pos is
// NULL is skipped; pos zeroed by the caller)
static void pwr_count_launch(hipStream_t st, const void* A, int32_t a_dtype, int64_t lda, int64_t na, const void* B,
                             int32_t b_dtype, int64_t ldb, int64_t nb, int64_t d, int32_t metric, double alpha,
                             double beta, int f32, const int64_t* row_off, const double* row_sc, int64_t row_n,
                             int32_t* row_pos, const int64_t* col_off, const double* col_sc, int64_t col_n,
                             int32_t* col_pos) {
  const dim3 grid((unsigned)std::max<int64_t>(1, (nb + PW_TB - 1) / PW_TB),
                  (unsigned)std::max<int64_t>(1, (na + PW_TA - 1) / PW_TA));
  PW_DISPATCH_METRIC(metric, M, PWR_TYPES(a_dtype, b_dtype, TA, TB, {
    hipLaunchKernelGGL((pwr_count_kernel<M, TA, TB>), grid, dim3(256), 0, st, (const TA*)A, lda, na, (const TB*)B, ldb,
                       nb, d, alpha, beta, f32, row_off, row_sc, row_n, row_pos, col_off, col_sc, col_n, col_pos,
                       (const unsigned long long*)nullptr, 0u, (int64_t)0);
  }))
}

void pwr_count_gated_launch(hipStream_t st, int32_t metric, const FltRows& r, double alpha, double beta,
                            const FltLists& l, const l2f_u64* gate) {
  // pwr_count_launch's tiles (at least one block row and column: the NaN-item rule) over at most 64 blocks per compute
  // unit: few enough that a shut gate costs microseconds, many enough that an open one keeps the plain grid's balance
  // (8 per compute unit left whole rounds of resident blocks half empty: +1.3 ms on a 13 ms count, DESIGN s4 K21)
  const int64_t tiles_x = std::max<int64_t>(1, (r.nb + PW_TB - 1) / PW_TB);
  const int64_t tiles = tiles_x * std::max<int64_t>(1, (r.na + PW_TA - 1) / PW_TA);
  const unsigned blocks = (unsigned)std::min<int64_t>(tiles, 64 * (int64_t)device_cus());
#define PWR_GATED(M, F32)                                                                                             \
  PWR_TYPES(r.a_dtype, r.b_dtype, TA, TB, {                                                                           \
    hipLaunchKernelGGL((pwr_count_kernel<M, TA, TB, true>), dim3(blocks), dim3(256), 0, st, (const TA*)r.A, r.lda,    \
                       r.na, (const TB*)r.B, r.ldb, r.nb, r.d, alpha, beta, F32, l.row_off, l.row_sc, l.row_n,        \
                       l.row_pos, l.col_off, l.col_sc, l.col_n, l.col_pos, gate, (unsigned)tiles_x, tiles);           \
  })
  // (the filters' words: fp64 under CMVE_PW_L2 / CMVE_PW_L1, float32 under CMVE_PW_JACCARD -- K24)
  if (metric == CMVE_PW_L1) { PWR_GATED(CMVE_PW_L1, 0) }
  else if (metric == CMVE_PW_JACCARD) { PWR_GATED(CMVE_PW_JACCARD, 1) }
  else { PWR_GATED(CMVE_PW_L2, 0) }
#undef PWR_GATED
}

}  // namespace cmve

using namespace cmve;

extern "C" int cmve_pairwise_positions_workspace(int64_t na, int64_t nb, int64_t row_items, int64_t col_items,
                                                 int32_t metric, int64_t* bytes) {
  CMVE_REQUIRE(bytes, "cmve_pairwise_positions_workspace: NULL argument");
  CMVE_REQUIRE(na >= 0 && nb >= 0 && row_items >= 0 && col_items >= 0,
               "cmve_pairwise_positions_workspace: bad shape (%lld, %lld; %lld, %lld items)", (long long)na,
               (long long)nb, (long long)row_items, (long long)col_items);
  CMVE_REQUIRE(metric >= CMVE_PW_SQ_L2 && metric <= CMVE_PW_DOT, "cmve_pairwise_positions_workspace: unknown metric %d",
               metric);
  CMVE_REQUIRE(row_items <= INT64_MAX / 16 && col_items <= INT64_MAX / 16,
               "cmve_pairwise_positions_workspace: the item count overflows");
  *bytes = (row_items + col_items) * (int64_t)sizeof(double);  // the item scores and nothing else
  return CMVE_OK;
}

extern "C" int cmve_pairwise_positions(cmve_handle_t h, const void* A, int32_t a_dtype, int64_t lda, int64_t na,
                                       const void* B, int32_t b_dtype, int64_t ldb, int64_t nb, int64_t d,
                                       int32_t metric, double alpha, double beta, int32_t score_dtype,
                                       const int64_t* row_off, const int32_t* row_idx, int64_t row_items,
                                       int32_t* row_pos, const int64_t* col_off, const int32_t* col_idx,
                                       int64_t col_items, int32_t* col_pos, void* ws, int64_t ws_bytes) {
  CMVE_REQUIRE(h && (A || !na) && (B || !nb), "cmve_pairwise_positions: NULL argument");
  CMVE_REQUIRE(na >= 0 && nb >= 0 && na < (1ll << 31) && nb < (1ll << 31) && d > 0 && lda >= d && ldb >= d,
               "cmve_pairwise_positions: bad shape");
  CMVE_REQUIRE(pwr_dtypes_ok(a_dtype, b_dtype, score_dtype), "cmve_pairwise_positions: dtypes must be CMVE_F32/CMVE_F64");
  if (!row_pos) row_items = 0;
  if (!col_pos) col_items = 0;
  int64_t need = 0;
  if (int rc = cmve_pairwise_positions_workspace(na, nb, row_items, col_items, metric, &need)) return rc;
  CMVE_REQUIRE(!row_pos || (row_off && (row_idx || !row_items)), "cmve_pairwise_positions: row lists missing");
  CMVE_REQUIRE(!col_pos || (col_off && (col_idx || !col_items)), "cmve_pairwise_positions: column lists missing");
  CMVE_REQUIRE(row_items < (1ll << 31) * 256 && col_items < (1ll << 31) * 256, "cmve_pairwise_positions: too many items");
  if (row_items + col_items == 0) return CMVE_OK;
  CMVE_REQUIRE(ws && ws_bytes >= need, "cmve_pairwise_positions: workspace too small (%lld < %lld bytes)",
               (long long)ws_bytes, (long long)need);
  CMVE_REQUIRE((((uintptr_t)ws) & 7) == 0, "cmve_pairwise_positions: workspace must be 8-byte aligned");
  CMVE_REQUIRE((na + PW_TA - 1) / PW_TA < 65536, "cmve_pairwise_positions: too many rows in A (%lld)", (long long)na);
  const hipStream_t st = h->stream;
  double* row_sc = (double*)ws;
  double* col_sc = row_sc + row_items;
  if (row_items) CMVE_HIP(hipMemsetAsync(row_pos, 0, sizeof(int32_t) * row_items, st));
  if (col_items) CMVE_HIP(hipMemsetAsync(col_pos, 0, sizeof(int32_t) * col_items, st));
  if (na == 0 || nb == 0) return CMVE_OK;  // no pair: every count is zero (and a NaN item's n - ... has n = 0)
  const int f32 = score_dtype == CMVE_F32;
  // its own item launches (an index outside the other side scores NaN), then the counting kernel of
  // cmve_pairwise_count with the whole sides as n
  if (row_items)
    pwr_item_launch(st, A, a_dtype, lda, na, B, b_dtype, ldb, nb, d, metric, alpha, beta, f32, row_off, row_idx,
                    row_items, 0, 0, 0, row_sc);
  if (col_items)
    pwr_item_launch(st, A, a_dtype, lda, na, B, b_dtype, ldb, nb, d, metric, alpha, beta, f32, col_off, col_idx,
                    col_items, 1, 0, 0, col_sc);
  pwr_count_launch(st, A, a_dtype, lda, na, B, b_dtype, ldb, nb, d, metric, alpha, beta, f32, row_off, row_sc, nb,
                   row_items ? row_pos : nullptr, col_off, col_sc, na, col_items ? col_pos : nullptr);
  return check_launch("pairwise_positions");
}

extern "C" int cmve_pairwise_item_scores(cmve_handle_t h, const void* A, int32_t a_dtype, int64_t lda, int64_t na,
                                         const void* B, int32_t b_dtype, int64_t ldb, int64_t nb, int64_t d,
                                         int32_t metric, double alpha, double beta, int32_t score_dtype,
                                         const int64_t* off, const int32_t* idx, int64_t n_lists, int64_t n_items,
                                         int32_t col_dir, int64_t idx_base, double* out) {
  CMVE_REQUIRE(h && (A || !na) && (B || !nb) && off && (n_items <= 0 || (idx && out)),
               "cmve_pairwise_item_scores: NULL argument");
  CMVE_REQUIRE(na >= 0 && nb >= 0 && na < (1ll << 31) && nb < (1ll << 31) && d > 0 && lda >= d && ldb >= d,
               "cmve_pairwise_item_scores: bad shape");
  CMVE_REQUIRE(pwr_dtypes_ok(a_dtype, b_dtype, score_dtype),
               "cmve_pairwise_item_scores: dtypes must be CMVE_F32/CMVE_F64");
  CMVE_REQUIRE(metric >= CMVE_PW_SQ_L2 && metric <= CMVE_PW_DOT, "cmve_pairwise_item_scores: unknown metric %d", metric);
  CMVE_REQUIRE(n_items >= 0 && n_items < (1ll << 31) * 256, "cmve_pairwise_item_scores: bad item count (%lld)",
               (long long)n_items);
  CMVE_REQUIRE(col_dir == 0 || col_dir == 1, "cmve_pairwise_item_scores: col_dir must be 0 or 1");
  CMVE_REQUIRE(n_lists == (col_dir ? nb : na),
               "cmve_pairwise_item_scores: %lld lists for the %lld rows that own them", (long long)n_lists,
               (long long)(col_dir ? nb : na));
  if (n_items == 0) return CMVE_OK;
  pwr_item_launch(h->stream, A, a_dtype, lda, na, B, b_dtype, ldb, nb, d, metric, alpha, beta,
                  score_dtype == CMVE_F32, off, idx, n_items, col_dir, idx_base, 1, out);
  return check_launch("pairwise_item_scores");
}

extern "C" int cmve_pairwise_count(cmve_handle_t h, const void* A, int32_t a_dtype, int64_t lda, int64_t na,
                                   const void* B, int32_t b_dtype, int64_t ldb, int64_t nb, int64_t d, int32_t metric,
                                   double alpha, double beta, int32_t score_dtype, const int64_t* row_off,
                                   const double* row_sc, int64_t row_items, int64_t row_n, int32_t* row_pos,
                                   const int64_t* col_off, const double* col_sc, int64_t col_items, int64_t col_n,
                                   int32_t* col_pos) {
  CMVE_REQUIRE(h && (A || !na) && (B || !nb), "cmve_pairwise_count: NULL argument");
  CMVE_REQUIRE(na >= 0 && nb >= 0 && na < (1ll << 31) && nb < (1ll << 31) && d > 0 && lda >= d && ldb >= d,
               "cmve_pairwise_count: bad shape");
  CMVE_REQUIRE(pwr_dtypes_ok(a_dtype, b_dtype, score_dtype), "cmve_pairwise_count: dtypes must be CMVE_F32/CMVE_F64");
  CMVE_REQUIRE(metric >= CMVE_PW_SQ_L2 && metric <= CMVE_PW_DOT, "cmve_pairwise_count: unknown metric %d", metric);
  FltLists l{row_off, row_sc, row_items, row_n, row_pos, col_off, col_sc, col_items, col_n, col_pos};
  if (int rc = flt_check_lists("cmve_pairwise_count", l)) return rc;
  if (l.row_items + l.col_items == 0) return CMVE_OK;
  CMVE_REQUIRE((na + PW_TA - 1) / PW_TA < 65536, "cmve_pairwise_count: too many rows in A (%lld)", (long long)na);
  const hipStream_t st = h->stream;
  if (l.row_items) CMVE_HIP(hipMemsetAsync(l.row_pos, 0, sizeof(int32_t) * l.row_items, st));
  if (l.col_items) CMVE_HIP(hipMemsetAsync(l.col_pos, 0, sizeof(int32_t) * l.col_items, st));
  // an empty shard has no pair to count; it still runs one block row / column where a direction has items AND an n
  // to apply: the NaN items' words are the caller's n, not this shard's
  if ((na == 0 || nb == 0) && !(l.row_items && row_n) && !(l.col_items && col_n)) return CMVE_OK;
  pwr_count_launch(st, A, a_dtype, lda, na, B, b_dtype, ldb, nb, d, metric, alpha, beta, score_dtype == CMVE_F32,
                   row_off, row_sc, row_n, l.row_pos, col_off, col_sc, col_n, l.col_pos);
  return check_launch("pairwise_count");
}

extern "C" int cmve_pairwise_list_ranks(cmve_handle_t h, const int64_t* off, const double* sc, const int32_t* pos,
                                        int64_t n_lists, int64_t n_m, int64_t* ranks) {
  CMVE_REQUIRE(h && off && sc && pos && (n_lists <= 0 || ranks), "cmve_pairwise_list_ranks: NULL argument");
  CMVE_REQUIRE(n_lists >= 0 && n_m >= 0 && n_lists < (1ll << 31) * 256,
               "cmve_pairwise_list_ranks: bad counts (%lld lists, n %lld)", (long long)n_lists, (long long)n_m);
  if (n_lists == 0) return CMVE_OK;
  hipLaunchKernelGGL(pwr_list_ranks_kernel, dim3((unsigned)((n_lists + 255) / 256)), dim3(256), 0, h->stream, off, sc,
                     pos, n_lists, n_m, ranks);
  return check_launch("pairwise_list_ranks");
}

extern "C" int cmve_pairwise_topk_workspace(int64_t n_q, int64_t n_g, int32_t k, int32_t metric, int64_t* min_bytes,
                                            int64_t* rec_bytes) {
  CMVE_REQUIRE(min_bytes && rec_bytes, "cmve_pairwise_topk_workspace: NULL argument");
  CMVE_REQUIRE(n_q >= 0 && n_g >= 0, "cmve_pairwise_topk_workspace: bad shape (%lld, %lld)", (long long)n_q,
               (long long)n_g);
  CMVE_REQUIRE(k >= 1 && k <= PWR_KMAX, "cmve_pairwise_topk_workspace: k must be in [1, %d]", PWR_KMAX);
  CMVE_REQUIRE(metric >= CMVE_PW_SQ_L2 && metric <= CMVE_PW_DOT, "cmve_pairwise_topk_workspace: unknown metric %d",
               metric);
  // the two best-lists (fp64 score + int64 id, k per query, double-buffered) and one 128-column chunk of scores
  CMVE_REQUIRE(n_q <= (INT64_MAX / 64) / ((int64_t)k + 128) && n_g <= INT64_MAX / 2,
               "cmve_pairwise_topk_workspace: n_q * k overflows");
  const int64_t best = n_q * (int64_t)k * 32;
  *min_bytes = best + n_q * 128 * 8;
  // recommended: the whole gallery in one chunk, or as many 128-column groups as 256 MiB of scores hold
  const int64_t cap = std::max<int64_t>((256ll << 20) / 8 / std::max<int64_t>(n_q, 1) / 128 * 128, 128);
  const int64_t S = pwr_segments(n_q, n_g, k);
  if (S > 1) {  // few queries: the segment lists beside the best-lists, the scores in S equal segments of >= k columns
    const int64_t seg = std::max(round_up128((std::max<int64_t>(n_g, 1) + S - 1) / S), round_up128(k));
    *rec_bytes = std::max(*min_bytes, pwr_seg_lists_bytes(n_q * (int64_t)k, S) + n_q * std::min(S * seg, cap) * 8);
    return CMVE_OK;
  }
  const int64_t scores = n_q * std::min(round_up128(std::max<int64_t>(n_g, 1)), cap) * 8;
  *rec_bytes = best + scores;
  return CMVE_OK;
}

extern "C" int cmve_pairwise_topk(cmve_handle_t h, const void* Q, int32_t q_dtype, int64_t ldq, int64_t n_q,
                                  const void* Gm, int32_t g_dtype, int64_t ldg, int64_t n_g, int64_t d,
                                  int32_t metric, double alpha, double beta, int32_t score_dtype, int32_t k,
                                  int32_t geometry, void* ws, int64_t ws_bytes, int64_t* out_idx, double* out_err) {
  CMVE_REQUIRE(h && (Q || !n_q) && (Gm || !n_g) && ((out_idx && out_err) || !n_q), "cmve_pairwise_topk: NULL argument");
  CMVE_REQUIRE(n_q >= 0 && n_g >= 0 && d > 0 && ldq >= d && ldg >= d, "cmve_pairwise_topk: bad shape");
  CMVE_REQUIRE(pwr_dtypes_ok(q_dtype, g_dtype, score_dtype), "cmve_pairwise_topk: dtypes must be CMVE_F32/CMVE_F64");
  CMVE_REQUIRE(geometry >= 0 && geometry <= 2 && (geometry != 2 || n_q <= PwSmall::TA),
               "cmve_pairwise_topk: geometry must be 0 (by n_q), 1 (64-row tiles) or 2 (8-row tiles, n_q <= 8)");
  int64_t need = 0, rec = 0;
  if (int rc = cmve_pairwise_topk_workspace(n_q, n_g, k, metric, &need, &rec)) return rc;
  if (n_q == 0) return CMVE_OK;
  CMVE_REQUIRE(ws && ws_bytes >= need, "cmve_pairwise_topk: workspace too small (%lld < %lld bytes)",
               (long long)ws_bytes, (long long)need);
  CMVE_REQUIRE((((uintptr_t)ws) & 7) == 0, "cmve_pairwise_topk: workspace must be 8-byte aligned");
  CMVE_REQUIRE((n_q + PW_TA - 1) / PW_TA < 65536, "cmve_pairwise_topk: too many query rows (%lld)", (long long)n_q);
  CMVE_REQUIRE(n_q * (int64_t)k < (1ll << 31) * 256, "cmve_pairwise_topk: too many outputs");
  const hipStream_t st = h->stream;
  const int64_t nk = n_q * (int64_t)k;
  double* best_s[2] = {(double*)ws, (double*)ws + nk};
  int64_t* best_i[2] = {(int64_t*)ws + 2 * nk, (int64_t*)ws + 3 * nk};
  double* scores = (double*)ws + 4 * nk;
  const bool small = geometry == 2 || (geometry == 0 && n_q <= PwSmall::TA);
  const int f32 = score_dtype == CMVE_F32;
  const int64_t esz = g_dtype == CMVE_F64 ? 8 : 4;
#define PWR_CHUNK(gp, nc, seg, ncols)                                                                                  \
  PW_DISPATCH_METRIC(metric, M, PWR_TYPES(q_dtype, g_dtype, TA, TB, {                                                  \
    if (small)                                                                                                         \
      hipLaunchKernelGGL((pwr_chunk_kernel<PwSmall, M, TA, TB>),                                                       \
                         dim3((unsigned)(((ncols) + PwSmall::TB - 1) / PwSmall::TB), 1), dim3(256), 0, st, (const TA*)Q, \
                         ldq, n_q, (const TB*)(gp), ldg, nc, d, -alpha, -beta, f32, scores, seg, ncols);                \
    else                                                                                                               \
      hipLaunchKernelGGL((pwr_chunk_kernel<PwWide, M, TA, TB>),                                                        \
                         dim3((unsigned)(((ncols) + PW_TB - 1) / PW_TB), (unsigned)((n_q + PW_TA - 1) / PW_TA)),        \
                         dim3(256), 0, st, (const TA*)Q, ldq, n_q, (const TB*)(gp), ldg, nc, d, -alpha, -beta, f32,     \
                         scores, seg, ncols);                                                                          \
  }))
  // Few queries and room in the workspace: the segmented merge.  The largest S <= pwr_segments(n_q) whose lists and
  // S segments of >= k columns (K12f then fills every slot of a segment's list) fit; S = 1 is the plain loop below.
  int64_t S = pwr_segments(n_q, n_g, k);
  const int64_t seg_min = round_up128(k);
  while (S > 1 && pwr_seg_lists_bytes(nk, S) + n_q * S * seg_min * 8 > ws_bytes) --S;
  if (S > 1) {
    double* X_s = (double*)ws;                       // [S + 1][n_q][k]: slab 0 the running best, 1.. the segments
    int64_t* X_i = (int64_t*)ws + (S + 1) * nk;
    double* T_s = (double*)ws + 2 * (S + 1) * nk;    // the merge's output, copied into slab 0
    int64_t* T_i = (int64_t*)ws + 2 * (S + 1) * nk + nk;
    scores = (double*)ws + (2 * S + 4) * nk;
    const int64_t seg = std::min((ws_bytes - pwr_seg_lists_bytes(nk, S)) / 8 / n_q / S / 128 * 128,
                                 std::max(round_up128((n_g + S - 1) / S), seg_min));
    CMVE_HIP(hipMemsetAsync(X_i, 0xff, nk * 8, st));  // an empty running best: every id -1
    for (int64_t j0 = 0; j0 < n_g; j0 += S * seg) {
      const int64_t nc = std::min(S * seg, n_g - j0), Se = (nc + seg - 1) / seg;
      PWR_CHUNK((const char*)Gm + j0 * ldg * esz, nc, seg, Se * seg)
      if (int rc = check_launch("pairwise_topk chunk")) return rc;
      if (int rc = cmve_topk_dense_merge(h, nullptr, nullptr, 0, scores, seg, Se * n_q, seg, 0, k, X_s + nk, X_i + nk))
        return rc;
      hipLaunchKernelGGL(pwr_segment_ids_kernel, dim3((unsigned)((Se * nk + 255) / 256)), dim3(256), 0, st, X_i + nk,
                         Se * nk, nk, seg, j0, n_g);
      if (int rc = merge_topk_launch(st, X_i, X_s, n_q, (int)(Se + 1), (int)k, (int64_t)k, nk, (int)k, T_i, T_s))
        return rc;
      CMVE_HIP(hipMemcpyAsync(X_s, T_s, nk * 8, hipMemcpyDeviceToDevice, st));
      CMVE_HIP(hipMemcpyAsync(X_i, T_i, nk * 8, hipMemcpyDeviceToDevice, st));
    }
    PW_DISPATCH_METRIC(metric, M, PWR_TYPES(q_dtype, g_dtype, TA, TB, {
      hipLaunchKernelGGL((pwr_finish_kernel<M, TA, TB>), dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, st,
                         (const TA*)Q, ldq, n_q, (const TB*)Gm, ldg, n_g, d, alpha, beta, f32, (const int64_t*)X_i,
                         (int64_t)k, (int64_t)k, out_idx, out_err);
    }))
    return check_launch("pairwise_topk");
  }
  // the chunk: as many 128-column groups as the workspace holds, at most the gallery
  const int64_t chunk = std::min((ws_bytes - nk * 32) / 8 / n_q / 128 * 128, round_up128(std::max<int64_t>(n_g, 1)));
  int64_t kb = 0;  // entries of the running best: min(k, columns merged so far), its row stride
  int cur = 0;
  for (int64_t j0 = 0; j0 < n_g; j0 += chunk) {
    const int64_t nc = std::min(chunk, n_g - j0);
    // -error = (-alpha) f + (-beta): round-to-nearest is symmetric, so this is exactly the negated score
    PWR_CHUNK((const char*)Gm + j0 * ldg * esz, nc, chunk, nc)
    if (int rc = check_launch("pairwise_topk chunk")) return rc;
    const int64_t kn = std::min<int64_t>(k, kb + nc);
    if (int rc = cmve_topk_dense_merge(h, best_s[cur], best_i[cur], kb, scores, chunk, n_q, nc, j0, (int32_t)kn,
                                       best_s[1 - cur], best_i[1 - cur]))
      return rc;
    kb = kn;
    cur = 1 - cur;
  }
  PW_DISPATCH_METRIC(metric, M, PWR_TYPES(q_dtype, g_dtype, TA, TB, {
    hipLaunchKernelGGL((pwr_finish_kernel<M, TA, TB>), dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, st,
                       (const TA*)Q, ldq, n_q, (const TB*)Gm, ldg, n_g, d, alpha, beta, f32,
                       (const int64_t*)best_i[cur], kb, (int64_t)k, out_idx, out_err);
  }))
  return check_launch("pairwise_topk");
#undef PWR_CHUNK
}
