// The pass kernel of the integer SAD top-k filters, written once (K23: l1_topk.hip under CMVE_PW_L1; K25:
// jaccard_topk.hip under CMVE_PW_JACCARD): the tile of the block and the round's tile q0 / 128 + ta of the tiled codes,
// l1f_sad_tile's 128 x 128 tile on 256 threads of 8 x 8 u32 accumulators, then the fp64 epilogue -- the sides' terms
// and the rows' state (l2t_row_state) into LDS, the 8 x 8 pairs with their bounds test, the two counters
// (l2t_flush) -- and the host pieces the two top-k entries share.  sad_count.h's sibling.  A filter supplies a policy P
// with only what differs:
//   P::Args                       the kernel's flat argument block: SadTopkArgs (the common prefix) plus the filter's
//                                 own scalars and pointers
//   P::NS                         the doubles a side carries per row
//   P::side<G>(a, v, i, lo, s, x) the terms of query i (G: of gallery row i); v: the row is in the pass
//   P::step(E.s)                  the grid's step as a row of pairs reads it: plain (l1) or re-read (jaccard)
//   P::pair<MODE>(a, pos, i, j, sad, s, xq, xg, thr, full, n_cand, n_excl)
//                                 SAD and two sides -> the pair's interval -> launch A's stored bound (MODE 0) or
//                                 launch B's verdict (MODE 1, ending in l2t_decide)
// l2t_pass_kernel (K20) keeps a kernel of its own: an MFMA tile on another thread layout.
#ifndef CMVE_SAD_TOPK_H
#define CMVE_SAD_TOPK_H
#include "l1_filter_tile.h"
#include "topk_filter_tile.h"

namespace cmve {

// the common prefix of a SAD pass kernel's flat argument block (a policy's Args derives from it and adds its own
// fields: one block, no nesting -- sad_count.h records what an embedded struct cost l1f_main_kernel)
struct SadTopkArgs {
  const uint32_t* q_codes;  // tiled (l1_filter_tile.h)
  const uint32_t* g_codes;
  const double* q_err;
  const double* g_err;
  const double* grid;
  int64_t q0, q_end;  // this round's queries; q0 is a multiple of 128
  int64_t ng;         // columns of this pass: the sample (A) or the gallery (B)
  int nkt;            // K tiles
  double alpha;
  float* ub;          // A: [q_end - q0][ub_ld] upper key bounds
  int64_t ub_ld;
  const double* thr;  // B: per query the threshold in the filter's own space (NaN: unresolved, nothing is appended)
  int32_t* cnt;       // B: candidates found per query
  int32_t* list;      // B: [q_end - q0][cap] column ids
  int64_t cap;
  l2f_u64* stats;     // {pairs excluded, candidates found, candidates re-scored, unresolved queries}
  int tiles_a, tiles_b;
};

// the epilogue's LDS, laid over the staging buffers once the K loop is done (thr .. n_excl: the names l2t_row_state /
// l2t_flush use)
template <int NS>
struct SadTopkEpi {
  double sq[NS][L1F_BM], sg[NS][L1F_BN];  // the sides' terms of the tile's rows / columns
  double thr[L1F_BM];
  int full[L1F_BM];  // the row's list had overflowed when this tile began: its candidates are counted, not appended
  int n_cand, n_excl;
  double s;  // the grid's step
};

// MODE 0: launch A (the witnesses' bounds), MODE 1: launch B (the candidates)
template <typename P, int MODE>
__device__ __forceinline__ void sad_topk_body(const typename P::Args& a) {
  using Epi = SadTopkEpi<P::NS>;
  static_assert(sizeof(Epi) <= L1F_SMEM, "the epilogue's LDS fits the staging buffers");
  __shared__ __attribute__((aligned(16))) char smem[L1F_SMEM];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  int ta, tb_;
  l2f_tile_of_block(blockIdx.x, a.tiles_a, a.tiles_b, ta, tb_);
  // q0 is a multiple of 128: the round's tile ta is tile q0 / 128 + ta of the tiled codes.  Both sets hold n_pad (a
  // multiple of 128) rows and d_pad elements: the tiles' blocks are in bounds.
  const int64_t qt = a.q0 / L1F_BM + ta;
  const int64_t i0 = qt * L1F_BM, j0 = (int64_t)tb_ * L1F_BN;

  // ---- the SADs: acc[u][v] of the pair (query i0 + l1f_row(ty, u), gallery row j0 + l1f_row(tx, v))
  uint32_t acc[8][8];
  l1f_sad_tile(a.q_codes + qt * a.nkt * L1F_TILE_DW, a.g_codes + (int64_t)tb_ * a.nkt * L1F_TILE_DW, a.nkt, smem, acc);

  // ---- epilogue (every wave has passed the loop's last barrier: smem is free): one threshold per row, no rounds ----
  Epi& E = *(Epi*)smem;
  double lo, s;
  l1f_grid_of(a.grid, lo, s);
  double x[P::NS];
  if (tid < L1F_BM) {
    const int64_t i = i0 + tid;
    const bool v = i < a.q_end;  // a row beyond the round: no interval (and never used)
    P::template side<false>(a, v, i, lo, s, x);
#pragma unroll
    for (int k = 0; k < P::NS; ++k) E.sq[k][tid] = x[k];
    l2t_row_state<MODE>(a, E, tid, i, v);
  } else {
    const int t = tid - L1F_BM;
    const int64_t j = j0 + t;
    P::template side<true>(a, j < a.ng, j, lo, s, x);
#pragma unroll
    for (int k = 0; k < P::NS; ++k) E.sg[k][t] = x[k];
  }
  if (tid == 0) {
    E.n_cand = E.n_excl = 0;
    E.s = s;
  }
  __syncthreads();
  const bool pos = a.alpha > 0.0;
  int n_cand = 0, n_excl = 0;
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int row = l1f_row(ty, u);
    const int64_t i = i0 + row;
    const double sv = P::step(E.s);
    double xq[P::NS];
#pragma unroll
    for (int k = 0; k < P::NS; ++k) xq[k] = E.sq[k][row];
    const double thr = MODE == 1 ? E.thr[row] : 0.0;
    const bool full = MODE == 1 ? E.full[row] != 0 : false;
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      const int col = l1f_row(tx, v);
      const int64_t j = j0 + col;
      if (i >= a.q_end || j >= a.ng) continue;
      double xg[P::NS];
#pragma unroll
      for (int k = 0; k < P::NS; ++k) xg[k] = E.sg[k][col];
      P::template pair<MODE>(a, pos, i, j, acc[u][v], sv, xq, xg, thr, full, n_cand, n_excl);
    }
  }
  l2t_flush<MODE>(a, E, tid, n_cand, n_excl);
}

// ---- the host side ------------------------------------------------------------------------------------------------------
// the common prefix of a pass kernel's argument block from what l2t_topk_run hands a pass launch (n_q: the whole
// call's queries, d: the rows' elements)
static inline SadTopkArgs sad_topk_args(const L2tRound& r, const L2tWs& w, const void* q_codes, const double* q_err,
                                        const void* g_codes, const double* g_err, const double* grid, int64_t n_q,
                                        int64_t d, double alpha) {
  int64_t n_pad = 0, d_pad = 0;
  l1f_pads(n_q, d, n_pad, d_pad);
  return SadTopkArgs{(const uint32_t*)q_codes, (const uint32_t*)g_codes, q_err, g_err, grid, r.q0, r.q_end, r.ng,
                     (int)(d_pad / L1F_BK), alpha, w.ub, w.ub_ld, w.thr, w.cnt, w.list, w.cap, w.stats, r.tiles_a,
                     r.tiles_b};
}

// the workspace of a top-k entry (`name`: the *_topk_workspace entry)
static inline int sad_topk_workspace(const char* name, int64_t n_q, int64_t n_g, int32_t k, int64_t cand_cap,
                                     int64_t sample_rows, int64_t* bytes) {
  CMVE_REQUIRE(bytes, "%s: NULL argument", name);
  if (int rc = l2t_check_params(name, k, cand_cap, sample_rows)) return rc;
  CMVE_REQUIRE(n_q >= 0 && n_g >= 0 && n_q < (1ll << 31) && n_g < (1ll << 31), "%s: bad shape (%lld, %lld rows)", name,
               (long long)n_q, (long long)n_g);
  *bytes = l2t_layout(n_q, n_g, k, cand_cap, sample_rows).bytes;
  return CMVE_OK;
}

}  // namespace cmve
#endif
