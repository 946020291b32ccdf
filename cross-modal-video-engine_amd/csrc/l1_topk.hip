// K23: cmve_pairwise_topk under the L1 measures (l1 / l1_norm: CMVE_PW_L1, fp64 score words) at the integer SAD rate
// -- what
//   LINAS-engine/inference.py:78-80      cal_error(video_embs, cap_emb, measure) -> np.argsort(errors[0])[:topK]
//   LINAS-engine/evaluation.py:22-35     cal_error under l1 / l1_norm
// compute per caption.  The k smallest errors are the k smallest keys  s L,  s = sign(alpha), L the true L1 distance
// of the pair (no square); K22's SAD of the uint16 codes (l1_filter_tile.h) brackets every pair's L, so K20's scheme
// (l2_topk.hip, topk_filter_tile.h) carries over launch by launch:
//   launch A   l1t_pass_kernel<0>        the SAD tile over the first `sample_rows` gallery rows; the epilogue stores
//                                        every pair's UPPER key bound (fp32, rounded up; +inf without an interval)
//   launch A'  l2t_threshold_kernel<false>  the k-th smallest stored bound per query, widened to an L1-distance
//                                        threshold beyond which a column's canonical word is STRICTLY worse than
//                                        every witness's (DESIGN s4, "K23")
//   launch B   l1t_pass_kernel<1>        the same tile over the whole gallery; a pair without an interval, or whose
//                                        lower key bound does not clear the threshold, is appended to its query's
//                                        candidate list (integer atomic counter)
//   launch C   l2t_finish_kernel<CMVE_PW_L1>  a block per query: the candidates on the canonical chain, sorted, k
//                                        emitted
// so out_idx / out_err are, word for word, cmve_pairwise_topk's.  The grid offset lo cancels in the SAD: rows
// clustered far from the origin keep intervals as tight as rows around it.  Plain vector stores and integer atomics
// only.  This file holds what is this filter's alone: the pass kernel's argument block, its interval and thread
// layout, and the entry's checks of its own operands.  The SAD tile is l1_filter_tile.h's (l1f_sad_tile, shared with
// K22's count kernel); the tail of the epilogue, launches A' and C and the host body (l2t_topk_run: checks, workspace,
// the rounds of four launches) are topk_filter_tile.h's, shared with K20.
#include "l1_filter_tile.h"
#include "topk_filter_tile.h"

namespace cmve {
namespace {

struct L1tArgs {
  const uint32_t* q_codes;  // tiled (l1_filter_tile.h)
  const uint32_t* g_codes;
  const double* q_err;
  const double* g_err;
  const double* grid;
  int64_t q0, q_end;  // this round's queries; q0 is a multiple of 128
  int64_t ng;         // columns of this pass: the sample (A) or the gallery (B)
  int nkt;            // K tiles
  double alpha, lim;
  float* ub;          // A: [q_end - q0][ub_ld] upper key bounds
  int64_t ub_ld;
  const double* thr;  // B: per query the L1-distance threshold (NaN: unresolved, nothing is appended)
  int32_t* cnt;       // B: candidates found per query
  int32_t* list;      // B: [q_end - q0][cap] column ids
  int64_t cap;
  l2f_u64* stats;     // {pairs excluded, candidates found, candidates re-scored, unresolved queries}
  int tiles_a, tiles_b;
};

// the epilogue's LDS, laid over the staging buffers once the K loop is done
struct L1tEpi {
  double qe[L1F_BM], ge[L1F_BN];  // row errors of the tile's rows / columns
  double thr[L1F_BM];
  int full[L1F_BM];  // the row's list had overflowed when this tile began: its candidates are counted, not appended
  int n_cand, n_excl;
  double s;  // the grid's step
};
static_assert(sizeof(L1tEpi) <= L1F_SMEM, "the epilogue's LDS fits the staging buffers");

// MODE 0: launch A (the witnesses' bounds), MODE 1: launch B (the candidates)
template <int MODE>
__global__ __launch_bounds__(256, 4) void l1t_pass_kernel(L1tArgs a) {
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
  L1tEpi& E = *(L1tEpi*)smem;
  if (tid < L1F_BM) {
    const int64_t i = i0 + tid;
    const bool v = i < a.q_end;
    E.qe[tid] = v ? a.q_err[i] : (double)NAN;  // a row beyond the round: no interval (and never used)
    l2t_row_state<MODE>(a, E, tid, i, v);
  } else {
    const int t = tid - L1F_BM;
    const int64_t j = j0 + t;
    E.ge[t] = j < a.ng ? a.g_err[j] : (double)NAN;
  }
  if (tid == 0) {
    E.n_cand = E.n_excl = 0;
    double lo_unused, s;
    l1f_grid_of(a.grid, lo_unused, s);
    E.s = s;
  }
  __syncthreads();
  const bool pos = a.alpha > 0.0;
  const double s = E.s;
  int n_cand = 0, n_excl = 0;
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int64_t i = i0 + l1f_row(ty, u);
    const double qe = E.qe[l1f_row(ty, u)];
    const double thr = MODE == 1 ? E.thr[l1f_row(ty, u)] : 0.0;
    const bool full = MODE == 1 ? E.full[l1f_row(ty, u)] != 0 : false;
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      const int64_t j = j0 + l1f_row(tx, v);
      if (i >= a.q_end || j >= a.ng) continue;
      double dlo, dhi;
      l1f_interval(acc[u][v], s, qe, E.ge[l1f_row(tx, v)], a.lim, dlo, dhi);
      l2t_pair<MODE>(a, pos, i, j, dlo, dhi, thr, full, n_cand, n_excl);
    }
  }
  l2t_flush<MODE>(a, E, tid, n_cand, n_excl);
}

}  // namespace
}  // namespace cmve

using namespace cmve;

extern "C" int cmve_l1_topk_workspace(int64_t n_q, int64_t n_g, int32_t k, int64_t cand_cap, int64_t sample_rows,
                                      int64_t* bytes) {
  CMVE_REQUIRE(bytes, "cmve_l1_topk_workspace: NULL argument");
  if (int rc = l2t_check_params("cmve_l1_topk_workspace", k, cand_cap, sample_rows)) return rc;
  CMVE_REQUIRE(n_q >= 0 && n_g >= 0 && n_q < (1ll << 31) && n_g < (1ll << 31),
               "cmve_l1_topk_workspace: bad shape (%lld, %lld rows)", (long long)n_q, (long long)n_g);
  *bytes = l2t_layout(n_q, n_g, k, cand_cap, sample_rows).bytes;
  return CMVE_OK;
}

extern "C" int cmve_l1_topk(cmve_handle_t h, const void* Q, int32_t q_dtype, int64_t ldq, int64_t n_q,
                            const void* q_codes, const double* q_err, const void* G, int32_t g_dtype, int64_t ldg,
                            int64_t n_g, const void* g_codes, const double* g_err, int64_t d, const double* grid,
                            double alpha, double beta, int32_t k, int64_t cand_cap, int64_t sample_rows, void* ws,
                            int64_t ws_bytes, int64_t* out_idx, double* out_err, int64_t* stats) {
  const char* name = "cmve_l1_topk";
  CMVE_REQUIRE(h && stats && (Q || !n_q) && (G || !n_g), "%s: NULL argument", name);
  auto own_checks = [&]() -> int {
    CMVE_REQUIRE(d > 0 && d <= L1F_D_MAX, "%s: d must be in [1, %lld] (%lld): the u32 SAD is exact up to there", name,
                 (long long)L1F_D_MAX, (long long)d);
    CMVE_REQUIRE(n_q >= 0 && n_g >= 0 && n_q < (1ll << 31) && n_g < (1ll << 31) && ldq >= d && ldg >= d,
                 "%s: bad shape", name);
    CMVE_REQUIRE(l1f_dtype_ok(q_dtype) && l1f_dtype_ok(g_dtype), "%s: rows must be CMVE_F32/CMVE_F64", name);
    CMVE_REQUIRE(grid && ((q_codes && q_err) || !n_q) && ((g_codes && g_err) || !n_g),
                 "%s: the codes, the row errors or the grid are missing (cmve_l1_grid, cmve_l1_pack)", name);
    CMVE_REQUIRE(((((uintptr_t)q_codes) | ((uintptr_t)g_codes)) & 15) == 0, "%s: codes must be 16-byte aligned", name);
    return CMVE_OK;
  };
  auto pass_launch = [&](int mode, hipStream_t st, const L2tRound& r, const L2tWs& w) {
    int64_t n_pad = 0, d_pad = 0;
    l1f_pads(n_q, d, n_pad, d_pad);
    const L1tArgs a{(const uint32_t*)q_codes, (const uint32_t*)g_codes, q_err, g_err, grid, r.q0, r.q_end, r.ng,
                    (int)(d_pad / L1F_BK), alpha,
                    (1e300 - fabs(beta)) / fabs(alpha),  // lim: below it alpha * S + beta cannot overflow
                    w.ub, w.ub_ld, w.thr, w.cnt, w.list, w.cap, w.stats, r.tiles_a, r.tiles_b};
    hipLaunchKernelGGL(mode == 0 ? l1t_pass_kernel<0> : l1t_pass_kernel<1>, dim3((unsigned)(r.tiles_a * r.tiles_b)),
                       dim3(256), 0, st, a);
  };
  return l2t_topk_run<CMVE_PW_L1>(name, "l1_topk", h, FltRows{Q, q_dtype, ldq, n_q, G, g_dtype, ldg, n_g, d}, alpha,
                                  beta, k, cand_cap, sample_rows, ws, ws_bytes, out_idx, out_err, stats,
                                  2.0 * ((double)d + 16.0) * L2F_U,  // rho: DESIGN s4 (K22)
                                  own_checks, pass_launch);
}
