// K20: cmve_pairwise_topk under the Euclidean measures (euclidean / l2 / l2_norm: CMVE_PW_L2, fp64 score words) at
// the MFMA rate -- what
//   LINAS-engine/inference.py:78-80      cal_error(video_embs, cap_emb, measure) -> np.argsort(errors[0])[:topK]
//   LINAS-engine/evaluation.py:22-35     cal_error under euclidean / l2 / l2_norm
// compute per caption.  The k smallest errors are the k smallest keys  s D,  s = sign(alpha), D the true squared
// distance of the pair; K19's fp16 MFMA cosine (l2_filter_tile.h) brackets every pair's key, so
//   launch A   l2t_pass_kernel<0>     the MFMA pass over the first `sample_rows` gallery rows; the epilogue stores every
//                                     pair's UPPER key bound (fp32, rounded up; +inf for a pair without an interval)
//   launch A'  l2t_threshold_kernel   per query the k-th smallest stored bound tau (radix select: k distinct columns --
//                                     the witnesses -- have a true key <= tau), widened to a squared-distance threshold
//                                     beyond which a column's canonical word is STRICTLY worse than every witness's
//                                     (DESIGN s4, "K20"); a query without k finite bounds is unresolved
//   launch B   l2t_pass_kernel<1>     the same pass over the whole gallery; a pair without an interval, or whose lower
//                                     key bound does not clear the threshold, is appended to its query's candidate
//                                     list (integer atomic counter; the order of a list does not matter)
//   launch C   l2t_finish_kernel      a block per query: every candidate re-scored on the canonical chain of
//                                     pairwise_tile.h (l2f_chain64, as K19's fix-up), sorted in LDS by (word asc with
//                                     NaN last, -0 == +0, id asc), the first k emitted
// so out_idx / out_err are, word for word, cmve_pairwise_topk's.  A query whose list overflows, or that has no
// threshold, gets out_idx[i, 0] = -2: the caller finishes it on the fp64 route.  Plain vector stores and integer
// atomics only; the queries are taken L2T_QC at a time so that the workspace has no n_q x n_g term.
// This file holds what is this filter's alone: the pass kernel's argument block, its interval and thread layout, and
// the entry's checks of its own operands.  The tail of the epilogue, launches A' and C, the sample, the layout, the
// parameter checks and the host body (l2t_topk_run: checks, workspace, the rounds of four launches) are
// topk_filter_tile.h's, shared with K23 (l1_topk.hip).
#include "topk_filter_tile.h"

namespace cmve {
namespace {

struct L2tArgs {
  const uint16_t* q16;  // [nq_pad, d_pad] fp16 unit rows
  const uint16_t* g16;
  const double* q_inv;  // 1 / ||row||
  const double* g_inv;
  const float* q_err;   // >= || x_hat - h16 ||
  const float* g_err;
  int64_t q0, q_end;    // this round's queries
  int64_t ng;           // columns of this pass: the sample (A) or the gallery (B)
  int64_t d_pad;
  double alpha;
  L2fConsts c;
  float* ub;            // A: [q_end - q0][ub_ld] upper key bounds
  int64_t ub_ld;
  const double* thr;    // B: per query the squared-distance threshold (NaN: unresolved, nothing is appended)
  int32_t* cnt;         // B: candidates found per query
  int32_t* list;        // B: [q_end - q0][cap] column ids
  int64_t cap;
  l2f_u64* stats;       // {pairs excluded, candidates found, candidates re-scored, unresolved queries}
  int tiles_a, tiles_b;
};

// the epilogue's LDS, laid over the staging buffers once the K loop is done
struct L2tEpi {
  double qn[L2F_BM], qe[L2F_BM], gn[L2F_BN], ge[L2F_BN];  // norms and row errors of the tile's rows / columns
  double thr[L2F_BM];
  int full[L2F_BM];  // the row's list had overflowed when this tile began: its candidates are counted, not appended
  int n_cand, n_excl;
};
static_assert(sizeof(L2tEpi) <= L2F_SMEM, "the epilogue's LDS fits the staging buffers");

// MODE 0: launch A (the witnesses' bounds), MODE 1: launch B (the candidates)
template <int MODE>
__global__ __launch_bounds__(256, 2) void l2t_pass_kernel(L2tArgs a) {
  __shared__ __attribute__((aligned(16))) char smem[L2F_SMEM];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, fr = lane & 15, fq = lane >> 4;
  int ta, tb_;
  l2f_tile_of_block(blockIdx.x, a.tiles_a, a.tiles_b, ta, tb_);
  // q0 is a multiple of 128 and both planes hold n_pad (a multiple of 256) rows: the tile's 128 rows are in bounds
  const int64_t i0 = a.q0 + (int64_t)ta * L2F_BM, j0 = (int64_t)tb_ * L2F_BN;
  l2f_f32x4 acc[4][4];
  l2f_gemm_tile(a.q16, a.g16, a.d_pad, i0, j0, smem, acc);

  L2tEpi& E = *(L2tEpi*)smem;
  if (tid < L2F_BM) {
    const int64_t i = i0 + tid;
    const bool v = i < a.q_end;
    E.qn[tid] = l2f_side_norm(i, v, a.q_inv);
    E.qe[tid] = l2f_side_err(i, v, a.q_err, a.c.theta);
    l2t_row_state<MODE>(a, E, tid, i, v);
  } else {
    const int t = tid - L2F_BM;
    const int64_t j = j0 + t;
    const bool v = j < a.ng;
    E.gn[t] = l2f_side_norm(j, v, a.g_inv);
    E.ge[t] = l2f_side_err(j, v, a.g_err, a.c.theta);
  }
  if (tid == 0) E.n_cand = E.n_excl = 0;
  __syncthreads();
  const bool pos = a.alpha > 0.0;
  const int rbase = wm * 64 + 4 * fq, cbase = wn * 64 + fr;
  int n_cand = 0, n_excl = 0;
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = rbase + 16 * m + r;
      const int64_t i = i0 + row;
      const double qn = E.qn[row], qe = E.qe[row];
      const double thr = MODE == 1 ? E.thr[row] : 0.0;
      const bool full = MODE == 1 ? E.full[row] != 0 : false;
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        const int col = cbase + 16 * n;
        const int64_t j = j0 + col;
        if (i >= a.q_end || j >= a.ng) continue;
        double dlo, dhi;
        l2f_interval(acc[m][n][r], qn, qe, E.gn[col], E.ge[col], a.c.gamma, a.c.kappa, dlo, dhi);
        l2t_pair<MODE>(a, pos, i, j, dlo, dhi, thr, full, n_cand, n_excl);
      }
    }
  l2t_flush<MODE>(a, E, tid, n_cand, n_excl);
}

}  // namespace
}  // namespace cmve

using namespace cmve;

extern "C" int cmve_l2_topk_workspace(const cmve_rows_t* q, const cmve_rows_t* g, int32_t k, int64_t cand_cap,
                                      int64_t sample_rows, int64_t* bytes) {
  CMVE_REQUIRE(q && g && bytes, "cmve_l2_topk_workspace: NULL argument");
  if (int rc = l2t_check_params("cmve_l2_topk_workspace", k, cand_cap, sample_rows)) return rc;
  CMVE_REQUIRE(q->n >= 0 && g->n >= 0 && q->n < (1ll << 31) && g->n < (1ll << 31) && q->d > 0 && q->d == g->d,
               "cmve_l2_topk_workspace: bad shape (%lld x %lld, %lld x %lld)", (long long)q->n, (long long)q->d,
               (long long)g->n, (long long)g->d);
  *bytes = l2t_layout(q->n, g->n, k, cand_cap, sample_rows).bytes;
  return CMVE_OK;
}

extern "C" int cmve_l2_topk(cmve_handle_t h, const cmve_rows_t* q, const cmve_rows_t* g, double alpha, double beta,
                            int32_t k, int64_t cand_cap, int64_t sample_rows, void* ws, int64_t ws_bytes,
                            int64_t* out_idx, double* out_err, int64_t* stats) {
  const char* name = "cmve_l2_topk";
  CMVE_REQUIRE(h && q && g && stats, "%s: NULL argument", name);
  const L2fConsts c = l2f_consts(q->d, q->d_pad);
  auto own_checks = [&]() -> int { return l2f_check_sets(name, q, g); };
  auto pass_launch = [&](int mode, hipStream_t st, const L2tRound& r, const L2tWs& w) {
    const L2tArgs a{q->h16, g->h16, q->inv_norm, g->inv_norm, q->err_h16, g->err_h16, r.q0, r.q_end, r.ng, q->d_pad,
                    alpha, c, w.ub, w.ub_ld, w.thr, w.cnt, w.list, w.cap, w.stats, r.tiles_a, r.tiles_b};
    hipLaunchKernelGGL(mode == 0 ? l2t_pass_kernel<0> : l2t_pass_kernel<1>, dim3((unsigned)(r.tiles_a * r.tiles_b)),
                       dim3(256), 0, st, a);
  };
  return l2t_topk_run<CMVE_PW_L2>(name, "l2_topk", h, FltRows{q->raw, q->raw_dtype, q->raw_ld, q->n, g->raw,
                                                                g->raw_dtype, g->raw_ld, g->n, q->d},
                                  alpha, beta, k, cand_cap, sample_rows, ws, ws_bytes, out_idx, out_err, stats, c.rho,
                                  own_checks, pass_launch);
}
