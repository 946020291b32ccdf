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
// Launches A' and C, the sample, the layout and the parameter checks are topk_filter_tile.h's, shared with K23
// (l1_topk.hip).
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
    if (MODE == 1) {
      E.thr[tid] = v ? a.thr[i - a.q0] : (double)NAN;
      // An overflowed list is lost (launch C asks only whether the counter exceeds cap), so its row stops appending:
      // rows clustered far from the origin -- every pair a candidate -- would otherwise serialise n_g atomics on
      // one address per query.  Read once per tile, off the pairs' path; the counter only grows, so a tile that
      // reads it early merely adds its own <= 128 candidates more.
      E.full[tid] = v ? __hip_atomic_load(a.cnt + (i - a.q0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > a.cap : 1;
    }
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
        if (MODE == 0) {
          // key = s D: its upper bound is dhi (alpha > 0) or -dlo (alpha < 0); NaN (no interval) becomes +inf
          a.ub[(i - a.q0) * a.ub_ld + j] = l2t_f32_up(pos ? dhi : -dlo);
        } else if (thr == thr) {
          // excluded only on a positive test: D is provably beyond the threshold (a NaN interval fails it)
          const bool out = pos ? dlo > thr : dhi < thr;
          if (out) {
            ++n_excl;
          } else {
            ++n_cand;
            if (!full) {
              const int64_t li = i - a.q0;
              const int32_t p = gadd(a.cnt + li, (int32_t)1);
              if (p < a.cap) a.list[li * a.cap + p] = (int32_t)j;
            }
          }
        }
      }
    }
  if (MODE == 1) {
    if (n_cand) atomicAdd(&E.n_cand, n_cand);
    if (n_excl) atomicAdd(&E.n_excl, n_excl);
    __syncthreads();
    if (tid == 0) {
      if (E.n_excl) gadd(a.stats + 0, (l2f_u64)E.n_excl);
      if (E.n_cand) gadd(a.stats + 1, (l2f_u64)E.n_cand);
    }
  }
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
  CMVE_REQUIRE(h && q && g && stats, "cmve_l2_topk: NULL argument");
  CMVE_REQUIRE(alpha != 0.0 && std::isfinite(alpha) && std::isfinite(beta),
               "cmve_l2_topk: alpha must be finite and non-zero, beta finite (%g, %g)", alpha, beta);
  if (int rc = l2t_check_params("cmve_l2_topk", k, cand_cap, sample_rows)) return rc;
  if (int rc = l2f_check_sets("cmve_l2_topk", q, g)) return rc;
  const int64_t n_q = q->n, n_g = g->n, d = q->d;
  CMVE_REQUIRE(k <= n_g || n_q == 0, "cmve_l2_topk: k exceeds the gallery (%d > %lld): clamp it", k, (long long)n_g);
  CMVE_REQUIRE((out_idx && out_err) || !n_q, "cmve_l2_topk: NULL output");
  const L2tLayout l = l2t_layout(n_q, n_g, k, cand_cap, sample_rows);
  CMVE_REQUIRE(n_q == 0 || (ws && ws_bytes >= l.bytes), "cmve_l2_topk: workspace too small (%lld < %lld bytes)",
               (long long)ws_bytes, (long long)l.bytes);
  CMVE_REQUIRE((((uintptr_t)ws) & 7) == 0, "cmve_l2_topk: workspace must be 8-byte aligned");
  const hipStream_t st = h->stream;
  CMVE_HIP(hipMemsetAsync(stats, 0, 4 * sizeof(int64_t), st));
  if (n_q == 0) return CMVE_OK;
  L2tArgs a;
  a.q16 = q->h16;
  a.g16 = g->h16;
  a.q_inv = q->inv_norm;
  a.g_inv = g->inv_norm;
  a.q_err = q->err_h16;
  a.g_err = g->err_h16;
  a.d_pad = q->d_pad;
  a.alpha = alpha;
  a.c = l2f_consts(d, q->d_pad);
  a.ub = (float*)((char*)ws + l.ub);
  a.ub_ld = l.ub_ld;
  double* thr = (double*)((char*)ws + l.thr);
  a.thr = thr;
  a.cnt = (int32_t*)((char*)ws + l.cnt);
  a.list = (int32_t*)((char*)ws + l.list);
  a.cap = cand_cap;
  a.stats = (l2f_u64*)stats;
  const int64_t tiles_s = (l.s + L2F_BN - 1) / L2F_BN, tiles_g = (n_g + L2F_BN - 1) / L2F_BN;
  for (int64_t q0 = 0; q0 < n_q; q0 += l.qc) {
    const int64_t nq = std::min(l.qc, n_q - q0);
    a.q0 = q0;
    a.q_end = q0 + nq;
    a.tiles_a = (int)((nq + L2F_BM - 1) / L2F_BM);  // <= 8: tiles_a * tiles_g < 2^31
    a.ng = l.s;
    a.tiles_b = (int)tiles_s;
    hipLaunchKernelGGL(l2t_pass_kernel<0>, dim3((unsigned)(a.tiles_a * tiles_s)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(l2t_threshold_kernel<true>, dim3((unsigned)nq), dim3(256), 0, st, (const float*)a.ub, a.ub_ld, l.s,
                       (int)k, alpha, beta, a.c.rho, thr, a.cnt);
    a.ng = n_g;
    a.tiles_b = (int)tiles_g;
    hipLaunchKernelGGL(l2t_pass_kernel<1>, dim3((unsigned)(a.tiles_a * tiles_g)), dim3(256), 0, st, a);
    PWR_TYPES(q->raw_dtype, g->raw_dtype, TA, TB, {
      hipLaunchKernelGGL((l2t_finish_kernel<CMVE_PW_L2, TA, TB>), dim3((unsigned)nq), dim3(256), 0, st, (const TA*)q->raw,
                         q->raw_ld, (const TB*)g->raw, g->raw_ld, d, alpha, beta, q0, (const double*)thr,
                         (const int32_t*)a.cnt, (const int32_t*)a.list, cand_cap, (int)k, out_idx, out_err, a.stats);
    })
    if (int rc = check_launch("l2_topk")) return rc;
  }
  return CMVE_OK;
}
