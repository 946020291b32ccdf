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
// only.  This file holds what is this filter's alone: the policy of the pass kernel (L1tPass: its own argument, a
// side's row error, l1f_interval + l2t_pair as the pair step) and the entry.  The pass kernel's body, its argument
// prefix and the workspace entry are sad_topk.h's, shared with K25; the SAD tile and the entry's checks of its own
// operands l1_filter_tile.h's (l1f_sad_tile, sad_checks: shared with the count kernels); the tail of the epilogue,
// launches A' and C and the host body (l2t_topk_run: checks, workspace, the rounds of four launches)
// topk_filter_tile.h's, shared with K20.
#include "sad_topk.h"

namespace cmve {
namespace {

// sad_topk.h's pass kernel under the L1 policy: a side carries its row error, a pair's interval is l1f_interval's and
// its step l2t_pair's
struct L1tPass {
  struct Args : SadTopkArgs {
    double lim;  // below it alpha * S + beta cannot overflow
  };
  static constexpr int NS = 1;
  template <bool G>
  static __device__ __forceinline__ void side(const Args& a, bool v, int64_t i, double, double, double (&x)[NS]) {
    x[0] = v ? (G ? a.g_err : a.q_err)[i] : (double)NAN;  // a row beyond the pass: no interval (and never used)
  }
  static __device__ __forceinline__ double step(const double& s) { return s; }
  template <int MODE>
  static __device__ __forceinline__ void pair(const Args& a, bool pos, int64_t i, int64_t j, uint32_t sad, double s,
                                              const double (&eq)[NS], const double (&eg)[NS], double thr, bool full,
                                              int& n_cand, int& n_excl) {
    double dlo, dhi;
    l1f_interval(sad, s, eq[0], eg[0], a.lim, dlo, dhi);
    l2t_pair<MODE>(a, pos, i, j, dlo, dhi, thr, full, n_cand, n_excl);
  }
};

// MODE 0: launch A (the witnesses' bounds), MODE 1: launch B (the candidates)
template <int MODE>
__global__ __launch_bounds__(256, 4) void l1t_pass_kernel(L1tPass::Args a) {
  sad_topk_body<L1tPass, MODE>(a);
}

}  // namespace
}  // namespace cmve

using namespace cmve;

extern "C" int cmve_l1_topk_workspace(int64_t n_q, int64_t n_g, int32_t k, int64_t cand_cap, int64_t sample_rows,
                                      int64_t* bytes) {
  return sad_topk_workspace("cmve_l1_topk_workspace", n_q, n_g, k, cand_cap, sample_rows, bytes);
}

extern "C" int cmve_l1_topk(cmve_handle_t h, const void* Q, int32_t q_dtype, int64_t ldq, int64_t n_q,
                            const void* q_codes, const double* q_err, const void* G, int32_t g_dtype, int64_t ldg,
                            int64_t n_g, const void* g_codes, const double* g_err, int64_t d, const double* grid,
                            double alpha, double beta, int32_t k, int64_t cand_cap, int64_t sample_rows, void* ws,
                            int64_t ws_bytes, int64_t* out_idx, double* out_err, int64_t* stats) {
  const char* name = "cmve_l1_topk";
  CMVE_REQUIRE(h && stats && (Q || !n_q) && (G || !n_g), "%s: NULL argument", name);
  const FltRows rows{Q, q_dtype, ldq, n_q, G, g_dtype, ldg, n_g, d};
  auto own_checks = [&]() -> int {
    return sad_checks(name, d, rows, q_codes, g_codes, grid, q_codes && q_err, g_codes && g_err,
                      "the codes, the row errors or the grid are missing (cmve_l1_grid, cmve_l1_pack)");
  };
  auto pass_launch = [&](int mode, hipStream_t st, const L2tRound& r, const L2tWs& w) {
    const L1tPass::Args a{sad_topk_args(r, w, q_codes, q_err, g_codes, g_err, grid, n_q, d, alpha),
                          (1e300 - fabs(beta)) / fabs(alpha)};
    hipLaunchKernelGGL(mode == 0 ? l1t_pass_kernel<0> : l1t_pass_kernel<1>, dim3((unsigned)(r.tiles_a * r.tiles_b)),
                       dim3(256), 0, st, a);
  };
  return l2t_topk_run<CMVE_PW_L1>(name, "l1_topk", h, rows, alpha, beta, k, cand_cap, sample_rows, ws, ws_bytes,
                                  out_idx, out_err, stats,
                                  2.0 * ((double)d + 16.0) * L2F_U,  // rho: DESIGN s4 (K22)
                                  own_checks, pass_launch);
}
