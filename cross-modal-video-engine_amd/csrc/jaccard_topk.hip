// K25: cmve_pairwise_topk under jaccard (CMVE_PW_JACCARD, float32 score words) at the integer SAD rate -- what
//   LINAS-engine/inference.py:78-80      cal_error(video_embs, cap_emb, 'jaccard') -> np.argsort(errors[0])[:topK]
//   LINAS-engine/evaluation.py:32-35     cal_error under jaccard
// compute per caption.  The k smallest errors are the k smallest keys  s q,  s = sign(alpha), q = I_c / U_c the real
// quotient of the pair's two canonical sums; K24's interval of the two sums (jaccard_filter_tile.h) brackets every
// pair's q, so K23's scheme (l1_topk.hip, topk_filter_tile.h) carries over launch by launch:
//   launch A   jact_pass_kernel<0>       the SAD tile over the first `sample_rows` gallery rows; the epilogue stores
//                                        every pair's UPPER key bound: the far end of the quotient interval, widened
//                                        past the division's rounding (fp32, rounded up; +inf without an interval).
//                                        The one division per pair of this file: the sample is a small part of the
//                                        gallery
//   launch A'  jact_threshold_kernel     the k-th smallest stored bound per query (l2t_kth_bound), moved to ONE
//                                        quotient-space threshold that is strict on the float32 WORDS (jact_widen:
//                                        the condition is checked on the device, DESIGN s4 "K25")
//   launch B   jact_pass_kernel<1>       the same tile over the whole gallery; a pair is excluded only when its whole
//                                        interval lies beyond the threshold (jacf_gt / jacf_lt: one select and one fp64
//                                        product, no division); a pair without an interval, or one that does not clear
//                                        it, is appended to its query's candidate list (integer atomic counter)
//   launch C   l2t_finish_kernel<CMVE_PW_JACCARD>  a block per query: the candidates on the canonical two-accumulator
//                                        chain with its one rounding to float32, sorted, k emitted
// so out_idx / out_err are, word for word, cmve_pairwise_topk's with score_dtype = CMVE_F32.  Plain vector stores and
// integer atomics only.  This file holds what is this filter's alone: the policy of the pass kernel (JactPass: its own
// arguments, a side's two terms, the re-read of the step, the pair step), the threshold and the entry.  The pass
// kernel's body, its argument prefix and the workspace entry are sad_topk.h's, shared with K23; the SAD tile and the
// entry's checks of its own operands l1_filter_tile.h's, the sides, the interval and the word-to-quotient map
// jaccard_filter_tile.h's (K24), the rest of the epilogue's tail, the select, launch C and the host body
// topk_filter_tile.h's.
#include "jaccard_filter_tile.h"
#include "sad_topk.h"

namespace cmve {
namespace {

// sad_topk.h's pass kernel under the jaccard policy: a side carries jacf_side's p and w, a pair's interval is
// jacf_interval's -- two sums, [ilo, ihi] and [ulo, uhi], ulo > 0 (NaN, NaN for the first: no interval) -- and its step
// l2t_pair's sibling: the test is an interval of two sums against ONE quotient
struct JactPass {
  struct Args : SadTopkArgs {
    const int64_t* q_qsum;  // exact code sums (cmve_jaccard_rowsums)
    const int64_t* g_qsum;
    const double* q_asum;  // >= sum |x|
    const double* g_asum;
    double d;
  };
  static constexpr int NS = 2;
  template <bool G>
  static __device__ __forceinline__ void side(const Args& a, bool v, int64_t i, double lo, double s, double (&x)[NS]) {
    jacf_side(v, v ? (G ? a.g_err : a.q_err)[i] : 0.0, v ? (G ? a.g_asum : a.q_asum)[i] : 0.0,
              v ? (double)(G ? a.g_qsum : a.q_qsum)[i] : 0.0, a.d, lo, s, x[0], x[1]);
  }
  // a volatile read, as sad_count.h's: the intervals are formed eight at a time, not hoisted as live doubles
  static __device__ __forceinline__ double step(const double& s) { return *(const volatile double*)&s; }
  template <int MODE>
  static __device__ __forceinline__ void pair(const Args& a, bool pos, int64_t i, int64_t j, uint32_t sad, double s,
                                              const double (&xq)[NS], const double (&xg)[NS], double thr, bool full,
                                              int& n_cand, int& n_excl) {
    double ilo, ihi, ulo, uhi;
    jacf_interval(sad, s, xq[0], xq[1], xg[0], xg[1], ilo, ihi, ulo, uhi);
    if (MODE == 0) {
      // key = s q: its upper bound is the far end of the quotient interval, q_hi (alpha > 0) or -q_lo (alpha < 0),
      // moved outward past the division's rounding and underflow; NaN (no interval) becomes +inf
      const double num = pos ? ihi : ilo;
      const double den = (num >= 0.0) == pos ? ulo : uhi;
      const double e = num / den;
      const double w = (8.0 * L2F_U) * fabs(e) + 1e-300;
      a.ub[(i - a.q0) * a.ub_ld + j] = l2t_f32_up(pos ? e + w : -(e - w));
    } else if (thr == thr) {
      // excluded only on a positive test: every quotient of the interval is provably beyond the threshold (a NaN
      // interval fails it)
      l2t_decide(a, pos ? jacf_gt(ilo, ulo, uhi, thr) : jacf_lt(ihi, ulo, uhi, thr), i, j, full, n_cand, n_excl);
    }
  }
};

// MODE 0: launch A (the witnesses' bounds), MODE 1: launch B (the candidates)
template <int MODE>
__global__ __launch_bounds__(256, 4) void jact_pass_kernel(JactPass::Args a) {
  sad_topk_body<JactPass, MODE>(a);
}

// the float32 after f (finite); +0 and -0 step to the least subnormal
__device__ __forceinline__ float jact_next32(float f) {
  const uint32_t b = __float_as_uint(f);
  return f == 0.f ? __uint_as_float(1u) : __uint_as_float(f > 0.f ? b + 1u : b - 1u);
}

// The witnesses' bound tau (key space: k distinct columns have s q <= tau) -> the ONE quotient-space threshold of
// launch B, or NaN when there is none.  DESIGN s4 "K25".  q_tau = s tau: every witness has q <= q_tau (alpha > 0) or
// q >= q_tau (alpha < 0).  Guess the float32 word t = fl32(alpha q_tau + beta), let t' be the next float32 and
// (T_l, T_u) = jacf_thresholds(t').  alpha > 0: if q_tau < T_l every witness's word is < t', i.e. <= t (K24 step 4),
// and a column whose quotient is provably above T_u has a word >= t' > t: strictly worse than k columns' words, so
// outside the top-k whatever its index.  alpha < 0 mirrors: q_tau > T_u puts the witnesses' words below t', a column
// with q < T_l has a word >= t'.  The condition is CHECKED here: the guess is not part of the proof; where it fails t
// moves one float32 up, at most 12 times.  No threshold: tau, t or t' not finite, or jacf_thresholds decides nothing.
__device__ double jact_widen(double tau, double alpha, double beta) {
  const bool pos = alpha > 0.0;
  const double inf = __builtin_huge_val();
  if (!(fabs(tau) < inf)) return (double)NAN;
  const double q_tau = pos ? tau : -tau;
  float t = (float)(alpha * q_tau + beta);
  for (int it = 0; it < 12; ++it) {
    if (!(fabsf(t) < __builtin_huge_valf())) return (double)NAN;
    const float tn = jact_next32(t);
    if (!(fabsf(tn) < __builtin_huge_valf())) return (double)NAN;
    double tl, tu;
    jacf_thresholds((double)tn, alpha, beta, tl, tu);
    if (!(tl == tl)) return (double)NAN;
    if (pos ? q_tau < tl : q_tau > tu) return pos ? tu : tl;
    t = tn;
  }
  return (double)NAN;
}

// launch A': one block per query; the query's candidate counter starts at zero here
__global__ __launch_bounds__(256) void jact_threshold_kernel(const float* __restrict__ ub, int64_t ub_ld, int64_t ns,
                                                             int k, double alpha, double beta,
                                                             double* __restrict__ thr, int32_t* __restrict__ cnt) {
  const float tau = l2t_kth_bound(ub + (int64_t)blockIdx.x * ub_ld, ns, k);
  if (threadIdx.x == 0) {
    thr[blockIdx.x] = jact_widen((double)tau, alpha, beta);
    cnt[blockIdx.x] = 0;
  }
}

}  // namespace
}  // namespace cmve

using namespace cmve;

extern "C" int cmve_jaccard_topk_workspace(int64_t n_q, int64_t n_g, int32_t k, int64_t cand_cap,
                                           int64_t sample_rows, int64_t* bytes) {
  return sad_topk_workspace("cmve_jaccard_topk_workspace", n_q, n_g, k, cand_cap, sample_rows, bytes);
}

extern "C" int cmve_jaccard_topk(cmve_handle_t h, const void* Q, int32_t q_dtype, int64_t ldq, int64_t n_q,
                                 const void* q_codes, const double* q_err, const int64_t* q_qsum,
                                 const double* q_asum, const void* G, int32_t g_dtype, int64_t ldg, int64_t n_g,
                                 const void* g_codes, const double* g_err, const int64_t* g_qsum,
                                 const double* g_asum, int64_t d, const double* grid, double alpha, double beta,
                                 int32_t k, int64_t cand_cap, int64_t sample_rows, void* ws, int64_t ws_bytes,
                                 int64_t* out_idx, double* out_err, int64_t* stats) {
  const char* name = "cmve_jaccard_topk";
  CMVE_REQUIRE(h && stats && (Q || !n_q) && (G || !n_g), "%s: NULL argument", name);
  const FltRows rows{Q, q_dtype, ldq, n_q, G, g_dtype, ldg, n_g, d};
  auto own_checks = [&]() -> int {
    return sad_checks(name, d, rows, q_codes, g_codes, grid, q_codes && q_err && q_qsum && q_asum,
                      g_codes && g_err && g_qsum && g_asum,
                      "the codes, the row errors, the row sums or the grid are missing (cmve_l1_grid, cmve_l1_pack, "
                      "cmve_jaccard_rowsums)");
  };
  auto pass_launch = [&](int mode, hipStream_t st, const L2tRound& r, const L2tWs& w) {
    const JactPass::Args a{sad_topk_args(r, w, q_codes, q_err, g_codes, g_err, grid, n_q, d, alpha), q_qsum, g_qsum,
                           q_asum, g_asum, (double)d};
    hipLaunchKernelGGL(mode == 0 ? jact_pass_kernel<0> : jact_pass_kernel<1>, dim3((unsigned)(r.tiles_a * r.tiles_b)),
                       dim3(256), 0, st, a);
  };
  auto thr_launch = [&](hipStream_t st, int64_t nq, int64_t ns, const L2tWs& w) {
    hipLaunchKernelGGL(jact_threshold_kernel, dim3((unsigned)nq), dim3(256), 0, st, (const float*)w.ub, w.ub_ld, ns,
                       (int)k, alpha, beta, w.thr, w.cnt);
  };
  return l2t_topk_run<CMVE_PW_JACCARD>(name, "jaccard_topk", h, rows, alpha, beta, k, cand_cap, sample_rows, ws, ws_bytes,
                                       out_idx, out_err, stats, own_checks, pass_launch, thr_launch);
}
