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
// integer atomics only.  This file holds what is this filter's alone: the pass kernel's argument block, its sides and
// interval, its pair step, the threshold and the entry's checks of its own operands.  The SAD tile is
// l1_filter_tile.h's, the sides, the interval and the word-to-quotient map jaccard_filter_tile.h's (K24), the rest of
// the epilogue's tail, the select, launch C and the host body topk_filter_tile.h's.
#include "jaccard_filter_tile.h"
#include "topk_filter_tile.h"

namespace cmve {
namespace {

struct JactArgs {
  const uint32_t* q_codes;  // tiled (l1_filter_tile.h)
  const uint32_t* g_codes;
  const double* q_err;
  const double* g_err;
  const int64_t* q_qsum;  // exact code sums (cmve_jaccard_rowsums)
  const int64_t* g_qsum;
  const double* q_asum;  // >= sum |x|
  const double* g_asum;
  const double* grid;
  int64_t q0, q_end;  // this round's queries; q0 is a multiple of 128
  int64_t ng;         // columns of this pass: the sample (A) or the gallery (B)
  int nkt;            // K tiles
  double alpha, d;
  float* ub;          // A: [q_end - q0][ub_ld] upper key bounds
  int64_t ub_ld;
  const double* thr;  // B: per query the quotient-space threshold (NaN: unresolved, nothing is appended)
  int32_t* cnt;       // B: candidates found per query
  int32_t* list;      // B: [q_end - q0][cap] column ids
  int64_t cap;
  l2f_u64* stats;     // {pairs excluded, candidates found, candidates re-scored, unresolved queries}
  int tiles_a, tiles_b;
};

// the epilogue's LDS, laid over the staging buffers once the K loop is done
struct JactEpi {
  double qp[L1F_BM], qw[L1F_BM];  // jacf_side's p and w of the tile's rows ...
  double gp[L1F_BN], gw[L1F_BN];  // ... and columns
  double thr[L1F_BM];
  int full[L1F_BM];  // the row's list had overflowed when this tile began: its candidates are counted, not appended
  int n_cand, n_excl;
  double s;  // the grid's step
};
static_assert(sizeof(JactEpi) <= L1F_SMEM, "the epilogue's LDS fits the staging buffers");

// One pair (query i, column j) whose two canonical sums lie in [ilo, ihi] and [ulo, uhi], ulo > 0 (NaN, NaN for the
// first: no interval); pos: alpha > 0.  l2t_pair's sibling: the test is an interval of two sums against ONE quotient.
template <int MODE>
__device__ __forceinline__ void jact_pair(const JactArgs& a, bool pos, int64_t i, int64_t j, double ilo, double ihi,
                                          double ulo, double uhi, double thr, bool full, int& n_cand, int& n_excl) {
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

// MODE 0: launch A (the witnesses' bounds), MODE 1: launch B (the candidates)
template <int MODE>
__global__ __launch_bounds__(256, 4) void jact_pass_kernel(JactArgs a) {
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
  JactEpi& E = *(JactEpi*)smem;
  double lo, s;
  l1f_grid_of(a.grid, lo, s);
  if (tid < L1F_BM) {
    const int64_t i = i0 + tid;
    const bool v = i < a.q_end;  // a row beyond the round: no interval (and never used)
    jacf_side(v, v ? a.q_err[i] : 0.0, v ? a.q_asum[i] : 0.0, v ? (double)a.q_qsum[i] : 0.0, a.d, lo, s, E.qp[tid],
              E.qw[tid]);
    l2t_row_state<MODE>(a, E, tid, i, v);
  } else {
    const int t = tid - L1F_BM;
    const int64_t j = j0 + t;
    const bool v = j < a.ng;
    jacf_side(v, v ? a.g_err[j] : 0.0, v ? a.g_asum[j] : 0.0, v ? (double)a.g_qsum[j] : 0.0, a.d, lo, s, E.gp[t],
              E.gw[t]);
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
    // a volatile read, as sad_count.h's: the intervals are formed eight at a time, not hoisted as live doubles
    const double sv = *(const volatile double*)&E.s;
    const double qp = E.qp[row], qw = E.qw[row];
    const double thr = MODE == 1 ? E.thr[row] : 0.0;
    const bool full = MODE == 1 ? E.full[row] != 0 : false;
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      const int col = l1f_row(tx, v);
      const int64_t j = j0 + col;
      if (i >= a.q_end || j >= a.ng) continue;
      double ilo, ihi, ulo, uhi;
      jacf_interval(acc[u][v], sv, qp, qw, E.gp[col], E.gw[col], ilo, ihi, ulo, uhi);
      jact_pair<MODE>(a, pos, i, j, ilo, ihi, ulo, uhi, thr, full, n_cand, n_excl);
    }
  }
  l2t_flush<MODE>(a, E, tid, n_cand, n_excl);
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
  CMVE_REQUIRE(bytes, "cmve_jaccard_topk_workspace: NULL argument");
  if (int rc = l2t_check_params("cmve_jaccard_topk_workspace", k, cand_cap, sample_rows)) return rc;
  CMVE_REQUIRE(n_q >= 0 && n_g >= 0 && n_q < (1ll << 31) && n_g < (1ll << 31),
               "cmve_jaccard_topk_workspace: bad shape (%lld, %lld rows)", (long long)n_q, (long long)n_g);
  *bytes = l2t_layout(n_q, n_g, k, cand_cap, sample_rows).bytes;
  return CMVE_OK;
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
  auto own_checks = [&]() -> int {
    CMVE_REQUIRE(d > 0 && d <= L1F_D_MAX, "%s: d must be in [1, %lld] (%lld): the u32 SAD is exact up to there", name,
                 (long long)L1F_D_MAX, (long long)d);
    CMVE_REQUIRE(n_q >= 0 && n_g >= 0 && n_q < (1ll << 31) && n_g < (1ll << 31) && ldq >= d && ldg >= d,
                 "%s: bad shape", name);
    CMVE_REQUIRE(l1f_dtype_ok(q_dtype) && l1f_dtype_ok(g_dtype), "%s: rows must be CMVE_F32/CMVE_F64", name);
    CMVE_REQUIRE(grid && ((q_codes && q_err && q_qsum && q_asum) || !n_q) &&
                     ((g_codes && g_err && g_qsum && g_asum) || !n_g),
                 "%s: the codes, the row errors, the row sums or the grid are missing (cmve_l1_grid, cmve_l1_pack, "
                 "cmve_jaccard_rowsums)", name);
    CMVE_REQUIRE(((((uintptr_t)q_codes) | ((uintptr_t)g_codes)) & 15) == 0, "%s: codes must be 16-byte aligned", name);
    return CMVE_OK;
  };
  auto pass_launch = [&](int mode, hipStream_t st, const L2tRound& r, const L2tWs& w) {
    int64_t n_pad = 0, d_pad = 0;
    l1f_pads(n_q, d, n_pad, d_pad);
    const JactArgs a{(const uint32_t*)q_codes, (const uint32_t*)g_codes, q_err, g_err, q_qsum, g_qsum, q_asum, g_asum,
                     grid, r.q0, r.q_end, r.ng, (int)(d_pad / L1F_BK), alpha, (double)d, w.ub, w.ub_ld, w.thr, w.cnt,
                     w.list, w.cap, w.stats, r.tiles_a, r.tiles_b};
    hipLaunchKernelGGL(mode == 0 ? jact_pass_kernel<0> : jact_pass_kernel<1>, dim3((unsigned)(r.tiles_a * r.tiles_b)),
                       dim3(256), 0, st, a);
  };
  auto thr_launch = [&](hipStream_t st, int64_t nq, int64_t ns, const L2tWs& w) {
    hipLaunchKernelGGL(jact_threshold_kernel, dim3((unsigned)nq), dim3(256), 0, st, (const float*)w.ub, w.ub_ld, ns,
                       (int)k, alpha, beta, w.thr, w.cnt);
  };
  return l2t_topk_run<CMVE_PW_JACCARD>(name, "jaccard_topk", h, FltRows{Q, q_dtype, ldq, n_q, G, g_dtype, ldg, n_g, d},
                                       alpha, beta, k, cand_cap, sample_rows, ws, ws_bytes, out_idx, out_err, stats,
                                       own_checks, pass_launch, thr_launch);
}
