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
//   jacf_main_kernel     sad_count.h's kernel body -- l1f_main_kernel's tile, block order, two-pass epilogue and
//                        thread layout -- under the policy JacfCount: the interval is of two sums, the tests are
//                        products against thresholds moved to quotient space once per (item, round): no division
//                        per pair
#include "jaccard_filter_tile.h"
#include "sad_count.h"

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

// ---- the count: sad_count.h's kernel under the jaccard policy -----------------------------------------------------------
struct JacfCount {
  struct Args : SadArgs {
    const int64_t* a_qsum;  // exact code sums
    const int64_t* b_qsum;
    const double* a_asum;  // >= sum |x|
    const double* b_asum;
    double d;
  };
  static constexpr int NS = 2;  // a side carries jacf_side's p and w
  struct Iv {
    double ilo, ihi, ulo, uhi;
  };
  template <bool B>
  static __device__ __forceinline__ void side(const Args& a, bool v, int64_t i, double lo, double s,
                                              double (&t)[NS]) {
    jacf_side(v, v ? (B ? a.b_err : a.a_err)[i] : 0.0, v ? (B ? a.b_asum : a.a_asum)[i] : 0.0,
              v ? (double)(B ? a.b_qsum : a.a_qsum)[i] : 0.0, a.d, lo, s, t[0], t[1]);
  }
  // (the item's edge moves to quotient space: the only divisions of the epilogue)
  static __device__ __forceinline__ void thresholds(const Args& a, double w, double& tl, double& tu) {
    jacf_thresholds(w, a.alpha, a.beta, tl, tu);
  }
  static __device__ __forceinline__ Iv interval(const Args&, uint32_t sad, double s, const double (&xa)[NS],
                                                const double (&xb)[NS]) {
    Iv iv;
    jacf_interval(sad, s, xa[0], xa[1], xb[0], xb[1], iv.ilo, iv.ihi, iv.ulo, iv.uhi);
    return iv;
  }
  static __device__ __forceinline__ bool has(const Iv& iv) { return iv.ilo == iv.ilo; }
  // (both product tests are formed, then one is picked: a pair is decided by either, whatever alpha's sign)
  static __device__ __forceinline__ bool below(const Iv& iv, bool pos, double tl, double tu) {
    const bool lt = jacf_lt(iv.ihi, iv.ulo, iv.uhi, tl), gt = jacf_gt(iv.ilo, iv.ulo, iv.uhi, tu);
    return pos ? lt : gt;
  }
  static __device__ __forceinline__ bool not_below(const Iv& iv, bool pos, double tl, double tu) {
    const bool lt = jacf_lt(iv.ihi, iv.ulo, iv.uhi, tl), gt = jacf_gt(iv.ilo, iv.ulo, iv.uhi, tu);
    return pos ? gt : lt;
  }
};

__global__ __launch_bounds__(256, 4) void jacf_main_kernel(JacfCount::Args a) { sad_count_body<JacfCount>(a); }

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
  return sad_count_workspace("cmve_jaccard_count_workspace", band_cap, bytes);
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
  const FltRows rows{A, a_dtype, lda, na, B, b_dtype, ldb, nb, d};
  auto own_checks = [&]() -> int {
    return sad_checks(name, d, rows, a_codes, b_codes, grid, a_codes && a_err && a_qsum && a_asum,
                            b_codes && b_err && b_qsum && b_asum,
                            "the codes, the row errors, the row sums or the grid are missing (cmve_l1_grid, "
                            "cmve_l1_pack, cmve_jaccard_rowsums)");
  };
  auto main_launch = [&](hipStream_t st, const FltArgs& f) {
    const JacfCount::Args g{sad_count_args(f, a_codes, a_err, b_codes, b_err, grid, d), a_qsum, b_qsum, a_asum,
                            b_asum, (double)d};
    hipLaunchKernelGGL(jacf_main_kernel, dim3((unsigned)(f.tiles_a * f.tiles_b)), dim3(256), 0, st, g);
  };
  // (resolve: an overflowing list is resolved on the device, from the start -- no entry leaves it to the host)
  return flt_count_run(name, "jaccard_count", h, CMVE_PW_JACCARD, rows, alpha, beta,
                       {row_off, row_sc, row_items, row_n, row_pos, col_off, col_sc, col_items, col_n, col_pos}, ws,
                       ws_bytes, stats, true, own_checks, main_launch);
}
