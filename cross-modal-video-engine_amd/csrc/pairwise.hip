// K10: all-pairs non-cosine measures -- the non-GEMM similarity matrices of
//   LINAS-engine/evaluation.py:17-35,41-72   cal_error / cal_error_batch: scipy cdist 'euclidean',
//                                            'minkowski' p=1, their /D - 1 normalised forms, and
//                                            -jaccard (torch fp32)
//   LINAS-engine/loss.py:13-73               order / euclidean / L1 / L1_norm / L2 / L2_norm /
//                                            jaccard training similarities
//                                            (their backward under TripletLoss: K17, pairwise_bwd.hip)
// out[i, j] = alpha * f(a_i, b_j) + beta with
//   SQ_L2   f = sum_k (a_k - b_k)^2              L2   f = sqrt(SQ_L2)
//   L1      f = sum_k |a_k - b_k|                ORDER f = sqrt(sum_k max(0, b_k - a_k)^2)
//   JACCARD f = sum_k min(a_k, b_k) / sum_k max(a_k, b_k)
//   DOT     f = sum_k a_k b_k (k-ordered fp64 fma chain: the top-k's exact dense fallback)
// No MFMA form exists for these reductions (min/max/abs per element): a VALU kernel with 64x128
// output tiles per 256-thread block, 4x8 outputs per thread, K staged through LDS in 32-deep
// slabs (converted to fp64 once on the way in), fp64 accumulation -- the reference's scipy path
// is fp64 (encode_* buffers are fp64, evaluation.py:102); its torch paths are fp32 and agree to
// fp32 rounding.
#include "pairwise_tile.h"

namespace cmve {

// Block tile 64 (A rows) x 128 (B rows), 256 threads as 16 x 16 (PwWide, pairwise_tile.h): thread (tx, ty) owns
// A rows {2ty + 32u + e} and B rows {2tx + 32v + e} (u < 2, v < 4, e < 2): 4 x 8 = 32 outputs.  The stage-and-
// accumulate loop and the finalisation are the shared chain of pairwise_tile.h (K18 runs the same one).
template <typename TA, typename TB, typename TO, int METRIC>
__global__ __launch_bounds__(256) void pairwise_kernel(const TA* __restrict__ A, int64_t lda, int64_t na,
                                                       const TB* __restrict__ B, int64_t ldb, int64_t nb, int64_t d,
                                                       double alpha, double beta, TO* __restrict__ out,
                                                       int64_t ldo) {
  __shared__ __attribute__((aligned(16))) double sa[PW_K][PwWide::PA];  // [k][row], converted to fp64 once
  __shared__ __attribute__((aligned(16))) double sb[PW_K][PwWide::PB];
  constexpr bool JAC = METRIC == CMVE_PW_JACCARD;
  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;
  const int64_t i0 = (int64_t)blockIdx.y * PW_TA, j0 = (int64_t)blockIdx.x * PW_TB;
  double s0[4][8] = {}, s1[JAC ? 4 : 1][JAC ? 8 : 1] = {};
  pw_tile_loop<PwWide, METRIC>(A, lda, na, B, ldb, nb, d, i0, j0, sa, sb, s0, s1);
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t i = i0 + 2 * ty + 32 * (u >> 1) + (u & 1);
    if (i >= na) continue;
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      const int64_t j = j0 + 2 * tx + 32 * (v >> 1) + (v & 1);
      if (j < nb)
        out[i * ldo + j] = (TO)pw_score<METRIC>(s0[u][v], JAC ? s1[JAC ? u : 0][JAC ? v : 0] : 0.0, alpha, beta);
    }
  }
}

}  // namespace cmve

using namespace cmve;

extern "C" int cmve_pairwise(cmve_handle_t h, const void* A, int32_t a_dtype, int64_t lda, int64_t na, const void* B,
                             int32_t b_dtype, int64_t ldb, int64_t nb, int64_t d, int32_t metric, double alpha,
                             double beta, void* out, int32_t out_dtype, int64_t ldo) {
  CMVE_REQUIRE(h && A && B && out, "cmve_pairwise: NULL argument");
  CMVE_REQUIRE(na >= 0 && nb >= 0 && d > 0 && lda >= d && ldb >= d && ldo >= nb, "cmve_pairwise: bad shape");
  CMVE_REQUIRE(metric >= CMVE_PW_SQ_L2 && metric <= CMVE_PW_DOT, "cmve_pairwise: unknown metric %d", metric);
  CMVE_REQUIRE((a_dtype == CMVE_F32 || a_dtype == CMVE_F64) && (b_dtype == CMVE_F32 || b_dtype == CMVE_F64) &&
                   (out_dtype == CMVE_F32 || out_dtype == CMVE_F64),
               "cmve_pairwise: dtypes must be CMVE_F32/CMVE_F64");
  if (na == 0 || nb == 0) return CMVE_OK;
  CMVE_REQUIRE((na + PW_TA - 1) / PW_TA < 65536, "cmve_pairwise: too many rows in A (%lld)", (long long)na);
  const dim3 grid((unsigned)((nb + PW_TB - 1) / PW_TB), (unsigned)((na + PW_TA - 1) / PW_TA));
#define PW_LAUNCH(TO)                                                                                       \
  hipLaunchKernelGGL((pairwise_kernel<TA, TB, TO, M>), grid, dim3(256), 0, h->stream, (const TA*)A, lda, na, \
                     (const TB*)B, ldb, nb, d, alpha, beta, (TO*)out, ldo)
  PW_DISPATCH_METRIC(metric, M, PWR_TYPES(a_dtype, b_dtype, TA, TB, {
    if (out_dtype == CMVE_F64) PW_LAUNCH(double);
    else PW_LAUNCH(float);
  }))
#undef PW_LAUNCH
  return check_launch("pairwise");
}
