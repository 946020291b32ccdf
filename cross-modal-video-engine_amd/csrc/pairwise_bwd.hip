// K17: the backward of K10 (pairwise.hip) for the measures LINAS-engine/loss.py trains with
//   LINAS-engine/loss.py:13-73,93-108   order / euclidean / L1 / L1_norm / L2 / L2_norm / jaccard sims under
//                                       TripletLoss(measure=...), differentiated by torch autograd there
// score[i, j] = alpha * f(A_i, B_j) + beta, dS = dL/dscore, w_ij = alpha * dS_ij:
//   dA[i, k] = sum_j w_ij * df/da_k (A_i, B_j)          dB[j, k] = sum_i w_ij * df/db_k (A_i, B_j)
//   SQ_L2   df/da_k = 2 (a_k - b_k)                      L1  df/da_k = sign(a_k - b_k)  (0 at a tie, as abs)
//   ORDER   t_k = b_k - a_k:  -t_k / f where t_k >= 0, exactly 0 where t_k < 0  (clamp's backward is a select;
//           a pair at distance 0 has the coefficient w / 0 = NaN or inf, hence NaN where t_k == 0: torch's
//           sqrt backward does the same)
//   JACCARD I = sum min, U = sum max:  m_k / U - I M_k / U^2,  m_k = [a < b] + [a == b] / 2,
//           M_k = [a > b] + [a == b] / 2  (torch.min / torch.max split the gradient at a tie)
//   df/db_k: the same expression with a and b swapped.
// The reference expands B x B x D tensors (100 MB each at B = 128, D = 1536) and autograd keeps several; here
// two launches per call and O(na nb) workspace:
//   launch 1 (pwb_coef_kernel)  per-pair coefficients in fp64 into the workspace: w (SQ_L2, L1), w / f (ORDER),
//            w / U and w I / U^2 (JACCARD).  f, I, U are re-accumulated in fp64 over d, one pair per thread in
//            16 x 16 pair tiles: K10's 64 x 128 tiles give a training batch (B = 128) two blocks.
//   launch 2 (pwb_grad_kernel<METRIC, SIDE>, once per requested side)  a block owns PWB_R output rows x 256
//            columns k, a thread one column: its PWB_R elements of the own operand stay in registers, the
//            opposite operand's element [o, k] is one coalesced load per lane shared by the PWB_R rows (no reuse
//            across lanes: it needs no LDS), and the coefficients c[r, o] -- the same for every lane -- are staged
//            through LDS in chunks of PWB_OC opposite rows and read as broadcasts.  A coefficient that is
//            exactly 0 is skipped (a wave-uniform branch; max_violation leaves <= 3 non-zeros per row and
//            column); NaN and inf are not zero.
// Deterministic: every output element is owned by one thread, which sums over the opposite rows in increasing
// order in fp64 and rounds to fp32 once; no atomics.
#include "cmve_internal.h"

namespace cmve {

constexpr int PWB_CT = 16, PWB_CK = 32, PWB_CP = PWB_CT + 1;  // coefficient pass: pair tile, k slab, LDS pitch
constexpr int PWB_R = 4, PWB_OC = 64, PWB_KT = 256;           // gradient pass: rows, coefficient chunk, columns

constexpr bool pwb_reduces(int metric) { return metric == CMVE_PW_ORDER || metric == CMVE_PW_JACCARD; }
constexpr int pwb_planes(int metric) { return metric == CMVE_PW_JACCARD ? 2 : 1; }

template <int METRIC>
__global__ __launch_bounds__(256) void pwb_coef_kernel(const float* __restrict__ A, int64_t lda, int64_t na,
                                                       const float* __restrict__ B, int64_t ldb, int64_t nb,
                                                       int64_t d, double alpha, const float* __restrict__ dS,
                                                       int64_t ldd, double* __restrict__ coef) {
  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;
  const int64_t i0 = (int64_t)blockIdx.y * PWB_CT, j0 = (int64_t)blockIdx.x * PWB_CT;
  double s0 = 0.0, s1 = 0.0;
  if constexpr (pwb_reduces(METRIC)) {
    __shared__ double sa[PWB_CK][PWB_CP], sb[PWB_CK][PWB_CP];  // [k][row], fp64 once on the way in
    for (int64_t k0 = 0; k0 < d; k0 += PWB_CK) {
      for (int e = tid; e < PWB_CT * PWB_CK; e += 256) {  // coalesced along k
        const int r = e / PWB_CK, k = e % PWB_CK;
        const int64_t kk = k0 + k;
        sa[k][r] = (i0 + r < na && kk < d) ? (double)A[(i0 + r) * lda + kk] : 0.0;
        sb[k][r] = (j0 + r < nb && kk < d) ? (double)B[(j0 + r) * ldb + kk] : 0.0;
      }
      __syncthreads();
      const int kn = (int)min<int64_t>(PWB_CK, d - k0);
      for (int k = 0; k < kn; ++k) {
        const double a = sa[k][ty], b = sb[k][tx];
        if constexpr (METRIC == CMVE_PW_ORDER) {
          const double t = fmax(b - a, 0.0);
          s0 = fma(t, t, s0);
        } else {
          s0 += fmin(a, b);
          s1 += fmax(a, b);
        }
      }
      __syncthreads();
    }
  }
  const int64_t i = i0 + ty, j = j0 + tx;
  if (i >= na || j >= nb) return;
  const double w = alpha * (double)dS[i * ldd + j];
  const int64_t p = i * nb + j;
  if constexpr (METRIC == CMVE_PW_ORDER) {
    coef[p] = w / sqrt(s0);  // plain arithmetic: 0 / 0 = NaN, x / 0 = inf at distance 0
  } else if constexpr (METRIC == CMVE_PW_JACCARD) {
    coef[p] = w / s1;
    coef[na * nb + p] = w * s0 / (s1 * s1);
  } else {
    coef[p] = w;
  }
}

// SIDE 0: X = A (own), Y = B (opposite), c[r, o] = coef[r * nb + o]; SIDE 1: X = B, Y = A, c[r, o] = coef[o * nb + r]:
// the caller passes the strides (cr, co) of c and the plane distance (JACCARD's second coefficient)
template <int METRIC, int SIDE>
__global__ __launch_bounds__(PWB_KT) void pwb_grad_kernel(const float* __restrict__ X, int64_t ldx, int64_t nx,
                                                          const float* __restrict__ Y, int64_t ldy, int64_t ny,
                                                          int64_t d, const double* __restrict__ coef, int64_t cr,
                                                          int64_t co, int64_t plane, float* __restrict__ dX,
                                                          int64_t lddx) {
  constexpr bool JAC = METRIC == CMVE_PW_JACCARD;
  __shared__ double sc[JAC ? 2 : 1][PWB_R][PWB_OC];
  const int tid = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * PWB_R;
  const int64_t k = (int64_t)blockIdx.y * PWB_KT + tid;
  const bool live = k < d;
  double x[PWB_R], acc[PWB_R];
#pragma unroll
  for (int r = 0; r < PWB_R; ++r) {
    x[r] = (live && r0 + r < nx) ? (double)X[(r0 + r) * ldx + k] : 0.0;
    acc[r] = 0.0;
  }
  for (int64_t o0 = 0; o0 < ny; o0 += PWB_OC) {
    static_assert(PWB_R * PWB_OC == PWB_KT, "one coefficient per thread and chunk");
    {
      // SIDE 0 reads along o (the fast index of coef), SIDE 1 along r
      const int r = SIDE == 0 ? tid / PWB_OC : tid % PWB_R, o = SIDE == 0 ? tid % PWB_OC : tid / PWB_R;
      const bool in = r0 + r < nx && o0 + o < ny;
      const int64_t p = (r0 + r) * cr + (o0 + o) * co;
      sc[0][r][o] = in ? coef[p] : 0.0;  // (0: skipped)
      if constexpr (JAC) sc[1][r][o] = in ? coef[plane + p] : 0.0;
    }
    __syncthreads();
    const int on = (int)min<int64_t>(PWB_OC, ny - o0);
#pragma unroll 4
    for (int o = 0; o < on; ++o) {
      const double y = live ? (double)Y[(o0 + o) * ldy + k] : 0.0;
#pragma unroll
      for (int r = 0; r < PWB_R; ++r) {
        const double c = sc[0][r][o];
        if constexpr (METRIC == CMVE_PW_SQ_L2) {
          if (c == 0.0) continue;
          acc[r] = fma(c, x[r] - y, acc[r]);  // (doubled at the end)
        } else if constexpr (METRIC == CMVE_PW_L1) {
          if (c == 0.0) continue;
          const double u = x[r] - y;
          acc[r] = fma(u > 0.0 ? 1.0 : (u < 0.0 ? -1.0 : 0.0), c, acc[r]);
        } else if constexpr (METRIC == CMVE_PW_ORDER) {
          if (c == 0.0) continue;
          const double t = SIDE == 0 ? y - x[r] : x[r] - y;  // b_k - a_k
          const double g = SIDE == 0 ? -(t * c) : t * c;
          acc[r] += t >= 0.0 ? g : 0.0;  // the select: a NaN or inf coefficient reaches only t_k >= 0
        } else {
          const double q = sc[1][r][o];
          if (c == 0.0 && q == 0.0) continue;
          acc[r] += x[r] < y ? c : (x[r] > y ? -q : 0.5 * (c - q));
        }
      }
    }
    __syncthreads();
  }
  if (!live) return;
#pragma unroll
  for (int r = 0; r < PWB_R; ++r)
    if (r0 + r < nx) dX[(r0 + r) * lddx + k] = (float)(METRIC == CMVE_PW_SQ_L2 ? 2.0 * acc[r] : acc[r]);
}

static bool pwb_metric_ok(int32_t m) {
  return m == CMVE_PW_SQ_L2 || m == CMVE_PW_L1 || m == CMVE_PW_ORDER || m == CMVE_PW_JACCARD;
}

}  // namespace cmve

using namespace cmve;

#define PWB_REQUIRE_METRIC(fn)                                                                                   \
  CMVE_REQUIRE(metric >= CMVE_PW_SQ_L2 && metric <= CMVE_PW_DOT, fn ": unknown metric %d", metric);              \
  CMVE_REQUIRE(pwb_metric_ok(metric), fn ": metric %d (CMVE_PW_L2 / CMVE_PW_DOT) has no backward: no loss.py " \
                                         "measure uses it", metric)

extern "C" int cmve_pairwise_bwd_workspace(int64_t na, int64_t nb, int32_t metric, int64_t* bytes) {
  CMVE_REQUIRE(bytes, "cmve_pairwise_bwd_workspace: NULL argument");
  CMVE_REQUIRE(na >= 0 && nb >= 0, "cmve_pairwise_bwd_workspace: bad shape (%lld, %lld)", (long long)na,
               (long long)nb);
  PWB_REQUIRE_METRIC("cmve_pairwise_bwd_workspace");
  CMVE_REQUIRE(nb == 0 || na <= (INT64_MAX / 16) / nb, "cmve_pairwise_bwd_workspace: na * nb overflows");
  *bytes = na * nb * pwb_planes(metric) * (int64_t)sizeof(double);
  return CMVE_OK;
}

extern "C" int cmve_pairwise_bwd(cmve_handle_t h, const float* A, int64_t lda, int64_t na, const float* B, int64_t ldb,
                                 int64_t nb, int64_t d, int32_t metric, double alpha, const float* dS, int64_t ldd,
                                 float* dA, int64_t ldda, float* dB, int64_t lddb, void* ws, int64_t ws_bytes) {
  // (an empty side may come with a NULL pointer: nothing of it is read)
  CMVE_REQUIRE(h && (A || !na) && (B || !nb) && (dS || !na || !nb), "cmve_pairwise_bwd: NULL argument");
  CMVE_REQUIRE(na >= 0 && nb >= 0 && d > 0 && lda >= d && ldb >= d && ldd >= nb, "cmve_pairwise_bwd: bad shape");
  CMVE_REQUIRE((!dA || ldda >= d) && (!dB || lddb >= d), "cmve_pairwise_bwd: bad gradient leading dimension");
  PWB_REQUIRE_METRIC("cmve_pairwise_bwd");
  int64_t need = 0;
  if (int rc = cmve_pairwise_bwd_workspace(na, nb, metric, &need)) return rc;
  if ((!dA && !dB) || (na == 0 && nb == 0)) return CMVE_OK;
  const int64_t kt = (d + PWB_KT - 1) / PWB_KT;
  CMVE_REQUIRE(kt < 65536, "cmve_pairwise_bwd: d too large (%lld)", (long long)d);
  const hipStream_t st = h->stream;
  double* coef = (double*)ws;
  if (na > 0 && nb > 0) {
    CMVE_REQUIRE(ws && ws_bytes >= need, "cmve_pairwise_bwd: workspace too small (%lld < %lld bytes)",
                 (long long)ws_bytes, (long long)need);
    CMVE_REQUIRE((((uintptr_t)ws) & 7) == 0, "cmve_pairwise_bwd: workspace must be 8-byte aligned");
    CMVE_REQUIRE((na + PWB_CT - 1) / PWB_CT < 65536, "cmve_pairwise_bwd: too many rows in A (%lld)", (long long)na);
    const dim3 cgrid((unsigned)((nb + PWB_CT - 1) / PWB_CT), (unsigned)((na + PWB_CT - 1) / PWB_CT));
#define PWB_COEF(M) \
  hipLaunchKernelGGL((pwb_coef_kernel<M>), cgrid, dim3(256), 0, st, A, lda, na, B, ldb, nb, d, alpha, dS, ldd, coef)
    switch (metric) {
      case CMVE_PW_SQ_L2: PWB_COEF(CMVE_PW_SQ_L2); break;
      case CMVE_PW_L1: PWB_COEF(CMVE_PW_L1); break;
      case CMVE_PW_ORDER: PWB_COEF(CMVE_PW_ORDER); break;
      default: PWB_COEF(CMVE_PW_JACCARD); break;
    }
#undef PWB_COEF
  }
  // an empty opposite side leaves a zero gradient (the o loop does not run; coef is not read)
  const int64_t plane = na * nb;
#define PWB_GRAD(M)                                                                                               \
  do {                                                                                                            \
    if (dA && na > 0)                                                                                             \
      hipLaunchKernelGGL((pwb_grad_kernel<M, 0>), dim3((unsigned)((na + PWB_R - 1) / PWB_R), (unsigned)kt),       \
                         dim3(PWB_KT), 0, st, A, lda, na, B, ldb, nb, d, coef, nb, (int64_t)1, plane, dA, ldda);  \
    if (dB && nb > 0)                                                                                             \
      hipLaunchKernelGGL((pwb_grad_kernel<M, 1>), dim3((unsigned)((nb + PWB_R - 1) / PWB_R), (unsigned)kt),       \
                         dim3(PWB_KT), 0, st, B, ldb, nb, A, lda, na, d, coef, (int64_t)1, nb, plane, dB, lddb);  \
  } while (0)
  switch (metric) {
    case CMVE_PW_SQ_L2: PWB_GRAD(CMVE_PW_SQ_L2); break;
    case CMVE_PW_L1: PWB_GRAD(CMVE_PW_L1); break;
    case CMVE_PW_ORDER: PWB_GRAD(CMVE_PW_ORDER); break;
    default: PWB_GRAD(CMVE_PW_JACCARD); break;
  }
#undef PWB_GRAD
  return check_launch("pairwise_bwd");
}
