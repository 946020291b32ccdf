// The MFMA filter of the Euclidean measures (CMVE_PW_L2, fp64 score words), shared by every kernel that decides a
// comparison of canonical words from an fp16 cosine:
//   K19 (l2_filter.hip: the count pass of the positions) and K20 (l2_topk.hip: the witness / candidate passes of the
//   top-k).
// One 128 x 128 tile of cosines over the packed unit planes (l2f_gemm_tile), the rigorous interval of a pair's
// squared distance (l2f_interval), the map of a score word back to squared-distance space (l2f_thresholds) and the
// canonical re-score of listed pairs (l2f_chain64) live here once; the derivation is DESIGN s4, "K19".
#ifndef CMVE_L2_FILTER_TILE_H
#define CMVE_L2_FILTER_TILE_H
#include "pairwise_tile.h"

namespace cmve {

typedef _Float16 l2f_f16x8 __attribute__((ext_vector_type(8)));
typedef float l2f_f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t l2f_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long l2f_u64;

constexpr int L2F_BM = 128, L2F_BN = 128, L2F_BK = 64;
constexpr int L2F_GM = 16;  // A tiles per group of the block order: 16 x 32 tiles in flight share 48 tiles of rows
constexpr int L2F_A_BYTES = L2F_BM * L2F_BK * 2, L2F_STAGE = (L2F_BM + L2F_BN) * L2F_BK * 2;
constexpr int L2F_SMEM = 2 * L2F_STAGE;  // the double-buffered staging of l2f_gemm_tile; the epilogues lay theirs over it
constexpr double L2F_U = 1.1102230246251565e-16;  // 2^-53
constexpr int L2F_KC = 16;  // l2f_chain64's k chunk

// the constants of DESIGN s4 (K19), every one rounded up generously
struct L2fConsts {
  double gamma;  // the MFMA accumulation term of score_error_bound (DESIGN s4)
  double theta;  // >= || fl(x * inv_norm) - x / ||x|| ||: the pack's x_hat against the true unit vector
  double kappa;  // relative slack on ||a||^2 + ||b||^2: the norms' roundings and the epilogue's own fp64 arithmetic
  double rho;    // relative slack of the canonical chain in distance space
};
static inline L2fConsts l2f_consts(int64_t d, int64_t d_pad) {
  L2fConsts c;
  const double n = (double)d_pad * (33.0 / 32.0), u = 1.0 / 8388608.0;
  c.gamma = n * u / (1.0 - n * u) * (1.0 + 1e-12);
  c.theta = ((double)d + 20.0) * L2F_U;
  c.kappa = 16.0 * ((double)d + 32.0) * L2F_U;
  c.rho = 2.0 * ((double)d + 16.0) * L2F_U;
  return c;
}

// What every filter entry asks of its two packed sets (host): the refusals name the entry.
static inline int l2f_check_sets(const char* name, const cmve_rows_t* a, const cmve_rows_t* b) {
  CMVE_REQUIRE(a->d > 0 && a->d == b->d && a->d_pad == b->d_pad, "%s: dimensions differ (%lld, %lld)", name,
               (long long)a->d, (long long)b->d);
  CMVE_REQUIRE(a->h16 && b->h16 && a->err_h16 && b->err_h16, "%s: a set was packed without its fp16 plane", name);
  CMVE_REQUIRE(a->eps == 0.0 && b->eps == 0.0, "%s: the sets must be packed with eps = 0", name);
  CMVE_REQUIRE(!(a->flags & CMVE_PACK_RAW) && !(b->flags & CMVE_PACK_RAW),
               "%s: CMVE_PACK_RAW sets hold no unit rows", name);
  const int64_t na = a->n, nb = b->n, d = a->d;
  CMVE_REQUIRE(na >= 0 && nb >= 0 && na < (1ll << 31) && nb < (1ll << 31) && a->n_pad >= na && b->n_pad >= nb &&
                   a->n_pad % CMVE_ROW_ALIGN == 0 && b->n_pad % CMVE_ROW_ALIGN == 0 && a->d_pad >= d &&
                   a->d_pad % CMVE_DIM_ALIGN == 0,
               "%s: bad shape", name);
  CMVE_REQUIRE((a->raw || !na) && (b->raw || !nb) && a->inv_norm && b->inv_norm && a->raw_ld >= d && b->raw_ld >= d,
               "%s: the sets' raw rows are missing", name);
  CMVE_REQUIRE((a->raw_dtype == CMVE_F32 || a->raw_dtype == CMVE_F64) &&
                   (b->raw_dtype == CMVE_F32 || b->raw_dtype == CMVE_F64),
               "%s: raw rows must be CMVE_F32/CMVE_F64", name);
  return CMVE_OK;
}

// the raw rows of both sides, the operands of every canonical score: what a filtered count (filter_count.h) and a
// filtered top-k (topk_filter_tile.h) hand the launches that re-score on the canonical chain
struct FltRows {
  const void* A;
  int32_t a_dtype;
  int64_t lda, na;
  const void* B;
  int32_t b_dtype;
  int64_t ldb, nb, d;
};

// The epilogues' side load of one tile row as l2f_interval takes it: the row's norm (from 1 / inv_norm) and its error
// (err_h16 + theta); NaN for a row beyond the set (no interval: its pairs are never decided)
__device__ __forceinline__ double l2f_side_norm(int64_t row, bool valid, const double* inv_norm) {
  return valid ? 1.0 / inv_norm[row] : (double)NAN;
}
__device__ __forceinline__ double l2f_side_err(int64_t row, bool valid, const float* err_h16, double theta) {
  return valid ? (double)err_h16[row] + theta : (double)NAN;
}

// The item word t mapped back to squared-distance space (DESIGN s4, K19).  A pair of true squared distance D has
// e(i, j) < t whenever   alpha > 0: D < tb,   alpha < 0: D > tb   and  e(i, j) >= t  whenever  alpha > 0: D > tn,
// alpha < 0: D < tn.  x = (t - beta) / alpha is the distance at which the real-number score equals t; sig covers the
// roundings of x itself and of the chain's alpha * x + beta (contracted or not); rho those of the sum, the
// subtractions and the square root.  A NaN item is never counted: every pair with a finite interval is not-below.
// SQUARED = false (K22, CMVE_PW_L1): D is the L1 distance itself -- no square -- and sig also carries the underflow of
// the chain's product alpha * S, 2^-1074 / |alpha| in distance space.
template <bool SQUARED = true>
__device__ __forceinline__ void l2f_thresholds(double t, double alpha, double beta, double rho, double& tb,
                                               double& tn) {
  const bool pos = alpha > 0.0;
  const double inf = __builtin_huge_val();
  const double none = pos ? -inf : inf;  // tb = tn = none: no pair is below, every finite one is not-below
  if (t != t) { tb = none; tn = none; return; }
  if (fabs(t) == inf) {  // a finite pair (the epilogue's overflow guard) is below +inf and not below -inf
    tb = tn = (t > 0.0) ? -none : none;
    return;
  }
  const double x = (t - beta) / alpha;
  double sig = 16.0 * L2F_U * ((fabs(t) + fabs(beta)) / fabs(alpha)) + 1e-290;
  if constexpr (!SQUARED) sig += 4.9406564584124654e-324 / fabs(alpha);
  const double xlo = x - sig, xhi = x + sig;
  const double l = xlo * (1.0 - rho), h = xhi * (1.0 + 2.0 * rho);
  const double lo_t = xlo > 0.0 ? (SQUARED ? l * l : l) * (1.0 - 4.0 * L2F_U) : -inf;  // D below it: the distance is below x
  const double hi_t = xhi > 0.0 ? (SQUARED ? h * h : h) * (1.0 + 4.0 * L2F_U) : 0.0;   // D above it: the distance is above x
  tb = pos ? lo_t : hi_t;
  tn = pos ? hi_t : lo_t;
}

// [dlo, dhi] holds the true squared distance of the pair (NaN, NaN when no such statement can be made)
__device__ __forceinline__ void l2f_interval(float c, double na_, double ea, double nb_, double eb, double gamma,
                                             double kappa, double& dlo, double& dhi) {
  const double sa = na_ * na_, sb = nb_ * nb_, ss = sa + sb, p = 2.0 * na_ * nb_;
  const double E = ea + (1.0 + ea) * eb + gamma * ((1.0 + ea) * (1.0 + eb)) + 1e-12;
  const double W = (p * E + ss * kappa) * (1.0 + 1e-9) + 1e-280;
  const double d2 = ss - p * (double)c;
  const bool ok = ss < 1e300;  // no overflow anywhere in the canonical chain; false for NaN
  dlo = ok ? d2 - W : (double)NAN;
  dhi = ok ? d2 + W : (double)NAN;
}

__device__ __forceinline__ uint32_t l2f_lds_off(int r, int chunk) {
  return (uint32_t)(r * (L2F_BK * 2) + ((chunk ^ (r & 7)) << 4));
}

// block order: groups of L2F_GM A tiles, inside a group the A tile runs fastest
__device__ __forceinline__ void l2f_tile_of_block(int64_t L, int tiles_a, int tiles_b, int& ta, int& tb) {
  const int64_t per = (int64_t)L2F_GM * tiles_b;
  const int g = (int)(L / per);
  const int64_t in = L - (int64_t)g * per;
  const int gs = min(L2F_GM, tiles_a - g * L2F_GM);
  ta = g * L2F_GM + (int)(in % gs);
  tb = (int)(in / gs);
}

// The GEMM of one tile, 256 threads: 4 waves of 64 x 64, 64-deep K-tiles double-buffered in smem (L2F_SMEM bytes,
// 16-byte aligned; register staged, XOR-swizzled 16-B chunks).  On return acc[m][n][r] is the fp16 MFMA cosine of the
// pair (A row i0 + wm 64 + 16 m + 4 fq + r, B row j0 + wn 64 + 16 n + fr), wm = wave >> 1, wn = wave & 1,
// fr = lane & 15, fq = lane >> 4, and every wave has passed the loop's last barrier: smem is free.
// Rows i0 .. i0 + 127 and j0 .. j0 + 127 are read whole: they must lie below the planes' n_pad (a multiple of 256).
__device__ __forceinline__ void l2f_gemm_tile(const uint16_t* __restrict__ a16, const uint16_t* __restrict__ b16,
                                              int64_t d_pad, int64_t i0, int64_t j0, char* smem,
                                              l2f_f32x4 (&acc)[4][4]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[m][n] = l2f_f32x4{0.f, 0.f, 0.f, 0.f};
  const int sc_ = tid & 7, sr = tid >> 3;  // staging: chunk sc_ of rows sr + 32 it
  const uint16_t* ga = a16 + (i0 + sr) * d_pad + sc_ * 8;
  const uint16_t* gb = b16 + (j0 + sr) * d_pad + sc_ * 8;
  const uint32_t soff = l2f_lds_off(sr, sc_);  // (sr + 32 it) & 7 == sr & 7
  l2f_u32x4 ra[4], rb[4];
  const int nk = (int)(d_pad / L2F_BK);
#define L2F_LOAD(kt)                                                                     \
  _Pragma("unroll") for (int it = 0; it < 4; ++it) {                                     \
    ra[it] = *(const l2f_u32x4*)(ga + (int64_t)(32 * it) * d_pad + (kt) * L2F_BK);       \
    rb[it] = *(const l2f_u32x4*)(gb + (int64_t)(32 * it) * d_pad + (kt) * L2F_BK);       \
  }
#define L2F_WRITE(buf)                                                                   \
  _Pragma("unroll") for (int it = 0; it < 4; ++it) {                                     \
    *(l2f_u32x4*)(smem + (buf) * L2F_STAGE + soff + it * 32 * (L2F_BK * 2)) = ra[it];    \
    *(l2f_u32x4*)(smem + (buf) * L2F_STAGE + L2F_A_BYTES + soff + it * 32 * (L2F_BK * 2)) = rb[it]; \
  }
  L2F_LOAD(0)
  L2F_WRITE(0)
  __syncthreads();
  const int fr = lane & 15, fq = lane >> 4;
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < nk) { L2F_LOAD(kt + 1) }
    const char* pa = smem + buf * L2F_STAGE;
    const char* pb = pa + L2F_A_BYTES;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      l2f_f16x8 fa[4], fb[4];
#pragma unroll
      for (int m = 0; m < 4; ++m) fa[m] = *(const l2f_f16x8*)(pa + l2f_lds_off(wm * 64 + m * 16 + fr, ks * 4 + fq));
#pragma unroll
      for (int n = 0; n < 4; ++n) fb[n] = *(const l2f_f16x8*)(pb + l2f_lds_off(wn * 64 + n * 16 + fr, ks * 4 + fq));
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n)
          acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[m], fb[n], acc[m][n], 0, 0, 0);
    }
    if (kt + 1 < nk) { L2F_WRITE(buf ^ 1) }
    __syncthreads();
  }
#undef L2F_LOAD
#undef L2F_WRITE
}

// The canonical sum (of squares: CMVE_PW_L2; of magnitudes: CMVE_PW_L1) of 64 listed pairs, one per lane of a wave:
// lane l's pair is (A row i, B row j) of ITS
// arguments.  The (a - b) chunks go through sd (this wave's [64][L2F_KC + 1] doubles of LDS) transposed, so the loads
// are coalesced (16 lanes read 128 contiguous bytes of a row); each lane then runs its own pair's chain, pw_acc with
// k ascending into one accumulator from zero.  Every lane must name rows that exist (an idle lane repeats a listed
// pair).  The barriers are the block's: every wave of the block calls this the same number of times with the same d.
// CMVE_PW_JACCARD (K24): the two sums of the pair -- the minima's is returned, the maxima's goes to *s1_out.  Its chain
// takes both elements, so a chunk is L2F_KC / 2 deep: the A elements in sd's columns 0 .. 7, the B elements in 8 .. 15.
template <int METRIC = CMVE_PW_L2, typename TA, typename TB>
__device__ __forceinline__ double l2f_chain64(const TA* __restrict__ A, int64_t lda, const TB* __restrict__ B,
                                              int64_t ldb, int64_t d, int i, int j, double (&sd)[64][L2F_KC + 1],
                                              int lane, double* s1_out = nullptr) {
  if constexpr (METRIC == CMVE_PW_JACCARD) {
    constexpr int KH = L2F_KC / 2;
    double s0 = 0.0, s1 = 0.0;
    for (int64_t k0 = 0; k0 < d; k0 += KH) {
#pragma unroll 4
      for (int it = 0; it < 16; ++it) {
        const int q = it * 4 + (lane >> 4), k = lane & 7, side = (lane >> 3) & 1;
        const int64_t qi = __shfl(i, q, 64), qj = __shfl(j, q, 64);
        double x = 0.0;
        if (k0 + k < d) x = side ? (double)B[qj * ldb + k0 + k] : (double)A[qi * lda + k0 + k];
        sd[q][side * KH + k] = x;
      }
      __syncthreads();
      const int kn = (int)min<int64_t>(KH, d - k0);
      for (int k = 0; k < kn; ++k) pw_acc<METRIC>(sd[lane][k], sd[lane][KH + k], s0, s1);
      __syncthreads();
    }
    *s1_out = s1;
    return s0;
  }
  double s = 0.0, unused = 0.0;
  for (int64_t k0 = 0; k0 < d; k0 += L2F_KC) {
#pragma unroll 4
    for (int it = 0; it < 16; ++it) {
      const int q = it * 4 + (lane >> 4), k = lane & 15;
      const int64_t qi = __shfl(i, q, 64), qj = __shfl(j, q, 64);
      double df = 0.0;
      if (k0 + k < d) df = (double)A[qi * lda + k0 + k] - (double)B[qj * ldb + k0 + k];
      sd[q][k] = df;
    }
    __syncthreads();
    const int kn = (int)min<int64_t>(L2F_KC, d - k0);
    // the subtraction was done above (exact fp64 either way): pw_acc's own  t - 0  leaves it as it is
    for (int k = 0; k < kn; ++k) pw_acc<METRIC>(sd[lane][k], 0.0, s, unused);
    __syncthreads();
  }
  return s;
}

}  // namespace cmve
#endif
