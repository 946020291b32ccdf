// The per-pair score chain of the non-cosine measures, shared by every kernel that produces a pair's score:
//   K10 (pairwise.hip: the stored matrix) and K18 (pairwise_rank.hip: matrix-free positions / top-k).
// A pair's score is: both inputs converted to fp64; pw_acc for k = 0 .. d-1 in ascending order into one
// accumulator (two for jaccard) that starts at zero; pw_final; alpha * x + beta (pw_score); one rounding to the
// score dtype.  The chain of one pair does not depend on the tile geometry or on which thread runs it, so two
// kernels that go through these functions produce the same bits -- the decisions K18 takes (ranks, positions,
// top-k order) are the ones the matrix path takes on K10's output.
#ifndef CMVE_PAIRWISE_TILE_H
#define CMVE_PAIRWISE_TILE_H
#include "cmve_internal.h"

namespace cmve {

template <int METRIC>
__device__ __forceinline__ void pw_acc(double a, double b, double& s0, double& s1) {
  if constexpr (METRIC == CMVE_PW_SQ_L2 || METRIC == CMVE_PW_L2) {
    const double t = a - b;
    s0 = fma(t, t, s0);
  } else if constexpr (METRIC == CMVE_PW_L1) {
    s0 += fabs(a - b);
  } else if constexpr (METRIC == CMVE_PW_ORDER) {
    const double t = fmax(b - a, 0.0);
    s0 = fma(t, t, s0);
  } else if constexpr (METRIC == CMVE_PW_DOT) {
    s0 = fma(a, b, s0);
  } else {  // JACCARD
    s0 += fmin(a, b);
    s1 += fmax(a, b);
  }
}

template <int METRIC>
__device__ __forceinline__ double pw_final(double s0, double s1) {
  if constexpr (METRIC == CMVE_PW_L2 || METRIC == CMVE_PW_ORDER) return sqrt(s0);
  else if constexpr (METRIC == CMVE_PW_JACCARD) return s0 / s1;
  else return s0;
}

// the one expression every stored or compared score goes through (before its rounding to the score dtype)
template <int METRIC>
__device__ __forceinline__ double pw_score(double s0, double s1, double alpha, double beta) {
  return alpha * pw_final<METRIC>(s0, s1) + beta;
}

// the one rounding to the score dtype (f32: float32 words, carried in a double)
__device__ __forceinline__ double pw_round(double x, int f32) { return f32 ? (double)(float)x : x; }

// the whole chain of one pair from its two rows (one thread: the listed items of K18, a handful per query)
template <int METRIC, typename TA, typename TB>
__device__ __forceinline__ double pw_pair_score(const TA* __restrict__ a, const TB* __restrict__ b, int64_t d,
                                                double alpha, double beta) {
  double s0 = 0.0, s1 = 0.0;
  for (int64_t k = 0; k < d; ++k) pw_acc<METRIC>((double)a[k], (double)b[k], s0, s1);
  return pw_score<METRIC>(s0, s1, alpha, beta);
}

// Tile geometry of a 256-thread block laid out as TX x NTY threads: thread (tx, ty) owns the A rows
// {2 ty + 2 NTY u + e} and the B rows {2 tx + 2 TX v + e} (u < UP, v < VP, e < 2) of a TA x TB tile, K staged
// through LDS in KS-deep slabs (converted to fp64 once on the way in).  Rows come in 16-byte pairs, consecutive
// across the lanes of a row group: the ds_read_b128 of a slab row are conflict-free.
template <int NTY_, int UP_, int VP_, int KS_>
struct PwGeom {
  static constexpr int NTY = NTY_, TX = 256 / NTY_, UP = UP_, VP = VP_, KS = KS_;
  static constexpr int TA = 2 * NTY * UP, TB = 2 * TX * VP, PA = TA + 2, PB = TB + 2;
  static constexpr int NA = 2 * UP, NB = 2 * VP;  // outputs per thread: NA x NB
  __device__ static __forceinline__ int arow(int ty, int u) { return 2 * ty + 2 * NTY * (u >> 1) + (u & 1); }
  __device__ static __forceinline__ int brow(int tx, int v) { return 2 * tx + 2 * TX * (v >> 1) + (v & 1); }
};
// K10's tile: 64 x 128, 16 x 16 threads, 4 x 8 outputs per thread from 2 + 4 ds_read_b128 per k (against 8
// ds_read_b64 per 16 outputs in a 4 x 4 layout -- the LDS port no longer matches the fp64 VALU rate)
using PwWide = PwGeom<16, 2, 4, 32>;
// a handful of query rows against a long gallery (inference.py's n_q = 1): 8 x 256, every thread owns 4 of the 8
// A rows and 2 B rows -- no 64 rows of padding to compute; 16-deep slabs keep the B stage within the LDS
using PwSmall = PwGeom<2, 2, 1, 16>;

constexpr int PW_TA = PwWide::TA, PW_TB = PwWide::TB, PW_K = PwWide::KS;

// Stage-and-accumulate over K for the tile at (i0, j0): s0 / s1 [NA][NB] must start at zero (s1 is [1][1] and
// untouched unless METRIC is jaccard).  Rows beyond na / nb are staged as zeros (their accumulators hold
// f(0, b) / f(a, 0): the caller must not use them); K stops at d (zero padding would bias L1 / jaccard).
template <typename G, int METRIC, typename TA, typename TB, int S1A, int S1B>
__device__ __forceinline__ void pw_tile_loop(const TA* __restrict__ A, int64_t lda, int64_t na,
                                             const TB* __restrict__ B, int64_t ldb, int64_t nb, int64_t d,
                                             int64_t i0, int64_t j0, double (&sa)[G::KS][G::PA],
                                             double (&sb)[G::KS][G::PB], double (&s0)[G::NA][G::NB],
                                             double (&s1)[S1A][S1B]) {
  constexpr bool JAC = METRIC == CMVE_PW_JACCARD;
  static_assert(S1A == (JAC ? G::NA : 1) && S1B == (JAC ? G::NB : 1), "s1 is [NA][NB] for jaccard, else [1][1]");
  const int tid = threadIdx.x;
  const int tx = tid % G::TX, ty = tid / G::TX;
  for (int64_t k0 = 0; k0 < d; k0 += G::KS) {
    for (int e = tid; e < G::TA * G::KS; e += 256) {  // coalesced along k
      const int r = e / G::KS, k = e % G::KS;
      const int64_t kk = k0 + k;
      sa[k][r] = (i0 + r < na && kk < d) ? (double)A[(i0 + r) * lda + kk] : 0.0;
    }
    for (int e = tid; e < G::TB * G::KS; e += 256) {
      const int r = e / G::KS, k = e % G::KS;
      const int64_t kk = k0 + k;
      sb[k][r] = (j0 + r < nb && kk < d) ? (double)B[(j0 + r) * ldb + kk] : 0.0;
    }
    __syncthreads();
    const int kn = (int)min<int64_t>(G::KS, d - k0);  // zero padding would bias L1 / jaccard: stop at d
    for (int k = 0; k < kn; ++k) {
      double av[G::NA], bv[G::NB];
#pragma unroll
      for (int u = 0; u < G::UP; ++u) {
        const double2 t = *(const double2*)&sa[k][2 * ty + 2 * G::NTY * u];
        av[2 * u] = t.x;
        av[2 * u + 1] = t.y;
      }
#pragma unroll
      for (int v = 0; v < G::VP; ++v) {
        const double2 t = *(const double2*)&sb[k][2 * tx + 2 * G::TX * v];
        bv[2 * v] = t.x;
        bv[2 * v + 1] = t.y;
      }
#pragma unroll
      for (int u = 0; u < G::NA; ++u)
#pragma unroll
        for (int v = 0; v < G::NB; ++v) {
          double dummy = 0.0;
          pw_acc<METRIC>(av[u], bv[v], s0[u][v], JAC ? s1[JAC ? u : 0][JAC ? v : 0] : dummy);
        }
    }
    __syncthreads();
  }
}

// Dispatch helpers of the entry points: PW_DISPATCH_METRIC(metric, M, stmt) runs stmt with the constant M
#define PW_DISPATCH_METRIC(metric, M, ...)                                        \
  switch (metric) {                                                               \
    case CMVE_PW_SQ_L2: { constexpr int M = CMVE_PW_SQ_L2; __VA_ARGS__; } break;  \
    case CMVE_PW_L2: { constexpr int M = CMVE_PW_L2; __VA_ARGS__; } break;        \
    case CMVE_PW_L1: { constexpr int M = CMVE_PW_L1; __VA_ARGS__; } break;        \
    case CMVE_PW_ORDER: { constexpr int M = CMVE_PW_ORDER; __VA_ARGS__; } break;  \
    case CMVE_PW_DOT: { constexpr int M = CMVE_PW_DOT; __VA_ARGS__; } break;      \
    default: { constexpr int M = CMVE_PW_JACCARD; __VA_ARGS__; } break;           \
  }
// PWR_TYPES(a, b, TA, TB, stmt): stmt with the element types of the two sides (CMVE_F32 / CMVE_F64 each)
#define PWR_TYPES(a_dtype, b_dtype, TA, TB, ...)                                    \
  if (a_dtype == CMVE_F64 && b_dtype == CMVE_F64) { using TA = double; using TB = double; __VA_ARGS__; } \
  else if (a_dtype == CMVE_F64) { using TA = double; using TB = float; __VA_ARGS__; }                    \
  else if (b_dtype == CMVE_F64) { using TA = float; using TB = double; __VA_ARGS__; }                    \
  else { using TA = float; using TB = float; __VA_ARGS__; }

}  // namespace cmve
#endif
