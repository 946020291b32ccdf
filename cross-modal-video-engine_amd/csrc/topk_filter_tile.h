// What the two filtered top-k entries share (K20: l2_topk.hip, the MFMA filter of CMVE_PW_L2; K23: l1_topk.hip, the SAD
// filter of CMVE_PW_L1), whatever brackets a pair's key: the stored upper bounds' rounding, launch A' (radix select of
// the k-th smallest bound and its widening to a threshold that is strict on the canonical words), launch C (re-score,
// sort, emit), the sample, the workspace layout and the checks of k / cand_cap / sample_rows.  A filter supplies its
// own pass kernel (launches A and B).  The derivations are DESIGN s4, "K20" and "K23".
#ifndef CMVE_TOPK_FILTER_TILE_H
#define CMVE_TOPK_FILTER_TILE_H
#include "l2_filter_tile.h"

namespace cmve {

constexpr int L2T_QC = 1024;        // queries per round of the four launches
constexpr int L2T_CAND_MAX = 2048;  // candidates launch C sorts in LDS: 12 bytes each beside l2f_chain64's staging

// the least fp32 at or above x, or one close to it (never below x); NaN -> +inf
__device__ __forceinline__ float l2t_f32_up(double x) {
  if (x != x) return __builtin_huge_valf();
  float f = (float)x;
  if ((double)f < x) {
    const uint32_t b = __float_as_uint(f);
    f = f > 0.f ? __uint_as_float(b + 1) : f < 0.f ? __uint_as_float(b - 1) : 1.17549435e-38f;
  }
  return f;
}

// The witnesses' bound tau (key space: k distinct columns have s D <= tau) -> the distance-space threshold of launch
// B, or NaN when there is none.  D is the squared distance (SQUARED: K20) or the L1 distance itself (K23).  DESIGN s4
// "K20": pick a score word t just on the far side of the witnesses and let l2f_thresholds speak for it.  alpha > 0:
// every witness has D <= Dt; if tb(t) > Dt each witness's canonical word is < t, and a column with D > tn(t) has a
// word >= t -- strictly worse than k columns' words, so outside the top-k whatever its index.  alpha < 0: every
// witness has D >= Dt = -tau; tb(t) < Dt makes their words < t and a column with D < tn(t) has a word >= t.  The
// condition on tb is CHECKED here, so the slack below is a first guess (rho relative on the distance, sigma absolute,
// as K19 steps 3-4; without the square also the underflow of alpha * S, as l2f_thresholds<false>) and not part of
// the proof.
template <bool SQUARED = true>
__device__ double l2t_widen(double tau, double alpha, double beta, double rho) {
  const bool pos = alpha > 0.0;
  if (!(fabs(tau) < __builtin_huge_val())) return (double)NAN;
  const double Dt = pos ? fmax(tau, 0.0) : -tau;
  if (!pos && !(Dt > 0.0)) return (double)NAN;  // the witnesses' distances have no positive lower bound
  const double y = SQUARED ? sqrt(Dt) : Dt;
  double slack = 4.0 * rho * y + 64.0 * L2F_U * (y + 2.0 * fabs(beta) / fabs(alpha)) + 1e-280;
  if constexpr (!SQUARED) slack += 4.0 * (4.9406564584124654e-324 / fabs(alpha));
  for (int it = 0; it < 12; ++it) {
    const double yy = pos ? y + slack : y - slack;
    const double t = alpha * yy + beta;
    double tb, tn;
    l2f_thresholds<SQUARED>(t, alpha, beta, rho, tb, tn);
    if (pos ? tb > Dt : tb < Dt) return tn;  // tn is never NaN for a non-NaN t
    slack *= 4.0;
  }
  return (double)NAN;
}

// order-preserving uint32 of an fp32 (smaller value -> smaller key)
__device__ __forceinline__ uint32_t l2t_key32(float f) {
  const uint32_t b = __float_as_uint(f);
  return (b >> 31) ? ~b : (b | 0x80000000u);
}

// launch A': one block per query.  The k-th smallest of its ns stored bounds by a 4 x 8-bit radix select, then the
// threshold; the query's candidate counter starts at zero here.
template <bool SQUARED>
__global__ __launch_bounds__(256) void l2t_threshold_kernel(const float* __restrict__ ub, int64_t ub_ld, int64_t ns,
                                                            int k, double alpha, double beta, double rho,
                                                            double* __restrict__ thr, int32_t* __restrict__ cnt) {
  __shared__ int hist[256];
  __shared__ uint32_t s_prefix;
  __shared__ int s_k;
  const int tid = threadIdx.x;
  const float* p = ub + (int64_t)blockIdx.x * ub_ld;
  uint32_t prefix = 0, mask = 0;
  int kk = k;  // the rank looked for among the values that match the prefix (ns >= k: it exists)
  for (int shift = 24; shift >= 0; shift -= 8) {
    hist[tid] = 0;
    __syncthreads();
    for (int64_t j = tid; j < ns; j += 256) {
      const uint32_t u = l2t_key32(p[j]);
      if ((u & mask) == prefix) atomicAdd(&hist[(u >> shift) & 255], 1);
    }
    __syncthreads();
    if (tid == 0) {
      int b = 0, below = 0;
      while (b < 255 && below + hist[b] < kk) below += hist[b++];
      s_prefix = prefix | ((uint32_t)b << shift);
      s_k = kk - below;
    }
    __syncthreads();
    prefix = s_prefix;
    kk = s_k;
    mask |= 255u << shift;
  }
  if (tid == 0) {
    const uint32_t b = (prefix >> 31) ? (prefix & 0x7fffffffu) : ~prefix;
    thr[blockIdx.x] = l2t_widen<SQUARED>((double)__uint_as_float(b), alpha, beta, rho);
    cnt[blockIdx.x] = 0;
  }
}

// the sort key of a canonical word: ascending, -0 == +0, every NaN last
__device__ __forceinline__ l2f_u64 l2t_ord(double w) {
  if (w != w) return ~0ull;
  if (w == 0.0) return 1ull << 63;
  const l2f_u64 b = (l2f_u64)__double_as_longlong(w);
  return (b >> 63) ? ~b : (b | (1ull << 63));
}

// launch C: one block per query of the round
template <int METRIC, typename TA, typename TB>
__global__ __launch_bounds__(256) void l2t_finish_kernel(const TA* __restrict__ Q, int64_t ldq,
                                                         const TB* __restrict__ G, int64_t ldg, int64_t d,
                                                         double alpha, double beta, int64_t q0,
                                                         const double* __restrict__ thr,
                                                         const int32_t* __restrict__ cnt,
                                                         const int32_t* __restrict__ list, int64_t cap, int k,
                                                         int64_t* __restrict__ out_idx, double* __restrict__ out_err,
                                                         l2f_u64* __restrict__ stats) {
  __shared__ double sd[4][64][L2F_KC + 1];
  __shared__ double sw[L2T_CAND_MAX];  // the candidates' words as the chain gives them (NaN payloads, -0 included)
  __shared__ int sid[L2T_CAND_MAX];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t gi = q0 + blockIdx.x;
  const int n = cnt[blockIdx.x];
  const double t = thr[blockIdx.x];
  // every test below is block-uniform.  n >= k holds whenever there is a threshold (the witnesses are candidates).
  if (!(t == t) || n > cap || n < k) {
    if (tid == 0) {
      out_idx[gi * k] = -2;
      gadd(stats + 3, (l2f_u64)1);
    }
    return;
  }
  const int32_t* mine = list + (int64_t)blockIdx.x * cap;
  for (int b0 = 0; b0 < n; b0 += 256) {
    const int p = b0 + tid;
    const bool live = p < n;
    const int j = mine[live ? p : b0];  // an idle lane repeats a candidate: its loads stay in bounds
    const double s = l2f_chain64<METRIC>(Q, ldq, G, ldg, d, (int)gi, j, sd[w], lane);
    if (live) {
      sw[p] = pw_score<METRIC>(s, 0.0, alpha, beta);
      sid[p] = j;
    }
  }
  if (tid == 0) gadd(stats + 2, (l2f_u64)n);
  int np = 2;
  while (np < n) np <<= 1;  // <= L2T_CAND_MAX, a power of two
  for (int p = n + tid; p < np; p += 256) {
    sw[p] = (double)NAN;
    sid[p] = 0x7fffffff;
  }
  __syncthreads();
  // bitonic sort by (l2t_ord(word), id): the ids are distinct, so the order is total (the padding never moves ahead)
  for (int size = 2; size <= np; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int e = tid; e < (np >> 1); e += 256) {
        const int lo = 2 * e - (e & (stride - 1)), hi = lo + stride;
        const double wl = sw[lo], wh = sw[hi];
        const int il = sid[lo], ih = sid[hi];
        const l2f_u64 ol = l2t_ord(wl), oh = l2t_ord(wh);
        const bool hi_first = oh < ol || (oh == ol && ih < il);
        const bool lo_first = ol < oh || (ol == oh && il < ih);
        if ((lo & size) == 0 ? hi_first : lo_first) {
          sw[lo] = wh;
          sw[hi] = wl;
          sid[lo] = ih;
          sid[hi] = il;
        }
      }
      __syncthreads();
    }
  for (int e = tid; e < k; e += 256) {
    out_idx[gi * k + e] = sid[e];
    out_err[gi * k + e] = sw[e];
  }
}

static inline int64_t l2t_round128(int64_t n) { return (n + 127) / 128 * 128; }

// the sample of launch A: the caller's, or max(k, 8) / 128 of the gallery within [1024, 65536] (the k-th of n_s sampled
// keys leaves about k n_g / n_s <= 128 gallery rows below it: launch C mostly re-scores one round of 256 candidates);
// at least k, a multiple of the tile, at most the gallery
static inline int64_t l2t_sample(int64_t n_g, int32_t k, int64_t sample_rows) {
  int64_t s = sample_rows > 0 ? sample_rows
                              : std::min<int64_t>(65536, std::max<int64_t>(1024, std::max<int64_t>(k, 8) * (n_g / 128)));
  s = l2t_round128(std::max<int64_t>(s, k));
  return std::min(s, std::max<int64_t>(n_g, 1));
}

struct L2tLayout {
  int64_t qc, s, ub_ld, thr, ub, list, cnt, bytes;
};
static inline L2tLayout l2t_layout(int64_t n_q, int64_t n_g, int32_t k, int64_t cand_cap, int64_t sample_rows) {
  L2tLayout l;
  l.qc = std::min<int64_t>(L2T_QC, l2t_round128(std::max<int64_t>(n_q, 1)));
  l.s = l2t_sample(n_g, k, sample_rows);
  l.ub_ld = l2t_round128(l.s);
  l.thr = 0;
  l.ub = l.thr + l.qc * 8;
  l.list = l.ub + l.qc * l.ub_ld * 4;
  l.cnt = l.list + l.qc * cand_cap * 4;
  l.bytes = (l.cnt + l.qc * 4 + 7) / 8 * 8;
  return l;
}

// what every top-k entry asks of k / cand_cap / sample_rows (the refusals name the entry)
static inline int l2t_check_params(const char* name, int32_t k, int64_t cand_cap, int64_t sample_rows) {
  CMVE_REQUIRE(k >= 1, "%s: k must be at least 1 (%d)", name, k);
  CMVE_REQUIRE(cand_cap >= k && cand_cap <= L2T_CAND_MAX, "%s: cand_cap must be in [k, %d] (%lld, k %d)", name,
               L2T_CAND_MAX, (long long)cand_cap, k);
  CMVE_REQUIRE(sample_rows >= 0 && sample_rows < (1ll << 31), "%s: bad sample_rows (%lld)", name,
               (long long)sample_rows);
  return CMVE_OK;
}

}  // namespace cmve
#endif
