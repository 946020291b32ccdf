// What the filtered top-k entries share (K20: l2_topk.hip, the MFMA filter of CMVE_PW_L2; K23: l1_topk.hip, the SAD
// filter of CMVE_PW_L1; K25: jaccard_topk.hip, the SAD filter of CMVE_PW_JACCARD with float32 words), whatever brackets
// a pair's key:
//   l2t_f32_up, l2t_row_state, l2t_pair, l2t_decide, l2t_flush   the tail of a pass kernel's epilogue once it holds a
//                          pair's interval: the stored upper bounds' rounding, the row's threshold and overflow flag,
//                          "launch A stores the bound, launch B excludes or appends", the two counters (K25 brackets
//                          two sums, not a distance: its pair step is its own and ends in l2t_decide)
//   l2t_kth_bound, l2t_threshold_kernel   launch A': radix select of the k-th smallest bound, widened to a threshold
//                          that is strict on the canonical words (K25 maps the bound through float32 words: a
//                          threshold kernel of its own around the same select)
//   l2t_finish_kernel      launch C: re-score, sort, emit
//   l2t_sample, l2t_layout, l2t_check_params   the sample, the workspace and the checks of k / cand_cap / sample_rows
//   l2t_topk_run           the host body: checks, memset, the rounds of four launches
// A filter supplies its operands' checks, its pass kernel (tile, interval, thread layout) and the launch of it; the
// two SAD filters' pass kernels are one body (sad_topk.h) under a policy each.  The derivations are DESIGN s4, "K20",
// "K23" and "K25".
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

// ---- the common tail of the two pass kernels' epilogues.  MODE 0: launch A (the witnesses' bounds), MODE 1: launch B
// (the candidates).  `Args` is the kernel's own flat argument block (L2tArgs; sad_topk.h's SadTopkArgs under a policy's
// Args): it names q0, thr, cnt, cap, ub, ub_ld, list and stats; `Epi` its epilogue LDS (L2tEpi, SadTopkEpi<NS>): it names
// thr[128] and full[128] by tile row, and n_cand and n_excl, zeroed before the pairs.  (The helpers take a, E and the global row i whole: handed `double& thr`, `int& full` or
// i - a.q0 instead, l2t_pass_kernel<1> compiles to another instruction stream; as they are, K20's two kernels keep
// the streams they had with the statements written out.)

// query row i (thread tid's row of the tile; `valid`: it exists) into the tile's LDS: its threshold, and whether its
// list had overflowed when this tile began.  An overflowed list is lost (launch C asks only whether the counter exceeds cap), so
// its row stops appending: rows clustered far from the origin -- every pair a candidate -- would otherwise serialise
// n_g atomics on one address per query.  Read once per row and tile, off the pairs' path; the counter only grows, so a
// tile that reads it early merely adds its own <= 128 candidates more.
template <int MODE, typename Args, typename Epi>
__device__ __forceinline__ void l2t_row_state(const Args& a, Epi& E, int tid, int64_t i, bool valid) {
  if (MODE == 1) {
    E.thr[tid] = valid ? a.thr[i - a.q0] : (double)NAN;
    E.full[tid] = valid ? __hip_atomic_load(a.cnt + (i - a.q0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > a.cap : 1;
  }
}

// launch B's verdict on the pair (query i, column j) of a query that has a threshold: `out` -- its key is provably
// beyond it -- counts it excluded; anything else is a candidate, appended unless the row's list was already full
template <typename Args>
__device__ __forceinline__ void l2t_decide(const Args& a, bool out, int64_t i, int64_t j, bool full, int& n_cand,
                                           int& n_excl) {
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

// one pair (query i, column j) whose distance lies in [dlo, dhi] (NaN, NaN: no interval); pos: alpha > 0
template <int MODE, typename Args>
__device__ __forceinline__ void l2t_pair(const Args& a, bool pos, int64_t i, int64_t j, double dlo, double dhi,
                                         double thr, bool full, int& n_cand, int& n_excl) {
  if (MODE == 0) {
    // key = s D: its upper bound is dhi (alpha > 0) or -dlo (alpha < 0); NaN (no interval) becomes +inf
    a.ub[(i - a.q0) * a.ub_ld + j] = l2t_f32_up(pos ? dhi : -dlo);
  } else if (thr == thr) {
    // excluded only on a positive test: D is provably beyond the threshold (a NaN interval fails it)
    l2t_decide(a, pos ? dlo > thr : dhi < thr, i, j, full, n_cand, n_excl);
  }
}

// the thread's counts through the block's LDS words into stats[0..1]: two integer atomics per tile
template <int MODE, typename Args, typename Epi>
__device__ __forceinline__ void l2t_flush(const Args& a, Epi& E, int tid, int n_cand, int n_excl) {
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

// The k-th smallest of the ns bounds at p by a 4 x 8-bit radix select, on the block's 256 threads (ns >= k: it
// exists); every thread returns it.
__device__ __forceinline__ float l2t_kth_bound(const float* __restrict__ p, int64_t ns, int k) {
  __shared__ int hist[256];
  __shared__ uint32_t s_prefix;
  __shared__ int s_k;
  const int tid = threadIdx.x;
  uint32_t prefix = 0, mask = 0;
  int kk = k;  // the rank looked for among the values that match the prefix
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
  return __uint_as_float((prefix >> 31) ? (prefix & 0x7fffffffu) : ~prefix);
}

// launch A': one block per query.  The k-th smallest of its ns stored bounds, then the threshold; the query's
// candidate counter starts at zero here.
template <bool SQUARED>
__global__ __launch_bounds__(256) void l2t_threshold_kernel(const float* __restrict__ ub, int64_t ub_ld, int64_t ns,
                                                            int k, double alpha, double beta, double rho,
                                                            double* __restrict__ thr, int32_t* __restrict__ cnt) {
  const float tau = l2t_kth_bound(ub + (int64_t)blockIdx.x * ub_ld, ns, k);
  if (threadIdx.x == 0) {
    thr[blockIdx.x] = l2t_widen<SQUARED>((double)tau, alpha, beta, rho);
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
    // (jaccard, K25: both sums, and the one rounding to the float32 word)
    constexpr bool JAC = METRIC == CMVE_PW_JACCARD;
    double s1 = 0.0;
    const double s = l2f_chain64<METRIC>(Q, ldq, G, ldg, d, (int)gi, j, sd[w], lane, JAC ? &s1 : nullptr);
    if (live) {
      sw[p] = pw_round(pw_score<METRIC>(s, s1, alpha, beta), JAC);
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

// ---- the host body -------------------------------------------------------------------------------------------------------
// what l2t_topk_run hands a filter's pass launch beside the filter's own operands: the workspace carved up (the same
// for every round) and one pass of one round.  The pass kernels keep their flat argument blocks (L2tArgs; SadTopkArgs,
// which sad_topk_args fills) and are filled from these: an embedded struct moves a kernel's scalar loads
// (filter_count.h).
struct L2tWs {
  float* ub;       // [qc][ub_ld] upper key bounds
  int64_t ub_ld;
  double* thr;     // per query of the round: the distance-space threshold
  int32_t* cnt;    // per query of the round: candidates found
  int32_t* list;   // [qc][cap] column ids
  int64_t cap;
  l2f_u64* stats;  // {pairs excluded, candidates found, candidates re-scored, unresolved queries}
};
struct L2tRound {
  int64_t q0, q_end;  // this round's queries; q0 is a multiple of 128
  int64_t ng;         // columns of this pass: the sample (launch A) or the gallery (launch B)
  int tiles_a, tiles_b;
};

// One filtered top-k on h's stream.  `name`: the entry (refusals), `label`: check_launch's; METRIC: CMVE_PW_L2 (the
// keys are squared distances), CMVE_PW_L1 or CMVE_PW_JACCARD (float32 words); r: the raw rows (q is A, the gallery
// B); own_checks(): the entry's checks of its own operands, run where they always ran (after the scaling and the
// parameters, before k against the gallery); pass_launch(mode, st, round, ws): the filter's pass kernel, MODE = mode,
// over round.tiles_a x round.tiles_b blocks of 256 threads; thr_launch(st, nq, ns, ws): launch A' -- nq blocks of 256
// threads that leave the round's ws.thr from the ns stored bounds per query and zero ws.cnt.
template <int METRIC, typename Own, typename Pass, typename Thr>
static inline int l2t_topk_run(const char* name, const char* label, cmve_handle_t h, const FltRows& r, double alpha,
                               double beta, int32_t k, int64_t cand_cap, int64_t sample_rows, void* ws,
                               int64_t ws_bytes, int64_t* out_idx, double* out_err, int64_t* stats,
                               Own own_checks, Pass pass_launch, Thr thr_launch) {
  CMVE_REQUIRE(alpha != 0.0 && std::isfinite(alpha) && std::isfinite(beta),
               "%s: alpha must be finite and non-zero, beta finite (%g, %g)", name, alpha, beta);
  if (int rc = l2t_check_params(name, k, cand_cap, sample_rows)) return rc;
  if (int rc = own_checks()) return rc;
  const int64_t n_q = r.na, n_g = r.nb;
  CMVE_REQUIRE(k <= n_g || n_q == 0, "%s: k exceeds the gallery (%d > %lld): clamp it", name, k, (long long)n_g);
  CMVE_REQUIRE((out_idx && out_err) || !n_q, "%s: NULL output", name);
  const L2tLayout l = l2t_layout(n_q, n_g, k, cand_cap, sample_rows);
  CMVE_REQUIRE(n_q == 0 || (ws && ws_bytes >= l.bytes), "%s: workspace too small (%lld < %lld bytes)", name,
               (long long)ws_bytes, (long long)l.bytes);
  CMVE_REQUIRE((((uintptr_t)ws) & 7) == 0, "%s: workspace must be 8-byte aligned", name);
  const hipStream_t st = h->stream;
  CMVE_HIP(hipMemsetAsync(stats, 0, 4 * sizeof(int64_t), st));
  if (n_q == 0) return CMVE_OK;
  char* base = (char*)ws;
  const L2tWs w{(float*)(base + l.ub), l.ub_ld, (double*)(base + l.thr), (int32_t*)(base + l.cnt),
                (int32_t*)(base + l.list), cand_cap, (l2f_u64*)stats};
  const int tiles_s = (int)((l.s + L2F_BN - 1) / L2F_BN), tiles_g = (int)((n_g + L2F_BN - 1) / L2F_BN);
  for (int64_t q0 = 0; q0 < n_q; q0 += l.qc) {
    const int64_t nq = std::min(l.qc, n_q - q0);
    const int tiles_a = (int)((nq + L2F_BM - 1) / L2F_BM);  // <= 8: tiles_a * tiles_g < 2^31
    pass_launch(0, st, L2tRound{q0, q0 + nq, l.s, tiles_a, tiles_s}, w);
    thr_launch(st, nq, l.s, w);
    pass_launch(1, st, L2tRound{q0, q0 + nq, n_g, tiles_a, tiles_g}, w);
    PWR_TYPES(r.a_dtype, r.b_dtype, TA, TB, {
      hipLaunchKernelGGL((l2t_finish_kernel<METRIC, TA, TB>), dim3((unsigned)nq), dim3(256), 0, st, (const TA*)r.A,
                         r.lda, (const TB*)r.B, r.ldb, r.d, alpha, beta, q0, (const double*)w.thr,
                         (const int32_t*)w.cnt, (const int32_t*)w.list, w.cap, (int)k, out_idx, out_err, w.stats);
    })
    if (int rc = check_launch(label)) return rc;
  }
  return CMVE_OK;
}

// ... with l2t_threshold_kernel as launch A' (K20, K23); rho: the canonical chain's relative slack in distance space
template <int METRIC, typename Own, typename Pass>
static inline int l2t_topk_run(const char* name, const char* label, cmve_handle_t h, const FltRows& r, double alpha,
                               double beta, int32_t k, int64_t cand_cap, int64_t sample_rows, void* ws,
                               int64_t ws_bytes, int64_t* out_idx, double* out_err, int64_t* stats, double rho,
                               Own own_checks, Pass pass_launch) {
  auto thr_launch = [&](hipStream_t st, int64_t nq, int64_t ns, const L2tWs& w) {
    hipLaunchKernelGGL(l2t_threshold_kernel<METRIC == CMVE_PW_L2>, dim3((unsigned)nq), dim3(256), 0, st,
                       (const float*)w.ub, w.ub_ld, ns, (int)k, alpha, beta, rho, w.thr, w.cnt);
  };
  return l2t_topk_run<METRIC>(name, label, h, r, alpha, beta, k, cand_cap, sample_rows, ws, ws_bytes, out_idx, out_err,
                              stats, own_checks, pass_launch, thr_launch);
}

}  // namespace cmve
#endif
