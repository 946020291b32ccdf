// K20: cmve_pairwise_topk under the Euclidean measures (euclidean / l2 / l2_norm: CMVE_PW_L2, fp64 score words) at
// the MFMA rate -- what
//   LINAS-engine/inference.py:78-80      cal_error(video_embs, cap_emb, measure) -> np.argsort(errors[0])[:topK]
//   LINAS-engine/evaluation.py:22-35     cal_error under euclidean / l2 / l2_norm
// compute per caption.  The k smallest errors are the k smallest keys  s D,  s = sign(alpha), D the true squared
// distance of the pair; K19's fp16 MFMA cosine (l2_filter_tile.h) brackets every pair's key, so
//   launch A   l2t_pass_kernel<0>     the MFMA pass over the first `sample_rows` gallery rows; the epilogue stores every
//                                     pair's UPPER key bound (fp32, rounded up; +inf for a pair without an interval)
//   launch A'  l2t_threshold_kernel   per query the k-th smallest stored bound tau (radix select: k distinct columns --
//                                     the witnesses -- have a true key <= tau), widened to a squared-distance threshold
//                                     beyond which a column's canonical word is STRICTLY worse than every witness's
//                                     (DESIGN s4, "K20"); a query without k finite bounds is unresolved
//   launch B   l2t_pass_kernel<1>     the same pass over the whole gallery; a pair without an interval, or whose lower
//                                     key bound does not clear the threshold, is appended to its query's candidate
//                                     list (integer atomic counter; the order of a list does not matter)
//   launch C   l2t_finish_kernel      a block per query: every candidate re-scored on the canonical chain of
//                                     pairwise_tile.h (l2f_chain64, as K19's fix-up), sorted in LDS by (word asc with
//                                     NaN last, -0 == +0, id asc), the first k emitted
// so out_idx / out_err are, word for word, cmve_pairwise_topk's.  A query whose list overflows, or that has no
// threshold, gets out_idx[i, 0] = -2: the caller finishes it on the fp64 route.  Plain vector stores and integer
// atomics only; the queries are taken L2T_QC at a time so that the workspace has no n_q x n_g term.
#include "l2_filter_tile.h"

namespace cmve {
namespace {

constexpr int L2T_QC = 1024;        // queries per round of the four launches
constexpr int L2T_CAND_MAX = 2048;  // candidates launch C sorts in LDS: 12 bytes each beside l2f_chain64's staging

struct L2tArgs {
  const uint16_t* q16;  // [nq_pad, d_pad] fp16 unit rows
  const uint16_t* g16;
  const double* q_inv;  // 1 / ||row||
  const double* g_inv;
  const float* q_err;   // >= || x_hat - h16 ||
  const float* g_err;
  int64_t q0, q_end;    // this round's queries
  int64_t ng;           // columns of this pass: the sample (A) or the gallery (B)
  int64_t d_pad;
  double alpha;
  L2fConsts c;
  float* ub;            // A: [q_end - q0][ub_ld] upper key bounds
  int64_t ub_ld;
  const double* thr;    // B: per query the squared-distance threshold (NaN: unresolved, nothing is appended)
  int32_t* cnt;         // B: candidates found per query
  int32_t* list;        // B: [q_end - q0][cap] column ids
  int64_t cap;
  l2f_u64* stats;       // {pairs excluded, candidates found, candidates re-scored, unresolved queries}
  int tiles_a, tiles_b;
};

// the epilogue's LDS, laid over the staging buffers once the K loop is done
struct L2tEpi {
  double qn[L2F_BM], qe[L2F_BM], gn[L2F_BN], ge[L2F_BN];  // norms and row errors of the tile's rows / columns
  double thr[L2F_BM];
  int full[L2F_BM];  // the row's list had overflowed when this tile began: its candidates are counted, not appended
  int n_cand, n_excl;
};
static_assert(sizeof(L2tEpi) <= L2F_SMEM, "the epilogue's LDS fits the staging buffers");

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

// MODE 0: launch A (the witnesses' bounds), MODE 1: launch B (the candidates)
template <int MODE>
__global__ __launch_bounds__(256, 2) void l2t_pass_kernel(L2tArgs a) {
  __shared__ __attribute__((aligned(16))) char smem[L2F_SMEM];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, fr = lane & 15, fq = lane >> 4;
  int ta, tb_;
  l2f_tile_of_block(blockIdx.x, a.tiles_a, a.tiles_b, ta, tb_);
  // q0 is a multiple of 128 and both planes hold n_pad (a multiple of 256) rows: the tile's 128 rows are in bounds
  const int64_t i0 = a.q0 + (int64_t)ta * L2F_BM, j0 = (int64_t)tb_ * L2F_BN;
  l2f_f32x4 acc[4][4];
  l2f_gemm_tile(a.q16, a.g16, a.d_pad, i0, j0, smem, acc);

  L2tEpi& E = *(L2tEpi*)smem;
  if (tid < L2F_BM) {
    const int64_t i = i0 + tid;
    const bool v = i < a.q_end;
    E.qn[tid] = l2f_side_norm(i, v, a.q_inv);
    E.qe[tid] = l2f_side_err(i, v, a.q_err, a.c.theta);
    if (MODE == 1) {
      E.thr[tid] = v ? a.thr[i - a.q0] : (double)NAN;
      // An overflowed list is lost (launch C asks only whether the counter exceeds cap), so its row stops appending:
      // rows clustered far from the origin -- every pair a candidate -- would otherwise serialise n_g atomics on
      // one address per query.  Read once per tile, off the pairs' path; the counter only grows, so a tile that
      // reads it early merely adds its own <= 128 candidates more.
      E.full[tid] = v ? __hip_atomic_load(a.cnt + (i - a.q0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > a.cap : 1;
    }
  } else {
    const int t = tid - L2F_BM;
    const int64_t j = j0 + t;
    const bool v = j < a.ng;
    E.gn[t] = l2f_side_norm(j, v, a.g_inv);
    E.ge[t] = l2f_side_err(j, v, a.g_err, a.c.theta);
  }
  if (tid == 0) E.n_cand = E.n_excl = 0;
  __syncthreads();
  const bool pos = a.alpha > 0.0;
  const int rbase = wm * 64 + 4 * fq, cbase = wn * 64 + fr;
  int n_cand = 0, n_excl = 0;
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = rbase + 16 * m + r;
      const int64_t i = i0 + row;
      const double qn = E.qn[row], qe = E.qe[row];
      const double thr = MODE == 1 ? E.thr[row] : 0.0;
      const bool full = MODE == 1 ? E.full[row] != 0 : false;
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        const int col = cbase + 16 * n;
        const int64_t j = j0 + col;
        if (i >= a.q_end || j >= a.ng) continue;
        double dlo, dhi;
        l2f_interval(acc[m][n][r], qn, qe, E.gn[col], E.ge[col], a.c.gamma, a.c.kappa, dlo, dhi);
        if (MODE == 0) {
          // key = s D: its upper bound is dhi (alpha > 0) or -dlo (alpha < 0); NaN (no interval) becomes +inf
          a.ub[(i - a.q0) * a.ub_ld + j] = l2t_f32_up(pos ? dhi : -dlo);
        } else if (thr == thr) {
          // excluded only on a positive test: D is provably beyond the threshold (a NaN interval fails it)
          const bool out = pos ? dlo > thr : dhi < thr;
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
      }
    }
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

// The witnesses' bound tau (key space: k distinct columns have s D <= tau) -> the squared-distance threshold of launch
// B, or NaN when there is none.  DESIGN s4 "K20": pick a score word t just on the far side of the witnesses and let
// K19's l2f_thresholds speak for it.  alpha > 0: every witness has D <= Dt; if tb(t) > Dt each witness's canonical
// word is < t, and a column with D > tn(t) has a word >= t -- strictly worse than k columns' words, so outside the
// top-k whatever its index.  alpha < 0: every witness has D >= Dt = -tau; tb(t) < Dt makes their words < t and a
// column with D < tn(t) has a word >= t.  The condition on tb is CHECKED here, so the slack below is a first guess
// (rho relative on sqrt(D), sigma absolute, as K19 steps 3-4) and not part of the proof.
__device__ double l2t_widen(double tau, double alpha, double beta, double rho) {
  const bool pos = alpha > 0.0;
  if (!(fabs(tau) < __builtin_huge_val())) return (double)NAN;
  const double Dt = pos ? fmax(tau, 0.0) : -tau;
  if (!pos && !(Dt > 0.0)) return (double)NAN;  // the witnesses' distances have no positive lower bound
  const double y = sqrt(Dt);
  double slack = 4.0 * rho * y + 64.0 * L2F_U * (y + 2.0 * fabs(beta) / fabs(alpha)) + 1e-280;
  for (int it = 0; it < 12; ++it) {
    const double yy = pos ? y + slack : y - slack;
    const double t = alpha * yy + beta;
    double tb, tn;
    l2f_thresholds(t, alpha, beta, rho, tb, tn);
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
    thr[blockIdx.x] = l2t_widen((double)__uint_as_float(b), alpha, beta, rho);
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
template <typename TA, typename TB>
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
    const double s = l2f_chain64(Q, ldq, G, ldg, d, (int)gi, j, sd[w], lane);
    if (live) {
      sw[p] = pw_score<CMVE_PW_L2>(s, 0.0, alpha, beta);
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

int64_t l2t_round128(int64_t n) { return (n + 127) / 128 * 128; }

// the sample of launch A: the caller's, or max(k, 8) / 128 of the gallery within [1024, 65536] (the k-th of n_s sampled
// keys leaves about k n_g / n_s <= 128 gallery rows below it: launch C mostly re-scores one round of 256 candidates);
// at least k, a multiple of the tile, at most the gallery
int64_t l2t_sample(int64_t n_g, int32_t k, int64_t sample_rows) {
  int64_t s = sample_rows > 0 ? sample_rows
                              : std::min<int64_t>(65536, std::max<int64_t>(1024, std::max<int64_t>(k, 8) * (n_g / 128)));
  s = l2t_round128(std::max<int64_t>(s, k));
  return std::min(s, std::max<int64_t>(n_g, 1));
}

struct L2tLayout {
  int64_t qc, s, ub_ld, thr, ub, list, cnt, bytes;
};
L2tLayout l2t_layout(int64_t n_q, int64_t n_g, int32_t k, int64_t cand_cap, int64_t sample_rows) {
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

// what both top-k entries ask of k / cand_cap / sample_rows (the refusals name the entry)
int l2t_check_params(const char* name, int32_t k, int64_t cand_cap, int64_t sample_rows) {
  CMVE_REQUIRE(k >= 1, "%s: k must be at least 1 (%d)", name, k);
  CMVE_REQUIRE(cand_cap >= k && cand_cap <= L2T_CAND_MAX, "%s: cand_cap must be in [k, %d] (%lld, k %d)", name,
               L2T_CAND_MAX, (long long)cand_cap, k);
  CMVE_REQUIRE(sample_rows >= 0 && sample_rows < (1ll << 31), "%s: bad sample_rows (%lld)", name,
               (long long)sample_rows);
  return CMVE_OK;
}

}  // namespace
}  // namespace cmve

using namespace cmve;

extern "C" int cmve_l2_topk_workspace(const cmve_rows_t* q, const cmve_rows_t* g, int32_t k, int64_t cand_cap,
                                      int64_t sample_rows, int64_t* bytes) {
  CMVE_REQUIRE(q && g && bytes, "cmve_l2_topk_workspace: NULL argument");
  if (int rc = l2t_check_params("cmve_l2_topk_workspace", k, cand_cap, sample_rows)) return rc;
  CMVE_REQUIRE(q->n >= 0 && g->n >= 0 && q->n < (1ll << 31) && g->n < (1ll << 31) && q->d > 0 && q->d == g->d,
               "cmve_l2_topk_workspace: bad shape (%lld x %lld, %lld x %lld)", (long long)q->n, (long long)q->d,
               (long long)g->n, (long long)g->d);
  *bytes = l2t_layout(q->n, g->n, k, cand_cap, sample_rows).bytes;
  return CMVE_OK;
}

extern "C" int cmve_l2_topk(cmve_handle_t h, const cmve_rows_t* q, const cmve_rows_t* g, double alpha, double beta,
                            int32_t k, int64_t cand_cap, int64_t sample_rows, void* ws, int64_t ws_bytes,
                            int64_t* out_idx, double* out_err, int64_t* stats) {
  CMVE_REQUIRE(h && q && g && stats, "cmve_l2_topk: NULL argument");
  CMVE_REQUIRE(alpha != 0.0 && std::isfinite(alpha) && std::isfinite(beta),
               "cmve_l2_topk: alpha must be finite and non-zero, beta finite (%g, %g)", alpha, beta);
  if (int rc = l2t_check_params("cmve_l2_topk", k, cand_cap, sample_rows)) return rc;
  if (int rc = l2f_check_sets("cmve_l2_topk", q, g)) return rc;
  const int64_t n_q = q->n, n_g = g->n, d = q->d;
  CMVE_REQUIRE(k <= n_g || n_q == 0, "cmve_l2_topk: k exceeds the gallery (%d > %lld): clamp it", k, (long long)n_g);
  CMVE_REQUIRE((out_idx && out_err) || !n_q, "cmve_l2_topk: NULL output");
  const L2tLayout l = l2t_layout(n_q, n_g, k, cand_cap, sample_rows);
  CMVE_REQUIRE(n_q == 0 || (ws && ws_bytes >= l.bytes), "cmve_l2_topk: workspace too small (%lld < %lld bytes)",
               (long long)ws_bytes, (long long)l.bytes);
  CMVE_REQUIRE((((uintptr_t)ws) & 7) == 0, "cmve_l2_topk: workspace must be 8-byte aligned");
  const hipStream_t st = h->stream;
  CMVE_HIP(hipMemsetAsync(stats, 0, 4 * sizeof(int64_t), st));
  if (n_q == 0) return CMVE_OK;
  L2tArgs a;
  a.q16 = q->h16;
  a.g16 = g->h16;
  a.q_inv = q->inv_norm;
  a.g_inv = g->inv_norm;
  a.q_err = q->err_h16;
  a.g_err = g->err_h16;
  a.d_pad = q->d_pad;
  a.alpha = alpha;
  a.c = l2f_consts(d, q->d_pad);
  a.ub = (float*)((char*)ws + l.ub);
  a.ub_ld = l.ub_ld;
  double* thr = (double*)((char*)ws + l.thr);
  a.thr = thr;
  a.cnt = (int32_t*)((char*)ws + l.cnt);
  a.list = (int32_t*)((char*)ws + l.list);
  a.cap = cand_cap;
  a.stats = (l2f_u64*)stats;
  const int64_t tiles_s = (l.s + L2F_BN - 1) / L2F_BN, tiles_g = (n_g + L2F_BN - 1) / L2F_BN;
  for (int64_t q0 = 0; q0 < n_q; q0 += l.qc) {
    const int64_t nq = std::min(l.qc, n_q - q0);
    a.q0 = q0;
    a.q_end = q0 + nq;
    a.tiles_a = (int)((nq + L2F_BM - 1) / L2F_BM);  // <= 8: tiles_a * tiles_g < 2^31
    a.ng = l.s;
    a.tiles_b = (int)tiles_s;
    hipLaunchKernelGGL(l2t_pass_kernel<0>, dim3((unsigned)(a.tiles_a * tiles_s)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(l2t_threshold_kernel, dim3((unsigned)nq), dim3(256), 0, st, (const float*)a.ub, a.ub_ld, l.s,
                       (int)k, alpha, beta, a.c.rho, thr, a.cnt);
    a.ng = n_g;
    a.tiles_b = (int)tiles_g;
    hipLaunchKernelGGL(l2t_pass_kernel<1>, dim3((unsigned)(a.tiles_a * tiles_g)), dim3(256), 0, st, a);
    PWR_TYPES(q->raw_dtype, g->raw_dtype, TA, TB, {
      hipLaunchKernelGGL((l2t_finish_kernel<TA, TB>), dim3((unsigned)nq), dim3(256), 0, st, (const TA*)q->raw,
                         q->raw_ld, (const TB*)g->raw, g->raw_ld, d, alpha, beta, q0, (const double*)thr,
                         (const int32_t*)a.cnt, (const int32_t*)a.list, cand_cap, (int)k, out_idx, out_err, a.stats);
    })
    if (int rc = check_launch("l2_topk")) return rc;
  }
  return CMVE_OK;
}
