// K23: cmve_pairwise_topk under the L1 measures (l1 / l1_norm: CMVE_PW_L1, fp64 score words) at the integer SAD rate
// -- what
//   LINAS-engine/inference.py:78-80      cal_error(video_embs, cap_emb, measure) -> np.argsort(errors[0])[:topK]
//   LINAS-engine/evaluation.py:22-35     cal_error under l1 / l1_norm
// compute per caption.  The k smallest errors are the k smallest keys  s L,  s = sign(alpha), L the true L1 distance
// of the pair (no square); K22's SAD of the uint16 codes (l1_filter_tile.h) brackets every pair's L, so K20's scheme
// (l2_topk.hip, topk_filter_tile.h) carries over launch by launch:
//   launch A   l1t_pass_kernel<0>        the SAD tile over the first `sample_rows` gallery rows; the epilogue stores
//                                        every pair's UPPER key bound (fp32, rounded up; +inf without an interval)
//   launch A'  l2t_threshold_kernel<false>  the k-th smallest stored bound per query, widened to an L1-distance
//                                        threshold beyond which a column's canonical word is STRICTLY worse than
//                                        every witness's (DESIGN s4, "K23")
//   launch B   l1t_pass_kernel<1>        the same tile over the whole gallery; a pair without an interval, or whose
//                                        lower key bound does not clear the threshold, is appended to its query's
//                                        candidate list (integer atomic counter)
//   launch C   l2t_finish_kernel<CMVE_PW_L1>  a block per query: the candidates on the canonical chain, sorted, k
//                                        emitted
// so out_idx / out_err are, word for word, cmve_pairwise_topk's.  The grid offset lo cancels in the SAD: rows
// clustered far from the origin keep intervals as tight as rows around it.  Plain vector stores and integer atomics
// only.
#include "l1_filter_tile.h"
#include "topk_filter_tile.h"

namespace cmve {
namespace {

struct L1tArgs {
  const uint32_t* q_codes;  // tiled (l1_filter_tile.h)
  const uint32_t* g_codes;
  const double* q_err;
  const double* g_err;
  const double* grid;
  int64_t q0, q_end;  // this round's queries; q0 is a multiple of 128
  int64_t ng;         // columns of this pass: the sample (A) or the gallery (B)
  int nkt;            // K tiles
  double alpha, lim;
  float* ub;          // A: [q_end - q0][ub_ld] upper key bounds
  int64_t ub_ld;
  const double* thr;  // B: per query the L1-distance threshold (NaN: unresolved, nothing is appended)
  int32_t* cnt;       // B: candidates found per query
  int32_t* list;      // B: [q_end - q0][cap] column ids
  int64_t cap;
  l2f_u64* stats;     // {pairs excluded, candidates found, candidates re-scored, unresolved queries}
  int tiles_a, tiles_b;
};

// the epilogue's LDS, laid over the staging buffers once the K loop is done
struct L1tEpi {
  double qe[L1F_BM], ge[L1F_BN];  // row errors of the tile's rows / columns
  double thr[L1F_BM];
  int full[L1F_BM];  // the row's list had overflowed when this tile began: its candidates are counted, not appended
  int n_cand, n_excl;
  double s;  // the grid's step
};
static_assert(sizeof(L1tEpi) <= L1F_SMEM, "the epilogue's LDS fits the staging buffers");

// thread (ty, tx) = (tid >> 4, tid & 15) owns the query rows l1t_row(ty, u) and the gallery rows l1t_row(tx, v) of the
// tile, u, v < 8: l1f_main_kernel's layout (two runs of four consecutive rows 64 apart)
__device__ __forceinline__ int l1t_row(int t, int u) { return (u >> 2) * 64 + t * 4 + (u & 3); }

// MODE 0: launch A (the witnesses' bounds), MODE 1: launch B (the candidates)
template <int MODE>
__global__ __launch_bounds__(256, 4) void l1t_pass_kernel(L1tArgs a) {
  __shared__ __attribute__((aligned(16))) char smem[L1F_SMEM];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  int ta, tb_;
  l2f_tile_of_block(blockIdx.x, a.tiles_a, a.tiles_b, ta, tb_);
  // q0 is a multiple of 128: the round's tile ta is tile q0 / 128 + ta of the tiled codes.  Both sets hold n_pad (a
  // multiple of 128) rows and d_pad elements: the tiles' blocks are in bounds.
  const int64_t qt = a.q0 / L1F_BM + ta;
  const int64_t i0 = qt * L1F_BM, j0 = (int64_t)tb_ * L1F_BN;

  // ---- the SADs.  This K loop is a COPY of l1f_main_kernel's (l1_filter.hip): the count kernel is tuned on its own
  // instruction stream and is not touched; a change to either loop is made in both.
  uint32_t acc[8][8];
#pragma unroll
  for (int u = 0; u < 8; ++u)
#pragma unroll
    for (int v = 0; v < 8; ++v) acc[u][v] = 0u;
  constexpr int Q = L1F_TILE_DW / 4;  // 16-byte pieces of a block: two per thread
  const l2f_u32x4* ga = (const l2f_u32x4*)(a.q_codes + qt * a.nkt * L1F_TILE_DW) + tid;
  const l2f_u32x4* gb = (const l2f_u32x4*)(a.g_codes + (int64_t)tb_ * a.nkt * L1F_TILE_DW) + tid;
  l2f_u32x4 ra[2], rb[2];
#define L1T_LOAD(kt)                                      \
  {                                                       \
    ra[0] = ga[(int64_t)(kt) * Q];                        \
    ra[1] = ga[(int64_t)(kt) * Q + 256];                  \
    rb[0] = gb[(int64_t)(kt) * Q];                        \
    rb[1] = gb[(int64_t)(kt) * Q + 256];                  \
  }
#define L1T_WRITE(buf)                                                             \
  {                                                                                \
    char* w_ = smem + (buf) * L1F_STAGE + tid * 16;                                \
    *(l2f_u32x4*)(w_) = ra[0];                                                     \
    *(l2f_u32x4*)(w_ + 4096) = ra[1];                                              \
    *(l2f_u32x4*)(w_ + L1F_TILE_DW * 4) = rb[0];                                   \
    *(l2f_u32x4*)(w_ + L1F_TILE_DW * 4 + 4096) = rb[1];                            \
  }
  L1T_LOAD(0)
  L1T_WRITE(0)
  __syncthreads();
  for (int kt = 0; kt < a.nkt; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < a.nkt) L1T_LOAD(kt + 1)
    const char* pa = smem + buf * L1F_STAGE + ty * 16;
    const char* pb = smem + buf * L1F_STAGE + L1F_TILE_DW * 4 + tx * 16;
#pragma unroll 2
    for (int kd = 0; kd < L1F_KD; ++kd) {
      const l2f_u32x4 a0 = *(const l2f_u32x4*)(pa + kd * 512), a1 = *(const l2f_u32x4*)(pa + kd * 512 + 256);
      const l2f_u32x4 b0 = *(const l2f_u32x4*)(pb + kd * 512), b1 = *(const l2f_u32x4*)(pb + kd * 512 + 256);
      const uint32_t av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
      const uint32_t bv[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
      for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int v = 0; v < 8; ++v) acc[u][v] = __builtin_amdgcn_sad_u16(av[u], bv[v], acc[u][v]);
    }
    if (kt + 1 < a.nkt) L1T_WRITE(buf ^ 1)
    __syncthreads();
  }
#undef L1T_LOAD
#undef L1T_WRITE

  // ---- epilogue (every wave has passed the loop's last barrier: smem is free): one threshold per row, no rounds ----
  L1tEpi& E = *(L1tEpi*)smem;
  if (tid < L1F_BM) {
    const int64_t i = i0 + tid;
    const bool v = i < a.q_end;
    E.qe[tid] = v ? a.q_err[i] : (double)NAN;  // a row beyond the round: no interval (and never used)
    if (MODE == 1) {
      E.thr[tid] = v ? a.thr[i - a.q0] : (double)NAN;
      // K20's read (l2_topk.hip): a row whose list has overflowed stops appending -- once per row and tile, off the
      // pairs' path; the counter only grows, so a tile that reads it early merely adds its own <= 128 candidates more
      E.full[tid] = v ? __hip_atomic_load(a.cnt + (i - a.q0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > a.cap : 1;
    }
  } else {
    const int t = tid - L1F_BM;
    const int64_t j = j0 + t;
    E.ge[t] = j < a.ng ? a.g_err[j] : (double)NAN;
  }
  if (tid == 0) {
    E.n_cand = E.n_excl = 0;
    double lo_unused, s;
    l1f_grid_of(a.grid, lo_unused, s);
    E.s = s;
  }
  __syncthreads();
  const bool pos = a.alpha > 0.0;
  const double s = E.s;
  int n_cand = 0, n_excl = 0;
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int64_t i = i0 + l1t_row(ty, u);
    const double qe = E.qe[l1t_row(ty, u)];
    const double thr = MODE == 1 ? E.thr[l1t_row(ty, u)] : 0.0;
    const bool full = MODE == 1 ? E.full[l1t_row(ty, u)] != 0 : false;
    const int64_t li = i - a.q0;
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      const int64_t j = j0 + l1t_row(tx, v);
      if (i >= a.q_end || j >= a.ng) continue;
      double dlo, dhi;
      l1f_interval(acc[u][v], s, qe, E.ge[l1t_row(tx, v)], a.lim, dlo, dhi);
      if (MODE == 0) {
        // key = s L: its upper bound is dhi (alpha > 0) or -dlo (alpha < 0); NaN (no interval) becomes +inf
        a.ub[li * a.ub_ld + j] = l2t_f32_up(pos ? dhi : -dlo);
      } else if (thr == thr) {
        // excluded only on a positive test: L is provably beyond the threshold (a NaN interval fails it)
        const bool out = pos ? dlo > thr : dhi < thr;
        if (out) {
          ++n_excl;
        } else {
          ++n_cand;
          if (!full) {
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

}  // namespace
}  // namespace cmve

using namespace cmve;

extern "C" int cmve_l1_topk_workspace(int64_t n_q, int64_t n_g, int32_t k, int64_t cand_cap, int64_t sample_rows,
                                      int64_t* bytes) {
  CMVE_REQUIRE(bytes, "cmve_l1_topk_workspace: NULL argument");
  if (int rc = l2t_check_params("cmve_l1_topk_workspace", k, cand_cap, sample_rows)) return rc;
  CMVE_REQUIRE(n_q >= 0 && n_g >= 0 && n_q < (1ll << 31) && n_g < (1ll << 31),
               "cmve_l1_topk_workspace: bad shape (%lld, %lld rows)", (long long)n_q, (long long)n_g);
  *bytes = l2t_layout(n_q, n_g, k, cand_cap, sample_rows).bytes;
  return CMVE_OK;
}

extern "C" int cmve_l1_topk(cmve_handle_t h, const void* Q, int32_t q_dtype, int64_t ldq, int64_t n_q,
                            const void* q_codes, const double* q_err, const void* G, int32_t g_dtype, int64_t ldg,
                            int64_t n_g, const void* g_codes, const double* g_err, int64_t d, const double* grid,
                            double alpha, double beta, int32_t k, int64_t cand_cap, int64_t sample_rows, void* ws,
                            int64_t ws_bytes, int64_t* out_idx, double* out_err, int64_t* stats) {
  const char* name = "cmve_l1_topk";
  CMVE_REQUIRE(h && stats && (Q || !n_q) && (G || !n_g), "%s: NULL argument", name);
  CMVE_REQUIRE(alpha != 0.0 && std::isfinite(alpha) && std::isfinite(beta),
               "%s: alpha must be finite and non-zero, beta finite (%g, %g)", name, alpha, beta);
  if (int rc = l2t_check_params(name, k, cand_cap, sample_rows)) return rc;
  CMVE_REQUIRE(d > 0 && d <= L1F_D_MAX, "%s: d must be in [1, %lld] (%lld): the u32 SAD is exact up to there", name,
               (long long)L1F_D_MAX, (long long)d);
  CMVE_REQUIRE(n_q >= 0 && n_g >= 0 && n_q < (1ll << 31) && n_g < (1ll << 31) && ldq >= d && ldg >= d,
               "%s: bad shape", name);
  CMVE_REQUIRE(l1f_dtype_ok(q_dtype) && l1f_dtype_ok(g_dtype), "%s: rows must be CMVE_F32/CMVE_F64", name);
  CMVE_REQUIRE(grid && ((q_codes && q_err) || !n_q) && ((g_codes && g_err) || !n_g),
               "%s: the codes, the row errors or the grid are missing (cmve_l1_grid, cmve_l1_pack)", name);
  CMVE_REQUIRE(((((uintptr_t)q_codes) | ((uintptr_t)g_codes)) & 15) == 0, "%s: codes must be 16-byte aligned", name);
  CMVE_REQUIRE(k <= n_g || n_q == 0, "%s: k exceeds the gallery (%d > %lld): clamp it", name, k, (long long)n_g);
  CMVE_REQUIRE((out_idx && out_err) || !n_q, "%s: NULL output", name);
  const L2tLayout l = l2t_layout(n_q, n_g, k, cand_cap, sample_rows);
  CMVE_REQUIRE(n_q == 0 || (ws && ws_bytes >= l.bytes), "%s: workspace too small (%lld < %lld bytes)", name,
               (long long)ws_bytes, (long long)l.bytes);
  CMVE_REQUIRE((((uintptr_t)ws) & 7) == 0, "%s: workspace must be 8-byte aligned", name);
  const hipStream_t st = h->stream;
  CMVE_HIP(hipMemsetAsync(stats, 0, 4 * sizeof(int64_t), st));
  if (n_q == 0) return CMVE_OK;
  int64_t n_pad = 0, d_pad = 0;
  l1f_pads(n_q, d, n_pad, d_pad);
  L1tArgs a;
  a.q_codes = (const uint32_t*)q_codes;
  a.g_codes = (const uint32_t*)g_codes;
  a.q_err = q_err;
  a.g_err = g_err;
  a.grid = grid;
  a.nkt = (int)(d_pad / L1F_BK);
  a.alpha = alpha;
  a.lim = (1e300 - fabs(beta)) / fabs(alpha);  // below it alpha * S + beta cannot overflow (as cmve_l1_count)
  a.ub = (float*)((char*)ws + l.ub);
  a.ub_ld = l.ub_ld;
  double* thr = (double*)((char*)ws + l.thr);
  a.thr = thr;
  a.cnt = (int32_t*)((char*)ws + l.cnt);
  a.list = (int32_t*)((char*)ws + l.list);
  a.cap = cand_cap;
  a.stats = (l2f_u64*)stats;
  const double rho = 2.0 * ((double)d + 16.0) * L2F_U;  // DESIGN s4 (K22)
  const int64_t tiles_s = (l.s + L1F_BN - 1) / L1F_BN, tiles_g = (n_g + L1F_BN - 1) / L1F_BN;
  for (int64_t q0 = 0; q0 < n_q; q0 += l.qc) {
    const int64_t nq = std::min(l.qc, n_q - q0);
    a.q0 = q0;
    a.q_end = q0 + nq;
    a.tiles_a = (int)((nq + L1F_BM - 1) / L1F_BM);  // <= 8: tiles_a * tiles_g < 2^31
    a.ng = l.s;
    a.tiles_b = (int)tiles_s;
    hipLaunchKernelGGL(l1t_pass_kernel<0>, dim3((unsigned)(a.tiles_a * tiles_s)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(l2t_threshold_kernel<false>, dim3((unsigned)nq), dim3(256), 0, st, (const float*)a.ub, a.ub_ld,
                       l.s, (int)k, alpha, beta, rho, thr, a.cnt);
    a.ng = n_g;
    a.tiles_b = (int)tiles_g;
    hipLaunchKernelGGL(l1t_pass_kernel<1>, dim3((unsigned)(a.tiles_a * tiles_g)), dim3(256), 0, st, a);
    PWR_TYPES(q_dtype, g_dtype, TA, TB, {
      hipLaunchKernelGGL((l2t_finish_kernel<CMVE_PW_L1, TA, TB>), dim3((unsigned)nq), dim3(256), 0, st, (const TA*)Q,
                         ldq, (const TB*)G, ldg, d, alpha, beta, q0, (const double*)thr, (const int32_t*)a.cnt,
                         (const int32_t*)a.list, cand_cap, (int)k, out_idx, out_err, a.stats);
    })
    if (int rc = check_launch("l1_topk")) return rc;
  }
  return CMVE_OK;
}
