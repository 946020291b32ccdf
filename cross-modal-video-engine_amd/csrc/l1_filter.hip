// K22: the count pass of K18 under the L1 measures (l1 / l1_norm: CMVE_PW_L1, fp64 score words) from an integer SAD
// filter -- what
//   LINAS-engine/evaluation.py:24-29 + util/metrics.py:61-157   cal_error(measure) -> eval_q2m's argsort loop /
//                                                               t2v_map / v2t_map
// decide per pair.  Both sets are quantised to uint16 codes on one grid (lo, s); sum_k |xa_k - xb_k| of the decoded
// rows is s * SAD(qa, qb) exactly, the SAD comes from v_sad_u16 (two elements per lane-instruction, exact in u32 for
// d <= 65,536), and the triangle inequality bounds the true distance within the two rows' quantisation errors of it.
// Every comparison  e(i, j) < item score  whose two sides lie further apart than that interval (and than every
// rounding of the canonical chain, DESIGN s4 "K22") is decided from the SAD; the other pairs -- the band -- are
// appended to a caller-owned list and re-scored on the canonical chain of pairwise_tile.h by K19's fix-up kernel, and
// a list that overflows is resolved on the device by K21's gated launches: the counts are, word for word,
// cmve_pairwise_count's, with no host read in between.
//   l1f_grid_kernel  min / max of the eligible elements into the two grid words (integer atomics on the words' bits:
//                    order-independent), accumulating so that two sets can share one grid
//   l1f_pack_kernel  rows -> codes in the tiled order of l1_filter_tile.h, and the rows' errors
//   l1f_main_kernel  128 x 128 tile, 256 threads of 8 x 8 u32 accumulators: the SADs are l1f_sad_tile's
//                    (l1_filter_tile.h; the one K loop, shared with K23's l1t_pass_kernel); fp64 epilogue as
//                    l2f_main_kernel's: interval test against each item, band append, counts (shuffle / LDS partial
//                    sums, one integer atomic per (item, tile): bit-reproducible)
#include "filter_count.h"
#include "l1_filter_tile.h"

namespace cmve {
namespace {

// ---- the grid ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void l1f_grid_init_kernel(double* __restrict__ grid) {
  if (threadIdx.x == 0) {
    grid[0] = __builtin_huge_val();
    grid[1] = -__builtin_huge_val();
  }
}

// min / max of finite doubles (never -0.0) through integer atomics on their bits: a non-negative double orders as
// its signed word, a negative one in reverse as its unsigned word, and every negative word lies below every
// non-negative one as signed and above it as unsigned
__device__ __forceinline__ void l1f_min_word(double* p, double x) {
  if (x >= 0.0) gmin((long long*)p, (long long)__double_as_longlong(x));
  else gmax((unsigned long long*)p, (unsigned long long)__double_as_longlong(x));
}
__device__ __forceinline__ void l1f_max_word(double* p, double x) {
  if (x >= 0.0) gmax((long long*)p, (long long)__double_as_longlong(x));
  else gmin((unsigned long long*)p, (unsigned long long)__double_as_longlong(x));
}

template <typename T>
__global__ __launch_bounds__(256) void l1f_grid_kernel(const T* __restrict__ X, int64_t ld, int64_t n, int64_t d,
                                                       double* __restrict__ grid) {
  double mn = __builtin_huge_val(), mx = -__builtin_huge_val();
  for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
    const T* row = X + i * ld;
    for (int64_t k = threadIdx.x; k < d; k += 256) {
      const double x = (double)row[k] + 0.0;  // (-0.0 -> +0.0)
      if (fabs(x) <= L1F_GRID_MAX) {          // false for NaN
        mn = fmin(mn, x);
        mx = fmax(mx, x);
      }
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    mn = fmin(mn, __shfl_xor(mn, o, 64));
    mx = fmax(mx, __shfl_xor(mx, o, 64));
  }
  if ((threadIdx.x & 63) == 0 && mn <= mx) {
    l1f_min_word(grid, mn);
    l1f_max_word(grid + 1, mx);
  }
}

// ---- the pack: a block per tile of 128 rows -----------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void l1f_pack_kernel(const T* __restrict__ X, int64_t ld, int64_t n, int64_t d,
                                                       int64_t d_pad, const double* __restrict__ grid,
                                                       uint32_t* __restrict__ codes, double* __restrict__ err) {
  __shared__ __attribute__((aligned(4))) uint16_t sq[L1F_BM][L1F_BK + 2];  // 17-dword rows: the dword reads are conflict-free
  double lo, s;
  l1f_grid_of(grid, lo, s);
  const int tid = threadIdx.x, kk = tid & 31, r0 = tid >> 5;  // element kk of rows r0 + 8 it
  const int64_t i0 = (int64_t)blockIdx.x * L1F_BM, nkt = d_pad / L1F_BK;
  double e[16];
#pragma unroll
  for (int it = 0; it < 16; ++it) e[it] = 0.0;
  for (int64_t kt = 0; kt < nkt; ++kt) {
    const int64_t k = kt * L1F_BK + kk;
#pragma unroll
    for (int it = 0; it < 16; ++it) {
      const int r = r0 + 8 * it;
      const int64_t i = i0 + r;
      uint32_t q = 0;  // the padding's code, in both sets
      if (i < n && k < d) {
        const double x = (double)X[i * ld + k];
        q = (uint32_t)fmin(fmax(rint((x - lo) / s), 0.0), 65535.0);  // (NaN -> 0)
        // |x - (lo + s q)| <= df (1 + u) + u |xh| (1 + u) + 2^-1075: the subtraction's rounding and the decode's
        const double xh = l1f_decode(q, lo, s);
        const double df = fabs(x - xh);
        const double term = df + (2.0 * L2F_U) * (df + fabs(xh)) + 1e-300;
        e[it] += fabs(x) <= L1F_X_MAX ? term : __builtin_huge_val();  // NaN, inf, huge: the row has no interval
      }
      sq[r][kk] = (uint16_t)q;
    }
    __syncthreads();
    uint32_t* out = codes + ((int64_t)blockIdx.x * nkt + kt) * L1F_TILE_DW;
#pragma unroll
    for (int it = 0; it < L1F_TILE_DW / 256; ++it) {
      const int idx = it * 256 + tid, kd = idx >> 7, row = idx & 127;
      out[idx] = *(const uint32_t*)&sq[row][2 * kd];
    }
    __syncthreads();
  }
  // the row's error: its 32 threads' partial sums (a fixed order: reproducible), rounded up past every rounding of
  // the terms and of the sum of d of them
  const double up = 1.0 + 4.0 * ((double)d + 8.0) * L2F_U;
#pragma unroll
  for (int it = 0; it < 16; ++it) {
    double v = e[it];
    v += __shfl_xor(v, 1, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 4, 64);
    v += __shfl_xor(v, 8, 64);
    v += __shfl_xor(v, 16, 64);
    const int64_t i = i0 + r0 + 8 * it;
    if (kk == 0 && i < n) err[i] = v * up + 1e-300;
  }
}

// ---- the count -----------------------------------------------------------------------------------------------------------
struct L1fArgs {
  const uint32_t* a_codes;  // tiled (l1_filter_tile.h)
  const uint32_t* b_codes;
  const double* a_err;
  const double* b_err;
  const double* grid;
  int64_t na, nb;
  int nkt;  // K tiles
  double alpha, beta, rho, lim;
  const int64_t* row_off;
  const double* row_sc;
  int32_t* row_pos;
  const int64_t* col_off;
  const double* col_sc;
  int32_t* col_pos;
  int2* band;
  int64_t cap;
  l2f_u64* stats;  // {decided, band found, band re-scored, overflow}
  int tiles_a, tiles_b;
};

// the epilogue's LDS, laid over the staging buffers once the K loop is done
struct L1fEpi {
  double ae[L1F_BM], be[L1F_BN];                              // row errors of the tile's rows / columns
  double rtb[L1F_BM], rtn[L1F_BM], ctb[L1F_BN], ctn[L1F_BN];  // one round's thresholds (below / not-below)
  int64_t ro[L1F_BM], co[L1F_BN];
  int mr[L1F_BM], mc[L1F_BN];
  int rc[L1F_BM], cc[L1F_BN];
  int s_m[2];
  int band_cnt;
  long long band_base;
  double s;  // the grid's step, re-read per row of a round (see the epilogue)
};
static_assert(sizeof(L1fEpi) <= L1F_SMEM, "the epilogue's LDS fits the staging buffers");

__global__ __launch_bounds__(256, 4) void l1f_main_kernel(L1fArgs a) {
  __shared__ __attribute__((aligned(16))) char smem[L1F_SMEM];
  const int tid = threadIdx.x, lane = tid & 63, tx = tid & 15, ty = tid >> 4;
  int ta, tb_;
  l2f_tile_of_block(blockIdx.x, a.tiles_a, a.tiles_b, ta, tb_);
  const int64_t i0 = (int64_t)ta * L1F_BM, j0 = (int64_t)tb_ * L1F_BN;

  // ---- the SADs: acc[u][v] of the pair (A row i0 + l1f_row(ty, u), B row j0 + l1f_row(tx, v)); the tiles' blocks lie
  // below the sets' n_pad (a multiple of 128) and d_pad: in bounds
  uint32_t acc[8][8];
  l1f_sad_tile(a.a_codes + (int64_t)ta * a.nkt * L1F_TILE_DW, a.b_codes + (int64_t)tb_ * a.nkt * L1F_TILE_DW, a.nkt,
               smem, acc);

  // ---- epilogue (every wave has passed the loop's last barrier: smem is free) ------------------------------------------
  L1fEpi& E = *(L1fEpi*)smem;
  if (tid < 2) E.s_m[tid] = 0;
  if (tid == 2) E.band_cnt = 0;
  if (tid == 3) {
    double lo_unused, s;
    l1f_grid_of(a.grid, lo_unused, s);
    E.s = s;
  }
  __syncthreads();
  if (tid < L1F_BM) {
    const int64_t i = i0 + tid;
    const bool v = i < a.na;
    E.ae[tid] = v ? a.a_err[i] : (double)NAN;  // a row beyond the set: no interval
    const int64_t o = (v && a.row_pos) ? a.row_off[i] : 0;
    const int m = (v && a.row_pos) ? (int)(a.row_off[i + 1] - o) : 0;
    E.ro[tid] = o;
    E.mr[tid] = m;
    E.rc[tid] = 0;
    if (m) atomicMax(&E.s_m[0], m);
  } else {
    const int t = tid - L1F_BM;
    const int64_t j = j0 + t;
    const bool v = j < a.nb;
    E.be[t] = v ? a.b_err[j] : (double)NAN;
    const int64_t o = (v && a.col_pos) ? a.col_off[j] : 0;
    const int m = (v && a.col_pos) ? (int)(a.col_off[j + 1] - o) : 0;
    E.co[t] = o;
    E.mc[t] = m;
    E.cc[t] = 0;
    if (m) atomicMax(&E.s_m[1], m);
  }
  __syncthreads();
  const int rounds = max(E.s_m[0], E.s_m[1]);  // block-uniform
  // bit u * 8 + v of `valid`: the pair exists
  uint64_t valid = 0, band = 0;
#pragma unroll
  for (int u = 0; u < 8; ++u)
#pragma unroll
    for (int v = 0; v < 8; ++v)
      if (i0 + l1f_row(ty, u) < a.na && j0 + l1f_row(tx, v) < a.nb) valid |= 1ull << (u * 8 + v);

  // one round: item `it` of every row and column list.  PASS 0 marks the pairs some item cannot decide, PASS 1
  // counts the decided ones.
  for (int pass = 0; pass < 2; ++pass) {
    for (int it = 0; it < rounds; ++it) {
      if (tid < L1F_BM) {
        double tb = (double)NAN, tn = (double)NAN;
        const bool has = it < E.mr[tid];
        if (has) l2f_thresholds<false>(a.row_sc[E.ro[tid] + it], a.alpha, a.beta, a.rho, tb, tn);
        E.rtb[tid] = tb;
        E.rtn[tid] = tn;
      } else {
        const int t = tid - L1F_BM;
        double tb = (double)NAN, tn = (double)NAN;
        const bool has = it < E.mc[t];
        if (has) l2f_thresholds<false>(a.col_sc[E.co[t] + it], a.alpha, a.beta, a.rho, tb, tn);
        E.ctb[t] = tb;
        E.ctn[t] = tn;
      }
      __syncthreads();
      const bool pos = a.alpha > 0.0;
      int ccnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      int rpack[2] = {0, 0};  // four rows' counts each, a byte a row (<= 8 per thread, <= 128 over the row's 16 lanes)
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int row = l1f_row(ty, u);
        // a volatile read: the 64 intervals are formed again in every round, eight at a time, instead of being
        // hoisted out of the rounds as 128 live doubles per thread
        const double s = *(const volatile double*)&E.s;
        const double ae = E.ae[row], rtb = E.rtb[row], rtn = E.rtn[row];
        const bool rhas = it < E.mr[row];
        int rcnt = 0;
#pragma unroll
        for (int v = 0; v < 8; ++v) {
          const int col = l1f_row(tx, v);
          const int bit = u * 8 + v;
          double dlo, dhi;
          l1f_interval(acc[u][v], s, ae, E.be[col], a.lim, dlo, dhi);
          const bool chas = it < E.mc[col];
          const double ctb = E.ctb[col], ctn = E.ctn[col];
          const bool rb = pos ? dhi < rtb : dlo > rtb, rn = pos ? dlo > rtn : dhi < rtn;
          const bool cb = pos ? dhi < ctb : dlo > ctb, cn = pos ? dlo > ctn : dhi < ctn;
          if (pass == 0) {
            // also a pair with no item to compare against must have an interval, so that decided + band = pairs
            const bool okr = rhas ? (rb || rn) : (dlo == dlo);
            const bool okc = chas ? (cb || cn) : (dlo == dlo);
            if (!(okr && okc)) band |= 1ull << bit;
          } else {
            const bool live = ((valid & ~band) >> bit) & 1;
            rcnt += (live && rhas && rb) ? 1 : 0;
            ccnt[v] += (live && chas && cb) ? 1 : 0;
          }
        }
        rpack[u >> 2] += rcnt << (8 * (u & 3));
      }
      if (pass == 1) {
        // rows: the 16 lanes tx = 0..15 of this wave share them
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          int p = rpack[h];
          p += __shfl_xor(p, 1, 64);
          p += __shfl_xor(p, 2, 64);
          p += __shfl_xor(p, 4, 64);
          p += __shfl_xor(p, 8, 64);
          if (tx == 0 && p) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int c = (p >> (8 * r)) & 255;
              if (c) atomicAdd(&E.rc[l1f_row(ty, 4 * h + r)], c);
            }
          }
        }
        // columns: the 4 lane groups of each of the 4 waves share them (<= 8 per thread, <= 32 per wave)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          int p = ccnt[4 * h] | (ccnt[4 * h + 1] << 8) | (ccnt[4 * h + 2] << 16) | (ccnt[4 * h + 3] << 24);
          p += __shfl_xor(p, 16, 64);
          p += __shfl_xor(p, 32, 64);
          if ((lane >> 4) == 0 && p) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int c = (p >> (8 * r)) & 255;
              if (c) atomicAdd(&E.cc[l1f_row(tx, 4 * h + r)], c);
            }
          }
        }
      }
      __syncthreads();
      if (pass == 1) {  // one integer atomic per (item, tile)
        if (tid < L1F_BM) {
          const int c = E.rc[tid];
          if (c && it < E.mr[tid]) gadd(a.row_pos + E.ro[tid] + it, (int32_t)c);
          E.rc[tid] = 0;
        } else {
          const int t = tid - L1F_BM;
          const int c = E.cc[t];
          if (c && it < E.mc[t]) gadd(a.col_pos + E.co[t] + it, (int32_t)c);
          E.cc[t] = 0;
        }
        // (the next round's threshold writes and this read touch different words; its barrier orders the counters)
      }
    }
    if (pass == 0) {
      if (rounds == 0) {  // no list in this tile: nothing to decide, but the pairs without an interval are band
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
          for (int v = 0; v < 8; ++v) {
            double dlo, dhi;
            l1f_interval(acc[u][v], E.s, E.ae[l1f_row(ty, u)], E.be[l1f_row(tx, v)], a.lim, dlo, dhi);
            if (!(dlo == dlo)) band |= 1ull << (u * 8 + v);
          }
      }
      // the band pairs, once each, into the caller's list
      band &= valid;
      const int nband = __popcll(band);
      int my = 0;
      if (nband) my = atomicAdd(&E.band_cnt, nband);
      __syncthreads();
      if (tid == 0) {
        const int total = E.band_cnt;
        const int nv = (int)(min<int64_t>(L1F_BM, a.na - i0) * min<int64_t>(L1F_BN, a.nb - j0));
        long long base = 0;
        if (total) {
          base = (long long)gadd(a.stats + 1, (l2f_u64)total);
          if (base + total > a.cap) gmax(a.stats + 3, (l2f_u64)1);
        }
        if (nv - total) gadd(a.stats + 0, (l2f_u64)(nv - total));
        E.band_base = base;
      }
      __syncthreads();
      if (nband) {
        long long p = E.band_base + my;
        uint64_t b = band;
        while (b) {
          const int bit = __ffsll((long long)b) - 1;
          b &= b - 1;
          if (p < a.cap) a.band[p] = make_int2((int)(i0 + l1f_row(ty, bit >> 3)), (int)(j0 + l1f_row(tx, bit & 7)));
          ++p;
        }
      }
    }
  }
}

}  // namespace
}  // namespace cmve

using namespace cmve;

extern "C" int cmve_l1_pack_size(int64_t n, int64_t d, int64_t* n_pad, int64_t* d_pad) {
  CMVE_REQUIRE(n_pad && d_pad, "cmve_l1_pack_size: NULL argument");
  CMVE_REQUIRE(n >= 0 && n < (1ll << 31) && d > 0 && d <= L1F_D_MAX,
               "cmve_l1_pack_size: bad shape (%lld x %lld; d <= %lld: the u32 SAD is exact up to there)", (long long)n,
               (long long)d, (long long)L1F_D_MAX);
  l1f_pads(n, d, *n_pad, *d_pad);
  return CMVE_OK;
}

extern "C" int cmve_l1_grid(cmve_handle_t h, const void* X, int32_t dtype, int64_t ld, int64_t n, int64_t d,
                            double* grid, int32_t accumulate) {
  CMVE_REQUIRE(h && grid && (X || !n), "cmve_l1_grid: NULL argument");
  CMVE_REQUIRE(n >= 0 && n < (1ll << 31) && d > 0 && d <= L1F_D_MAX && ld >= d, "cmve_l1_grid: bad shape");
  CMVE_REQUIRE(l1f_dtype_ok(dtype), "cmve_l1_grid: rows must be CMVE_F32/CMVE_F64");
  const hipStream_t st = h->stream;
  if (!accumulate) hipLaunchKernelGGL(l1f_grid_init_kernel, dim3(1), dim3(64), 0, st, grid);
  if (n) {
    const unsigned blocks = (unsigned)std::min<int64_t>(n, 8 * (int64_t)device_cus());
    if (dtype == CMVE_F64)
      hipLaunchKernelGGL((l1f_grid_kernel<double>), dim3(blocks), dim3(256), 0, st, (const double*)X, ld, n, d, grid);
    else
      hipLaunchKernelGGL((l1f_grid_kernel<float>), dim3(blocks), dim3(256), 0, st, (const float*)X, ld, n, d, grid);
  }
  return check_launch("l1_grid");
}

extern "C" int cmve_l1_pack(cmve_handle_t h, const void* X, int32_t dtype, int64_t ld, int64_t n, int64_t d,
                            const double* grid, void* codes, int64_t n_pad, int64_t d_pad, double* err) {
  CMVE_REQUIRE(h && grid && (X || !n) && ((codes && err) || !n), "cmve_l1_pack: NULL argument");
  CMVE_REQUIRE(n >= 0 && n < (1ll << 31) && d > 0 && d <= L1F_D_MAX && ld >= d, "cmve_l1_pack: bad shape");
  CMVE_REQUIRE(l1f_dtype_ok(dtype), "cmve_l1_pack: rows must be CMVE_F32/CMVE_F64");
  int64_t np = 0, dp = 0;
  l1f_pads(n, d, np, dp);
  CMVE_REQUIRE(n_pad >= np && n_pad % L1F_BM == 0 && d_pad == dp,
               "cmve_l1_pack: short pad (%lld x %lld given, cmve_l1_pack_size says %lld x %lld)", (long long)n_pad,
               (long long)d_pad, (long long)np, (long long)dp);
  CMVE_REQUIRE((((uintptr_t)codes) & 15) == 0, "cmve_l1_pack: codes must be 16-byte aligned");
  if (n == 0) return CMVE_OK;
  const dim3 grid_dim((unsigned)(np / L1F_BM));
  if (dtype == CMVE_F64)
    hipLaunchKernelGGL((l1f_pack_kernel<double>), grid_dim, dim3(256), 0, h->stream, (const double*)X, ld, n, d, dp, grid,
                       (uint32_t*)codes, err);
  else
    hipLaunchKernelGGL((l1f_pack_kernel<float>), grid_dim, dim3(256), 0, h->stream, (const float*)X, ld, n, d, dp, grid,
                       (uint32_t*)codes, err);
  return check_launch("l1_pack");
}

extern "C" int cmve_l1_count_workspace(int64_t band_cap, int64_t* bytes) {
  CMVE_REQUIRE(bytes, "cmve_l1_count_workspace: NULL argument");
  CMVE_REQUIRE(band_cap >= 0 && band_cap <= INT64_MAX / 8, "cmve_l1_count_workspace: bad band capacity (%lld)",
               (long long)band_cap);
  *bytes = band_cap * (int64_t)sizeof(int2);  // the band list and nothing else: (i, j) per slot
  return CMVE_OK;
}

extern "C" int cmve_l1_count(cmve_handle_t h, const void* A, int32_t a_dtype, int64_t lda, int64_t na,
                             const void* a_codes, const double* a_err, const void* B, int32_t b_dtype, int64_t ldb,
                             int64_t nb, const void* b_codes, const double* b_err, int64_t d, const double* grid,
                             double alpha, double beta, const int64_t* row_off, const double* row_sc,
                             int64_t row_items, int64_t row_n, int32_t* row_pos, const int64_t* col_off,
                             const double* col_sc, int64_t col_items, int64_t col_n, int32_t* col_pos, void* ws,
                             int64_t ws_bytes, int64_t* stats) {
  const char* name = "cmve_l1_count";
  CMVE_REQUIRE(h && stats && (A || !na) && (B || !nb), "%s: NULL argument", name);
  auto own_checks = [&]() -> int {
    CMVE_REQUIRE(d > 0 && d <= L1F_D_MAX, "%s: d must be in [1, %lld] (%lld): the u32 SAD is exact up to there", name,
                 (long long)L1F_D_MAX, (long long)d);
    CMVE_REQUIRE(na >= 0 && nb >= 0 && na < (1ll << 31) && nb < (1ll << 31) && lda >= d && ldb >= d, "%s: bad shape",
                 name);
    CMVE_REQUIRE(l1f_dtype_ok(a_dtype) && l1f_dtype_ok(b_dtype), "%s: rows must be CMVE_F32/CMVE_F64", name);
    CMVE_REQUIRE(grid && ((a_codes && a_err) || !na) && ((b_codes && b_err) || !nb),
                 "%s: the codes, the row errors or the grid are missing (cmve_l1_grid, cmve_l1_pack)", name);
    CMVE_REQUIRE(((((uintptr_t)a_codes) | ((uintptr_t)b_codes)) & 15) == 0, "%s: codes must be 16-byte aligned", name);
    return CMVE_OK;
  };
  auto main_launch = [&](hipStream_t st, const FltArgs& f) {
    int64_t n_pad = 0, d_pad = 0;
    l1f_pads(na, d, n_pad, d_pad);
    // (the kernel's own flat argument block: embedding FltArgs moved its scalar loads and cost the kernel 1.2%)
    const FltLists& l = f.lists;
    const L1fArgs g{(const uint32_t*)a_codes, (const uint32_t*)b_codes, a_err, b_err, grid, f.na, f.nb,
                    (int)(d_pad / L1F_BK), f.alpha, f.beta,
                    2.0 * ((double)d + 16.0) * L2F_U,    // rho: DESIGN s4 (K22)
                    (1e300 - fabs(beta)) / fabs(alpha),  // lim: below it alpha * S + beta cannot overflow
                    l.row_off, l.row_sc, l.row_pos, l.col_off, l.col_sc, l.col_pos, f.band.band, f.band.cap,
                    f.band.stats, f.tiles_a, f.tiles_b};
    hipLaunchKernelGGL(l1f_main_kernel, dim3((unsigned)(f.tiles_a * f.tiles_b)), dim3(256), 0, st, g);
  };
  // (resolve: an overflowing list is resolved on the device, from the start -- no entry leaves it to the host)
  return flt_count_run(name, "l1_count", h, CMVE_PW_L1, FltRows{A, a_dtype, lda, na, B, b_dtype, ldb, nb, d}, alpha, beta,
                       {row_off, row_sc, row_items, row_n, row_pos, col_off, col_sc, col_items, col_n, col_pos}, ws,
                       ws_bytes, stats, true, own_checks, main_launch);
}
