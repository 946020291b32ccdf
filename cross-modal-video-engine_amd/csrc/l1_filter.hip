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
//   l1f_main_kernel  sad_count.h's kernel body (128 x 128 tile, 256 threads of 8 x 8 u32 accumulators from
//                    l1f_sad_tile, the one K loop shared with K23's l1t_pass_kernel; fp64 epilogue: interval test
//                    against each item, band append, counts, bit-reproducible) under the policy L1fCount: a row's
//                    error, l2f_thresholds, l1f_interval and its two-bound comparisons
#include "sad_count.h"

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

// ---- the count: sad_count.h's kernel under the L1 policy ----------------------------------------------------------------
struct L1fCount {
  struct Args : SadArgs {
    double rho, lim;
  };
  static constexpr int NS = 1;  // a side carries its row error
  struct Iv {
    double dlo, dhi;
  };
  template <bool B>
  static __device__ __forceinline__ void side(const Args& a, bool v, int64_t i, double, double, double (&t)[NS]) {
    t[0] = v ? (B ? a.b_err : a.a_err)[i] : (double)NAN;  // a row beyond the set: no interval
  }
  // (below / not-below thresholds)
  static __device__ __forceinline__ void thresholds(const Args& a, double w, double& tb, double& tn) {
    l2f_thresholds<false>(w, a.alpha, a.beta, a.rho, tb, tn);
  }
  static __device__ __forceinline__ Iv interval(const Args& a, uint32_t sad, double s, const double (&ea)[NS],
                                                const double (&eb)[NS]) {
    Iv iv;
    l1f_interval(sad, s, ea[0], eb[0], a.lim, iv.dlo, iv.dhi);
    return iv;
  }
  static __device__ __forceinline__ bool has(const Iv& iv) { return iv.dlo == iv.dlo; }
  static __device__ __forceinline__ bool below(const Iv& iv, bool pos, double tb, double) {
    return pos ? iv.dhi < tb : iv.dlo > tb;
  }
  static __device__ __forceinline__ bool not_below(const Iv& iv, bool pos, double, double tn) {
    return pos ? iv.dlo > tn : iv.dhi < tn;
  }
};

__global__ __launch_bounds__(256, 4) void l1f_main_kernel(L1fCount::Args a) { sad_count_body<L1fCount>(a); }

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
  return sad_count_workspace("cmve_l1_count_workspace", band_cap, bytes);
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
  const FltRows rows{A, a_dtype, lda, na, B, b_dtype, ldb, nb, d};
  auto own_checks = [&]() -> int {
    return sad_checks(name, d, rows, a_codes, b_codes, grid, a_codes && a_err, b_codes && b_err,
                            "the codes, the row errors or the grid are missing (cmve_l1_grid, cmve_l1_pack)");
  };
  auto main_launch = [&](hipStream_t st, const FltArgs& f) {
    const L1fCount::Args g{sad_count_args(f, a_codes, a_err, b_codes, b_err, grid, d),
                           2.0 * ((double)d + 16.0) * L2F_U,     // rho: DESIGN s4 (K22)
                           (1e300 - fabs(beta)) / fabs(alpha)};  // lim: below it alpha * S + beta cannot overflow
    hipLaunchKernelGGL(l1f_main_kernel, dim3((unsigned)(f.tiles_a * f.tiles_b)), dim3(256), 0, st, g);
  };
  // (resolve: an overflowing list is resolved on the device, from the start -- no entry leaves it to the host)
  return flt_count_run(name, "l1_count", h, CMVE_PW_L1, rows, alpha, beta,
                       {row_off, row_sc, row_items, row_n, row_pos, col_off, col_sc, col_items, col_n, col_pos}, ws,
                       ws_bytes, stats, true, own_checks, main_launch);
}
