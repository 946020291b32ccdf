// The integer SAD filter of the L1 measures (CMVE_PW_L1, fp64 score words: l1 / l1_norm) -- the pieces its kernels
// share (K22, l1_filter.hip: the count pass; K23, l1_topk.hip: the witness / candidate passes of the top-k): the grid
// both sets are quantised on, the tiled order of the uint16 codes, the pads, one 128 x 128 tile of SADs (l1f_sad_tile)
// and the interval of a pair's L1 distance.  The derivation is DESIGN s4, "K22".
//   codes  a row's elements as q_k = clamp(rint((x_k - lo) / s), 0, 65535) on ONE grid (lo, s) for both sets; two
//          codes to a dword, stored [row tile of 128][K tile of 32 elements][16 code dwords][128 rows]: a (row tile,
//          K tile) block is 8 KiB that the main kernel copies to LDS as it lies, and the 8 rows a thread owns of one
//          code dword are two 16-byte reads.  Padding (rows beyond n, elements beyond d) is code 0 in both sets: it
//          adds 0 to every SAD.
//   err    >= sum_k |x_k - (lo + s q_k)| per row (fp64, rounded up); +inf for a row with a non-finite element or one
//          above 1e150 in magnitude: "no interval", every pair of the row goes to the canonical chain.
#ifndef CMVE_L1_FILTER_TILE_H
#define CMVE_L1_FILTER_TILE_H
#include "l2_filter_tile.h"

namespace cmve {

constexpr int L1F_BM = 128, L1F_BN = 128;  // the tile: l2f_tile_of_block's order serves both filters
static_assert(L1F_BM == L2F_BM && L1F_BN == L2F_BN, "one block order for both filters");
constexpr int L1F_BK = 32;                 // elements of a K tile
constexpr int L1F_KD = L1F_BK / 2;         // its code dwords per row
constexpr int L1F_TILE_DW = L1F_KD * 128;  // dwords of one (row tile, K tile) block
constexpr int L1F_STAGE = 2 * L1F_TILE_DW * 4;  // bytes of one LDS stage: the A block, then the B block
constexpr int L1F_SMEM = 2 * L1F_STAGE;         // double-buffered
constexpr int64_t L1F_D_MAX = 65536;       // 65535 * 65536 < 2^32: the u32 SAD is exact up to here
constexpr double L1F_X_MAX = 1e150;        // a larger element: the row has no interval
constexpr double L1F_GRID_MAX = 1e30;      // a larger element takes no part in the grid's min / max

// the pads of a set of n rows of d elements
static inline void l1f_pads(int64_t n, int64_t d, int64_t& n_pad, int64_t& d_pad) {
  n_pad = (n + L1F_BM - 1) / L1F_BM * L1F_BM;
  d_pad = (d + L1F_BK - 1) / L1F_BK * L1F_BK;
}

// the raw rows every L1 entry takes beside the codes
static inline bool l1f_dtype_ok(int32_t t) { return t == CMVE_F32 || t == CMVE_F64; }

// what the four SAD entries (K22 / K24: the counts, K23 / K25: the top-ks) ask of their own operands (`name`: the
// entry; r: the raw rows, a top-k's queries as A).  a_have / b_have: every per-row array of the side is there;
// `missing`: the entry's words for one that is not
static inline int sad_checks(const char* name, int64_t d, const FltRows& r, const void* a_codes, const void* b_codes,
                             const double* grid, bool a_have, bool b_have, const char* missing) {
  CMVE_REQUIRE(d > 0 && d <= L1F_D_MAX, "%s: d must be in [1, %lld] (%lld): the u32 SAD is exact up to there", name,
               (long long)L1F_D_MAX, (long long)d);
  CMVE_REQUIRE(r.na >= 0 && r.nb >= 0 && r.na < (1ll << 31) && r.nb < (1ll << 31) && r.lda >= d && r.ldb >= d,
               "%s: bad shape", name);
  CMVE_REQUIRE(l1f_dtype_ok(r.a_dtype) && l1f_dtype_ok(r.b_dtype), "%s: rows must be CMVE_F32/CMVE_F64", name);
  CMVE_REQUIRE(grid && (a_have || !r.na) && (b_have || !r.nb), "%s: %s", name, missing);
  CMVE_REQUIRE(((((uintptr_t)a_codes) | ((uintptr_t)b_codes)) & 15) == 0, "%s: codes must be 16-byte aligned", name);
  return CMVE_OK;
}

// THE grid (lo, s) every kernel derives from the two device words {lo, hi}: min and max of the eligible elements.
// No eligible element (the words are still +inf, -inf), hi == lo, NaN: lo = 0, s = 1.  Any grid is a correct one --
// a bad one only enlarges the rows' errors, and with them the band.
__device__ __forceinline__ void l1f_grid_of(const double* __restrict__ grid, double& lo, double& s) {
  const double g_lo = grid[0], g_hi = grid[1];
  const bool ok = g_hi > g_lo;
  lo = ok ? g_lo + 0.0 : 0.0;  // (-0.0 + 0.0 = +0.0: one word for a zero minimum)
  s = ok ? (g_hi - g_lo) / 65535.0 : 1.0;
}

// the value a code stands for, as the pack's error and DESIGN s4 (K22) account for it: ONE rounding
__device__ __forceinline__ double l1f_decode(uint32_t q, double lo, double s) { return fma((double)q, s, lo); }

// [dlo, dhi] holds the true L1 distance of a pair with code SAD `sad` and row errors ea, eb (NaN, NaN when no such
// statement can be made: an infinite or NaN error, or a distance whose canonical word could overflow -- `lim` is
// (1e300 - |beta|) / |alpha|).  s * SAD is the codes' distance exactly in real arithmetic; 4u of it pays for this
// product's and the two sums' roundings.
__device__ __forceinline__ void l1f_interval(uint32_t sad, double s, double ea, double eb, double lim, double& dlo,
                                             double& dhi) {
  const double m = s * (double)sad;
  const double W = ((ea + eb) + (4.0 * L2F_U) * m) * (1.0 + 1e-9) + 1e-280;
  const double hi = m + W;
  const bool ok = hi < lim;  // false for NaN and +inf
  dlo = ok ? m - W : (double)NAN;
  dhi = ok ? hi : (double)NAN;
}

// thread (ty, tx) = (tid >> 4, tid & 15) of a tile's 256 owns the A rows l1f_row(ty, u) and the B rows l1f_row(tx, v) of
// the tile, u, v < 8: two runs of four consecutive rows 64 apart -- a 16-lane group's ds_read_b128 of a run covers 256
// contiguous bytes
__device__ __forceinline__ int l1f_row(int t, int u) { return (u >> 2) * 64 + t * 4 + (u & 3); }

// The SADs of one tile, 256 threads of 8 x 8 u32 accumulators: 32-element K tiles double-buffered in smem (L1F_SMEM
// bytes, 16-byte aligned; register staged, a straight copy of the packed blocks -- k-major, so a thread's 8 rows of a
// code dword are two ds_read_b128).  a_blk / b_blk: the first (row tile, K tile) block of the tile's A rows / B rows in
// the tiled codes; the nkt (>= 1) blocks of either side follow one another.  On return acc[u][v] is the SAD of the pair
// (A row l1f_row(ty, u), B row l1f_row(tx, v)) of the tile, and every wave has passed the loop's last barrier: smem is
// free.  The blocks are read whole: the row tiles must lie below the sets' n_pad (a multiple of 128; cmve_l1_pack_size).
__device__ __forceinline__ void l1f_sad_tile(const uint32_t* __restrict__ a_blk, const uint32_t* __restrict__ b_blk,
                                             int nkt, char* smem, uint32_t (&acc)[8][8]) {
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
#pragma unroll
  for (int u = 0; u < 8; ++u)
#pragma unroll
    for (int v = 0; v < 8; ++v) acc[u][v] = 0u;
  constexpr int Q = L1F_TILE_DW / 4;  // 16-byte pieces of a block: two per thread
  const l2f_u32x4* ga = (const l2f_u32x4*)a_blk + tid;
  const l2f_u32x4* gb = (const l2f_u32x4*)b_blk + tid;
  l2f_u32x4 ra[2], rb[2];
#define L1F_LOAD(kt)                       \
  {                                        \
    ra[0] = ga[(int64_t)(kt) * Q];         \
    ra[1] = ga[(int64_t)(kt) * Q + 256];   \
    rb[0] = gb[(int64_t)(kt) * Q];         \
    rb[1] = gb[(int64_t)(kt) * Q + 256];   \
  }
#define L1F_WRITE(buf)                                    \
  {                                                       \
    char* w_ = smem + (buf) * L1F_STAGE + tid * 16;       \
    *(l2f_u32x4*)(w_) = ra[0];                            \
    *(l2f_u32x4*)(w_ + 4096) = ra[1];                     \
    *(l2f_u32x4*)(w_ + L1F_TILE_DW * 4) = rb[0];          \
    *(l2f_u32x4*)(w_ + L1F_TILE_DW * 4 + 4096) = rb[1];   \
  }
  L1F_LOAD(0)
  L1F_WRITE(0)
  __syncthreads();
  for (int kt = 0; kt < nkt; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < nkt) L1F_LOAD(kt + 1)
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
    if (kt + 1 < nkt) L1F_WRITE(buf ^ 1)
    __syncthreads();
  }
#undef L1F_LOAD
#undef L1F_WRITE
}

}  // namespace cmve
#endif
