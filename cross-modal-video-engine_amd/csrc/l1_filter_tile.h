// The integer SAD filter of the L1 measures (CMVE_PW_L1, fp64 score words: l1 / l1_norm), K22 -- the pieces its
// kernels share (l1_filter.hip): the grid both sets are quantised on, the tiled order of the uint16 codes, the
// interval of a pair's L1 distance and the pads.  The derivation is DESIGN s4, "K22".
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

}  // namespace cmve
#endif
