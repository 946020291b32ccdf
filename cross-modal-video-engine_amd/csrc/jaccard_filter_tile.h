// The integer SAD filter under jaccard (CMVE_PW_JACCARD, float32 score words) -- what K24 (jaccard_filter.hip) adds to
// the pieces of l1_filter_tile.h: the codes, the grid, the rows' errors and the SAD tile are K22's as they are; here
// are the per-row terms a jaccard side carries, the interval of a pair's two sums and the map of a float32 item word
// back to quotient space.  The derivation is DESIGN s4, "K24".
//   On the grid a code stands for g = lo + s q, so  sum_k min(ga_k, gb_k) = (P - s SAD) / 2  and
//   sum_k max(ga_k, gb_k) = (P + s SAD) / 2  with  P = 2 d lo + s (sum qa + sum qb): both from integers.  min and max
//   are 1-Lipschitz per element, so the true sums lie within err_a + err_b of those, and the canonical chains within
//   (d + 2) u (S_a + S_b) of the true sums (S >= sum_k |x_k|: with mixed signs a chain's error is relative to the
//   sum of magnitudes, not to the sum).
#ifndef CMVE_JACCARD_FILTER_TILE_H
#define CMVE_JACCARD_FILTER_TILE_H
#include "l1_filter_tile.h"

namespace cmve {

// the two per-row terms of a side as the epilogue takes them: p = d lo + s Q (the row's half of P) and
// w = err + (d + 2) u S + 16 u (|d lo| + s Q) (the row's half of the interval's width; the last term pays every
// rounding of p, of P and of the two sums formed from it).  A row beyond the set, or one with no interval (err or S
// infinite), gets w = NaN / +inf: its pairs are never decided.
__device__ __forceinline__ void jacf_side(bool valid, double err, double S, double Q, double d, double lo, double s,
                                          double& p, double& w) {
  const double dl = d * lo, sq = s * Q;
  p = dl + sq;
  w = valid ? err + ((d + 2.0) * L2F_U) * S + (16.0 * L2F_U) * (fabs(dl) + sq) : (double)NAN;
}

// [ilo, ihi] holds the canonical chain's sum of minima of the pair and [ulo, uhi] its sum of maxima, ulo > 0 (NaN,
// NaN for the first when no such statement can be made: an infinite or NaN width, a sum of maxima that may be zero or
// negative, or one that could overflow).  s SAD is the codes' L1 distance exactly in real arithmetic; 16 u of it pays
// for this product's rounding and its share of the sums'.  The 1e-280 puts every bound strictly outside the true
// value by more than any underflow of the threshold products (jacf_lt / jacf_gt).
__device__ __forceinline__ void jacf_interval(uint32_t sad, double s, double pa, double wa, double pb, double wb,
                                              double& ilo, double& ihi, double& ulo, double& uhi) {
  const double m = s * (double)sad, P = pa + pb;
  const double W = ((wa + wb) + (16.0 * L2F_U) * m) * (1.0 + 1e-9) + 1e-280;
  const double ih = 0.5 * (P - m), uh = 0.5 * (P + m);
  ulo = uh - W;
  uhi = uh + W;
  const bool ok = W < 1e300 && ulo > 0.0 && uhi < 1e300;  // false for NaN
  ilo = ok ? ih - W : (double)NAN;
  ihi = ok ? ih + W : (double)NAN;
}

// the quotient of every (I, U) of the interval lies below T / above T: two fp64 products, no division.  T carries the
// products' roundings (jacf_thresholds); a NaN anywhere says no.
__device__ __forceinline__ bool jacf_lt(double ihi, double ulo, double uhi, double T) {
  return ihi < T * (T >= 0.0 ? ulo : uhi);
}
__device__ __forceinline__ bool jacf_gt(double ilo, double ulo, double uhi, double T) {
  return ilo > T * (T >= 0.0 ? uhi : ulo);
}

// The float32 item word t (carried in a double) mapped back to quotient space.  The word of a pair is the monotone
// image of its real quotient q = I_c / U_c: fl64(q), alpha * . + beta (contracted or not), one rounding to float32.
// So e < t holds iff the fp64 value y lies below mid, the float32 rounding boundary between pred32(t) and t (exact in
// fp64; y == mid is a tie the band decides), and it suffices to bound ONE point: x = (mid - beta) / alpha with sig
// covering the roundings of x itself, of the quotient, the product and the sum (and their underflows).
//   q < tl  =>  y < mid on the side of smaller q,   q > tu  =>  y past mid on the side of larger q.
// alpha > 0: below iff q < tl, not below iff q > tu; alpha < 0: below iff q > tu, not below iff q < tl.  The last
// 4 u pay the rounding of the product T * U in jacf_lt / jacf_gt.  t = +inf is the boundary above FLT_MAX like any
// other word; a NaN or -inf item is never counted: every pair with an interval is not-below.  Where x is not finite
// nothing is decided (NaN, NaN).
__device__ __forceinline__ void jacf_thresholds(double t, double alpha, double beta, double& tl, double& tu) {
  const bool pos = alpha > 0.0;
  const double inf = __builtin_huge_val();
  if (t != t || t == -inf) {  // no pair is below
    tl = pos ? -inf : inf;    // pos: q < -inf never (below), q > -inf always (not below); else the mirror
    tu = tl;
    return;
  }
  double mid;
  if (t == inf) {
    mid = 0x1.ffffffp127;  // FLT_MAX + half an ulp: y below it rounds to a finite word
  } else {
    const float tf = (float)t;  // exact: t is a float32 value
    const uint32_t b = __float_as_uint(tf);
    const float pf = tf == 0.0f ? -__uint_as_float(1u) : __uint_as_float(tf > 0.0f ? b - 1u : b + 1u);
    mid = fabsf(pf) == __builtin_huge_valf() ? t - 0x1p103 : 0.5 * ((double)pf + t);  // (-FLT_MAX: below it is -inf)
  }
  const double x = (mid - beta) / alpha;
  const double sig = 16.0 * L2F_U * ((fabs(mid) + fabs(beta)) / fabs(alpha)) + 1e-290 +
                     4.9406564584124654e-324 / fabs(alpha);
  const double xlo = x - sig, xhi = x + sig;
  const bool ok = fabs(x) < 1e300 && sig < 1e300;  // false for NaN
  tl = ok ? xlo - (4.0 * L2F_U) * fabs(xlo) : (double)NAN;
  tu = ok ? xhi + (4.0 * L2F_U) * fabs(xhi) : (double)NAN;
}

}  // namespace cmve
#endif
