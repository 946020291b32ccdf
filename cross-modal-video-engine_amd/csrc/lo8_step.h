// The level-2 residual byte as a bit step on fp32(h) ("step code"): encode and decode, integer only, for the host
// and the device (tests/test_lo8_step_host.py compiles it into a stand-alone program and compares it with its numpy
// model word for word).
//
// An element x (fp64, normalised) is packed as xf = fp32(x), h = fp16(xf), hf = fp32(h); X = bits(xf), B = bits(hf).
// For a normal fp16 h, ulp16(h) / 256 is exactly 32 ulps of hf, so a step of 32 on hf's bit pattern is the step the
// byte counts.  The sign bit is never reached: the code is sign-magnitude, u > 128 is away from zero.
//   decode:  x2 = as_float(B - 4096 + 32 u)          = as_float(B + 32 (u - 128))
//   encode:  D = (int32)(X - B)   (xf and h have the same sign: the difference of the magnitudes)
//            u = clamp((D + 4096 + 16) >> 5, 0, 255)   (arithmetic shift: the nearest step, a tie to the larger magnitude)
//            u = 128 when h is +-0 or hf is not finite (x2 = hf)
// For a normal |h| > 2^-14, |D| <= 2^12 (half an ulp16 in ulp32(hf)), so only the upper clamp acts (the last half step
// before |h| + ulp16(h) / 2: |xf - x2| <= one step there, half a step elsewhere).  The cases off that line:
//   - xf below a power of two h: the cell below h and the bit step are both half as wide, |D| <= 2^12 still and
//     |xf - x2| <= 1/4 of h's step;
//   - |h| = 2^-14 from below (the cell below is as wide as the one above, in half-size steps): the byte covers half
//     of it, |xf - x2| <= 2^-26;
//   - h an fp16 subnormal (hf is a normal fp32 number with its own, finer, ulp): |xf - x2| <= 2^-25;
//   - h = 0: x2 = 0, |xf - x2| <= 2^-25.
// A nonzero h has mag(B) >= 0x33800000 (2^-24), so B - 4096 + 32 u never crosses zero, never becomes an fp32
// denormal and stays in its binade or the one below: x2 is zero or a normal fp32 number, xf - x2 is exact in fp32
// (the two lie within a factor of two) and the row bound is taken from it (lo8_bound).  NaN stays NaN under the add.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LO8_STEP_FN __host__ __device__ inline
#else
#define LO8_STEP_FN inline
#endif

// the byte of xf (bits X) beside h (fp32(h)'s bits B)
LO8_STEP_FN uint32_t lo8_step_encode(uint32_t X, uint32_t B) {
  const int32_t v = ((int32_t)(X - B) + (4096 + 16)) >> 5;
  const uint32_t u = (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
  // h = +-0 (B << 1 == 0) or hf inf / NaN (B << 1 >= 0xff000000): one unsigned compare of (B << 1) - 1
  return ((B << 1) - 1u >= 0xfeffffffu) ? 128u : u;
}
// x2's bits from B and the byte u
LO8_STEP_FN uint32_t lo8_step_decode(uint32_t B, uint32_t u) { return B - 4096u + (u << 5); }
// the same from q = u - 128 as a signed integer (the level-2 step flips the four top bits of a plane dword once
// and extracts its bytes sign-extended: B - 4096 + 32 u == B + 32 q mod 2^32).  sh is 5: a parameter only so that
// a kernel can hold it in a register
LO8_STEP_FN uint32_t lo8_step_decode_q(uint32_t B, int32_t q, int sh = 5) { return B + ((uint32_t)q << sh); }
