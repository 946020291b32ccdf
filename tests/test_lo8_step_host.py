"""The level-2 residual byte as a bit step on fp32(h) (csrc/lo8_step.h), modelled in numpy and compared with the
arithmetic code it replaced (tests/test_lo8_host.py keeps that code's own model).

With xf = fp32(x), h = fp16(xf), X = bits(xf), B = bits(fp32(h)):
  encode  D = (int32)(X - B),  u = clamp((D + 4096 + 16) >> 5, 0, 255),  u = 128 when h is +-0 or not finite
  decode  x2 = as_float(B - 4096 + 32 u)
Checked over every fp16 value in [0, 1], both signs, 40 residuals each (1.2 M values), and on rows; the header itself
is compiled into a stand-alone program and compared with the model word for word.

Where the step code and the arithmetic code may differ (everywhere else x2 must be the same number):
  (a) negative values on the last half step before +-ulp16/2, the ties included (|D| >= 4080): the code is
      sign-magnitude, so the clamp sits at +magnitude where the arithmetic code's sat at +value;
  (b) xf below a power of two h: the bit step is half as wide there (|xf - x2| <= scale / 4);
  (c) |h| = 2^-14 approached from below (|xf - x2| <= 2^-26);  (d) subnormal h;  (e) h = 0 (both <= 2^-25);
  (f) exact half-step ties, D = 16 (mod 32): the arithmetic code rounded them to even (rint), the integer code rounds
      them to the larger magnitude; the error is scale / 2 either way.  (f) is 1 in 64 of random fp32 values: x2 is the same
      number on 98.1% of the elements of normalised Gaussian rows.
In (a) and (f) the two codes' errors obey the same bounds (scale under the clamp, scale / 2 at a tie)."""
import os
import shutil
import subprocess

import numpy as np

N_PATTERNS = 40
U32, I32, F32, F64 = np.uint32, np.int32, np.float32, np.float64


# ---- the step code ----
def encode(xf):
    """xf (fp32) -> h (fp16), B, u (uint32 in [0, 255]), D."""
    assert xf.dtype == F32
    with np.errstate(over="ignore"):  # (a value past fp16's range gives h = inf: u = 128)
        h = xf.astype(np.float16)
    B = h.astype(F32).view(U32)
    D = (xf.view(U32) - B).view(I32)
    u = np.clip((D + I32(4096 + 16)) >> I32(5), 0, 255).astype(U32)
    special = ((B << U32(1)) == 0) | ((B << U32(1)) >= U32(0xFF000000))
    return h, B, np.where(special, U32(128), u), D


def decode(B, u):
    return (B - U32(4096) + (u << U32(5))).view(F32)


# ---- the arithmetic code it replaced (lo8_elem / l16_x of the parent) ----
def _old_scale(hf):
    bits = np.maximum(hf.view(U32) & U32(0x7F800000), U32(113 << 23)) - U32(18 << 23)
    return bits.view(F32), bits


def old_x2(xf):
    hf = xf.astype(np.float16).astype(F32)
    scale, bits = _old_scale(hf)
    inv = (U32(254 << 23) - bits).view(F32)
    q = np.clip(np.rint((xf - hf) * inv), -128.0, 127.0)
    return hf.astype(F64) + q.astype(F64) * scale.astype(F64), scale.astype(F64)


def _all_values():
    """Every fp16 value in [0, 1], both signs, each with N_PATTERNS residuals in units of its own ulp16: the ties
    +-1/2, 0, +-1/4 (-1/4 below a power of two is the tie of the half-width cell there), +-(1/2 - 2^-12),
    -(1/4 - 2^-12), -1/8, -3/16 (inside the half-width cell) and 30 random ones."""
    hb = np.arange(0, 0x3C00 + 1, dtype=np.uint16)
    hb = np.concatenate([hb, hb | np.uint16(0x8000)])
    h = hb.view(np.float16).astype(F64)
    e = np.maximum((hb >> 10) & 31, 1).astype(np.int64)
    ulp = np.ldexp(1.0, e - 25)
    rng = np.random.default_rng(0)
    fixed = np.array([0.5, -0.5, 0.0, 0.25, -0.25, 0.5 - 2.0 ** -12, -(0.5 - 2.0 ** -12), -(0.25 - 2.0 ** -12),
                      -0.125, -0.1875])
    r = np.concatenate([np.broadcast_to(fixed, (h.size, fixed.size)),
                        rng.uniform(-0.5, 0.5, (h.size, N_PATTERNS - fixed.size))], axis=1)
    # (the residual is towards / away from zero for both signs: |x| = |h| + r ulp)
    x = np.where(hb[:, None] & 0x8000, -1.0, 1.0) * (np.abs(h)[:, None] + r * ulp[:, None])
    return x.astype(F32).ravel()


def _classes(xf, h, B, D):
    """Masks of the cases (a)-(f) of the module docstring."""
    hb = h.view(np.uint16)
    mag = hb & np.uint16(0x7FFF)
    neg = (hb & np.uint16(0x8000)) != 0
    a = neg & (np.abs(D) >= 4080) & (mag >= 0x0400)
    b = ((mag & 0x03FF) == 0) & (mag > 0x0400) & (D < 0)
    c = (mag == 0x0400) & (D < 0)
    d = (mag < 0x0400) & (mag > 0)
    e = mag == 0
    f = (D & I32(31)) == 16
    return a, b, c, d, e, f


def test_step_code_every_fp16_value():
    xf = _all_values()
    assert xf.size == 2 * (0x3C00 + 1) * N_PATTERNS  # 1.2 M values
    h, B, u, D = encode(xf)
    x2 = decode(B, u)
    hb = h.view(np.uint16)
    mag = hb & np.uint16(0x7FFF)
    assert (mag < 0x0400).sum() > 40000 and (mag == 0).sum() > 0  # (zeros and subnormals are in the set)
    # x2 is zero or a normal fp32 number, of h's sign
    ax2 = np.abs(x2)
    assert np.all(np.isfinite(x2)) and np.all((ax2 == 0) | (ax2 >= np.finfo(F32).tiny))
    assert np.array_equal(x2.view(U32) >> U32(31), B >> U32(31))
    # xf - x2 is exact in fp32
    x64, x264 = xf.astype(F64), x2.astype(F64)
    assert np.array_equal((xf - x2).astype(F64), x64 - x264)
    # u = 128 and x2 = h for h = +-0
    assert np.all(u[mag == 0] == 128) and np.all(x2[mag == 0] == 0)
    # the error, in units of scale = ulp16(h) / 256
    old, scale = old_x2(xf)
    err = np.abs(x64 - x264)
    a, b, c, d, e, f = _classes(xf, h, B, D)
    normal = mag > 0x0400  # normal |h| > 2^-14
    clamp_hi = ((D + I32(4096 + 16)) >> I32(5)) > 255
    assert clamp_hi[normal].any() and b.any() and c.any() and a.any() and f.any()
    assert np.all(err[normal & ~clamp_hi] <= 0.5 * scale[normal & ~clamp_hi])
    assert np.all(err[normal & clamp_hi] <= scale[normal & clamp_hi])
    assert np.all(err[b] <= 0.25 * scale[b])
    # (the lower clamp never acts on a normal |h| > 2^-14: |D| <= 2^12 there, below a power of two as well)
    assert np.all(np.abs(D[normal]) <= 4096)
    at14 = mag == 0x0400
    assert np.all(err[at14] <= 2.0 ** -26) and (err[at14] == 2.0 ** -26).any()
    assert np.all(err[mag < 0x0400] <= 2.0 ** -25)
    # the same number as the arithmetic code's everywhere else
    same = x264 == old
    allowed = a | b | c | d | e | f
    print("x2 equal to the arithmetic code's on %.4f of the values; outside (a)-(f): %d differ"
          % (same.mean(), int((~same & ~allowed).sum())))
    assert np.all(same | allowed)
    # at a half-step tie (f) the two choices are equally far from xf
    ff = f & normal & ~a & ~b
    assert np.array_equal(err[ff], np.abs(x64 - old)[ff])


def _bound(res32):
    """lo8_bound of the row's fp32 sum of squared residuals, rounded up to fp32."""
    ss = F64(np.sum(res32 * res32, dtype=F32))
    b = np.sqrt(ss) * (1.0 + 1e-4) + 5.9605e-8 * (1.0 + 1e-6) + 1e-12
    f = F32(b)
    return f if F64(f) >= b else np.nextafter(f, F32(np.inf))


def _row_bounds(x):
    """(step code's bound, its true error, the arithmetic code's bound) of one fp64 row."""
    xf = x.astype(F32)
    h, B, u, D = encode(xf)
    x2 = decode(B, u)
    old, _ = old_x2(xf)
    res_old = (xf.astype(F64) - old).astype(F32)  # (exact in fp32: test_lo8_host.py)
    return _bound(xf - x2), np.sqrt(np.sum((x - x2.astype(F64)) ** 2)), _bound(res_old)


def test_step_code_row_bound():
    """lo8_bound of the decoded values dominates the true ||x - x2|| on normalised Gaussian rows of 1,024 elements at
    scales 1 ... 2^-30; its mean stays within 1% of the arithmetic code's on the same rows at scale 1, and within 15%
    on rows with 40% of the columns scaled by 2^-13 (fp16 subnormals after normalising)."""
    rng = np.random.default_rng(1)
    for s in range(0, 31):
        for _ in range(8):
            x = rng.standard_normal(1024)
            x = x / np.sqrt(np.sum(x * x)) * 2.0 ** -s
            b, true, _ = _row_bounds(x)
            assert F64(b) >= true, (s, float(b), true)
    new1, old1, news, olds = [], [], [], []
    sub = rng.permutation(1024)[:(2 * 1024) // 5]
    for _ in range(200):
        x = rng.standard_normal(1024)
        y = x.copy()
        y[sub] *= 2.0 ** -13
        for v, n_, o_ in ((x, new1, old1), (y, news, olds)):
            v = v / np.sqrt(np.sum(v * v))
            b, true, bo = _row_bounds(v)
            assert F64(b) >= true
            n_.append(float(b))
            o_.append(float(bo))
    r1, rs = np.mean(new1) / np.mean(old1), np.mean(news) / np.mean(olds)
    print("mean row bound, step / arithmetic: Gaussian %.4e / %.4e (%.4f), 40%% subnormal columns %.4e / %.4e (%.4f)"
          % (np.mean(new1), np.mean(old1), r1, np.mean(news), np.mean(olds), rs))
    assert abs(r1 - 1.0) <= 0.01
    assert abs(rs - 1.0) <= 0.15


_MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include "lo8_step.h"
// stdin: n pairs (X, B) of uint32; stdout: n triples (u, bits(x2), bits(x2) through the signed form)
int main(int argc, char** argv) {
  const size_t n = (size_t)atol(argv[1]);
  uint32_t* in = (uint32_t*)malloc(n * 8);
  uint32_t* out = (uint32_t*)malloc(n * 12);
  if (!in || !out || fread(in, 8, n, stdin) != n) return 2;
  for (size_t i = 0; i < n; ++i) {
    const uint32_t X = in[2 * i], B = in[2 * i + 1];
    const uint32_t u = lo8_step_encode(X, B);
    out[3 * i] = u;
    out[3 * i + 1] = lo8_step_decode(B, u);
    out[3 * i + 2] = lo8_step_decode_q(B, (int32_t)u - 128);
  }
  return fwrite(out, 12, n, stdout) == n ? 0 : 3;
}
"""


def test_step_code_header_on_the_host(tmp_path):
    """csrc/lo8_step.h, compiled by the host's C++ compiler into a program of its own, gives the model's (u, bits(x2))
    for the same 1.2 M values word for word."""
    import pytest
    cxx = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cross-modal-video-engine_amd",
                       "csrc")
    src = tmp_path / "lo8_step_main.cpp"
    src.write_text(_MAIN)
    exe = tmp_path / "lo8_step_main"
    subprocess.run([cxx, "-O1", "-std=c++11", "-Wall", "-Werror", "-I", inc, "-o", str(exe), str(src)], check=True)
    xf = _all_values()
    h, B, u, D = encode(xf)
    x2 = decode(B, u)
    pairs = np.stack([xf.view(U32), B], axis=1).astype(U32)
    p = subprocess.run([str(exe), str(xf.size)], input=pairs.tobytes(), stdout=subprocess.PIPE, check=True)
    got = np.frombuffer(p.stdout, dtype=U32).reshape(-1, 3)
    assert got.shape[0] == xf.size
    assert np.array_equal(got[:, 0], u)
    assert np.array_equal(got[:, 1], x2.view(U32))
    assert np.array_equal(got[:, 2], x2.view(U32))
    # not-finite h: u = 128, x2 = hf
    sp = np.array([[0x7F800001, 0x7FC00000], [0x477FF000, 0x7F800000], [0xC77FF000, 0xFF800000]], dtype=U32)
    p = subprocess.run([str(exe), "3"], input=sp.tobytes(), stdout=subprocess.PIPE, check=True)
    got = np.frombuffer(p.stdout, dtype=U32).reshape(-1, 3)
    assert np.all(got[:, 0] == 128) and np.array_equal(got[:, 1], sp[:, 1])
    hh, BB, uu, _ = encode(sp[:, 0].copy().view(F32))
    assert np.all(uu == 128)
