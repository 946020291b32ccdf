"""The 8-bit residual plane of the level-2 re-score (lo8_elem / l16_x, csrc/cmve_internal.h), modelled in numpy.

With xf = fp32(x), h = fp16(xf), d2 = xf - h, E = max(h's biased exponent field, 1) and scale = 2^(E - 33)
(= ulp16(h) / 256), the plane stores u = clamp(rint(d2 / scale), -128, 127) + 128 and level 2 rebuilds
x2 = fmaf(u, scale, fmaf(-128, scale, h)).  An fp32 FMA rounds the exact a * b + c once, so it is exact precisely when
that value is an fp32 number: the model forms every such value in fp64 (exact: at most 33 significant bits) and
asserts that the round trip through fp32 keeps it."""
import numpy as np

N_PATTERNS = 40


def _scale(hf):
    """scale = 2^(E - 33) from fp32(h) the way the kernels do: the exponent field, max with E = 1's, a subtraction."""
    bits = np.maximum(hf.view(np.uint32) & np.uint32(0x7F800000), np.uint32(113 << 23)) - np.uint32(18 << 23)
    return bits.view(np.float32), bits


def encode(xf):
    """xf (fp32) -> h (fp16), u (uint8), d2, scale, and the fp32 residual d2 - q scale."""
    assert xf.dtype == np.float32
    h = xf.astype(np.float16)
    hf = h.astype(np.float32)
    d2 = xf - hf
    scale, bits = _scale(hf)
    inv = (np.uint32(254 << 23) - bits).view(np.float32)
    q = np.clip(np.rint(d2 * inv), -128.0, 127.0).astype(np.float32)
    res = d2 - q * scale  # (fp32 arithmetic; its exactness is asserted by the caller against fp64)
    return h, (q + np.float32(128.0)).astype(np.uint8), d2, scale, res, q


def decode64(h, u):
    """x2 in fp64 with the two FMA stages' exact values (inner, outer)."""
    hf = h.astype(np.float32)
    scale, _ = _scale(hf)
    inner = hf.astype(np.float64) - 128.0 * scale.astype(np.float64)
    outer = inner + u.astype(np.float64) * scale.astype(np.float64)
    return inner, outer


def _is_f32(v64):
    with np.errstate(over="ignore"):
        return v64.astype(np.float32).astype(np.float64) == v64


def _all_values():
    """Every fp16 value in [0, 1], both signs, each with N_PATTERNS residuals in units of its own ulp16: +-1/2 (the
    ties; +1/2 on an even mantissa is the clamp), 0, +-1/4, +-(1/2 - 2^-12) and 33 random ones."""
    hb = np.arange(0, 0x3C00 + 1, dtype=np.uint16)
    hb = np.concatenate([hb, hb | np.uint16(0x8000)])
    h = hb.view(np.float16).astype(np.float64)
    e = np.maximum((hb >> 10) & 31, 1).astype(np.int64)
    ulp = np.ldexp(1.0, e - 25)
    rng = np.random.default_rng(0)
    fixed = np.array([0.5, -0.5, 0.0, 0.25, -0.25, 0.5 - 2.0 ** -12, -(0.5 - 2.0 ** -12)])
    r = np.concatenate([np.broadcast_to(fixed, (h.size, fixed.size)),
                        rng.uniform(-0.5, 0.5, (h.size, N_PATTERNS - fixed.size))], axis=1)
    x = h[:, None] + r * ulp[:, None]
    return x.astype(np.float32).ravel()


def test_lo8_encode_decode_exact():
    xf = _all_values()
    assert xf.size == 2 * (0x3C00 + 1) * N_PATTERNS  # 1.2 M values
    h, u, d2, scale, res, q = encode(xf)
    hb = h.view(np.uint16)
    # the scale from fp32(h)'s bits is 2^(E - 33), E = max(fp16 exponent field, 1): subnormals share E = 1's
    e = np.maximum((hb >> 10) & 31, 1).astype(np.int64)
    assert np.array_equal(scale.astype(np.float64), np.ldexp(1.0, e - 33))
    assert ((hb & 0x7FFF) < 0x0400).sum() > 40000  # (zeros and subnormals are in the set)
    x64, h64, s64 = xf.astype(np.float64), h.astype(np.float64), scale.astype(np.float64)
    # d2 exact in fp32
    assert np.array_equal(d2.astype(np.float64), x64 - h64)
    # |d2| <= ulp16(h) / 2 = 128 scale: the lower clamp never acts, the upper one only on the last half step below
    # +ulp16 / 2 (127.5 <= d2 / scale <= 128)
    t = (x64 - h64) / s64
    assert np.abs(t).max() <= 128.0
    clamped = np.rint(t) > 127.0
    assert (t[clamped] == 128.0).any() and np.all(t[clamped] >= 127.5)
    assert np.array_equal(q[clamped], np.full(int(clamped.sum()), 127.0, np.float32))
    assert (t == -128.0).any()  # (the -ulp16 / 2 ties are in the set; q = -128 needs no clamp)
    # the residual d2 - q scale is exact in fp32
    assert np.array_equal(res.astype(np.float64), (x64 - h64) - q.astype(np.float64) * s64)
    # both FMAs of the decode are exact, and x2 = h + q scale
    inner, x2 = decode64(h, u)
    assert _is_f32(inner).all() and _is_f32(x2).all()
    assert np.array_equal(x2, h64 + q.astype(np.float64) * s64)
    # |xf - x2| <= scale / 2; under the clamp it is (d2 / scale - 127) scale <= scale, = scale only at +ulp16 / 2
    err = np.abs(x64 - x2)
    assert np.all(err[~clamped] <= 0.5 * s64[~clamped])
    assert np.array_equal(err[clamped], (t[clamped] - 127.0) * s64[clamped])
    assert np.all(err <= s64) and np.array_equal(err == s64, t == 128.0)


def _bound(res32):
    """lo8_bound of the row's fp32 sum of squared residuals, rounded up to fp32."""
    ss = np.float64(np.sum(res32 * res32, dtype=np.float32))
    b = np.sqrt(ss) * (1.0 + 1e-4) + 5.9605e-8 * (1.0 + 1e-6) + 1e-12
    f = np.float32(b)
    return f if np.float64(f) >= b else np.nextafter(f, np.float32(np.inf))


def test_lo8_row_bound_dominates():
    """The row bound sqrt(sum (d2 - q scale)^2) (1 + 1e-4) + 2^-24 terms dominates the true ||x - x2|| of fp64 rows:
    normalised Gaussian rows of 1,024 elements at scales 1, 2^-1, ... 2^-30 (||x|| <= 1: the 2^-24 ||x|| term holds);
    at scale 1 the bound's mean is reported (8.8e-7 on these rows; the bf16 plane's was 3.1e-7)."""
    rng = np.random.default_rng(1)
    at1 = []
    for s in range(0, 31):
        for _ in range(8):
            x = rng.standard_normal(1024)
            x = x / np.sqrt(np.sum(x * x)) * 2.0 ** -s
            xf = x.astype(np.float32)
            h, u, d2, scale, res, q = encode(xf)
            _, x2 = decode64(h, u)
            true = np.sqrt(np.sum((x - x2) ** 2))
            b = _bound(res)
            assert np.float64(b) >= true, (s, float(b), true)
            if s == 0:
                at1.append(float(b))
    print("mean row bound at scale 1: %.3e" % np.mean(at1))
    # per element |xf - x2| <= scale / 2 = 2^-9 ulp16(h), and a normalised row's elements lie below 1 (ulp16 <= 2^-11)
    assert np.max(at1) < (np.sqrt(1024) * 2.0 ** -20 + 2.0 ** -24) * (1.0 + 2e-4)
