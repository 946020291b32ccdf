"""K1 (cmve_pack_rows), K1' (cmve_l2norm_rows), K5a (cmve_gt_thresholds / cmve_rank_thresholds) and the score
bound |s~ - cos| <= E at its tight cases, through the C ABI.

The cosine route's exactness argument rests on three things this file pins from both sides:
the per-row bounds err_* cover the distance between the unit row and each STORED plane, and are not loose
(a bound taken from the wrong accumulator would still "hold"); the thresholds thr_hi / thr_lo round
outwards; and the MFMA score of any pair is within E of the cosine, on rows whose representation errors
line up (constant and non-negative rows: the Cauchy-Schwarz term is attained) as on Gaussian ones.  Rows
come from ten families (below); every reference is numpy in np.longdouble from the raw rows, the planes
are restated bit for bit from the device's own inv_norm, and every output is a window of a canary buffer.
"""
import ctypes

import numpy as np
import pytest
import torch

from _windows import Pad, _within, _E, _f32_up, _f32_down

pytestmark = pytest.mark.gpu

LD = np.longdouble
F32, F64 = 0, 1
NP = {F32: np.float32, F64: np.float64}
TORCH = {F32: torch.float32, F64: torch.float64}
BF16, BF16X3, F16 = 0, 1, 2  # CMVE_SIM_*: also the slot of err_max
MODES = {BF16: "bf16", BF16X3: "bf16x3", F16: "f16"}
PACK_RAW = 1
INF, NAN = np.inf, np.nan
U52, U50, U24, U22 = 2.0 ** -52, 2.0 ** -50, 2.0 ** -24, 2.0 ** -22


def _api():
    from cmve import engine
    from cmve._lib import lib, check, Rows
    return engine.handle(), lib, check, Rows


# ------------------------------------------------------------------ row families
FAMILIES = ("gauss", "absgauss", "const", "alt", "onehot", "subn", "big", "small", "tiny", "zero")


def _family(name, rng, d, dt):
    """One row in fp64 (the caller casts).  big / small: 2^+-60 for fp64 input, 2^+-30 for fp32."""
    g = rng.standard_normal(d)
    e = 60 if dt == F64 else 30
    if name == "gauss":
        return g
    if name == "absgauss":
        return np.abs(g)
    if name == "const":
        return np.full(d, 0.37)  # every element rounds the same way: the aligned case of Cauchy-Schwarz
    if name == "alt":
        return (1 - 2 * (np.arange(d) % 2)) * (1 + 1e-3 * g)
    if name == "onehot":
        x = 1e-6 * (1 + 0.1 * g)  # fp16 subnormals or zeros after normalising
        x[rng.integers(d)] = 1.0
        return x
    if name == "subn":
        return g * 2.0 ** -rng.integers(0, 21, d)  # at d = 1000 several hundred fp16 subnormals
    if name == "big":
        return g * 2.0 ** e
    if name == "small":
        return g * 2.0 ** -e
    if name == "tiny":
        return g * 1e-14  # its norm is under eps = 1e-12
    return np.zeros(d)


def _rows(names, rng, d, dt):
    if len(names) == 0:
        return np.zeros((0, d), NP[dt])
    return np.stack([_family(f, rng, d, dt) for f in names]).astype(NP[dt])


# ------------------------------------------------------------------ numpy restatements
def _f2bf(xf):
    """cmve_internal.h:86 -- fp32 -> bf16 words, round to nearest even, NaN kept."""
    u = np.ascontiguousarray(xf, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7fff + ((u >> 16) & 1)) & 0xffffffff) >> 16
    nan = (u & 0x7fffffff) > 0x7f800000
    r[nan] = (u[nan] >> 16) | 0x40
    return r.astype(np.uint16)


def _bf2f(b):
    return (np.asarray(b, np.uint16).astype(np.uint32) << 16).view(np.float32)


def _norms(x):
    return np.sqrt((x.astype(LD) ** 2).sum(axis=1))


# ------------------------------------------------------------------ a packed set whose every buffer is a window
class Packed:
    def __init__(self, x, dt, ld=None, off=0, lo=True, h16=True, eps=0.0, flags=0):
        h, lib, check, Rows = _api()
        self.x, self.dt, self.eps, self.flags = x, dt, eps, flags
        self.n, self.d = x.shape
        np_, dp_ = ctypes.c_int64(), ctypes.c_int64()
        check(lib.cmve_pack_size(self.n, self.d, ctypes.byref(np_), ctypes.byref(dp_)), "cmve_pack_size")
        self.n_pad, self.d_pad = np_.value, dp_.value
        self.raw = Pad(self.n, self.d, ld=ld, off=off, dtype=TORCH[dt], data=x if self.n else None)
        self.hi = Pad(self.n_pad, self.d_pad, dtype=torch.int16)
        self.lo = Pad(self.n_pad, self.d_pad, dtype=torch.int16) if lo else None
        self.h16 = Pad(self.n_pad, self.d_pad, dtype=torch.int16) if h16 else None
        self.inv = Pad(1, self.n_pad, dtype=torch.float64)
        self.err_hi, self.err_hilo = Pad(1, self.n_pad), Pad(1, self.n_pad)
        self.err_h16 = Pad(1, self.n_pad) if h16 else None
        self.err_max = Pad(1, 3)
        r = Rows()
        r.n, r.d, r.n_pad, r.d_pad = self.n, self.d, self.n_pad, self.d_pad
        r.hi, r.lo, r.h16 = self.hi.ptr.value, (self.lo.ptr.value if lo else None), (self.h16.ptr.value if h16 else None)
        r.raw, r.raw_dtype, r.flags, r.raw_ld, r.eps = self.raw.ptr.value, dt, flags, self.raw.ld, eps
        r.inv_norm, r.err_hi, r.err_hilo = self.inv.ptr.value, self.err_hi.ptr.value, self.err_hilo.ptr.value
        r.err_h16, r.err_max = (self.err_h16.ptr.value if h16 else None), self.err_max.ptr.value
        self.rows = r
        self.vec = self.d % 4 == 0 and (self.raw.ld * x.itemsize) % 16 == 0 and self.raw.aligned16

    def outputs(self):
        return [p for p in (self.hi, self.lo, self.h16, self.inv, self.err_hi, self.err_hilo, self.err_h16,
                            self.err_max) if p is not None]

    def pack(self):
        h, lib, check, _ = _api()
        check(lib.cmve_pack_rows(h, ctypes.byref(self.rows)), "cmve_pack_rows")
        for p in self.outputs():
            p.assert_canary("a pack output")
        return self

    def result(self):
        w = lambda p: None if p is None else p.numpy().view(np.uint16)
        f = lambda p: None if p is None else p.numpy()[0]
        return dict(hi=w(self.hi), lo=w(self.lo), h16=w(self.h16), inv=f(self.inv), err_hi=f(self.err_hi),
                    err_hilo=f(self.err_hilo), err_h16=f(self.err_h16), err_max=f(self.err_max))


def _check_pack(out, x, eps, flags, what):
    """Every assertion on one packed set; `out` holds the device's arrays (Packed.result)."""
    n, d = x.shape
    n_pad, d_pad = out["hi"].shape
    raw = bool(flags & PACK_RAW)
    nrm = _norms(x)
    with np.errstate(all="ignore"):
        inv_ref = np.ones(n, LD) if raw else (1 / np.maximum(nrm, LD(eps)) if eps > 0 else 1 / nrm)
        inv = out["inv"][:n]
        # inv_norm: the fp64 fma chains of row_sumsq (d / 64 per lane), six butterfly adds, sqrt, division
        _within(inv, inv_ref.astype(np.float64), (d / 64 + 8) * U52 * np.abs(inv_ref.astype(np.float64)), f"{what} inv_norm")
        zero = nrm == 0
        if raw:
            assert (inv == 1).all()
        elif eps > 0:
            assert (inv[zero] == 1 / eps).all()
        else:
            assert np.isinf(inv[zero]).all()
        # planes, bit for bit from the device's own inv_norm: one fp64 product, one rounding to fp32
        xh = x.astype(np.float64) * inv[:, None]
        xf = xh.astype(np.float32)
        hi = _f2bf(xf)
        lo = _f2bf(xf - _bf2f(hi))
        h16 = xf.astype(np.float16).view(np.uint16)
    dead = np.isnan(xh).any(axis=1)  # a zero row at eps = 0: 0 * inf
    assert np.array_equal(dead, zero & (eps == 0) & (not raw))
    for name, want, nan_above in (("hi", hi, 0x7f80), ("lo", lo, 0x7f80), ("h16", h16, 0x7c00)):
        got = out[name]
        if got is None:
            continue
        assert np.array_equal(got[:n, :d][~dead], want[~dead]), f"{what} {name}: plane words differ"
        assert ((got[:n, :d][dead] & 0x7fff) > nan_above).all(), f"{what} {name}: a zero row at eps = 0 is NaN"
        assert not got[:, d:].any() and not got[n:].any(), f"{what} {name}: padding is zero words"
    for name in ("inv", "err_hi", "err_hilo", "err_h16"):
        if out[name] is not None:
            assert (out[name][n:] == 0).all(), f"{what} {name}: padding rows hold 0"
    # bounds, from both sides: r <= err <= r (1 + 2^-22) + 2e-12 with r = ||x^ - stored plane|| in longdouble.
    # pack_row_planes gives f32_round_up(sqrt(e) (1 + 1e-9) + 1e-12), e the fp64 sum of squared residuals of
    # fp64(x inv): within (d / 64 + 9) 2^-52 of x^ per unit of norm, far inside the 1e-12.
    with np.errstate(all="ignore"):
        xhat = x.astype(LD) * inv_ref[:, None]
        xhat[zero] = 0 if (eps > 0 or raw) else NAN
        stored = {"err_hi": _bf2f(out["hi"][:n, :d]).astype(LD)}
        # (lo NULL: err_hilo is still written, for the lo words the kernel formed -- the ones restated above)
        stored["err_hilo"] = stored["err_hi"] + _bf2f(lo if out["lo"] is None else out["lo"][:n, :d]).astype(LD)
        if out["h16"] is not None:
            stored["err_h16"] = out["h16"][:n, :d].view(np.float16).astype(LD)
        for name, plane in stored.items():
            r = np.sqrt(((xhat - plane) ** 2).sum(axis=1)).astype(np.float64)
            err = out[name][:n].astype(np.float64)
            assert np.isnan(err[dead]).all(), f"{what} {name}: the bound of a NaN row is NaN"
            ok = ~dead
            assert (r[ok] <= err[ok]).all(), f"{what} {name}: bound below the distance, worst " \
                                             f"{(r[ok] / err[ok]).max() if ok.any() else 0}"
            assert (err[ok] <= r[ok] * (1 + U22) + 2e-12).all(), f"{what} {name}: bound loose, worst err / r " \
                                                                 f"{(err[ok] / np.maximum(r[ok], 1e-300)).max() if ok.any() else 0}"
    # err_max
    if raw:
        assert np.isinf(out["err_max"]).all() and (out["err_max"] > 0).all()
    else:
        mx = lambda e: np.float32(0) if e is None or n == 0 or np.isnan(e[:n]).all() else np.nanmax(e[:n])
        want = [mx(out["err_hi"]), mx(out["err_hilo"]), mx(out["err_h16"])]
        assert out["err_max"].tolist() == [float(w) for w in want], f"{what} err_max"


# ------------------------------------------------------------------ 1. cmve_pack_rows
def _windows(d, dt):
    """(ld, off) of the raw windows: A reaches the 16-byte path when d % 4 == 0 (ld a multiple of 4 elements, base
    aligned); B1 (ld = d + 1) and B2 (A's ld, base one element in) miss it."""
    lda = d + 4 if d % 4 == 0 else d
    return (lda, 0), (d + 1, 0), (lda, 1)


@pytest.mark.parametrize("dt", [F32, F64])
@pytest.mark.parametrize("d", [1, 3, 4, 31, 64, 65, 257, 1000, 1536])
def test_pack_rows_planes_bounds_and_paths(d, dt):
    """cmve_pack_rows at n = 257 (two row blocks of 4 and a part; n_pad = 512), 256 (no padding row), 3, 1 and 0,
    the ten families cycling over the rows, through raw windows that reach the 16-byte path (d = 4, 64, 1000,
    1536) and windows that miss it; lo and h16 given or NULL; eps 0 and 1e-12 (the `tiny` rows have a norm under
    it, the zero rows are NaN at eps = 0); CMVE_PACK_RAW.  d = 1 .. 65 are under, at and over one 64-lane step
    of the scalar path, 257 and 1000 several steps with a part, 1000 and 1536 four and six steps of the 16-byte
    path.  The two paths agree in every plane word on the rows where their inv_norm agree."""
    rng = np.random.default_rng(10 * d + dt)
    A, B1, B2 = _windows(d, dt)
    fams = [FAMILIES[(r + d) % len(FAMILIES)] for r in range(257)]
    x = _rows(fams, rng, d, dt)
    cfgs = [  # n, window, lo, h16, eps, flags
        (257, A, True, True, 0.0, 0), (257, B1, True, True, 0.0, 0), (257, B2, True, True, 1e-12, 0),
        (257, A, True, True, 1e-12, 0), (256, A, False, False, 1e-12, 0), (3, B1, False, True, 0.0, 0),
        (3, A, True, False, 1e-12, 0), (1, B2, True, True, 0.0, 0), (0, A, True, True, 0.0, 0)]
    res = {}
    for n, (ld, off), lo, h16, eps, flags in cfgs:
        P = Packed(x[:n], dt, ld=ld, off=off, lo=lo, h16=h16, eps=eps, flags=flags)
        assert P.vec == (d % 4 == 0 and (ld, off) == A)
        out = P.pack().result()
        _check_pack(out, x[:n], eps, flags, f"n {n} d {d} ld {ld} off {off} eps {eps}")
        res[(n, (ld, off), eps)] = out
    # the same values under CMVE_PACK_RAW (no normalisation): rows of ordinary size only (an fp16 plane of 2^60 is inf)
    keep = [r for r in range(40) if fams[r] in ("gauss", "absgauss", "const", "alt", "subn")]
    for ld, off in (A, B1):
        P = Packed(x[keep], dt, ld=ld, off=off, flags=PACK_RAW)
        _check_pack(P.pack().result(), x[keep], 0.0, PACK_RAW, f"raw d {d} ld {ld}")
    if d % 4 == 0:
        for eps, scalar in ((0.0, B1), (1e-12, B2)):
            a, b = res[(257, A, eps)], res[(257, scalar, eps)]
            same = (a["inv"] == b["inv"]) | (np.isnan(a["inv"]) & np.isnan(b["inv"]))
            for name in ("hi", "lo", "h16"):
                assert np.array_equal(a[name][same], b[name][same]), f"d {d}: {name} differs between the paths"
            print(f"PATHS d={d} dt={dt} eps={eps}: inv_norm differs on {int((~same[:257]).sum())} of 257 rows")


def test_pack_rows_refusals():
    """n_pad or d_pad not cmve_pack_size's, raw_ld < d, eps < 0, h16 without err_h16 and the reverse, an unknown
    raw_dtype, a NULL hi / handle: refused, and no output is written."""
    h, lib, check, Rows = _api()
    x = np.ones((3, 8))
    P = Packed(x, F64)
    good = P.rows

    def refused(**change):
        r = Rows()
        ctypes.memmove(ctypes.byref(r), ctypes.byref(good), ctypes.sizeof(Rows))
        for k, v in change.items():
            setattr(r, k, v)
        assert lib.cmve_pack_rows(h, ctypes.byref(r)) != 0, f"accepted {change}"
        for p in P.outputs():
            p.assert_untouched(f"an output of a refused cmve_pack_rows {change}")

    refused(n_pad=512)
    refused(n_pad=128)
    refused(d_pad=128)
    refused(d_pad=8)
    refused(raw_ld=7)
    refused(eps=-1e-12)
    refused(err_h16=None)
    refused(h16=None)
    refused(raw_dtype=2)
    refused(raw_dtype=-1)
    refused(hi=None)
    refused(inv_norm=None)
    refused(err_max=None)
    refused(raw=None)
    refused(d=0)
    assert lib.cmve_pack_rows(None, ctypes.byref(good)) != 0
    assert lib.cmve_pack_rows(h, None) != 0
    P.pack()  # and the set it was derived from packs


# ------------------------------------------------------------------ 2. cmve_l2norm_rows
@pytest.mark.parametrize("xdt,ydt", [(F32, F32), (F32, F64), (F64, F32), (F64, F64)])
@pytest.mark.parametrize("d", [1, 63, 64, 65, 1000])
def test_l2norm_rows_dtypes_strides_and_zero_rows(d, xdt, ydt):
    """y = x / max(||x||, eps) against longdouble, ldx = d + 3 and ldy = d + 2 (NaN between the rows of x, a canary
    between those of y), n = 0, 1 and 5 (a block holds four rows), eps 0 and 1e-12.  fp64 output within (d / 64
    + 8) 2^-52 relative (the fma chains, butterfly, sqrt, division); fp32 output one rounding more: 2^-24
    relative, or the spacing 2^-149 of fp32 subnormals below the normal range.  Zero rows: NaN at eps = 0, zeros
    at eps > 0; `tiny` rows (norm under 1e-12) are divided by eps."""
    h, lib, check, _ = _api()
    rng = np.random.default_rng(d + 7 * xdt + 3 * ydt)
    x = _rows(["gauss", "subn", "big" if d % 2 else "small", "tiny", "zero"], rng, d, xdt)
    for n in (0, 1, 5):
        for eps in (0.0, 1e-12):
            xs = x[(d % 5):(d % 5) + 1] if n == 1 else x[:n]
            X = Pad(n, d, ld=d + 3, dtype=TORCH[xdt], data=xs if n else None)
            Y = Pad(n, d, ld=d + 2, dtype=TORCH[ydt])
            check(lib.cmve_l2norm_rows(h, X.ptr, xdt, d + 3, Y.ptr, ydt, d + 2, n, d, eps), "cmve_l2norm_rows")
            Y.assert_canary("y")
            if n == 0:
                Y.assert_untouched("y of an empty cmve_l2norm_rows")
                continue
            nrm = _norms(xs)
            with np.errstate(all="ignore"):
                want = xs.astype(LD) / (np.maximum(nrm, LD(eps)) if eps > 0 else nrm)[:, None]
            want64 = want.astype(np.float64)
            bound = (d / 64 + 8) * U52 * np.abs(want64)
            if ydt == F32:
                bound = bound + np.maximum(U24 * np.abs(want64), 2.0 ** -149)
            _within(Y.numpy(), want64, bound, f"n {n} eps {eps}")
            z = nrm == 0
            got = Y.numpy()
            assert np.isnan(got[z]).all() if eps == 0 else (got[z] == 0).all()


def test_l2norm_rows_refusals():
    h, lib, check, _ = _api()
    X, Y = Pad(2, 8, dtype=torch.float64, data=np.ones((2, 8))), Pad(2, 8, dtype=torch.float64)
    for args in ((None, F64, 8, Y.ptr, F64, 8, 2, 8, 0.0), (X.ptr, F64, 8, None, F64, 8, 2, 8, 0.0),
                 (X.ptr, F64, 7, Y.ptr, F64, 8, 2, 8, 0.0), (X.ptr, F64, 8, Y.ptr, F64, 7, 2, 8, 0.0),
                 (X.ptr, 2, 8, Y.ptr, F64, 8, 2, 8, 0.0), (X.ptr, F64, 8, Y.ptr, 3, 8, 2, 8, 0.0),
                 (X.ptr, F64, 8, Y.ptr, F64, 8, -1, 8, 0.0), (X.ptr, F64, 8, Y.ptr, F64, 8, 2, 0, 0.0)):
        assert lib.cmve_l2norm_rows(h, *args) != 0, args
        Y.assert_untouched("y of a refused cmve_l2norm_rows")
    assert lib.cmve_l2norm_rows(None, X.ptr, F64, 8, Y.ptr, F64, 8, 2, 8, 0.0) != 0


# ------------------------------------------------------------------ 3. cmve_gt_thresholds / cmve_rank_thresholds
A_FAMS = ("gauss", "const", "subn", "big", "zero")
B_FAMS = ("gauss", "absgauss", "const", "alt", "onehot", "small", "zero")
# CSR lists of the five a rows over the seven b rows (b row 6 and a row 4 are zero rows: NaN scores)
THR_LISTS = (
    [[0, 2, 3], [], [4], [6, 1, 5], [0, 1]],  # several; empty; one; one names a zero row; a zero a row
    [[6], [6, 6], [], [2], []],               # only zero rows, once and twice
)


def _thr_outputs(n_pad):
    return Pad(1, n_pad, dtype=torch.float64), Pad(1, n_pad), Pad(1, n_pad)


@pytest.mark.parametrize("adt,bdt", [(F32, F32), (F32, F64), (F64, F32), (F64, F64)])
@pytest.mark.parametrize("d", [3, 64, 65, 1000])
def test_thresholds_round_outwards(d, adt, bdt):
    """sgt = the maximum over the non-NaN GT of dot(raw_a, raw_b) (inv_a inv_b), against longdouble within (d + 8)
    2^-52 (|cos| <= 1: the bound is absolute); empty list NaN, all-NaN list +inf, rows [n, n_pad) NaN with both
    thresholds +inf.  With E = score_error_bound(err_a[row], err_max_b[mode], d_pad, mode) restated in fp64 from
    the device's words, thr_hi is the least fp32 >= sgt + E and thr_lo the greatest <= sgt - E, a relative 2^-50
    allowed in sgt +- E for the device's contraction: both round OUTWARDS.  cmve_rank_thresholds gives the same
    words from the same sgt.  d = 3 / 64 / 65 / 1000: a part of one lane step, one, one and an element, and the
    16-byte rows of wave_dot64."""
    h, lib, check, _ = _api()
    rng = np.random.default_rng(100 * d + 2 * adt + bdt)
    xa, xb = _rows(A_FAMS, rng, d, adt), _rows(B_FAMS, rng, d, bdt)
    a, b = Packed(xa, adt).pack(), Packed(xb, bdt).pack()
    ra, rb = a.result(), b.result()
    inv_a, inv_b = ra["inv"][:5].astype(LD), rb["inv"][:7].astype(LD)
    with np.errstate(all="ignore"):
        cos = (xa.astype(LD) @ xb.astype(LD).T) * (inv_a[:, None] * inv_b[None, :])
    assert np.isnan(cos[4]).all() and np.isnan(cos[:, 6]).all() and not np.isnan(cos[:4, :6]).any()
    for lists in THR_LISTS:
        off = torch.from_numpy(np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int64)).cuda()
        idx = torch.from_numpy(np.array([k for l in lists for k in l] + [0], np.int32)).cuda()
        want_sgt = np.full(a.n_pad, NAN)
        for i, l in enumerate(lists):
            if l:
                s = cos[i, l].astype(np.float64)
                want_sgt[i] = INF if np.isnan(s).all() else np.nanmax(s)
        for mode in MODES:
            sgt, hi, lo = _thr_outputs(a.n_pad)
            check(lib.cmve_gt_thresholds(h, ctypes.byref(a.rows), ctypes.byref(b.rows), mode, off.data_ptr(),
                                         idx.data_ptr(), sgt.ptr, hi.ptr, lo.ptr), "cmve_gt_thresholds")
            for p in (sgt, hi, lo):
                p.assert_canary("a threshold output")
            g_sgt, g_hi, g_lo = sgt.numpy()[0], hi.numpy()[0], lo.numpy()[0]
            _within(g_sgt, want_sgt, (d + 8) * U52, f"sgt {MODES[mode]}")
            assert (g_hi[5:] == INF).all() and (g_lo[5:] == INF).all()
            err_a = ra[("err_hi", "err_hilo", "err_h16")[mode]][:5]
            E = _E(err_a, rb["err_max"][mode], a.d_pad, mode)
            for i in range(5):
                s = g_sgt[i]
                if not s < INF:  # NaN (empty) or +inf (every GT NaN): never counted
                    assert g_hi[i] == INF and g_lo[i] == INF
                    continue
                up, dn = s + E[i], s - E[i]
                assert float(g_hi[i]) >= up - abs(up) * U50, f"thr_hi row {i} {MODES[mode]} below sgt + E"
                assert g_hi[i] <= _f32_up(up + abs(up) * U50), f"thr_hi row {i} {MODES[mode]} not the least fp32"
                assert float(g_lo[i]) <= dn + abs(dn) * U50, f"thr_lo row {i} {MODES[mode]} above sgt - E"
                assert g_lo[i] >= _f32_down(dn - abs(dn) * U50), f"thr_lo row {i} {MODES[mode]} not the greatest fp32"
            hi2, lo2 = Pad(1, a.n_pad), Pad(1, a.n_pad)
            check(lib.cmve_rank_thresholds(h, ctypes.byref(a.rows), ctypes.byref(b.rows), mode, sgt.ptr, hi2.ptr,
                                           lo2.ptr), "cmve_rank_thresholds")
            hi2.assert_canary("thr_hi")
            lo2.assert_canary("thr_lo")
            assert np.array_equal(hi2.numpy().view(np.uint32), hi.numpy().view(np.uint32))
            assert np.array_equal(lo2.numpy().view(np.uint32), lo.numpy().view(np.uint32))


def test_thresholds_refusals():
    """CMVE_PACK_RAW sets, mismatched d_pad, an unknown mode, a set without h16 asked for CMVE_SIM_F16, NULL
    outputs: refused by both entries, nothing written."""
    h, lib, check, Rows = _api()
    rng = np.random.default_rng(5)
    a = Packed(_rows(A_FAMS[:3], rng, 8, F64), F64).pack()
    b = Packed(_rows(B_FAMS[:3], rng, 8, F64), F64).pack()
    a_no16 = Packed(_rows(A_FAMS[:3], rng, 8, F64), F64, h16=False).pack()
    off = torch.tensor([0, 1, 2, 3], dtype=torch.int64, device="cuda")
    idx = torch.tensor([0, 1, 2], dtype=torch.int32, device="cuda")
    sgt, hi, lo = _thr_outputs(a.n_pad)
    sgt_in = torch.zeros(a.n_pad, dtype=torch.float64, device="cuda")

    def variant(src, **change):
        r = Rows()
        ctypes.memmove(ctypes.byref(r), ctypes.byref(src.rows), ctypes.sizeof(Rows))
        for k, v in change.items():
            setattr(r, k, v)
        return r

    cases = [(variant(a, flags=PACK_RAW), b.rows, F16), (a.rows, variant(b, flags=PACK_RAW), F16),
             (variant(a, d_pad=128), b.rows, F16), (a.rows, b.rows, 3), (a.rows, b.rows, -1), (a_no16.rows, b.rows, F16)]
    for ar, br, mode in cases:
        st = lib.cmve_gt_thresholds(h, ctypes.byref(ar), ctypes.byref(br), mode, off.data_ptr(), idx.data_ptr(),
                                    sgt.ptr, hi.ptr, lo.ptr)
        assert st != 0
        st = lib.cmve_rank_thresholds(h, ctypes.byref(ar), ctypes.byref(br), mode, sgt_in.data_ptr(), hi.ptr, lo.ptr)
        assert st != 0
        for p in (sgt, hi, lo):
            p.assert_untouched("an output of a refused threshold call")
    ar, br = ctypes.byref(a.rows), ctypes.byref(b.rows)
    for outs in ((None, hi.ptr, lo.ptr), (sgt.ptr, None, lo.ptr), (sgt.ptr, hi.ptr, None)):
        assert lib.cmve_gt_thresholds(h, ar, br, F16, off.data_ptr(), idx.data_ptr(), *outs) != 0
        assert lib.cmve_rank_thresholds(h, ar, br, F16, *outs) != 0
    assert lib.cmve_gt_thresholds(h, ar, br, F16, None, idx.data_ptr(), sgt.ptr, hi.ptr, lo.ptr) != 0
    assert lib.cmve_gt_thresholds(None, ar, br, F16, off.data_ptr(), idx.data_ptr(), sgt.ptr, hi.ptr, lo.ptr) != 0
    for p in (sgt, hi, lo):
        p.assert_untouched("an output of a refused threshold call")


# ------------------------------------------------------------------ 4. |s~ - cos| <= E where it is tight
def _pairing(name, rng, d, dt):
    """5 query rows and 7 gallery rows of the pairing."""
    if name == "const":  # cosine 1, every element's error the same: the aligned case
        return _rows(["const"] * 5, rng, d, dt), _rows(["const"] * 7, rng, d, dt)
    if name == "absgauss":  # against themselves: cosine 1 on the diagonal, about 2 / pi off it, errors of one sign
        g = _rows(["absgauss"] * 7, rng, d, dt)
        return g[:5].copy(), g
    if name == "alt":  # against their own negation: cosine near -1
        g = _rows(["alt"] * 7, rng, d, dt)
        return g[:5].copy(), -g
    return _rows(["subn"] * 5, rng, d, dt), _rows(["gauss"] * 7, rng, d, dt)


@pytest.mark.parametrize("pairing", ["const", "absgauss", "alt", "subn"])
@pytest.mark.parametrize("d", [1, 31, 64, 65, 1000, 1536])
def test_score_within_bound_on_aligned_rows(d, pairing):
    """cmve_sim_store (alpha 1, beta 0, fp32 out, ldo = 10 for 7 columns) in the three modes against the
    longdouble cosine of the raw rows.  The bound is E(err[i], err[j]) from the device's per-row planes
    (score_error_bound restated) plus the half-ulp of the fp32 store.  The test prints max |s~ - cos| / E per
    mode; DESIGN.md s7 records the maxima."""
    h, lib, check, _ = _api()
    dt = F64 if d % 2 else F32
    rng = np.random.default_rng(1000 + d)
    xq, xg = _pairing(pairing, rng, d, dt)
    q, g = Packed(xq, dt).pack(), Packed(xg, dt).pack()
    rq, rg = q.result(), g.result()
    cos = ((xq.astype(LD) @ xg.astype(LD).T) / (_norms(xq)[:, None] * _norms(xg)[None, :])).astype(np.float64)
    if pairing == "subn" and d == 1000:  # the family is what it says, counted on the host
        sub = rq["h16"][:5, :d].view(np.float16)
        n_sub = ((np.abs(sub) < 2.0 ** -14)).sum(axis=1)
        assert (n_sub > 200).all(), n_sub
    for mode in MODES:
        key = ("err_hi", "err_hilo", "err_h16")[mode]
        E = _E(rq[key][:5, None], rg[key][None, :7], q.d_pad, mode)
        out = Pad(5, 7, ld=10)
        check(lib.cmve_sim_store(h, ctypes.byref(q.rows), ctypes.byref(g.rows), mode, 1.0, 0.0, out.ptr, F32, 10),
              "cmve_sim_store")
        out.assert_canary("scores")
        got = out.numpy().astype(np.float64)
        ratio = np.abs(got - cos) / E
        print(f"RATIO pairing={pairing} d={d} mode={MODES[mode]} max={ratio.max():.4f}")
        _within(got, cos, E + U24 * np.abs(got), f"{pairing} d {d} {MODES[mode]}: |s~ - cos| / E up to {ratio.max():.3f}")
