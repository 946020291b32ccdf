"""K4a (cmve_sim_store: EPI_STORE) and K3 (cmve_linear: EPI_BIAS / EPI_LINEAR) through the C ABI, in the three
tile geometries of sim.hip's one MFMA kernel and its three precisions.

Operands are packed by cmve_pack_rows (ordinary packing for cmve_sim_store, CMVE_PACK_RAW for cmve_linear, lo and
h16 planes always) and handed to the GEMM as descriptor VIEWS of one packed set: n <= n_pad, n_pad % 128 == 0,
plane pointers advanced by whole rows (what topk.hip and dist.py pass).  launch_sim picks the geometry from the two
n_pad alone (_phased / _g64 restate its rule), so one pack serves many shapes and each call asserts the geometry it
takes.  Every output, bias, BN column and residual is a window of a canary buffer, checked after every call.

Reference and bound, both from the planes the device stored (read back, exact in fp64): S = the sum over d_pad of
the plane products the mode multiplies (BF16 hi.hi, F16 h16.h16, BF16X3 hi.hi + hi.lo + lo.hi), A = the same sum
over absolute values; the accumulator is within gamma A of S with gamma = n u / (1 - n u), u = 2^-23, n = d_pad
33/32 (x 3 for BF16X3): score_error_bound's gamma, taken from _E.  Each fp32 step of an epilogue (alpha *, + beta,
+ bias, + resid, * bn_scale, + bn_shift) adds 2^-23 |its result| (one rounding is 2^-24: an fma contraction cannot
matter); errors pass through alpha, bn_scale and the activations' Lipschitz constants (ReLU 1, sigmoid 1 / 4,
QuickGELU 1.1 >= sup |f'| = 1.0998 near 1.702 v = 2.4); the expf step of QuickGELU / sigmoid gets what
test_activations_edges allows these expressions: rtol 1e-6, atol 1e-7 on the activation's output.

THE BOUND CAN FAIL: before each GPU call the test asserts on the CPU that four wrong results lie outside the bound
in at least one element of every tile compared -- S without the last 32 real values of k, S without the hi.lo term
(BF16X3), the bias / the BN pair of the tile one tile width to the left, the residual read at ldo instead of ldr.
For that every fourth row (0, 4, ...) on both sides is of a constant family (its lo plane has one sign per level, so
the cross term does not average out as it does on Gaussian rows) and bias / BN / residual values are functions of
the indices.  At d = 1 under ordinary packing every row is +-1, every lo word 0 and the cross term identically 0:
there the test asserts that instead.

Each call prints RATIO geo mode epi max |got - want| / bound; DESIGN.md s7 records the maxima.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from _windows import Pad, _within, _E, _phased, _g64

pytestmark = pytest.mark.gpu

F32, F64 = 0, 1
TORCH = {F32: torch.float32, F64: torch.float64}
BF16, BF16X3, F16 = 0, 1, 2
MODES = {BF16: "bf16", BF16X3: "bf16x3", F16: "f16"}
PACK_RAW = 1
U23 = 2.0 ** -23
TILE = {"g64": 64, "g128": 128, "g256": 256}
ACT_L = {0: 1.0, 1: 1.0, 2: 1.1, 3: 0.25}
GELU_C = float(np.float32(1.702))
AB = ((1.0, 0.0), (-1.0, 1.0), (100.0, 0.0), (-1.0, 0.0))  # the (alpha, beta) pairs cmve.h lists


def _api():
    from cmve import engine
    from cmve._lib import lib, check, Rows
    return engine.handle(), lib, check, Rows


def _geo(nq_pad, ng_pad):
    return "g256" if _phased(nq_pad, ng_pad) else ("g64" if _g64(nq_pad, ng_pad) else "g128")


# ------------------------------------------------------------------ rows and packed sets
LEVELS = ((1.0, 3.0), (1.0, 5.0), (2.0, 7.0))


def _make_rows(n, d, seed, raw, scale=1.0, cscale=1.0):
    """Gaussian rows (times scale); every fourth row of a constant family.  Raw operands: 0.37 cscale times a small
    integer, positive (the product of two such rows passes ReLU).  Rows that cmve_pack_rows normalises: two levels
    alternating along k (one constant would normalise to 1 / sqrt(d), a power of two at d = 64 and 256 with an
    all-zero lo plane), the sign alternating from one such row to the next."""
    x = np.random.default_rng(seed).standard_normal((n, d)) * scale
    for r in range(0, n, 4):
        m = r // 4
        if raw:
            x[r] = 0.37 * (1 + m % 5) * cscale
        else:
            a, b = LEVELS[m % 3]
            x[r] = np.where(np.arange(d) % 2 == 0, a, b) * 0.37 * (-1) ** (m // 3 % 2)
    return x.astype(np.float32)


class Set:
    """x [n, d] fp32 packed by cmve_pack_rows with lo and h16 planes; hi / lo / h16: the stored planes in fp64."""

    def __init__(self, x, raw):
        h, lib, check, Rows = _api()
        self.n, self.d = x.shape
        np_, dp_ = ctypes.c_int64(), ctypes.c_int64()
        check(lib.cmve_pack_size(self.n, self.d, ctypes.byref(np_), ctypes.byref(dp_)), "cmve_pack_size")
        self.n_pad, self.d_pad = np_.value, dp_.value
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
        self.raw = torch.from_numpy(np.ascontiguousarray(x)).cuda()
        self.planes = z((3, self.n_pad, self.d_pad), torch.int16)
        self.inv, self.err, self.err_max = z(self.n_pad, torch.float64), z((3, self.n_pad), torch.float32), \
            z(3, torch.float32)
        r = Rows()
        r.n, r.d, r.n_pad, r.d_pad = self.n, self.d, self.n_pad, self.d_pad
        r.hi, r.lo, r.h16 = (self.planes[k].data_ptr() for k in range(3))
        r.raw, r.raw_dtype, r.flags, r.raw_ld, r.eps = self.raw.data_ptr(), F32, (PACK_RAW if raw else 0), self.d, 0.0
        r.inv_norm, r.err_max = self.inv.data_ptr(), self.err_max.data_ptr()
        r.err_hi, r.err_hilo, r.err_h16 = (self.err[k].data_ptr() for k in range(3))
        check(lib.cmve_pack_rows(h, ctypes.byref(r)), "cmve_pack_rows")
        self.rows = r
        w = self.planes.cpu().numpy().view(np.uint16)
        bf = lambda b: (b.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
        self.hi, self.lo, self.h16 = bf(w[0]), bf(w[1]), w[2].view(np.float16).astype(np.float64)
        assert not w[:, self.n:].any() and not w[:, :, self.d:].any(), "padding rows and columns are zero words"

    def view(self, r0, rows, rows_pad, **change):
        """The descriptor of rows [r0, r0 + rows) with rows_pad padded rows, plane pointers advanced by r0 whole rows;
        change: fields overwritten after that (the refusals)."""
        _, _, _, Rows = _api()
        assert r0 + rows_pad <= self.n_pad and r0 + rows <= self.n and rows <= rows_pad
        r = Rows()
        ctypes.memmove(ctypes.byref(r), ctypes.byref(self.rows), ctypes.sizeof(Rows))
        r.n, r.n_pad = rows, rows_pad
        r.hi, r.lo, r.h16 = (self.planes[k].data_ptr() + r0 * self.d_pad * 2 for k in range(3))
        for k, v in change.items():
            setattr(r, k, v)
        return r


@functools.lru_cache(maxsize=None)
def _packed(n, d, seed, raw, scale=1.0, cscale=1.0):
    return Set(_make_rows(n, d, seed, raw, scale, cscale), raw)


def _gamma(d_pad, mode):
    return _E(0.0, 0.0, d_pad, mode) - 1e-12  # score_error_bound with both row bounds 0, less its constant


def _products(q, g, mode, qi, gi, drop_k=False, cross=True):
    """S and A [len(qi), len(gi)] over the stored planes of rows qi of q and gi of g.  drop_k: without the last 32
    values of k below d; cross = False: without the hi.lo term."""
    k1 = q.d - min(32, q.d) if drop_k else q.d_pad
    if mode == F16:
        pairs = [(q.h16, g.h16)]
    elif mode == BF16:
        pairs = [(q.hi, g.hi)]
    else:
        pairs = [(q.hi, g.hi), (q.lo, g.hi)] + ([(q.hi, g.lo)] if cross else [])
    S = A = 0.0
    with np.errstate(invalid="ignore"):
        for a, b in pairs:
            a, b = a[qi, :k1], b[gi, :k1]
            S = S + a @ b.T
            A = A + np.abs(a) @ np.abs(b).T
    return S, A


def _step(v, e):
    """One fp32 operation whose exact result is v, on operands off by e in all."""
    with np.errstate(invalid="ignore"):
        return e + U23 * (np.abs(v) + e)


def _store_want(S, A, d_pad, mode, alpha, beta):
    e = abs(alpha) * _gamma(d_pad, mode) * A
    p = alpha * S
    e = _step(p, e)
    v = p + beta
    return v, _step(v, e)


def _act(v, relu):
    with np.errstate(all="ignore"):
        if relu == 1:
            return np.maximum(v, 0.0)  # torch.relu: a NaN passes
        if relu == 2:
            return v / (1.0 + np.exp(-GELU_C * v))
        if relu == 3:
            return 1.0 / (1.0 + np.exp(-v))
    return v


def _linear_want(S, A, d_pad, mode, bias, relu, resid, bn):
    """BN(resid + act(S + bias)) in fp64 and its bound; bias [F], resid [rows, F], bn = (scale, shift) or None."""
    with np.errstate(invalid="ignore", over="ignore"):
        e = _gamma(d_pad, mode) * A
        v = S + (0.0 if bias is None else bias[None, :])
        e = _step(v, e)
        v = _act(v, relu)
        if relu >= 2:
            e = ACT_L[relu] * e + 1e-6 * np.abs(v) + 1e-7
        if resid is not None:
            v = resid + v
            e = _step(v, e)
        if bn is not None:
            p = v * bn[0][None, :]
            e = _step(p, np.abs(bn[0])[None, :] * e)
            v = p + bn[1][None, :]
            e = _step(v, e)
    return v, e


def _must_fail(wrong, want, bound, rows, tile, what):
    """The wrong result is outside the bound (or non-finite where the want is finite) in at least one element of
    every tile x tile block of the compared elements; rows: the rows' indices in the output."""
    with np.errstate(invalid="ignore"):
        fw, fr = np.isfinite(want), np.isfinite(wrong)
        bad = fw & ((fr & (np.abs(wrong - want) > bound)) | ~fr)
    rt = np.asarray(rows) // tile
    nc = -(-bad.shape[1] // tile)
    padded = np.zeros((bad.shape[0], nc * tile), bool)
    padded[:, :bad.shape[1]] = bad
    for t in np.unique(rt):
        hit = padded[rt == t].reshape(-1, nc, tile).any(axis=(0, 2))
        assert hit.all(), f"{what}: inside the bound in all of row tile {t}, column tiles {np.flatnonzero(~hit)[:8]}"


def _sample_rows(n, tile):
    """The first and the last valid row of every row tile and one row of each of its 16-row MFMA blocks."""
    rows = set()
    for t in range(-(-n // tile)):
        lo, hi = t * tile, min(n, (t + 1) * tile)
        rows |= {lo, hi - 1}
        rows |= {r for r in (lo + i * 16 + (5 * i + t) % 16 for i in range(tile // 16)) if r < hi}
    return np.array(sorted(rows))


def _ratio(got, want, bound):
    fin = np.isfinite(want) & (bound > 0)
    return float((np.abs(got[fin] - want[fin]) / bound[fin]).max()) if fin.any() else 0.0


def _gather(pad, rows):
    return pad.t[torch.from_numpy(np.asarray(rows)).cuda()].cpu().numpy().astype(np.float64)


# ------------------------------------------------------------------ cmve_sim_store
def _store(q, g, qv, gv, mode, ab=(1.0, 0.0), geo="g64", dts=(F32,), rows=None, what=""):
    """One cmve_sim_store of the views qv = (r0, n, n_pad) of q and gv of g per out_dtype, ldo = ng + 3, compared on
    `rows` (all by default); with both dtypes the fp64 output holds exactly the fp32 words.  Returns the Pads."""
    h, lib, check, _ = _api()
    (r0, n, nq_pad), (c0, ng, ng_pad) = qv, gv
    qd, gd = q.view(*qv), g.view(*gv)
    assert _geo(nq_pad, ng_pad) == geo, f"{what}: takes {_geo(nq_pad, ng_pad)}"
    rows = np.arange(n) if rows is None else rows
    what = f"{what} {geo} {MODES[mode]} store n {n} ng {ng} d {q.d} ab {ab}"
    qi, gi = r0 + rows, np.arange(c0, c0 + ng)
    S, A = _products(q, g, mode, qi, gi)
    want, bound = _store_want(S, A, q.d_pad, mode, *ab)
    tile = TILE[geo]
    wrong, _ = _store_want(_products(q, g, mode, qi, gi, drop_k=True)[0], A, q.d_pad, mode, *ab)
    _must_fail(wrong, want, bound, rows, tile, f"{what}: the last 32 k dropped")
    if mode == BF16X3:
        if q.d == 1 and not (q.rows.flags & PACK_RAW):
            assert not q.lo.any() and not g.lo.any()  # unit rows of one element: +-1, no residual, no cross term
        else:
            wrong, _ = _store_want(_products(q, g, mode, qi, gi, cross=False)[0], A, q.d_pad, mode, *ab)
            _must_fail(wrong, want, bound, rows, tile, f"{what}: hi.lo dropped")
    outs = {}
    for dt in dts:
        out = Pad(n, ng, ld=ng + 3, dtype=TORCH[dt])
        check(lib.cmve_sim_store(h, ctypes.byref(qd), ctypes.byref(gd), mode, ab[0], ab[1], out.ptr, dt, ng + 3),
              "cmve_sim_store")
        out.assert_canary(f"{what} out")
        got = _gather(out, rows)
        print(f"RATIO geo={geo} mode={MODES[mode]} epi=store dt={dt} d={q.d} max={_ratio(got, want, bound):.4f}")
        _within(got, want, bound, f"{what} dt {dt}")
        outs[dt] = out
    if len(outs) == 2:
        assert torch.equal(outs[F64].t, outs[F32].t.double()), f"{what}: fp64 output is not the fp32 words"
    return outs


@pytest.mark.parametrize("d", [1, 63, 64, 65, 192, 256, 320, 448])
def test_store_k_loop_g64(d):
    """G64 ring (Geo<4, 1, 1>, EPI_STORE, 4 stages): nk0 = d_pad / 64 = 1, 1, 1, 2, 3 never fill the ring, 4 fills
    it, 5 and 7 wrap it (the refill of K-tile t - 1's buffer); 256 x 2048 rows (4 x 32 tiles), the three modes."""
    q, g = _packed(256, d, 1, False), _packed(2048, d, 2, False)
    assert q.d_pad // 64 == {1: 1, 63: 1, 64: 1, 65: 2, 192: 3, 256: 4, 320: 5, 448: 7}[d]
    for mode in MODES:
        _store(q, g, (0, 256, 256), (0, 2048, 2048), mode, geo="g64")


@pytest.mark.parametrize("d", [64, 128, 192])
def test_store_k_loop_g128(d):
    """G128 2-stage loop (Geo<2, 2, 4>, EPI_STORE): nk0 = 1 (no second stage), 2, 3; 256 x 8192 rows (2 x 64
    tiles: the first grid that leaves G64), the three modes."""
    q, g = _packed(4096, d, 3, False), _packed(8192, d, 4, False)
    for mode in MODES:
        _store(q, g, (512, 256, 256), (0, 8192, 8192), mode, geo="g128")


@pytest.mark.parametrize("d", [64, 128, 192])
def test_store_k_loop_g256(d):
    """Persistent G256 (Geo<2, 4, 8>, phased, EPI_STORE) at 4096 x 8192: 512 tiles, the smallest persistent grid,
    two tiles per block on 256 CUs.  nk = 1, 2, 3 in BF16 / F16 (the prologue's `nk > 1` and the `t + 2 < nk`
    refill at their first values) and 3, 6, 9 in BF16X3 (plane_of's walk).  Compared on _sample_rows of every row
    tile, all columns; test_bit_identity_store compares the whole output with G128's."""
    q, g = _packed(4096, d, 3, False), _packed(8192, d, 4, False)
    for mode in MODES:
        _store(q, g, (0, 4096, 4096), (0, 8192, 8192), mode, geo="g256", rows=_sample_rows(4096, 256))


MASK_N = (1, 63, 64, 65, 127, 129, 256)


@pytest.mark.parametrize("n", MASK_N)
def test_store_masks_g64(n):
    """G64, d = 320 (nk0 = 5): n x ng over {1, 63, 64, 65, 127, 129, 256}^2, ldo = ng + 3, fp32 and fp64 output;
    the views take n_pad = 128, 256 and 384 (padded tiles wholly masked; 128 and 384 are no multiple of 256) from
    row offsets 0, 128 and 256, the modes and the (alpha, beta) pairs cycle."""
    q, g = _packed(640, 320, 5, False), _packed(2560, 320, 6, False)
    for k, ng in enumerate(MASK_N):
        c = k + MASK_N.index(n)
        nq_pad = max(128 * (1 + c % 3), -(-n // 128) * 128)
        ng_pad = max((128, 384, 2048, 256)[c % 4], -(-ng // 128) * 128)
        _store(q, g, (128 * (c % 3), n, nq_pad), (128 * (k % 3), ng, ng_pad), c % 3, ab=AB[c % 4], geo="g64",
               dts=(F32, F64))


@pytest.mark.parametrize("n", [127, 128, 129])
def test_store_masks_g128(n):
    """G128, d = 65 (nk0 = 2): 127 / 128 / 129 of 256 padded rows against 8192 and 8065 columns (the last column
    tile one row short), ldo = ng + 3, both output dtypes."""
    q, g = _packed(4096, 65, 7, False), _packed(8192, 65, 8, False)
    for k, ng in enumerate((8192, 8065)):
        _store(q, g, (256, n, 256), (0, ng, 8192), (n + k) % 3, ab=AB[(n + k) % 4], geo="g128", dts=(F32, F64))


@pytest.mark.parametrize("n,ng,mode,ab", [(1, 8192, BF16, AB[1]), (3841, 7937, BF16X3, AB[2]),
                                          (3841, 8192, F16, AB[3])])
def test_store_masks_g256(n, ng, mode, ab):
    """Persistent G256, d = 64: one valid row of 4096 padded ones (every other row of 16 row tiles masked), 3841
    rows (one row into the last row tile) and 7937 columns (one into the last column tile), ldo = ng + 3, both
    output dtypes; compared on _sample_rows."""
    q, g = _packed(4096, 64, 3, False), _packed(8192, 64, 4, False)
    _store(q, g, (0, n, 4096), (0, ng, 8192), mode, ab=ab, geo="g256", dts=(F32, F64), rows=_sample_rows(n, 256))


# ------------------------------------------------------------------ cmve_linear
def _bias_col(F):
    return (((np.arange(F) * 37) % 1021) / 1021.0 - 0.3).astype(np.float32)


def _bn_cols(F):
    j = np.arange(F)
    s = (0.5 + ((j * 53) % 1019) / 1019.0) * np.where(j % 7 == 3, -1.0, 1.0)
    return s.astype(np.float32), (((j * 29) % 1013) / 1013.0 - 0.5).astype(np.float32)


def _resid_at(i, j):
    """The residual's value at row i, column j: exact in fp32."""
    return ((np.asarray(i)[:, None] * 7 + np.asarray(j)[None, :] * 13) % 101 - 50) / 64.0


class Operands:
    """bias, BN pair, residual (ldr = F + 5) and output (ldo = F + 3) of an n x F cmve_linear, each a canary window
    or absent; the residual is filled on the device from _resid_at's rule."""

    def __init__(self, n, F, bias, resid, bn, bias_vals=None):
        self.n, self.F, self.ldo, self.ldr = n, F, F + 3, F + 5
        self.bias_v = (_bias_col(F) if bias_vals is None else bias_vals) if bias else None
        self.bn_v = _bn_cols(F) if bn else None
        self.bias = Pad(1, F, data=self.bias_v[None]) if bias else None
        self.bn = tuple(Pad(1, F, data=v[None]) for v in self.bn_v) if bn else None
        self.resid = None
        if resid:
            self.resid = Pad(n, F, ld=self.ldr)
            i, j = torch.arange(n, device="cuda")[:, None], torch.arange(F, device="cuda")[None, :]
            self.resid.t.copy_((((i * 7 + j * 13) % 101 - 50).double() / 64.0).float())
        self.out = Pad(n, F, ld=self.ldo)

    def ptrs(self, r0=0, c0=0, out=None):
        """(bias, bn_scale, bn_shift, resid, out) of the sub-problem whose first element is (r0, c0)."""
        at = lambda p, off: None if p is None else ctypes.c_void_p(p.ptr.value + 4 * off)
        bn = self.bn or (None, None)
        return at(self.bias, c0), at(bn[0], c0), at(bn[1], c0), at(self.resid, r0 * self.ldr + c0), \
            at(out or self.out, r0 * self.ldo + c0)

    def resid_rows(self, rows, ld=None):
        """The residual of `rows` as the kernel reads it with leading dimension ld (ldr: its values; another: what
        lies there, NaN in the gap columns)."""
        if self.resid is None:
            return None
        if ld is None or ld == self.ldr:
            return _resid_at(rows, np.arange(self.F))
        flat = np.asarray(rows)[:, None] * ld + np.arange(self.F)[None, :]
        i, j = flat // self.ldr, flat % self.ldr
        with np.errstate(invalid="ignore"):
            return np.where(j < self.F, ((i * 7 + j * 13) % 101 - 50) / 64.0, np.nan)

    def assert_canaries(self, what):
        for p in (self.bias, self.resid, self.out) + (self.bn or ()):
            if p is not None:
                p.assert_canary(what)


def _linear(x, w, xv, wv, mode, relu, ops, geo, epi, rows=None, what=""):
    """One cmve_linear of the views xv of x and wv of w into ops.out, compared on `rows` of the output."""
    h, lib, check, _ = _api()
    (r0, n, nx_pad), (c0, F, nw_pad) = xv, wv
    assert (n, F) == (ops.n, ops.F)
    xd, wd = x.view(*xv), w.view(*wv)
    assert _geo(nx_pad, nw_pad) == geo, f"{what}: takes {_geo(nx_pad, nw_pad)}"
    # cmve_linear's rule: bias (+ ReLU) alone is EPI_BIAS, anything else EPI_LINEAR
    took = "bias" if ops.resid is None and ops.bn is None and relu <= 1 else "linear"
    assert took == epi, f"{what}: takes EPI_{took.upper()}"
    rows = np.arange(n) if rows is None else rows
    what = f"{what} {geo} {MODES[mode]} {epi} relu {relu} bias {ops.bias is not None} resid " \
           f"{ops.resid is not None} bn {ops.bn is not None} K {x.d}"
    xi, wi = r0 + rows, np.arange(c0, c0 + F)
    S, A = _products(x, w, mode, xi, wi)
    res = ops.resid_rows(rows)
    want, bound = _linear_want(S, A, x.d_pad, mode, ops.bias_v, relu, res, ops.bn_v)
    tile = TILE[geo]
    mutants = {"the last 32 k dropped": dict(S=_products(x, w, mode, xi, wi, drop_k=True)[0])}
    if mode == BF16X3:
        mutants["hi.lo dropped"] = dict(S=_products(x, w, mode, xi, wi, cross=False)[0])
    if ops.bias is not None:
        mutants["the bias of the tile to the left"] = dict(bias=np.roll(ops.bias_v, tile))
    if ops.bn is not None:
        mutants["the BN pair of the tile to the left"] = dict(bn=tuple(np.roll(v, tile) for v in ops.bn_v))
    if ops.resid is not None:
        mutants["resid at ldo"] = dict(resid=ops.resid_rows(rows, ops.ldo))
    for name, ch in mutants.items():
        arg = dict(S=S, bias=ops.bias_v, resid=res, bn=ops.bn_v)
        arg.update(ch)
        wrong, _ = _linear_want(arg["S"], A, x.d_pad, mode, arg["bias"], relu, arg["resid"], arg["bn"])
        _must_fail(wrong, want, bound, rows, tile, f"{what}: {name}")
    b, s, t, r, o = ops.ptrs()
    check(lib.cmve_linear(h, ctypes.byref(xd), ctypes.byref(wd), mode, b, s, t, r, ops.ldr, relu, o, ops.ldo),
          "cmve_linear")
    ops.assert_canaries(what)
    got = _gather(ops.out, rows)
    print(f"RATIO geo={geo} mode={MODES[mode]} epi={epi} relu={relu} K={x.d} max={_ratio(got, want, bound):.4f}")
    _within(got, want, bound, what)
    return got, want


def _xw(n, F, K, seed):
    """Raw operands of an n x F projection over K: x of unit scale, w's Gaussian rows of scale 1 / sqrt(K) and its
    constant rows of 1 / K: x.w of unit scale on every kind of pair (no activation saturates)."""
    return _packed(n, K, seed, True), _packed(F, K, seed + 1, True, 1.0 / np.sqrt(K), 1.0 / K)


@pytest.mark.parametrize("relu", [0, 1, 2, 3])
def test_linear_epilogue_matrix_g64(relu):
    """G64 ring, 65 x 129 (2 x 3 tiles, the last of each one row / column wide), K = 65 (nk0 = 2), BF16X3: bias
    NULL / given x resid NULL / given (ldr = F + 5, ldo = F + 3) x BN NULL / given, in the order BN(resid + act(x.w
    + b)).  EPI_BIAS exactly when relu <= 1 with neither resid nor BN, EPI_LINEAR otherwise."""
    x, w = _xw(65, 129, 65, 20)
    for bias in (False, True):
        for resid in (False, True):
            for bn in (False, True):
                epi = "bias" if relu <= 1 and not resid and not bn else "linear"
                _linear(x, w, (0, 65, 256), (0, 129, 256), BF16X3, relu, Operands(65, 129, bias, resid, bn), "g64", epi)


@pytest.mark.parametrize("mode", [BF16, F16])
def test_linear_single_plane_modes_g64(mode):
    """The same shape in BF16 and F16 (one plane pair per K-tile): EPI_BIAS with ReLU, EPI_LINEAR with sigmoid +
    resid + BN."""
    x, w = _xw(65, 129, 65, 20)
    _linear(x, w, (0, 65, 256), (0, 129, 256), mode, 1, Operands(65, 129, True, False, False), "g64", "bias")
    _linear(x, w, (0, 65, 256), (0, 129, 256), mode, 3, Operands(65, 129, True, True, True), "g64", "linear")


@pytest.mark.parametrize("relu,resid,bn", [(0, False, False), (1, False, False), (1, True, False), (2, True, False),
                                           (3, True, False), (1, True, True)])
def test_linear_non_finite(relu, resid, bn):
    """65 x 129, K = 65, BF16X3 on G64: row 7 of x is NaN, row 70 of w is NaN, bias[100] = +inf.  Output row 7 and
    column 70 are NaN and nothing else is (a NaN passes through ReLU as through torch.relu); column 100 is +inf
    through identity, ReLU and QuickGELU, 1 + resid through sigmoid."""
    xs, ws = _make_rows(65, 65, 30, True), _make_rows(129, 65, 31, True, 1.0 / np.sqrt(65), 1.0 / 65)
    xs[7], ws[70] = np.nan, np.nan
    x, w = Set(xs, True), Set(ws, True)
    bias = _bias_col(129)
    bias[100] = np.inf
    ops = Operands(65, 129, True, resid, bn, bias_vals=bias)
    epi = "bias" if relu <= 1 and not resid and not bn else "linear"
    got, _ = _linear(x, w, (0, 65, 256), (0, 129, 256), BF16X3, relu, ops, "g64", epi)
    nan = np.zeros((65, 129), bool)
    nan[7], nan[:, 70] = True, True
    assert np.array_equal(np.isnan(got), nan), "NaN outside row 7 / column 70, or missing inside"
    col = np.delete(got[:, 100], 7)
    if bn:
        assert (col == -np.inf).all() if _bn_cols(129)[0][100] < 0 else (col == np.inf).all()
    elif relu == 3:
        assert np.array_equal(col, np.delete(1.0 + _resid_at(np.arange(65), [100])[:, 0], 7))
    else:
        assert (col == np.inf).all()


def _linear_big(geo, K, cfg):
    relu, bias, resid, bn, epi = cfg
    n, F = (4096, 8192) if geo == "g256" else (256, 8192)
    x, w = _xw(4096, 8192, K, 40)
    ops = Operands(n, F, bias, resid, bn)
    rows = np.array(sorted({r for t in range(n // TILE[geo]) for r in (t * TILE[geo], (t + 1) * TILE[geo] - 1)}))
    _linear(x, w, (0, n, n), (0, F, F), BF16X3, relu, ops, geo, epi, rows=rows)
    return x, w, ops


CFG_BIAS = (1, True, False, False, "bias")        # ReLU(x.w + b)
CFG_LINEAR = (2, True, True, True, "linear")      # BN(resid + QuickGELU(x.w + b))


@pytest.mark.parametrize("cfg", [CFG_BIAS, CFG_LINEAR], ids=["bias", "linear"])
def test_linear_g128(cfg):
    """G128 2-stage loop, 256 x 8192, BF16X3 at K = 64 (one K-tile: the three plane pairs once): EPI_BIAS with ReLU
    and EPI_LINEAR with QuickGELU + resid + BN, column-indexed bias / BN; the first and last row of both row tiles
    against the reference."""
    _linear_big("g128", 64, cfg)


def _blocks_linear(x, w, ops, relu, out, blocks, cols, geo):
    """Recompute row blocks of 256 (against the column ranges `cols` of w) of ops' problem through views, into
    `out`: a window of all of ops' rows, or of the one block's."""
    h, lib, check, _ = _api()
    at = lambda p, off: None if p is None else ctypes.c_void_p(p.ptr.value + 4 * off)
    bn = ops.bn or (None, None)
    for bk in blocks:
        r0 = 256 * bk
        o0 = r0 if out.t.shape[0] == ops.n else 0
        for c0, nc in cols:
            xd, wd = x.view(r0, 256, 256), w.view(c0, nc, nc)
            assert _geo(256, nc) == geo
            check(lib.cmve_linear(h, ctypes.byref(xd), ctypes.byref(wd), BF16X3, at(ops.bias, c0), at(bn[0], c0),
                                  at(bn[1], c0), at(ops.resid, r0 * ops.ldr + c0), ops.ldr, relu,
                                  at(out, o0 * ops.ldo + c0), ops.ldo), "cmve_linear")


@pytest.mark.parametrize("cfg,K", [(CFG_BIAS, 64), (CFG_LINEAR, 192)], ids=["bias-K64", "linear-K192"])
def test_linear_g256_and_bit_identity(cfg, K):
    """Persistent G256, 4096 x 8192, BF16X3: nk = 3 (K = 64) and 9 (K = 192).  Every block walks two tiles, so the
    second tile's bias / BN columns are the ones fetch_cols prefetched under the first tile's epilogue (the CPU
    check: the columns of the tile 256 to the left are outside the bound in every tile).  Sample rows against the
    reference; then the WHOLE output bit for bit against 16 row-block views that take G128, and block 5 against
    four column views of 2048 that take G64: launch_sim's "same MFMA sequence in every geometry", which
    combine_batches' bit-equality rests on."""
    x, w, ops = _linear_big("g256", K, cfg)
    relu = cfg[0]
    o128 = Pad(4096, 8192, ld=ops.ldo)
    _blocks_linear(x, w, ops, relu, o128, range(16), [(0, 8192)], "g128")
    o128.assert_canary("G128 blocks")
    assert torch.equal(ops.out.t, o128.t), "G256 and G128 differ in some bit"
    del o128
    o64 = Pad(256, 8192, ld=ops.ldo)
    _blocks_linear(x, w, ops, relu, o64, [5], [(2048 * c, 2048) for c in range(4)], "g64")
    o64.assert_canary("G64 blocks")
    assert torch.equal(ops.out.t[1280:1536], o64.t), "G256 and G64 differ in some bit"


@pytest.mark.parametrize("mode", list(MODES))
def test_bit_identity_store(mode):
    """cmve_sim_store at 4096 x 8192, d = 192 (nk0 = 3), alpha 100: the persistent G256 output bit for bit against
    16 row-block views of 256 that take G128, and block 5 against four column views of 2048 that take G64."""
    h, lib, check, _ = _api()
    q, g = _packed(4096, 192, 3, False), _packed(8192, 192, 4, False)
    ld = 8195
    o256 = _store(q, g, (0, 4096, 4096), (0, 8192, 8192), mode, ab=AB[2], geo="g256", rows=_sample_rows(4096, 256))[F32]
    o128, o64 = Pad(4096, 8192, ld=ld), Pad(256, 8192, ld=ld)
    for bk in range(16):
        assert _geo(256, 8192) == "g128"
        check(lib.cmve_sim_store(h, ctypes.byref(q.view(256 * bk, 256, 256)), ctypes.byref(g.view(0, 8192, 8192)), mode,
                                 100.0, 0.0, ctypes.c_void_p(o128.ptr.value + 4 * 256 * bk * ld), F32, ld), "cmve_sim_store")
    o128.assert_canary("G128 blocks")
    assert torch.equal(o256.t, o128.t), "G256 and G128 differ in some bit"
    for c in range(4):
        assert _geo(256, 2048) == "g64"
        check(lib.cmve_sim_store(h, ctypes.byref(q.view(1280, 256, 256)), ctypes.byref(g.view(2048 * c, 2048, 2048)),
                                 mode, 100.0, 0.0, ctypes.c_void_p(o64.ptr.value + 4 * 2048 * c), F32, ld), "cmve_sim_store")
    o64.assert_canary("G64 blocks")
    assert torch.equal(o256.t[1280:1536], o64.t), "G256 and G64 differ in some bit"


# ------------------------------------------------------------------ empty and refused
def _small():
    return _packed(5, 8, 50, False), _packed(7, 8, 51, False), _packed(7, 16, 52, False), _packed(7, 65, 53, False)


def test_empty_sets_write_nothing():
    """n == 0 or ng == 0: CMVE_OK from both entries, no launch, nothing written."""
    h, lib, check, _ = _api()
    q, g, _, _ = _small()
    for qv, gv in (((0, 0, 256), (0, 7, 256)), ((0, 5, 256), (0, 0, 256)), ((0, 0, 128), (0, 0, 128))):
        qd, gd = q.view(*qv), g.view(*gv)
        for dt in (F32, F64):
            out = Pad(5, 7, ld=10, dtype=TORCH[dt])
            check(lib.cmve_sim_store(h, ctypes.byref(qd), ctypes.byref(gd), BF16X3, 1.0, 0.0, out.ptr, dt, 10),
                  "cmve_sim_store")
            out.assert_untouched("the output of an empty cmve_sim_store")
        ops = Operands(5, 7, True, True, True)
        b, s, t, r, o = ops.ptrs()
        check(lib.cmve_linear(h, ctypes.byref(qd), ctypes.byref(gd), BF16X3, b, s, t, r, ops.ldr, 2, o, ops.ldo),
              "cmve_linear")
        ops.out.assert_untouched("the output of an empty cmve_linear")


def test_refusals():
    """Refused with a non-zero status, every output left all-canary, and each refusal followed by a valid call that
    gives the first valid call's words.  By both entries: NULL handle / rows / out, ldo < ng, d or d_pad
    mismatched, n_pad % 128 != 0, n > n_pad, an unknown mode, BF16X3 without lo, F16 without h16.  By cmve_linear:
    bn_scale without bn_shift and the reverse, resid with ldr < F_out, relu = -1 and 4.  By cmve_sim_store: an
    out_dtype other than F32 / F64."""
    h, lib, check, _ = _api()
    q, g, g16, g65 = _small()
    qd, gd = q.view(0, 5, 256), g.view(0, 7, 256)
    ops = Operands(5, 7, True, True, True)
    out = Pad(5, 7, ld=10)
    B, Sc, Sh, R, O = ops.ptrs()

    def store(qd=qd, gd=gd, mode=BF16X3, out=out.ptr, dt=F32, ldo=10, hh=h):
        return lib.cmve_sim_store(hh, None if qd is None else ctypes.byref(qd), None if gd is None else ctypes.byref(gd),
                                  mode, 1.0, 0.0, out, dt, ldo)

    def linear(qd=qd, gd=gd, mode=BF16X3, b=B, s=Sc, t=Sh, r=R, ldr=ops.ldr, relu=2, o=O, ldo=ops.ldo, hh=h):
        return lib.cmve_linear(hh, None if qd is None else ctypes.byref(qd), None if gd is None else ctypes.byref(gd),
                               mode, b, s, t, r, ldr, relu, o, ldo)

    def valid():
        o1, o2 = Pad(5, 7, ld=10), Operands(5, 7, True, True, True)
        assert store(out=o1.ptr) == 0
        assert linear(o=o2.ptrs()[4]) == 0
        o1.assert_canary("valid store")
        o2.out.assert_canary("valid linear")
        return o1.numpy().view(np.uint32), o2.out.numpy().view(np.uint32)

    first = valid()

    def refused(fn, **kw):
        assert fn(**kw) != 0, f"{fn.__name__} accepted {kw}"
        out.assert_untouched(f"the output of a refused cmve_sim_store {kw}")
        ops.out.assert_untouched(f"the output of a refused cmve_linear {kw}")
        again = valid()
        assert np.array_equal(again[0], first[0]) and np.array_equal(again[1], first[1]), f"after {kw}"

    both = [dict(hh=None), dict(qd=None), dict(gd=None), dict(ldo=6),
            dict(gd=g16.view(0, 7, 256)), dict(gd=g65.view(0, 7, 256)), dict(gd=g.view(0, 7, 256, d_pad=128)),
            dict(gd=g.view(0, 7, 256, d=9)), dict(qd=q.view(0, 5, 256, n_pad=64)), dict(gd=g.view(0, 7, 256, n_pad=192)),
            dict(qd=q.view(0, 5, 256, n=257)), dict(gd=g.view(0, 7, 128, n=129)), dict(mode=3), dict(mode=-1),
            dict(qd=q.view(0, 5, 256, lo=None)), dict(gd=g.view(0, 7, 256, lo=None)),
            dict(mode=F16, qd=q.view(0, 5, 256, h16=None)), dict(mode=F16, gd=g.view(0, 7, 256, h16=None)),
            dict(mode=BF16, qd=q.view(0, 5, 256, hi=None))]
    for kw in both:
        refused(store, **kw)
        refused(linear, **kw)
    refused(store, out=None)
    refused(linear, o=None)
    for kw in (dict(t=None), dict(s=None), dict(ldr=6), dict(relu=-1), dict(relu=4)):
        refused(linear, **kw)
    for dt in (2, 3, 4, -1):
        refused(store, dt=dt)
