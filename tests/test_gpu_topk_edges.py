"""K12a-e (cmve_topk), K13 (cmve_topk_batch) and the EPI_TOPK epilogue through the C ABI: the branches, caps, ties
and the 2E band that the workload-sized cases of test_gpu_topk.py do not enter.

Every call gets its outputs as windows of canary buffers and its workspace as cmve_topk_workspace() floats inside a
larger buffer pre-filled with +2.0 (a score above every cosine: a stray read of the workspace or of a padding column
would win, where a NaN never counts).  The reference is numpy in this file: the cosine of the raw rows in longdouble
(fp64 products over longdouble norms for the two largest shapes), ordered by (score descending, index ascending) with
NaN columns last in index order.  Before each call the REFERENCE CONDITION is asserted on the CPU: any two gallery
rows among the first k + 1 of that order, or tied with the k-th, are bit-identical rows (a tie decided by index; two
NaN columns count as such a tie) or differ in exact cosine by at least 1e-9, and so does the best row under the k-th
and its ties -- far above the fp64 re-score's own error, so ids are demanded bit-exact and scores to 1e-13.

Where a case aims at one side of a cap the rule (bin of the k-th score, tau = round_down(L - 2E), band s~ >= T~_k -
2E) is restated on the s~ the call left in the workspace and the side is asserted: _rule() below.

Pinned behaviour beyond the header: a column whose cosine is NaN is reported with score -inf (the header says so
since this file); a refusal that comes after the argument checks (short workspace, missing plane) has already
cleared *overflow.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from _windows import Pad, _E, _f32_down, _phased, _g64

pytestmark = pytest.mark.gpu

LD = np.longdouble
F32, F64 = 0, 1
NP = {F32: np.float32, F64: np.float64}
BF16, BF16X3, F16 = 0, 1, 2
MODES = {BF16: "bf16", BF16X3: "bf16x3", F16: "f16"}
INF, NAN = np.inf, np.nan
TOPK_CAP, CAND_CAP, HBINS, CHUNK_MIN = 4096, 8192, 4096, 16384
BT_LCAP, BT_BAND, BT_TARGET = 512, 256, 128
TAIL = 256  # floats after the workspace that must stay +2.0
E_INVALID = -1


def _api():
    from cmve import engine
    from cmve._lib import lib, check, Rows
    return engine.handle(), lib, check, Rows


def _msg():
    from cmve._lib import lib
    return lib.cmve_last_error().decode(errors="replace")


# ------------------------------------------------------------------ packed sets
class S:
    """Rows x packed by engine.RowSet; raw_ld: the raw rows move to a buffer of that leading dimension whose gap
    columns hold 1e30 and the set is packed again by cmve_pack_rows on the changed descriptor."""

    def __init__(self, x, eps=0.0, lo=True, h16=True, raw_ld=None):
        from cmve import engine
        h, lib, check, _ = _api()
        self.x, self.eps, self.n, self.d = x, eps, x.shape[0], x.shape[1]
        self.rs = engine.RowSet(x, eps=eps, with_lo=lo, with_f16=h16)
        self.desc = self.rs.desc
        self.n_pad, self.d_pad = self.rs.n_pad, self.rs.d_pad
        if raw_ld is not None:
            self.buf = torch.full((self.n * raw_ld + 8,), 1e30, dtype=self.rs.raw.dtype, device="cuda")
            torch.as_strided(self.buf, (self.n, self.d), (raw_ld, 1)).copy_(self.rs.raw)
            self.desc.raw, self.desc.raw_ld = self.buf.data_ptr(), raw_ld
            check(lib.cmve_pack_rows(h, ctypes.byref(self.desc)), "cmve_pack_rows")

    def err(self, mode):
        t = (self.rs.err_hi, self.rs.err_hilo, self.rs.err_h16)[mode]
        return t[:self.n].cpu().numpy().astype(np.float64)

    def err_max(self, mode):
        return float(self.rs.err_max.cpu().numpy()[mode])

    def variant(self, **change):
        _, _, _, Rows = _api()
        r = Rows()
        ctypes.memmove(ctypes.byref(r), ctypes.byref(self.desc), ctypes.sizeof(Rows))
        for k, v in change.items():
            setattr(r, k, v)
        return r


# ------------------------------------------------------------------ the reference
def _norms(x):
    return np.sqrt((x.astype(LD) ** 2).sum(axis=1))


def _cos(xq, xg, eps=0.0):
    """fp64 [n_q, n_g]: longdouble throughout, or (above 2e7 products) fp64 dot products over longdouble norms."""
    nq, ng = _norms(xq), _norms(xg)
    if eps > 0:
        nq, ng = np.maximum(nq, LD(eps)), np.maximum(ng, LD(eps))
    with np.errstate(all="ignore"):
        if xq.shape[0] * xg.shape[0] * xq.shape[1] > 2e7:
            return (xq.astype(np.float64) @ xg.astype(np.float64).T) / (nq[:, None] * ng[None, :]).astype(np.float64)
        return ((xq.astype(LD) @ xg.astype(LD).T) / (nq[:, None] * ng[None, :])).astype(np.float64)


def _ref(cos, xg, k, what=""):
    """(idx int64 [n_q, k], score fp64 [n_q, k]) of the reference order: -1 / NaN past the gallery, -inf at a NaN
    column.  Asserts the reference condition (module docstring) for every query."""
    nq, ng = cos.shape
    kk = min(k, ng)
    idx, sc = np.full((nq, k), -1, np.int64), np.full((nq, k), NAN)
    if ng == 0:
        return idx, sc
    key = np.where(np.isnan(cos), -INF, cos)
    for i in range(nq):
        ki = key[i]
        kth = np.partition(ki, ng - kk)[ng - kk]
        c = np.flatnonzero(ki >= kth)  # the first k and everything tied with the k-th
        c = c[np.lexsort((c, -ki[c]))]
        s = ki[c]
        with np.errstate(invalid="ignore"):
            close = np.flatnonzero(~(s[:-1] - s[1:] >= 1e-9))
        if close.size:
            a, b = c[close], c[close + 1]
            tie = (xg[a] == xg[b]).all(axis=1) | (np.isnan(cos[i, a]) & np.isnan(cos[i, b]))
            assert tie.all(), f"{what} query {i}: columns {a[~tie][:4]} / {b[~tie][:4]} are neither bit-identical " \
                              f"nor 1e-9 apart"
        if c.size < ng:  # the best row under the k-th and its ties: the (k + 1)-th, or the first past a tie group
            nxt = ki[ki < kth].max()
            assert kth - nxt >= 1e-9, f"{what} query {i}: the next row is {kth - nxt:.2e} under the k-th"
        idx[i, :kk], sc[i, :kk] = c[:kk], s[:kk]
    return idx, sc


def _assert_rows(idx, sc, ridx, rsc, what):
    bad = np.flatnonzero((idx != ridx).any(axis=1))
    assert bad.size == 0, f"{what}: ids differ in {bad.size} rows, first {bad[0]}: {idx[bad[0]][:8]} against " \
                          f"{ridx[bad[0]][:8]}"
    fin = np.isfinite(rsc)
    assert np.array_equal(np.isnan(sc), np.isnan(rsc)), f"{what}: NaN scores (empty slots) differ"
    assert (sc[rsc == -INF] == -INF).all(), f"{what}: a NaN column's score is -inf"
    if fin.any():
        err = np.abs(sc[fin] - rsc[fin]).max()
        assert err <= 1e-13, f"{what}: scores off by {err:.3e}"


# ------------------------------------------------------------------ cmve_topk with windows, and its rule restated
def _al64(x):
    return (x + 63) & ~63


def _topk_layout(nq, n_pad):
    w = {"scores": 0}
    w["hist"] = _al64(nq * n_pad)
    w["tau"] = w["hist"] + _al64(nq * HBINS)
    w["keepall"] = w["tau"] + _al64(nq)
    w["cnt"] = w["keepall"] + _al64(nq)
    w["cand"] = w["cnt"] + _al64(nq)
    w["total"] = w["cand"] + _al64(nq * CAND_CAP)
    return w


def _topk_ws_floats(q, g, k):
    _, lib, check, _ = _api()
    nf = ctypes.c_int64()
    check(lib.cmve_topk_workspace(ctypes.byref(q.desc), ctypes.byref(g.desc), k, ctypes.byref(nf)),
          "cmve_topk_workspace")
    assert nf.value == _topk_layout(max(q.n, 1), g.n_pad)["total"]
    return nf.value


def _topk(q, g, mode, k, want_ws=True):
    """One cmve_topk call: (idx int64 [n_q, k], score [n_q, k], overflow, the workspace as numpy or None)."""
    h, lib, check, _ = _api()
    nf = _topk_ws_floats(q, g, k)
    ws = torch.full((nf + TAIL,), 2.0, dtype=torch.float32, device="cuda")
    idx, sc, ovf = Pad(q.n, k, dtype=torch.int32), Pad(q.n, k, dtype=torch.float64), Pad(1, 1, dtype=torch.int32)
    check(lib.cmve_topk(h, ctypes.byref(q.desc), ctypes.byref(g.desc), mode, k, ws.data_ptr(), nf, idx.ptr, sc.ptr,
                        ovf.ptr), "cmve_topk")
    for p, name in ((idx, "out_idx"), (sc, "out_score"), (ovf, "overflow")):
        p.assert_canary(name)
    assert bool((ws[nf:] == 2.0).all()), "cmve_topk wrote past its workspace"
    return idx.numpy().astype(np.int64), sc.numpy(), int(ovf.numpy()[0, 0]), ws[:nf].cpu().numpy() if want_ws else None


def _stilde(ws, q, g):
    return ws[:q.n * g.n_pad].reshape(q.n, g.n_pad)


def _bins(v):
    """score_bin: (s + 1) * 2048 in fp32, clamped to [0, 4095], truncated."""
    v = np.asarray(v, np.float32)
    return np.clip((v + np.float32(1)) * np.float32(2048), np.float32(0), np.float32(HBINS - 1)).astype(np.int64)


def _tau_of(v, k, E):
    """K12c on the finite scores v: (tau, keepall, bin of the k-th)."""
    if v.size < k:
        return -INF, True, -1
    h = np.bincount(_bins(v), minlength=HBINS)
    b = HBINS - 1 - int(np.searchsorted(np.cumsum(h[::-1]), k))
    L = -INF if b == 0 else b / 2048.0 - 1.0 - 2.0 ** -20
    return float(_f32_down(L - 2.0 * E)), False, b


def _rule(ws, q, g, mode, k):
    """K12b-e restated per query on the s~ of the workspace: tau, keepall, the candidate count (list source up to
    CAND_CAP, the dense row above), T~_k and the band count; tau, keepall and the count are also compared with the
    words the kernels left in the workspace."""
    st = _stilde(ws, q, g)[:, :g.n]
    E = _E(q.err(mode), g.err_max(mode), g.d_pad, mode)
    w = _topk_layout(q.n, g.n_pad)
    out = []
    for i in range(q.n):
        v = st[i][~np.isnan(st[i])]
        tau, keepall, b = _tau_of(v, k, E[i])
        if keepall:
            r = dict(tau=tau, keepall=True, bin=b, cand=g.n, band=g.n, Tk=None)
        else:
            Tk = np.sort(v)[-k]
            thr = float(_f32_down(float(Tk) - 2.0 * E[i]))
            r = dict(tau=tau, keepall=False, bin=b, cand=int((v >= np.float32(tau)).sum()), Tk=float(Tk),
                     band=int((v >= np.float32(thr)).sum()))
        r["dense"] = r["cand"] > CAND_CAP
        assert ws[w["tau"] + i] == np.float32(tau), f"query {i}: tau {ws[w['tau'] + i]!r} against {tau!r}"
        assert (ws[w["keepall"]:].view(np.int32)[i] != 0) == keepall
        assert ws[w["cnt"]:].view(np.uint32)[i] == r["cand"], f"query {i}: candidate count"
        out.append(r)
    return out


def _check_topk(q, g, mode, k, cos=None, what=""):
    """Reference (with its condition) -> call -> ids and scores where no band overflowed.  Returns (overflow, rule)."""
    cos = _cos(q.x, g.x, q.eps) if cos is None else cos
    ridx, rsc = _ref(cos, g.x, k, what)
    idx, sc, ovf, ws = _topk(q, g, mode, k)
    rule = _rule(ws, q, g, mode, k) if g.n else []
    assert (ovf != 0) == any(r["band"] > TOPK_CAP for r in rule), f"{what}: overflow {ovf} against the restated bands"
    if not ovf:
        _assert_rows(idx, sc, ridx, rsc, what)
    return ovf, rule


def _planted(cs, d=64, dt=np.float64, sign=1.0):
    """Rows (c, sign sqrt(1 - c^2), 0, ...): the cosine against e0 is c."""
    cs = np.asarray(cs, np.float64)
    g = np.zeros((cs.size, d), dt)
    g[:, 0], g[:, 1] = cs, sign * np.sqrt(1.0 - cs * cs)
    return g


def _e0(n=1, d=64, dt=np.float64, tilt=None):
    q = np.zeros((n, d), dt)
    q[:, 0] = 1.0
    if tilt is not None:
        q[:, 1] = tilt
    return q


# ------------------------------------------------------------------ A. K12a
A_FAMS = ("gauss", "absgauss", "const", "alt", "subn")
A_NQ, A_NG = (1, 15, 16, 17, 31, 32), (1, 15, 16, 17, 65, 257, 1000)


def _family(name, rng, d):
    g = rng.standard_normal(d)
    if name == "gauss":
        return g
    if name == "absgauss":
        return np.abs(g)
    if name == "const":
        return np.full(d, 0.37)
    if name == "alt":
        return (1 - 2 * (np.arange(d) % 2)) * (1 + 0.05 * g)
    return g * 2.0 ** -rng.integers(0, 21, d)  # subn: fp16 subnormals after normalising


@functools.lru_cache(maxsize=None)
def _a_data(d):
    """33 query rows and 1000 gallery rows of dimension d, the five families cycling over the rows (d = 1: +-0.37
    only, where every cosine is +-1 and the rows of one sign are bit-identical), and their cosines.  fp32 rows for
    even d, fp64 for odd.  The sets of a case are prefixes of these."""
    rng = np.random.default_rng(7000 + d)
    dt = np.float64 if d % 2 else np.float32
    if d == 1:
        xq = (0.37 * (1 - 2 * (np.arange(33) % 2)))[:, None].astype(dt)
        xg = (0.37 * (1 - 2 * ((np.arange(1000) % 3) == 1)))[:, None].astype(dt)
    else:
        xq = np.stack([_family(A_FAMS[(r + 2) % 5], rng, d) for r in range(33)]).astype(dt)
        xg = np.stack([_family(A_FAMS[r % 5], rng, d) for r in range(1000)]).astype(dt)
    return xq, xg, _cos(xq, xg)


def _gemv_fits(nq, d_pad, mode):
    return nq <= 32 and (1 if nq <= 16 else 2) * (2 if mode == BF16X3 else 1) * 16 * d_pad * 2 <= 160 * 1024


def _check_scores(q, g, mode, k, cos, what):
    """|s~ - cos| <= E(err_q[i], err_g[j]) on every real pair from the workspace, then ids / scores.  Returns the
    largest ratio."""
    ridx, rsc = _ref(cos, g.x, k, what)
    idx, sc, ovf, ws = _topk(q, g, mode, k)
    st = _stilde(ws, q, g)
    E = _E(q.err(mode)[:, None], g.err(mode)[None, :], g.d_pad, mode)
    ratio = np.abs(st[:, :g.n].astype(np.float64) - cos) / E
    assert not np.isnan(st[:, :g.n]).any() and ratio.max() <= 1.0, f"{what}: |s~ - cos| / E up to {ratio.max():.4f}"
    assert ovf == 0
    _assert_rows(idx, sc, ridx, rsc, what)
    return ratio.max()


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("d", [1, 31, 64, 65, 257, 512])
def test_gemv_scores_within_bound(d, mode):
    """K12a at n_q in {1, 15, 16, 17, 31, 32} (one and two query tiles, full and ragged) x n_g in {1, 15, 16, 17, 65,
    257, 1000} (under, at and over one 16-row group; several blocks), d of 2, 4, 10 and 16 k-steps (under one load
    group of 8, one group and a tail of 2, two groups).  Every s~ of the workspace is within E of the longdouble
    cosine; ids and scores at k = min(10, n_g).  Prints the largest ratio (DESIGN.md s7 records it)."""
    xq, xg, cos = _a_data(d)
    qs = {n: S(xq[:n]) for n in A_NQ}
    worst = 0.0
    for ng in A_NG:
        g = S(xg[:ng])
        for nq in A_NQ:
            assert _gemv_fits(nq, g.d_pad, mode)
            worst = max(worst, _check_scores(qs[nq], g, mode, min(10, ng), cos[:nq, :ng],
                                             f"{MODES[mode]} d {d} n_q {nq} n_g {ng}"))
    print(f"RATIO K12a d={d} mode={MODES[mode]} max={worst:.4f}")


@pytest.mark.parametrize("mode,nq,d,gemv", [(BF16, 33, 64, False), (F16, 33, 257, False), (BF16X3, 16, 1344, True),
                                            (BF16X3, 17, 1344, False), (F16, 32, 2560, True), (F16, 32, 2624, False)])
def test_gemv_boundary(mode, nq, d, gemv):
    """The hand-over to the GEMM: 33 queries; two query tiles whose LDS image passes 160 KiB (BF16X3 with two planes
    at d_pad = 1344: 168 KiB; F16 at d_pad = 2624: 164 KiB), and the last shapes that still fit (one tile at 1344;
    exactly 160 KiB at 2560).  The same bound and reference on both sides."""
    rng = np.random.default_rng(100 * nq + d)
    xq = rng.standard_normal((nq, d)).astype(np.float32)
    xg = rng.standard_normal((257, d)).astype(np.float32)
    q, g = S(xq), S(xg)
    assert g.d_pad == d + (-d % 64) and _gemv_fits(nq, g.d_pad, mode) == gemv
    r = _check_scores(q, g, mode, 10, _cos(xq, xg), f"{MODES[mode]} n_q {nq} d {d}")
    print(f"RATIO boundary n_q={nq} d={d} mode={MODES[mode]} gemv={gemv} max={r:.4f}")


# ------------------------------------------------------------------ B. K12b-e through cmve_topk
@pytest.mark.parametrize("mode", [F16, BF16X3])
def test_hist_bin_edges_top_bin_and_bin_zero(mode):
    """Scores planted at the lower edge 0.5 of bin 3072 and a step or two of the fp32 sum either side (q = (1, 2^-23,
    0, ..) against (0.5, +-sqrt(3)/2) and (0.5, 0, sqrt(3)/2)), with the k-th score on each of the three; duplicates
    of the query (s~ = 1: the clamp of the top bin); antipodal rows (s~ = -1: bin 0, L = tau = -inf)."""
    q = S(_e0(tilt=2.0 ** -23))
    s3 = np.sqrt(0.75)
    edge = np.zeros((3, 64))
    edge[:, 0] = 0.5
    edge[0, 1], edge[1, 2], edge[2, 1] = s3, s3, -s3
    rng = np.random.default_rng(31)
    xg = np.concatenate([_planted(rng.uniform(-0.5, 0.3, 100)), _planted([0.8, 0.7, 0.6]), edge,
                         _planted(rng.uniform(-0.5, 0.3, 100))])
    g = S(xg)
    for k in (4, 5, 6):  # the k-th best is column 103 (above the edge), 104 (on it), 105 (below)
        ovf, rule = _check_topk(q, g, mode, k, what=f"edge k {k}")
        assert ovf == 0 and not rule[0]["dense"]
    st = _stilde(_topk(q, g, mode, 5)[3], q, g)[0]
    above, at, below = st[103], st[104], st[105]
    assert at == np.float32(0.5) and 0 < above - at <= 2.0 ** -22 and 0 < at - below <= 2.0 ** -22, (above, at, below)
    assert list(_bins([above, at, below])) == [3072, 3072, 3071]
    assert _rule(_topk(q, g, mode, 5)[3], q, g, mode, 5)[0]["bin"] == 3072
    assert _rule(_topk(q, g, mode, 6)[3], q, g, mode, 6)[0]["bin"] == 3071
    # the top bin: five copies of the query and two rows just under it; k = 3 ends among the copies
    xg = np.concatenate([_planted(rng.uniform(-0.5, 0.3, 50)), np.repeat(q.x, 5, axis=0), _planted([0.9999, 0.9998]),
                         _planted(rng.uniform(-0.5, 0.3, 50))])
    g = S(xg)
    ovf, rule = _check_topk(q, g, mode, 3, what="top bin")
    assert ovf == 0 and rule[0]["bin"] == HBINS - 1 and rule[0]["Tk"] >= 1.0
    # bin 0: 37 antipodal copies and three better rows, k = 5
    xg = np.concatenate([np.repeat(-q.x, 20, axis=0), _planted([0.3, -0.2, 0.1]), np.repeat(-q.x, 17, axis=0)])
    g = S(xg)
    ovf, rule = _check_topk(q, g, mode, 5, what="bin 0")
    assert ovf == 0 and rule[0]["bin"] == 0 and rule[0]["tau"] == -INF and rule[0]["cand"] == 40


def test_shape_corners():
    """k in {1, 2, n_g, 2048}; n_g = 1; k > n_g (idx -1 / score NaN past the gallery)."""
    rng = np.random.default_rng(41)
    xq = rng.standard_normal((2, 64)).astype(np.float32)
    xg = rng.standard_normal((3000, 64)).astype(np.float32)
    q, cos = S(xq), _cos(xq, xg)
    g = S(xg)
    for k in (1, 2, 2048):
        assert _check_topk(q, g, F16, k, cos, f"k {k}")[0] == 0
    for ng, k in ((5, 5), (5, 8), (1, 1), (1, 3), (17, 2048)):
        g = S(xg[:ng])
        for mode in MODES:
            assert _check_topk(q, g, mode, k, cos[:, :ng], f"n_g {ng} k {k}")[0] == 0
        idx, sc, _, _ = _topk(q, g, F16, k, want_ws=False)
        assert (idx[:, ng:] == -1).all() and np.isnan(sc[:, ng:]).all() and (idx[:, :min(k, ng)] >= 0).all()


@pytest.mark.parametrize("ng", [257, 1000])
def test_all_scores_negative(ng):
    """Every cosine in [-0.9, -0.1]: the +2.0 of the padding columns [n_g, n_pad) never enters a histogram, a
    candidate list or a band (GEMV for 3 queries, the GEMM's store for 40)."""
    rng = np.random.default_rng(ng)
    xg = _planted(rng.uniform(-0.9, -0.1, ng), sign=np.where(rng.random(ng) < 0.5, -1.0, 1.0))
    for nq in (3, 40):
        q = S(_e0(nq, tilt=np.linspace(-0.02, 0.02, nq)))
        cos = _cos(q.x, xg)
        assert cos.max() < 0
        for mode in MODES:
            ovf, rule = _check_topk(q, S(xg), mode, 10, cos, f"n_g {ng} n_q {nq} {MODES[mode]}")
            assert ovf == 0 and all(r["Tk"] < 0 for r in rule)


def _chunks(nq, ng):
    want, mx = max(1, 1024 // nq), max(1, -(-ng // CHUNK_MIN))
    n = min(want, mx)
    chunk = (-(-ng // n) + 255) & ~255
    return chunk, -(-ng // chunk)


@pytest.mark.parametrize("nq", [1, 3])
@pytest.mark.parametrize("ng", [16385, 40000])
def test_multi_chunk_histogram_and_collect(nq, ng):
    """Two and three chunks of K12b / K12d (atomically merged histograms, one candidate counter per query): the k
    best lie on the last column of every chunk, the first of the next, and column n_g - 1."""
    chunk, nch = _chunks(nq, ng)
    assert nch == (2 if ng == 16385 else 3) and chunk % 256 == 0
    rng = np.random.default_rng(ng + nq)
    cs = rng.uniform(-0.6, 0.6, ng)
    spots = sorted({c * chunk - 1 for c in range(1, nch)} | {c * chunk for c in range(1, nch)} | {ng - 1})
    cs[spots] = 0.95 - 0.01 * np.arange(len(spots))
    xg = _planted(cs, dt=np.float32)
    q = S(_e0(nq, dt=np.float32, tilt=np.linspace(0.0, 0.02, nq)))
    g = S(xg)
    cos = _cos(q.x, xg)
    for k in (len(spots), len(spots) + 3):
        for mode in (F16, BF16X3):
            ovf, rule = _check_topk(q, g, mode, k, cos, f"n_g {ng} n_q {nq} k {k} {MODES[mode]}")
            assert ovf == 0 and not any(r["dense"] for r in rule)
    assert sorted(_ref(cos, xg, len(spots))[0][0]) == spots


def _dense_gallery():
    """12,000 rows: nine clear winners, the 10th at 0.50046 (near the top of bin 3072, whose lower edge is 0.5), and
    11,990 cosines evenly spaced over the 6e-4 below it (5e-8 apart)."""
    cs = np.concatenate([np.linspace(0.7, 0.6, 9), [0.50046], 0.50046 - 6e-4 * np.arange(1, 11991) / 11990.0])
    return _planted(cs[np.random.default_rng(5).permutation(cs.size)])


def test_dense_source():
    """K12e's dense-row source: BF16X3 finds more than CAND_CAP = 8192 candidates (tau sits 2E under the bin's lower
    edge) and a band under TOPK_CAP: overflow 0, ids exact.  The same gallery in F16, whose 2E is wider than the
    cluster: every row is in the band, which sets overflow."""
    xg = _dense_gallery()
    q, g = S(_e0()), S(xg)
    cos = _cos(q.x, xg)
    ovf, rule = _check_topk(q, g, BF16X3, 10, cos, "dense bf16x3")
    print(f"DENSE bf16x3: candidates {rule[0]['cand']} band {rule[0]['band']}")
    assert rule[0]["dense"] and rule[0]["band"] <= TOPK_CAP and ovf == 0 and rule[0]["bin"] == 3072
    ovf, rule = _check_topk(q, g, F16, 10, cos, "dense f16")
    print(f"DENSE f16: candidates {rule[0]['cand']} band {rule[0]['band']}")
    assert rule[0]["dense"] and rule[0]["band"] > TOPK_CAP and ovf != 0


@pytest.mark.parametrize("ndup,ng", [(4091, 5000), (4092, 5000), (5000, 6000), (8187, 9000), (9000, 10000)])
def test_band_overflow_sets_and_clears(ndup, ng):
    """Bit-identical rows at the k-th score under five clear winners, every other row far below tau.  4,091: the band
    holds exactly TOPK_CAP = 4096 columns, no overflow, the duplicates in index order; 4,092: one more, overflow.
    5,000 of 6,000 go through the candidate list; 8,187 make exactly CAND_CAP = 8192 candidates, the last size of the
    list; 9,000 of 10,000 take the dense row.  Every mode agrees; a benign call into the same window clears
    *overflow; engine.topk returns the duplicates in index order (through its dense fp64 fallback past the cap)."""
    from cmve import engine
    h, lib, check, _ = _api()
    rng = np.random.default_rng(ndup)
    cs = rng.uniform(-0.5, 0.3, ng)
    dup = np.sort(rng.choice(ng, ndup, replace=False))
    cs[dup] = 0.625
    top = np.setdiff1d(np.arange(ng), dup)[:5]
    cs[top] = [0.9, 0.85, 0.8, 0.75, 0.7]
    xg = _planted(cs)
    q, g = S(_e0()), S(xg)
    cos = _cos(q.x, xg)
    ridx, rsc = _ref(cos, xg, 10, "band overflow")
    assert list(ridx[0]) == list(top) + list(dup[:5])
    for mode in MODES:
        ovf, rule = _check_topk(q, g, mode, 10, cos, f"dup {ndup} {MODES[mode]}")
        assert rule[0]["band"] == rule[0]["cand"] == ndup + 5 and (ovf != 0) == (ndup + 5 > TOPK_CAP)
        assert rule[0]["dense"] == (ndup + 5 > CAND_CAP)
    # the same overflow word, set by hand, is cleared by a call that does not overflow
    nf = _topk_ws_floats(q, g, 10)
    ws = torch.full((nf,), 2.0, dtype=torch.float32, device="cuda")
    idx, sc, ovf = Pad(1, 10, dtype=torch.int32), Pad(1, 10, dtype=torch.float64), Pad(1, 1, dtype=torch.int32)
    args = lambda gg: (h, ctypes.byref(q.desc), ctypes.byref(gg.desc), F16, 10, ws.data_ptr(), nf, idx.ptr, sc.ptr,
                       ovf.ptr)
    ovf.t.fill_(1)
    check(lib.cmve_topk(*args(g)), "cmve_topk")
    assert (ovf.numpy()[0, 0] != 0) == (ndup + 5 > TOPK_CAP)
    ovf.t.fill_(1)
    benign = S(xg[:50])
    ws2 = _topk_ws_floats(q, benign, 10)
    assert ws2 <= nf
    check(lib.cmve_topk(*args(benign)), "cmve_topk")
    assert ovf.numpy()[0, 0] == 0
    i2, s2 = engine.topk(q.rs, g.rs, 10)
    _assert_rows(i2, s2, ridx, rsc, f"engine.topk dup {ndup}")


@pytest.mark.parametrize("ng", [3000, 9000])
def test_fewer_than_k_finite_scores(ng):
    """Zero gallery rows at eps = 0 (NaN cosines) and five finite rows, k = 12: K12c keeps every column.  3,000
    columns go through the list and all fit the band: the finite five, then NaN columns by index with score -inf.
    9,000 take the dense row and overflow.  A zero QUERY row has only NaN columns: ids 0 .. k-1, scores -inf."""
    rng = np.random.default_rng(ng)
    xg = np.zeros((ng, 64))
    live = np.sort(rng.choice(ng, 5, replace=False))
    xg[live] = _planted([0.3, -0.2, 0.5, 0.1, -0.7])
    xq = np.concatenate([_e0(), np.zeros((1, 64)), _e0(tilt=0.1)])
    q, g = S(xq), S(xg)
    cos = _cos(xq, xg)
    assert np.isnan(cos[1]).all() and np.isfinite(cos[0]).sum() == 5
    for mode in MODES:
        ovf, rule = _check_topk(q, g, mode, 12, cos, f"n_g {ng} {MODES[mode]}")
        assert all(r["keepall"] and r["cand"] == ng for r in rule)
        assert (ovf != 0) == (ng > TOPK_CAP) and rule[0]["dense"] == (ng > CAND_CAP)
    if ng <= TOPK_CAP:
        idx, sc, _, _ = _topk(q, g, F16, 12, want_ws=False)
        nan = np.setdiff1d(np.arange(ng), live)[:12]
        assert list(idx[1]) == list(nan) and (sc[1] == -INF).all()
        assert sorted(idx[0][:5]) == list(live) and list(idx[0][5:]) == list(nan[:7]) and (sc[0][5:] == -INF).all()
    # a zero query row among live ones against a live gallery
    xg2 = _planted(rng.uniform(-0.5, 0.5, 300))
    assert _check_topk(q, S(xg2), F16, 12, what="zero query row")[0] == 0


@pytest.mark.parametrize("qdt,gdt", [(F32, F32), (F32, F64), (F64, F32), (F64, F64)])
def test_raw_dtype_pairs_and_strided_rows(qdt, gdt):
    """The four instances of the fp64 re-score, on contiguous raw rows and on rows with raw_ld = d + 3 (queries) and
    d + 1 (gallery) whose gap columns hold 1e30: a read of them would move the re-score.  d = 65: no 16-byte rows."""
    rng = np.random.default_rng(10 * qdt + gdt)
    xq = rng.standard_normal((5, 65)).astype(NP[qdt])
    xg = rng.standard_normal((300, 65)).astype(NP[gdt])
    cos = _cos(xq, xg)
    for ldq, ldg in ((None, None), (68, 66), (66, 68)):
        q, g = S(xq, raw_ld=ldq), S(xg, raw_ld=ldg)
        for mode in MODES:
            assert _check_topk(q, g, mode, 10, cos, f"ld {ldq} {ldg} {MODES[mode]}")[0] == 0


class Empty:
    """A packed set seen with n = 0 (planes, raw rows and n_pad of the real set behind it)."""

    def __init__(self, s):
        self.s, self.desc, self.n, self.n_pad, self.d_pad, self.x, self.eps = s, s.variant(n=0), 0, s.n_pad, s.d_pad, \
            s.x[:0], s.eps


def test_empty_sets():
    """q->n == 0: nothing but *overflow is written.  g->n == 0: idx -1 (scores and workspace are left alone).  Both
    entries."""
    h, lib, check, _ = _api()
    xg = np.random.default_rng(1).standard_normal((20, 64))
    g, q = S(xg), S(_e0(3))
    q0, g0 = Empty(q), Empty(g)
    idx, sc, ovf = Pad(1, 4, dtype=torch.int32), Pad(1, 4, dtype=torch.float64), Pad(1, 1, dtype=torch.int32)
    ws = torch.full((_topk_ws_floats(q0, g, 4),), 2.0, dtype=torch.float32, device="cuda")
    check(lib.cmve_topk(h, ctypes.byref(q0.desc), ctypes.byref(g.desc), F16, 4, ws.data_ptr(), ws.numel(), idx.ptr,
                        sc.ptr, ovf.ptr), "cmve_topk")
    idx.assert_untouched("out_idx of an empty query set")
    sc.assert_untouched("out_score of an empty query set")
    assert ovf.numpy()[0, 0] == 0 and bool((ws == 2.0).all())
    idx, sc, ovf, ws = _topk(q, g0, F16, 4)
    assert (idx == -1).all() and np.isnan(sc).all() and ovf == 0 and (ws == 2.0).all()
    bidx, bsc, un, ws = _batch(q, g0, F16, 4)
    assert un == 0 and (bidx == -1).all() and bool((ws == 2.0).all())
    bidx, bsc, un, ws = _batch(q0, g, F16, 4)
    assert un == 0 and bidx.shape == (0, 4) and bool((ws == 2.0).all())


def _refusal_windows(nq, k):
    return Pad(nq, k, dtype=torch.int32), Pad(nq, k, dtype=torch.float64), Pad(1, 1, dtype=torch.int32)


def test_topk_refusals():
    """Each refusal returns CMVE_E_INVALID with its message and leaves out_idx / out_score unwritten; *overflow is
    unwritten by the argument checks and already cleared by the later ones (short workspace, missing plane)."""
    h, lib, check, _ = _api()
    rng = np.random.default_rng(2)
    xq, xg = rng.standard_normal((3, 64)), rng.standard_normal((50, 64))
    q, g = S(xq), S(xg)
    nf = _topk_ws_floats(q, g, 5)
    ws = torch.full((nf,), 2.0, dtype=torch.float32, device="cuda")
    idx, sc, ovf = _refusal_windows(3, 5)
    g32, g100 = S(rng.standard_normal((50, 32))), S(rng.standard_normal((50, 100)))
    q_no16, q_nolo = S(xq, h16=False), S(xq, lo=False)
    qd, gd = q.desc, g.desc

    def call(qq=qd, gg=gd, mode=F16, k=5, w=ws.data_ptr(), n=nf, i=idx.ptr, s=sc.ptr, o=ovf.ptr, hh=h):
        return lib.cmve_topk(hh, None if qq is None else ctypes.byref(qq), None if gg is None else ctypes.byref(gg),
                             mode, k, w, n, i, s, o)

    early = [(dict(k=0), "k must be >= 1"), (dict(k=2049), "k must be <= 2048"), (dict(k=-3), "k must be >= 1"),
             (dict(hh=None), "NULL"), (dict(qq=None), "NULL"), (dict(gg=None), "NULL"), (dict(w=None), "NULL"),
             (dict(i=None), "NULL"), (dict(s=None), "NULL"), (dict(o=None), "NULL"),
             (dict(qq=q.variant(flags=1)), "CMVE_PACK_RAW"), (dict(gg=g.variant(flags=1)), "CMVE_PACK_RAW"),
             (dict(gg=g32.desc), "dimension mismatch"), (dict(gg=g100.desc), "dimension mismatch"),
             (dict(qq=q.variant(raw=None)), "raw rows"), (dict(gg=g.variant(inv_norm=None)), "raw rows"),
             (dict(mode=3), "unknown mode"), (dict(mode=-1), "unknown mode")]
    for change, text in early:
        assert call(**change) == E_INVALID and text in _msg(), (change, _msg())
        for p in (idx, sc, ovf):
            p.assert_untouched(f"an output of a cmve_topk refused for {text}")
    late = [(dict(n=nf - 1), "workspace has"), (dict(qq=q_no16.desc), "error plane"),
            (dict(qq=q.variant(h16=None)), "F16 needs h16"), (dict(gg=g.variant(h16=None)), "F16 needs h16"),
            (dict(qq=q_nolo.desc, mode=BF16X3), "BF16X3 needs lo"),
            (dict(gg=g.variant(lo=None), mode=BF16X3), "BF16X3 needs lo")]
    for change, text in late:
        ovf.flat.fill_(-77)
        assert call(**change) == E_INVALID and text in _msg(), (change, _msg())
        idx.assert_untouched(f"out_idx of a cmve_topk refused for {text}")
        sc.assert_untouched(f"out_score of a cmve_topk refused for {text}")
        ovf.assert_canary("overflow")
        assert ovf.numpy()[0, 0] == 0
    assert bool((ws == 2.0).all()), "a refused cmve_topk wrote its workspace"
    n_out = ctypes.c_int64(-5)
    for k in (0, 2049):
        assert lib.cmve_topk_workspace(ctypes.byref(qd), ctypes.byref(gd), k, ctypes.byref(n_out)) == E_INVALID
    assert lib.cmve_topk_workspace(ctypes.byref(qd), ctypes.byref(gd), 5, None) == E_INVALID and n_out.value == -5
    assert call() == 0  # and the call they were derived from runs


# ------------------------------------------------------------------ C. K13
def _batch_layout(nq, nq_pad, ng, ng_pad, k):
    w = {}
    want = -(-k * ng // BT_TARGET)
    w["ns"] = min(ng, max(want, 2 * k))
    w["ns_pad"] = min(ng_pad, (w["ns"] + 255) & ~255)
    w["sc"] = 0
    w["hist"] = _al64(nq * w["ns_pad"])
    w["tau"] = w["hist"] + _al64(nq * HBINS)
    w["keepall"] = w["tau"] + _al64(nq)
    w["hi"] = w["keepall"] + _al64(nq)
    w["lo"] = w["hi"] + _al64(nq_pad)
    w["cand"] = w["lo"] + _al64(nq_pad)
    w["nb"] = (nq_pad + 255) // 256
    w["cap_b"] = 256 * BT_LCAP
    w["total"] = w["cand"] + 2 * (w["nb"] + w["nb"] * w["cap_b"])
    return w


def _batch(q, g, mode, k):
    """One cmve_topk_batch call: (idx int64 [n_q, k], score, unresolved, the workspace as a device tensor)."""
    h, lib, check, _ = _api()
    ns, nf = ctypes.c_int64(), ctypes.c_int64()
    check(lib.cmve_topk_batch_workspace(ctypes.byref(q.desc), ctypes.byref(g.desc), k, ctypes.byref(ns),
                                        ctypes.byref(nf)), "cmve_topk_batch_workspace")
    w = _batch_layout(max(q.n, 1), max(q.n_pad, 256), g.n, g.n_pad, k)
    assert (ns.value, nf.value) == (w["ns"], w["total"])
    ws = torch.full((nf.value + TAIL,), 2.0, dtype=torch.float32, device="cuda")
    idx, sc, un = Pad(q.n, k, dtype=torch.int32), Pad(q.n, k, dtype=torch.float64), Pad(1, 1, dtype=torch.int32)
    check(lib.cmve_topk_batch(h, ctypes.byref(q.desc), ctypes.byref(g.desc), mode, k, ws.data_ptr(), nf.value,
                              idx.ptr, sc.ptr, un.ptr), "cmve_topk_batch")
    for p, name in ((idx, "out_idx"), (sc, "out_score"), (un, "unresolved")):
        p.assert_canary(name)
    assert bool((ws[nf.value:] == 2.0).all()), "cmve_topk_batch wrote past its workspace"
    return idx.numpy().astype(np.int64), sc.numpy(), int(un.numpy()[0, 0]), ws[:nf.value]


def _batch_state(ws, q, g, mode, k):
    """K13 restated from the workspace of a call.  tau / keepall of every query from the sample's s~ (compared with
    the kernel's words); the entry count of every bucket; for a bucket that did not overflow, every query's entry
    count and -- from the s~ keys its entries carry -- its band count, s~ >= round_down(T~_k - 2E) with T~_k the
    k-th largest of its entries.  `cause` marks the queries the rules leave unresolved: a bucket over 256 * 512
    entries, keepall, no finite tau, more than 512 or fewer than k entries, a band over 256."""
    w = _batch_layout(q.n, q.n_pad, g.n, g.n_pad, k)
    host = ws[:w["cand"]].cpu().numpy()
    st = host[:q.n * w["ns_pad"]].reshape(q.n, w["ns_pad"])[:, :w["ns"]]
    E = _E(q.err(mode), g.err_max(mode), g.d_pad, mode)
    tau, keepall = np.zeros(q.n), np.zeros(q.n, bool)
    for i in range(q.n):
        tau[i], keepall[i], _ = _tau_of(st[i][~np.isnan(st[i])], k, E[i])
        assert (host[w["keepall"]:].view(np.int32)[i] != 0) == keepall[i]
        if not keepall[i]:
            assert host[w["tau"] + i] == np.float32(tau[i]), f"query {i}: tau"
    cand = ws[w["cand"]:w["total"]].view(torch.int64)
    bucket = cand[:w["nb"]].cpu().numpy()
    rows = w["nb"] * 256
    entries, band, b_ovf = np.zeros(rows, np.int64), np.zeros(rows, np.int64), np.zeros(rows, bool)
    for b in range(w["nb"]):
        if bucket[b] > w["cap_b"]:
            b_ovf[256 * b:256 * b + 256], entries[256 * b:256 * b + 256] = True, -1
        elif bucket[b] > 0:
            e = cand[w["nb"] + b * w["cap_b"]:w["nb"] + b * w["cap_b"] + int(bucket[b])].cpu().numpy()
            rl = (e >> 24) & 255
            assert ((e & 0xffffff) < g.n).all() and (256 * b + rl < q.n).all(), "an entry names a padding row or column"
            entries[256 * b:256 * b + 256] = np.bincount(rl, minlength=256)
            key = ((e >> 32) & 0xffffffff).astype(np.uint32)  # topk_key: larger score, larger key
            sv = np.where(key & np.uint32(0x80000000), key & np.uint32(0x7fffffff), ~key).view(np.float32)
            order = np.argsort(rl, kind="stable")
            ends = np.cumsum(entries[256 * b:256 * b + 256])
            for r in np.flatnonzero(entries[256 * b:256 * b + 256]):
                i = 256 * b + r
                sr = np.sort(sv[order[ends[r] - entries[i]:ends[r]]])
                assert (sr >= np.float32(tau[i])).all(), f"query {i}: an entry under tau"
                if k <= sr.size <= BT_LCAP:
                    band[i] = (sr >= _f32_down(float(sr[-k]) - 2.0 * E[i])).sum()
    n = q.n
    cause = b_ovf[:n] | keepall | ~np.isfinite(tau) | (entries[:n] > BT_LCAP) | (entries[:n] < k) | (band[:n] > BT_BAND)
    return dict(tau=tau, keepall=keepall, bucket=bucket, entries=entries[:n], band=band[:n], cause=cause, E=E, w=w)


def _check_batch(q, g, mode, k, cos=None, what="", complete=True):
    """The contract of every call: a row equals the reference or is wholly -2 / NaN; *unresolved counts the -2 rows;
    the -2 rows are exactly those with a restated cause (_batch_state), so no failure hides behind the fallback; the
    unresolved rows, sent through cmve_topk as engine.topk does, equal the reference too.  Returns (mask of the
    unresolved rows, the restated state)."""
    cos = _cos(q.x, g.x, q.eps) if cos is None else cos
    ridx, rsc = _ref(cos, g.x, k, what)
    idx, sc, unres, ws = _batch(q, g, mode, k)
    un = idx[:, 0] == -2
    assert ((idx == -2).all(axis=1) == un).all() and ((idx == -2).any(axis=1) == un).all(), f"{what}: a row half -2"
    assert np.isnan(sc[un]).all() and unres == int(un.sum()), f"{what}: unresolved {unres} against {int(un.sum())}"
    st = _batch_state(ws, q, g, mode, k)
    odd = np.flatnonzero(un != st["cause"])
    assert odd.size == 0, f"{what}: rows {odd[:8]} are {'un' if un[odd[0]] else ''}resolved against the rules: " \
                          f"entries {st['entries'][odd[:8]]} band {st['band'][odd[:8]]}"
    _assert_rows(idx[~un], sc[~un], ridx[~un], rsc[~un], what)
    if complete and un.any():
        sub = S(q.x[un], eps=q.eps)
        i2, s2, ovf, _ = _topk(sub, g, mode, k, want_ws=False)
        assert ovf == 0
        _assert_rows(i2, s2, ridx[un], rsc[un], f"{what} (completed by cmve_topk)")
    st["idx"] = idx
    return un, st


@functools.lru_cache(maxsize=None)
def _gauss_problem(nq, ng, seed):
    rng = np.random.default_rng(seed)
    xg = rng.standard_normal((ng, 64)).astype(np.float32)
    xq = (xg[rng.integers(0, ng, nq)] + 2.0 * rng.standard_normal((nq, 64))).astype(np.float32)
    return xq, xg, _cos(xq, xg)


@pytest.mark.parametrize("k", [1, 5, 32])
@pytest.mark.parametrize("nq,ng,geo", [(200, 4000, "g64"), (300, 4099, "g128"), (1000, 32700, "g256")])
def test_batch_geometries(nq, ng, geo, k):
    """EPI_TOPK in the three tile geometries (the G64 ring kernel is below engine.topk's 512-query gate), Gaussian
    rows at d = 64.  A query's entry count is roughly geometric around 128 at k = 1 (P(> 512) ~ e^-4): there the
    unresolved rows are exactly those with more than 512 entries; at k = 5 and 32 every row resolves."""
    xq, xg, cos = _gauss_problem(nq, ng, 11)
    q, g = S(xq), S(xg)
    took = "g256" if _phased(q.n_pad, g.n_pad) else ("g64" if _g64(q.n_pad, g.n_pad) else "g128")
    assert took == geo
    un, st = _check_batch(q, g, F16, k, cos, f"{geo} k {k}")
    assert (un == (st["entries"] > BT_LCAP)).all(), "a row unresolved for another cause than its entry count"
    assert k == 1 or not un.any(), f"{int(un.sum())} of {nq} unresolved"
    print(f"BATCH {geo} k={k}: unresolved {int(un.sum())} of {nq}, entries per query up to {st['entries'].max()}")


@pytest.mark.parametrize("nq", [1, 16, 17, 255, 256, 257])
def test_batch_ragged_queries(nq):
    """A partial last finish block (16 queries each), a partial query tile, rows in a second bucket."""
    xq, xg, cos = _gauss_problem(257, 4000, 12)
    q, g = S(xq[:nq]), S(xg)
    un, _ = _check_batch(q, g, F16, 5, cos[:nq], f"n_q {nq}")
    assert not un.any(), f"rows {np.flatnonzero(un)} unresolved"


def _grouped(ng, ns, group_cs, k, rng, lo=-0.6, hi=0.2):
    """A gallery for q = e0 with a planted high group: its k lowest cosines lie in the sample (rows [0, ns)), the
    rest outside it; every other row is a filler in [lo, hi].  Returns (rows, the group's columns)."""
    cs = rng.uniform(lo, hi, ng)
    group_cs = np.sort(np.asarray(group_cs))
    inside = np.sort(rng.choice(ns, k, replace=False))
    outside = ns + np.sort(rng.choice(ng - ns, group_cs.size - k, replace=False))
    cs[inside] = group_cs[:k]
    cs[outside] = group_cs[k:][rng.permutation(group_cs.size - k)]
    return _planted(cs), np.concatenate([inside, outside])


@pytest.mark.parametrize("mode", [F16, BF16X3])
def test_batch_entry_cap(mode):
    """BT_LCAP: a group of exactly 512 rows above tau resolves (as one of exactly k rows does), 513 do not.  The
    group's cosines run from 0.56295 (near the top of the bin whose lower edge is 0.5625) to 0.95, 7.6e-4 apart at
    512 rows: the band of the k-th best holds a few rows.  Its k lowest are in the sample, so tau = round_down(0.5625
    - 2^-20 - 2E): more than E under every group row and hundreds of E above every filler (<= 0.2) -- no s~ can be
    on the wrong side."""
    rng = np.random.default_rng(51)
    ng, k, nq = 8192, 4, 3
    for size in (k, 512, 513):  # (k: the shortest list that can resolve, m >= k)
        w = _batch_layout(nq, 256, ng, ng, k)
        xg, _ = _grouped(ng, w["ns"], np.linspace(0.56295, 0.95, size), k, rng)
        q, g = S(_e0(nq)), S(xg)
        un, st = _check_batch(q, g, mode, k, what=f"group of {size} {MODES[mode]}")
        assert (st["tau"] > 0.2 + 20 * st["E"]).all() and (st["tau"] < 0.56295 - st["E"]).all()
        assert (st["entries"] == size).all(), st["entries"]
        assert un.all() == (size > BT_LCAP) and un.any() == (size > BT_LCAP)


@pytest.mark.parametrize("mode", [F16, BF16X3])
def test_batch_band_cap(mode):
    """BT_BAND: 256 bit-identical rows as the best of the gallery resolve to the first k by index; 257 do not."""
    rng = np.random.default_rng(52)
    ng, k, nq = 8192, 8, 2
    for size in (256, 257):
        w = _batch_layout(nq, 256, ng, ng, k)
        xg, cols = _grouped(ng, w["ns"], np.full(size, 0.75), k, rng)
        q, g = S(_e0(nq)), S(xg)
        un, st = _check_batch(q, g, mode, k, what=f"{size} duplicates {MODES[mode]}")
        assert (st["entries"] == size).all() and (st["band"] == size).all(), (st["entries"], st["band"])
        assert un.all() == (size > BT_BAND) and un.any() == (size > BT_BAND)
        assert list(_ref(_cos(q.x, xg), xg, k)[0][0]) == list(np.sort(cols)[:k])


def test_batch_bucket_cap():
    """256 * 512 entries per 256-query tile: 200 queries along e0 with 600 entries each and 56 along e2 with 300 each
    send 136,800 entries to bucket 0, so every row of that tile is unresolved -- also the 56 whose own 300 entries
    would have fitted -- while the 20 e2 queries of the next tile resolve."""
    rng = np.random.default_rng(53)
    ng, k = 16384, 4
    w = _batch_layout(276, 512, ng, ng, k)
    xg, ca = _grouped(ng, w["ns"], np.linspace(0.56295, 0.95, 600), k, rng)
    free = np.setdiff1d(np.arange(ng), ca)
    inside = free[free < w["ns"]][:k]
    cb = np.concatenate([inside, rng.choice(free[free >= w["ns"]], 300 - k, replace=False)])
    # the e2 group: (0, sqrt(1 - c^2), c, 0, ...), its k lowest in the sample; the e0 queries score it 0, a filler,
    # as the e2 queries score every other row
    csb = np.linspace(0.56295, 0.95, 300)
    xg[cb] = 0.0
    xg[cb, 2] = csb
    xg[cb, 1] = np.sqrt(1.0 - csb * csb)
    xq = np.zeros((276, 64))
    xq[:200, 0] = 1.0
    xq[200:, 2] = 1.0
    q, g = S(xq), S(xg)
    un, st = _check_batch(q, g, F16, k, what="bucket cap")
    assert st["bucket"][0] == 200 * 600 + 56 * 300 > st["w"]["cap_b"] and st["bucket"][1] == 20 * 300
    assert un[:256].all() and not un[256:].any() and (st["entries"][256:] == 300).all()


@pytest.mark.parametrize("nq,ng", [(200, 4099), (257, 1000), (40, 300)])
def test_batch_all_scores_negative(nq, ng):
    """Every cosine negative, ragged n_g and n_q: the zero rows of the padding (score 0, above every real score)
    emit nothing, for padded columns and for padded query rows alike."""
    rng = np.random.default_rng(ng)
    xg = _planted(rng.uniform(-0.9, -0.1, ng), sign=np.where(rng.random(ng) < 0.5, -1.0, 1.0))
    q, g = S(_e0(nq, tilt=np.linspace(-0.05, 0.05, nq))), S(xg)
    for mode in MODES:
        un, st = _check_batch(q, g, mode, 5, what=f"negative {nq} x {ng} {MODES[mode]}")  # (no entry in the padding)
        assert (st["tau"] < 0).all() and not un.any(), f"rows {np.flatnonzero(un)} unresolved"
        assert st["bucket"].sum() == st["entries"].sum()


def test_batch_sample_edge_cases():
    """A sample with fewer than k finite rows (keepall), a sample whose k-th score is -1 (bin 0: tau = -inf) and a
    zero query row are unresolved; NaN gallery rows outside the sample never enter a resolved row."""
    rng = np.random.default_rng(54)
    ng, k = 4096, 4
    ns = _batch_layout(4, 256, ng, ng, k)["ns"]
    xg = _planted(rng.uniform(-0.5, 0.5, ng))
    xg[ns + 5:ns + 400:7] = 0.0          # NaN rows outside the sample
    xg[2:ns] = 0.0                       # the sample of the e0 queries: two finite rows
    xq = np.concatenate([_e0(2, tilt=[0.0, 0.01]), np.zeros((1, 64))])
    q, g = S(xq), S(xg)
    un, st = _check_batch(q, g, F16, k, what="keepall sample")
    assert st["keepall"].all() and un.all() and st["bucket"].sum() == 0
    # a sample of antipodal rows around three better ones: the k-th best of the sample is -1
    xg = _planted(rng.uniform(-0.5, 0.5, ng))
    xg[:ns] = -_e0(ns)
    xg[[3, 40, 77]] = _planted([0.2, 0.1, 0.3])
    xg[ns + 5:ns + 400:7] = 0.0
    xq = np.concatenate([_e0(2), _planted([0.6])])
    q, g = S(xq), S(xg)
    un, st = _check_batch(q, g, F16, k, what="bin-0 sample")
    assert (st["tau"][:2] == -INF).all() and un[:2].all()
    # live sample, NaN rows beyond it, a zero query row between live ones
    xg = _planted(rng.uniform(-0.5, 0.5, ng))
    xg[ns + 5:ns + 900:3] = 0.0
    xq = np.concatenate([_e0(1), np.zeros((1, 64)), _e0(1, tilt=0.3)])
    q, g = S(xq), S(xg)
    un, st = _check_batch(q, g, F16, k, what="zero query row")
    assert list(un) == [False, True, False]
    assert not np.isin(st["idx"][~un], np.flatnonzero(~xg.any(axis=1))).any()


@pytest.mark.parametrize("qdt,gdt", [(F32, F32), (F32, F64), (F64, F32), (F64, F64)])
def test_batch_modes_and_dtype_pairs(qdt, gdt):
    """The three modes on one shape in each of the four raw dtype pairs, the raw rows strided (gaps at 1e30)."""
    xq, xg, _ = _gauss_problem(100, 3000, 13)
    xq, xg = xq.astype(NP[qdt]), xg.astype(NP[gdt])
    cos = _cos(xq, xg)
    q, g = S(xq, raw_ld=67), S(xg, raw_ld=65)
    for mode in MODES:
        un, _ = _check_batch(q, g, mode, 5, cos, f"{MODES[mode]} {qdt} {gdt}")
        assert not un.any(), f"rows {np.flatnonzero(un)} unresolved"


def test_batch_refusals():
    """k = 0 / 33, a short workspace, CMVE_PACK_RAW, an unknown mode, a dimension mismatch, NULL arguments: refused
    with CMVE_E_INVALID and a message; out_idx / out_score unwritten (*unresolved is cleared before the workspace
    check, unwritten by the others)."""
    h, lib, check, _ = _api()
    rng = np.random.default_rng(3)
    q, g = S(rng.standard_normal((20, 64))), S(rng.standard_normal((500, 64)))
    g32 = S(rng.standard_normal((500, 32)))
    ns, nf = ctypes.c_int64(), ctypes.c_int64()
    check(lib.cmve_topk_batch_workspace(ctypes.byref(q.desc), ctypes.byref(g.desc), 5, ctypes.byref(ns),
                                        ctypes.byref(nf)), "cmve_topk_batch_workspace")
    ws = torch.full((nf.value,), 2.0, dtype=torch.float32, device="cuda")
    idx, sc, un = _refusal_windows(20, 5)

    def call(qq=q.desc, gg=g.desc, mode=F16, k=5, w=ws.data_ptr(), n=nf.value, i=idx.ptr, s=sc.ptr, o=un.ptr):
        return lib.cmve_topk_batch(h, ctypes.byref(qq), ctypes.byref(gg), mode, k, w, n, i, s, o)

    for change, text in [(dict(k=0), "k must be in [1, 32]"), (dict(k=33), "k must be in [1, 32]"),
                         (dict(qq=q.variant(flags=1)), "CMVE_PACK_RAW"), (dict(gg=g.variant(flags=1)), "CMVE_PACK_RAW"),
                         (dict(mode=3), "unknown mode"), (dict(gg=g32.desc), "dimension mismatch"),
                         (dict(w=None), "NULL"), (dict(i=None), "NULL"), (dict(s=None), "NULL"),
                         (dict(o=None), "NULL")]:
        assert call(**change) == E_INVALID and text in _msg(), (change, _msg())
        for p in (idx, sc, un):
            p.assert_untouched(f"an output of a cmve_topk_batch refused for {text}")
    assert call(n=nf.value - 1) == E_INVALID and "workspace has" in _msg()
    idx.assert_untouched("out_idx")
    sc.assert_untouched("out_score")
    assert un.numpy()[0, 0] == 0
    assert bool((ws == 2.0).all())
    assert lib.cmve_topk_batch_workspace(ctypes.byref(q.desc), ctypes.byref(g.desc), 33, None, ctypes.byref(nf)) \
        == E_INVALID
    assert call() == 0


# ------------------------------------------------------------------ D. an order inverted by more than E
def _plane(x, mode):
    """The value an element of the unit row takes in the plane of the mode (fp32 first, as the pack kernel)."""
    xf = np.asarray(x, np.float64).astype(np.float32)
    if mode == F16:
        return xf.astype(np.float16).astype(np.float64)
    u = xf.view(np.uint32).astype(np.uint64)
    r = (((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16) & 0xffffffff  # bf16, round to nearest even
    return r.astype(np.uint32).view(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def _inverted_pair(mode):
    """The search of DESIGN.md s7 (top-k edges): a Gaussian query q at d = 64, dq = plane(q^) - q^; gallery rows are
    sign vectors over 8 (exact in fp16 and bf16, norm exactly 1: their planes are the rows, E = eq + gamma (1 + eq)
    + 1e-12), for which s~ - cos = <dq, g> up to the fp32 sum.  2e5 rows are drawn biased toward sign(dq) (each sign
    flipped with probability p in {0.1, 0.15, 0.2}) and 2e5 biased against; the pair (a, b) with cos_a - cos_b in
    (1e-9, 1e-5) and cos_a > -0.1 (room for fillers below) maximises (dev_b - dev_a - gap) / E.  The fillers are
    4,094 sign vectors biased against sign(q), at least 0.06 under cos_a, the best first (they are the batch path's
    sample).  Returns (q, a, b, fillers, emulated ratio)."""
    rng = np.random.default_rng(2025)
    d, N = 64, 200000
    q = rng.standard_normal(d)
    qh = q / np.linalg.norm(q)
    dq = _plane(qh, mode) - qh
    eq = np.linalg.norm(dq)
    n = d * 33.0 / 32.0
    gam = n * 2.0 ** -23 / (1 - n * 2.0 ** -23)
    E = eq + gam * (1 + eq) + 1e-12
    sg = np.where(dq < 0, -1.0, 1.0)
    best = (-INF,)
    for p in (0.1, 0.15, 0.2):
        sb = np.where(rng.random((N, d)) < p, -sg, sg) / 8.0
        sa = np.where(rng.random((N, d)) < p, sg, -sg) / 8.0
        cb, ca, db, da = sb @ qh, sa @ qh, sb @ dq, sa @ dq
        ob = np.argsort(cb)
        pos = np.searchsorted(cb[ob], ca) - 1
        jb = ob[np.clip(pos, 0, N - 1)]
        gap = np.where((pos >= 0) & (ca > -0.1), ca - cb[jb], INF)
        score = np.where((gap > 1e-9) & (gap < 1e-5), (db[jb] - da - gap) / E, -INF)
        ia = int(np.argmax(score))
        if score[ia] > best[0]:
            best = (float(score[ia]), sa[ia].copy(), sb[jb[ia]].copy(), float(ca[ia]))
    ratio, a, b, cos_a = best
    f = np.where(rng.random((8000, d)) < 0.8, -np.sign(qh), np.sign(qh)) / 8.0
    cf = f @ qh
    f = f[cf <= cos_a - 0.06]
    f = f[np.argsort(-(f @ qh), kind="stable")][:4094]
    assert f.shape[0] == 4094
    return q[None, :], a, b, f, ratio


@pytest.mark.parametrize("mode", [F16, BF16])
def test_order_inverted_by_more_than_E(mode):
    """The true best row a scores BELOW b by more than E in s~ (emulated ratio >= 1.1 asserted first; the device's
    (s~_b - s~_a) / E printed and asserted > 1): only the full 2E band keeps a.  Through cmve_topk at k = 1, through
    cmve_topk_batch with a and b outside the sample, and through the rank path with GT = a (rank 1)."""
    from cmve import engine
    xq, a, b, fill, ratio = _inverted_pair(mode)
    print(f"INVERT {MODES[mode]}: emulated (dev_b - dev_a - gap) / E = {ratio:.3f}")
    assert ratio >= 1.1
    ia, ib = 3000, 2000
    xg = np.concatenate([fill[:ib], b[None], fill[ib:ia - 1], a[None], fill[ia - 1:]])
    assert xg.shape[0] == 4096 and (xg[ia] == a).all() and (xg[ib] == b).all()
    q, g = S(xq), S(xg)
    assert g.err_max(mode) <= 2e-12  # sign vectors over 8 are their own planes
    cos = _cos(xq, xg)
    assert np.argmax(cos[0]) == ia and 1e-9 < cos[0, ia] - cos[0, ib] < 1e-5 and np.sort(cos[0])[-3] < cos[0, ib] - 0.05
    assert _check_topk(q, g, mode, 1, cos, "inverted pair")[0] == 0
    idx, _, _, ws = _topk(q, g, mode, 1)
    st = _stilde(ws, q, g)[0]
    E = _E(q.err(mode), g.err_max(mode), g.d_pad, mode)[0]
    dev = (float(st[ib]) - float(st[ia])) / E
    print(f"INVERT {MODES[mode]}: device (s~_b - s~_a) / E = {dev:.3f}, E = {E:.3e}")
    assert dev > 1.0 and idx[0, 0] == ia
    ns = _batch_layout(1, 256, 4096, 4096, 1)["ns"]
    assert ns < ib
    un, _ = _check_batch(q, g, mode, 1, cos, "inverted pair, batch")
    assert not un.any()
    ranks, _, _ = engine.gt_rank_counts(q.rs, g.rs, row_gts=[[ia]], mode=mode)
    assert list(ranks) == [1]
