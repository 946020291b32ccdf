"""K24's host-only surface: the declarations of the new entries, the workspace arithmetic of
cmve_jaccard_count_workspace and its refusals, the ``filter="jaccard"`` dispatch -- and a numpy restatement of the bound
of DESIGN s4 (K24), run over adversarial rows against the canonical two-accumulator chain with float32 words: it may
decide nothing wrongly and must leave less than 1/8 of the pairs to the re-score.  No kernel is launched, no GPU
needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cmve_jaccard_rowsums", "cmve_jaccard_count_workspace", "cmve_jaccard_count")


def test_header_declares_and_library_exports_the_entries():
    from cmve import _lib
    src = open(os.path.join(ROOT, "include", "cmve.h")).read()
    for name in NAMES:
        assert re.search(r"^int\s+%s\s*\(" % name, src, re.M), f"{name} is not declared in cmve.h"
        assert hasattr(_lib.lib, name) and name in _lib.exported_symbols()
    # every entry cites what it replaces
    doc = src[src.index("/* K24:"):src.index("int cmve_jaccard_rowsums")]
    assert doc.count("evaluation.py:32-35") >= len(NAMES) and doc.count("metrics.py:61-157") >= len(NAMES)
    assert ":56-72" in doc
    # additive: the ABI is still 21 and the K19 / K21 / K22 entries are still there
    assert "#define CMVE_ABI_VERSION 21" in src and _lib.lib.cmve_abi_version() == 21
    for old in ("cmve_l2_count", "cmve_l2_count_resolved", "cmve_l1_pack_size", "cmve_l1_grid", "cmve_l1_pack",
                "cmve_l1_count_workspace", "cmve_l1_count", "cmve_pairwise_count"):
        assert re.search(r"^int\s+%s\s*\(" % old, src, re.M) and old in _lib.exported_symbols()


def test_the_count_takes_the_resolved_entrys_list_arguments():
    src = open(os.path.join(ROOT, "include", "cmve.h")).read()

    def params(name):
        m = re.search(r"^int\s+%s\s*\(([^;]*)\);" % name, src, re.M | re.S)
        return re.sub(r"\s+", " ", m.group(1)).strip()

    tail = params("cmve_l2_count_resolved").split("double alpha, double beta, ")[1]
    mine = params("cmve_jaccard_count")
    assert mine.endswith("double alpha, double beta, " + tail)
    # cmve_l1_count's head with the two per-row arrays added on each side
    head = params("cmve_l1_count").split("double alpha, double beta, ")[0]
    head = head.replace("const double* a_err, ", "const double* a_err, const int64_t* a_qsum, const double* a_asum, ")
    head = head.replace("const double* b_err, ", "const double* b_err, const int64_t* b_qsum, const double* b_asum, ")
    assert mine.startswith(head)


def test_workspace_arithmetic_and_refusals():
    from cmve import _lib, engine
    for cap in (0, 1, 8, 1 << 20):
        assert engine.jaccard_count_workspace(cap) == 8 * cap == engine.l1_count_workspace(cap)
    nbytes = C.c_int64()
    for cap in (-1, -(1 << 40), (1 << 63) - 1, (1 << 60) + 1):
        assert _lib.lib.cmve_jaccard_count_workspace(cap, C.byref(nbytes)) < 0
        assert b"cmve_jaccard_count_workspace" in _lib.lib.cmve_last_error()
    assert _lib.lib.cmve_jaccard_count_workspace(8, None) < 0
    assert b"cmve_jaccard_count_workspace" in _lib.lib.cmve_last_error()


def test_filter_jaccard_refuses_before_any_device_call():
    import torch
    from cmve import _lib, engine

    class NoDevice:
        """Rows that fail loudly if the call gets as far as touching them."""
        def __getattr__(self, name):
            raise AssertionError("the call touched its operands before refusing")

    a = b = NoDevice()
    for fn in (engine.pairwise_count, engine.pairwise_gt_ranks, engine.pairwise_gt_positions, engine.pairwise_gt_eval):
        with pytest.raises(ValueError, match='filter="jaccard" needs PW_JACCARD'):
            fn(a, b, _lib.PW_L1, 1.0, 0.0, torch.float64, filter="jaccard")
        with pytest.raises(ValueError, match='filter="jaccard".*float32 score words'):
            fn(a, b, _lib.PW_JACCARD, -1.0, 0.0, torch.float64, filter="jaccard")
        for alpha, beta in ((0.0, 0.0), (float("nan"), 0.0), (float("inf"), 0.0), (1.0, float("inf")),
                            (-1.0, float("nan"))):
            with pytest.raises(ValueError, match='filter="jaccard".*alpha finite and non-zero'):
                fn(a, b, _lib.PW_JACCARD, alpha, beta, torch.float32, filter="jaccard")
    # the other forced routes keep refusing jaccard with their own words
    with pytest.raises(ValueError, match="PW_L2"):
        engine.pairwise_count(a, b, _lib.PW_JACCARD, -1.0, 0.0, torch.float32, filter=True)
    with pytest.raises(ValueError, match="PW_L1"):
        engine.pairwise_count(a, b, _lib.PW_JACCARD, -1.0, 0.0, torch.float32, filter="l1")
    # the auto threshold: off, or above the 300 x 520 the tests expect on the K18 route
    assert engine.JACCARD_FILTER_MIN_PAIRS is None or engine.JACCARD_FILTER_MIN_PAIRS > 300 * 520
    assert engine._filter_route("x", None, _lib.PW_JACCARD, -1.0, 0.0, torch.float64, False, (1 << 40, 64, True)) is None


# ---- the bound of DESIGN s4 (K24), restated in numpy -------------------------------------------------------------------

U = 2.0 ** -53
NA, NB = 300, 520


def _ulps(v, steps):
    for _ in range(steps):
        v = np.nextafter(v, v.dtype.type(np.inf))
    return v


def _adversarial(d, dt_a, dt_b, nonneg):
    """The recipe of tests/test_l1_filter_host.py; ``nonneg``: the rows as np.abs(rows)."""
    rng = np.random.default_rng(d)
    b = rng.standard_normal((NB, d))
    pick = rng.integers(0, 200, NA)
    pick[20] = 7
    a = b[pick] + 0.5 * rng.standard_normal((NA, d))
    if nonneg:
        a, b = np.abs(a), np.abs(b)
    with np.errstate(over="ignore"):
        a, b = a.astype(dt_a), b.astype(dt_b)
        b[256:296] = b[0:40]
        for t in range(40):
            row = b[7].copy()
            row[t % d] = _ulps(row[t % d], (1, 2, 4)[t % 3])
            b[300 + t] = row
        a[10], b[400] = 0.0, 0.0
        a[11], b[401] = 1e200, 1e200
        a[12], b[402] = 1e-200, 1e-200
        a[13, 5 % d], b[403, 3] = np.inf, np.inf
        a[14, 0], b[404, 1] = np.nan, np.nan
    rows = [[int(p)] for p in pick]
    rows[20] = [7, 300, 301, 305, 320, 263, 339]
    rows[21] = []
    rows[22] = [5, 5]
    rows[23] = [404, 3, 404]
    rows[24] = [400, 401, 402, 403]
    rows[10], rows[11], rows[12], rows[13], rows[14] = [1], [2, 401], [3, 402], [4], [6, 404]
    cols = [[] for _ in range(NB)]
    for i, p in enumerate(pick):
        cols[int(p)].append(i)
    for j in range(30):
        cols[j] = list(map(int, rng.integers(0, NA, 20)))
    cols[31], cols[32], cols[33] = [4, 4], [14, 2, 14], []
    for j in (400, 401, 402, 403, 404, 300, 263):
        cols[j] = [20, 10, 11, 12, 13, 14]
    return a.astype(np.float64), b.astype(np.float64), rows, cols


def _grid(*sets):
    """(lo, s) from the min / max of the eligible elements (|x| <= 1e30) of the sets."""
    el = np.concatenate([x[np.abs(x) <= 1e30] for x in sets])
    if el.size == 0 or not el.max() > el.min():
        return 0.0, 1.0
    return float(el.min()) + 0.0, float((el.max() - el.min()) / 65535.0)


def _pack(x, lo, s):
    """K22's codes and row errors (tests/test_l1_filter_host.py), and K24's two extras: the exact code sum and
    S >= sum |x| (+inf where err is)."""
    d = x.shape[1]
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.clip(np.nan_to_num(np.rint((x - lo) / s), nan=0.0), 0.0, 65535.0)
        xh = q * s + lo
        df = np.abs(x - xh)
        term = df + 4.0 * U * (df + np.abs(xh)) + 1e-300
        term = np.where(np.abs(x) <= 1e150, term, np.inf)
        err = term.sum(axis=1) * (1.0 + 4.0 * (d + 8.0) * U) + 1e-300
        mag = np.where(np.abs(x) <= 1e150, np.abs(x), np.inf)
        asum = mag.sum(axis=1) * (1.0 + 4.0 * (d + 8.0) * U) + 1e-300
    q = q.astype(np.int64)
    return q, err, q.sum(axis=1), asum


def _side(err, asum, qsum, d, lo, s):
    """jacf_side: the row's half of P and of the interval's width."""
    with np.errstate(invalid="ignore", over="ignore"):
        dl, sq = d * lo, s * qsum.astype(np.float64)
        return dl + sq, err + ((d + 2.0) * U) * asum + (16.0 * U) * (abs(dl) + sq)


def _mid(t):
    """The float32 rounding boundary below the finite-or-+inf float32 word t, exact in fp64."""
    if t == np.inf:
        return float.fromhex("0x1.ffffffp127")
    p = np.nextafter(np.float32(t), np.float32(-np.inf))
    if np.isinf(p):
        return float(t) - 2.0 ** 103
    return 0.5 * (float(p) + float(t))


def _thresholds(t, alpha, beta):
    """(tl, tu) of jacf_thresholds for an item word that is neither NaN nor -inf; (nan, nan): nothing decided."""
    mid = _mid(t)
    with np.errstate(over="ignore", invalid="ignore"):
        x = np.float64(mid - beta) / np.float64(alpha)
        sig = 16.0 * U * ((abs(mid) + abs(beta)) / abs(alpha)) + 1e-290 + 2.0 ** -1074 / abs(alpha)
        if not (abs(x) < 1e300 and sig < 1e300):
            return np.nan, np.nan
        xlo, xhi = x - sig, x + sig
        return xlo - 4.0 * U * abs(xlo), xhi + 4.0 * U * abs(xhi)


def _canonical(a, b, alpha, beta):
    """The canonical float32 words: fmin / fmax summed for k ascending into two accumulators from zero, s0 / s1,
    alpha x + beta, ONE rounding to float32."""
    s0 = np.zeros((a.shape[0], b.shape[0]))
    s1 = np.zeros((a.shape[0], b.shape[0]))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for k in range(a.shape[1]):
            s0 += np.fmin(a[:, k][:, None], b[:, k][None, :])
            s1 += np.fmax(a[:, k][:, None], b[:, k][None, :])
        return (alpha * (s0 / s1) + beta).astype(np.float32)


CASES = [(dts, nonneg, ab)
         for dts in ((np.float32, np.float32), (np.float64, np.float64), (np.float32, np.float64))
         for nonneg in (True, False) for ab in ((-1.0, 0.0), (1.0, 0.0))]
CASES += [((np.float32, np.float32), True, (-0.5, 0.25)), ((np.float64, np.float64), False, (-0.5, 0.25))]


def _case_id(c):
    (da, db), nonneg, (alpha, beta) = c
    dt = "f32" if db == np.float32 else ("f64" if da == np.float64 else "mixed")
    return "%s-%s-a%gb%g" % (dt, "nonneg" if nonneg else "signed", alpha, beta)


@pytest.mark.parametrize("case", CASES, ids=[_case_id(c) for c in CASES])
def test_numpy_model_of_the_bound_decides_nothing_wrongly(case):
    dts, nonneg, (alpha, beta) = case
    d = 67
    a, b, rows, cols = _adversarial(d, *dts, nonneg)
    e = _canonical(a, b, alpha, beta).astype(np.float64)    # float32 words carried in doubles
    lo, s = _grid(a, b)
    qa, ea, Qa, Sa = _pack(a, lo, s)
    qb, eb, Qb, Sb = _pack(b, lo, s)
    sad = np.abs(qa[:, None, :] - qb[None, :, :]).sum(axis=2)
    assert sad.max() < 2 ** 32
    pa, wa = _side(ea, Sa, Qa, float(d), lo, s)
    pb, wb = _side(eb, Sb, Qb, float(d), lo, s)
    with np.errstate(invalid="ignore", over="ignore"):
        m = s * sad.astype(np.float64)
        P = pa[:, None] + pb[None, :]
        W = ((wa[:, None] + wb[None, :]) + 16.0 * U * m) * (1.0 + 1e-9) + 1e-280
        ih, uh = 0.5 * (P - m), 0.5 * (P + m)
        ulo, uhi = uh - W, uh + W
        ok = (W < 1e300) & (ulo > 0.0) & (uhi < 1e300)
        ilo, ihi = np.where(ok, ih - W, np.nan), np.where(ok, ih + W, np.nan)

    def lt(ihi_, ulo_, uhi_, T):
        with np.errstate(invalid="ignore", over="ignore"):
            return ihi_ < T * (ulo_ if T >= 0.0 else uhi_)

    def gt(ilo_, ulo_, uhi_, T):
        with np.errstate(invalid="ignore", over="ignore"):
            return ilo_ > T * (uhi_ if T >= 0.0 else ulo_)

    band = ~ok
    decided = wrong = 0
    for lists, by_row in ((rows, True), (cols, False)):
        for owner, items in enumerate(lists):
            sl = (owner, slice(None)) if by_row else (slice(None), owner)
            ilo_, ihi_, ulo_, uhi_, words, has = ilo[sl], ihi[sl], ulo[sl], uhi[sl], e[sl], ok[sl]
            for it in items:
                t = e[owner, it] if by_row else e[it, owner]
                if np.isnan(t) or t == -np.inf:
                    below, notbelow = np.zeros(words.shape, bool), has.copy()   # never counted
                else:
                    tl, tu = _thresholds(t, alpha, beta)
                    if np.isnan(tl):
                        below = notbelow = np.zeros(words.shape, bool)
                    else:
                        q_lt, q_gt = lt(ihi_, ulo_, uhi_, tl), gt(ilo_, ulo_, uhi_, tu)
                        below, notbelow = (q_lt, q_gt) if alpha > 0 else (q_gt, q_lt)
                und = ~(below | notbelow)
                if by_row:
                    band[owner] |= und
                else:
                    band[:, owner] |= und
                with np.errstate(invalid="ignore"):
                    truth = words < t
                wrong += int((below & ~truth).sum() + (notbelow & truth).sum())
                decided += int((below | notbelow).sum())
    print("decided comparisons %d, wrong %d, band %d of %d (%.2f%%)" % (decided, wrong, band.sum(), band.size,
                                                                         100.0 * band.sum() / band.size))
    assert wrong == 0 and decided > 0
    assert 0 < band.sum() < NA * NB // 8
