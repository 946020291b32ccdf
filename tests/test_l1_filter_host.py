"""K22's host-only surface: the pad / workspace arithmetic of cmve_l1_pack_size and cmve_l1_count_workspace and
their refusals, the declarations of the new entries, the ``filter="l1"`` dispatch -- and a numpy restatement of the
bound of DESIGN s4 (K22), run over adversarial rows against the canonical chain: it may decide nothing wrongly and
must leave less than 1/8 of the pairs to the re-score.  No kernel is launched, no GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cmve_l1_pack_size", "cmve_l1_grid", "cmve_l1_pack", "cmve_l1_count_workspace", "cmve_l1_count")


def test_header_declares_and_library_exports_the_entries():
    from cmve import _lib
    src = open(os.path.join(ROOT, "include", "cmve.h")).read()
    for name in NAMES:
        assert re.search(r"^int\s+%s\s*\(" % name, src, re.M), f"{name} is not declared in cmve.h"
        assert hasattr(_lib.lib, name) and name in _lib.exported_symbols()
    # every entry cites what it replaces
    doc = src[src.index("/* K22:"):src.index("int cmve_l1_pack_size")]
    assert doc.count("evaluation.py:24-29") >= len(NAMES) - 1 and doc.count("metrics.py:61-157") >= len(NAMES) - 1
    # additive: the ABI is still 21 and the Euclidean entries are still there
    assert "#define CMVE_ABI_VERSION 21" in src and _lib.lib.cmve_abi_version() == 21
    for old in ("cmve_l2_count_workspace", "cmve_l2_count", "cmve_l2_count_resolved", "cmve_pairwise_count"):
        assert re.search(r"^int\s+%s\s*\(" % old, src, re.M) and old in _lib.exported_symbols()


def test_the_count_takes_the_resolved_entrys_list_arguments():
    src = open(os.path.join(ROOT, "include", "cmve.h")).read()

    def params(name):
        m = re.search(r"^int\s+%s\s*\(([^;]*)\);" % name, src, re.M | re.S)
        return re.sub(r"\s+", " ", m.group(1)).strip()

    tail = params("cmve_l2_count_resolved").split("double alpha, double beta, ")[1]
    assert params("cmve_l1_count").endswith("double alpha, double beta, " + tail)


def test_pack_size_and_workspace_arithmetic():
    from cmve import _lib, engine
    for n, d, want in ((0, 1, (0, 32)), (1, 1, (128, 32)), (128, 32, (128, 32)), (129, 33, (256, 64)),
                       (300, 67, (384, 96)), (520, 1024, (640, 1024)), (131072, 65536, (131072, 65536))):
        assert engine.l1_pack_size(n, d) == want
    for cap in (0, 1, 8, 1 << 20):
        assert engine.l1_count_workspace(cap) == 8 * cap
    n_pad, d_pad, nbytes = C.c_int64(), C.c_int64(), C.c_int64()
    for n, d in ((-1, 4), (4, 0), (4, -3), (4, 65537), (1 << 31, 4)):
        assert _lib.lib.cmve_l1_pack_size(n, d, C.byref(n_pad), C.byref(d_pad)) < 0
        assert b"cmve_l1_pack_size" in _lib.lib.cmve_last_error()
    assert _lib.lib.cmve_l1_pack_size(4, 4, None, C.byref(d_pad)) < 0
    for cap in (-1, (1 << 63) - 1):
        assert _lib.lib.cmve_l1_count_workspace(cap, C.byref(nbytes)) < 0
        assert b"cmve_l1_count_workspace" in _lib.lib.cmve_last_error()
    assert _lib.lib.cmve_l1_count_workspace(8, None) < 0


def test_filter_l1_refuses_before_any_device_call():
    import torch
    from cmve import _lib, engine

    class NoDevice:
        """Rows that fail loudly if the call gets as far as touching them."""
        def __getattr__(self, name):
            raise AssertionError("the call touched its operands before refusing")

    a = b = NoDevice()
    for fn in (engine.pairwise_count, engine.pairwise_gt_ranks, engine.pairwise_gt_positions, engine.pairwise_gt_eval):
        with pytest.raises(ValueError, match="PW_L1"):
            fn(a, b, _lib.PW_L2, 1.0, 0.0, torch.float64, filter="l1")
        with pytest.raises(ValueError, match="float64 score words"):
            fn(a, b, _lib.PW_L1, 1.0, 0.0, torch.float32, filter="l1")
        for alpha, beta in ((0.0, 0.0), (float("nan"), 0.0), (float("inf"), 0.0), (1.0, float("inf"))):
            with pytest.raises(ValueError, match="alpha finite and non-zero"):
                fn(a, b, _lib.PW_L1, alpha, beta, torch.float64, filter="l1")
    # filter=True keeps speaking for PW_L2 alone
    with pytest.raises(ValueError, match="PW_L2"):
        engine.pairwise_count(a, b, _lib.PW_L1, 1.0, 0.0, torch.float64, filter=True)
    # the auto threshold: off, or above the 300 x 520 an existing test expects on the fp64 route
    assert engine.L1_FILTER_MIN_PAIRS is None or engine.L1_FILTER_MIN_PAIRS > 300 * 520
    assert engine._l2_count_stats(np.array([7, 5, 3, 1], np.int64)) == dict(decided=7, band=5, rescored=3, overflow=1)


def test_every_sad_filter_record_routes_with_the_words_it_had(monkeypatch):
    """The routes ``_filter_route`` gives for the SAD filters, record by record: the texts and results are literals."""
    import torch
    from cmve import _lib, engine
    want = {"l1": (_lib.PW_L1, torch.float64, torch.float32, "L1_FILTER_MIN_PAIRS", 8192 * 8192,
                   'x: filter="l1" needs PW_L1 with float64 score words, alpha finite and non-zero, beta finite'),
            "jaccard": (_lib.PW_JACCARD, torch.float32, torch.float64, "JACCARD_FILTER_MIN_PAIRS", 8192 * 8192,
                        'x: filter="jaccard" needs PW_JACCARD with float32 score words, alpha finite and non-zero, '
                        "beta finite")}
    assert list(engine._SAD_FILTERS) == list(want)
    for route in engine._SAD_FILTERS:
        metric, dt, other_dt, min_name, min_pairs, text = want[route]
        assert getattr(engine, min_name) == min_pairs
        for l2_scaling in (False, True):
            assert engine._filter_route("x", route, metric, -1.0, 0.25, dt, l2_scaling) == route
            for m, t, alpha, beta in ((_lib.PW_L2, dt, 1.0, 0.0), (_lib.PW_SQ_L2, dt, 1.0, 0.0), (metric, other_dt, 1.0, 0.0),
                                      (metric, dt, 0.0, 0.0), (metric, dt, float("nan"), 0.0),
                                      (metric, dt, float("inf"), 0.0), (metric, dt, 1.0, float("inf"))):
                with pytest.raises(ValueError) as ei:
                    engine._filter_route("x", route, m, alpha, beta, t, l2_scaling)
                assert str(ei.value) == text
            # a forced route is settled before the sizes are known; False and True never become this route later
            for flt in (route, False, True):
                assert engine._filter_route("x", flt, metric, 1.0, 0.0, dt, l2_scaling, (1 << 40, 64, True)) is None

        def auto(pairs, d=64, m=metric, t=dt, alpha=1.0, beta=0.0):
            return engine._filter_route("x", None, m, alpha, beta, t, False, (pairs, d, True))
        assert auto(min_pairs - 1) is None and auto(min_pairs) == route and auto(1 << 40) == route
        assert auto(min_pairs, d=65536) == route and auto(1 << 40, d=65537) is None
        assert auto(1 << 40, t=other_dt) is None and auto(1 << 40, alpha=0.0) is None
        assert auto(1 << 40, beta=float("nan")) is None
        monkeypatch.setattr(engine, min_name, 1)       # the name is read at call time
        assert auto(0) is None and auto(1) == route
        monkeypatch.setattr(engine, min_name, None)    # None: never automatically; the forced route stays
        assert auto(1 << 62) is None
        assert engine._filter_route("x", route, metric, 1.0, 0.0, dt, False) == route
        monkeypatch.undo()
    # before the sizes are known nothing is automatic
    assert engine._filter_route("x", None, _lib.PW_L1, 1.0, 0.0, torch.float64, False) is None


# ---- the bound of DESIGN s4 (K22), restated in numpy ---------------------------------------------------------------------

U = 2.0 ** -53
NA, NB = 300, 520


def _ulps(v, steps):
    for _ in range(steps):
        v = np.nextafter(v, v.dtype.type(np.inf))
    return v


def _adversarial(d, dt_a, dt_b):
    """The recipe of tests/test_gpu_l2_filter.py."""
    rng = np.random.default_rng(d)
    b = rng.standard_normal((NB, d))
    pick = rng.integers(0, 200, NA)
    pick[20] = 7
    a = b[pick] + 0.5 * rng.standard_normal((NA, d))
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
    """codes and the rows' errors: err >= sum |x - (lo + s q)|, +inf for a row with an element beyond 1e150 / NaN."""
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.clip(np.nan_to_num(np.rint((x - lo) / s), nan=0.0), 0.0, 65535.0)
        xh = q * s + lo                                      # (two roundings here, one on the device: charged below)
        df = np.abs(x - xh)
        term = df + 4.0 * U * (df + np.abs(xh)) + 1e-300
        term = np.where(np.abs(x) <= 1e150, term, np.inf)
        err = term.sum(axis=1) * (1.0 + 4.0 * (x.shape[1] + 8.0) * U) + 1e-300
    return q.astype(np.int64), err


def _thresholds(t, alpha, beta, d):
    """(T_lo, T_hi) of DESIGN s4 (K22) for finite item words t."""
    rho = 2.0 * (d + 16.0) * U
    x = (t - beta) / alpha
    sig = 16.0 * U * (np.abs(t) + abs(beta)) / abs(alpha) + 1e-290 + 2.0 ** -1074 / abs(alpha)
    xlo, xhi = x - sig, x + sig
    t_lo = np.where(xlo > 0.0, xlo * (1.0 - rho) * (1.0 - 4.0 * U), -np.inf)
    t_hi = np.where(xhi > 0.0, xhi * (1.0 + 2.0 * rho) * (1.0 + 4.0 * U), 0.0)
    return t_lo, t_hi


def _canonical(a, b, alpha, beta):
    """The canonical words: |a_k - b_k| summed for k ascending into one accumulator from zero, then alpha S + beta."""
    s = np.zeros((a.shape[0], b.shape[0]))
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(a.shape[1]):
            s += np.abs(a[:, k][:, None] - b[:, k][None, :])
        return alpha * s + beta


@pytest.mark.parametrize("ab", [(1.0, 0.0), (None, -1.0), (1.0, -1.0), (None, 0.0)], ids=["l1", "l1_norm", "a1b-1", "a-1/Db0"])
@pytest.mark.parametrize("dts", [(np.float32, np.float32), (np.float64, np.float64), (np.float32, np.float64)],
                         ids=["f32", "f64", "mixed"])
def test_numpy_model_of_the_bound_decides_nothing_wrongly(dts, ab):
    d = 67
    a, b, rows, cols = _adversarial(d, *dts)
    alpha, beta = (-1.0 / d if ab[0] is None else ab[0]), ab[1]
    e = _canonical(a, b, alpha, beta)
    lo, s = _grid(a, b)
    qa, ea = _pack(a, lo, s)
    qb, eb = _pack(b, lo, s)
    sad = np.abs(qa[:, None, :] - qb[None, :, :]).sum(axis=2)
    assert sad.max() < 2 ** 32
    with np.errstate(invalid="ignore", over="ignore"):
        m = s * sad.astype(np.float64)
        w = ((ea[:, None] + eb[None, :]) + 4.0 * U * m) * (1.0 + 1e-9) + 1e-280
        ok = (m + w) < (1e300 - abs(beta)) / abs(alpha)
        dlo, dhi = np.where(ok, m - w, np.nan), np.where(ok, m + w, np.nan)
    band = ~ok
    decided = wrong = 0
    for lists, by_row in ((rows, True), (cols, False)):
        for owner, items in enumerate(lists):
            lo_, hi_ = (dlo[owner], dhi[owner]) if by_row else (dlo[:, owner], dhi[:, owner])
            words = e[owner] if by_row else e[:, owner]
            for it in items:
                t = e[owner, it] if by_row else e[it, owner]
                if np.isnan(t):
                    below = np.zeros(words.shape, bool)
                    notbelow = ~np.isnan(lo_)                # never counted: every pair with an interval
                elif np.isinf(t):
                    below = ~np.isnan(lo_) if t > 0 else np.zeros(words.shape, bool)
                    notbelow = ~below & ~np.isnan(lo_)
                else:
                    t_lo, t_hi = _thresholds(np.float64(t), alpha, beta, d)
                    with np.errstate(invalid="ignore"):
                        below = (hi_ < t_lo) if alpha > 0 else (lo_ > t_hi)
                        notbelow = (lo_ > t_hi) if alpha > 0 else (hi_ < t_lo)
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
