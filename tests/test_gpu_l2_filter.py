"""K19 on the GPU: the count pass of the Euclidean measures (euclidean / l2 / l2_norm) through the fp16 MFMA filter.

The contract: the filter decides only comparisons that its rigorous bound (DESIGN s4, K19) puts out of reach of
every rounding, and re-scores the rest on the canonical fp64 chain -- so positions and ranks equal the fp64 route
(K18) WORD FOR WORD, ties, near-ties, NaN, inf, overflowing and underflowing rows included -- and it must actually
filter: a build that sends every pair to the re-score does not pass."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NA, NB = 300, 520


@pytest.fixture(scope="module")
def fx(golden):
    return golden("measures_retrieval")


def _both(a, b, alpha, beta, rows, cols, metric=None):
    import torch
    from cmve import _lib, engine
    metric = _lib.PW_L2 if metric is None else metric
    f = engine._PairwisePositions(a, b, metric, alpha, beta, torch.float64, rows, cols, filter=True)
    e = engine._PairwisePositions(a, b, metric, alpha, beta, torch.float64, rows, cols, filter=False)
    assert e.filter_stats is None
    return f, e


def _assert_same_words(f, e):
    for side in (0, 1):
        if e.lists[side] is None:
            assert f.positions(side) is None and f.ranks(side) is None
            continue
        assert f.pos[side].dtype == np.int64 and np.array_equal(f.pos[side], e.pos[side])
        assert np.array_equal(f.nan[side], e.nan[side])
        for x, y in zip(f.positions(side), e.positions(side)):
            assert np.array_equal(x, y)
        assert np.array_equal(f.ranks(side), e.ranks(side))


def _assert_accounted(st, pairs):
    assert st is not None
    if not st["fallback"]:
        assert st["overflow"] == 0
        assert st["decided"] + st["band"] == pairs and st["rescored"] == st["band"]


# ---- 1. reference parity -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", ["euclidean", "l2", "l2_norm"])
def test_reference_parity_under_the_filter(fx, m):
    from cmve import engine
    from cmve.linas import evaluation as E, metrics as M
    from cmve.linas.validate import cal_perf_embeddings
    vid, cap = fx["vid"], fx["cap"]
    v2t_gt, t2v_gt = M.get_gt(list(fx["video_ids"]), list(fx["caption_ids"]))
    c, v = E.measure_rows(cap, m), E.measure_rows(vid, m)
    metric, alpha, beta, _, sc_dt = E.measure_spec(m, v.shape[1])
    rr, cr = engine.pairwise_gt_ranks(c, v, metric, alpha, beta, sc_dt, M._lists(t2v_gt, len(cap)), v2t_gt,
                                      filter=True)
    assert np.array_equal(rr, fx["t2v_ranks_" + m]) and np.array_equal(cr, fx["v2t_ranks_" + m])
    v2t, t2v = cal_perf_embeddings(vid, cap, list(fx["video_ids"]), list(fx["caption_ids"]), measure=m, filter=True)
    ref = fx["cal_perf_" + m]
    np.testing.assert_allclose(np.array(v2t), ref[0], rtol=0, atol=1e-12)
    np.testing.assert_allclose(np.array(t2v), ref[1], rtol=0, atol=1e-12)


# ---- 2. word for word against the fp64 route -----------------------------------------------------------------------------

def _ulps(v, steps):
    for _ in range(steps):
        v = np.nextafter(v, v.dtype.type(np.inf))
    return v


def _adversarial(d, dt_a, dt_b):
    """Gaussian rows with planted GTs plus everything that can break a filter: exact duplicates 256 rows apart,
    a block of 1 / 2 / 4-ulp perturbations of one row, zero, huge, tiny, inf and NaN rows; lists with 0, 1, several
    and 20 items, repeated items, NaN items."""
    rng = np.random.default_rng(d)
    b = rng.standard_normal((NB, d))
    pick = rng.integers(0, 200, NA)
    pick[20] = 7
    a = b[pick] + 0.5 * rng.standard_normal((NA, d))
    with np.errstate(over="ignore"):
        a, b = a.astype(dt_a), b.astype(dt_b)
        b[256:296] = b[0:40]                       # exact ties under the strict <
        for t in range(40):                        # near-ties only the canonical chain can order
            row = b[7].copy()
            row[t % d] = _ulps(row[t % d], (1, 2, 4)[t % 3])
            b[300 + t] = row
        a[10], b[400] = 0.0, 0.0
        a[11], b[401] = 1e200, 1e200               # (+inf in float32)
        a[12], b[402] = 1e-200, 1e-200             # (zero in float32)
        a[13, 5 % d], b[403, 3] = np.inf, np.inf
        a[14, 0], b[404, 1] = np.nan, np.nan
    rows = [[int(p)] for p in pick]
    rows[20] = [7, 300, 301, 305, 320, 263, 339]   # the near-tie block and the duplicate of its centre
    rows[21] = []
    rows[22] = [5, 5]
    rows[23] = [404, 3, 404]                       # NaN items
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
    return a, b, rows, cols


@pytest.fixture(scope="module")
def adversarial():
    cache = {}

    def get(d, dt_a, dt_b):
        key = (d, dt_a, dt_b)
        if key not in cache:
            cache[key] = _adversarial(d, dt_a, dt_b)
        return cache[key]
    return get


@pytest.mark.parametrize("ab", [(1.0, 0.0), (None, -1.0), (1.0, -1.0), (None, 0.0)], ids=["l2", "l2_norm", "a1b-1", "a-1/Db0"])
@pytest.mark.parametrize("dts", [(np.float32, np.float32), (np.float64, np.float64), (np.float32, np.float64)],
                         ids=["f32", "f64", "mixed"])
@pytest.mark.parametrize("d", [67, 1024])
def test_words_equal_the_fp64_route(adversarial, d, dts, ab):
    a, b, rows, cols = adversarial(d, *dts)
    alpha = -1.0 / d if ab[0] is None else ab[0]
    f, e = _both(a, b, alpha, ab[1], rows, cols)
    _assert_same_words(f, e)
    _assert_accounted(f.filter_stats, NA * NB)
    assert not f.filter_stats["fallback"] and 0 < f.filter_stats["band"] < NA * NB // 8


def test_one_direction_and_empty_sides(adversarial):
    from cmve import engine
    a, b, rows, cols = adversarial(67, np.float64, np.float64)
    for r, c in ((rows, None), (None, cols)):
        f, e = _both(a, b, 1.0, 0.0, r, c)
        _assert_same_words(f, e)
    for aa, bb, r, c in ((a[:0], b, [], [[] for _ in range(NB)]), (a, b[:0], [[] for _ in range(NA)], [])):
        f, e = _both(aa, bb, -1.0 / 67, -1.0, r, c)
        _assert_same_words(f, e)
    # items naming rows when the other side is empty keep cmve_pairwise_positions' words as well
    f, e = _both(a[:5], b[:0], 1.0, 0.0, [[], [], [], [], []], [])
    _assert_same_words(f, e)


# ---- 3. clustered rows far from the origin ---------------------------------------------------------------------------------

def test_clustered_rows_fall_back_and_say_so():
    rng = np.random.default_rng(3)
    na, nb, d = 256, 384, 256
    b = 100.0 + rng.standard_normal((nb, d))
    a = 100.0 + rng.standard_normal((na, d))
    rows = [[int(j)] for j in rng.integers(0, nb, na)]
    cols = [[int(i)] for i in rng.integers(0, na, nb)]
    f, e = _both(a, b, 1.0, 0.0, rows, cols)
    _assert_same_words(f, e)
    st = f.filter_stats
    assert st is not None and (st["redone"] or st["fallback"])
    if st["fallback"]:
        assert st["overflow"] == 1 and st["band"] * 8 > na * nb
    else:
        _assert_accounted(st, na * nb)


# ---- 4. the filter actually filters ----------------------------------------------------------------------------------------

def test_filter_decides_almost_every_pair():
    rng = np.random.default_rng(0)
    na, nb, d = 512, 2048, 1024
    a = rng.standard_normal((na, d))
    b = rng.standard_normal((nb, d))
    rows = [[int(j)] for j in rng.integers(0, nb, na)]
    f, e = _both(a, b, 1.0, 0.0, rows, None)
    _assert_same_words(f, e)
    st = f.filter_stats
    print("random item: decided %d of %d (%.2f%%), band %d" % (st["decided"], na * nb, 100.0 * st["decided"] / (na * nb),
                                                                st["band"]))
    assert st["decided"] + st["band"] == na * nb and st["rescored"] == st["band"] and not st["fallback"]
    assert st["decided"] >= 0.90 * na * nb
    # planted GTs: the band is little more than the GT pairs
    a = b[:na] + 0.5 * rng.standard_normal((na, d))
    rows = [[i] for i in range(na)]
    cols = [[j] if j < na else [] for j in range(nb)]
    f, e = _both(a, b, 1.0, 0.0, rows, cols)
    _assert_same_words(f, e)
    st = f.filter_stats
    print("planted GTs: decided %d of %d (%.3f%%), band %d" % (st["decided"], na * nb,
                                                                100.0 * st["decided"] / (na * nb), st["band"]))
    assert st["decided"] + st["band"] == na * nb and st["rescored"] == st["band"] and not st["fallback"]
    assert st["decided"] >= 0.99 * na * nb


# ---- 5. auto dispatch ------------------------------------------------------------------------------------------------------

def test_auto_dispatch_follows_the_crossover():
    import torch
    from cmve import _lib, engine
    rng = np.random.default_rng(5)
    na, d = 512, 64
    nb_at = -(-engine.L2_FILTER_MIN_PAIRS // na)
    b_all = rng.standard_normal((nb_at, d))
    a = b_all[:na] + 0.5 * rng.standard_normal((na, d))
    rows = [[i] for i in range(na)]
    for nb, taken in ((nb_at - 1, False), (nb_at, True)):
        assert (na * nb >= engine.L2_FILTER_MIN_PAIRS) == taken
        b = b_all[:nb]
        cols = [[j] if j < na else [] for j in range(nb)]
        auto = engine._PairwisePositions(a, b, _lib.PW_L2, 1.0, 0.0, torch.float64, rows, cols)
        assert (auto.filter_stats is not None) == taken
        f, e = _both(a, b, 1.0, 0.0, rows, cols)
        _assert_same_words(auto, e)
        _assert_same_words(f, e)
        # l1, and fp32 score words, never take the filter
        assert engine._PairwisePositions(a, b, _lib.PW_L1, 1.0, 0.0, torch.float64, rows, cols).filter_stats is None
        assert engine._PairwisePositions(a, b, _lib.PW_L2, 1.0, 0.0, torch.float32, rows, cols).filter_stats is None


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing():
    import torch
    from cmve import _lib, engine
    rng = np.random.default_rng(6)
    a, b = rng.standard_normal((40, 67)), rng.standard_normal((50, 67))
    ra, rb = engine.RowSet(a, with_lo=False), engine.RowSet(b, with_lo=False)
    dev = ra.device
    rows = [[i] for i in range(40)]
    off, idx = engine.csr(rows, dev)
    sc = torch.zeros(40, dtype=torch.float64, device=dev)
    ws = torch.empty(1024, dtype=torch.int64, device=dev)

    def call(x, y, alpha, beta=0.0):
        pos = torch.full((40,), 77, dtype=torch.int32, device=dev)
        stats = torch.full((4,), 77, dtype=torch.int64, device=dev)
        rc = _lib.lib.cmve_l2_count(engine.handle(dev), C.byref(x.desc), C.byref(y.desc), alpha, beta,
                                    engine._ptr(off), engine._ptr(sc), 40, y.n, engine._ptr(pos), None, None, 0, x.n,
                                    None, engine._ptr(ws), 8 * 1024, engine._ptr(stats))
        msg = _lib.lib.cmve_last_error()
        torch.cuda.synchronize()
        untouched = bool((pos == 77).all()) and bool((stats == 77).all())
        return rc, msg, untouched

    rc, msg, untouched = call(ra, rb, 1.0)
    assert rc == 0 and not untouched                      # the accepted call, for contrast
    for alpha, beta in ((0.0, 0.0), (float("nan"), 0.0), (float("inf"), 0.0), (1.0, float("inf"))):
        rc, msg, untouched = call(ra, rb, alpha, beta)
        assert rc < 0 and b"cmve_l2_count" in msg and b"alpha" in msg and untouched
    rc, msg, untouched = call(ra, engine.RowSet(b, with_lo=False, with_f16=False), 1.0)
    assert rc < 0 and b"cmve_l2_count" in msg and b"fp16 plane" in msg and untouched
    rc, msg, untouched = call(ra, engine.RowSet(b[:, :66], with_lo=False), 1.0)
    assert rc < 0 and b"cmve_l2_count" in msg and b"dimensions differ" in msg and untouched
    rc, msg, untouched = call(ra, engine.RowSet(b, eps=1e-12, with_lo=False), 1.0)
    assert rc < 0 and b"eps" in msg and untouched
    rc, msg, untouched = call(ra, engine.RowSet(b, with_lo=False, raw_rows=True), 1.0)
    assert rc < 0 and b"CMVE_PACK_RAW" in msg and untouched
    # the Python route refuses what the entry cannot express: fp32 score words, another metric
    with pytest.raises(ValueError, match="float64 score words"):
        engine.pairwise_gt_ranks(a, b, _lib.PW_L2, 1.0, 0.0, torch.float32, rows, None, filter=True)
    with pytest.raises(ValueError, match="PW_L2"):
        engine.pairwise_gt_ranks(a, b, _lib.PW_L1, 1.0, 0.0, torch.float64, rows, None, filter=True)
    with pytest.raises(_lib.CmveError, match="alpha"):
        engine.pairwise_gt_ranks(a, b, _lib.PW_L2, 0.0, 0.0, torch.float64, rows, None, filter=True)


# ---- the four count entries share one check of the lists (flt_check_lists) ------------------------------------------------

def test_the_four_count_entries_refuse_bad_lists_alike():
    """cmve_pairwise_count, cmve_l2_count, cmve_l2_count_resolved and cmve_l1_count on 4 x 4 rows of d = 4: the same
    bad lists get the same code and, past the entry's name, the same words.  Every refusal precedes the first
    launch."""
    import torch
    from cmve import _lib, engine
    lib = _lib.lib
    rng = np.random.default_rng(4)
    a, b = engine.to_device(rng.standard_normal((4, 4))), engine.to_device(rng.standard_normal((4, 4)))
    dev = a.device
    h = engine.handle(dev)
    ra, rb = engine.RowSet(a, with_lo=False, device=dev), engine.RowSet(b, with_lo=False, device=dev)
    sa = engine.L1Set(a)
    sb = engine.L1Set(b, grid=sa.grid)
    off = torch.arange(5, dtype=torch.int64, device=dev)
    sc = torch.zeros(4, dtype=torch.float64, device=dev)
    pos = torch.zeros(4, dtype=torch.int32, device=dev)
    ws = torch.empty(64, dtype=torch.int64, device=dev)
    stats = torch.zeros(4, dtype=torch.int64, device=dev)
    p = engine._ptr
    raw = lambda x: (p(x), _lib.CMVE_F64, 4, 4)
    tail = (p(ws), 8 * 64, p(stats))
    entries = {
        "cmve_pairwise_count": lambda l: lib.cmve_pairwise_count(h, *raw(a), *raw(b), 4, _lib.PW_L2, 1.0, 0.0,
                                                                 _lib.CMVE_F64, *l),
        "cmve_l2_count": lambda l: lib.cmve_l2_count(h, C.byref(ra.desc), C.byref(rb.desc), 1.0, 0.0, *l, *tail),
        "cmve_l2_count_resolved": lambda l: lib.cmve_l2_count_resolved(h, C.byref(ra.desc), C.byref(rb.desc), 1.0, 0.0,
                                                                       *l, *tail),
        "cmve_l1_count": lambda l: lib.cmve_l1_count(h, *raw(a), p(sa.codes), p(sa.err), *raw(b), p(sb.codes),
                                                     p(sb.err), 4, p(sa.grid), 1.0, 0.0, *l, *tail),
    }
    good_row, no_col = (p(off), p(sc), 4, 4, p(pos)), (None, None, 0, 0, None)
    bad = {
        "negative row_items": (p(off), p(sc), -1, 4, p(pos)) + no_col,
        "row_n = 2^31": (p(off), p(sc), 4, 1 << 31, p(pos)) + no_col,
        "row_pos without row_off": (None, p(sc), 4, 4, p(pos)) + no_col,
        "col_pos without col_sc": good_row + (p(off), None, 4, 4, p(pos)),
    }
    for what, lists in bad.items():
        seen = set()
        for name, call in entries.items():
            rc = call(lists)
            msg = lib.cmve_last_error()
            assert rc < 0 and msg.startswith(name.encode() + b": "), (what, name, rc, msg)
            seen.add((rc, msg[len(name):]))
        assert len(seen) == 1, (what, seen)
    assert {m for _, m in seen} == {b": column lists missing"}
    torch.cuda.synchronize()
    assert not bool(stats.any()) and not bool(pos.any())  # nothing ran
