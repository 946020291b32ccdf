"""K24 on the GPU: the count pass under jaccard (float32 score words) through the integer SAD filter.

The contract: the filter decides only comparisons that its rigorous bound (DESIGN s4, K24) puts out of reach of
every rounding -- the float32 one included -- and re-scores the rest on the canonical two-accumulator chain, so
positions and ranks equal the K18 route WORD FOR WORD, ties, near-ties, NaN words (a zero sum of maxima), inf and huge
rows included, whether or not the band list held the band -- and it must actually filter: a build that sends every
pair to the re-score does not pass."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NA, NB = 300, 520
AB = [(-1.0, 0.0), (1.0, 0.0), (-0.5, 0.25)]
AB_IDS = ["a-1b0", "a1b0", "a-.5b.25"]
DTS = [(np.float32, np.float32), (np.float64, np.float64), (np.float32, np.float64)]
DTS_IDS = ["f32", "f64", "mixed"]


@pytest.fixture(scope="module")
def fx(golden):
    return golden("measures_retrieval")


def _both(a, b, alpha, beta, rows, cols, flt="jaccard"):
    import torch
    from cmve import _lib, engine
    f = engine._PairwisePositions(a, b, _lib.PW_JACCARD, alpha, beta, torch.float32, rows, cols, filter=flt)
    e = engine._PairwisePositions(a, b, _lib.PW_JACCARD, alpha, beta, torch.float32, rows, cols, filter=False)
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
    assert st is not None and st["redone"] is False and st["fallback"] is False
    assert st["overflow"] == 0
    assert st["decided"] + st["band"] == pairs and st["rescored"] == st["band"]


# ---- 1. reference parity -----------------------------------------------------------------------------------------------

def test_reference_parity_under_the_filter(fx):
    from cmve import engine
    from cmve.linas import evaluation as E, metrics as M
    from cmve.linas.validate import cal_perf_embeddings
    vid, cap = fx["vid_p"], fx["cap_p"]
    v2t_gt, t2v_gt = M.get_gt(list(fx["video_ids"]), list(fx["caption_ids"]))
    c, v = E.measure_rows(cap, "jaccard"), E.measure_rows(vid, "jaccard")
    metric, alpha, beta, _, sc_dt = E.measure_spec("jaccard", v.shape[1])
    rr, cr = engine.pairwise_gt_ranks(c, v, metric, alpha, beta, sc_dt, M._lists(t2v_gt, len(cap)), v2t_gt,
                                      filter="jaccard")
    assert np.array_equal(rr, fx["t2v_ranks_jaccard"]) and np.array_equal(cr, fx["v2t_ranks_jaccard"])
    v2t, t2v = cal_perf_embeddings(vid, cap, list(fx["video_ids"]), list(fx["caption_ids"]), measure="jaccard",
                                   filter="jaccard")
    ref = fx["cal_perf_jaccard"]
    np.testing.assert_allclose(np.array(v2t), ref[0], rtol=0, atol=1e-12)
    np.testing.assert_allclose(np.array(t2v), ref[1], rtol=0, atol=1e-12)


# ---- 2. word for word against the K18 route --------------------------------------------------------------------------------

def _ulps(v, steps):
    for _ in range(steps):
        v = np.nextafter(v, v.dtype.type(np.inf))
    return v


def _adversarial(d, dt_a, dt_b, nonneg):
    """The recipe of tests/test_gpu_l1_filter.py (``nonneg``: on np.abs of the Gaussian rows): planted GTs plus exact
    duplicates 256 rows apart, a block of 1 / 2 / 4-ulp perturbations of one row, zero (a NaN word against one
    another: the sum of maxima is 0), huge, tiny, inf and NaN rows; lists with 0, 1, several and 20 items, repeated
    items, NaN items."""
    rng = np.random.default_rng(d)
    b = rng.standard_normal((NB, d))
    pick = rng.integers(0, 200, NA)
    pick[20] = 7
    a = b[pick] + 0.5 * rng.standard_normal((NA, d))
    if nonneg:
        a, b = np.abs(a), np.abs(b)
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
    rows[10], rows[11], rows[12], rows[13], rows[14] = [1, 400], [2, 401], [3, 402], [4], [6, 404]
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

    def get(d, dt_a, dt_b, nonneg=True):
        key = (d, dt_a, dt_b, nonneg)
        if key not in cache:
            cache[key] = _adversarial(d, dt_a, dt_b, nonneg)
        return cache[key]
    return get


@pytest.mark.parametrize("ab", AB, ids=AB_IDS)
@pytest.mark.parametrize("dts", DTS, ids=DTS_IDS)
@pytest.mark.parametrize("d", [67, 1024])
@pytest.mark.parametrize("nonneg", [True, False], ids=["nonneg", "signed"])
def test_words_equal_the_k18_route(adversarial, nonneg, d, dts, ab):
    a, b, rows, cols = adversarial(d, *dts, nonneg)
    f, e = _both(a, b, ab[0], ab[1], rows, cols)
    _assert_same_words(f, e)
    st = f.filter_stats
    print("d %d: decided %d, band %d (%.2f%%)" % (d, st["decided"], st["band"], 100.0 * st["band"] / (NA * NB)))
    _assert_accounted(st, NA * NB)
    assert 0 < st["band"] < NA * NB // 8            # the filter must actually filter


def test_the_zero_rows_give_a_nan_word_on_both_routes(adversarial):
    a, b, rows, cols = adversarial(67, np.float32, np.float32, True)
    f, e = _both(a, b, -1.0, 0.0, [[400] if i == 10 else [] for i in range(NA)],
                 [[10] if j == 400 else [] for j in range(NB)])
    _assert_same_words(f, e)
    assert e.nan[0].tolist() == [True] and f.nan[0].tolist() == [True]
    assert e.nan[1].tolist() == [True] and f.nan[1].tolist() == [True]
    assert f.ranks(0)[10] == NB and f.ranks(1)[400] == NA       # a list whose items all score NaN ranks n


# ---- 3. float32 ties on purpose ------------------------------------------------------------------------------------------

def test_float32_ties_are_not_counted():
    """Gallery rows 1 .. 12 differ from row 0 by 1 - 4 fp64 ulps of one element: their fp64 chains differ, their float32
    words against any caption are EQUAL.  Listed as items of every caption, the strict < counts none of them against
    another: all thirteen get one position, exactly as on K18."""
    rng = np.random.default_rng(24)
    na, nb, d = 140, 150, 64
    a = np.abs(rng.standard_normal((na, d))).astype(np.float32).astype(np.float64)
    b = np.abs(rng.standard_normal((nb, d))).astype(np.float32).astype(np.float64)
    for t in range(1, 13):
        row = b[0].copy()
        row[(5 * t) % d] = _ulps(row[(5 * t) % d], 1 + t % 4)
        b[t] = row
    assert len({b[t].tobytes() for t in range(13)}) == 13
    tied = list(range(13))
    rows = [tied + [20 + i % 100] for i in range(na)]
    cols = [[j % na, (j + 7) % na] for j in range(nb)]
    for alpha, beta in AB:
        f, e = _both(a, b, alpha, beta, rows, cols)
        _assert_same_words(f, e)
        _assert_accounted(f.filter_stats, na * nb)
        for p in f.positions(0):
            assert len(set(p[:13].tolist())) == 1


# ---- 4. extremes -----------------------------------------------------------------------------------------------------------

def test_extreme_codes_clamped_rows_and_signs():
    import torch
    from cmve import _lib, engine
    rng = np.random.default_rng(24)
    na, nb, d = 140, 150, 1024
    a, b = rng.uniform(0.0, 1.0, (na, d)), rng.uniform(0.0, 1.0, (nb, d))
    a[0], b[0] = 0.0, 3.0             # all-lo against all-hi: the SAD is 65535 * 1024 > 2^24
    a[1], b[1] = 3.0, 0.0
    rows = [[int(j)] for j in rng.integers(0, nb, na)]
    rows[0], rows[1], rows[2] = [0, 1, 5], [1, 0], [0, 1]
    cols = [[int(i)] for i in rng.integers(0, na, nb)]
    cols[0], cols[1] = [0, 1, 7], [1, 0]
    for alpha, beta in ((-1.0, 0.0), (1.0, 0.0)):
        f, e = _both(a, b, alpha, beta, rows, cols)
        _assert_same_words(f, e)
        _assert_accounted(f.filter_stats, na * nb)
    # a caption far outside the grid of a resident gallery clamps: its error is large, its words are the same
    P = _Problem(a, b, rows, cols, -1.0, 0.0)
    g = engine.JaccardSet(P.b)
    base = _stats(P.count(P.side(0, nb), P.side(1, na), b=g, filter="jaccard", return_stats=True)[2])
    far = P.a.clone()
    far[3] = 50.0
    far[4, ::2] = 1e6
    Q = _Problem(far, P.b, rows, cols, -1.0, 0.0)
    row, col = Q.side(0, nb), Q.side(1, na)
    e_r, e_c = Q.count(row, col, filter=False)
    f_r, f_c, st = Q.count(row, col, b=g, filter="jaccard", return_stats=True)
    assert _same(f_r, e_r) and _same(f_c, e_c)
    s = _stats(st)
    assert s["overflow"] == 0 and s["decided"] + s["band"] == na * nb and s["rescored"] == s["band"]
    assert s["band"] >= base["band"]                                 # only the band grows
    # d = 1
    a1, b1 = np.abs(rng.standard_normal((37, 1))), np.abs(rng.standard_normal((41, 1)))
    b1[5] = a1[3]
    f, e = _both(a1, b1, -1.0, 0.0, [[int(j)] for j in rng.integers(0, 41, 37)], [[3, 0] for _ in range(41)])
    _assert_same_words(f, e)
    _assert_accounted(f.filter_stats, 37 * 41)
    # a negative sum of maxima (all-negative rows) and one that is exactly zero: no interval, the canonical words
    an, bn = rng.standard_normal((40, 8)), rng.standard_normal((50, 8))
    an[0], bn[0] = -np.abs(an[0]) - 0.1, -np.abs(bn[0]) - 0.1
    an[1], bn[1] = [1.0, -1.0, 0.5, -0.5, 0.0, 0.0, 0.0, 0.0], [-1.0, -1.0, -0.5, -0.5, -2.0, 0.0, -3.0, 0.0]
    assert np.maximum(an[0], bn[0]).sum() < 0 and np.maximum(an[1], bn[1]).sum() == 0.0
    rows40 = [[i % 50] for i in range(40)]
    rows40[0], rows40[1], rows40[2] = [0, 1], [1, 0, 2], [0, 1]
    cols50 = [[0, 1, j % 40] for j in range(50)]
    for alpha, beta in AB:
        f, e = _both(an, bn, alpha, beta, rows40, cols50)
        _assert_same_words(f, e)
        _assert_accounted(f.filter_stats, 40 * 50)
        assert f.filter_stats["band"] >= 2


# ---- 5. an overflowing band list is resolved on the device -------------------------------------------------------------------

class _Problem:
    """Rows on the device and both CSR sides with their float32 item words from pairwise_item_scores (computed
    once)."""

    def __init__(self, a, b, rows, cols, alpha, beta):
        import torch
        from cmve import _lib, engine
        self.a, self.b = engine.to_device(a), engine.to_device(b)
        self.alpha, self.beta = alpha, beta
        self.pairs = self.a.shape[0] * self.b.shape[0]
        dev = self.a.device
        self.sides = []
        for lists, col_dir in ((rows, False), (cols, True)):
            off, idx = engine.csr(lists, dev)
            items = sum(len(l) for l in lists)
            sc = engine.pairwise_item_scores(self.a, self.b, _lib.PW_JACCARD, alpha, beta, torch.float32, off, idx,
                                             items, col_dir, 0)
            self.sides.append((off, sc.contiguous()))

    def side(self, which, n):
        off, sc = self.sides[which]
        return (off, sc, n)

    def count(self, row, col, a=None, b=None, **kw):
        import torch
        from cmve import _lib, engine
        return engine.pairwise_count(self.a if a is None else a, self.b if b is None else b, _lib.PW_JACCARD,
                                     self.alpha, self.beta, torch.float32, row=row, col=col, **kw)


def _same(x, y):
    import torch
    if x is None or y is None:
        return x is None and y is None
    return x.dtype == torch.int32 and torch.equal(x, y)


def _stats(t):
    decided, band, rescored, overflow = (int(v) for v in t.cpu().numpy())
    return {"decided": decided, "band": band, "rescored": rescored, "overflow": overflow}


@pytest.mark.parametrize("d", [67, 1024])
def test_overflow_is_resolved_on_the_device(adversarial, monkeypatch, d):
    import torch
    P = _Problem(*adversarial(d, np.float32, np.float64), -1.0, 0.0)
    dev = P.a.device
    row, col = P.side(0, NB), P.side(1, NA)
    e_r, e_c = P.count(row, col, filter=False)
    full = _stats(P.count(row, col, filter="jaccard", return_stats=True)[2])
    assert full["overflow"] == 0 and full["rescored"] == full["band"] > 1
    for cap in (0, 1):
        f_r, f_c, st = P.count(row, col, filter="jaccard", band=torch.empty(cap, dtype=torch.int64, device=dev),
                               return_stats=True)
        assert _same(f_r, e_r) and _same(f_c, e_c)
        small = _stats(st)
        assert small["overflow"] == 1 and small["rescored"] == 0
        assert small["band"] == full["band"] and small["decided"] == full["decided"]   # band reports the whole need
    # one direction at a time, and the shard form (n = 0: the NaN items' words stay 0)
    band = torch.empty(1, dtype=torch.int64, device=dev)
    for row_, col_ in ((P.side(0, NB), None), (None, P.side(1, NA)), (P.side(0, 0), P.side(1, 0))):
        e_ = P.count(row_, col_, filter=False)
        f_r, f_c, st = P.count(row_, col_, filter="jaccard", band=band, return_stats=True)
        assert _same(f_r, e_[0]) and _same(f_c, e_[1]) and _stats(st)["overflow"] == 1
    # the positions route says that the canonical count ran
    from cmve import engine
    monkeypatch.setattr(engine, "l2_band_cap", lambda pairs: 1)
    a, b, rows, cols = adversarial(d, np.float32, np.float64)
    f, e = _both(a, b, -1.0, 0.0, rows, cols)
    _assert_same_words(f, e)
    assert f.filter_stats["fallback"] is True and f.filter_stats["overflow"] == 1 and not f.filter_stats["redone"]


# ---- 6. a resident side -----------------------------------------------------------------------------------------------------

def test_resident_gallery_over_two_batches(adversarial, monkeypatch):
    import torch
    from cmve import engine
    a, b, rows, cols = adversarial(67, np.float32, np.float32)
    calls = {"cmve_l1_pack": 0, "cmve_jaccard_rowsums": 0, "cmve_l1_grid": 0}
    for name in calls:
        def wrap(*args, _f=getattr(engine.lib, name), _n=name):
            calls[_n] += 1
            return _f(*args)
        monkeypatch.setattr(engine.lib, name, wrap, raising=False)
    g = engine.JaccardSet(b)
    assert isinstance(g, engine.L1Set) and g.qsum.dtype == torch.int64 and g.asum.dtype == torch.float64
    assert calls == {"cmve_l1_pack": 1, "cmve_jaccard_rowsums": 1, "cmve_l1_grid": 1}
    # the exact code sums are the stored codes'; S bounds sum |x| and is +inf exactly where err is
    codes = g.codes.view(torch.int16).cpu().numpy().view(np.uint16).astype(np.int64)
    assert codes.sum() == int(g.qsum[:NB].sum())
    bd = b.astype(np.float64)
    asum, err = g.asum[:NB].cpu().numpy(), g.err[:NB].cpu().numpy()
    assert np.array_equal(np.isinf(asum), np.isinf(err)) and np.isinf(asum).sum() == 3
    fin = ~np.isinf(asum)
    mag = np.abs(bd[fin]).sum(axis=1)
    assert (asum[fin] >= mag).all() and (asum[fin] <= mag * 1.000001 + 1e-299).all()
    lo, hi = (float(v) for v in g.grid.cpu())
    # two caption batches against the one packed gallery: plain rows (packed on the gallery's grid inside the call),
    # then a JaccardSet the caller packed
    for sl in (slice(0, 160), slice(160, NA)):
        aa, rr = a[sl], rows[sl]
        cc = [[i - sl.start for i in c if sl.start <= i < sl.stop] for c in cols]
        P = _Problem(aa, b, rr, cc, -1.0, 0.0)
        row, col = P.side(0, NB), P.side(1, aa.shape[0])
        e_r, e_c = P.count(row, col, filter=False)
        before = dict(calls)
        f_r, f_c, st1 = P.count(row, col, b=g, filter="jaccard", return_stats=True)
        assert _same(f_r, e_r) and _same(f_c, e_c)
        assert calls["cmve_l1_pack"] == before["cmve_l1_pack"] + 1                 # the captions alone
        assert calls["cmve_jaccard_rowsums"] == before["cmve_jaccard_rowsums"] + 1
        assert calls["cmve_l1_grid"] == before["cmve_l1_grid"]                     # the gallery's grid serves
        caps = engine.JaccardSet(P.a, grid=g.grid)
        assert caps.grid.data_ptr() == g.grid.data_ptr()
        before = dict(calls)
        f_r, f_c, st2 = P.count(row, col, a=caps, b=g, filter="jaccard", return_stats=True)
        assert calls == before                                                      # nothing packed again
        assert _same(f_r, e_r) and _same(f_c, e_c) and torch.equal(st1, st2)
        s = _stats(st2)
        assert s["overflow"] == 0 and s["decided"] + s["band"] == P.pairs and s["rescored"] == s["band"]
    assert (float(g.grid[0]), float(g.grid[1])) == (lo, hi)          # packing on a grid does not move it
    # a JaccardSet is the K18 route's operand through its raw rows; an L1Set holds no row sums; sets on different
    # grids are refused
    z = P.count(row, col, b=g, filter=False, return_stats=True)
    assert _same(z[0], e_r) and _same(z[1], e_c) and z[2] is None
    with pytest.raises(TypeError, match="JaccardSet"):
        P.count(row, None, b=engine.L1Set(P.b), filter="jaccard")
    with pytest.raises(ValueError, match="different grids"):
        P.count(row, None, a=engine.JaccardSet(P.a), b=g, filter="jaccard")


# ---- 7. degenerate -----------------------------------------------------------------------------------------------------------

def test_degenerate_shapes_and_grids(adversarial):
    import torch
    from cmve import engine
    a, b, rows, cols = adversarial(67, np.float64, np.float64)
    for r, c in ((rows, None), (None, cols)):
        f, e = _both(a, b, -1.0, 0.0, r, c)
        _assert_same_words(f, e)
        _assert_accounted(f.filter_stats, NA * NB)
    for aa, bb, r, c in ((a[:0], b, [], [[] for _ in range(NB)]), (a, b[:0], [[] for _ in range(NA)], []),
                         (a[:5], b[:0], [[], [], [], [], []], [])):
        f, e = _both(aa, bb, -1.0, 0.0, r, c)
        _assert_same_words(f, e)
    # empty lists everywhere: nothing to count, nothing launched
    f, e = _both(a, b, -1.0, 0.0, [[] for _ in range(NA)], [[] for _ in range(NB)])
    _assert_same_words(f, e)
    # empty sides through pairwise_count: the NaN items still get the caller's n
    P = _Problem(a, b, rows, cols, -1.0, 0.0)
    dev = P.a.device
    nan = float("nan")
    coff = torch.tensor([0, 2, 3] + [3] * (NB - 2), dtype=torch.int64, device=dev)
    csc = torch.tensor([nan, 1.0, nan], dtype=torch.float64, device=dev)
    roff0 = torch.zeros(1, dtype=torch.int64, device=dev)
    none_sc = torch.empty(0, dtype=torch.float64, device=dev)
    for cn in (7, 0):
        row, col = (roff0, none_sc, NB), (coff, csc, cn)
        e_ = P.count(row, col, a=P.a[:0], filter=False)
        f_r, f_c, st = P.count(row, col, a=P.a[:0], filter="jaccard", return_stats=True)
        assert _same(f_r, e_[0]) and _same(f_c, e_[1]) and _stats(st) == dict(decided=0, band=0, rescored=0, overflow=0)
        if cn:
            assert f_c.tolist() == [cn - 1, 0, cn - 1]
    # a grid from constant rows (hi == lo): lo = 0, s = 1 -- every row of the other set is far off it
    const = np.full((40, 67), 0.25)
    g = engine.JaccardSet(const)
    assert float(g.grid[0]) == float(g.grid[1]) == 0.25
    rows40 = [[i % NB] for i in range(40)]
    cols40 = [[j % 40] for j in range(NB)]
    Pc = _Problem(const, b, rows40, cols40, -1.0, 0.0)
    row, col = Pc.side(0, NB), Pc.side(1, 40)
    e_r, e_c = Pc.count(row, col, filter=False)
    f_r, f_c, st = Pc.count(row, col, a=g, filter="jaccard", return_stats=True)
    assert _same(f_r, e_r) and _same(f_c, e_c)
    s = _stats(st)
    assert s["decided"] + s["band"] == 40 * NB
    # constant rows on both sides: every word is exactly -1, every comparison a tie
    f, e = _both(const, const[:33], -1.0, 0.0, [[i % 33] for i in range(40)], [[j] for j in range(33)])
    _assert_same_words(f, e)
    # no eligible element at all: the empty grid
    allnan = np.full((3, 67), np.nan)
    gn = engine.JaccardSet(allnan)
    assert float(gn.grid[0]) == float("inf") and float(gn.grid[1]) == float("-inf")
    f, e = _both(allnan, b[:9], -1.0, 0.0, [[0], [1], [2]], [[0] for _ in range(9)])
    _assert_same_words(f, e)


def test_a_tile_with_no_list_in_it():
    """130 x 130 x 33 with lists only on rows < 128: the two tiles of rows 128 and 129 hold no list at all, so the
    epilogue has nothing to decide there -- but row 129 holds a NaN, its pairs have no interval, and every one of them must still
    reach the band list so that decided + band = pairs."""
    n, d = 130, 33
    rng = np.random.default_rng(24)
    a, b = np.abs(rng.standard_normal((n, d))), np.abs(rng.standard_normal((n, d)))
    a[129, 5] = np.nan
    rows = [[i % 128] if i < 128 else [] for i in range(n)]
    f, e = _both(a, b, -1.0, 0.0, rows, None)
    _assert_same_words(f, e)
    st = f.filter_stats
    assert st is not None and st["decided"] + st["band"] == n * n
    assert st["band"] >= n
    assert st["rescored"] == st["band"] and st["overflow"] == 0


# ---- 7b. the seams of the one count body (sad_count.h) ---------------------------------------------------------------------

def _seams():
    """129 x 257 x 33: 2 x 3 tiles whose last row tile and last column tile hold ONE row, d no multiple of the
    32-element K tile (two K tiles).  Row lists of 0, 1, 3 and 5 items side by side in a tile (the tile's rounds exceed
    most lists' lengths); the only column list is that of row 256, the one row of the last column tile, and names row
    128, the one row of the last row tile.  Ten exact duplicates and a NaN row put pairs into the band."""
    na, nb, d = 129, 257, 33
    rng = np.random.default_rng(na * nb)
    b = rng.standard_normal((nb, d))
    pick = rng.integers(0, nb, na)
    a = b[pick] + 0.5 * rng.standard_normal((na, d))
    a, b = np.abs(a), np.abs(b)
    b[130:140] = b[0:10]
    a[5, 3] = np.nan
    rows = [([int(pick[i])] + list(map(int, rng.integers(0, nb, 4))))[:(0, 1, 3, 5)[i % 4]] for i in range(na)]
    rows[128] = [int(pick[128]), 256, 0, 130, 256]
    cols = [[] for _ in range(nb)]
    cols[256] = [128, 3, 128, 7, 0]
    return a, b, rows, cols


@pytest.fixture(scope="module")
def seams():
    return _seams()


@pytest.mark.parametrize("alpha", [1.0, -1.0], ids=["a1", "a-1"])
@pytest.mark.parametrize("lists", ["both", "no_rows", "no_cols"])
def test_seams_of_the_one_count_body(seams, lists, alpha):
    a, b, rows, cols = seams
    pairs = a.shape[0] * b.shape[0]
    f, e = _both(a, b, alpha, 0.0, None if lists == "no_rows" else rows, None if lists == "no_cols" else cols)
    _assert_same_words(f, e)
    st = f.filter_stats
    print("%s: decided %d, band %d (%.2f%%)" % (lists, st["decided"], st["band"], 100.0 * st["band"] / pairs))
    _assert_accounted(st, pairs)                    # decided + band == 129 * 257, rescored == band, overflow == 0
    assert pairs == 129 * 257 and 0 < st["band"] < pairs // 8


# ---- 8. dispatch -------------------------------------------------------------------------------------------------------------

def test_dispatch(adversarial, monkeypatch):
    import torch
    from cmve import _lib, engine
    a, b, rows, cols = adversarial(67, np.float32, np.float32)
    J, f32 = _lib.PW_JACCARD, torch.float32
    with pytest.raises(ValueError, match='filter="jaccard"'):
        engine.pairwise_gt_ranks(a, b, _lib.PW_L1, 1.0, 0.0, torch.float64, rows, None, filter="jaccard")
    with pytest.raises(ValueError, match="float32 score words"):
        engine.pairwise_gt_ranks(a, b, J, -1.0, 0.0, torch.float64, rows, None, filter="jaccard")
    with pytest.raises(ValueError, match="alpha"):
        engine.pairwise_gt_ranks(a, b, J, 0.0, 0.0, f32, rows, None, filter="jaccard")
    # the other forced routes still refuse jaccard
    with pytest.raises(ValueError, match="PW_L1"):
        engine.pairwise_gt_ranks(a, b, J, -1.0, 0.0, f32, rows, None, filter="l1")
    with pytest.raises(ValueError, match="PW_L2"):
        engine.pairwise_gt_ranks(a, b, J, -1.0, 0.0, f32, rows, None, filter=True)
    with pytest.raises(ValueError, match="PW_L2"):
        engine.pairwise_count(a, b, J, -1.0, 0.0, f32, filter=True)
    e = engine._PairwisePositions(a, b, J, -1.0, 0.0, f32, rows, cols, filter=False)
    # auto: never while the threshold is None ...
    monkeypatch.setattr(engine, "JACCARD_FILTER_MIN_PAIRS", None)
    auto = engine._PairwisePositions(a, b, J, -1.0, 0.0, f32, rows, cols)
    assert auto.filter_stats is None
    _assert_same_words(auto, e)
    # ... and the filter once the threshold says so
    monkeypatch.setattr(engine, "JACCARD_FILTER_MIN_PAIRS", 1)
    auto = engine._PairwisePositions(a, b, J, -1.0, 0.0, f32, rows, cols)
    _assert_accounted(auto.filter_stats, NA * NB)
    _assert_same_words(auto, e)
    P = _Problem(a, b, rows, cols, -1.0, 0.0)
    f_r, f_c, st = P.count(P.side(0, NB), P.side(1, NA), return_stats=True)
    assert st is not None and _stats(st)["overflow"] == 0
    # float64 words and the other measures never take it, whatever the threshold
    assert engine._PairwisePositions(a, b, J, -1.0, 0.0, torch.float64, rows, cols).filter_stats is None
    assert engine._PairwisePositions(a, b, _lib.PW_SQ_L2, 1.0, 0.0, f32, rows, cols).filter_stats is None


# ---- 9. the C entry's refusals -------------------------------------------------------------------------------------------------

def test_refusals_of_the_entry():
    import torch
    from cmve import _lib, engine
    rng = np.random.default_rng(6)
    a = engine.to_device(np.abs(rng.standard_normal((40, 67))))
    b = engine.to_device(np.abs(rng.standard_normal((50, 67))))
    dev = a.device
    sa = engine.JaccardSet(a)
    sb = engine.JaccardSet(b, grid=sa.grid)
    off, idx = engine.csr([[i] for i in range(40)], dev)
    sc = torch.zeros(40, dtype=torch.float64, device=dev)
    ws = torch.empty(1024, dtype=torch.int64, device=dev)

    def call(alpha=-1.0, beta=0.0, d=67, codes=sb.codes, err=sb.err, qsum=sb.qsum, asum=sb.asum, grid=sa.grid,
             a_dtype=_lib.CMVE_F64):
        pos = torch.full((40,), 77, dtype=torch.int32, device=dev)
        stats = torch.full((4,), 77, dtype=torch.int64, device=dev)
        p = engine._ptr
        rc = _lib.lib.cmve_jaccard_count(engine.handle(dev), p(a), a_dtype, 67, 40, p(sa.codes), p(sa.err), p(sa.qsum),
                                         p(sa.asum), p(b), _lib.CMVE_F64, 67, 50, p(codes), p(err), p(qsum), p(asum),
                                         d, p(grid), alpha, beta, p(off), p(sc), 40, 50, p(pos), None, None, 0, 40,
                                         None, p(ws), 8 * 1024, p(stats))
        msg = _lib.lib.cmve_last_error()
        torch.cuda.synchronize()
        return rc, msg, bool((pos == 77).all()) and bool((stats == 77).all())

    rc, msg, untouched = call()
    assert rc == 0 and not untouched                      # the accepted call, for contrast
    for alpha, beta in ((0.0, 0.0), (float("nan"), 0.0), (float("inf"), 0.0), (1.0, float("inf")),
                        (1.0, float("nan"))):
        rc, msg, untouched = call(alpha, beta)
        assert rc < 0 and b"cmve_jaccard_count" in msg and b"alpha" in msg and untouched
    rc, msg, untouched = call(d=65537)
    assert rc < 0 and b"cmve_jaccard_count" in msg and b"65536" in msg and untouched
    for kw in (dict(codes=None), dict(err=None), dict(qsum=None), dict(asum=None), dict(grid=None)):
        rc, msg, untouched = call(**kw)
        assert rc < 0 and b"cmve_jaccard_count" in msg and b"missing" in msg and untouched
    rc, msg, untouched = call(a_dtype=_lib.CMVE_BF16)
    assert rc < 0 and b"cmve_jaccard_count" in msg and b"CMVE_F32/CMVE_F64" in msg and untouched
    # the row sums' own entry: a short pad, a NULL output
    n_pad, d_pad = engine.l1_pack_size(50, 67)
    for np_, dp_ in ((n_pad - 128, d_pad), (n_pad, d_pad - 32), (n_pad + 1, d_pad)):
        rc = _lib.lib.cmve_jaccard_rowsums(engine.handle(dev), engine._ptr(b), _lib.CMVE_F64, 67, 50, 67,
                                           engine._ptr(sa.grid), np_, dp_, engine._ptr(sb.qsum), engine._ptr(sb.asum))
        assert rc < 0 and b"cmve_jaccard_rowsums" in _lib.lib.cmve_last_error()
    rc = _lib.lib.cmve_jaccard_rowsums(engine.handle(dev), engine._ptr(b), _lib.CMVE_F64, 67, 50, 67,
                                       engine._ptr(sa.grid), n_pad, d_pad, None, engine._ptr(sb.asum))
    assert rc < 0 and b"cmve_jaccard_rowsums" in _lib.lib.cmve_last_error()
