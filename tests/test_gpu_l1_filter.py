"""K22 on the GPU: the count pass of the L1 measures (l1 / l1_norm) through the integer SAD filter.

The contract: the filter decides only comparisons that its rigorous bound (DESIGN s4, K22) puts out of reach of
every rounding, and re-scores the rest on the canonical fp64 chain -- so positions and ranks equal the fp64 route
(K18) WORD FOR WORD, ties, near-ties, NaN, inf and huge rows included, whether or not the band list held the band --
and it must actually filter: a build that sends every pair to the re-score does not pass."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NA, NB = 300, 520
AB = [(1.0, 0.0), (None, -1.0), (1.0, -1.0), (None, 0.0)]
AB_IDS = ["l1", "l1_norm", "a1b-1", "a-1/Db0"]
DTS = [(np.float32, np.float32), (np.float64, np.float64), (np.float32, np.float64)]
DTS_IDS = ["f32", "f64", "mixed"]


@pytest.fixture(scope="module")
def fx(golden):
    return golden("measures_retrieval")


def _both(a, b, alpha, beta, rows, cols):
    import torch
    from cmve import _lib, engine
    f = engine._PairwisePositions(a, b, _lib.PW_L1, alpha, beta, torch.float64, rows, cols, filter="l1")
    e = engine._PairwisePositions(a, b, _lib.PW_L1, alpha, beta, torch.float64, rows, cols, filter=False)
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

@pytest.mark.parametrize("m", ["l1", "l1_norm"])
def test_reference_parity_under_the_filter(fx, m):
    from cmve import engine
    from cmve.linas import evaluation as E, metrics as M
    from cmve.linas.validate import cal_perf_embeddings
    vid, cap = fx["vid"], fx["cap"]
    v2t_gt, t2v_gt = M.get_gt(list(fx["video_ids"]), list(fx["caption_ids"]))
    c, v = E.measure_rows(cap, m), E.measure_rows(vid, m)
    metric, alpha, beta, _, sc_dt = E.measure_spec(m, v.shape[1])
    rr, cr = engine.pairwise_gt_ranks(c, v, metric, alpha, beta, sc_dt, M._lists(t2v_gt, len(cap)), v2t_gt,
                                      filter="l1")
    assert np.array_equal(rr, fx["t2v_ranks_" + m]) and np.array_equal(cr, fx["v2t_ranks_" + m])
    v2t, t2v = cal_perf_embeddings(vid, cap, list(fx["video_ids"]), list(fx["caption_ids"]), measure=m, filter="l1")
    ref = fx["cal_perf_" + m]
    np.testing.assert_allclose(np.array(v2t), ref[0], rtol=0, atol=1e-12)
    np.testing.assert_allclose(np.array(t2v), ref[1], rtol=0, atol=1e-12)


# ---- 2. word for word against the fp64 route -----------------------------------------------------------------------------

def _ulps(v, steps):
    for _ in range(steps):
        v = np.nextafter(v, v.dtype.type(np.inf))
    return v


def _adversarial(d, dt_a, dt_b):
    """The recipe of tests/test_gpu_l2_filter.py: Gaussian rows with planted GTs plus everything that can break a
    filter: exact duplicates 256 rows apart, a block of 1 / 2 / 4-ulp perturbations of one row, zero, huge, tiny, inf
    and NaN rows; lists with 0, 1, several and 20 items, repeated items, NaN items."""
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


@pytest.mark.parametrize("ab", AB, ids=AB_IDS)
@pytest.mark.parametrize("dts", DTS, ids=DTS_IDS)
@pytest.mark.parametrize("d", [67, 1024])
def test_words_equal_the_fp64_route(adversarial, d, dts, ab):
    a, b, rows, cols = adversarial(d, *dts)
    alpha = -1.0 / d if ab[0] is None else ab[0]
    f, e = _both(a, b, alpha, ab[1], rows, cols)
    _assert_same_words(f, e)
    st = f.filter_stats
    print("d %d: decided %d, band %d (%.2f%%)" % (d, st["decided"], st["band"], 100.0 * st["band"] / (NA * NB)))
    _assert_accounted(st, NA * NB)
    assert 0 < st["band"] < NA * NB // 8            # the filter must actually filter


# ---- 3. extremes ---------------------------------------------------------------------------------------------------------

def test_extreme_codes_and_clamped_rows():
    import torch
    from cmve import _lib, engine
    rng = np.random.default_rng(22)
    na, nb, d = 140, 150, 1024
    a, b = rng.uniform(-1.0, 1.0, (na, d)), rng.uniform(-1.0, 1.0, (nb, d))
    a[0], b[0] = -3.0, 3.0            # all-lo against all-hi: the SAD is 65535 * 1024 > 2^24
    a[1], b[1] = 3.0, -3.0
    rows = [[int(j)] for j in rng.integers(0, nb, na)]
    rows[0], rows[1], rows[2] = [0, 1, 5], [1, 0], [0, 1]
    cols = [[int(i)] for i in rng.integers(0, na, nb)]
    cols[0], cols[1] = [0, 1, 7], [1, 0]
    for alpha, beta in ((1.0, 0.0), (-1.0 / d, -1.0)):
        f, e = _both(a, b, alpha, beta, rows, cols)
        _assert_same_words(f, e)
        _assert_accounted(f.filter_stats, na * nb)
    # a row far outside the grid of a resident gallery clamps: its error is large, its words are the same
    P = _Problem(a, b, rows, cols, 1.0, 0.0)
    g = engine.L1Set(P.b)
    far = P.a.clone()
    far[3] = 50.0
    far[4, ::2] = -1e6
    Q = _Problem(far, P.b, rows, cols, 1.0, 0.0)
    row, col = Q.side(0, nb), Q.side(1, na)
    e_r, e_c = Q.count(row, col, filter=False)
    f_r, f_c, st = Q.count(row, col, b=g, filter="l1", return_stats=True)
    assert _same(f_r, e_r) and _same(f_c, e_c)
    s = _stats(st)
    assert s["overflow"] == 0 and s["decided"] + s["band"] == na * nb and s["rescored"] == s["band"]
    # d = 1
    a1, b1 = rng.standard_normal((37, 1)), rng.standard_normal((41, 1))
    b1[5] = a1[3]
    f, e = _both(a1, b1, 1.0, 0.0, [[int(j)] for j in rng.integers(0, 41, 37)], [[3, 0] for _ in range(41)])
    _assert_same_words(f, e)
    _assert_accounted(f.filter_stats, 37 * 41)


# ---- 4. an overflowing band list is resolved on the device -------------------------------------------------------------------

class _Problem:
    """Rows on the device and both CSR sides with their item words from pairwise_item_scores (computed once)."""

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
            sc = engine.pairwise_item_scores(self.a, self.b, _lib.PW_L1, alpha, beta, torch.float64, off, idx, items,
                                             col_dir, 0)
            self.sides.append((off, sc.contiguous()))

    def side(self, which, n):
        off, sc = self.sides[which]
        return (off, sc, n)

    def count(self, row, col, a=None, b=None, **kw):
        import torch
        from cmve import _lib, engine
        return engine.pairwise_count(self.a if a is None else a, self.b if b is None else b, _lib.PW_L1, self.alpha,
                                     self.beta, torch.float64, row=row, col=col, **kw)


def _same(x, y):
    import torch
    if x is None or y is None:
        return x is None and y is None
    return x.dtype == torch.int32 and torch.equal(x, y)


def _stats(t):
    decided, band, rescored, overflow = (int(v) for v in t.cpu().numpy())
    return {"decided": decided, "band": band, "rescored": rescored, "overflow": overflow}


@pytest.mark.parametrize("ab", [AB[0], AB[1]], ids=AB_IDS[:2])
@pytest.mark.parametrize("d", [67, 1024])
def test_overflow_is_resolved_on_the_device(adversarial, monkeypatch, d, ab):
    import torch
    alpha = -1.0 / d if ab[0] is None else ab[0]
    P = _Problem(*adversarial(d, np.float32, np.float64), alpha, ab[1])
    dev = P.a.device
    for rn, cn in ((NB, NA), (0, 0)):
        row, col = P.side(0, rn), P.side(1, cn)
        e_r, e_c = P.count(row, col, filter=False)
        f_r, f_c, st = P.count(row, col, filter="l1", band=torch.empty(8, dtype=torch.int64, device=dev),
                               return_stats=True)
        assert _same(f_r, e_r) and _same(f_c, e_c)
        small = _stats(st)
        assert small["overflow"] == 1 and small["rescored"] == 0 and small["band"] > 8
        assert small["decided"] + small["band"] == P.pairs                # band reports the whole need
        f_r, f_c, st = P.count(row, col, filter="l1", band=torch.empty(small["band"], dtype=torch.int64, device=dev),
                               return_stats=True)
        assert _same(f_r, e_r) and _same(f_c, e_c)
        assert _stats(st) == dict(decided=small["decided"], band=small["band"], rescored=small["band"], overflow=0)
    # no slot at all, one direction at a time
    band = torch.empty(0, dtype=torch.int64, device=dev)
    for row, col in ((P.side(0, NB), None), (None, P.side(1, NA))):
        e_r, e_c = P.count(row, col, filter=False)
        f_r, f_c, st = P.count(row, col, filter="l1", band=band, return_stats=True)
        assert _same(f_r, e_r) and _same(f_c, e_c) and _stats(st)["overflow"] == 1
    # the positions route says that the canonical count ran
    from cmve import engine
    monkeypatch.setattr(engine, "l2_band_cap", lambda pairs: 8)
    a, b, rows, cols = adversarial(d, np.float32, np.float64)
    f, e = _both(a, b, alpha, ab[1], rows, cols)
    _assert_same_words(f, e)
    assert f.filter_stats["fallback"] is True and f.filter_stats["overflow"] == 1 and not f.filter_stats["redone"]


# ---- 5. a resident side -----------------------------------------------------------------------------------------------------

def test_resident_gallery_over_two_batches(adversarial):
    import torch
    from cmve import engine
    a, b, rows, cols = adversarial(67, np.float64, np.float64)
    P = _Problem(a, b, rows, cols, -1.0 / 67, -1.0)
    g = engine.L1Set(P.b)
    assert g.raw.data_ptr() == P.b.data_ptr() and g.codes.dtype == torch.int16 and g.err.dtype == torch.float64
    assert (g.n_pad, g.d_pad) == engine.l1_pack_size(NB, 67) and g.grid.shape == (2,)
    lo, hi = (float(v) for v in g.grid.cpu())
    fin = b[np.isfinite(b) & (np.abs(b) <= 1e30)]
    assert lo == fin.min() and hi == fin.max()
    row, col = P.side(0, NB), P.side(1, NA)
    e_r, e_c = P.count(row, col, filter=False)
    # batch 1: plain captions, packed on the gallery's grid inside the call; batch 2: an L1Set the caller packed
    f_r, f_c, st1 = P.count(row, col, b=g, filter="l1", return_stats=True)
    assert _same(f_r, e_r) and _same(f_c, e_c)
    caps = engine.L1Set(P.a, grid=g.grid)
    assert caps.grid.data_ptr() == g.grid.data_ptr()
    f_r, f_c, st2 = P.count(row, col, a=caps, b=g, filter="l1", return_stats=True)
    assert _same(f_r, e_r) and _same(f_c, e_c) and torch.equal(st1, st2)
    s = _stats(st2)
    assert s["overflow"] == 0 and s["decided"] + s["band"] == P.pairs and s["rescored"] == s["band"]
    assert (float(g.grid[0]), float(g.grid[1])) == (lo, hi)          # packing on a grid does not move it
    # a second batch with elements outside the gallery's range
    a2 = a.copy()
    a2[30:60] *= 40.0
    a2[61] += 1e4
    P2 = _Problem(a2, b, rows, cols, -1.0 / 67, -1.0)
    row, col = P2.side(0, NB), P2.side(1, NA)
    e_r, e_c = P2.count(row, col, filter=False)
    x = P2.count(row, col, b=g, filter="l1", return_stats=True)
    y = P2.count(row, col, b=g, filter="l1", return_stats=True)
    assert _same(x[0], e_r) and _same(x[1], e_c)
    assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) and torch.equal(x[2], y[2])
    assert _stats(x[2])["overflow"] == 0
    # an L1Set is the fp64 route's operand through its raw rows; sets on different grids are refused
    z = P2.count(row, col, b=g, filter=False, return_stats=True)
    assert _same(z[0], e_r) and _same(z[1], e_c) and z[2] is None
    with pytest.raises(ValueError, match="different grids"):
        P.count(P.side(0, NB), None, a=engine.L1Set(P.a), b=g, filter="l1")


# ---- 6. degenerate -----------------------------------------------------------------------------------------------------------

def test_degenerate_shapes_and_grids(adversarial):
    import torch
    from cmve import engine
    a, b, rows, cols = adversarial(67, np.float64, np.float64)
    for r, c in ((rows, None), (None, cols)):
        f, e = _both(a, b, 1.0, 0.0, r, c)
        _assert_same_words(f, e)
        _assert_accounted(f.filter_stats, NA * NB)
    for aa, bb, r, c in ((a[:0], b, [], [[] for _ in range(NB)]), (a, b[:0], [[] for _ in range(NA)], []),
                         (a[:5], b[:0], [[], [], [], [], []], [])):
        f, e = _both(aa, bb, -1.0 / 67, -1.0, r, c)
        _assert_same_words(f, e)
    # empty lists everywhere: nothing to count, nothing launched
    f, e = _both(a, b, 1.0, 0.0, [[] for _ in range(NA)], [[] for _ in range(NB)])
    _assert_same_words(f, e)
    # empty sides through pairwise_count: the NaN items still get the caller's n
    P = _Problem(a, b, rows, cols, 1.0, 0.0)
    dev = P.a.device
    nan = float("nan")
    coff = torch.tensor([0, 2, 3] + [3] * (NB - 2), dtype=torch.int64, device=dev)
    csc = torch.tensor([nan, 1.0, nan], dtype=torch.float64, device=dev)
    roff0 = torch.zeros(1, dtype=torch.int64, device=dev)
    none_sc = torch.empty(0, dtype=torch.float64, device=dev)
    for cn in (7, 0):
        row, col = (roff0, none_sc, NB), (coff, csc, cn)
        e_ = P.count(row, col, a=P.a[:0], filter=False)
        f_r, f_c, st = P.count(row, col, a=P.a[:0], filter="l1", return_stats=True)
        assert _same(f_r, e_[0]) and _same(f_c, e_[1]) and _stats(st) == dict(decided=0, band=0, rescored=0, overflow=0)
        if cn:
            assert f_c.tolist() == [cn - 1, 0, cn - 1]
    # a grid from constant rows (hi == lo): lo = 0, s = 1 -- every row of the other set is far off it
    const = np.full((40, 67), 0.25)
    g = engine.L1Set(const)
    assert float(g.grid[0]) == float(g.grid[1]) == 0.25
    rows40 = [[i % NB] for i in range(40)]
    cols40 = [[j % 40] for j in range(NB)]
    Pc = _Problem(const, b, rows40, cols40, 1.0, 0.0)
    row, col = Pc.side(0, NB), Pc.side(1, 40)
    e_r, e_c = Pc.count(row, col, filter=False)
    f_r, f_c, st = Pc.count(row, col, a=g, filter="l1", return_stats=True)
    assert _same(f_r, e_r) and _same(f_c, e_c)
    s = _stats(st)
    assert s["decided"] + s["band"] == 40 * NB
    # constant rows on both sides: every distance is exactly 0, every comparison a tie
    f, e = _both(const, const[:33], 1.0, 0.0, [[i % 33] for i in range(40)], [[j] for j in range(33)])
    _assert_same_words(f, e)
    # no eligible element at all: the empty grid
    allnan = np.full((3, 67), np.nan)
    gn = engine.L1Set(allnan)
    assert float(gn.grid[0]) == float("inf") and float(gn.grid[1]) == float("-inf")
    f, e = _both(allnan, b[:9], 1.0, 0.0, [[0], [1], [2]], [[0] for _ in range(9)])
    _assert_same_words(f, e)


# ---- 7. dispatch -------------------------------------------------------------------------------------------------------------

def test_dispatch(adversarial, monkeypatch):
    import torch
    from cmve import _lib, engine
    a, b, rows, cols = adversarial(67, np.float64, np.float64)
    with pytest.raises(ValueError, match="PW_L1"):
        engine.pairwise_gt_ranks(a, b, _lib.PW_L2, 1.0, 0.0, torch.float64, rows, None, filter="l1")
    with pytest.raises(ValueError, match="float64 score words"):
        engine.pairwise_gt_ranks(a, b, _lib.PW_L1, 1.0, 0.0, torch.float32, rows, None, filter="l1")
    with pytest.raises(ValueError, match="alpha"):
        engine.pairwise_gt_ranks(a, b, _lib.PW_L1, 0.0, 0.0, torch.float64, rows, None, filter="l1")
    with pytest.raises(ValueError, match="PW_L1"):
        engine.pairwise_count(a, b, _lib.PW_L2, 1.0, 0.0, torch.float64, filter="l1")
    # auto: 300 x 520 stays on the fp64 route ...
    assert engine.L1_FILTER_MIN_PAIRS is None or engine.L1_FILTER_MIN_PAIRS > NA * NB
    auto = engine._PairwisePositions(a, b, _lib.PW_L1, 1.0, 0.0, torch.float64, rows, cols)
    assert auto.filter_stats is None
    e = engine._PairwisePositions(a, b, _lib.PW_L1, 1.0, 0.0, torch.float64, rows, cols, filter=False)
    # ... and takes the filter once the threshold says so
    monkeypatch.setattr(engine, "L1_FILTER_MIN_PAIRS", 1)
    auto = engine._PairwisePositions(a, b, _lib.PW_L1, 1.0, 0.0, torch.float64, rows, cols)
    _assert_accounted(auto.filter_stats, NA * NB)
    _assert_same_words(auto, e)
    P = _Problem(a, b, rows, cols, 1.0, 0.0)
    f_r, f_c, st = P.count(P.side(0, NB), P.side(1, NA), return_stats=True)
    assert st is not None and _stats(st)["overflow"] == 0
    # the other measures and fp32 words never take it, whatever the threshold
    assert engine._PairwisePositions(a, b, _lib.PW_SQ_L2, 1.0, 0.0, torch.float64, rows, cols).filter_stats is None
    assert engine._PairwisePositions(a, b, _lib.PW_L1, 1.0, 0.0, torch.float32, rows, cols).filter_stats is None


def test_refusals_of_the_entry():
    import ctypes as C
    import torch
    from cmve import _lib, engine
    rng = np.random.default_rng(6)
    a, b = engine.to_device(rng.standard_normal((40, 67))), engine.to_device(rng.standard_normal((50, 67)))
    dev = a.device
    sa = engine.L1Set(a)
    sb = engine.L1Set(b, grid=sa.grid)
    off, idx = engine.csr([[i] for i in range(40)], dev)
    sc = torch.zeros(40, dtype=torch.float64, device=dev)
    ws = torch.empty(1024, dtype=torch.int64, device=dev)

    def call(alpha=1.0, beta=0.0, d=67, codes=sb.codes, err=sb.err, grid=sa.grid):
        pos = torch.full((40,), 77, dtype=torch.int32, device=dev)
        stats = torch.full((4,), 77, dtype=torch.int64, device=dev)
        rc = _lib.lib.cmve_l1_count(engine.handle(dev), engine._ptr(a), _lib.CMVE_F64, 67, 40, engine._ptr(sa.codes),
                                    engine._ptr(sa.err), engine._ptr(b), _lib.CMVE_F64, 67, 50, engine._ptr(codes),
                                    engine._ptr(err), d, engine._ptr(grid), alpha, beta, engine._ptr(off),
                                    engine._ptr(sc), 40, 50, engine._ptr(pos), None, None, 0, 40, None,
                                    engine._ptr(ws), 8 * 1024, engine._ptr(stats))
        msg = _lib.lib.cmve_last_error()
        torch.cuda.synchronize()
        return rc, msg, bool((pos == 77).all()) and bool((stats == 77).all())

    rc, msg, untouched = call()
    assert rc == 0 and not untouched                      # the accepted call, for contrast
    for alpha, beta in ((0.0, 0.0), (float("nan"), 0.0), (float("inf"), 0.0), (1.0, float("inf"))):
        rc, msg, untouched = call(alpha, beta)
        assert rc < 0 and b"cmve_l1_count" in msg and b"alpha" in msg and untouched
    rc, msg, untouched = call(d=65537)
    assert rc < 0 and b"cmve_l1_count" in msg and b"65536" in msg and untouched
    for kw in (dict(codes=None), dict(err=None), dict(grid=None)):
        rc, msg, untouched = call(**kw)
        assert rc < 0 and b"cmve_l1_count" in msg and b"missing" in msg and untouched
    # a short pad
    n_pad, d_pad = engine.l1_pack_size(50, 67)
    for np_, dp_ in ((n_pad - 128, d_pad), (n_pad, d_pad - 32), (n_pad + 1, d_pad)):
        rc = _lib.lib.cmve_l1_pack(engine.handle(dev), engine._ptr(b), _lib.CMVE_F64, 67, 50, 67, engine._ptr(sa.grid),
                                   engine._ptr(sb.codes), np_, dp_, engine._ptr(sb.err))
        assert rc < 0 and b"short pad" in _lib.lib.cmve_last_error()


# ---- 8. a tile without a list (both filters share the epilogue's branch for it) -------------------------------------------

@pytest.mark.parametrize("flt", ["l1", True], ids=["l1", "l2"])
def test_a_tile_with_no_list_in_it(flt):
    """256 x 130 x 33: the tiles of rows 128..255 hold no list at all (empty row lists, no column lists), so the count
    epilogue has nothing to decide there -- but row 200 holds a NaN, its pairs have no interval, and every one of
    them must still reach the band list so that decided + band = pairs."""
    import torch
    from cmve import _lib, engine
    na, nb, d = 256, 130, 33
    rng = np.random.default_rng(22)
    a, b = rng.standard_normal((na, d)), rng.standard_normal((nb, d))
    a[200, 5] = np.nan
    rows = [[i % nb] if i < 128 else [] for i in range(na)]
    metric = _lib.PW_L1 if flt == "l1" else _lib.PW_L2
    a, b = engine.to_device(a), engine.to_device(b)
    f = engine._PairwisePositions(a, b, metric, 1.0, 0.0, torch.float64, rows, None, filter=flt)
    e = engine._PairwisePositions(a, b, metric, 1.0, 0.0, torch.float64, rows, None, filter=False)
    assert e.filter_stats is None
    _assert_same_words(f, e)
    st = f.filter_stats
    assert st is not None and st["decided"] + st["band"] == na * nb
    assert st["band"] >= nb
    assert st["rescored"] == st["band"] and st["overflow"] == 0


# ---- 9. the seams of the one count body (sad_count.h) ---------------------------------------------------------------------

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
