"""K21 on the GPU: cmve_l2_count_resolved through engine.pairwise_count(filter=True) -- the count pass of the
Euclidean measures through the fp16 MFMA filter, exact whatever the band list does and decided on the device.

The contract: row_pos / col_pos equal cmve_pairwise_count's (filter=False) WORD FOR WORD -- ties, near-ties, NaN, inf,
overflowing and underflowing rows, NaN items, the caller's n included -- whether the band list held the band, held one
pair or had no slot at all; the counters say which happened; and with a list that fits it must actually filter."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NA, NB = 300, 520
AB = [(1.0, 0.0), (None, -1.0), (1.0, -1.0), (None, 0.0)]
AB_IDS = ["l2", "l2_norm", "a1b-1", "a-1/Db0"]
DTS = [(np.float32, np.float32), (np.float64, np.float64), (np.float32, np.float64)]
DTS_IDS = ["f32", "f64", "mixed"]


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


class _Problem:
    """Rows on the device and both CSR sides with their item words from pairwise_item_scores (computed once)."""

    def __init__(self, a, b, rows, cols, alpha, beta):
        import torch
        from cmve import _lib, engine
        self.a, self.b = engine.to_device(a), engine.to_device(b)
        self.alpha, self.beta = alpha, beta
        self.pairs = a.shape[0] * b.shape[0]
        dev = self.a.device
        self.sides = []
        for lists, col_dir in ((rows, False), (cols, True)):
            off, idx = engine.csr(lists, dev)
            items = sum(len(l) for l in lists)
            sc = engine.pairwise_item_scores(self.a, self.b, _lib.PW_L2, alpha, beta, torch.float64, off, idx, items,
                                             col_dir, 0)
            self.sides.append((off, sc.contiguous()))

    def side(self, which, n):
        off, sc = self.sides[which]
        return (off, sc, n)

    def count(self, row, col, a=None, b=None, **kw):
        import torch
        from cmve import _lib, engine
        return engine.pairwise_count(self.a if a is None else a, self.b if b is None else b, _lib.PW_L2, self.alpha,
                                     self.beta, torch.float64, row=row, col=col, **kw)


def _same(x, y):
    import torch
    if x is None or y is None:
        return x is None and y is None
    return x.dtype == torch.int32 and torch.equal(x, y)


def _stats(t):
    decided, band, rescored, overflow = (int(v) for v in t.cpu().numpy())
    return {"decided": decided, "band": band, "rescored": rescored, "overflow": overflow}


@pytest.fixture(scope="module")
def problems():
    cache = {}

    def get(d, dts, ab):
        key = (d, dts, ab)
        if key not in cache:
            alpha = -1.0 / d if ab[0] is None else ab[0]
            cache[key] = _Problem(*_adversarial(d, *dts), alpha, ab[1])
        return cache[key]
    return get


# ---- 1. the words equal the fp64 route ---------------------------------------------------------------------------------

@pytest.mark.parametrize("ab", AB, ids=AB_IDS)
@pytest.mark.parametrize("dts", DTS, ids=DTS_IDS)
@pytest.mark.parametrize("d", [67, 1024])
def test_words_equal_the_fp64_route(problems, d, dts, ab):
    import torch
    P = problems(d, dts, ab)
    # the caller's n: the other side's size, and 0 ("another shard stores the NaN words")
    for rn, cn in ((NB, NA), (0, 0)):
        for row, col in ((P.side(0, rn), None), (None, P.side(1, cn)), (P.side(0, rn), P.side(1, cn))):
            e_r, e_c = P.count(row, col, filter=False)
            f_r, f_c, st = P.count(row, col, filter=True, return_stats=True)
            assert _same(f_r, e_r) and _same(f_c, e_c)
            assert st.dtype == torch.int64 and st.shape == (4,) and st.is_cuda
            s = _stats(st)
            # the default list holds this band (the parent's own test pins 0 < band < pairs / 8 on these rows)
            assert s["overflow"] == 0 and s["decided"] + s["band"] == P.pairs and s["rescored"] == s["band"]
    # the NaN items' words really differ between the two n (the case is not vacuous)
    with_n, without = P.count(P.side(0, NB), None, filter=True)[0], P.count(P.side(0, 0), None, filter=True)[0]
    assert not torch.equal(with_n, without)


def test_packed_sides_and_return_shapes(problems):
    import torch
    from cmve import engine
    P = problems(67, DTS[1], AB[1])
    row, col = P.side(0, NB), P.side(1, NA)
    e_r, e_c = P.count(row, col, filter=False)
    ra = engine.RowSet(P.a, eps=0.0, with_lo=False)
    rb = engine.RowSet(P.b, eps=0.0, with_lo=False)
    assert rb.raw.data_ptr() == P.b.data_ptr()  # the pack keeps the rows it is given
    for a, b in ((ra, rb), (None, rb), (ra, None)):
        f_r, f_c, st = P.count(row, col, a=a, b=b, filter=True, return_stats=True)
        assert _same(f_r, e_r) and _same(f_c, e_c) and _stats(st)["overflow"] == 0
        # a packed side is the fp64 route's operand through its raw rows
        g_r, g_c, none = P.count(row, col, a=a, b=b, filter=False, return_stats=True)
        assert _same(g_r, e_r) and _same(g_c, e_c) and none is None
    assert len(P.count(row, col, filter=True)) == 2
    # below L2_FILTER_MIN_PAIRS the auto rule leaves the call on the fp64 route
    assert NA * NB < engine.L2_FILTER_MIN_PAIRS
    a_r, a_c, none = P.count(row, col, return_stats=True)
    assert _same(a_r, e_r) and _same(a_c, e_c) and none is None
    with pytest.raises(TypeError, match="band"):
        P.count(row, col, filter=True, band=torch.empty(8, dtype=torch.int32, device=P.a.device))


def test_empty_sides_and_no_items(problems):
    import torch
    P = problems(67, DTS[1], AB[0])
    dev = P.a.device
    nan = float("nan")
    # no caption: the column lists' NaN items still get the caller's n
    coff = torch.tensor([0, 2, 3] + [3] * (NB - 2), dtype=torch.int64, device=dev)
    csc = torch.tensor([nan, 1.0, nan], dtype=torch.float64, device=dev)
    roff0 = torch.zeros(1, dtype=torch.int64, device=dev)
    none_sc = torch.empty(0, dtype=torch.float64, device=dev)
    for cn in (7, 0):
        row, col = (roff0, none_sc, NB), (coff, csc, cn)
        e = P.count(row, col, a=P.a[:0], filter=False)
        f_r, f_c, st = P.count(row, col, a=P.a[:0], filter=True, return_stats=True)
        assert _same(f_r, e[0]) and _same(f_c, e[1]) and _stats(st) == dict(decided=0, band=0, rescored=0, overflow=0)
        if cn:
            assert f_c.tolist() == [cn - 1, 0, cn - 1]
    # no video
    roff = torch.tensor([0, 1] + [1] * (NA - 1), dtype=torch.int64, device=dev)
    rsc = torch.tensor([nan], dtype=torch.float64, device=dev)
    row, col = (roff, rsc, 9), (roff0, none_sc, NA)
    e = P.count(row, col, b=P.b[:0], filter=False)
    f = P.count(row, col, b=P.b[:0], filter=True)
    assert _same(f[0], e[0]) and _same(f[1], e[1]) and f[0].tolist() == [8]
    # no item on either side: nothing to count, the counters are zeroed
    roff = torch.zeros(NA + 1, dtype=torch.int64, device=dev)
    coff = torch.zeros(NB + 1, dtype=torch.int64, device=dev)
    f_r, f_c, st = P.count((roff, none_sc, NB), (coff, none_sc, NA), filter=True, return_stats=True)
    assert f_r.numel() == 0 and f_c.numel() == 0 and _stats(st) == dict(decided=0, band=0, rescored=0, overflow=0)


# ---- 2. an overflowing band list is resolved on the device -----------------------------------------------------------------

@pytest.mark.parametrize("ab", AB, ids=AB_IDS)
@pytest.mark.parametrize("dts", DTS, ids=DTS_IDS)
@pytest.mark.parametrize("d", [67, 1024])
def test_overflow_is_resolved_on_the_device(problems, d, dts, ab):
    import torch
    P = problems(d, dts, ab)
    dev = P.a.device
    for rn, cn in ((NB, NA), (0, 0)):
        row, col = P.side(0, rn), P.side(1, cn)
        e_r, e_c = P.count(row, col, filter=False)
        large = _stats(P.count(row, col, filter=True, band=torch.empty(NA * NB, dtype=torch.int64, device=dev),
                               return_stats=True)[2])
        assert large["overflow"] == 0 and large["band"] > 1
        for slots in (1, 0):
            band = torch.empty(slots, dtype=torch.int64, device=dev)
            f_r, f_c, st = P.count(row, col, filter=True, band=band, return_stats=True)
            assert _same(f_r, e_r) and _same(f_c, e_c)
            s = _stats(st)
            assert s["overflow"] == 1 and s["rescored"] == 0
            assert s["band"] == large["band"] and s["decided"] == large["decided"]
    # one direction at a time through the gated path as well
    band = torch.empty(1, dtype=torch.int64, device=dev)
    for row, col in ((P.side(0, NB), None), (None, P.side(1, NA))):
        e_r, e_c = P.count(row, col, filter=False)
        f_r, f_c, st = P.count(row, col, filter=True, band=band, return_stats=True)
        assert _same(f_r, e_r) and _same(f_c, e_c) and _stats(st)["overflow"] == 1


def test_clustered_rows_are_exact_with_the_default_list():
    """The rows of test_clustered_rows_fall_back_and_say_so: clustered far from the origin, the filter decides next
    to nothing -- the words are still the fp64 route's, and the counters say how they were made."""
    import torch
    rng = np.random.default_rng(3)
    na, nb, d = 256, 384, 256
    b = 100.0 + rng.standard_normal((nb, d))
    a = 100.0 + rng.standard_normal((na, d))
    rows = [[int(j)] for j in rng.integers(0, nb, na)]
    cols = [[int(i)] for i in rng.integers(0, na, nb)]
    P = _Problem(a, b, rows, cols, 1.0, 0.0)
    row, col = P.side(0, nb), P.side(1, na)
    e_r, e_c = P.count(row, col, filter=False)
    f_r, f_c, st = P.count(row, col, filter=True, return_stats=True)
    assert _same(f_r, e_r) and _same(f_c, e_c)
    s = _stats(st)
    print("clustered rows:", s)
    assert s["overflow"] == 1 or (s["decided"] + s["band"] == na * nb and s["rescored"] == s["band"])
    if s["overflow"]:
        assert s["rescored"] == 0 and s["band"] > P.pairs // 8  # what l2_band_plan turns into "stop asking"


# ---- 3. it filters -----------------------------------------------------------------------------------------------------------

def test_filter_decides_almost_every_pair():
    """Planted GTs, the recipe whose >= 99% the parent's test_filter_decides_almost_every_pair pins for cmve_l2_count:
    whether a pair is decided depends on its two rows and the item word, not on the entry."""
    rng = np.random.default_rng(0)
    na, nb, d = 512, 2048, 1024
    b = rng.standard_normal((nb, d))
    a = b[:na] + 0.5 * rng.standard_normal((na, d))
    rows = [[i] for i in range(na)]
    cols = [[j] if j < na else [] for j in range(nb)]
    P = _Problem(a, b, rows, cols, 1.0, 0.0)
    row, col = P.side(0, nb), P.side(1, na)
    e_r, e_c = P.count(row, col, filter=False)
    f_r, f_c, st = P.count(row, col, filter=True, return_stats=True)
    assert _same(f_r, e_r) and _same(f_c, e_c)
    s = _stats(st)
    print("planted GTs: decided %d of %d (%.3f%%), band %d" % (s["decided"], na * nb, 100.0 * s["decided"] / (na * nb),
                                                                s["band"]))
    assert s["overflow"] == 0
    assert s["decided"] + s["band"] == na * nb and s["rescored"] == s["band"]
    assert s["decided"] >= 0.99 * na * nb


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------

def test_refusals_name_the_entry_and_launch_nothing():
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
    NAME = b"cmve_l2_count_resolved"

    def call(x, y, alpha, beta=0.0, ws_ptr=None, ws_bytes=8 * 1024, row_n=None):
        pos = torch.full((40,), 77, dtype=torch.int32, device=dev)
        stats = torch.full((4,), 77, dtype=torch.int64, device=dev)
        rc = _lib.lib.cmve_l2_count_resolved(engine.handle(dev), C.byref(x.desc), C.byref(y.desc), alpha, beta,
                                             engine._ptr(off), engine._ptr(sc), 40, y.n if row_n is None else row_n,
                                             engine._ptr(pos), None, None, 0, x.n, None,
                                             engine._ptr(ws) if ws_ptr is None else ws_ptr, ws_bytes,
                                             engine._ptr(stats))
        msg = _lib.lib.cmve_last_error()
        torch.cuda.synchronize()
        untouched = bool((pos == 77).all()) and bool((stats == 77).all())
        return rc, msg, untouched

    rc, msg, untouched = call(ra, rb, 1.0)
    assert rc == 0 and not untouched                      # the accepted call, for contrast
    for alpha, beta in ((0.0, 0.0), (float("nan"), 0.0), (float("inf"), 0.0), (1.0, float("inf"))):
        rc, msg, untouched = call(ra, rb, alpha, beta)
        assert rc < 0 and NAME in msg and b"alpha" in msg and untouched
    rc, msg, untouched = call(ra, engine.RowSet(b, with_lo=False, with_f16=False), 1.0)
    assert rc < 0 and NAME in msg and b"fp16 plane" in msg and untouched
    rc, msg, untouched = call(ra, engine.RowSet(b[:, :66], with_lo=False), 1.0)
    assert rc < 0 and NAME in msg and b"dimensions differ" in msg and untouched
    rc, msg, untouched = call(ra, engine.RowSet(b, eps=1e-12, with_lo=False), 1.0)
    assert rc < 0 and NAME in msg and b"eps" in msg and untouched
    rc, msg, untouched = call(ra, engine.RowSet(b, with_lo=False, raw_rows=True), 1.0)
    assert rc < 0 and NAME in msg and b"CMVE_PACK_RAW" in msg and untouched
    rc, msg, untouched = call(ra, rb, 1.0, row_n=-1)
    assert rc < 0 and NAME in msg and b"bad counts" in msg and untouched
    rc, msg, untouched = call(ra, rb, 1.0, ws_ptr=C.c_void_p(0), ws_bytes=64)
    assert rc < 0 and NAME in msg and b"workspace missing" in msg and untouched
    rc, msg, untouched = call(ra, rb, 1.0, ws_ptr=C.c_void_p(ws.data_ptr() + 4), ws_bytes=64)
    assert rc < 0 and NAME in msg and b"8-byte aligned" in msg and untouched
    # the same refusal through cmve_l2_count still carries that entry's own name
    stats = torch.zeros(4, dtype=torch.int64, device=dev)
    pos = torch.zeros(40, dtype=torch.int32, device=dev)
    rc = _lib.lib.cmve_l2_count(engine.handle(dev), C.byref(ra.desc), C.byref(rb.desc), 0.0, 0.0, engine._ptr(off),
                                engine._ptr(sc), 40, 50, engine._ptr(pos), None, None, 0, 40, None, engine._ptr(ws),
                                8 * 1024, engine._ptr(stats))
    assert rc < 0 and _lib.lib.cmve_last_error().startswith(b"cmve_l2_count: ")
    # the Python route refuses what the entry cannot express
    with pytest.raises(ValueError, match="float64 score words"):
        engine.pairwise_count(ra, rb, _lib.PW_L2, 1.0, 0.0, torch.float32, row=(off, sc, 50), filter=True)
    with pytest.raises(ValueError, match="PW_L2"):
        engine.pairwise_count(ra, rb, _lib.PW_L1, 1.0, 0.0, torch.float64, row=(off, sc, 50), filter=True)
    with pytest.raises(_lib.CmveError, match="fp16 plane"):
        engine.pairwise_count(ra, engine.RowSet(b, with_lo=False, with_f16=False), _lib.PW_L2, 1.0, 0.0, torch.float64,
                              row=(off, sc, 50), filter=True)
