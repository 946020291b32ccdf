"""K20 on the GPU: the exact top-k of the Euclidean measures (euclidean / l2 / l2_norm) through the fp16 MFMA filter.

The contract: ids AND error words equal the fp64 route (``engine.pairwise_topk(filter=False)``, K18) word for word --
ties, near-ties, NaN, inf, overflowing and underflowing rows included; a query the filter cannot resolve is finished
on the fp64 route and reported; and the filter must actually filter."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NQ, NG = 300, 520          # three query tiles, five gallery tiles, partial tiles both ways
SPECIAL_Q = (10, 11, 12, 13, 14)
SPECIAL_G = (400, 401, 402, 403, 404)
AB = [(1.0, 0.0), (None, -1.0), (1.0, -1.0), (None, 0.0)]
AB_IDS = ["l2", "l2_norm", "a1b-1", "a-1/Db0"]
DTS = [(np.float32, np.float32), (np.float64, np.float64), (np.float32, np.float64)]
DT_IDS = ["f32", "f64", "mixed"]


def _words(x):
    return np.ascontiguousarray(x).view(np.int64)


def _same(got, want):
    assert got[0].dtype == np.int64 and got[0].shape == want[0].shape
    assert np.array_equal(got[0], want[0]), np.argwhere(got[0] != want[0])[:5]
    assert np.array_equal(_words(got[1]), _words(want[1]))


def _topk(q, g, alpha, beta, k, **kw):
    import torch
    from cmve import _lib, engine
    return engine.pairwise_topk(q, g, _lib.PW_L2, alpha, beta, torch.float64, k, **kw)


@pytest.fixture(scope="module")
def fx(golden):
    return golden("measures_retrieval")


# ---- 1. reference parity -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", ["euclidean", "l2", "l2_norm"])
def test_reference_parity_under_the_filter(fx, m):
    from cmve.linas.inference import GalleryScorer
    sc = GalleryScorer(fx["vid"], measure=m, filter=True)
    assert sc._packed is not None and sc._packed.raw.data_ptr() == sc.gallery.data_ptr()  # no second copy
    assert np.array_equal(sc.topk_indices(fx["cap"], 10), fx["top10_" + m])
    assert np.array_equal(GalleryScorer(fx["vid"], measure=m, filter=False).topk_indices(fx["cap"], 10),
                          fx["top10_" + m])


# ---- 2. word for word against the fp64 route -----------------------------------------------------------------------------

def _ulps(v, steps):
    for _ in range(steps):
        v = np.nextafter(v, v.dtype.type(np.inf))
    return v


def _adversarial(d, dt_q, dt_g):
    """Gaussian gallery, queries near gallery rows, plus everything that can break a filter: exact duplicates 256
    rows apart, a block of 40 1 / 2 / 4-ulp perturbations of one row (and a query whose top-k is that block), zero,
    huge, tiny, inf and NaN rows on both sides."""
    rng = np.random.default_rng(1000 + d)
    g = rng.standard_normal((NG, d))
    pick = rng.integers(0, 200, NQ)
    pick[20] = 7
    q = g[pick] + 0.5 * rng.standard_normal((NQ, d))
    with np.errstate(over="ignore"):
        q, g = q.astype(dt_q), g.astype(dt_g)
        g[256:296] = g[0:40]                       # exact ties: the index decides
        for t in range(40):                        # near-ties only the canonical chain can order
            row = g[7].copy()
            row[t % d] = _ulps(row[t % d], (1, 2, 4)[t % 3])
            g[300 + t] = row
        q[10], g[400] = 0.0, 0.0
        q[11], g[401] = 1e200, 1e200               # (+inf in float32)
        q[12], g[402] = 1e-200, 1e-200             # (zero in float32)
        q[13, 5 % d], g[403, 3] = np.inf, np.inf
        q[14, 0], g[404, 1] = np.nan, np.nan
    return q, g


@pytest.fixture(scope="module")
def adversarial():
    """(q, g, exact squared distances of the ordinary rows) by (d, dtypes); the fp64 route's top-64 by (.., alpha,
    beta): computed once, shared, never changed (the top-k of a smaller k is its prefix)."""
    sets, refs = {}, {}

    def get(d, dts, ab=None):
        if (d, dts) not in sets:
            q, g = _adversarial(d, *dts)
            q64, g64 = q.astype(np.float64), g.astype(np.float64)
            with np.errstate(all="ignore"):
                D = ((q64[:, None, :] - g64[None, :, :]) ** 2).sum(-1) if d < 128 else \
                    (q64 ** 2).sum(1)[:, None] + (g64 ** 2).sum(1)[None, :] - 2.0 * q64 @ g64.T
            sets[(d, dts)] = (q, g, D)
        if ab is None:
            return sets[(d, dts)]
        if (d, dts, ab) not in refs:
            q, g, _ = sets[(d, dts)]
            refs[(d, dts, ab)] = _topk(q, g, ab[0], ab[1], 64, filter=False)
        return sets[(d, dts)] + (refs[(d, dts, ab)],)
    return get


def _precondition(D, alpha, k, sample):
    """A condition on the INPUTS: for every ordinary query, the columns whose exact key s D lies within 1% of the
    k-th smallest key among the first `sample` columns, plus the special rows, number at most 480 (< cand_cap)."""
    ord_q = np.setdiff1d(np.arange(NQ), SPECIAL_Q)
    ord_g = np.setdiff1d(np.arange(NG), SPECIAL_G)
    key = np.sign(alpha) * D[np.ix_(ord_q, ord_g)]
    kth = np.sort(key[:, ord_g < sample], axis=1)[:, k - 1]
    count = (key <= (kth + 0.01 * np.abs(kth))[:, None]).sum(1) + len(SPECIAL_G)
    assert count.max() <= 480, count.max()


@pytest.mark.parametrize("ab", AB, ids=AB_IDS)
@pytest.mark.parametrize("dts", DTS, ids=DT_IDS)
@pytest.mark.parametrize("d", [67, 1024])
def test_words_equal_the_fp64_route(adversarial, d, dts, ab):
    from cmve import engine
    ab = (-1.0 / d if ab[0] is None else ab[0], ab[1])
    q, g, D, ref = adversarial(d, dts, ab)
    rq, rg = engine.RowSet(q, with_lo=False), engine.RowSet(g, with_lo=False)
    # k = 64 keeps the default sample (the whole gallery here): half of 128 sample rows would be its witnesses
    for k, sample in ((1, 128), (10, 128), (1, None), (10, None), (64, None)):
        _precondition(D, ab[0], k, 128 if sample else NG)
        idx, err, st = _topk(rq, rg, *ab, k, filter=True, cand_cap=512, sample_rows=sample, return_stats=True)
        print("d %d k %d sample %s: %s" % (d, k, sample, st))
        _same((idx, err), (ref[0][:, :k], ref[1][:, :k]))
        # the five special queries have no bound at all: unresolved by contract, finished on the fp64 route
        assert st["unresolved"] == len(SPECIAL_Q) == st["fallback_rows"] and not st["fallback"]
        assert st["rescored"] == st["candidates"] and 0 < st["candidates"] < NQ * NG
        assert st["excluded"] + st["candidates"] == (NQ - len(SPECIAL_Q)) * NG
    # the filter filters: with the default sample nearly every pair of a resolved query is excluded for k = 10
    _, _, st = _topk(rq, rg, *ab, 10, filter=True, return_stats=True)
    assert st["excluded"] >= 0.8 * (NQ - len(SPECIAL_Q)) * NG


# ---- 3. small and edge shapes --------------------------------------------------------------------------------------------

def test_small_and_edge_shapes(adversarial):
    q, g, _ = adversarial(67, (np.float64, np.float64))
    g300 = g[:300]
    for nq in (1, 5):
        for ab in ((1.0, 0.0), (-1.0 / 67, -1.0)):
            for k in (1, 10, 300, 400):  # k = n_g; k > n_g is clamped
                got = _topk(q[20:20 + nq], g300, *ab, k, filter=True, return_stats=True)
                _same(got[:2], _topk(q[20:20 + nq], g300, *ab, k, filter=False))
                assert got[0].shape[1] == min(k, 300) and got[2] is not None
    # fewer finite rows than k: NaN last, in index order
    few = g[:12].copy()
    few[[1, 2, 4, 5, 7, 8, 10, 11], 0] = np.nan
    got = _topk(q[:5], few, 1.0, 0.0, 10, filter=True, return_stats=True)
    _same(got[:2], _topk(q[:5], few, 1.0, 0.0, 10, filter=False))
    assert list(got[0][0, 4:]) == [1, 2, 4, 5, 7, 8] and np.isnan(got[1][:, 4:]).all()
    assert got[2]["unresolved"] == 5
    # a zero query row and a NaN query row, alone and in a batch
    for rows in ([10], [14], [9, 10, 14, 15]):
        for ab in ((1.0, 0.0), (-1.0 / 67, -1.0)):
            _same(_topk(q[rows], g, *ab, 10, filter=True), _topk(q[rows], g, *ab, 10, filter=False))


def test_two_rounds():
    """More than 1024 queries: the host body's second round of four launches (query 1024 is tile 8 of the packed
    planes), which K23's route shares."""
    rng = np.random.default_rng(26)
    n_q, n_g, d = 1025, 130, 8
    g = rng.standard_normal((n_g, d))
    q = rng.standard_normal((n_q, d))
    for ab in ((1.0, 0.0), (-1.0 / d, -1.0)):
        got = _topk(q, g, *ab, 3, filter=True, return_stats=True)
        _same(got[:2], _topk(q, g, *ab, 3, filter=False))
        st = got[2]
        print("two rounds, alpha %g: %s" % (ab[0], st))
        # 130 columns are below cand_cap: no list overflows, every pair of a resolved query is excluded or a candidate
        assert st["excluded"] + st["candidates"] == (n_q - st["unresolved"]) * n_g
        one = _topk(q[77:78], g, *ab, 3, filter=True)
        _same(one, (got[0][77:78], got[1][77:78]))


# ---- 4. the fallback is exact and says so --------------------------------------------------------------------------------

def test_fallback_is_exact_and_says_so(adversarial):
    q, g, _, ref = adversarial(67, (np.float64, np.float64), (1.0, 0.0))
    # no room beyond k: a query with any candidate besides its top-k is unresolved
    got = _topk(q, g, 1.0, 0.0, 10, filter=True, cand_cap=10, sample_rows=128, return_stats=True)
    _same(got[:2], (ref[0][:, :10], ref[1][:, :10]))
    st = got[2]
    assert st["unresolved"] > NQ // 2 and st["fallback_rows"] >= st["unresolved"] and st["fallback_rows"] > 0
    # rows clustered far from the origin (||a - b||^2 << ||a||^2): every bound is wider than every distance, every
    # gallery row is a candidate of every query, the lists overflow and the whole call takes the fp64 route
    rng = np.random.default_rng(3)
    gc = 100.0 + rng.standard_normal((2304, 64))
    qc = 100.0 + rng.standard_normal((130, 64))
    for ab in ((1.0, 0.0), (-1.0 / 64, -1.0)):
        got = _topk(qc, gc, *ab, 10, filter=True, return_stats=True)
        _same(got[:2], _topk(qc, gc, *ab, 10, filter=False))
        assert got[2]["fallback"] and got[2]["fallback_rows"] == 130 and got[2]["unresolved"] == 130
    # the sample is the far cluster, the rest of the gallery is near: a loose threshold, the lists overflow
    gl = rng.standard_normal((NG, 64))
    gl[:128] += 100.0
    ql = rng.standard_normal((40, 64))
    got = _topk(ql, gl, 1.0, 0.0, 10, filter=True, cand_cap=256, sample_rows=128, return_stats=True)
    _same(got[:2], _topk(ql, gl, 1.0, 0.0, 10, filter=False))
    assert got[2]["unresolved"] == 40 and got[2]["fallback"]


def test_scorer_asks_a_falling_back_gallery_once_and_keeps_one_workspace(adversarial, monkeypatch):
    from cmve import engine
    from cmve.linas.inference import GalleryScorer
    monkeypatch.setattr(engine, "L2_TOPK_FILTER_MIN_GALLERY", 1)
    rng = np.random.default_rng(4)
    gc = 100.0 + rng.standard_normal((2304, 64))
    qc = 100.0 + rng.standard_normal((130, 64))
    want = GalleryScorer(gc, measure="l2", filter=False).topk_indices(qc, 10)
    sc = GalleryScorer(gc, measure="l2")
    assert not sc._filter_off
    assert np.array_equal(sc.topk_indices(qc, 10), want) and sc._filter_off   # tried, handed back whole, latched
    assert np.array_equal(sc.topk_indices(qc, 10), want) and sc._filter_off   # the fp64 route from now on
    forced = GalleryScorer(gc, measure="l2", filter=True)                     # filter=True keeps asking
    assert np.array_equal(forced.topk_indices(qc, 10), want)
    # an ordinary gallery: the resident workspace is the filter's, not K18's recommended size beside it
    q, g, _, ref = adversarial(67, (np.float64, np.float64), (1.0, 0.0))
    sc = GalleryScorer(g, measure="l2")
    assert np.array_equal(sc.topk_indices(q, 10), ref[0][:, :10]) and not sc._filter_off
    rq = engine.RowSet(q, with_lo=False)
    assert sc._ws.numel() == engine.l2_topk_workspace(rq, sc._packed, 10)
    off = GalleryScorer(g, measure="l2", filter=False)
    off.topk_indices(q, 10)
    assert off._packed is None and off._ws.numel() == engine.pairwise_topk_workspace(NQ, NG, 10, engine._lib.PW_L2)[1]


# ---- 5. the low-level entry marks exactly the rows it cannot resolve -----------------------------------------------------

def _entry(rq, rg, alpha, beta, k, cap, sample):
    """cmve_l2_topk through the C ABI with a workspace of the test's own: (idx, err, stats, per-query counters).
    cmve.h documents the tail of the workspace: the last 4 * min(1024, round_up128(n_q)) bytes are the int32
    candidate counters of the last round of queries (exact up to cand_cap; above it: overflowed)."""
    import torch
    from cmve import _lib, engine
    dev = rg.device
    nbytes = engine.l2_topk_workspace(rq, rg, k, cap, sample)
    ws = torch.zeros(nbytes // 4, dtype=torch.int32, device=dev)
    idx = torch.full((rq.n, k), -7, dtype=torch.int64, device=dev)
    err = torch.zeros((rq.n, k), dtype=torch.float64, device=dev)
    st = torch.zeros(4, dtype=torch.int64, device=dev)
    rc = _lib.lib.cmve_l2_topk(engine.handle(dev), C.byref(rq.desc), C.byref(rg.desc), alpha, beta, k, cap, sample,
                               engine._ptr(ws), nbytes, engine._ptr(idx), engine._ptr(err), engine._ptr(st))
    assert rc == 0, _lib.lib.cmve_last_error()
    assert rq.n <= 1024  # one round: the counters are this call's
    qc = min(1024, (rq.n + 127) // 128 * 128)
    return idx.cpu().numpy(), err.cpu().numpy(), st.cpu().numpy(), ws[-qc:][:rq.n].cpu().numpy()


def test_low_level_marking(adversarial):
    from cmve import engine
    q, g, _, ref = adversarial(1024, (np.float64, np.float64), (1.0, 0.0))
    rq, rg = engine.RowSet(q, with_lo=False), engine.RowSet(g, with_lo=False)
    big_i, big_e, big, counts = _entry(rq, rg, 1.0, 0.0, 10, 2048, 128)
    tiny_i, tiny_e, tiny, tiny_counts = _entry(rq, rg, 1.0, 0.0, 10, 12, 128)
    no_threshold = big_i[:, 0] == -2
    assert sorted(np.flatnonzero(no_threshold)) == list(SPECIAL_Q) and big[3] == len(SPECIAL_Q)
    # nothing overflows 2048 slots here: the counters are exact, and they add up to the candidates found
    assert (counts[~no_threshold] >= 10).all() and (counts[no_threshold] == 0).all() and counts.sum() == big[1]
    over = counts > 12
    assert 0 < over.sum() < NQ
    # a list that fits has the same counter under the small cap; one that does not stops just past the cap
    assert np.array_equal(tiny_counts[~over], counts[~over]) and (tiny_counts[over] > 12).all()
    assert np.array_equal(tiny_i[:, 0] == -2, over | no_threshold) and tiny[3] == (over | no_threshold).sum()
    assert tiny[2] == counts[~(over | no_threshold)].sum() and tiny[1] == big[1] and tiny[0] == big[0]
    # the rows it does resolve hold the fp64 route's words
    ok = ~(over | no_threshold)
    assert np.array_equal(tiny_i[ok], ref[0][ok, :10]) and np.array_equal(_words(tiny_e[ok]), _words(ref[1][ok, :10]))
    assert np.array_equal(big_i[~no_threshold], ref[0][~no_threshold, :10])
    assert np.array_equal(_words(big_e[~no_threshold]), _words(ref[1][~no_threshold, :10]))
    # the Python wrapper reports the same totals
    _, _, st = engine.l2_topk(rq, rg, 1.0, 0.0, 10, cand_cap=12, sample_rows=128)
    assert [st[n] for n in ("excluded", "candidates", "rescored", "unresolved")] == list(tiny)


# ---- 6. dispatch ------------------------------------------------------------------------------------------------------------

def test_dispatch(adversarial, monkeypatch):
    import torch
    from cmve import _lib, engine
    q, g, _, ref = adversarial(67, (np.float64, np.float64), (1.0, 0.0))
    with pytest.raises(ValueError, match="PW_L2"):
        engine.pairwise_topk(q, g, _lib.PW_L1, 1.0, 0.0, torch.float64, 10, filter=True)
    with pytest.raises(ValueError, match="float64 score words"):
        engine.pairwise_topk(q, g, _lib.PW_L2, 1.0, 0.0, torch.float32, 10, filter=True)
    with pytest.raises(_lib.CmveError, match="alpha"):
        _topk(q, g, 0.0, 0.0, 10, filter=True)
    # below the crossover auto is the fp64 route
    assert not engine.l2_topk_auto(NQ, NG)
    got = _topk(q, g, 1.0, 0.0, 10, return_stats=True)
    assert got[2] is None
    _same(got[:2], (ref[0][:, :10], ref[1][:, :10]))
    assert _topk(q, g, 1.0, 0.0, 10, filter=False, return_stats=True)[2] is None
    # l1, and fp32 score words, never take the filter
    monkeypatch.setattr(engine, "L2_TOPK_FILTER_MIN_Q", 1)
    monkeypatch.setattr(engine, "L2_TOPK_FILTER_MIN_PAIRS", 1)
    assert engine.pairwise_topk(q, g, _lib.PW_L1, 1.0, 0.0, torch.float64, 10, return_stats=True)[2] is None
    assert engine.pairwise_topk(q, g, _lib.PW_L2, 1.0, 0.0, torch.float32, 10, return_stats=True)[2] is None
    # with the thresholds down auto takes the filter: the same words, device tensors when asked
    got = _topk(q, g, 1.0, 0.0, 10, return_stats=True)
    assert got[2] is not None and got[2]["candidates"] > 0
    _same(got[:2], (ref[0][:, :10], ref[1][:, :10]))
    dev_i, dev_e = _topk(q, g, 1.0, 0.0, 10, to_host=False)
    assert dev_i.is_cuda and dev_e.is_cuda
    _same((dev_i.cpu().numpy(), dev_e.cpu().numpy()), (ref[0][:, :10], ref[1][:, :10]))
    # (k above the filter's limit would take the fp64 route, but that limit is K18's own: nothing to dispatch)
    assert engine.L2_TOPK_CAND_MAX == _lib.TOPK_MAX


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing():
    import torch
    from cmve import _lib, engine
    rng = np.random.default_rng(6)
    a, b = rng.standard_normal((40, 67)), rng.standard_normal((50, 67))
    ra, rb = engine.RowSet(a, with_lo=False), engine.RowSet(b, with_lo=False)
    dev = ra.device
    need = engine.l2_topk_workspace(ra, rb, 10, 512, 0)
    ws = torch.empty(need // 8, dtype=torch.int64, device=dev)

    def call(x, y, alpha=1.0, beta=0.0, k=10, cap=512, sample=0, nbytes=need):
        idx = torch.full((40, 10), 77, dtype=torch.int64, device=dev)
        err = torch.full((40, 10), 77.0, dtype=torch.float64, device=dev)
        stats = torch.full((4,), 77, dtype=torch.int64, device=dev)
        rc = _lib.lib.cmve_l2_topk(engine.handle(dev), C.byref(x.desc), C.byref(y.desc), alpha, beta, k, cap, sample,
                                   engine._ptr(ws), nbytes, engine._ptr(idx), engine._ptr(err), engine._ptr(stats))
        msg = _lib.lib.cmve_last_error()
        torch.cuda.synchronize()
        untouched = bool((idx == 77).all()) and bool((err == 77.0).all()) and bool((stats == 77).all())
        return rc, msg, untouched

    rc, msg, untouched = call(ra, rb)
    assert rc == 0 and not untouched                      # the accepted call, for contrast
    for kw, word in (({"k": 0}, b"k must be"), ({"k": -1}, b"k must be"), ({"k": 10, "cap": 9}, b"cand_cap"),
                     ({"cap": 2049}, b"cand_cap"), ({"k": 51}, b"exceeds the gallery"), ({"sample": -1}, b"sample_rows"),
                     ({"alpha": 0.0}, b"alpha"), ({"alpha": float("nan")}, b"alpha"), ({"alpha": float("inf")}, b"alpha"),
                     ({"beta": float("inf")}, b"alpha"), ({"beta": float("nan")}, b"alpha"),
                     ({"nbytes": need - 8}, b"workspace too small")):
        rc, msg, untouched = call(ra, rb, **kw)
        assert rc < 0 and b"cmve_l2_topk" in msg and word in msg and untouched, (kw, msg)
    rc, msg, untouched = call(ra, engine.RowSet(b, with_lo=False, with_f16=False))
    assert rc < 0 and b"cmve_l2_topk" in msg and b"fp16 plane" in msg and untouched
    rc, msg, untouched = call(engine.RowSet(a, with_lo=False, with_f16=False), rb)
    assert rc < 0 and b"fp16 plane" in msg and untouched
    rc, msg, untouched = call(ra, engine.RowSet(b[:, :66], with_lo=False))
    assert rc < 0 and b"cmve_l2_topk" in msg and b"dimensions differ" in msg and untouched
    rc, msg, untouched = call(ra, engine.RowSet(b, eps=1e-12, with_lo=False))
    assert rc < 0 and b"eps" in msg and untouched
    rc, msg, untouched = call(ra, engine.RowSet(b, with_lo=False, raw_rows=True))
    assert rc < 0 and b"CMVE_PACK_RAW" in msg and untouched


# ---- 8. sharded ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cuts", [(0, 260, 520), (0, 520, 520)], ids=["2x260", "520+0"])
def test_sharded_topk_takes_the_filter(adversarial, monkeypatch, cuts):
    import torch
    from cmve import dist as D, engine
    q, g, _, ref = adversarial(67, (np.float64, np.float64), (1.0, 0.0))
    monkeypatch.setattr(engine, "L2_TOPK_FILTER_MIN_Q", 1)
    monkeypatch.setattr(engine, "L2_TOPK_FILTER_MIN_PAIRS", 1)

    def body(r, comm):
        sh = D.ShardedGallery(g[cuts[r]:cuts[r + 1]], offset=cuts[r], n_global=NG, comm=comm, measure="l2")
        q_local = torch.from_numpy(q[150 * r:150 * r + 150].copy()).cuda()
        ids, err = sh.topk(q_local, 10)
        return ids, err, sh._pw_packed is not None, sh.n

    for ids, err, packed, n in D.LocalGroup(2).run(body):
        _same((ids, err), (ref[0][:, :10], ref[1][:, :10]))
        assert packed == (n > 0)
