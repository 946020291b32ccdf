"""K23 on the GPU: the exact top-k of the L1 measures (l1 / l1_norm) through the integer SAD filter.

The contract: ids AND error words equal the fp64 route (``engine.pairwise_topk(filter=False)``, K18) word for word --
ties, near-ties, NaN, inf, overflowing and underflowing rows included; a query the filter cannot resolve is finished
on the fp64 route and reported; the filter must actually filter; and rows clustered far from the origin -- which K20
hands back to the fp64 route -- are resolved, because the grid's offset cancels in the SAD."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NQ, NG = 300, 520          # three query tiles, five gallery tiles, partial tiles both ways
SPECIAL_Q = (10, 11, 12, 13, 14)
SPECIAL_G = (400, 401, 402, 403, 404)
NO_INTERVAL_G = (401, 403, 404)
NO_INTERVAL_Q = (11, 13, 14)  # 1e200 (above the pack's 1e150), inf, NaN; the zero and 1e-200 rows HAVE an L1 interval
AB = [(1.0, 0.0), (None, -1.0), (1.0, -1.0), (None, 0.0)]
AB_IDS = ["l1", "l1_norm", "a1b-1", "a-1/Db0"]
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
    return engine.pairwise_topk(q, g, _lib.PW_L1, alpha, beta, torch.float64, k, **kw)


def _accounted(st, n_q, n_g):
    """Every pair of a resolved query is excluded or a candidate; an unresolved query contributes to neither."""
    assert st["excluded"] + st["candidates"] == (n_q - st["unresolved"]) * n_g, st


@pytest.fixture(scope="module")
def fx(golden):
    return golden("measures_retrieval")


# ---- 1. reference parity -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", ["l1", "l1_norm"])
def test_reference_parity_under_the_filter(fx, m):
    from cmve import engine
    from cmve.linas.inference import GalleryScorer
    sc = GalleryScorer(fx["vid"], measure=m, filter="l1")
    assert isinstance(sc._packed, engine.L1Set) and sc._packed.raw.data_ptr() == sc.gallery.data_ptr()  # no second copy
    assert np.array_equal(sc.topk_indices(fx["cap"], 10), fx["top10_" + m])


# ---- 2. word for word against the fp64 route -----------------------------------------------------------------------------

def _ulps(v, steps):
    for _ in range(steps):
        v = np.nextafter(v, v.dtype.type(np.inf))
    return v


def _adversarial(d, dt_q, dt_g):
    """The recipe of tests/test_gpu_l2_topk.py: Gaussian gallery, queries near gallery rows, exact duplicates 256
    rows apart, a block of 40 1 / 2 / 4-ulp perturbations of one row (and a query whose top-k is that block), zero,
    huge, tiny, inf and NaN rows on both sides."""
    rng = np.random.default_rng(1000 + d)
    g = rng.standard_normal((NG, d))
    pick = rng.integers(0, 200, NQ)
    pick[20] = 7
    q = g[pick] + 0.5 * rng.standard_normal((NQ, d))
    with np.errstate(over="ignore"):
        q, g = q.astype(dt_q), g.astype(dt_g)
        g[256:296] = g[0:40]
        for t in range(40):
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
    """(q, g, L1 distances of all rows) by (d, dtypes); the fp64 route's top-64 by (.., alpha, beta): computed once,
    shared, never changed (the top-k of a smaller k is its prefix)."""
    sets, refs = {}, {}

    def get(d, dts, ab=None):
        if (d, dts) not in sets:
            q, g = _adversarial(d, *dts)
            q64, g64 = q.astype(np.float64), g.astype(np.float64)
            D = np.zeros((NQ, NG))
            with np.errstate(all="ignore"):
                for k0 in range(0, d, 64):
                    D += np.abs(q64[:, None, k0:k0 + 64] - g64[None, :, k0:k0 + 64]).sum(-1)
            sets[(d, dts)] = (q, g, D)
        if ab is None:
            return sets[(d, dts)]
        if (d, dts, ab) not in refs:
            q, g, _ = sets[(d, dts)]
            refs[(d, dts, ab)] = _topk(q, g, ab[0], ab[1], 64, filter=False)
        return sets[(d, dts)] + (refs[(d, dts, ab)],)
    return get


def _precondition(D, alpha, k, sample):
    """A condition on the INPUTS: for every query with an interval, the columns whose exact key s L lies within 1% of
    the k-th smallest key among the first `sample` columns, plus the special rows, number at most 480 (< cand_cap).
    (The interval's half-width is at most 2.6e-4 of the distance here; the maximum over all cases is 200.)"""
    ord_q = np.setdiff1d(np.arange(NQ), NO_INTERVAL_Q)  # (the zero and 1e-200 queries are the filter's too)
    ord_g = np.setdiff1d(np.arange(NG), NO_INTERVAL_G)
    key = np.sign(alpha) * D[np.ix_(ord_q, ord_g)]
    kth = np.sort(key[:, ord_g < sample], axis=1)[:, k - 1]
    count = (key <= (kth + 0.01 * np.abs(kth))[:, None]).sum(1) + len(SPECIAL_G)
    assert count.max() <= 480, count.max()
    return int(count.max())


@pytest.mark.parametrize("ab", AB, ids=AB_IDS)
@pytest.mark.parametrize("dts", DTS, ids=DT_IDS)
@pytest.mark.parametrize("d", [67, 1024])
def test_words_equal_the_fp64_route(adversarial, d, dts, ab):
    from cmve import engine
    ab = (-1.0 / d if ab[0] is None else ab[0], ab[1])
    q, g, D, ref = adversarial(d, dts, ab)
    qd, gd = engine.to_device(q), engine.to_device(g)  # plain rows: the two sets share a grid made from both
    pairs = (NQ - len(NO_INTERVAL_Q)) * NG
    for k, sample in ((1, 128), (10, 128), (1, None), (10, None), (64, None)):
        _precondition(D, ab[0], k, 128 if sample else NG)
        idx, err, st = _topk(qd, gd, *ab, k, filter="l1", cand_cap=512, sample_rows=sample, return_stats=True)
        print("d %d k %d sample %s: %s" % (d, k, sample, st))
        _same((idx, err), (ref[0][:, :k], ref[1][:, :k]))
        # the rows without an interval are unresolved by contract and finished on the fp64 route; the zero and the
        # 1e-200 query (10, 12) are resolved: unlike K20's cosine, the SAD brackets them
        assert st["unresolved"] == len(NO_INTERVAL_Q) == st["fallback_rows"] and not st["fallback"]
        assert st["rescored"] == st["candidates"] and 0 < st["candidates"] < NQ * NG
        assert st["excluded"] + st["candidates"] == pairs
    # the filter filters: with the default sample and k = 10 less than 1/8 of a resolved query's pairs are candidates
    i10, e10, st = _topk(qd, gd, *ab, 10, filter="l1", return_stats=True)
    print("d %d default: %s (%.2f%% candidates)" % (d, st, 100.0 * st["candidates"] / pairs))
    _same((i10, e10), (ref[0][:, :10], ref[1][:, :10]))
    assert st["candidates"] * 8 < pairs and st["excluded"] + st["candidates"] == pairs


def test_which_special_queries_are_resolved(adversarial):
    from cmve import engine
    q, g, _, ref = adversarial(67, (np.float64, np.float64), (1.0, 0.0))
    idx, _, st = engine.l1_topk(*_sets(q, g), 1.0, 0.0, 10, cand_cap=512)
    assert sorted(np.flatnonzero(idx.cpu().numpy()[:, 0] == -2)) == list(NO_INTERVAL_Q) and st["unresolved"] == 3


def _sets(q, g):
    """Both sides as L1Set on one grid made from both."""
    from cmve import engine
    qd, gd = engine.to_device(q), engine.to_device(g)
    grid = engine.l1_grid(gd, engine.l1_grid(qd))
    return engine.L1Set(qd, grid=grid), engine.L1Set(gd, grid=grid)


# ---- 3. a distant cluster resolves -----------------------------------------------------------------------------------------

def test_a_distant_cluster_resolves():
    """Rows clustered far from the origin: K20's cosine brackets nothing there (every query goes back to the fp64
    route); the SAD does not see the offset at all."""
    from cmve import engine
    rng = np.random.default_rng(23)
    g = rng.standard_normal((300, 67)) + 1000.0
    q = g[rng.integers(0, 300, 140)] + 0.5 * rng.standard_normal((140, 67))
    gs = engine.L1Set(g)  # the resident gallery's own grid
    for ab in ((1.0, 0.0), (-1.0 / 67, -1.0)):
        got = _topk(q, gs, *ab, 10, filter="l1", return_stats=True)
        _same(got[:2], _topk(q, g, *ab, 10, filter=False))
        assert got[2]["unresolved"] == 0 and not got[2]["fallback"] and got[2]["excluded"] > 0
        _accounted(got[2], 140, 300)


# ---- 4. off-grid and extreme codes ---------------------------------------------------------------------------------------

def test_extreme_codes_and_clamped_rows():
    from cmve import engine
    rng = np.random.default_rng(22)
    na, nb, d = 140, 150, 1024
    a, b = rng.uniform(-1.0, 1.0, (na, d)), rng.uniform(-1.0, 1.0, (nb, d))
    a[0], b[0] = -3.0, 3.0            # all-lo against all-hi: the SAD is 65535 * 1024 > 2^24
    a[1], b[1] = 3.0, -3.0
    for ab in ((1.0, 0.0), (-1.0 / d, -1.0)):
        got = _topk(a, b, *ab, 10, filter="l1", return_stats=True)
        _same(got[:2], _topk(a, b, *ab, 10, filter=False))
        _accounted(got[2], na, nb)
        if ab[0] < 0:
            assert got[0][0, 0] == 0 and got[0][1, 0] == 1  # l1_norm: the farthest row is the best
    # rows far outside the grid of a resident gallery clamp: their errors are large, their words are the same
    gs = engine.L1Set(b)
    far = a.copy()
    far[3] = 50.0
    far[4, ::2] = -1e6
    for ab in ((1.0, 0.0), (-1.0 / d, -1.0)):
        got = _topk(far, gs, *ab, 10, filter="l1", return_stats=True)
        _same(got[:2], _topk(far, b, *ab, 10, filter=False))
        _accounted(got[2], na, nb)
    # d = 1, with one exact duplicate
    a1, b1 = rng.standard_normal((37, 1)), rng.standard_normal((41, 1))
    b1[5] = a1[3]
    for ab in ((1.0, 0.0), (-1.0, -1.0)):
        got = _topk(a1, b1, *ab, 5, filter="l1", return_stats=True)
        _same(got[:2], _topk(a1, b1, *ab, 5, filter=False))
        _accounted(got[2], 37, 41)
    assert _topk(a1, b1, 1.0, 0.0, 1, filter="l1")[0][3, 0] == 5


# ---- 5. the round loop ---------------------------------------------------------------------------------------------------

def test_two_rounds_and_small_shapes():
    rng = np.random.default_rng(24)
    g = rng.standard_normal((130, 8))
    q = rng.standard_normal((1025, 8))  # two rounds: query 1024 is tile 8 of the tiled codes
    for ab in ((1.0, 0.0), (-1.0 / 8, -1.0)):
        got = _topk(q, g, *ab, 3, filter="l1", return_stats=True)
        _same(got[:2], _topk(q, g, *ab, 3, filter=False))
        assert got[2]["unresolved"] == 0
        _accounted(got[2], 1025, 130)
        one = _topk(q[77:78], g, *ab, 3, filter="l1", return_stats=True)
        _same(one[:2], (got[0][77:78], got[1][77:78]))
        few = _topk(q[:9], g[:5], *ab, 5, filter="l1", return_stats=True)
        _same(few[:2], _topk(q[:9], g[:5], *ab, 5, filter=False))
        assert few[2] is not None and sorted(few[0][0]) == [0, 1, 2, 3, 4]


# ---- 6. ties and degenerate grids ----------------------------------------------------------------------------------------

def test_ties_degenerate_grid_and_empty_sets():
    import torch
    from cmve import _lib, engine
    rng = np.random.default_rng(25)
    g = np.full((40, 16), 2.5)
    q = rng.standard_normal((9, 16))
    gs = engine.L1Set(g)  # hi == lo: the grid falls back to lo = 0, s = 1
    for ab in ((1.0, 0.0), (-1.0 / 16, -1.0)):
        got = _topk(q, gs, *ab, 7, filter="l1", return_stats=True)
        _same(got[:2], _topk(q, g, *ab, 7, filter=False))
        assert (got[0] == np.arange(7)[None, :]).all() and got[2]["unresolved"] == 0  # all words tie: the index decides
    # n_q = 0: empty outputs, zeroed counters
    empty = engine.L1Set(torch.zeros((0, 16), dtype=torch.float64, device=gs.device), grid=gs.grid)
    idx, err, st = engine.l1_topk(empty, gs, 1.0, 0.0, 7)
    assert idx.shape == (0, 7) and err.shape == (0, 7) and st == dict(excluded=0, candidates=0, rescored=0, unresolved=0)
    # k > n_g: clamped by pairwise_topk, refused by the entry
    got = _topk(q, gs, 1.0, 0.0, 400, filter="l1", return_stats=True)
    assert got[0].shape == (9, 40) and got[2] is not None
    _same(got[:2], _topk(q, g, 1.0, 0.0, 400, filter=False))
    with pytest.raises(_lib.CmveError, match="clamp it"):
        engine.l1_topk(engine.L1Set(q, grid=gs.grid), gs, 1.0, 0.0, 41)
    # two sets on different grids
    with pytest.raises(ValueError, match="different grids"):
        engine.l1_topk(engine.L1Set(q), gs, 1.0, 0.0, 7)
    with pytest.raises(ValueError, match="different grids"):
        _topk(engine.L1Set(q), gs, 1.0, 0.0, 7, filter="l1")


# ---- 7. overflowing lists ------------------------------------------------------------------------------------------------

def _entry(qs, gs, alpha, beta, k, cap, sample):
    """engine.l1_topk with a workspace of the test's own: (idx, err, stats list, per-query candidate counters).
    cmve.h documents the tail of the workspace: the last 4 * min(1024, round_up128(n_q)) bytes are the int32
    candidate counters of the last round of queries (exact up to cand_cap; above it: overflowed)."""
    import torch
    from cmve import engine
    nbytes = engine.l1_topk_workspace(qs, gs, k, cap, sample)
    ws = torch.zeros(nbytes // 8, dtype=torch.int64, device=gs.device)
    idx, err, st = engine.l1_topk(qs, gs, alpha, beta, k, cand_cap=cap, sample_rows=sample, ws=ws)
    assert qs.n <= 1024  # one round: the counters are this call's
    qc = min(1024, (qs.n + 127) // 128 * 128)
    counts = ws.view(torch.int32)[-qc:][:qs.n].cpu().numpy()
    return (idx.cpu().numpy(), err.cpu().numpy(),
            [st[n] for n in ("excluded", "candidates", "rescored", "unresolved")], counts)


def test_overflowing_lists_are_marked_and_handed_back(adversarial):
    q, g, _, ref = adversarial(67, (np.float64, np.float64), (1.0, 0.0))
    qs, gs = _sets(q, g)
    big_i, big_e, big, counts = _entry(qs, gs, 1.0, 0.0, 10, 2048, 128)
    tiny_i, tiny_e, tiny, tiny_counts = _entry(qs, gs, 1.0, 0.0, 10, 12, 128)
    no_threshold = big_i[:, 0] == -2
    assert sorted(np.flatnonzero(no_threshold)) == list(NO_INTERVAL_Q) and big[3] == len(NO_INTERVAL_Q)
    # nothing overflows 2048 slots here: the counters are exact, and they add up to the candidates found
    assert (counts[~no_threshold] >= 10).all() and (counts[no_threshold] == 0).all() and counts.sum() == big[1]
    over = counts > 12
    print("lists above 12 candidates: %d of %d" % (over.sum(), NQ))
    assert over.sum() > 0
    # a list that fits has the same counter under the small cap; one that does not stops just past the cap
    assert np.array_equal(tiny_counts[~over], counts[~over]) and (tiny_counts[over] > 12).all()
    assert np.array_equal(tiny_i[:, 0] == -2, over | no_threshold) and tiny[3] == (over | no_threshold).sum()
    assert tiny[2] == counts[~(over | no_threshold)].sum() and tiny[1] == big[1] and tiny[0] == big[0]
    # the rows it does resolve hold the fp64 route's words
    ok = ~(over | no_threshold)
    assert np.array_equal(tiny_i[ok], ref[0][ok, :10]) and np.array_equal(_words(tiny_e[ok]), _words(ref[1][ok, :10]))
    assert np.array_equal(big_i[~no_threshold], ref[0][~no_threshold, :10])
    assert np.array_equal(_words(big_e[~no_threshold]), _words(ref[1][~no_threshold, :10]))
    # a cap at the median list: some lists fit, some do not, and exactly the latter are marked
    mid = max(10, int(np.median(counts[~no_threshold])))
    mid_i, mid_e, mid_st, _ = _entry(qs, gs, 1.0, 0.0, 10, mid, 128)
    fits = ~((counts > mid) | no_threshold)
    assert 0 < fits.sum() < NQ and np.array_equal(mid_i[:, 0] == -2, ~fits) and mid_st[3] == (~fits).sum()
    assert np.array_equal(mid_i[fits], ref[0][fits, :10]) and np.array_equal(_words(mid_e[fits]), _words(ref[1][fits, :10]))
    assert mid_st[2] == counts[fits].sum() and mid_st[1] == big[1] and mid_st[0] == big[0]
    # through pairwise_topk: more than a quarter unresolved, so the whole call is handed back -- and is exact
    assert (over | no_threshold).sum() > NQ // 4
    got = _topk(qs, gs, 1.0, 0.0, 10, filter="l1", cand_cap=12, sample_rows=128, return_stats=True)
    _same(got[:2], (ref[0][:, :10], ref[1][:, :10]))
    assert got[2]["fallback"] and got[2]["fallback_rows"] == NQ and got[2]["unresolved"] == tiny[3]


# ---- 8. dispatch and the scorer --------------------------------------------------------------------------------------------

def test_dispatch_and_the_scorer(adversarial, monkeypatch):
    import torch
    from cmve import _lib, engine
    from cmve.linas.inference import GalleryScorer
    q, g, _, ref = adversarial(67, (np.float64, np.float64), (1.0, 0.0))
    # while the rule says no, auto is the fp64 route (and no pack is made)
    for name in ("L1_TOPK_FILTER_MIN_Q", "L1_TOPK_FILTER_MIN_PLAIN_PAIRS", "L1_TOPK_FILTER_MIN_PAIRS",
                 "L1_TOPK_FILTER_MIN_GALLERY"):
        monkeypatch.setattr(engine, name, None)
    assert _topk(q, g, 1.0, 0.0, 10, return_stats=True)[2] is None
    assert GalleryScorer(g, measure="l1")._packed is None
    assert _topk(q, g, 1.0, 0.0, 10, filter=False, return_stats=True)[2] is None
    # with the thresholds down auto takes the filter: the same words, device tensors when asked
    monkeypatch.setattr(engine, "L1_TOPK_FILTER_MIN_Q", 1)
    monkeypatch.setattr(engine, "L1_TOPK_FILTER_MIN_PLAIN_PAIRS", 1)  # plain rows
    monkeypatch.setattr(engine, "L1_TOPK_FILTER_MIN_PAIRS", 1)        # a packed gallery: the scorer's
    got = _topk(q, g, 1.0, 0.0, 10, return_stats=True)
    assert got[2] is not None and got[2]["candidates"] > 0
    _same(got[:2], (ref[0][:, :10], ref[1][:, :10]))
    dev_i, dev_e = _topk(q, g, 1.0, 0.0, 10, to_host=False)
    assert dev_i.is_cuda and dev_e.is_cuda
    _same((dev_i.cpu().numpy(), dev_e.cpu().numpy()), (ref[0][:, :10], ref[1][:, :10]))
    # fp32 score words and the Euclidean metric never take the SAD filter
    assert engine.pairwise_topk(q, g, _lib.PW_L1, 1.0, 0.0, torch.float32, 10, return_stats=True)[2] is None
    # the scorer: the gallery is packed ONCE (on its own grid), the workspace is the filter's
    packs = []
    real = engine.L1Set

    class Counting(real):
        def __init__(self, x, grid=None, device=None):
            packs.append(grid is None)
            super().__init__(x, grid=grid, device=device)

    monkeypatch.setattr(engine, "L1Set", Counting)
    sc = GalleryScorer(g, measure="l1")
    assert isinstance(sc._packed, real) and sc._packed.raw.data_ptr() == sc.gallery.data_ptr()
    for _ in range(2):
        assert np.array_equal(sc.topk_indices(q, 10), ref[0][:, :10]) and not sc._filter_off
    assert packs == [True, False, False]  # the gallery once, the queries per call on its grid
    assert sc._ws.numel() == engine.l1_topk_workspace(NQ, NG, 10)
    off = GalleryScorer(g, measure="l1", filter=False)
    assert np.array_equal(off.topk_indices(q, 10), ref[0][:, :10])
    assert off._packed is None and off._ws.numel() == engine.pairwise_topk_workspace(NQ, NG, 10, _lib.PW_L1)[1]
    ignored = GalleryScorer(g, measure="l1_norm", filter=True)  # filter=True speaks for the Euclidean measures alone
    assert ignored._packed is None


# ---- 9. refusals -----------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing():
    import torch
    from cmve import _lib, engine
    rng = np.random.default_rng(6)
    a, b = rng.standard_normal((40, 67)), rng.standard_normal((50, 67))
    qs, gs = _sets(a, b)
    dev = gs.device
    need = engine.l1_topk_workspace(40, 50, 10, 512, 0)
    ws = torch.empty(need // 8, dtype=torch.int64, device=dev)
    P = engine._ptr
    base = dict(h=engine.handle(dev), Q=P(qs.raw), qdt=_lib.CMVE_F64, ldq=67, nq=40, qc=P(qs.codes), qe=P(qs.err),
                G=P(gs.raw), gdt=_lib.CMVE_F64, ldg=67, ng=50, gc=P(gs.codes), ge=P(gs.err), d=67, grid=P(gs.grid),
                alpha=1.0, beta=0.0, k=10, cap=512, sample=0, ws=P(ws), nbytes=need, idx=True, err=True, stats=True)

    def call(**kw):
        a_ = dict(base, **kw)
        idx = torch.full((40, 10), 77, dtype=torch.int64, device=dev)
        err = torch.full((40, 10), 77.0, dtype=torch.float64, device=dev)
        stats = torch.full((4,), 77, dtype=torch.int64, device=dev)
        rc = _lib.lib.cmve_l1_topk(a_["h"], a_["Q"], a_["qdt"], a_["ldq"], a_["nq"], a_["qc"], a_["qe"], a_["G"],
                                   a_["gdt"], a_["ldg"], a_["ng"], a_["gc"], a_["ge"], a_["d"], a_["grid"],
                                   a_["alpha"], a_["beta"], a_["k"], a_["cap"], a_["sample"], a_["ws"], a_["nbytes"],
                                   P(idx) if a_["idx"] else None, P(err) if a_["err"] else None,
                                   P(stats) if a_["stats"] else None)
        msg = _lib.lib.cmve_last_error()
        torch.cuda.synchronize()
        untouched = bool((idx == 77).all()) and bool((err == 77.0).all()) and bool((stats == 77).all())
        return rc, msg, untouched

    rc, msg, untouched = call()
    assert rc == 0 and not untouched                      # the accepted call, for contrast
    odd = ws.view(torch.uint8)[4:]                       # a workspace that is not 8-byte aligned
    for kw, word in (({"h": None}, b"NULL"), ({"Q": None}, b"NULL"), ({"G": None}, b"NULL"), ({"stats": False}, b"NULL"),
                     ({"qc": None}, b"codes"), ({"ge": None}, b"codes"), ({"grid": None}, b"grid"),
                     ({"alpha": 0.0}, b"alpha"), ({"alpha": float("nan")}, b"alpha"), ({"alpha": float("inf")}, b"alpha"),
                     ({"beta": float("inf")}, b"alpha"), ({"beta": float("nan")}, b"alpha"),
                     ({"d": 0}, b"d must be"), ({"d": 65537, "ldq": 65537, "ldg": 65537}, b"d must be"),
                     ({"nq": 1 << 31}, b"bad shape"), ({"ng": 1 << 31}, b"bad shape"), ({"ldq": 66}, b"bad shape"),
                     ({"qdt": _lib.CMVE_BF16}, b"CMVE_F32/CMVE_F64"),
                     ({"k": 0}, b"k must be"), ({"k": -1}, b"k must be"), ({"k": 51}, b"clamp it"),
                     ({"k": 10, "cap": 9}, b"cand_cap"), ({"cap": 2049}, b"cand_cap"), ({"sample": -1}, b"sample_rows"),
                     ({"sample": 1 << 31}, b"sample_rows"),
                     ({"nbytes": need - 8}, b"workspace too small"), ({"ws": None}, b"workspace too small"),
                     ({"ws": engine._ptr(odd)}, b"8-byte aligned"),
                     ({"idx": False}, b"NULL output"), ({"err": False}, b"NULL output")):
        rc, msg, untouched = call(**kw)
        assert rc < 0 and b"cmve_l1_topk" in msg and word in msg and untouched, (kw, msg)
