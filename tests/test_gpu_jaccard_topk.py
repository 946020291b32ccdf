"""K25 on the GPU: the exact top-k under jaccard (float32 score words) through the integer SAD filter.

The contract: ids AND error words equal the K18 route (``engine.pairwise_topk(filter=False)``) word for word -- float32
ties, near-ties, NaN, inf, overflowing and underflowing rows included; a query the filter cannot resolve is finished
on the K18 route WITH FLOAT32 WORDS and reported; the filter must actually filter.  Which queries the device leaves
unresolved is derived from the numpy port of its decision (tests/jaccard_topk_model.py), not written down here."""
import numpy as np
import pytest

import jaccard_topk_model as M

pytestmark = pytest.mark.gpu

NQ, NG = M.NQ, M.NG
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
    return engine.pairwise_topk(q, g, _lib.PW_JACCARD, alpha, beta, torch.float32, k, **kw)


def _accounted(st, n_q, n_g):
    """Every pair of a resolved query is excluded or a candidate; an unresolved query contributes to neither."""
    assert st["excluded"] + st["candidates"] == (n_q - st["unresolved"]) * n_g, st
    assert st["rescored"] <= st["candidates"]


def _sets(q, g):
    """Both sides as JaccardSet on one grid made from both."""
    from cmve import engine
    qd, gd = engine.to_device(q), engine.to_device(g)
    grid = engine.l1_grid(gd, engine.l1_grid(qd))
    return engine.JaccardSet(qd, grid=grid), engine.JaccardSet(gd, grid=grid)


@pytest.fixture(scope="module")
def fx(golden):
    return golden("measures_retrieval")


# ---- 1. reference parity -----------------------------------------------------------------------------------------------

def test_reference_parity_under_the_filter(fx):
    from cmve import engine
    from cmve.linas.inference import GalleryScorer
    sc = GalleryScorer(fx["vid_p"], measure="jaccard", filter="jaccard")
    assert isinstance(sc._packed, engine.JaccardSet) and sc._packed.raw.data_ptr() == sc.gallery.data_ptr()
    assert np.array_equal(sc.topk_indices(fx["cap_p"], 10), fx["top10_jaccard"])


# ---- 2. word for word against the K18 route ------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def adversarial():
    """By (nonneg, d, dtypes): K24's adversarial rows in their storage dtypes and the model's intervals; with (alpha,
    beta) also the K18 route's top-64 -- computed once, shared, never changed (a smaller k is its prefix)."""
    sets, refs = {}, {}

    def get(nonneg, d, dts, ab=None):
        key = (nonneg, d, dts)
        if key not in sets:
            a, b = M.rows(d, dts, nonneg)
            with np.errstate(over="ignore"):
                sets[key] = (a.astype(dts[0]), b.astype(dts[1]), a, b, M.intervals(a, b))
        if ab is None:
            return sets[key]
        if key + (ab,) not in refs:
            refs[key + (ab,)] = _topk(sets[key][0], sets[key][1], ab[0], ab[1], 64, filter=False)
        return sets[key] + (refs[key + (ab,)],)
    return get


@pytest.mark.parametrize("ab", M.AB, ids=["a-1b0", "a1b0", "a-.5b.25"])
@pytest.mark.parametrize("dts", DTS, ids=DT_IDS)
@pytest.mark.parametrize("d", [67, 1024])
@pytest.mark.parametrize("nonneg", [True, False], ids=["nonneg", "signed"])
def test_words_equal_the_k18_route(adversarial, nonneg, d, dts, ab):
    from cmve import engine
    q, g, a64, b64, iv, ref = adversarial(nonneg, d, dts, ab)
    qd, gd = engine.to_device(q), engine.to_device(g)  # plain rows: the two sets share a grid made from both
    assert ref[1].dtype == np.float64 and np.array_equal(_words(ref[1]), _words(ref[1].astype(np.float32).astype(np.float64)))
    for k, sample in M.K_SAMPLE:
        thr, _, cand = M.decide(a64, b64, ab[0], ab[1], k, sample, iv)
        want_un = np.flatnonzero(M.unresolved(thr, cand, k, 512))
        assert want_un.tolist() == ([10, 11, 12, 13, 14] if nonneg else [11, 13, 14])
        ordinary = np.setdiff1d(np.arange(NQ), want_un)
        assert cand[ordinary].sum(axis=1).max() <= 480  # the precondition: cand_cap = 512 cannot hide an overflow
        idx, err, st = _topk(qd, gd, *ab, k, filter="jaccard", cand_cap=512, sample_rows=sample, return_stats=True)
        print("d %d k %d sample %s: %s" % (d, k, sample, st))
        _same((idx, err), (ref[0][:, :k], ref[1][:, :k]))
        assert st["unresolved"] == len(want_un) == st["fallback_rows"] and not st["fallback"]
        # excluded + candidates = the pairs of the queries that have a threshold, rescored = the candidates of the
        # resolved ones: on signed rows the unresolved queries are exactly those without a threshold, on non-negative
        # rows queries 10 and 12 have one, count every column a candidate and overflow cand_cap
        over = np.setdiff1d(want_un, np.flatnonzero(np.isnan(thr)))
        assert over.tolist() == ([10, 12] if nonneg else []) and cand[over].all()
        assert st["excluded"] + st["candidates"] == (NQ - st["unresolved"] + len(over)) * NG
        assert st["rescored"] == st["candidates"] - len(over) * NG and 0 < st["rescored"] < NQ * NG
    # the filter filters: with the default sample and k = 10 less than 1/8 of the resolved queries' pairs are candidates
    entry = engine.jaccard_topk(*_sets(q, g), ab[0], ab[1], 10, cand_cap=512)
    un = np.flatnonzero(entry[0].cpu().numpy()[:, 0] == -2)
    assert un.tolist() == want_un.tolist()
    i10, e10, st = _topk(qd, gd, *ab, 10, filter="jaccard", cand_cap=1024, return_stats=True)
    _same((i10, e10), (ref[0][:, :10], ref[1][:, :10]))
    pairs = (NQ - st["unresolved"]) * NG
    print("d %d default: %s (%.2f%% candidates)" % (d, st, 100.0 * st["candidates"] / pairs))
    assert st["unresolved"] == 3 and st["excluded"] + st["candidates"] == pairs and st["rescored"] == st["candidates"]
    assert st["candidates"] * 8 < pairs


# ---- 3. ties -------------------------------------------------------------------------------------------------------------

def test_the_all_tie_query_resolves_inside_the_filter(adversarial):
    """Non-negative rows: every word of the zero query is alpha * 0 + beta except the NaN of a zero gallery row
    (0 / 0: row 400), which sorts last.  k = 512 is the most the filter can resolve -- the five special gallery rows
    have no interval against the zero query, so at most 515 bounds of the sample are finite -- and shows the order:
    the ids are the first 512 columns that are not NaN, in index order, so 400 < 512 is passed over."""
    from cmve import engine
    q, g, *_ = adversarial(True, 67, DTS[0])
    qs, gs = _sets(q, g)
    for ab in M.AB:
        idx, err, st = engine.jaccard_topk(qs, gs, ab[0], ab[1], 512, cand_cap=1024)
        idx, err = idx.cpu().numpy(), err.cpu().numpy()
        want = _topk(q[10:11], g, *ab, NG, filter=False)
        assert idx[10, 0] != -2 and np.array_equal(idx[10], want[0][0, :512])
        assert np.array_equal(_words(err[10]), _words(want[1][0, :512]))
        assert idx[10].tolist() == sorted(idx[10].tolist()) and 400 not in idx[10] and len(np.unique(err[10])) == 1
        nan_cols = np.flatnonzero(np.isnan(want[1][0]))
        assert 400 in want[0][0, -len(nan_cols):] and np.isnan(want[1][0, -len(nan_cols):]).all()  # K18: NaN last


def test_the_float32_tie_block(adversarial):
    """Query 20's best rows are row 7, its duplicate 263 and the 40 perturbed copies 300..339: many collapse to one
    float32 word, and the index decides."""
    for nonneg in (True, False):
        for dts in (DTS[0], DTS[1]):
            q, g, *_ = adversarial(nonneg, 67, dts)
            for ab in M.AB:
                want = _topk(q[20:21], g, *ab, 64, filter=False)
                got = _topk(q[20:21], g, *ab, 64, filter="jaccard", return_stats=True)
                _same(got[:2], want)
                assert got[2]["unresolved"] == 0
                if nonneg and ab[0] < 0:  # -jaccard: the block is the best; float32 ties inside it
                    assert set(want[0][0, :42].tolist()) == set(range(300, 340)) | {7, 263}
                    assert len(np.unique(want[1][0, :42])) < 42


# ---- 4. the round loop, small shapes, degenerate grids ---------------------------------------------------------------------

def test_two_rounds_and_small_shapes():
    rng = np.random.default_rng(24)
    g = np.abs(rng.standard_normal((130, 8))).astype(np.float32)
    q = np.abs(rng.standard_normal((1025, 8))).astype(np.float32)  # two rounds: query 1024 is tile 8 of the codes
    for ab in M.AB:
        got = _topk(q, g, *ab, 3, filter="jaccard", return_stats=True)
        _same(got[:2], _topk(q, g, *ab, 3, filter=False))
        assert got[2]["unresolved"] == 0
        _accounted(got[2], 1025, 130)
        one = _topk(q[77:78], g, *ab, 3, filter="jaccard", return_stats=True)
        _same(one[:2], (got[0][77:78], got[1][77:78]))
        few = _topk(q[:9], g[:5], *ab, 5, filter="jaccard", return_stats=True)  # n_g = k
        _same(few[:2], _topk(q[:9], g[:5], *ab, 5, filter=False))
        assert few[2] is not None and sorted(few[0][0]) == [0, 1, 2, 3, 4]


def test_degenerate_grid_and_empty_sets():
    import torch
    from cmve import _lib, engine
    rng = np.random.default_rng(25)
    g = np.full((40, 16), 2.5, np.float32)
    q = np.abs(rng.standard_normal((9, 16))).astype(np.float32)
    gs = engine.JaccardSet(g)  # hi == lo: the grid falls back to lo = 0, s = 1
    for ab in M.AB:
        got = _topk(q, gs, *ab, 7, filter="jaccard", return_stats=True)
        _same(got[:2], _topk(q, g, *ab, 7, filter=False))
        assert (got[0] == np.arange(7)[None, :]).all()  # all words of a query tie: the index decides
    zero = torch.zeros((0, 16), dtype=torch.float32, device=gs.device)
    # n_q = 0: empty outputs, zeroed counters
    idx, err, st = engine.jaccard_topk(engine.JaccardSet(zero, grid=gs.grid), gs, 1.0, 0.0, 7)
    assert idx.shape == (0, 7) and err.shape == (0, 7) and st == dict(excluded=0, candidates=0, rescored=0, unresolved=0)
    # n_g = 0: k is clamped to nothing by pairwise_topk, the entry refuses k > n_g
    got = _topk(q, zero, 1.0, 0.0, 7, filter="jaccard", return_stats=True)
    assert got[0].shape == (9, 0) and got[2] is None
    # k > n_g: clamped by pairwise_topk, refused by the entry
    got = _topk(q, gs, 1.0, 0.0, 400, filter="jaccard", return_stats=True)
    assert got[0].shape == (9, 40) and got[2] is not None
    _same(got[:2], _topk(q, g, 1.0, 0.0, 400, filter=False))
    with pytest.raises(_lib.CmveError, match="clamp it"):
        engine.jaccard_topk(engine.JaccardSet(q, grid=gs.grid), gs, 1.0, 0.0, 41)
    # two sets on different grids; packs of the wrong kind
    with pytest.raises(ValueError, match="different grids"):
        engine.jaccard_topk(engine.JaccardSet(q), gs, 1.0, 0.0, 7)
    with pytest.raises(TypeError, match="JaccardSet"):
        _topk(q, engine.L1Set(g), 1.0, 0.0, 7, filter="jaccard")
    with pytest.raises(TypeError, match="RowSet"):
        _topk(q, engine.RowSet(g, with_lo=False), 1.0, 0.0, 7, filter="jaccard")


def test_extreme_codes_and_clamped_rows():
    from cmve import engine
    rng = np.random.default_rng(22)
    na, nb, d = 140, 150, 1024
    a, b = rng.uniform(-1.0, 1.0, (na, d)), rng.uniform(-1.0, 1.0, (nb, d))
    a[0], b[0] = -3.0, 3.0            # all-lo against all-hi: the SAD is 65535 * 1024 > 2^24
    a[1], b[1] = 3.0, -3.0
    for x, y in ((a, b), (np.abs(a), np.abs(b))):
        for ab in M.AB:
            got = _topk(x, y, *ab, 10, filter="jaccard", return_stats=True)
            _same(got[:2], _topk(x, y, *ab, 10, filter=False))
            _accounted(got[2], na, nb)
    # rows far outside the grid of a resident gallery clamp: their errors are large, their words are the same
    gs = engine.JaccardSet(np.abs(b).astype(np.float32))
    far = np.abs(a).astype(np.float32)
    far[3] = 50.0
    far[4, ::2] = 1e6
    for ab in M.AB:
        got = _topk(far, gs, *ab, 10, filter="jaccard", return_stats=True)
        _same(got[:2], _topk(far, gs.raw, *ab, 10, filter=False))
        _accounted(got[2], na, nb)
    # d = 1, with one exact duplicate
    a1, b1 = np.abs(rng.standard_normal((37, 1))) + 0.1, np.abs(rng.standard_normal((41, 1))) + 0.1
    b1[5] = a1[3]
    for ab in M.AB:
        got = _topk(a1, b1, *ab, 5, filter="jaccard", return_stats=True)
        _same(got[:2], _topk(a1, b1, *ab, 5, filter=False))
        _accounted(got[2], 37, 41)
    assert _topk(a1, b1, -1.0, 0.0, 1, filter="jaccard")[0][3, 0] == 5  # jaccard 1: the best under -jaccard


# ---- 5. overflowing lists ------------------------------------------------------------------------------------------------

def test_overflowing_lists_are_marked_and_handed_back(adversarial):
    from cmve import engine
    q, g, _, _, _, ref = adversarial(False, 67, DTS[0], (-1.0, 0.0))
    qs, gs = _sets(q, g)
    big = engine.jaccard_topk(qs, gs, -1.0, 0.0, 10, cand_cap=2048, sample_rows=128)
    tiny = engine.jaccard_topk(qs, gs, -1.0, 0.0, 10, cand_cap=10, sample_rows=128)
    big_i, tiny_i, tiny_e = big[0].cpu().numpy(), tiny[0].cpu().numpy(), tiny[1].cpu().numpy()
    no_thr = big_i[:, 0] == -2
    assert np.flatnonzero(no_thr).tolist() == [11, 13, 14] and big[2]["unresolved"] == 3
    marked = tiny_i[:, 0] == -2
    assert (marked | ~no_thr).all() and marked.sum() > NQ // 4 and tiny[2]["unresolved"] == marked.sum()
    assert tiny[2]["candidates"] == big[2]["candidates"] and tiny[2]["excluded"] == big[2]["excluded"]
    assert tiny[2]["rescored"] == 10 * int((~marked).sum())  # a list that fits cand_cap = k holds exactly k
    ok = ~marked
    assert np.array_equal(tiny_i[ok], ref[0][ok, :10]) and np.array_equal(_words(tiny_e[ok]), _words(ref[1][ok, :10]))
    # through pairwise_topk: more than L2_TOPK_MAX_UNRESOLVED of the queries, so the whole call is handed back
    assert marked.sum() > engine.L2_TOPK_MAX_UNRESOLVED * NQ
    got = _topk(qs, gs, -1.0, 0.0, 10, filter="jaccard", cand_cap=10, sample_rows=128, return_stats=True)
    _same(got[:2], (ref[0][:, :10], ref[1][:, :10]))
    assert got[2]["fallback"] and got[2]["fallback_rows"] == NQ and got[2]["unresolved"] == marked.sum()
    # a few unresolved rows are re-run alone, with float32 words
    some = _topk(qs, gs, -1.0, 0.0, 10, filter="jaccard", return_stats=True)
    _same(some[:2], (ref[0][:, :10], ref[1][:, :10]))
    assert some[2]["fallback_rows"] == 3 and not some[2]["fallback"]


# ---- 6. dispatch and the scorer --------------------------------------------------------------------------------------------

AUTO = ("JACCARD_TOPK_FILTER_MIN_Q", "JACCARD_TOPK_FILTER_MIN_PLAIN_PAIRS", "JACCARD_TOPK_FILTER_MIN_PAIRS",
        "JACCARD_TOPK_FILTER_MIN_GALLERY")


def test_dispatch(adversarial, monkeypatch):
    import torch
    from cmve import _lib, engine
    q, g, _, _, _, ref = adversarial(False, 67, DTS[0], (-1.0, 0.0))
    want = (ref[0][:, :10], ref[1][:, :10])
    for name in AUTO:
        monkeypatch.setattr(engine, name, None)
    gs = engine.JaccardSet(g)
    assert _topk(q, g, -1.0, 0.0, 10, return_stats=True)[2] is None   # never while the constants are None
    assert _topk(q, gs, -1.0, 0.0, 10, return_stats=True)[2] is None
    assert _topk(q, g, -1.0, 0.0, 10, filter=False, return_stats=True)[2] is None
    monkeypatch.setattr(engine, "JACCARD_TOPK_FILTER_MIN_PAIRS", 1)   # a packed gallery
    assert _topk(q, g, -1.0, 0.0, 10, return_stats=True)[2] is None
    got = _topk(q, gs, -1.0, 0.0, 10, return_stats=True)
    assert got[2] is not None and got[2]["candidates"] > 0
    _same(got[:2], want)
    monkeypatch.setattr(engine, "JACCARD_TOPK_FILTER_MIN_Q", 1)
    monkeypatch.setattr(engine, "JACCARD_TOPK_FILTER_MIN_PLAIN_PAIRS", 1)  # plain rows
    got = _topk(q, g, -1.0, 0.0, 10, return_stats=True)
    assert got[2] is not None and got[2]["candidates"] > 0
    _same(got[:2], want)
    dev_i, dev_e = _topk(q, g, -1.0, 0.0, 10, to_host=False)
    assert dev_i.is_cuda and dev_e.is_cuda
    _same((dev_i.cpu().numpy(), dev_e.cpu().numpy()), want)
    # float64 words under jaccard, and the other measures, never take it
    assert engine.pairwise_topk(q, g, _lib.PW_JACCARD, -1.0, 0.0, torch.float64, 10, return_stats=True)[2] is None
    assert engine.pairwise_topk(q, g, _lib.PW_L1, 1.0, 0.0, torch.float32, 10, return_stats=True)[2] is None


def test_the_scorer_latch_and_filter_false(adversarial, monkeypatch):
    from cmve import _lib, engine
    from cmve.linas.inference import GalleryScorer
    q, g, _, _, _, ref = adversarial(False, 67, DTS[0], (-1.0, 0.0))
    for name in AUTO:
        monkeypatch.setattr(engine, name, None)
    assert GalleryScorer(g, measure="jaccard")._packed is None        # the rule could take no call: no pack
    off = GalleryScorer(g, measure="jaccard", filter=False)
    assert np.array_equal(off.topk_indices(q, 10), ref[0][:, :10])
    assert off._packed is None and off._ws.numel() == engine.pairwise_topk_workspace(NQ, NG, 10, _lib.PW_JACCARD)[1]
    assert GalleryScorer(g, measure="jaccard", filter=True)._packed is None  # True speaks for the Euclidean measures
    monkeypatch.setattr(engine, "JACCARD_TOPK_FILTER_MIN_PAIRS", 1)
    calls = []
    real = engine.jaccard_topk
    monkeypatch.setattr(engine, "jaccard_topk", lambda *x, **kw: calls.append(1) or real(*x, **kw))
    sc = GalleryScorer(g, measure="jaccard")
    assert isinstance(sc._packed, engine.JaccardSet) and sc._packed.raw.data_ptr() == sc.gallery.data_ptr()
    for _ in range(2):
        assert np.array_equal(sc.topk_indices(q, 10), ref[0][:, :10]) and not sc._filter_off
    assert len(calls) == 2 and sc._ws.numel() == engine.jaccard_topk_workspace(NQ, NG, 10)
    # a call the filter hands back whole latches the automatic filter off; a forced scorer keeps asking
    monkeypatch.setattr(engine, "L2_TOPK_MAX_UNRESOLVED", 0.0)
    assert np.array_equal(sc.topk_indices(q, 10), ref[0][:, :10]) and sc._filter_off and len(calls) == 3
    assert np.array_equal(sc.topk_indices(q, 10), ref[0][:, :10]) and len(calls) == 3
    forced = GalleryScorer(g, measure="jaccard", filter="jaccard")
    for n in (4, 5):
        assert np.array_equal(forced.topk_indices(q, 10), ref[0][:, :10]) and len(calls) == n


# ---- 7. refusals and the packs ---------------------------------------------------------------------------------------------

def test_refusals_launch_nothing():
    import torch
    from cmve import _lib, engine
    rng = np.random.default_rng(6)
    a, b = rng.standard_normal((40, 67)), rng.standard_normal((50, 67))
    qs, gs = _sets(a, b)
    dev = gs.device
    need = engine.jaccard_topk_workspace(40, 50, 10, 512, 0)
    ws = torch.empty(need // 8, dtype=torch.int64, device=dev)
    P = engine._ptr
    base = dict(h=engine.handle(dev), Q=P(qs.raw), qdt=_lib.CMVE_F64, ldq=67, nq=40, qc=P(qs.codes), qe=P(qs.err),
                qq=P(qs.qsum), qa=P(qs.asum), G=P(gs.raw), gdt=_lib.CMVE_F64, ldg=67, ng=50, gc=P(gs.codes),
                ge=P(gs.err), gq=P(gs.qsum), ga=P(gs.asum), d=67, grid=P(gs.grid), alpha=1.0, beta=0.0, k=10, cap=512,
                sample=0, ws=P(ws), nbytes=need, idx=True, err=True, stats=True)

    def call(**kw):
        a_ = dict(base, **kw)
        idx = torch.full((40, 10), 77, dtype=torch.int64, device=dev)
        err = torch.full((40, 10), 77.0, dtype=torch.float64, device=dev)
        stats = torch.full((4,), 77, dtype=torch.int64, device=dev)
        rc = _lib.lib.cmve_jaccard_topk(a_["h"], a_["Q"], a_["qdt"], a_["ldq"], a_["nq"], a_["qc"], a_["qe"], a_["qq"],
                                        a_["qa"], a_["G"], a_["gdt"], a_["ldg"], a_["ng"], a_["gc"], a_["ge"],
                                        a_["gq"], a_["ga"], a_["d"], a_["grid"], a_["alpha"], a_["beta"], a_["k"],
                                        a_["cap"], a_["sample"], a_["ws"], a_["nbytes"],
                                        P(idx) if a_["idx"] else None, P(err) if a_["err"] else None,
                                        P(stats) if a_["stats"] else None)
        msg = _lib.lib.cmve_last_error()
        torch.cuda.synchronize()
        untouched = bool((idx == 77).all()) and bool((err == 77.0).all()) and bool((stats == 77).all())
        return rc, msg, untouched

    rc, msg, untouched = call()
    assert rc == 0 and not untouched                      # the accepted call, for contrast
    odd = ws.view(torch.uint8)[4:]                       # a workspace that is not 8-byte aligned
    sums = b"cmve_jaccard_rowsums"
    for kw, word in (({"h": None}, b"NULL"), ({"Q": None}, b"NULL"), ({"G": None}, b"NULL"), ({"stats": False}, b"NULL"),
                     ({"qc": None}, b"codes"), ({"ge": None}, b"codes"), ({"grid": None}, b"grid"),
                     ({"qq": None}, sums), ({"qa": None}, sums), ({"gq": None}, sums), ({"ga": None}, sums),
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
        assert rc < 0 and b"cmve_jaccard_topk" in msg and word in msg and untouched, (kw, msg)


def test_row_sums_of_the_packed_sets_are_the_stored_codes(adversarial):
    import torch
    q, g, *_ = adversarial(True, 67, DTS[0])
    for s in _sets(q, g):
        codes = s.codes.view(torch.int16).cpu().numpy().view(np.uint16).astype(np.int64)
        assert codes.sum() == int(s.qsum[:s.n].sum())
