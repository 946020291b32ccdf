"""ShardedGallery(measure="jaccard", filter="jaccard") on the GPU: the sharded evaluation's count pass through the
integer SAD filter under jaccard (K24) and the shard's top-k through K25, the shards in ONE process through LocalGroup
(one thread + HIP stream each), as tests/test_gpu_dist_l1_filter.py does for the L1 measures.

The contract is K21's: every method returns what the K18 route (filter=False) returns, word for word, whatever each
shard's band list does; ``filter_stats`` says what each shard's filter did; the methods that end on the host grow a
shard's band list; the shard is packed once, lazily, as a JaccardSet on its own grid, and the count and the top-k share
that pack."""
import numpy as np
import pytest

import test_jaccard_filter_host as K24

pytestmark = pytest.mark.gpu

NA, NB = K24.NA, K24.NB
GOLDEN_CUTS = (0, 5, 5, 20, 37, 141)        # an empty shard and four uneven ones
ADVERSARIAL_CUTS = (0, 128, 128, 391, 520)  # an empty shard, a shard of exactly one tile, two partial ones


@pytest.fixture(scope="module")
def fx(golden):
    return golden("measures_retrieval")


@pytest.fixture(scope="module")
def gts(fx):
    from oracle import retrieval as R
    return R.get_gt(list(fx["video_ids"]), list(fx["caption_ids"]))  # (v2t list, t2v dict)


@pytest.fixture(scope="module")
def adversarial():
    """K24's adversarial float32 rows and GT lists, non-negative (the measure's natural inputs)."""
    a, b, rows, cols = K24._adversarial(67, np.float32, np.float32, True)
    return a.astype(np.float32), b.astype(np.float32), rows, cols


def _slices(n, world, even):
    c = np.linspace(0, n, world + 1).astype(int)
    if not even and world > 1:
        c[1:-1] += 3
    return c


def _accounted(st, pairs):
    """decided + band = pairs and rescored = band on a shard whose list held its band (an empty shard: all zero)."""
    assert st is not None and set(st) == {"decided", "band", "rescored", "overflow", "fallback"}
    assert st["fallback"] == (st["overflow"] == 1)
    assert st["overflow"] == 1 or (st["decided"] + st["band"] == pairs and st["rescored"] == st["band"])


def _solo(vid, **kw):
    """A world-1 shard (no process group: every collective is a no-op)."""
    from cmve import dist as D
    return D.ShardedGallery(vid, offset=0, n_global=vid.shape[0], measure="jaccard", **kw)


def _whole_gallery_topk(a, b, k):
    from cmve import engine
    from cmve.linas.evaluation import measure_spec
    metric, alpha, beta, _, sc_dt = measure_spec("jaccard", b.shape[1])
    return engine.pairwise_topk(a, b, metric, alpha, beta, sc_dt, k, filter=False)


# ---- golden parity ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cuts", [(0, 141), GOLDEN_CUTS], ids=lambda c: "-".join(map(str, c)))
def test_reference_parity_over_shards(fx, gts, cuts):
    import torch
    from cmve import dist as D
    vid, cap = fx["vid_p"], fx["cap_p"]
    v2t, t2v = gts
    n_g, n_q, world = vid.shape[0], cap.shape[0], len(cuts) - 1
    t2v_lists = [t2v[i] for i in range(n_q)]
    qc = _slices(n_q, world, even=False)

    def body(r, comm):
        sh = D.ShardedGallery(vid[cuts[r]:cuts[r + 1]], offset=cuts[r], n_global=n_g, comm=comm, measure="jaccard",
                              filter="jaccard")
        q_local = torch.from_numpy(cap[qc[r]:qc[r + 1]].copy()).cuda()
        ev = sh.evaluate(q_local, t2v_lists, v2t)
        st = sh.filter_stats
        return ev, st, sh.topk(q_local, 10), sh.n

    for (r_t, r_v), st, (ids, _), n in D.LocalGroup(world).run(body):
        assert np.array_equal(r_t, fx["t2v_ranks_jaccard"]) and np.array_equal(r_v, fx["v2t_ranks_jaccard"])
        assert np.array_equal(ids, fx["top10_jaccard"])
        # (the golden captions reach 7.2 where the videos end at 3.9: packed on the shard's own grid their elements
        # clamp, their row errors are large and the band list may overflow -- resolved on the device, the same words)
        _accounted(st, n_q * n)


# ---- word-equal with filter=False ------------------------------------------------------------------------------------------

def _every_method(a, b, rows, cols, cuts, filter):
    """Per rank: what evaluate, cal_perf, rank_queries, evaluate_device and topk return, and the shard's filter_stats
    after each count."""
    import torch
    from cmve import dist as D
    world = len(cuts) - 1
    n_q, n_g = a.shape[0], b.shape[0]
    qc = _slices(n_q, world, even=True)  # rank_queries gathers equal slices

    def body(r, comm):
        sh = D.ShardedGallery(b[cuts[r]:cuts[r + 1]], offset=cuts[r], n_global=n_g, comm=comm, measure="jaccard",
                              filter=filter)
        q_local = torch.from_numpy(a[qc[r]:qc[r + 1]].copy()).cuda()
        stats = []
        ev = sh.evaluate(q_local, rows, cols)
        stats.append(sh.filter_stats)
        perf = sh.cal_perf(q_local, cols, rows)
        stats.append(sh.filter_stats)
        q_all = D.all_gather_var(q_local, comm)
        if n_q % world == 0:
            rq = sh.rank_queries(q_local, sh.local_gt_csr(rows), n_q)
        else:  # rank_queries gathers equal slices: the gathered form takes any
            rq = sh.rank_queries_device(q_all, sh.local_gt_csr(rows), n_q)[0].cpu().numpy().astype(np.int64)
        stats.append(sh.filter_stats)
        t2v, v2t, rec, ovf = sh.evaluate_device(q_all, sh.local_gt_csr(rows), sh.local_v2t_csr(cols), n_q)
        stats.append(sh.filter_stats)
        dev = (t2v.cpu().numpy(), v2t.cpu().numpy(), rec.cpu().numpy(), bool(ovf.item()))
        top = sh.topk(q_local, 10)
        return ev, perf, rq, dev, stats, sh.n, sh._pw_filter_off, top

    return D.LocalGroup(world).run(body)


def _assert_word_equal(got, want, n_q, in_grid=True):
    """in_grid: the captions' elements lie on the shards' grids, so no band list overflows and no shard latches."""
    for (ev, perf, rq, dev, stats, n, off, top), (ev0, perf0, rq0, dev0, stats0, _, _, top0) in zip(got, want):
        assert np.array_equal(ev[0], ev0[0]) and np.array_equal(ev[1], ev0[1])          # ranks
        assert np.array_equal(np.array(perf, float), np.array(perf0, float))           # recalls and mAP positions
        assert rq.dtype == np.int64 and np.array_equal(rq, rq0) and np.array_equal(rq, ev0[0])
        for x, y in zip(dev[:3], dev0[:3]):
            assert np.array_equal(x, y)
        assert dev[3] is False and dev0[3] is False
        assert np.array_equal(top[0], top0[0])                                           # top-k ids and words
        assert np.array_equal(np.ascontiguousarray(top[1]).view(np.int64), np.ascontiguousarray(top0[1]).view(np.int64))
        assert stats0 == [None] * 4 and (not off or not in_grid)
        for st in stats:
            if st is not None or in_grid:  # (a shard that latched the K18 route stops reporting)
                _accounted(st, n_q * n)
                assert st["overflow"] == 0 or not in_grid


def test_word_equal_with_the_k18_route(fx, gts, adversarial):
    a, b, rows, cols = adversarial
    _assert_word_equal(_every_method(a, b, rows, cols, ADVERSARIAL_CUTS, "jaccard"),
                       _every_method(a, b, rows, cols, ADVERSARIAL_CUTS, False), NA)
    v2t, t2v = gts
    vid, cap = fx["vid_p"], fx["cap_p"]
    t2v_lists = [t2v[i] for i in range(cap.shape[0])]
    _assert_word_equal(_every_method(cap, vid, t2v_lists, v2t, GOLDEN_CUTS, "jaccard"),
                       _every_method(cap, vid, t2v_lists, v2t, GOLDEN_CUTS, False), cap.shape[0], in_grid=False)


def test_sharded_topk_equals_the_whole_gallery(adversarial, monkeypatch):
    import torch
    from cmve import dist as D, engine
    a, b, _, _ = adversarial
    cuts = ADVERSARIAL_CUTS
    world = len(cuts) - 1
    qc = _slices(NA, world, even=False)
    calls = []
    real = engine.jaccard_topk
    monkeypatch.setattr(engine, "jaccard_topk", lambda *x, **kw: calls.append(1) or real(*x, **kw))

    def body(r, comm):
        sh = D.ShardedGallery(b[cuts[r]:cuts[r + 1]], offset=cuts[r], n_global=NB, comm=comm, measure="jaccard",
                              filter="jaccard")
        q_local = torch.from_numpy(a[qc[r]:qc[r + 1]].copy()).cuda()
        out = [sh.topk(q_local, k) for k in (7, 64)]
        return out, sh._pw_packed is not None, sh.n

    want = {k: _whole_gallery_topk(a, b, k) for k in (7, 64)}
    for out, packed, n in D.LocalGroup(world).run(body):
        for k, (ids, err) in zip((7, 64), out):
            assert ids.dtype == np.int64 and np.array_equal(ids, want[k][0])
            assert np.array_equal(np.ascontiguousarray(err).view(np.int64), want[k][1].view(np.int64))
        assert packed == (n > 0)
    assert len(calls) == 2 * sum(1 for r in range(world) if cuts[r + 1] > cuts[r])  # K25 ran on every non-empty shard


# ---- the pack, the thresholds, the band list ---------------------------------------------------------------------------------

def test_pack_is_lazy_shared_and_absent_below_the_thresholds(fx, gts, monkeypatch):
    import torch
    from cmve import engine
    v2t, t2v = gts
    vid, cap = fx["vid_p"], fx["cap_p"]
    q = torch.from_numpy(cap.copy()).cuda()
    t2v_lists = [t2v[i] for i in range(cap.shape[0])]
    packs = []
    real = engine.JaccardSet

    class Counting(real):
        def __init__(self, x, grid=None, device=None):
            packs.append(grid is None)
            super().__init__(x, grid=grid, device=device)

    monkeypatch.setattr(engine, "JaccardSet", Counting)
    # filter=None below both thresholds: no pack, no filter, the K18 route's words
    assert not engine.jaccard_topk_auto(cap.shape[0], vid.shape[0], packed=True)
    assert engine.JACCARD_FILTER_MIN_PAIRS is None or cap.shape[0] * vid.shape[0] < engine.JACCARD_FILTER_MIN_PAIRS
    auto = _solo(vid)
    r_t, r_v = auto.evaluate(q, t2v_lists, v2t)
    ids, _ = auto.topk(q, 10)
    assert auto._pw_packed is None and auto.filter_stats is None and packs == []
    assert np.array_equal(r_t, fx["t2v_ranks_jaccard"]) and np.array_equal(r_v, fx["v2t_ranks_jaccard"])
    assert np.array_equal(ids, fx["top10_jaccard"])
    # filter=False: the same, for the top-k too
    off = _solo(vid, filter=False)
    off.topk(q, 10)
    off.evaluate(q, t2v_lists, v2t)
    assert off._pw_packed is None and off.filter_stats is None and packs == []
    # filter="jaccard": made by the first call that needs it -- here the top-k -- and shared with the count
    sh = _solo(vid, filter="jaccard")
    assert sh._pw_packed is None
    ids, _ = sh.topk(q, 10)
    packed = sh._pw_packed
    assert isinstance(packed, real) and packed.raw.data_ptr() == sh.shard.data_ptr()  # no second copy
    assert packs.count(True) == 1 and np.array_equal(ids, fx["top10_jaccard"])
    r_t, r_v = sh.evaluate(q, t2v_lists, v2t)
    assert sh._pw_packed is packed and packs.count(True) == 1  # the shard once; the captions per call on its grid
    assert sh.filter_stats is not None and np.array_equal(r_t, fx["t2v_ranks_jaccard"])
    # filter=None above the thresholds takes K24 and K25 (the thresholds lowered: the shapes stay small)
    monkeypatch.setattr(engine, "JACCARD_FILTER_MIN_PAIRS", 1)
    monkeypatch.setattr(engine, "JACCARD_TOPK_FILTER_MIN_PAIRS", 1)
    low = _solo(vid)
    r_t, r_v = low.evaluate(q, t2v_lists, v2t)
    assert low.filter_stats is not None and low._pw_packed is not None
    assert np.array_equal(r_t, fx["t2v_ranks_jaccard"]) and np.array_equal(r_v, fx["v2t_ranks_jaccard"])
    _accounted(low.filter_stats, cap.shape[0] * vid.shape[0])
    calls = []
    real_topk = engine.jaccard_topk
    monkeypatch.setattr(engine, "jaccard_topk", lambda *x, **kw: calls.append(1) or real_topk(*x, **kw))
    low = _solo(vid)  # (a fresh shard: a count whose band exceeds 1/8 of the pairs latches its shard onto K18)
    assert np.array_equal(low.topk(q, 10)[0], fx["top10_jaccard"]) and calls == [1] and low._pw_packed is not None
    # the other families' words under jaccard
    with pytest.raises(ValueError, match='filter="l1"'):
        _solo(vid, filter="l1")
    with pytest.raises(ValueError, match="Euclidean"):
        _solo(vid, filter=True)


def test_a_small_band_list_overflows_is_exact_and_grows(adversarial):
    import torch
    from cmve import engine
    a, b, rows, cols = adversarial
    q = torch.from_numpy(a).cuda()
    want = _solo(b, filter=False).evaluate(q, rows, cols)
    sh = _solo(b, filter="jaccard", band_cap=1)
    assert sh._pw_packed is None  # lazy
    first = sh.evaluate(q, rows, cols)
    st1 = sh.filter_stats
    assert st1["fallback"] and st1["overflow"] == 1 and st1["rescored"] == 0 and 1 < st1["band"] <= NA * NB // 8
    assert not sh._pw_filter_off and sh._pw_band.numel() == st1["band"]  # _pw_plan grew the list to the reported need
    packed = sh._pw_packed
    assert isinstance(packed, engine.JaccardSet) and packed.raw.data_ptr() == sh.shard.data_ptr()
    second = sh.evaluate(q, rows, cols)
    st2 = sh.filter_stats
    assert not st2["fallback"] and st2["overflow"] == 0
    assert st2["band"] == st1["band"] and st2["rescored"] == st2["band"] and st2["decided"] + st2["band"] == NA * NB
    assert sh._pw_packed is packed  # packed once
    for got in (first, second):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # the top-k shares the pack
    ids, err = sh.topk(q, 5)
    assert sh._pw_packed is packed
    w_i, w_e = _whole_gallery_topk(a, b, 5)
    assert np.array_equal(ids, w_i) and np.array_equal(np.ascontiguousarray(err).view(np.int64), w_e.view(np.int64))
