"""ShardedGallery(measure=<l1 / l1_norm>, filter="l1") on the GPU: the sharded evaluation's count pass through the
integer SAD filter (K22) and the shard's top-k through K23, the shards in ONE process through LocalGroup (one thread +
HIP stream each).

The contract is K21's: every method returns what the fp64 route (filter=False) returns, word for word, whatever each
shard's band list does -- an overflow is resolved on that shard's device, so nothing synchronises and no flag rides a
collective; ``filter_stats`` says what each shard's filter did; the methods that end on the host grow a shard's band
list; the shard is packed once, lazily, on its own grid, and the count and the top-k share that pack."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L1_MEASURES = ["l1", "l1_norm"]
NA, NB = 300, 520


@pytest.fixture(scope="module")
def fx(golden):
    return golden("measures_retrieval")


@pytest.fixture(scope="module")
def gts(fx):
    from oracle import retrieval as R
    return R.get_gt(list(fx["video_ids"]), list(fx["caption_ids"]))  # (v2t list, t2v dict)


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


GOLDEN_CUTS = (0, 5, 5, 20, 37, 141)        # an empty shard and four uneven ones
ADVERSARIAL_CUTS = (0, 128, 128, 391, 520)  # an empty shard, a shard of exactly one tile, two partial ones


# ---- golden parity ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cuts", [(0, 141), GOLDEN_CUTS], ids=lambda c: "-".join(map(str, c)))
@pytest.mark.parametrize("m", L1_MEASURES)
def test_reference_parity_over_shards(fx, gts, m, cuts):
    import torch
    from cmve import dist as D
    vid, cap = fx["vid"], fx["cap"]
    v2t, t2v = gts
    n_g, n_q, world = vid.shape[0], cap.shape[0], len(cuts) - 1
    t2v_lists = [t2v[i] for i in range(n_q)]
    qc = _slices(n_q, world, even=False)

    def body(r, comm):
        sh = D.ShardedGallery(vid[cuts[r]:cuts[r + 1]], offset=cuts[r], n_global=n_g, comm=comm, measure=m,
                              filter="l1")
        q_local = torch.from_numpy(cap[qc[r]:qc[r + 1]].copy()).cuda()
        ev = sh.evaluate(q_local, t2v_lists, v2t)
        st = sh.filter_stats
        return ev, sh.cal_perf(q_local, v2t, t2v), st, sh.filter_stats, sh.n

    ref = fx["cal_perf_" + m]
    for (r_t, r_v), perf, st_ev, st_perf, n in D.LocalGroup(world).run(body):
        assert np.array_equal(r_t, fx["t2v_ranks_" + m]) and np.array_equal(r_v, fx["v2t_ranks_" + m])
        np.testing.assert_allclose(np.array(perf[0], float), ref[0], rtol=0, atol=1e-12)
        np.testing.assert_allclose(np.array(perf[1], float), ref[1], rtol=0, atol=1e-12)
        _accounted(st_ev, n_q * n)
        _accounted(st_perf, n_q * n)
        assert st_ev["overflow"] == 0


# ---- word-equal with filter=False ------------------------------------------------------------------------------------------

def _ulps(v, steps):
    for _ in range(steps):
        v = np.nextafter(v, v.dtype.type(np.inf))
    return v


def _adversarial(d):
    """The fp64 rows of tests/test_gpu_l2_filter.py's recipe: planted GTs, exact duplicates 256 rows apart, 1 / 2 /
    4-ulp near-ties, zero, huge, tiny, inf and NaN rows; lists with 0, 1, several and 20 items, repeats, NaN items."""
    rng = np.random.default_rng(d)
    b = rng.standard_normal((NB, d))
    pick = rng.integers(0, 200, NA)
    pick[20] = 7
    a = b[pick] + 0.5 * rng.standard_normal((NA, d))
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
    return a, b, rows, cols


@pytest.fixture(scope="module")
def adversarial():
    return _adversarial(67)


def _every_method(a, b, rows, cols, cuts, m, filter):
    """Per rank: what evaluate, cal_perf, rank_queries and evaluate_device return, and the shard's filter_stats after
    each of them."""
    import torch
    from cmve import dist as D
    world = len(cuts) - 1
    n_q, n_g = a.shape[0], b.shape[0]
    qc = _slices(n_q, world, even=True)  # rank_queries gathers equal slices

    def body(r, comm):
        sh = D.ShardedGallery(b[cuts[r]:cuts[r + 1]], offset=cuts[r], n_global=n_g, comm=comm, measure=m,
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
        assert t2v.is_cuda and v2t.is_cuda and rec.is_cuda and ovf.is_cuda and ovf.dtype == torch.bool
        stats.append(sh.filter_stats)
        dev = (t2v.cpu().numpy(), v2t.cpu().numpy(), rec.cpu().numpy(), bool(ovf.item()))
        return ev, perf, rq, dev, stats, sh.n, sh._pw_filter_off

    return D.LocalGroup(world).run(body)


def _assert_word_equal(got, want, n_q):
    for (ev, perf, rq, dev, stats, n, off), (ev0, perf0, rq0, dev0, stats0, _, _) in zip(got, want):
        assert np.array_equal(ev[0], ev0[0]) and np.array_equal(ev[1], ev0[1])
        assert ev[0].dtype == np.int64 and ev[1].dtype == np.int64
        assert np.array_equal(np.array(perf, float), np.array(perf0, float))
        assert rq.dtype == np.int64 and np.array_equal(rq, rq0) and np.array_equal(rq, ev0[0])
        for x, y in zip(dev[:3], dev0[:3]):  # t2v ranks, this shard's v2t ranks, the v2t recall sums
            assert np.array_equal(x, y)
        assert dev[3] is False and dev0[3] is False
        assert stats0 == [None] * 4 and not off
        for st in stats:
            _accounted(st, n_q * n)
            assert st["overflow"] == 0


@pytest.mark.parametrize("m", L1_MEASURES)
def test_word_equal_with_the_fp64_route(fx, gts, adversarial, m):
    a, b, rows, cols = adversarial
    _assert_word_equal(_every_method(a, b, rows, cols, ADVERSARIAL_CUTS, m, "l1"),
                       _every_method(a, b, rows, cols, ADVERSARIAL_CUTS, m, False), NA)
    v2t, t2v = gts
    vid, cap = fx["vid"], fx["cap"]
    t2v_lists = [t2v[i] for i in range(cap.shape[0])]
    _assert_word_equal(_every_method(cap, vid, t2v_lists, v2t, GOLDEN_CUTS, m, "l1"),
                       _every_method(cap, vid, t2v_lists, v2t, GOLDEN_CUTS, m, False), cap.shape[0])


# ---- band overflow, growth, the shared pack ----------------------------------------------------------------------------------

def _solo(vid, m, **kw):
    """A world-1 shard (no process group: every collective is a no-op)."""
    from cmve import dist as D
    return D.ShardedGallery(vid, offset=0, n_global=vid.shape[0], measure=m, **kw)


def test_a_small_band_list_overflows_is_exact_and_grows(adversarial):
    import torch
    from cmve import engine
    a, b, rows, cols = adversarial
    q = torch.from_numpy(a).cuda()
    want = _solo(b, "l1", filter=False).evaluate(q, rows, cols)
    sh = _solo(b, "l1", filter="l1", band_cap=1)
    assert sh._pw_packed is None  # lazy
    first = sh.evaluate(q, rows, cols)
    st1 = sh.filter_stats
    assert st1["fallback"] and st1["overflow"] == 1 and st1["rescored"] == 0 and 1 < st1["band"] <= NA * NB // 8
    assert not sh._pw_filter_off and sh._pw_band.numel() == st1["band"]  # _pw_plan grew the list to the reported need
    packed = sh._pw_packed
    assert isinstance(packed, engine.L1Set) and packed.raw.data_ptr() == sh.shard.data_ptr()  # no second copy
    # the device route neither reads the counters nor replans
    t2v = sh.rank_queries(q, sh.local_gt_csr(rows), NA, return_host=False)
    assert np.array_equal(t2v.cpu().numpy(), want[0])
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
    w_i, w_e = _whole_gallery_topk(a, b, "l1", 5)
    assert np.array_equal(ids, w_i) and np.array_equal(err.view(np.int64), w_e.view(np.int64))


def _whole_gallery_topk(a, b, m, k):
    from cmve import engine
    from cmve.linas.evaluation import measure_spec
    metric, alpha, beta, _, sc_dt = measure_spec(m, b.shape[1])
    return engine.pairwise_topk(a, b, metric, alpha, beta, sc_dt, k, filter=False)


@pytest.mark.parametrize("m", L1_MEASURES)
def test_sharded_topk_equals_the_whole_gallery(adversarial, monkeypatch, m):
    import torch
    from cmve import dist as D, engine
    a, b, _, _ = adversarial
    cuts = ADVERSARIAL_CUTS
    world = len(cuts) - 1
    qc = _slices(NA, world, even=False)
    calls = []
    real = engine.l1_topk
    monkeypatch.setattr(engine, "l1_topk", lambda *x, **kw: calls.append(1) or real(*x, **kw))

    def body(r, comm):
        sh = D.ShardedGallery(b[cuts[r]:cuts[r + 1]], offset=cuts[r], n_global=NB, comm=comm, measure=m, filter="l1")
        q_local = torch.from_numpy(a[qc[r]:qc[r + 1]].copy()).cuda()
        out = [sh.topk(q_local, k) for k in (7, 64)]
        return out, sh._pw_packed is not None, sh.n

    want = {k: _whole_gallery_topk(a, b, m, k) for k in (7, 64)}
    for out, packed, n in D.LocalGroup(world).run(body):
        for k, (ids, err) in zip((7, 64), out):
            assert ids.dtype == np.int64 and np.array_equal(ids, want[k][0])
            assert np.array_equal(np.ascontiguousarray(err).view(np.int64), want[k][1].view(np.int64))
        assert packed == (n > 0)
    assert len(calls) == 2 * sum(1 for r in range(world) if cuts[r + 1] > cuts[r])  # K23 ran on every non-empty shard


def test_pack_is_lazy_shared_and_absent_below_the_thresholds(fx, gts, monkeypatch):
    import torch
    from cmve import engine
    v2t, t2v = gts
    vid, cap = fx["vid"], fx["cap"]
    q = torch.from_numpy(cap.copy()).cuda()
    t2v_lists = [t2v[i] for i in range(cap.shape[0])]
    packs = []
    real = engine.L1Set

    class Counting(real):
        def __init__(self, x, grid=None, device=None):
            packs.append(grid is None)
            super().__init__(x, grid=grid, device=device)

    monkeypatch.setattr(engine, "L1Set", Counting)
    # filter=None below both thresholds: no pack, no filter, the fp64 route's words
    assert not engine.l1_topk_auto(cap.shape[0], vid.shape[0], packed=True)
    assert engine.L1_FILTER_MIN_PAIRS is None or cap.shape[0] * vid.shape[0] < engine.L1_FILTER_MIN_PAIRS
    auto = _solo(vid, "l1")
    r_t, r_v = auto.evaluate(q, t2v_lists, v2t)
    ids, _ = auto.topk(q, 10)
    assert auto._pw_packed is None and auto.filter_stats is None and packs == []
    assert np.array_equal(r_t, fx["t2v_ranks_l1"]) and np.array_equal(r_v, fx["v2t_ranks_l1"])
    assert np.array_equal(ids, fx["top10_l1"])
    # filter=False: the same, for the top-k too
    off = _solo(vid, "l1", filter=False)
    off.topk(q, 10)
    assert off._pw_packed is None and packs == []
    # filter="l1": made by the first call that needs it -- here the top-k -- and shared with the count
    sh = _solo(vid, "l1_norm", filter="l1")
    assert sh._pw_packed is None
    ids, _ = sh.topk(q, 10)
    packed = sh._pw_packed
    assert packed is not None and packs.count(True) == 1 and np.array_equal(ids, fx["top10_l1_norm"])
    r_t, r_v = sh.evaluate(q, t2v_lists, v2t)
    assert sh._pw_packed is packed and packs.count(True) == 1  # the shard once; the captions per call on its grid
    assert sh.filter_stats is not None and np.array_equal(r_t, fx["t2v_ranks_l1_norm"])
    # filter=None above the count's threshold takes K22 (the threshold lowered: the shapes stay small)
    monkeypatch.setattr(engine, "L1_FILTER_MIN_PAIRS", 1)
    low = _solo(vid, "l1")
    r_t, r_v = low.evaluate(q, t2v_lists, v2t)
    assert low.filter_stats is not None and low._pw_packed is not None
    assert np.array_equal(r_t, fx["t2v_ranks_l1"]) and np.array_equal(r_v, fx["v2t_ranks_l1"])
    _accounted(low.filter_stats, cap.shape[0] * vid.shape[0])
    # jaccard has no filter
    with pytest.raises(ValueError, match='filter="l1"'):
        _solo(fx["vid_p"], "jaccard", filter="l1")
