"""ShardedGallery(measure=<euclidean / l2 / l2_norm>, filter=) on the GPU: the sharded evaluation's count pass through
the fp16 MFMA filter (K21), the shards in ONE process through LocalGroup (one thread + HIP stream each).

The contract: every method returns what the fp64 route (filter=False) returns, word for word, whatever each shard's
band list does -- an overflow is resolved on that shard's device, so nothing synchronises and no flag rides a
collective; ``filter_stats`` says what each shard's filter did; the methods that end on the host grow a shard's band
list or switch its later passes to the fp64 route; and with lists that fit the filter decides almost every pair."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L2_MEASURES = ["euclidean", "l2", "l2_norm"]
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
    assert st is not None and set(st) == {"decided", "band", "rescored", "overflow", "fallback"}
    assert st["fallback"] == (st["overflow"] == 1)
    assert st["overflow"] == 1 or (st["decided"] + st["band"] == pairs and st["rescored"] == st["band"])


# ---- 5. reference parity over shards ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("cuts", [(0, 141), (0, 70, 141), (0, 128, 141), (0, 0, 141), (0, 141, 141)],
                         ids=lambda c: "-".join(map(str, c)))
@pytest.mark.parametrize("m", L2_MEASURES)
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
                              filter=True)
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


# ---- 6. word-equal with filter=False -----------------------------------------------------------------------------------------

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
    cache = {}

    def get(d):
        if d not in cache:
            cache[d] = _adversarial(d)
        return cache[d]
    return get


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
        rq = sh.rank_queries(q_local, sh.local_gt_csr(rows), n_q)
        stats.append(sh.filter_stats)
        q_all = D.all_gather_var(q_local, comm)
        t2v, v2t, rec, ovf = sh.evaluate_device(q_all, sh.local_gt_csr(rows), sh.local_v2t_csr(cols), n_q)
        assert t2v.is_cuda and v2t.is_cuda and rec.is_cuda and ovf.is_cuda and ovf.dtype == torch.bool
        stats.append(sh.filter_stats)
        dev = (t2v.cpu().numpy(), v2t.cpu().numpy(), rec.cpu().numpy(), bool(ovf.item()))
        return ev, perf, rq, dev, stats, sh.n, sh._pw_filter_off

    return D.LocalGroup(world).run(body)


@pytest.mark.parametrize("cuts", [(0, 520), (0, 130, 520), (0, 256, 384, 520), (0, 0, 520)],
                         ids=lambda c: "-".join(map(str, c)))
@pytest.mark.parametrize("m", ["l2", "l2_norm"])
@pytest.mark.parametrize("d", [67, 1024])
def test_word_equal_with_the_fp64_route(adversarial, d, m, cuts):
    a, b, rows, cols = adversarial(d)
    got = _every_method(a, b, rows, cols, cuts, m, True)
    want = _every_method(a, b, rows, cols, cuts, m, False)
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
            _accounted(st, NA * n)


# ---- 7. it filters, sharded ----------------------------------------------------------------------------------------------------

def test_filter_decides_almost_every_pair_sharded():
    import torch
    from cmve import _lib, engine, dist as D
    rng = np.random.default_rng(0)
    na, nb, d = 512, 2048, 1024
    b = rng.standard_normal((nb, d))
    a = b[:na] + 0.5 * rng.standard_normal((na, d))
    rows = [[i] for i in range(na)]
    cols = [[j] if j < na else [] for j in range(nb)]
    want_t, want_v = engine.pairwise_gt_ranks(a, b, _lib.PW_L2, 1.0, 0.0, torch.float64, rows, cols, filter=False)
    cuts = (0, 1024, 2048)

    def body(r, comm):
        sh = D.ShardedGallery(b[cuts[r]:cuts[r + 1]], offset=cuts[r], n_global=nb, comm=comm, measure="l2",
                              filter=True)
        q_local = torch.from_numpy(a[256 * r:256 * r + 256].copy()).cuda()
        return sh.evaluate(q_local, rows, cols), sh.filter_stats

    res = D.LocalGroup(2).run(body)
    decided = 0
    for (t2v, v2t), st in res:
        assert np.array_equal(t2v, want_t) and np.array_equal(v2t, want_v)
        assert st["overflow"] == 0 and not st["fallback"]
        assert st["decided"] + st["band"] == na * 1024 and st["rescored"] == st["band"]
        decided += st["decided"]
    print("planted GTs over 2 shards: decided %d of %d (%.3f%%)" % (decided, na * nb, 100.0 * decided / (na * nb)))
    assert decided >= 0.99 * na * nb


# ---- 8. auto, growth and latch -----------------------------------------------------------------------------------------------------

def _solo(vid, m, **kw):
    """A world-1 shard (no process group: every collective is a no-op)."""
    from cmve import dist as D
    return D.ShardedGallery(vid, offset=0, n_global=vid.shape[0], measure=m, **kw)


def test_auto_follows_the_crossover(monkeypatch):
    import torch
    from cmve import _lib, engine
    routes = []
    real = engine.pairwise_count

    def spy(*args, **kw):  # the route the SHARD asks for: it never leaves the choice to the engine's own auto rule
        routes.append(kw.get("filter", "unset"))
        return real(*args, **kw)

    monkeypatch.setattr(engine, "pairwise_count", spy)
    rng = np.random.default_rng(5)
    na, d = 512, 64
    nb_at = -(-engine.L2_FILTER_MIN_PAIRS // na)
    b_all = rng.standard_normal((nb_at, d))
    a = b_all[:na] + 0.5 * rng.standard_normal((na, d))
    q = torch.from_numpy(a).cuda()
    rows = [[i] for i in range(na)]
    for nb, taken in ((nb_at - 1, False), (nb_at, True)):
        assert (na * nb >= engine.L2_FILTER_MIN_PAIRS) == taken
        b = b_all[:nb]
        cols = [[j] if j < na else [] for j in range(nb)]
        auto, off = _solo(b, "l2"), _solo(b, "l2", filter=False)
        del routes[:]
        got, want = auto.evaluate(q, rows, cols), off.evaluate(q, rows, cols)
        assert routes == [taken, False]
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert (auto.filter_stats is not None) == taken and off.filter_stats is None
        if taken:
            _accounted(auto.filter_stats, na * nb)
            assert auto._pw_packed is not None and off._pw_packed is None
        # l1 never takes the filter, whatever the size
        l1 = _solo(b, "l1")
        l1.evaluate(q, rows, None)
        assert l1.filter_stats is None and l1._pw_packed is None and routes[-1] is False
        # engine.pairwise_count's own auto rule, on plain rows: the same threshold
        dev = q.device
        off_, idx = engine.csr(rows, dev)
        bt = engine.to_device(b)
        sc = engine.pairwise_item_scores(q, bt, _lib.PW_L2, 1.0, 0.0, torch.float64, off_, idx, na, False, 0)
        e_r, _ = real(q, bt, _lib.PW_L2, 1.0, 0.0, torch.float64, row=(off_, sc, nb), filter=False)
        a_r, _, st = real(q, bt, _lib.PW_L2, 1.0, 0.0, torch.float64, row=(off_, sc, nb), return_stats=True)
        assert torch.equal(a_r, e_r) and (st is not None) == taken


def test_other_measures_ignore_none_and_refuse_true(fx, gts):
    import torch
    v2t, t2v = gts
    for m, vid, cap in (("jaccard", fx["vid_p"], fx["cap_p"]), ("l1", fx["vid"], fx["cap"]),
                        ("l1_norm", fx["vid"], fx["cap"])):
        sh = _solo(vid, m)
        r_t, r_v = sh.evaluate(torch.from_numpy(cap.copy()).cuda(), [t2v[i] for i in range(cap.shape[0])], v2t)
        assert np.array_equal(r_t, fx["t2v_ranks_" + m]) and np.array_equal(r_v, fx["v2t_ranks_" + m])
        assert sh.filter_stats is None
        with pytest.raises(ValueError, match="Euclidean"):
            _solo(vid, m, filter=True)


def test_a_small_band_list_grows_after_a_pass_that_ends_on_the_host():
    import torch
    rng = np.random.default_rng(8)
    na, nb, d = 256, 1024, 256
    b = rng.standard_normal((nb, d))
    a = b[:na] + 0.5 * rng.standard_normal((na, d))
    q = torch.from_numpy(a).cuda()
    rows = [[i] for i in range(na)]
    cols = [[j] if j < na else [] for j in range(nb)]
    want = _solo(b, "l2", filter=False).evaluate(q, rows, cols)
    sh = _solo(b, "l2", filter=True, band_cap=1)
    first = sh.evaluate(q, rows, cols)
    st1 = sh.filter_stats
    assert st1["fallback"] and st1["overflow"] == 1 and st1["rescored"] == 0 and 1 < st1["band"] <= na * nb // 8
    assert not sh._pw_filter_off and sh._pw_band.numel() == st1["band"]
    packed = sh._pw_packed
    # the device route neither reads the counters nor replans
    t2v = sh.rank_queries(q, sh.local_gt_csr(rows), na, return_host=False)
    assert np.array_equal(t2v.cpu().numpy(), want[0])
    second = sh.evaluate(q, rows, cols)
    st2 = sh.filter_stats
    assert not st2["fallback"] and st2["overflow"] == 0
    assert st2["band"] == st1["band"] and st2["rescored"] == st2["band"] and st2["decided"] + st2["band"] == na * nb
    assert sh._pw_packed is packed  # packed once
    for got in (first, second):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # the top-k shares the pack
    ids, _ = sh.topk(q, 5)
    assert sh._pw_packed is packed and np.array_equal(ids[:, 0], np.arange(na))


def test_clustered_rows_latch_the_fp64_route():
    import torch
    rng = np.random.default_rng(3)
    na, nb, d = 256, 384, 256
    b = 100.0 + rng.standard_normal((nb, d))
    a = 100.0 + rng.standard_normal((na, d))
    q = torch.from_numpy(a).cuda()
    rows = [[int(j)] for j in rng.integers(0, nb, na)]
    cols = [[int(i)] for i in rng.integers(0, na, nb)]
    ref = _solo(b, "l2", filter=False)
    want, want_perf = ref.evaluate(q, rows, cols), ref.cal_perf(q, cols, rows)
    sh = _solo(b, "l2", filter=True)
    first = sh.evaluate(q, rows, cols)
    st = sh.filter_stats
    print("clustered shard:", st)
    assert st is not None and st["fallback"] and st["band"] * 8 > na * nb
    assert sh._pw_filter_off
    second = sh.evaluate(q, rows, cols)
    assert sh.filter_stats is None  # the latch: this shard's later passes stay on the fp64 route
    perf = sh.cal_perf(q, cols, rows)
    assert sh.filter_stats is None
    for got in (first, second):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(np.array(perf, float), np.array(want_perf, float))
