"""ShardedGallery(measure='cosine', filter="cosine") on the GPU (K27): the sharded evaluation under cosine from ONE fp16
MFMA pass per shard, the shards in ONE process through LocalGroup (one thread + HIP stream each).

The contract: every method returns what today's route (filter=None: the rank GEMM, up to three passes per shard)
returns, word for word, whatever each shard's band list does -- an overflow is resolved on that shard's device, NaN
items' words included; the positions are the unsharded ``engine.cos_gt_eval``'s; ``filter_stats`` says what each
shard's filter did; and with lists that fit the filter decides almost every pair.

Two things about the rows and lists of tests/test_gpu_cos_positions.py that the sharded methods force on this file:
cal_perf's t2v lists give caption 7 its planted video (a caption without GT is a KeyError in the reference and an
IndexError in today's cal_perf; ``evaluate``, ``rank_queries`` and ``evaluate_device`` keep the empty list), and
``rank_queries``, which gathers equal slices, ranks the first 128 captions in equal slices (129 do not split evenly
over 2 or 4 ranks; a caption's t2v rank does not depend on the other captions, so its words are ``evaluate``'s; the
129th caption, which names the last video, goes through the other three methods)."""
import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu

NRQ = 128  # the captions rank_queries ranks (module docstring)
NA, NB, D = 129, 257, 96  # one row past a tile on the caption side, one past two tiles (and the 256-row pad) on the videos'
CUTS = [(0, 257), (0, 130, 257), (0, 128, 257), (0, 0, 257), (0, 257, 257), (0, 64, 128, 192, 257)]
DTYPES = {"f32f32": (np.float32, np.float32), "f64f64": (np.float64, np.float64), "f32f64": (np.float32, np.float64)}
_ids = lambda c: "-".join(map(str, c))  # noqa: E731


def _adversarial(dt_c=np.float32, dt_v=np.float32):
    """tests/test_gpu_cos_positions.py's recipe: exact duplicates, one-ulp near-ties, zero-norm rows; lists of 0 / 1 /
    37 items, repeats, lone NaN items, a list of only NaN items."""
    rng = np.random.default_rng(26)
    v = rng.standard_normal((NB, D)).astype(dt_v)
    pick = rng.integers(0, 190, NA)
    c = (v[pick].astype(np.float64) + 1.5 * rng.standard_normal((NA, D))).astype(dt_c)
    v[200], v[256] = v[3], v[3]          # exact duplicates: ties under the strict >, no index tie-break
    v[201] = v[4]
    v[201, 11] = np.nextafter(v[201, 11], dt_v(np.inf))  # one element's last bit
    c[100] = c[5]
    c[101] = c[6]
    c[101, 0] = np.nextafter(c[101, 0], dt_c(-np.inf))
    v[50], c[60] = 0.0, 0.0              # zero norm: NaN items, a NaN column and a NaN row
    t2v = [[int(p)] for p in pick]
    t2v[7] = []
    t2v[8] = [3, 200, 256, 4, 201, 50] + [int(x) for x in rng.permutation(190) if x != 50][:31]  # 37 items, one NaN
    t2v[9] = [5, 5]                      # an item repeated inside a list
    t2v[10] = [50]                       # a lone NaN item
    t2v[11] = [50, 12, 50]               # NaN items around a finite one
    t2v[60] = [1, 2]                     # every item NaN (the caption has no norm)
    t2v[128] = [256, 0]                  # the last caption names the last video
    assert len(t2v[8]) == 37
    v2t = [[] for _ in range(NB)]
    for i, p in enumerate(pick):
        v2t[int(p)].append(i)
    v2t[3] = [5, 100, 6, 101, 60]        # the duplicate captions, the near-tie and the NaN caption
    v2t[200] = [5, 100]
    v2t[50] = [1, 2, 60]
    v2t[256] = [128, 0, 128]
    v2t[255] = [int(x) for x in rng.permutation(NA)[:37]]
    v2t[254] = []
    t2v_perf = [list(l) for l in t2v]
    t2v_perf[7] = [int(pick[7])]         # cal_perf: every caption has a GT (module docstring)
    return c, v, t2v, v2t, t2v_perf


_ADV = {}


def _adv(dt):
    if dt not in _ADV:
        _ADV[dt] = _adversarial(*DTYPES[dt])
    return _ADV[dt]


def _slices(n, world):
    c = np.linspace(0, n, world + 1).astype(int)
    if world > 1:
        c[1:-1] += 3  # uneven
    return c


def _accounted(st, pairs):
    assert st is not None and set(st) == {"decided", "band", "rescored", "overflow", "fallback"}
    assert st["fallback"] == (st["overflow"] == 1)
    assert st["overflow"] == 1 or (st["decided"] + st["band"] == pairs and st["rescored"] == st["band"])


_RUNS = {}


def _every_method(dt, cuts, filter, band_cap=None):
    """Per rank: what evaluate, cal_perf, rank_queries and evaluate_device return on FRESH shards each (so that a
    small band list overflows under every one of them), the shard's filter_stats after each, and under the filter
    the positions of the one pass; computed once per case."""
    key = (dt, cuts, filter, band_cap)
    if key in _RUNS:
        return _RUNS[key]
    import torch
    from cmve import _lib, dist as D
    c, v, t2v, v2t, t2v_perf = _adv(dt)
    world = len(cuts) - 1
    qc = _slices(NA, world)

    def body(r, comm):
        def shard():
            return D.ShardedGallery(v[cuts[r]:cuts[r + 1]], offset=cuts[r], n_global=NB, comm=comm, with_lo=False,
                                    filter=filter, band_cap=band_cap)

        q_local = torch.from_numpy(c[qc[r]:qc[r + 1]].copy()).cuda()
        stats = {}
        sh = shard()
        ev = sh.evaluate(q_local, t2v, v2t)
        stats["evaluate"] = sh.filter_stats
        sh = shard()
        perf = sh.cal_perf(q_local, v2t, t2v_perf)
        stats["cal_perf"] = sh.filter_stats
        band = getattr(sh, "_pw_band", None)  # (today's shard has no band list)
        grown = None if band is None else band.numel()
        again = sh.evaluate(q_local, t2v, v2t)  # the pass after the list has grown
        stats["next"] = sh.filter_stats
        sh = shard()
        q_all = D.all_gather_var(q_local, comm)
        t, vv, rec, ovf = sh.evaluate_device(q_all, sh.local_gt_csr(t2v), sh.local_v2t_csr(v2t), NA)
        assert t.is_cuda and vv.is_cuda and rec.is_cuda and ovf.is_cuda and ovf.dtype == torch.bool
        stats["evaluate_device"] = sh.filter_stats
        dev = (t.cpu().numpy(), vv.cpu().numpy(), rec.cpu().numpy(), bool(ovf.item()))
        per = NRQ // world
        rq = sh.rank_queries(torch.from_numpy(c[r * per:(r + 1) * per].copy()).cuda(), sh.local_gt_csr(t2v[:NRQ]), NRQ)
        stats["rank_queries"] = sh.filter_stats
        pos = None
        if filter == "cosine":
            sh = shard()
            _, t_pos, _, v_pos = sh._pw_evaluate_gathered(sh._pw_rows(q_all), NA, t2v, v2t)
            pos = (t_pos, v_pos)
        else:  # today's v2t positions of this shard's videos (1-based)
            pos = (None, sh._positions(sh._pack(q_all, _lib.SIM_F16), sh.local_v2t_lists(v2t), _lib.SIM_F16))
        return dict(ev=ev, perf=perf, again=again, dev=dev, rq=rq, stats=stats, n=sh.n, pos=pos, grown=grown)

    _RUNS[key] = D.LocalGroup(world).run(body)
    return _RUNS[key]


def _same_words(got, want):
    for g, w in zip(got, want):
        assert g["ev"][0].dtype == np.int64 and g["ev"][1].dtype == np.int64
        assert np.array_equal(g["ev"][0], w["ev"][0]) and np.array_equal(g["ev"][1], w["ev"][1])
        assert np.array_equal(g["again"][0], w["ev"][0]) and np.array_equal(g["again"][1], w["ev"][1])
        print("cal_perf:", g["perf"], w["perf"])
        np.testing.assert_allclose(np.array(g["perf"], float), np.array(w["perf"], float), rtol=0, atol=1e-12)
        assert g["rq"].dtype == np.int64 and np.array_equal(g["rq"], w["rq"]) and np.array_equal(g["rq"], w["ev"][0][:NRQ])
        for x, y in zip(g["dev"][:3], w["dev"][:3]):  # t2v ranks, this shard's v2t ranks, the v2t recall sums
            assert np.array_equal(x, y)
        assert g["dev"][3] is False and w["dev"][3] is False


_UNSHARDED = {}


def _unsharded(dt):
    """engine.cos_gt_eval on the whole gallery, and today's positions (the expanded rank pass)."""
    if dt not in _UNSHARDED:
        from cmve import engine
        c, v, t2v, v2t, _ = _adv(dt)
        caps, vids = engine.RowSet(c, with_lo=False), engine.RowSet(v, with_lo=False)
        _UNSHARDED[dt] = (engine.cos_gt_eval(caps, vids, t2v, v2t), engine.gt_positions_fused(caps, vids, t2v),
                          engine.gt_positions_fused(vids, caps, v2t))
    return _UNSHARDED[dt]


# ---- 1. word-equal with today's route, every method -------------------------------------------------------------------------

@pytest.mark.parametrize("cuts", CUTS, ids=_ids)
@pytest.mark.parametrize("dt", list(DTYPES))
def test_word_equal_with_todays_route(dt, cuts):
    got, want = _every_method(dt, cuts, "cosine"), _every_method(dt, cuts, None)
    _same_words(got, want)
    ((tp, tr), (vp, vr)), tp_today, vp_today = _unsharded(dt)
    t_flat = np.concatenate([np.asarray(p, np.int64) for p in tp])
    assert np.array_equal(t_flat, np.concatenate([np.asarray(p, np.int64) for p in tp_today]))
    for r, (g, w) in enumerate(zip(got, want)):
        assert all(s is None for s in w["stats"].values())
        for method, st in g["stats"].items():
            _accounted(st, (NRQ if method == "rank_queries" else NA) * g["n"])
        # the unsharded one pass: ranks of both directions, the position of every item
        assert np.array_equal(g["ev"][0], tr) and np.array_equal(g["ev"][1], vr)
        assert np.array_equal(g["pos"][0] + 1, t_flat)
        mine = vp[cuts[r]:cuts[r + 1]]
        v_flat = np.concatenate([np.asarray(p, np.int64) for p in mine] + [np.zeros(0, np.int64)])
        assert np.array_equal(g["pos"][1] + 1, v_flat)
        # today's positions: the unsharded expanded pass (t2v), this shard's own (v2t)
        today = np.concatenate([np.asarray(p, np.int64) for p in w["pos"][1]] + [np.zeros(0, np.int64)])
        assert np.array_equal(g["pos"][1] + 1, today)
        assert np.array_equal(today, np.concatenate([np.asarray(p, np.int64) for p in vp_today[cuts[r]:cuts[r + 1]]]
                                                    + [np.zeros(0, np.int64)]))


# ---- 2. reference parity over shards, 5. the filter filters -----------------------------------------------------------------

MULTI_CUTS = [(0, 200), (0, 70, 200), (0, 128, 200)]
_MULTI = {}


def _multi(cuts):
    if cuts not in _MULTI:
        import torch
        from cmve import dist as D
        from cmve.linas import metrics as M
        v, c, vid, cid = synth.multi_caption_embeddings()
        v2t_gt, t2v_gt = M.get_gt(vid, cid)
        n_g, n_q, world = v.shape[0], c.shape[0], len(cuts) - 1
        qc = _slices(n_q, world)

        def body(r, comm):
            sh = D.ShardedGallery(v[cuts[r]:cuts[r + 1]], offset=cuts[r], n_global=n_g, comm=comm, filter="cosine")
            q_local = torch.from_numpy(c[qc[r]:qc[r + 1]].copy()).cuda()
            perf = sh.cal_perf(q_local, v2t_gt, t2v_gt)
            return perf, sh.filter_stats, sh.n

        _MULTI[cuts] = (D.LocalGroup(world).run(body), n_q, n_g)
    return _MULTI[cuts]


@pytest.mark.parametrize("cuts", MULTI_CUTS, ids=_ids)
def test_reference_parity_over_shards(golden, cuts):
    g = golden("retrieval_multi")
    res, _, _ = _multi(cuts)
    for perf, _, _ in res:
        print("cal_perf:", perf)
        np.testing.assert_allclose(np.array(perf[0], float), g["v2t"], rtol=0, atol=1e-12)
        np.testing.assert_allclose(np.array(perf[1], float), g["t2v"], rtol=0, atol=1e-12)


@pytest.mark.parametrize("cuts", MULTI_CUTS, ids=_ids)
def test_the_filter_filters_sharded(cuts):
    res, n_q, n_g = _multi(cuts)
    assert (n_q, n_g) == (4000, 200)
    decided = band = 0
    for _, st, n in res:
        print("shard of %d videos:" % n, st)
        assert st["overflow"] == 0 and not st["fallback"] and st["rescored"] == st["band"]
        assert st["decided"] + st["band"] == n_q * n
        decided, band = decided + st["decided"], band + st["band"]
    print("%s: band %d of %d pairs (%.3f %%)" % (_ids(cuts), band, n_q * n_g, 100.0 * band / (n_q * n_g)))
    assert decided + band == 4000 * 200
    assert band <= 0.02 * 4000 * 200  # (a cap against a route that sends every pair to the re-score)


# ---- 3. overflow resolved on the device -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("cuts", CUTS, ids=_ids)
def test_overflow_is_resolved_on_the_device(cuts):
    got, want = _every_method("f32f32", cuts, "cosine", band_cap=8), _every_method("f32f32", cuts, None)
    _same_words(got, want)
    full = _every_method("f32f32", cuts, "cosine")
    for g, f in zip(got, full):
        print("shard of %d videos:" % g["n"], g["stats"], "list grown to", g["grown"])
        assert np.array_equal(g["pos"][0], f["pos"][0]) and np.array_equal(g["pos"][1], f["pos"][1])
        if g["n"] == 0:
            continue
        for method in ("evaluate", "cal_perf", "evaluate_device", "rank_queries"):
            st = g["stats"][method]
            assert st["fallback"] and st["overflow"] == 1 and st["rescored"] == 0 and st["band"] > 8, method
        # the need is the band of a list that fits: cal_perf's pass asks for both directions, as evaluate's does
        assert g["stats"]["cal_perf"]["band"] >= f["stats"]["evaluate"]["band"] > 8
        assert g["grown"] >= g["stats"]["cal_perf"]["band"]
        nxt = g["stats"]["next"]
        assert nxt["overflow"] == 0 and not nxt["fallback"] and nxt["decided"] + nxt["band"] == NA * g["n"]
        assert nxt["rescored"] == nxt["band"]


# ---- 4. the entries alone -------------------------------------------------------------------------------------------------------

def _sides(caps, vids, t2v, v2t):
    from cmve import engine
    dev = caps.device
    out = []
    for lists, col_dir, n in ((t2v, False, vids.n), (v2t, True, caps.n)):
        off, idx = engine.csr(lists, dev)
        items = sum(len(l) for l in lists)
        out.append((off, engine.cos_item_scores(caps, vids, off, idx, items, col_dir), n))
    return out


def test_resolved_count_gives_the_words_of_a_full_list():
    import torch
    from cmve import engine
    c, v, t2v, v2t, _ = _adv("f32f32")
    caps, vids = engine.RowSet(c, with_lo=False), engine.RowSet(v, with_lo=False)
    row, col = _sides(caps, vids, t2v, v2t)
    dev = caps.device
    rp, cp, st = engine.cos_count(caps, vids, row, col, band=torch.empty(NA * NB, dtype=torch.int64, device=dev))
    rp, cp, st = rp.cpu().numpy(), cp.cpu().numpy(), st.cpu().numpy()
    need = int(st[1])
    assert st[3] == 0 and need > 8 and st[2] == need and st[0] + need == NA * NB
    assert (rp[np.isnan(row[1].cpu().numpy())] > 0).all()  # the NaN items' words: what a wiping resolve loses
    for cap, overflow in ((8, 1), (need - 1, 1), (need, 0)):
        words = []
        for _ in range(2):
            r2, c2, s2 = engine.cos_count(caps, vids, row, col, band=torch.empty(cap, dtype=torch.int64, device=dev),
                                          resolved=True)
            words.append((r2.cpu().numpy(), c2.cpu().numpy(), s2.cpu().numpy()))
        (r2, c2, s2), (r3, c3, s3) = words
        assert np.array_equal(r2, rp) and np.array_equal(c2, cp), cap
        assert np.array_equal(r2, r3) and np.array_equal(c2, c3) and np.array_equal(s2, s3)
        assert s2[3] == overflow and s2[1] == need and s2[0] == st[0] and s2[2] == (0 if overflow else need)
    # one direction alone, overflowing
    r2, c2, _ = engine.cos_count(caps, vids, row, None, band=torch.empty(8, dtype=torch.int64, device=dev),
                                 resolved=True)
    assert c2 is None and np.array_equal(r2.cpu().numpy(), rp)
    r2, c2, _ = engine.cos_count(caps, vids, None, col, band=torch.empty(8, dtype=torch.int64, device=dev),
                                 resolved=True)
    assert r2 is None and np.array_equal(c2.cpu().numpy(), cp)


@pytest.mark.parametrize("dt", list(DTYPES))
def test_sharded_item_words_sum_to_the_owners(dt):
    import ctypes as C
    import torch
    from cmve import _lib, engine
    c, v, t2v, v2t, _ = _adv(dt)
    caps, vids = engine.RowSet(c, with_lo=False), engine.RowSet(v, with_lo=False)
    dev = caps.device
    off, idx = engine.csr(t2v, dev)
    items = sum(len(l) for l in t2v)
    whole = engine.cos_item_scores(caps, vids, off, idx, items).cpu().numpy().view(np.int64)
    ids = np.array([g for l in t2v for g in l])
    assert np.isnan(whole.view(np.float64)).sum() >= 6
    total = np.zeros(items, np.int64)
    for lo, hi in ((0, 51), (51, 51), (51, 200), (200, 257)):
        part = engine.RowSet(v[lo:hi], with_lo=False)
        w = engine.cos_item_scores(caps, part, off, idx, items, idx_base=lo).cpu().numpy().view(np.int64)
        own = (ids >= lo) & (ids < hi)
        assert np.array_equal(w[own], whole[own]) and (w[~own] == 0).all()
        total += w
    assert np.array_equal(total, whole)  # bit for bit, the NaN items' bits included
    # the column direction: the lists are the shard's videos', the captions are all here (idx_base = 0)
    lo, hi = 3, 201
    part = engine.RowSet(v[lo:hi], with_lo=False)
    coff, cidx = engine.csr(v2t[lo:hi], dev)
    citems = sum(len(l) for l in v2t[lo:hi])
    foff, fidx = engine.csr(v2t, dev)
    full = engine.cos_item_scores(caps, vids, foff, fidx, sum(len(l) for l in v2t), True).cpu().numpy().view(np.int64)
    start = sum(len(l) for l in v2t[:lo])
    got = engine.cos_item_scores(caps, part, coff, cidx, citems, True, idx_base=0).cpu().numpy().view(np.int64)
    assert np.array_equal(got, full[start:start + citems])
    # a negative idx_base is refused before any launch
    out = torch.full((items,), -77.0, dtype=torch.float64, device=dev)
    assert _lib.lib.cmve_cos_item_scores_sharded(engine.handle(dev), C.byref(caps.desc), C.byref(vids.desc),
                                                 off.data_ptr(), idx.data_ptr(), NA, items, 0, -1, out.data_ptr()) < 0
    assert b"cmve_cos_item_scores_sharded" in _lib.lib.cmve_last_error()
    torch.cuda.synchronize()
    assert bool((out == -77.0).all().item())


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------

def test_refusals():
    import torch
    from cmve import _lib, dist as D
    c, v, t2v, v2t, t2v_perf = _adv("f32f32")
    with pytest.raises(ValueError, match='filter="cosine"'):
        D.ShardedGallery(v, offset=0, n_global=NB, measure="l2", filter="cosine")
    with pytest.raises(ValueError, match='filter="cosine"'):
        D.ShardedGallery(v, offset=0, n_global=NB, eps=1e-12, filter="cosine")
    with pytest.raises(ValueError, match='filter="cosine"'):
        D.ShardedGallery(v, offset=0, n_global=NB, with_f16=False, filter="cosine")
    with pytest.raises(ValueError, match="Euclidean"):
        D.ShardedGallery(v, offset=0, n_global=NB, filter=True)
    sh = D.ShardedGallery(v, offset=0, n_global=NB, with_lo=True, filter="cosine")
    q = torch.from_numpy(c).cuda()
    for call in (lambda: sh.evaluate(q, t2v, v2t, mode=_lib.SIM_BF16X3),
                 lambda: sh.cal_perf(q, v2t, t2v_perf, mode=_lib.SIM_BF16X3),
                 lambda: sh.rank_queries(q, sh.local_gt_csr(t2v), NA, mode=_lib.SIM_BF16X3),
                 lambda: sh.rank_queries_device(q, sh.local_gt_csr(t2v), NA, mode=_lib.SIM_BF16X3),
                 lambda: sh.evaluate_device(q, sh.local_gt_csr(t2v), sh.local_v2t_csr(v2t), NA,
                                            mode=_lib.SIM_BF16X3)):
        with pytest.raises(ValueError, match="SIM_F16"):
            call()
    assert sh.filter_stats is None
    want = D.ShardedGallery(v, offset=0, n_global=NB, with_lo=True).evaluate(q, t2v, v2t)
    got = sh.evaluate(q, t2v, v2t)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    _accounted(sh.filter_stats, NA * NB)
    ids, sc = sh.topk(q, 5, mode=_lib.SIM_BF16X3)  # topk is unchanged
    ids0, sc0 = D.ShardedGallery(v, offset=0, n_global=NB, with_lo=True).topk(q, 5, mode=_lib.SIM_BF16X3)
    assert np.array_equal(ids, ids0) and np.array_equal(sc, sc0, equal_nan=True)


# ---- 7. a shard whose band is large keeps the pass ------------------------------------------------------------------------------

def test_one_shard_with_a_band_above_an_eighth_keeps_the_collectives():
    """World 2, one shard clustered around one direction and one of ordinary rows: on the first shard almost every
    cosine lies inside the filter's bound of its item words, so its band exceeds 1/8 of its pairs (where the measure
    family latches its count kernel); the other shard's does not.  Both must go on issuing the one pass's collectives
    -- a shard that changed route alone would leave the other waiting -- so the clustered shard only grows its list:
    the same words as today's route on every call, filter_stats on every pass, no overflow on the pass after."""
    import torch
    from cmve import dist as D
    rng = np.random.default_rng(3)
    na, nb, d, cut = 256, 384, 256, 192
    b = rng.standard_normal((nb, d)).astype(np.float32)
    b[:cut] += 100.0
    a = (100.0 + rng.standard_normal((na, d))).astype(np.float32)
    rows = [[int(j)] for j in rng.integers(0, nb, na)]
    cols = [[int(i)] for i in rng.integers(0, na, cut)] + [[] for _ in range(nb - cut)]
    cuts = (0, cut, nb)

    def run(flt):
        def body(r, comm):
            sh = D.ShardedGallery(b[cuts[r]:cuts[r + 1]], offset=cuts[r], n_global=nb, comm=comm, filter=flt)
            q_local = torch.from_numpy(a[128 * r:128 * r + 128].copy()).cuda()
            out, stats = [], []
            for _ in range(2):
                out.append(sh.evaluate(q_local, rows, cols))
                stats.append(sh.filter_stats)
            out.append(sh.cal_perf(q_local, cols, rows))
            stats.append(sh.filter_stats)
            out.append(sh.rank_queries(q_local, sh.local_gt_csr(rows), na))
            stats.append(sh.filter_stats)
            return out, stats, sh.n

        return D.LocalGroup(2).run(body)

    got, want = run("cosine"), run(None)
    shares = []
    for (out, stats, n), (out0, stats0, _) in zip(got, want):
        print("shard of %d videos:" % n, stats)
        assert stats0 == [None] * 4 and all(st is not None for st in stats)
        for x, y in zip(out[:2], out0[:2]):
            assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])
        np.testing.assert_allclose(np.array(out[2], float), np.array(out0[2], float), rtol=0, atol=1e-12)
        assert np.array_equal(out[3], out0[3]) and np.array_equal(out[3], out0[0][0])
        for st in stats[1:]:  # the list holds the band from the second pass on, however large the band is
            assert st["overflow"] == 0 and st["rescored"] == st["band"] and st["decided"] + st["band"] == na * n
        shares.append(stats[0]["band"] / float(na * n))
    assert shares[0] > 0.125 and shares[1] < 0.125, shares
    assert got[0][1][0]["fallback"]  # the default list is an eighth of the pairs: the first pass was resolved on the device
