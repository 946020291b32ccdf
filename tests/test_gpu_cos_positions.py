"""K26 on the GPU: the exact position of every listed item under cosine, both directions, from ONE fp16 MFMA pass.

The contract: the filter decides only comparisons that its rigorous bound (DESIGN s4, K26) puts out of reach, and
re-scores the rest with the canonical cos64 -- so positions equal ``engine.gt_positions_fused`` and ranks equal
``engine.gt_rank_counts`` WORD FOR WORD, ties, near-ties, zero-norm rows and odd shapes included -- and it must
actually filter: a build that sends every pair to the re-score does not pass."""
import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu

# (n_v, captions per video, d): 4000 x 200 x 128 is synth.multi_caption_embeddings()'s default; 390 x 130 x 67 pads
# d 67 -> 128 and the videos 130 -> 256; 1500 x 300 x 1024 is the benchmark's row width
SHAPES = {"4000x200x128": (200, 20, 128), "390x130x67": (130, 3, 67), "1500x300x1024": (300, 5, 1024)}
DTYPES = {"f32f32": (np.float32, np.float32), "f64f64": (np.float64, np.float64), "f32f64": (np.float32, np.float64)}


def _lists(n_v, per):
    t2v = [[i // per] for i in range(n_v * per)]
    v2t = [list(range(j * per, (j + 1) * per)) for j in range(n_v)]
    return t2v, v2t


_CASES = {}


def _case(shape, dt):
    """The two packed sets, the lists and today's words for them (computed once, never changed)."""
    from cmve import engine
    key = (shape, dt)
    if key not in _CASES:
        n_v, per, d = SHAPES[shape]
        v, c, _, _ = synth.multi_caption_embeddings(n_v=n_v, per=per, d=d)
        caps, vids = engine.RowSet(c.astype(DTYPES[dt][0]), with_lo=False), engine.RowSet(v.astype(DTYPES[dt][1]),
                                                                                         with_lo=False)
        t2v, v2t = _lists(n_v, per)
        _CASES[key] = (caps, vids, t2v, v2t, _oracle(caps, vids, t2v, v2t))
    return _CASES[key]


def _oracle(caps, vids, t2v, v2t):
    """Today's route: positions from the expanded rank pass, ranks from the fused two-direction count."""
    from cmve import engine
    tp = engine.gt_positions_fused(caps, vids, t2v) if t2v is not None else None
    vp = engine.gt_positions_fused(vids, caps, v2t) if v2t is not None else None
    tr, vr, _ = engine.gt_rank_counts(caps, vids, row_gts=t2v, col_gts=v2t)
    return tp, tr, vp, vr


def _assert_same_words(got, want):
    (tp, tr), (vp, vr) = got
    for p, r, wp, wr in ((tp, tr, want[0], want[1]), (vp, vr, want[2], want[3])):
        if wp is None:
            assert p is None and r is None
            continue
        assert len(p) == len(wp)
        for x, y in zip(p, wp):
            assert x.dtype == np.int64 and np.array_equal(x, y), (x, y)
        assert r.dtype == np.int64 and np.array_equal(r, wr)


def _count(caps, vids, t2v, v2t, band=None):
    """One cmve_cos_count over the lists: (row words, column words, the four counters), on the host."""
    import torch
    from cmve import engine
    dev = caps.device
    args = []
    for lists, col_dir, n in ((t2v, False, vids.n), (v2t, True, caps.n)):
        if lists is None:
            args.append(None)
            continue
        off, idx = engine.csr(lists, dev)
        items = sum(len(l) for l in lists)
        args.append((off, engine.cos_item_scores(caps, vids, off, idx, items, col_dir), n))
    if band is not None:
        band = torch.empty(band, dtype=torch.int64, device=dev)
    rp, cp, st = engine.cos_count(caps, vids, args[0], args[1], band=band)
    return (None if rp is None else rp.cpu().numpy(), None if cp is None else cp.cpu().numpy(),
            [int(x) for x in st.cpu().numpy()])


# ---- 1. the words are today's ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_positions_and_ranks_equal_todays_route(shape, dt):
    from cmve import engine
    caps, vids, t2v, v2t, want = _case(shape, dt)
    _assert_same_words(engine.cos_gt_eval(caps, vids, t2v, v2t), want)
    st = engine.cos_gt_eval.stats
    assert st["overflow"] == 0 and not st["redone"]


# ---- 2. reference parity -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["retrieval_multi", "retrieval_c1"])
def test_cal_perf_reproduces_the_reference_tuples(golden, name):
    from cmve.linas import evaluation as E, metrics as M, validate as V
    g = golden(name)
    v, c, vid, cid = synth.multi_caption_embeddings() if name == "retrieval_multi" else synth.c1_embeddings()
    v2t_gt, t2v_gt = M.get_gt(vid, cid)
    errors = E.cal_error(v, c)
    v2t, t2v = V.cal_perf(errors, v2t_gt, t2v_gt, filter="cosine")
    np.testing.assert_allclose(v2t, g["v2t"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(t2v, g["t2v"], rtol=0, atol=1e-12)
    v2t_e, t2v_e = V.cal_perf_embeddings(v, c, vid, cid, filter="cosine")
    np.testing.assert_allclose(v2t_e, g["v2t"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(t2v_e, g["t2v"], rtol=0, atol=1e-12)
    # the two mAPs alone, from the same errors
    assert abs(M.t2v_map(errors, t2v_gt, filter="cosine") - g["t2v"][5]) <= 1e-12
    assert abs(M.v2t_map(errors, v2t_gt, filter="cosine") - g["v2t"][5]) <= 1e-12


def test_auto_route_takes_the_one_pass_count_only_where_it_saves_a_pass(golden, monkeypatch):
    from cmve import engine
    from cmve.linas import validate as V
    g = golden("retrieval_multi")
    v, c, vid, cid = synth.multi_caption_embeddings()
    calls = []
    real = engine.cos_gt_eval_flat  # (what cal_perf's one-pass route calls; cos_gt_eval wraps it too)
    monkeypatch.setattr(engine, "cos_gt_eval_flat", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    monkeypatch.setattr(engine, "COS_FILTER_MIN_PAIRS", None)
    V.cal_perf_embeddings(v, c, vid, cid)
    monkeypatch.setattr(engine, "COS_FILTER_MIN_PAIRS", 4000 * 200 + 1)
    V.cal_perf_embeddings(v, c, vid, cid)
    assert not calls  # never automatically while None, nor below the threshold
    monkeypatch.setattr(engine, "COS_FILTER_MIN_PAIRS", 4000 * 200)
    v2t, t2v = V.cal_perf_embeddings(v, c, vid, cid)
    assert len(calls) == 1
    np.testing.assert_allclose(v2t, g["v2t"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(t2v, g["t2v"], rtol=0, atol=1e-12)
    v1, c1, vid1, cid1 = synth.c1_embeddings(n=300, d=64)  # one caption per video: today's route is one pass
    V.cal_perf_embeddings(v1, c1, vid1, cid1)
    assert len(calls) == 1


@pytest.mark.parametrize("tag", ["a", "b"])
def test_nan_rows_rank_as_the_reference_does(golden, tag):
    """retrieval_nan.npz: zero-norm rows (no eps: NaN scores) -- a lone NaN GT ranks last, a list mixing NaN and finite
    GTs takes the finite one, empty lists give n_m + 1; the rows numpy leaves undefined follow the documented rule."""
    from cmve import engine
    g = golden("retrieval_nan")
    v, c, own = g[tag + "_videos"], g[tag + "_captions"], g[tag + "_owner"]
    t2v = [[int(o)] for o in own]
    v2t = [[i for i in range(c.shape[0]) if own[i] == j] for j in range(v.shape[0])]
    exp_t, exp_v = g[tag + "_t2v_ranks"].astype(np.int64), g[tag + "_v2t_ranks"].astype(np.int64)
    exp_t[~g[tag + "_t2v_defined"]] = v.shape[0]
    exp_v[~g[tag + "_v2t_defined"]] = c.shape[0]
    caps, vids = engine.RowSet(c, with_lo=False), engine.RowSet(v, with_lo=False)
    got = engine.cos_gt_eval(caps, vids, t2v, v2t)
    assert np.array_equal(got[0][1], exp_t) and np.array_equal(got[1][1], exp_v)
    _assert_same_words(got, _oracle(caps, vids, t2v, v2t))


# ---- 3. adversarial lists and rows --------------------------------------------------------------------------------------------

NA, NB, D = 129, 257, 96  # one row past a tile on the caption side, one past two tiles (and the 256-row pad) on the videos'


def _adversarial(dt_c=np.float32, dt_v=np.float32):
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
    return c, v, t2v, v2t


@pytest.fixture(scope="module")
def adversarial():
    from cmve import engine
    c, v, t2v, v2t = _adversarial()
    caps, vids = engine.RowSet(c, with_lo=False), engine.RowSet(v, with_lo=False)
    return caps, vids, t2v, v2t, _oracle(caps, vids, t2v, v2t)


def test_adversarial_rows_and_lists(adversarial):
    from cmve import engine
    caps, vids, t2v, v2t, want = adversarial
    assert {len(l) for l in t2v} >= {0, 1, 37} and {len(l) for l in v2t} >= {0, 1, 37}
    got = engine.cos_gt_eval(caps, vids, t2v, v2t)
    _assert_same_words(got, want)
    # what the definitions say where they can be read off: duplicates tie, NaN items take the list's last places
    tp, vp = got[0][0], got[1][0]
    assert tp[8][0] == tp[8][1] == tp[8][2] and tp[9][0] == tp[9][1]
    assert tp[8][5] == NB and tp[10][0] == NB and list(tp[11][[0, 2]]) == [NB - 1, NB] and list(tp[60]) == [NB - 1, NB]
    assert vp[3][0] == vp[3][1] and vp[3][4] == NA and list(vp[50]) == [NA - 2, NA - 1, NA]
    assert got[0][1][7] == NB + 1 and got[1][1][254] == NA + 1 and got[0][1][60] == NB and got[1][1][50] == NA
    st = engine.cos_gt_eval.stats
    assert st["decided"] + st["band"] == NA * NB and st["rescored"] == st["band"]
    assert st["band"] >= NA + NB - 1  # the NaN row and the NaN column have no bound: all their pairs are band


def test_adversarial_rows_f64_and_mixed():
    from cmve import engine
    for dt_c, dt_v in ((np.float64, np.float64), (np.float32, np.float64)):
        c, v, t2v, v2t = _adversarial(dt_c, dt_v)
        caps, vids = engine.RowSet(c, with_lo=False), engine.RowSet(v, with_lo=False)
        _assert_same_words(engine.cos_gt_eval(caps, vids, t2v, v2t), _oracle(caps, vids, t2v, v2t))


def test_one_direction_only(adversarial):
    from cmve import engine
    caps, vids, t2v, v2t, want = adversarial
    _assert_same_words(engine.cos_gt_eval(caps, vids, row_lists=t2v), (want[0], want[1], None, None))
    _assert_same_words(engine.cos_gt_eval(caps, vids, col_lists=v2t), (None, None, want[2], want[3]))


def test_empty_sides():
    from cmve import engine
    rng = np.random.default_rng(3)
    some = engine.RowSet(rng.standard_normal((5, D)).astype(np.float32), with_lo=False)
    none = engine.RowSet(np.zeros((0, D), np.float32), with_lo=False)
    (tp, tr), (vp, vr) = engine.cos_gt_eval(none, some, [], [[] for _ in range(5)])       # na = 0
    assert tp == [] and tr.size == 0 and all(p.size == 0 for p in vp) and list(vr) == [1] * 5
    (tp, tr), (vp, vr) = engine.cos_gt_eval(some, none, [[] for _ in range(5)], [])       # nb = 0
    assert vp == [] and vr.size == 0 and all(p.size == 0 for p in tp) and list(tr) == [1] * 5
    assert engine.cos_gt_eval.stats["decided"] == 0 and engine.cos_gt_eval.stats["band"] == 0


# ---- 4. band overflow ---------------------------------------------------------------------------------------------------------

def test_band_overflow_reports_the_need_and_one_redo_suffices(adversarial):
    from cmve import engine
    caps, vids, t2v, v2t, want = adversarial
    _, _, full = _count(caps, vids, t2v, v2t)
    assert full[3] == 0 and full[1] > 8
    _, _, st = _count(caps, vids, t2v, v2t, band=8)
    assert st[3] == 1 and st[1] == full[1] and st[2] == 0 and st[0] == full[0]
    _assert_same_words(engine.cos_gt_eval(caps, vids, t2v, v2t, band_cap=8), want)
    assert engine.cos_gt_eval.stats["redone"] and engine.cos_gt_eval.stats["overflow"] == 0
    assert engine.cos_gt_eval.stats["band"] == full[1] == engine.cos_gt_eval.stats["rescored"]


# ---- 5. the filter filters ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", list(SHAPES))
def test_the_filter_decides_almost_every_pair(shape):
    caps, vids, t2v, v2t, _ = _case(shape, "f32f32")
    _, _, st = _count(caps, vids, t2v, v2t)
    pairs = caps.n * vids.n
    print(f"{shape}: decided {st[0]}, band {st[1]} ({100.0 * st[1] / pairs:.3f} % of {pairs} pairs)")
    assert st[3] == 0 and st[0] + st[1] == pairs and st[2] == st[1]
    assert st[1] >= caps.n          # every GT pair equals its own item's word: it cannot be decided
    assert st[1] <= 0.02 * pairs    # (a cap against a kernel that sends everything to the band, not a measurement)


# ---- 6. determinism ------------------------------------------------------------------------------------------------------------

def test_two_calls_give_identical_words_and_counters():
    caps, vids, t2v, v2t, _ = _case("390x130x67", "f32f64")
    a, b = _count(caps, vids, t2v, v2t), _count(caps, vids, t2v, v2t)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


# ---- 7. refusals launch nothing ---------------------------------------------------------------------------------------------------

def test_refusals_leave_the_outputs_untouched():
    import torch
    from cmve import _lib, engine
    rng = np.random.default_rng(9)
    x, y = rng.standard_normal((40, 64)).astype(np.float32), rng.standard_normal((30, 64)).astype(np.float32)
    good_a, good_b = engine.RowSet(x, with_lo=False), engine.RowSet(y, with_lo=False)
    dev = good_a.device
    t2v = [[i % 30] for i in range(40)]
    v2t = [[j] for j in range(30)]
    roff, ridx = engine.csr(t2v, dev)
    coff, cidx = engine.csr(v2t, dev)
    rsc = engine.cos_item_scores(good_a, good_b, roff, ridx, 40)
    csc = engine.cos_item_scores(good_a, good_b, coff, cidx, 30, col_dir=True)
    SENT = -77

    def outputs():
        return (torch.full((40,), SENT, dtype=torch.int32, device=dev),
                torch.full((30,), SENT, dtype=torch.int32, device=dev),
                torch.full((4,), SENT, dtype=torch.int64, device=dev),
                torch.full((64,), SENT, dtype=torch.int64, device=dev),
                torch.full((40,), float(SENT), dtype=torch.float64, device=dev))

    def untouched(outs):
        torch.cuda.synchronize()
        return all(bool((o == SENT).all().item()) for o in outs)

    bad_sets = {
        "no fp16 plane": (engine.RowSet(x, with_lo=False, with_f16=False), good_b),
        "eps != 0": (good_a, engine.RowSet(y, eps=1e-12, with_lo=False)),
        "CMVE_PACK_RAW": (engine.RowSet(x, with_lo=False, raw_rows=True), good_b),
        "mismatched d": (good_a, engine.RowSet(rng.standard_normal((30, 32)).astype(np.float32), with_lo=False)),
    }
    for what, (a, b) in bad_sets.items():
        outs = outputs()
        with pytest.raises((_lib.CmveError, ValueError)):
            engine.cos_count(a, b, (roff, rsc, 30), (coff, csc, 40), band=outs[3], stats=outs[2], row_pos=outs[0],
                             col_pos=outs[1])
        with pytest.raises((_lib.CmveError, ValueError)):
            engine.cos_item_scores(a, b, roff, ridx, 40, out=outs[4])
        assert untouched(outs), what
    # mismatched d at the C entries themselves
    outs = outputs()
    a, b = bad_sets["mismatched d"]
    import ctypes as C
    assert _lib.lib.cmve_cos_count(engine.handle(dev), C.byref(a.desc), C.byref(b.desc), roff.data_ptr(),
                                   rsc.data_ptr(), 40, 30, outs[0].data_ptr(), coff.data_ptr(), csc.data_ptr(), 30, 40,
                                   outs[1].data_ptr(), outs[3].data_ptr(), 512, outs[2].data_ptr()) < 0
    assert b"cmve_cos_count" in _lib.lib.cmve_last_error()
    assert _lib.lib.cmve_cos_item_scores(engine.handle(dev), C.byref(a.desc), C.byref(b.desc), roff.data_ptr(),
                                         ridx.data_ptr(), 40, 40, 0, outs[4].data_ptr()) < 0
    assert b"cmve_cos_item_scores" in _lib.lib.cmve_last_error()
    assert untouched(outs)
    # the lists (flt_check_lists): a negative n, n past int32, item words missing, offsets missing
    h, da, db = engine.handle(dev), C.byref(good_a.desc), C.byref(good_b.desc)
    bad_lists = {
        "negative n": (roff.data_ptr(), rsc.data_ptr(), 40, -1),
        "n past int32": (roff.data_ptr(), rsc.data_ptr(), 40, 1 << 31),
        "negative items": (roff.data_ptr(), rsc.data_ptr(), -1, 30),
        "no item words": (roff.data_ptr(), None, 40, 30),
        "no offsets": (None, rsc.data_ptr(), 40, 30),
    }
    for what, (off, sc, items, n) in bad_lists.items():
        outs = outputs()
        assert _lib.lib.cmve_cos_count(h, da, db, off, sc, items, n, outs[0].data_ptr(), coff.data_ptr(),
                                       csc.data_ptr(), 30, 40, outs[1].data_ptr(), outs[3].data_ptr(), 512,
                                       outs[2].data_ptr()) < 0, what
        assert b"cmve_cos_count" in _lib.lib.cmve_last_error()
        assert untouched(outs), what
    # a workspace that is not 8-byte aligned, and item lists that do not belong to the rows that own them
    outs = outputs()
    assert _lib.lib.cmve_cos_count(h, da, db, roff.data_ptr(), rsc.data_ptr(), 40, 30, outs[0].data_ptr(),
                                   coff.data_ptr(), csc.data_ptr(), 30, 40, outs[1].data_ptr(), outs[3].data_ptr() + 4,
                                   256, outs[2].data_ptr()) < 0
    assert _lib.lib.cmve_cos_item_scores(h, da, db, roff.data_ptr(), ridx.data_ptr(), 39, 40, 0,
                                         outs[4].data_ptr()) < 0
    assert _lib.lib.cmve_cos_item_scores(h, da, db, roff.data_ptr(), ridx.data_ptr(), 40, 40, 2,
                                         outs[4].data_ptr()) < 0
    assert untouched(outs)
    # and the good call still works afterwards
    rp, cp, st = engine.cos_count(good_a, good_b, (roff, rsc, 30), (coff, csc, 40))
    st = st.cpu().numpy()
    assert st[0] + st[1] == 40 * 30 and st[2] == st[1] and st[3] == 0
