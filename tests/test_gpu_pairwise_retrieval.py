"""K18 on the GPU: matrix-free ranks, mAP positions and top-k under the non-cosine measures.

The contract: every decision is taken on the value cmve_pairwise (K10) would store, so the new paths agree WORD
FOR WORD with cmve_gt_positions_from_matrix / cmve_rank_from_matrix / a stable argsort on K10's matrix -- ties,
empty lists and NaN included -- and, on the tie-free recorded fixture, with the reference."""
import contextlib
import io
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MEASURES = ["euclidean", "l1", "l2", "l1_norm", "l2_norm", "jaccard"]
METRICS = ["PW_SQ_L2", "PW_L2", "PW_L1", "PW_ORDER", "PW_JACCARD", "PW_DOT"]


@pytest.fixture(scope="module")
def fx(golden):
    return golden("measures_retrieval")


def _embs(fx, m):
    return (fx["vid_p"], fx["cap_p"]) if m == "jaccard" else (fx["vid"], fx["cap"])


# ---- 1. reference parity through the three routes ----------------------------------------------------------

@pytest.mark.parametrize("m", MEASURES)
def test_reference_parity_cal_perf_embeddings(fx, m):
    from cmve.linas.validate import cal_perf_embeddings
    vid, cap = _embs(fx, m)
    v2t, t2v = cal_perf_embeddings(vid, cap, list(fx["video_ids"]), list(fx["caption_ids"]), measure=m)
    ref = fx["cal_perf_" + m]
    np.testing.assert_allclose(np.array(v2t), ref[0], rtol=0, atol=1e-12)
    np.testing.assert_allclose(np.array(t2v), ref[1], rtol=0, atol=1e-12)


@pytest.mark.parametrize("m", MEASURES)
def test_reference_parity_attribute_route(fx, m):
    """cal_error (cal_error_batch for jaccard: cal_error returns the reference's torch tensor) + cal_perf /
    eval_q2m / t2v_map / v2t_map: the errors carry the device rows and never go back to the GPU."""
    from cmve import engine
    from cmve.linas import evaluation as E, metrics as M, validate as V
    vid, cap = _embs(fx, m)
    errors = E.cal_error_batch(vid, cap, m) if m == "jaccard" else E.cal_error(vid, cap, m)
    assert errors._cmve_pw is not None and errors._cmve is None
    assert (errors * 1.0)._cmve_pw is None and errors.T._cmve_pw is None  # any view or transform drops it
    v2t_gt, t2v_gt = M.get_gt(list(fx["video_ids"]), list(fx["caption_ids"]))
    calls = []
    orig = engine.rank_from_matrix, M.gt_positions
    engine.rank_from_matrix = lambda *a, **k: calls.append("rank_from_matrix") or orig[0](*a, **k)
    M.gt_positions = lambda *a, **k: calls.append("gt_positions") or orig[1](*a, **k)
    try:
        v2t, t2v = V.cal_perf(errors, v2t_gt, t2v_gt)
        t2v_ranks = M.gt_ranks(errors, t2v_gt)
        q2m = M.eval_q2m(errors, t2v_gt)
        t2v_map, v2t_map = M.t2v_map(errors, t2v_gt), M.v2t_map(errors, v2t_gt)
    finally:
        engine.rank_from_matrix, M.gt_positions = orig
    assert calls == [], "the attribute route fell back to the matrix path"
    ref = fx["cal_perf_" + m]
    np.testing.assert_allclose(np.array(v2t), ref[0], rtol=0, atol=1e-12)
    np.testing.assert_allclose(np.array(t2v), ref[1], rtol=0, atol=1e-12)
    assert np.array_equal(t2v_ranks, fx["t2v_ranks_" + m])
    np.testing.assert_allclose(np.array(q2m), fx["t2v_q2m_" + m], rtol=0, atol=1e-12)
    assert abs(t2v_map - float(fx["t2v_map_" + m])) <= 1e-12
    assert abs(v2t_map - float(fx["v2t_map_" + m])) <= 1e-12
    if m == "jaccard":
        import torch
        assert torch.is_tensor(E.cal_error(vid, cap, m))  # the reference's return type: stays on the matrix path


@pytest.mark.parametrize("m", MEASURES)
def test_reference_parity_ranks_and_gallery_scorer(fx, m):
    from cmve import engine
    from cmve.linas import evaluation as E, metrics as M
    from cmve.linas.inference import GalleryScorer
    vid, cap = _embs(fx, m)
    v2t_gt, t2v_gt = M.get_gt(list(fx["video_ids"]), list(fx["caption_ids"]))
    c, v = E.measure_rows(cap, m), E.measure_rows(vid, m)
    metric, alpha, beta, in_dt, sc_dt = E.measure_spec(m, v.shape[1])
    assert c.dtype == in_dt and v.dtype == in_dt
    rr, cr = engine.pairwise_gt_ranks(c, v, metric, alpha, beta, sc_dt, M._lists(t2v_gt, len(cap)), v2t_gt)
    assert np.array_equal(rr, fx["t2v_ranks_" + m]) and np.array_equal(cr, fx["v2t_ranks_" + m])
    scorer = GalleryScorer(vid, list(fx["video_ids"]), measure=m)
    assert scorer.gallery.dtype == in_dt and tuple(scorer.gallery.shape) == vid.shape  # resident, unnormalised
    assert np.array_equal(scorer.topk_indices(cap, 10), fx["top10_" + m])
    one = scorer.topk_ids(cap[3], 10)  # inference.py's case: a single caption
    assert one == [str(fx["video_ids"][j]) for j in fx["top10_" + m][3]]


# ---- 2-4, 7. bit-equality with the matrix path -----------------------------------------------------------------

def _lists(rng, n, n_other):
    """GT lists of 0, 1 and 3 items (repeats allowed)"""
    return [list(map(int, rng.integers(0, n_other, (0, 1, 3)[int(rng.integers(0, 3))]))) if n_other else []
            for _ in range(n)]


def _matrix_path(a, b, metric, alpha, beta, sc_dt, rows, cols):
    from cmve import engine
    from cmve.linas import metrics as M
    e = engine.pairwise(a, b, metric, alpha, beta, sc_dt)
    return (M.gt_positions(e, rows), M.gt_positions(e, cols, transposed=True),
            engine.rank_from_matrix(e, rows), engine.rank_from_matrix(e, cols, transposed=True))


def _assert_same(a, b, metric, alpha, beta, sc_dt, rows, cols):
    from cmve import engine
    rp, cp, rr, cr = _matrix_path(a, b, metric, alpha, beta, sc_dt, rows, cols)
    out = []
    for _ in range(2):  # determinism: two runs return identical arrays
        gp, gc = engine.pairwise_gt_positions(a, b, metric, alpha, beta, sc_dt, rows, cols)
        gr, gcr = engine.pairwise_gt_ranks(a, b, metric, alpha, beta, sc_dt, rows, cols)
        for got, want in ((gp, rp), (gc, cp)):
            assert len(got) == len(want)
            for x, y in zip(got, want):
                assert x.dtype == np.int64 and np.array_equal(x, y)
        assert np.array_equal(gr, rr) and np.array_equal(gcr, cr)
        out.append((np.concatenate(gp + [np.zeros(0, np.int64)]), np.concatenate(gc + [np.zeros(0, np.int64)]), gr,
                    gcr))
    for x, y in zip(*out):
        assert np.array_equal(x, y)
    # one direction alone gives the same words
    only_r = engine.pairwise_gt_ranks(a, b, metric, alpha, beta, sc_dt, row_lists=rows)
    only_c = engine.pairwise_gt_ranks(a, b, metric, alpha, beta, sc_dt, col_lists=cols)
    assert only_r[1] is None and only_c[0] is None
    assert np.array_equal(only_r[0], rr) and np.array_equal(only_c[1], cr)


@pytest.mark.parametrize("shape", [(1, 1, 1), (63, 65, 31), (64, 130, 33), (200, 7, 515)])
@pytest.mark.parametrize("name", METRICS)
def test_bit_equal_with_the_matrix_path(name, shape):
    import torch
    from cmve import _lib
    metric = getattr(_lib, name)
    na, nb, d = shape
    rng = np.random.default_rng(1000 * metric + na)
    pos = name == "PW_JACCARD"
    A = rng.standard_normal((na, d + 5))
    B = rng.standard_normal((nb, d))
    if pos:
        A, B = np.abs(A), np.abs(B)
    if na > 2 and nb > 2:  # duplicated rows on both sides: exact ties, so the strict < is exercised
        A[na // 2] = A[0]
        A[na - 1] = A[0]
        B[nb // 2] = B[1]
        B[nb - 1] = B[1]
        A[1, :d] = B[1]  # and an exact zero distance
    rows, cols = _lists(rng, na, nb), _lists(rng, nb, na)
    if na > 2 and nb > 2:
        rows[0] = [1, nb // 2, nb - 1]  # the tied items themselves
        cols[1] = [0, na // 2, na - 1]
    dev = torch.device("cuda")
    for a_dt, b_dt in ((torch.float64, torch.float64), (torch.float32, torch.float64), (torch.float32, torch.float32)):
        a = torch.from_numpy(A).to(dev, a_dt)[:, :d]  # row-strided A (lda = d + 5)
        b = torch.from_numpy(B).to(dev, b_dt)
        assert a.stride(0) == d + 5
        for sc_dt in (torch.float64, torch.float32):
            _assert_same(a, b, metric, -1.0 / d, -1.0, sc_dt, rows, cols)
    _assert_same(a, b, metric, 1.0, 0.0, torch.float64, rows, cols)


def test_partial_tile_padding_never_counts():
    """65 x 129: one row and one column past the 64 x 128 tile.  K10 stages the tile's missing rows as zeros; with
    A = 0.1 randn a zero row would beat every real item (the distance to the origin is the smallest)."""
    import torch
    from cmve import _lib
    rng = np.random.default_rng(7)
    dev = torch.device("cuda")
    A = torch.from_numpy(0.1 * rng.standard_normal((65, 33))).to(dev)
    B = torch.from_numpy(rng.standard_normal((129, 33))).to(dev)
    for a, b in ((A, B), (B, A)):
        na, nb = a.shape[0], b.shape[0]
        rows = [[int(j)] for j in rng.integers(0, nb, na)]
        cols = [[int(i)] for i in rng.integers(0, na, nb)]
        _assert_same(a, b, _lib.PW_L2, 1.0, 0.0, torch.float64, rows, cols)
        _assert_same(a, b, _lib.PW_L2, 1.0, 0.0, torch.float32, rows, cols)


def test_nan_rules():
    """jaccard of an all-zero caption and an all-zero video is 0 / 0: item lists that are all-NaN, mixed and
    empty must give cmve_gt_positions_from_matrix's / cmve_rank_from_matrix's words."""
    import torch
    from cmve import _lib, engine
    rng = np.random.default_rng(11)
    dev = torch.device("cuda")
    A = np.abs(rng.standard_normal((70, 19))).astype(np.float32)
    B = np.abs(rng.standard_normal((131, 19))).astype(np.float32)
    A[5] = 0.0
    A[66] = 0.0
    B[9] = 0.0
    B[130] = 0.0
    a, b = torch.from_numpy(A).to(dev), torch.from_numpy(B).to(dev)
    e = engine.pairwise(a, b, _lib.PW_JACCARD, -1.0, 0.0, torch.float32).cpu().numpy()
    assert np.isnan(e[5, 9]) and np.isnan(e[66, 130]) and np.isnan(e[5, 130]) and not np.isnan(e[5, 8])
    rows = [[int(j)] for j in rng.integers(0, 131, 70)]
    cols = [[int(i)] for i in rng.integers(0, 70, 131)]
    rows[5] = [9, 130]          # all NaN
    rows[66] = [130, 3, 9, 4]   # mixed
    rows[7] = []                # empty
    rows[8] = [9, 130, 9]       # finite scores of a row that holds NaN elsewhere (video 9 / 130 are zero rows)
    cols[9] = [5, 66]
    cols[130] = [66, 1, 5]
    cols[10] = []
    cols[11] = [5, 66, 2]
    _assert_same(a, b, _lib.PW_JACCARD, -1.0, 0.0, torch.float32, rows, cols)
    _assert_same(a, b, _lib.PW_JACCARD, 1.0, 0.0, torch.float64, rows, cols)
    rr, cr = engine.pairwise_gt_ranks(a, b, _lib.PW_JACCARD, -1.0, 0.0, torch.float32, rows, cols)
    assert rr[5] == 131 and rr[7] == 132 and cr[9] == 70 and cr[10] == 71


# ---- 5, 7. top-k ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def topk_case():
    """65 queries x 1000 gallery rows, d = 33; gallery rows 128 apart are exact duplicates (index order decides
    the tie ACROSS the 128-column chunks); K10's matrix and its stable argsort, computed once."""
    import torch
    from cmve import _lib, engine
    rng = np.random.default_rng(5)
    G = rng.standard_normal((1000, 33))
    Q = rng.standard_normal((65, 33))
    G[3] = Q[0] + 0.01 * rng.standard_normal(33)   # the nearest rows of queries 0 and 5 ...
    G[77] = Q[5] + 0.01 * rng.standard_normal(33)
    for j in range(128, 1000, 128):                # ... have an exact copy in every later chunk
        G[j + 3] = G[3]
        G[j + 77] = G[77]
    dev = torch.device("cuda")
    q, g = torch.from_numpy(Q).to(dev), torch.from_numpy(G).to(dev)
    e = engine.pairwise(q, g, _lib.PW_L1, 1.0, 0.0, torch.float64).cpu().numpy()
    order = np.argsort(e, axis=1, kind="stable")
    assert list(order[0, :8]) == list(range(3, 1000, 128)) and len(set(e[0, order[0, :8]])) == 1
    return q, g, e, order


@pytest.mark.parametrize("n_q", [1, 7, 9, 65])
def test_topk_equals_stable_argsort(topk_case, n_q):
    import torch
    from cmve import _lib, engine
    q, g, e, order = topk_case
    args = (_lib.PW_L1, 1.0, 0.0, torch.float64)
    for k in (1, 10, 1000):
        lo, rec = engine.pairwise_topk_workspace(n_q, 1000, k, _lib.PW_L1)
        assert lo == n_q * k * 32 + n_q * 128 * 8 < rec  # the minimum holds one of the eight 128-column chunks
        want_i, want_e = order[:n_q, :k], np.take_along_axis(e[:n_q], order[:n_q, :k], 1)
        runs = []
        for ws_bytes in (rec, lo, rec):  # recommended, minimum (eight chunks merge), and again (determinism)
            idx, err = engine.pairwise_topk(q[:n_q], g, *args, k, ws_bytes=ws_bytes)
            assert idx.dtype == np.int64 and np.array_equal(idx, want_i)
            assert np.array_equal(err, want_e)
            runs.append((idx, err))
        assert np.array_equal(runs[0][0], runs[2][0]) and np.array_equal(runs[0][1], runs[2][1])


def test_topk_geometries_and_limits(topk_case):
    import torch
    from cmve import _lib, engine
    q, g, e, order = topk_case
    for name, sc_dt in (("PW_L1", torch.float64), ("PW_L2", torch.float32), ("PW_DOT", torch.float64)):
        metric = getattr(_lib, name)
        small = engine.pairwise_topk(q[:8], g, metric, -0.5, 2.0, sc_dt, 10, geometry=2)
        wide = engine.pairwise_topk(q[:8], g, metric, -0.5, 2.0, sc_dt, 10, geometry=1)
        auto = engine.pairwise_topk(q[:8], g, metric, -0.5, 2.0, sc_dt, 10)
        mat = engine.pairwise(q[:8], g, metric, -0.5, 2.0, sc_dt).cpu().numpy().astype(np.float64)
        o = np.argsort(mat, axis=1, kind="stable")[:, :10]
        for idx, err in (small, wide, auto):
            assert np.array_equal(idx, o) and np.array_equal(err, np.take_along_axis(mat, o, 1))
    with pytest.raises(_lib.CmveError, match="geometry"):
        engine.pairwise_topk(q[:9], g, _lib.PW_L1, 1.0, 0.0, torch.float64, 10, geometry=2)
    # k > n_g clamps
    idx, err = engine.pairwise_topk(q[:3], g[:5], _lib.PW_L1, 1.0, 0.0, torch.float64, 10)
    assert idx.shape == (3, 5) and np.array_equal(idx, np.argsort(e[:3, :5], axis=1, kind="stable"))
    # k > TOPK_MAX raises
    big = torch.zeros((_lib.TOPK_MAX + 10, 33), dtype=torch.float64, device=g.device)
    with pytest.raises(ValueError, match="k <="):
        engine.pairwise_topk(q[:1], big, _lib.PW_L1, 1.0, 0.0, torch.float64, _lib.TOPK_MAX + 1)
    # f32 queries against the fp64 gallery, a row-strided gallery view, NaN last
    qn = q[:4].to(torch.float32).clone()
    gv = torch.cat([g, g], 1)[:, :33]
    assert gv.stride(0) == 66
    idx, err = engine.pairwise_topk(qn, gv, _lib.PW_L2, 1.0, 0.0, torch.float64, 12)
    mat = engine.pairwise(qn, gv, _lib.PW_L2, 1.0, 0.0, torch.float64).cpu().numpy()
    assert np.array_equal(idx, np.argsort(mat, axis=1, kind="stable")[:, :12])
    gz = torch.abs(g[:300].to(torch.float32)).clone()
    gz[17] = 0.0
    gz[250] = 0.0
    qz = torch.abs(q[:2].to(torch.float32)).clone()
    qz[1] = 0.0  # every error of query 1 is NaN or -0/x = 0
    idx, err = engine.pairwise_topk(qz, gz, _lib.PW_JACCARD, -1.0, 0.0, torch.float32, 300,
                                    ws_bytes=engine.pairwise_topk_workspace(2, 300, 300, _lib.PW_JACCARD)[0])
    mat = engine.pairwise(qz, gz, _lib.PW_JACCARD, -1.0, 0.0, torch.float32).cpu().numpy().astype(np.float64)
    o = np.argsort(mat, axis=1, kind="stable")
    assert np.array_equal(idx, o) and np.array_equal(err, np.take_along_axis(mat, o, 1), equal_nan=True)
    assert np.isnan(err[1, -2:]).all() and list(idx[1, -2:]) == [17, 250] and not np.isnan(err[0]).any()
    # NaN on the segmented route (few queries, the recommended workspace: three 128-column segments, the last one
    # padded): query 1 ties at -0 against the 49 non-zero rows (251..299; row 250 is zero already), then NaN in index order
    gz[:250] = 0.0
    idx, err = engine.pairwise_topk(qz, gz, _lib.PW_JACCARD, -1.0, 0.0, torch.float32, 100)
    mat = engine.pairwise(qz, gz, _lib.PW_JACCARD, -1.0, 0.0, torch.float32).cpu().numpy().astype(np.float64)
    o = np.argsort(mat, axis=1, kind="stable")[:, :100]
    assert np.array_equal(idx, o) and np.array_equal(err, np.take_along_axis(mat, o, 1), equal_nan=True)
    assert list(idx[1]) == list(range(251, 300)) + list(range(51)) and np.isnan(err[1, 49:]).all()


# ---- 6. memory ---------------------------------------------------------------------------------------------------

def test_no_buffer_proportional_to_the_pair_count():
    import torch
    from cmve import _lib, engine
    from cmve.linas.validate import cal_perf_embeddings
    MIB = 1 << 20
    dev = torch.device("cuda")
    gen = torch.Generator(device="cpu").manual_seed(3)
    # evaluation: 2,000 captions x 3,000 videos x 64 -- the fp64 matrix would be 48 MB
    vid = torch.randn((3000, 64), generator=gen, dtype=torch.float64).to(dev)
    cap = torch.randn((2000, 64), generator=gen, dtype=torch.float64).to(dev)
    video_ids = ["v%d" % j for j in range(3000)]
    caption_ids = ["v%d#0" % (i % 3000) for i in range(2000)]
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    v2t, t2v = cal_perf_embeddings(vid, cap, video_ids, caption_ids, measure="l1")
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print("cal_perf_embeddings(l1) 2000 x 3000 x 64: peak rise %.2f MiB" % (rise / MIB))
    assert rise < 8 * MIB
    assert len(v2t) == 6 and len(t2v) == 6 and 0.0 < t2v[5] <= 1.0
    del vid, cap
    # top-k: 3,000 queries x 40,000 gallery rows x 8 -- the fp64 matrix would be 960 MB
    g = torch.randn((40000, 8), generator=gen, dtype=torch.float64).to(dev)
    q = torch.randn((3000, 8), generator=gen, dtype=torch.float64).to(dev)
    rec = engine.pairwise_topk_workspace(3000, 40000, 10, _lib.PW_L1)[1]
    assert rec <= 256 * MIB + 3000 * 10 * 32
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    idx, err = engine.pairwise_topk(q, g, _lib.PW_L1, 1.0, 0.0, torch.float64, 10, to_host=False)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print("pairwise_topk 3000 x 40000 x 8: peak rise %.2f MiB (recommended workspace %.2f MiB)"
          % (rise / MIB, rec / MIB))
    assert rise <= rec + 8 * MIB
    # spot-check three queries against K10's rows
    for i in (0, 1499, 2999):
        row = engine.pairwise(q[i:i + 1], g, _lib.PW_L1, 1.0, 0.0, torch.float64).cpu().numpy()[0]
        o = np.argsort(row, kind="stable")[:10]
        assert np.array_equal(idx[i].cpu().numpy(), o) and np.array_equal(err[i].cpu().numpy(), row[o])


# ---- 8. CLI --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", ["l1", "jaccard"])
def test_cli_non_cosine_branch(fx, m, tmp_path, monkeypatch):
    """inference.main(--gallery ... --query-emb ... --measure m) and a direct call of its retrieval branch: the
    ids printed are the fixture's."""
    from cmve.linas import inference
    vid, cap = _embs(fx, m)
    gal, qry = str(tmp_path / "gallery.npz"), str(tmp_path / "query.npy")
    np.savez(gal, video_embs=vid, video_ids=fx["video_ids"])
    np.save(qry, cap[11:12])
    want = [str(fx["video_ids"][j]) for j in fx["top10_" + m][11]]
    # the branch itself
    assert inference._retrieve(vid, [str(v) for v in fx["video_ids"]], cap[11:12], m, 10) == want

    # through main(): --gallery + --query-emb bypass the checkpoint, --measure stands in for its opt.measure
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", os.environ.get("HIP_VISIBLE_DEVICES", "0"))  # main() exports --gpu
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        got = inference.main(["--gallery", gal, "--query-emb", qry, "--topK", "10", "--measure", m,
                              "--gpu", os.environ["HIP_VISIBLE_DEVICES"]])
    assert got == want
    assert buf.getvalue().strip() == str(want)
