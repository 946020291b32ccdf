"""ShardedGallery(..., measure=) on the GPU: the sharded evaluation and top-k under the six non-cosine measures
(LINAS-engine/evaluation.py:17-36), the shards in ONE process through LocalGroup (one thread + HIP stream each).

The contract: K18's positions count with a strict < and no index tie-break, so a position is the plain sum over the
gallery shards of their counts against the same item score -- the sharded result is WORD FOR WORD the unsharded
one (engine.pairwise_gt_eval / engine.pairwise_topk on the concatenated gallery), ties and NaN included, and on
the tie-free recorded fixture it is the reference's."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MEASURES = ["euclidean", "l1", "l2", "l1_norm", "l2_norm", "jaccard"]
METRICS = ["PW_SQ_L2", "PW_L2", "PW_L1", "PW_ORDER", "PW_JACCARD", "PW_DOT"]
CUTS = [(0, 141), (0, 70, 141), (0, 128, 141), (0, 64, 128, 141), (0, 141, 141), (0, 0, 141)]


@pytest.fixture(scope="module")
def fx(golden):
    return golden("measures_retrieval")


@pytest.fixture(scope="module")
def gts(fx):
    from oracle import retrieval as R
    return R.get_gt(list(fx["video_ids"]), list(fx["caption_ids"]))  # (v2t list, t2v dict)


def _embs(fx, m):
    return (fx["vid_p"], fx["cap_p"]) if m == "jaccard" else (fx["vid"], fx["cap"])


def _words(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def _slices(n, world, even):
    """Caption slices per rank: equal, or uneven (the all_gather_var route)."""
    if even or world == 1:
        return np.linspace(0, n, world + 1).astype(int)
    c = np.linspace(0, n, world + 1).astype(int)
    c[1:-1] += 3
    return c


# ---- 1. reference parity -------------------------------------------------------------------------------------

@pytest.mark.parametrize("cuts", CUTS, ids=lambda c: "-".join(map(str, c)))
@pytest.mark.parametrize("m", MEASURES)
def test_reference_parity_over_shards(fx, gts, m, cuts):
    import torch
    from cmve import dist as D
    vid, cap = _embs(fx, m)
    v2t, t2v = gts
    n_g, n_q, world = vid.shape[0], cap.shape[0], len(cuts) - 1
    t2v_lists = [t2v[i] for i in range(n_q)]
    qc = _slices(n_q, world, even=False)

    def body(r, comm):
        sh = D.ShardedGallery(vid[cuts[r]:cuts[r + 1]], offset=cuts[r], n_global=n_g, comm=comm, measure=m)
        assert sh.shard.shape == (cuts[r + 1] - cuts[r], vid.shape[1])  # resident, unnormalised
        q_local = torch.from_numpy(cap[qc[r]:qc[r + 1]].copy()).cuda()
        return sh.evaluate(q_local, t2v_lists, v2t), sh.cal_perf(q_local, v2t, t2v), sh.topk(q_local, 10)

    ref = fx["cal_perf_" + m]
    for (r_t, r_v), perf, (ids, err) in D.LocalGroup(world).run(body):
        assert np.array_equal(r_t, fx["t2v_ranks_" + m]) and np.array_equal(r_v, fx["v2t_ranks_" + m])
        np.testing.assert_allclose(np.array(perf[0], float), ref[0], rtol=0, atol=1e-12)
        np.testing.assert_allclose(np.array(perf[1], float), ref[1], rtol=0, atol=1e-12)
        assert ids.dtype == np.int64 and np.array_equal(ids, fx["top10_" + m])
        assert err.dtype == np.float64 and (np.diff(err, axis=1) >= 0).all()


# ---- 2. word-for-word equality with the unsharded K18 -------------------------------------------------------------

def _tied_problem(m):
    """40 captions x 37 videos, D = 5, entries in {0, 1, 2}: many tied pairs; duplicate gallery rows in different
    shards; one gallery row and one caption row with NaN; an all-zero row on each side (jaccard's 0 / 0); GT lists
    of 0, 1 and 3 items with repeats."""
    rng = np.random.default_rng(17)
    dt = np.float32 if m == "jaccard" else np.float64
    G = rng.integers(0, 3, (37, 5)).astype(dt)
    Q = rng.integers(0, 3, (40, 5)).astype(dt)
    G[30] = G[2]
    G[14] = G[12]
    G[13] = G[12]       # a tie straddling the cut at 13
    Q[7] = G[12]        # and a caption at distance 0 from the three
    G[20] = 0.0
    Q[9] = 0.0
    G[33, 1] = np.nan
    Q[21, 4] = np.nan
    sizes = (0, 1, 3)
    t2v = [list(map(int, rng.integers(0, 37, sizes[int(rng.integers(0, 3))]))) for _ in range(40)]
    v2t = [list(map(int, rng.integers(0, 40, sizes[int(rng.integers(0, 3))]))) for _ in range(37)]
    t2v[7], t2v[9], t2v[21], t2v[3] = [13, 12, 14], [20, 33, 20], [5], [33, 33, 1]
    v2t[20], v2t[33], v2t[12] = [9, 21, 9], [4], [7, 7, 21]
    return G, Q, t2v, v2t


@pytest.mark.parametrize("cuts", [(0, 13, 37), (0, 5, 5, 20, 37), (0, 0, 31, 37)], ids=lambda c: "-".join(map(str, c)))
@pytest.mark.parametrize("m", MEASURES)
def test_word_equal_with_the_unsharded_k18(m, cuts):
    import torch
    from cmve import engine, dist as D
    from cmve.linas import evaluation as E
    G, Q, t2v, v2t = _tied_problem(m)
    n_g, n_q, world = G.shape[0], Q.shape[0], len(cuts) - 1
    c, v = E.measure_rows(Q, m), E.measure_rows(G, m)
    metric, alpha, beta, _, sc_dt = E.measure_spec(m, 5)
    (tp, tr), (vp, vr) = engine.pairwise_gt_eval(c, v, metric, alpha, beta, sc_dt, t2v, v2t)
    want_i, want_e = engine.pairwise_topk(c, v, metric, alpha, beta, sc_dt, 10)
    tp = np.concatenate(tp + [np.zeros(0, np.int64)]) - 1
    qc = _slices(n_q, world, even=False)

    def body(r, comm):
        sh = D.ShardedGallery(G[cuts[r]:cuts[r + 1]], offset=cuts[r], n_global=n_g, comm=comm, measure=m)
        q_local = torch.from_numpy(Q[qc[r]:qc[r + 1]].copy()).cuda()
        out = []
        for _ in range(2):  # determinism: two runs give the same words
            q_all = D.all_gather_var(q_local, comm)
            t_r, t_p, v_r, v_p = sh._pw_evaluate_gathered(sh._pw_rows(q_all), n_q, t2v, v2t)
            ids, err = sh.topk(q_local, 10)
            out.append((t_r, t_p, v_r, v_p, ids, err))
        return out

    res = D.LocalGroup(world).run(body)
    for r, runs in enumerate(res):
        for t_r, t_p, v_r, v_p, ids, err in runs:
            assert np.array_equal(t_r, tr) and np.array_equal(t_p, tp)
            assert np.array_equal(v_r, vr)
            want_vp = np.concatenate(vp[cuts[r]:cuts[r + 1]] + [np.zeros(0, np.int64)]) - 1
            assert np.array_equal(v_p, want_vp)
            assert np.array_equal(ids, want_i) and np.array_equal(_words(err), _words(want_e))
        for x, y in zip(*runs):
            assert np.array_equal(x, y, equal_nan=True)
    if m != "jaccard":  # (fmin / fmax drop a NaN operand: jaccard's NaN comes from the all-zero rows instead)
        assert np.isnan(want_e[21]).all() and np.isnan(want_e[:, -1]).sum() == 1  # the NaN caption; NaN ranks last


# ---- 3. the entries alone, no communicator ---------------------------------------------------------------------------

def _lists(rng, n, n_other):
    return [list(map(int, rng.integers(0, n_other, (0, 1, 3)[int(rng.integers(0, 3))]))) if n_other else []
            for _ in range(n)]


def _sharded_by_hand(a, b, args, rows, cols, cuts, n_owner=0):
    """Positions and ranks of both directions from the three entries over slices of b: the item scores merged by
    an int64 SUM of their words, the row positions summed, the column positions concatenated."""
    import torch
    from cmve import engine
    dev = a.device
    na, nb = a.shape[0], b.shape[0]
    roff, ridx = engine.csr(rows, dev)
    ritems = sum(len(l) for l in rows)
    words = torch.zeros(ritems, dtype=torch.int64, device=dev)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        words += engine.pairwise_item_scores(a, b[lo:hi], *args, roff, ridx, ritems, False, lo).view(torch.int64)
    row_sc = words.view(torch.float64)
    row_pos = torch.zeros(ritems, dtype=torch.int64, device=dev)
    col_pos, col_sc = [], []
    for s, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
        coff, cidx = engine.csr(cols[lo:hi], dev)
        citems = sum(len(l) for l in cols[lo:hi])
        csc = engine.pairwise_item_scores(a, b[lo:hi], *args, coff, cidx, citems, True, 0)
        rp, cp = engine.pairwise_count(a, b[lo:hi], *args, row=(roff, row_sc, nb if s == n_owner else 0),
                                       col=(coff, csc, na))
        assert rp.dtype == torch.int32 and cp.dtype == torch.int32 and rp.is_cuda
        row_pos += rp
        col_pos.append(cp)
        col_sc.append(csc)
    col_pos, col_sc = torch.cat(col_pos), torch.cat(col_sc)
    coff, _ = engine.csr(cols, dev)
    rr = engine.pairwise_list_ranks(roff, row_sc, row_pos.to(torch.int32), nb)
    cr = engine.pairwise_list_ranks(coff, col_sc, col_pos, na)
    assert rr.dtype == torch.int64 and rr.is_cuda
    return row_pos.cpu().numpy(), col_pos.cpu().numpy().astype(np.int64), rr.cpu().numpy(), cr.cpu().numpy()


@pytest.mark.parametrize("shape", [(1, 1, 1), (63, 65, 31), (64, 130, 33), (200, 7, 515)])
@pytest.mark.parametrize("name", METRICS)
def test_entries_sum_to_the_whole(name, shape):
    import torch
    from cmve import _lib, engine
    metric = getattr(_lib, name)
    na, nb, d = shape
    rng = np.random.default_rng(2000 * metric + na)
    A = rng.standard_normal((na, d + 3))
    B = rng.standard_normal((nb, d))
    if name == "PW_JACCARD":
        A, B = np.abs(A), np.abs(B)
    if na > 2 and nb > 2:  # duplicates on both sides (exact ties), a NaN row on each side and, for jaccard (whose
        A[na - 1] = A[0]   # fmin / fmax drop a NaN operand), a 0 / 0 pair
        B[nb // 2] = B[1]
        B[nb - 1] = B[1]
        A[na - 2, 0] = np.nan
        B[nb - 2, 0] = np.nan
        if name == "PW_JACCARD":
            A[2] = 0.0
            B[2] = 0.0
    rows, cols = _lists(rng, na, nb), _lists(rng, nb, na)
    if na > 2 and nb > 2:
        rows[0] = [1, nb // 2, nb - 1]
        rows[2] = [2, 0, 2]
        cols[2] = [2, 2, 1]
        rows[1] = [nb - 2, 0, nb - 2]          # NaN items beside a number: the NaN rule summed over the slices
        rows[na - 2] = [1, nb - 2]             # a NaN caption row: every item NaN
        cols[nb - 2] = [0, na - 2, 0]          # a NaN video row, in whichever slice holds it
        cols[1] = [na - 2, 3, na - 2]
    dev = torch.device("cuda")
    for dt in (torch.float64, torch.float32):
        a = torch.from_numpy(A).to(dev, dt)[:, :d]  # row-strided A
        b = torch.from_numpy(B).to(dev, dt)
        args = (metric, -1.0 / d, -1.0, dt)
        wp, wc = engine.pairwise_gt_positions(a, b, *args, rows, cols)
        wr, wcr = engine.pairwise_gt_ranks(a, b, *args, rows, cols)
        wp = np.concatenate(wp + [np.zeros(0, np.int64)]) - 1
        wc = np.concatenate(wc + [np.zeros(0, np.int64)]) - 1
        for cut in (min(128, nb), nb // 2, 0):  # a tile edge (or an empty last slice), off it, an empty first slice
            for owner in (0, 1):                # whichever slice passes n: the sum is the same
                rp, cp, rr, cr = _sharded_by_hand(a, b, args, rows, cols, (0, cut, nb), owner)
                assert np.array_equal(rp, wp) and np.array_equal(cp, wc), (cut, owner)
                assert np.array_equal(rr, wr) and np.array_equal(cr, wcr), (cut, owner)


def test_nan_rule_of_the_count_entry():
    """row_n = 0 leaves a NaN item's word 0; an EMPTY slice given the n still applies the rule; list_ranks on empty
    and all-NaN lists."""
    import torch
    from cmve import _lib, engine
    dev = torch.device("cuda")
    rng = np.random.default_rng(3)
    a = torch.from_numpy(rng.standard_normal((5, 9))).to(dev)
    b = torch.from_numpy(rng.standard_normal((7, 9))).to(dev)
    args = (_lib.PW_L1, 1.0, 0.0, torch.float64)
    rows = [[0, 1, 2], [], [3], [4, 4], [5]]
    off, _ = engine.csr(rows, dev)
    nan = float("nan")
    sc = torch.tensor([nan, 1e9, nan, nan, -1.0, nan, 1e9], dtype=torch.float64, device=dev)
    p0, none = engine.pairwise_count(a, b, *args, row=(off, sc, 0))
    assert none is None and p0.tolist() == [0, 7, 0, 0, 0, 0, 7]
    p7, _ = engine.pairwise_count(a, b, *args, row=(off, sc, 100))
    assert p7.tolist() == [98, 7, 99, 99, 0, 99, 7]
    pe, _ = engine.pairwise_count(a, b[:0], *args, row=(off, sc, 100))  # an empty shard that passes the n
    assert pe.tolist() == [98, 0, 99, 99, 0, 99, 0]
    pz, _ = engine.pairwise_count(a, b[:0], *args, row=(off, sc, 0))
    assert pz.tolist() == [0] * 7
    # the column direction over an empty A
    coff, _ = engine.csr([[0], [], [1, 1]] + [[]] * 4, dev)
    csc = torch.tensor([nan, 2.0, nan], dtype=torch.float64, device=dev)
    _, ce = engine.pairwise_count(a[:0], b, *args, col=(coff, csc, 40))
    assert ce.tolist() == [39, 0, 39]
    ranks = engine.pairwise_list_ranks(off, sc, p7, 100)
    assert ranks.tolist() == [8, 101, 100, 1, 8]
    assert engine.pairwise_list_ranks(off[:1], sc[:0], p7[:0], 100).numel() == 0


# ---- 4. top-k edges -----------------------------------------------------------------------------------------------------

def test_topk_edges():
    import torch
    from cmve import engine, dist as D
    from cmve.linas import evaluation as E
    m = "l1"
    G, Q, _, _ = _tied_problem(m)
    G, Q = np.nan_to_num(G, nan=1.0), np.nan_to_num(Q, nan=1.0)
    n_g, cuts = G.shape[0], (0, 13, 37)
    c, v = E.measure_rows(Q, m), E.measure_rows(G, m)
    metric, alpha, beta, _, sc_dt = E.measure_spec(m, 5)
    want = {k: engine.pairwise_topk(c, v, metric, alpha, beta, sc_dt, k) for k in (30, 50)}
    one = engine.pairwise_topk(c[7:8], v, metric, alpha, beta, sc_dt, 10)
    assert want[50][0].shape == (40, 37) and list(one[0][0, :3]) == [12, 13, 14] and one[1][0, 2] == 0.0

    def body(r, comm):
        sh = D.ShardedGallery(G[cuts[r]:cuts[r + 1]], offset=cuts[r], n_global=n_g, comm=comm, measure=m)
        q_local = torch.from_numpy(Q[20 * r:20 * r + 20].copy()).cuda()
        single = torch.from_numpy(Q[7:8] if r == 0 else Q[:0]).cuda()  # one caption, held by rank 0 alone
        return sh.topk(q_local, 30), sh.topk(q_local, 50), sh.topk(single, 10)

    for k30, k50, single in D.LocalGroup(2).run(body):
        for got, exp in ((k30, want[30]), (k50, want[50]), (single, one)):  # k > both shards; k > n_global clamps
            assert got[0].shape == exp[0].shape
            assert np.array_equal(got[0], exp[0]) and np.array_equal(_words(got[1]), _words(exp[1]))


# ---- 5. world-1 CAbiComm: the int64 SUM goes through cmve_dist_allreduce on the device --------------------------------

def test_world1_over_the_c_abi_communicator(fx, gts):
    import torch
    from cmve.dist import CAbiComm, ShardedGallery
    m = "l1"
    vid, cap = _embs(fx, m)
    v2t, t2v = gts
    n_g, n_q = vid.shape[0], cap.shape[0]
    dev = torch.device("cuda", 0)
    comm = CAbiComm(dev)
    try:
        calls = []
        reduce = comm.all_reduce
        comm.all_reduce = lambda t, op: calls.append((t.dtype, op)) or reduce(t, op)
        sh = ShardedGallery(vid, offset=0, n_global=n_g, device=dev, comm=comm, measure=m)
        qt = torch.from_numpy(cap).to(dev)
        r_t, r_v = sh.evaluate(qt, [t2v[i] for i in range(n_q)], v2t)
        assert calls[:2] == [(torch.int64, "sum"), (torch.int64, "sum")]  # the score words, then the positions
        assert np.array_equal(r_t, fx["t2v_ranks_" + m]) and np.array_equal(r_v, fx["v2t_ranks_" + m])
        perf = sh.cal_perf(qt, v2t, t2v)
        np.testing.assert_allclose(np.array(perf, float), fx["cal_perf_" + m], rtol=0, atol=1e-12)
        ids, _ = sh.topk(qt, 10)
        assert np.array_equal(ids, fx["top10_" + m])
    finally:
        comm.close()


# ---- 6. argument checks of the three entries ----------------------------------------------------------------------------

def test_argument_checks_name_their_entry():
    import torch
    from cmve import _lib, engine
    lib = _lib.lib
    dev = torch.device("cuda")
    h = engine.handle(dev)
    a = torch.zeros((4, 8), dtype=torch.float64, device=dev)
    b = torch.zeros((6, 8), dtype=torch.float64, device=dev)
    off, idx = engine.csr([[0], [1], [2], [3]], dev)
    coff, _ = engine.csr([[0]] * 6, dev)
    sc = torch.zeros(6, dtype=torch.float64, device=dev)
    pos = torch.zeros(6, dtype=torch.int32, device=dev)
    out = torch.zeros(4, dtype=torch.int64, device=dev)
    P, F64, L1 = engine._ptr, _lib.CMVE_F64, _lib.PW_L1

    def items(A=P(a), a_dt=F64, lda=8, na=4, B=P(b), b_dt=F64, ldb=8, nb=6, d=8, metric=L1, s_dt=F64, o=P(off),
              i=P(idx), n_lists=4, n_items=4, col_dir=0, res=P(sc)):
        return lib.cmve_pairwise_item_scores(h, A, a_dt, lda, na, B, b_dt, ldb, nb, d, metric, 1.0, 0.0, s_dt, o, i,
                                             n_lists, n_items, col_dir, 0, res)

    def count(A=P(a), a_dt=F64, lda=8, na=4, B=P(b), ldb=8, nb=6, d=8, metric=L1, ro=P(off), rs=P(sc), ri=4, rn=6,
              rp=P(pos), co=None, cs=None, ci=0, cn=0, cp=None):
        return lib.cmve_pairwise_count(h, A, a_dt, lda, na, B, F64, ldb, nb, d, metric, 1.0, 0.0, F64, ro, rs, ri, rn,
                                       rp, co, cs, ci, cn, cp)

    def bad(rc, entry, what):
        err = lib.cmve_last_error()
        assert rc < 0 and entry in err and what in err, (rc, err)

    assert items() == 0 and count() == 0
    e = b"cmve_pairwise_item_scores"
    bad(items(A=None), e, b"NULL")
    bad(items(o=None), e, b"NULL")
    bad(items(res=None), e, b"NULL")
    bad(items(a_dt=_lib.CMVE_I32), e, b"dtypes")
    bad(items(s_dt=7), e, b"dtypes")
    bad(items(lda=7), e, b"bad shape")       # d mismatch: a row shorter than d
    bad(items(d=0), e, b"bad shape")
    bad(items(na=-1, n_lists=-1), e, b"bad shape")
    bad(items(n_items=-1), e, b"item count")
    bad(items(metric=99), e, b"unknown metric")
    bad(items(n_lists=6), e, b"lists")       # row lists, but one per B row
    bad(items(col_dir=2), e, b"col_dir")
    e = b"cmve_pairwise_count"
    bad(count(B=None), e, b"NULL")
    bad(count(a_dt=3), e, b"dtypes")
    bad(count(ldb=5), e, b"bad shape")
    bad(count(nb=-2), e, b"bad shape")
    bad(count(ri=-1), e, b"bad counts")
    bad(count(rn=-1), e, b"bad counts")
    bad(count(metric=-1), e, b"unknown metric")
    bad(count(ro=None), e, b"row lists missing")
    bad(count(rs=None), e, b"row lists missing")
    bad(count(cp=P(pos), co=None, ci=6), e, b"column lists missing")
    bad(count(cp=P(pos), co=P(coff), cs=None, ci=6), e, b"column lists missing")
    e = b"cmve_pairwise_list_ranks"
    assert lib.cmve_pairwise_list_ranks(h, P(off), P(sc), P(pos), 4, 6, P(out)) == 0
    bad(lib.cmve_pairwise_list_ranks(h, None, P(sc), P(pos), 4, 6, P(out)), e, b"NULL")
    bad(lib.cmve_pairwise_list_ranks(h, P(off), P(sc), P(pos), 4, 6, None), e, b"NULL")
    bad(lib.cmve_pairwise_list_ranks(h, P(off), P(sc), P(pos), -1, 6, P(out)), e, b"bad counts")
    bad(lib.cmve_pairwise_list_ranks(h, P(off), P(sc), P(pos), 4, -6, P(out)), e, b"bad counts")
    torch.cuda.synchronize()
    # and the bindings
    with pytest.raises(ValueError, match="do not match"):
        engine.pairwise_item_scores(a, b[:, :5], L1, 1.0, 0.0, torch.float64, off, idx, 4)
    with pytest.raises(ValueError, match="lists for"):
        engine.pairwise_count(a, b, L1, 1.0, 0.0, torch.float64, row=(coff, sc, 6))
    with pytest.raises(ValueError, match="unknown measure"):
        from cmve.dist import ShardedGallery
        ShardedGallery(b, offset=0, n_global=6, measure="chebyshev")


def test_gt_id_outside_the_gallery_raises(fx):
    import torch
    from cmve.dist import ShardedGallery
    sh = ShardedGallery(fx["vid"], offset=0, n_global=141, measure="l2")
    q = torch.from_numpy(fx["cap"][:4].copy()).cuda()
    with pytest.raises(ValueError, match="outside"):
        sh.evaluate(q, [[0], [141], [2], [3]], None)
    with pytest.raises(ValueError, match="outside"):
        sh.evaluate(q, None, [[4]] + [[]] * 140)
    # the device route: n_q is known only there, so that is where the caption ids are checked
    col = sh.local_v2t_csr([[4]] + [[]] * 140)
    with pytest.raises(ValueError, match=r"caption id outside \[0, 4\)"):
        sh.evaluate_device(q, None, col, 4)
    with pytest.raises(ValueError, match="outside"):
        sh.local_v2t_csr([[-1]] + [[]] * 140)
    assert sh.evaluate_device(q, None, sh.local_v2t_csr([[3]] + [[]] * 140), 4)[1].shape == (141,)
