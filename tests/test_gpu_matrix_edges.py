"""Edge shapes, ties and non-finite values of the matrix, list and merge kernels, through the C ABI.

rank.hip (rank_rows / rank_cols / gtpos_rows / gtpos_cols / gt_ranks), pairwise_rank.hip's list ranks,
merge.hip (the k-way merge) and topk.hip's K12f are the ground the matrix-free and filtered routes are
compared with; here they are compared with the definitions of include/cmve.h restated in numpy.  Matrix
values come from a small integer grid, so ties are everywhere and the strict `<` decides, with +-inf,
-0.0 next to +0.0 and NaN planted at GT and non-GT entries.  Every matrix has ld = n_cols + 3 and its
padding columns hold a value that WOULD count (-1e300 / -3e38; +1e300 where the largest wins): a read
past n_cols changes a count, which NaN padding never would.  Every output is a window of a canary
buffer, checked after each call; a refused call must leave its outputs as they were.
"""
import ctypes

import numpy as np
import pytest
import torch

from _windows import Pad

pytestmark = pytest.mark.gpu

F32, F64, BF16 = 0, 1, 2  # CMVE_F32 / CMVE_F64 / CMVE_BF16 (the last: a dtype the matrix entries refuse)
NP = {F32: np.float32, F64: np.float64}
TORCH = {F32: torch.float32, F64: torch.float64}
LOW = {F32: -3e38, F64: -1e300}  # the read canary of a counting kernel: below every entry, so it would count
INF, NAN = np.inf, np.nan


def _api():
    from cmve import engine
    from cmve._lib import lib
    return engine.handle(), lib


def _ok(status, what):
    from cmve._lib import check
    check(status, what)


def _dev(a, dtype):
    """A device copy of a host index array, one spare element long (an empty array still has an address)."""
    a = np.concatenate([np.asarray(a, dtype).ravel(), np.zeros(1, dtype)])
    return torch.from_numpy(a).cuda()


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _csr(lists):
    off = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int64)
    idx = np.array([k for l in lists for k in l], np.int32)
    return off, idx


def _matrix(e, dt, fill=None, extra=3):
    """e on the device with ld = n_cols + extra, the padding columns holding the read canary."""
    rows, cols = e.shape
    full = np.full((rows, cols + extra), LOW[dt] if fill is None else fill, NP[dt])
    full[:, :cols] = e
    return Pad(rows, cols + extra, dtype=TORCH[dt], data=full)


def _grid(rng, rows, cols, dt):
    """Integers in [-3, 3] with +-inf, -0.0 and NaN planted: about a seventh of the entries each way tie."""
    e = rng.integers(-3, 4, (rows, cols)).astype(NP[dt])
    u = rng.random((rows, cols))
    e[u < 0.04] = INF
    e[(u >= 0.04) & (u < 0.08)] = -INF
    e[(u >= 0.08) & (u < 0.14)] = -0.0
    e[(u >= 0.14) & (u < 0.20)] = NAN
    return e


# ---- the definitions of include/cmve.h, one list at a time (v: the list's row or column, fp64) ----
def _cnt_ref(v, items):
    if len(items) == 0:
        return 0
    g = v[np.asarray(items)]
    if np.isnan(g).all():
        return v.size - 1
    return int(np.sum(v < np.nanmin(g)))  # NaN < x is False: a NaN entry never counts


def _pos_ref(v, items):
    g = v[np.asarray(items, np.int64)] if len(items) else np.zeros(0)
    n_nan, seen, out = int(np.isnan(g).sum()), 0, []
    for t in g:
        if np.isnan(t):
            out.append(v.size - n_nan + seen)
            seen += 1
        else:
            out.append(int(np.sum(v < t)))
    return out


KINDS = ("empty", "one", "three", "all_nan", "mixed", "neg_inf", "pos_inf")


def _plant_list(rng, v, kind):
    """A GT list of the given kind for the vector v (a view: the planted values land in the matrix)."""
    n = v.size
    a = rng.integers(0, n, 2)
    three = [int(a[0]), int(a[1]), int(a[0])]  # a repeat
    if kind == "empty":
        return []
    if kind == "one":
        return [int(a[0])]
    if kind == "three":
        v[a[0]], v[a[1]] = 1, 1  # equal GT values
        return three
    if kind == "all_nan":
        v[a] = NAN
        return three
    if kind == "mixed":
        v[a[1]] = 2
        v[a[0]] = NAN  # (n = 1: the one entry is NaN, an all-NaN list)
        return three
    if kind == "neg_inf":
        v[a[1]] = -INF  # nothing is below it: count 0
        return three
    v[a[0]] = INF  # pos_inf: every non-NaN entry below +inf counts
    return [int(a[0])]


def _call_matrix(fn, E, dt, n_rows, n_cols, transposed, lists, n_out):
    h, lib = _api()
    off, idx = _csr(lists)
    off_d, idx_d = _dev(off, np.int64), _dev(idx, np.int32)
    out = Pad(1, n_out, dtype=torch.int32)  # starts as -77: garbage the entry must not rely on
    st = getattr(lib, fn)(h, E.ptr, dt, n_rows, n_cols, n_cols + 3, transposed, _p(off_d), _p(idx_d), out.ptr)
    _ok(st, fn)
    got = out.numpy()[0]
    out.assert_canary(fn)
    return got


# ------------------------------------------------------------------ 1. cmve_rank_from_matrix
@pytest.mark.parametrize("dt", [F32, F64])
@pytest.mark.parametrize("n_rows", [1, 5])
@pytest.mark.parametrize("n_cols", [1, 255, 256, 257, 600])
def test_rank_rows_ties_nonfinite_and_lists(n_cols, n_rows, dt):
    """rank_rows_kernel: one block of 256 threads per row, so 255 / 256 / 257 / 600 columns are under one
    stride, exactly one, one element over, and two strides and a part.  Every kind of list (empty, one item,
    three with a repeat and equal values, all NaN, NaN and a number, a -inf GT, a +inf GT) meets every shape."""
    rng = np.random.default_rng(1000 * n_cols + 10 * n_rows + dt)
    for start in range(0, len(KINDS), n_rows):
        e = _grid(rng, n_rows, n_cols, dt)
        kinds = [KINDS[(start + r) % len(KINDS)] for r in range(n_rows)]
        lists = [_plant_list(rng, e[r], kinds[r]) for r in range(n_rows)]
        got = _call_matrix("cmve_rank_from_matrix", _matrix(e, dt), dt, n_rows, n_cols, 0, lists, n_rows)
        want = [_cnt_ref(e[r].astype(np.float64), lists[r]) for r in range(n_rows)]
        assert got.tolist() == want, f"kinds {kinds}"
        for r, kind in enumerate(kinds):
            if kind == "neg_inf":
                assert got[r] == 0
            if kind == "pos_inf":
                assert got[r] == int(np.sum(e[r] < INF))


RANK_COLS = [(r, c, dt) for r in (1, 3, 255, 256, 257, 513) for c in (1, 255, 257) for dt in (F32, F64)] \
    + [(16385, 65, F32)]


@pytest.mark.parametrize("n_rows,n_cols,dt", RANK_COLS)
def test_rank_cols_splits_and_all_nan_once(n_rows, n_cols, dt):
    """rank_cols_kernel: a thread per column (255 / 257: under and over one block), the rows split over
    blockIdx.y in ceil(n_rows / 256) parts, 64 at the most: 1 part up to 256 rows, 2 at 257, 3 at 513, and at
    16385 rows 64 parts of 257 rows, the first size at which a part is longer than 256.  cnt starts as
    garbage (the entry zeroes it); a column whose list is all NaN gets n_rows - 1 from split 0 alone."""
    rng = np.random.default_rng(100000 * dt + 300 * n_rows + n_cols)
    splits = min(64, -(-n_rows // 256))
    assert (n_rows > 256) == (splits > 1) and (-(-n_rows // splits) > 256) == (n_rows == 16385)
    for shift in range(len(KINDS) if n_cols == 1 else 1):
        e = _grid(rng, n_rows, n_cols, dt)
        kinds = [KINDS[(c + shift) % len(KINDS)] for c in range(n_cols)]
        lists = [_plant_list(rng, e[:, c], kinds[c]) for c in range(n_cols)]
        got = _call_matrix("cmve_rank_from_matrix", _matrix(e, dt), dt, n_rows, n_cols, 1, lists, n_cols)
        e64 = e.astype(np.float64)
        want = [_cnt_ref(e64[:, c], lists[c]) for c in range(n_cols)]
        assert got.tolist() == want
        for c, kind in enumerate(kinds):
            if kind == "all_nan" or (kind == "mixed" and n_rows == 1):
                assert got[c] == n_rows - 1, f"column {c}: n_rows - 1 added {got[c] / max(n_rows - 1, 1)} times"


# ------------------------------------------------------------------ 2. cmve_gt_positions_from_matrix
GTPOS_LENS = (0, 1, 63, 64, 65, 128, 130)


@pytest.mark.parametrize("dt", [F32, F64])
@pytest.mark.parametrize("n_cols", [1, 255, 257, 700])
def test_gtpos_rows_chunks_and_nan_run(n_cols, dt):
    """gtpos_rows_kernel sorts a list in chunks of MAXG = 64 items: lists of 0, 1, 63, 64, 65, 128 and 130
    items (one per row, with repeats, and equal values from the grid) are under, at and over one and two
    chunks.  NaN items sit at places 3, 60, 66 and 129 of a list: on both sides of the chunk boundary, so the
    NaN positions n - n_nan + (place among the NaN items) must keep running from chunk to chunk."""
    rng = np.random.default_rng(77 * n_cols + dt)
    e = _grid(rng, len(GTPOS_LENS), n_cols, dt)
    lists = []
    for r, m in enumerate(GTPOS_LENS):
        l = rng.integers(0, n_cols, m).tolist()
        for place in (3, 60, 66, 129):
            if place < m:
                e[r, l[place]] = NAN
        lists.append(l)
    got = _call_matrix("cmve_gt_positions_from_matrix", _matrix(e, dt), dt, len(GTPOS_LENS), n_cols, 0, lists,
                       sum(GTPOS_LENS))
    e64 = e.astype(np.float64)
    want = [p for r, l in enumerate(lists) for p in _pos_ref(e64[r], l)]
    assert got.tolist() == want
    if n_cols > 1:  # the case is what it says: NaN items in both chunks of the longest list
        nan_at = np.flatnonzero(np.isnan(e64[-1, lists[-1]]))
        assert (nan_at < 64).any() and (nan_at >= 128).any()


@pytest.mark.parametrize("dt", [F32, F64])
@pytest.mark.parametrize("n_rows", [1, 2, 3, 4, 5, 257])
@pytest.mark.parametrize("n_cols", [1, 63, 64, 65, 130])
def test_gtpos_cols_slices_and_ragged_lists(n_cols, n_rows, dt):
    """gtpos_cols_kernel: a block per 64 columns (63 / 64 / 65 / 130: the last block partly or wholly out of
    range), four row slices [n_rows s / 4, n_rows (s + 1) / 4) per block, partly empty under 4 rows.  The
    lists of one block are ragged (0, 1, 7 and n_rows + 3 items, the last with repeats by necessity), so the
    block-uniform trip count outruns most columns; NaN items take the last positions in list order."""
    rng = np.random.default_rng(9000 * dt + 100 * n_rows + n_cols)
    e = _grid(rng, n_rows, n_cols, dt)
    lens = (0, 1, 7, n_rows + 3)
    lists = []
    for c in range(n_cols):
        l = rng.integers(0, n_rows, lens[(c + n_rows) % 4]).tolist()
        if len(l) > 1 and c % 3 == 0:
            e[l[0], c] = NAN
            e[l[-1], c] = NAN
        lists.append(l)
    got = _call_matrix("cmve_gt_positions_from_matrix", _matrix(e, dt), dt, n_rows, n_cols, 1, lists,
                       sum(map(len, lists)))
    e64 = e.astype(np.float64)
    want = [p for c, l in enumerate(lists) for p in _pos_ref(e64[:, c], l)]
    assert got.tolist() == want


@pytest.mark.parametrize("fn", ["cmve_rank_from_matrix", "cmve_gt_positions_from_matrix"])
def test_matrix_entries_refuse_and_leave_outputs(fn):
    """A NULL argument, ld < n_cols and a dtype outside F32 / F64 are refused, both orientations, and the
    output is not written; an empty matrix is CMVE_OK and writes nothing either."""
    h, lib = _api()
    E = _matrix(np.zeros((4, 6)), F64)
    off_d, idx_d = _dev([0, 1, 2, 3, 4, 4, 4, 4], np.int64), _dev([0, 1, 2, 3], np.int32)
    out = Pad(1, 8, dtype=torch.int32)
    good = dict(e=E.ptr, dt=F64, r=4, c=6, ld=9, off=_p(off_d), idx=_p(idx_d), out=out.ptr)
    bad = [dict(e=None), dict(off=None), dict(idx=None), dict(out=None), dict(ld=5), dict(dt=BF16), dict(dt=-1),
           dict(r=-1), dict(c=-1)]
    for tr in (0, 1):
        for change in bad:
            a = {**good, **change}
            st = getattr(lib, fn)(h, a["e"], a["dt"], a["r"], a["c"], a["ld"], tr, a["off"], a["idx"], a["out"])
            assert st != 0, f"{fn} accepted {change}"
            out.assert_untouched(f"the output of a refused {fn} {change}")
        for r, c in ((0, 6), (4, 0)):
            assert getattr(lib, fn)(h, E.ptr, F64, r, c, 9, tr, _p(off_d), _p(idx_d), out.ptr) == 0
            out.assert_untouched(f"the output of an empty {fn}")
    assert getattr(lib, fn)(None, E.ptr, F64, 4, 6, 9, 0, _p(off_d), _p(idx_d), out.ptr) != 0


# ------------------------------------------------------------------ 3. cmve_gt_ranks
@pytest.mark.parametrize("outs", ["ranks+recall", "ranks", "recall"])
@pytest.mark.parametrize("n", [0, 1, 1023, 1025, 5000])
def test_gt_ranks_rules_and_recall_sums(n, outs):
    """gt_ranks_kernel: with recall one block of 1024 threads strides over the rows (1023 / 1025 / 5000: under
    one stride, one over, five strides with a part), without it ceil(n / 1024) blocks.  sgt NaN -> n_m + 1,
    +inf -> n_m, else cnt + 1, whatever cnt holds; the four recall words are numpy's sums; n = 0 zeroes
    recall and leaves ranks alone."""
    h, lib = _api()
    n_m = 1000
    rng = np.random.default_rng(n)
    cnt = rng.integers(0, 14, n).astype(np.int32)  # ranks on both sides of 1, 5 and 10
    sgt = rng.standard_normal(n)
    u = rng.random(n)
    sgt[u < 0.15] = NAN
    sgt[(u >= 0.15) & (u < 0.3)] = INF
    sgt[(u >= 0.3) & (u < 0.4)] = -INF  # a number like any other: cnt + 1
    cnt[u < 0.3] = 3  # would be rank 4 if the count were used
    cnt_d, sgt_d = _dev(cnt, np.int32), _dev(sgt, np.float64)
    ranks = Pad(1, n, dtype=torch.int64) if "ranks" in outs else None
    recall = Pad(1, 4, dtype=torch.int64) if "recall" in outs else None
    st = lib.cmve_gt_ranks(h, _p(cnt_d), _p(sgt_d), n, n_m, ranks.ptr if ranks else None,
                           recall.ptr if recall else None)
    _ok(st, "cmve_gt_ranks")
    want = np.where(np.isnan(sgt), n_m + 1, np.where(sgt == INF, n_m, cnt.astype(np.int64) + 1))
    if ranks:
        assert np.array_equal(ranks.numpy()[0], want)
        ranks.assert_canary("ranks")
    if recall:
        assert recall.numpy()[0].tolist() == [int((want <= 1).sum()), int((want <= 5).sum()),
                                              int((want <= 10).sum()), int(want.sum())]
        recall.assert_canary("recall")


def test_gt_ranks_refusals():
    h, lib = _api()
    cnt_d, sgt_d = _dev(np.zeros(8), np.int32), _dev(np.zeros(8), np.float64)
    ranks, recall = Pad(1, 8, dtype=torch.int64), Pad(1, 4, dtype=torch.int64)
    for args in ((None, _p(sgt_d), 8, 10, ranks.ptr, recall.ptr), (_p(cnt_d), None, 8, 10, ranks.ptr, recall.ptr),
                 (_p(cnt_d), _p(sgt_d), -1, 10, ranks.ptr, recall.ptr),
                 (_p(cnt_d), _p(sgt_d), 8, -1, ranks.ptr, recall.ptr)):
        assert lib.cmve_gt_ranks(h, *args) != 0
        ranks.assert_untouched("ranks of a refused cmve_gt_ranks")
        recall.assert_untouched("recall of a refused cmve_gt_ranks")
    assert lib.cmve_gt_ranks(h, _p(cnt_d), _p(sgt_d), 8, 10, None, None) != 0  # no output
    assert lib.cmve_gt_ranks(None, _p(cnt_d), _p(sgt_d), 8, 10, ranks.ptr, recall.ptr) != 0


# ------------------------------------------------------------------ 4. cmve_pairwise_list_ranks
@pytest.mark.parametrize("n_lists", [1, 255, 257])
def test_pairwise_list_ranks_nan_items_ignored(n_lists):
    """A thread per list (255 / 257: under and over one block).  ranks = 1 + the least position over the
    non-NaN items; an empty list n_m + 1; an all-NaN list n_m; a NaN item that holds the smallest position
    of its list (position 0) is ignored."""
    h, lib = _api()
    n_m = 1000
    rng = np.random.default_rng(n_lists)
    for first in range(4 if n_lists == 1 else 1):
        lists_sc, lists_pos, want = [], [], []
        for l in range(n_lists):
            kind = (l + first) % 4
            m = (0, 3, 4, 1 + l % 5)[kind]
            sc, pos = rng.standard_normal(m), rng.integers(1, n_m, m)
            if kind == 1:
                sc[:] = NAN
            if kind == 2:
                sc[1], pos[1] = NAN, 0  # the smallest position of the list, on a NaN item
            ok = ~np.isnan(sc)
            want.append(n_m + 1 if m == 0 else (n_m if not ok.any() else 1 + int(pos[ok].min())))
            lists_sc.append(sc)
            lists_pos.append(pos)
        off_d = _dev(np.concatenate([[0], np.cumsum([len(s) for s in lists_sc])]), np.int64)
        sc_d = _dev(np.concatenate(lists_sc), np.float64)
        pos_d = _dev(np.concatenate(lists_pos), np.int32)
        ranks = Pad(1, n_lists, dtype=torch.int64)
        st = lib.cmve_pairwise_list_ranks(h, _p(off_d), _p(sc_d), _p(pos_d), n_lists, n_m, ranks.ptr)
        _ok(st, "cmve_pairwise_list_ranks")
        assert ranks.numpy()[0].tolist() == want
        ranks.assert_canary("list ranks")


def test_pairwise_list_ranks_refusals():
    h, lib = _api()
    off_d, sc_d, pos_d = _dev([0, 1, 2], np.int64), _dev([0.5, 0.25], np.float64), _dev([3, 4], np.int32)
    ranks = Pad(1, 2, dtype=torch.int64)
    o, s, p = _p(off_d), _p(sc_d), _p(pos_d)
    for args in ((None, s, p, 2, 10, ranks.ptr), (o, None, p, 2, 10, ranks.ptr), (o, s, None, 2, 10, ranks.ptr),
                 (o, s, p, 2, 10, None), (o, s, p, -1, 10, ranks.ptr), (o, s, p, 2, -1, ranks.ptr)):
        assert lib.cmve_pairwise_list_ranks(h, *args) != 0
        ranks.assert_untouched("ranks of a refused cmve_pairwise_list_ranks")
    assert lib.cmve_pairwise_list_ranks(None, o, s, p, 2, 10, ranks.ptr) != 0
    assert lib.cmve_pairwise_list_ranks(h, o, s, p, 0, 10, ranks.ptr) == 0  # no lists: nothing written
    ranks.assert_untouched("ranks of an empty cmve_pairwise_list_ranks")


# ------------------------------------------------------------------ 5. cmve_merge_topk
MERGE_GRID = np.array([-INF, -1.0, -0.0, 0.0, 1.0, 2.0, INF, NAN])


def _order(scores, ids):
    """(numbers before NaN, score desc, id asc); -0.0 and +0.0 compare equal, so the id decides between them."""
    nan = np.isnan(scores)
    return np.lexsort((ids, np.where(nan, 0.0, -scores), nan))


def _merge_inputs(rng, n_q, lists, k_in):
    """Sorted runs [n_q, lists, k_in] with empty slots (id -1, a garbage score) at their tails, whole empty
    runs, and -- from three queries on -- a last query whose every run is empty."""
    ids = np.full((n_q, lists, k_in), -1, np.int64)
    sc = np.full((n_q, lists, k_in), 7e77)  # garbage that would win if an empty slot were read as an entry
    for q in range(n_q):
        pool = rng.permutation(4 * lists * k_in)  # distinct ids over the query, in no order across runs
        for l in range(lists):
            v = int(rng.choice([0, k_in, rng.integers(0, k_in + 1)]))
            if n_q >= 3 and q == n_q - 1:
                v = 0
            s, i = rng.choice(MERGE_GRID, v), pool[l * k_in:l * k_in + v].astype(np.int64)
            o = _order(s, i)
            sc[q, l, :v], ids[q, l, :v] = s[o], i[o]
    return ids, sc


@pytest.mark.parametrize("k_in", [1, 5, 7])
@pytest.mark.parametrize("lists", [1, 2, 3, 63, 64])
def test_merge_topk_ties_nan_and_empty_runs(lists, k_in):
    """merge_topk_kernel: lane l holds run l (63 / 64: one lane idle, none), four queries per block (n_q = 1,
    3, 4, 5, 9: part of a block, a whole one, one over, two and a part).  k_out = 1, k_in, lists k_in and
    lists k_in + 3 (more than there is: the tail is id -1, score NaN).  Scores come from eight grid values, so
    equal scores meet across runs and the lower id must win; NaN ranks after -inf; -0.0 ties +0.0."""
    h, lib = _api()
    rng = np.random.default_rng(100 * lists + k_in)
    for n_q in (1, 3, 4, 5, 9):
        ids, sc = _merge_inputs(rng, n_q, lists, k_in)
        ids_d, sc_d = _dev(ids, np.int64), _dev(sc, np.float64)
        for k_out in sorted({1, k_in, lists * k_in, lists * k_in + 3}):
            out_i, out_s = Pad(n_q, k_out, dtype=torch.int64), Pad(n_q, k_out, dtype=torch.float64)
            st = lib.cmve_merge_topk(h, _p(ids_d), _p(sc_d), n_q, lists, k_in, k_out, out_i.ptr, out_s.ptr)
            _ok(st, "cmve_merge_topk")
            gi, gs = out_i.numpy(), out_s.numpy()
            out_i.assert_canary("merged ids")
            out_s.assert_canary("merged scores")
            for q in range(n_q):
                valid = ids[q].ravel() >= 0
                vi, vs = ids[q].ravel()[valid], sc[q].ravel()[valid]
                o = _order(vs, vi)[:k_out]
                wi = np.concatenate([vi[o], np.full(k_out - o.size, -1, np.int64)])
                ws = np.concatenate([vs[o], np.full(k_out - o.size, NAN)])
                what = f"n_q {n_q} k_out {k_out} query {q}"
                assert gi[q].tolist() == wi.tolist(), what
                assert np.array_equal(gs[q], ws, equal_nan=True), what
                assert np.array_equal(np.signbit(gs[q])[~np.isnan(ws)], np.signbit(ws)[~np.isnan(ws)]), what
            if n_q >= 3:  # every run empty
                assert (gi[-1] == -1).all() and np.isnan(gs[-1]).all()


def test_merge_topk_refusals():
    """NULL arguments, lists of 0 and 65, k_in or k_out of 0: refused, outputs not written; no queries: CMVE_OK,
    nothing written."""
    h, lib = _api()
    ids_d, sc_d = _dev(np.arange(12), np.int64), _dev(np.zeros(12), np.float64)
    out_i, out_s = Pad(2, 4, dtype=torch.int64), Pad(2, 4, dtype=torch.float64)
    i, s = _p(ids_d), _p(sc_d)
    for args in ((None, s, 2, 2, 3, 4, out_i.ptr, out_s.ptr), (i, None, 2, 2, 3, 4, out_i.ptr, out_s.ptr),
                 (i, s, 2, 2, 3, 4, None, out_s.ptr), (i, s, 2, 2, 3, 4, out_i.ptr, None),
                 (i, s, 2, 0, 3, 4, out_i.ptr, out_s.ptr), (i, s, 2, 65, 3, 4, out_i.ptr, out_s.ptr),
                 (i, s, 2, 2, 0, 4, out_i.ptr, out_s.ptr), (i, s, 2, 2, 3, 0, out_i.ptr, out_s.ptr),
                 (i, s, -1, 2, 3, 4, out_i.ptr, out_s.ptr)):
        assert lib.cmve_merge_topk(h, *args) != 0, args[2:6]
        out_i.assert_untouched("ids of a refused cmve_merge_topk")
        out_s.assert_untouched("scores of a refused cmve_merge_topk")
    assert lib.cmve_merge_topk(None, i, s, 2, 2, 3, 4, out_i.ptr, out_s.ptr) != 0
    assert lib.cmve_merge_topk(h, i, s, 0, 2, 3, 4, out_i.ptr, out_s.ptr) == 0
    out_i.assert_untouched("ids of a cmve_merge_topk without queries")


# ------------------------------------------------------------------ 6. cmve_topk_dense_merge (K12f)
def _dense_ref(best_s, best_i, chunk, j0, k):
    """Per row the k best of [running best | chunk (ids j0 + c)] by (score desc, id asc), NaN as -inf and -0.0
    as +0.0; short rows end in id -1, score -inf."""
    n_rows = chunk.shape[0]
    wi, ws = np.full((n_rows, k), -1, np.int64), np.full((n_rows, k), -INF)
    for r in range(n_rows):
        s = np.concatenate([best_s[r], chunk[r]])
        i = np.concatenate([best_i[r], j0 + np.arange(chunk.shape[1], dtype=np.int64)])
        s = np.where(np.isnan(s), -INF, s)
        o = np.lexsort((i, -s))[:k]
        wi[r, :o.size], ws[r, :o.size] = i[o], s[o]
    return wi, ws


def _dense_call(best_s, best_i, chunk, j0, k):
    """The rows of the chunk are lds = nc + 5 apart, the padding at +1e300: read, it would win."""
    h, lib = _api()
    n_rows, kb, nc = chunk.shape[0], best_s.shape[1], chunk.shape[1]
    bs = Pad(n_rows, kb, dtype=torch.float64, data=best_s) if kb else None
    bi = Pad(n_rows, kb, dtype=torch.int64, data=best_i) if kb else None
    S = _matrix(chunk, F64, fill=1e300, extra=5) if nc else None
    out_s, out_i = Pad(n_rows, k, dtype=torch.float64), Pad(n_rows, k, dtype=torch.int64)
    st = lib.cmve_topk_dense_merge(h, bs.ptr if kb else None, bi.ptr if kb else None, kb, S.ptr if nc else None,
                                   nc + 5 if nc else 0, n_rows, nc, j0, k, out_s.ptr, out_i.ptr)
    _ok(st, "cmve_topk_dense_merge")
    out_s.assert_canary("K12f scores")
    out_i.assert_canary("K12f ids")
    return out_i, out_s


DENSE_GRID = np.array([-INF, -1.0, -0.0, 0.0, 1.0, INF])


@pytest.mark.parametrize("k", [64, 170])
@pytest.mark.parametrize("j0", [0, 2 ** 40 + 3])
def test_topk_dense_merge_ties_wide_ids_and_padded_rows(j0, k):
    """Six score values over 300 columns and a running best of 4 (kb < k) whose ids are unordered, below and
    above the chunk's and up to 2^41: the k-th score is tied some fifty ways (k = 64: among the 1.0; k = 170:
    among the zeros, where -0.0 ties +0.0 and the id decides) and the id radix picks, at j0 = 2^40 + 3 in its
    upper bytes.  +-inf are scores like any other.  The padding of the rows would win if it were read."""
    rng = np.random.default_rng(j0 % 1000 + k)
    n_rows, nc = 3, 300
    chunk = rng.choice(DENSE_GRID, (n_rows, nc))
    best_s = rng.choice(DENSE_GRID[2:5], (n_rows, 4))
    if j0 == 0:
        best_i = np.array([[900, 2005, 2 ** 41, 800], [2 ** 33 + 1, 2007, 1000, 2006], [301, 300, 3001, 3000]], np.int64)
    else:
        best_i = np.array([[j0 + 900, 5, 2 ** 41, j0 + 800], [2 ** 33 + 1, 7, j0 + 1000, 6],
                           [j0 + 301, j0 + 300, 1, 0]], np.int64)
    out_i, out_s = _dense_call(best_s, best_i, chunk, j0, k)
    wi, ws = _dense_ref(best_s, best_i, chunk, j0, k)
    assert np.array_equal(out_i.numpy(), wi)
    assert np.array_equal(out_s.numpy(), ws)
    tied = [(np.concatenate([best_s[r], chunk[r]]) == ws[r, -1]).sum() for r in range(n_rows)]
    assert min(tied) > 20, "the k-th score is to be heavily tied"
    if k == 170:
        assert (ws[:, -1] == 0).all(), "the k-th score is to be a zero"


@pytest.mark.parametrize("k", [1, 2047, 2048])
def test_topk_dense_merge_all_equal(k):
    """Every score equal over nc = 5000 > TD_KMAX columns: the whole selection is the id radix's, ids j0 .. j0
    + k - 1 in order, at k = 1, TD_KMAX - 1 and TD_KMAX."""
    chunk = np.full((2, 5000), 0.25)
    out_i, out_s = _dense_call(np.zeros((2, 0)), np.zeros((2, 0), np.int64), chunk, 11, k)
    assert np.array_equal(out_i.numpy(), np.tile(11 + np.arange(k), (2, 1)))
    assert (out_s.numpy() == 0.25).all()


def test_topk_dense_merge_empty_sides():
    """nc = 0 with kb > 0: the running best in order, the rest id -1 / -inf.  kb = nc = 0: all -1 / -inf.
    n_rows = 0: CMVE_OK, nothing written."""
    best_s = np.array([[0.5, 2.0, 0.5], [-INF, INF, 0.0]])
    best_i = np.array([[9, 4, 3], [2, 8, 2 ** 35]], np.int64)
    none_s, none_i = np.zeros((2, 0)), np.zeros((2, 0), np.int64)
    out_i, out_s = _dense_call(best_s, best_i, none_s, 0, 5)
    wi, ws = _dense_ref(best_s, best_i, none_s, 0, 5)
    assert wi.tolist() == [[4, 3, 9, -1, -1], [8, 2 ** 35, 2, -1, -1]]
    assert np.array_equal(out_i.numpy(), wi) and np.array_equal(out_s.numpy(), ws)
    out_i, out_s = _dense_call(none_s, none_i, none_s, 0, 5)
    assert (out_i.numpy() == -1).all() and (out_s.numpy() == -INF).all()
    h, lib = _api()
    bs, bi = Pad(2, 3, dtype=torch.float64, data=best_s), Pad(2, 3, dtype=torch.int64, data=best_i)
    out_s, out_i = Pad(2, 5, dtype=torch.float64), Pad(2, 5, dtype=torch.int64)
    assert lib.cmve_topk_dense_merge(h, bs.ptr, bi.ptr, 3, bs.ptr, 3, 0, 3, 0, 5, out_s.ptr, out_i.ptr) == 0
    out_s.assert_untouched("K12f scores with no rows")
    out_i.assert_untouched("K12f ids with no rows")


def test_topk_dense_merge_refusals():
    """k = 2049, kb > k, lds < nc, NULL arguments and out aliasing the running best: refused, nothing written."""
    h, lib = _api()
    bs, bi = Pad(2, 3, dtype=torch.float64, data=np.zeros((2, 3))), Pad(2, 3, dtype=torch.int64, data=np.zeros((2, 3)))
    S = Pad(2, 8, dtype=torch.float64, data=np.zeros((2, 8)))
    out_s, out_i = Pad(2, 2049, dtype=torch.float64), Pad(2, 2049, dtype=torch.int64)
    good = dict(bs=bs.ptr, bi=bi.ptr, kb=3, s=S.ptr, lds=8, n=2, nc=8, j0=0, k=5, os=out_s.ptr, oi=out_i.ptr)
    bad = [dict(k=2049), dict(k=0), dict(kb=6), dict(lds=7), dict(j0=-1), dict(bs=None), dict(bi=None), dict(s=None),
           dict(os=None), dict(oi=None)]
    for change in bad:
        a = {**good, **change}
        st = lib.cmve_topk_dense_merge(h, a["bs"], a["bi"], a["kb"], a["s"], a["lds"], a["n"], a["nc"], a["j0"],
                                       a["k"], a["os"], a["oi"])
        assert st != 0, f"accepted {change}"
        out_s.assert_untouched(f"K12f scores after a refused {change}")
        out_i.assert_untouched(f"K12f ids after a refused {change}")
    assert lib.cmve_topk_dense_merge(None, bs.ptr, bi.ptr, 3, S.ptr, 8, 2, 8, 0, 5, out_s.ptr, out_i.ptr) != 0
    before_s, before_i = bs.flat.clone(), bi.flat.clone()
    assert lib.cmve_topk_dense_merge(h, bs.ptr, bi.ptr, 3, S.ptr, 8, 2, 8, 0, 3, bs.ptr, out_i.ptr) != 0
    assert lib.cmve_topk_dense_merge(h, bs.ptr, bi.ptr, 3, S.ptr, 8, 2, 8, 0, 3, out_s.ptr, bi.ptr) != 0
    assert torch.equal(before_s.view(torch.int64), bs.flat.view(torch.int64)) and torch.equal(before_i, bi.flat)
    out_s.assert_untouched("K12f scores after an aliased call")
    out_i.assert_untouched("K12f ids after an aliased call")
