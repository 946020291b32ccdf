"""K18's workspace sizing (cmve_pairwise_positions_workspace, cmve_pairwise_topk_workspace): host only -- no
kernel is launched, no GPU needed.

Neither workspace holds anything proportional to the pair count: the positions' is the item scores alone, the
top-k's its best-lists (with few queries also the per-segment lists) plus one chunk of scores."""
import ctypes as C

import pytest

METRICS = ["PW_SQ_L2", "PW_L2", "PW_L1", "PW_ORDER", "PW_JACCARD", "PW_DOT"]
MIB = 1 << 20


def _pos_ws(na, nb, ri, ci, metric):
    from cmve import _lib
    n = C.c_int64(-1)
    return _lib.lib.cmve_pairwise_positions_workspace(na, nb, ri, ci, metric, C.byref(n)), n.value


def _topk_ws(n_q, n_g, k, metric):
    from cmve import _lib
    lo, rec = C.c_int64(-1), C.c_int64(-1)
    return _lib.lib.cmve_pairwise_topk_workspace(n_q, n_g, k, metric, C.byref(lo), C.byref(rec)), lo.value, rec.value


def _err():
    from cmve import _lib
    return _lib.lib.cmve_last_error()


@pytest.mark.parametrize("name", METRICS)
def test_positions_workspace_is_the_item_scores(name):
    from cmve import _lib
    metric = getattr(_lib, name)
    assert _pos_ws(150, 141, 150, 150, metric) == (0, 8 * 300)
    assert _pos_ws(150, 141, 150, 0, metric) == (0, 8 * 150)
    assert _pos_ws(150, 141, 0, 7, metric) == (0, 8 * 7)
    # independent of the pair count
    assert _pos_ws(59800, 2990, 59800, 59800, metric) == (0, 8 * 2 * 59800)
    assert _pos_ws(16384, 1 << 20, 16384, 16384, metric) == (0, 8 * 2 * 16384)
    assert _pos_ws(0, 0, 0, 0, metric) == (0, 0)
    assert _pos_ws(0, 141, 0, 0, metric) == (0, 0)


def test_positions_workspace_refuses_bad_arguments():
    from cmve import _lib
    for args in ((-1, 1, 0, 0), (1, -1, 0, 0), (1, 1, -1, 0), (1, 1, 0, -1)):
        rc, _ = _pos_ws(*args, _lib.PW_L1)
        assert rc < 0 and b"cmve_pairwise_positions_workspace" in _err() and b"bad shape" in _err()
    rc, _ = _pos_ws(1, 1, 1, 1, 17)
    assert rc < 0 and b"cmve_pairwise_positions_workspace" in _err() and b"unknown metric" in _err()
    rc, _ = _pos_ws(1, 1, 1, 1, -1)
    assert rc < 0 and b"unknown metric" in _err()
    assert _lib.lib.cmve_pairwise_positions_workspace(1, 1, 1, 1, _lib.PW_L1, None) < 0
    assert b"cmve_pairwise_positions_workspace" in _err() and b"NULL" in _err()
    rc, _ = _pos_ws(1, 1, 1 << 62, 1 << 62, _lib.PW_L1)
    assert rc < 0 and b"cmve_pairwise_positions_workspace" in _err() and b"overflows" in _err()


@pytest.mark.parametrize("name", METRICS)
def test_topk_workspace_minimum_and_recommended(name):
    from cmve import _lib
    metric = getattr(_lib, name)
    # minimum: the two best-lists (fp64 score + int64 id, double-buffered: 32 bytes per (query, slot)) and one
    # 128-column chunk of fp64 scores
    rc, lo, rec = _topk_ws(300, 1000, 10, metric)
    assert rc == 0 and lo == 300 * 10 * 32 + 300 * 128 * 8
    assert rec == 300 * 10 * 32 + 300 * 1024 * 8        # the whole gallery (rounded up to 128 columns) fits
    rc, lo2, _ = _topk_ws(600, 1000, 10, metric)
    assert rc == 0 and lo2 == 2 * lo                     # linear in n_q
    rc, lo3, _ = _topk_ws(300, 1000, 20, metric)
    assert rc == 0 and lo3 - lo == 300 * 10 * 32         # the best-lists grow with k, the chunk does not
    rc, lo4, _ = _topk_ws(300, 1 << 20, 10, metric)
    assert rc == 0 and lo4 == lo                         # the minimum does not depend on the gallery
    # recommended: at most 256 MiB of scores plus the lists for n_q <= 65,536.  Below 256 queries the lists are
    # the running best, up to 63 per-segment lists and the merge's output: (2 S + 4) * n_q * k * 8 bytes.
    for n_q in (1, 16, 255, 256, 1000, 3000, 65536):
        rc, lo, rec = _topk_ws(n_q, 1 << 20, 10, metric)
        lists = (130 if n_q < 256 else 4) * n_q * 10 * 8
        assert rc == 0 and lo <= rec <= 256 * MIB + lists
        assert (rec - 4 * n_q * 10 * 8) % 8 == 0
    rc, lo, rec = _topk_ws(1, 1 << 20, 10, metric)
    assert rec == 130 * 10 * 8 + 63 * 16768 * 8          # one query: 63 segments of ceil(2^20 / 63) -> 16,768 columns
    rc, lo, rec = _topk_ws(7, 1000, 10, metric)
    assert lo == 7 * 10 * 32 + 7 * 128 * 8 and rec == 20 * 70 * 8 + 7 * 1024 * 8   # 8 segments of 128 columns
    rc, lo, rec = _topk_ws(7, 1000, 1000, metric)
    assert rec == 7 * 1000 * 32 + 7 * 1024 * 8           # a segment holds >= k columns: one segment, the plain lists
    # zero sizes
    assert _topk_ws(0, 1000, 10, metric) == (0, 0, 0)
    rc, lo, rec = _topk_ws(7, 0, 10, metric)
    assert rc == 0 and lo == rec == 7 * 10 * 32 + 7 * 128 * 8
    rc, lo, rec = _topk_ws(300, 0, 10, metric)
    assert rc == 0 and lo == rec == 300 * 10 * 32 + 300 * 128 * 8


def test_topk_workspace_refuses_bad_arguments():
    from cmve import _lib
    for args in ((-1, 10, 1), (10, -1, 1)):
        rc, _, _ = _topk_ws(*args, _lib.PW_L1)
        assert rc < 0 and b"cmve_pairwise_topk_workspace" in _err() and b"bad shape" in _err()
    for k in (0, -3, _lib.TOPK_MAX + 1):
        rc, _, _ = _topk_ws(10, 10, k, _lib.PW_L1)
        assert rc < 0 and b"cmve_pairwise_topk_workspace" in _err() and b"k must be" in _err()
    assert _topk_ws(10, 10, _lib.TOPK_MAX, _lib.PW_L1)[0] == 0
    rc, _, _ = _topk_ws(10, 10, 1, 17)
    assert rc < 0 and b"cmve_pairwise_topk_workspace" in _err() and b"unknown metric" in _err()
    lo = C.c_int64()
    assert _lib.lib.cmve_pairwise_topk_workspace(10, 10, 1, _lib.PW_L1, None, C.byref(lo)) < 0
    assert b"cmve_pairwise_topk_workspace" in _err() and b"NULL" in _err()
    assert _lib.lib.cmve_pairwise_topk_workspace(10, 10, 1, _lib.PW_L1, C.byref(lo), None) < 0
    assert b"NULL" in _err()
    rc, _, _ = _topk_ws(1 << 60, 10, 2048, _lib.PW_L1)
    assert rc < 0 and b"cmve_pairwise_topk_workspace" in _err() and b"overflows" in _err()


def test_engine_wrappers_size_without_a_gpu():
    from cmve import _lib, engine
    assert engine.pairwise_positions_workspace(33, 37, 5, 9, _lib.PW_JACCARD) == 8 * 14
    assert engine.pairwise_topk_workspace(7, 1000, 10, _lib.PW_L1) == _topk_ws(7, 1000, 10, _lib.PW_L1)[1:]
    with pytest.raises(_lib.CmveError, match="cmve_pairwise_topk_workspace"):
        engine.pairwise_topk_workspace(7, 1000, 0, _lib.PW_L1)


def test_measure_table_is_the_single_source():
    """cmve.linas.evaluation keeps ONE measure table for the matrix path and the matrix-free paths."""
    import torch
    from cmve import _lib
    from cmve.linas import evaluation as E
    assert set(E.MEASURES) == {"euclidean", "l2", "l1", "l1_norm", "l2_norm", "jaccard"}
    assert E.measure_spec("l1_norm", 64) == (_lib.PW_L1, -1.0 / 64, -1.0, torch.float64, torch.float64)
    assert E.measure_spec("jaccard", 64) == (_lib.PW_JACCARD, -1.0, 0.0, torch.float32, torch.float32)
    with pytest.raises(ValueError, match="unknown measure"):
        E.measure_spec("order", 64)
