"""K26's host-only surface: the declarations of the three new entries, the workspace arithmetic of
cmve_cos_count_workspace and its refusals, and the ``filter="cosine"`` refusals that need no device.  No kernel is
launched, no GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cmve_cos_item_scores", "cmve_cos_count_workspace", "cmve_cos_count")


def _src():
    return open(os.path.join(ROOT, "include", "cmve.h")).read()


def _params(src, name):
    m = re.search(r"^int\s+%s\s*\(([^;]*)\);" % name, src, re.M | re.S)
    return re.sub(r"\s+", " ", m.group(1)).strip()


def test_header_declares_and_library_exports_the_entries():
    from cmve import _lib
    src = _src()
    for name in NAMES:
        assert re.search(r"^int\s+%s\s*\(" % name, src, re.M), f"{name} is not declared in cmve.h"
        assert hasattr(_lib.lib, name) and name in _lib.exported_symbols()
    # every entry cites what it replaces
    doc = src[src.index("/* K26:"):src.index("int cmve_cos_item_scores")]
    for cite in ("evaluation.py:17-21", "metrics.py:61-102,124-157", "validate.py:15-54"):
        assert doc.count(cite) >= len(NAMES), cite
    # additive: the ABI is still 21 and the earlier count entries are still there
    assert "#define CMVE_ABI_VERSION 21" in src and _lib.lib.cmve_abi_version() == 21 == _lib.ABI_VERSION
    for old in ("cmve_l2_count", "cmve_l2_count_resolved", "cmve_l1_count", "cmve_jaccard_count", "cmve_pairwise_count",
                "cmve_pairwise_list_ranks", "cmve_gt_thresholds", "cmve_rank_fixup"):
        assert re.search(r"^int\s+%s\s*\(" % old, src, re.M) and old in _lib.exported_symbols()


def test_the_count_takes_the_l2_entrys_list_arguments():
    src = _src()
    l2 = _params(src, "cmve_l2_count")
    assert _params(src, "cmve_cos_count") == l2.replace("double alpha, double beta, ", "")
    assert _params(src, "cmve_cos_count_workspace") == _params(src, "cmve_l2_count_workspace")
    assert _params(src, "cmve_cos_item_scores") == (
        "cmve_handle_t h, const cmve_rows_t* a, const cmve_rows_t* b, const int64_t* off, const int32_t* idx, "
        "int64_t n_lists, int64_t n_items, int32_t col_dir, double* out")


def _rows(n, d):
    from cmve import _lib
    r = _lib.Rows()
    r.n, r.d, r.n_pad, r.d_pad = n, d, -(-max(n, 1) // 256) * 256, -(-d // 64) * 64
    return r


def test_workspace_arithmetic_and_refusals_without_a_device():
    from cmve import _lib
    a, b = _rows(59800, 1024), _rows(2990, 1024)
    nbytes = C.c_int64(-1)
    for cap in (0, 1, 8, 1 << 20, (1 << 60) - 1):
        assert _lib.lib.cmve_cos_count_workspace(C.byref(a), C.byref(b), cap, C.byref(nbytes)) == 0
        assert nbytes.value == 8 * cap
    for cap in (-1, -(1 << 40), (1 << 63) - 1, (1 << 60) + 1):
        assert _lib.lib.cmve_cos_count_workspace(C.byref(a), C.byref(b), cap, C.byref(nbytes)) < 0
        assert b"cmve_cos_count_workspace" in _lib.lib.cmve_last_error()
    assert _lib.lib.cmve_cos_count_workspace(C.byref(a), C.byref(b), 8, None) < 0
    assert _lib.lib.cmve_cos_count_workspace(None, C.byref(b), 8, C.byref(nbytes)) < 0
    assert _lib.lib.cmve_cos_count_workspace(C.byref(a), C.byref(_rows(2990, 512)), 8, C.byref(nbytes)) < 0
    assert b"cmve_cos_count_workspace" in _lib.lib.cmve_last_error()


def test_dispatch_constant_and_route_rule():
    from cmve import engine
    from cmve.linas import metrics as M
    assert hasattr(engine, "COS_FILTER_MIN_PAIRS")
    assert engine.COS_FILTER_MIN_PAIRS is None or engine.COS_FILTER_MIN_PAIRS > 0
    single, multi = [[0], [1]], [[0, 1], []]
    assert M.cosine_one_pass("cosine", 2, 2, single)
    saved = engine.COS_FILTER_MIN_PAIRS
    try:
        engine.COS_FILTER_MIN_PAIRS = None
        assert not M.cosine_one_pass(None, 1 << 20, 1 << 20, multi)
        engine.COS_FILTER_MIN_PAIRS = 16
        assert M.cosine_one_pass(None, 4, 4, single, multi)
        assert not M.cosine_one_pass(None, 4, 4, single)      # today's route runs one pass: nothing to save
        assert not M.cosine_one_pass(None, 3, 5, multi)       # below the threshold
        assert not M.cosine_one_pass(False, 4, 4, multi)
    finally:
        engine.COS_FILTER_MIN_PAIRS = saved


def test_filter_cosine_with_another_measure_is_a_value_error():
    from cmve.linas import metrics as M, validate as V
    from cmve.linas.evaluation import ErrorMatrix
    plain = np.zeros((2, 3))
    pw = plain.view(ErrorMatrix)
    pw._cmve_pw = (None, None, "l2")
    for errors in (plain, pw):
        with pytest.raises(ValueError, match='filter="cosine"'):
            V.cal_perf(errors, [[0], [1], []], {0: [0], 1: [1]}, filter="cosine")
        with pytest.raises(ValueError, match='filter="cosine"'):
            M.t2v_map(errors, {0: [0], 1: [1]}, filter="cosine")
        with pytest.raises(ValueError, match='filter="cosine"'):
            M.v2t_map(errors, [[0], [1], []], filter="cosine")
    for measure in ("l2", "l1", "jaccard", "euclidean"):
        with pytest.raises(ValueError, match='filter="cosine"'):
            V.cal_perf_embeddings(np.ones((2, 4)), np.ones((2, 4)), ["v0", "v1"], ["v0#0", "v1#0"], measure=measure,
                                  filter="cosine")


def test_vectorised_aps_are_ap_from_positions_bit_for_bit():
    from cmve.linas import metrics as M
    rng = np.random.default_rng(26)
    for lens in (np.full(3000, 20), rng.integers(0, 40, 2000), np.zeros(5, np.int64)):
        offs = np.zeros(lens.size + 1, np.int64)
        np.cumsum(lens, out=offs[1:])
        pos = rng.integers(1, 60000, int(offs[-1])).astype(np.int64)
        lists = [pos[offs[i]:offs[i + 1]] for i in range(lens.size)]
        assert np.array_equal(M.ap_flat(offs, pos), np.array([M.ap_from_positions(p) for p in lists]))
        assert np.array_equal(M.ap_flat(offs, pos, first_only=True),
                              np.array([M.ap_from_positions(p[:1]) for p in lists]))
        assert M.maps_from_flat((offs, pos), (offs, pos)) == M.maps_from_positions(lists, lists)
