"""K20's host-only surface (cmve_l2_topk_workspace, the declarations, the Python arguments): no kernel is launched,
no GPU needed.

The workspace of cmve_l2_topk is what ONE round of min(1024, round_up128(n_q)) queries needs: per query the sample's
upper key bounds (4 bytes per sample row, rounded up to the 128-row tile), the candidate list (4 bytes per slot), the
threshold (8) and the counter (4)."""
import ctypes as C
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rows(n, d):
    from cmve import _lib
    r = _lib.Rows()
    r.n, r.d = n, d
    r.n_pad, r.d_pad = (n + 255) // 256 * 256, (d + 63) // 64 * 64
    return r


def _ws(q, g, k, cap, sample):
    from cmve import _lib
    n = C.c_int64(-1)
    return _lib.lib.cmve_l2_topk_workspace(C.byref(q), C.byref(g), k, cap, sample, C.byref(n)), n.value


def _err():
    from cmve import _lib
    return _lib.lib.cmve_last_error()


def test_header_declares_and_library_exports_the_entries():
    from cmve import _lib
    src = open(os.path.join(ROOT, "include", "cmve.h")).read()
    for name in ("cmve_l2_topk_workspace", "cmve_l2_topk"):
        assert re.search(r"^int\s+%s\s*\(" % name, src, re.M), f"{name} is not declared in cmve.h"
        assert hasattr(_lib.lib, name) and name in _lib.exported_symbols()
    assert "#define CMVE_ABI_VERSION 21" in src and _lib.lib.cmve_abi_version() == 21
    assert "inference.py:78-80" in src[src.index("K20"):] and "evaluation.py:22-35" in src[src.index("K20"):]


def test_workspace_is_monotone_and_has_no_pair_term():
    q, g = _rows(1000, 1024), _rows(1 << 20, 1024)
    per_query = lambda cap, s: 4 * ((s + 127) // 128 * 128) + 4 * cap + 12
    # cand_cap: 4 bytes per slot and query of a round (1000 queries round up to 1024)
    sizes = [_ws(q, g, 10, cap, 4096) for cap in (10, 11, 512, 2048)]
    assert all(rc == 0 for rc, _ in sizes)
    assert [b for _, b in sizes] == [1024 * per_query(cap, 4096) for cap in (10, 11, 512, 2048)]
    # sample_rows: monotone, in steps of the 128-row tile, clamped to the gallery
    by_sample = [_ws(q, g, 10, 512, s)[1] for s in (1, 128, 129, 4096, 1 << 19, 1 << 20, 1 << 21)]
    assert by_sample == sorted(by_sample) and by_sample[0] == by_sample[1] < by_sample[2]
    assert by_sample[-1] == by_sample[-2] == 1024 * per_query(512, 1 << 20)
    # the sample is at least k
    assert _ws(q, g, 300, 512, 1)[1] == 1024 * per_query(512, 384)
    # the default sample: max(k, 8) / 128 of the gallery within [1024, 65536], never more than the gallery
    assert _ws(q, _rows(1 << 18, 1024), 10, 512, 0)[1] == 1024 * per_query(512, 10 * (1 << 11))
    assert _ws(q, _rows(1 << 18, 1024), 1, 512, 0)[1] == 1024 * per_query(512, 8 * (1 << 11))
    assert _ws(q, g, 64, 512, 0)[1] == 1024 * per_query(512, 65536)
    assert _ws(q, _rows(520, 1024), 10, 512, 0)[1] == 1024 * per_query(512, 520)
    # no term in n_q * n_g: past one round of queries the size does not depend on n_q at all, and a small batch
    # pays for its own rows only
    assert _ws(_rows(1 << 20, 1024), g, 10, 512, 0)[1] == _ws(_rows(1024, 1024), g, 10, 512, 0)[1]
    assert _ws(_rows(1, 1024), g, 10, 512, 0)[1] == 128 * per_query(512, 65536)
    assert _ws(_rows(0, 1024), g, 10, 512, 0)[0] == 0
    # d plays no part
    assert _ws(_rows(1000, 67), _rows(1 << 20, 67), 10, 512, 4096) == (0, 1024 * per_query(512, 4096))


def test_workspace_refuses_bad_arguments():
    from cmve import _lib
    q, g = _rows(300, 67), _rows(520, 67)
    n = C.c_int64()
    for args, word in (((0, 512, 0), b"k must be"), ((-3, 512, 0), b"k must be"), ((11, 10, 0), b"cand_cap"),
                       ((10, 2049, 0), b"cand_cap"), ((10, 512, -1), b"sample_rows")):
        rc, _ = _ws(q, g, *args)
        assert rc < 0 and b"cmve_l2_topk_workspace" in _err() and word in _err(), (args, _err())
    rc, _ = _ws(q, _rows(520, 68), 10, 512, 0)
    assert rc < 0 and b"cmve_l2_topk_workspace" in _err() and b"bad shape" in _err()
    f = _lib.lib.cmve_l2_topk_workspace
    assert f(None, C.byref(g), 10, 512, 0, C.byref(n)) < 0 and b"cmve_l2_topk_workspace" in _err() and b"NULL" in _err()
    assert f(C.byref(q), None, 10, 512, 0, C.byref(n)) < 0 and b"NULL" in _err()
    assert f(C.byref(q), C.byref(g), 10, 512, 0, None) < 0 and b"NULL" in _err()


def test_python_arguments_need_no_gpu():
    from cmve import engine
    from cmve.linas.inference import GalleryScorer
    assert inspect.signature(engine.pairwise_topk).parameters["filter"].default is None
    assert "filter" in inspect.signature(GalleryScorer.__init__).parameters
    assert inspect.signature(GalleryScorer.__init__).parameters["filter"].default is None
    for name in ("l2_topk", "l2_topk_workspace"):
        p = inspect.signature(getattr(engine, name)).parameters
        assert p["cand_cap"].default is None and p["sample_rows"].default is None
    assert isinstance(engine.L2_TOPK_FILTER_MIN_Q, int) and isinstance(engine.L2_TOPK_FILTER_MIN_PAIRS, int)
    assert 1 <= engine.L2_TOPK_CAND_MAX <= 2048 and 0 < engine.L2_TOPK_MAX_UNRESOLVED < 1
    assert not engine.l2_topk_auto(engine.L2_TOPK_FILTER_MIN_Q - 1, 1 << 40)
    assert engine.l2_topk_auto(max(engine.L2_TOPK_FILTER_MIN_Q, 1), engine.L2_TOPK_FILTER_MIN_PAIRS)
    # a packed gallery needs no minimum of queries: the gallery's size or the pair count decides
    assert engine.l2_topk_auto(1, engine.L2_TOPK_FILTER_MIN_GALLERY, packed=True)
    assert not engine.l2_topk_auto(1, engine.L2_TOPK_FILTER_MIN_GALLERY - 1, packed=True)
    assert not engine.l2_topk_auto(0, 1 << 40, packed=True) and not engine.l2_topk_auto(5, 0, packed=True)
