"""K19's host-only surface (cmve_l2_count_workspace, the declarations): no kernel is launched, no GPU needed.

The workspace of cmve_l2_count is the band list alone: one (i, j) pair of int32 -- 8 bytes -- per slot."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rows(n, d):
    from cmve import _lib
    r = _lib.Rows()
    r.n, r.d = n, d
    r.n_pad, r.d_pad = (n + 255) // 256 * 256, (d + 63) // 64 * 64
    return r


def _ws(a, b, cap):
    from cmve import _lib
    n = C.c_int64(-1)
    return _lib.lib.cmve_l2_count_workspace(C.byref(a), C.byref(b), cap, C.byref(n)), n.value


def _err():
    from cmve import _lib
    return _lib.lib.cmve_last_error()


def test_workspace_grows_by_eight_bytes_per_band_slot():
    a, b = _rows(16384, 1024), _rows(131072, 1024)
    rc0, b0 = _ws(a, b, 0)
    rc1, b1 = _ws(a, b, 1)
    rc2, b2 = _ws(a, b, 1 << 20)
    assert (rc0, rc1, rc2) == (0, 0, 0)
    assert b1 - b0 == 8 and b2 - b0 == 8 << 20
    # nothing proportional to the pair count or to the sets
    assert _ws(_rows(300, 67), _rows(520, 67), 1 << 20) == (0, b2)
    assert _ws(_rows(0, 67), _rows(0, 67), 5) == (0, b0 + 40)


def test_workspace_refuses_bad_arguments():
    from cmve import _lib
    a, b = _rows(300, 67), _rows(520, 67)
    rc, _ = _ws(a, b, -1)
    assert rc < 0 and b"cmve_l2_count_workspace" in _err() and b"capacity" in _err()
    n = C.c_int64()
    assert _lib.lib.cmve_l2_count_workspace(None, C.byref(b), 1, C.byref(n)) < 0
    assert b"cmve_l2_count_workspace" in _err() and b"NULL" in _err()
    assert _lib.lib.cmve_l2_count_workspace(C.byref(a), None, 1, C.byref(n)) < 0 and b"NULL" in _err()
    assert _lib.lib.cmve_l2_count_workspace(C.byref(a), C.byref(b), 1, None) < 0 and b"NULL" in _err()
    rc, _ = _ws(a, _rows(520, 68), 1)
    assert rc < 0 and b"cmve_l2_count_workspace" in _err() and b"bad shape" in _err()


def test_header_declares_and_library_exports_the_entries():
    from cmve import _lib
    src = open(os.path.join(ROOT, "include", "cmve.h")).read()
    for name in ("cmve_l2_count_workspace", "cmve_l2_count"):
        assert re.search(r"^int\s+%s\s*\(" % name, src, re.M), f"{name} is not declared in cmve.h"
        assert hasattr(_lib.lib, name) and name in _lib.exported_symbols()
    assert "#define CMVE_ABI_VERSION 21" in src and _lib.lib.cmve_abi_version() == 21


def test_engine_wrapper_and_filter_argument_need_no_gpu():
    import inspect
    from cmve import engine
    assert isinstance(engine.L2_FILTER_MIN_PAIRS, int) and engine.L2_FILTER_MIN_PAIRS > 0
    for f in (engine.pairwise_gt_positions, engine.pairwise_gt_ranks, engine.pairwise_gt_eval,
              engine._PairwisePositions.__init__):
        assert inspect.signature(f).parameters["filter"].default is None


def test_each_entry_refuses_a_set_without_its_fp16_plane_under_its_own_name():
    """The checks on the two sets are shared by the three entries (l2f_check_sets); the refusal still begins with
    the name of the entry that was called.  Every check runs before the handle is used, so a host buffer stands in
    for it and nothing is launched."""
    from cmve import _lib
    a, b = _rows(300, 67), _rows(520, 67)  # h16 / err_h16 are NULL: packed without the fp16 plane
    h = C.create_string_buffer(256)
    stats = (C.c_int64 * 4)()
    lib = _lib.lib
    for name in ("cmve_l2_count", "cmve_l2_count_resolved"):
        rc = getattr(lib, name)(h, C.byref(a), C.byref(b), 1.0, 0.0, None, None, 0, 0, None, None, None, 0, 0, None,
                                None, 0, stats)
        assert rc < 0 and _err().startswith(name.encode() + b": a set was packed without its fp16 plane"), _err()
    rc = lib.cmve_l2_topk(h, C.byref(a), C.byref(b), 1.0, 0.0, 10, 2048, 0, None, 0, None, None, stats)
    assert rc < 0 and _err().startswith(b"cmve_l2_topk: a set was packed without its fp16 plane"), _err()
