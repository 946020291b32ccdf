"""cmve_pairwise_bwd_workspace (K17's workspace sizing): host only -- no kernel is launched, no GPU needed.

The workspace holds the per-pair coefficients of the backward, so it is O(na * nb) and independent of d:
no na x nb x d intermediate exists."""
import ctypes as C

import pytest

METRICS = ["PW_SQ_L2", "PW_L1", "PW_ORDER", "PW_JACCARD"]


def _ws(na, nb, metric):
    from cmve import _lib
    n = C.c_int64(-1)
    return _lib.lib.cmve_pairwise_bwd_workspace(na, nb, metric, C.byref(n)), n.value


@pytest.mark.parametrize("name", METRICS)
def test_workspace_grows_with_the_pair_count(name):
    from cmve import _lib
    metric = getattr(_lib, name)
    rc, b1 = _ws(128, 128, metric)
    assert rc == 0 and 0 < b1 <= 128 * 128 * 16  # at most two fp64 coefficients per pair
    rc, b2 = _ws(256, 128, metric)
    assert rc == 0 and b2 == 2 * b1
    rc, b3 = _ws(128, 256, metric)
    assert rc == 0 and b3 == 2 * b1
    rc, b0 = _ws(0, 128, metric)
    assert rc == 0 and b0 == 0


def test_engine_wrapper_sizes_without_a_gpu():
    from cmve import _lib, engine
    assert engine.pairwise_bwd_workspace(33, 37, _lib.PW_JACCARD) == _ws(33, 37, _lib.PW_JACCARD)[1]


def test_workspace_refuses_bad_arguments():
    from cmve import _lib
    rc, _ = _ws(-1, 128, _lib.PW_L1)
    assert rc < 0 and b"cmve_pairwise_bwd_workspace" in _lib.lib.cmve_last_error()
    rc, _ = _ws(128, -1, _lib.PW_L1)
    assert rc < 0 and b"bad shape" in _lib.lib.cmve_last_error()
    for name in ("PW_L2", "PW_DOT"):  # no loss.py measure uses them
        rc, _ = _ws(128, 128, getattr(_lib, name))
        assert rc < 0 and b"no backward" in _lib.lib.cmve_last_error()
    rc, _ = _ws(128, 128, 17)
    assert rc < 0 and b"unknown metric" in _lib.lib.cmve_last_error()
    assert _lib.lib.cmve_pairwise_bwd_workspace(128, 128, _lib.PW_L1, None) < 0
    assert b"NULL" in _lib.lib.cmve_last_error()
    rc, _ = _ws(1 << 40, 1 << 40, _lib.PW_L1)
    assert rc < 0 and b"overflows" in _lib.lib.cmve_last_error()
