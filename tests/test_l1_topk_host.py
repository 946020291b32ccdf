"""K23's host-only surface (cmve_l1_topk_workspace, the declarations, the Python arguments and refusals, the auto
rule): no kernel is launched, no GPU needed.

The workspace of cmve_l1_topk is cmve_l2_topk's: what ONE round of min(1024, round_up128(n_q)) queries needs -- per
query the sample's upper key bounds (4 bytes per sample row, rounded up to the 128-row tile), the candidate list
(4 bytes per slot), the threshold (8) and the counter (4)."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cmve_l1_topk_workspace", "cmve_l1_topk")


def _ws(n_q, n_g, k, cap, sample):
    from cmve import _lib
    n = C.c_int64(-1)
    return _lib.lib.cmve_l1_topk_workspace(n_q, n_g, k, cap, sample, C.byref(n)), n.value


def _err():
    from cmve import _lib
    return _lib.lib.cmve_last_error()


class NoDevice:
    """Rows that fail loudly if the call gets as far as touching them."""
    def __getattr__(self, name):
        raise AssertionError("the call touched its operands before refusing")


def test_header_declares_and_library_exports_the_entries():
    from cmve import _lib
    src = open(os.path.join(ROOT, "include", "cmve.h")).read()
    for name in NAMES:
        assert re.search(r"^int\s+%s\s*\(" % name, src, re.M), f"{name} is not declared in cmve.h"
        assert hasattr(_lib.lib, name) and name in _lib.exported_symbols()
    assert "#define CMVE_ABI_VERSION 21" in src and _lib.lib.cmve_abi_version() == 21  # additive
    doc = src[src.index("/* K23:"):src.index("int cmve_l1_topk_workspace")]
    assert "inference.py:78-80" in doc and "evaluation.py:22-35" in doc
    for old in ("cmve_l2_topk_workspace", "cmve_l2_topk", "cmve_l1_count", "cmve_pairwise_topk"):
        assert re.search(r"^int\s+%s\s*\(" % old, src, re.M) and old in _lib.exported_symbols()


def test_the_entry_takes_the_counts_sides_and_the_euclidean_tail():
    src = open(os.path.join(ROOT, "include", "cmve.h")).read()

    def params(name):
        m = re.search(r"^int\s+%s\s*\(([^;]*)\);" % name, src, re.M | re.S)
        return re.sub(r"\s+", " ", m.group(1)).strip()

    count, l2, l1 = params("cmve_l1_count"), params("cmve_l2_topk"), params("cmve_l1_topk")
    sides = count.split("int64_t d, const double* grid")[0]  # (h, A .. a_err, B .. b_err,)
    for a, b in (("A", "Q"), ("B", "G"), ("a_", "q_"), ("b_", "g_"), ("lda", "ldq"), ("ldb", "ldg"), ("na", "n_q"),
                 ("nb", "n_g")):
        sides = re.sub(r"\b%s(?=\b|[a-z])" % a if a.endswith("_") else r"\b%s\b" % a, b, sides)
    assert l1.startswith(sides + "int64_t d, const double* grid, double alpha, double beta, ")
    assert l1.endswith(l2.split("double alpha, double beta, ")[1])  # k, cand_cap, sample_rows, ws .. stats


def test_workspace_equals_the_layout_formula():
    per_query = lambda cap, s: 4 * ((s + 127) // 128 * 128) + 4 * cap + 12
    big = 1 << 20
    sizes = [_ws(1000, big, 10, cap, 4096) for cap in (10, 11, 512, 2048)]
    assert [b for _, b in sizes] == [1024 * per_query(cap, 4096) for cap in (10, 11, 512, 2048)]
    assert all(rc == 0 for rc, _ in sizes)
    by_sample = [_ws(1000, big, 10, 512, s)[1] for s in (1, 128, 129, 4096, 1 << 19, 1 << 20, 1 << 21)]
    assert by_sample == sorted(by_sample) and by_sample[0] == by_sample[1] < by_sample[2]
    assert by_sample[-1] == by_sample[-2] == 1024 * per_query(512, big)
    assert _ws(1000, big, 300, 512, 1)[1] == 1024 * per_query(512, 384)           # the sample is at least k
    assert _ws(1000, 1 << 18, 10, 512, 0)[1] == 1024 * per_query(512, 10 * (1 << 11))  # the default sample
    assert _ws(1000, 1 << 18, 1, 512, 0)[1] == 1024 * per_query(512, 8 * (1 << 11))
    assert _ws(1000, big, 64, 512, 0)[1] == 1024 * per_query(512, 65536)
    assert _ws(1000, 520, 10, 512, 0)[1] == 1024 * per_query(512, 520)
    # no n_q * n_g term; a small batch pays for its own rows only; an empty batch is accepted
    assert _ws(big, big, 10, 512, 0)[1] == _ws(1024, big, 10, 512, 0)[1]
    assert _ws(1, big, 10, 512, 0)[1] == 128 * per_query(512, 65536)
    assert _ws(0, big, 10, 512, 0)[0] == 0
    # the same formula as the Euclidean entry's
    from cmve import _lib, engine
    q, g = _lib.Rows(), _lib.Rows()
    q.n, q.d, g.n, g.d = 300, 67, 520, 67
    n = C.c_int64()
    for k, cap, sample in ((10, 512, 0), (64, 2048, 128), (1, 12, 129)):
        assert _lib.lib.cmve_l2_topk_workspace(C.byref(q), C.byref(g), k, cap, sample, C.byref(n)) == 0
        assert engine.l1_topk_workspace(300, 520, k, cap, sample) == n.value
    assert engine.l1_topk_workspace(300, 520, 10) == engine.l1_topk_workspace(300, 520, 10, engine.L1_TOPK_CAND_MAX, 0)


def test_workspace_refuses_bad_arguments():
    from cmve import _lib
    for args, word in (((300, 520, 0, 512, 0), b"k must be"), ((300, 520, -3, 512, 0), b"k must be"),
                       ((300, 520, 11, 10, 0), b"cand_cap"), ((300, 520, 10, 2049, 0), b"cand_cap"),
                       ((300, 520, 10, 512, -1), b"sample_rows"), ((-1, 520, 10, 512, 0), b"bad shape"),
                       ((300, 1 << 31, 10, 512, 0), b"bad shape")):
        rc, _ = _ws(*args)
        assert rc < 0 and b"cmve_l1_topk_workspace" in _err() and word in _err(), (args, _err())
    assert _lib.lib.cmve_l1_topk_workspace(300, 520, 10, 512, 0, None) < 0 and b"NULL" in _err()


def test_filter_l1_refuses_before_any_device_call():
    import torch
    from cmve import _lib, engine
    from cmve import dist as D
    a = b = NoDevice()
    with pytest.raises(ValueError, match="PW_L1"):
        engine.pairwise_topk(a, b, _lib.PW_L2, 1.0, 0.0, torch.float64, 10, filter="l1")
    with pytest.raises(ValueError, match="float64 score words"):
        engine.pairwise_topk(a, b, _lib.PW_L1, 1.0, 0.0, torch.float32, 10, filter="l1")
    for alpha, beta in ((0.0, 0.0), (float("nan"), 0.0), (float("inf"), 0.0), (1.0, float("inf"))):
        with pytest.raises(ValueError, match="alpha finite and non-zero"):
            engine.pairwise_topk(a, b, _lib.PW_L1, alpha, beta, torch.float64, 10, filter="l1")
    # filter=True keeps speaking for PW_L2 alone
    with pytest.raises(ValueError, match="PW_L2"):
        engine.pairwise_topk(a, b, _lib.PW_L1, 1.0, 0.0, torch.float64, 10, filter=True)

    # two packs on different grids (stand-ins: the rule looks at the grid tensors' addresses and nothing else)
    class Grid:
        def __init__(self, p):
            self.p = p

        def data_ptr(self):
            return self.p

    class Pack:
        def __init__(self, p):
            self.grid = Grid(p)

    with pytest.raises(ValueError, match="different grids"):
        engine._l1_sets(None, None, Pack(8), Pack(16))
    one = Pack(8)
    assert engine._l1_sets(None, None, one, Pack(8))[0] is one
    # the sharded gallery: filter="l1" needs an L1 measure, filter=True a Euclidean one
    for measure in ("l2", "euclidean", "jaccard", "cosine"):
        with pytest.raises(ValueError, match='filter="l1"'):
            D.ShardedGallery(NoDevice(), offset=0, n_global=4, comm=D.LocalGroup(1), measure=measure, filter="l1")
    with pytest.raises(ValueError, match="Euclidean"):
        D.ShardedGallery(NoDevice(), offset=0, n_global=4, comm=D.LocalGroup(1), measure="l1", filter=True)


def test_auto_rule_and_python_arguments(monkeypatch):
    from cmve import engine
    from cmve.linas.inference import GalleryScorer
    assert engine.L1_TOPK_CAND_MAX == engine.L2_TOPK_CAND_MAX == 2048
    for name in ("l1_topk", "l1_topk_workspace"):
        p = inspect.signature(getattr(engine, name)).parameters
        assert p["cand_cap"].default is None and p["sample_rows"].default is None
    assert list(inspect.signature(engine.l1_topk).parameters)[:5] == ["q", "g", "alpha", "beta", "k"]
    assert "filter" in inspect.signature(GalleryScorer.__init__).parameters
    names = ("L1_TOPK_FILTER_MIN_Q", "L1_TOPK_FILTER_MIN_PAIRS", "L1_TOPK_FILTER_MIN_GALLERY",
             "L1_TOPK_FILTER_MIN_PLAIN_PAIRS")
    for n in names:
        v = getattr(engine, n)
        assert v is None or (isinstance(v, int) and v >= 1)
    # never for an empty side, whatever the constants
    for packed in (False, True):
        assert not engine.l1_topk_auto(0, 1 << 40, packed=packed) and not engine.l1_topk_auto(5, 0, packed=packed)
        assert not engine.l1_topk_auto(-1, 1 << 40, packed=packed)
    # the existing dispatch test expects PW_L1 at 300 x 520 plain rows on the fp64 route
    assert not engine.l1_topk_auto(300, 520)
    # never while the constants are None
    for n in names:
        monkeypatch.setattr(engine, n, None)
    for packed in (False, True):
        assert not engine.l1_topk_auto(1 << 20, 1 << 30, packed=packed)
    # and a rule of its own: the Euclidean constants play no part
    monkeypatch.setattr(engine, "L2_TOPK_FILTER_MIN_Q", 1)
    monkeypatch.setattr(engine, "L2_TOPK_FILTER_MIN_PAIRS", 1)
    monkeypatch.setattr(engine, "L2_TOPK_FILTER_MIN_GALLERY", 1)
    assert not engine.l1_topk_auto(1 << 20, 1 << 30, packed=True) and not engine.l1_topk_auto(1 << 20, 1 << 30)
    # plain rows: queries AND pairs; a packed gallery: its size OR the pairs -- each clause switched on by its constant
    monkeypatch.setattr(engine, "L1_TOPK_FILTER_MIN_Q", 4)
    assert not engine.l1_topk_auto(1 << 20, 1 << 30)
    monkeypatch.setattr(engine, "L1_TOPK_FILTER_MIN_PLAIN_PAIRS", 4000)
    assert engine.l1_topk_auto(4, 1000) and not engine.l1_topk_auto(3, 1 << 20) and not engine.l1_topk_auto(4, 999)
    assert not engine.l1_topk_auto(1 << 20, 1 << 30, packed=True)
    monkeypatch.setattr(engine, "L1_TOPK_FILTER_MIN_PAIRS", 4000)
    assert engine.l1_topk_auto(1, 4000, packed=True) and not engine.l1_topk_auto(1, 3999, packed=True)
    monkeypatch.setattr(engine, "L1_TOPK_FILTER_MIN_GALLERY", 100)
    assert engine.l1_topk_auto(1, 100, packed=True) and not engine.l1_topk_auto(1, 100)


def test_pairwise_topk_under_l1_never_reads_the_euclidean_constants(monkeypatch):
    """filter=None with PW_L1: the route is decided by l1_topk_auto alone.  The Euclidean constants are replaced by
    objects that fail on any use; the call must get as far as the fp64 entry (which here has no device to run on:
    the operands are stand-ins that stop it right after the route is decided)."""
    import torch
    from cmve import _lib, engine

    class Poison:
        def _no(self, *a):
            raise AssertionError("pairwise_topk(PW_L1) read an L2_TOPK_* constant")
        __le__ = __lt__ = __ge__ = __gt__ = __eq__ = __bool__ = __int__ = __index__ = __rmul__ = __mul__ = _no

    for n in ("L2_TOPK_FILTER_MIN_Q", "L2_TOPK_FILTER_MIN_PAIRS", "L2_TOPK_FILTER_MIN_GALLERY"):
        monkeypatch.setattr(engine, n, Poison())
    seen = []
    monkeypatch.setattr(engine, "l1_topk_auto", lambda n_q, n_g, packed=False: seen.append((n_q, n_g, packed)) or False)

    class Stop(Exception):
        pass

    def stop(*a, **k):
        raise Stop()

    monkeypatch.setattr(engine, "pairwise_topk_workspace", stop)  # the first thing the fp64 route asks for
    rows = lambda n: torch.zeros((n, 8), dtype=torch.float64)
    monkeypatch.setattr(engine, "_pw_pair", lambda a, b, name: (a, b))
    with pytest.raises(Stop):
        engine.pairwise_topk(rows(300), rows(520), _lib.PW_L1, 1.0, 0.0, torch.float64, 10)
    assert seen == [(300, 520, False)]
