"""K21's host-only surface: the declaration of cmve_l2_count_resolved, the ``filter`` arguments of
engine.pairwise_count and ShardedGallery, and the band policy engine.l2_band_plan.  No kernel is launched, no GPU
needed."""
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_entry():
    from cmve import _lib
    src = open(os.path.join(ROOT, "include", "cmve.h")).read()
    name = "cmve_l2_count_resolved"
    assert re.search(r"^int\s+%s\s*\(" % name, src, re.M), f"{name} is not declared in cmve.h"
    assert hasattr(_lib.lib, name) and name in _lib.exported_symbols()
    # additive: the entries it stands beside are still there, and the ABI is still 21
    for old in ("cmve_l2_count_workspace", "cmve_l2_count", "cmve_pairwise_count"):
        assert re.search(r"^int\s+%s\s*\(" % old, src, re.M) and old in _lib.exported_symbols()
    assert "#define CMVE_ABI_VERSION 21" in src and _lib.lib.cmve_abi_version() == 21


def test_the_new_entry_takes_cmve_l2_counts_arguments():
    src = open(os.path.join(ROOT, "include", "cmve.h")).read()

    def params(name):
        m = re.search(r"^int\s+%s\s*\(([^;]*)\);" % name, src, re.M | re.S)
        return re.sub(r"\s+", " ", m.group(1)).strip()

    assert params("cmve_l2_count_resolved") == params("cmve_l2_count")


def test_filter_arguments_need_no_gpu():
    from cmve import engine
    from cmve.dist import ShardedGallery
    p = inspect.signature(engine.pairwise_count).parameters
    assert p["filter"].default is None and p["band"].default is None and p["return_stats"].default is False
    assert inspect.signature(ShardedGallery.__init__).parameters["filter"].default is None
    assert isinstance(ShardedGallery.filter_stats, property)


def test_band_plan_boundaries():
    from cmve.engine import l2_band_plan
    pairs = 8000
    # no overflow: the capacity stays, whatever the band
    assert l2_band_plan(pairs, 0, 0, 123) == 123
    assert l2_band_plan(pairs, 123, 0, 123) == 123
    assert l2_band_plan(pairs, 5000, False, 77) == 77
    # overflow with a band the filter still pays for: the reported need, the boundary band * 8 == pairs included
    assert l2_band_plan(pairs, 124, 1, 123) == 124
    assert l2_band_plan(pairs, 999, 1, 1) == 999
    assert l2_band_plan(pairs, 1000, 1, 1) == 1000
    # above 1/8 of the pairs: stop asking the filter
    assert l2_band_plan(pairs, 1001, 1, 1) is None
    assert l2_band_plan(pairs, pairs, 1, 0) is None
    # capacity 0 and numpy integers
    assert l2_band_plan(np.int64(pairs), np.int64(1), np.int64(1), 0) == 1
    assert l2_band_plan(0, 0, 0, 1) == 1


def test_first_band_capacity_is_the_unsharded_routes():
    from cmve.engine import l2_band_cap
    for pairs in (0, 1, 7, 8, 1 << 16, 1 << 19, (1 << 19) + 8, 1 << 23, (1 << 23) + 128, 16384 * 131072):
        assert l2_band_cap(pairs) == max(1, min(pairs // 8, max(1 << 16, pairs // 128)))


def test_filter_true_refuses_what_the_entry_cannot_express_before_any_device_call():
    import torch
    from cmve import _lib, engine

    class NoDevice:
        """Rows that fail loudly if the call gets as far as touching them."""
        def __getattr__(self, name):
            raise AssertionError("pairwise_count touched its operands before refusing")

    a = b = NoDevice()
    with pytest.raises(ValueError, match="PW_L2"):
        engine.pairwise_count(a, b, _lib.PW_L1, 1.0, 0.0, torch.float64, filter=True)
    with pytest.raises(ValueError, match="float64 score words"):
        engine.pairwise_count(a, b, _lib.PW_L2, 1.0, 0.0, torch.float32, filter=True)
    with pytest.raises(ValueError, match="alpha"):
        engine.pairwise_count(a, b, _lib.PW_L2, 0.0, 0.0, torch.float64, filter=True)
    for alpha, beta in ((float("nan"), 0.0), (float("inf"), 0.0), (1.0, float("inf")), (1.0, float("nan"))):
        with pytest.raises(ValueError, match="finite"):
            engine.pairwise_count(a, b, _lib.PW_L2, alpha, beta, torch.float64, filter=True)


@pytest.mark.parametrize("m", ["cosine", "l1", "l1_norm", "jaccard"])
def test_sharded_filter_true_needs_a_euclidean_measure(m):
    from cmve.dist import ShardedGallery

    class NoComm:
        rank, world = 0, 1

    with pytest.raises(ValueError, match="Euclidean"):
        ShardedGallery(np.zeros((4, 8), np.float32), offset=0, n_global=4, comm=NoComm(), measure=m, filter=True)


@pytest.fixture
def cpu_families(monkeypatch):
    """cmve.dist with both families' device-side set-up replaced by CPU tensors (oracle-style, as the gloo tests)."""
    import torch
    from cmve import dist as D

    def setup(self, local_embs, with_lo, eps, device, with_f16, cap):
        self.shard, self.n, self.device = torch.as_tensor(local_embs), len(local_embs), torch.device("cpu")
        self.eps, self.ws = eps, object()

    monkeypatch.setattr(D.CosineShardedGallery, "_setup", setup)
    monkeypatch.setattr(D.MeasureShardedGallery, "_pw_rows", lambda self, x: torch.as_tensor(x))
    return D


class _World1:
    rank, world = 0, 1


def test_the_one_constructor_builds_the_family_of_the_measure(cpu_families):
    D = cpu_families
    rows = np.zeros((4, 8), np.float32)
    cos = D.ShardedGallery(rows, offset=0, n_global=4, comm=_World1())
    assert type(cos) is D.CosineShardedGallery and isinstance(cos, D.ShardedGallery) and cos.measure == "cosine"
    for m in ("euclidean", "l1", "l2", "l1_norm", "l2_norm", "jaccard"):
        sh = D.ShardedGallery(rows, offset=0, n_global=4, comm=_World1(), measure=m)
        assert type(sh) is D.MeasureShardedGallery and isinstance(sh, D.ShardedGallery) and sh.measure == m
    # the measure given by position, as the signature allows
    assert type(D.ShardedGallery(rows, 0, 4, False, 0.0, None, True, _World1(), 8, "l1")) is D.MeasureShardedGallery
    with pytest.raises(ValueError, match="unknown measure"):
        D.ShardedGallery(rows, offset=0, n_global=4, comm=_World1(), measure="chebyshev")

    # a family named directly, or a subclass of one, is itself
    class Mine(D.MeasureShardedGallery):
        pass

    assert type(D.CosineShardedGallery(rows, offset=0, n_global=4, comm=_World1())) is D.CosineShardedGallery
    assert type(D.MeasureShardedGallery(rows, offset=0, n_global=4, comm=_World1(), measure="l2")) \
        is D.MeasureShardedGallery
    assert type(Mine(rows, offset=0, n_global=4, comm=_World1(), measure="jaccard")) is Mine

    # ... for its own measures only; what overrides the arithmetic subclasses a family, not the base alone
    class Bare(D.ShardedGallery):
        pass

    for cls, m in ((D.CosineShardedGallery, "l1"), (D.MeasureShardedGallery, "cosine"), (Mine, "cosine"),
                   (Bare, "cosine"), (Bare, "l2")):
        with pytest.raises(ValueError, match="needs a (Cosine|Measure)ShardedGallery"):
            cls(rows, offset=0, n_global=4, comm=_World1(), measure=m)


def test_each_family_holds_its_own_state_only(cpu_families):
    D = cpu_families
    rows = np.zeros((4, 8), np.float32)
    cos = D.ShardedGallery(rows, offset=0, n_global=4, comm=_World1())
    assert not [a for a in dir(cos) if a.startswith("_pw_")]
    assert hasattr(cos, "ws") and cos.eps == 0.0 and cos.filter_stats is None
    for m, f in (("l1", None), ("l2", None), ("l2", True), ("euclidean", False)):
        sh = D.ShardedGallery(rows, offset=0, n_global=4, comm=_World1(), measure=m, filter=f)
        assert not hasattr(sh, "ws") and not hasattr(sh, "eps") and sh.filter_stats is None
        assert sh._pw_packed is None and sh._pw_band is None and sh._pw_filter_off is False and sh.n == 4


def test_one_decoder_names_the_four_counters():
    from cmve import engine
    st = engine._l2_count_stats(np.array([7, 5, 3, 1], np.int64))
    assert st == {"decided": 7, "band": 5, "rescored": 3, "overflow": 1}
    assert list(st) == ["decided", "band", "rescored", "overflow"] and all(type(v) is int for v in st.values())
