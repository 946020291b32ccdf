"""K25's host-only surface (cmve_jaccard_topk_workspace, the declarations, the Python arguments and refusals, the auto
rule, the routing of ``pairwise_topk``, the sharded and serving constructors) and a numpy port of the device's
decision -- jact_widen and launches A / A' / B (tests/jaccard_topk_model.py) -- run over K24's adversarial rows against
the canonical float32 words.  No kernel is launched, no GPU needed."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import jaccard_topk_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cmve_jaccard_topk_workspace", "cmve_jaccard_topk")
AUTO = ("JACCARD_TOPK_FILTER_MIN_Q", "JACCARD_TOPK_FILTER_MIN_PAIRS", "JACCARD_TOPK_FILTER_MIN_GALLERY",
        "JACCARD_TOPK_FILTER_MIN_PLAIN_PAIRS")


class NoDevice:
    """Rows that fail loudly if the call gets as far as touching them."""
    def __getattr__(self, name):
        raise AssertionError("the call touched its operands before refusing")


def _ws(n_q, n_g, k, cap, sample):
    from cmve import _lib
    n = C.c_int64(-1)
    return _lib.lib.cmve_jaccard_topk_workspace(n_q, n_g, k, cap, sample, C.byref(n)), n.value


def _err():
    from cmve import _lib
    return _lib.lib.cmve_last_error()


def _params(src, name):
    m = re.search(r"^int\s+%s\s*\(([^;]*)\);" % name, src, re.M | re.S)
    return re.sub(r"\s+", " ", m.group(1)).strip()


def test_header_declares_and_library_exports_the_entries():
    from cmve import _lib
    src = open(os.path.join(ROOT, "include", "cmve.h")).read()
    for name in NAMES:
        assert re.search(r"^int\s+%s\s*\(" % name, src, re.M), f"{name} is not declared in cmve.h"
        assert hasattr(_lib.lib, name) and name in _lib.exported_symbols()
    doc = src[src.index("/* K25:"):src.index("int cmve_jaccard_topk_workspace")]
    assert "inference.py:78-80" in doc and "evaluation.py:32-35" in doc
    assert "#define CMVE_ABI_VERSION 21" in src and _lib.lib.cmve_abi_version() == 21
    for old in ("cmve_l1_topk", "cmve_l2_topk", "cmve_jaccard_count", "cmve_jaccard_rowsums", "cmve_pairwise_topk"):
        assert re.search(r"^int\s+%s\s*\(" % old, src, re.M) and old in _lib.exported_symbols()


def test_the_entry_takes_l1_topks_arguments_plus_the_row_sums():
    src = open(os.path.join(ROOT, "include", "cmve.h")).read()
    want = _params(src, "cmve_l1_topk")
    want = want.replace("const double* q_err, ", "const double* q_err, const int64_t* q_qsum, const double* q_asum, ")
    want = want.replace("const double* g_err, ", "const double* g_err, const int64_t* g_qsum, const double* g_asum, ")
    assert _params(src, "cmve_jaccard_topk") == want
    assert _params(src, "cmve_jaccard_topk_workspace") == _params(src, "cmve_l1_topk_workspace")
    from cmve import _lib
    assert len(_lib.SIGNATURES["cmve_jaccard_topk"][1]) == len(_lib.SIGNATURES["cmve_l1_topk"][1]) + 4


def test_workspace_is_the_layout_formula_and_l1_topks():
    from cmve import engine
    r128 = lambda n: (n + 127) // 128 * 128  # noqa: E731
    for n_q, n_g, k, cap, sample in ((300, 520, 10, 512, 0), (300, 520, 64, 2048, 128), (1, 131072, 10, 2048, 0),
                                     (5000, 1 << 20, 32, 100, 0), (0, 0, 1, 1, 0), (1025, 130, 3, 2048, 7)):
        rc, got = _ws(n_q, n_g, k, cap, sample)
        qc = min(1024, r128(max(n_q, 1)))
        s = M.sample_of(n_g, k, sample)
        want = qc * 8 + qc * r128(s) * 4 + qc * cap * 4 + qc * 4
        assert rc == 0 and got == (want + 7) // 8 * 8, (n_q, n_g, k, cap, sample, got, want)
        assert got == engine.l1_topk_workspace(n_q, n_g, k, cap, sample)
        assert got == engine.jaccard_topk_workspace(n_q, n_g, k, cap, sample)
    assert engine.jaccard_topk_workspace(300, 520, 10) == engine.jaccard_topk_workspace(
        300, 520, 10, engine.JACCARD_TOPK_CAND_MAX, 0)
    for args, word in (((300, 520, 0, 512, 0), b"k must be"), ((300, 520, 10, 9, 0), b"cand_cap"),
                       ((300, 520, 10, 2049, 0), b"cand_cap"), ((300, 520, 10, 512, -1), b"sample_rows"),
                       ((300, 520, 10, 512, 1 << 31), b"sample_rows"), ((-1, 520, 10, 512, 0), b"bad shape"),
                       ((300, 1 << 31, 10, 512, 0), b"bad shape")):
        rc, _ = _ws(*args)
        assert rc < 0 and b"cmve_jaccard_topk_workspace" in _err() and word in _err(), (args, _err())
    from cmve import _lib
    assert _lib.lib.cmve_jaccard_topk_workspace(300, 520, 10, 512, 0, None) < 0 and b"NULL" in _err()


def test_filter_jaccard_refuses_before_any_device_call():
    import torch
    from cmve import _lib, engine
    a = b = NoDevice()
    with pytest.raises(ValueError, match='filter="jaccard" needs PW_JACCARD'):
        engine.pairwise_topk(a, b, _lib.PW_L1, 1.0, 0.0, torch.float32, 10, filter="jaccard")
    with pytest.raises(ValueError, match='filter="jaccard" needs PW_JACCARD'):
        engine.pairwise_topk(a, b, _lib.PW_L2, 1.0, 0.0, torch.float64, 10, filter="jaccard")
    with pytest.raises(ValueError, match='filter="jaccard".*float32 score words'):
        engine.pairwise_topk(a, b, _lib.PW_JACCARD, -1.0, 0.0, torch.float64, 10, filter="jaccard")
    for alpha, beta in ((0.0, 0.0), (float("nan"), 0.0), (float("inf"), 0.0), (1.0, float("inf")),
                        (-1.0, float("nan"))):
        with pytest.raises(ValueError, match='filter="jaccard".*alpha finite and non-zero'):
            engine.pairwise_topk(a, b, _lib.PW_JACCARD, alpha, beta, torch.float32, 10, filter="jaccard")
    # the other forced routes keep their words
    with pytest.raises(ValueError, match="PW_L2"):
        engine.pairwise_topk(a, b, _lib.PW_JACCARD, -1.0, 0.0, torch.float32, 10, filter=True)
    with pytest.raises(ValueError, match="PW_L1"):
        engine.pairwise_topk(a, b, _lib.PW_JACCARD, -1.0, 0.0, torch.float32, 10, filter="l1")
    with pytest.raises(ValueError, match="float64 score words"):
        engine.pairwise_topk(a, b, _lib.PW_L1, 1.0, 0.0, torch.float32, 10, filter="l1")


def test_auto_rule_and_python_arguments(monkeypatch):
    from cmve import engine
    assert engine.JACCARD_TOPK_CAND_MAX == engine.L2_TOPK_CAND_MAX == 2048
    for name in ("jaccard_topk", "jaccard_topk_workspace"):
        p = inspect.signature(getattr(engine, name)).parameters
        assert p["cand_cap"].default is None and p["sample_rows"].default is None
    assert list(inspect.signature(engine.jaccard_topk).parameters) == ["q", "g", "alpha", "beta", "k", "cand_cap",
                                                                         "sample_rows", "ws"]
    for n in AUTO:
        v = getattr(engine, n)
        assert v is None or (isinstance(v, int) and v >= 1)
    for packed in (False, True):
        assert not engine.jaccard_topk_auto(0, 1 << 40, packed=packed)
        assert not engine.jaccard_topk_auto(5, 0, packed=packed) and not engine.jaccard_topk_auto(-1, 1 << 40, packed=packed)
    # the sharded tests expect 300 x 520 plain rows on the K18 route
    assert not engine.jaccard_topk_auto(300, 520)
    for n in AUTO:
        monkeypatch.setattr(engine, n, None)
    for packed in (False, True):
        assert not engine.jaccard_topk_auto(1 << 20, 1 << 30, packed=packed)
    # a rule of its own: the other filters' constants play no part
    for n in ("L2_TOPK_FILTER_MIN_Q", "L2_TOPK_FILTER_MIN_PAIRS", "L2_TOPK_FILTER_MIN_GALLERY", "L1_TOPK_FILTER_MIN_Q",
              "L1_TOPK_FILTER_MIN_PAIRS", "L1_TOPK_FILTER_MIN_GALLERY", "L1_TOPK_FILTER_MIN_PLAIN_PAIRS"):
        monkeypatch.setattr(engine, n, 1)
    assert not engine.jaccard_topk_auto(1 << 20, 1 << 30, packed=True) and not engine.jaccard_topk_auto(1 << 20, 1 << 30)
    # plain rows: queries AND pairs; a packed gallery: its size OR the pairs -- each clause switched on by its constant
    monkeypatch.setattr(engine, "JACCARD_TOPK_FILTER_MIN_Q", 4)
    assert not engine.jaccard_topk_auto(1 << 20, 1 << 30)
    monkeypatch.setattr(engine, "JACCARD_TOPK_FILTER_MIN_PLAIN_PAIRS", 4000)
    assert engine.jaccard_topk_auto(4, 1000) and not engine.jaccard_topk_auto(3, 1 << 20)
    assert not engine.jaccard_topk_auto(4, 999) and not engine.jaccard_topk_auto(1 << 20, 1 << 30, packed=True)
    monkeypatch.setattr(engine, "JACCARD_TOPK_FILTER_MIN_PAIRS", 4000)
    assert engine.jaccard_topk_auto(1, 4000, packed=True) and not engine.jaccard_topk_auto(1, 3999, packed=True)
    monkeypatch.setattr(engine, "JACCARD_TOPK_FILTER_MIN_GALLERY", 100)
    assert engine.jaccard_topk_auto(1, 100, packed=True) and not engine.jaccard_topk_auto(1, 100)


def test_pairwise_topk_under_jaccard_reads_its_own_rule_alone(monkeypatch):
    """filter=None with PW_JACCARD and float32 words: the route is decided by jaccard_topk_auto alone.  The L1 and L2
    constants are replaced by objects that fail on any use; the call must get as far as the K18 entry (the operands
    are stand-ins that stop it right after the route is decided)."""
    import torch
    from cmve import _lib, engine

    class Poison:
        def _no(self, *a):
            raise AssertionError("pairwise_topk(PW_JACCARD) read another filter's constant")
        __le__ = __lt__ = __ge__ = __gt__ = __eq__ = __bool__ = __int__ = __index__ = __rmul__ = __mul__ = _no

    for n in ("L2_TOPK_FILTER_MIN_Q", "L2_TOPK_FILTER_MIN_PAIRS", "L2_TOPK_FILTER_MIN_GALLERY", "L1_TOPK_FILTER_MIN_Q",
              "L1_TOPK_FILTER_MIN_PAIRS", "L1_TOPK_FILTER_MIN_GALLERY", "L1_TOPK_FILTER_MIN_PLAIN_PAIRS"):
        monkeypatch.setattr(engine, n, Poison())
    seen = []
    monkeypatch.setattr(engine, "jaccard_topk_auto",
                        lambda n_q, n_g, packed=False: seen.append((n_q, n_g, packed)) or False)
    for other in ("l1_topk_auto", "l2_topk_auto"):
        monkeypatch.setattr(engine, other, lambda *a, **k: (_ for _ in ()).throw(AssertionError("another rule was asked")))

    class Stop(Exception):
        pass

    def stop(*a, **k):
        raise Stop()

    monkeypatch.setattr(engine, "pairwise_topk_workspace", stop)  # the first thing the K18 route asks for
    rows = lambda n: torch.zeros((n, 8), dtype=torch.float32)  # noqa: E731
    monkeypatch.setattr(engine, "_pw_pair", lambda a, b, name: (a, b))
    with pytest.raises(Stop):
        engine.pairwise_topk(rows(300), rows(520), _lib.PW_JACCARD, -1.0, 0.0, torch.float32, 10)
    assert seen == [(300, 520, False)]
    # float64 words under jaccard have no filter: no rule is asked at all
    with pytest.raises(Stop):
        engine.pairwise_topk(rows(300), rows(520), _lib.PW_JACCARD, -1.0, 0.0, torch.float64, 10)
    assert len(seen) == 1


def test_no_route_falls_through_to_the_euclidean_arm(monkeypatch):
    """The latent misroute: a jaccard request that reached the filtered arms used to pack a RowSet and call
    cmve_l2_topk.  With the jaccard call stubbed, filter="jaccard" must reach it and nothing Euclidean."""
    import torch
    from cmve import _lib, engine

    class Stop(Exception):
        pass

    def no(*a, **k):
        raise AssertionError("the Euclidean arm ran under a jaccard request")

    def stop(*a, **k):
        raise Stop()

    monkeypatch.setattr(engine, "RowSet", type("RowSet", (), {"__init__": no}))
    monkeypatch.setattr(engine, "l2_topk", no)
    monkeypatch.setattr(engine, "l1_topk", no)
    monkeypatch.setattr(engine, "_l1_sets", stop)  # the first thing the jaccard arm does
    monkeypatch.setattr(engine, "_pw_pair", lambda a, b, name: (a, b))
    rows = lambda n: torch.zeros((n, 8), dtype=torch.float32)  # noqa: E731
    with pytest.raises(Stop):
        engine.pairwise_topk(rows(3), rows(5), _lib.PW_JACCARD, -1.0, 0.0, torch.float32, 2, filter="jaccard")


def test_sharded_and_serving_constructors_refuse_with_their_words():
    from cmve import dist as D
    from cmve.linas.inference import GalleryScorer
    shard = lambda **kw: D.ShardedGallery(NoDevice(), offset=0, n_global=4, comm=D.LocalGroup(1), **kw)  # noqa: E731
    with pytest.raises(ValueError, match='filter="l1"'):
        shard(measure="jaccard", filter="l1")
    with pytest.raises(ValueError, match="Euclidean"):
        shard(measure="jaccard", filter=True)
    for measure in ("l1", "l1_norm", "l2", "euclidean", "cosine"):
        with pytest.raises(ValueError, match='filter="jaccard"'):
            shard(measure=measure, filter="jaccard")
        with pytest.raises(ValueError, match='filter="jaccard"'):
            GalleryScorer(NoDevice(), measure=measure, filter="jaccard")


# ---- the decision of launches A / A' / B, restated in numpy ----------------------------------------------------------

def test_numpy_port_of_jact_widen():
    """The check inside jact_widen is the proof: whenever a threshold comes back, the float32 word of q_tau (and of
    every quotient on the witnesses' side of it) is strictly below the word of any quotient beyond the threshold."""
    rng = np.random.default_rng(5)
    for alpha, beta in M.AB + ((3.0, -7.0), (-1e-3, 1e3), (1e20, 0.0)):
        pos = alpha > 0.0
        taus = np.concatenate([rng.uniform(-1.0, 1.0, 200), [0.0, 1.0, -1.0, M.F32_MIN_NORMAL, 1e-30, -1e-30]])
        accepted = np.zeros(13, np.int64)
        for tau in taus.astype(np.float32):
            thr, guess = M.widen(tau, alpha, beta)
            accepted[guess] += 1
            if np.isnan(thr):
                continue
            q_tau = float(tau) if pos else -float(tau)
            far = np.nextafter(thr, np.inf if pos else -np.inf)  # the nearest quotient an excluded column can have
            w_tau, w_far = np.float32(alpha * q_tau + beta), np.float32(alpha * far + beta)
            assert w_tau < w_far, (alpha, beta, tau, thr)
        print("alpha %g beta %g: accepted guess histogram %s (0: none)" % (alpha, beta, accepted.tolist()))
        assert accepted[1] + accepted[2] == len(taus)  # the first or the second guess
    for bad in (np.inf, -np.inf, np.nan):
        assert np.isnan(M.widen(bad, 1.0, 0.0)[0])
    assert np.isnan(M.widen(1.0, 3e38, 3e38)[0])       # t is +inf
    assert np.isnan(M.widen(1.0, 3.4028234e38, 0.0)[0])  # t is FLT_MAX: there is no finite t'


MODEL_CASES = [(nonneg, d, dts) for nonneg in (True, False) for d in (67, 1024)
               for dts in ((np.float32, np.float32), (np.float64, np.float64))]


@pytest.mark.parametrize("case", MODEL_CASES,
                         ids=["%s-d%d-%s" % ("nonneg" if c[0] else "signed", c[1], "f32" if c[2][0] == np.float32 else "f64")
                              for c in MODEL_CASES])
def test_numpy_model_of_the_whole_decision(case):
    nonneg, d, dts = case
    a, b = M.rows(d, dts, nonneg)
    iv = M.intervals(a, b)
    has = ~np.isnan(iv[0])
    no_interval_q = np.flatnonzero(~has.any(axis=1))
    assert no_interval_q.tolist() == [11, 13, 14]   # the 1e200, inf and NaN rows
    if not nonneg and d == 67:
        lone = (~has)[np.setdiff1d(np.arange(M.NQ), no_interval_q)][:, np.setdiff1d(np.arange(M.NG), (401, 403, 404))]
        print("signed d = 67: %d pairs of ordinary rows without an interval, at most %d per query"
              % (lone.sum(), lone.sum(axis=1).max()))
    special = (10, 12) if nonneg else ()           # every word is +-0 there: all columns tie
    ordinary = np.setdiff1d(np.arange(M.NQ), list(no_interval_q) + list(special))
    for alpha, beta in M.AB:
        e = M.K24._canonical(a, b, alpha, beta)
        top = np.stack([M.order(e[i])[:64] for i in range(M.NQ)])
        for k, sample in M.K_SAMPLE:
            thr, guess, cand = M.decide(a, b, alpha, beta, k, sample, iv)
            un = np.isnan(thr)
            assert np.flatnonzero(un).tolist() == no_interval_q.tolist()
            assert set(guess[~un].tolist()) <= {1, 2}
            wrong = 0
            for i in np.flatnonzero(~un):
                ids = np.flatnonzero(cand[i])
                got = ids[M.order(e[i, ids])[:k]]
                wrong += not np.array_equal(got, top[i, :k])
            n = cand[ordinary].sum(axis=1)
            print("a %g b %g k %d sample %d: wrong %d, guesses (1st, 2nd) %s, candidates per ordinary query max %d "
                  "mean %.1f" % (alpha, beta, k, sample, wrong, np.bincount(guess[~un], minlength=3)[1:].tolist(),
                                 n.max(), n.mean()))
            assert wrong == 0
            # a cap, not a measurement: the GPU test's cand_cap = 512 cannot hide an overflow
            assert n.max() <= 480
            if special:
                assert cand[list(special)].all()   # all 520 columns: they overflow 512 and resolve at 1024
