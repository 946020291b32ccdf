"""K23 / K25 on the GPU: the SAD filters' DECISIONS, not only their results.

Equal ids and words do not show that a pass kernel still decides what it decided: the fallback repairs a filter that
excludes less.  ``tests/golden/sad_topk_counters.json`` holds the four counters {excluded, candidates, rescored,
unresolved} of ``engine.l1_topk`` and ``engine.jaccard_topk`` as recorded before the two pass kernels became one body
(csrc/sad_topk.h); the same integers must come out now.

The shape: 130 queries (two query tiles, the second ragged) over 1100 gallery rows (a ragged last gallery tile; with
the default 1024-row sample launch B sees 76 columns launch A never bounded), d = 70 (below one K tile's pad), k = 10,
both signs of alpha, float32 and float64 rows.  With the default cand_cap = 2048 > n_g no list can overflow, so the
counters do not depend on the order of the atomics."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NQ, NG, D, K = 130, 1100, 70, 10
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sad_topk_counters.json")
COUNTERS = ("excluded", "candidates", "rescored", "unresolved")
ROUTES = ("l1", "jaccard")
ALPHAS = (1.0, -1.0)
DTYPES = ("float32", "float64")


def case_key(route, alpha, dtype):
    return "%s/alpha%+d/%s" % (route, int(alpha), dtype)


def rows(route, dtype):
    """(queries, gallery) from numpy.random.RandomState on the host; non-negative for jaccard."""
    rs = np.random.RandomState(2500 + ROUTES.index(route))
    q, g = rs.standard_normal((NQ, D)), rs.standard_normal((NG, D))
    if route == "jaccard":
        q, g = np.abs(q), np.abs(g)
    return q.astype(dtype), g.astype(dtype)


def run_case(route, alpha, dtype):
    """((idx, err) of the filter's own entry, its four counters, (idx, err) of ``filter=False``), all on the host."""
    import torch
    from cmve import _lib, engine
    q, g = rows(route, dtype)
    qd, gd = engine.to_device(q), engine.to_device(g)
    grid = engine.l1_grid(gd, engine.l1_grid(qd))
    cls, fn, metric, words = {"l1": (engine.L1Set, engine.l1_topk, _lib.PW_L1, torch.float64),
                              "jaccard": (engine.JaccardSet, engine.jaccard_topk, _lib.PW_JACCARD, torch.float32)}[route]
    idx, err, st = fn(cls(qd, grid=grid), cls(gd, grid=grid), alpha, 0.0, K)
    ref = engine.pairwise_topk(qd, gd, metric, alpha, 0.0, words, K, filter=False)
    return (idx.cpu().numpy(), err.cpu().numpy()), {c: int(st[c]) for c in COUNTERS}, ref


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("alpha", ALPHAS, ids=["pos", "neg"])
@pytest.mark.parametrize("route", ROUTES)
def test_the_filter_decides_what_it_decided(recorded, route, alpha, dtype):
    got, st, ref = run_case(route, alpha, dtype)
    print(case_key(route, alpha, dtype), st)
    assert st == recorded[case_key(route, alpha, dtype)]
    assert st["unresolved"] == 0
    assert st["excluded"] + st["candidates"] == NQ * NG and st["rescored"] == st["candidates"]
    assert np.array_equal(got[0], ref[0])
    assert np.array_equal(np.ascontiguousarray(got[1]).view(np.int64), np.ascontiguousarray(ref[1]).view(np.int64))
