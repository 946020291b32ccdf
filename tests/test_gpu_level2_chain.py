"""The level-2 re-score of the rank GEMM (fp16 + bf16 residual planes, sim.hip "level 2:") on small evaluations whose
tiles hold fewer listed pairs than the block has waves, a partial second tile, rows of one to four sixteen-element
lane groups, and rows scaled so that 36 to 41% of the normalised elements are fp16 subnormals (where h + lo, formed in
fp32, is at its thinnest).  Ranks == the oracle's exact counts (R.exact_scores64 + R.rank_counts) in both directions,
for one evaluation and for a batch of two."""

import functools

import numpy as np
import pytest

from oracle import retrieval as R

pytestmark = pytest.mark.gpu

# n, d, k, noise, seed, colscale, paired
CASES = [
    (130, 1024, 2, 3e-3, 11, True, True),
    (130, 1024, 3, 3e-3, 12, True, True),
    (130, 1024, 5, 3e-3, 7, True, True),
    (200, 1024, 37, 3e-3, 3, True, True),
    (200, 1024, 37, 3e-3, 3, False, True),
    (200, 256, 37, 3e-3, 4, True, True),
    (333, 512, 50, 3e-3, 5, True, False),
    (200, 768, 37, 3e-4, 6, True, False),
]
# out[12] (level-3 pairs, 13 here) of the batch == out[12] of the single run: the order of a pair's level-2 sum is
# the pair's alone, not the kernel geometry's
L3_EQUAL_CASE = CASES[2]
# The k = 37 and k = 50 cases above put k (k - 1) > 1,024 band pairs into one tile, past the LDS list: those tiles
# take the per-wave fp64 re-score, not level 2.  These keep every tile listed (20 or 380 pairs, smallest gaps 1e-9 to
# 3e-8) so that level 2 itself runs on rows of one, two and three lane groups.
CASES += [
    (130, 256, 5, 3e-3, 21, True, True),
    (130, 512, 5, 3e-3, 22, True, True),
    (130, 768, 5, 3e-3, 23, True, True),
    (200, 768, 20, 3e-3, 24, True, False),
    (130, 256, 20, 3e-3, 25, True, True),
    (200, 512, 20, 3e-3, 26, True, True),
]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def _inputs(n, d, k, noise, seed, colscale, paired):
    """_dense_inputs of test_gpu_retrieval.py (k near-duplicate captions / videos) with a per-column scale: the
    upper half of the columns is scaled by 2^-8 .. 2^-14."""
    rng = np.random.default_rng(seed)
    sc = np.ones(d)
    if colscale:
        sc[d // 2:] = 2.0 ** -rng.integers(8, 15, size=d - d // 2)
    v = rng.standard_normal((n, d)) * sc
    v[:k] = v[0] + noise * rng.standard_normal((k, d)) * sc
    c = v + 0.8 * rng.standard_normal((n, d)) * sc
    c[:k] = v[0] + noise * rng.standard_normal((k, d)) * sc
    t2v = [[i] for i in range(n)]
    v2t = [[j] for j in range(n)] if paired else [[j, (j + 1) % n] if j % 3 == 0 else [j] for j in range(n)]
    return c, v, t2v, v2t


def _min_gap(s, gts):
    """the smallest distance between a row's GT score (the best of its GTs) and any other score of the row"""
    gap = np.inf
    for i, g in enumerate(gts):
        best = g[int(np.argmax(s[i, g]))]
        dist = np.abs(s[i] - s[i, best])
        dist[best] = np.inf
        gap = min(gap, float(dist.min()))
    return gap


@functools.lru_cache(maxsize=None)
def _case(case):
    """inputs, oracle ranks and the smallest score gap of a case (computed once, shared, left unchanged)"""
    c, v, t2v, v2t = _inputs(*case)
    s = R.exact_scores64(c, v)
    gap = min(_min_gap(s, t2v), _min_gap(s.T, v2t))
    er, ec = R.rank_counts(s, t2v), R.rank_counts(s.T, v2t)
    for x in (c, v, er, ec):
        x.setflags(write=False)
    return c, v, t2v, v2t, er, ec, gap


@pytest.mark.parametrize("case", CASES, ids=lambda c: "n%d_d%d_k%d_s%d_%s_%s" % (
    c[0], c[1], c[2], c[4], "scaled" if c[5] else "plain", "paired" if c[6] else "multigt"))
def test_level2_chain_ranks(torch_cuda, case):
    import torch
    from cmve import engine
    c, v, t2v, v2t, er, ec, gap = _case(case)
    n, d = c.shape
    print("smallest gap between a score and its row's / column's GT score: %.3g" % gap)
    assert gap >= 1e-12, "the input is at fault: the oracle's order is not safely the exact one"
    ct, vt = torch.from_numpy(c.copy()).cuda(), torch.from_numpy(v.copy()).cuda()
    sess = engine.RankSession(n, n, d, row_gts=t2v, col_gts=v2t, dtype=torch.float64)
    assert sess.paired == case[6]
    r, cc = sess.run(ct, vt)
    single = sess.out.cpu().numpy().copy()
    assert single[9] == 0
    assert np.array_equal(r, er) and np.array_equal(cc, ec)
    sb = [engine.RankSession(n, n, d, row_gts=t2v, col_gts=v2t, dtype=torch.float64) for _ in range(2)]
    b = engine.RankBatch(sb, [(ct, vt), (ct.clone(), vt.clone())])
    b.run()
    torch.cuda.synchronize()
    outs = [x.out.cpu().numpy().copy() for x in sb]
    b.close()
    for h in outs:
        assert h[9] == 0
        assert np.array_equal(h[16:16 + n], er) and np.array_equal(h[16 + n:], ec)
    print("level-3 pairs: single %d, batch %d / %d; band pairs %d" % (single[12], outs[0][12], outs[1][12], single[8]))
    if case == L3_EQUAL_CASE:
        assert outs[0][12] == single[12] and outs[1][12] == single[12]
