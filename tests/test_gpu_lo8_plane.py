"""The 8-bit residual plane of the level-2 re-score on the GPU (lo8_elem / l16_x, csrc/cmve_internal.h; the writers
pack_f16_lo8 and pack_regs_lane, csrc/eval.hip): small evaluations through RankSession.run, RankBatch.run and
RankBatch.run_chained whose ranks, R@K and rank sums must equal the oracle's exact fp64 counts, and whose level-3
count out[12] must be the same from a batch as from the evaluation run alone.

Rows (every set): near-duplicate groups at 3e-3 noise (decided at level 2, some at its bound's edge) and 3e-4 noise
(inside the level-2 bound: they reach level 3), 16 and 10 rows in the first row tile and a pair in the second, so
tiles hold from 2 to a few hundred band pairs; 40% of the columns scaled by 2^-13, which makes their normalised
elements fp16 subnormals; three rows of norm exactly 1 (two elements 1/2, the rest dyadic) whose other elements sit
exactly on +ulp16/2 and -ulp16/2 of an fp16 value (the byte's clamp at +127, and -128); a NaN row.  A set is used
only if the oracle's own smallest gap between a pair's score and its GT score is at least 6.5e-13 (far above fp64
summation-order noise): the seeds below leave none out, and the test asserts it."""
import math

import numpy as np
import pytest

from oracle import retrieval as R

pytestmark = pytest.mark.gpu

MIN_GAP = 6.5e-13


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no ROCm GPU")
    return torch


def _two_squares(n):
    a = math.isqrt(n)
    while a >= 0 and 2 * a * a >= n:
        b = math.isqrt(n - a * a)
        if a * a + b * b == n:
            return a, b
        a -= 1
    return None


def _four_squares(n):
    """n = a^2 + b^2 + c^2 + d^2 (Lagrange), the largest terms first."""
    a = math.isqrt(n)
    while True:
        r1 = n - a * a
        b = math.isqrt(r1)
        while b >= 0 and r1 - b * b < 4096:
            cd = _two_squares(r1 - b * b)
            if cd:
                return a, b, cd[0], cd[1]
            b -= 1
        a -= 1


def _unit_row(d, k, rng):
    """A row of norm exactly 1 in units of 2^-17: two elements 2^16 (= 1/2), k elements 3073 and k elements 3071
    (fp16 keeps 3072 = 1.5 * 2^11 of them, an even mantissa: the residuals are exactly +ulp16/2 and -ulp16/2), and
    four elements that complete the sum of squares to 2^34.  Every square and partial sum is an integer below 2^35,
    so the fp64 norm is exactly 1 in any summation order and the normalised elements are the elements themselves."""
    e = [1 << 16, 1 << 16] + [3073] * k + [3071] * k
    e += list(_four_squares((1 << 34) - sum(x * x for x in e)))
    assert sum(x * x for x in e) == 1 << 34 and len(e) <= d
    row = np.zeros(d)
    row[rng.permutation(d)[:len(e)]] = np.array(e, dtype=np.float64) * 2.0 ** -17
    row *= rng.choice([-1.0, 1.0], d)
    assert np.sum(row * row) == 1.0
    return row


def _rows(n_q, n_g, d, seed):
    rng = np.random.default_rng(seed)
    n = max(n_q, n_g)
    v = rng.standard_normal((n, d))
    c = v + 0.8 * rng.standard_normal((n, d))
    for lo, k, noise in ((0, 16, 3e-3), (40, 10, 3e-4), (128, 2, 3e-4)):
        v[lo:lo + k] = v[lo] + noise * rng.standard_normal((k, d))
        c[lo:lo + k] = v[lo] + noise * rng.standard_normal((k, d))
    sub = rng.permutation(d)[:(2 * d) // 5]
    v[:, sub] *= 2.0 ** -13
    c[:, sub] *= 2.0 ** -13
    for t, k in enumerate((60, 50, 40)):
        v[100 + t] = _unit_row(d, k, rng)
        c[100 + t] = _unit_row(d, k, rng)
    c[90, 7] = np.nan
    return c[:n_q].copy(), v[:n_g].copy()


def _expected(c, v, rows, cols):
    with np.errstate(invalid="ignore"):
        s = R.exact_scores64(c, v)
    # the oracle's own smallest gap between a pair's score and the row's / column's best GT score
    gap = np.inf
    for sc, gts in ((s, rows), (s.T, cols)):
        for i, l in enumerate(gts):
            g = sc[i, l]
            g = g[np.isfinite(g)]
            if g.size == 0:
                continue
            o = np.delete(sc[i], l)
            o = o[np.isfinite(o)]
            gap = min(gap, np.abs(o - g.max()).min())
    er, ec = R.rank_counts(s, rows), R.rank_counts(s.T, cols)
    return er, ec, gap, s


def _head(er, ec, n_q, n_g):
    # (cmve_eval_ranks' head: #rank <= 1 / 5 / 10 and the rank sum, t2v then v2t)
    return [int((er <= k).sum()) for k in (1, 5, 10)] + [int(er.sum())] + \
           [int((ec <= k).sum()) for k in (1, 5, 10)] + [int(ec.sum())]


def _check(out, er, ec, n_q, n_g):
    h = out.cpu().numpy()
    assert h[9] == 0 and h[11] == 0
    assert np.array_equal(h[16:16 + n_q], er) and np.array_equal(h[16 + n_q:16 + n_q + n_g], ec)
    assert h[:8].tolist() == _head(er, ec, n_q, n_g)
    return int(h[12])


def _run_all(torch, engine, n_q, n_g, d, rows, cols, seeds, expect_paired):
    """Two sets: each alone, both in a batch, and two batches chained; returns the level-3 counts (alone)."""
    sets, exp = [], []
    for seed in seeds:
        c, v = _rows(n_q, n_g, d, seed)
        er, ec, gap, s = _expected(c, v, rows, cols)
        print("seed %d: oracle's smallest score gap %.3e, NaN scores %d" % (seed, gap, int(np.isnan(s).sum())))
        assert gap >= MIN_GAP, "pick another seed: the oracle's own order is not safe for this set"
        sets.append((torch.from_numpy(c).cuda(), torch.from_numpy(v).cuda()))
        exp.append((er, ec))
    mk = lambda: engine.RankSession(n_q, n_g, d, row_gts=rows, col_gts=cols, dtype=torch.float64)
    l3 = []
    for (cq, gv), (er, ec) in zip(sets, exp):
        s1 = mk()
        assert s1.paired == expect_paired
        s1.run(cq, gv)
        torch.cuda.synchronize()
        l3.append(_check(s1.out, er, ec, n_q, n_g))
    print("level-3 pairs (out[12]) per evaluation:", l3)
    sess = [mk() for _ in sets]
    b0 = engine.RankBatch(sess, sets)
    b0.run()
    torch.cuda.synchronize()
    for s_, (er, ec), n3 in zip(sess, exp, l3):
        assert _check(s_.out, er, ec, n_q, n_g) == n3  # the batch sends the same pairs to level 3
    # chained: b0, b1 (the same sets in the other order, its own sessions), b0 again
    sess1 = [mk() for _ in sets]
    b1 = engine.RankBatch(sess1, [(cq.clone(), gv.clone()) for cq, gv in sets[::-1]])
    for s_ in sess + sess1:
        s_.out[:13].fill_(-7)
        s_.out[16:].fill_(-7)
    prev = None
    for b in (b0, b1, b0):
        b.run_chained(prev)
        prev = b
    prev.finish()
    torch.cuda.synchronize()
    for s_, (er, ec), n3 in zip(sess, exp, l3):
        assert _check(s_.out, er, ec, n_q, n_g) == n3
    for s_, (er, ec), n3 in zip(sess1, exp[::-1], l3[::-1]):
        assert _check(s_.out, er, ec, n_q, n_g) == n3
    b0.close()
    b1.close()
    return l3


@pytest.mark.parametrize("d", [256, 768, 1024])
def test_lo8_paired(torch_cuda, d):
    """Paired fp64 sets of n = 130 rows (two row tiles, the second partial) through the specialised prep
    (pack_f16_lo8): d = 256 (one chunk: 4-B residual stores), 768 (an 8-B pair and the odd chunk's 4-B tail) and
    1,024 (the quad transpose, 16-B stores)."""
    from cmve import engine
    n = 130
    rows = [[i] for i in range(n)]
    l3 = _run_all(torch_cuda, engine, n, n, d, rows, rows, (11, 12), True)
    assert max(l3) > 0  # (the 3e-4 groups reach level 3)


@pytest.mark.parametrize("n_q,n_g", [(130, 150), (150, 130)])
def test_lo8_unpaired_multi_gt(torch_cuda, n_q, n_g):
    """Multi-GT lists with n_q != n_g at d = 512: no pairing, so the general register prep writes the plane
    (pack_regs_lane's F16 branch, one dword per lane and chunk)."""
    from cmve import engine
    rng = np.random.default_rng(3)
    rows = [sorted(int(x) for x in rng.choice(n_g, size=1 + i % 3, replace=False)) for i in range(n_q)]
    cols = [[] for _ in range(n_g)]
    for i, l in enumerate(rows):
        for j in l:
            cols[j].append(i)
    _run_all(torch_cuda, engine, n_q, n_g, 512, rows, cols, (21, 22), False)
