"""The step code of the level-2 residual byte on the GPU (csrc/lo8_step.h; the writers pack_f16_lo8 and
pack_regs_lane, csrc/eval.hip; the decode l16_x, csrc/cmve_internal.h): small evaluations through RankSession.run,
RankBatch.run and RankBatch.run_chained whose ranks, R@K and rank sums must equal the oracle's exact fp64 counts, and
whose level-3 count out[12] must be the same from a batch as from the evaluation run alone.

Rows: tests/test_gpu_lo8_plane.py's construction -- near-duplicate groups at 3e-3 noise (decided at level 2) and 3e-4
noise (inside the level-2 bound: they reach level 3), 40% of the columns scaled by 2^-13 (fp16 subnormals after
normalising), a NaN row -- and three rows of norm exactly 1 that hold the step code's edge cases as they are (the
normalised elements are the elements themselves): 2^-5 (1 - 2^-13) and its likes just below a power of two,
+-(2^-14 - 2^-26), fp16-subnormal elements with a residual, exact zeros, and elements exactly on +ulp16/2 and
-ulp16/2 of an fp16 value, of both signs.  Each of them is the query row and the gallery row of its index (a GT
score of exactly 1) and has a twin gallery row with two elements exchanged, whose score is 2^-32 below 1: the
pair is inside the level-2 bound, so level 2 decodes these elements on both sides and level 3 decides the pair.
A set is used only if the oracle's own smallest gap between a pair's score and its GT score is at least 6.5e-13;
the seeds below leave none out, and the test asserts it."""
import math

import numpy as np
import pytest

from oracle import retrieval as R

pytestmark = pytest.mark.gpu

MIN_GAP = 6.5e-13
UNIT = 2.0 ** -26  # the edge rows' elements are integers in this unit; their squares sum to 2^52
SPECIAL, TWIN = 60, 63  # rows SPECIAL + t (t = 0, 1, 2) and their twins TWIN + t


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
        while b >= 0 and r1 - b * b < (1 << 16):
            cd = _two_squares(r1 - b * b)
            if cd:
                return a, b, cd[0], cd[1]
            b -= 1
        a -= 1


def _edge_row(d, k, rng):
    """A row of norm exactly 1 (integers in units of 2^-26 whose squares sum to 2^52: every partial sum is an integer
    below 2^53, so the fp64 norm is 1 in any summation order) and its twin.  Elements: two of 1/2; k each of
    (2^13 - 1) 2^-18 = 2^-5 (1 - 2^-13), (2^13 - 1) 2^-21 and 2^-9 (1 - 2^-14) (below a power of two, inside the
    half-width cell); k of 2^-14 - 2^-26 and k of 2^-14 - 2^-25 (the edge of that cell); fp16 subnormals 37 2^-24 +
    2^-26 and 2^-24 - 2^-26; 3073 2^-17 and 3071 2^-17 (fp16 keeps 3072: the residuals are exactly +-ulp16/2); four
    elements that complete the sum of squares.  Signs alternate within every kind.  The twin exchanges one 3073 2^-17
    with one 3071 2^-17 of the same sign: its score with the row is 1 - (2 * 2^-17)^2 = 1 - 2^-32."""
    kinds = [(1 << 13) - 1 << 8, (1 << 13) - 1 << 5, (1 << 14) - 1 << 3, (1 << 12) - 1, (1 << 12) - 2, 37 * 4 + 1, 3,
             3073 << 9, 3071 << 9]
    e, sg = [1 << 25, 1 << 25], [1, 1]
    for v in kinds:
        e += [v] * k
        sg += [1 if i % 2 == 0 else -1 for i in range(k)]
    rest = _four_squares((1 << 52) - sum(x * x for x in e))
    e += list(rest)
    sg += [1, -1, 1, -1]
    assert sum(x * x for x in e) == 1 << 52 and len(e) <= d // 2  # (at least half of the row is exact zeros)
    pos = rng.permutation(d)[:len(e)]
    row = np.zeros(d)
    row[pos] = np.array(e, dtype=np.float64) * np.array(sg, dtype=np.float64) * UNIT
    assert np.sum(row * row) == 1.0
    i3, i1 = 2 + 7 * k, 2 + 8 * k  # the first 3073 and the first 3071, both positive
    twin = row.copy()
    twin[pos[i3]], twin[pos[i1]] = row[pos[i1]], row[pos[i3]]
    assert np.sum(twin * twin) == 1.0 and 1.0 - np.dot(row, twin) == 2.0 ** -32
    return row, twin


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
    for t, k in enumerate((12, 9, 6)):
        row, twin = _edge_row(d, k, rng)
        v[SPECIAL + t] = row
        c[SPECIAL + t] = row
        v[TWIN + t] = twin
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
    return R.rank_counts(s, rows), R.rank_counts(s.T, cols), gap, s


_CACHE = {}


def _case(n_q, n_g, d, rows, cols, seeds):
    """The sets and the oracle's answers of a shape (CPU), computed once."""
    key = (n_q, n_g, d, seeds)
    if key not in _CACHE:
        out = []
        for seed in seeds:
            c, v = _rows(n_q, n_g, d, seed)
            er, ec, gap, s = _expected(c, v, rows, cols)
            out.append((c, v, er, ec, gap))
        _CACHE[key] = out
    return _CACHE[key]


def _head(er, ec):
    # (cmve_eval_ranks' head: #rank <= 1 / 5 / 10 and the rank sum, t2v then v2t)
    return [int((er <= k).sum()) for k in (1, 5, 10)] + [int(er.sum())] + \
           [int((ec <= k).sum()) for k in (1, 5, 10)] + [int(ec.sum())]


def _check(out, er, ec, n_q, n_g):
    h = out.cpu().numpy()
    assert h[9] == 0 and h[11] == 0
    assert np.array_equal(h[16:16 + n_q], er) and np.array_equal(h[16 + n_q:16 + n_q + n_g], ec)
    assert h[:8].tolist() == _head(er, ec)
    return int(h[12])


def _run_all(torch, engine, n_q, n_g, d, rows, cols, seeds, expect_paired):
    """Two sets: each alone, both in a batch, and two batches chained; returns the level-3 counts (alone)."""
    sets, exp = [], []
    for c, v, er, ec, gap in _case(n_q, n_g, d, rows, cols, seeds):
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


PAIRED = (160, 160, 1024, (31, 32))
UNPAIRED = (96, 160, 512, (41, 42))


def _paired_gts():
    rows = [[i] for i in range(PAIRED[0])]
    return rows, rows


def _unpaired_gts():
    n_q, n_g = UNPAIRED[:2]
    rng = np.random.default_rng(3)
    rows = [sorted(int(x) for x in rng.choice(n_g, size=1 + i % 3, replace=False)) for i in range(n_q)]
    for t in range(3):  # (the edge rows keep their own gallery row as the GT: score exactly 1)
        rows[SPECIAL + t] = [SPECIAL + t]
    cols = [[] for _ in range(n_g)]
    for i, l in enumerate(rows):
        for j in l:
            cols[j].append(i)
    return rows, cols


def test_step_paired(torch_cuda):
    """Paired fp64 sets of n = 160 rows (two row tiles, the second partial) at d = 1,024 through the specialised prep
    (pack_f16_lo8: the quad transpose, 16-B stores)."""
    from cmve import engine
    n_q, n_g, d, seeds = PAIRED
    rows, cols = _paired_gts()
    l3 = _run_all(torch_cuda, engine, n_q, n_g, d, rows, cols, seeds, True)
    assert min(l3) > 0  # (the 3e-4 groups and the edge rows' twins reach level 3)


def test_step_unpaired_multi_gt(torch_cuda):
    """Multi-GT lists with n_q = 96, n_g = 160 at d = 512: no pairing, so the general register prep writes the plane
    (pack_regs_lane's F16 branch, one dword per lane and chunk)."""
    from cmve import engine
    n_q, n_g, d, seeds = UNPAIRED
    rows, cols = _unpaired_gts()
    l3 = _run_all(torch_cuda, engine, n_q, n_g, d, rows, cols, seeds, False)
    assert min(l3) > 0
