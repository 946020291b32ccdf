"""Golden vectors for retrieval under the non-cosine evaluation measures (K18), produced by running the
REFERENCE's own functions on small seeded inputs:

  LINAS-engine/evaluation.py:17-36      cal_error        euclidean / l1 / l2 / l1_norm / l2_norm / jaccard
  LINAS-engine/util/metrics.py:106-157  get_gt, eval_q2m (both orientations)
  LINAS-engine/util/metrics.py:61-102   t2v_map, v2t_map
  LINAS-engine/validate.py:15-54        cal_perf
  LINAS-engine/inference.py:79          np.argsort(errors[i])[:10]

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_measures_retrieval.py <reference root>
Writes tests/golden/measures_retrieval.npz: the inputs, the id lists (unicode arrays: the loader uses
allow_pickle=False), the ranks, the metric tuples and the top-10 ids -- not the error matrices.

Shape: 141 videos, 150 captions (nine videos own two), D = 67: three row tiles, two column tiles and a K-slab
tail of the 64 x 128 x 32 kernel tile.  Signed inputs for the cdist measures, non-negative for jaccard.

Conditioning: ranks and top-10 ids are integers, so the fixture is only meaningful if rounding cannot move
them.  With E = the largest deviation of the reference's result from an fp64 restatement, the script searches
seeds until, for every measure, every |e_GT - e_other| in a GT's row and column and every gap among each row's
11 smallest errors is at least 8 E -- and ASSERTS it for the seed it writes.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

MEASURES = ["euclidean", "l1", "l2", "l1_norm", "l2_norm", "jaccard"]
N_V, N_C, D, TOP = 141, 150, 67, 10
MARGIN = 8.0


def inputs(seed):
    rng = np.random.default_rng(seed)
    vid = rng.standard_normal((N_V, D))
    owner = np.concatenate([np.arange(N_V), np.arange(N_C - N_V)])  # the first nine videos own two captions
    owner = owner[rng.permutation(N_C)]
    cap = vid[owner] + 1.5 * rng.standard_normal((N_C, D))
    counts = {}
    caption_ids = []
    for o in owner:
        counts[o] = counts.get(o, 0) + 1
        caption_ids.append("video%d#enc#%d" % (o, counts[o] - 1))
    video_ids = ["video%d" % j for j in range(N_V)]
    return dict(vid=vid, cap=cap, vid_p=np.abs(vid).astype(np.float32), cap_p=np.abs(cap).astype(np.float32),
                video_ids=np.array(video_ids), caption_ids=np.array(caption_ids))


def restate64(cap, vid, measure):
    """The measure in fp64 numpy (for E only: nothing of it is stored)."""
    c, v = np.asarray(cap, np.float64), np.asarray(vid, np.float64)
    diff = c[:, None, :] - v[None, :, :]
    if measure in ("euclidean", "l2"):
        return np.sqrt((diff * diff).sum(-1))
    if measure == "l1":
        return np.abs(diff).sum(-1)
    if measure == "l1_norm":
        return -np.abs(diff).sum(-1) / v.shape[1] - 1
    if measure == "l2_norm":
        return -np.sqrt((diff * diff).sum(-1)) / v.shape[1] - 1
    return -np.minimum(c[:, None, :], v[None, :, :]).sum(-1) / np.maximum(c[:, None, :], v[None, :, :]).sum(-1)


def min_gaps(e, t2v_gt, v2t_gt):
    """(least |e_GT - e_other| over every GT's row and column, least gap among each row's 11 smallest)"""
    e = np.asarray(e, np.float64)
    g = np.inf
    for i in range(e.shape[0]):
        for j in t2v_gt[i]:
            row = np.abs(e[i] - e[i, j])
            row[j] = np.inf
            col = np.abs(e[:, j] - e[i, j])
            col[i] = np.inf
            g = min(g, row.min(), col.min())
    top = np.sort(e, axis=1)[:, :TOP + 1]
    return g, np.diff(top, axis=1).min()


def ranks_of(e, gts, n_q):
    """eval_q2m's loop (metrics.py:137-147) on the reference's matrix, keeping the ranks it only aggregates"""
    n_m = e.shape[1]
    out = np.zeros(n_q, np.int32)
    for i in range(n_q):
        order = np.argsort(e[i])
        rank = n_m + 1
        for k in gts[i]:
            rank = min(rank, int(np.where(order == k)[0][0]) + 1)
        out[i] = rank
    return out


def run(ref, x):
    evaluation, metrics, validate = ref
    video_ids, caption_ids = list(x["video_ids"]), list(x["caption_ids"])
    v2t_gt, t2v_gt = metrics.get_gt(video_ids, caption_ids)
    out, ok = {}, True
    for m in MEASURES:
        c, v = (x["cap_p"], x["vid_p"]) if m == "jaccard" else (x["cap"], x["vid"])
        e = evaluation.cal_error(v, c, m)
        e = np.asarray(e.numpy() if hasattr(e, "numpy") else e)
        E = float(np.abs(e.astype(np.float64) - restate64(c, v, m)).max())
        g_gt, g_top = min_gaps(e, t2v_gt, v2t_gt)
        need = MARGIN * E
        good = g_gt >= need and g_top >= need and g_gt > 0 and g_top > 0
        print("  %-9s E %.3g  GT gap %.3g  top-11 gap %.3g  %s" % (m, E, g_gt, g_top, "ok" if good else "TOO CLOSE"))
        ok = ok and good
        if not good:
            continue
        t2v_q2m = tuple(metrics.eval_q2m(e, t2v_gt))
        v2t_q2m = tuple(metrics.eval_q2m(e.T, v2t_gt))
        t2v_ranks, v2t_ranks = ranks_of(e, t2v_gt, N_C), ranks_of(e.T, v2t_gt, N_V)
        assert np.isclose(t2v_ranks.mean(), t2v_q2m[4]) and np.isclose(v2t_ranks.mean(), v2t_q2m[4])
        out["t2v_ranks_" + m], out["v2t_ranks_" + m] = t2v_ranks, v2t_ranks
        out["t2v_q2m_" + m], out["v2t_q2m_" + m] = np.array(t2v_q2m, np.float64), np.array(v2t_q2m, np.float64)
        out["t2v_map_" + m] = np.float64(metrics.t2v_map(e, t2v_gt))
        out["v2t_map_" + m] = np.float64(metrics.v2t_map(e, v2t_gt))
        out["cal_perf_" + m] = np.array(validate.cal_perf(e, v2t_gt, t2v_gt), np.float64)  # [v2t, t2v] x 6
        out["top10_" + m] = np.stack([np.argsort(e[i])[:TOP] for i in range(N_C)]).astype(np.int64)
    return out, ok


def main(ref_root):
    sys.path.insert(0, os.path.join(ref_root, "LINAS-engine"))
    import evaluation  # noqa
    import util.metrics as metrics  # noqa
    import validate  # noqa
    for seed in range(64):
        print("seed", seed)
        x = inputs(seed)
        out, ok = run((evaluation, metrics, validate), x)
        if ok:
            break
    assert ok, "no seed of 0..63 met the gap condition for every measure"
    out.update(x)
    out["seed"] = np.int64(seed)
    path = os.path.join(HERE, "measures_retrieval.npz")
    np.savez_compressed(path, **out)
    print("seed %d -> %s (%d bytes)" % (seed, path, os.path.getsize(path)))
    assert os.path.getsize(path) < 512 * 1024


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: make_golden_measures_retrieval.py <reference root>")
    main(sys.argv[1])
