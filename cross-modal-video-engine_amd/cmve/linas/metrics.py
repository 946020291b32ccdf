"""Drop-in mirror of ``LINAS-engine/util/metrics.py`` (retrieval metrics) on libcmve.so.

  get_gt(video_ids, caption_ids)          metrics.py:106-120  (host; bucketed, same output)
  eval_q2m(scores, q2m_gts)               metrics.py:124-157  -> (r1, r5, r10, medr, meanr)
  t2v_map(c2i, t2v_gts)                   metrics.py:61-79
  v2t_map(c2i, v2t_gts)                   metrics.py:83-102
The per-row argsort of the reference is replaced by rank counting on the GPU:
position of item k in np.argsort(row) == #{j : e_j < e_k} on tie-free rows.
``scores`` that are an ``ErrorMatrix`` from cmve.linas.evaluation.cal_error are ranked
by the fused exact path (fp64 decisions, no matrix re-read).  Errors of a non-cosine measure that carry
their device-resident rows (``ErrorMatrix._cmve_pw``) are ranked matrix-free by K18: the same words the
matrix path gives, without the upload.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import engine
from .._lib import lib, check, CMVE_F32, CMVE_F64  # noqa: F401
from .evaluation import ErrorMatrix


def get_gt(video_ids, caption_ids):
    buckets = {}
    for i, cap_id in enumerate(caption_ids):
        buckets.setdefault(cap_id.split('#', 1)[0], []).append(i)
    v2t_gt = [list(buckets.get(vid_id, [])) for vid_id in video_ids]
    t2v_gt = {}
    for i, t_gts in enumerate(v2t_gt):
        for t_gt in t_gts:
            t2v_gt.setdefault(t_gt, [])
            t2v_gt[t_gt].append(i)
    return v2t_gt, t2v_gt


def _lists(gts, n):
    if isinstance(gts, dict):
        return [gts[i] for i in range(n)]  # KeyError on a missing caption, like metrics.py:142
    return [gts[i] for i in range(n)]


def metrics_from_ranks(gt_ranks):
    gt_ranks = np.asarray(gt_ranks)
    n_q = gt_ranks.shape[0]
    r1 = 100.0 * len(np.where(gt_ranks <= 1)[0]) / n_q
    r5 = 100.0 * len(np.where(gt_ranks <= 5)[0]) / n_q
    r10 = 100.0 * len(np.where(gt_ranks <= 10)[0]) / n_q
    medr = np.median(gt_ranks)
    meanr = gt_ranks.mean()
    return (r1, r5, r10, medr, meanr)


def _fused_sets(scores):
    meta = getattr(scores, '_cmve', None) if isinstance(scores, ErrorMatrix) else None
    return meta


def _measure_sets(errors):
    """(captions, videos, measure) of errors that carry their non-cosine rows, else None."""
    return getattr(errors, '_cmve_pw', None) if isinstance(errors, ErrorMatrix) else None


def measure_eval(caps, vids, measure, row_lists=None, col_lists=None, filter=None):
    """((t2v positions, t2v ranks), (v2t positions, v2t ranks)) under a non-cosine measure from ONE
    cmve_pairwise_positions call over the device-resident rows; a direction without lists gives (None, None).
    ``filter``: None -- euclidean / l2 / l2_norm take the MFMA filter (K19) from ``engine.L2_FILTER_MIN_PAIRS``
    pairs on, the same words; True / False force it on (those three measures only) / off.  ``"l1"`` forces the
    integer SAD filter of l1 / l1_norm (K22: the same words; those two measures only), which None takes from
    ``engine.L1_FILTER_MIN_PAIRS`` pairs on when that is set.  ``"jaccard"`` forces the same SAD filter under jaccard
    (K24: float32 words, the same words; that measure only), which None takes from
    ``engine.JACCARD_FILTER_MIN_PAIRS`` pairs on when that is set."""
    from .evaluation import measure_spec
    metric, alpha, beta, _, sc_dt = measure_spec(measure, vids.shape[1])
    return engine.pairwise_gt_eval(caps, vids, metric, alpha, beta, sc_dt, row_lists, col_lists, filter)


def cosine_sets(errors, filter=None):
    """(captions RowSet, videos RowSet) of errors = -cos that carry their packed sets, else None.  ``filter="cosine"``
    asks for the one-pass route (K26), which speaks for those errors alone: anything else is a ValueError."""
    meta = _fused_sets(errors)
    if meta is not None and meta[2] < 0:
        return meta[0], meta[1]
    if filter == "cosine":
        raise ValueError('filter="cosine" needs errors that carry their packed cosine sets (cal_error under cosine), '
                         "or measure='cosine'")
    return None


def cosine_one_pass(filter, n_c, n_v, *lists) -> bool:
    """Whether a cosine evaluation takes the one-pass route (K26, ``engine.cos_gt_eval``): ``filter="cosine"`` forces
    it; None takes it where today's route would run a second or third rank pass -- some list holds more than one item
    -- and n_c * n_v reaches ``engine.COS_FILTER_MIN_PAIRS`` (never while that is None)."""
    if filter == "cosine":
        return True
    min_pairs = engine.COS_FILTER_MIN_PAIRS  # (read at call time)
    return (filter is None and min_pairs is not None and n_c * n_v >= min_pairs
            and any(len(l) > 1 for ls in lists for l in ls))


def maps_from_positions(t2v_pos, v2t_pos):
    """(t2v_map, v2t_map) of metrics.py:61-102 from every GT item's position: the t2v AP scores the FIRST GT video
    of each caption alone (1 / its position), the v2t AP all GT captions of each video."""
    t2v = float(np.mean([ap_from_positions(p[:1]) for p in t2v_pos]))
    v2t = float(np.mean([ap_from_positions(p) for p in v2t_pos]))
    return t2v, v2t


def ap_flat(offs, pos, first_only=False):
    """``ap_from_positions`` of every list of a CSR side at once (offs int64 [n + 1], 1-based positions in list
    order), the same floats: lists of one length are sorted and summed as the rows of one matrix.  ``first_only``:
    each list's FIRST item alone (the t2v AP of metrics.py:61-79)."""
    offs, pos = np.asarray(offs, np.int64), np.asarray(pos)
    lens = np.diff(offs)
    out = np.zeros(lens.size, np.float64)
    if first_only:
        has = lens > 0
        out[has] = 1.0 / pos[offs[:-1][has]].astype(np.float64)
        return out
    for m in np.unique(lens):
        if m == 0:
            continue
        which = np.flatnonzero(lens == m)
        p = np.sort(pos[offs[which][:, None] + np.arange(m)[None, :]].astype(np.float64), axis=1)
        out[which] = np.sum(np.arange(1, m + 1) / p, axis=1) / m
    return out


def maps_from_flat(t2v, v2t):
    """``maps_from_positions`` from ``engine.cos_gt_eval_flat``'s sides."""
    return float(np.mean(ap_flat(t2v[0], t2v[1], first_only=True))), float(np.mean(ap_flat(v2t[0], v2t[1])))


def gt_ranks(scores, q2m_gts):
    """1-based best-GT rank per query (metrics.py:137-147)."""
    n_q, n_m = scores.shape
    lists = _lists(q2m_gts, n_q)
    meta = _fused_sets(scores)
    if meta is not None:
        caps, vids, sign = meta
        if sign < 0:  # errors = -cos: rank by cos descending
            r, _, _ = engine.gt_rank_counts(caps, vids, row_gts=lists)
            return r.astype(np.int32)
    pw = _measure_sets(scores)
    if pw is not None:
        return measure_eval(*pw, row_lists=lists)[0][1].astype(np.int32)
    return engine.rank_from_matrix(scores, lists).astype(np.int32)


def eval_q2m(scores, q2m_gts):
    return metrics_from_ranks(gt_ranks(scores, q2m_gts))


def gt_positions(errors, lists, transposed=False):
    """1-based positions of every GT item of every query in the ascending sort of its row
    (columns when transposed); returns a list of int arrays aligned with ``lists``."""
    device = engine.default_device()
    e = engine.to_device(errors, device)
    n_rows, n_cols = e.shape
    off, idx = engine.csr(lists, device)
    pos = torch.zeros(max(int(off[-1].item()), 1), dtype=torch.int32, device=device)
    check(lib.cmve_gt_positions_from_matrix(engine.handle(device), engine._ptr(e), engine._dtype_code(e), n_rows,
                                            n_cols, e.stride(0), 1 if transposed else 0, engine._ptr(off),
                                            engine._ptr(idx), engine._ptr(pos)), "cmve_gt_positions_from_matrix")
    p = pos.cpu().numpy().astype(np.int64) + 1
    offs = off.cpu().numpy()
    return [p[offs[i]:offs[i + 1]] for i in range(len(lists))]


def ap_from_positions(positions):
    """APScorer on a ranked list (LINAS-engine/basic/metric.py:31-46) from the positions of its
    relevant items: the m-th relevant item at position p_m contributes m / p_m."""
    p = np.sort(np.asarray(positions, np.float64))
    if p.size == 0:
        return 0.0
    return float(np.sum(np.arange(1, p.size + 1) / p) / p.size)


def t2v_map(c2i, t2v_gts, filter=None):
    """metrics.py:61-79: AP of the FIRST GT video of each caption (= 1 / its position).  ``filter="cosine"``: the
    positions from the one-pass count (K26) -- errors = -cos with their packed sets only."""
    n_q = c2i.shape[0]
    firsts = [[_lists(t2v_gts, n_q)[i][0]] for i in range(n_q)]
    cos = cosine_sets(c2i, filter)
    if cos is not None:
        caps, vids = cos
        if cosine_one_pass(filter, n_q, c2i.shape[1]):
            offs, pos, _ = engine.cos_gt_eval_flat(caps, vids, row_lists=firsts)[0]
            return float(np.mean(ap_flat(offs, pos)))
        r, _, _ = engine.gt_rank_counts(caps, vids, row_gts=firsts)
        return float(np.mean(1.0 / r))
    pw = _measure_sets(c2i)
    if pw is not None:
        pos = measure_eval(*pw, row_lists=firsts)[0][0]
        return float(np.mean([ap_from_positions(p) for p in pos]))
    pos = gt_positions(c2i, firsts)
    return float(np.mean([ap_from_positions(p) for p in pos]))


def v2t_map(c2i, v2t_gts, filter=None):
    """metrics.py:83-102: AP over all GT captions of each video (columns of c2i).  ``filter``: ``t2v_map``'s; None
    also takes the one-pass count where today's route expands the captions (``cosine_one_pass``)."""
    n_v = c2i.shape[1]
    lists = _lists(v2t_gts, n_v)
    cos = cosine_sets(c2i, filter)
    if cos is not None:
        caps, vids = cos
        if cosine_one_pass(filter, c2i.shape[0], n_v, lists):
            offs, pos, _ = engine.cos_gt_eval_flat(caps, vids, col_lists=lists)[1]
            return float(np.mean(ap_flat(offs, pos)))
        if all(len(l) <= 1 for l in lists):
            _, c, _ = engine.gt_rank_counts(caps, vids, col_gts=lists)
            return float(np.mean([1.0 / c[j] if lists[j] else 0.0 for j in range(n_v)]))
        pos = engine.gt_positions_fused(vids, caps, lists)
        return float(np.mean([ap_from_positions(p) for p in pos]))
    pw = _measure_sets(c2i)
    if pw is not None:
        pos = measure_eval(*pw, col_lists=lists)[1][0]
        return float(np.mean([ap_from_positions(p) for p in pos]))
    pos = gt_positions(c2i, lists, transposed=True)
    return float(np.mean([ap_from_positions(p) for p in pos]))
