"""Drop-in mirror of ``LINAS-engine/validate.py`` ``cal_perf`` (+ ``norm_score``) on libcmve.so.

``cal_perf(t2v_all_errors, v2t_gt, t2v_gt, tb_logger=None, model=None)`` returns the
reference's two 6-tuples (validate.py:15-54).  When ``t2v_all_errors`` comes from
``cmve.linas.evaluation.cal_error`` both directions are ranked in ONE fused GEMM pass
(t2v = row counts, v2t = column counts) with fp64-exact decisions.
"""
from __future__ import annotations

import logging

import numpy as np

from .. import engine
from . import metrics
from .evaluation import ErrorMatrix


def norm_score(t2v_all_errors):
    """validate.py:7-11 (host elementwise)."""
    s = -t2v_all_errors
    s = s - np.min(s)
    s = s / np.max(s)
    return -s


def _log(tag, r1, r5, r10, medr, meanr, m):
    logging.info(" * %s:" % tag)
    logging.info(" * r_1_5_10, medr, meanr: {}".format([round(r1, 1), round(r5, 1), round(r10, 1), round(medr, 1),
                                                         round(meanr, 1)]))
    logging.info(" * recall sum: {}".format(round(r1 + r5 + r10, 1)))
    logging.info(" * mAP: {}".format(round(m, 4)))
    logging.info(" * " + '-' * 10)


def _cosine_one_pass(caps, vids, t2v_lists, v2t_lists):
    """Both directions' ranks and both mAPs under cosine from ONE ``engine.cos_gt_eval_flat`` call (K26)."""
    t2v, v2t = engine.cos_gt_eval_flat(caps, vids, t2v_lists, v2t_lists)
    return (t2v[2], v2t[2]) + metrics.maps_from_flat(t2v, v2t)


def cal_perf(t2v_all_errors, v2t_gt, t2v_gt, tb_logger=None, model=None, filter=None):
    """``filter="cosine"`` (errors = -cos with their packed sets only, else ValueError): every rank and mAP position
    from one MFMA pass over the pairs (K26); None takes it where today's route would run a second or third pass and
    ``engine.COS_FILTER_MIN_PAIRS`` is set and reached."""
    n_c, n_v = t2v_all_errors.shape
    t2v_lists = metrics._lists(t2v_gt, n_c)
    v2t_lists = metrics._lists(v2t_gt, n_v)
    cos = metrics.cosine_sets(t2v_all_errors, filter)
    if cos is not None and metrics.cosine_one_pass(filter, n_c, n_v, t2v_lists, v2t_lists):
        t2v_ranks, v2t_ranks, t2v_map_score, v2t_map_score = _cosine_one_pass(*cos, t2v_lists, v2t_lists)
    elif cos is not None:
        caps, vids = cos
        t2v_ranks, v2t_ranks, _ = engine.gt_rank_counts(caps, vids, row_gts=t2v_lists, col_gts=v2t_lists)
        if all(len(l) == 1 for l in t2v_lists):
            t2v_map_score = float(np.mean(1.0 / t2v_ranks))
        else:
            t2v_map_score = metrics.t2v_map(t2v_all_errors, t2v_gt)
        if all(len(l) <= 1 for l in v2t_lists):
            v2t_map_score = float(np.mean([1.0 / v2t_ranks[j] if v2t_lists[j] else 0.0 for j in range(n_v)]))
        else:
            v2t_map_score = metrics.v2t_map(t2v_all_errors, v2t_gt)
    elif metrics._measure_sets(t2v_all_errors) is not None:
        # a non-cosine measure with its rows on the device: both directions' ranks and every mAP position from one
        # matrix-free pass (K18)
        caps, vids, measure = metrics._measure_sets(t2v_all_errors)
        (t2v_pos, t2v_ranks), (v2t_pos, v2t_ranks) = metrics.measure_eval(caps, vids, measure, t2v_lists, v2t_lists)
        t2v_map_score, v2t_map_score = metrics.maps_from_positions(t2v_pos, v2t_pos)
    else:
        t2v_ranks = engine.rank_from_matrix(t2v_all_errors, t2v_lists)
        v2t_ranks = engine.rank_from_matrix(t2v_all_errors, v2t_lists, transposed=True)
        t2v_map_score = metrics.t2v_map(t2v_all_errors, t2v_gt)
        v2t_map_score = metrics.v2t_map(t2v_all_errors, v2t_gt)

    (t2v_r1, t2v_r5, t2v_r10, t2v_medr, t2v_meanr) = metrics.metrics_from_ranks(t2v_ranks.astype(np.int32))
    (v2t_r1, v2t_r5, v2t_r10, v2t_medr, v2t_meanr) = metrics.metrics_from_ranks(v2t_ranks.astype(np.int32))
    _log("Text to Video", t2v_r1, t2v_r5, t2v_r10, t2v_medr, t2v_meanr, t2v_map_score)
    _log("Video to text", v2t_r1, v2t_r5, v2t_r10, v2t_medr, v2t_meanr, v2t_map_score)
    if tb_logger is not None:
        step = getattr(model, 'Eiters', 0)
        for k, v in (('v2t_r1', v2t_r1), ('v2t_r5', v2t_r5), ('v2t_r10', v2t_r10), ('v2t_medr', v2t_medr),
                     ('v2t_meanr', v2t_meanr), ('t2v_r1', t2v_r1), ('t2v_r5', t2v_r5), ('t2v_r10', t2v_r10),
                     ('t2v_medr', t2v_medr), ('t2v_meanr', t2v_meanr), ('v2t_map', v2t_map_score),
                     ('t2v_map', t2v_map_score)):
            tb_logger.log_value(k, v, step=step)
    return ((v2t_r1, v2t_r5, v2t_r10, v2t_medr, v2t_meanr, v2t_map_score),
            (t2v_r1, t2v_r5, t2v_r10, t2v_medr, t2v_meanr, t2v_map_score))


def cal_perf_embeddings(video_embs, cap_embs, video_ids, caption_ids, measure='cosine', filter=None):
    """tester.py:133-139 in one call: get_gt -> fused two-direction rank -> cal_perf tuples,
    without materialising the N_c x N_v error matrix on host.  A non-cosine ``measure`` (the cdist branches and
    jaccard of evaluation.py:22-35) never forms the matrix at all, on the device or the host (K18); ``filter`` is
    ``metrics.measure_eval``'s (auto: the Euclidean measures count at the MFMA rate on large sets, K19;
    ``filter="l1"``: l1 / l1_norm through the integer SAD filter, K22; ``filter="jaccard"``: jaccard through the same
    filter, K24).  Under cosine ``filter="cosine"`` takes every rank and mAP position from ONE MFMA pass (K26,
    ``cal_perf``'s rule for None); with any other measure it is a ValueError."""
    v2t_gt, t2v_gt = metrics.get_gt(video_ids, caption_ids)
    if measure != 'cosine':
        if filter == "cosine":
            raise ValueError(f'filter="cosine" needs measure=\'cosine\', got {measure!r}')
        from .evaluation import measure_rows
        caps, vids = measure_rows(cap_embs, measure), measure_rows(video_embs, measure)
        t2v_lists = metrics._lists(t2v_gt, caps.shape[0])
        (t2v_pos, t2v_ranks), (v2t_pos, v2t_ranks) = metrics.measure_eval(caps, vids, measure, t2v_lists, v2t_gt, filter)
        t2v_map, v2t_map = metrics.maps_from_positions(t2v_pos, v2t_pos)
        return (metrics.metrics_from_ranks(v2t_ranks.astype(np.int32)) + (v2t_map,),
                metrics.metrics_from_ranks(t2v_ranks.astype(np.int32)) + (t2v_map,))
    caps = engine.RowSet(np.asarray(cap_embs), eps=0.0, with_lo=False)
    vids = engine.RowSet(np.asarray(video_embs), eps=0.0, with_lo=False)
    n_c, n_v = caps.n, vids.n
    t2v_lists = metrics._lists(t2v_gt, n_c)
    if metrics.cosine_one_pass(filter, n_c, n_v, t2v_lists, v2t_gt):
        t2v_ranks, v2t_ranks, t2v_map, v2t_map = _cosine_one_pass(caps, vids, t2v_lists, v2t_gt)
        return (metrics.metrics_from_ranks(v2t_ranks) + (v2t_map,), metrics.metrics_from_ranks(t2v_ranks) + (t2v_map,))
    t2v_ranks, v2t_ranks, _ = engine.gt_rank_counts(caps, vids, row_gts=t2v_lists, col_gts=v2t_gt)
    t2v = metrics.metrics_from_ranks(t2v_ranks)
    v2t = metrics.metrics_from_ranks(v2t_ranks)
    firsts = [[l[0]] for l in t2v_lists]
    if all(len(l) == 1 for l in t2v_lists):
        t2v_map = float(np.mean(1.0 / t2v_ranks))
    else:
        r, _, _ = engine.gt_rank_counts(caps, vids, row_gts=firsts)
        t2v_map = float(np.mean(1.0 / r))
    if all(len(l) <= 1 for l in v2t_gt):
        v2t_map = float(np.mean([1.0 / v2t_ranks[j] if v2t_gt[j] else 0.0 for j in range(n_v)]))
    else:
        pos = engine.gt_positions_fused(vids, caps, v2t_gt)
        v2t_map = float(np.mean([metrics.ap_from_positions(p) for p in pos]))
    return v2t + (v2t_map,), t2v + (t2v_map,)
