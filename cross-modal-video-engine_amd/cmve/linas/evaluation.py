"""Drop-in mirror of ``LINAS-engine/evaluation.py`` backed by libcmve.so.

Same names, argument meaning and return types as the reference:
  l2norm(X)                                  evaluation.py:10-14
  cal_error(videos, captions, measure)       evaluation.py:17-36  -> ndarray[N_c, N_v] (= -cos; the
                                             euclidean / l1 / l2 / l1_norm / l2_norm / jaccard branches
                                             on the K10 all-pairs kernel)
  cal_error_batch(..., batch_size)           evaluation.py:41-72
  cal_simi(captions, videos, measure)        evaluation.py:75-84  -> ndarray[N_c, N_v] (= +cos)
  encode_vid / encode_text                   evaluation.py:88-171
The cosine matrix is computed on the GPU by the split-bf16 MFMA kernel (|err| ~1e-6,
within the north-star's 1e-4).  The returned array is an ``ErrorMatrix``: a plain
ndarray that also remembers the device-resident packed embeddings, so that
``cmve.linas.validate.cal_perf`` / ``cmve.linas.metrics.eval_q2m`` rank it with the
fused exact path (fp64-exact ranks, matrix never re-read) instead of the matrix path.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import engine
from .._lib import SIM_BF16X3, PW_L1, PW_L2, PW_JACCARD


class ErrorMatrix(np.ndarray):
    """ndarray of errors that carries the packed (captions, videos) sets it was made from."""

    _cmve = None  # (captions RowSet, videos RowSet, sign) -- dropped by any view/transform
    # non-cosine measures: (captions, videos, measure) -- the device-resident rows in the measure's input dtype; the
    # metrics rank them matrix-free (K18).  Separate from _cmve, whose sign logic is cosine's; dropped likewise.
    _cmve_pw = None

    def __array_finalize__(self, obj):
        self._cmve = None
        self._cmve_pw = None


def _as_error_matrix(arr: np.ndarray, caps, vids, sign):
    out = arr.view(ErrorMatrix)
    out._cmve = (caps, vids, sign)
    return out


def _result_dtype(a, b):
    dt = np.result_type(np.asarray(a).dtype, np.asarray(b).dtype)
    return torch.float64 if dt == np.float64 else torch.float32


def l2norm(X):
    """Row L2 normalisation on the GPU, no epsilon (zero row -> NaN), dtype preserved."""
    X = np.asarray(X)
    rs = engine.RowSet(X, eps=0.0, with_lo=False)
    dt = torch.float64 if X.dtype == np.float64 else torch.float32
    return rs.normalized(dt).cpu().numpy()


def _cosine(videos, captions, sign):
    caps = engine.RowSet(np.asarray(captions), eps=0.0, with_lo=True)
    vids = engine.RowSet(np.asarray(videos), eps=0.0, with_lo=True)
    out = engine.sim_store(caps, vids, alpha=float(sign), beta=0.0, mode=SIM_BF16X3,
                           out_dtype=_result_dtype(captions, videos))
    return _as_error_matrix(out.cpu().numpy(), caps, vids, sign)


# evaluation.py:22-35 / 56-71: measure -> (metric, alpha(D), beta, input dtype, score dtype).  The scipy cdist
# branches work in fp64 whatever the input dtype; jaccard goes through torch.Tensor(...) (fp32 inputs) and returns
# -jaccard_sim in fp32.  The ONE table of the matrix path (K10) and the matrix-free paths (K18).
MEASURES = {
    'euclidean': (PW_L2, lambda D: 1.0, 0.0, torch.float64, torch.float64),
    'l2': (PW_L2, lambda D: 1.0, 0.0, torch.float64, torch.float64),
    'l1': (PW_L1, lambda D: 1.0, 0.0, torch.float64, torch.float64),
    'l1_norm': (PW_L1, lambda D: -1.0 / D, -1.0, torch.float64, torch.float64),
    'l2_norm': (PW_L2, lambda D: -1.0 / D, -1.0, torch.float64, torch.float64),
    'jaccard': (PW_JACCARD, lambda D: -1.0, 0.0, torch.float32, torch.float32),
}


def measure_spec(measure, D):
    """(metric, alpha, beta, input dtype, score dtype) of a non-cosine evaluation measure at dimension D."""
    if measure not in MEASURES:
        raise ValueError(f"cmve.cal_error: unknown measure {measure!r}")
    metric, alpha, beta, in_dt, sc_dt = MEASURES[measure]
    return metric, alpha(D), beta, in_dt, sc_dt


def measure_rows(x, measure, device=None):
    """Rows resident on the device in the measure's input dtype (fp64 for the cdist branches, fp32 for jaccard)."""
    in_dt = measure_spec(measure, 1)[3]
    if torch.is_tensor(x):
        return engine.to_device(x if x.dim() == 2 else x[None, :], device, in_dt)
    return engine.to_device(np.atleast_2d(np.asarray(x)), device, in_dt)


def _as_measure_matrix(arr: np.ndarray, caps, vids, measure):
    out = arr.view(ErrorMatrix)
    out._cmve_pw = (caps, vids, measure)
    return out


def _measure(videos, captions, measure):
    c, v = measure_rows(captions, measure), measure_rows(videos, measure)
    metric, alpha, beta, _, sc_dt = measure_spec(measure, v.shape[1])
    out = engine.pairwise(c, v, metric, alpha, beta, sc_dt).cpu()
    if measure == 'jaccard':  # a torch tensor, as the reference returns: no attribute to carry the rows
        return out
    return _as_measure_matrix(out.numpy(), c, v, measure)


def cal_error(videos, captions, measure='cosine'):
    """errors[N_c, N_v] (evaluation.py:17-36): -cos, or the cdist / jaccard branches.

    Under the five cdist measures the ndarray remembers the device-resident rows and the measure, so that
    ``cal_perf`` / ``eval_q2m`` / ``t2v_map`` / ``v2t_map`` rank them matrix-free (K18) instead of uploading the
    matrix again.  ``cal_error(..., 'jaccard')`` returns a torch tensor, as the reference does: it cannot carry
    that attribute and stays on the matrix path (``cal_error_batch`` returns the ndarray that does)."""
    if measure == 'cosine':
        return _cosine(videos, captions, -1)
    return _measure(videos, captions, measure)


def cal_error_batch(videos, captions, measure='cosine', batch_size=2000):
    """evaluation.py:41-72 -- the caption batching only bounds the reference's jaccard memory;
    the all-pairs kernel never materialises the [N_c, N_v, D] broadcast, so one call covers it
    (the jaccard result is a float32 ndarray here, as np.append makes it in the reference)."""
    if measure != 'jaccard':
        return cal_error(videos, captions, measure)
    c, v = measure_rows(captions, measure), measure_rows(videos, measure)
    metric, alpha, beta, _, sc_dt = measure_spec(measure, v.shape[1])
    return _as_measure_matrix(engine.pairwise(c, v, metric, alpha, beta, sc_dt).cpu().numpy(), c, v, measure)


def cal_simi(captions, videos, measure='cosine'):
    """+cos(caption_i, video_j) or +jaccard as a float32 torch tensor (evaluation.py:75-84)."""
    if measure == 'cosine':
        return _cosine(videos, captions, +1)
    if measure == 'jaccard':
        dev = engine.default_device()
        c = engine.to_device(np.asarray(captions), dev, torch.float32)
        v = engine.to_device(np.asarray(videos), dev, torch.float32)
        return engine.pairwise(c, v, PW_JACCARD, 1.0, 0.0, torch.float32).cpu()
    raise ValueError(f"cmve.cal_simi: measure {measure!r} has no branch in the reference (evaluation.py:75-84)")


def _encode(encoder_call, data_loader, return_ids):
    embeddings = None
    ids = [''] * len(data_loader.dataset)
    for batch in data_loader:
        *datas, idxs, data_ids = batch
        emb = encoder_call(*datas)
        if embeddings is None:
            embeddings = np.zeros((len(data_loader.dataset), emb.size(1)))  # float64, as evaluation.py:102
        embeddings[list(idxs)] = emb.detach().cpu().numpy()
        for j, idx in enumerate(idxs):
            ids[idx] = data_ids[j]
    return (embeddings, ids) if return_ids else embeddings


def encode_vid(encoder, data_loader, return_ids=True):
    """evaluation.py:88-116: loader yields (datas, idxs, ids); float64 host buffer."""
    return _encode(lambda datas: encoder(datas), data_loader, return_ids)


def encode_text(encoder, data_loader, style, return_ids=True):
    """evaluation.py:119-171: 'distill_from_best_model' -> (datas, idxs, ids);
    'GT' -> (datas, support_datas, idxs, ids)."""
    if style == 'distill_from_best_model':
        return _encode(lambda datas: encoder(datas), data_loader, return_ids)
    if style == 'GT':
        return _encode(lambda datas, support: encoder(datas, support), data_loader, return_ids)
    raise ValueError(f"encode_text: unknown style {style!r}")
