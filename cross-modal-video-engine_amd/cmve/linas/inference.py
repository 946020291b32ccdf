"""Drop-in mirror of the ``LINAS-engine/inference.py`` gallery scorer + CLI.

Reference hot loop (inference.py:76-82):
    errors = evaluation.cal_error(video_embs, cap_emb, options.measure)   # re-normalises the gallery
    inds = np.argsort(errors[0])[:opt.topK]                               # full O(N log N) sort
    print([video_ids[i] for i in inds])
Here the gallery is normalised and packed into HBM ONCE (``GalleryScorer``) and each
query batch is scored by ``cmve_topk``: a gallery-streaming fp16 MFMA GEMV for up to 32
queries (the GEMM beyond), a histogram bound on the k-th score, and an exact fp64 re-score
of the error band: same ids, same order (score desc; ties by index) as the reference's
argsort on tie-free scores.

CLI (same flags and flow as inference.py:37-82; run from the directory that holds the
reference's ``student_support_set_8/`` and ``dataset/``):
  python -m cmve.linas.inference --input "a man ..." --topK 10 --gpu 0
  1. checkpoint ``student_support_set_8/model_best.pth.tar`` -> get_model(opt.model)(opt),
     load_state_dict(checkpoint['model'], 'test'), val_start (weights-only load, cmve.linas.checkpoint)
  2. gallery: ``video_data.pt`` if it exists (weights-only), else BigFile features of
     dataset/<test collection>/FeatureData/<visual_feature> + video2frames.txt -> encode_vid(
     model.embed_vis_distill, ...) on the GPU, written back to ``video_data.pt``
  3. vocabularies dataset/<train collection>/TextData/vocabulary/{bow,rnn}/<vocab>.pkl (restricted
     unpickler) -> process_cap(--input) -> embed_txt_distill
  4. exact top-K of the errors on HBM (GalleryScorer; under the checkpoint's opt.measure: cosine on the packed
     gallery, a cdist / jaccard measure through the matrix-free top-k of K18), printed as the id list
``--gpu`` is exported as HIP_VISIBLE_DEVICES before the GPU is touched (the reference's
CUDA_VISIBLE_DEVICES, inference.py:47); its default is '0' rather than the reference's '5', which
would hide every GPU of a box with fewer than six.  ``--query-emb`` (a .npy caption embedding)
and ``--gallery`` (an .npz with video_embs / video_ids) bypass steps 3 and 1-2 respectively; ``--measure``
overrides the checkpoint's opt.measure (with both bypasses no checkpoint is read: cosine unless given).
"""
from __future__ import annotations

import argparse
import functools
import os
import sys

import numpy as np

from .. import engine
from .._lib import SIM_F16


class GalleryScorer:
    """A video gallery resident in HBM, normalised once (LINAS l2norm, no eps).

    ``measure``: 'cosine', or a cdist / jaccard measure of evaluation.py:22-35 -- the gallery then stays resident
    UNNORMALISED in the measure's input dtype (fp64 for the cdist branches, fp32 for jaccard) and every query
    batch is served by the matrix-free exact top-k of K18 (``engine.pairwise_topk``): the ids of
    ``np.argsort(cal_error(video_embs, cap_emb, measure)[i], kind='stable')[:topK]``.

    Under 'euclidean', 'l2' and 'l2_norm' the gallery is also packed once for the MFMA-filtered top-k of K20
    (``engine.pairwise_topk(filter=)``: the same ids, the same words): its fp16 and bf16 unit planes stay resident
    beside the fp64 rows, 2 x 2 bytes per element -- half the fp64 rows' bytes again, plus 20 bytes per row -- and
    the rows themselves are not copied.  ``filter``: None -- the filter from ``engine.L2_TOPK_FILTER_MIN_GALLERY``
    gallery rows or ``engine.L2_TOPK_FILTER_MIN_PAIRS`` pairs per call (``engine.l2_topk_auto``); True / False force it / the fp64 route of K18 (False
    also skips the pack).  The pack's bf16 plane is not read by K20 (the pack kernel always writes it): half of the
    extra bytes serve the cosine kernels' layout only.  A call that falls back to the fp64 route as a whole turns the
    automatic filter off for this scorer.

    Under 'l1' and 'l1_norm' the SAD-filtered top-k of K23 serves (``engine.pairwise_topk(filter="l1")``: the same ids,
    the same words): ``filter="l1"`` forces it, None takes it when ``engine.l1_topk_auto(n_q, n_g, packed=True)``
    says it pays, False is the fp64 route of K18 and skips the pack; ``filter=True`` speaks for the Euclidean
    measures alone and is ignored here (no pack).  The gallery is then packed once as an ``engine.L1Set`` on its own
    grid -- uint16 codes, 2 bytes per element beside the fp64 rows, plus 8 bytes per row; the rows are not copied --
    and each call packs its queries on that grid.  One workspace stays resident, sized for the route taken, and a
    call handed back whole turns the automatic filter off, as above.

    Under 'jaccard' the SAD-filtered top-k of K25 serves in the same way (``engine.pairwise_topk(filter="jaccard")``:
    float32 words, the same ids): ``filter="jaccard"`` forces it, None takes it when
    ``engine.jaccard_topk_auto(n_q, n_g, packed=True)`` says it pays, False skips the pack, True is ignored.  The
    gallery is packed once as an ``engine.JaccardSet`` over the gallery rows themselves (the codes and 24 bytes per
    row; no second copy).  ``filter="jaccard"`` under any other measure is a ValueError."""

    def __init__(self, video_embs, video_ids=None, with_lo=True, measure='cosine', filter=None):
        self.measure = measure
        self.filter = filter
        self.video_ids = list(video_ids) if video_ids is not None else None
        self._ws = None
        self._packed = None
        self._filter_off = False  # latched by a call the filter handed back whole
        if isinstance(filter, str) and filter == "jaccard" and measure != 'jaccard':
            raise ValueError(f'GalleryScorer: filter="jaccard" speaks for the jaccard measure, not {measure!r}')
        if measure != 'cosine':
            from .evaluation import measure_rows
            self.gallery = measure_rows(video_embs, measure)
            if measure in ('euclidean', 'l2', 'l2_norm') and filter is not False and self.gallery.shape[0]:
                self._packed = engine.RowSet(self.gallery, eps=0.0, with_lo=False, device=self.gallery.device)
                self.gallery = self._packed.raw  # the pack keeps the rows it was given: no second copy
            # l1 / l1_norm (K23): packed when forced, or when the auto rule could take some call over this gallery
            # (never while its constants are None); filter=True speaks for the Euclidean measures alone
            # jaccard (K25): the same, as a JaccardSet under filter="jaccard" and its own rule
            n_g = self.gallery.shape[0]
            sad = self._sad_route()
            if sad is not None and n_g and 1 <= self.gallery.shape[1] <= engine.L1_D_MAX and (
                    (isinstance(filter, str) and filter == sad)
                    or (filter is None and engine.sad_topk_auto(sad, 1 << 30, n_g, packed=True))):
                self._packed = engine.sad_set(sad, self.gallery)
                self.gallery = self._packed.raw
            return
        emb = video_embs if hasattr(video_embs, "data_ptr") else np.asarray(video_embs)
        self.gallery = engine.RowSet(emb, eps=0.0, with_lo=with_lo)
        self._ws = None
        self._q = {}    # resident query sets by (rows, dim, dtype): re-packed in place per call
        self._out = {}  # resident top-k outputs by (rows, k)

    def _sad_route(self):
        """The SAD-filtered top-k that serves this measure: its ``filter`` word (``engine.sad_route_of``), or None."""
        from .evaluation import measure_spec
        metric, _, _, _, sc_dt = measure_spec(self.measure, 1)
        return engine.sad_route_of(metric, sc_dt)

    def topk_indices(self, cap_embs, topK=10):
        """[N_q, topK] gallery indices, best first (== np.argsort(cal_error(...)[i])[:topK])."""
        import torch
        if self.measure != 'cosine':
            return self._measure_topk(cap_embs, topK)
        if not torch.is_tensor(cap_embs):
            cap_embs = np.atleast_2d(np.asarray(cap_embs))
        elif cap_embs.dim() == 1:
            cap_embs = cap_embs[None, :]
        key = (tuple(cap_embs.shape), str(cap_embs.dtype))
        q = self._q.get(key)
        if q is None:
            q = self._q[key] = engine.RowSet(cap_embs, eps=0.0, with_lo=self.gallery.has_lo,
                                             device=self.gallery.device)
        else:
            q.repack(cap_embs)
        k = min(topK, self.gallery.n)
        need = engine.topk_workspace_floats(q, self.gallery, k)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.float32, device=self.gallery.device)
        out = self._out.get((q.n, k))
        if out is None:
            dev = self.gallery.device
            out = self._out[(q.n, k)] = (torch.empty((max(q.n, 1), k), dtype=torch.int32, device=dev),
                                         torch.empty((max(q.n, 1), k), dtype=torch.float64, device=dev),
                                         torch.zeros(1, dtype=torch.int32, device=dev))
        idx, _ = engine.topk(q, self.gallery, topK, mode=SIM_F16, scores_ws=self._ws, out=out)
        return idx

    def _measure_topk(self, cap_embs, topK):
        import torch
        from .evaluation import measure_rows, measure_spec
        g = self.gallery
        q = measure_rows(cap_embs, self.measure, g.device)
        metric, alpha, beta, _, sc_dt = measure_spec(self.measure, g.shape[1])
        k = min(int(topK), g.shape[0])
        # the route this call will take, as engine.pairwise_topk decides it; a gallery whose calls fell back to the
        # fp64 route as a whole (rows clustered far from the origin) is not asked again under filter=None
        flt = False
        sad = self._sad_route() if isinstance(self._packed, engine.L1Set) else None
        if self._packed is not None and q.shape[0] and 1 <= k <= engine.L2_TOPK_CAND_MAX:
            forced = (isinstance(self.filter, str) and self.filter == sad) if sad else self.filter is True
            auto = functools.partial(engine.sad_topk_auto, sad) if sad else engine.l2_topk_auto
            flt = forced or (self.filter is None and not self._filter_off
                             and auto(q.shape[0], g.shape[0], packed=True))
        # ONE workspace stays resident between calls, sized for that route only and grown when a call needs more
        need = 0
        if flt and sad:
            # (the queries are packed on the gallery's grid)
            need = engine.sad_topk_workspace(sad, q.shape[0], g.shape[0], k)
        elif flt:
            q = engine.RowSet(q, eps=0.0, with_lo=False, device=g.device)
            need = engine.l2_topk_workspace(q, self._packed, k)
        elif 1 <= k <= engine._lib.TOPK_MAX:
            need = engine.pairwise_topk_workspace(q.shape[0], g.shape[0], k, metric)[1]
        if need and (self._ws is None or self._ws.numel() < need):
            self._ws = torch.empty(need, dtype=torch.uint8, device=g.device)
        idx, _, st = engine.pairwise_topk(q, self._packed if flt else g, metric, alpha, beta, sc_dt, k, ws=self._ws,
                                          filter=(sad if sad else True) if flt else False, return_stats=True)
        if st is not None and st["fallback"]:
            self._filter_off = True
        return idx

    def topk_ids(self, cap_emb, topK=10):
        inds = self.topk_indices(cap_emb, topK)[0]
        return [self.video_ids[i] for i in inds]


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--input', default='a man and a woman is talking.', type=str, help='input sentence')
    p.add_argument('--topK', default=10, type=int, help='return top-k videos')
    p.add_argument('--gpu', default='0', type=str, help='gpu device')
    p.add_argument('--checkpoint', default='student_support_set_8/model_best.pth.tar', type=str,
                   help='LINAS model_best.pth.tar (inference.py:49), loaded weights-only')
    p.add_argument('--rootpath', default='dataset/', type=str, help='dataset root (inference.py:55)')
    p.add_argument('--video-cache', default='video_data.pt', type=str,
                   help='gallery cache {video_embs, video_ids} (inference.py:57-67)')
    p.add_argument('--gallery', default=None, type=str,
                   help='.npz with video_embs [N,D] and video_ids instead of the cache / BigFile')
    p.add_argument('--query-emb', default=None, type=str,
                   help='.npy caption embedding [1,D] instead of encoding --input')
    p.add_argument('--measure', default=None, type=str,
                   help="similarity measure (default: the checkpoint's opt.measure, cosine without a checkpoint)")
    p.add_argument('--rnn-vocab', default=None, type=str, help='rnn vocabulary (default: the checkpoint opt path)')
    p.add_argument('--bow-vocab', default=None, type=str, help='bow vocabulary (default: the checkpoint opt path)')
    return p.parse_args(argv)


def _gallery(opt, model, options):
    """inference.py:57-67: the video_data.pt cache, else encode_vid over the BigFile features."""
    from . import bigfile as B
    if opt.gallery is not None:
        data = np.load(opt.gallery, allow_pickle=False)
        return data['video_embs'], [str(v) for v in data['video_ids']]
    if os.path.exists(opt.video_cache):
        return B.load_video_cache(opt.video_cache)
    if model is None:
        sys.exit("cmve inference: no gallery (give --gallery, a %s cache, or the checkpoint)" % opt.video_cache)
    from .evaluation import encode_vid
    feat_dir = os.path.join(opt.rootpath, options.collections_pathname['test'], 'FeatureData', options.visual_feature)
    visual_feats = B.BigFile(feat_dir)
    video2frames = B.read_dict(os.path.join(feat_dir, 'video2frames.txt'))
    loader = B.VideoBatchLoader(visual_feats, video2frames, video_ids=list(video2frames.keys()),
                                batch_size=options.batch_size, device=model.device)
    video_embs, video_ids = encode_vid(model.embed_vis_distill, loader)
    B.save_video_cache(opt.video_cache, video_embs, video_ids)
    return video_embs, video_ids


def main(argv=None):
    opt = parse_args(argv)
    os.environ["HIP_VISIBLE_DEVICES"] = opt.gpu
    model = options = None
    if opt.query_emb is None or (opt.gallery is None and not os.path.exists(opt.video_cache)):
        from .checkpoint import load_checkpoint, get_model
        checkpoint = load_checkpoint(opt.checkpoint)
        options = checkpoint['opt']
        model = get_model(options.model)(options)
        model.load_state_dict(checkpoint['model'], 'test')
        model.Eiters = checkpoint['Eiters']
        model.val_start()
    video_embs, video_ids = _gallery(opt, model, options)
    if opt.query_emb is not None:
        cap_emb = np.load(opt.query_emb, allow_pickle=False).astype(np.float32)
    else:
        from . import text as T
        voc = os.path.join(opt.rootpath, options.collections_pathname['train'], 'TextData', 'vocabulary')
        bow_vocab = T.load_vocab(opt.bow_vocab or os.path.join(voc, 'bow', options.vocab + '.pkl'))
        vocab = T.load_vocab(opt.rnn_vocab or os.path.join(voc, 'rnn', options.vocab + '.pkl'))
        bow2vec = T.get_text_encoder('bow')(bow_vocab)
        cap_emb = model.embed_txt_distill(T.process_cap(opt.input, vocab, bow2vec)).cpu().numpy()
    measure = opt.measure or (getattr(options, 'measure', 'cosine') if options is not None else 'cosine')
    results = _retrieve(video_embs, video_ids, cap_emb, measure, opt.topK)
    print(results)
    return results


def _retrieve(video_embs, video_ids, cap_emb, measure, topK):
    """inference.py:78-80 under any measure: cosine on the packed gallery, a cdist / jaccard measure on the
    unnormalised resident gallery through the matrix-free top-k (K18) -- no errors[1, N] row on the host."""
    if measure == 'cosine':
        return GalleryScorer(video_embs, [str(v) for v in video_ids]).topk_ids(cap_emb, topK)
    return GalleryScorer(video_embs, list(video_ids), measure=measure).topk_ids(cap_emb, topK)


if __name__ == '__main__':
    main()
