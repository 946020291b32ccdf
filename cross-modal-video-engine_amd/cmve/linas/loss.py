"""Mirror of ``LINAS-engine/loss.py`` (TripletLoss + cosine_sim) on libcmve.so, with autograd.

``TripletLoss(margin, measure, max_violation, cost_style, direction).forward(s, im)`` keeps the
reference's signature and semantics (loss.py:83-153): s = caption embeddings, im = video
embeddings, S = sim(im, s) by ``measure`` (loss.py:93-108).  Forward and backward are HIP kernels:
K6 on an fp32 S, which is im . s^T by ``cmve_gemm_f32`` for cosine (loss.py:7-10) and the K10
all-pairs kernel for order / euclidean / l1 / l2 / l1_norm / l2_norm / jaccard (loss.py:13-73),
whose backward is K17 (``cmve_pairwise_bwd``).
"""
from __future__ import annotations

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from .. import engine
from .._lib import lib, check, PW_SQ_L2, PW_L1, PW_ORDER, PW_JACCARD


def _h(t):
    return engine.handle(t.device)


def gemm_f32(a: torch.Tensor, b: torch.Tensor, trans_a=False, trans_b=False, alpha=1.0) -> torch.Tensor:
    """alpha * op(a) @ op(b) in fp32 on the HIP GEMM (row-major, contiguous inputs)."""
    a = a.contiguous().float()
    b = b.contiguous().float()
    M = a.shape[1] if trans_a else a.shape[0]
    K = a.shape[0] if trans_a else a.shape[1]
    N = b.shape[0] if trans_b else b.shape[1]
    out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    check(lib.cmve_gemm_f32(_h(a), int(trans_a), int(trans_b), M, N, K, float(alpha), engine._ptr(a), a.stride(0),
                            engine._ptr(b), b.stride(0), 0.0, engine._ptr(out), out.stride(0)), "cmve_gemm_f32")
    return out


def cosine_sim(im, s):
    """loss.py:7-10: im.mm(s.t())."""
    return gemm_f32(im, s, trans_b=True)


# ---- non-cosine similarities (loss.py:13-73) on the K10 all-pairs kernel: score[i_im, j_s] ----
# forward only: a caller that needs their gradient gets an error, not a silently detached result
# (TripletLoss(measure=...) below is the differentiable user)
def _pw(im, s, metric, alpha, beta):
    if torch.is_grad_enabled() and (im.requires_grad or s.requires_grad):
        raise NotImplementedError("cmve: the non-cosine similarities are forward-only (evaluation); their "
                                  "backward is not on the MI355X path")
    dev = im.device if im.is_cuda else engine.default_device()
    a = engine.to_device(im, dev, torch.float32)
    b = engine.to_device(s, dev, torch.float32)
    return engine.pairwise(a, b, metric, alpha, beta, torch.float32)


def order_sim(im, s):
    """loss.py:13-19: -sqrt(sum max(0, s_j - im_i)^2)."""
    return _pw(im, s, PW_ORDER, -1.0, 0.0)


def euclidean_sim(im, s):
    """loss.py:22-28: -sum (s_j - im_i)^2 (squared, as the reference)."""
    return _pw(im, s, PW_SQ_L2, -1.0, 0.0)


def L1_sim(im, s):
    """loss.py:31-37."""
    return _pw(im, s, PW_L1, -1.0, 0.0)


def L1_sim_norm(im, s):
    """loss.py:39-45: L1 / D - 1."""
    return _pw(im, s, PW_L1, 1.0 / im.shape[1], -1.0)


def L2_sim(im, s):
    """loss.py:48-54: -sum (s_j - im_i)^2."""
    return _pw(im, s, PW_SQ_L2, -1.0, 0.0)


def L2_sim_norm(im, s):
    """loss.py:56-62: sum (s_j - im_i)^2 / D - 1."""
    return _pw(im, s, PW_SQ_L2, 1.0 / im.shape[1], -1.0)


def jaccard_sim(im, s):
    """loss.py:65-73: sum min / sum max."""
    return _pw(im, s, PW_JACCARD, 1.0, 0.0)


_DIRS = {"v2t": 1, "t2v": 2, "all": 3}


def _triplet_fwd(ctx, S, margin, max_violation, dirs, mean_style):
    """K6 forward on an fp32 score matrix; returns (loss, row_arg, col_arg)."""
    B = S.shape[0]
    dev = S.device
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    rv = torch.empty(B, dtype=torch.float32, device=dev)
    ra = torch.empty(B, dtype=torch.int32, device=dev)
    cv = torch.empty(B, dtype=torch.float32, device=dev)
    ca = torch.empty(B, dtype=torch.int32, device=dev)
    check(lib.cmve_triplet_fwd(_h(S), engine._ptr(S), S.stride(0), B, float(margin), int(max_violation), dirs,
                               int(mean_style), engine._ptr(loss), engine._ptr(rv), engine._ptr(ra),
                               engine._ptr(cv), engine._ptr(ca)), "cmve_triplet_fwd")
    ctx.cfg = (float(margin), int(max_violation), dirs, int(mean_style))
    return loss, ra, ca


def _triplet_bwd(ctx, S, ra, ca, g):
    """K6 backward: dL/dS for the upstream gradient g."""
    margin, mv, dirs, mean_style = ctx.cfg
    g = g.reshape(1).float().contiguous()
    dS = torch.empty_like(S)
    check(lib.cmve_triplet_bwd(_h(S), engine._ptr(S), S.stride(0), S.shape[0], margin, mv, dirs, mean_style,
                               engine._ptr(g), engine._ptr(ra), engine._ptr(ca), engine._ptr(dS), dS.stride(0)),
          "cmve_triplet_bwd")
    return dS


class _TripletFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, s, im, margin, max_violation, dirs, mean_style):
        S = cosine_sim(im.detach(), s.detach())
        loss, ra, ca = _triplet_fwd(ctx, S, margin, max_violation, dirs, mean_style)
        ctx.save_for_backward(s.detach(), im.detach(), S, ra, ca)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        s, im, S, ra, ca = ctx.saved_tensors
        dS = _triplet_bwd(ctx, S, ra, ca, g)
        d_im = gemm_f32(dS, s)                 # dL/dim = dS . s
        d_s = gemm_f32(dS, im, trans_a=True)   # dL/ds  = dS^T . im
        return d_s.to(s.dtype), d_im.to(im.dtype), None, None, None, None


class _TripletMeasureFn(torch.autograd.Function):
    """TripletLoss over score = alpha * f(im_i, s_j) + beta for a K10 metric f; backward K6 then K17."""

    @staticmethod
    def forward(ctx, s, im, metric, alpha, beta, margin, max_violation, dirs, mean_style):
        if not (s.is_cuda and im.is_cuda):
            raise ValueError("cmve TripletLoss: the non-cosine measures take device tensors")
        b = s.detach().contiguous().float()
        a = im.detach().contiguous().float()
        S = engine.pairwise(a, b, metric, alpha, beta, torch.float32)
        loss, ra, ca = _triplet_fwd(ctx, S, margin, max_violation, dirs, mean_style)
        ctx.save_for_backward(b, a, S, ra, ca)
        ctx.pw = (metric, float(alpha))
        ctx.dtypes = (s.dtype, im.dtype)
        return loss[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        b, a, S, ra, ca = ctx.saved_tensors
        metric, alpha = ctx.pw
        need_s, need_im = ctx.needs_input_grad[:2]
        d_s = d_im = None
        if need_s or need_im:
            dS = _triplet_bwd(ctx, S, ra, ca, g)
            d_im, d_s = engine.pairwise_bwd(a, b, metric, alpha, dS, need_a=need_im, need_b=need_s)
            d_s = d_s.to(ctx.dtypes[0]) if need_s else None
            d_im = d_im.to(ctx.dtypes[1]) if need_im else None
        return d_s, d_im, None, None, None, None, None, None, None


# loss.py:93-108: measure -> (metric, alpha, beta) of score = alpha * f + beta, alpha None = 1 / D: the
# normalised forms really are +dist / D - 1 in the reference (loss.py:44,61)
_MEASURES = {
    'order': (PW_ORDER, -1.0, 0.0),
    'euclidean': (PW_SQ_L2, -1.0, 0.0),
    'l2': (PW_SQ_L2, -1.0, 0.0),
    'l1': (PW_L1, -1.0, 0.0),
    'l1_norm': (PW_L1, None, -1.0),
    'l2_norm': (PW_SQ_L2, None, -1.0),
    'jaccard': (PW_JACCARD, 1.0, 0.0),
}


class TripletLoss(nn.Module):
    """loss.py:83-153 -- triplet ranking loss under any of the reference's measures; a value that is
    none of them falls through to cosine, as loss.py:107-108."""

    def __init__(self, margin=0, measure=False, max_violation=False, cost_style='sum', direction='all'):
        super().__init__()
        self.measure = _MEASURES.get(measure) if isinstance(measure, str) else None
        self.margin = margin
        self.cost_style = cost_style
        self.direction = direction
        self.max_violation = max_violation

    def forward(self, s, im):
        if self.direction not in _DIRS:
            # the reference falls through to Variable(torch.zeros(1)) for both terms (loss.py:145-148)
            return torch.zeros((), device=s.device)
        if self.measure is not None:
            metric, alpha, beta = self.measure
            alpha = 1.0 / im.shape[1] if alpha is None else alpha
            return _TripletMeasureFn.apply(s, im, metric, alpha, beta, self.margin, self.max_violation,
                                           _DIRS[self.direction], self.cost_style != 'sum')
        return _TripletFn.apply(s, im, self.margin, self.max_violation, _DIRS[self.direction],
                                self.cost_style != 'sum')


NAME_TO_SIM = {'cosine': cosine_sim, 'order': order_sim, 'euclidean': euclidean_sim, 'jaccard': jaccard_sim}


def get_sim(name):
    assert name in NAME_TO_SIM, '%s not supported.' % name
    return NAME_TO_SIM[name]
