"""TripletLoss under the non-cosine measures: forward + backward time and peak memory per measure on the GPU
(K10 + K6 + K17), against torch eager on the same GPU running the reference's method -- the broadcast
B x B x D formulas of LINAS-engine/loss.py:13-73 written out below, under torch autograd -- the only
baseline there is for this path.  Prints one JSON line.

Shapes: B = 128 and 256 at D = 1536 (the reference trainer's defaults are B = 128, D = 1536,
trainer.py:67-68,95); max_violation on and off, direction all, margin 0.2, cost_style sum.
Times are device events around REPS steps after WARMUP steps; peak memory is what one step allocates on top
of its inputs, its two gradients included (torch.cuda.max_memory_allocated after a reset, read with no
gradient of an earlier step resident).  "parts" times the K10 forward and the K17
backward (dense dS, both sides) alone, per shape and measure."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "cross-modal-video-engine_amd"), ROOT):
    sys.path.insert(0, p)
import torch  # noqa: E402

from cmve import engine, _lib  # noqa: E402
from cmve.linas.loss import TripletLoss  # noqa: E402

# measure -> (K10 metric, alpha, beta) of score = alpha * f + beta (loss.py:13-73; alpha None = 1 / D), for "parts"
MEASURE_TABLE = {"order": (_lib.PW_ORDER, -1.0, 0.0), "euclidean": (_lib.PW_SQ_L2, -1.0, 0.0),
                 "jaccard": (_lib.PW_JACCARD, 1.0, 0.0), "l1": (_lib.PW_L1, -1.0, 0.0),
                 "l2": (_lib.PW_SQ_L2, -1.0, 0.0), "l1_norm": (_lib.PW_L1, None, -1.0),
                 "l2_norm": (_lib.PW_SQ_L2, None, -1.0)}
MEASURES = list(MEASURE_TABLE)
MARGIN = 0.2


def eager_sim(measure, im, s):
    """score[i, j] of video i and caption j, by expansion to B x B x D as the reference does."""
    d = s.unsqueeze(0) - im.unsqueeze(1)  # [i, j, :] = s_j - im_i
    if measure == "order":
        return -d.clamp(min=0).pow(2).sum(2).sqrt()
    if measure in ("euclidean", "l2"):
        return -d.pow(2).sum(2)
    if measure == "l1":
        return -d.abs().sum(2)
    if measure == "l1_norm":
        return d.abs().sum(2) / im.size(1) - 1
    if measure == "l2_norm":
        return d.pow(2).sum(2) / im.size(1) - 1
    a, b = im.unsqueeze(1).expand(-1, s.size(0), -1), s.unsqueeze(0).expand(im.size(0), -1, -1)
    return torch.min(a, b).sum(-1) / torch.max(a, b).sum(-1)


def eager_triplet(measure, mv, s, im):
    scores = eager_sim(measure, im, s)
    diag = scores.diag().view(-1, 1)
    eye = torch.eye(scores.size(0), device=scores.device) > .5
    cost_s = (MARGIN + scores - diag).clamp(min=0).masked_fill(eye, 0)
    cost_im = (MARGIN + scores - diag.t()).clamp(min=0).masked_fill(eye, 0)
    if mv:
        cost_s, cost_im = cost_s.max(1)[0], cost_im.max(0)[0]
    return cost_s.sum() + cost_im.sum()


def measure_step(step, s, im, warmup, reps):
    def once():
        s.grad = im.grad = None
        step(s, im).backward()
    for _ in range(warmup):
        once()
    s.grad = im.grad = None  # the warm-up's gradients must not stand in for the measured step's
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    once()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        once()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, peak


def time_call(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    d = int(os.environ.get("D", 1536))
    batches = [int(b) for b in os.environ.get("BATCHES", "128,256").split(",")]
    warmup, reps = int(os.environ.get("WARMUP", 5)), int(os.environ.get("REPS", 50))
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    rows, parts = [], []
    for B in batches:
        s0 = torch.randn((B, d), device=dev, generator=gen)
        im0 = torch.randn((B, d), device=dev, generator=gen)
        for m in MEASURES:
            if m == "jaccard":
                s, im = s0.abs(), im0.abs()
            else:
                s, im = torch.nn.functional.normalize(s0, dim=1), torch.nn.functional.normalize(im0, dim=1)
            s.requires_grad_(True)
            im.requires_grad_(True)
            for mv in (True, False):
                crit = TripletLoss(margin=MARGIN, measure=m, max_violation=mv)
                ms, peak = measure_step(crit, s, im, warmup, reps)
                ems, epeak = measure_step(lambda a, b: eager_triplet(m, mv, a, b), s, im, warmup, reps)
                rows.append({"B": B, "D": d, "measure": m, "max_violation": mv, "hip_ms": round(ms, 4),
                             "eager_ms": round(ems, 4), "hip_peak_bytes": peak, "eager_peak_bytes": epeak,
                             "speedup": round(ems / ms, 2), "memory_ratio": round(epeak / max(peak, 1), 1)})
            # where the step's time goes: the K10 forward and the K17 backward (dense dS, both sides) alone
            metric, alpha, beta = MEASURE_TABLE[m]
            alpha = 1.0 / d if alpha is None else alpha
            a, b = im.detach(), s.detach()
            dS = torch.randn((B, B), device=dev, generator=gen)
            parts.append({"B": B, "D": d, "measure": m,
                          "k10_fwd_ms": round(time_call(lambda: engine.pairwise(a, b, metric, alpha, beta,
                                                                                torch.float32), warmup, reps), 4),
                          "k17_bwd_dense_ms": round(time_call(lambda: engine.pairwise_bwd(a, b, metric, alpha, dS),
                                                              warmup, reps), 4)})
    print(json.dumps({
        "metric": "TripletLoss(measure) forward + backward, ms per step and peak bytes allocated by one step",
        "config": {"margin": MARGIN, "direction": "all", "cost_style": "sum", "dtype": "f32", "warmup": warmup,
                   "reps": reps, "timing": "device events"},
        "hip": "K10 cmve_pairwise + K6 cmve_triplet_fwd/bwd + K17 cmve_pairwise_bwd",
        "baseline": "torch eager on the same GPU, B x B x D broadcast formulas (the reference's method) + autograd",
        "rows": rows, "parts": parts}))


if __name__ == "__main__":
    main()
