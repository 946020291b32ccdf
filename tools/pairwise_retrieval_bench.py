"""Retrieval under the non-cosine measures (l1, l2, jaccard) on one GPU: the matrix route against the
matrix-free route (K18).  Writes one JSON document (default profiles/pairwise_retrieval.json) and prints it.

  evaluation  59,800 captions x 2,990 videos x 1536 (msrvtt10k test), host embeddings in, the two
              cal_perf tuples out:
                matrix  cal_error(videos, captions, m) -> host matrix -> cal_perf (K10, then the matrix uploaded
                        again for cmve_rank_from_matrix / cmve_gt_positions_from_matrix)
                fused   cal_perf_embeddings(..., measure=m) (K18: cmve_pairwise_positions, no matrix anywhere)
  top-10      n_q in {1, 16, 1000} captions x 1,048,576 videos x 1024:
                matrix  cal_error(video_embs, cap_embs, m) -> np.argsort(errors[i])[:10] per caption
                        (inference.py:78-80: the gallery goes to the device on every call)
                fused   GalleryScorer(video_embs, measure=m).topk_indices(cap_embs, 10): the gallery resident,
                        cmve_pairwise_topk
              beside n_q = 1 the floor: the resident gallery's bytes over the measured HBM rate.

Wall times are host clocks around calls that end with their results on the host (a device synchronise); each
figure is the median of REPS (default 20) repeats after WARMUP (default 2).  A configuration whose single repeat
costs more than BUDGET_S / REPS seconds is repeated as often as BUDGET_S (default 30) allows, at least once, and
its "reps" says how often; "not measured" marks what was skipped, with the reason.  Peak device memory is the
rise of torch.cuda.max_memory_allocated over what was allocated before the call.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "cross-modal-video-engine_amd"), ROOT):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from cmve.linas import evaluation, metrics, validate  # noqa: E402
from cmve.linas.inference import GalleryScorer  # noqa: E402

MEASURES = ["l1", "l2", "jaccard"]
HBM_MEASURED_BPS = 6.29e12  # float4 copy rate measured on the MI355X (8.0 TB/s specified)


def timed(fn, warmup, reps, budget_s):
    """(median seconds, repeats, peak device bytes over the baseline, last result)"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    first = time.perf_counter() - t0
    peak = torch.cuda.max_memory_allocated() - base
    if first * reps > budget_s:
        reps = max(int(budget_s / first), 0)
        warmup = 0
    times = [] if reps else [first]
    for _ in range(warmup):
        fn()
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return statistics.median(times), len(times), peak, out


def host_rows(n, d, seed, positive):
    """fp64 host rows (what encode_vid / encode_text return), generated on the device"""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn((n, d), device="cuda", generator=gen, dtype=torch.float32)
    x = (x.abs() if positive else x).to(torch.float64).cpu().numpy()
    torch.cuda.empty_cache()
    return x


def bench_eval(doc, save, n_c, n_v, d, warmup, reps, budget_s):
    video_ids = ["video%d" % j for j in range(n_v)]
    caption_ids = ["video%d#%d" % (i % n_v, i // n_v) for i in range(n_c)]
    v2t_gt, t2v_gt = metrics.get_gt(video_ids, caption_ids)
    for m in MEASURES:
        vid, cap = host_rows(n_v, d, 1, m == "jaccard"), host_rows(n_c, d, 2, m == "jaccard")

        def matrix_route():
            e = evaluation.cal_error(vid, cap, m)
            e = e if torch.is_tensor(e) else np.asarray(e)  # a plain matrix: cal_perf takes the matrix path
            return validate.cal_perf(e, v2t_gt, t2v_gt)

        def fused_route():
            return validate.cal_perf_embeddings(vid, cap, video_ids, caption_ids, measure=m)

        tf, rf, pf, of = timed(fused_route, warmup, reps, budget_s)
        tm, rm, pm, om = timed(matrix_route, warmup, reps, budget_s)
        itemsize = 4 if m == "jaccard" else 8
        row = {"measure": m, "n_c": n_c, "n_v": n_v, "d": d,
               "matrix": {"wall_s": round(tm, 4), "reps": rm, "peak_device_bytes": pm,
                          "host_matrix_bytes": n_c * n_v * itemsize},
               "fused": {"wall_s": round(tf, 4), "reps": rf, "peak_device_bytes": pf, "host_matrix_bytes": 0},
               "speedup": round(tm / tf, 2), "peak_device_ratio": round(pm / max(pf, 1), 1),
               "same_tuples": bool(np.allclose(np.array(of), np.array(om), rtol=0, atol=1e-12))}
        doc["evaluation"].append(row)
        save()
        print(json.dumps(row), flush=True)
        del vid, cap


def bench_topk(doc, save, n_g, d, nqs, warmup, reps, budget_s, matrix_max_nq, kept=None):
    for m in MEASURES:
        gal = host_rows(n_g, d, 3, m == "jaccard")
        scorer = GalleryScorer(gal, measure=m)
        g_bytes = scorer.gallery.numel() * scorer.gallery.element_size()
        for n_q in nqs:
            cap = host_rows(n_q, d, 4 + n_q, m == "jaccard")

            def fused_route():
                return scorer.topk_indices(cap, 10)

            def matrix_route():
                e = np.asarray(evaluation.cal_error(gal, cap, m))
                return np.stack([np.argsort(e[i], kind="stable")[:10] for i in range(n_q)])

            tf, rf, pf, of = timed(fused_route, warmup, reps, budget_s)
            row = {"measure": m, "n_q": n_q, "n_g": n_g, "d": d, "k": 10, "resident_gallery_bytes": g_bytes,
                   "fused": {"wall_s": round(tf, 5), "reps": rf, "peak_device_bytes": pf, "host_matrix_bytes": 0}}
            if n_q == 1:
                floor = g_bytes / HBM_MEASURED_BPS
                row["hbm_floor_s"] = round(floor, 6)
                row["fused_over_floor"] = round(tf / floor, 2)
            old = (kept or {}).get((m, n_q, n_g, d))
            if old is not None:  # --keep-matrix: the matrix route's figures of the earlier call (its code is unchanged)
                row["matrix"] = old["matrix"]
                if isinstance(old["matrix"], dict):
                    row["speedup"] = round(old["matrix"]["wall_s"] / tf, 1)
                    row["matrix_kept_from_earlier_call"] = True
            elif n_q <= matrix_max_nq or m == MEASURES[0]:
                # the matrix route holds the resident gallery's memory too (the scorer stays alive): its peak is
                # what the call itself adds
                try:
                    tm, rm, pm, om = timed(matrix_route, warmup, reps, budget_s)
                    row["matrix"] = {"wall_s": round(tm, 4), "reps": rm, "peak_device_bytes": pm,
                                     "host_matrix_bytes": n_q * n_g * (4 if m == "jaccard" else 8)}
                    row["speedup"] = round(tm / tf, 1)
                    row["same_ids"] = bool(np.array_equal(of, om))
                except MemoryError as ex:
                    row["matrix"] = "not measured: the %d-byte host matrix does not fit (%s)" % (n_q * n_g * 8, ex)
            else:
                row["matrix"] = ("not measured: one repeat is %d host argsorts of %d errors, measured for %s only"
                                 % (n_q, n_g, MEASURES[0]))
            doc["topk"].append(row)
            save()
            print(json.dumps(row), flush=True)
        del scorer, gal
        torch.cuda.empty_cache()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairwise_retrieval.json"))
    ap.add_argument("--sections", default="evaluation,topk")
    ap.add_argument("--eval-shape", default="59800,2990,1536")
    ap.add_argument("--gallery-shape", default="1048576,1024")
    ap.add_argument("--nq", default="1,16,1000")
    ap.add_argument("--matrix-max-nq", type=int, default=16,
                    help="largest n_q whose matrix route is timed for every measure (beyond: the first measure only)")
    ap.add_argument("--keep-matrix", action="store_true",
                    help="top-k: re-time the fused route only and keep the matrix route's figures already in --out")
    a = ap.parse_args(argv)
    warmup, reps = int(os.environ.get("WARMUP", 2)), int(os.environ.get("REPS", 20))
    budget_s = float(os.environ.get("BUDGET_S", 30))
    assert torch.cuda.is_available(), "pairwise_retrieval_bench needs the GPU: nothing here is measured without it"
    torch.cuda.set_device(0)
    doc = {"what": "retrieval under non-cosine measures: matrix route (K10 + host matrix) against the matrix-free "
                   "route (K18), one MI355X",
           "config": {"warmup": warmup, "reps": reps, "budget_s": budget_s, "timing": "host clock around calls that "
                      "end on the host, median", "hbm_measured_bytes_per_s": HBM_MEASURED_BPS,
                      "device": torch.cuda.get_device_name(0)},
           "evaluation": [], "topk": []}
    kept = None
    if os.path.exists(a.out):  # sections measured by an earlier call are kept
        with open(a.out) as f:
            old = json.load(f)
        if a.keep_matrix:
            kept = {(r["measure"], r["n_q"], r["n_g"], r["d"]): r for r in old.get("topk", []) if "matrix" in r}
        for k in ("evaluation", "topk"):
            if k not in a.sections.split(","):
                doc[k] = old.get(k, [])

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")

    if "evaluation" in a.sections.split(","):
        n_c, n_v, d = (int(x) for x in a.eval_shape.split(","))
        bench_eval(doc, save, n_c, n_v, d, warmup, reps, budget_s)
    if "topk" in a.sections.split(","):
        n_g, d = (int(x) for x in a.gallery_shape.split(","))
        bench_topk(doc, save, n_g, d, [int(x) for x in a.nq.split(",")], warmup, reps, budget_s, a.matrix_max_nq,
                   kept)
    save()
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
