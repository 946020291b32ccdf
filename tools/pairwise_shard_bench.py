"""The sharded evaluation under the non-cosine measures (ShardedGallery(..., measure=)) on ONE GPU.  Writes one JSON
document (default profiles/pairwise_sharded.json) and prints it.

  (a) world-1 overhead   59,800 captions x 2,990 videos x 1536 (the shape of profiles/pairwise_retrieval.json), l1 and
                         jaccard, host embeddings in, the two cal_perf tuples out, the two routes alternating:
                           unsharded  validate.cal_perf_embeddings(..., measure=m)      (cmve_pairwise_positions)
                           world-1    metrics.get_gt(...) (cal_perf_embeddings runs it inside), then
                                      ShardedGallery(videos, 0, n_v, measure=m).cal_perf(captions, ...)
                                      (cmve_pairwise_item_scores + cmve_pairwise_count + cmve_pairwise_list_ranks)
                         REPS (default 5) repeats each after WARMUP (default 1): median, min and max of both, the
                         overhead against the unsharded spread, and where EACH route's time goes (single timings of
                         its pieces).
  (b) shard-local step   16,384 captions x (131,072 / N) videos x 1024 under l2, N = 1, 2, 4, 8: the item scores of
                         both directions plus the ONE counting pass, what a rank of an N-GPU job runs between its
                         collectives.  Each N's time beside time(N = 1) / N.

Every figure is the device time between two events on the stream around the call (the calls of (a) end on the host,
so that is their wall time too).  NOT measured: the collectives over RCCL at N > 1 -- one GPU cannot run them, so no
speed-up of an N-GPU job is derived from (b).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "cross-modal-video-engine_amd"), ROOT):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from cmve import dist as D  # noqa: E402
from cmve.linas import metrics, validate  # noqa: E402
from cmve.linas.evaluation import measure_rows  # noqa: E402


def event_time(fn):
    """(seconds between two device events around fn, its result)"""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    out = fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / 1e3, out


def stats(times):
    return {"median_s": round(statistics.median(times), 5), "min_s": round(min(times), 5),
            "max_s": round(max(times), 5), "spread_s": round(max(times) - min(times), 5), "reps": len(times)}


def host_rows(n, d, seed, positive):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn((n, d), device="cuda", generator=gen, dtype=torch.float32)
    x = (x.abs() if positive else x).to(torch.float64).cpu().numpy()
    torch.cuda.empty_cache()
    return x


def bench_world1(doc, save, n_c, n_v, d, warmup, reps):
    video_ids = ["video%d" % j for j in range(n_v)]
    caption_ids = ["video%d#%d" % (i % n_v, i // n_v) for i in range(n_c)]
    for m in ("l1", "jaccard"):
        vid, cap = host_rows(n_v, d, 1, m == "jaccard"), host_rows(n_c, d, 2, m == "jaccard")

        def unsharded():
            return validate.cal_perf_embeddings(vid, cap, video_ids, caption_ids, measure=m)

        def world1():  # the same work from the same inputs: get_gt is inside cal_perf_embeddings too
            v2t_gt, t2v_gt = metrics.get_gt(video_ids, caption_ids)
            return D.ShardedGallery(vid, offset=0, n_global=n_v, measure=m).cal_perf(cap, v2t_gt, t2v_gt)

        tu, tw = [], []
        for r in range(warmup + reps):  # alternating: both routes see the same neighbours on the machine
            a, ou = event_time(unsharded)
            b, ow = event_time(world1)
            if r >= warmup:
                tu.append(a)
                tw.append(b)
        # where each route's time goes: one more call of each, piece by piece (single timings)
        t_gt, (v2t_gt, t2v_gt) = event_time(lambda: metrics.get_gt(video_ids, caption_ids))
        t_urows, (uc, uv) = event_time(lambda: (measure_rows(cap, m), measure_rows(vid, m)))
        t2v_l = metrics._lists(t2v_gt, n_c)
        t_ueval, ((tp, tr), (vp, vr)) = event_time(lambda: metrics.measure_eval(uc, uv, m, t2v_l, v2t_gt))
        t_umaps, _ = event_time(lambda: (metrics.maps_from_positions(tp, vp),
                                         metrics.metrics_from_ranks(vr.astype(np.int32)),
                                         metrics.metrics_from_ranks(tr.astype(np.int32))))
        del uc, uv
        t_make, sh = event_time(lambda: D.ShardedGallery(vid, offset=0, n_global=n_v, measure=m))
        t_rows, q = event_time(lambda: sh._pw_rows(cap))
        t2v_lists = [t2v_gt[i] for i in range(n_c)]
        t_csr, (row, col) = event_time(lambda: (sh._pw_csr(t2v_lists, n_v, "GT video"),
                                                sh._pw_csr(sh.local_v2t_lists(v2t_gt), n_c, "GT caption")))
        t_pass, _ = event_time(lambda: sh._pw_pass(q, n_c, row, col))
        su, sw = stats(tu), stats(tw)
        over = sw["median_s"] - su["median_s"]
        res = {"measure": m, "n_c": n_c, "n_v": n_v, "d": d, "unsharded": su, "world1": sw,
               "world1_overhead_s": round(over, 5), "world1_over_unsharded": round(sw["median_s"] / su["median_s"], 4),
               "overhead_exceeds_unsharded_spread": bool(over > su["spread_s"]),
               "unsharded_pieces_s": {"get_gt": round(t_gt, 5), "rows_to_device": round(t_urows, 5),
                                      "csr_positions_and_host_ranks": round(t_ueval, 5),
                                      "maps_and_metrics_on_host": round(t_umaps, 5)},
               "world1_pieces_s": {"get_gt": round(t_gt, 5), "gallery_to_device": round(t_make, 5),
                                   "captions_to_device": round(t_rows, 5),
                                   "gt_lists_checked_and_csr": round(t_csr, 5),
                                   "item_scores_count_ranks_on_device": round(t_pass, 5),
                                   "rest_host_ranks_gather_and_map": round(max(sw["median_s"] - t_gt - t_make - t_rows
                                                                               - t_csr - t_pass, 0.0), 5)},
               "same_tuples": bool(np.allclose(np.array(ou), np.array(ow), rtol=0, atol=1e-12))}
        doc["world1_overhead"].append(res)
        save()
        print(json.dumps(res), flush=True)
        del vid, cap, sh, q
        torch.cuda.empty_cache()


def bench_shard_step(doc, save, n_q, n_g, d, shards, warmup, reps):
    m = "l2"
    gen = torch.Generator(device="cuda").manual_seed(5)
    gal = torch.randn((n_g, d), device="cuda", generator=gen, dtype=torch.float64)
    q = torch.randn((n_q, d), device="cuda", generator=gen, dtype=torch.float64)
    t2v = [[i % n_g] for i in range(n_q)]
    base = None
    for N in shards:
        n = n_g // N
        sh = D.ShardedGallery(gal[:n], offset=0, n_global=n_g, measure=m)  # rank 0's shard of an N-rank job
        row = sh._pw_csr(t2v, n_g, "GT video")
        v2t = [[i for i in range(j, n_q, n_g)] for j in range(n)]
        col = sh._pw_csr(v2t, n_q, "GT caption")

        def step():
            r_sc = sh._pw_items(q, row[:2], row[2], False, 0)
            c_sc = sh._pw_items(q, col[:2], col[2], True, 0)
            return sh._pw_count(q, (row[0], r_sc, n_g), (col[0], c_sc, n_q))

        times = [event_time(step)[0] for _ in range(warmup + reps)][warmup:]
        st = stats(times)
        if base is None:
            base = st["median_s"] * N  # N = 1 comes first
        ideal = base / N
        out = {"measure": m, "n_q": n_q, "n_g": n_g, "d": d, "N": N, "shard_rows": n, "step": st,
               "n1_over_N_s": round(ideal, 5), "step_over_ideal": round(st["median_s"] / ideal, 4)}
        doc["shard_local_step"].append(out)
        save()
        print(json.dumps(out), flush=True)
        del sh


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairwise_sharded.json"))
    ap.add_argument("--sections", default="world1,step")
    ap.add_argument("--eval-shape", default="59800,2990,1536")
    ap.add_argument("--step-shape", default="16384,131072,1024")
    ap.add_argument("--shards", default="1,2,4,8")
    a = ap.parse_args(argv)
    warmup, reps = int(os.environ.get("WARMUP", 1)), int(os.environ.get("REPS", 5))
    assert torch.cuda.is_available(), "pairwise_shard_bench needs the GPU: nothing here is measured without it"
    torch.cuda.set_device(0)
    doc = {"what": "ShardedGallery(..., measure=): the world-1 route against the unsharded K18 call, and the "
                   "shard-local step at 1/N of the gallery, one MI355X",
           "config": {"warmup": warmup, "reps": reps, "timing": "device events around the call, median of reps",
                      "device": torch.cuda.get_device_name(0)},
           "not_measured": "the collectives over RCCL at N > 1 (one GPU; RCCL has never run at N > 1 here): the "
                           "shard-local step says what a rank computes between them, not what an N-GPU job gains",
           "world1_overhead": [], "shard_local_step": []}

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")

    if "world1" in a.sections.split(","):
        n_c, n_v, d = (int(x) for x in a.eval_shape.split(","))
        bench_world1(doc, save, n_c, n_v, d, warmup, reps)
    if "step" in a.sections.split(","):
        n_q, n_g, d = (int(x) for x in a.step_shape.split(","))
        shards = sorted(int(x) for x in a.shards.split(","))
        assert shards[0] == 1, "N = 1 is the yardstick of the others"
        bench_shard_step(doc, save, n_q, n_g, d, shards, warmup, reps)
    save()
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
