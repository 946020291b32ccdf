"""ShardedGallery(measure='cosine').cal_perf with several captions per video at world 1: today's rank passes against
the one pass per shard (K27, filter="cosine") on one GPU.  Writes one JSON document (default
profiles/cos_positions_sharded.json) and prints each size as it is measured.

  routes   ShardedGallery(videos, 0, n_v, with_lo=False, filter=...).cal_perf(captions, v2t_gt, t2v_gt) on a shard
           that holds the whole gallery (world 1: every collective is a copy or skipped).  filter=None -- today's
           passes: the fused two-direction rank count, and the v2t mAP from a rank pass over an expanded query set
           with one row per caption -- against filter="cosine": global-id lists, item words, ONE
           cmve_cos_count_resolved, list ranks.  Captions on the device in, the two 6-tuples out, both shards resident
           in this process, the routes alternating repeat by repeat; the tuples of the two routes must be equal at
           every size.
  shapes   D = 1024, 20 captions per video, synth.multi_caption_embeddings rows (float64, as the reference's buffers):
           59,800 x 2,990 (the msrvtt10k test split); 327,680 x 16,384
  count    per size, on the shard's own lists and band list: the item words of both directions and the whole
           cmve_cos_count_resolved, with the pairs the pass decided and the band it left

Times are device events around calls that end in a synchronise (a copy to the host), medians of --reps (default 10)
repeats after --warmup (default 1).  No profiler, no counters."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "cross-modal-video-engine_amd"), ROOT, os.path.join(ROOT, "tests", "golden"),
          os.path.dirname(os.path.abspath(__file__))):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import synth  # noqa: E402
from cmve import dist as D  # noqa: E402
from cmve.linas import metrics  # noqa: E402
from l2_filter_bench import alternate, stage_times, stats  # noqa: E402

SHAPES = ((59800, 2990), (327680, 16384))
PER, DIM = 20, 1024


def bench_size(n_c, n_v, warmup, reps):
    assert n_c == n_v * PER
    v, c, vid, cid = synth.multi_caption_embeddings(n_v=n_v, per=PER, d=DIM)
    v2t_gt, t2v_gt = metrics.get_gt(vid, cid)
    shards = {flt: D.ShardedGallery(v, offset=0, n_global=n_v, with_lo=False, filter=flt) for flt in (None, "cosine")}
    q = torch.from_numpy(c).to(shards[None].device)
    out = {}

    def route(flt):
        def run():
            out[flt] = shards[flt].cal_perf(q, v2t_gt, t2v_gt)
            torch.cuda.synchronize()
        return run

    t = alternate({"today": route(None), "one_pass": route("cosine")}, warmup, reps)
    same = bool(np.array_equal(np.array(out[None], np.float64), np.array(out["cosine"], np.float64)))
    med = {k: statistics.median(x) for k, x in t.items()}
    spread = sum(max(x) - min(x) for x in t.values())
    sh = shards["cosine"]
    res = {"n_c": n_c, "n_v": n_v, "d": DIM, "per_video": PER, "pairs": n_c * n_v, "world": 1,
           "today": stats(t["today"]), "one_pass": stats(t["one_pass"]),
           "speedup": round(med["today"] / med["one_pass"], 3), "combined_spread_s": round(spread, 6),
           "one_pass_wins": bool(med["today"] - med["one_pass"] > spread),
           "difference_exceeds_spread": bool(abs(med["today"] - med["one_pass"]) > spread), "same_tuples": same,
           "tuples": [list(map(float, x)) for x in out["cosine"]], "stats": sh.filter_stats,
           "band_slots": int(sh._pw_band.numel())}
    out.clear()

    # the count alone: the pass's own launches on the packed captions
    t2v_lists, v2t_lists = [t2v_gt[i] for i in range(n_c)], [v2t_gt[j] for j in range(n_v)]
    caps = sh._pw_rows(q)
    row = sh._pw_csr(t2v_lists, n_v, "GT video")
    col = sh._pw_csr(sh.local_v2t_lists(v2t_lists), n_c, "GT caption")
    words = {}

    def items():
        words["row"] = sh._pw_items(caps, row[:2], row[2], False, 0)
        words["col"] = sh._pw_items(caps, col[:2], col[2], True, 0)

    stages = [("item_words", items),
              ("count_resolved", lambda: sh._pw_count(caps, (row[0], words["row"], n_v), (col[0], words["col"], n_c)))]
    launches = []
    for r in range(warmup + reps):
        s = stage_times(stages)
        if r >= warmup:
            launches.append(dict({k: round(x, 6) for k, x in s.items()}, **sh.filter_stats))
    res["launches"] = launches
    res["launch_medians_s"] = {k: round(statistics.median(x[k] for x in launches), 6) for k, _ in stages}
    res["band_share"] = launches[-1]["band"] / float(n_c * n_v)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cos_positions_sharded.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--max-captions", type=int, default=SHAPES[-1][0], help="skip the sizes above this many captions")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "cos_positions_sharded_bench needs the GPU: nothing here is measured without it"
    assert a.reps >= 10, "at least 10 repeats per route"
    doc = {"tool": "tools/cos_positions_sharded_bench.py", "device": torch.cuda.get_device_name(0), "reps": a.reps,
           "warmup": a.warmup, "timer": "device events around calls that end in a synchronise", "sizes": []}
    for n_c, n_v in SHAPES:
        if n_c > a.max_captions:
            doc["sizes"].append({"n_c": n_c, "n_v": n_v, "not_measured": True})
            continue
        res = bench_size(n_c, n_v, a.warmup, a.reps)
        doc["sizes"].append(res)
        print(json.dumps({k: res[k] for k in res if k != "launches"}), flush=True)
        assert res["same_tuples"], "the two routes disagree"
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
