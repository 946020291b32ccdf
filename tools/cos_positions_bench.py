"""cal_perf under cosine with several captions per video: today's rank passes against the one-pass count (K26) on one
GPU.  Writes one JSON document (default profiles/cos_positions.json) and prints each size as it is measured.

  routes   validate.cal_perf_embeddings(videos, captions, ids, measure='cosine') with filter=None while
           engine.COS_FILTER_MIN_PAIRS is None -- today's passes: the fused two-direction rank count, and the v2t mAP
           from a rank pass over an expanded query set with one row per caption -- against filter="cosine": item
           words, ONE cmve_cos_count, list ranks.  Host embeddings in, the two 6-tuples out, both routes in this
           process, alternating repeat by repeat; the tuples of the two routes must be equal at every size.
  shapes   D = 1024, 20 captions per video, synth.multi_caption_embeddings rows (float64, as the reference's buffers):
           20,000 x 1,000; 59,800 x 2,990 (the msrvtt10k test split); 327,680 x 16,384
  launches per size, on sets already packed: the item words of both directions, cmve_cos_count without a band list
           (memsets, NaN items and the MFMA pass: the main kernel's time), and the whole cmve_cos_count; with the
           pairs the pass decided and the band it left

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
from cmve import engine  # noqa: E402
from cmve.linas import metrics, validate  # noqa: E402
from l2_filter_bench import alternate, stage_times, stats  # noqa: E402

SHAPES = ((20000, 1000), (59800, 2990), (327680, 16384))
PER, D = 20, 1024


def bench_size(n_c, n_v, warmup, reps):
    assert n_c == n_v * PER
    v, c, vid, cid = synth.multi_caption_embeddings(n_v=n_v, per=PER, d=D)
    out = {}

    def route(flt):
        def run():
            out[flt] = validate.cal_perf_embeddings(v, c, vid, cid, filter=flt)
            torch.cuda.synchronize()
        return run

    saved = engine.COS_FILTER_MIN_PAIRS
    engine.COS_FILTER_MIN_PAIRS = None  # filter=None is today's route whatever the committed constant says
    try:
        t = alternate({"today": route(None), "one_pass": route("cosine")}, warmup, reps)
    finally:
        engine.COS_FILTER_MIN_PAIRS = saved
    same = bool(np.array_equal(np.array(out[None], np.float64), np.array(out["cosine"], np.float64)))
    med = {k: statistics.median(x) for k, x in t.items()}
    spread = sum(max(x) - min(x) for x in t.values())
    res = {"n_c": n_c, "n_v": n_v, "d": D, "per_video": PER, "pairs": n_c * n_v,
           "today": stats(t["today"]), "one_pass": stats(t["one_pass"]),
           "speedup": round(med["today"] / med["one_pass"], 3), "combined_spread_s": round(spread, 6),
           "one_pass_wins": bool(med["today"] - med["one_pass"] > spread), "same_tuples": same,
           "stats": dict(engine.cos_gt_eval.stats)}
    out.clear()

    # the launches alone, on resident sets
    v2t_gt, t2v_gt = metrics.get_gt(vid, cid)
    caps, vids = engine.RowSet(c, with_lo=False), engine.RowSet(v, with_lo=False)
    dev = caps.device
    roff, ridx = engine.csr(metrics._lists(t2v_gt, n_c), dev)
    coff, cidx = engine.csr(v2t_gt, dev)
    rsc = torch.empty(n_c, dtype=torch.float64, device=dev)
    csc = torch.empty(n_c, dtype=torch.float64, device=dev)
    band = torch.empty(max(res["stats"]["band"], 1), dtype=torch.int64, device=dev)
    none = torch.empty(0, dtype=torch.int64, device=dev)
    st_main = torch.empty(4, dtype=torch.int64, device=dev)
    st_full = torch.empty(4, dtype=torch.int64, device=dev)
    stages = [
        ("item_words", lambda: (engine.cos_item_scores(caps, vids, roff, ridx, n_c, False, out=rsc),
                                engine.cos_item_scores(caps, vids, coff, cidx, n_c, True, out=csc))),
        ("count_without_band_list", lambda: engine.cos_count(caps, vids, (roff, rsc, n_v), (coff, csc, n_c),
                                                             band=none, stats=st_main)),
        ("count", lambda: engine.cos_count(caps, vids, (roff, rsc, n_v), (coff, csc, n_c), band=band, stats=st_full)),
    ]
    launches = []
    for r in range(warmup + reps):
        s = stage_times(stages)
        if r >= warmup:
            m, f = st_main.cpu().numpy(), st_full.cpu().numpy()
            launches.append(dict({k: round(x, 6) for k, x in s.items()}, decided=int(m[0]), band=int(m[1]),
                                 rescored=int(f[2]), overflow=int(f[3])))
    res["launches"] = launches
    res["launch_medians_s"] = {k: round(statistics.median(x[k] for x in launches), 6) for k, _ in stages}
    res["band_share"] = launches[-1]["band"] / float(n_c * n_v)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cos_positions.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--max-captions", type=int, default=SHAPES[-1][0], help="skip the sizes above this many captions")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "cos_positions_bench needs the GPU: nothing here is measured without it"
    assert a.reps >= 10, "at least 10 repeats per route"
    doc = {"tool": "tools/cos_positions_bench.py", "device": torch.cuda.get_device_name(0), "reps": a.reps,
           "warmup": a.warmup, "timer": "device events around calls that end in a synchronise", "sizes": []}
    for n_c, n_v in SHAPES:
        if n_c > a.max_captions:
            doc["sizes"].append({"n_c": n_c, "n_v": n_v, "not_measured": True})
            continue
        res = bench_size(n_c, n_v, a.warmup, a.reps)
        doc["sizes"].append(res)
        print(json.dumps({k: res[k] for k in res if k != "launches"}), flush=True)
        assert res["same_tuples"], "the two routes disagree"
        wins = [s["pairs"] for s in doc["sizes"] if s.get("one_pass_wins")]
        doc["crossover_pairs"] = min(wins) if wins else None
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    print("crossover_pairs:", doc.get("crossover_pairs"))


if __name__ == "__main__":
    main()
