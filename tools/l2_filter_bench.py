"""The MFMA-filtered count pass of the Euclidean measures (K19) against the fp64 route (K18) on one GPU.  Writes one
JSON document (default profiles/l2_filter.json) and prints each section as it is measured.

  speedup    16,384 captions x 131,072 videos x 1024 (the shape of DESIGN s6), l2, planted GTs (caption = its video
             + 0.5 N(0, 1)), fp64 rows resident on the device:
               call      one engine.pairwise_gt_eval(..., filter=False / True) -- lists in, positions and ranks out
               launches  the device work alone: fp64 route = both item launches + cmve_pairwise_count (the "step" of
                         profiles/pairwise_sharded.json); filter route = pack A, pack B, both item launches,
                         cmve_l2_count; cmve_l2_count with no band list is the MFMA pass alone, the difference to
                         the whole call is the re-score of the band
  crossover  both routes at na = nb in {256 .. 4096}, D = 1024, one pairwise_gt_eval each: the smallest size at
             which the filter wins by more than the spread of the repeats sets engine.L2_FILTER_MIN_PAIRS
  cal_perf   cal_perf_embeddings(..., measure='l2') at 59,800 x 2,990 x 1536, host embeddings in, tuples out (host
             clock, as profiles/pairwise_retrieval.json): random rows as there, and planted GTs

  sharded    (--sections sharded, written to profiles/l2_filter_sharded.json) the sharded evaluation's count pass (K21),
             a world-1 ShardedGallery(measure='l2'), filter=True against filter=False (the fp64 route of K18):
               headline   evaluate_device at the speedup shape, planted GTs; the shard's pack apart (a one-time cost)
               gate       cmve_l2_count_resolved against cmve_l2_count on the same inputs with a list that holds the
                          band: what the two gated launches cost when they do nothing
               overflow   rows clustered far from the origin (100 + N(0, 1)), 1000 captions over the gallery: a pass
                          whose list overflows (filter + canonical count) against the fp64 route, and the next pass
                          once a host-ending method has latched the fp64 route
               crossover  evaluate_device at n_q = n in {1024, 2048, 4096}, the shard already packed

Times are device events around the calls (the user-facing cal_perf: host clock), medians of REPS (default 5)
repeats after WARMUP (default 1), the two routes alternating repeat by repeat."""
import argparse
import ctypes as C
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

from cmve import _lib, engine  # noqa: E402
from cmve._lib import lib, check  # noqa: E402
from cmve.linas import validate  # noqa: E402

F64 = torch.float64


def event_time(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    out = fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / 1e3, out


def stats(times):
    return {"median_s": round(statistics.median(times), 6), "min_s": round(min(times), 6),
            "max_s": round(max(times), 6), "spread_s": round(max(times) - min(times), 6), "reps": len(times)}


def alternate(fns, warmup, reps, timer=event_time):
    """{name: [seconds]} with the routes alternating repeat by repeat"""
    out = {k: [] for k in fns}
    for r in range(warmup + reps):
        for k, fn in fns.items():
            t = timer(fn)[0]
            if r >= warmup:
                out[k].append(t)
    return out


def planted(n_q, n_g, d, seed, noise=0.5):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    gal = torch.randn((n_g, d), device="cuda", generator=gen, dtype=F64)
    q = gal[:n_q] + noise * torch.randn((n_q, d), device="cuda", generator=gen, dtype=F64)
    rows = [[i] for i in range(n_q)]
    cols = [[j] if j < n_q else [] for j in range(n_g)]
    return q, gal, rows, cols


def stage_times(stages):
    """device seconds of each (name, fn) in order, one event between neighbours"""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(stages) + 1)]
    torch.cuda.synchronize()
    ev[0].record()
    for i, (_, fn) in enumerate(stages):
        fn()
        ev[i + 1].record()
    ev[-1].synchronize()
    return {name: ev[i].elapsed_time(ev[i + 1]) / 1e3 for i, (name, _) in enumerate(stages)}


def bench_speedup(doc, save, n_q, n_g, d, warmup, reps):
    q, gal, rows, cols = planted(n_q, n_g, d, 5)
    dev = q.device
    alpha, beta = 1.0, 0.0
    holder = {}

    def call(flt):
        r = engine._PairwisePositions(q, gal, _lib.PW_L2, alpha, beta, F64, rows, cols, filter=flt)
        holder[flt] = r
        return r

    t = alternate({"fp64": lambda: call(False), "filter": lambda: call(True)}, warmup, reps)
    same = all(np.array_equal(holder[True].pos[s], holder[False].pos[s]) for s in (0, 1))
    st = holder[True].filter_stats
    res = {"n_q": n_q, "n_g": n_g, "d": d, "measure": "l2", "rows": "fp64, planted GTs",
           "call": {"fp64": stats(t["fp64"]), "filter": stats(t["filter"]),
                    "speedup": round(statistics.median(t["fp64"]) / statistics.median(t["filter"]), 2)},
           "same_words": bool(same), "filter_stats": st, "band_share": st["band"] / float(n_q * n_g)}
    holder.clear()
    # the launches alone
    roff, ridx = engine.csr(rows, dev)
    coff, cidx = engine.csr(cols, dev)
    ri, ci = n_q, n_q
    h = engine.handle(dev)

    def fp64_step():
        r_sc = engine.pairwise_item_scores(q, gal, _lib.PW_L2, alpha, beta, F64, roff, ridx, ri, False, 0)
        c_sc = engine.pairwise_item_scores(q, gal, _lib.PW_L2, alpha, beta, F64, coff, cidx, ci, True, 0)
        return engine.pairwise_count(q, gal, _lib.PW_L2, alpha, beta, F64, (roff, r_sc, n_g), (coff, c_sc, n_q),
                                     filter=False)

    ra, rb = engine.RowSet(q, with_lo=False), engine.RowSet(gal, with_lo=False)
    cap = max(st["band"], 1)
    ws = torch.empty(cap, dtype=torch.int64, device=dev)
    cnt = torch.empty(4, dtype=torch.int64, device=dev)
    rpos = torch.empty(ri, dtype=torch.int32, device=dev)
    cpos = torch.empty(ci, dtype=torch.int32, device=dev)
    sc = {}

    def pack(rs):
        check(lib.cmve_pack_rows(h, C.byref(rs.desc)), "cmve_pack_rows")

    def items():
        sc["r"] = engine.pairwise_item_scores(q, gal, _lib.PW_L2, alpha, beta, F64, roff, ridx, ri, False, 0)
        sc["c"] = engine.pairwise_item_scores(q, gal, _lib.PW_L2, alpha, beta, F64, coff, cidx, ci, True, 0)

    def count(nbytes):
        check(lib.cmve_l2_count(h, C.byref(ra.desc), C.byref(rb.desc), alpha, beta, engine._ptr(roff),
                                engine._ptr(sc["r"]), ri, n_g, engine._ptr(rpos), engine._ptr(coff),
                                engine._ptr(sc["c"]), ci, n_q, engine._ptr(cpos), engine._ptr(ws), nbytes,
                                engine._ptr(cnt)), "cmve_l2_count")

    stages = [("pack_captions", lambda: pack(ra)), ("pack_videos", lambda: pack(rb)), ("item_scores", items),
              ("l2_count_mfma_pass_only", lambda: count(0)), ("l2_count", lambda: count(8 * cap))]
    per = {name: [] for name, _ in stages}
    step = []
    for r in range(warmup + reps):
        ts = event_time(fp64_step)[0]
        tt = stage_times(stages)
        if r >= warmup:
            step.append(ts)
            for k, v in tt.items():
                per[k].append(v)
    med = {k: statistics.median(v) for k, v in per.items()}
    filt = med["pack_captions"] + med["pack_videos"] + med["item_scores"] + med["l2_count"]
    res["launches"] = {
        "fp64_item_scores_and_count": stats(step),
        "filter": {k: stats(v) for k, v in per.items()},
        "filter_band_rescore_s": round(med["l2_count"] - med["l2_count_mfma_pass_only"], 6),
        "filter_total_s": round(filt, 6),
        "speedup": round(statistics.median(step) / filt, 2),
        "mfma_pass_tflops": round(2.0 * n_q * n_g * rb.d_pad / med["l2_count_mfma_pass_only"] / 1e12, 1)}
    doc["speedup"] = res
    save()
    print(json.dumps(res), flush=True)


def bench_crossover(doc, save, sizes, d, warmup, reps):
    table, chosen = [], None
    for n in sizes:
        q, gal, rows, cols = planted(n, n, d, 7 + n)
        t = alternate({"fp64": lambda: engine.pairwise_gt_eval(q, gal, _lib.PW_L2, 1.0, 0.0, F64, rows, cols, False),
                       "filter": lambda: engine.pairwise_gt_eval(q, gal, _lib.PW_L2, 1.0, 0.0, F64, rows, cols, True)},
                      warmup, reps)
        a, b = stats(t["fp64"]), stats(t["filter"])
        wins = a["median_s"] - b["median_s"] > max(a["spread_s"], b["spread_s"])
        table.append({"na": n, "nb": n, "d": d, "fp64": a, "filter": b, "filter_wins_beyond_spread": bool(wins)})
        if wins and chosen is None:
            chosen = n
        print(json.dumps(table[-1]), flush=True)
    doc["crossover"] = {"table": table, "smallest_winning_size": chosen,
                        "min_pairs": None if chosen is None else chosen * chosen,
                        "engine_L2_FILTER_MIN_PAIRS": engine.L2_FILTER_MIN_PAIRS}
    save()


def bench_sharded(doc, save, n_q, n_g, d, sizes, warmup, reps):
    from cmve import dist as D

    def pair_of_shards(gal):
        return {f: D.ShardedGallery(gal, offset=0, n_global=gal.shape[0], measure="l2", filter=f)
                for f in (False, True)}

    def both_routes(shards, q, rows, cols, n):
        """evaluate_device on the two shards, alternating; (stats fp64, stats filter, same words, filter_stats)"""
        row_csr = shards[True].local_gt_csr(rows)
        col_csr = shards[True].local_v2t_csr(cols) if cols is not None else None
        last = {}

        def run(f):
            last[f] = shards[f].evaluate_device(q, row_csr, col_csr, n)
            return last[f]

        t = alternate({"fp64": lambda: run(False), "filter": lambda: run(True)}, warmup, reps)
        same = all(x is None or torch.equal(x, y) for x, y in zip(last[True][:3], last[False][:3]))
        return stats(t["fp64"]), stats(t["filter"]), bool(same), shards[True].filter_stats

    def verdict(a, b):
        return bool(a["median_s"] - b["median_s"] > a["spread_s"] + b["spread_s"])

    # ---- headline + gate ----
    q, gal, rows, cols = planted(n_q, n_g, d, 5)
    shards = pair_of_shards(gal)
    h = engine.handle(q.device)
    t_first_pack = event_time(shards[True]._pw_pack)[0]
    packs = [event_time(lambda: check(lib.cmve_pack_rows(h, C.byref(shards[True]._pw_packed.desc)), "cmve_pack_rows"))[0]
             for _ in range(reps)]
    a, b, same, st = both_routes(shards, q, rows, cols, n_q)
    head = {"n_q": n_q, "n_g": n_g, "d": d, "measure": "l2", "rows": "fp64, planted GTs", "world": 1,
            "call": "ShardedGallery.evaluate_device, both directions", "fp64": a, "filter": b,
            "speedup": round(a["median_s"] / b["median_s"], 2), "filter_wins_beyond_both_spreads": verdict(a, b),
            "same_words": same, "filter_stats": st, "band_slots": int(shards[True]._pw_band.numel()),
            "shard_pack_one_time": {"first_call_s": round(t_first_pack, 6), "repack": stats(packs)}}
    doc["headline"] = head
    save()
    print(json.dumps(head), flush=True)

    roff, ridx = engine.csr(rows, q.device)
    coff, cidx = engine.csr(cols, q.device)
    r_sc = engine.pairwise_item_scores(q, gal, _lib.PW_L2, 1.0, 0.0, F64, roff, ridx, n_q, False, 0)
    c_sc = engine.pairwise_item_scores(q, gal, _lib.PW_L2, 1.0, 0.0, F64, coff, cidx, n_q, True, 0)
    ra, rb = engine.RowSet(q, with_lo=False), shards[True]._pw_packed
    ws = torch.empty(max(st["band"], 1), dtype=torch.int64, device=q.device)
    cnt = torch.empty(4, dtype=torch.int64, device=q.device)
    rpos = torch.empty(n_q, dtype=torch.int32, device=q.device)
    cpos = torch.empty(n_q, dtype=torch.int32, device=q.device)

    def entry(fn, name):
        check(fn(h, C.byref(ra.desc), C.byref(rb.desc), 1.0, 0.0, engine._ptr(roff), engine._ptr(r_sc), n_q, n_g,
                 engine._ptr(rpos), engine._ptr(coff), engine._ptr(c_sc), n_q, n_q, engine._ptr(cpos),
                 engine._ptr(ws), 8 * ws.numel(), engine._ptr(cnt)), name)

    t = alternate({"l2_count": lambda: entry(lib.cmve_l2_count, "cmve_l2_count"),
                   "resolved": lambda: entry(lib.cmve_l2_count_resolved, "cmve_l2_count_resolved")}, warmup, reps)
    a, b = stats(t["l2_count"]), stats(t["resolved"])
    gate = {"cmve_l2_count": a, "cmve_l2_count_resolved": b, "overflow": int(cnt[3].item()),
            "gated_count_tiles": int(-(-n_g // 128) * -(-n_q // 64)),
            "difference_s": round(b["median_s"] - a["median_s"], 6),
            "beyond_the_spread": bool(b["median_s"] - a["median_s"] > max(a["spread_s"], b["spread_s"]))}
    doc["gate"] = gate
    save()
    print(json.dumps(gate), flush=True)
    del shards, q, gal, ra, rb, ws, r_sc, c_sc, rows, cols
    torch.cuda.empty_cache()

    # ---- a pass that overflows, and the pass after the latch ----
    n_c = 1000
    gen = torch.Generator(device="cuda").manual_seed(3)
    gal = 100.0 + torch.randn((n_g, d), device="cuda", generator=gen, dtype=F64)
    q = 100.0 + torch.randn((n_c, d), device="cuda", generator=gen, dtype=F64)
    rows = [[int(j)] for j in np.random.default_rng(3).integers(0, n_g, n_c)]
    shards = pair_of_shards(gal)
    shards[True]._pw_pack()
    a, b, same, st = both_routes(shards, q, rows, None, n_c)
    over = {"n_q": n_c, "n_g": n_g, "d": d, "rows": "100 + N(0, 1)", "fp64": a, "overflowing_pass": b,
            "same_words": same, "filter_stats": st}
    shards[True]._pw_plan()  # what evaluate / cal_perf / rank_queries do after their result copies
    a, b, same, st2 = both_routes(shards, q, rows, None, n_c)
    over["after_the_latch"] = {"latched": bool(shards[True]._pw_filter_off), "fp64": a, "latched_pass": b,
                               "same_words": same, "filter_stats": st2}
    doc["overflow"] = over
    save()
    print(json.dumps(over), flush=True)
    del shards, q, gal
    torch.cuda.empty_cache()

    # ---- crossover, the shard already packed ----
    table, chosen = [], None
    for n in sizes:
        q, gal, rows, cols = planted(n, n, d, 7 + n)
        shards = pair_of_shards(gal)
        shards[True]._pw_pack()
        a, b, same, st = both_routes(shards, q, rows, cols, n)
        wins = verdict(a, b)
        table.append({"n_q": n, "n": n, "d": d, "fp64": a, "filter": b, "same_words": same,
                      "filter_wins_beyond_both_spreads": wins})
        if wins and chosen is None:
            chosen = n
        print(json.dumps(table[-1]), flush=True)
    doc["crossover"] = {"table": table, "smallest_winning_size": chosen,
                        "engine_L2_FILTER_MIN_PAIRS": engine.L2_FILTER_MIN_PAIRS}
    save()


def host_clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def bench_cal_perf(doc, save, n_c, n_v, d, warmup, reps):
    video_ids = ["video%d" % j for j in range(n_v)]
    caption_ids = ["video%d#%d" % (i % n_v, i // n_v) for i in range(n_c)]
    rng = np.random.default_rng(11)
    out = []
    for kind in ("random rows", "planted GTs"):
        vid = rng.standard_normal((n_v, d))
        cap = rng.standard_normal((n_c, d))
        if kind == "planted GTs":
            cap = vid[np.arange(n_c) % n_v] + 0.5 * cap
        seen = {}

        def run(flt):
            r = validate.cal_perf_embeddings(vid, cap, video_ids, caption_ids, measure="l2", filter=flt)
            seen[flt] = r
            return r

        t = alternate({"fp64": lambda: run(False), "auto": lambda: run(None)}, warmup, reps, host_clock)
        caps_d, vids_d = engine.to_device(cap), engine.to_device(vid)
        v2t = [[i for i in range(j, n_c, n_v)] for j in range(n_v)]
        probe = engine._PairwisePositions(caps_d, vids_d, _lib.PW_L2, 1.0, 0.0, F64,
                                          [[i % n_v] for i in range(n_c)], v2t)
        row = {"n_c": n_c, "n_v": n_v, "d": d, "measure": "l2", "rows": kind, "timing": "host clock",
               "filter_false": stats(t["fp64"]), "auto": stats(t["auto"]), "auto_filter_stats": probe.filter_stats,
               "same_tuples": bool(np.allclose(np.array(seen[False]), np.array(seen[None]), rtol=0, atol=0))}
        out.append(row)
        print(json.dumps(row), flush=True)
        del caps_d, vids_d, probe
    doc["cal_perf_embeddings"] = out
    save()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "l2_filter.json"))
    ap.add_argument("--sections", default="speedup,crossover,cal_perf")
    ap.add_argument("--shape", default="16384,131072,1024")
    ap.add_argument("--sizes", default="256,512,1024,2048,4096")
    ap.add_argument("--eval-shape", default="59800,2990,1536")
    ap.add_argument("--sharded-out", default=os.path.join(ROOT, "profiles", "l2_filter_sharded.json"))
    ap.add_argument("--sharded-sizes", default="1024,2048,4096")
    a = ap.parse_args(argv)
    warmup, reps = int(os.environ.get("WARMUP", 1)), int(os.environ.get("REPS", 5))
    assert torch.cuda.is_available(), "l2_filter_bench needs the GPU: nothing here is measured without it"
    torch.cuda.set_device(0)
    doc = {"what": "the Euclidean measures' count pass: fp64 route (K18) against the MFMA filter (K19), one MI355X",
           "config": {"warmup": warmup, "reps": reps, "timing": "device events around the calls, medians, the routes "
                      "alternating (cal_perf_embeddings: host clock)", "device": torch.cuda.get_device_name(0)}}
    if os.path.exists(a.out):  # sections measured by an earlier call are kept
        with open(a.out) as f:
            old = json.load(f)
        for k in ("speedup", "crossover", "cal_perf_embeddings"):
            if k in old:
                doc[k] = old[k]

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")

    sections = a.sections.split(",")
    if "crossover" in sections:
        bench_crossover(doc, save, [int(x) for x in a.sizes.split(",")], 1024, warmup, reps)
    if "speedup" in sections:
        n_q, n_g, d = (int(x) for x in a.shape.split(","))
        bench_speedup(doc, save, n_q, n_g, d, warmup, reps)
    if "cal_perf" in sections:
        n_c, n_v, d = (int(x) for x in a.eval_shape.split(","))
        bench_cal_perf(doc, save, n_c, n_v, d, warmup, reps)
    if sections != ["sharded"]:
        save()
    if "sharded" in sections:  # a document of its own
        sdoc = {"what": "the sharded evaluation's count pass under l2: ShardedGallery(filter=False), the fp64 route "
                        "(K18), against filter=True, cmve_l2_count_resolved (K21); world 1, one MI355X",
                "config": doc["config"]}
        if os.path.exists(a.sharded_out):  # records of an earlier build (gate_full_grid) are kept
            with open(a.sharded_out) as f:
                sdoc.update({k: v for k, v in json.load(f).items() if k not in sdoc and k.startswith("gate_")})

        def ssave():
            os.makedirs(os.path.dirname(a.sharded_out), exist_ok=True)
            with open(a.sharded_out, "w") as f:
                json.dump(sdoc, f, indent=1)
                f.write("\n")

        n_q, n_g, d = (int(x) for x in a.shape.split(","))
        bench_sharded(sdoc, ssave, n_q, n_g, d, [int(x) for x in a.sharded_sizes.split(",")], warmup, reps)


if __name__ == "__main__":
    main()
