"""The SAD-filtered exact top-k under jaccard (K25) against the K18 route on one GPU.  Writes one JSON document (default
profiles/jaccard_topk.json) and prints each row as it is measured.

  topk     top-10 under -jaccard (alpha = -1, float32 words) over non-negative float32 rows, D = 1024: n_q in {1, 64,
           1000} over 131,072 and 1,048,576 gallery rows, and 16,384 x 131,072 (the gallery_shard shape of DESIGN s6).
           Every shape runs twice: with the gallery RESIDENT (an engine.JaccardSet packed once, as GalleryScorer and
           the sharded gallery hold it; the pack is timed on its own) and as PLAIN rows (grid, both packs and both row
           sums inside every timed call).
  sharded  one MeasureShardedGallery(measure='jaccard').evaluate_device at 16,384 x 131,072 (a world of one),
           filter="jaccard" (K24's count over the resident pack) against filter=False.

Every row times engine.pairwise_topk(filter=False) -- the parent commit's route, the only baseline -- and
filter="jaccard" in the same process, outputs left on the device; ids AND error words must be equal, and the row says
so.  Times are device events around the calls, medians of REPS (default 5) repeats after WARMUP (default 1), none
dropped, the two routes alternating repeat by repeat; "spread_s" is max - min of the repeats.  "launches" is one more
filter="jaccard" call under torch.profiler: device time by kernel (pack = grid + query pack + row sums, A / B = the two
SAD passes, A' = the threshold, C = the finish); "sad_rate" is launch B's ceil128(n_q) * n_g * (d / 2)
lane-instructions over its time, and its share of the 3.16e13 / s that K22's count kernel reaches
(profiles/l1_filter.json)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "cross-modal-video-engine_amd"), ROOT):
    sys.path.insert(0, p)
import torch  # noqa: E402

from cmve import _lib, engine  # noqa: E402

F32 = torch.float32
ROUTE = "jaccard"
SAD_RATE = 3.16e13  # K22's measured v_sad_u16 lane-instructions per second
KERNELS = (("A", ("jact_pass_kernel<0>", "jact_pass_kernelILi0")), ("A'", ("jact_threshold_kernel",)),
           ("B", ("jact_pass_kernel<1>", "jact_pass_kernelILi1")), ("C", ("l2t_finish_kernel",)),
           ("pack", ("l1f_pack", "l1f_grid", "jacf_rowsums")))
AUTO = ("JACCARD_TOPK_FILTER_MIN_Q", "JACCARD_TOPK_FILTER_MIN_PAIRS", "JACCARD_TOPK_FILTER_MIN_GALLERY",
        "JACCARD_TOPK_FILTER_MIN_PLAIN_PAIRS")


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


def launches(fn):
    """device seconds by launch of one call, from the profiler's kernel records (None if it records none)"""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            fn()
            torch.cuda.synchronize()
        out, other = {name: 0.0 for name, _ in KERNELS}, 0.0
        for ev in prof.events():
            if str(ev.device_type).endswith("CUDA") and ev.name and not ev.name.startswith("Memcpy"):
                dur = getattr(ev, "device_time", None) or getattr(ev, "cuda_time", 0.0)
                for name, keys in KERNELS:
                    if any(key in ev.name for key in keys):
                        out[name] += dur / 1e6
                        break
                else:
                    other += dur / 1e6
        out["other"] = other
        return {k: round(v, 6) for k, v in out.items()} if sum(out.values()) > 0 else None
    except Exception as e:  # the profiler is a convenience of the tool, not of the product
        return {"error": repr(e)}


def gallery(n_g, d, gen):
    """non-negative float32 rows: the measure's natural inputs"""
    return torch.randn((n_g, d), device="cuda", generator=gen, dtype=F32).abs_()


def queries(g, n_q, gen):
    """captions near gallery rows spread over the gallery (planted: |row i * n_g / n_q + noise|)"""
    rows = torch.arange(n_q, device="cuda") * (g.shape[0] // n_q)
    return (g[rows] + 0.5 * torch.randn((n_q, g.shape[1]), device="cuda", generator=gen, dtype=F32)).abs_()


def compare(g_op, q, form, k, warmup, reps):
    """g_op: an engine.JaccardSet (resident) or the plain rows; form: the row's label"""
    d = q.shape[1]
    n_g = g_op.n if isinstance(g_op, engine.JaccardSet) else g_op.shape[0]
    seen = {}

    def run(flt):
        seen[flt] = engine.pairwise_topk(q, g_op, _lib.PW_JACCARD, -1.0, 0.0, F32, k, to_host=False, filter=flt,
                                         return_stats=True)

    t = {False: [], ROUTE: []}
    for r in range(warmup + reps):
        for flt in (False, ROUTE):
            s = event_time(lambda: run(flt))[0]
            if r >= warmup:
                t[flt].append(s)
    a, b = stats(t[False]), stats(t[ROUTE])
    same_ids = bool(torch.equal(seen[False][0], seen[ROUTE][0]))
    same_words = bool(torch.equal(seen[False][1].view(torch.int64), seen[ROUTE][1].view(torch.int64)))
    st = seen[ROUTE][2]
    row = {"n_q": q.shape[0], "n_g": n_g, "d": d, "measure": "jaccard", "k": k, "gallery": form, "k18": a,
           "filter": b, "speedup": round(a["median_s"] / b["median_s"], 2),
           "filter_wins_beyond_spread": bool(a["median_s"] - b["median_s"] > a["spread_s"] + b["spread_s"]),
           "same_ids": same_ids, "same_words": same_words, "topk_stats": st,
           "candidates_per_query": round(st["candidates"] / max(q.shape[0] - st["unresolved"], 1), 2),
           "unresolved": st["unresolved"]}
    row["launches"] = launches(lambda: run(ROUTE))
    if isinstance(row["launches"], dict) and row["launches"].get("B"):
        lane = -(-q.shape[0] // 128) * 128 * n_g * (d / 2)
        row["launch_B_s"] = row["launches"]["B"]
        row["sad_rate"] = float("%.4g" % (lane / row["launches"]["B"]))
        row["sad_rate_share"] = round(lane / row["launches"]["B"] / SAD_RATE, 3)
    print(json.dumps(row), flush=True)
    assert same_ids and same_words, "the filter's ids or words differ from the K18 route's"
    return row


def sharded(n_q, n_g, d, warmup, reps):
    from cmve import dist as D
    gen = torch.Generator(device="cuda").manual_seed(7)
    g = gallery(n_g, d, gen)
    q = queries(g, n_q, gen)
    step = n_g // n_q
    rows = [[i * step] for i in range(n_q)]
    cols = [[j // step] if j % step == 0 else [] for j in range(n_g)]
    out, t = {}, {False: [], ROUTE: []}
    sh = {flt: D.ShardedGallery(g, offset=0, n_global=n_g, measure="jaccard", filter=flt) for flt in (False, ROUTE)}
    csr = {flt: (s.local_gt_csr(rows), s.local_v2t_csr(cols)) for flt, s in sh.items()}
    for r in range(warmup + reps):
        for flt in (False, ROUTE):
            s, (row_csr, col_csr) = sh[flt], csr[flt]
            sec, res = event_time(lambda: s.evaluate_device(q, row_csr, col_csr, n_q))
            out[flt] = res
            if r >= warmup:
                t[flt].append(sec)
    a, b = stats(t[False]), stats(t[ROUTE])
    same = all(bool(torch.equal(x, y)) for x, y in zip(out[False][:3], out[ROUTE][:3]))
    row = {"n_q": n_q, "n_g": n_g, "d": d, "measure": "jaccard",
           "what": "MeasureShardedGallery.evaluate_device, world 1", "k18": a, "filter": b,
           "speedup": round(a["median_s"] / b["median_s"], 2),
           "filter_wins_beyond_spread": bool(a["median_s"] - b["median_s"] > a["spread_s"] + b["spread_s"]),
           "same_ranks": same, "filter_stats": sh[ROUTE].filter_stats}
    print(json.dumps(row), flush=True)
    assert same, "the filtered evaluation's ranks differ from the K18 route's"
    return row


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jaccard_topk.json"))
    ap.add_argument("--sections", default="topk_131072,topk_1048576,sharded")
    ap.add_argument("--d", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    a = ap.parse_args(argv)
    warmup, reps = int(os.environ.get("WARMUP", 1)), int(os.environ.get("REPS", 5))
    assert torch.cuda.is_available(), "jaccard_topk_bench needs the GPU: nothing here is measured without it"
    torch.cuda.set_device(0)
    doc = {"what": "exact top-k under jaccard (float32 words): K18 route against the SAD filter (K25), one MI355X",
           "config": dict({"warmup": warmup, "reps": reps, "k": a.k, "d": a.d, "timing": "device events around "
                           "engine.pairwise_topk(to_host=False), medians of the repeats (none dropped), the routes "
                           "alternating; resident: the gallery is a JaccardSet packed once and the queries are packed "
                           "on its grid inside the timed call; plain: grid, both packs and row sums inside the timed "
                           "call", "rows": "non-negative float32 (|N(0, 1)|), queries planted near gallery rows",
                           "device": torch.cuda.get_device_name(0), "sad_rate_ceiling": SAD_RATE},
                          **{"engine_" + n: getattr(engine, n) for n in AUTO})}
    keys = ("topk_131072", "topk_1048576", "sharded")
    if os.path.exists(a.out):  # sections measured by an earlier call are kept
        with open(a.out) as f:
            old = json.load(f)
        for key in keys:
            if key in old:
                doc[key] = old[key]

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")

    sections = a.sections.split(",")
    for n_g, nqs in ((131072, (1, 64, 1000, 16384)), (1 << 20, (1, 64, 1000))):
        key = "topk_%d" % n_g
        if key not in sections:
            continue
        gen = torch.Generator(device="cuda").manual_seed(20 + n_g)
        g = gallery(n_g, a.d, gen)
        event_time(lambda: engine.JaccardSet(g))
        t_pack, gs = event_time(lambda: engine.JaccardSet(g))
        rows = []
        for n_q in nqs:
            q = queries(g, n_q, gen)
            rows.append(compare(gs, q, "resident", a.k, warmup, reps))
            rows.append(compare(g, q, "plain", a.k, warmup, reps))
        doc[key] = {"pack_gallery_s": round(t_pack, 6), "rows": rows}
        del gs, g
        save()
    if "sharded" in sections:
        doc["sharded"] = sharded(16384, 131072, a.d, warmup, reps)
        save()
    save()


if __name__ == "__main__":
    main()
