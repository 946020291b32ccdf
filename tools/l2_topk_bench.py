"""The MFMA-filtered exact top-k of the Euclidean measures (K20) against the fp64 route (K18) on one GPU.  Writes one
JSON document (default profiles/l2_topk.json) and prints each row as it is measured.

  gallery_1m  top-10 under l2 and l2_norm over a resident 1,048,576 x 1024 fp64 gallery (packed once, as
              GalleryScorer does; the pack is timed on its own) at n_q = 1, 16 and 1000
  shard       16,384 captions x 131,072 videos x 1024 (the gallery_shard shape of DESIGN s6), l2
  crossover   a 16,384-row and a 131,072-row gallery, n_q from 1 to 1024: where the filter wins by more than the
              spread of the repeats sets engine.L2_TOPK_FILTER_MIN_Q / _MIN_PAIRS / _MIN_GALLERY (engine.l2_topk_auto);
              pack_gallery_s is what a gallery given as plain rows pays inside every call on top of "filter"
  clustered   rows clustered far from the origin (100 + N(0, 1): every bound is wider than every distance), 1000
              queries over 131,072 rows: what a call costs that the filter hands back whole (A, A', B, then the fp64
              route), the first call and the later ones of a GalleryScorer, which asks the filter only once

Every row times engine.pairwise_topk(filter=False) -- the parent commit's route -- and filter=True in the same
process, queries packed inside the timed call, outputs left on the device; ids AND error words must be equal.
Times are device events around the calls, medians of REPS (default 5) repeats after WARMUP (default 1), the two
routes alternating repeat by repeat.  "launches" is one more filter=True call under torch.profiler: device time by
kernel (pack = the query pack, A / B = the two MFMA passes, A' = the threshold, C = the finish)."""
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

F64 = torch.float64
MEASURES = {"l2": lambda d: (1.0, 0.0), "l2_norm": lambda d: (-1.0 / d, -1.0)}
KERNELS = (("A", ("l2t_pass_kernel<0>", "l2t_pass_kernelILi0")), ("A'", ("l2t_threshold_kernel",)),
           ("B", ("l2t_pass_kernel<1>", "l2t_pass_kernelILi1")), ("C", ("l2t_finish_kernel",)), ("pack", ("pack",)))


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


def gallery(n_g, d, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    g = torch.randn((n_g, d), device="cuda", generator=gen, dtype=F64)
    t, _ = event_time(lambda: engine.RowSet(g, with_lo=False))
    t, gs = event_time(lambda: engine.RowSet(g, with_lo=False))
    return gs, gen, t


def queries(gs, n_q, gen):
    """captions near gallery rows spread over the gallery (planted: row i * n_g / n_q + noise)"""
    rows = torch.arange(n_q, device="cuda") * (gs.n // n_q)
    return gs.raw[rows] + 0.5 * torch.randn((n_q, gs.d), device="cuda", generator=gen, dtype=F64)


def compare(gs, q, measure, k, warmup, reps, with_launches=True):
    alpha, beta = MEASURES[measure](gs.d)
    seen = {}

    def run(flt):
        seen[flt] = engine.pairwise_topk(q, gs, _lib.PW_L2, alpha, beta, F64, k, to_host=False, filter=flt,
                                         return_stats=True)

    t = {False: [], True: []}
    for r in range(warmup + reps):
        for flt in (False, True):
            s = event_time(lambda: run(flt))[0]
            if r >= warmup:
                t[flt].append(s)
    a, b = stats(t[False]), stats(t[True])
    same_ids = bool(torch.equal(seen[False][0], seen[True][0]))
    same_words = bool(torch.equal(seen[False][1].view(torch.int64), seen[True][1].view(torch.int64)))
    assert same_ids, "the filter's ids differ from the fp64 route's"
    row = {"n_q": q.shape[0], "n_g": gs.n, "d": gs.d, "measure": measure, "k": k, "fp64": a, "filter": b,
           "speedup": round(a["median_s"] / b["median_s"], 2),
           "filter_wins_beyond_spread": bool(a["median_s"] - b["median_s"] > a["spread_s"] + b["spread_s"]),
           "same_ids": same_ids, "same_words": same_words, "topk_stats": seen[True][2]}
    if with_launches:
        row["launches"] = launches(lambda: run(True))
    print(json.dumps(row), flush=True)
    return row


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "l2_topk.json"))
    ap.add_argument("--sections", default="crossover,shard,gallery_1m,clustered")
    ap.add_argument("--d", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    a = ap.parse_args(argv)
    warmup, reps = int(os.environ.get("WARMUP", 1)), int(os.environ.get("REPS", 5))
    assert torch.cuda.is_available(), "l2_topk_bench needs the GPU: nothing here is measured without it"
    torch.cuda.set_device(0)
    doc = {"what": "exact top-k under the Euclidean measures: fp64 route (K18) against the MFMA filter (K20), one MI355X",
           "config": {"warmup": warmup, "reps": reps, "k": a.k, "timing": "device events around "
                      "engine.pairwise_topk(to_host=False), medians, the routes alternating; the gallery is resident "
                      "and packed once, the queries are packed inside the timed call",
                      "device": torch.cuda.get_device_name(0),
                      "engine_L2_TOPK_FILTER_MIN_Q": engine.L2_TOPK_FILTER_MIN_Q,
                      "engine_L2_TOPK_FILTER_MIN_PAIRS": engine.L2_TOPK_FILTER_MIN_PAIRS,
                      "engine_L2_TOPK_FILTER_MIN_GALLERY": engine.L2_TOPK_FILTER_MIN_GALLERY}}
    if os.path.exists(a.out):  # sections measured by an earlier call are kept
        with open(a.out) as f:
            old = json.load(f)
        for key in ("crossover", "shard", "gallery_1m", "clustered"):
            if key in old:
                doc[key] = old[key]

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")

    sections = a.sections.split(",")
    if "crossover" in sections:
        rows = []
        for n_g, nqs in ((16384, (1, 4, 16, 64, 256, 1024)), (131072, (1, 4, 16, 64, 256))):
            gs, gen, t_pack = gallery(n_g, a.d, 20 + n_g)
            for n_q in nqs:
                rows.append(compare(gs, queries(gs, n_q, gen), "l2", a.k, warmup, reps, with_launches=False))
                rows[-1]["pack_gallery_s"] = round(t_pack, 6)
            del gs
        doc["crossover"] = rows
        save()
    if "shard" in sections:
        gs, gen, t_pack = gallery(131072, a.d, 5)
        doc["shard"] = compare(gs, queries(gs, 16384, gen), "l2", a.k, warmup, reps)
        doc["shard"]["pack_gallery_s"] = round(t_pack, 6)
        del gs
        save()
    if "gallery_1m" in sections:
        gs, gen, t_pack = gallery(1 << 20, a.d, 9)
        rows = []
        for measure in ("l2", "l2_norm"):
            for n_q in (1, 16, 1000):
                rows.append(compare(gs, queries(gs, n_q, gen), measure, a.k, warmup, reps))
        doc["gallery_1m"] = {"pack_gallery_s": round(t_pack, 6), "rows": rows}
        save()
    if "clustered" in sections:
        from cmve.linas.inference import GalleryScorer
        gen = torch.Generator(device="cuda").manual_seed(31)
        g = 100.0 + torch.randn((131072, a.d), device="cuda", generator=gen, dtype=F64)
        q = 100.0 + torch.randn((1000, a.d), device="cuda", generator=gen, dtype=F64)
        gs = engine.RowSet(g, with_lo=False)
        row = compare(gs, q, "l2", a.k, warmup, reps)  # filter=True on every repeat: the whole cost, every time
        sc = GalleryScorer(g, measure="l2")  # filter=None: the first call tries the filter, the later ones do not
        first, ids = event_time(lambda: sc.topk_indices(q, a.k))
        later = [event_time(lambda: sc.topk_indices(q, a.k))[0] for _ in range(reps)]
        ref = GalleryScorer(g, measure="l2", filter=False)
        plain = [event_time(lambda: ref.topk_indices(q, a.k))[0] for _ in range(warmup + reps)][warmup:]
        row["scorer_auto"] = {"first_call_s": round(first, 6), "later_calls": stats(later), "latched": sc._filter_off,
                              "filter_false": stats(plain),
                              "same_ids": bool((ids == ref.topk_indices(q, a.k)).all())}
        doc["clustered"] = row
        print(json.dumps(row["scorer_auto"]), flush=True)
        save()
    save()


if __name__ == "__main__":
    main()
