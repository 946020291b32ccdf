"""The SAD-filtered count pass under jaccard (K24) against the K18 route on one GPU.  Writes one JSON document (default
profiles/jaccard_filter.json) and prints each section as it is measured.

  headline   16,384 captions x 131,072 videos x 1024 (the shape of DESIGN s6), jaccard as evaluation.py scores it
             (alpha = -1, float32 words), non-negative float32 rows resident on the device, planted GTs (caption =
             |its video + 0.5 N(0, 1)|):
               call      one engine.pairwise_gt_eval(..., filter=False / "jaccard") -- lists in, positions and ranks out
               launches  the device work alone: K18 route = both item launches + cmve_pairwise_count; filter route =
                         grid, pack A, pack B, row sums A, row sums B (each listed), both item launches,
                         cmve_jaccard_count
  sad_rate   cmve_jaccard_count at the headline shape with NaN item words: every pair with an interval is decided
             not-below, the fix-up and the gated launches do nothing -- the main kernel (K loop + epilogue) alone.
             Its SAD lane-instructions per second, na_pad * nb_pad * d_pad / 2 over that time, beside K22's (the same
             K loop: profiles/l1_filter.json) and the ceiling a full-rate 32-bit VALU op would have: 256 CUs x 4 SIMDs
             x 16 lanes x 2.4 GHz = 3.9e13.
  crossover  both routes at na = nb in {256 .. 16384}, D = 1024, one pairwise_gt_eval each: the smallest size at
             which the filter wins by more than the two routes' combined spread would set
             engine.JACCARD_FILTER_MIN_PAIRS

filter=False is the only baseline; the words are checked equal in every row.  Times are device events around the
calls, medians of REPS (default 5) repeats after WARMUP (default 1), the two routes alternating repeat by repeat."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "cross-modal-video-engine_amd"), ROOT, os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from cmve import _lib, engine  # noqa: E402
from cmve._lib import lib, check  # noqa: E402
from l2_filter_bench import alternate, event_time, stage_times, stats  # noqa: E402

F32, F64 = torch.float32, torch.float64
J = _lib.PW_JACCARD
ALPHA, BETA = -1.0, 0.0
SAD_CEILING = 256 * 4 * 16 * 2.4e9
K22_SAD_RATE = 3.16e13  # profiles/l1_filter.json: the identical K loop under l1f_main_kernel's epilogue


def wins(a, b):
    return bool(a["median_s"] - b["median_s"] > a["spread_s"] + b["spread_s"])


def planted(n_q, n_g, d, seed, noise=0.5):
    """non-negative float32 rows, caption i planted on video i"""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    gal = torch.randn((n_g, d), device="cuda", generator=gen, dtype=F32).abs_()
    q = (gal[:n_q] + noise * torch.randn((n_q, d), device="cuda", generator=gen, dtype=F32)).abs_()
    rows = [[i] for i in range(n_q)]
    cols = [[j] if j < n_q else [] for j in range(n_g)]
    return q, gal, rows, cols


def bench_headline(doc, save, n_q, n_g, d, warmup, reps):
    q, gal, rows, cols = planted(n_q, n_g, d, 5)
    dev = q.device
    holder = {}

    def call(flt):
        holder[flt] = engine._PairwisePositions(q, gal, J, ALPHA, BETA, F32, rows, cols, filter=flt)
        return holder[flt]

    t = alternate({"k18": lambda: call(False), "filter": lambda: call("jaccard")}, warmup, reps)
    same = all(np.array_equal(holder["jaccard"].pos[s], holder[False].pos[s]) for s in (0, 1))
    st = holder["jaccard"].filter_stats
    a, b = stats(t["k18"]), stats(t["filter"])
    res = {"n_q": n_q, "n_g": n_g, "d": d, "measure": "jaccard", "alpha": ALPHA, "beta": BETA,
           "rows": "float32, non-negative, planted GTs",
           "call": {"k18": a, "filter": b, "speedup": round(a["median_s"] / b["median_s"], 2),
                    "filter_wins_beyond_both_spreads": wins(a, b)},
           "same_words": bool(same), "filter_stats": st, "band_share": st["band"] / float(n_q * n_g)}
    holder.clear()
    # the launches alone
    roff, ridx = engine.csr(rows, dev)
    coff, cidx = engine.csr(cols, dev)
    ri, ci = n_q, n_q
    h = engine.handle(dev)

    def k18_step():
        r_sc = engine.pairwise_item_scores(q, gal, J, ALPHA, BETA, F32, roff, ridx, ri, False, 0)
        c_sc = engine.pairwise_item_scores(q, gal, J, ALPHA, BETA, F32, coff, cidx, ci, True, 0)
        return engine.pairwise_count(q, gal, J, ALPHA, BETA, F32, (roff, r_sc, n_g), (coff, c_sc, n_q), filter=False)

    grid = engine.l1_grid(gal, engine.l1_grid(q))
    sa, sb = engine.JaccardSet(q, grid=grid), engine.JaccardSet(gal, grid=grid)
    band = torch.empty(engine.l2_band_cap(n_q * n_g), dtype=torch.int64, device=dev)
    cnt = torch.empty(4, dtype=torch.int64, device=dev)
    rpos = torch.empty(ri, dtype=torch.int32, device=dev)
    cpos = torch.empty(ci, dtype=torch.int32, device=dev)
    sc = {}

    def make_grid():
        engine.l1_grid(gal, engine.l1_grid(q))

    def pack(s):
        check(lib.cmve_l1_pack(h, engine._ptr(s.raw), _lib.CMVE_F32, s.raw.stride(0), s.n, s.d, engine._ptr(grid),
                               engine._ptr(s.codes), s.n_pad, s.d_pad, engine._ptr(s.err)), "cmve_l1_pack")

    def rowsums(s):
        check(lib.cmve_jaccard_rowsums(h, engine._ptr(s.raw), _lib.CMVE_F32, s.raw.stride(0), s.n, s.d,
                                       engine._ptr(grid), s.n_pad, s.d_pad, engine._ptr(s.qsum), engine._ptr(s.asum)),
              "cmve_jaccard_rowsums")

    def items():
        sc["r"] = engine.pairwise_item_scores(q, gal, J, ALPHA, BETA, F32, roff, ridx, ri, False, 0)
        sc["c"] = engine.pairwise_item_scores(q, gal, J, ALPHA, BETA, F32, coff, cidx, ci, True, 0)

    def count(r_sc, c_sc):
        engine._jaccard_count_call(h, sa, sb, ALPHA, BETA, (roff, r_sc, ri, n_g, rpos), (coff, c_sc, ci, n_q, cpos),
                                   band, 8 * band.numel(), cnt)

    nan_r = torch.full((ri,), float("nan"), dtype=F64, device=dev)
    nan_c = torch.full((ci,), float("nan"), dtype=F64, device=dev)
    stages = [("grid_both_sets", make_grid), ("pack_captions", lambda: pack(sa)), ("pack_videos", lambda: pack(sb)),
              ("rowsums_captions", lambda: rowsums(sa)), ("rowsums_videos", lambda: rowsums(sb)),
              ("item_scores", items), ("jaccard_count", lambda: count(sc["r"], sc["c"])),
              ("jaccard_count_main_kernel_only", lambda: count(nan_r, nan_c))]
    per = {name: [] for name, _ in stages}
    step, nan_stats = [], None
    for r in range(warmup + reps):
        ts = event_time(k18_step)[0]
        tt = stage_times(stages)
        nan_stats = engine._l2_count_stats(cnt.cpu().numpy())
        if r >= warmup:
            step.append(ts)
            for k, v in tt.items():
                per[k].append(v)
    med = {k: statistics.median(v) for k, v in per.items()}
    parts = ("grid_both_sets", "pack_captions", "pack_videos", "rowsums_captions", "rowsums_videos", "item_scores",
             "jaccard_count")
    filt = sum(med[k] for k in parts)
    res["launches"] = {
        "k18_item_scores_and_count": stats(step),
        "filter": {k: stats(v) for k, v in per.items()},
        "filter_band_rescore_s": round(med["jaccard_count"] - med["jaccard_count_main_kernel_only"], 6),
        "filter_total_s": round(filt, 6),
        "filter_total_resident_gallery_s": round(filt - med["pack_videos"] - med["rowsums_videos"], 6),
        "speedup": round(statistics.median(step) / filt, 2)}
    sads = sa.n_pad * sb.n_pad * sa.d_pad / 2.0
    rate = sads / med["jaccard_count_main_kernel_only"]
    res["sad_rate"] = {
        "what": "cmve_jaccard_count with NaN item words (fix-up and gated launches idle): K loop + epilogue",
        "stats_of_that_call": nan_stats, "seconds": stats(per["jaccard_count_main_kernel_only"]),
        "sad_lane_instructions": sads, "sad_lane_instructions_per_s": rate,
        "k22_sad_lane_instructions_per_s": K22_SAD_RATE, "share_of_k22": round(rate / K22_SAD_RATE, 3),
        "ceiling_full_rate_valu": SAD_CEILING, "share_of_ceiling": round(rate / SAD_CEILING, 3)}
    doc["headline"] = res
    save()
    print(json.dumps(res), flush=True)


def bench_crossover(doc, save, sizes, d, warmup, reps):
    table, chosen = [], None
    for n in sizes:
        q, gal, rows, cols = planted(n, n, d, 7 + n)
        last = {}

        def run(flt):
            last[flt] = engine.pairwise_gt_eval(q, gal, J, ALPHA, BETA, F32, rows, cols, flt)

        t = alternate({"k18": lambda: run(False), "filter": lambda: run("jaccard")}, warmup, reps)
        same = all(np.array_equal(x, y) for s in (0, 1) for x, y in zip(last[False][s][0], last["jaccard"][s][0])) and \
            all(np.array_equal(last[False][s][1], last["jaccard"][s][1]) for s in (0, 1))
        a, b = stats(t["k18"]), stats(t["filter"])
        w = wins(a, b)
        table.append({"na": n, "nb": n, "d": d, "k18": a, "filter": b, "same_words": bool(same),
                      "filter_wins_beyond_both_spreads": w})
        if w and chosen is None:
            chosen = n
        if not w:  # a size that loses after one that won: the threshold is the first size from which every one wins
            chosen = None
        print(json.dumps(table[-1]), flush=True)
    doc["crossover"] = {"table": table, "smallest_size_from_which_every_size_wins": chosen,
                        "min_pairs": None if chosen is None else chosen * chosen,
                        "engine_JACCARD_FILTER_MIN_PAIRS": engine.JACCARD_FILTER_MIN_PAIRS}
    save()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jaccard_filter.json"))
    ap.add_argument("--sections", default="crossover,headline")
    ap.add_argument("--shape", default="16384,131072,1024")
    ap.add_argument("--sizes", default="256,512,1024,2048,4096,8192,16384")
    a = ap.parse_args(argv)
    warmup, reps = int(os.environ.get("WARMUP", 1)), int(os.environ.get("REPS", 5))
    assert torch.cuda.is_available(), "jaccard_filter_bench needs the GPU: nothing here is measured without it"
    torch.cuda.set_device(0)
    doc = {"what": "jaccard's count pass: K18 route against the integer SAD filter (K24), one MI355X",
           "config": {"warmup": warmup, "reps": reps, "timing": "device events around the calls, medians, the routes "
                      "alternating", "device": torch.cuda.get_device_name(0)}}
    if os.path.exists(a.out):  # sections measured by an earlier call are kept
        with open(a.out) as f:
            old = json.load(f)
        for k in ("headline", "crossover"):
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
    if "headline" in sections:
        n_q, n_g, d = (int(x) for x in a.shape.split(","))
        bench_headline(doc, save, n_q, n_g, d, warmup, reps)
    save()


if __name__ == "__main__":
    main()
