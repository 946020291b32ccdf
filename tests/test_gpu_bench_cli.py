"""bench.py as the driver runs it: a plain run is the headline alone (no leg, roofline or CPU baseline in its line),
--steps sets the timed steps, and --dump-outputs writes the last timed step's evaluations -- ranks that agree with
their own R@K / rank sums and, for input set 0, with the reference's golden ranks."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs(tmp_path, golden):
    steps, per_step = 3, 64  # 192 evaluations: every one of the 24 input sets is in the last step
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", "1", "--evals-per-step", str(per_step), "--dump-outputs", str(tmp_path / "out")],
                       cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == steps and line["config"]["evaluations_timed"] == steps * per_step
    assert line["unit"] == "pairs/s" and line["higher_is_better"] is True and line["dtype"] == "f16"
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(1e6 * per_step / (line["ms_per_step"] * 1e-3), rel=1e-9)
    assert line["recall"]["parity_exact"] is True
    for key in ("roofline", "cpu_baseline", "gallery_shard", "gallery_1m", "c3_sharded", "single_set_replay",
                "kernel_ms_isolated_batch", "inference_topk"):
        assert key not in line, f"{key} belongs to --full"
    files = sorted(os.listdir(tmp_path / "out"))
    assert files == ["input_set.npy", "recall_rank_sums.npy", "t2v_ranks.npy", "v2t_ranks.npy"]
    arr = {f[:-4]: np.load(tmp_path / "out" / f) for f in files}
    assert all(a.dtype == np.float64 for a in arr.values())
    assert sum(a.nbytes for a in arr.values()) <= 64 << 20
    t2v, v2t, sums, sets = arr["t2v_ranks"], arr["v2t_ranks"], arr["recall_rank_sums"], arr["input_set"]
    assert t2v.shape == (per_step, 1000) and v2t.shape == (per_step, 1000) and sets.shape == (per_step,)
    exp = np.stack([(t2v <= 1).sum(1), (t2v <= 5).sum(1), (t2v <= 10).sum(1), t2v.sum(1),
                    (v2t <= 1).sum(1), (v2t <= 5).sum(1), (v2t <= 10).sum(1), v2t.sum(1)], 1)
    assert np.array_equal(sums, exp)
    assert set(sets.astype(int).tolist()) == set(range(24))
    gold = golden("retrieval_c1")
    first = {}
    for i, j in enumerate(sets.astype(int).tolist()):  # one input set -> one answer; set 0 -> the golden ranks
        k = first.setdefault(j, i)
        assert np.array_equal(t2v[i], t2v[k]) and np.array_equal(v2t[i], v2t[k])
    assert np.array_equal(t2v[first[0]], gold["t2v_ranks"]) and np.array_equal(v2t[first[0]], gold["v2t_ranks"])
