#!/bin/bash
# round 6: A/B of bench.py argument variants of the headline on one box, alternating, two passes:
#   AB_CFGS="name|--arg1 x --arg2 y;name2|..." (the base line is always run first in each pass)
R=${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/../.." && pwd)}
cd "$R" && mkdir -p gpurun_out/ab || exit 1
A="--full --steps 20 --warmup 5 --no-shard-leg --no-extras --no-cpu-baseline --no-replay"
IFS=';' read -ra CFGS <<< "base|;${AB_CFGS}"
for r in 1 2; do
  for v in "${CFGS[@]}"; do
    [ -z "$v" ] && continue
    n=${v%%|*}; f=${v#*|}
    timeout -k 10 150 python bench.py $A $f > gpurun_out/ab/${n}_$r.log 2>&1 || { echo "$n failed"; tail -3 gpurun_out/ab/${n}_$r.log; exit 1; }
    python3 - "$n" "$r" <<'PY'
import json, sys
n, r = sys.argv[1], sys.argv[2]
d = json.loads(open(f"gpurun_out/ab/{n}_{r}.log").read().strip().splitlines()[-1])
k = d.get("kernel_ms_isolated_batch") or {}
ki = d.get("kernel_ms_inflight") or {}
print(f"{n}: {d['value']:.4g} parity {d['recall']['parity_exact']} b2b {d['single_eval_back_to_back_ms']:.4f} "
      f"iso " + " ".join(f"{a}={b * 1e3:.1f}" for a, b in k.items()) + " | inflight " +
      " ".join(f"{a}={b * 1e3:.1f}" for a, b in ki.items()))
PY
  done
done
