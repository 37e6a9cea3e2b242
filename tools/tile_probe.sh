#!/bin/bash
# generic (runtime tile size) instances at three tile sizes, next to the default T = 256 instances
O=$(mktemp -d)
for cfg in "X=1 --tile 256" "MS_NO_FAST=1 --tile 256" "MS_NO_FAST=1 --tile 512" "MS_NO_FAST=1 --tile 128"; do
  e=${cfg%% *}; a=${cfg#* }
  env $e python bench.py --full --cpu-steps 0 --headline-only --steps 200 --warmup 30 $a > $O/tp.json 2> $O/tp.err || { echo "$cfg FAILED"; tail -n 3 $O/tp.err; continue; }
  python - "$cfg" "$O/tp.json" <<'PY'
import json, sys
d = json.load(open(sys.argv[2]))
print(f"{sys.argv[1]:28s} {d['value']:8.0f} steps/s  acc {d['steps_accepted']} trials {d['line_search_trials']} ",
      {n: round(v["avg_us"], 1) for n, v in d["kernels"].items()})
PY
done
