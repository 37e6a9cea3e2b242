#!/bin/bash
# A/B a set of alternative library builds (build_variants/lib_*.so, e.g. different occupancy
# attributes) on the headline bench: prints steps/s and per-kernel HIP-event averages.
O=$(mktemp -d)
for so in "" build_variants/lib_*.so; do
  name=${so:-default}
  MEMBRANE_HIP_LIB=${so:+$PWD/$so} python bench.py --full --cpu-steps 0 "$@" > $O/ab.json 2> $O/ab.err || { echo "$name FAILED"; tail -n 3 $O/ab.err; continue; }
  python - "$name" "$O/ab.json" <<'PY'
import json, sys
d = json.load(open(sys.argv[2]))
print(sys.argv[1], round(d["value"]), round(d.get("deterministic_mode", {}).get("value", 0)),
      {n: round(v["avg_us"], 1) for n, v in d["kernels"].items()})
PY
done
