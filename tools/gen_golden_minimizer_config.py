#!/usr/bin/env python3
"""Record what Minimizer._device() and compute_energy_breakdown() do, on the CPU, under the recording stub: the cases and
the recording are tests/minimizer_config_cases.py; this writes tests/golden/minimizer_config_log.json.

The file is a characterisation of one commit: run this on a checkout of the commit whose behaviour is to be kept (with
this tool, tests/minimizer_stub.py and tests/minimizer_config_cases.py copied into it) and commit the output next to the
change.  tests/test_minimizer_config_host.py then compares the code under test with that record, never with itself.

    python tools/gen_golden_minimizer_config.py [--out tests/golden/minimizer_config_log.json]
"""

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "minimizer_config_log.json"))
    args = ap.parse_args()
    import minimizer_config_cases as cases

    rec = cases.record_all()
    with open(args.out, "w") as fh:  # one line per case
        sections = []
        for sec in sorted(rec):
            rows = [json.dumps(n) + ": " + json.dumps(rec[sec][n], sort_keys=True, separators=(",", ":")) for n in sorted(rec[sec])]
            sections.append(json.dumps(sec) + ": {\n" + ",\n".join(rows) + "\n}")
        fh.write("{\n" + ",\n".join(sections) + "\n}\n")
    print(f"{args.out}: {len(rec['config'])} configurations, {len(rec['errors'])} refusals, "
          f"{len(rec['breakdown'])} breakdowns, {os.path.getsize(args.out)} bytes")
    for name, err in rec["errors"].items():
        print(f"  {name}: {err['type']}: {(err['message'] or '')[:90]}")


if __name__ == "__main__":
    main()
