#!/usr/bin/env python3
"""Compare the register / scratch / occupancy figures of two builds of the device code.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=fast -Iinclude -Imembrane_solver_amd/csrc \\
        -Rpass-analysis=kernel-resource-usage -c membrane_solver_amd/csrc/ms_kernels.hip -o /dev/null 2> new.log
    python3 tools/kernel_resources.py old.log new.log [--filter k_energy,k_gradient] [--all]

Parses the compiler's kernel-resource-usage remarks of both logs and prints, per kernel instantiation (demangled with
c++filt when it is installed), the rows whose VGPRs, scratch bytes or waves/SIMD differ, the instantiations only one
log has, and a verdict: it FAILS (exit status 1) when an instantiation present in both logs -- restricted to --filter
-- has more scratch in the new log than in the old one or fewer waves/SIMD.  --all prints every common row.
"""

from __future__ import annotations

import argparse
import re
import shutil
import subprocess
import sys

# (the compiler puts "file:line:col: " between "remark:" and the text when the build carries line information)
_NAME = re.compile(r"remark: (?:\S+:\d+:\d+: +)?Function Name: (\S+)")
_FIELD = re.compile(r"remark:\s+(?:\S+:\d+:\d+:\s+)?(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|"
                    r"LDS Size \[bytes/block\]|TotalSGPRs|VGPRs Spill|SGPRs Spill): (\d+)")
_KEYS = {"VGPRs": "vgpr", "AGPRs": "agpr", "ScratchSize [bytes/lane]": "scratch", "Occupancy [waves/SIMD]": "waves",
         "LDS Size [bytes/block]": "lds", "TotalSGPRs": "sgpr", "VGPRs Spill": "vspill", "SGPRs Spill": "sspill"}


def parse(path):
    """-> {mangled kernel name: {vgpr, agpr, scratch, waves, lds, sgpr, vspill, sspill}}"""
    out, cur = {}, None
    with open(path, errors="replace") as fh:
        for line in fh:
            m = _NAME.search(line)
            if m:
                cur = out.setdefault(m.group(1), {})
                continue
            m = _FIELD.search(line)
            if m and cur is not None:
                cur[_KEYS[m.group(1)]] = int(m.group(2))
    return out


def demangle(names):
    names = list(names)
    tool = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not tool or not names:
        return {n: n for n in names}
    res = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=False)
    lines = res.stdout.splitlines()
    if len(lines) != len(names):
        return {n: n for n in names}
    short = {}
    for n, d in zip(names, lines):
        d = re.sub(r"^void ", "", d)
        d = re.sub(r"\(.*\)$", "", d).replace("ms::", "").replace("(anonymous namespace)::", "")
        d = re.sub(r"\((bool|int)\)", "", d).replace(", ", ",")
        short[n] = d
    return short


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--filter", default="k_energy,k_gradient",
                    help="comma-separated substrings of the demangled names the verdict covers ('' = every kernel)")
    ap.add_argument("--all", action="store_true", help="print every common instantiation, not only the changed ones")
    args = ap.parse_args(argv)
    old, new = parse(args.old), parse(args.new)
    names = demangle(sorted(set(old) | set(new)))
    wanted = [s for s in args.filter.split(",") if s]

    def covered(n):
        return not wanted or any(s in names[n] for s in wanted)

    common = [n for n in sorted(old, key=lambda n: names[n]) if n in new and covered(n)]
    bad, changed = [], 0
    print("%-64s %11s %11s %11s" % ("instantiation", "VGPRs", "scratch", "waves/SIMD"))
    for n in common:
        o, w = old[n], new[n]
        diff = any(o.get(k) != w.get(k) for k in ("vgpr", "scratch", "waves"))
        worse = w.get("scratch", 0) > o.get("scratch", 0) or w.get("waves", 0) < o.get("waves", 0)
        if worse:
            bad.append(names[n])
        if diff:
            changed += 1
        if diff or args.all:
            print("%-64s %4d -> %4d %4d -> %4d %4d -> %4d%s" % (names[n], o.get("vgpr", -1), w.get("vgpr", -1),
                                                             o.get("scratch", -1), w.get("scratch", -1),
                                                             o.get("waves", -1), w.get("waves", -1),
                                                             "   <-- WORSE" if worse else ""))
    for n in sorted(set(new) - set(old), key=lambda n: names[n]):
        if covered(n):
            w = new[n]
            print("%-64s    new: %4d        %4d        %4d" % (names[n], w.get("vgpr", -1), w.get("scratch", -1),
                                                             w.get("waves", -1)))
    for n in sorted(set(old) - set(new), key=lambda n: names[n]):
        if covered(n):
            print("%-64s    gone" % names[n])
    print("%d instantiations in both logs, %d with different VGPRs / scratch / occupancy, %d with more scratch or lower "
          "occupancy" % (len(common), changed, len(bad)))
    print("FAIL: " + ", ".join(bad) if bad else "OK")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
