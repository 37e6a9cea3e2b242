"""Cost of the tilt_rim_source_bilayer lane: the nested leaflet relaxation of the bilayer-source deck
(tests/golden/rim_bilayer_relax.npz: 84 vertices, 12 rim edges, gamma 50, its pins; tilt_inner_steps as the fixture caps
them), median of repeated runs after warm-up.

    python3 tools/bench_rim_bilayer.py --lane bilayer              # this tree, the module itself
    python3 tools/bench_rim_bilayer.py --lane pair --root PARENT   # another checkout of the project (the parent commit):
                                                                   # tilt_rim_source_in + _out with equal parameters

The two lanes are the same physics (the reference's docstring; tools/gen_golden_rim_bilayer.py asserts it), so ``pair`` on
the parent commit is the baseline the bilayer lane is compared with: run the two alternately in one session, a fresh
process each, and compare the medians with the baseline's own run-to-run range.  Every relaxation starts from the
fixture's initial tilts (re-uploaded outside the timed window).  Prints one JSON line with the median, the range and the
rim kernels' launches per evaluation (not the bench contract: bench.py stays the headline metric)."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--lane", choices=["bilayer", "pair"], default="bilayer")
ap.add_argument("--root", default=HERE, help="checkout whose membrane_solver_amd is imported and timed")
ap.add_argument("--runs", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))

from membrane_solver_amd.geometry.mesh import ArrayMesh  # noqa: E402
from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager  # noqa: E402
from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager  # noqa: E402
from membrane_solver_amd.runtime.minimizer import Minimizer  # noqa: E402
from membrane_solver_amd.runtime.steppers import GradientDescent  # noqa: E402

g = dict(np.load(os.path.join(HERE, "tests", "golden", "rim_bilayer_relax.npz"), allow_pickle=False))
gp = json.loads(str(g["gp_json"]))
mods = [str(m) for m in g["modules"]]
if args.lane == "pair":
    mods = [m for m in mods if m != "tilt_rim_source_bilayer"] + ["tilt_rim_source_in", "tilt_rim_source_out"]
    for key in ("group", "strength"):
        val = gp.pop("tilt_rim_source_" + key)
        gp["tilt_rim_source_%s_in" % key] = gp["tilt_rim_source_%s_out" % key] = val
cons = [str(m) for m in g["constraint_modules"]]
mesh = ArrayMesh(g["positions"], g["tri"], fixed=g["fixed"], tilts_in=g["tilts_in0"], tilts_out=g["tilts_out0"],
                 tilt_fixed_in=g["tilt_fixed_in"], tilt_fixed_out=g["tilt_fixed_out"], global_parameters=gp,
                 energy_modules=mods, constraint_modules=cons, edges=g["edges"],
                 vertex_options={int(k): v for k, v in json.loads(str(g["vopts"])).items()})
mz = Minimizer(mesh, mesh.global_parameters, GradientDescent(), EnergyModuleManager(mods), ConstraintModuleManager(cons),
               quiet=True)
mir, dm = mz._device()
rp = mz._tilt_relax_params()


def launches():
    if args.lane == "bilayer":
        return np.array(list(dm.rim_source_bilayer_stats().values()), dtype=float)
    return sum(np.array(list(dm.leaflet_rim_source_stats(lf).values()), dtype=float) for lf in ("in", "out"))


times, evals, per_eval = [], 0, None
for k in range(args.warmup + args.runs):
    mir._leaflet_keys.pop("in", None)
    mir._leaflet_keys.pop("out", None)
    mz._device()  # the initial tilts again
    dm.fetch_scalars()
    before = launches()
    t0 = time.perf_counter()
    _it, evals = dm.relax_leaflet_tilts(**rp)
    dt = time.perf_counter() - t0
    per_eval = (launches() - before) / max(evals, 1)
    if k >= args.warmup:
        times.append(dt)
E = float(dm.energy().sum())
print(json.dumps({"lane": args.lane, "root": os.path.relpath(os.path.abspath(args.root), HERE), "median_s": float(np.median(times)),
                  "min_s": float(np.min(times)), "max_s": float(np.max(times)), "runs": args.runs, "evaluations": int(evals),
                  "rim_launches_per_evaluation": {"frame": per_eval[0], "coef": per_eval[1], "apply": per_eval[2]},
                  "E_total": E, "E_total_reference": float(g["E_total"])}), flush=True)
