"""Cost of the pins on a disk_patch of about 2 M facets (surface + bending, gradient descent): steps/s with the rim on
pin_to_circle (fixed mode, on the unit circle it starts on) against the same rim held by ``fixed``.  With pins every
line-search trial runs unchained (guard, trial positions, k_pin_enforce, energy) and the gradient passes through
k_pin_grad; with a fixed rim the line-search queue chains its rounds.  Prints one JSON line.  For the kernel rows run
it once more under ``rocprofv3 --kernel-trace --stats -- python tools/bench_pins.py (PYTHONPATH at the repository root) --only pinned``."""
import argparse
import json
import sys
import time

import numpy as np

from membrane_solver_amd import meshgen
from membrane_solver_amd.geometry.mesh import ArrayMesh
from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager
from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager
from membrane_solver_amd.runtime.minimizer import Minimizer
from membrane_solver_amd.runtime.steppers import GradientDescent

ap = argparse.ArgumentParser()
ap.add_argument("--rings", type=int, default=580, help="disk_patch rings (nf = 6 rings^2: 580 -> 2.0 M facets)")
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--only", choices=["pinned", "fixed"], default=None)
args = ap.parse_args()

P, T, B = meshgen.disk_patch(args.rings, jitter=0.1, seed=3)
rng = np.random.default_rng(2)
P = P.copy()
P[:, 2] += 0.002 * rng.normal(size=len(P))
rim = np.flatnonzero(B)
gp = {"surface_tension": 1.0, "bending_modulus": 1.0, "spontaneous_curvature": 0.0, "pin_to_circle_radius": 1.0}
mods = ["surface", "bending"]


def run(kind):
    if kind == "pinned":
        mesh = ArrayMesh(P, T, global_parameters=dict(gp), energy_modules=mods, constraint_modules=["pin_to_circle"],
                         vertex_options={int(i): {"constraints": ["pin_to_circle"]} for i in rim})
        cons = ["pin_to_circle"]
    else:
        mesh = ArrayMesh(P, T, fixed=B, global_parameters=dict(gp), energy_modules=mods)
        cons = []
    mz = Minimizer(mesh, mesh.global_parameters, GradientDescent(), EnergyModuleManager(mods),
                   ConstraintModuleManager(cons), energy_modules=mods, constraint_modules=cons, quiet=True,
                   step_size=1e-6)
    print("[bench_pins] %s: set-up done, warm-up" % kind, file=sys.stderr, flush=True)
    mz.minimize(args.warmup, sync_mesh=False)
    _mir, dm = mz._device()
    dm.energy()  # (a sync point before the clock starts)
    t0 = time.perf_counter()
    r = mz.minimize(args.steps, sync_mesh=False)
    dt = time.perf_counter() - t0
    it = int(mz.last_run["iterations"])
    out = {"steps_per_s": it / dt, "ms_per_step": 1e3 * dt / it, "iterations": it,
           "accepted": mz.last_run["accepted"], "trials": mz.last_run["trials"], "energy": r["energy"]}
    if kind == "pinned":
        out["pin_stats"] = dm.pin_stats()
        out["lane"] = mz.pin_tables.lane
    out["resident_steps"] = dm.resident_stats()["steps"]
    return out


res = {"workload": "disk_patch rings=%d nf=%d nv=%d rim=%d, surface + bending, GD" % (args.rings, len(T), len(P),
                                                                                      len(rim)),
       "steps": args.steps, "warmup": args.warmup}
for kind in (["pinned", "fixed"] if args.only is None else [args.only]):
    res[kind] = run(kind)
if "pinned" in res and "fixed" in res:
    res["pinned_over_fixed"] = res["pinned"]["steps_per_s"] / res["fixed"]["steps_per_s"]
print(json.dumps(res))
