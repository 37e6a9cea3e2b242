"""Cost of the enforce-only constraints on the line search's enforcer lane: steps/s of surface + bending (CG) on an open
disk of about 2 M facets with no constraint module, with the rim loop held by ``perimeter``, and with ``fixed_plane``
-- the three configurations alternating in ONE process, same steps and warm-up -- and the trials each ran.  The two
kernels' own times come from a separate run of this script under ``rocprofv3 --kernel-trace --stats`` (k_fixed_plane moves
49 B per vertex: 48 B of positions read and written back as 24 + 24, and the flag).  Prints one JSON line (not the bench
contract: bench.py stays the headline metric)."""
import argparse
import json
import time

import numpy as np

from membrane_solver_amd import meshgen
from membrane_solver_amd.geometry.mesh import ArrayMesh
from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager
from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager
from membrane_solver_amd.runtime.minimizer import Minimizer
from membrane_solver_amd.runtime.steppers import ConjugateGradient

ap = argparse.ArgumentParser()
ap.add_argument("--rings", type=int, default=577, help="disk_patch rings (nf = 6 n^2: 577 gives 1 997 574 facets)")
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--rounds", type=int, default=2, help="alternations of the configurations")
ap.add_argument("--configs", default="none,perimeter,fixed_plane")
args = ap.parse_args()

P, T, B = meshgen.disk_patch(args.rings)
n_rim = 6 * args.rings
s = len(P) - n_rim  # the last ring's vertices, in order around the circle
assert B[s:].all() and not B[:s].any()
rim = np.stack([s + np.arange(n_rim), s + (np.arange(n_rim) + 1) % n_rim], axis=1)
P0 = float(np.linalg.norm(P[rim[:, 1]] - P[rim[:, 0]], axis=1).sum())


def make(config):
    gp = {"surface_tension": 1.0, "bending_modulus": 1.0, "spontaneous_curvature": 0.2}
    cons = []
    if config == "perimeter":
        gp["perimeter_constraints"] = [{"edges": list(range(1, n_rim + 1)), "target_perimeter": 0.97 * P0}]
        cons = ["perimeter"]
    elif config == "fixed_plane":
        gp.update({"fixed_plane_normal": [0.2, -0.1, 1.0], "fixed_plane_point": [0.0, 0.0, 0.1]})
        cons = ["fixed_plane"]
    mods = ["surface", "bending"]
    mesh = ArrayMesh(P, T, global_parameters=gp, edges=rim, energy_modules=mods, constraint_modules=cons)
    mz = Minimizer(mesh, mesh.global_parameters, ConjugateGradient(), EnergyModuleManager(mods), ConstraintModuleManager(cons),
                   quiet=True, step_size=1e-6)
    mz.minimize(args.warmup, sync_mesh=False)
    return mz, mesh._hip_mirror.dm


def window(mz):
    t0 = time.perf_counter()
    mz.minimize(args.steps, sync_mesh=False)
    return args.steps / (time.perf_counter() - t0), int(mz.last_run["trials"])


configs = args.configs.split(",")
built = {c: make(c) for c in configs}
rates = {c: [] for c in configs}
trials = {c: [] for c in configs}
for _ in range(args.rounds):
    for c in configs:
        r, t = window(built[c][0])
        rates[c].append(r)
        trials[c].append(t)
print(json.dumps({"workload": f"disk_patch({args.rings}) (nv={len(P)}, nf={len(T)}, rim edges {n_rim}), surface + bending, CG, "
                              f"{args.steps} steps after {args.warmup}, {args.rounds} alternations",
                  "steps_per_s": rates, "median": {c: float(np.median(v)) for c, v in rates.items()}, "trials": trials,
                  "queue_rounds": {c: built[c][1].queue_stats()["rounds"] for c in configs},
                  "enforce_only_stats": {c: built[c][1].enforce_only_stats() for c in configs}}), flush=True)
