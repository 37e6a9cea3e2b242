"""Cost of the body_area_penalty module on the bending lane: steps/s of surface + bending + volume row (CG, projection
off) with and without the module, on the 131 220-facet and the 2 048 000-facet icosphere, same steps and warm-up,
the two configurations alternating in ONE process; then the K_A / K_C kernel times of both from an event-timed
window.  Prints one JSON line per size (not the bench contract: bench.py stays the headline metric)."""
import argparse
import json
import time

import numpy as np

from membrane_solver_amd import meshgen
from membrane_solver_amd.geometry.mesh import ArrayBody, ArrayMesh
from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager
from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager
from membrane_solver_amd.runtime.minimizer import Minimizer
from membrane_solver_amd.runtime.steppers import ConjugateGradient

ap = argparse.ArgumentParser()
ap.add_argument("--freqs", default="81,320", help="icosphere frequencies (nf = 20 f^2)")
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--rounds", type=int, default=3, help="alternations of the two configurations")
args = ap.parse_args()


def make(P, T, with_module):
    A = 0.5 * np.linalg.norm(np.cross(P[T[:, 1]] - P[T[:, 0]], P[T[:, 2]] - P[T[:, 0]]), axis=1).sum()
    V = np.einsum("ij,ij->i", np.cross(P[T[:, 1]], P[T[:, 2]]), P[T[:, 0]]).sum() / 6.0
    gp = {"surface_tension": 1.0, "bending_modulus": 1.0, "spontaneous_curvature": 0.2, "area_stiffness": 10.0,
          "volume_constraint_mode": "lagrange", "volume_projection_during_minimization": False}
    mods = ["surface", "bending"] + (["body_area_penalty"] if with_module else [])
    mesh = ArrayMesh(P, T, global_parameters=gp, energy_modules=mods, constraint_modules=["volume"],
                     bodies=[ArrayBody(target_volume=float(V), options={"area_target": 0.98 * float(A)})])
    mz = Minimizer(mesh, mesh.global_parameters, ConjugateGradient(), EnergyModuleManager(mods),
                   ConstraintModuleManager(["volume"]), quiet=True, step_size=1e-6)
    mz.minimize(args.warmup, sync_mesh=False)
    return mz, mesh._hip_mirror.dm


def window(mz):
    t0 = time.perf_counter()
    mz.minimize(args.steps, sync_mesh=False)
    return args.steps / (time.perf_counter() - t0)


def kernels(mz, dm):
    dm.profile_enable(True)
    dm.profile_read()
    mz.minimize(args.steps, sync_mesh=False)
    pr = dm.profile_read()
    dm.profile_enable(False)
    return {k: {"avg_us": 1e3 * ms / n, "launches_per_step": n / args.steps} for k, (ms, n) in pr.items() if n}


for freq in [int(f) for f in args.freqs.split(",")]:
    P, T = meshgen.icosphere(freq)
    P = meshgen.smooth_displace(P, 0.05)
    base, dm0 = make(P, T, False)
    area, dm1 = make(P, T, True)
    rates = {"without": [], "with": []}
    for _ in range(args.rounds):
        rates["without"].append(window(base))
        rates["with"].append(window(area))
    med = {k: float(np.median(v)) for k, v in rates.items()}
    print(json.dumps({"workload": f"icosphere f={freq} (nf={len(T)}), surface + bending + volume row, CG, "
                                  f"{args.steps} steps after {args.warmup}, {args.rounds} alternations",
                      "steps_per_s_without": rates["without"], "steps_per_s_with": rates["with"],
                      "median_without": med["without"], "median_with": med["with"],
                      "ratio_with_over_without": med["with"] / med["without"],
                      "queue_rounds_without": dm0.queue_stats()["rounds"], "queue_rounds_with": dm1.queue_stats()["rounds"],
                      "kernels_without": kernels(base, dm0), "kernels_with": kernels(area, dm1)}), flush=True)
