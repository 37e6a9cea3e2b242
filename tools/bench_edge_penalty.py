"""Cost of the edge_length_penalty module: steps/s of surface + bending (CG) on the 2 048 000-facet icosphere with ALL
3 072 000 edges given a target (0.95 of their length), against the same mesh with the module off but forced into the
same host-decided lane (MS_SPECULATE=0: no rounds queued on the device), the two configurations alternating in ONE
process; then the microseconds of k_edgepen_energy and k_edgepen_grad from HIP events around their launches.  The
windows time the in-library loop alone: the Minimizer resolves the targets again at every minimize() call (a Python
pass over the edges, seconds at this size), which is configuration, not stepping.  Prints one JSON line (not the
bench contract: bench.py stays the headline metric)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("MS_SPECULATE", "0")  # the module-off context takes the host-decided lane too

from membrane_solver_amd import _lib as L  # noqa: E402
from membrane_solver_amd import meshgen  # noqa: E402
from membrane_solver_amd.geometry.mesh import ArrayMesh  # noqa: E402
from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager  # noqa: E402
from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager  # noqa: E402
from membrane_solver_amd.runtime.minimizer import Minimizer  # noqa: E402
from membrane_solver_amd.runtime.steppers import ConjugateGradient  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--freq", type=int, default=320, help="icosphere frequency (nf = 20 f^2)")
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--rounds", type=int, default=3, help="alternations of the two configurations")
args = ap.parse_args()


def all_sides(P, T):
    """(tail, head) of every triangle side once"""
    a = np.concatenate([T[:, 0], T[:, 1], T[:, 2]]).astype(np.int64)
    b = np.concatenate([T[:, 1], T[:, 2], T[:, 0]]).astype(np.int64)
    key = np.unique(np.minimum(a, b) * len(P) + np.maximum(a, b))
    return np.stack([key // len(P), key % len(P)], axis=1)


def make(P, T, edges, with_module):
    gp = {"surface_tension": 1.0, "bending_modulus": 1.0, "spontaneous_curvature": 0.2, "edge_stiffness": 10.0}
    mods = ["surface", "bending"] + (["edge_length_penalty"] if with_module else [])
    ln = np.linalg.norm(P[edges[:, 1]] - P[edges[:, 0]], axis=1)
    mesh = ArrayMesh(P, T, global_parameters=gp, energy_modules=mods, edges=edges,
                     edge_options={k: {"target_length": float(x)} for k, x in enumerate(0.95 * ln)})
    mz = Minimizer(mesh, mesh.global_parameters, ConjugateGradient(), EnergyModuleManager(mods),
                   ConstraintModuleManager([]), quiet=True, step_size=1e-6)
    mz.minimize(args.warmup, sync_mesh=False)
    return mz, mesh._hip_mirror.dm


def window(mz):
    mir, dm = mz._device_nosync()
    t0 = time.perf_counter()
    mz._minimize_in_library(mir, dm, args.steps, False)
    return args.steps / (time.perf_counter() - t0)


P, T = meshgen.icosphere(args.freq)
P = meshgen.smooth_displace(P, 0.05)
edges = all_sides(P, T)
base, dm0 = make(P, T, edges, False)
pen, dm1 = make(P, T, edges, True)
assert dm1.modules & L.MS_MOD_EDGE_LENGTH_PENALTY and not dm0.modules & L.MS_MOD_EDGE_LENGTH_PENALTY
rates = {"without": [], "with": []}
for _ in range(args.rounds):
    rates["without"].append(window(base))
    rates["with"].append(window(pen))
med = {k: float(np.median(v)) for k, v in rates.items()}
before = dm1.edge_penalty_stats()  # (also drops the event sums so far)
dm1.profile_enable(True)
window(pen)
ls = dm1.edge_penalty_stats()
for key in ("energy_launches", "grad_launches"):
    ls[key] -= before[key]
dm1.profile_read()
dm1.profile_enable(False)
print(json.dumps({"workload": f"icosphere f={args.freq} (nf={len(T)}), surface + bending, CG, host-decided lane, "
                              f"{len(edges)} targeted edges, {args.steps} steps after {args.warmup}, {args.rounds} alternations",
                  "steps_per_s_without": rates["without"], "steps_per_s_with": rates["with"],
                  "median_without": med["without"], "median_with": med["with"],
                  "ratio_with_over_without": med["with"] / med["without"],
                  "us_per_step_added": 1e6 / med["with"] - 1e6 / med["without"],
                  "queue_rounds_without": dm0.queue_stats()["rounds"], "queue_rounds_with": dm1.queue_stats()["rounds"],
                  "k_edgepen_energy_us": ls["energy_us"] / max(1, ls["energy_launches"]),
                  "k_edgepen_grad_us": ls["grad_us"] / max(1, ls["grad_launches"]),
                  "k_edgepen_energy_launches_per_step": ls["energy_launches"] / args.steps,
                  "k_edgepen_grad_launches_per_step": ls["grad_launches"] / args.steps}), flush=True)
