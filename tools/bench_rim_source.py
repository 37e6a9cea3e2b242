"""Cost of the tilt_rim_source_in lane: (1) one nested leaflet relaxation on the reference's milestone-C annulus
(tests/golden/rim_source_milestone_c.npz: 24 vertices, 8 rim edges, follow mode; 50 inner steps, step 0.05, tilt_tol 0
-- the call the reference's benchmarks/benchmark_tilt_relaxation.py times), median of repeated runs after warm-up, with
the module and -- the fused evaluator's lane -- without it; (2) steps/s of the disk6 trajectory's deck
(tests/golden/traj_disk6_gd_rimsource_nested_cg.npz) with the module on and off.  Every relaxation starts from the
fixture's initial tilts (re-uploaded outside the timed window).  Prints one JSON line (not the bench contract: bench.py
stays the headline metric).  There is no pass threshold: this lane is launch-per-kernel and host-driven."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from membrane_solver_amd.geometry.mesh import ArrayMesh  # noqa: E402
from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager  # noqa: E402
from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager  # noqa: E402
from membrane_solver_amd.runtime.minimizer import Minimizer  # noqa: E402
from membrane_solver_amd.runtime.steppers import GradientDescent  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--steps", type=int, default=20)
args = ap.parse_args()


def golden(name):
    return dict(np.load(os.path.join(ROOT, "tests", "golden", name), allow_pickle=False))


def opts(text):
    return {int(k): v for k, v in json.loads(str(text)).items()}


def relaxation(with_module):
    g = golden("rim_source_milestone_c.npz")
    mods = [str(m) for m in g["modules"] if with_module or str(m) != "tilt_rim_source_in"]
    mesh = ArrayMesh(g["positions"], g["tri"], tilts_in=g["tilts_in0"], tilts_out=g["tilts_out0"],
                     tilt_fixed_in=g["tilt_fixed_in"], tilt_fixed_out=g["tilt_fixed_out"],
                     global_parameters=json.loads(str(g["gp_json"])), energy_modules=mods, constraint_modules=[],
                     edges=g["edges"], vertex_options=opts(g["vopts"]))
    mz = Minimizer(mesh, mesh.global_parameters, GradientDescent(), EnergyModuleManager(mods), ConstraintModuleManager([]),
                   quiet=True)
    mir, dm = mz._device()
    rp = mz._tilt_relax_params()
    times, evals = [], 0
    for k in range(args.warmup + args.runs):
        mir._leaflet_keys.pop("in", None)
        mir._leaflet_keys.pop("out", None)
        mz._device()  # the initial tilts again
        dm.fetch_scalars()
        t0 = time.perf_counter()
        _it, evals = dm.relax_leaflet_tilts(**rp)
        dt = time.perf_counter() - t0
        if k >= args.warmup:
            times.append(dt)
    st = dm.exec_stats()
    return {"median_s": float(np.median(times)), "min_s": float(np.min(times)), "evaluations": int(evals),
            "relax_fused_runs": st["relax_fused"], "relax_programs": st["relax_programs"],
            "E_total": float(dm.energy().sum())}


def stepping(with_module):
    g = golden("traj_disk6_gd_rimsource_nested_cg.npz")
    mods = [str(m) for m in g["modules"] if with_module or str(m) != "tilt_rim_source_in"]
    mesh = ArrayMesh(g["positions0"], g["tri"], fixed=g["fixed"], surface_tension=g["gamma"], tilts_in=g["tilts_in0"],
                     tilts_out=g["tilts_out0"], tilt_fixed_in=g["tilt_fixed_in"], tilt_fixed_out=g["tilt_fixed_out"],
                     global_parameters=json.loads(str(g["gp_json"])), energy_modules=mods, constraint_modules=[],
                     edges=g["edges"], vertex_options=opts(g["vopts"]))
    mz = Minimizer(mesh, mesh.global_parameters, GradientDescent(), EnergyModuleManager(mods), ConstraintModuleManager([]),
                   quiet=True, step_size=1e-3)
    mz.minimize(5, sync_mesh=False)
    rates = []
    for _ in range(3):
        mir, dm = mz._device_nosync()
        t0 = time.perf_counter()
        mz._minimize_in_library(mir, dm, args.steps, False)
        rates.append(args.steps / (time.perf_counter() - t0))
    return {"steps_per_s": rates, "median_steps_per_s": float(np.median(rates))}


out = {"workload": "milestone-C annulus (24 vertices, 32 facets, 8 rim edges, follow mode): one nested leaflet relaxation, "
                   f"50 inner steps, step 0.05, tilt_tol 0; median of {args.runs} runs after {args.warmup}; and the disk6 "
                   f"deck (127 vertices), GD + nested CG relaxation, {args.steps} steps x 3 windows",
       "relaxation_with_module": relaxation(True), "relaxation_without_module": relaxation(False),
       "disk6_step_with_module": stepping(True), "disk6_step_without_module": stepping(False)}
print(json.dumps(out), flush=True)
