"""Cost of the pins-next-to-tilt-modules lane.  Prints one JSON line per variant (not the bench contract: bench.py stays
the headline metric).

Workload: the soft_source deck of tests/golden/traj_softsource_deck_gd_pins.npz (84 vertices, 144 facets, both
leaflets' bending_tilt and tilt modules, the inner rim source, pin_to_plane + pin_to_circle, a nested relaxation of 40
inner steps, fixed step size): --steps minimizer iterations after --warmup, the median wall time of --runs runs, each on
a context of its own.

--mode device     the device Minimizer (ms_minimize), at the default settings, with MS_EXEC_PINS=0 (the pin kernels
                  flush the one-tile interpreter instead of being recorded by it) and with MS_EXEC=0 (a launch per
                  kernel instead of the interpreter)
--mode reference  the reference's own Minimizer on the same deck file and the same iterations, on this host's CPU
                  (--reference DIR: its checkout; imported at run time)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--mode", choices=("device", "reference"), default="device")
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--reference", default=None)
args = ap.parse_args()
DECK = "meshes/caveolin/kozlov_1disk_3d_tensionless_single_leaflet_soft_source.yaml"


def device_run(env):
    from membrane_solver_amd.geometry.mesh import ArrayMesh
    from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager
    from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager
    from membrane_solver_amd.runtime.minimizer import Minimizer
    from membrane_solver_amd.runtime.steppers import GradientDescent

    for k, v in env.items():
        os.environ[k] = v
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "traj_softsource_deck_gd_pins.npz"), allow_pickle=False))
    opts = lambda t: {int(k): v for k, v in json.loads(str(t)).items()}  # noqa: E731
    mods, cons = [str(m) for m in g["modules"]], [str(m) for m in g["constraint_modules"]]
    times, stats = [], {}
    for _ in range(args.runs):
        mesh = ArrayMesh(g["positions0"], g["tri"], fixed=g["fixed"], surface_tension=g["gamma"],
                         global_parameters=json.loads(str(g["gp_json"])), energy_modules=mods, constraint_modules=cons,
                         edges=g["edges"], vertex_options=opts(g["vopts"]), edge_options=opts(g["eopts"]),
                         tilts_in=g["tilts_in0"], tilts_out=g["tilts_out0"], tilt_fixed_in=g["tilt_fixed_in"],
                         tilt_fixed_out=g["tilt_fixed_out"])
        mz = Minimizer(mesh, mesh.global_parameters, GradientDescent(), EnergyModuleManager(mods),
                       ConstraintModuleManager(cons), quiet=True, step_size=float(g["step_size0"]))
        _mir, dm = mz._device()
        mz.minimize(args.warmup, sync_mesh=False)
        dm.fetch_scalars()
        p0 = dm.pin_stats()
        t0 = time.perf_counter()
        res = mz.minimize(args.steps, sync_mesh=False)
        dm.fetch_scalars()
        times.append(time.perf_counter() - t0)
        p1 = dm.pin_stats()
        stats = {"iterations": int(res["iterations"]), "accepted": int(mz.last_run["accepted"]),
                 "trials": int(mz.last_run["trials"]), "pin_trials": p1["trials"] - p0["trials"],
                 "pin_enforce_launches": p1["enforce_launches"] - p0["enforce_launches"], "energy": float(res["energy"]),
                 "interpreter": bool(dm.exec_stats()["active"]), "k_exec_launches": int(dm.exec_stats()["packs"])}
        mesh._hip_mirror.dm.close()
    for k in env:
        os.environ.pop(k, None)
    med = float(np.median(times))
    return dict(stats, env=env, median_s=med, min_s=float(np.min(times)), max_s=float(np.max(times)),
                steps_per_s=stats["iterations"] / med)


def reference_run():
    sys.dont_write_bytecode = True
    sys.path.insert(0, args.reference)
    from geometry.geom_io import load_data, parse_geometry
    from runtime.constraint_manager import ConstraintModuleManager
    from runtime.energy_manager import EnergyModuleManager
    from runtime.minimizer import Minimizer
    from runtime.steppers.gradient_descent import GradientDescent

    times, last = [], None
    for _ in range(args.runs):
        mesh = parse_geometry(load_data(os.path.join(args.reference, DECK)))
        mesh.global_parameters.update({"mesh_quality_auto_repair_enabled": False})
        mz = Minimizer(mesh, mesh.global_parameters, GradientDescent(), EnergyModuleManager(mesh.energy_modules),
                       ConstraintModuleManager(mesh.constraint_modules), quiet=True,
                       step_size=float(mesh.global_parameters.get("step_size")))
        mz.minimize(args.warmup)
        t0 = time.perf_counter()
        last = mz.minimize(args.steps)
        times.append(time.perf_counter() - t0)
    med = float(np.median(times))
    return {"iterations": int(last["iterations"]), "energy": float(last["energy"]), "median_s": med,
            "min_s": float(np.min(times)), "max_s": float(np.max(times)), "steps_per_s": int(last["iterations"]) / med,
            "cpus": os.cpu_count()}


head = {"workload": f"soft_source deck, {args.steps} iterations after {args.warmup}, median of {args.runs} runs"}
if args.mode == "reference":
    if not args.reference:
        sys.exit("--mode reference needs --reference DIR")
    print(json.dumps(dict(head, variant="reference (host CPU)", **reference_run())), flush=True)
else:
    for name, env in (("default", {}), ("MS_EXEC_PINS=0", {"MS_EXEC_PINS": "0"}), ("MS_EXEC=0", {"MS_EXEC": "0"})):
        print(json.dumps(dict(head, variant=name, **device_run(env))), flush=True)
