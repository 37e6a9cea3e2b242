"""Cost of the tilt_thetaB_contact_in lane.

    python3 tools/bench_thetab_contact.py kernels   # k_thetab_geom + k_thetab_apply at ring sizes 64, 1024 and 4096
    python3 tools/bench_thetab_contact.py relax     # a 40-iteration leaflet relaxation on the 84-vertex annulus, with
                                                    # and without the module
    python3 tools/bench_thetab_contact.py trace --db 64:DB 1024:DB 4096:DB
                                                    # per-kernel device times out of kernel-trace databases

``kernels``: the module alone on a disk mesh whose first n rows are the ring (any rows will do: the kernels only read
their positions).  Two host-timed calls per ring size, each one geometry launch + one apply launch: an evaluation (with
the fold of the scalars and their fetch) and the scalar update (with a 24-byte copy).  Both carry the launch and
synchronisation latency of a small kernel pair; what grows with the ring size is the kernels' own time (the rank
count of k_thetab_geom is quadratic in the ring size).  For the per-kernel device times run
``kernels --rows N --runs 20`` under ``rocprofv3 --kernel-trace`` once per ring size and hand the databases it writes
(rocpd SQLite) to ``trace``, which prints mean and minimum of the two kernels' dispatches.
``relax``: tests/golden/rim_bilayer_relax.npz's annulus (84 vertices, its pins), the deck's module
list with tilt_thetaB_contact_in in legacy mode on the pinned rim rows added or not; median wall time of repeated
relaxations from the fixture's initial tilts.  Prints one JSON line per measurement (not the bench contract: bench.py
stays the headline metric)."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("what", choices=["kernels", "relax", "trace"])
ap.add_argument("--db", nargs="*", default=[], metavar="ROWS:PATH", help="kernel-trace databases of `trace`")
ap.add_argument("--rows", type=int, nargs="*", default=[64, 1024, 4096], help="ring sizes of `kernels`")
ap.add_argument("--runs", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
args = ap.parse_args()
sys.path.insert(0, HERE)


def bench_kernels():
    from membrane_solver_amd import _lib as L
    from membrane_solver_amd import meshgen
    from membrane_solver_amd.device import DeviceMesh

    P, T, _B = meshgen.disk_patch(38)  # 4447 vertices
    rng = np.random.default_rng(3)
    for n in args.rows:
        dm = DeviceMesh(P, T)
        dm.set_leaflet_tilts("in", 0.3 * rng.normal(size=P.shape), tilt_modulus=0.0)
        dm.set_leaflet_tilts("out", np.zeros_like(P), tilt_modulus=0.0)
        dm.set_thetab_contact(np.arange(1, n + 1) % len(P), center=(0.01, 0.02, 0.0), k=3.0, gamma=0.7,
                              work_mode="field_linear", penalty_mode="legacy")
        dm.set_thetab_value(0.1)
        dm.set_params(modules=L.MS_MOD_TILT_THETAB_CONTACT_IN)
        evaluation, update = [], []
        for k in range(args.warmup + args.runs):
            t0 = time.perf_counter()
            dm.leaflet_tilt_energy_and_gradient(want_gradient=False)  # geometry + apply + fold + fetch
            t1 = time.perf_counter()
            dm.update_thetab_value()  # geometry + apply (scalars only) + a 24-byte copy
            t2 = time.perf_counter()
            if k >= args.warmup:
                evaluation.append(t1 - t0)
                update.append(t2 - t1)
        print(json.dumps({"what": "kernels", "ring_rows": n, "evaluation_median_us": 1e6 * float(np.median(evaluation)),
                          "evaluation_min_us": 1e6 * float(np.min(evaluation)),
                          "scalar_update_median_us": 1e6 * float(np.median(update)),
                          "scalar_update_min_us": 1e6 * float(np.min(update)), "runs": args.runs,
                          "launches": dm.thetab_contact_stats()}), flush=True)
        dm.close()


def bench_relax():
    from membrane_solver_amd.geometry.mesh import ArrayMesh
    from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager
    from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager
    from membrane_solver_amd.runtime.minimizer import Minimizer
    from membrane_solver_amd.runtime.steppers import GradientDescent

    g = dict(np.load(os.path.join(HERE, "tests", "golden", "rim_bilayer_relax.npz"), allow_pickle=False))
    vo = {int(k): v for k, v in json.loads(str(g["vopts"])).items()}
    rim = sorted(r for r, o in vo.items() if o.get("pin_to_circle_group") is not None or "pin_to_circle" in (o.get("constraints") or []))
    for with_module in (False, True):
        gp = json.loads(str(g["gp_json"]))
        gp.update({"tilt_inner_steps": 40, "tilt_thetaB_group_in": "ring", "tilt_thetaB_normal": [0.0, 0.0, 1.0],
                   "tilt_thetaB_strength_in": 4.0, "tilt_thetaB_contact_strength_in": 0.6, "tilt_thetaB_value": 0.08,
                   "tilt_thetaB_contact_penalty_mode": "legacy"})
        mods = [str(m) for m in g["modules"]] + (["tilt_thetaB_contact_in"] if with_module else [])
        cons = [str(m) for m in g["constraint_modules"]]
        vopts = {r: dict(o, **({"tilt_thetaB_group": "ring"} if r in rim else {})) for r, o in vo.items()}
        mesh = ArrayMesh(g["positions"], g["tri"], fixed=g["fixed"], tilts_in=g["tilts_in0"], tilts_out=g["tilts_out0"],
                         tilt_fixed_in=g["tilt_fixed_in"], tilt_fixed_out=g["tilt_fixed_out"], global_parameters=gp,
                         energy_modules=mods, constraint_modules=cons, edges=g["edges"], vertex_options=vopts)
        mz = Minimizer(mesh, mesh.global_parameters, GradientDescent(), EnergyModuleManager(mods),
                       ConstraintModuleManager(cons), quiet=True)
        mir, dm = mz._device()
        rp = mz._tilt_relax_params()
        times, evals, iters = [], 0, 0
        for k in range(args.warmup + args.runs):
            mir._leaflet_keys.pop("in", None)
            mir._leaflet_keys.pop("out", None)
            mz._device()  # the initial tilts again
            dm.fetch_scalars()
            t0 = time.perf_counter()
            iters, evals = dm.relax_leaflet_tilts(**rp)
            dt = time.perf_counter() - t0
            if k >= args.warmup:
                times.append(dt)
        print(json.dumps({"what": "relax", "with_module": with_module, "ring_rows": len(rim) if with_module else 0,
                          "median_ms": 1e3 * float(np.median(times)), "min_ms": 1e3 * float(np.min(times)),
                          "max_ms": 1e3 * float(np.max(times)), "runs": args.runs, "iterations": int(iters),
                          "evaluations": int(evals), "launches": dm.thetab_contact_stats()}), flush=True)


def kernel_trace():
    """mean / min duration of the two kernels' dispatches in each database (tables rocpd_kernel_dispatch* and
    rocpd_info_kernel_symbol* of the profiler's SQLite output)"""
    import sqlite3

    for item in args.db:
        rows, path = item.split(":", 1)
        con = sqlite3.connect(path)
        tabs = [r[0] for r in con.execute("select name from sqlite_master where type in ('table', 'view')")]
        disp = [t for t in tabs if "rocpd" in t and "kernel_dispatch" in t][0]
        sym = [t for t in tabs if "rocpd" in t and "kernel_symbol" in t][0]
        out = {"what": "kernel_trace", "ring_rows": int(rows)}
        for name, n, mean, low in con.execute(
                f"select s.kernel_name, count(*), avg(d.end - d.start), min(d.end - d.start) from {disp} d join {sym} s "
                "on d.kernel_id = s.id where s.kernel_name like '%k_thetab_%' group by s.kernel_name order by s.kernel_name"):
            k = "k_thetab_geom" if "k_thetab_geom" in name else "k_thetab_apply"
            out[k] = {"dispatches": int(n), "mean_us": mean / 1e3, "min_us": low / 1e3}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    {"kernels": bench_kernels, "relax": bench_relax, "trace": kernel_trace}[args.what]()
