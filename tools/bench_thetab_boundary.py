"""Cost of the tilt_thetaB_boundary_in lane.

    python3 tools/bench_thetab_boundary.py kernels  # k_tbb_geom + k_tbb_apply at ring sizes 64, 1024 and 4096
    python3 tools/bench_thetab_boundary.py relax    # the 40-iteration leaflet relaxation on the 84-vertex annulus, with
                                                    # and without the constraint
    python3 tools/bench_thetab_boundary.py trace --db 64:DB 1024:DB 4096:DB
                                                    # per-kernel device times out of kernel-trace databases

``kernels``: the constraint on a disk mesh (5677 vertices) whose first n rows are the ring (any rows will do: the
kernels read their positions and their facets).  Per ring size the enforcement (one geometry launch + one apply launch)
and, to set the ring's CSR normals against a full-mesh vertex-normal pass on the same mesh,
ms_project_tilts_to_tangent.  The host clock around them reads the calls' host cost (the launches are asynchronous and
the scalar fetch between them does not wait for the stream): it is no kernel time.  For the per-kernel device times run
``kernels --rows N --runs 20`` under ``rocprofv3 --kernel-trace`` once per ring size and hand the databases it writes
(rocpd SQLite) to ``trace``, which prints mean and minimum of the dispatches of k_tbb_geom, k_tbb_apply and the
full-mesh tilt kernel.
``relax``: tests/golden/thetab_boundary_relax.npz's annulus and module list (label cg_step1_plain), with the constraint
listed or not; median wall time of repeated relaxations from the fixture's initial tilts.  The run without the
constraint is what a parent checkout measures with its own copy of this mode's code path
(tools/bench_thetab_contact.py relax measures a different module list).  Prints one JSON line per measurement (not the
bench contract: bench.py stays the headline metric)."""
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
ap.add_argument("--without-only", action="store_true", help="`relax`: only the run without the constraint (a checkout "
                "that does not know the module)")
ap.add_argument("--root", default=HERE, help="checkout whose package is measured (`relax --without-only`)")
args = ap.parse_args()
sys.path.insert(0, args.root)


def bench_kernels():
    from membrane_solver_amd import _lib as L
    from membrane_solver_amd import meshgen
    from membrane_solver_amd.device import DeviceMesh

    P, T, _B = meshgen.disk_patch(43)  # 5677 vertices, several tiles
    rng = np.random.default_rng(3)
    tin = 0.3 * rng.normal(size=P.shape)
    for n in args.rows:
        dm = DeviceMesh(P, T)
        dm.set_leaflet_tilts("in", tin, tilt_modulus=1.0)
        dm.set_leaflet_tilts("out", np.zeros_like(P), tilt_modulus=1.0)
        dm.set_thetab_boundary(np.arange(1, n + 1) % len(P), center=(0.01, 0.02, 0.0), normal=(0.0, 0.0, 1.0))
        dm.set_thetab_value(0.1)
        dm.set_params(modules=L.MS_MOD_TILT_IN | L.MS_MOD_TILT_OUT)
        enforce, normals = [], []
        for k in range(args.warmup + args.runs):
            dm.fetch_scalars()
            t0 = time.perf_counter()
            dm.thetab_boundary_enforce()  # geometry + apply
            dm.fetch_scalars()
            t1 = time.perf_counter()
            dm.project_tilts_to_tangent()  # the full-mesh normal pass (+ the projection of every row)
            dm.fetch_scalars()
            t2 = time.perf_counter()
            if k >= args.warmup:
                enforce.append(t1 - t0)
                normals.append(t2 - t1)
        print(json.dumps({"what": "kernels", "ring_rows": n, "vertices": len(P),
                          "enforce_median_us": 1e6 * float(np.median(enforce)), "enforce_min_us": 1e6 * float(np.min(enforce)),
                          "full_mesh_projection_median_us": 1e6 * float(np.median(normals)),
                          "full_mesh_projection_min_us": 1e6 * float(np.min(normals)), "runs": args.runs,
                          "launches": dm.thetab_boundary_stats()}), flush=True)
        dm.close()


def bench_relax():
    from membrane_solver_amd.geometry.mesh import ArrayMesh
    from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager
    from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager
    from membrane_solver_amd.runtime.minimizer import Minimizer
    from membrane_solver_amd.runtime.steppers import GradientDescent

    g = dict(np.load(os.path.join(HERE, "tests", "golden", "thetab_boundary_relax.npz"), allow_pickle=False))
    label = "cg_step1_plain"
    vo = {int(k): v for k, v in json.loads(str(g["vopts"])).items()}
    mods = [str(m) for m in g[label + "__modules"]]
    for with_constraint in ((False,) if args.without_only else (False, True)):
        cons = ["tilt_thetaB_boundary_in"] if with_constraint else []
        mesh = ArrayMesh(g["positions"], g["tri"], fixed=g["fixed"], tilts_in=g[label + "__tilts_in0"],
                         tilts_out=g[label + "__tilts_out0"], tilt_fixed_in=g[label + "__tilt_fixed_in"],
                         global_parameters=json.loads(str(g[label + "__gp_json"])), energy_modules=mods,
                         constraint_modules=cons, edges=g["edges"], vertex_options=vo)
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
        out = {"what": "relax", "root": os.path.relpath(args.root, HERE), "with_constraint": with_constraint,
               "median_ms": 1e3 * float(np.median(times)), "min_ms": 1e3 * float(np.min(times)),
               "max_ms": 1e3 * float(np.max(times)), "runs": args.runs, "iterations": int(iters), "evaluations": int(evals)}
        if hasattr(dm, "thetab_boundary_stats"):
            out["launches"] = dm.thetab_boundary_stats()
        print(json.dumps(out), flush=True)


def kernel_trace():
    """mean / min duration of the kernels' dispatches in each database (tables rocpd_kernel_dispatch* and
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
                "on d.kernel_id = s.id where s.kernel_name like '%k_tbb_%' or s.kernel_name like '%k_tilt%' "
                "group by s.kernel_name order by s.kernel_name"):
            short = ("k_tbb_geom" if "k_tbb_geom" in name else "k_tbb_apply" if "k_tbb_apply" in name else
                     "k_tilt<2> (full mesh)" if "k_tiltILi2E" in name or "k_tilt<2>" in name else name)
            out[short] = {"dispatches": int(n), "mean_us": mean / 1e3, "min_us": low / 1e3}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    {"kernels": bench_kernels, "relax": bench_relax, "trace": kernel_trace}[args.what]()
