"""Cost of the rim_slope_match_out lane (non-zero strength).

    python3 tools/bench_rim_slope_match.py kernels   # k_rsm_geom + k_rsm_apply at rim sizes 64, 1024 and 4096
    python3 tools/bench_rim_slope_match.py relax     # the 40-iteration leaflet relaxation of the fixture, with and
                                                     # without the module
    python3 tools/bench_rim_slope_match.py trace --db 64:CSV 1024:CSV 4096:CSV
                                                     # per-kernel device times out of the profiler's kernel_stats files

``kernels``: the module alone on a disk mesh; the first n rows are the rim, the next n + n / 8 (n - n / 8 at the row
limit) the outer ring (unequal counts: the arc-length interpolation, its serial prefix and the binary searches run) and
the next n / 2 the disk ring
(the mean variant); any rows will do, the kernels only read their positions.  One host-timed call per rim size: an
evaluation with both tilt gradients (one geometry launch + one apply launch, the fold of the scalars and their fetch).
It carries the launch and synchronisation latency of a small kernel pair; what grows with the ring size is the kernels'
own time (the rank count of k_rsm_geom is quadratic in the ring size, once per ring).  For the per-kernel device times
run ``kernels --rows N --runs 20`` under ``rocprofv3 --kernel-trace --stats --output-format csv`` once per rim size and
hand the ``*kernel_stats.csv`` files it writes to ``trace``, which prints mean and minimum of the two kernels' dispatches.
``relax``: tests/golden/rim_slope_match_relax.npz (127 vertices; rim 18, outer 24, disk 12), its module list with or
without rim_slope_match_out; median wall time of repeated relaxations from the fixture's initial tilts.  Prints one
JSON line per measurement (not the bench contract: bench.py stays the headline metric)."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("what", choices=["kernels", "relax", "trace"])
ap.add_argument("--db", nargs="*", default=[], metavar="ROWS:PATH", help="kernel_stats csv files of `trace`")
ap.add_argument("--rows", type=int, nargs="*", default=[64, 1024, 4096], help="rim sizes of `kernels`")
ap.add_argument("--runs", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
args = ap.parse_args()
sys.path.insert(0, HERE)
NAME = "rim_slope_match_out"


def bench_kernels():
    from membrane_solver_amd import _lib as L
    from membrane_solver_amd import meshgen
    from membrane_solver_amd.device import DeviceMesh

    P, T, _B = meshgen.disk_patch(60)  # 10981 vertices
    rng = np.random.default_rng(3)
    for n in args.rows:
        n_out = n + n // 8 if n + n // 8 <= L.MS_RIM_MATCH_MAX_ROWS else n - n // 8  # (never the rim's count)
        n_disk = n // 2
        assert n + n_out + n_disk < len(P)
        dm = DeviceMesh(P, T)
        dm.set_leaflet_tilts("in", 0.3 * rng.normal(size=P.shape), tilt_modulus=0.0)
        dm.set_leaflet_tilts("out", 0.3 * rng.normal(size=P.shape), tilt_modulus=0.0)
        dm.set_rim_match(np.arange(1, n + 1), np.arange(n + 1, n + 1 + n_out),
                         np.arange(n + 1 + n_out, n + 1 + n_out + n_disk), center=(0.01, 0.02, 0.0), strength=3.0)
        dm.set_params(modules=L.MS_MOD_RIM_SLOPE_MATCH_OUT)
        evaluation = []
        for k in range(args.warmup + args.runs):
            t0 = time.perf_counter()
            dm.leaflet_tilt_energy_and_gradient(want_gradient=True)  # geometry + apply + fold + fetch + two copies
            t1 = time.perf_counter()
            if k >= args.warmup:
                evaluation.append(t1 - t0)
        print(json.dumps({"what": "kernels", "rim_rows": n, "outer_rows": n_out, "disk_rows": n_disk,
                          "evaluation_median_us": 1e6 * float(np.median(evaluation)),
                          "evaluation_min_us": 1e6 * float(np.min(evaluation)), "runs": args.runs,
                          "launches": dm.rim_match_stats()}), flush=True)
        dm.close()


def bench_relax():
    from membrane_solver_amd.geometry.mesh import ArrayMesh
    from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager
    from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager
    from membrane_solver_amd.runtime.minimizer import Minimizer
    from membrane_solver_amd.runtime.steppers import GradientDescent

    g = dict(np.load(os.path.join(HERE, "tests", "golden", "rim_slope_match_relax.npz"), allow_pickle=False))
    vo = {int(k): v for k, v in json.loads(str(g["vopts"])).items()}
    for with_module in (False, True):
        gp = json.loads(str(g["gp_json"]))
        mods = [str(m) for m in g["modules"] if with_module or str(m) != NAME]
        mesh = ArrayMesh(g["positions"], g["tri"], fixed=g["fixed"], tilts_in=g["tilts_in0"], tilts_out=g["tilts_out0"],
                         global_parameters=gp, energy_modules=mods, constraint_modules=[], edges=g["edges"],
                         vertex_options=vo)
        mz = Minimizer(mesh, mesh.global_parameters, GradientDescent(), EnergyModuleManager(mods),
                       ConstraintModuleManager([]), quiet=True)
        mir, dm = mz._device()
        rp = mz._tilt_relax_params()
        times, evals, iters = [], 0, 0
        for k in range(args.warmup + args.runs):
            mir._leaflet_keys.pop("in", None)
            mir._leaflet_keys.pop("out", None)
            mz._device()  # the initial tilts again
            dm.energy()   # (the bending_tilt record: not part of the relaxation)
            t0 = time.perf_counter()
            iters, evals = dm.relax_leaflet_tilts(**rp)
            dt = time.perf_counter() - t0
            if k >= args.warmup:
                times.append(dt)
        print(json.dumps({"what": "relax", "with_module": with_module, "median_ms": 1e3 * float(np.median(times)),
                          "min_ms": 1e3 * float(np.min(times)), "max_ms": 1e3 * float(np.max(times)), "runs": args.runs,
                          "iterations": int(iters), "evaluations": int(evals), "launches": dm.rim_match_stats()}),
              flush=True)


def kernel_trace():
    """calls, mean and minimum duration of the two kernels out of each run's kernel_stats csv (rocprofv3 --kernel-trace
    --stats --output-format csv)"""
    import csv

    for item in args.db:
        rows, path = item.split(":", 1)
        out = {"what": "kernel_trace", "rim_rows": int(rows)}
        with open(path, newline="") as fh:
            for rec in csv.DictReader(fh):
                for k in ("k_rsm_geom", "k_rsm_apply"):
                    if k in rec["Name"]:
                        out[k] = {"dispatches": int(rec["Calls"]), "mean_us": float(rec["AverageNs"]) / 1e3,
                                  "min_us": float(rec["MinNs"]) / 1e3, "max_us": float(rec["MaxNs"]) / 1e3}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    {"kernels": bench_kernels, "relax": bench_relax, "trace": kernel_trace}[args.what]()
