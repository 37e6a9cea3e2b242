"""Cost of the tilt_coupling lane.  Prints one JSON line (not the bench contract: bench.py stays the headline metric).

--mode relax    (1) the milestone-B tracking relaxation (tests/golden/tilt_coupling_milestone_b.npz: flat annulus of 60
                vertices, k_c = 10 "difference", up to 1000 inner steps, tilt_tol 1e-6: 253 evaluations), median wall time
                of repeated runs after warm-up, with the streaming kernel k_couple_vec and with the same evaluations forced through
                the tile kernel (MS_COUPLE_VEC=0, read by ms_set_tilt_coupling); (2) the same comparison for a CG
                relaxation of --iters iterations on an icosphere of --freq (tilt_in + tilt_out + tilt_coupling).
--mode kernels  --evals evaluations of the energy (k_tilt<0> per leaflet, k_couple<0>) and of the energy with the raw
                shape gradient (k_tilt<1> per leaflet, k_couple<1>) on the icosphere of --freq, MS_TSEARCH=0 so that the
                magnitude modules keep their own launches.  Meant to run under a kernel trace of its own
                (rocprofv3 --kernel-trace --stats -- python tools/bench_tilt_coupling.py --mode kernels); the JSON line
                carries the algorithmic bytes of the four kernels for the comparison.
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
ap.add_argument("--mode", choices=("relax", "kernels"), default="relax")
ap.add_argument("--runs", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--freq", type=int, default=320, help="icosphere frequency (320 -> 2 048 000 facets)")
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--evals", type=int, default=20)
args = ap.parse_args()
if args.mode == "kernels":
    os.environ["MS_TSEARCH"] = "0"

from membrane_solver_amd import _lib as L  # noqa: E402
from membrane_solver_amd import meshgen  # noqa: E402
from membrane_solver_amd.device import DeviceMesh  # noqa: E402


def golden(name):
    return dict(np.load(os.path.join(ROOT, "tests", "golden", name), allow_pickle=False))


def milestone_b(vec):
    from membrane_solver_amd.geometry.mesh import ArrayMesh
    from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager
    from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager
    from membrane_solver_amd.runtime.minimizer import Minimizer
    from membrane_solver_amd.runtime.steppers import GradientDescent

    os.environ["MS_COUPLE_VEC"] = "1" if vec else "0"
    g = golden("tilt_coupling_milestone_b.npz")
    mods = [str(m) for m in g["modules"]]
    mesh = ArrayMesh(g["positions"], g["tri"], fixed=g["fixed"], tilts_in=g["tilts_in0"], tilts_out=g["tilts_out0"],
                     tilt_fixed_in=g["tilt_fixed_in"], tilt_fixed_out=g["tilt_fixed_out"],
                     global_parameters=json.loads(str(g["gp_json"])), energy_modules=mods, constraint_modules=[])
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
    return {"median_s": float(np.median(times)), "min_s": float(np.min(times)), "evaluations": int(evals),
            "launches": dm.tilt_coupling_stats(), "E_total": float(dm.energy().sum())}


def sphere_device():
    P, T = meshgen.icosphere(args.freq)
    P = meshgen.smooth_displace(P, 0.05)
    rng = np.random.default_rng(3)
    nrm = P / np.linalg.norm(P, axis=1)[:, None]
    fields = []
    for scale in (0.3, 0.25):
        t = scale * rng.normal(size=P.shape)
        fields.append(t - np.einsum("ij,ij->i", t, nrm)[:, None] * nrm)
    dm = DeviceMesh(P, T)
    return dm, fields, len(P), len(T)


def sphere_relax(vec):
    os.environ["MS_COUPLE_VEC"] = "1" if vec else "0"
    dm, (tin, tout), nv, nf = sphere_device()
    dm.set_tilt_coupling(3.0, -1)
    dm.set_params(modules=L.MS_MOD_TILT_IN | L.MS_MOD_TILT_OUT | L.MS_MOD_TILT_COUPLING)
    times, evals = [], 0
    for k in range(args.warmup + args.runs):
        dm.set_leaflet_tilts("in", tin, tilt_modulus=2.0)
        dm.set_leaflet_tilts("out", tout, tilt_modulus=1.4)
        dm.fetch_scalars()
        t0 = time.perf_counter()
        _it, evals = dm.relax_leaflet_tilts(solver="cg", max_iters=args.iters, step_size=0.05, tol=0.0)
        dt = time.perf_counter() - t0
        if k >= args.warmup:
            times.append(dt)
    out = {"nv": nv, "nf": nf, "median_s": float(np.median(times)), "min_s": float(np.min(times)),
           "evaluations": int(evals), "launches": dm.tilt_coupling_stats()}
    dm.close()
    return out


def kernels():
    dm, (tin, tout), nv, nf = sphere_device()
    dm.set_leaflet_tilts("in", tin, tilt_modulus=2.0)
    dm.set_leaflet_tilts("out", tout, tilt_modulus=1.4)
    dm.set_tilt_coupling(3.0, -1)
    dm.set_params(modules=L.MS_MOD_TILT_IN | L.MS_MOD_TILT_OUT | L.MS_MOD_TILT_COUPLING)
    e = None
    for _ in range(args.evals):
        dm.energy_and_gradient(want_grad=False, raw=True)  # k_tilt<0> x 2, k_couple<0>; then k_tilt<1> x 2, k_couple<1>
        e = dm.energy()
    st = dm.tilt_coupling_stats()
    dm.close()
    # algorithmic bytes per launch (halo rows and the per-tile offsets left out): positions 24 nv, a tilt field 24 nv,
    # flags nv, a facet record 8 nf; MODE 1 adds the vertex -> corner CSR (2 bytes x 3 nf), g read and written (48 nv)
    # and a tilt gradient written (24 nv, k_tilt<1>) or two of them read and written (96 nv, k_couple<1>)
    b = {"k_tilt<0>": 49 * nv + 8 * nf, "k_couple<0>": 73 * nv + 8 * nf,
         "k_tilt<1>": 49 * nv + 8 * nf + 6 * nf + 48 * nv + 24 * nv,
         "k_couple<1>": 73 * nv + 8 * nf + 6 * nf + 48 * nv + 96 * nv}
    return {"nv": nv, "nf": nf, "evaluations": args.evals, "launches": st, "energies": [float(v) for v in e],
            "algorithmic_bytes": b, "byte_ratio_mode0": b["k_couple<0>"] / b["k_tilt<0>"],
            "byte_ratio_mode1": b["k_couple<1>"] / b["k_tilt<1>"]}


if args.mode == "kernels":
    out = {"mode": "kernels", "result": kernels()}
else:
    out = {"mode": "relax",
           "workload": f"milestone-B annulus (60 vertices): one nested relaxation, median of {args.runs} runs after "
                       f"{args.warmup}; icosphere f={args.freq}: CG relaxation of {args.iters} iterations, same statistics",
           "milestone_b_vec": milestone_b(True), "milestone_b_tile": milestone_b(False),
           "sphere_vec": sphere_relax(True), "sphere_tile": sphere_relax(False)}
print(json.dumps(out), flush=True)
