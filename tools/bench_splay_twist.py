"""Cost of the tilt_splay_twist_in lane.  Prints one JSON line (not the bench contract: bench.py stays the headline metric).

--mode kernels  --evals evaluations of the inner leaflet's energy (k_tsmooth<0>, k_splay<0>) and of its energy with the
                tilt gradient (k_tsmooth<1>, k_splay<1>) on the icosphere of --freq (320 -> nv = 1 024 002,
                nf = 2 048 000), tilt_smoothness_in + tilt_splay_twist_in alone, MS_TSEARCH=0 so that the smoothness
                module keeps its own launches: the four kernels from the same process, on the same rows and records.
                Meant to run under a kernel trace of its own, without counters
                (rocprofv3 --kernel-trace --stats -- python tools/bench_splay_twist.py --mode kernels).  The algorithmic
                bytes of k_splay<M> are k_tsmooth<M>'s (the same rows, the same records): the ratio to read is time
                against time.
--mode relax    a CG relaxation of --iters iterations of tilt_in + tilt_splay_twist_in on the same icosphere, median
                wall time of --runs runs after --warmup.  Plain CG unless --jacobi: the leaflet Jacobi diagonal
                (runtime/preconditioners.py:62-146) has no splay / twist part, so next to tilt_in alone it is k_t A_v
                (~1e-5 at this mesh size) and scales the direction until no step size of the search's ladder descends:
                the preconditioned run ends after one iteration of twelve rejected trials.
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
ap.add_argument("--jacobi", action="store_true", help="relax: with the Jacobi preconditioner")
args = ap.parse_args()
if args.mode == "kernels":
    os.environ["MS_TSEARCH"] = "0"

from membrane_solver_amd import _lib as L  # noqa: E402
from membrane_solver_amd import meshgen  # noqa: E402
from membrane_solver_amd.device import DeviceMesh  # noqa: E402


def sphere_device():
    P, T = meshgen.icosphere(args.freq)
    P = meshgen.smooth_displace(P, 0.05)
    rng = np.random.default_rng(3)
    nrm = P / np.linalg.norm(P, axis=1)[:, None]
    t = 0.3 * rng.normal(size=P.shape)
    tin = t - np.einsum("ij,ij->i", t, nrm)[:, None] * nrm
    return DeviceMesh(P, T), tin, len(P), len(T)


def kernels():
    dm, tin, nv, nf = sphere_device()
    dm.set_leaflet_tilts("in", tin, tilt_modulus=0.0, smoothness=0.6)
    dm.set_leaflet_tilts("out", np.zeros_like(tin), tilt_modulus=0.0, smoothness=0.0)
    dm.set_tilt_splay_twist(0.7, 0.4)
    dm.set_params(modules=L.MS_MOD_TILT_SMOOTH_IN | L.MS_MOD_TILT_SPLAY_TWIST_IN)
    E, e = 0.0, None
    for _ in range(args.evals):
        e = dm.energy()  # k_tsmooth<0>, k_splay<0>
        E, _gi, _go = dm.leaflet_tilt_energy_and_gradient(want_gradient=False)  # k_tsmooth<1>, k_splay<1>
    st = dm.tilt_splay_twist_stats()
    own = dm.tilt_splay_twist_energy()
    dm.close()
    # algorithmic bytes per launch, the same for both kernels of a mode (halo rows and the per-tile offsets left out):
    # positions 24 nv, the tilt field 24 nv, flags nv, a facet record 8 nf; MODE 1 adds the vertex -> corner CSR
    # (2 bytes x 3 nf) and the tilt gradient read and written (48 nv)
    b = {"mode0": 49 * nv + 8 * nf, "mode1": 49 * nv + 8 * nf + 6 * nf + 48 * nv}
    return {"nv": nv, "nf": nf, "evaluations": args.evals, "launches": st, "energies": [float(v) for v in e],
            "leaflet_energy": float(E), "own_energy": float(own), "algorithmic_bytes": b}


def relax():
    dm, tin, nv, nf = sphere_device()
    dm.set_tilt_splay_twist(0.7, 0.4)
    dm.set_params(modules=L.MS_MOD_TILT_IN | L.MS_MOD_TILT_SPLAY_TWIST_IN)
    times, evals, iters = [], 0, 0
    for k in range(args.warmup + args.runs):
        dm.set_leaflet_tilts("in", tin, tilt_modulus=2.0, smoothness=0.0)
        dm.set_leaflet_tilts("out", np.zeros_like(tin), tilt_modulus=0.0, smoothness=0.0)
        dm.fetch_scalars()
        t0 = time.perf_counter()
        iters, evals = dm.relax_leaflet_tilts(solver="cg", max_iters=args.iters, step_size=0.05, tol=0.0,
                                              jacobi=args.jacobi)
        dt = time.perf_counter() - t0
        if k >= args.warmup:
            times.append(dt)
    out = {"nv": nv, "nf": nf, "median_s": float(np.median(times)), "min_s": float(np.min(times)),
           "max_s": float(np.max(times)), "jacobi": bool(args.jacobi), "iterations": int(iters), "evaluations": int(evals),
           "launches": dm.tilt_splay_twist_stats()}
    dm.close()
    return out


if args.mode == "kernels":
    out = {"mode": "kernels", "result": kernels()}
else:
    out = {"mode": "relax",
           "workload": f"icosphere f={args.freq}: CG relaxation of {args.iters} iterations of tilt_in + tilt_splay_twist_in, "
                       f"{'Jacobi-preconditioned' if args.jacobi else 'plain'} CG, median of {args.runs} runs after {args.warmup}",
           "result": relax()}
print(json.dumps(out), flush=True)
