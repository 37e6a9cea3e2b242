#!/usr/bin/env python3
"""Generate tests/golden/area_cases.npz and traj_*_area_*.npz by running the REFERENCE's body_area_penalty.

    PYTHONDONTWRITEBYTECODE=1 python3 tools/gen_golden_area.py [--reference DIR]

Data only: deterministic inputs and what the reference's modules/energy/body_area_penalty.py and Minimizer made of
them.
"""

from __future__ import annotations

import argparse
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "tests", "golden")

ap = argparse.ArgumentParser()
ap.add_argument("--reference", default="/root/reference")
ap.add_argument("--out", default=OUT, help="directory the fixtures are written to")
args = ap.parse_args()
OUT = args.out
os.makedirs(OUT, exist_ok=True)
sys.dont_write_bytecode = True
sys.path.insert(0, args.reference)
sys.path.insert(0, ROOT)

from core.parameters.global_parameters import GlobalParameters  # noqa: E402
from core.parameters.resolver import ParameterResolver  # noqa: E402
from geometry.entities import Body, Edge, Facet, Mesh, Vertex  # noqa: E402
from modules.energy import body_area_penalty as ref_area  # noqa: E402
from runtime.constraint_manager import ConstraintModuleManager  # noqa: E402
from runtime.energy_manager import EnergyModuleManager  # noqa: E402
from runtime.minimizer import Minimizer  # noqa: E402
from runtime.steppers.conjugate_gradient import ConjugateGradient  # noqa: E402
from runtime.steppers.gradient_descent import GradientDescent  # noqa: E402

from membrane_solver_amd import meshgen  # noqa: E402


def save_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps: the same arrays give the same bytes on every run."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for key, val in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(val), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())


def build(P, T, gp, vopts=None):
    """Reference Mesh of the triangles T; returns the mesh and its edge table (tail, head) in edge-id order."""
    m = Mesh()
    for i, p in enumerate(P):
        m.vertices[i] = Vertex(i, np.array(p, float), options=dict((vopts or {}).get(i, {})))
    emap, nid = {}, 1
    for fi, (a, b, c) in enumerate(T):
        se = []
        for u, v in ((a, b), (b, c), (c, a)):
            k = (min(u, v), max(u, v))
            e = emap.get(k)
            if e is None:
                e = nid
                emap[k] = e
                m.edges[e] = Edge(e, int(u), int(v), options={})
                nid += 1
            se.append(e if m.edges[e].tail_index == u else -e)
        m.facets[fi] = Facet(fi, se, options={})
    m.global_parameters = GlobalParameters(dict(gp))
    m.build_connectivity_maps()
    m.build_facet_vertex_loops()
    edges = np.array([[m.edges[e].tail_index, m.edges[e].head_index] for e in sorted(m.edges)], dtype=np.int64)
    return m, edges


def body_area(m, facets):
    pos = m.positions_view()
    idx = m.vertex_index_to_row
    return float(sum(m.facets[f].compute_area_and_gradient(m, positions=pos, index_map=idx)[0] for f in facets))


def add_body(m, facets=None, options=None, target_volume=None):
    """One body over `facets` (None: every facet); returns (body, facet rows, its area at the current positions)."""
    rows = sorted(m.facets.keys()) if facets is None else [int(f) for f in facets]
    b = Body(0, list(rows), target_volume=target_volume, options=dict(options or {}))
    m.bodies[0] = b
    return b, np.array(rows, dtype=np.int64), body_area(m, rows)


def ico(freq):
    P, T = meshgen.icosphere(freq)
    return meshgen.smooth_displace(P, 0.05), T


def upper_facets(P, T, z_min=0.2):
    return np.flatnonzero(P[T].mean(axis=1)[:, 2] > z_min)


def disk5():
    P, T, B = meshgen.disk_patch(5)
    return P, T, B


def gen_cases():
    P4, T4 = ico(4)
    P8, T8 = ico(8)
    Pd, Td, _Bd = disk5()
    up4, up8 = upper_facets(P4, T4), upper_facets(P8, T8)
    # name -> (P, T, body facets | None, global area_stiffness | None, body area_stiffness | None, A0 / A | None)
    cases = {
        "ico4_global_above": (P4, T4, None, 5.0, None, 0.9),
        "ico4_global_below": (P4, T4, None, 5.0, None, 1.1),
        "ico4_body_stiffness": (P4, T4, None, 3.0, 7.0, 0.95),
        "ico4_subset_above": (P4, T4, up4, None, 12.0, 0.8),
        "ico8_global_above": (P8, T8, None, 40.0, None, 0.9),
        "ico8_subset_below": (P8, T8, up8, 2.5, None, 1.2),
        "disk5_global_above": (Pd, Td, None, 9.0, None, 0.7),
        "disk5_body_below": (Pd, Td, None, None, 4.0, 1.3),
        "ico4_no_target": (P4, T4, None, 5.0, None, None),
        "ico4_zero_stiffness": (P4, T4, None, 0.0, None, 0.9),
    }
    out, names = {}, []
    for name, (P, T, facets, k_glob, k_body, ratio) in cases.items():
        gp = {} if k_glob is None else {"area_stiffness": k_glob}
        m, _edges = build(P, T, gp)
        b, rows, A = add_body(m, facets)
        if k_body is not None:
            b.options["area_stiffness"] = k_body
        if ratio is not None:
            b.options["area_target"] = ratio * A
        pos = m.positions_view().copy()
        g = np.zeros_like(pos)
        E = ref_area.compute_energy_and_gradient_array(m, m.global_parameters, ParameterResolver(m.global_parameters),
                                                       positions=pos, index_map=m.vertex_index_to_row, grad_arr=g)
        out.update({name + "__positions": pos, name + "__tri": np.asarray(T, dtype=np.int32),
                    name + "__body_facets": rows, name + "__gp": np.array(repr(gp)),
                    name + "__body_options": np.array(repr(dict(b.options))), name + "__area": np.array(A),
                    name + "__energy": np.array(float(E)), name + "__grad": g})
        names.append(name)
        print("%-22s nf=%5d body=%5d A=%.12f E=%.16g max|g|=%.6g" % (name, len(T), len(rows), A, E, np.abs(g).max()))
    out["names"] = np.array(names)
    save_npz(os.path.join(OUT, "area_cases.npz"), out)


def run_traj(fname, m, edges, stepper, n_steps, step_size, body_rows, extra=None):
    em = EnergyModuleManager(m.energy_modules)
    cm = ConstraintModuleManager(m.constraint_modules)
    mz = Minimizer(m, m.global_parameters, stepper, em, cm, quiet=True, step_size=step_size)
    pos0 = m.positions_view().copy()
    log = []
    orig = stepper.step

    def logged(mesh, grad, step_size, energy_fn, constraint_enforcer=None, trial_energy_fn=None):
        r = orig(mesh, grad, step_size, energy_fn, constraint_enforcer=constraint_enforcer,
                 trial_energy_fn=trial_energy_fn)
        log.append((float(bool(r[0])), float(r[1]), float(r[2])))
        return r

    stepper.step = logged
    res = mz.minimize(n_steps)
    b = m.bodies[0]
    vo = {i: dict(m.vertices[i].options) for i in m.vertices if m.vertices[i].options}
    out = {"positions0": pos0, "tri": np.asarray(m.triangle_row_cache()[0], dtype=np.int32),
           "fixed": m.fixed_mask.copy(), "edges": edges, "vopts": np.array(repr(vo)), "eopts": np.array(repr({})),
           "gp": np.array(repr(dict(extra.pop("gp")))),
           "energy_modules": np.array(list(m.energy_modules)), "constraint_modules": np.array(list(m.constraint_modules)),
           "step_log": np.array(log), "E_final": np.array(res["energy"]), "positions_final": m.positions_view().copy(),
           "step_size_final": np.array(mz.step_size), "n_steps": np.array(n_steps), "step_size0": np.array(step_size),
           "stepper": np.array(type(stepper).__name__),
           "area_target": np.array(float(b.options["area_target"])),
           "area_stiffness": np.array(float(b.options.get("area_stiffness", m.global_parameters.get("area_stiffness")))),
           "body_facets": np.asarray(body_rows, dtype=np.int64), "body_options": np.array(repr(dict(b.options)))}
    if b.target_volume is not None:
        out["target_volume"] = np.array(float(b.target_volume))
    out.update(extra)
    save_npz(os.path.join(OUT, fname), out)
    print(fname, "E_final=%.16g" % out["E_final"], out["step_log"].tolist())


def gen_trajectories():
    quiet = {"mesh_quality_auto_repair_enabled": False}
    P4, T4 = ico(4)
    P8, T8 = ico(8)

    # 1, 2: surface + area penalty, GD, a small and a large first step (the large one backtracks)
    for fname, step in (("traj_ico4_gd_area_surface.npz", 1e-3), ("traj_ico4_gd_area_surface_backtrack.npz", 0.2)):
        gp = dict(quiet, surface_tension=1.0, area_stiffness=50.0)
        m, edges = build(P4, T4, gp)
        b, rows, A = add_body(m, target_volume=None)
        b.options["area_target"] = 0.9 * A
        m.energy_modules = ["surface", "body_area_penalty"]
        m.constraint_modules = []
        run_traj(fname, m, edges, GradientDescent(), 6, step, rows, extra={"gp": gp})

    # 3: bending (gamma = 0) + area penalty, Lagrange volume row with the projection off, CG
    gp = dict(quiet, surface_tension=0.0, bending_modulus=1.0, bending_energy_model="helfrich",
              spontaneous_curvature=0.0, area_stiffness=100.0, volume_constraint_mode="lagrange",
              volume_projection_during_minimization=False)
    m, edges = build(P8, T8, gp)
    b, rows, A = add_body(m, target_volume=None)
    b.target_volume = float(b.compute_volume(m))
    b.options["area_target"] = 1.05 * A
    m.energy_modules = ["surface", "bending", "body_area_penalty"]
    m.constraint_modules = ["volume"]
    run_traj("traj_ico8_cg_area_bending_volume_row.npz", m, edges, ConjugateGradient(), 8, 2e-3, rows, extra={"gp": gp})

    # 4: bending + area penalty, volume projected on every trial (enforcer lane), GD
    gp = dict(quiet, bending_modulus=1.0, bending_energy_model="helfrich", spontaneous_curvature=0.0,
              area_stiffness=20.0, volume_constraint_mode="lagrange", volume_projection_during_minimization=True)
    m, edges = build(P4, T4, gp)
    b, rows, A = add_body(m, target_volume=None)
    b.target_volume = float(b.compute_volume(m))
    b.options["area_target"] = 0.95 * A
    m.energy_modules = ["bending", "body_area_penalty"]
    m.constraint_modules = ["volume"]
    run_traj("traj_ico4_gd_area_bending_volume_enforcer.npz", m, edges, GradientDescent(), 6, 5e-2, rows,
             extra={"gp": gp})

    # 5: surface + volume penalty + area penalty, CG
    gp = dict(quiet, surface_tension=1.0, area_stiffness=50.0, volume_constraint_mode="penalty", volume_stiffness=200.0)
    m, edges = build(P4, T4, gp)
    b, rows, A = add_body(m, target_volume=None)
    b.target_volume = 0.95 * float(b.compute_volume(m))
    b.options["area_target"] = 0.9 * A
    m.energy_modules = ["surface", "volume", "body_area_penalty"]
    m.constraint_modules = []
    run_traj("traj_ico4_cg_area_volume_penalty.npz", m, edges, ConjugateGradient(), 8, 1e-3, rows, extra={"gp": gp})

    # 6: open disk, rim on pin_to_circle, surface + bending + area penalty, GD
    Pd, Td, Bd = disk5()
    gp = dict(quiet, surface_tension=1.0, bending_modulus=1.0, bending_energy_model="helfrich",
              spontaneous_curvature=0.0, area_stiffness=30.0, pin_to_circle_radius=1.0)
    m, edges = build(Pd, Td, gp, vopts={int(i): {"constraints": ["pin_to_circle"]} for i in np.flatnonzero(Bd)})
    b, rows, A = add_body(m, target_volume=None)
    b.options["area_target"] = 1.3 * A
    m.energy_modules = ["surface", "bending", "body_area_penalty"]
    m.constraint_modules = ["pin_to_circle"]
    run_traj("traj_disk5_gd_area_pins_circle.npz", m, edges, GradientDescent(), 6, 1e-3, rows, extra={"gp": gp})

    # 7: a body that owns the facets with centroid z > 0.2 only, stiffness in the body's options, GD
    gp = dict(quiet, surface_tension=1.0)
    m, edges = build(P4, T4, gp)
    b, rows, A = add_body(m, facets=upper_facets(P4, T4), target_volume=None)
    b.options["area_target"] = 0.85 * A
    b.options["area_stiffness"] = 25.0
    m.energy_modules = ["surface", "body_area_penalty"]
    m.constraint_modules = []
    run_traj("traj_ico4_gd_area_subset_body.npz", m, edges, GradientDescent(), 6, 1e-3, rows, extra={"gp": gp})


if __name__ == "__main__":
    gen_cases()
    gen_trajectories()
