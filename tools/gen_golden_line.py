#!/usr/bin/env python3
"""Generate tests/golden/line_cases.npz and traj_*_line_*.npz by running the REFERENCE's line_tension module.

    PYTHONDONTWRITEBYTECODE=1 python3 tools/gen_golden_line.py [--reference DIR]

Data only: deterministic inputs and what the reference's modules/energy/line_tension.py and Minimizer made of them.
Every trajectory fixture is asserted to have the property it is named for before it is written.
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
from modules.energy import line_tension as ref_line  # noqa: E402
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


def edge_table(T):
    """(ne, 2) tail / head rows in the order build() numbers the edges, and the facets on each edge."""
    emap, rows, facets = {}, [], []
    for fi, (a, b, c) in enumerate(T):
        for u, v in ((a, b), (b, c), (c, a)):
            k = (min(u, v), max(u, v))
            if k not in emap:
                emap[k] = len(rows)
                rows.append((int(u), int(v)))
                facets.append([])
            facets[emap[k]].append(fi)
    return np.array(rows, dtype=np.int64), facets


def build(P, T, gp, vopts=None, eopts=None):
    """Reference Mesh of the triangles T; edge k of edge_table(T) is the reference's edge k + 1."""
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
                m.edges[e] = Edge(e, int(u), int(v), options=dict((eopts or {}).get(e - 1, {})))
                nid += 1
            se.append(e if m.edges[e].tail_index == u else -e)
        m.facets[fi] = Facet(fi, se, options={})
    m.global_parameters = GlobalParameters(dict(gp))
    m.build_connectivity_maps()
    m.build_facet_vertex_loops()
    edges = np.array([[m.edges[e].tail_index, m.edges[e].head_index] for e in sorted(m.edges)], dtype=np.int64)
    return m, edges


def ico(freq):
    P, T = meshgen.icosphere(freq)
    return meshgen.smooth_displace(P, 0.05), T


def upper_facets(P, T, z_min=0.2):
    return np.flatnonzero(P[T].mean(axis=1)[:, 2] > z_min)


def rim_edges(T):
    """edges with one facet: the open boundary"""
    _rows, facets = edge_table(T)
    return [k for k, f in enumerate(facets) if len(f) == 1]


def loop_edges(P, T):
    """edges between a facet of upper_facets and one outside it: the boundary loop of that patch"""
    up = set(int(f) for f in upper_facets(P, T))
    _rows, facets = edge_table(T)
    return [k for k, f in enumerate(facets) if len(f) == 2 and ((f[0] in up) != (f[1] in up))]


def loop_options(loop):
    """every way the reference selects an edge and resolves its gamma, over the edges of one loop"""
    eo = {}
    for j, k in enumerate(loop):
        if j % 3 == 1:
            eo[k] = {"energy": "line_tension", "line_tension": 0.5 + 0.125 * j}  # per-edge override
        elif j % 3 == 2:
            eo[k] = {"energy": ["surface", "line_tension"]}  # a list that contains it, global gamma
        else:
            eo[k] = {"energy": ("line_tension",)}  # a tuple
    eo[loop[0]] = {"line_tension": 1.75}  # tagged by the key alone
    eo[loop[4]] = {"energy": "line_tension", "line_tension": 0.0}  # gamma 0: skipped
    return eo


def gen_cases():
    Pd, Td, _Bd = meshgen.disk_patch(5)
    P4, T4 = ico(4)
    P4u, _ = meshgen.icosphere(4)
    P8u, T8 = meshgen.icosphere(8)
    rim = rim_edges(Td)
    loop = loop_edges(P4, T4)
    assert len(rim) == 30, len(rim)
    assert len(loop) == 22, len(loop)
    all4 = {k: {"energy": "line_tension"} for k in range(len(edge_table(T4)[0]))}
    all8 = {k: {"energy": "line_tension"} for k in range(len(edge_table(T8)[0]))}
    assert len(all8) == 1920
    lo = loop_options(loop)
    # two tagged vertices made coincident: the head of a charged loop edge moved onto its tail
    rows4, _f = edge_table(T4)
    P4c = P4.copy()
    kc = loop[7]
    assert "line_tension" not in lo[kc] or lo[kc]["line_tension"]
    P4c[rows4[kc, 1]] = P4c[rows4[kc, 0]]
    cases = {
        "disk5_rim_global": (Pd, Td, {k: {"energy": ["line_tension"]} for k in rim}, {"line_tension": 1.25}),
        "ico4_loop_mixed": (P4, T4, lo, {"line_tension": 0.75}),
        "ico4_all_edges": (P4u, T4, all4, {"line_tension": 2.0}),
        "ico8_all_edges": (P8u, T8, all8, {"line_tension": 0.5}),
        "ico4_loop_coincident": (P4c, T4, lo, {"line_tension": 0.75}),
        "ico4_nothing_tagged": (P4, T4, {}, {"line_tension": 3.0}),
    }
    out, names = {}, []
    for name, (P, T, eo, gp) in cases.items():
        m, edges = build(P, T, gp, eopts=eo)
        pos = m.positions_view().copy()
        g = np.zeros_like(pos)
        res = ParameterResolver(m.global_parameters)
        E = ref_line.compute_energy_and_gradient_array(m, m.global_parameters, res, positions=pos,
                                                       index_map=m.vertex_index_to_row, grad_arr=g)
        E2, gd = ref_line.compute_energy_and_gradient(m, m.global_parameters, res)
        assert abs(E2 - E) <= 1e-13 * max(abs(E), 1.0)
        n_charged = sum(1 for e in ref_line._edges_with_line_tension(m)
                        if m.edges[e].options.get("line_tension", gp["line_tension"]))
        out.update({name + "__positions": pos, name + "__tri": np.asarray(T, dtype=np.int32), name + "__edges": edges,
                    name + "__eopts": np.array(repr(eo)), name + "__gp": np.array(repr(gp)),
                    name + "__energy": np.array(float(E)), name + "__grad": g, name + "__n_charged": np.array(n_charged)})
        names.append(name)
        print("%-22s nf=%5d tagged=%5d charged=%5d E=%.16g max|g|=%.6g" % (name, len(T), len(eo), n_charged, E,
                                                                          np.abs(g).max()))
    assert out["ico4_loop_coincident__energy"] < out["ico4_loop_mixed__energy"]
    assert out["ico4_nothing_tagged__energy"] == 0.0 and not out["ico4_nothing_tagged__grad"].any()
    out["names"] = np.array(names)
    save_npz(os.path.join(OUT, "line_cases.npz"), out)


def run_traj(fname, m, edges, eopts, stepper, n_steps, step_size, gp, check):
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
    vo = {i: dict(m.vertices[i].options) for i in m.vertices if m.vertices[i].options}
    out = {"positions0": pos0, "tri": np.asarray(m.triangle_row_cache()[0], dtype=np.int32),
           "fixed": m.fixed_mask.copy(), "edges": edges, "vopts": np.array(repr(vo)), "eopts": np.array(repr(eopts)),
           "gp": np.array(repr(dict(gp))),
           "energy_modules": np.array(list(m.energy_modules)), "constraint_modules": np.array(list(m.constraint_modules)),
           "step_log": np.array(log), "E_final": np.array(res["energy"]), "positions_final": m.positions_view().copy(),
           "step_size_final": np.array(mz.step_size), "n_steps": np.array(n_steps), "step_size0": np.array(step_size),
           "stepper": np.array(type(stepper).__name__)}
    if m.bodies:
        b = m.bodies[0]
        out["body_options"] = np.array(repr(dict(b.options)))
        if b.target_volume is not None:
            out["target_volume"] = np.array(float(b.target_volume))
    L = out["step_log"]
    check(L)
    save_npz(os.path.join(OUT, fname), out)
    print(fname, "E_final=%.16g" % out["E_final"], L.tolist())


def accepted(L):
    return int((L[:, 0] > 0).sum())


def gen_trajectories():
    quiet = {"mesh_quality_auto_repair_enabled": False}
    Pd, Td, Bd = meshgen.disk_patch(5)
    rim = rim_edges(Td)
    rim_opts = {k: {"energy": "line_tension"} for k in rim}
    P4, T4 = ico(4)
    P8, T8 = ico(8)

    # a, b: open disk, surface + line tension on the rim, GD; a small first step (six accepted steps) and one that
    # backtracks
    def six_accepted(L):
        assert len(L) == 6 and accepted(L) == 6, L

    def first_backtracks(L):
        # (an accepted first step whose alpha lies below the step size it was given: some trial before it was rejected)
        assert L[0, 0] > 0 and L[0, 1] < 1.5 * 2.0 * 0.999, L

    for fname, step, check in (("traj_disk5_gd_line_surface.npz", 1e-2, six_accepted),
                               ("traj_disk5_gd_line_surface_backtrack.npz", 2.0, first_backtracks)):
        gp = dict(quiet, surface_tension=1.0, line_tension=0.8)
        m, edges = build(Pd, Td, gp, eopts=rim_opts)
        m.energy_modules = ["surface", "line_tension"]
        m.constraint_modules = []
        run_traj(fname, m, edges, rim_opts, GradientDescent(), 6, step, gp, check)

    # c: the soft square-to-circle: rim on pin_to_plane, body_area_penalty + line tension, surface tension 0
    gp = dict(quiet, surface_tension=0.0, line_tension=1.0, area_stiffness=40.0)
    vo = {int(i): {"constraints": ["pin_to_plane"]} for i in np.flatnonzero(Bd)}
    m, edges = build(Pd, Td, gp, vopts=vo, eopts=rim_opts)
    b = Body(0, sorted(m.facets.keys()), target_volume=None, options={})
    m.bodies[0] = b
    pos, idx = m.positions_view(), m.vertex_index_to_row
    A = float(sum(m.facets[f].compute_area_and_gradient(m, positions=pos, index_map=idx)[0] for f in m.facets))
    b.options["area_target"] = 1.1 * A
    m.energy_modules = ["body_area_penalty", "line_tension"]
    m.constraint_modules = ["pin_to_plane"]

    def some_accepted(L):
        assert accepted(L) >= 3, L

    run_traj("traj_disk5_gd_line_softsquare_pins_plane.npz", m, edges, rim_opts, GradientDescent(), 6, 1e-2, gp, some_accepted)

    # d, e: closed vesicle with a domain boundary: bending + volume row + the tagged loop, CG (accepted steps and
    # non-descent restarts); ico8 is multi-tile at both tile sizes
    def cg_accepts_and_restarts(L):
        assert accepted(L) >= 2 and int((L[:, 0] == 0).sum()) >= 1, L

    for fname, P, T, n in (("traj_ico4_cg_line_bending_volume_row.npz", P4, T4, 10),
                           ("traj_ico8_cg_line_bending_volume_row.npz", P8, T8, 10)):
        loop = loop_edges(P, T)
        lo = {k: {"energy": "line_tension"} for k in loop}
        gp = dict(quiet, surface_tension=0.0, bending_modulus=1.0, bending_energy_model="helfrich",
                  spontaneous_curvature=0.0, line_tension=0.6, volume_constraint_mode="lagrange",
                  volume_projection_during_minimization=False)
        m, edges = build(P, T, gp, eopts=lo)
        b = Body(0, sorted(m.facets.keys()), target_volume=None, options={})
        m.bodies[0] = b
        b.target_volume = float(b.compute_volume(m))
        m.energy_modules = ["surface", "bending", "line_tension"]
        m.constraint_modules = ["volume"]
        run_traj(fname, m, edges, lo, ConjugateGradient(), n, 2e-3, gp, cg_accepts_and_restarts)

    # f: volume projected on every trial (the enforcer lane), GD
    loop = loop_edges(P4, T4)
    lo = {k: {"energy": "line_tension"} for k in loop}
    gp = dict(quiet, bending_modulus=1.0, bending_energy_model="helfrich", spontaneous_curvature=0.0,
              line_tension=0.6, volume_constraint_mode="lagrange", volume_projection_during_minimization=True)
    m, edges = build(P4, T4, gp, eopts=lo)
    b = Body(0, sorted(m.facets.keys()), target_volume=None, options={})
    m.bodies[0] = b
    b.target_volume = float(b.compute_volume(m))
    m.energy_modules = ["bending", "line_tension"]
    m.constraint_modules = ["volume"]
    run_traj("traj_ico4_gd_line_bending_volume_enforcer.npz", m, edges, lo, GradientDescent(), 6, 5e-2, gp,
             some_accepted)


if __name__ == "__main__":
    gen_cases()
    gen_trajectories()
