#!/usr/bin/env python3
"""Generate tests/golden/edge_penalty_cases.npz and traj_*_edgepen*.npz by running the REFERENCE's edge_length_penalty
module.

    PYTHONDONTWRITEBYTECODE=1 python3 tools/gen_golden_edge_penalty.py [--reference DIR]

Data only: deterministic inputs and what the reference's modules/energy/edge_length_penalty.py (and, where both edge
modules are on, line_tension.py) and Minimizer made of them.  Every trajectory fixture is asserted to have the property
it is named for before it is written, and is run a second time from start positions perturbed by 1e-13 relative: the
accept / reject sequence and the step sizes must not change, so no fixture hangs on a rounding-level Armijo decision.
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
from geometry.geom_io import load_data, parse_geometry  # noqa: E402
from modules.energy import edge_length_penalty as ref_pen  # noqa: E402
from modules.energy import line_tension as ref_line  # noqa: E402
from runtime.constraint_manager import ConstraintModuleManager  # noqa: E402
from runtime.energy_manager import EnergyModuleManager  # noqa: E402
from runtime.minimizer import Minimizer  # noqa: E402
from runtime.refinement import refine_polygonal_facets, refine_triangle_mesh  # noqa: E402
from runtime.steppers.conjugate_gradient import ConjugateGradient  # noqa: E402
from runtime.steppers.gradient_descent import GradientDescent  # noqa: E402

from membrane_solver_amd import meshgen  # noqa: E402

PEN = "edge_length_penalty"


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


def rim_edges(T):
    """edges with one facet: the open boundary"""
    _rows, facets = edge_table(T)
    return [k for k, f in enumerate(facets) if len(f) == 1]


def lengths(P, rows):
    return np.linalg.norm(P[rows[:, 1]] - P[rows[:, 0]], axis=1)


def targets(P, T, keep=lambda k: True, tag=True):
    """{edge: options} with targets at 0.9 / 1.1 of the initial length, alternating, on the edges ``keep`` selects"""
    rows, _f = edge_table(T)
    ln = lengths(np.asarray(P, float), rows)
    eo = {}
    for k in range(len(rows)):
        if keep(k):
            eo[k] = {"target_length": float((0.9 if k % 2 == 0 else 1.1) * ln[k])}
            if tag:
                eo[k]["energy"] = [PEN]
    return eo


def gen_cases():
    Pd, Td, _Bd = meshgen.disk_patch(5)
    P4, T4 = ico(4)
    P8u, T8 = meshgen.icosphere(8)
    rows4, _f = edge_table(T4)
    ln4 = lengths(P4, rows4)
    rim = rim_edges(Td)
    assert len(rim) == 30, len(rim)
    third = targets(P4, T4, keep=lambda k: k % 3 != 2)
    all8 = targets(P8u, T8)
    assert len(all8) == 1920
    # every way an edge is selected and then charged or not (edge_length_penalty.py:16-22, :40-42)
    mixed = {}
    for k in range(len(rows4)):
        L0 = float((0.9 if k % 2 == 0 else 1.1) * ln4[k])
        j = k % 8
        if j == 0:
            mixed[k] = {"energy": PEN}                                   # tagged by a string, no target: not charged
        elif j == 1:
            mixed[k] = {"energy": [PEN], "target_length": None}          # tagged, target None: not charged
        elif j == 2:
            mixed[k] = {"target_length": L0}                             # a target and no tag: charged
        elif j == 3:
            mixed[k] = {"energy": "surface", "target_length": L0}        # another module's tag and a target: charged
        elif j == 4:
            mixed[k] = {"energy": ["surface", PEN], "target_length": L0}  # a list that contains it
        elif j == 5:
            mixed[k] = {"energy": PEN, "target_length": L0, "edge_stiffness": 7.0}  # (the edge's own k is ignored)
        elif j == 6:
            mixed[k] = {"energy": ["surface"]}                           # neither
    n_mixed = sum(1 for o in mixed.values() if o.get("target_length") is not None)
    # one charged edge collapsed: its head moved onto its tail
    P4c = P4.copy()
    kc = next(k for k in sorted(third) if k > 40)
    P4c[rows4[kc, 1]] = P4c[rows4[kc, 0]]
    # both edge modules on the same edges
    both = {k: dict(o, energy=["line_tension", PEN]) for k, o in targets(P4, T4, keep=lambda k: k % 4 == 0).items()}
    cases = {
        "ico4_third_untargeted": (P4, T4, third, {"edge_stiffness": 40.0}),
        "ico8_all_edges": (P8u, T8, all8, {"edge_stiffness": 25.0}),
        "disk5_rim_target_zero": (Pd, Td, {k: {"energy": [PEN], "target_length": 0.0} for k in rim},
                                  {"edge_stiffness": 3.0}),
        "ico4_tag_and_target_mixed": (P4, T4, mixed, {"edge_stiffness": 60.0}),
        "ico4_default_stiffness": (P4, T4, third, {}),
        "ico4_zero_stiffness": (P4, T4, third, {"edge_stiffness": 0.0}),
        "ico4_one_edge_collapsed": (P4c, T4, third, {"edge_stiffness": 40.0}),
        "ico4_both_edge_modules": (P4, T4, both, {"edge_stiffness": 40.0, "line_tension": 0.75}),
    }
    out, names = {}, []
    for name, (P, T, eo, gp) in cases.items():
        m, edges = build(P, T, gp, eopts=eo)
        pos = m.positions_view().copy()
        g = np.zeros_like(pos)
        res = ParameterResolver(m.global_parameters)
        E = ref_pen.compute_energy_and_gradient_array(m, m.global_parameters, res, positions=pos,
                                                      index_map=m.vertex_index_to_row, grad_arr=g)
        n_charged = sum(1 for e in ref_pen._edges_to_constrain(m) if m.edges[e].options.get("target_length") is not None)
        out.update({name + "__positions": pos, name + "__tri": np.asarray(T, dtype=np.int32), name + "__edges": edges,
                    name + "__eopts": np.array(repr(eo)), name + "__gp": np.array(repr(gp)),
                    name + "__energy": np.array(float(E)), name + "__grad": g, name + "__n_charged": np.array(n_charged)})
        if "line_tension" in gp:  # the other edge module's share, from the reference's line_tension.py
            gl = np.zeros_like(pos)
            El = ref_line.compute_energy_and_gradient_array(m, m.global_parameters, res, positions=pos,
                                                            index_map=m.vertex_index_to_row, grad_arr=gl)
            assert El > 0.0
            out.update({name + "__energy_line": np.array(float(El)), name + "__grad_line": gl})
        names.append(name)
        print("%-26s nf=%5d options=%5d charged=%5d E=%.16g max|g|=%.6g" % (name, len(T), len(eo), n_charged, E,
                                                                            np.abs(g).max()))
    assert int(out["ico4_tag_and_target_mixed__n_charged"]) == n_mixed and 0 < n_mixed < len(mixed)
    assert out["ico4_zero_stiffness__energy"] == 0.0 and not out["ico4_zero_stiffness__grad"].any()
    assert abs(out["ico4_default_stiffness__energy"] - 2.5 * out["ico4_third_untargeted__energy"]) \
        <= 1e-12 * out["ico4_default_stiffness__energy"]  # k = 100 against k = 40
    assert int(out["ico4_one_edge_collapsed__n_charged"]) == int(out["ico4_third_untargeted__n_charged"])
    assert int(out["ico8_all_edges__n_charged"]) == 1920
    out["names"] = np.array(names)
    save_npz(os.path.join(OUT, "edge_penalty_cases.npz"), out)


def run_once(m, stepper, n_steps, step_size):
    em = EnergyModuleManager(m.energy_modules)
    cm = ConstraintModuleManager(m.constraint_modules)
    mz = Minimizer(m, m.global_parameters, stepper, em, cm, quiet=True, step_size=step_size)
    log = []
    orig = stepper.step

    def logged(mesh, grad, step_size, energy_fn, constraint_enforcer=None, trial_energy_fn=None):
        r = orig(mesh, grad, step_size, energy_fn, constraint_enforcer=constraint_enforcer,
                 trial_energy_fn=trial_energy_fn)
        log.append((float(bool(r[0])), float(r[1]), float(r[2])))
        return r

    stepper.step = logged
    res = mz.minimize(n_steps)
    return np.array(log), res, mz


def run_traj(fname, make, eopts, stepper_cls, n_steps, step_size, gp, check):
    """``make(perturb)`` builds the reference mesh (a fresh one per run) -> (mesh, edges)."""
    m, edges = make(0.0)
    pos0 = m.positions_view().copy()
    L, res, mz = run_once(m, stepper_cls(), n_steps, step_size)
    rows = m.vertex_index_to_row
    vo = {int(rows[i]): dict(m.vertices[i].options) for i in m.vertices if m.vertices[i].options}
    out = {"positions0": pos0, "tri": np.asarray(m.triangle_row_cache()[0], dtype=np.int32),
           "fixed": m.fixed_mask.copy(), "edges": edges, "vopts": np.array(repr(vo)), "eopts": np.array(repr(eopts)),
           "gp": np.array(repr(dict(gp))),
           "energy_modules": np.array(list(m.energy_modules)), "constraint_modules": np.array(list(m.constraint_modules)),
           "step_log": L, "E_final": np.array(res["energy"]), "positions_final": m.positions_view().copy(),
           "step_size_final": np.array(mz.step_size), "n_steps": np.array(n_steps), "step_size0": np.array(step_size),
           "stepper": np.array(stepper_cls.__name__)}
    if m.bodies:
        b = m.bodies[0]
        out["body_options"] = np.array(repr(dict(b.options)))
        if b.target_volume is not None:
            out["target_volume"] = np.array(float(b.target_volume))
    check(L)
    # no decision of the fixture is a rounding-level one: the same accept / reject sequence and step sizes from start
    # positions perturbed by 1e-13 relative
    m2, _e = make(1e-13)
    L2, _res2, _mz2 = run_once(m2, stepper_cls(), n_steps, step_size)
    assert L2.shape == L.shape and np.array_equal(L2[:, 0], L[:, 0]) and np.array_equal(L2[:, 1], L[:, 1]), (fname, L, L2)
    save_npz(os.path.join(OUT, fname), out)
    print(fname, "E_final=%.16g" % out["E_final"], L.tolist())


def accepted(L):
    return int((L[:, 0] > 0).sum())


def perturbed(P, rel):
    """positions moved by ``rel`` relative, a fixed pattern"""
    P = np.asarray(P, float)
    if rel == 0.0:
        return P
    return P * (1.0 + rel * np.random.default_rng(7).uniform(-1.0, 1.0, P.shape))


def strip_mesh(path, rel):
    """The folding deck's sheet: read by the reference's reader, refined twice (its macro's ``r2``), every edge's target
    its current length (what the "fix edges" command seeds), then a seeded perturbation in z."""
    m = parse_geometry(load_data(path))
    for _ in range(2):
        m = refine_polygonal_facets(m)
        m = refine_triangle_mesh(m)
    m.build_connectivity_maps()
    m.build_facet_vertex_loops()
    eopts = {}
    for k, e in enumerate(m.edges.values()):
        o = {"energy": [PEN], "target_length": float(e.compute_length(m))}
        e.options = dict(e.options or {}, **o)
        eopts[k] = o
    rng = np.random.default_rng(20261019)
    rows = m.vertex_index_to_row
    bump = 0.05 * rng.uniform(-1.0, 1.0, len(rows))
    for vid, v in m.vertices.items():
        if not getattr(v, "fixed", False):
            v.position = np.array(v.position, float) + np.array([0.0, 0.0, bump[rows[vid]]])
    if rel:
        P = perturbed(np.array([m.vertices[v].position for v in m.vertices]), rel)
        for j, vid in enumerate(m.vertices):
            m.vertices[vid].position = P[j]
    m.increment_version()
    edges = np.array([[rows[e.tail_index], rows[e.head_index]] for e in m.edges.values()], dtype=np.int64)
    return m, edges, eopts


def gen_trajectories():
    quiet = {"mesh_quality_auto_repair_enabled": False}
    Pd, Td, Bd = meshgen.disk_patch(5)
    P4, T4 = ico(4)
    P8, T8 = ico(8)

    def some_accepted(L):
        assert accepted(L) >= 3, L

    def accepted_and_falling(L):
        acc = L[L[:, 0] > 0, 2]
        assert len(acc) >= 3 and np.all(np.diff(acc) < 0.0), L

    # a: the sheet of bench_spontaneous_folding.json: helfrich bending with c0 = 2 against inextensible edges, two fixed
    # vertices, no surface module (slot 0 carries the penalty alone), GD
    deck = os.path.join(args.reference, "benchmarks", "inputs", "bench_spontaneous_folding.json")
    gp_a = dict(quiet, bending_modulus=10.0, bending_energy_model="helfrich", spontaneous_curvature=2.0,
                surface_tension=0.0, volume_constraint_mode="none", step_size=0.01, edge_stiffness=100.0)
    _m, _edges, eo_a = strip_mesh(deck, 0.0)

    def make_a(rel):
        m, edges, _eo = strip_mesh(deck, rel)
        for key, val in gp_a.items():
            m.global_parameters.set(key, val)
        assert int(np.asarray(m.fixed_mask).sum()) == 2
        m.energy_modules = ["bending", PEN]
        m.constraint_modules = []
        return m, edges

    run_traj("traj_strip_gd_bending_edgepen.npz", make_a, eo_a, GradientDescent, 6, 1e-4, gp_a, accepted_and_falling)

    # b: closed vesicle, surface + the penalty on two thirds of the edges, GD, a start step that backtracks
    eo4 = targets(P4, T4, keep=lambda k: k % 3 != 2)

    def first_backtracks(L):
        # (an accepted first step whose alpha lies below the step size it was given: some trial before it was rejected)
        assert L[0, 0] > 0 and L[0, 1] < 1.5 * 0.5 * 0.999, L

    gp_b = dict(quiet, surface_tension=1.0, edge_stiffness=20.0)

    def make_b(rel):
        m, edges = build(perturbed(P4, rel), T4, gp_b, eopts=eo4)
        m.energy_modules = ["surface", PEN]
        m.constraint_modules = []
        return m, edges

    run_traj("traj_ico4_gd_edgepen_surface_backtrack.npz", make_b, eo4, GradientDescent, 6, 0.5, gp_b, first_backtracks)

    # c, d: bending + volume row in the KKT + the penalty, CG; ico8 is multi-tile at both tile sizes, so <g,gC> is
    # corrected across workgroups
    def cg_accepts(L):
        assert accepted(L) >= 4, L

    for fname, P, T, n in (("traj_ico4_cg_edgepen_bending_volume_row.npz", P4, T4, 10),
                           ("traj_ico8_cg_edgepen_bending_volume_row.npz", P8, T8, 10)):
        eo = targets(P, T, keep=lambda k: k % 3 != 2)
        gp = dict(quiet, surface_tension=0.0, bending_modulus=1.0, bending_energy_model="helfrich",
                  spontaneous_curvature=0.0, edge_stiffness=20.0, volume_constraint_mode="lagrange",
                  volume_projection_during_minimization=False)

        def make_cd(rel, P=P, T=T, eo=eo, gp=gp):
            m, edges = build(perturbed(P, rel), T, gp, eopts=eo)
            b = Body(0, sorted(m.facets.keys()), target_volume=None, options={})
            m.bodies[0] = b
            b.target_volume = float(b.compute_volume(m))
            m.energy_modules = ["bending", PEN]
            m.constraint_modules = ["volume"]
            return m, edges

        run_traj(fname, make_cd, eo, ConjugateGradient, n, 2e-3, gp, cg_accepts)

    # e: volume projected on every trial (the enforcer lane), GD
    gp_e = dict(quiet, bending_modulus=1.0, bending_energy_model="helfrich", spontaneous_curvature=0.0,
                edge_stiffness=20.0, volume_constraint_mode="lagrange", volume_projection_during_minimization=True)

    def make_e(rel):
        m, edges = build(perturbed(P4, rel), T4, gp_e, eopts=eo4)
        b = Body(0, sorted(m.facets.keys()), target_volume=None, options={})
        m.bodies[0] = b
        b.target_volume = float(b.compute_volume(m))
        m.energy_modules = ["bending", PEN]
        m.constraint_modules = ["volume"]
        return m, edges

    run_traj("traj_ico4_gd_edgepen_bending_volume_enforcer.npz", make_e, eo4, GradientDescent, 6, 1e-2, gp_e,
             some_accepted)

    # f: open disk, surface + both edge modules on the rim + the rim on pin_to_plane, GD
    rim = rim_edges(Td)
    rows_d, _f = edge_table(Td)
    ln_d = lengths(Pd, rows_d)
    eo_f = {k: {"energy": ["line_tension", PEN], "target_length": float(0.9 * ln_d[k])} for k in rim}
    gp_f = dict(quiet, surface_tension=1.0, line_tension=0.8, edge_stiffness=30.0)
    vo_f = {int(i): {"constraints": ["pin_to_plane"]} for i in np.flatnonzero(Bd)}

    def make_f(rel):
        m, edges = build(perturbed(Pd, rel), Td, gp_f, vopts=vo_f, eopts=eo_f)
        m.energy_modules = ["surface", "line_tension", PEN]
        m.constraint_modules = ["pin_to_plane"]
        return m, edges

    run_traj("traj_disk5_gd_edgepen_linetension_surface_pins_plane.npz", make_f, eo_f, GradientDescent, 6, 1e-2, gp_f,
             some_accepted)


if __name__ == "__main__":
    gen_cases()
    gen_trajectories()
