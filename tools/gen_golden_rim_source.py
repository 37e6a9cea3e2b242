#!/usr/bin/env python3
"""Generate tests/golden/rim_source_cases.npz, rim_source_milestone_c.npz and traj_*_rimsource_*.npz by running the
REFERENCE's tilt_rim_source_in / tilt_rim_source_out modules.

    PYTHONDONTWRITEBYTECODE=1 python3 tools/gen_golden_rim_source.py [--reference DIR]

Data only: deterministic inputs and what the reference's modules/energy/tilt_rim_source_in.py, its _out twin, the
leaflet relaxation and the Minimizer made of them.  Every fixture is asserted to have the property it is named for
before it is written, and every trajectory is rerun from positions perturbed by 1e-13 and must keep its accept / reject
sequence and its step sizes.

Line-search protocol of the trajectories.  The device step keeps, after a rejected trial, the tilts projected onto that
trial's surface: the reference's mesh-mutating line search (a stepper whose ``step`` takes no ``trial_energy_fn``), as
in every leaflet trajectory of oracle/gen_golden.py.  The two fixed-frame trajectories are generated that way and carry
the rejected trials.  The follow-mode trajectory pins the reference's array fast path instead (``trial_energy_fn``
accepted): there the mesh stays at the search's baseline, so tilt_rim_source_in.py:318 gives every trial the BASELINE
center while midpoints and lengths are the trial's.  With every trial accepted the two protocols differ in nothing but
that center, so the fixture is asserted to accept every trial, in both protocols, and to differ from the mesh-mutating
run in every trial energy.  Its module list leaves tilt_smoothness out: on the fast path the reference evaluates that
module with cotangent weights cached for the mesh's positions, not the trial's, which no device lane reproduces.
"""

from __future__ import annotations

import argparse
import importlib
import io
import json
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
from geometry.entities import Edge, Facet, Mesh, Vertex  # noqa: E402
from geometry.geom_io import load_data, parse_geometry  # noqa: E402
from runtime.constraint_manager import ConstraintModuleManager  # noqa: E402
from runtime.energy_manager import EnergyModuleManager  # noqa: E402
from runtime.minimizer import Minimizer  # noqa: E402
from runtime.steppers.conjugate_gradient import ConjugateGradient  # noqa: E402
from runtime.steppers.gradient_descent import GradientDescent  # noqa: E402

from membrane_solver_amd import meshgen  # noqa: E402

REF = {lf: importlib.import_module(f"modules.energy.tilt_rim_source_{lf}") for lf in ("in", "out")}


def save_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps: the same arrays give the same bytes on every run."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for key, val in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(val), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())


def jdump(obj):
    return np.array(json.dumps(obj, sort_keys=True))


def build(P, T, gp, vopts=None, eopts=None, fixed=None):
    """Reference Mesh of the triangles T; edge k of the returned table is the reference's edge k + 1."""
    m = Mesh()
    for i, p in enumerate(P):
        m.vertices[i] = Vertex(i, np.array(p, float), options=dict((vopts or {}).get(i, {})))
        if fixed is not None and fixed[i]:
            m.vertices[i].fixed = True
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


def ring_rows(r):
    """rows of ring r of meshgen.disk_patch (ring r has 6 r vertices, after the center and the rings inside it)"""
    start = 1 + 3 * r * (r - 1)
    return list(range(start, start + 6 * r))


def ring_edge_numbers(edges, rows):
    rs = set(rows)
    return [k for k, (t, h) in enumerate(edges) if int(t) in rs and int(h) in rs]


def tangent_tilts(m, rng, scale):
    pos = m.positions_view()
    tl = scale * rng.normal(size=pos.shape)
    nrm = m.vertex_normals(pos)
    return tl - np.einsum("ij,ij->i", tl, nrm)[:, None] * nrm


def reference_terms(m, lf, positions, tilts):
    """(gamma L dots) per rim edge from the reference's own selection, strengths and frame; None when it has none"""
    mod = REF[lf]
    res = ParameterResolver(m.global_parameters)
    group = mod._resolve_group(res)
    if group is None:
        return None
    payload = mod._rim_selection_payload(m, group=group, mode=mod._resolve_edge_mode(res))
    if payload is None:
        return None
    gamma = np.array([mod._resolve_strength(res, m.edges[int(e)]) for e in payload["edge_ids"]], dtype=float)
    if payload["follow"]:
        center, normal = mod._resolve_followed_circle_frame(m, rows=payload["rim_rows"], normal_row=payload["normal_row"])
    elif lf == "in":
        center, normal = mod._fixed_circle_frame(m, res, normal_row=payload["normal_row"])
    else:
        center, normal = mod._resolve_center(res), np.array([0.0, 0.0, 1.0])
    p0, p1 = positions[payload["tails"]], positions[payload["heads"]]
    r = 0.5 * (p0 + p1) - center[None, :]
    r = r - (r @ normal)[:, None] * normal[None, :]
    rn = np.linalg.norm(r, axis=1)
    r_hat = np.zeros_like(r)
    r_hat[rn > 1e-12] = r[rn > 1e-12] / rn[rn > 1e-12][:, None]
    dots = np.einsum("ij,ij->i", 0.5 * (tilts[payload["tails"]] + tilts[payload["heads"]]), r_hat)
    return {"terms": gamma * np.linalg.norm(p1 - p0, axis=1) * dots, "rn": rn, "gamma": gamma,
            "follow": bool(payload["follow"]), "n_edges": len(gamma)}


def gen_cases():
    meshes = {"disk4": meshgen.disk_patch(4), "disk6": meshgen.disk_patch(6, bulge=0.3, jitter=0.02, seed=11)}
    out, names = {}, []
    for mname, (P, T, B) in meshes.items():
        n_rings = 4 if mname == "disk4" else 6
        brows = [int(i) for i in np.flatnonzero(B)]
        r3 = ring_rows(3)
        m0, edges0 = build(P, T, {})
        e_ring3 = ring_edge_numbers(edges0, r3)
        e_bnd = ring_edge_numbers(edges0, brows)
        assert len(e_ring3) == 18 and len(e_bnd) == 6 * n_rings
        tilted = (np.array([0.2, -0.1, 1.0]) / np.linalg.norm([0.2, -0.1, 1.0])).tolist()
        grp = lambda rows, name="rim", **extra: {int(r): dict({"pin_to_circle_group": name}, **extra) for r in rows}  # noqa: E731
        per_edge = {}
        for j, k in enumerate(e_ring3):
            if j % 3 == 0:
                per_edge[k] = {"tilt_rim_source_strength_in": 1.5 + 0.25 * j}
            elif j % 3 == 1:
                per_edge[k] = {"tilt_rim_source_strength_in": 0.0}
        mid_k = e_bnd[5]
        mid_center = (0.5 * (P[edges0[mid_k, 0]] + P[edges0[mid_k, 1]])).tolist()
        # the "default" group: the key with value None on some rim vertices, other options without the key on the others
        dflt = {int(r): ({"pin_to_circle_group": None} if j % 2 else {"constraints": ["pin_to_circle"]})
                for j, r in enumerate(brows)}
        cases = {
            "a_boundary_global": ("in", grp(brows), {}, {"tilt_rim_source_group_in": "rim", "tilt_rim_source_strength_in": 2.5}, None),
            "a_default_group": ("in", dflt, {}, {"tilt_rim_source_group_in": "default", "tilt_rim_source_strength_in": 1.25}, None),
            "b_ring3_all_per_edge": ("in", grp(r3), per_edge, {"tilt_rim_source_group_in": "rim", "tilt_rim_source_edge_mode": "all",
                                                              "tilt_rim_source_strength_in": None}, None),
            "c_contact_keys": ("in", grp(brows), {}, {"tilt_rim_source_group_in": "rim", "tilt_rim_source_contact_h": 0.7,
                                                      "tilt_rim_source_contact_delta_epsilon_over_a_in": 3.0}, None),
            "c_contact_si": ("in", grp(brows), {}, {"tilt_rim_source_group_in": "rim", "tilt_rim_source_contact_h_in": 2.0e-9,
                                                    "tilt_rim_source_contact_delta_epsilon": 4.0e-21,
                                                    "tilt_rim_source_contact_a": 0.5e-18,
                                                    "tilt_rim_source_contact_units": "si",
                                                    "tilt_rim_source_contact_length_unit_m": 1.0e-8,
                                                    "tilt_rim_source_contact_kappa_ref_J": 4.0e-20}, None),
            "c_contact_gamma": ("in", grp(brows), {}, {"tilt_rim_source_group_in": "rim", "tilt_rim_source_contact_gamma": 0.9}, None),
            "d_tilted_frame": ("in", grp(r3, pin_to_circle_normal=[0.2, -0.1, 1.0]), {},
                               {"tilt_rim_source_group_in": "rim", "tilt_rim_source_edge_mode": "all",
                                "tilt_rim_source_strength_in": 3.0, "tilt_rim_source_center": [0.07, -0.04, 0.11]}, None),
            "e_center_on_midpoint": ("in", grp(brows), {}, {"tilt_rim_source_group_in": "rim", "tilt_rim_source_strength_in": 2.0,
                                                            "tilt_rim_source_center": mid_center}, None),
            "f_follow": ("in", grp(r3, pin_to_circle_mode="fit", pin_to_circle_normal=tilted), {},
                         {"tilt_rim_source_group_in": "rim", "tilt_rim_source_edge_mode": "all",
                          "tilt_rim_source_strength_in": 1.75, "tilt_rim_source_center": [5.0, 5.0, 5.0]}, None),
            "f_follow_moved": ("in", grp(r3, pin_to_circle_mode="fit", pin_to_circle_normal=tilted), {},
                               {"tilt_rim_source_group_in": "rim", "tilt_rim_source_edge_mode": "all",
                                "tilt_rim_source_strength_in": 1.75}, "moved"),
            "g_out_leaflet": ("out", grp(r3, pin_to_circle_normal=[0.2, -0.1, 1.0]), {},
                              {"tilt_rim_source_group_out": "rim", "tilt_rim_source_edge_mode": "all",
                               "tilt_rim_source_strength_out": 2.25, "tilt_rim_source_contact_gamma_in": 9.0}, None),
            "g_out_follow": ("out", grp(brows, pin_to_circle_mode="fit", pin_to_circle_normal=[0.0, 0.0, 2.0]), {},
                             {"tilt_rim_source_group_out": "rim", "tilt_rim_source_contact_gamma_out": 1.1}, None),
            "h_no_group": ("in", grp(brows), {}, {"tilt_rim_source_strength_in": 2.0}, None),
            "h_all_gamma_zero": ("in", grp(brows), {}, {"tilt_rim_source_group_in": "rim", "tilt_rim_source_strength_in": 0.0}, None),
            "h_boundary_mode_interior": ("in", grp(r3), {}, {"tilt_rim_source_group_in": "rim", "tilt_rim_source_strength_in": 2.0}, None),
        }
        for cname, (lf, vo, eo, gp, moved) in cases.items():
            gp = {k: v for k, v in gp.items() if v is not None}
            name = f"{mname}_{cname}"
            m, edges = build(P, T, gp, vopts=vo, eopts=eo)
            rng = np.random.default_rng(5)
            tin, tout = tangent_tilts(m, rng, 0.3), tangent_tilts(m, rng, 0.25)
            pos = m.positions_view().copy()
            if moved:  # evaluated on positions that are not the mesh's: the followed center stays the mesh's (:318)
                pos = pos + 0.03 * np.random.default_rng(9).normal(size=pos.shape)
            res = ParameterResolver(m.global_parameters)
            g = np.zeros_like(pos)
            tg = np.zeros_like(pos)
            kw = {"tilt_in_grad_arr": tg} if lf == "in" else {"tilt_out_grad_arr": tg}
            E = REF[lf].compute_energy_and_gradient_array(m, m.global_parameters, res, positions=pos,
                                                          index_map=m.vertex_index_to_row, grad_arr=g, tilts_in=tin,
                                                          tilts_out=tout, **kw)
            E2 = REF[lf].compute_energy_array(m, m.global_parameters, res, positions=pos, index_map=m.vertex_index_to_row,
                                              tilts_in=tin, tilts_out=tout)
            assert E2 == E and not g.any()
            terms = reference_terms(m, lf, pos, tin if lf == "in" else tout)
            if cname.startswith("h_"):
                assert E == 0.0 and not tg.any(), name
                scale = 0.0
            else:
                assert terms is not None and abs(-terms["terms"].sum() - E) <= 1e-13 * np.abs(terms["terms"]).sum(), name
                scale = float(np.abs(terms["terms"]).sum())
                assert E != 0.0 and tg.any()
                if cname == "b_ring3_all_per_edge":
                    assert (terms["gamma"] == 0).sum() == 12 and (terms["gamma"] != 0).sum() == 6
                if cname == "e_center_on_midpoint":
                    assert (terms["rn"] <= 1e-12).sum() == 1
                if cname.startswith("f_") or cname == "g_out_follow":
                    assert terms["follow"]
                if cname == "c_contact_si":
                    assert abs(terms["gamma"][0] - 2.0e-9 * (4.0e-21 / 0.5e-18) * 1.0e-8 / 4.0e-20) < 1e-18
            if not moved:  # (the dict API evaluates the mesh's own positions and tilts)
                m.set_tilts_in_from_array(tin)
                m.set_tilts_out_from_array(tout)
                Ed, gd, tgd = REF[lf].compute_energy_and_gradient(m, m.global_parameters, res)
                assert abs(Ed - E) <= 1e-13 * max(scale, 1e-300) and gd == {}
                assert sorted(tgd) == [int(r) for r in np.flatnonzero(np.any(tg != 0.0, axis=1))]
            out.update({name + "__positions": m.positions_view().copy(), name + "__eval_positions": pos,
                        name + "__tri": np.asarray(T, dtype=np.int32), name + "__edges": edges,
                        name + "__vopts": jdump({str(k): v for k, v in vo.items()}),
                        name + "__eopts": jdump({str(k): v for k, v in eo.items()}), name + "__gp": jdump(gp),
                        name + "__leaflet": np.array(lf), name + "__tilts_in": tin, name + "__tilts_out": tout,
                        name + "__E": np.array(float(E)), name + "__tilt_grad": tg, name + "__E_scale": np.array(scale),
                        name + "__n_rim_edges": np.array(0 if terms is None else terms["n_edges"])})
            names.append(name)
            print("%-34s rim edges %3d E=% .16g scale=%.6g" % (name, 0 if terms is None else terms["n_edges"], E, scale))
    out["names"] = np.array(names)
    save_npz(os.path.join(OUT, "rim_source_cases.npz"), out)


# ---------------------------------------------------------------------------------------------------------------------
def set_fields(m, seed, scale, fixed_in_every=0, fixed_out_every=0):
    rng = np.random.default_rng(seed)
    tin, tout = tangent_tilts(m, rng, scale), tangent_tilts(m, rng, 0.8 * scale)
    m.set_tilts_in_from_array(tin)
    m.set_tilts_out_from_array(tout)
    nv = len(m.vertex_ids)
    fin, fout = np.zeros(nv, bool), np.zeros(nv, bool)
    if fixed_in_every:
        fin[::fixed_in_every] = True
        for i in np.flatnonzero(fin):
            m.vertices[int(i)].tilt_fixed_in = True
    if fixed_out_every:
        fout[1::fixed_out_every] = True
        for i in np.flatnonzero(fout):
            m.vertices[int(i)].tilt_fixed_out = True
    return tin, tout, fin, fout


def run_once(P, T, gp, vo, mods, stepper_cls, n_steps, step_size, fixed, fast_path, fixed_every):
    m, edges = build(P, T, gp, vopts=vo, fixed=fixed)
    tin, tout, fin, fout = set_fields(m, 33, 0.3, *fixed_every)
    m.energy_modules = list(mods)
    m.constraint_modules = []
    stepper = stepper_cls()
    mz = Minimizer(m, m.global_parameters, stepper, EnergyModuleManager(m.energy_modules),
                   ConstraintModuleManager(m.constraint_modules), quiet=True, step_size=step_size)
    log = []
    orig = stepper.step
    if fast_path:
        def logged(mesh, grad, step_size, energy_fn, constraint_enforcer=None, trial_energy_fn=None):
            assert trial_energy_fn is not None
            r = orig(mesh, grad, step_size, energy_fn, constraint_enforcer=constraint_enforcer,
                     trial_energy_fn=trial_energy_fn)
            log.append((float(bool(r[0])), float(r[1]), float(r[2])))
            return r
    else:
        def logged(mesh, grad, step_size, energy_fn, constraint_enforcer=None):
            r = orig(mesh, grad, step_size, energy_fn, constraint_enforcer=constraint_enforcer)
            log.append((float(bool(r[0])), float(r[1]), float(r[2])))
            return r
    stepper.step = logged
    pos0 = m.positions_view().copy()
    E0, g0 = mz.compute_energy_and_gradient_array()
    res = mz.minimize(n_steps)
    return {"positions0": pos0, "tri": np.asarray(m.triangle_row_cache()[0], dtype=np.int32), "fixed": m.fixed_mask.copy(),
            "edges": edges, "vopts": jdump({str(k): v for k, v in vo.items()}), "tilt_fixed_in": fin, "tilt_fixed_out": fout,
            "gamma": m.get_facet_parameter_array("surface_tension").copy(), "E0": np.array(E0), "grad0": np.array(g0),
            "tilts_in0": tin, "tilts_out0": tout, "positions_final": m.positions_view().copy(),
            "tilts_in_final": np.ascontiguousarray(m.tilts_in_view()).copy(),
            "tilts_out_final": np.ascontiguousarray(m.tilts_out_view()).copy(), "step_log": np.array(log),
            "E_final": np.array(res["energy"]), "n_steps": np.array(n_steps), "step_size0": np.array(step_size),
            "gp_json": jdump(gp), "modules": np.array(list(mods)), "stepper": np.array(stepper_cls.__name__),
            "fast_path": np.array(bool(fast_path))}


def run_traj(fname, P, T, gp, vo, mods, stepper_cls, n_steps, step_size, fixed, check, fast_path=False, fixed_every=(0, 0)):
    out = run_once(P, T, gp, vo, mods, stepper_cls, n_steps, step_size, fixed, fast_path, fixed_every)
    L = out["step_log"]
    check(L, out)
    # stability: the same run from positions perturbed by 1e-13 keeps every decision and every step size
    Pp = np.asarray(P, dtype=float) + 1e-13 * np.random.default_rng(77).normal(size=np.shape(P))
    again = run_once(Pp, T, gp, vo, mods, stepper_cls, n_steps, step_size, fixed, fast_path, fixed_every)["step_log"]
    assert again.shape == L.shape and np.array_equal(again[:, 0], L[:, 0]) and np.allclose(again[:, 1], L[:, 1], rtol=1e-9), fname
    save_npz(os.path.join(OUT, fname), out)
    print(fname, "E_final=%.16g" % out["E_final"], L[:, :2].tolist())
    return out


def gen_trajectories():
    quiet = {"mesh_quality_auto_repair_enabled": False, "volume_constraint_mode": "lagrange",
             "volume_projection_during_minimization": False}
    P6, T6, B6 = meshgen.disk_patch(6, bulge=0.3, jitter=0.02, seed=11)
    P5, T5, B5 = meshgen.disk_patch(5, bulge=0.3, jitter=0.02, seed=7)
    r3 = ring_rows(3)
    vo = {int(r): {"pin_to_circle_group": "rim", "pin_to_circle_normal": [0.0, 0.0, 1.0]} for r in r3}
    base = dict(quiet, surface_tension=1.0, tilt_modulus_in=2.0, tilt_modulus_out=1.4, bending_modulus=0.6,
                tilt_rim_source_group_in="rim", tilt_rim_source_strength_in=0.8, tilt_rim_source_edge_mode="all",
                tilt_rim_source_center=[0.02, -0.01, 0.0])

    def some_trial_rejected(step0):
        def check(L, _out):
            # an accepted step whose alpha lies below the step size it was given: a trial before it was rejected
            assert (L[:, 0] > 0).sum() >= 3, L
            given = np.concatenate([[step0], L[:-1, 1]])
            assert np.any((L[:, 0] > 0) & (L[:, 1] < 1.5 * given * 0.999)), L
        return check

    # 1: GD + nested CG relaxation, fixed frame, boundary vertices fixed, a first step that backtracks
    mods1 = ["tilt_in", "tilt_out", "tilt_smoothness_in", "tilt_rim_source_in"]
    run_traj("traj_disk6_gd_rimsource_nested_cg.npz", P6, T6,
             dict(base, tilt_solve_mode="nested", tilt_solver="cg", tilt_step_size=0.05, tilt_inner_steps=5),
             vo, mods1, GradientDescent, 5, 0.5, B6, some_trial_rejected(0.5), fixed_every=(7, 0))
    # 2: CG + coupled relaxation, both leaflets' bending_tilt and the outer rim source as well
    mods2 = ["tilt_in", "tilt_out", "tilt_smoothness_in", "bending_tilt_in", "bending_tilt_out", "tilt_rim_source_in",
             "tilt_rim_source_out"]

    def some_accepted(L, _out):
        assert (L[:, 0] > 0).sum() >= 3, L

    run_traj("traj_disk6_cg_rimsource_coupled_gd.npz", P6, T6,
             dict(base, tilt_solve_mode="coupled", tilt_solver="gd", tilt_step_size=0.03, tilt_coupled_steps=3,
                  tilt_rim_source_group_out="rim", tilt_rim_source_contact_gamma_out=-0.5, spontaneous_curvature=0.05),
             vo, mods2, ConjugateGradient, 5, 2e-3, B6, some_accepted)
    # 3: follow mode without an enforcer, the reference's array fast path: every trial takes the BASELINE center
    vof = {int(r): {"pin_to_circle_group": "rim", "pin_to_circle_mode": "fit", "pin_to_circle_normal": [0.0, 0.0, 1.0]}
           for r in r3}
    gpf = dict(base, tilt_rim_source_strength_in=3.0)
    gpf.pop("tilt_rim_source_center")

    # (no tilt_smoothness here: on the array fast path the reference evaluates it with the cotangent weights cached for
    # the MESH's positions, whatever positions it is handed -- another property of that path, and not this module's)
    mods3 = ["surface", "tilt_in", "tilt_out", "tilt_rim_source_in"]

    def all_accepted(L, _out):
        assert len(L) == 4 and (L[:, 0] > 0).all(), L
        assert np.allclose(L[:, 1], 1.5 * np.concatenate([[2e-2], L[:-1, 1]]), rtol=1e-12), L  # (no trial rejected)

    fast = run_traj("traj_disk5_gd_rimsource_follow_fastpath.npz", P5, T5, gpf, vof, mods3, GradientDescent, 4, 2e-2,
                    B5, all_accepted, fast_path=True)
    slow = run_once(P5, T5, gpf, vof, mods3, GradientDescent, 4, 2e-2, B5, False, (0, 0))
    all_accepted(slow["step_log"], slow)  # the same decisions: what differs is the center the trials were given
    diff = np.abs(fast["step_log"][:, 2] - slow["step_log"][:, 2]) / np.abs(fast["step_log"][:, 2])
    print("follow quirk: trial energies differ from the mesh-mutating run by", diff.tolist())
    assert diff.min() > 1e-9, "the baseline-center quirk does not show in this trajectory"


# ---------------------------------------------------------------------------------------------------------------------
def gen_milestone_c():
    """The reference's benchmark of one nested leaflet relaxation (benchmarks/benchmark_tilt_relaxation.py) on
    meshes/caveolin/kozlov_annulus_milestone_c_soft_source.yaml: 50 inner steps, step 0.05, tilt_tol 0."""
    deck = os.path.join(args.reference, "meshes", "caveolin", "kozlov_annulus_milestone_c_soft_source.yaml")
    mesh = parse_geometry(load_data(deck))
    mesh.global_parameters.update({"tilt_solve_mode": "nested", "tilt_inner_steps": 50, "tilt_step_size": 0.05,
                                   "tilt_tol": 0.0})
    mz = Minimizer(mesh, mesh.global_parameters, GradientDescent(), EnergyModuleManager(mesh.energy_modules),
                   ConstraintModuleManager(mesh.constraint_modules), quiet=True)
    mz.enforce_constraints_after_mesh_ops(mesh)
    mesh.project_tilts_to_tangent()
    positions = mesh.positions_view()
    pos0 = positions.copy()
    tin0, tout0 = np.array(mesh.tilts_in_view(), copy=True), np.array(mesh.tilts_out_view(), copy=True)
    mgr = mz._tilt_relaxation_manager
    count = [0]

    def counted(fn):
        def wrapper(*a, **k):
            count[0] += 1
            return fn(*a, **k)
        return wrapper

    mgr.compute_energy_and_leaflet_tilt_gradients_array_fn = counted(mgr.compute_energy_and_leaflet_tilt_gradients_array_fn)
    mgr.compute_tilt_dependent_energy_with_leaflet_tilts_fn = counted(mgr.compute_tilt_dependent_energy_with_leaflet_tilts_fn)
    assert mz._uses_leaflet_tilts()
    mz._relax_leaflet_tilts(positions=positions, mode="nested")
    assert np.array_equal(mesh.positions_view(), pos0)
    rows = mesh.vertex_index_to_row
    tri = np.asarray(mesh.triangle_row_cache()[0], dtype=np.int32)
    edges = np.array([[rows[mesh.edges[e].tail_index], rows[mesh.edges[e].head_index]] for e in sorted(mesh.edges)],
                     dtype=np.int64)
    keep = ("pin_to_circle_group", "pin_to_circle_normal", "pin_to_circle_mode")
    vo, group = {}, []
    fin, fout = np.zeros(len(rows), bool), np.zeros(len(rows), bool)
    for vid, v in mesh.vertices.items():
        o = {k: v.options[k] for k in keep if k in (v.options or {})}
        if o:
            vo[str(rows[vid])] = o
        group.append(str((v.options or {}).get("pin_to_circle_group", "")))
        fin[rows[vid]] = bool(getattr(v, "tilt_fixed_in", False))
        fout[rows[vid]] = bool(getattr(v, "tilt_fixed_out", False))
    res = ParameterResolver(mesh.global_parameters)
    tin, tout = np.array(mesh.tilts_in_view(), copy=True), np.array(mesh.tilts_out_view(), copy=True)
    E_rim = REF["in"].compute_energy_array(mesh, mesh.global_parameters, res, positions=positions,
                                           index_map=rows, tilts_in=tin, tilts_out=tout)
    E_total = float(mz.compute_energy())
    gp = {k: v for k, v in mesh.global_parameters.to_dict().items()
          if isinstance(v, (int, float, str, bool, list)) and (k.startswith(("tilt_", "bending_", "pin_to_circle",
                                                                             "spontaneous_", "surface_")))}
    n_rim = reference_terms(mesh, "in", positions, tin)["n_edges"]
    assert len(rows) == 24 and len(tri) == 32 and n_rim == 8 and reference_terms(mesh, "in", positions, tin)["follow"]
    print("milestone C: E_rim=%.16g E_total=%.16g evaluations=%d" % (E_rim, E_total, count[0]))
    assert abs(E_rim - (-5766.9967)) < 1e-3 and abs(E_total - (-2883.5217)) < 1e-3
    save_npz(os.path.join(OUT, "rim_source_milestone_c.npz"),
             {"positions": pos0, "tri": tri, "edges": edges, "vertex_group": np.array(group), "vopts": jdump(vo),
              "tilt_fixed_in": fin, "tilt_fixed_out": fout, "gp_json": jdump(gp),
              "modules": np.array(list(mesh.energy_modules)), "tilts_in0": tin0, "tilts_out0": tout0,
              "tilts_in_final": tin, "tilts_out_final": tout, "E_rim": np.array(float(E_rim)),
              "E_total": np.array(E_total), "n_evaluations": np.array(count[0])})


if __name__ == "__main__":
    gen_cases()
    gen_milestone_c()
    gen_trajectories()
