#!/usr/bin/env python3
"""Generate tests/golden/tilt_coupling_cases.npz, tilt_coupling_milestone_b.npz and traj_*_coupling_*.npz by running the
REFERENCE's tilt_coupling module, its leaflet relaxation and its Minimizer.

    PYTHONDONTWRITEBYTECODE=1 python3 tools/gen_golden_tilt_coupling.py [--reference DIR]

Data only: deterministic inputs and what the reference's modules/energy/tilt_coupling.py made of them.  Every fixture is
asserted to have the property it is named for before it is written, and every trajectory is rerun from positions
perturbed by 1e-13 and must keep its accept / reject sequence and its step sizes.  The trajectories use the reference's
mesh-mutating line search (a stepper whose ``step`` takes no ``trial_energy_fn``), as every leaflet trajectory of
oracle/gen_golden.py does: after a rejected trial the tilts projected onto that trial's surface are kept.
"""

from __future__ import annotations

import argparse
import importlib
import inspect
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
from runtime.constraint_manager import ConstraintModuleManager  # noqa: E402
from runtime.energy_manager import EnergyModuleManager  # noqa: E402
from runtime.minimizer import Minimizer  # noqa: E402
from runtime.steppers.conjugate_gradient import ConjugateGradient  # noqa: E402
from runtime.steppers.gradient_descent import GradientDescent  # noqa: E402

from membrane_solver_amd import meshgen  # noqa: E402

REF = importlib.import_module("modules.energy.tilt_coupling")


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


def build(P, T, gp, vopts=None, fixed=None):
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
            k = (min(int(u), int(v)), max(int(u), int(v)))
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


def ring_rows(r):
    """rows of ring r of meshgen.disk_patch (ring r has 6 r vertices, after the center and the rings inside it)"""
    start = 1 + 3 * r * (r - 1)
    return list(range(start, start + 6 * r))


def tangent_tilts(m, rng, scale):
    pos = m.positions_view()
    tl = scale * rng.normal(size=pos.shape)
    nrm = m.vertex_normals(pos)
    return tl - np.einsum("ij,ij->i", tl, nrm)[:, None] * nrm


def facet_terms(pos, tri, tin, tout, k_c, sign):
    """coeff_f A_f of the masked facets and the mask (tilt_coupling.py:153-171 again, for the scales)"""
    d = tout + sign * tin
    q = np.einsum("ij,ij->i", d, d)
    v0, v1, v2 = pos[tri[:, 0]], pos[tri[:, 1]], pos[tri[:, 2]]
    nn = np.linalg.norm(np.cross(v1 - v0, v2 - v0), axis=1)
    mask = nn >= 1e-12
    return 0.5 * k_c * (q[tri[mask]].sum(axis=1) / 3.0) * (0.5 * nn[mask]), mask, nn


# ---------------------------------------------------------------------------------------------------------------------
def gen_cases():
    Pi, Ti = meshgen.icosphere(4)
    Pi = meshgen.smooth_displace(Pi, 0.05) + 0.02 * np.random.default_rng(21).normal(size=Pi.shape)
    P6, T6, _B6 = meshgen.disk_patch(6, bulge=0.3, jitter=0.02, seed=11)
    # two facets collapsed to exactly zero area: a ring-3 vertex put on the very point of its neighbour along the ring
    P6z = P6.copy()
    a, b = ring_rows(3)[4], ring_rows(3)[5]
    P6z[b] = P6z[a]
    meshes = {"disk4": meshgen.disk_patch(4)[:2], "disk6": (P6, T6), "ico4": (Pi, np.asarray(Ti)), "disk6z": (P6z, T6)}
    # name: (mesh, gp, what)
    cases = {
        "disk4_difference": ("disk4", {"tilt_coupling_modulus": 3.5, "tilt_coupling_mode": "difference"}, ""),
        "disk4_sum": ("disk4", {"tilt_coupling_modulus": 2.25, "tilt_coupling_mode": "sum"}, ""),
        "disk6_difference": ("disk6", {"tilt_coupling_modulus": 10.0, "tilt_coupling_mode": "difference"}, ""),
        "disk6_sum_alias_plus": ("disk6", {"tilt_coupling_modulus": 1.75, "tilt_coupling_mode": " Plus "}, ""),
        "disk6_difference_alias_sub": ("disk6", {"tilt_coupling_modulus": 0.8, "tilt_coupling_mode": "SUB"}, ""),
        "disk6_misspelt_key": ("disk6", {"tilt_coupling_modulus": 4.0, "tilt_couping_mode": "diff"}, ""),
        "disk6_moved": ("disk6", {"tilt_coupling_modulus": 2.0, "tilt_coupling_mode": "sum"}, "moved"),
        "disk6_unknown_mode": ("disk6", {"tilt_coupling_modulus": 2.0, "tilt_coupling_mode": "product"}, "off"),
        "disk6_absent_mode": ("disk6", {"tilt_coupling_modulus": 2.0}, "off"),
        "disk6_zero_modulus": ("disk6", {"tilt_coupling_modulus": 0.0, "tilt_coupling_mode": "difference"}, "off"),
        "disk6_cancelling_difference": ("disk6", {"tilt_coupling_modulus": 6.0, "tilt_coupling_mode": "difference"}, "cancel"),
        "disk6_cancelling_sum": ("disk6", {"tilt_coupling_modulus": 6.0, "tilt_coupling_mode": "sum"}, "cancel"),
        "disk6z_zero_area_difference": ("disk6z", {"tilt_coupling_modulus": 3.0, "tilt_coupling_mode": "difference"}, "zero_area"),
        "ico4_difference": ("ico4", {"tilt_coupling_modulus": 5.0, "tilt_coupling_mode": "difference"}, ""),
        "ico4_sum_moved": ("ico4", {"tilt_coupling_modulus": 1.3, "tilt_coupling_mode": "add"}, "moved"),
    }
    out, names = {}, []
    for name, (mname, gp, what) in cases.items():
        P, T = meshes[mname]
        T = np.asarray(T, dtype=np.int32)
        m, _edges = build(P, T, gp)
        res = ParameterResolver(m.global_parameters)
        rng = np.random.default_rng(5)
        if mname == "disk6z":  # (the vertex normals of the collapsed facets' corners are still defined by the others)
            tin, tout = 0.3 * rng.normal(size=P.shape), 0.25 * rng.normal(size=P.shape)
        else:
            tin, tout = tangent_tilts(m, rng, 0.3), tangent_tilts(m, rng, 0.25)
        sign = REF._resolve_coupling_mode(res)
        k_c = REF._resolve_coupling_modulus(res)
        if what == "cancel":  # t_out = -s t_in everywhere: d = 0 exactly
            tout = -sign * tin
        pos = m.positions_view().copy()
        if what == "moved":  # evaluated on positions that are not the mesh's
            pos = pos + 0.03 * np.random.default_rng(9).normal(size=pos.shape)
        g, tgi, tgo = np.zeros_like(pos), np.zeros_like(pos), np.zeros_like(pos)
        kw = dict(positions=pos, index_map=m.vertex_index_to_row, tilts_in=tin, tilts_out=tout)
        if what == "zero_area":
            # With a facet masked out the reference's array API cannot be asked for tilt gradients: it hands
            # Mesh.barycentric_vertex_areas the already masked areas together with the mask (tilt_coupling.py:185-191)
            # and numpy refuses the second masking.  Energy and shape gradient come from the array API, the tilt
            # gradient from the reference's dict API, which sums the masked thirds itself (:97-109); it returns the
            # OUT gradient, and the IN gradient is s times it (:197, :203).
            try:
                REF.compute_energy_and_gradient_array(m, m.global_parameters, res, grad_arr=None,
                                                      tilt_in_grad_arr=tgi.copy(), tilt_out_grad_arr=None, **kw)
                raise AssertionError("the reference's array API took a masked facet: use it for the tilt gradients")
            except IndexError:
                pass
            E = REF.compute_energy_and_gradient_array(m, m.global_parameters, res, grad_arr=g, **kw)
            m.set_tilts_in_from_array(tin)
            m.set_tilts_out_from_array(tout)
            _Ed, _gd, tgd0 = REF.compute_energy_and_gradient(m, m.global_parameters, res)
            tgo = np.array([tgd0[i] for i in range(len(P))])
            tgi = sign * tgo
        else:
            E = REF.compute_energy_and_gradient_array(m, m.global_parameters, res, grad_arr=g, tilt_in_grad_arr=tgi,
                                                      tilt_out_grad_arr=tgo, **kw)
        E2 = REF.compute_energy_array(m, m.global_parameters, res, **kw)
        assert E2 == E, name
        E_scale, g_scale, tg_scale = 0.0, 0.0, 0.0
        if what == "off":
            assert sign is None or k_c == 0.0
            assert E == 0.0 and not g.any() and not tgi.any() and not tgo.any(), name
        else:
            assert sign in (-1, 1) and k_c != 0.0, name
            terms, mask, nn = facet_terms(pos, T, tin, tout, k_c, sign)
            E_scale = float(np.abs(terms).sum())
            assert abs(E - E_scale) <= 1e-13 * max(E_scale, 1e-300), name  # (the sum does not cancel)
            if what == "cancel":
                assert E == 0.0 and not g.any() and not tgi.any() and not tgo.any(), name
                # the scales of the uncancelled field: the same positions, t_out = 0
                z = np.zeros_like(tin)
                g2, ti2, to2 = np.zeros_like(pos), np.zeros_like(pos), np.zeros_like(pos)
                E_scale = float(REF.compute_energy_and_gradient_array(
                    m, m.global_parameters, res, grad_arr=g2, tilt_in_grad_arr=ti2, tilt_out_grad_arr=to2,
                    positions=pos, index_map=m.vertex_index_to_row, tilts_in=tin, tilts_out=z))
                g_scale, tg_scale = float(np.max(np.abs(g2))), float(np.max(np.abs(to2)))
                assert E_scale > 0.0 and g_scale > 0.0 and tg_scale > 0.0
            else:
                assert E > 0.0 and g.any() and tgi.any() and tgo.any(), name
                g_scale, tg_scale = float(np.max(np.abs(g))), float(np.max(np.abs(tgo)))
            if what == "zero_area":
                assert (~mask).sum() == 2 and np.all(nn[~mask] == 0.0), name  # exactly 0: both area rules agree
        assert np.array_equal(tgi, (sign or 0) * tgo), name
        if what != "moved":  # the dict API evaluates the mesh's own positions and tilts
            m.set_tilts_in_from_array(tin)
            m.set_tilts_out_from_array(tout)
            Ed, gd, tgd = REF.compute_energy_and_gradient(m, m.global_parameters, res)
            assert abs(Ed - E) <= 1e-13 * max(E_scale, 1e-300), name
            assert sorted(gd) == sorted(tgd) == list(range(len(P))), name
            tgd_arr = np.array([tgd[i] for i in range(len(P))])
            assert np.max(np.abs(tgd_arr - tgo)) <= 1e-13 * max(tg_scale, 1e-300), name  # the OUT gradient
        # (positions and triangles once per mesh; the evaluation positions where they differ from the mesh's; the IN
        # gradient is s times the OUT gradient to the bit -- asserted above -- and is not stored)
        out["mesh__" + mname + "__positions"] = m.positions_view().copy()
        out["mesh__" + mname + "__tri"] = T
        if what == "moved":
            out[name + "__eval_positions"] = pos
        out.update({name + "__mesh": np.array(mname), name + "__gp": jdump(gp), name + "__what": np.array(what),
                    name + "__tilts_in": tin, name + "__tilts_out": tout, name + "__E": np.array(float(E)),
                    name + "__grad": g, name + "__tilt_grad_out": tgo, name + "__E_scale": np.array(E_scale),
                    name + "__grad_scale": np.array(g_scale), name + "__tilt_grad_scale": np.array(tg_scale),
                    name + "__sign": np.array(0 if sign is None else int(sign)), name + "__k_c": np.array(float(k_c))})
        names.append(name)
        print("%-32s nv %3d E=% .16g scale=%.6g" % (name, len(P), E, E_scale))
    out["names"] = np.array(names)
    # the module's public surface, as names: the plugin must offer the same entry points with the same parameters
    out["signatures"] = jdump({fn: [[p.name, str(p.kind), p.default is not inspect.Parameter.empty]
                                    for p in inspect.signature(getattr(REF, fn)).parameters.values()]
                               for fn in REF.__all__})
    out["uses_tilt_leaflets"] = np.array(bool(REF.USES_TILT_LEAFLETS))
    save_npz(os.path.join(OUT, "tilt_coupling_cases.npz"), out)


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


def run_once(P, T, gp, vo, mods, stepper_cls, n_steps, step_size, fixed, fixed_every):
    m, edges = build(P, T, gp, vopts=vo, fixed=fixed)
    tin, tout, fin, fout = set_fields(m, 33, 0.3, *fixed_every)
    m.energy_modules = list(mods)
    m.constraint_modules = []
    stepper = stepper_cls()
    mz = Minimizer(m, m.global_parameters, stepper, EnergyModuleManager(m.energy_modules),
                   ConstraintModuleManager(m.constraint_modules), quiet=True, step_size=step_size)
    log = []
    orig = stepper.step

    def logged(mesh, grad, step_size, energy_fn, constraint_enforcer=None):
        r = orig(mesh, grad, step_size, energy_fn, constraint_enforcer=constraint_enforcer)
        log.append((float(bool(r[0])), float(r[1]), float(r[2])))
        return r

    stepper.step = logged
    pos0 = m.positions_view().copy()
    E0, g0 = mz.compute_energy_and_gradient_array()
    res = mz.minimize(n_steps)
    bd = mz.compute_energy_breakdown()
    return {"positions0": pos0, "tri": np.asarray(m.triangle_row_cache()[0], dtype=np.int32),
            "fixed": m.fixed_mask.copy() if fixed is not None else np.zeros(len(P), bool),
            "edges": edges, "vopts": jdump({str(k): v for k, v in vo.items()}), "tilt_fixed_in": fin, "tilt_fixed_out": fout,
            "gamma": m.get_facet_parameter_array("surface_tension").copy(), "E0": np.array(E0), "grad0": np.array(g0),
            "tilts_in0": tin, "tilts_out0": tout, "positions_final": m.positions_view().copy(),
            "tilts_in_final": np.ascontiguousarray(m.tilts_in_view()).copy(),
            "tilts_out_final": np.ascontiguousarray(m.tilts_out_view()).copy(), "step_log": np.array(log),
            "E_final": np.array(res["energy"]), "E_coupling_final": np.array(float(bd["tilt_coupling"])),
            "n_steps": np.array(n_steps), "step_size0": np.array(step_size),
            "gp_json": jdump(gp), "modules": np.array(list(mods)), "stepper": np.array(stepper_cls.__name__)}


def run_traj(fname, P, T, gp, vo, mods, stepper_cls, n_steps, step_size, fixed, check, fixed_every=(0, 0)):
    out = run_once(P, T, gp, vo, mods, stepper_cls, n_steps, step_size, fixed, fixed_every)
    L = out["step_log"]
    check(L, out)
    assert float(out["E_coupling_final"]) > 0.0, fname
    # stability: the same run from positions perturbed by 1e-13 keeps every decision and every step size
    Pp = np.asarray(P, dtype=float) + 1e-13 * np.random.default_rng(77).normal(size=np.shape(P))
    again = run_once(Pp, T, gp, vo, mods, stepper_cls, n_steps, step_size, fixed, fixed_every)["step_log"]
    assert again.shape == L.shape and np.array_equal(again[:, 0], L[:, 0]) and np.allclose(again[:, 1], L[:, 1], rtol=1e-9), fname
    save_npz(os.path.join(OUT, fname), out)
    print(fname, "E_final=%.16g" % out["E_final"], L[:, :2].tolist())
    return out


def gen_trajectories():
    quiet = {"mesh_quality_auto_repair_enabled": False, "volume_constraint_mode": "lagrange",
             "volume_projection_during_minimization": False}
    P6, T6, B6 = meshgen.disk_patch(6, bulge=0.3, jitter=0.02, seed=11)
    r3 = ring_rows(3)
    vo = {int(r): {"pin_to_circle_group": "rim", "pin_to_circle_normal": [0.0, 0.0, 1.0]} for r in r3}
    base = dict(quiet, surface_tension=1.0, tilt_modulus_in=2.0, tilt_modulus_out=1.4, bending_modulus_in=0.6,
                bending_modulus_out=0.45, tilt_rim_source_group_in="rim", tilt_rim_source_strength_in=0.8,
                tilt_rim_source_edge_mode="all", tilt_rim_source_center=[0.02, -0.01, 0.0],
                tilt_coupling_modulus=3.0, tilt_coupling_mode="difference")
    mods = ["tilt_in", "tilt_out", "tilt_smoothness_in", "tilt_smoothness_out", "tilt_rim_source_in", "tilt_coupling"]

    def some_accepted(L, _out):
        assert (L[:, 0] > 0).sum() >= 3, L

    def some_trial_rejected(step0):
        def check(L, _out):
            # an accepted step whose alpha lies below the step size it was given: a trial before it was rejected
            assert (L[:, 0] > 0).sum() >= 3, L
            given = np.concatenate([[step0], L[:-1, 1]])
            assert np.any((L[:, 0] > 0) & (L[:, 1] < 1.5 * given * 0.999)), L
        return check

    # 1: GD + nested CG relaxation, boundary vertices fixed, some inner tilts clamped
    run_traj("traj_disk6_gd_coupling_nested_cg.npz", P6, T6,
             dict(base, tilt_solve_mode="nested", tilt_solver="cg", tilt_step_size=0.05, tilt_inner_steps=5),
             vo, mods, GradientDescent, 5, 0.05, B6, some_accepted, fixed_every=(7, 0))
    # 2: CG + coupled GD relaxation, the "sum" mode's sign on the same deck would be another deck: "difference" again,
    # clamped outer tilts this time
    run_traj("traj_disk6_cg_coupling_coupled_gd.npz", P6, T6,
             dict(base, tilt_solve_mode="coupled", tilt_solver="gd", tilt_step_size=0.03, tilt_coupled_steps=3),
             vo, mods, ConjugateGradient, 5, 2e-3, B6, some_accepted, fixed_every=(0, 5))
    # 3: closed noisy icosphere, surface + both magnitudes + coupling ("sum"), a first step size that has to backtrack:
    # the rejected trial's projection of both leaflets is kept
    Pi, Ti = meshgen.icosphere(4)
    Pi = meshgen.smooth_displace(Pi, 0.05) + 0.02 * np.random.default_rng(21).normal(size=Pi.shape)
    gp3 = dict(quiet, surface_tension=1.0, tilt_modulus_in=1.1, tilt_modulus_out=0.7, tilt_coupling_modulus=4.0,
               tilt_coupling_mode="sum")
    run_traj("traj_ico4_gd_coupling_surface_backtrack.npz", Pi, np.asarray(Ti), gp3, {},
             ["surface", "tilt_in", "tilt_out", "tilt_coupling"], GradientDescent, 5, 0.5, None, some_trial_rejected(0.5))


# ---------------------------------------------------------------------------------------------------------------------
def gen_milestone_b():
    """The shape of the reference's milestone-B tracking test (tests/test_caveolin_annulus_milestone_b.py,
    test_kozlov_annulus_coupling_tracking): a flat annulus, tilt_in clamped to the radial unit vector on the inner rim
    and to zero on the outer rim, k_c = 10 in "difference" mode, one nested relaxation of 1000 inner steps."""
    n, radii = 12, (1.0, 1.5, 2.0, 2.5, 3.0)
    P, rings = [], []
    for r in radii:
        rows = []
        for k in range(n):
            ang = 2.0 * np.pi * k / n
            rows.append(len(P))
            P.append([r * np.cos(ang), r * np.sin(ang), 0.0])
        rings.append(rows)
    T = []
    for a, b in zip(rings[:-1], rings[1:]):
        for k in range(n):
            k1 = (k + 1) % n
            T.append((a[k], a[k1], b[k]))
            T.append((b[k], a[k1], b[k1]))
    P, T = np.array(P), np.array(T, dtype=np.int32)
    # (that deck's module list: the outer leaflet has no module but the coupling, nothing else holds t_out)
    gp = {"surface_tension": 0.0, "tilt_modulus_in": 1.0, "bending_modulus_in": 1.0, "tilt_coupling_modulus": 10.0,
          "tilt_coupling_mode": "difference", "tilt_solve_mode": "nested", "tilt_step_size": 0.05,
          "tilt_inner_steps": 1000, "tilt_tol": 1e-6, "mesh_quality_auto_repair_enabled": False}
    mods = ["tilt_smoothness_in", "tilt_in", "tilt_coupling"]
    fin = np.zeros(len(P), bool)
    fin[rings[0] + rings[-1]] = True
    tin0 = np.zeros_like(P)
    for k, row in enumerate(rings[0]):
        ang = 2.0 * np.pi * k / n
        tin0[row] = [np.cos(ang), np.sin(ang), 0.0]

    def run(noise):
        """one relaxation from the initial fields (+ in-plane noise on the free rows) ->
        (mesh, minimizer, edges, (gradient evaluations, energy evaluations, iterations))"""
        m, edges = build(P, T, gp, fixed=np.ones(len(P), bool))
        for row in np.flatnonzero(fin):
            m.vertices[int(row)].tilt_fixed_in = True
        rng = np.random.default_rng(77)
        pert = noise * rng.normal(size=(2,) + P.shape)
        pert[:, :, 2] = 0.0
        pert[0][fin] = 0.0
        m.set_tilts_in_from_array(tin0 + pert[0])
        m.set_tilts_out_from_array(pert[1])
        m.energy_modules = list(mods)
        m.constraint_modules = []
        mz = Minimizer(m, m.global_parameters, GradientDescent(), EnergyModuleManager(m.energy_modules),
                       ConstraintModuleManager(m.constraint_modules), quiet=True)
        mgr = mz._tilt_relaxation_manager
        count = [0, 0]  # gradient evaluations, energy-only evaluations (the line searches' trials)

        def counted(fn, k):
            def wrapper(*a, **kw):
                count[k] += 1
                return fn(*a, **kw)
            return wrapper

        mgr.compute_energy_and_leaflet_tilt_gradients_array_fn = counted(mgr.compute_energy_and_leaflet_tilt_gradients_array_fn, 0)
        mgr.compute_tilt_dependent_energy_with_leaflet_tilts_fn = counted(mgr.compute_tilt_dependent_energy_with_leaflet_tilts_fn, 1)
        assert mz._uses_leaflet_tilts()
        pos0 = m.positions_view().copy()
        mz._relax_leaflet_tilts(positions=m.positions_view(), mode="nested")
        assert np.array_equal(m.positions_view(), pos0)
        # CG: one gradient evaluation before the loop, one at the end of every iteration that accepted a step; the run
        # ends with the gradient evaluation that meets tilt_tol, so the line searches -- the iterations -- are one fewer
        stop = str(mgr.last_leaflet_relaxation_stats.get("stop_reason"))
        assert stop == "converged", stop
        n_iter = count[0] - 1
        assert 0 < n_iter < int(gp["tilt_inner_steps"]) and count[1] >= n_iter
        return m, mz, edges, (count[0], count[1], n_iter)

    m, mz, edges, counts = run(0.0)
    n_evals = counts[0] + counts[1]
    # stability: the same relaxation from fields perturbed by 1e-13 stops after the same iterations and evaluations
    # (tilt_tol 1e-6: with 1e-8 and below the count changes with such a perturbation -- CG at its rounding floor -- and
    # no two implementations could agree on it) and ends within the relaxation tests' tolerance of the same fields
    for noise in (1e-13, -1e-13):
        m2, _mz2, _e2, n2 = run(noise)
        assert n2 == counts, "the relaxation's stopping point depends on rounding"
        for a, b in ((m2.tilts_in_view(), m.tilts_in_view()), (m2.tilts_out_view(), m.tilts_out_view())):
            dev = float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(np.asarray(b))))
            print("   perturbed by %g: final fields differ by %.3g" % (noise, dev))
            assert dev < 1e-9
    count = [n_evals]
    pos0 = m.positions_view().copy()
    tin, tout = np.array(m.tilts_in_view(), copy=True), np.array(m.tilts_out_view(), copy=True)
    diff = np.linalg.norm(tin - tout, axis=1)
    # t_out tracks t_in (the reference test's own assertions)
    assert np.mean(diff) < 0.1 and np.max(np.linalg.norm(tout, axis=1)) > 0.9, (np.mean(diff), np.max(np.linalg.norm(tout, axis=1)))
    res = ParameterResolver(m.global_parameters)
    E_c = REF.compute_energy_array(m, m.global_parameters, res, positions=m.positions_view(),
                                   index_map=m.vertex_index_to_row, tilts_in=tin, tilts_out=tout)
    E_total = float(mz.compute_energy())
    print("milestone B: mean|t_in - t_out|=%.4g max|t_out|=%.4g E_coupling=%.16g E_total=%.16g evaluations=%d"
          % (np.mean(diff), np.max(np.linalg.norm(tout, axis=1)), E_c, E_total, count[0]))
    save_npz(os.path.join(OUT, "tilt_coupling_milestone_b.npz"),
             {"positions": pos0, "tri": T, "edges": edges, "fixed": np.ones(len(P), bool), "tilt_fixed_in": fin,
              "tilt_fixed_out": np.zeros(len(P), bool), "gp_json": jdump(gp), "modules": np.array(mods),
              "tilts_in0": tin0, "tilts_out0": np.zeros_like(P), "tilts_in_final": tin, "tilts_out_final": tout,
              "E_coupling": np.array(float(E_c)), "E_total": np.array(E_total), "n_evaluations": np.array(count[0]),
              "n_gradient_evaluations": np.array(counts[0]), "n_energy_evaluations": np.array(counts[1]),
              "n_iterations": np.array(counts[2])})


if __name__ == "__main__":
    gen_cases()
    gen_milestone_b()
    gen_trajectories()
