#!/usr/bin/env python3
"""Generate tests/golden/leaflet_absent_cases.npz, leaflet_absent_relax.npz and traj_disk6_gd_leaflet_absent_pins.npz by
running the REFERENCE's leaflet_presence helpers, its tilt_out / tilt_smoothness_out modules, its leaflet relaxation and
its Minimizer with ``leaflet_out_absent_presets`` set.

    PYTHONDONTWRITEBYTECODE=1 python3 tools/gen_golden_leaflet_absent.py [--reference DIR]

Data only: deterministic inputs and what the reference made of them.  Every fixture is asserted to have the property it
is named for before it is written; the relaxations and the trajectory are rerun from inputs perturbed by 1e-13 and must
keep their evaluation counts, their accept / reject sequence and their step sizes.  The library is used for one thing:
its tiling planner (ms_plan_tiling, host code) says which tile owns a row, for the fixture whose mask edge has to cross a
tile boundary.
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
from modules.energy.leaflet_presence import leaflet_absent_vertex_mask, leaflet_present_triangle_mask  # noqa: E402
from runtime.constraint_manager import ConstraintModuleManager  # noqa: E402
from runtime.energy_manager import EnergyModuleManager  # noqa: E402
from runtime.leaflet_validation import validate_leaflet_absence_topology  # noqa: E402
from runtime.minimizer import Minimizer  # noqa: E402
from runtime.preconditioners import build_leaflet_tilt_cg_preconditioner  # noqa: E402
from runtime.steppers.gradient_descent import GradientDescent  # noqa: E402
from runtime.steppers.tilt_relaxation import _tilt_vertex_areas_from_triangles  # noqa: E402

from membrane_solver_amd import _lib as L  # noqa: E402
from membrane_solver_amd import meshgen  # noqa: E402

TILT_OUT = importlib.import_module("modules.energy.tilt_out")
TS_OUT = importlib.import_module("modules.energy.tilt_smoothness_out")
TILT_IN = importlib.import_module("modules.energy.tilt_in")
TS_IN = importlib.import_module("modules.energy.tilt_smoothness_in")


def save_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps: the same arrays give the same bytes on every run."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for key, val in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(val), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())
    assert os.path.getsize(path) < (1 << 20), (path, os.path.getsize(path))


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
    """rows of ring r of meshgen.disk_patch (ring 0 is the center; ring r has 6 r vertices)"""
    if r == 0:
        return [0]
    start = 1 + 3 * r * (r - 1)
    return list(range(start, start + 6 * r))


def rings_upto(r):
    return [row for k in range(r + 1) for row in ring_rows(k)]


def preset_options(rows, extra=None):
    vo = {int(r): {"preset": "disk"} for r in rows}
    for r, o in (extra or {}).items():
        vo[int(r)] = dict(vo.get(int(r), {}), **o)
    return vo


def tangent_tilts(m, rng, scale):
    pos = m.positions_view()
    tl = scale * rng.normal(size=pos.shape)
    nrm = m.vertex_normals(pos)
    return tl - np.einsum("ij,ij->i", tl, nrm)[:, None] * nrm


def tile_of_rows(P, T, tile_vertices=0):
    """library tile that owns each external row (ms_plan_tiling: the context's own planner, on the host)"""
    pos = np.ascontiguousarray(P, dtype=np.float64)
    tri = np.ascontiguousarray(T, dtype=np.int32)
    stats = np.zeros(8, dtype=np.int64)
    perm = np.zeros(len(pos), dtype=np.int32)
    L.check(L.lib().ms_plan_tiling(len(pos), len(tri), pos.ctypes.data_as(L._D), tri.ctypes.data_as(L._I32),
                                   int(tile_vertices), 1, stats.ctypes.data_as(L._I64), perm.ctypes.data_as(L._I32)),
            None, "ms_plan_tiling")
    own = int(tile_vertices) if tile_vertices else 256
    tile = np.empty(len(pos), dtype=np.int64)
    tile[perm] = np.arange(len(pos)) // own  # perm[i] = external row of library row i
    return tile, int(stats[0])


BASE_GP = {"tilt_modulus_in": 2.0, "tilt_modulus_out": 1.4, "bending_modulus_in": 0.6, "bending_modulus_out": 0.45,
           "leaflet_out_absent_presets": ["disk"], "leaflet_out_absence_mode": "triangles",
           "mesh_quality_auto_repair_enabled": False}


def module_eval(mod, m, res, pos, tin, tout, leaflet):
    g, tg = np.zeros_like(pos), np.zeros_like(pos)
    kw = {"tilt_in_grad_arr": tg} if leaflet == "in" else {"tilt_out_grad_arr": tg}
    E = mod.compute_energy_and_gradient_array(m, m.global_parameters, res, positions=pos, index_map=m.vertex_index_to_row,
                                              grad_arr=g, tilts_in=tin, tilts_out=tout, **kw)
    return float(E), g, tg


# ---------------------------------------------------------------------------------------------------------------------
def gen_cases():
    P4, T4, _B4 = meshgen.disk_patch(4)
    P12, T12, _B12 = meshgen.disk_patch(12)
    P6, T6, _B6 = meshgen.disk_patch(6, bulge=0.3, jitter=0.02, seed=11)
    # two facets collapsed to exactly zero area: a ring-3 vertex put on the very point of its neighbour along the ring
    # (the disk6z construction of gen_golden_tilt_coupling.py)
    P6z = P6.copy()
    za, zb = ring_rows(3)[4], ring_rows(3)[5]
    P6z[zb] = P6z[za]
    meshes = {"disk4": (P4, np.asarray(T4, np.int32)), "disk12": (P12, np.asarray(T12, np.int32)),
              "disk6z": (P6z, np.asarray(T6, np.int32))}
    assert len(P4) == 61 and len(P12) == 469

    # the ring whose mask edge crosses the boundary between the two tiles of disk12 (default tile size)
    tile12, n_tiles12 = tile_of_rows(P12, T12)
    assert n_tiles12 >= 2, n_tiles12
    cross_ring = None
    for r in range(2, 11):
        ab = np.zeros(len(P12), bool)
        ab[rings_upto(r)] = True
        masked = np.any(ab[T12], axis=1)
        straddle = masked & np.any(~ab[T12], axis=1)  # the mask's edge: masked facets with a present corner
        two_tiles = np.array([len(set(tile12[f])) > 1 for f in T12])
        if np.any(straddle & two_tiles):
            cross_ring = r
            break
    assert cross_ring is not None, "no ring of disk12 puts the mask edge across a tile boundary"

    # a present row with exactly one kept facet: a boundary row of disk4 whose other neighbours are all absent
    T4a = np.asarray(T4)
    v1 = ring_rows(4)[1]
    star = [f for f in T4a if v1 in f]
    f0 = star[0]
    one_rows = sorted({int(r) for f in star for r in f} - {int(r) for r in f0})
    one_rows = sorted(set(one_rows) | {0})

    # name: (mesh, absent rows, mass mode, tilt_fixed_out rows, what)
    cases = {
        "disk4_ring1_lumped": ("disk4", rings_upto(1), "lumped", [], ""),
        "disk4_ring1_consistent": ("disk4", rings_upto(1), "consistent", [], ""),
        "disk4_ring2_lumped": ("disk4", rings_upto(2), "lumped", [], ""),
        "disk4_ring2_consistent": ("disk4", rings_upto(2), "consistent", [], ""),
        "disk12_cross_lumped": ("disk12", rings_upto(cross_ring), "lumped", [], "cross"),
        "disk12_cross_consistent": ("disk12", rings_upto(cross_ring), "consistent", [], "cross"),
        "disk4_all_absent": ("disk4", list(range(len(P4))), "lumped", [], "all"),
        "disk6z_zero_area_kept": ("disk6z", rings_upto(2), "lumped", [], "zero_area"),
        "disk4_absent_and_fixed": ("disk4", rings_upto(1), "lumped", [0, ring_rows(1)[2], ring_rows(3)[5]], "fixed"),
        "disk4_one_kept_facet": ("disk4", one_rows, "consistent", [], "one_facet"),
        "disk4_no_mask": ("disk4", [], "lumped", [], "none"),
    }
    out, names = {}, []
    for name, (mname, rows, mass, fixed_out, what) in cases.items():
        P, T = meshes[mname]
        gp = dict(BASE_GP, tilt_mass_mode_out=mass, tilt_mass_mode_in="lumped")
        if what == "none":
            gp["leaflet_out_absent_presets"] = []
        vo = preset_options(rows)
        m, edges = build(P, T, gp, vopts=vo)
        for r in fixed_out:
            m.vertices[int(r)].tilt_fixed_out = True
        res = ParameterResolver(m.global_parameters)
        rng = np.random.default_rng(5)
        if mname == "disk6z":  # (the vertex normals of the collapsed facets' corners are still defined by the others)
            tin, tout = 0.3 * rng.normal(size=P.shape), 0.25 * rng.normal(size=P.shape)
        else:
            tin, tout = tangent_tilts(m, rng, 0.3), tangent_tilts(m, rng, 0.25)
        pos = m.positions_view().copy()
        tri = np.asarray(m.triangle_row_cache()[0], dtype=np.int32)
        assert np.array_equal(tri, T), name
        absent = np.array(leaflet_absent_vertex_mask(m, m.global_parameters, leaflet="out"), copy=True)
        want = np.zeros(len(P), bool)
        want[rows] = True
        assert np.array_equal(absent, want), name
        kept = leaflet_present_triangle_mask(m, tri, absent_vertex_mask=absent)
        assert not leaflet_absent_vertex_mask(m, m.global_parameters, leaflet="in").any()
        # the validation: triangles mode passes, strict raises exactly when a facet straddles
        validate_leaflet_absence_topology(m, m.global_parameters)
        straddles = bool(np.any(np.any(absent[tri], axis=1) & np.any(~absent[tri], axis=1)))
        m.global_parameters.set("leaflet_out_absence_mode", "strict")
        try:
            validate_leaflet_absence_topology(m, m.global_parameters)
            raised = False
        except ValueError:
            raised = True
        m.global_parameters.set("leaflet_out_absence_mode", "triangles")
        assert raised == straddles, name
        E_t, g_t, tg_t = module_eval(TILT_OUT, m, res, pos, tin, tout, "out")
        E_s, g_s, tg_s = module_eval(TS_OUT, m, res, pos, tin, tout, "out")
        E_ti, g_ti, tg_ti = module_eval(TILT_IN, m, res, pos, tin, tout, "in")
        E_si, _g_si, tg_si = module_eval(TS_IN, m, res, pos, tin, tout, "in")
        assert not g_s.any(), name  # (the smoothness modules have no shape gradient)
        # the relaxation's geometry (tilt_relaxation.py:675-697, preconditioners.py:62-146)
        va_in = _tilt_vertex_areas_from_triangles(n_vertices=len(P), tri_rows=tri, positions=pos)
        tri_out = tri[kept] if kept.size else tri
        va_out = (va_in if not absent.any() else np.zeros(len(P)) if tri_out.size == 0 else
                  _tilt_vertex_areas_from_triangles(n_vertices=len(P), tri_rows=tri_out, positions=pos))
        fin = np.zeros(len(P), bool)
        fout = np.zeros(len(P), bool)
        fout[fixed_out] = True
        minv_in, minv_out = build_leaflet_tilt_cg_preconditioner(
            m, res, None, positions=pos, index_map=m.vertex_index_to_row, fixed_mask_in=fin, fixed_mask_out=fout,
            tilt_vertex_areas_in=va_in, tilt_vertex_areas_out=va_out)
        # ---- the property each fixture is named for
        nn = np.linalg.norm(np.cross(pos[tri[:, 1]] - pos[tri[:, 0]], pos[tri[:, 2]] - pos[tri[:, 0]]), axis=1)
        if what == "all":
            assert absent.all() and not kept.any()
            assert E_t == 0.0 and E_s == 0.0 and not g_t.any() and not tg_t.any() and not tg_s.any(), name
            assert not va_out.any(), name
        elif what == "none":
            assert not absent.any() and kept.all() and np.array_equal(va_out, va_in), name
        else:
            assert absent.any() and kept.any() and not kept.all(), name
            assert E_t > 0.0 and E_s > 0.0 and g_t.any() and tg_t.any() and tg_s.any(), name
            assert not tg_t[absent].any() and not tg_s[absent].any() and not va_out[absent].any(), name
            # an absent row's diagonal is its smoothness part alone (unmasked: preconditioners.py:121-140)
            _mi, minv_full = build_leaflet_tilt_cg_preconditioner(
                m, res, None, positions=pos, index_map=m.vertex_index_to_row, fixed_mask_in=fin, fixed_mask_out=fout,
                tilt_vertex_areas_in=va_in, tilt_vertex_areas_out=va_in)
            free = absent & ~fout
            assert np.all(minv_out[free] > minv_full[free]), name
            # the mask changes the result: the same evaluation without it differs
            m.global_parameters.set("leaflet_out_absent_presets", [])
            E_full, _gf, _tf = module_eval(TILT_OUT, m, res, pos, tin, tout, "out")
            Es_full, _gs, _ts = module_eval(TS_OUT, m, res, pos, tin, tout, "out")
            m.global_parameters.set("leaflet_out_absent_presets", ["disk"])
            assert E_full > E_t * (1 + 1e-6) and abs(Es_full - E_s) > 1e-6 * abs(E_s), name
        if what == "cross":
            tile, n_tiles = tile_of_rows(P, T)
            masked_two = [f for f, k in zip(tri, kept) if not k and len(set(tile[f])) > 1]
            assert n_tiles >= 2 and len(masked_two) >= 1, name
            # ... with the absent corner in one tile and the facet reaching into the other (a halo row's flag decides)
            assert any(len({int(tile[r]) for r in f if absent[r]} ^ {int(tile[r]) for r in f}) > 0 for f in masked_two), name
            out[name + "__tile_of_row"] = tile
        if what == "zero_area":
            zero = nn == 0.0
            assert zero.sum() == 2, name
            masked_rows = set(np.flatnonzero(absent).tolist())
            kept_zero = [f for f, k, z in zip(tri, kept, zero) if k and z]
            assert len(kept_zero) >= 1, name
            # adjacent to the mask: the kept zero-area facet shares an edge with a masked facet
            adj = False
            for f in kept_zero:
                for g2, k in zip(tri, kept):
                    if not k and len(set(f.tolist()) & set(g2.tolist())) >= 2:
                        adj = True
            assert adj and masked_rows, name
        if what == "fixed":
            assert absent[fixed_out[0]] and absent[fixed_out[1]] and not absent[fixed_out[2]], name
            assert np.all(minv_out[fixed_out] == 1.0), name
        if what == "one_facet":
            present_one = [r for r in np.flatnonzero(~absent) if sum(1 for f, k in zip(tri, kept) if k and r in f) == 1]
            assert v1 in present_one, name
            assert va_out[v1] > 0.0 and np.any(tg_t[v1] != 0.0), name
        out["mesh__" + mname + "__positions"] = pos
        out["mesh__" + mname + "__tri"] = tri
        out["mesh__" + mname + "__edges"] = edges
        out.update({name + "__mesh": np.array(mname), name + "__gp": jdump(gp), name + "__what": np.array(what),
                    name + "__vopts": jdump({str(k): v for k, v in vo.items()}), name + "__tilt_fixed_out": fout,
                    name + "__tilts_in": tin, name + "__tilts_out": tout, name + "__absent": absent, name + "__kept": kept,
                    name + "__straddles": np.array(straddles),
                    name + "__E_tilt_out": np.array(E_t), name + "__grad_tilt_out": g_t, name + "__tilt_grad_tilt_out": tg_t,
                    name + "__E_smooth_out": np.array(E_s), name + "__tilt_grad_smooth_out": tg_s,
                    name + "__E_tilt_in": np.array(E_ti), name + "__grad_tilt_in": g_ti, name + "__tilt_grad_tilt_in": tg_ti,
                    name + "__E_smooth_in": np.array(E_si), name + "__tilt_grad_smooth_in": tg_si,
                    name + "__va_in": va_in, name + "__va_out": va_out, name + "__minv_in": minv_in,
                    name + "__minv_out": minv_out})
        names.append(name)
        print("%-28s nv %3d absent %3d kept %4d/%4d E_tilt_out=%.16g E_smooth_out=%.16g" %
              (name, len(P), int(absent.sum()), int(kept.sum()), len(kept), E_t, E_s))
    out["names"] = np.array(names)
    out["cross_ring"] = np.array(cross_ring)
    save_npz(os.path.join(OUT, "leaflet_absent_cases.npz"), out)


# ---------------------------------------------------------------------------------------------------------------------
RELAX_MODS = ["tilt_in", "tilt_out", "tilt_smoothness_in", "tilt_smoothness_out"]


def relax_once(P, T, gp, vo, fixed_out, noise, mods=RELAX_MODS):
    m, edges = build(P, T, gp, vopts=vo, fixed=np.ones(len(P), bool))
    for r in fixed_out:
        m.vertices[int(r)].tilt_fixed_out = True
    rng = np.random.default_rng(33)
    tin0, tout0 = tangent_tilts(m, rng, 0.3), tangent_tilts(m, rng, 0.24)
    pert = noise * np.random.default_rng(77).normal(size=(2,) + P.shape)
    m.set_tilts_in_from_array(tin0 + pert[0])
    m.set_tilts_out_from_array(tout0 + pert[1])
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
    stats = dict(mgr.last_leaflet_relaxation_stats)
    return {"mesh": m, "mz": mz, "edges": edges, "counts": (count[0], count[1]), "tin0": tin0, "tout0": tout0,
            "tin": np.array(m.tilts_in_view(), copy=True), "tout": np.array(m.tilts_out_view(), copy=True),
            "active_outer_area_rows": int(stats.get("active_outer_area_rows", -1))}


def gen_relax():
    """One nested CG relaxation of 40 iterations (Jacobi diagonal, tilt_tol 0) of both leaflets with the outer one absent
    on the inner rings: on the one-tile disk4 and on disk12 with the mask edge across the tile boundary; an absent row
    and a present row carry tilt_fixed_out.  The same two once more with tilt_coupling in the list (disk4c, disk12c): the
    coupling is NOT masked (tilt_coupling.py:160-203 takes every facet, the full vertex areas), so it moves t_out on the
    absent rows."""
    cases = np.load(os.path.join(OUT, "leaflet_absent_cases.npz"), allow_pickle=False)
    cross_ring = int(cases["cross_ring"])
    out = {}
    for name, n_rings, mask_ring, coupled in (("disk4", 4, 2, False), ("disk12", 12, cross_ring, False),
                                              ("disk4c", 4, 2, True), ("disk12c", 12, cross_ring, True)):
        P, T, _B = meshgen.disk_patch(n_rings)
        T = np.asarray(T, np.int32)
        gp = dict(BASE_GP, tilt_solve_mode="nested", tilt_solver="cg", tilt_step_size=0.05, tilt_inner_steps=40,
                  tilt_tol=0.0, tilt_cg_preconditioner="jacobi")
        mods = list(RELAX_MODS)
        if coupled:
            gp.update(tilt_coupling_modulus=3.0, tilt_coupling_mode="difference")
            mods.append("tilt_coupling")
        rows = rings_upto(mask_ring)
        vo = preset_options(rows)
        fixed_out = [ring_rows(1)[2], ring_rows(mask_ring + 1)[3]]
        r = relax_once(P, T, gp, vo, fixed_out, 0.0, mods)
        m = r["mesh"]
        absent = leaflet_absent_vertex_mask(m, m.global_parameters, leaflet="out")
        assert absent[fixed_out[0]] and not absent[fixed_out[1]]
        n_grad, n_en = r["counts"]
        assert n_grad - 1 == 40, (name, r["counts"])  # every iteration accepted a step and none met the tolerance
        # an absent row's t_out never moves (no area, no kept smoothness facet: its gradient is zero), but it is
        # projected onto the tangent plane like every other row
        nrm = m.vertex_normals(m.positions_view())
        proj0 = r["tout0"] - np.einsum("ij,ij->i", r["tout0"], nrm)[:, None] * nrm
        free_absent = absent.copy()
        free_absent[fixed_out] = False
        if coupled:  # ... unless the coupling, which keeps every facet, pulls it towards t_in
            assert np.min(np.linalg.norm(r["tout"][free_absent] - proj0[free_absent], axis=1)) > 1e-3, name
        else:
            assert np.max(np.abs(r["tout"][absent] - proj0[absent])) <= 1e-15, name
        assert np.max(np.abs(r["tout"][~absent] - proj0[~absent])) > 1e-3, name
        assert r["active_outer_area_rows"] == int((~absent).sum()), name
        noise_t = 0.0
        for noise in (1e-13, -1e-13):
            r2 = relax_once(P, T, gp, vo, fixed_out, noise, mods)
            assert r2["counts"] == r["counts"], "the relaxation's evaluation count depends on rounding"
            for a, b in ((r2["tin"], r["tin"]), (r2["tout"], r["tout"])):
                noise_t = max(noise_t, float(np.max(np.abs(a - b)) / np.max(np.abs(b))))
        assert noise_t < 1e-9, noise_t
        E_total = float(r["mz"].compute_energy())
        fout = np.zeros(len(P), bool)
        fout[fixed_out] = True
        out.update({name + "__positions": m.positions_view().copy(), name + "__tri": T, name + "__edges": r["edges"],
                    name + "__gp_json": jdump(gp), name + "__vopts": jdump({str(k): v for k, v in vo.items()}),
                    name + "__absent": np.array(absent, copy=True), name + "__tilt_fixed_out": fout,
                    name + "__tilts_in0": r["tin0"], name + "__tilts_out0": r["tout0"], name + "__tilts_in_final": r["tin"],
                    name + "__tilts_out_final": r["tout"], name + "__E_total": np.array(E_total),
                    name + "__n_gradient_evaluations": np.array(n_grad), name + "__n_energy_evaluations": np.array(n_en),
                    name + "__n_accepted": np.array(n_grad - 1), name + "__noise_tilts": np.array(noise_t),
                    name + "__modules": np.array(mods)})
        print("relax %-7s nv %3d absent %3d gradient evaluations %d energy evaluations %d E_total=%.16g noise %.3g" %
              (name, len(P), int(absent.sum()), n_grad, n_en, E_total, noise_t))
    out["modules"] = np.array(RELAX_MODS)
    save_npz(os.path.join(OUT, "leaflet_absent_relax.npz"), out)


# ---------------------------------------------------------------------------------------------------------------------
TRAJ_MODS = ["tilt_in", "tilt_out", "tilt_smoothness_in", "tilt_smoothness_out", "bending_tilt_in"]
TRAJ_CONS = ["pin_to_circle", "pin_to_plane"]


def traj_once(P, T, gp, vo, n_steps, step_size, perturb):
    def make(noise):
        Pn = np.asarray(P, float) + noise * np.random.default_rng(77).normal(size=np.shape(P))
        m, edges = build(Pn, T, gp, vopts=vo)
        rng = np.random.default_rng(33)
        m.set_tilts_in_from_array(tangent_tilts(m, rng, 0.3))
        m.set_tilts_out_from_array(tangent_tilts(m, rng, 0.24))
        m.energy_modules = list(TRAJ_MODS)
        m.constraint_modules = list(TRAJ_CONS)
        return m, edges

    # E0 / grad0 come from a mesh of their own: an evaluation before minimize() has enforced the pins leaves geometry
    # in the reference's caches that its first iteration then reads
    probe, _e = make(perturb)
    pz = Minimizer(probe, probe.global_parameters, GradientDescent(), EnergyModuleManager(probe.energy_modules),
                   ConstraintModuleManager(probe.constraint_modules), quiet=True, step_size=step_size)
    E0, g0 = pz.compute_energy_and_gradient_array()
    E0, g0 = float(E0), np.array(g0, copy=True)
    m, edges = make(perturb)
    stepper = GradientDescent()
    mz = Minimizer(m, m.global_parameters, stepper, EnergyModuleManager(m.energy_modules),
                   ConstraintModuleManager(m.constraint_modules), quiet=True, step_size=step_size)
    log = []
    orig = stepper.step

    def logged(msh, grad, step, energy_fn, constraint_enforcer=None, **kw):
        r = orig(msh, grad, step, energy_fn, constraint_enforcer=constraint_enforcer, **kw)
        log.append((float(bool(r[0])), float(r[1]), float(r[2])))
        return r

    stepper.step = logged
    pos0 = m.positions_view().copy()
    tin0, tout0 = np.array(m.tilts_in_view(), copy=True), np.array(m.tilts_out_view(), copy=True)
    res = mz.minimize(n_steps)
    bd = mz.compute_energy_breakdown()
    absent = np.array(leaflet_absent_vertex_mask(m, m.global_parameters, leaflet="out"), copy=True)
    return {"positions0": pos0, "tri": np.asarray(m.triangle_row_cache()[0], dtype=np.int32), "fixed": m.fixed_mask.copy(),
            "edges": edges, "vopts": jdump({str(k): v for k, v in vo.items()}), "tilt_fixed_in": np.zeros(len(P), bool),
            "tilt_fixed_out": np.zeros(len(P), bool), "gamma": m.get_facet_parameter_array("surface_tension").copy(),
            "E0": np.array(E0), "grad0": g0, "tilts_in0": tin0, "tilts_out0": tout0,
            "positions_final": m.positions_view().copy(), "tilts_in_final": np.array(m.tilts_in_view(), copy=True),
            "tilts_out_final": np.array(m.tilts_out_view(), copy=True), "step_log": np.array(log),
            "E_final": np.array(res["energy"]), "E_tilt_out_final": np.array(float(bd["tilt_out"])),
            "E_smooth_out_final": np.array(float(bd["tilt_smoothness_out"])), "absent": absent,
            "n_steps": np.array(n_steps), "step_size0": np.array(step_size), "gp_json": jdump(gp),
            "modules": np.array(list(TRAJ_MODS)), "constraint_modules": np.array(list(TRAJ_CONS)),
            "stepper": np.array("GradientDescent")}


def gen_trajectory():
    """Six GD steps on the jittered 6-ring disk: both leaflets' magnitude and smoothness modules and bending_tilt_in, the
    outer leaflet absent on rings 0-2, a slide-mode pin_to_circle group on the boundary ring and a fixed-mode pin_to_plane
    on ring 3 (the pins of traj_disk6_cg_coupling_pins_slide.npz), a nested CG relaxation of 5 iterations per step.  Every
    module of the list is tilt-dependent (the reference's relaxation accepts a tilt step against the TOTAL energy at x)."""
    P, T, B = meshgen.disk_patch(6, bulge=0.3, jitter=0.02, seed=11)
    T = np.asarray(T, np.int32)
    ring3 = ring_rows(3)
    vo = {int(r): {"constraints": ["pin_to_circle"], "pin_to_circle_group": "rim", "pin_to_circle_mode": "slide",
                   "pin_to_circle_normal": [0.0, 0.0, 1.0]} for r in np.flatnonzero(B)}
    z3 = float(np.mean(P[ring3, 2]))
    for r in ring3:
        vo[int(r)] = {"constraints": ["pin_to_plane"], "pin_to_plane_normal": [0.0, 0.0, 1.0],
                      "pin_to_plane_point": [0.0, 0.0, z3], "pin_to_plane_mode": "fixed"}
    for r in rings_upto(2):
        vo[int(r)] = dict(vo.get(int(r), {}), preset="disk")
    gp = dict(BASE_GP, bending_modulus=0.6, spontaneous_curvature=0.05, tilt_solve_mode="nested", tilt_solver="cg",
              tilt_step_size=0.05, tilt_inner_steps=5)
    out = traj_once(P, T, gp, vo, 6, 2e-2, 0.0)
    Lg = out["step_log"]
    assert len(Lg) == 6 and (Lg[:, 0] > 0).sum() >= 3, Lg
    assert out["absent"].sum() == len(rings_upto(2)) and float(out["E_tilt_out_final"]) > 0.0
    assert float(out["E_smooth_out_final"]) > 0.0
    again = traj_once(P, T, gp, vo, 6, 2e-2, 1e-13)
    A = again["step_log"]
    assert A.shape == Lg.shape and np.array_equal(A[:, 0], Lg[:, 0]) and np.allclose(A[:, 1], Lg[:, 1], rtol=1e-9), (A, Lg)
    rel = lambda a, b: float(np.max(np.abs(a - b)) / np.max(np.abs(b)))  # noqa: E731
    out["noise_energy"] = np.array(max(float(np.max(np.abs(A[:, 2] - Lg[:, 2]) / np.abs(Lg[:, 2]))),
                                       abs(float(again["E_final"]) - float(out["E_final"])) / abs(float(out["E_final"]))))
    out["noise_positions"] = np.array(rel(again["positions_final"], out["positions_final"]))
    out["noise_tilts"] = np.array(max(rel(again["tilts_in_final"], out["tilts_in_final"]),
                                      rel(again["tilts_out_final"], out["tilts_out_final"])))
    # the mask matters to this trajectory: without it the first energy differs
    gp_full = dict(gp, leaflet_out_absent_presets=[])
    full = traj_once(P, T, gp_full, vo, 1, 2e-2, 0.0)
    assert abs(float(full["E0"]) - float(out["E0"])) > 1e-6 * abs(float(out["E0"]))
    save_npz(os.path.join(OUT, "traj_disk6_gd_leaflet_absent_pins.npz"), out)
    print("traj_disk6_gd_leaflet_absent_pins.npz E_final=%.16g" % out["E_final"], Lg[:, :2].tolist(),
          "noise E %.3g x %.3g t %.3g" % (out["noise_energy"], out["noise_positions"], out["noise_tilts"]))


if __name__ == "__main__":
    gen_cases()
    gen_relax()
    gen_trajectory()
