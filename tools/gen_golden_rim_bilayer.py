#!/usr/bin/env python3
"""Generate tests/golden/rim_bilayer_cases.npz, rim_bilayer_large.npz, rim_bilayer_relax.npz and
traj_*_rimbilayer_*.npz by running the REFERENCE's tilt_rim_source_bilayer module.

    PYTHONDONTWRITEBYTECODE=1 python3 tools/gen_golden_rim_bilayer.py [--reference DIR]

Data only: deterministic inputs and what the reference's modules/energy/tilt_rim_source_bilayer.py, the leaflet
relaxation and the Minimizer made of them.  Every fixture is asserted to have the property it is named for before it is
written.  Every trajectory and the relaxation are rerun from a start perturbed by 1e-13 and must keep their accept /
reject sequence, step sizes and evaluation counts; how far energies, positions and tilts move under that perturbation is
recorded (``noise_*``): the bar of the device tests is max(1e-12, 10 x that spread).

The mesh builders, the npz writer and the trajectory protocol (mesh-mutating line search with the rejected trials; the
follow-mode trajectory on the reference's array fast path, without tilt_smoothness_*) are those of
tools/gen_golden_rim_source.py, imported from there.

The relaxation fixture is meshes/caveolin/kozlov_1disk_3d_tensionless_bilayer_source.yaml as the deck sets it (nested,
tilt_step_size 0.05, tilt_tol 1e-10, its pins enforced before the relaxation).  RELAX_CAPS lists the tilt_inner_steps
tried in order, the deck's 800 first: the first one whose iteration and evaluation counts survive the perturbation is
recorded.
"""

from __future__ import annotations

import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden_rim_source as rs  # noqa: E402  (parses --reference / --out and puts the reference on sys.path)

from core.parameters.resolver import ParameterResolver  # noqa: E402
from geometry.geom_io import load_data, parse_geometry  # noqa: E402
from runtime.constraint_manager import ConstraintModuleManager  # noqa: E402
from runtime.energy_manager import EnergyModuleManager  # noqa: E402
from runtime.minimizer import Minimizer  # noqa: E402
from runtime.steppers.conjugate_gradient import ConjugateGradient  # noqa: E402
from runtime.steppers.gradient_descent import GradientDescent  # noqa: E402

from membrane_solver_amd import meshgen  # noqa: E402

OUT = rs.OUT
REF = importlib.import_module("modules.energy.tilt_rim_source_bilayer")
NAME = "tilt_rim_source_bilayer"
DECK = os.path.join(rs.args.reference, "meshes", "caveolin", "kozlov_1disk_3d_tensionless_bilayer_source.yaml")
RELAX_CAPS = (800, 400, 200, 100, 50, 25)
save_npz, jdump, build, ring_rows, ring_edge_numbers, tangent_tilts = (rs.save_npz, rs.jdump, rs.build, rs.ring_rows,
                                                                       rs.ring_edge_numbers, rs.tangent_tilts)


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(float(np.max(np.abs(np.asarray(b)))), 1e-300))


def reference_terms(m, positions, tin, tout):
    """(gamma L dots) per rim edge from the reference's own selection, strengths and frame; None when it has none"""
    res = ParameterResolver(m.global_parameters)
    group = REF._resolve_group(res)
    if group is None:
        return None
    payload = REF._rim_selection_payload(m, group=group, mode=REF._resolve_edge_mode(res))
    if payload is None:
        return None
    gamma = np.array([REF._resolve_strength(res, m.edges[int(e)]) for e in payload["edge_ids"]], dtype=float)
    if payload["follow"]:
        center, normal = REF._resolve_followed_circle_frame(m, rows=payload["rim_rows"], normal_row=payload["normal_row"])
    else:
        center, normal = REF._resolve_center(res), np.array([0.0, 0.0, 1.0])
    tails, heads = payload["tails"], payload["heads"]
    p0, p1 = positions[tails], positions[heads]
    r = 0.5 * (p0 + p1) - center[None, :]
    r = r - (r @ normal)[:, None] * normal[None, :]
    rn = np.linalg.norm(r, axis=1)
    r_hat = np.zeros_like(r)
    r_hat[rn > 1e-12] = r[rn > 1e-12] / rn[rn > 1e-12][:, None]
    tsum = 0.5 * (tin[tails] + tin[heads]) + 0.5 * (tout[tails] + tout[heads])
    return {"terms": gamma * np.linalg.norm(p1 - p0, axis=1) * np.einsum("ij,ij->i", tsum, r_hat), "rn": rn, "gamma": gamma,
            "follow": bool(payload["follow"]), "n_edges": len(gamma), "rim_rows": np.asarray(payload["rim_rows"])}


def evaluate(m, pos, tin, tout):
    """the reference's array API, energy-only API and the invariants every case has: no shape gradient, the two tilt
    gradients bit for bit the same"""
    res = ParameterResolver(m.global_parameters)
    g, gi, go = np.zeros_like(pos), np.zeros_like(pos), np.zeros_like(pos)
    E = REF.compute_energy_and_gradient_array(m, m.global_parameters, res, positions=pos, index_map=m.vertex_index_to_row,
                                              grad_arr=g, tilts_in=tin, tilts_out=tout, tilt_in_grad_arr=gi,
                                              tilt_out_grad_arr=go)
    E2 = REF.compute_energy_array(m, m.global_parameters, res, positions=pos, index_map=m.vertex_index_to_row,
                                  tilts_in=tin, tilts_out=tout)
    assert E2 == E and not g.any() and np.array_equal(gi, go)
    return float(E), gi


def deck_mesh():
    """The deck's 84-vertex annulus with its pins enforced -> (reference mesh, minimizer)"""
    mesh = parse_geometry(load_data(DECK))
    mz = Minimizer(mesh, mesh.global_parameters, GradientDescent(), EnergyModuleManager(mesh.energy_modules),
                   ConstraintModuleManager(mesh.constraint_modules), quiet=True)
    mz.enforce_constraints_after_mesh_ops(mesh)
    mesh.project_tilts_to_tangent()
    return mesh, mz


def deck_tables(mesh):
    rows = mesh.vertex_index_to_row
    tri = np.asarray(mesh.triangle_row_cache()[0], dtype=np.int32)
    edges = np.array([[rows[mesh.edges[e].tail_index], rows[mesh.edges[e].head_index]] for e in sorted(mesh.edges)],
                     dtype=np.int64)
    vo = {}
    fin, fout, fixed = np.zeros(len(rows), bool), np.zeros(len(rows), bool), np.zeros(len(rows), bool)
    plain = (int, float, str, bool, list)
    for vid, v in mesh.vertices.items():
        o = {k: val for k, val in (v.options or {}).items() if isinstance(val, plain)}
        if o:
            vo[str(rows[vid])] = o
        fin[rows[vid]] = bool(getattr(v, "tilt_fixed_in", False))
        fout[rows[vid]] = bool(getattr(v, "tilt_fixed_out", False))
        fixed[rows[vid]] = bool(getattr(v, "fixed", False))
    gp = {k: v for k, v in mesh.global_parameters.to_dict().items()
          if isinstance(v, plain) and k.startswith(("tilt_", "bending_", "pin_to_", "spontaneous_", "surface_", "step_size"))}
    return tri, edges, vo, fin, fout, fixed, gp


def gen_cases():
    meshes = {"disk4": meshgen.disk_patch(4), "disk6": meshgen.disk_patch(6, bulge=0.3, jitter=0.02, seed=11)}
    out, names = {}, []
    tilted = (np.array([0.2, -0.1, 1.0]) / np.linalg.norm([0.2, -0.1, 1.0])).tolist()

    def record(name, m, edges, T, vo, eo, gp, pos, tin, tout, E, tg, terms):
        scale = 0.0 if terms is None else float(np.abs(terms["terms"]).sum())
        out.update({name + "__positions": m.positions_view().copy(), name + "__eval_positions": pos,
                    name + "__tri": np.asarray(T, dtype=np.int32), name + "__edges": edges,
                    name + "__vopts": jdump({str(k): v for k, v in vo.items()}),
                    name + "__eopts": jdump({str(k): v for k, v in eo.items()}), name + "__gp": jdump(gp),
                    name + "__tilts_in": tin, name + "__tilts_out": tout, name + "__E": np.array(float(E)),
                    name + "__tilt_grad": tg, name + "__E_scale": np.array(scale),
                    name + "__n_rim_edges": np.array(0 if terms is None else terms["n_edges"])})
        names.append(name)
        print("%-36s rim edges %3d E=% .16g scale=%.6g" % (name, 0 if terms is None else terms["n_edges"], E, scale))

    for mname, (P, T, B) in meshes.items():
        n_rings = 4 if mname == "disk4" else 6
        brows = [int(i) for i in np.flatnonzero(B)]
        r3 = ring_rows(3)
        _m0, edges0 = build(P, T, {})
        e_ring3, e_bnd = ring_edge_numbers(edges0, r3), ring_edge_numbers(edges0, brows)
        assert len(e_ring3) == 18 and len(e_bnd) == 6 * n_rings
        grp = lambda rows, name="rim", **extra: {int(r): dict({"pin_to_circle_group": name}, **extra) for r in rows}  # noqa: E731
        per_edge = {}
        for j, k in enumerate(e_ring3):
            if j % 3 == 0:
                per_edge[k] = {"tilt_rim_source_strength": 1.5 + 0.25 * j}
            elif j % 3 == 1:
                per_edge[k] = {"tilt_rim_source_strength": 0.0}
        one_zero = {e_bnd[2]: {"tilt_rim_source_strength": 0.0}}
        mid_k = e_bnd[5]
        mid_center = (0.5 * (P[edges0[mid_k, 0]] + P[edges0[mid_k, 1]]))
        mid_center = [float(mid_center[0]), float(mid_center[1]), 0.37]  # (on the axis through the midpoint: r = 0)
        G, S = "tilt_rim_source_group", "tilt_rim_source_strength"
        fixed_tilted = {G: "rim", "tilt_rim_source_edge_mode": "all", S: 3.0, "tilt_rim_source_center": [0.07, -0.04, 0.11]}
        cases = {
            "a_boundary_global": (grp(brows), {}, {G: "rim", S: 2.5}, None),
            "b_ring3_all_per_edge": (grp(r3), per_edge, {G: "rim", "tilt_rim_source_edge_mode": "all"}, None),
            "b_one_zero_edge_follow": (grp(brows, pin_to_circle_mode="fit", pin_to_circle_normal=[0.0, 0.0, 2.0]), one_zero,
                                       {G: "rim", S: 1.2}, None),
            # the leaflet-suffixed keys next to it are NOT this module's
            "c_contact_keys": (grp(brows), {}, {G: "rim", "tilt_rim_source_contact_h": 0.7,
                                                "tilt_rim_source_contact_delta_epsilon_over_a": 3.0,
                                                "tilt_rim_source_strength_in": 7.0, "tilt_rim_source_contact_gamma_out": 9.0,
                                                "tilt_rim_source_group_in": "other"}, None),
            "c_contact_si": (grp(brows), {}, {G: "rim", "tilt_rim_source_contact_h": 2.0e-9,
                                              "tilt_rim_source_contact_delta_epsilon": 4.0e-21,
                                              "tilt_rim_source_contact_a": 0.5e-18, "tilt_rim_source_contact_units": "si",
                                              "tilt_rim_source_contact_length_unit_m": 1.0e-8,
                                              "tilt_rim_source_contact_kappa_ref_J": 4.0e-20}, None),
            "d_fixed_frame_ignores_row_normal": (grp(r3, pin_to_circle_normal=[0.2, -0.1, 1.0]), {}, fixed_tilted, None),
            "e_midpoint_on_axis": (grp(brows), {}, {G: "rim", S: 2.0, "tilt_rim_source_center": mid_center}, None),
            "f_follow": (grp(r3, pin_to_circle_mode="fit", pin_to_circle_normal=tilted), {},
                         {G: "rim", "tilt_rim_source_edge_mode": "all", S: 1.75, "tilt_rim_source_center": [5.0, 5.0, 5.0]}, None),
            "f_follow_moved": (grp(r3, pin_to_circle_mode="fit", pin_to_circle_normal=tilted), {},
                               {G: "rim", "tilt_rim_source_edge_mode": "all", S: 1.75}, "moved"),
            "h_no_group": (grp(brows), {}, {S: 2.0, "tilt_rim_source_group_in": "rim", "tilt_rim_source_group_out": "rim"}, None),
            "h_blank_group": (grp(brows), {}, {G: "  ", S: 2.0}, None),
            "h_all_gamma_zero": (grp(brows), {}, {G: "rim", S: 0.0, "tilt_rim_source_strength_in": 2.0}, None),
            "h_boundary_mode_interior": (grp(r3), {}, {G: "rim", S: 2.0}, None),
        }
        for cname, (vo, eo, gp, moved) in cases.items():
            name = f"{mname}_{cname}"
            m, edges = build(P, T, gp, vopts=vo, eopts=eo)
            rng = np.random.default_rng(5)
            tin, tout = tangent_tilts(m, rng, 0.3), tangent_tilts(m, rng, 0.25)
            pos = m.positions_view().copy()
            if moved:  # evaluated on positions that are not the mesh's: the followed center stays the mesh's (:355)
                pos = pos + 0.03 * np.random.default_rng(9).normal(size=pos.shape)
            E, tg = evaluate(m, pos, tin, tout)
            terms = reference_terms(m, pos, tin, tout)
            if cname.startswith("h_"):
                assert E == 0.0 and not tg.any(), name
            else:
                assert terms is not None and abs(-terms["terms"].sum() - E) <= 1e-13 * np.abs(terms["terms"]).sum(), name
                assert E != 0.0 and tg.any()
                if cname == "b_ring3_all_per_edge":
                    assert (terms["gamma"] == 0).sum() == 12 and (terms["gamma"] != 0).sum() == 6
                if cname == "b_one_zero_edge_follow":
                    assert (terms["gamma"] == 0).sum() == 1 and terms["follow"] and len(terms["rim_rows"]) == len(brows)
                if cname == "c_contact_keys":
                    assert np.all(terms["gamma"] == 0.7 * 3.0)
                if cname == "c_contact_si":
                    assert abs(terms["gamma"][0] - 2.0e-9 * (4.0e-21 / 0.5e-18) * 1.0e-8 / 4.0e-20) < 1e-18
                if cname == "d_fixed_frame_ignores_row_normal":  # the same case without the rows' normal: the same doubles
                    m2, _ = build(P, T, gp, vopts=grp(r3), eopts=eo)
                    E_plain, tg_plain = evaluate(m2, pos, tin, tout)
                    assert E_plain == E and np.array_equal(tg_plain, tg)
                    # ... while the inner-leaflet module would read it
                    gpi = {"tilt_rim_source_group_in": "rim", "tilt_rim_source_edge_mode": "all",
                           "tilt_rim_source_strength_in": 3.0, "tilt_rim_source_center": [0.07, -0.04, 0.11]}
                    mi, _ = build(P, T, gpi, vopts=vo, eopts=eo)
                    Ei = rs.REF["in"].compute_energy_array(mi, mi.global_parameters, ParameterResolver(mi.global_parameters),
                                                           positions=pos, index_map=mi.vertex_index_to_row, tilts_in=tin + tout,
                                                           tilts_out=tout)
                    assert abs(Ei - E) > 1e-6 * abs(E)
                if cname == "e_midpoint_on_axis":
                    assert (terms["rn"] <= 1e-12).sum() == 1
                if cname.startswith("f_"):
                    assert terms["follow"]
            if not moved:  # (the dict API evaluates the mesh's own positions and tilts)
                m.set_tilts_in_from_array(tin)
                m.set_tilts_out_from_array(tout)
                res = ParameterResolver(m.global_parameters)
                Ed, gd, tgi, tgo = REF.compute_energy_and_gradient(m, m.global_parameters, res)
                scale = 0.0 if terms is None else float(np.abs(terms["terms"]).sum())
                assert abs(Ed - E) <= 1e-13 * max(scale, 1e-300) and gd == {}
                assert sorted(tgi) == sorted(tgo) == [int(r) for r in np.flatnonzero(np.any(tg != 0.0, axis=1))]
                assert REF.compute_energy_and_gradient(m, m.global_parameters, res, compute_gradient=False) == (Ed, {})
            record(name, m, edges, T, vo, eo, gp, pos, tin, tout, E, tg, terms)
    # the deck's annulus with the deck's own parameters: 12 rim edges, 12 rim rows, gamma 50
    mesh, _mz = deck_mesh()
    tri, edges, vo, _fin, _fout, _fixed, gp = deck_tables(mesh)
    rng = np.random.default_rng(5)
    tin, tout = tangent_tilts(mesh, rng, 0.3), tangent_tilts(mesh, rng, 0.25)
    pos = mesh.positions_view().copy()
    E, tg = evaluate(mesh, pos, tin, tout)
    terms = reference_terms(mesh, pos, tin, tout)
    assert len(pos) == 84 and terms["n_edges"] == 12 and len(terms["rim_rows"]) == 12 and not terms["follow"]
    # the docstring's equivalence: the two leaflet modules with equal parameters give this energy
    gpe = dict(mesh.global_parameters.to_dict(), tilt_rim_source_group_in="inner", tilt_rim_source_group_out="inner",
               tilt_rim_source_strength_in=50.0, tilt_rim_source_strength_out=50.0)
    me, _ = build(pos, tri, gpe, vopts={int(k): v for k, v in vo.items()})
    rese = ParameterResolver(me.global_parameters)
    E_io = sum(rs.REF[lf].compute_energy_array(me, me.global_parameters, rese, positions=pos, index_map=me.vertex_index_to_row,
                                               tilts_in=tin, tilts_out=tout) for lf in ("in", "out"))
    assert abs(E_io - E) <= 1e-13 * np.abs(terms["terms"]).sum()
    record("annulus_deck", mesh, edges, tri, {int(k): v for k, v in vo.items()}, {}, gp, pos, tin, tout, E, tg, terms)
    out["names"] = np.array(names)
    import inspect
    out["reference_signatures"] = jdump({fn: [p for p in inspect.signature(getattr(REF, fn)).parameters]
                                         for fn in ("compute_energy_and_gradient", "compute_energy_and_gradient_array",
                                                    "compute_energy_array")})
    out["reference_flags"] = jdump({"USES_TILT_LEAFLETS": bool(REF.USES_TILT_LEAFLETS),
                                    "IS_EXTERNAL_WORK": bool(REF.IS_EXTERNAL_WORK)})
    save_npz(os.path.join(OUT, "rim_bilayer_cases.npz"), out)


def gen_large():
    """disk_patch(44): a boundary ring of 264 rows -- the smallest rim whose apply launch has a second workgroup.  Only
    the rim rows' tilts and gradients are stored; the test rebuilds the mesh and fills the other tilt rows with zeros."""
    P, T, B = meshgen.disk_patch(44)
    brows = np.flatnonzero(B)
    assert len(brows) == 264
    gp = {"tilt_rim_source_group": "rim", "tilt_rim_source_strength": 1.3, "tilt_rim_source_center": [0.3, -0.2, 0.0]}
    vo = {int(r): {"pin_to_circle_group": "rim"} for r in brows}
    m, _edges = build(P, T, gp, vopts=vo)
    rng = np.random.default_rng(5)
    tin, tout = np.zeros_like(P), np.zeros_like(P)
    tin[brows] = 0.3 * rng.normal(size=(264, 3))
    tout[brows] = 0.25 * rng.normal(size=(264, 3))
    pos = m.positions_view().copy()
    E, tg = evaluate(m, pos, tin, tout)
    terms = reference_terms(m, pos, tin, tout)
    assert terms["n_edges"] == 264 and np.array_equal(np.flatnonzero(np.any(tg != 0.0, axis=1)), brows)
    print("large rim: 264 rows E=%.16g scale=%.6g" % (E, np.abs(terms["terms"]).sum()))
    save_npz(os.path.join(OUT, "rim_bilayer_large.npz"),
             {"rings": np.array(44), "gp": jdump(gp), "rim_rows": brows.astype(np.int32), "tilts_in_rim": tin[brows],
              "tilts_out_rim": tout[brows], "E": np.array(E), "tilt_grad_rim": tg[brows],
              "E_scale": np.array(float(np.abs(terms["terms"]).sum()))})


# ---------------------------------------------------------------------------------------------------------------------
def gen_relax():
    def run(cap, noise):
        mesh, mz = deck_mesh()
        mesh.global_parameters.update({"tilt_inner_steps": int(cap)})
        rows = mesh.vertex_index_to_row
        nv = len(rows)
        free_in = np.array([not getattr(mesh.vertices[v], "tilt_fixed_in", False) for v in mesh.vertex_ids])
        free_out = np.array([not getattr(mesh.vertices[v], "tilt_fixed_out", False) for v in mesh.vertex_ids])
        # a start off the zero field: the deck's fields start at 0, where a 1e-13 perturbation would be the whole field
        tin0 = tangent_tilts(mesh, np.random.default_rng(33), 0.05) * free_in[:, None]
        tout0 = tangent_tilts(mesh, np.random.default_rng(34), 0.04) * free_out[:, None]
        pert = noise * np.random.default_rng(77).normal(size=(nv, 3))
        pert[:, 2] = 0.0  # (the annulus is flat: the perturbed field stays tangent)
        mesh.set_tilts_in_from_array(tin0 + pert * free_in[:, None])
        mesh.set_tilts_out_from_array(tout0 + pert * free_out[:, None])
        mgr = mz._tilt_relaxation_manager
        count = [0, 0]

        def counted(fn, k):
            def wrapper(*a, **kw):
                count[k] += 1
                return fn(*a, **kw)
            return wrapper

        mgr.compute_energy_and_leaflet_tilt_gradients_array_fn = counted(mgr.compute_energy_and_leaflet_tilt_gradients_array_fn, 0)
        mgr.compute_tilt_dependent_energy_with_leaflet_tilts_fn = counted(mgr.compute_tilt_dependent_energy_with_leaflet_tilts_fn, 1)
        assert mz._uses_leaflet_tilts()
        pos0 = mesh.positions_view().copy()
        mz._relax_leaflet_tilts(positions=mesh.positions_view(), mode="nested")
        assert np.array_equal(mesh.positions_view(), pos0)
        stop = str(mgr.last_leaflet_relaxation_stats.get("stop_reason"))
        return mesh, mz, tin0, tout0, (count[0], count[1]), stop

    for cap in RELAX_CAPS:
        mesh, mz, tin0, tout0, counts, stop = run(cap, 0.0)
        stable = stop in ("converged", "completed_max_iters")
        spread_t, spread_e = 0.0, 0.0
        E_total = float(mz.compute_energy())
        for noise in (1e-13, -1e-13):
            m2, mz2, _a, _b, n2, stop2 = run(cap, noise)
            dev = max(rel(m2.tilts_in_view(), mesh.tilts_in_view()), rel(m2.tilts_out_view(), mesh.tilts_out_view()))
            de = abs(float(mz2.compute_energy()) - E_total) / abs(E_total)
            print("   tilt_inner_steps %d perturbed by %g: counts %s vs %s (%s), fields differ by %.3g, energy by %.3g"
                  % (cap, noise, n2, counts, stop2, dev, de))
            stable = stable and n2 == counts and stop2 == stop and dev < 1e-9
            spread_t, spread_e = max(spread_t, dev), max(spread_e, de)
        if stable:
            break
    assert stable, "the relaxation's stopping point depends on rounding at every tilt_inner_steps tried"
    tri, edges, vo, fin, fout, fixed, gp = deck_tables(mesh)
    tin, tout = np.array(mesh.tilts_in_view(), copy=True), np.array(mesh.tilts_out_view(), copy=True)
    res = ParameterResolver(mesh.global_parameters)
    E_rim = REF.compute_energy_array(mesh, mesh.global_parameters, res, positions=mesh.positions_view(),
                                     index_map=mesh.vertex_index_to_row, tilts_in=tin, tilts_out=tout)
    assert E_rim < 0.0 and np.max(np.abs(tin - tin0)) > 1e-3 and np.max(np.abs(tout - tout0)) > 1e-3
    assert not tin[fin].any() and not tout[fout].any()
    print("relaxation: tilt_inner_steps %d (%s) gradient evaluations %d energy evaluations %d E_rim=%.16g E_total=%.16g "
          "spread tilts %.3g energy %.3g" % (cap, stop, counts[0], counts[1], E_rim, E_total, spread_t, spread_e))
    save_npz(os.path.join(OUT, "rim_bilayer_relax.npz"),
             {"positions": mesh.positions_view().copy(), "tri": tri, "edges": edges, "fixed": fixed, "vopts": jdump(vo),
              "tilt_fixed_in": fin, "tilt_fixed_out": fout, "gp_json": jdump(gp),
              "modules": np.array(list(mesh.energy_modules)), "constraint_modules": np.array(list(mesh.constraint_modules)),
              "tilts_in0": tin0, "tilts_out0": tout0, "tilts_in_final": tin, "tilts_out_final": tout,
              "E_rim": np.array(float(E_rim)), "E_total": np.array(E_total), "tilt_inner_steps": np.array(int(cap)),
              "n_gradient_evaluations": np.array(counts[0]), "n_energy_evaluations": np.array(counts[1]),
              "n_evaluations": np.array(counts[0] + counts[1]), "stop_reason": np.array(stop),
              "noise_tilts": np.array(spread_t), "noise_energy": np.array(spread_e)})


# ---------------------------------------------------------------------------------------------------------------------
def run_traj(fname, P, T, gp, vo, mods, stepper_cls, n_steps, step_size, fixed, check, fast_path=False):
    def once(Pin):
        out = rs.run_once(Pin, T, gp, vo, mods, stepper_cls, n_steps, step_size, fixed, fast_path, (0, 0))
        m, _ = build(out["positions_final"], T, gp, vopts=vo)
        E_rim, _tg = evaluate(m, out["positions_final"], out["tilts_in_final"], out["tilts_out_final"])
        out["E_rim_final"] = np.array(E_rim)
        return out

    out = once(P)
    L = out["step_log"]
    check(L, out)
    assert float(out["E_rim_final"]) != 0.0, fname
    again = once(np.asarray(P, dtype=float) + 1e-13 * np.random.default_rng(77).normal(size=np.shape(P)))
    A = again["step_log"]
    assert A.shape == L.shape and np.array_equal(A[:, 0], L[:, 0]) and np.allclose(A[:, 1], L[:, 1], rtol=1e-9), fname
    out["noise_energy"] = np.array(max(float(np.max(np.abs(A[:, 2] - L[:, 2]) / np.abs(L[:, 2]))),
                                       abs(float(again["E_final"]) - float(out["E_final"])) / abs(float(out["E_final"]))))
    out["noise_positions"] = np.array(rel(again["positions_final"], out["positions_final"]))
    out["noise_tilts"] = np.array(max(rel(again["tilts_in_final"], out["tilts_in_final"]),
                                      rel(again["tilts_out_final"], out["tilts_out_final"])))
    save_npz(os.path.join(OUT, fname), out)
    print(fname, "E_final=%.16g" % out["E_final"], L[:, :2].tolist(),
          "noise E %.3g x %.3g t %.3g" % (out["noise_energy"], out["noise_positions"], out["noise_tilts"]))
    return out


def relaxations_restart_alike(P, T, gp, vo, mods, stepper_cls, n_steps, step_size, fixed):
    """Every nested relaxation inside the reference's trajectory gives the tilts the reference gives when the same
    relaxation is restarted, in a fresh Minimizer, from the positions and tilts it started from."""
    def minimizer(pos, tin, tout):
        m, _ = build(pos, T, gp, vopts=vo, fixed=fixed)
        m.set_tilts_in_from_array(tin)
        m.set_tilts_out_from_array(tout)
        m.energy_modules, m.constraint_modules = list(mods), []
        return m, Minimizer(m, m.global_parameters, stepper_cls(), EnergyModuleManager(m.energy_modules),
                            ConstraintModuleManager([]), quiet=True, step_size=step_size)

    m0, _ = build(P, T, gp, vopts=vo, fixed=fixed)
    tin0, tout0, _fin, _fout = rs.set_fields(m0, 33, 0.3)
    m, mz = minimizer(P, tin0, tout0)
    snaps, orig = [], mz._relax_leaflet_tilts

    def hooked(*a, **k):
        pre = (m.positions_view().copy(), np.array(m.tilts_in_view()), np.array(m.tilts_out_view()))
        r = orig(*a, **k)
        snaps.append((pre, np.array(m.tilts_in_view()), np.array(m.tilts_out_view())))
        return r

    mz._relax_leaflet_tilts = hooked
    mz.minimize(n_steps)
    assert len(snaps) >= 2
    for pre, tin, tout in snaps:
        m2, mz2 = minimizer(*pre)
        mz2._relax_leaflet_tilts(positions=m2.positions_view(), mode="nested")
        dev = max(rel(m2.tilts_in_view(), tin), rel(m2.tilts_out_view(), tout))
        assert dev <= 1e-12, "a relaxation inside the trajectory differs from its restart by %.3g" % dev


def gen_trajectories():
    quiet = {"mesh_quality_auto_repair_enabled": False, "volume_constraint_mode": "lagrange",
             "volume_projection_during_minimization": False}
    P6, T6, B6 = meshgen.disk_patch(6, bulge=0.3, jitter=0.02, seed=11)
    P5, T5, B5 = meshgen.disk_patch(5, bulge=0.3, jitter=0.02, seed=7)
    r3 = ring_rows(3)
    vo = {int(r): {"pin_to_circle_group": "rim", "pin_to_circle_normal": [0.0, 0.0, 1.0]} for r in r3}
    base = dict(quiet, surface_tension=1.0, tilt_modulus_in=2.0, tilt_modulus_out=1.4, bending_modulus=0.6,
                tilt_rim_source_group="rim", tilt_rim_source_strength=0.8, tilt_rim_source_edge_mode="all",
                tilt_rim_source_center=[0.02, -0.01, 0.0])

    def some_trial_rejected(step0):
        def check(L, _out):
            # an accepted step whose alpha lies below the step size it was given: a trial before it was rejected
            assert (L[:, 0] > 0).sum() >= 3, L
            given = np.concatenate([[step0], L[:-1, 1]])
            assert np.any((L[:, 0] > 0) & (L[:, 1] < 1.5 * given * 0.999)), L
        return check

    def some_accepted(L, _out):
        assert (L[:, 0] > 0).sum() >= 3, L

    # 1: GD + nested CG relaxation, fixed frame, boundary vertices fixed, a step that backtracks.  No bending_modulus: no
    # module of this list reads it, but the reference's leaflet Jacobi diagonal (runtime/preconditioners.py:62-150) would
    # -- with cotangent weights that are not those of the positions it is handed, so that a relaxation inside a
    # trajectory differs from the same relaxation restarted from the same positions and tilts.  The fixture has to be a
    # function of its inputs: relaxations_restart_alike asserts that on the reference alone.
    # (Without that part the diagonal is k_t A_v alone; moduli of 20 / 14 keep the five CG iterations a descent that the
    # shape steps can follow: with 2 / 1.4 the reference rejects every shape step after the first.)
    gp1 = dict(base, tilt_solve_mode="nested", tilt_solver="cg", tilt_step_size=0.05, tilt_inner_steps=5,
               tilt_modulus_in=20.0, tilt_modulus_out=14.0)
    gp1.pop("bending_modulus")
    mods1 = ["surface", "tilt_in", "tilt_out", NAME]
    relaxations_restart_alike(P6, T6, gp1, vo, mods1, GradientDescent, 3, 0.5, B6)
    run_traj("traj_disk6_gd_rimbilayer_nested_cg.npz", P6, T6, gp1, vo, mods1, GradientDescent, 5, 0.5, B6,
             some_trial_rejected(0.5))
    # 2: CG + coupled relaxation with both leaflets' bending_tilt
    run_traj("traj_disk6_cg_rimbilayer_coupled_gd.npz", P6, T6,
             dict(base, tilt_solve_mode="coupled", tilt_solver="gd", tilt_step_size=0.03, tilt_coupled_steps=3,
                  spontaneous_curvature=0.05),
             vo, ["tilt_in", "tilt_out", "bending_tilt_in", "bending_tilt_out", NAME], ConjugateGradient, 5, 2e-3, B6,
             some_accepted)
    # 3: follow mode without an enforcer, the reference's array fast path: every trial takes the BASELINE center
    vof = {int(r): {"pin_to_circle_group": "rim", "pin_to_circle_mode": "fit", "pin_to_circle_normal": [0.0, 0.0, 1.0]}
           for r in r3}
    gpf = dict(base, tilt_rim_source_strength=3.0)
    gpf.pop("tilt_rim_source_center")
    mods3 = ["surface", "tilt_in", "tilt_out", NAME]

    def all_accepted(L, _out):
        assert len(L) == 4 and (L[:, 0] > 0).all(), L
        assert np.allclose(L[:, 1], 1.5 * np.concatenate([[2e-2], L[:-1, 1]]), rtol=1e-12), L  # (no trial rejected)

    fast = run_traj("traj_disk5_gd_rimbilayer_follow_fastpath.npz", P5, T5, gpf, vof, mods3, GradientDescent, 4, 2e-2, B5,
                    all_accepted, fast_path=True)
    slow = rs.run_once(P5, T5, gpf, vof, mods3, GradientDescent, 4, 2e-2, B5, False, (0, 0))
    all_accepted(slow["step_log"], slow)  # the same decisions: what differs is the center the trials were given
    diff = np.abs(fast["step_log"][:, 2] - slow["step_log"][:, 2]) / np.abs(fast["step_log"][:, 2])
    print("follow quirk: trial energies differ from the mesh-mutating run by", diff.tolist())
    assert diff.min() > 1e-9, "the baseline-center quirk does not show in this trajectory"


if __name__ == "__main__":
    gen_cases()
    gen_large()
    gen_relax()
    gen_trajectories()
