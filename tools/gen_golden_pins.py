#!/usr/bin/env python3
"""Generate tests/golden/pin_*.npz and traj_*_pins_*.npz by running the REFERENCE's pin_to_plane / pin_to_circle.

    PYTHONDONTWRITEBYTECODE=1 python3 tools/gen_golden_pins.py [--reference DIR]

Data only: seeded inputs and what the reference's enforce_all / apply_gradient_modifications_array / Minimizer
made of them.
"""

from __future__ import annotations

import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "tests", "golden")

ap = argparse.ArgumentParser()
ap.add_argument("--reference", default="/root/reference")
ap.add_argument("--only-new", action="store_true", help="volume cases, deck trajectories and deck decisions only")
args = ap.parse_args()
sys.dont_write_bytecode = True
sys.path.insert(0, args.reference)
sys.path.insert(0, ROOT)

from core.parameters.global_parameters import GlobalParameters  # noqa: E402
from geometry.entities import Body, Edge, Facet, Mesh, Vertex  # noqa: E402
from geometry.geom_io import load_data, parse_geometry  # noqa: E402
from modules.constraints import volume as cvolume  # noqa: E402
from runtime.constraint_projection import _coalesce_sparse_row_payload, _solve_kkt_system  # noqa: E402
from runtime.constraint_manager import ConstraintModuleManager  # noqa: E402
from runtime.energy_manager import EnergyModuleManager  # noqa: E402
from runtime.minimizer import Minimizer  # noqa: E402
from runtime.steppers.conjugate_gradient import ConjugateGradient  # noqa: E402
from runtime.steppers.gradient_descent import GradientDescent  # noqa: E402

from membrane_solver_amd import meshgen  # noqa: E402


def build(P, T, gp, fixed=None, vopts=None, eopts=None):
    """Reference Mesh with per-vertex options (vopts[row]) and per-edge options (eopts[(u, v)] for u < v); returns
    the mesh and its edge table (tail, head) in edge-id order."""
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
                m.edges[e] = Edge(e, int(u), int(v), options=dict((eopts or {}).get(k, {})))
                nid += 1
            se.append(e if m.edges[e].tail_index == u else -e)
        m.facets[fi] = Facet(fi, se, options={})
    m.global_parameters = GlobalParameters(dict(gp))
    m.build_connectivity_maps()
    m.build_facet_vertex_loops()
    edges = np.array([[m.edges[e].tail_index, m.edges[e].head_index] for e in sorted(m.edges)], dtype=np.int64)
    return m, edges


def ring_rows(P, B):
    return np.flatnonzero(B)


def ring_edges(T, B):
    out = set()
    for a, b, c in T:
        for u, v in ((a, b), (b, c), (c, a)):
            if B[u] and B[v]:
                out.add((min(u, v), max(u, v)))
    return sorted(out)


def opts_table(m, edges):
    """Options as the ArrayMesh takes them: vertex rows -> dict, edge index (edge-id order) -> dict."""
    vo = {i: dict(m.vertices[i].options) for i in m.vertices if m.vertices[i].options}
    eo = {k: dict(m.edges[e].options) for k, e in enumerate(sorted(m.edges)) if m.edges[e].options}
    return vo, eo


def gen_cases():
    Pd, Td, Bd = meshgen.disk_patch(5, jitter=0.15, seed=5)
    rng = np.random.default_rng(11)
    Pd = Pd + rng.normal(scale=0.03, size=Pd.shape)
    ring = ring_rows(Pd, Bd)
    redges = ring_edges(Td, Bd)
    band = np.flatnonzero(np.abs(np.linalg.norm(Pd[:, :2], axis=1) - 0.5) < 0.12)
    circ = {"constraints": ["pin_to_circle"]}
    plane = {"constraints": ["pin_to_plane"]}
    both = {"constraints": ["pin_to_plane", "pin_to_circle"]}
    fix2 = np.zeros(len(Pd), bool)
    fix2[ring[::5]] = True
    cases = {
        "plane_fixed_vertices": ({"pin_to_plane_point": [0, 0, 0.05]}, {int(i): plane for i in ring}, {}, None),
        "plane_fixed_edges": ({"pin_to_plane_normal": [0, 0, 2.0]}, {}, {e: plane for e in redges}, None),
        "plane_slide": ({"pin_to_plane_mode": "slide"}, {int(i): plane for i in band}, {}, None),
        "plane_slide_fixed_members": ({"pin_to_plane_mode": "slide"}, {int(i): plane for i in ring}, {}, fix2),
        "circle_fixed_vertices": ({"pin_to_circle_radius": 1.02}, {int(i): circ for i in ring}, {}, None),
        "circle_fixed_edges": ({"pin_to_circle_radius": 0.98, "pin_to_circle_point": [0, 0, 0.02]}, {},
                               {e: circ for e in redges}, None),
        "circle_slide": ({"pin_to_circle_mode": "slide", "pin_to_circle_normal": [0, 0, 1]},
                         {int(i): circ for i in ring}, {}, None),
        "circle_slide_radius_fixed_members": ({"pin_to_circle_mode": "slide", "pin_to_circle_normal": [0, 0, 1],
                                               "pin_to_circle_radius": 1.0}, {int(i): circ for i in ring}, {}, fix2),
        "plane_and_circle_same_vertex": ({"pin_to_circle_radius": 1.0}, {int(i): both for i in ring}, {}, None),
        "plane_slide_circle_slide": ({"pin_to_plane_mode": "slide", "pin_to_circle_mode": "slide",
                                      "pin_to_circle_normal": [0, 0, 1]}, {int(i): both for i in ring}, {}, None),
    }
    out = {}
    names = []
    for name, (gp, vopts, eopts, fixed) in cases.items():
        m, edges = build(Pd, Td, gp, fixed=fixed, vopts=vopts, eopts=eopts)
        mods = ["pin_to_plane", "pin_to_circle"]
        cm = ConstraintModuleManager(mods)
        pos0 = m.positions_view().copy()
        G = rng.normal(size=pos0.shape)
        g1 = G.copy()
        cm.apply_gradient_modifications_array(g1, m, m.global_parameters)
        cm.enforce_all(m, global_params=m.global_parameters, context="minimize")
        m.increment_version()
        pos1 = m.positions_view().copy()
        vo, eo = opts_table(m, edges)
        out[name + "__positions0"] = pos0
        out[name + "__positions1"] = pos1
        out[name + "__grad0"] = G
        out[name + "__grad1"] = g1
        out[name + "__fixed"] = np.zeros(len(Pd), bool) if fixed is None else fixed
        out[name + "__edges"] = edges
        out[name + "__vopts"] = np.array(repr(vo))
        out[name + "__eopts"] = np.array(repr(eo))
        out[name + "__gp"] = np.array(repr(gp))
        names.append(name)
    out["tri"] = Td
    out["names"] = np.array(names)
    np.savez_compressed(os.path.join(OUT, "pin_cases.npz"), **out)
    print("pin_cases.npz", names)


def run_traj(fname, m, edges, stepper, n_steps, step_size, extra=None):
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
    vo, eo = opts_table(m, edges)
    out = {"positions0": pos0, "tri": np.asarray(m.triangle_row_cache()[0], dtype=np.int32),
           "fixed": m.fixed_mask.copy(), "edges": edges, "vopts": np.array(repr(vo)), "eopts": np.array(repr(eo)),
           "gp": np.array(repr(dict(m.global_parameters.to_dict() if hasattr(m.global_parameters, "to_dict")
                                    else {}))),
           "energy_modules": np.array(list(m.energy_modules)), "constraint_modules": np.array(list(m.constraint_modules)),
           "step_log": np.array(log), "E_final": np.array(res["energy"]), "positions_final": m.positions_view().copy(),
           "step_size_final": np.array(mz.step_size), "n_steps": np.array(n_steps), "step_size0": np.array(step_size),
           "stepper": np.array(type(stepper).__name__)}
    out.update(extra or {})
    np.savez_compressed(os.path.join(OUT, fname), **out)
    print(fname, "E_final=%.16g" % out["E_final"], out["step_log"].tolist())


def gen_trajectories():
    base = {"surface_tension": 1.0, "bending_modulus": 1.0, "bending_energy_model": "helfrich",
            "spontaneous_curvature": 0.0, "mesh_quality_auto_repair_enabled": False}
    Pd, Td, Bd = meshgen.disk_patch(5, jitter=0.15, seed=5)
    rng = np.random.default_rng(7)
    Pd = Pd + np.stack([np.zeros(len(Pd)), np.zeros(len(Pd)), rng.normal(scale=0.04, size=len(Pd))], axis=1)
    ring = ring_rows(Pd, Bd)
    circ = {"constraints": ["pin_to_circle"]}
    both = {"constraints": ["pin_to_plane", "pin_to_circle"]}
    gp = dict(base, pin_to_circle_radius=1.0)
    m, edges = build(Pd, Td, gp, vopts={int(i): circ for i in ring})
    m.energy_modules = ["surface", "bending"]
    m.constraint_modules = ["pin_to_circle"]
    run_traj("traj_disk5_gd_pins_circle_fixed.npz", m, edges, GradientDescent(), 6, 1e-3)
    gp = dict(base, pin_to_plane_mode="slide", pin_to_circle_mode="slide", pin_to_circle_normal=[0, 0, 1])
    m, edges = build(Pd, Td, gp, vopts={int(i): both for i in ring})
    m.energy_modules = ["surface", "bending"]
    m.constraint_modules = ["pin_to_plane", "pin_to_circle"]
    run_traj("traj_disk5_cg_pins_slide_skip.npz", m, edges, ConjugateGradient(), 8, 1e-3)


def add_body(m):
    b = Body(0, list(m.facets.keys()), target_volume=None)
    m.bodies[0] = b
    b.target_volume = float(b.compute_volume(m))
    return b


def ico8_band():
    P, T = meshgen.icosphere(8)
    P = meshgen.smooth_displace(P, 0.05)
    band = np.flatnonzero(np.abs(P[:, 2]) < 0.04)
    return P, T, band


def gen_volume_cases():
    """Pins with the Lagrange volume row: the band on pin_to_plane fixed (full rank), and on both pins (skip)."""
    P, T, band = ico8_band()
    rng = np.random.default_rng(13)
    plane = {"constraints": ["pin_to_plane"]}
    both = {"constraints": ["pin_to_plane", "pin_to_circle"]}
    cases = {"volume_plane_fixed": ({}, {int(i): plane for i in band}),
             "volume_plane_and_circle": ({"pin_to_circle_radius": 1.0}, {int(i): both for i in band})}
    out, names = {}, []
    for name, (gp, vopts) in cases.items():
        gp = dict(gp, volume_constraint_mode="lagrange", volume_projection_during_minimization=False)
        m, edges = build(P, T, gp, vopts=vopts)
        add_body(m)
        mods = ["pin_to_plane", "pin_to_circle", "volume"]
        cm = ConstraintModuleManager(mods)
        pos0 = m.positions_view().copy()
        vg = cvolume.constraint_gradients_array(m, m.global_parameters, positions=pos0,
                                                index_map=m.vertex_index_to_row)[0]
        G = rng.normal(size=pos0.shape)
        g1 = G.copy()
        cm.apply_gradient_modifications_array(g1, m, m.global_parameters)
        cm.enforce_all(m, global_params=m.global_parameters, context="minimize")  # (the volume projection is off)
        m.increment_version()
        vo, eo = opts_table(m, edges)
        out.update({name + "__positions0": pos0, name + "__positions1": m.positions_view().copy(),
                    name + "__grad0": G, name + "__grad1": g1, name + "__vgrad": np.asarray(vg),
                    name + "__fixed": np.zeros(len(P), bool), name + "__edges": edges,
                    name + "__vopts": np.array(repr(vo)), name + "__eopts": np.array(repr(eo)),
                    name + "__gp": np.array(repr(gp))})
        names.append(name)
    out["tri"] = T
    out["names"] = np.array(names)
    np.savez_compressed(os.path.join(OUT, "pin_volume_cases.npz"), **out)
    print("pin_volume_cases.npz", names)


def gen_volume_trajectories():
    P, T, band = ico8_band()
    plane = {"constraints": ["pin_to_plane"]}
    for proj, fname, n in ((False, "traj_ico8_gd_pins_volume_kkt.npz", 6), (True, "traj_ico8_gd_pins_volume_enforcer.npz", 6)):
        gp = {"surface_tension": 1.0, "volume_constraint_mode": "lagrange",
              "volume_projection_during_minimization": proj, "mesh_quality_auto_repair_enabled": False}
        m, edges = build(P, T, gp, vopts={int(i): plane for i in band})
        add_body(m)
        m.energy_modules = ["surface"]
        m.constraint_modules = ["pin_to_plane", "volume"]
        run_traj(fname, m, edges, GradientDescent(), n, 2e-2,
                 extra={"gp": np.array(repr(gp)), "target_volume": np.array(m.bodies[0].target_volume)})


def gen_deck_trajectories():
    for deck, n in (("catenoid.json", 8), ("good_min_cap.json", 8)):
        m = parse_geometry(load_data(os.path.join(args.reference, "meshes", deck)))
        gpd = {k: v for k, v in m.global_parameters.to_dict().items()} if hasattr(m.global_parameters, "to_dict") \
            else dict(load_data(os.path.join(args.reference, "meshes", deck)).get("global_parameters", {}))
        edges = np.array([[m.edges[e].tail_index, m.edges[e].head_index] for e in sorted(m.edges)], dtype=np.int64)
        m.build_position_cache()
        rows = m.vertex_index_to_row
        edges = np.array([[rows[t], rows[h]] for t, h in edges], dtype=np.int64)
        extra = {"gp": np.array(repr(_plain(gpd)))}
        if m.bodies:
            b = next(iter(m.bodies.values()))
            extra["target_volume"] = np.array(float(b.target_volume if b.target_volume is not None
                                                    else b.options.get("target_volume")))
        vo = {rows[v]: _plain(m.vertices[v].options) for v in m.vertices if m.vertices[v].options}
        eo = {k: _plain(m.edges[e].options) for k, e in enumerate(sorted(m.edges)) if m.edges[e].options}
        stepper = GradientDescent()
        fname = "traj_%s_gd_pins_fixed_rings.npz" % deck.split(".")[0]
        extra["vopts_rows"] = np.array(repr(vo))
        extra["eopts_rows"] = np.array(repr(eo))
        extra["edge_rows"] = edges
        run_traj(fname, m, edges, stepper, n, 1e-3, extra=extra)


def _plain(d):
    out = {}
    for k, v in (d or {}).items():
        if isinstance(v, (int, float, str, bool)) or v is None:
            out[k] = v
        elif isinstance(v, (list, tuple, np.ndarray)):
            out[k] = [x if isinstance(x, (str, bool)) else float(x) for x in np.asarray(v).tolist()] \
                if not isinstance(v, (list, tuple)) or all(not isinstance(x, str) for x in v) else list(v)
    return out


def _deck_files():
    out = []
    for sub in ("meshes", "benchmarks/inputs", "tests/fixtures"):
        base = os.path.join(args.reference, sub)
        for dp, _dn, fn in os.walk(base):
            for f in sorted(fn):
                if f.endswith((".json", ".yaml", ".yml")):
                    path = os.path.join(dp, f)
                    try:
                        txt = open(path).read()
                    except OSError:
                        continue
                    if "pin_to_plane" in txt or "pin_to_circle" in txt:
                        out.append(path)
    return sorted(out)


_PIN_KEYS = ("constraints",)


def _pin_opts(o):
    if not o:
        return None
    d = {k: v for k, v in o.items() if k.startswith("pin_to_") or k == "constraints"}
    c = d.get("constraints")
    if c is None:
        return None
    return _plain(d)


def gen_deck_decisions():
    """Per deck that uses pins: the reference's row count, rank of C and KKT outcome (pins + a Lagrange volume row),
    and the reduced inputs the resolver needs to repeat the decision (pinned vertices only; the volume row's part on
    the other vertices as one extra row of the same norm)."""
    out, names = {}, []
    for path in _deck_files():
        name = os.path.relpath(path, args.reference)
        try:
            m = parse_geometry(load_data(path))
        except Exception as e:  # noqa: BLE001
            print("skip (parse)", name, type(e).__name__, e)
            continue
        cons = [c for c in m.constraint_modules if c in ("pin_to_plane", "pin_to_circle", "volume")]
        gp = m.global_parameters
        pos = m.positions_view()
        idx = m.vertex_index_to_row
        sparse, dense = [], []
        try:
            for c in cons:
                if c == "volume":
                    if gp.get("volume_constraint_mode", "lagrange") != "lagrange" or not m.bodies:
                        continue
                    g = cvolume.constraint_gradients_array(m, gp, positions=pos, index_map=idx)
                    dense.extend(g or [])
                    continue
                mod = __import__("modules.constraints." + c, fromlist=["x"])
                for payload in mod.constraint_gradients_rows_array(m, gp, positions=pos, index_map=idx) or []:
                    r, v = _coalesce_sparse_row_payload(np.asarray(payload[0]).reshape(-1), np.asarray(payload[1], float))
                    if r.size:
                        sparse.append((r, v))
        except Exception as e:  # noqa: BLE001
            print("skip (rows)", name, type(e).__name__, e)
            continue
        k = len(dense) + len(sparse)
        if k == 0:
            decision, rank = "none", 0
        else:
            C = np.zeros((k, pos.size))
            for i, g in enumerate(dense):
                C[i] = np.asarray(g).reshape(-1)
            for j, (r, v) in enumerate(sparse):
                np.add.at(C[len(dense) + j].reshape(-1, 3), r, v)
            rank = int(np.linalg.matrix_rank(C))
            if k == 1:
                decision = "project"
            else:
                A = C @ C.T
                A[np.diag_indices_from(A)] += 1e-18
                decision = "project" if _solve_kkt_system(A, C @ np.ones(pos.size)) is not None else "skip"
        # reduced inputs
        tagged_e = [(m.edges[e].tail_index, m.edges[e].head_index, _pin_opts(m.edges[e].options))
                    for e in m.edges if _pin_opts(m.edges[e].options)]
        vids = set(v for v in m.vertices if _pin_opts(m.vertices[v].options))
        for t, h, _o in tagged_e:
            vids.update((t, h))
        vids = sorted(vids)
        red = {v: i for i, v in enumerate(vids)}
        X = np.array([pos[idx[v]] for v in vids] + [[0.0, 0.0, 0.0]])
        vg = np.zeros((len(vids) + 1, 3))
        if dense:
            g = np.asarray(dense[0])
            for v in vids:
                vg[red[v]] = g[idx[v]]
            rest = float(np.sum(g * g) - np.sum(vg * vg))
            vg[-1, 0] = np.sqrt(max(rest, 0.0))
        fixed = np.array([bool(getattr(m.vertices[v], "fixed", False)) for v in vids] + [False])
        vo = {red[v]: _pin_opts(m.vertices[v].options) for v in vids if _pin_opts(m.vertices[v].options)}
        er = np.array([[red[t], red[h]] for t, h, _o in tagged_e], dtype=np.int64).reshape(-1, 2)
        eo = {i: o for i, (_t, _h, o) in enumerate(tagged_e)}
        gpd = {kk: vv for kk, vv in (gp.to_dict() if hasattr(gp, "to_dict") else {}).items()
               if kk.startswith("pin_to_")}
        key = "d%03d" % len(names)
        out.update({key + "__name": np.array(name), key + "__n_rows": np.array(k), key + "__rank": np.array(rank),
                    key + "__decision": np.array(decision), key + "__positions": X, key + "__fixed": fixed,
                    key + "__vgrad": vg, key + "__has_volume": np.array(bool(dense)),
                    key + "__vopts": np.array(repr(vo)), key + "__edges": er, key + "__eopts": np.array(repr(eo)),
                    key + "__gp": np.array(repr(_plain(gpd))), key + "__cons": np.array(cons)})
        names.append(key)
        print(name, k, rank, decision)
    out["keys"] = np.array(names)
    np.savez_compressed(os.path.join(OUT, "pin_deck_decisions.npz"), **out)


if __name__ == "__main__":
    if "--only-new" not in sys.argv:
        gen_cases()
        gen_trajectories()
    gen_volume_cases()
    gen_volume_trajectories()
    gen_deck_trajectories()
    gen_deck_decisions()
