#!/usr/bin/env python3
"""Generate tests/golden/traj_*_pins*.npz of the pins-next-to-tilt-modules lane by running the REFERENCE's Minimizer.

    PYTHONDONTWRITEBYTECODE=1 python3 tools/gen_golden_pins_tilt.py --reference DIR [--out DIR]

Data only: a deck (or a seeded mesh) as arrays and option tables, and what the reference's Minimizer, its steppers and
its mesh-mutating line search (runtime/steppers/line_search.py:428-498, the loop an enforcer selects) made of it.  The
same inputs give the same bytes on every run.

Besides the keys of traj_disk6_gd_rimsource_nested_cg.npz every file carries
  trial_log   one row per energy evaluation of a line-search trial:
              (step, alpha, E_trial, E0 + c alpha <g,d>, accepted, max row move of the tilt projection on that trial)
  search_log  one row per search: (E0, <g,d>, step size given, trials evaluated, guard rejections)
  tilts_*_steps  the tilt fields after every step
  positions_at_x, tilts_*_at_x  per search: the positions and the tilts after energy_fn's projection at x, which is
              what the search snapshots and a rejected trial restores
(grad0 is the reference's compute_energy_and_gradient_array: after the pins' KKT projection and the fixed rows' zeroing;
the disk6 file also carries grad0_raw, the same gradient with no constraint module loaded)
and every file is asserted to have the properties it is named for before it is written.
"""

from __future__ import annotations

import argparse
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
ap.add_argument("--reference", required=True, help="checkout of the reference project (imported at run time)")
ap.add_argument("--out", default=OUT, help="directory the fixtures are written to")
args = ap.parse_args()
OUT = args.out
os.makedirs(OUT, exist_ok=True)
sys.dont_write_bytecode = True
sys.path.insert(0, args.reference)
sys.path.insert(0, ROOT)

from core.parameters.global_parameters import GlobalParameters  # noqa: E402
from geometry.entities import Edge, Facet, Mesh, Vertex  # noqa: E402
from geometry.geom_io import load_data, parse_geometry  # noqa: E402
from runtime.constraint_manager import ConstraintModuleManager  # noqa: E402
from runtime.energy_manager import EnergyModuleManager  # noqa: E402
from runtime.minimizer import Minimizer  # noqa: E402
from runtime.steppers import line_search as ls_mod  # noqa: E402
from runtime.steppers import conjugate_gradient as cg_mod  # noqa: E402
from runtime.steppers import gradient_descent as gd_mod  # noqa: E402

from membrane_solver_amd import meshgen  # noqa: E402

C1, BETA = 1e-4, 0.7  # (the steppers' defaults; asserted against the stepper below)


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


def plain(d):
    """options / parameters as JSON: numbers, strings, booleans and flat lists of them"""
    out = {}
    for k, v in (d or {}).items():
        if isinstance(v, (bool, str)) or v is None:
            out[k] = v
        elif isinstance(v, (int, float, np.integer, np.floating)):
            out[k] = float(v) if isinstance(v, (float, np.floating)) else int(v)
        elif isinstance(v, (list, tuple, np.ndarray)):
            out[k] = [x if isinstance(x, (str, bool)) else float(x) for x in np.asarray(v, dtype=object).tolist()]
    return out


def build(P, T, gp, vopts=None, fixed=None):
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
                m.edges[e] = Edge(e, int(u), int(v), options={})
                nid += 1
            se.append(e if m.edges[e].tail_index == u else -e)
        m.facets[fi] = Facet(fi, se, options={})
    m.global_parameters = GlobalParameters(dict(gp))
    m.build_connectivity_maps()
    m.build_facet_vertex_loops()
    return m


def tangent_tilts(m, rng, scale):
    pos = m.positions_view()
    tl = scale * rng.normal(size=pos.shape)
    nrm = m.vertex_normals(pos)
    return tl - np.einsum("ij,ij->i", tl, nrm)[:, None] * nrm


class SearchSpy:
    """Wraps the line search the steppers call: logs every trial evaluation, its alpha, its Armijo bound, and how far
    energy_fn's projection moved the stored tilts on that trial."""

    def __init__(self, single):
        self.trials, self.searches, self.step = [], [], 0
        self.at_x = []  # per search: (positions, tilt fields) as the search snapshots them
        self.single = single
        self.orig = ls_mod.backtracking_line_search_array

    def fields(self, mesh):
        if self.single:
            return (np.array(mesh.tilts_view(), copy=True),)
        return np.array(mesh.tilts_in_view(), copy=True), np.array(mesh.tilts_out_view(), copy=True)

    def __call__(self, mesh, direction, gradient, step_size, energy_fn, vertex_ids, **kw):
        assert kw.get("constraint_enforcer") is not None, "the fixture is about the enforcer lane"
        assert kw.get("beta", BETA) == BETA and kw.get("c", C1) == C1
        enforcer = kw["constraint_enforcer"]
        gdd = float(np.sum(gradient * direction))
        state = {"n_energy": 0, "E0": None, "snap": None, "alpha": None, "n_enf": 0}
        base = mesh.positions_view().copy()
        rows = np.flatnonzero(~mesh.fixed_mask)
        lead = rows[np.argmax(np.linalg.norm(direction[rows], axis=1))] if rows.size else 0

        def spy_enforcer(msh):
            # the positions are x + alpha d here (un-enforced): alpha from the row that moves most, snapped to the ladder
            mv = msh.positions_view()[lead] - base[lead]
            a_est = float(mv @ direction[lead]) / float(direction[lead] @ direction[lead])
            k = int(round(np.log(a_est / step_size) / np.log(BETA)))
            a = step_size
            for _ in range(k):
                a *= BETA
            assert abs(a - a_est) <= 1e-9 * a, (a, a_est)
            state["alpha"] = a
            state["k"] = k
            state["n_enf"] += 1
            return enforcer(msh)

        def spy_energy():
            E = float(energy_fn())
            if state["n_energy"] == 0:
                state["E0"] = E
                state["snap"] = self.fields(mesh)  # (what the search snapshots: the tilts projected at x)
                self.at_x.append((mesh.positions_view().copy(),) + state["snap"])
            else:
                now = self.fields(mesh)
                move = max(float(np.max(np.linalg.norm(a - b, axis=1))) for a, b in zip(now, state["snap"]))
                rhs = state["E0"] + C1 * state["alpha"] * gdd
                self.trials.append([self.step, state["alpha"], E, rhs, float(E <= rhs), move])
            state["n_energy"] += 1
            return E

        kw["constraint_enforcer"] = spy_enforcer
        kw.pop("trial_energy_fn", None)
        r = self.orig(mesh, direction, gradient, step_size, spy_energy, vertex_ids, trial_energy_fn=None, **kw)
        n_tr = state["n_energy"] - 1
        guard = 0
        if n_tr > 0:
            guard = (state["k"] + 1) - n_tr  # ladder positions used up to the last evaluated trial minus the evaluated ones
        self.searches.append([state["E0"], gdd, step_size, n_tr, guard])
        if not r[0] and n_tr > 0:  # rejected to the end: the tilts are the snapshot again, bit for bit
            for a, b in zip(self.fields(mesh), state["snap"]):
                assert np.array_equal(a, b)
        self.step += 1
        return r


def run(make_mesh, stepper_mod, stepper_cls, n_steps, step_size, single):
    # E0 / grad0 come from a mesh of their own: an evaluation BEFORE minimize() has enforced the pins leaves geometry in
    # the reference's caches that its first iteration then reads (the soft_source deck's pins move its rounded
    # coordinates by 3e-9, and the trajectory after such a probe differs by 1e-8 in the outer leaflet's tilts)
    probe = make_mesh()
    pz = Minimizer(probe, probe.global_parameters, stepper_cls(), EnergyModuleManager(probe.energy_modules),
                   ConstraintModuleManager(probe.constraint_modules), quiet=True, step_size=step_size)
    probe_E0, probe_g0 = pz.compute_energy_and_gradient_array()
    probe_E0, probe_g0 = float(probe_E0), np.array(probe_g0, copy=True)
    mesh = make_mesh()
    spy = SearchSpy(single)
    stepper_mod.backtracking_line_search_array = spy
    try:
        stepper = stepper_cls()
        assert stepper.beta == BETA and stepper.c == C1
        mz = Minimizer(mesh, mesh.global_parameters, stepper, EnergyModuleManager(mesh.energy_modules),
                       ConstraintModuleManager(mesh.constraint_modules), quiet=True, step_size=step_size)
        log, per_step = [], []
        orig = stepper.step

        def logged(msh, grad, step, energy_fn, constraint_enforcer=None, trial_energy_fn=None):
            r = orig(msh, grad, step, energy_fn, constraint_enforcer=constraint_enforcer, trial_energy_fn=trial_energy_fn)
            log.append((float(bool(r[0])), float(r[1]), float(r[2])))
            return r

        stepper.step = logged
        mesh.build_position_cache()
        rows = mesh.vertex_index_to_row
        order = sorted(mesh.vertices, key=lambda v: rows[v])
        pos0 = mesh.positions_view().copy()
        t0 = (np.array(mesh.tilts_view(), copy=True), np.array(mesh.tilts_in_view(), copy=True),
              np.array(mesh.tilts_out_view(), copy=True))
        tri = np.asarray(mesh.triangle_row_cache()[0], dtype=np.int32)
        edges = np.array([[rows[mesh.edges[e].tail_index], rows[mesh.edges[e].head_index]] for e in sorted(mesh.edges)],
                         dtype=np.int64)
        vo = {str(rows[v]): plain(mesh.vertices[v].options) for v in order if plain(mesh.vertices[v].options)}
        eo = {str(k): plain(mesh.edges[e].options) for k, e in enumerate(sorted(mesh.edges)) if plain(mesh.edges[e].options)}
        flag = lambda name: np.array([bool(getattr(mesh.vertices[v], name, False)) for v in order])  # noqa: E731
        fixed = mesh.fixed_mask.copy()

        def after_step(msh, i):
            if i > 0:
                per_step.append((np.array(msh.tilts_view(), copy=True), np.array(msh.tilts_in_view(), copy=True),
                                 np.array(msh.tilts_out_view(), copy=True)))

        res = mz.minimize(n_steps, callback=after_step)
        per_step.append((np.array(mesh.tilts_view(), copy=True), np.array(mesh.tilts_in_view(), copy=True),
                         np.array(mesh.tilts_out_view(), copy=True)))
    finally:
        stepper_mod.backtracking_line_search_array = spy.orig
    gp = plain(mesh.global_parameters.to_dict())
    out = {"positions0": pos0, "tri": tri, "fixed": fixed, "edges": edges, "vopts": jdump(vo), "eopts": jdump(eo),
           "tilt_fixed": flag("tilt_fixed"), "tilt_fixed_in": flag("tilt_fixed_in"), "tilt_fixed_out": flag("tilt_fixed_out"),
           "gamma": mesh.get_facet_parameter_array("surface_tension").copy(), "E0": np.array(probe_E0),
           "grad0": np.array(probe_g0), "tilts0": t0[0], "tilts_in0": t0[1],
           "tilts_out0": t0[2], "positions_final": mesh.positions_view().copy(),
           "tilts_final": per_step[-1][0], "tilts_in_final": per_step[-1][1], "tilts_out_final": per_step[-1][2],
           "tilts_steps": np.array([p[0] for p in per_step]), "tilts_in_steps": np.array([p[1] for p in per_step]),
           "tilts_out_steps": np.array([p[2] for p in per_step]), "step_log": np.array(log),
           "positions_at_x": np.array([a[0] for a in spy.at_x]),
           **({"tilts_at_x": np.array([a[1] for a in spy.at_x])} if single else
              {"tilts_in_at_x": np.array([a[1] for a in spy.at_x]), "tilts_out_at_x": np.array([a[2] for a in spy.at_x])}),
           "trial_log": np.array(spy.trials).reshape(-1, 6), "search_log": np.array(spy.searches).reshape(-1, 5),
           "E_final": np.array(res["energy"]), "n_steps": np.array(n_steps), "step_size0": np.array(step_size),
           "gp_json": jdump(gp), "modules": np.array(list(mesh.energy_modules)),
           "constraint_modules": np.array(list(mesh.constraint_modules)), "stepper": np.array(stepper_cls.__name__),
           "fast_path": np.array(False), "armijo_c": np.array(C1), "beta": np.array(BETA)}
    return out


def armijo_margin_ok(out):
    """every trial's distance from its Armijo bound is at least 1e-9 |E0|: no decision hangs on rounding"""
    tl, sl = out["trial_log"], out["search_log"]
    for row in tl:
        e0 = sl[int(row[0]), 0]
        assert abs(row[2] - row[3]) >= 1e-9 * abs(e0), ("Armijo margin", row.tolist(), e0)


def finish(fname, out):
    armijo_margin_ok(out)
    assert len(out["tilts_in_steps"]) == int(out["n_steps"]) == len(out["step_log"])
    save_npz(os.path.join(OUT, fname), out)
    size = os.path.getsize(os.path.join(OUT, fname))
    assert size < (1 << 20), size
    tl = out["trial_log"]
    print(fname, size, "bytes; trials per step", [int((tl[:, 0] == s).sum()) for s in range(int(out["n_steps"]))],
          "accepted", out["step_log"][:, 0].tolist(), "E_final=%.16g" % out["E_final"])


def gen_softsource():
    """meshes/caveolin/kozlov_1disk_3d_tensionless_single_leaflet_soft_source.yaml as data, 4 GD steps from the deck's
    own step size (0.006, step_size_mode fixed)."""
    deck = os.path.join(args.reference, "meshes", "caveolin", "kozlov_1disk_3d_tensionless_single_leaflet_soft_source.yaml")

    def make():
        mesh = parse_geometry(load_data(deck))
        mesh.global_parameters.update({"mesh_quality_auto_repair_enabled": False})
        return mesh

    out = run(make, gd_mod, gd_mod.GradientDescent, 4, float(make().global_parameters.get("step_size")), single=False)
    assert len(out["positions0"]) == 84 and len(out["tri"]) == 144
    tl, sl, L = out["trial_log"], out["search_log"], out["step_log"]
    for s in range(3):  # steps 1-3: rejected trials, then an accepted one
        rows = tl[tl[:, 0] == s]
        assert L[s, 0] == 1.0 and len(rows) >= 2 and rows[-1, 4] == 1.0 and not rows[:-1, 4].any(), (s, rows)
    rows = tl[tl[:, 0] == 3]
    assert L[3, 0] == 0.0 and len(rows) + int(sl[3, 4]) == 10 and not rows[:, 4].any(), rows  # step 4 runs out
    rej = tl[tl[:, 4] == 0.0]
    assert rej[:, 5].max() > 1e-9, "no rejected trial moved a tilt row: a lane without the restore would pass"
    finish("traj_softsource_deck_gd_pins.npz", out)


def gen_disk6_coupling():
    """disk6, CG, coupled relaxation: a slide-mode pin_to_circle group on the rim, a fixed-mode pin_to_plane on ring 3."""
    P, T, B = meshgen.disk_patch(6, bulge=0.3, jitter=0.02, seed=11)
    ring3 = list(range(1 + 3 * 3 * 2, 1 + 3 * 3 * 2 + 18))
    vo = {int(r): {"constraints": ["pin_to_circle"], "pin_to_circle_group": "rim", "pin_to_circle_mode": "slide",
                   "pin_to_circle_normal": [0.0, 0.0, 1.0]} for r in np.flatnonzero(B)}
    z3 = float(np.mean(P[ring3, 2]))
    for r in ring3:
        vo[int(r)] = {"constraints": ["pin_to_plane"], "pin_to_plane_normal": [0.0, 0.0, 1.0],
                      "pin_to_plane_point": [0.0, 0.0, z3], "pin_to_plane_mode": "fixed"}
    gp = {"mesh_quality_auto_repair_enabled": False, "surface_tension": 1.0, "tilt_modulus_in": 2.0, "tilt_modulus_out": 1.4,
          "bending_modulus": 0.6, "bending_modulus_in": 0.6, "bending_modulus_out": 0.6, "spontaneous_curvature": 0.05,
          "tilt_coupling_modulus": 0.9, "tilt_coupling_mode": "difference",
          "tilt_solve_mode": "coupled", "tilt_solver": "gd", "tilt_step_size": 0.03, "tilt_coupled_steps": 3}

    def make():
        m = build(P, T, gp, vopts=vo)
        rng = np.random.default_rng(33)
        m.set_tilts_in_from_array(tangent_tilts(m, rng, 0.3))
        m.set_tilts_out_from_array(tangent_tilts(m, rng, 0.24))
        m.energy_modules = ["surface", "tilt_in", "tilt_out", "tilt_coupling", "bending_tilt_in"]
        m.constraint_modules = ["pin_to_circle", "pin_to_plane"]
        return m

    # the KKT solve projects: the pins change the raw gradient
    m = make()
    m.constraint_modules = []
    mz = Minimizer(m, m.global_parameters, gd_mod.GradientDescent(), EnergyModuleManager(m.energy_modules),
                   ConstraintModuleManager([]), quiet=True)
    g_raw = np.array(mz.compute_energy_and_gradient_array()[1], copy=True)
    out = run(make, cg_mod, cg_mod.ConjugateGradient, 6, 2e-2, single=False)
    assert len(out["positions0"]) == 127
    out["grad0_raw"] = np.array(g_raw)
    assert np.max(np.abs(out["grad0"] - g_raw)) > 1e-6 * np.max(np.abs(g_raw)), "the pins' rows were not projected out"
    assert (out["trial_log"][:, 4] == 0.0).any(), "no trial was rejected"
    finish("traj_disk6_cg_coupling_pins_slide.npz", out)


def gen_ico4():
    """icosphere(4) (162 vertices), single field: tilt + bending_tilt, a fixed-mode pin_to_plane on an equatorial band."""
    P, T = meshgen.icosphere(4)
    P = meshgen.smooth_displace(P, 0.05)
    band = np.flatnonzero(np.abs(P[:, 2]) < 0.12)
    assert 8 <= len(band) <= 40 and len(P) == 162, (len(band), len(P))
    vo = {int(r): {"constraints": ["pin_to_plane"], "pin_to_plane_normal": [0.0, 0.0, 1.0],
                   "pin_to_plane_point": [0.0, 0.0, 0.0], "pin_to_plane_mode": "fixed"} for r in band}
    gp = {"mesh_quality_auto_repair_enabled": False, "tilt_rigidity": 1.5, "tilt_modulus": 1.5, "bending_modulus": 0.8,
          "bending_energy_model": "helfrich", "spontaneous_curvature": 0.1}

    def make():
        m = build(P, T, gp, vopts=vo)
        m.set_tilts_from_array(tangent_tilts(m, np.random.default_rng(5), 0.3))
        m.energy_modules = ["tilt", "bending_tilt"]
        m.constraint_modules = ["pin_to_plane"]
        return m

    out = run(make, gd_mod, gd_mod.GradientDescent, 5, 2e-2, single=True)
    assert out["step_log"][:, 0].sum() >= 3
    finish("traj_ico4_gd_bt_pins_plane.npz", out)


if __name__ == "__main__":
    gen_softsource()
    gen_disk6_coupling()
    gen_ico4()
