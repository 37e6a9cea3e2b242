#!/usr/bin/env python3
"""Generate tests/golden/enforce_only_cases.npz, traj_*_perim_*.npz and traj_*_fplane_*.npz by running the REFERENCE's
perimeter / fixed_plane.

    PYTHONDONTWRITEBYTECODE=1 python3 tools/gen_golden_enforce_only.py [--reference DIR]

Data only: deterministic inputs and what the reference's modules/constraints/perimeter.py, fixed_plane.py, its
ConstraintModuleManager and its Minimizer made of them.  Every trajectory must have at least half of its steps accepted
by the reference.  Every |delta| < tol and norm_sq < 1e-18 decision perimeter.py takes, in the enforcer cases and inside
the trajectories, must keep a factor of 2 from its threshold (a reordered sum must not be able to flip one): the script
follows the module with a NumPy restatement of it and stops otherwise.
"""

from __future__ import annotations

import argparse
import io
import json
import os
import sys
import types
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
from geometry.entities import Body, Edge, Facet, Mesh, Vertex  # noqa: E402
from geometry.geom_io import load_data, parse_geometry  # noqa: E402
from modules.constraints import fixed_plane as ref_fixed_plane  # noqa: E402
from modules.constraints import perimeter as ref_perimeter  # noqa: E402
from runtime.constraint_manager import ConstraintModuleManager  # noqa: E402
from runtime.energy_manager import EnergyModuleManager  # noqa: E402
from runtime.minimizer import Minimizer  # noqa: E402
from runtime.steppers.conjugate_gradient import ConjugateGradient  # noqa: E402
from runtime.steppers.gradient_descent import GradientDescent  # noqa: E402

from membrane_solver_amd import meshgen  # noqa: E402

QUIET = {"mesh_quality_auto_repair_enabled": False}
GP_S = dict(QUIET, surface_tension=1.0, volume_constraint_mode="lagrange")
GP_SB = dict(QUIET, surface_tension=1.0, bending_modulus=1.0, bending_energy_model="helfrich", spontaneous_curvature=0.0,
             volume_constraint_mode="lagrange")


def save_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps: the same arrays give the same bytes on every run."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for key, val in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(val), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())


def build(P, T, gp, fixed_rows=()):
    """Reference Mesh of the triangles T with the rows of `fixed_rows` fixed; -> (mesh, {(lo, hi): edge id})."""
    fixed_rows = set(int(i) for i in fixed_rows)
    m = Mesh()
    for i, p in enumerate(P):
        m.vertices[i] = Vertex(i, np.array(p, float), options={"fixed": True} if i in fixed_rows else {})
        if i in fixed_rows:
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
    return m, emap


def edge_table(m):
    """(n_edges, 2) rows [tail, head]: row k is the reference's edge k + 1."""
    return np.array([[m.edges[e].tail_index, m.edges[e].head_index] for e in range(1, len(m.edges) + 1)], dtype=np.int32)


def rim_edges(T, emap):
    """ids of the edges that lie on one triangle only, ascending."""
    cnt = {}
    for a, b, c in T:
        for u, v in ((a, b), (b, c), (c, a)):
            k = (min(u, v), max(u, v))
            cnt[k] = cnt.get(k, 0) + 1
    return sorted(emap[k] for k, n in cnt.items() if n == 1)


def loop_length(m, signed):
    return float(sum(np.linalg.norm(m.vertices[m.get_edge(s).head_index].position - m.vertices[m.get_edge(s).tail_index].position)
                     for s in signed))


class TooClose(SystemExit):
    """A decision of perimeter.py within a factor of 2 of its threshold: these inputs make no fixture."""


class Margins:
    """NumPy restatement of perimeter.enforce_constraint (perimeter.py:27-74) that notes how far every decision stays
    from its threshold."""

    def __init__(self):
        self.worst_tol = np.inf   # min over decisions of max(|delta| / tol, tol / |delta|)
        self.worst_norm = np.inf

    def note(self, value, thr, which):
        r = np.inf if value == 0.0 else max(value / thr, thr / value)
        setattr(self, which, min(getattr(self, which), r))
        if r < 2.0:
            raise TooClose("a perimeter decision lies within a factor of 2 of its threshold: %r against %r" % (value, thr))

    def run(self, X, fixed, loops, tol=1e-10, max_iter=3):
        """loops: [(tail rows, head rows, target)] -> (positions, passes per loop, P per loop)"""
        X = np.array(X, dtype=float, copy=True)
        passes, per = [], []
        for tail, head, target in loops:
            n, P = 0, 0.0
            for _ in range(max_iter):
                vec = X[head] - X[tail]
                ln = np.array([np.linalg.norm(v) for v in vec])
                P = 0.0
                for v in ln:
                    P += v
                delta = P - target
                self.note(abs(delta), tol, "worst_tol")
                if abs(delta) < tol:
                    break
                g = {}
                for t, h, v, l_ in zip(tail, head, vec, ln):
                    if l_ < 1e-12:
                        continue
                    d = v / l_
                    g.setdefault(int(t), np.zeros(3))
                    g.setdefault(int(h), np.zeros(3))
                    g[int(t)] += -d
                    g[int(h)] += d
                norm_sq = sum(np.dot(v, v) for v in g.values())
                self.note(float(norm_sq), 1e-18, "worst_norm")
                if norm_sq < 1e-18:
                    break
                lam = delta / (norm_sq + 1e-18)
                for r, v in g.items():
                    if not fixed[r]:
                        X[r] -= lam * v
                n += 1
            passes.append(n)
            per.append(P)
        return X, np.array(passes, dtype=np.int32), np.array(per)


def resolve(m, cons):
    """The entries of `cons` that do something as [(tail rows, head rows, target)] (rows == vertex ids here)."""
    out = []
    for c in cons:
        if not c.get("edges") or c.get("target_perimeter") is None:
            continue
        es = [m.get_edge(s) for s in c["edges"]]
        out.append((np.array([e.tail_index for e in es]), np.array([e.head_index for e in es]), float(c["target_perimeter"])))
    return out


def flat_loops(loops):
    off = np.cumsum([0] + [len(t) for t, _h, _p in loops]).astype(np.int32)
    tail = np.concatenate([t for t, _h, _p in loops] or [np.zeros(0)]).astype(np.int32)
    head = np.concatenate([h for _t, h, _p in loops] or [np.zeros(0)]).astype(np.int32)
    return off, tail, head, np.array([p for _t, _h, p in loops], dtype=float)


def ring_start(r):
    return 0 if r == 0 else 1 + 3 * r * (r - 1)


def gen_cases():
    out, pnames, fnames = {}, [], []
    margins = Margins()

    def perim_case(name, n_rings, make_cons, fixed_rows=(), merge=False, keep_tri=True):
        P, T, _B = meshgen.disk_patch(n_rings)
        P = np.array(P, dtype=float)
        m0, emap = build(P, T, QUIET)
        rim = rim_edges(T, emap)
        if merge:  # the head of the first rim edge merged into its tail: a listed edge of length 0
            e = m0.edges[rim[0]]
            P[e.head_index] = P[e.tail_index]
        m, emap = build(P, T, QUIET, fixed_rows)
        cons = make_cons(m, emap, rim)
        m.global_parameters.set("perimeter_constraints", cons)
        pos0 = m.positions_view().copy()
        loops = resolve(m, cons)
        X_np, passes, per = margins.run(pos0, m.fixed_mask, loops)
        ref_perimeter.enforce_constraint(m)
        X = np.array([m.vertices[i].position for i in range(len(P))])
        if np.abs(X - X_np).max() > 1e-13:
            raise SystemExit(name + ": the restatement left the reference's result")
        off, tail, head, target = flat_loops(loops)
        touched = np.flatnonzero(np.any(X != pos0, axis=1)).astype(np.int32)
        out.update({name + "__positions": pos0, name + "__fixed": m.fixed_mask.copy(), name + "__loop_off": off,
                    name + "__tail": tail, name + "__head": head, name + "__target": target, name + "__passes": passes,
                    name + "__perimeter": per, name + "__touched": touched, name + "__positions_touched": X[touched],
                    name + "__constraints": np.array(repr(cons))})
        if keep_tri:
            out.update({name + "__tri": np.asarray(T, dtype=np.int32), name + "__edges": edge_table(m)})
        pnames.append(name)
        print("%-22s nv=%5d loops=%d entries=%4d passes=%s P=%s touched=%d" % (
            name, len(P), len(loops), len(tail), passes.tolist(), ["%.12f" % p for p in per], len(touched)))

    def rim_at(ratio, alternate=False):
        def make(m, emap, rim):
            es = [(-e if alternate and k % 2 else e) for k, e in enumerate(rim)]
            return [{"edges": es, "target_perimeter": ratio * loop_length(m, es)}]
        return make

    def two_loops(m, emap, rim):
        # the rim, an entry without a target, and a spoke from the centre plus the rim arc it ends on
        n = 5
        spoke = []
        for r in range(n):
            k = (min(ring_start(r), ring_start(r + 1)), max(ring_start(r), ring_start(r + 1)))
            if k not in emap:
                raise SystemExit("disk_patch: no spoke edge between rings %d and %d" % (r, r + 1))
            spoke.append(emap[k])
        arc = [e for e in rim if ring_start(n) in (m.edges[e].tail_index, m.edges[e].head_index)]
        second = spoke + [-arc[0]] + rim[3:9]
        return [{"edges": list(rim), "target_perimeter": 0.97 * loop_length(m, rim)},
                {"edges": list(rim)},
                {"edges": second, "target_perimeter": 1.02 * loop_length(m, second)}]

    def duplicate(m, emap, rim):
        es = list(rim) + [rim[4]]
        return [{"edges": es, "target_perimeter": 0.97 * loop_length(m, es)}]

    def zero_pass(m, emap, rim):
        return [{"edges": list(rim), "target_perimeter": loop_length(m, rim)}]

    def single_zero(m, emap, rim):
        return [{"edges": [rim[0]], "target_perimeter": 1.0}]

    perim_case("perim_disk5_rim", 5, rim_at(0.97, alternate=True))
    perim_case("perim_disk12_rim_fixed7", 12, rim_at(0.97), fixed_rows=np.arange(0, 469, 7))
    perim_case("perim_disk48_rim", 48, rim_at(0.97), keep_tri=False)
    perim_case("perim_disk5_exhaust", 5, rim_at(0.8))
    perim_case("perim_disk5_zero_pass", 5, zero_pass)
    perim_case("perim_disk5_two_loops", 5, two_loops)
    perim_case("perim_disk5_duplicate", 5, duplicate)
    perim_case("perim_disk5_merged", 5, rim_at(0.97), merge=True)
    perim_case("perim_disk5_single_zero", 5, single_zero, merge=True)
    print("perimeter decisions: closest to tol by a factor of %.3g, to 1e-18 by %.3g" % (margins.worst_tol, margins.worst_norm))

    def plane_case(name, P, T, gp, fixed_rows=()):
        m, _ = build(P, T, dict(QUIET, **gp), fixed_rows)
        pos0 = m.positions_view().copy()
        ref_fixed_plane.enforce_constraint(m)
        X = np.array([m.vertices[i].position for i in range(len(P))])
        out.update({name + "__positions": pos0, name + "__tri": np.asarray(T, dtype=np.int32), name + "__fixed": m.fixed_mask.copy(),
                    name + "__gp": np.array(repr(gp)), name + "__positions_final": X})
        fnames.append(name)
        n = np.asarray(gp.get("fixed_plane_normal", (0.0, 0.0, 1.0)), dtype=float)
        q = np.asarray(gp.get("fixed_plane_point", (0.0, 0.0, 0.0)), dtype=float)
        d = (X - q) @ (n / np.linalg.norm(n))
        free = ~m.fixed_mask
        print("%-22s nv=%4d free rows off the plane by %.3g, fixed rows by %.3g" % (
            name, len(P), np.abs(d[free]).max(), np.abs(d[~free]).max() if (~free).any() else 0.0))

    P5, T5, B5 = meshgen.disk_patch(5)
    P12, T12, B12 = meshgen.disk_patch(12)
    P4, T4 = meshgen.icosphere(4)
    P4 = meshgen.smooth_displace(P4, 0.05)
    oblique = {"fixed_plane_normal": [0.2, -0.1, 1.0], "fixed_plane_point": [0.0, 0.0, 0.1]}
    plane_case("fplane_disk5_default", P5, T5, {})
    plane_case("fplane_ico4_default", P4, T4, {})
    plane_case("fplane_disk12_oblique", P12, T12, oblique)
    plane_case("fplane_disk12_oblique_fixed", P12, T12, oblique, fixed_rows=np.flatnonzero(B12)[::2])
    plane_case("fplane_disk5_default_fixed", P5, T5, {}, fixed_rows=np.flatnonzero(B5)[::2])
    out["perimeter_names"] = np.array(pnames)
    out["fixed_plane_names"] = np.array(fnames)
    save_npz(os.path.join(OUT, "enforce_only_cases.npz"), out)


def minimizer(m, emods, cmods, stepper, step_size, margins):
    m.energy_modules = list(emods)
    m.constraint_modules = list(cmods)
    cm = ConstraintModuleManager(list(cmods))
    if "perimeter" in cmods:
        def checked(mesh, **kw):  # the restatement first, on a copy, for the decisions' margins; then the module itself
            ids = list(mesh.vertices.keys())
            X = np.array([mesh.vertices[i].position for i in ids])
            fixed = np.array([bool(getattr(mesh.vertices[i], "fixed", False)) for i in ids])
            margins.run(X, fixed, resolve(mesh, mesh.global_parameters.get("perimeter_constraints") or []))
            return ref_perimeter.enforce_constraint(mesh, **kw)

        cm.modules["perimeter"] = types.SimpleNamespace(enforce_constraint=checked, __name__="perimeter")
    return Minimizer(m, m.global_parameters, stepper, EnergyModuleManager(list(emods)), cm, quiet=True, step_size=step_size)


def run_traj(fname, m, emods, cmods, stepper, n_steps, step_size, gp, body_rows=None):
    margins = Margins()
    mz = minimizer(m, emods, cmods, stepper, step_size, margins)
    pos0 = m.positions_view().copy()
    log = []
    orig = stepper.step

    def logged(mesh, grad, step_size, energy_fn, constraint_enforcer=None, trial_energy_fn=None):
        r = orig(mesh, grad, step_size, energy_fn, constraint_enforcer=constraint_enforcer, trial_energy_fn=trial_energy_fn)
        log.append((float(bool(r[0])), float(r[1]), float(r[2])))
        return r

    stepper.step = logged
    res = mz.minimize(n_steps)
    out = {"positions0": pos0, "tri": np.asarray(m.triangle_row_cache()[0], dtype=np.int32), "edges": edge_table(m),
           "fixed": m.fixed_mask.copy(), "gp": np.array(repr(dict(gp))), "energy_modules": np.array(list(emods)),
           "constraint_modules": np.array(list(cmods)), "step_log": np.array(log), "E_final": np.array(res["energy"]),
           "positions_final": m.positions_view().copy(), "step_size_final": np.array(mz.step_size),
           "n_steps": np.array(n_steps), "step_size0": np.array(step_size), "stepper": np.array(type(stepper).__name__)}
    if body_rows is not None:
        b = m.bodies[0]
        out.update({"body_facets": np.asarray(body_rows, dtype=np.int64), "body_options": np.array(repr(dict(b.options)))})
        if b.target_volume is not None:
            out["target_volume"] = np.array(float(b.target_volume))
    save_npz(os.path.join(OUT, fname), out)
    accepted = int(sum(r[0] for r in log))
    print(fname, "E_final=%.16g accepted %d of %d" % (out["E_final"], accepted, len(log)), [(int(a), s) for a, s, _e in log],
          "margins %.3g %.3g" % (margins.worst_tol, margins.worst_norm))
    if 2 * accepted < len(log):
        raise TooFewAccepted(fname + ": the reference accepted fewer than half of the steps")


def facets_area(m, facets):
    pos = m.positions_view()
    idx = m.vertex_index_to_row
    return float(sum(m.facets[f].compute_area_and_gradient(m, positions=pos, index_map=idx)[0] for f in facets))


def add_body(m, rows=None):
    rows = sorted(m.facets.keys()) if rows is None else [int(f) for f in rows]
    b = Body(0, list(rows), target_volume=None, options={})
    m.bodies[0] = b
    return b, np.array(rows, dtype=np.int64)


class TooFewAccepted(SystemExit):
    """The reference accepted fewer than half of a trajectory's steps: these inputs make no fixture."""


NO_FIXTURE = []  # configurations none of whose targets gave a fixture (printed at the end)


def first_clear(what, ratios, run, required=True):
    """run(ratio) for the first of `ratios` whose trajectory keeps every perimeter decision clear of its threshold and has
    half of its steps accepted -> whether one did (the script stops when none does and one is required)."""
    for ratio in ratios:
        try:
            run(ratio)
            return True
        except (TooClose, TooFewAccepted) as e:
            print("%s at %.3f: %s -- next ratio" % (what, ratio, e))
    if required:
        raise SystemExit(what + ": no ratio gives a fixture")
    return False


PERIM_RATIOS = (0.97, 0.975, 0.965, 0.96)   # 3 % below the rim's length first
ICO_RATIOS = (0.98, 0.97, 0.985, 0.99, 0.95, 0.96, 0.93, 0.9)   # 2 % below the listed length first


def gen_trajectories():
    steppers = (("gd", GradientDescent), ("cg", ConjugateGradient))
    # the rim of an open disk held 3 % below its length, alone and next to body_area at the disk's own area
    for n in (5, 12):
        P, T, B = meshgen.disk_patch(n)
        for tag, stepper in steppers:
            for area in (False, True):
                fname = "traj_disk%d_%s_perim_%s.npz" % (n, tag, "area" if area else "alone")

                def run(ratio, area=area, stepper=stepper, fname=fname):
                    m, emap = build(P, T, GP_S)
                    rim = rim_edges(T, emap)
                    cons = [{"edges": list(rim), "target_perimeter": ratio * loop_length(m, rim)}]
                    gp = dict(GP_S, perimeter_constraints=cons)
                    m.global_parameters.set("perimeter_constraints", cons)
                    rows = None
                    cmods = ["perimeter"]
                    if area:
                        # (the body owns the inner facets: over the whole disk its row is the surface gradient itself)
                        b, rows = add_body(m, np.flatnonzero(np.linalg.norm(P[T].mean(axis=1)[:, :2], axis=1) < 0.7))
                        b.options["target_area"] = facets_area(m, rows)
                        cmods = ["perimeter", "body_area"]
                    run_traj(fname, m, ["surface"], cmods, stepper(), 8, 1e-3, gp, rows)

                first_clear(fname, PERIM_RATIOS, run)
    # (the Minimizer refuses perimeter / fixed_plane in front of volume and of an area constraint over vertices they move:
    # the reference takes that projection's first pass from positions cached before them, DESIGN.md section 4y.  The
    # fixtures of those pairs below are written all the same: they are what the change that reproduces it will need)
    # a closed surface: the edges whose midpoint lies above z = 0.5 listed, next to the volume constraint (its row with the
    # drift check, or its enforcer on every trial) and, in half of the runs, body_area at the surface's own area.  Each
    # configuration takes the first target that clears the decision guard and has half of its steps accepted.
    for freq in (4, 8):
        P, T = meshgen.icosphere(freq)
        P = meshgen.smooth_displace(P, 0.05)
        for tag, stepper in steppers:
            for proj in (False, True):
                for area in (False, True):
                    fname = "traj_ico%d_%s_perim_volume_%s%s.npz" % (freq, tag, "enforcer" if proj else "row",
                                                                     "_area" if area else "")

                    def run(ratio, P=P, T=T, stepper=stepper, proj=proj, area=area, fname=fname):
                        gp0 = dict(GP_SB, volume_projection_during_minimization=proj)
                        m, emap = build(P, T, gp0)
                        listed = sorted(e for (u, v), e in emap.items() if 0.5 * (P[u][2] + P[v][2]) > 0.5)
                        cons = [{"edges": listed, "target_perimeter": ratio * loop_length(m, listed)}]
                        gp = dict(gp0, perimeter_constraints=cons)
                        m.global_parameters.set("perimeter_constraints", cons)
                        b, rows = add_body(m)
                        b.target_volume = float(b.compute_volume(m))
                        cmods = ["perimeter", "volume"]
                        if area:
                            b.options["target_area"] = facets_area(m, rows)
                            cmods.append("body_area")
                        run_traj(fname, m, ["surface", "bending"], cmods, stepper(), 8, 1e-3, gp, rows)

                    if not first_clear(fname, ICO_RATIOS, run, required=False):
                        NO_FIXTURE.append(fname)
    # fixed_plane in front of the other enforcers that have no pins: perimeter on the rim, body_area over the inner facets
    oblique = {"fixed_plane_normal": [0.2, -0.1, 1.0], "fixed_plane_point": [0.0, 0.0, 0.1]}
    P, T, B = meshgen.disk_patch(5)
    for tag, stepper in steppers:
        for other in ("perimeter", "body_area"):
            fname = "traj_disk5_%s_fplane_%s.npz" % (tag, "perim" if other == "perimeter" else "area")

            def run(ratio, stepper=stepper, other=other, fname=fname):
                gp = dict(GP_S, **oblique)
                m, emap = build(P, T, gp, fixed_rows=np.flatnonzero(B)[::4])
                rows = None
                if other == "perimeter":
                    rim = rim_edges(T, emap)
                    cons = [{"edges": list(rim), "target_perimeter": ratio * loop_length(m, rim)}]
                    gp = dict(gp, perimeter_constraints=cons)
                    m.global_parameters.set("perimeter_constraints", cons)
                else:
                    b, rows = add_body(m, np.flatnonzero(np.linalg.norm(P[T].mean(axis=1)[:, :2], axis=1) < 0.7))
                    b.options["target_area"] = ratio * facets_area(m, rows)
                run_traj(fname, m, ["surface"], ["fixed_plane", other], stepper(), 8, 1e-3, gp, rows)

            first_clear(fname, PERIM_RATIOS, run)
    # fixed_plane: every second rim vertex fixed (the fixed ones stay off the plane), default and oblique plane
    for n in (5, 12):
        P, T, B = meshgen.disk_patch(n)
        for tag, stepper in steppers:
            for ptag, plane in (("default", {}), ("oblique", oblique)):
                gp = dict(GP_S, **plane)
                m, _ = build(P, T, gp, fixed_rows=np.flatnonzero(B)[::2])
                run_traj("traj_disk%d_%s_fplane_%s.npz" % (n, tag, ptag), m, ["surface"], ["fixed_plane"], stepper(), 8, 1e-3, gp)


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


def gen_decks():
    """The three annulus decks that list fixed_plane next to pin_to_circle, stored as data, 5 GD steps each.  The decks
    are flat already (a fixed_plane that did nothing would pass them): the free vertices between the two rims first get
    a seeded offset of order 0.05, off the plane and within it."""
    for deck in ("annulus_flat_no_tilt", "kozlov_annulus_flat_soft_source", "kozlov_annulus_flat_hard_source"):
        mesh = parse_geometry(load_data(os.path.join(args.reference, "meshes", "caveolin", deck + ".yaml")))
        mesh.global_parameters.update({"mesh_quality_auto_repair_enabled": False})
        rng = np.random.default_rng(11)
        lifted = 0
        for vid in sorted(mesh.vertices):
            v = mesh.vertices[vid]
            if getattr(v, "fixed", False) or "pin_to_circle" in ((v.options or {}).get("constraints") or []):
                continue
            v.position[:] += 0.05 * rng.standard_normal(3)  # (in the plane as well: the symmetric decks start at rest)
            lifted += 1
        if lifted == 0:
            raise SystemExit(deck + ": no free vertex between the rims to lift off the plane")
        if deck == "annulus_flat_no_tilt":
            # flat, between pinned rims, the deck's area is constant: with its uniform surface tension it takes no step.  A
            # seeded tension per facet (0.5 .. 1.5) makes the energy depend on where the free vertices lie in the plane
            for fid in sorted(mesh.facets):
                mesh.facets[fid].options["surface_tension"] = float(rng.uniform(0.5, 1.5))
        mesh.increment_version()
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
        flags = {k: flag(k) for k in ("tilt_fixed", "tilt_fixed_in", "tilt_fixed_out")}
        fixed = mesh.fixed_mask.copy()
        gamma = mesh.get_facet_parameter_array("surface_tension").copy()
        step_size = 1e-3
        stepper = GradientDescent()
        mz = Minimizer(mesh, mesh.global_parameters, stepper, EnergyModuleManager(mesh.energy_modules),
                       ConstraintModuleManager(mesh.constraint_modules), quiet=True, step_size=step_size)
        log = []
        orig = stepper.step

        def logged(msh, grad, step, energy_fn, constraint_enforcer=None, trial_energy_fn=None, orig=orig, log=log):
            r = orig(msh, grad, step, energy_fn, constraint_enforcer=constraint_enforcer, trial_energy_fn=trial_energy_fn)
            log.append((float(bool(r[0])), float(r[1]), float(r[2])))
            return r

        stepper.step = logged
        res = mz.minimize(5)
        out = {"positions0": pos0, "tri": tri, "fixed": fixed, "edges": edges, "vopts": np.array(json.dumps(vo, sort_keys=True)),
               "eopts": np.array(json.dumps(eo, sort_keys=True)), "gamma": gamma, "tilts0": t0[0], "tilts_in0": t0[1],
               "tilts_out0": t0[2], "positions_final": mesh.positions_view().copy(),
               "tilts_final": np.array(mesh.tilts_view(), copy=True), "tilts_in_final": np.array(mesh.tilts_in_view(), copy=True),
               "tilts_out_final": np.array(mesh.tilts_out_view(), copy=True), "step_log": np.array(log),
               "E_final": np.array(res["energy"]), "step_size_final": np.array(mz.step_size), "n_steps": np.array(5),
               "step_size0": np.array(step_size), "stepper": np.array("GradientDescent"),
               "gp_json": np.array(json.dumps(plain(mesh.global_parameters.to_dict()), sort_keys=True)),
               "energy_modules": np.array(list(mesh.energy_modules)), "constraint_modules": np.array(list(mesh.constraint_modules)),
               "lifted": np.array(lifted), **flags}
        fname = "traj_%s_gd_fplane_pins.npz" % deck
        save_npz(os.path.join(OUT, fname), out)
        accepted = int(sum(r[0] for r in log))
        print(fname, "nv=%d lifted=%d max|z0|=%.3g max|z_final| of free rows=%.3g E_final=%.16g accepted %d of %d" % (
            len(pos0), lifted, np.abs(pos0[:, 2]).max(), np.abs(out["positions_final"][~fixed, 2]).max(), out["E_final"],
            accepted, len(log)), [(int(a), s) for a, s, _e in log], list(mesh.energy_modules), list(mesh.constraint_modules))
        if 2 * accepted < len(log) or not log:
            raise SystemExit(fname + ": the reference accepted fewer than half of the steps")


if __name__ == "__main__":
    gen_cases()
    gen_trajectories()
    gen_decks()
    if NO_FIXTURE:
        print("no fixture (no target cleared the decision guard with half of the steps accepted):", NO_FIXTURE)
