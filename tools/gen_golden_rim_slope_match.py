#!/usr/bin/env python3
"""Generate tests/golden/rim_slope_match_cases.npz, rim_slope_match_relax.npz, the two traj_disk6_*_rsm_*.npz and
traj_deck_gd_rsm_profile.npz by running the REFERENCE's rim_slope_match_out module with a non-zero strength.

    PYTHONDONTWRITEBYTECODE=1 python3 tools/gen_golden_rim_slope_match.py [--reference DIR]

Data only: deterministic inputs and what the reference's modules/energy/rim_slope_match_out.py and the leaflet relaxation
made of them.  The mesh builders, the npz writer and the tilt fields are those of tools/gen_golden_rim_source.py, imported
from there.

Ring rules.  The module orders each ring by np.argsort(atan2) and pairs rim and outer entries BY INDEX, so both a tie and
atan2's branch cut decide the answer.  Asserted inside the reference's own _order_by_angle, at every position the
reference evaluates: adjacent angles of an ordered ring differ by at least 1e-6 rad, and every angle keeps
pi - |angle| >= 1e-6.  meshgen.disk_patch is rotated about z by a fixed irrational angle for that: unrotated it has a
vertex on the negative x axis.  Threshold margins, asserted at every evaluation of the module as well (its
array entry point is wrapped): no |dr| in [0.5e-8, 2e-8] and no r_len in [0.5e-12, 2e-12]; rows exactly on a threshold's failing side (dr == 0, a rim row on the center) are cases.

The cases store the rings only (rows, positions, tilts, expected gradient rows): the mesh is the rotated disk_patch with
its vertices renumbered by a seeded permutation, which the tests rebuild -- the vertex ids are scrambled against the
angular order and the sort decides the answer.

The relaxation and the trajectories are rerun from a start perturbed by 1e-13 and must keep their evaluation counts, stop
reason, accept / reject sequence and step sizes; a trajectory must also come out the same with the reference's geometry
caches switched off.  How far tilts, positions and energy move under that perturbation is recorded (``noise_*``): the bar of the device tests is
max(1e-12, 10 x that spread).
"""

from __future__ import annotations

import functools
import importlib
import inspect
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden_rim_source as rs  # noqa: E402  (parses --reference / --out and puts the reference on sys.path)

from core.parameters.resolver import ParameterResolver  # noqa: E402
from runtime.constraint_manager import ConstraintModuleManager  # noqa: E402
from runtime.energy_manager import EnergyModuleManager  # noqa: E402
from runtime.minimizer import Minimizer  # noqa: E402
from runtime.steppers.conjugate_gradient import ConjugateGradient  # noqa: E402
from runtime.steppers.gradient_descent import GradientDescent  # noqa: E402

from membrane_solver_amd import meshgen  # noqa: E402

OUT = rs.OUT
REF = importlib.import_module("modules.energy.rim_slope_match_out")
NAME = "rim_slope_match_out"
MIN_GAP = 1e-6
ROT = float(np.sqrt(2.0) / 3.0)  # radians about z
RELAX_CAPS = (40, 20, 10, 5)
save_npz, jdump, build, ring_rows = rs.save_npz, rs.jdump, rs.build, rs.ring_rows

# --- the ring rules, asserted where the reference orders a ring --------------------------------------------------------
_orig_order = REF._order_by_angle
GAPS, CUTS = [], []


def _checked_order(positions, *, center, normal):
    order = _orig_order(positions, center=center, normal=normal)
    if len(order):
        # the angles again, as geometry/plane_ops.order_by_angle forms them (no projection first)
        u, v = REF._orthonormal_basis(normal)
        rel_ = positions - center[None, :]
        ang = np.arctan2(rel_ @ v, rel_ @ u)[order]
        cut = float(np.min(np.pi - np.abs(ang)))
        CUTS.append(cut)
        assert cut >= MIN_GAP, "a ring angle within 1e-6 rad of atan2's branch cut: %g" % cut
        if len(order) > 1:
            gaps = np.diff(np.concatenate([ang, [ang[0] + 2.0 * np.pi]]))
            GAPS.append(float(gaps.min()))
            assert gaps.min() >= MIN_GAP, "adjacent ring angles closer than 1e-6 rad: %g" % gaps.min()
    return order


REF._order_by_angle = _checked_order


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(float(np.max(np.abs(np.asarray(b)))), 1e-300))


def rotated_disk(n_rings, **kw):
    P, T, B = meshgen.disk_patch(n_rings, **kw)
    c, s = np.cos(ROT), np.sin(ROT)
    P = np.asarray(P, dtype=float) @ np.array([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]])
    return P, T, B


def permuted_disk(n_rings, perm_seed, **kw):
    """the rotated disk_patch with vertex i renumbered perm[i] -> (P, T, perm)"""
    P, T, _B = rotated_disk(n_rings, **kw)
    perm = np.random.default_rng(perm_seed).permutation(len(P))
    P2 = np.empty_like(P)
    P2[perm] = P
    return P2, perm[np.asarray(T)].astype(np.int32), perm


def pick(rings, n):
    """n rows spread evenly over the pool of the given mesh rings"""
    pool = [r for ring in rings for r in ring_rows(ring)]
    assert 0 <= n <= len(pool), (rings, n, len(pool))
    return [pool[(i * len(pool)) // n] for i in range(n)]


def margins(pos, rim, outer, res):
    """|dr| and r_len of an evaluation as the reference forms them: none may sit next to its threshold"""
    center, normal = REF._resolve_center(res), REF._resolve_normal(res)
    if len(rim) == 0 or len(outer) == 0 or normal is None:
        return
    rim_o = rim[_orig_order(pos[rim], center=center, normal=normal)]
    out_o = outer[_orig_order(pos[outer], center=center, normal=normal)]
    rim_pos, out_pos = pos[rim_o], pos[out_o]
    if len(rim_o) != len(out_o):
        s_rim, total = REF._arc_length_params(rim_pos)
        interp = REF._interp_ring_positions(out_pos, s_rim) if total > 0.0 else None
        if interp is None:
            return
        out_pos = interp[0]

    def radius(p):
        r = p - center[None, :]
        return np.linalg.norm(r - (r @ normal)[:, None] * normal[None, :], axis=1)

    r_len = radius(rim_pos)
    dr = np.abs(radius(out_pos) - r_len)
    assert not np.any((dr >= 0.5e-8) & (dr <= 2e-8)), "|dr| next to its threshold"
    assert not np.any((r_len >= 0.5e-12) & (r_len <= 2e-12)), "r_len next to its threshold"


# the threshold margins, asserted at EVERY evaluation of the reference's module (cases, relaxation, trajectories and their
# trials alike): the module's array entry point is wrapped for the whole run, beneath the counters
_orig_compute = REF.compute_energy_and_gradient_array
N_MARGIN_CHECKS = [0]


@functools.wraps(_orig_compute)  # (the evaluation manager reads the signature to choose the keywords it passes)
def _checked_compute(mesh, global_params, param_resolver, **kw):
    group = REF._resolve_group(param_resolver, "rim_slope_match_group")
    outer_group = REF._resolve_group(param_resolver, "rim_slope_match_outer_group")
    if group is not None and outer_group is not None and REF._resolve_strength(param_resolver) != 0.0:
        margins(np.asarray(kw["positions"]), REF._collect_group_rows(mesh, group),
                REF._collect_group_rows(mesh, outer_group), param_resolver)
        N_MARGIN_CHECKS[0] += 1
    return _orig_compute(mesh, global_params, param_resolver, **kw)


REF.compute_energy_and_gradient_array = _checked_compute


def evaluate(m, pos, tin, tout):
    """array API with and without the shape gradient, the energy-only API: the same energy and tilt gradients"""
    res = ParameterResolver(m.global_parameters)
    kw = dict(positions=pos, index_map=m.vertex_index_to_row)
    g, gi, go = np.zeros_like(pos), np.zeros_like(pos), np.zeros_like(pos)
    E = REF.compute_energy_and_gradient_array(m, m.global_parameters, res, grad_arr=g, tilts_in=tin, tilts_out=tout,
                                              tilt_in_grad_arr=gi, tilt_out_grad_arr=go, **kw)
    gi2, go2 = np.zeros_like(pos), np.zeros_like(pos)
    E2 = REF.compute_energy_and_gradient_array(m, m.global_parameters, res, grad_arr=None, tilts_in=tin, tilts_out=tout,
                                               tilt_in_grad_arr=gi2, tilt_out_grad_arr=go2, **kw)
    assert E2 == E and np.array_equal(gi2, gi) and np.array_equal(go2, go)  # grad_arr=None only skips the shape gradient
    return float(E), g, gi, go


def gen_cases():
    out, names = {}, []
    oblique = [1.0 / 3.0, 2.0 / 3.0, 2.0 / 3.0]
    near_x = (np.array([0.95, 0.1, 0.2]) / np.linalg.norm([0.95, 0.1, 0.2])).tolist()
    G, GO, GD, K = "rim_slope_match_group", "rim_slope_match_outer_group", "rim_slope_match_disk_group", "rim_slope_match_strength"
    base = {G: "rim", GO: "outer", K: 3.0, "rim_slope_match_normal": [0.0, 0.0, 1.0],
            "rim_slope_match_center": [0.03, -0.02, 0.01]}
    withdisk = dict(base, **{GD: "disk"})
    # (name, mesh rings, (rim rings, n), (outer rings, n), (disk rings, n), parameters, special)
    specs = []
    for n in (1, 2, 3, 4):
        specs.append(("n%03d" % n, 4, ([2], n), ([3], n), ([1], 0), base, None))
    for n in (63, 64, 65):
        specs.append(("n%03d" % n, 11, ([11], n), ([9, 10], n), ([8], 0), base, None))
    # (the three sizes about one thread per row on the multi-tile mesh; two of them carry the disk variants as well)
    specs += [
        ("n255", 43, ([43], 255), ([41, 42], 255), ([40], 0), base, None),
        ("n256_disk_local", 43, ([43], 256), ([41, 42], 256), ([39, 40], 256), withdisk, None),
        ("n257_outer_less_disk_mean", 43, ([43], 257), ([42], 252), ([41], 246), withdisk, None),
        ("n065_outer_2x_disk_mean", 22, ([11], 65), ([22], 130), ([10], 60), withdisk, None),
        ("outer_equal", 6, ([3], 18), ([4], 18), ([2], 0), base, None),
        ("outer_2x", 6, ([3], 18), ([6], 36), ([2], 0), base, None),
        ("outer_plus1", 6, ([3], 18), ([4], 19), ([2], 0), base, None),
        ("outer_less", 6, ([3], 18), ([4], 11), ([2], 0), base, None),
        ("outer_two_rows", 6, ([3], 18), ([4], 2), ([2], 0), base, None),
        ("outer_one_row", 6, ([3], 18), ([4], 1), ([2], 0), base, None),
        ("disk_local", 6, ([3], 12), ([4], 12), ([2], 12), withdisk, None),
        ("disk_local_outer_2x", 6, ([3], 12), ([4], 24), ([2], 12), withdisk, None),
        ("disk_mean", 6, ([3], 18), ([4], 18), ([2], 12), withdisk, None),
        ("disk_mean_outer_plus1", 6, ([3], 18), ([4], 19), ([2], 12), withdisk, None),
        ("disk_mean_outer_less", 6, ([3], 18), ([4], 11), ([2], 7), withdisk, None),
        ("disk_equals_rim", 6, ([3], 18), ([4], 18), ([2], 12), dict(base, **{GD: "rim"}), None),
        ("disk_group_empty", 6, ([3], 18), ([4], 18), ([2], 0), withdisk, None),
        ("disk_one_row", 6, ([3], 18), ([4], 18), ([2], 1), withdisk, None),
        ("mode_ring_average", 6, ([3], 18), ([4], 19), ([2], 12), dict(withdisk, rim_slope_match_mode=" Ring_Average_Radial_v1 "), None),
        ("normal_oblique", 6, ([3], 18), ([4], 24), ([2], 12), dict(withdisk, rim_slope_match_normal=oblique), None),
        ("normal_unnormalised", 6, ([3], 18), ([4], 24), ([2], 12), dict(withdisk, rim_slope_match_normal=[0.0, 0.0, 2.5]), None),
        ("normal_near_x", 6, ([3], 18), ([4], 24), ([2], 12), dict(withdisk, rim_slope_match_normal=near_x), None),
        ("normal_oblique_equal", 6, ([3], 18), ([4], 18), ([1, 2], 18), dict(withdisk, rim_slope_match_normal=oblique), None),
        ("center_default", 6, ([3], 18), ([4], 24), ([2], 12), {k: v for k, v in withdisk.items() if k != "rim_slope_match_center"}, None),
        ("invalid_dr_zero", 6, ([3], 18), ([4], 18), ([2], 12), withdisk, "dr_zero_one"),
        ("invalid_row_on_center", 6, ([3], 18), ([4], 24), ([2], 12), withdisk, "on_center"),
        ("all_invalid", 6, ([3], 18), ([4], 18), ([2], 12), withdisk, "dr_zero_all"),
        ("rim_without_length", 6, ([3], 1), ([4], 5), ([2], 0), base, None),
        ("outer_empty", 6, ([3], 18), ([4], 0), ([2], 12), withdisk, None),
        ("rim_empty", 6, ([3], 0), ([4], 18), ([2], 12), withdisk, None),
        ("no_outer_group", 6, ([3], 18), ([4], 18), ([2], 12), {k: v for k, v in withdisk.items() if k != GO}, None),
        ("strength_zero", 6, ([3], 18), ([4], 18), ([2], 12), dict(withdisk, **{K: 0.0}), None),
        ("strength_negative", 6, ([3], 18), ([4], 24), ([2], 12), dict(withdisk, **{K: -0.7}), None),
    ]
    for cname, n_rings, rim_s, out_s, disk_s, gp, special in specs:
        P, T, perm = permuted_disk(n_rings, 2000 + n_rings, bulge=0.2)
        rng = np.random.default_rng(11 + len(names))
        ext = {}
        for key, (rings, n) in (("rim", rim_s), ("outer", out_s), ("disk", disk_s)):
            ext[key] = np.sort(perm[np.asarray(pick(rings, n), dtype=np.int64)])  # vertex_ids order
        pos = P.copy()
        for key, rows in ext.items():
            # every ring perturbed radially, out of plane and -- a fraction of the ring's spacing -- in angle
            n = len(rows)
            if n == 0:
                continue
            # (radially a fraction of the spacing between the mesh's rings: rim and outer radii stay apart, so that
            # phi = dh / dr does not amplify the last bits of dr into the energy)
            xy = pos[rows, :2] * (1.0 + (0.15 / n_rings) * np.clip(rng.normal(size=(n, 1)), -2.0, 2.0))
            dphi = (0.2 * 2.0 * np.pi / max(n, 6)) * rng.uniform(-1.0, 1.0, size=n)
            pos[rows, 0] = xy[:, 0] * np.cos(dphi) - xy[:, 1] * np.sin(dphi)
            pos[rows, 1] = xy[:, 0] * np.sin(dphi) + xy[:, 1] * np.cos(dphi)
            pos[rows, 2] += 0.03 * rng.normal(size=n)
        gp = dict(gp)
        center = np.asarray(gp.get("rim_slope_match_center", [0.0, 0.0, 0.0]), dtype=float)
        normal = np.asarray(gp["rim_slope_match_normal"], dtype=float)
        normal = normal / np.linalg.norm(normal)
        if special in ("dr_zero_one", "dr_zero_all"):
            # an outer row exactly above its rim partner (normal z): r_out == r_rim bit for bit, dr == 0
            ro = ext["rim"][_orig_order(pos[ext["rim"]], center=center, normal=normal)]
            oo = ext["outer"][_orig_order(pos[ext["outer"]], center=center, normal=normal)]
            for q in (range(len(ro)) if special == "dr_zero_all" else [5]):
                pos[oo[q]] = pos[ro[q]] + np.array([0.0, 0.0, 0.07 + 0.01 * q])
            assert np.array_equal(ext["outer"][_orig_order(pos[ext["outer"]], center=center, normal=normal)], oo)
        if special == "on_center":  # one rim row projected onto the center: r_len == 0 exactly
            gp["rim_slope_match_center"] = [float(pos[ext["rim"][0], 0]), float(pos[ext["rim"][0], 1]), 0.4]
        vo = {}
        for key, rows in ext.items():
            for r in rows:
                vo[int(r)] = {"rim_slope_match_group": key}
        free = [int(r) for r in perm[:3] if int(r) not in vo]
        vo[free[0]] = {"rim_slope_match_group": "elsewhere"}  # (another group's row)
        m, _edges = build(pos, T, gp, vopts=vo)
        assert np.array_equal(m.positions_view(), pos)  # (builds the row tables as well)
        tin, tout = np.zeros_like(pos), np.zeros_like(pos)
        for key, rows in ext.items():
            # (rings of 60 rows and more carry tilts only where the module reads them: the fixture stays small)
            if n_rings < 11 or key in ("rim", "disk"):
                tin[rows] = 0.3 * rng.normal(size=(len(rows), 3))
            if n_rings < 11 or key == "rim":
                tout[rows] = 0.25 * rng.normal(size=(len(rows), 3))
        E, g, gi, go = evaluate(m, pos, tin, tout)
        every = np.unique(np.concatenate([ext["rim"], ext["outer"], ext["disk"]])).astype(np.int64)
        rest = np.ones(len(pos), bool)
        rest[every] = False
        assert not g[rest].any() and not gi[rest].any() and not go[rest].any()
        off = cname in ("all_invalid", "rim_without_length", "outer_empty", "rim_empty", "no_outer_group", "strength_zero",
                        "outer_one_row", "n001")  # (n001: one rim row has no arc length, every weight is 0)
        if off:
            assert E == 0.0 and not g.any() and not gi.any() and not go.any(), cname
        else:
            assert E != 0.0 and g.any() and go.any(), cname
            natural = np.array([int(perm[r]) for r in pick(*rim_s)])
            assert len(natural) < 3 or not np.array_equal(natural, ext["rim"]), "the vertex ids are not scrambled"
            has_disk = gp.get(GD) == "disk" and len(ext["disk"]) > 1  # (one disk row: a mean without a weight, no term)
            assert gi.any() == has_disk, cname
        if cname == "normal_near_x":
            assert abs(near_x[0]) > 0.9
        if cname.startswith("n25"):
            assert len(P) > 5000  # (several tiles at the default tile size)
        out.update({cname + "__mesh": jdump({"n_rings": n_rings, "perm_seed": 2000 + n_rings, "bulge": 0.2, "rot": ROT}),
                    cname + "__gp": jdump(gp), cname + "__elsewhere": np.array(free[0], dtype=np.int32),
                    cname + "__rows": every.astype(np.int32), cname + "__positions": pos[every],
                    cname + "__tilts_in": tin[every], cname + "__tilts_out": tout[every], cname + "__E": np.array(E),
                    cname + "__grad": g[every], cname + "__tilt_in_grad": gi[every], cname + "__tilt_out_grad": go[every]})
        for key, rows in ext.items():
            out[cname + "__" + key] = rows.astype(np.int32)
        names.append(cname)
        print("%-28s rim %3d outer %3d disk %3d E=% .16g" % (cname, len(ext["rim"]), len(ext["outer"]), len(ext["disk"]), E))
    out["names"] = np.array(names)
    out["reference_signatures"] = jdump({fn: [p for p in inspect.signature(getattr(REF, fn)).parameters]
                                         for fn in ("compute_energy_and_gradient", "compute_energy_and_gradient_array")})
    out["reference_flags"] = jdump({"USES_TILT_LEAFLETS": bool(REF.USES_TILT_LEAFLETS)})
    save_npz(os.path.join(OUT, "rim_slope_match_cases.npz"), out)
    print("smallest angular gap over the cases: %.3g rad, closest to the branch cut: %.3g rad" % (min(GAPS), min(CUTS)))


# ---------------------------------------------------------------------------------------------------------------------
def gen_relax():
    """One nested CG leaflet relaxation with the module next to tilt_in/out and bending_tilt_in/out: unequal counts
    (rim 18, outer 24) and the mean-disk variant (disk 12)."""
    P, T, B = rotated_disk(6, bulge=0.3, jitter=0.02, seed=11)
    tag = {}
    for key, ring in (("rim", 3), ("outer", 4), ("disk", 2)):
        for r in ring_rows(ring):
            tag[int(r)] = {"rim_slope_match_group": key}
    mods = ["tilt_in", "tilt_out", "bending_tilt_in", "bending_tilt_out", NAME]
    gp = {"tilt_modulus_in": 2.0, "tilt_modulus_out": 1.4, "bending_modulus": 0.6, "spontaneous_curvature": 0.05,
          "rim_slope_match_group": "rim", "rim_slope_match_outer_group": "outer", "rim_slope_match_disk_group": "disk",
          "rim_slope_match_strength": 200.0, "rim_slope_match_normal": [0.0, 0.0, 1.0],
          "rim_slope_match_center": [0.02, -0.01, 0.0], "tilt_solve_mode": "nested", "tilt_solver": "cg",
          "tilt_step_size": 0.05, "tilt_tol": 1e-10}
    out = {}

    def run(cap, noise):
        m, _edges = build(P, T, dict(gp, tilt_inner_steps=int(cap)), vopts=tag, fixed=B)
        tin0, tout0, _fi, _fo = rs.set_fields(m, 33, 0.05)
        pert = noise * np.random.default_rng(77).normal(size=tin0.shape)
        nrm = m.vertex_normals(m.positions_view())
        pert = pert - np.einsum("ij,ij->i", pert, nrm)[:, None] * nrm
        m.set_tilts_in_from_array(tin0 + pert)
        m.set_tilts_out_from_array(tout0 + pert)
        m.energy_modules, m.constraint_modules = list(mods), []
        mz = Minimizer(m, m.global_parameters, GradientDescent(), EnergyModuleManager(mods), ConstraintModuleManager([]),
                       quiet=True)
        mgr = mz._tilt_relaxation_manager
        count = [0, 0]

        def counted(fn, k):
            def wrapper(*a, **kw):
                count[k] += 1
                return fn(*a, **kw)
            return wrapper

        mgr.compute_energy_and_leaflet_tilt_gradients_array_fn = counted(mgr.compute_energy_and_leaflet_tilt_gradients_array_fn, 0)
        mgr.compute_tilt_dependent_energy_with_leaflet_tilts_fn = counted(mgr.compute_tilt_dependent_energy_with_leaflet_tilts_fn, 1)
        mz._relax_leaflet_tilts(positions=m.positions_view(), mode="nested")
        stop = str(mgr.last_leaflet_relaxation_stats.get("stop_reason"))
        return m, mz, tin0, tout0, (count[0], count[1]), stop

    for cap in RELAX_CAPS:
        m, mz, tin0, tout0, counts, stop = run(cap, 0.0)
        E_total = float(mz.compute_energy())
        stable, spread_t, spread_e = True, 0.0, 0.0
        for noise in (1e-13, -1e-13):
            m2, mz2, _a, _b, n2, stop2 = run(cap, noise)
            dev = max(rel(m2.tilts_in_view(), m.tilts_in_view()), rel(m2.tilts_out_view(), m.tilts_out_view()))
            de = abs(float(mz2.compute_energy()) - E_total) / abs(E_total)
            stable = stable and n2 == counts and stop2 == stop and dev < 1e-9
            spread_t, spread_e = max(spread_t, dev), max(spread_e, de)
        if stable:
            break
    assert stable, "the relaxation's stopping point depends on rounding at every tilt_inner_steps tried"
    tin, tout = np.array(m.tilts_in_view(), copy=True), np.array(m.tilts_out_view(), copy=True)
    pos = m.positions_view().copy()
    E_own, _g, _gi, _go = evaluate(m, pos, tin, tout)
    assert E_own != 0.0 and np.max(np.abs(tout - tout0)) > 1e-4
    print("relaxation: tilt_inner_steps %d (%s) gradient evaluations %d energy evaluations %d E_own=%.16g E_total=%.16g "
          "spread tilts %.3g energy %.3g" % (cap, stop, counts[0], counts[1], E_own, E_total, spread_t, spread_e))
    m0, edges = build(P, T, {}, vopts=tag, fixed=B)
    out.update({"gp_json": jdump(dict(gp, tilt_inner_steps=int(cap))), "tilts_in0": tin0, "tilts_out0": tout0,
                "tilts_in_final": tin, "tilts_out_final": tout, "E_own": np.array(E_own), "E_total": np.array(E_total),
                "tilt_inner_steps": np.array(int(cap)), "n_gradient_evaluations": np.array(counts[0]),
                "n_energy_evaluations": np.array(counts[1]), "stop_reason": np.array(stop),
                "noise_tilts": np.array(spread_t), "noise_energy": np.array(spread_e), "positions": np.asarray(P),
                "tri": np.asarray(T, dtype=np.int32), "edges": edges, "fixed": np.asarray(B),
                "vopts": jdump({str(k): v for k, v in tag.items()}), "modules": np.array(mods)})
    save_npz(os.path.join(OUT, "rim_slope_match_relax.npz"), out)


# ---------------------------------------------------------------------------------------------------------------------
class Counter:
    """counts the module's evaluations: with a shape gradient asked for, and without (the line search's)"""

    def __init__(self):
        self.n = [0, 0]

    def __enter__(self):
        self._orig = REF.compute_energy_and_gradient_array
        orig = self._orig

        @functools.wraps(orig)  # (the evaluation manager reads the signature to choose the keywords it passes)
        def wrapped(*a, **kw):
            self.n[0 if kw.get("grad_arr") is not None else 1] += 1
            return orig(*a, **kw)

        REF.compute_energy_and_gradient_array = wrapped
        return self

    def __exit__(self, *exc):
        REF.compute_energy_and_gradient_array = self._orig


class NoGeometryCache:
    """The reference without its per-mesh geometry caches (Mesh._geometry_cache_active)"""

    def __enter__(self):
        from geometry.entities import Mesh

        self._cls, self._orig = Mesh, Mesh._geometry_cache_active
        Mesh._geometry_cache_active = lambda mesh, positions: False
        return self

    def __exit__(self, *exc):
        self._cls._geometry_cache_active = self._orig


def run_once(P, T, gp, vo, mods, cons, stepper_cls, n_steps, step_size, fixed):
    m, edges = build(P, T, gp, vopts=vo, fixed=fixed)
    tin, tout, fin, fout = rs.set_fields(m, 33, 0.3)
    m.energy_modules, m.constraint_modules = list(mods), list(cons)
    stepper = stepper_cls()
    log, ls_evals = [], []
    orig = stepper.step

    def logged(mesh, grad, step_size, energy_fn, constraint_enforcer=None):
        n0 = list(cnt.n)
        r = orig(mesh, grad, step_size, energy_fn, constraint_enforcer=constraint_enforcer)
        log.append((float(bool(r[0])), float(r[1]), float(r[2])))
        ls_evals.append(sum(cnt.n) - sum(n0))  # the module's evaluations inside this line search
        return r

    stepper.step = logged
    with Counter() as cnt:
        mz = Minimizer(m, m.global_parameters, stepper, EnergyModuleManager(m.energy_modules),
                       ConstraintModuleManager(m.constraint_modules), quiet=True, step_size=step_size)
        pos0 = m.positions_view().copy()
        E0, g0 = mz.compute_energy_and_gradient_array()
        cnt.n[:] = [0, 0]
        res = mz.minimize(n_steps)
        counts = tuple(cnt.n)
    pos = m.positions_view().copy()
    tin_f, tout_f = np.ascontiguousarray(m.tilts_in_view()).copy(), np.ascontiguousarray(m.tilts_out_view()).copy()
    mf, _ = build(pos, T, gp, vopts=vo)
    E_own, _g, _gi, _go = evaluate(mf, mf.positions_view().copy(), tin_f, tout_f)  # (builds the row tables as well)
    return {"positions0": pos0, "tri": np.asarray(m.triangle_row_cache()[0], dtype=np.int32), "fixed": m.fixed_mask.copy(),
            "edges": edges, "vopts": jdump({str(k): v for k, v in vo.items()}), "tilt_fixed_in": fin, "tilt_fixed_out": fout,
            "gamma": m.get_facet_parameter_array("surface_tension").copy(), "E0": np.array(E0), "grad0": np.array(g0),
            "tilts_in0": tin, "tilts_out0": tout, "positions_final": pos, "tilts_in_final": tin_f,
            "tilts_out_final": tout_f, "step_log": np.array(log), "E_final": np.array(res["energy"]),
            "n_steps": np.array(n_steps), "step_size0": np.array(step_size), "gp_json": jdump(gp),
            "modules": np.array(list(mods)), "constraint_modules": np.array(list(cons), dtype="U32"),
            "stepper": np.array(stepper_cls.__name__), "eval_counts": np.array(counts),
            "line_search_evals": np.array(ls_evals), "E_own_final": np.array(E_own)}


def run_traj(fname, P, T, gp, vo, mods, cons, stepper_cls, n_steps, step_size, fixed):
    args = (P, T, gp, vo, mods, cons, stepper_cls, n_steps, step_size, fixed)
    out = run_once(*args)
    with NoGeometryCache():  # the fixture must be a function of its inputs: the same run without the reference's caches
        plain = run_once(*args)
    assert np.array_equal(plain["step_log"][:, :2], out["step_log"][:, :2]), fname
    assert np.allclose(plain["step_log"][:, 2], out["step_log"][:, 2], rtol=1e-12, atol=0), \
        (fname, "the reference's geometry caches change this trajectory")
    L = out["step_log"]
    assert (L[:, 0] > 0).sum() >= 3 and float(out["E_own_final"]) != 0.0, L
    again = run_once(np.asarray(P, dtype=float) + 1e-13 * np.random.default_rng(77).normal(size=np.shape(P)), *args[1:])
    A = again["step_log"]
    assert A.shape == L.shape and np.array_equal(A[:, 0], L[:, 0]) and np.allclose(A[:, 1], L[:, 1], rtol=1e-9), fname
    assert np.array_equal(again["eval_counts"], out["eval_counts"]), fname
    assert np.array_equal(again["line_search_evals"], out["line_search_evals"]), fname
    out["noise_energy"] = np.array(max(float(np.max(np.abs(A[:, 2] - L[:, 2]) / np.abs(L[:, 2]))),
                                       abs(float(again["E_final"]) - float(out["E_final"])) / abs(float(out["E_final"]))))
    out["noise_positions"] = np.array(rel(again["positions_final"], out["positions_final"]))
    out["noise_tilts"] = np.array(max(rel(again["tilts_in_final"], out["tilts_in_final"]),
                                      rel(again["tilts_out_final"], out["tilts_out_final"])))
    save_npz(os.path.join(OUT, fname), out)
    print(fname, "E_final=%.16g" % out["E_final"], L[:, :2].tolist(), "evals", out["eval_counts"].tolist(), "per line search",
          out["line_search_evals"].tolist(), "noise E %.3g x %.3g t %.3g" % (out["noise_energy"], out["noise_positions"],
                                                                            out["noise_tilts"]))


def gen_trajectories():
    """Two runs of 5 steps on the jittered, rotated 6-ring disk (rim 18, outer 24: interpolated; disk 12: the mean variant)
    next to tilt_in + tilt_out (run 1: and surface).  1: GD, strength 0.1 (the reference's kozlov_two_holes setting), nested CG
    relaxation.  2: CG, strength 200 (the single-leaflet profile deck's), coupled relaxation, the rim ring pinned to its
    circle -- a stand-in for that deck's fixed circles."""
    quiet = {"mesh_quality_auto_repair_enabled": False, "volume_constraint_mode": "lagrange",
             "volume_projection_during_minimization": False}
    P, T, B = rotated_disk(6, bulge=0.3, jitter=0.02, seed=11)
    tag = {}
    for key, ring in (("rim", 3), ("outer", 4), ("disk", 2)):
        for r in ring_rows(ring):
            tag[int(r)] = {"rim_slope_match_group": key}
    base = dict(quiet, surface_tension=1.0, tilt_modulus_in=20.0, tilt_modulus_out=14.0, rim_slope_match_group="rim",
                rim_slope_match_outer_group="outer", rim_slope_match_disk_group="disk",
                rim_slope_match_normal=[0.0, 0.0, 1.0], rim_slope_match_center=[0.02, -0.01, 0.0])
    mods = ["surface", "tilt_in", "tilt_out", NAME]
    gp1 = dict(base, rim_slope_match_strength=0.1, tilt_solve_mode="nested", tilt_solver="cg", tilt_step_size=0.05,
               tilt_inner_steps=5)
    run_traj("traj_disk6_gd_rsm_weak_unequal.npz", P, T, gp1, tag, mods, [], GradientDescent, 5, 0.5, B)
    pinned = dict(tag)
    for r in ring_rows(3):
        pinned[int(r)] = dict(tag[int(r)], constraints=["pin_to_circle"], pin_to_circle_group="rim",
                              pin_to_circle_mode="slide", pin_to_circle_normal=[0.0, 0.0, 1.0])
    gp2 = dict(base, rim_slope_match_strength=200.0, tilt_modulus_in=2.0, tilt_modulus_out=1.4, bending_modulus=0.6,
               spontaneous_curvature=0.05, tilt_solve_mode="coupled", tilt_solver="gd", tilt_step_size=0.03,
               tilt_coupled_steps=3)
    # (no surface module, as in that deck: every module of the list is tilt-dependent.  The reference's relaxation accepts
    # a tilt step on E_tilt-dependent(trial) <= E_total(x), the device on tilt-dependent energies on both sides: with a
    # tilt-independent module in the list the two differ as soon as a relaxation step backtracks, as it does here)
    run_traj("traj_disk6_cg_rsm_strong_pins.npz", P, T, gp2, pinned, mods[1:], ["pin_to_circle"], ConjugateGradient, 5, 2e-3,
             B)


# ---------------------------------------------------------------------------------------------------------------------
DECK = "kozlov_1disk_3d_tensionless_single_leaflet_profile.yaml"


def plain(d):
    """options / parameters as JSON data (tuples and arrays to lists)"""
    if isinstance(d, dict):
        return {str(k): plain(v) for k, v in d.items()}
    if isinstance(d, (list, tuple, np.ndarray)):
        return [plain(v) for v in d]
    if isinstance(d, (np.floating, np.integer, np.bool_)):
        return d.item()
    return d


def run_deck(make, stepper_cls, n_steps, step_size, perturb=0.0):
    """n_steps of the reference's Minimizer on the deck as it parses it -> the fixture's arrays.  E0 / grad0 come from a
    mesh of their own: an evaluation before minimize() has enforced the pins leaves geometry in the reference's caches."""
    probe = make()
    pz = Minimizer(probe, probe.global_parameters, stepper_cls(), EnergyModuleManager(probe.energy_modules),
                   ConstraintModuleManager(probe.constraint_modules), quiet=True, step_size=step_size)
    E0, g0 = pz.compute_energy_and_gradient_array()
    E0, g0 = float(E0), np.array(g0, copy=True)
    mesh = make()
    if perturb:
        rng = np.random.default_rng(77)
        for vid in mesh.vertex_ids if mesh.vertex_ids is not None else sorted(mesh.vertices):
            v = mesh.vertices[int(vid)]
            v.position = np.asarray(v.position, dtype=float) + perturb * rng.normal(size=3)
        mesh.increment_version()
    stepper = stepper_cls()
    log, ls_evals = [], []
    orig = stepper.step

    def logged(msh, grad, step, energy_fn, constraint_enforcer=None, **kw):
        n0 = sum(cnt.n)
        r = orig(msh, grad, step, energy_fn, constraint_enforcer=constraint_enforcer, **kw)
        log.append((float(bool(r[0])), float(r[1]), float(r[2])))
        ls_evals.append(sum(cnt.n) - n0)
        return r

    stepper.step = logged
    with Counter() as cnt:
        mz = Minimizer(mesh, mesh.global_parameters, stepper, EnergyModuleManager(mesh.energy_modules),
                       ConstraintModuleManager(mesh.constraint_modules), quiet=True, step_size=step_size)
        mesh.build_position_cache()
        rows = mesh.vertex_index_to_row
        order = sorted(mesh.vertices, key=lambda v: rows[v])
        pos0 = mesh.positions_view().copy()
        tin0, tout0 = np.array(mesh.tilts_in_view(), copy=True), np.array(mesh.tilts_out_view(), copy=True)
        tri = np.asarray(mesh.triangle_row_cache()[0], dtype=np.int32)
        edges = np.array([[rows[mesh.edges[e].tail_index], rows[mesh.edges[e].head_index]] for e in sorted(mesh.edges)],
                         dtype=np.int64)
        vo = {str(rows[v]): plain(mesh.vertices[v].options) for v in order if plain(mesh.vertices[v].options)}
        flag = lambda name: np.array([bool(getattr(mesh.vertices[v], name, False)) for v in order])  # noqa: E731
        fixed = mesh.fixed_mask.copy()
        cnt.n[:] = [0, 0]
        res = mz.minimize(n_steps)
        counts = tuple(cnt.n)
    E_own = REF.compute_energy_and_gradient_array(
        mesh, mesh.global_parameters, ParameterResolver(mesh.global_parameters), positions=mesh.positions_view(),
        index_map=mesh.vertex_index_to_row, grad_arr=None, tilts_in=np.array(mesh.tilts_in_view(), copy=True),
        tilts_out=np.array(mesh.tilts_out_view(), copy=True))
    assert float(E_own) != 0.0
    return {"positions0": pos0, "tri": tri, "fixed": fixed, "edges": edges, "vopts": jdump(vo),
            "E_own_final": np.array(float(E_own)), "tilt_fixed_in": flag("tilt_fixed_in"), "tilt_fixed_out": flag("tilt_fixed_out"),
            "gamma": mesh.get_facet_parameter_array("surface_tension").copy(), "E0": np.array(E0), "grad0": g0,
            "tilts_in0": tin0, "tilts_out0": tout0, "positions_final": mesh.positions_view().copy(),
            "tilts_in_final": np.array(mesh.tilts_in_view(), copy=True),
            "tilts_out_final": np.array(mesh.tilts_out_view(), copy=True), "step_log": np.array(log),
            "E_final": np.array(res["energy"]), "n_steps": np.array(n_steps), "step_size0": np.array(step_size),
            "gp_json": jdump(plain(mesh.global_parameters.to_dict())), "modules": np.array(list(mesh.energy_modules)),
            "constraint_modules": np.array(list(mesh.constraint_modules)), "stepper": np.array(stepper_cls.__name__),
            "eval_counts": np.array(counts), "line_search_evals": np.array(ls_evals)}


def gen_deck():
    """The reference's own single-leaflet profile deck (109 vertices; strength 200, the mean-disk variant, fixed circles
    and planes), its module list and pins, 5 GD steps at the deck's step size."""
    deck = os.path.join(rs.args.reference, "meshes", "caveolin", DECK)

    def make():
        mesh = rs.parse_geometry(rs.load_data(deck))
        mesh.global_parameters.update({"mesh_quality_auto_repair_enabled": False})
        # the deck's rings have a vertex on the negative x axis, exactly on atan2's branch cut: the whole mesh is turned
        # about z by ROT (every frame of the deck -- circles, planes, the disk target, this module -- is the z axis through
        # the origin, so nothing else changes)
        c, sn = np.cos(ROT), np.sin(ROT)
        for v in mesh.vertices.values():
            x, y, z = (float(t) for t in v.position)
            v.position = np.array([c * x - sn * y, sn * x + c * y, z])
        mesh.increment_version()
        return mesh

    step = float(make().global_parameters.get("step_size"))
    out = run_deck(make, GradientDescent, 5, step)
    with NoGeometryCache():
        nocache = run_deck(make, GradientDescent, 5, step)
    same = np.array_equal(nocache["step_log"][:, :2], out["step_log"][:, :2]) and \
        np.allclose(nocache["step_log"][:, 2], out["step_log"][:, 2], rtol=1e-12, atol=0)
    print("deck", list(out["modules"]), list(out["constraint_modules"]), "cached == cache-free:", same)
    # the fixture must be a function of its inputs: a module would be dropped only if the two runs differed (they do not)
    assert same, (out["step_log"].tolist(), nocache["step_log"].tolist())
    L = out["step_log"]
    assert (L[:, 0] > 0).sum() >= 3
    again = run_deck(make, GradientDescent, 5, step, perturb=1e-13)
    A = again["step_log"]
    assert A.shape == L.shape and np.array_equal(A[:, 0], L[:, 0]) and np.allclose(A[:, 1], L[:, 1], rtol=1e-9)
    assert np.array_equal(again["eval_counts"], out["eval_counts"])
    assert np.array_equal(again["line_search_evals"], out["line_search_evals"])
    out["noise_energy"] = np.array(max(float(np.max(np.abs(A[:, 2] - L[:, 2]) / np.abs(L[:, 2]))),
                                       abs(float(again["E_final"]) - float(out["E_final"])) / abs(float(out["E_final"]))))
    out["noise_positions"] = np.array(rel(again["positions_final"], out["positions_final"]))
    out["noise_tilts"] = np.array(max(rel(again["tilts_in_final"], out["tilts_in_final"]),
                                      rel(again["tilts_out_final"], out["tilts_out_final"])))
    assert len(out["positions0"]) == 109
    save_npz(os.path.join(OUT, "traj_deck_gd_rsm_profile.npz"), out)
    print("traj_deck_gd_rsm_profile.npz E_final=%.16g" % out["E_final"], L[:, :2].tolist(), "evals",
          out["eval_counts"].tolist(), "per line search", out["line_search_evals"].tolist(),
          "noise E %.3g x %.3g t %.3g" % (out["noise_energy"], out["noise_positions"], out["noise_tilts"]))


if __name__ == "__main__":
    gen_cases()
    gen_relax()
    gen_trajectories()
    gen_deck()
    print("smallest angular gap over everything the reference evaluated: %.3g rad; closest to the branch cut: %.3g rad; "
          "threshold margins checked at %d evaluations" % (min(GAPS), min(CUTS), N_MARGIN_CHECKS[0]))
