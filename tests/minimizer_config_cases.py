"""The cases behind tests/golden/minimizer_config_log.json and what is recorded for each: what Minimizer._device() hands
to the device and the mirror (tests/minimizer_stub.py stands in for both), which refusal it raises, and what
compute_energy_breakdown() makes of a device with distinct energies.  tools/gen_golden_minimizer_config.py writes the
record of one checkout; tests/test_minimizer_config_host.py compares the code under test with the committed one."""

import contextlib
import glob
import hashlib
import json
import os

import numpy as np

from membrane_solver_amd import _lib as L
from membrane_solver_amd import meshgen
from membrane_solver_amd.geometry.mesh import ArrayBody, ArrayMesh
from membrane_solver_amd.runtime import minimizer as mzmod
from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager
from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager
from membrane_solver_amd.runtime.steppers import GradientDescent

from minimizer_stub import RecordingMirror

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STATE = ("_const_energy", "_thetab_update", "_pins_active", "_tbb_active", "_fplane_active", "_perim_active", "_area_con")


def canon(v):
    """JSON form of a logged value: arrays as shape, dtype and a sha256 prefix, floats by repr, the rest verbatim."""
    if isinstance(v, np.ndarray):
        return ["ndarray", list(v.shape), v.dtype.str, hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest()[:16]]
    if isinstance(v, (bool, np.bool_)):
        return bool(v)
    if isinstance(v, (int, np.integer)):
        return int(v)
    if isinstance(v, (float, np.floating)):
        return repr(float(v))
    if v is None or isinstance(v, str):
        return v
    if isinstance(v, bytes):
        return ["bytes", len(v), hashlib.sha256(v).hexdigest()[:16]]
    if isinstance(v, dict):
        return {str(k): canon(x) for k, x in sorted(v.items(), key=lambda kv: str(kv[0]))}
    if isinstance(v, (list, tuple)):
        return [canon(x) for x in v]
    if hasattr(v, "_asdict"):
        return canon(v._asdict())
    if hasattr(v, "to_dict") or not hasattr(v, "__dict__"):
        return "<" + type(v).__name__ + ">"  # (the parameters object itself: the case's input)
    return canon({k: x for k, x in vars(v).items() if not k.startswith("_")})


def _edge_table(T):
    a = np.concatenate([T[:, 0], T[:, 1], T[:, 2]])
    b = np.concatenate([T[:, 1], T[:, 2], T[:, 0]])
    return np.unique(np.stack([np.minimum(a, b), np.maximum(a, b)], axis=1), axis=0).astype(np.int64)


def _ring(r):
    start = 1 + 3 * r * (r - 1)
    return list(range(start, start + 6 * r))


def _opts(text):
    return {int(k): v for k, v in json.loads(str(text)).items()}


def minimizer(mesh, mods, cons=(), **kw):
    mods, cons = list(mods), list(cons)
    return mzmod.Minimizer(mesh, mesh.global_parameters, GradientDescent(), EnergyModuleManager(mods),
                           ConstraintModuleManager(cons), energy_modules=mods, constraint_modules=cons, quiet=True, **kw)


# -- the trajectory fixtures -------------------------------------------------------------------------------------------
def traj_files():
    out = []
    for path in sorted(glob.glob(os.path.join(GOLD, "traj_*.npz"))):
        with np.load(path) as z:
            if "gp_json" in z.files and "modules" in z.files:
                out.append(os.path.basename(path))
    return out


def traj_minimizer(fname):
    g = np.load(os.path.join(GOLD, fname))
    have = set(g.files)
    mods = [str(m) for m in g["modules"]]
    cons = [str(m) for m in g["constraint_modules"]] if "constraint_modules" in have else []
    kw = {}
    if "vopts" in have:
        kw["vertex_options"] = _opts(g["vopts"])
    if "eopts" in have:
        kw["edge_options"] = _opts(g["eopts"])
    if "edges" in have:
        kw["edges"] = g["edges"]
    if "disk_rows" in have:
        kw["disk_rows_in"] = kw["disk_rows_out"] = g["disk_rows"]
    if "tilts0" in have:
        kw["tilts"], kw["tilt_fixed"] = g["tilts0"], g["tilt_fixed"]
    mesh = ArrayMesh(g["positions0"], g["tri"], fixed=g["fixed"], surface_tension=g["gamma"], tilts_in=g["tilts_in0"],
                     tilts_out=g["tilts_out0"], tilt_fixed_in=g["tilt_fixed_in"], tilt_fixed_out=g["tilt_fixed_out"],
                     global_parameters=json.loads(str(g["gp_json"])), energy_modules=mods, constraint_modules=cons, **kw)
    return minimizer(mesh, mods, cons)


def traj_changes(mz):
    """One parameter inside the key of every keyed table the deck uses, and parameters outside all of them."""
    gp, names = mz.global_params, set(mz.energy_module_names) | set(mz.constraint_module_names)
    num = lambda key, default: float(gp.get(key) or default) * 1.5  # noqa: E731
    out = [("outside_every_key", {"volume_tolerance": 0.0625})]
    for lf in ("in", "out"):
        if "tilt_disk_target_" + lf in names:
            out.append(("disk_target_" + lf, {"tilt_disk_target_strength_" + lf: num("tilt_disk_target_strength_" + lf, 1.0)}))
        if "bending_tilt_" + lf in names:
            out.append(("bending_" + lf, {"bending_modulus_" + lf: num("bending_modulus_" + lf, 2.0)}))
    if names & {"tilt_rim_source_in", "tilt_rim_source_out", "tilt_rim_source_bilayer"}:
        out.append(("rim_source_center", {"tilt_rim_source_center": [0.0, 0.0, 0.25]}))
    if names & {"tilt_thetaB_contact_in", "tilt_thetaB_boundary_in"}:
        out.append(("thetab_value", {"tilt_thetaB_value": num("tilt_thetaB_value", 0.25)}))  # (outside: sent every time)
        out.append(("thetab_center", {"tilt_thetaB_center": [0.0, 0.0, 0.125]}))
    if "rim_slope_match_out" in names:
        out.append(("rim_match_center", {"rim_slope_match_center": [0.0, 0.0, 0.125]}))
    if "tilt_coupling" in names:
        out.append(("coupling", {"tilt_coupling_modulus": num("tilt_coupling_modulus", 1.0)}))
    if "tilt_splay_twist_in" in names:
        out.append(("splay_twist", {"tilt_twist_modulus_in": num("tilt_twist_modulus_in", 0.5)}))
    if mz._pin_names:
        out.append(("pins_fixed_mask", "flip_fixed"))
    out.append(("tilt_modulus", {"tilt_modulus_in": num("tilt_modulus_in", 1.0)}))  # (a leaflet parameter, no table's key)
    return out


# -- hand-built cases --------------------------------------------------------------------------------------------------
P3, T3, B3 = meshgen.disk_patch(3)
E3 = _edge_table(T3)
ICO_P, ICO_T = meshgen.icosphere(1)
RIM3 = [int(r) for r in np.flatnonzero(B3)]


def _disk(gp, mods, cons=(), **kw):
    mesh = ArrayMesh(P3, T3, global_parameters=dict(gp), energy_modules=list(mods), constraint_modules=list(cons), **kw)
    return minimizer(mesh, mods, cons)


def _ico(gp, mods, cons=(), **kw):
    mesh = ArrayMesh(ICO_P, ICO_T, global_parameters=dict(gp), energy_modules=list(mods), constraint_modules=list(cons), **kw)
    return minimizer(mesh, mods, cons)


def _body(**kw):
    return [ArrayBody(**kw)]


HEAD = {"surface_tension": 1.0, "bending_modulus": 1.0}
LEAF = {"tilt_modulus_in": 1.0, "tilt_modulus_out": 1.5}
THETAB = {"tilt_thetaB_group_in": "ring", "tilt_thetaB_strength_in": 3.0, "tilt_thetaB_contact_strength_in": 0.7,
          "tilt_thetaB_value": 0.11, "tilt_thetaB_normal": [0.0, 0.0, 2.0]}
RING_VO = {r: {"tilt_thetaB_group": "ring"} for r in _ring(2)}
RSM = {"rim_slope_match_group": "rim", "rim_slope_match_outer_group": "outer", "rim_slope_match_disk_group": "disk",
       "rim_slope_match_strength": 2.0, "rim_slope_match_normal": [0.0, 0.0, 1.0]}
RSM_VO = {r: {"rim_slope_match_group": key} for key, ring in (("disk", 1), ("rim", 2), ("outer", 3)) for r in _ring(ring)}
BILAYER = {"tilt_rim_source_group": "rim", "tilt_rim_source_strength": 2.0}
RIM_VO = {r: {"pin_to_circle_group": "rim"} for r in RIM3}
FIT_VO = {r: {"pin_to_circle_group": "rim", "pin_to_circle_mode": "fit", "pin_to_circle_normal": [0.0, 0.0, 1.0]} for r in RIM3}
PLANE_VO = {r: {"constraints": ["pin_to_plane"], "pin_to_plane_normal": [0.0, 0.0, 1.0], "pin_to_plane_point": [0.0, 0.0, 0.0]}
            for r in RIM3}
SPLAY = {"tilt_splay_modulus_in": 0.7, "tilt_twist_modulus_in": 0.4}
OUT_FIRST = {"tilt_disk_target_group_in": "disk", "tilt_disk_target_group_out": "disk", "tilt_disk_target_strength_in": 2.0,
             "tilt_disk_target_strength_out": 3.0, "tilt_disk_target_theta_B": 0.2, "tilt_disk_target_normal": [0.0, 0.0, 1.0],
             "tilt_rim_source_group_in": "rim", "tilt_rim_source_group_out": "rim", "tilt_rim_source_strength_in": 1.5,
             "tilt_rim_source_strength_out": 2.5}
PERIM = {"perimeter_constraints": [{"edges": [1, 2, 3], "target_perimeter": 1.0}]}
ABSENT_VO = {r: {"preset": "rim"} for r in RIM3}

# name -> (builder, [(label, change)]): a change is a dict for global_params.update or "flip_fixed"
HAND = {
    "headline_lagrange": (lambda: _ico(HEAD, ["surface", "bending", "volume"], ["volume"], bodies=_body(target_volume=4.0)),
                          [("volume_stiffness", {"volume_stiffness": 10.0}), ("outside", {"volume_tolerance": 0.0625})]),
    "headline_no_projection": (lambda: _ico(dict(HEAD, volume_projection_during_minimization=False),
                                            ["surface", "bending", "volume"], ["volume"], bodies=_body(target_volume=4.0)), []),
    "volume_penalty": (lambda: _ico(dict(HEAD, volume_constraint_mode="penalty", volume_stiffness=50.0),
                                    ["surface", "volume"], bodies=_body(target_volume=4.0)),
                       [("volume_stiffness", {"volume_stiffness": 75.0})]),
    "bending_approx": (lambda: _ico(dict(HEAD, bending_gradient_mode="approx", bending_energy_model="willmore"),
                                    ["surface", "bending"]), [("mode", {"bending_gradient_mode": "analytic"})]),
    "bending_analytic_open": (lambda: _disk(dict(HEAD, bending_energy_model="helfrich", spontaneous_curvature=0.1),
                                            ["bending", "surface"]), [("model", {"bending_energy_model": "willmore"})]),
    "body_area_penalty": (lambda: _ico(dict(HEAD, area_stiffness=5.0), ["surface", "body_area_penalty"],
                                       bodies=_body(options={"area_target": 12.0})),
                          [("area_stiffness", {"area_stiffness": 7.0}), ("outside", {"volume_tolerance": 0.0625})]),
    "line_tension": (lambda: _disk(dict(HEAD, line_tension=1.5), ["surface", "line_tension"], edges=E3,
                                   edge_options={0: {"energy": "line_tension"}, 4: {"energy": ["line_tension"]}}),
                     [("line_tension", {"line_tension": 2.5}), ("outside", {"volume_tolerance": 0.0625})]),
    "line_tension_untagged": (lambda: _disk(HEAD, ["surface", "line_tension"], edges=E3, edge_options={}), []),
    "edge_length_penalty": (lambda: _disk(dict(HEAD, edge_stiffness=20.0), ["surface", "bending", "edge_length_penalty"],
                                          edges=E3, edge_options={0: {"target_length": 0.5}, 3: {"target_length": 0.25}}),
                            [("edge_stiffness", {"edge_stiffness": 30.0}), ("outside", {"volume_tolerance": 0.0625})]),
    "edge_modules_together": (lambda: _disk(dict(HEAD, line_tension=1.0), ["surface", "line_tension", "edge_length_penalty"],
                                            edges=E3, edge_options={0: {"target_length": 0.5, "energy": ["line_tension"]}}), []),
    "tilt_single": (lambda: _disk(dict(HEAD, tilt_rigidity=1.0, tilt_smoothness_rigidity=0.5),
                                  ["surface", "tilt", "tilt_smoothness"], tilts=np.zeros_like(P3)),
                    [("smoothness", {"tilt_smoothness_rigidity": 0.75}), ("switched_off", {"tilt_rigidity": 0.0})]),
    "bending_tilt_single": (lambda: _disk(dict(HEAD, tilt_rigidity=1.0), ["tilt", "bending_tilt"], tilts=np.zeros_like(P3)), []),
    "gaussian_curvature": (lambda: _ico(dict(HEAD, gaussian_modulus=0.5), ["surface", "gaussian_curvature"]),
                           [("gaussian_modulus", {"gaussian_modulus": 0.75})]),
    "rim_match_strength_zero": (lambda: _disk(dict(LEAF, **dict(RSM, rim_slope_match_strength=0.0)),
                                              ["tilt_in", "tilt_out", "rim_slope_match_out"], vertex_options=RSM_VO),
                                [("strength_on", {"rim_slope_match_strength": 2.0}), ("center", {"rim_slope_match_center": [0.0, 0.0, 0.5]}),
                                 ("strength_off", {"rim_slope_match_strength": 0.0})]),
    "rim_match_no_rings": (lambda: _disk(dict(LEAF, **RSM), ["tilt_in", "tilt_out", "rim_slope_match_out"]), []),
    "body_area": (lambda: _ico(HEAD, ["surface", "bending"], ["body_area"], bodies=_body(options={"target_area": 12.0})), []),
    "volume_body_area": (lambda: _ico(HEAD, ["surface"], ["volume", "body_area"],
                                      bodies=_body(target_volume=4.0, options={"target_area": 12.0})), []),
    "body_area_no_target": (lambda: _ico(HEAD, ["surface"], ["body_area"], bodies=_body()), []),
    "global_area": (lambda: _ico(dict(HEAD, target_surface_area=11.5), ["surface", "bending"], ["global_area"]),
                    [("target", {"target_surface_area": 11.0})]),
    "fixed_plane": (lambda: _disk(dict(HEAD, fixed_plane_normal=[0.0, 0.0, 2.0], fixed_plane_point=[0.0, 0.0, 0.25]),
                                  ["surface"], ["fixed_plane"]),
                    [("point", {"fixed_plane_point": [0.0, 0.0, 0.5]}), ("outside", {"volume_tolerance": 0.0625})]),
    "fixed_plane_tilt_pins": (lambda: _disk(dict(HEAD, **LEAF), ["surface", "tilt_in"], ["fixed_plane", "pin_to_plane"],
                                            vertex_options=PLANE_VO), [("pins_fixed_mask", "flip_fixed")]),
    "perimeter": (lambda: _disk(dict(HEAD, **PERIM), ["surface"], ["perimeter"], edges=E3),
                  [("target", {"perimeter_constraints": [{"edges": [1, 2, 3], "target_perimeter": 1.25}]}),
                   ("outside", {"volume_tolerance": 0.0625})]),
    "perimeter_body_area": (lambda: _disk(dict(HEAD, **PERIM), ["surface"], ["perimeter", "body_area"], edges=E3,
                                          bodies=_body(facet_rows=np.arange(len(T3) - 6, len(T3)), options={"target_area": 3.0})), []),
    "pins_volume": (lambda: _disk(HEAD, ["surface"], ["pin_to_plane", "volume"], vertex_options=PLANE_VO,
                                  bodies=_body(target_volume=0.5)), [("pins_fixed_mask", "flip_fixed")]),
    "leaflet_absent": (lambda: _disk(dict(LEAF, leaflet_out_absent_presets=["rim"], leaflet_out_absence_mode="triangles",
                                          bending_modulus_out=0.5),
                                     ["tilt_in", "tilt_out", "tilt_smoothness_out"], vertex_options=ABSENT_VO),
                       [("absence_mode", {"leaflet_out_absence_mode": "facets"}), ("outside", {"volume_tolerance": 0.0625}),
                        ("presets_off", {"leaflet_out_absent_presets": []})]),
    "splay_twist": (lambda: _disk(dict(LEAF, **SPLAY), ["tilt_in", "tilt_splay_twist_in"]),
                    [("twist", {"tilt_twist_modulus_in": 0.9}), ("outside", {"volume_tolerance": 0.0625})]),
    # the two leaflets' tables go up in the order the modules are listed
    "leaflets_out_before_in": (lambda: _disk(dict(LEAF, **OUT_FIRST), ["tilt_in", "tilt_out", "tilt_disk_target_out",
                                                                     "tilt_disk_target_in", "tilt_rim_source_out",
                                                                     "tilt_rim_source_in"], edges=E3, vertex_options=RIM_VO,
                                             disk_rows_in=np.arange(7), disk_rows_out=np.arange(7)), []),
    "deterministic": (lambda: minimizer(ArrayMesh(ICO_P, ICO_T, global_parameters=dict(HEAD)), ["surface"], deterministic=True), []),
}


# one per raise of _device(), _rim_match_params, _thetab_boundary_params, _upload_pins, _upload_enforce_only, with that
# violation alone -> (builder, True where the refusal reads nothing from the device)
def _open_approx(mods, **kw):
    return _disk(dict(HEAD, bending_gradient_mode="approx", tilt_rigidity=1.0), mods, tilts=np.zeros_like(P3), **kw)


ERRORS = {
    "bilayer_single_field": (lambda: _disk(dict(BILAYER, tilt_rigidity=1.0), ["tilt", "tilt_rim_source_bilayer"], edges=E3,
                                           vertex_options=RIM_VO), True),
    "bilayer_follow_pins": (lambda: _disk(dict(LEAF, **BILAYER), ["tilt_in", "tilt_rim_source_bilayer"], ["pin_to_circle"],
                                          edges=E3, vertex_options=FIT_VO), True),
    "bilayer_not_finite": (lambda: _disk(dict(LEAF, **dict(BILAYER, tilt_rim_source_strength=float("nan"))),
                                         ["tilt_in", "tilt_rim_source_bilayer"], edges=E3, vertex_options=RIM_VO), True),
    "thetab_contact_single_field": (lambda: _disk(dict(THETAB, tilt_rigidity=1.0), ["tilt", "tilt_thetaB_contact_in"],
                                                  vertex_options=RING_VO), True),
    "bending_and_bending_tilt": (lambda: _disk(dict(HEAD, tilt_rigidity=1.0), ["bending", "tilt", "bending_tilt"]), True),
    "approx_bending_tilt_not_last": (lambda: _open_approx(["tilt", "bending_tilt", "surface"]), True),
    "approx_line_tension_open": (lambda: _disk(dict(HEAD, bending_gradient_mode="approx", line_tension=1.0),
                                               ["line_tension", "bending"], edges=E3,
                                               edge_options={0: {"energy": "line_tension"}}), False),
    "approx_edge_penalty_open": (lambda: _disk(dict(HEAD, bending_gradient_mode="approx"), ["edge_length_penalty", "bending"],
                                               edges=E3, edge_options={0: {"target_length": 0.5}}), False),
    "approx_bending_not_last": (lambda: _disk(dict(HEAD, bending_gradient_mode="approx"), ["bending", "surface"]), True),
    "splay_single_field": (lambda: _disk(dict(SPLAY, tilt_rigidity=1.0), ["tilt", "tilt_splay_twist_in"]), True),
    "splay_pins": (lambda: _disk(dict(LEAF, **SPLAY), ["tilt_in", "tilt_splay_twist_in"], ["pin_to_plane"]), True),
    "splay_fixed_plane": (lambda: _disk(dict(LEAF, **SPLAY), ["tilt_in", "tilt_splay_twist_in"], ["fixed_plane"]), True),
    "splay_volume": (lambda: _disk(dict(LEAF, **SPLAY), ["tilt_in", "tilt_splay_twist_in"], ["volume"]), True),
    "single_and_leaflet": (lambda: _disk(dict(LEAF, tilt_rigidity=1.0), ["tilt", "tilt_in"]), True),
    "leaflet_reduced_energy": (lambda: _disk(dict(LEAF, line_search_reduced_energy=True), ["tilt_in"]), True),
    "bending_tilt_out_absent": (lambda: _disk(dict(LEAF, bending_modulus=1.0, leaflet_out_absent_presets=["rim"],
                                                   leaflet_out_absence_mode="triangles"),
                                              ["tilt_in", "bending_tilt_out"], vertex_options=ABSENT_VO), True),
    "absence_topology_strict": (lambda: _disk(dict(LEAF, leaflet_out_absent_presets=["rim"]), ["tilt_in", "tilt_out"],
                                              vertex_options=ABSENT_VO), True),
    "bending_next_to_bending_tilt_in": (lambda: _disk(dict(LEAF, **HEAD), ["bending", "bending_tilt_in"]), True),
    "single_reduced_energy": (lambda: _disk({"tilt_rigidity": 1.0, "line_search_reduced_energy": True}, ["tilt"]), True),
    "single_transport_model": (lambda: _disk({"tilt_rigidity": 1.0, "tilt_transport_model": "connection_v1"}, ["tilt"]), True),
    "fixed_plane_bilayer_follow": (lambda: _disk(dict(LEAF, **BILAYER), ["tilt_in", "tilt_rim_source_bilayer"], ["fixed_plane"],
                                                 edges=E3, vertex_options=FIT_VO), True),
    "rim_match_no_outer_module": (lambda: _disk(dict(LEAF, **RSM), ["tilt_in", "rim_slope_match_out"], vertex_options=RSM_VO), True),
    "rim_match_single_field": (lambda: _disk(dict(LEAF, tilt_rigidity=1.0, **RSM), ["tilt", "tilt_out", "rim_slope_match_out"],
                                             vertex_options=RSM_VO), True),
    "rim_match_disk_no_inner_module": (lambda: _disk(dict(LEAF, **RSM), ["tilt_out", "rim_slope_match_out"],
                                                     vertex_options=RSM_VO), True),
    "tbb_single_field": (lambda: _disk(dict(THETAB, tilt_rigidity=1.0), ["tilt"], ["tilt_thetaB_boundary_in"],
                                       vertex_options=RING_VO), True),
    "tbb_no_inner_module": (lambda: _disk(dict(LEAF, **THETAB), ["tilt_out"], ["tilt_thetaB_boundary_in"],
                                          vertex_options=RING_VO), True),
    "tbb_volume": (lambda: _disk(dict(LEAF, **THETAB), ["tilt_in"], ["volume", "tilt_thetaB_boundary_in"],
                                 vertex_options=RING_VO), True),
    "tbb_pins_pin_nothing": (lambda: _disk(dict(LEAF, **THETAB), ["tilt_in"], ["pin_to_plane", "tilt_thetaB_boundary_in"],
                                           vertex_options=RING_VO), True),
    "tbb_pins_drift_check": (lambda: _disk(dict(LEAF, volume_projection_during_minimization=False, **THETAB), ["tilt_in"],
                                           ["pin_to_plane", "tilt_thetaB_boundary_in"], vertex_options={**RING_VO, **PLANE_VO},
                                           bodies=_body(target_volume=0.5)), True),
    "pins_tilt_volume": (lambda: _disk(LEAF, ["tilt_in"], ["pin_to_plane", "volume"], vertex_options=PLANE_VO), False),
    "perimeter_on_body_area_facets": (lambda: _disk(dict(HEAD, **PERIM), ["surface"], ["perimeter", "body_area"], edges=E3,
                                                    bodies=_body(facet_rows=np.arange(6), options={"target_area": 3.0})), False),
}


# -- recording ---------------------------------------------------------------------------------------------------------
def _take(mir):
    log = [[name, canon(a), canon(k)] for name, a, k in mir.calls]
    del mir.calls[:]
    return log


@contextlib.contextmanager
def _stubbed(build):
    """-> (minimizer, mirror) with ``minimizer.mirror_for`` handing out one recording mirror"""
    mir = RecordingMirror()
    saved = mzmod.mirror_for
    mzmod.mirror_for = lambda mesh, **_kw: (setattr(mir, "mesh", mesh), mir)[1]
    try:
        yield build(), mir
    finally:
        mzmod.mirror_for = saved


def record_config(build, changes):
    """The call log of the first _device(), of an unchanged second call and of a call after every change, with the
    Minimizer's own state after each; ``changes`` may be a function of the minimizer."""
    with _stubbed(build) as (mz, mir):
        out = {"modules": mz.energy_module_names, "constraints": mz.constraint_module_names, "calls": []}
        steps = [("first", None), ("second", None)] + list(changes(mz) if callable(changes) else changes)
        for label, change in steps:
            if change == "flip_fixed":
                mz.mesh._fixed[0] = not mz.mesh._fixed[0]
            elif change:
                mz.global_params.update(change)
            mz._device()
            out["calls"].append({"after": label, "log": _take(mir), "modules_set": int(mir.dm.modules),
                                 "state": {k: canon(getattr(mz, k, None)) for k in STATE}})
        return out


def record_error(build):
    with _stubbed(build) as (mz, mir):
        try:
            mz._device()
        except Exception as exc:  # noqa: BLE001 (the type is what is recorded)
            return {"type": type(exc).__name__, "message": str(exc), "log": _take(mir)}
        return {"type": None, "message": None, "log": _take(mir)}


class FakeEnergies:
    """What compute_energy_breakdown reads of a DeviceMesh, every value distinct and none a sum of the others."""

    GETTERS = {"area_penalty_energy": 0.3125, "line_energy": 0.4375, "edge_penalty_energy": 0.5625,
               "tilt_coupling_energy": 0.0703125, "rim_source_bilayer_energy": -0.1015625, "thetab_contact_energy": -0.1328125,
               "tilt_splay_twist_energy": 0.0546875, "rim_match_energies": (0.19921875, 0.0859375, 0.11328125)}

    def __init__(self, modules):
        self.modules = modules

    def energy(self):
        return np.array([7.1, 5.3, 3.7, 2.9])

    def fetch_scalars(self):
        return 0.01 + 0.37 * np.arange(1, L.MS_NSCAL + 1) ** 1.5

    def leaflet_rim_source_energy(self, leaflet):
        return {"in": 0.0234375, "out": 0.0390625}[leaflet]

    def __getattr__(self, name):
        if name in self.GETTERS:
            return lambda: self.GETTERS[name]
        raise AttributeError(name)


def record_breakdown(build):
    """compute_energy_breakdown over FakeEnergies with the module mask the configuration set, and with every listed
    module's bit on."""
    with _stubbed(build) as (mz, mir):
        mz._device()
        every = 0
        for n in mz.energy_module_names:
            every |= mzmod._ENERGY_BITS[n]
        out = {}
        for label, mask in (("as_configured", int(mir.dm.modules)), ("every_bit_on", every)):
            dev = FakeEnergies(mask)
            mz._device = lambda dev=dev: (None, dev)
            out[label] = {k: repr(float(v)) for k, v in mz.compute_energy_breakdown().items()}
        return out


def shares_an_entry(mz):
    """Two or more listed modules share an energies[] entry, or a ride-along term is listed."""
    slots = [mzmod._ENERGY_SLOT[n] for n in mz.energy_module_names]
    riders = {"tilt_rim_source_in", "tilt_rim_source_out", "tilt_coupling", "tilt_splay_twist_in", "tilt_rim_source_bilayer",
              "tilt_thetaB_contact_in", "rim_slope_match_out"}
    return any(s is not None and slots.count(s) > 1 for s in slots) or bool(riders & set(mz.energy_module_names))


def _rsm_disk6():
    P, T, _B = meshgen.disk_patch(6)
    vo = {r: {"rim_slope_match_group": key} for key, ring in (("disk", 2), ("rim", 3), ("outer", 4)) for r in _ring(ring)}
    mods = ["surface", "tilt_in", "tilt_out", "tilt_smoothness_in", "rim_slope_match_out"]
    return minimizer(ArrayMesh(P, T, global_parameters=dict(LEAF, bending_modulus_in=0.5, **RSM), vertex_options=vo,
                               energy_modules=mods), mods)


BREAKDOWN_EXTRA = {"rim_match_disk_ring": _rsm_disk6,
                   "rim_match_lone_sharer": lambda: _disk(dict(LEAF, **RSM), ["tilt_in", "tilt_out", "rim_slope_match_out"],
                                                          vertex_options=RSM_VO)}


def record_all():
    cfg, brk = {}, {}
    for fname in traj_files():
        cfg[fname] = record_config(lambda: traj_minimizer(fname), traj_changes)
        brk[fname] = record_breakdown(lambda: traj_minimizer(fname))
    for name, (build, changes) in HAND.items():
        cfg[name] = record_config(build, changes)
        if shares_an_entry(build()):
            brk[name] = record_breakdown(build)
    for name, build in BREAKDOWN_EXTRA.items():
        brk[name] = record_breakdown(build)
    errors = {name: dict(record_error(build), device_free=free) for name, (build, free) in ERRORS.items()}
    return {"config": cfg, "errors": errors, "breakdown": brk}
