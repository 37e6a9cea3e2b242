"""Shared pieces of the two-leaflet tilt plugins (tilt_in, tilt_out, tilt_smoothness_in, tilt_smoothness_out).

Parameter resolution follows the reference's helpers (modules/energy/tilt_params.py:6-23,
modules/energy/tilt_smoothness_utils.py:95-100, runtime/preconditioners.py:111-120); the toggles the
device path does not implement raise ``MembraneHipError`` instead of being ignored.
"""

from __future__ import annotations

import numpy as np

from ... import _lib as L
from ...geometry.mesh import mirror_for

LEAFLET_BITS = {("tilt", "in"): L.MS_MOD_TILT_IN, ("tilt", "out"): L.MS_MOD_TILT_OUT,
                ("smooth", "in"): L.MS_MOD_TILT_SMOOTH_IN, ("smooth", "out"): L.MS_MOD_TILT_SMOOTH_OUT,
                ("bt", "in"): L.MS_MOD_BENDING_TILT_IN, ("bt", "out"): L.MS_MOD_BENDING_TILT_OUT,
                ("disk", "in"): L.MS_MOD_TILT_DISK_TARGET_IN, ("disk", "out"): L.MS_MOD_TILT_DISK_TARGET_OUT,
                ("rim", "in"): L.MS_MOD_TILT_RIM_SOURCE_IN, ("rim", "out"): L.MS_MOD_TILT_RIM_SOURCE_OUT}

# options of the reference's leaflet modules that change their result and are not on the device path
_UNSUPPORTED_KEYS = (
    "leaflet_out_absent_presets", "leaflet_in_absent_presets",  # leaflet_presence.py
    "tilt_in_exclude_shared_rim_outer_rows", "tilt_out_exclude_shared_rim_outer_rows",
    "tilt_exclude_shared_rim_outer_rows_in", "tilt_exclude_shared_rim_outer_rows_out",
    "tilt_out_exclude_shared_rim_rows", "tilt_exclude_shared_rim_rows_out",
    "tilt_in_shared_rim_outer_shell_mass_mode", "tilt_out_shared_rim_outer_shell_mass_mode",
    "tilt_axisymmetric_about_thetaB_center", "inner_coupled_update_mode", "tilt_relax_energy_guard_factor",
    "tilt_thetaB_optimize",
    # bending_tilt_leaflet.py toggles (bt_params.py:13-222, bt_selection.py, bt_divergence.py)
    "theory_parity_lane", "bending_tilt_assume_J0_presets", "bending_tilt_assume_J0_presets_in",
    "bending_tilt_assume_J0_presets_out", "bending_tilt_base_term_reference_mode",
    "bending_tilt_base_term_reference_mode_in", "bending_tilt_base_term_reference_mode_out",
    "bending_tilt_base_term_boundary_group_in", "bending_tilt_base_term_boundary_group_out",
    "bending_tilt_base_term_region_mode", "bending_tilt_in_update_mode",
    "bending_tilt_in_scaffold_shape_stencil_mode", "bending_tilt_interface_divergence_mode",
    "bending_tilt_out_interface_divergence_mode",
)


def _get(param_resolver, global_params, key):
    val = param_resolver.get(None, key) if param_resolver is not None else None
    if val is None and global_params is not None:
        val = global_params.get(key)
    return val


def normalize_preset_list(raw) -> list:
    """_normalize_preset_list (leaflet_presence.py:16-31): a string is one preset, a list / tuple / set its stripped,
    non-empty items, anything else nothing."""
    if raw is None:
        return []
    if isinstance(raw, str):
        val = raw.strip()
        return [val] if val else []
    if isinstance(raw, (list, tuple, set)):
        return [s for s in (str(item).strip() for item in raw if item is not None) if s]
    return []


def vertex_options_by_row(mesh) -> dict:
    """{row: options} of the rows that carry options: vertex options of a reference Mesh, or ``vertex_options`` of an
    array mesh (as tilt_thetaB_boundary_in.group_rows reads them)."""
    verts = getattr(mesh, "vertices", None)
    row_of = mesh.vertex_index_to_row
    out = {}
    if isinstance(verts, dict):
        for vid in mesh.vertex_ids:
            opts = getattr(verts[int(vid)], "options", None) or {}
            row = row_of.get(int(vid))
            if row is not None and opts:
                out[int(row)] = opts
    else:
        nv = len(mesh.vertex_ids)
        for row, opts in (getattr(mesh, "vertex_options", None) or {}).items():  # (keyed by row)
            if opts and 0 <= int(row) < nv:
                out[int(row)] = opts
    return out


def absent_mask(mesh, global_params, leaflet: str) -> np.ndarray:
    """leaflet_absent_vertex_mask (leaflet_presence.py:34-122): (nv,) bool, True where the row's vertex option
    ``preset`` is in ``leaflet_<leaflet>_absent_presets``.  (The rows the reference restores for
    ``rim_slope_match_mode: physical_edge_staggered_v1`` are not: check_supported refuses that mode next to a mask.)"""
    nv = len(mesh.vertex_ids)
    mask = np.zeros(nv, dtype=bool)
    lf = str(leaflet or "").strip().lower()
    if lf not in {"in", "out"} or global_params is None:
        return mask
    presets = set(normalize_preset_list(global_params.get(f"leaflet_{lf}_absent_presets")))
    if not presets:
        return mask
    for row, opts in vertex_options_by_row(mesh).items():
        preset = opts.get("preset")
        try:
            if preset in presets:
                mask[row] = True
        except TypeError:  # (an unhashable preset is in no set)
            pass
    return mask


def kept_facets(tri_rows, absent) -> np.ndarray:
    """leaflet_present_triangle_mask (leaflet_presence.py:158-170): (nf,) bool, True where none of the three rows is
    absent."""
    if tri_rows is None or len(tri_rows) == 0:
        return np.zeros(0, dtype=bool)
    absent = np.asarray(absent, dtype=bool)
    if absent.size == 0:
        return np.ones(len(tri_rows), dtype=bool)
    return ~np.any(absent[np.asarray(tri_rows)], axis=1)


def validate_absence_topology(mesh, global_params) -> None:
    """validate_leaflet_absence_topology (runtime/leaflet_validation.py:22-84): in ``leaflet_out_absence_mode: strict``
    (the default) a triangle with absent and present rows raises ValueError; ``triangles`` (facet / facets / triangle)
    accepts."""
    mode = str(global_params.get("leaflet_out_absence_mode", "strict") or "strict").strip().lower()
    if mode in {"triangles", "facet", "facets", "triangle"}:
        return
    tri, _f = mesh.triangle_row_cache()
    if tri is None or len(tri) == 0:
        return
    absent = absent_mask(mesh, global_params, "out")
    if not np.any(absent):
        return
    tri = np.asarray(tri)
    tri_abs = absent[tri]
    bad = np.any(tri_abs, axis=1) & np.any(~tri_abs, axis=1)
    if not np.any(bad):
        return
    idxs = np.nonzero(bad)[0]
    vopts = vertex_options_by_row(mesh)
    examples = [{"tri_index": int(i), "rows": tuple(int(r) for r in tri[i]),
                 "presets": tuple(str((vopts.get(int(r)) or {}).get("preset") or "") for r in tri[i])} for i in idxs[:5]]
    raise ValueError("Leaflet absence topology invalid: outer leaflet marked absent on some presets but mesh contains "
                     f"triangles that straddle absent/present vertices. bad_triangles={int(idxs.size)} examples={examples}")


def _cached_absent_mask(mesh, gp) -> np.ndarray:
    """absent_mask(mesh, gp, "out"), resolved once per topology and preset list and kept on the mesh (as the reference
    keeps ``_leaflet_absent_mask_cache``): check_supported runs at every configuration and every plugin call.  Vertex
    presets edited in place need ``clear_absent_cache(mesh)`` (Minimizer.refresh_modules calls it)."""
    key = (getattr(mesh, "_vertex_ids_version", 0), getattr(mesh, "_topology_version", 0),
           getattr(mesh, "_facet_loops_version", 0), len(mesh.vertex_ids),
           tuple(sorted(normalize_preset_list(gp.get("leaflet_out_absent_presets")))))
    hit = getattr(mesh, "_hip_absent_out_cache", None)
    if hit is not None and hit[0] == key:
        return hit[1]
    mask = absent_mask(mesh, gp, "out")
    mask.setflags(write=False)
    try:
        mesh._hip_absent_out_cache = (key, mask)
    except AttributeError:  # (a mesh object that takes no new attribute: resolved every time)
        pass
    return mask


def clear_absent_cache(mesh) -> None:
    if getattr(mesh, "_hip_absent_out_cache", None) is not None:
        mesh._hip_absent_out_cache = None


def absent_out_rows(mesh, global_params):
    """The outer leaflet's absence mask for the device ((nv,) bool with a row set) or None when no preset list is
    given; everything about the two lists that the device path does not take is refused here."""
    gp = global_params if global_params is not None else {}
    raw_in = gp.get("leaflet_in_absent_presets")
    if normalize_preset_list(raw_in):
        raise L.MembraneHipError(f"leaflet tilt option leaflet_in_absent_presets={raw_in!r} is outside the HIP hot path "
                                 "(an absent inner leaflet: the reference's relaxation keeps the unmasked inner areas "
                                 "while its tilt_in module masks)")
    raw = gp.get("leaflet_out_absent_presets")
    if not normalize_preset_list(raw):
        return None
    absent = _cached_absent_mask(mesh, gp) if mesh is not None else np.zeros(0, dtype=bool)
    if not np.any(absent):
        raise L.MembraneHipError(f"leaflet tilt option leaflet_out_absent_presets={raw!r} selects no row of this mesh and "
                                 "is outside the HIP hot path (a mesh that lost its vertex options would otherwise run a "
                                 "full outer leaflet without a word)")
    mode = str(gp.get("rim_slope_match_mode") or "").strip().lower()
    if mode == "physical_edge_staggered_v1":
        raise L.MembraneHipError("leaflet_out_absent_presets next to rim_slope_match_mode=physical_edge_staggered_v1 (the "
                                 "continuation shell rows the reference keeps present) is outside the HIP hot path")
    return absent


_ABSENT_KEYS = ("leaflet_out_absent_presets", "leaflet_in_absent_presets")


def check_supported(global_params, mesh=None) -> None:
    """``mesh``: the mesh the options are read for -- without one a preset list can select no row and is refused."""
    absent_out_rows(mesh, global_params)
    for key in _UNSUPPORTED_KEYS:
        if key in _ABSENT_KEYS:
            continue
        val = global_params.get(key) if global_params is not None else None
        if val in (None, False, 0, 0.0, "", "off", "none", [], ()):
            continue
        raise L.MembraneHipError(f"leaflet tilt option {key}={val!r} is outside the HIP hot path")
    model = str(global_params.get("tilt_transport_model", "ambient_v1") or "ambient_v1").strip().lower()
    if model != "ambient_v1":
        raise L.MembraneHipError("tilt_transport_model other than ambient_v1 is outside the HIP hot path")
    cadence = str(global_params.get("tilt_projection_cadence", "per_step") or "per_step").strip().lower()
    if cadence not in {"per_step", "per_pass"}:
        raise ValueError("tilt_projection_cadence must be 'per_step' or 'per_pass'.")
    fb = str(global_params.get("tilt_cg_rejection_fallback", "off") or "off").strip().lower()
    if fb not in {"off", "gd"}:
        raise ValueError("tilt_cg_rejection_fallback must be 'off' or 'gd'.")
    if fb == "gd":
        raise L.MembraneHipError("tilt_cg_rejection_fallback=gd is outside the HIP hot path")


def tilt_modulus(param_resolver, global_params, leaflet: str) -> float:
    k = _get(param_resolver, global_params, f"tilt_modulus_{leaflet}")
    if k is None:
        k = _get(param_resolver, global_params, f"tilt_modolus_{leaflet}")  # legacy typo fallback
    return float(k or 0.0)


def tilt_mass_mode(param_resolver, global_params, leaflet: str) -> str:
    mode = _get(param_resolver, global_params, f"tilt_mass_mode_{leaflet}")
    if mode is None:
        mode = _get(param_resolver, global_params, "tilt_mass_mode")
    txt = str(mode or "lumped").strip().lower()
    if txt not in {"lumped", "consistent"}:
        raise ValueError(f"tilt_mass_mode_{leaflet} must be 'lumped' or 'consistent'.")
    return txt


def smoothness_rigidity(param_resolver, global_params, leaflet: str) -> float:
    k = _get(param_resolver, global_params, f"bending_modulus_{leaflet}")
    if k is None:
        k = _get(param_resolver, global_params, "bending_modulus")
    return float(k or 0.0)


def precond_smoothness(param_resolver, global_params, leaflet: str) -> float:
    """Rigidity in the leaflet Jacobi diagonal: ``get(bending_modulus_<l>) or get(bending_modulus) or 0``."""
    return float(_get(param_resolver, global_params, f"bending_modulus_{leaflet}")
                 or _get(param_resolver, global_params, "bending_modulus") or 0.0)


def relax_tilt_modulus(param_resolver, global_params, leaflet: str) -> float:
    """The relaxation's fast path reads ``tilt_modulus_<l>`` only (evaluation_manager.py:566, 674)."""
    return float(_get(param_resolver, global_params, f"tilt_modulus_{leaflet}") or 0.0)


def bending_params(mesh, global_params, leaflet: str):
    """(kappa, c0) arrays of bending_tilt_in/out (bt_params.py:225-318): leaflet modulus / spontaneous curvature with
    the global fallbacks; per-vertex arrays of an ArrayMesh override like vertex options do."""
    nv = len(mesh.vertex_ids)
    k = global_params.get(f"bending_modulus_{leaflet}")
    if k is None:
        k = global_params.get("bending_modulus", 0.0)
    c = global_params.get(f"spontaneous_curvature_{leaflet}")
    if c is None:
        c = global_params.get("spontaneous_curvature")
        if c is None:
            c = global_params.get("intrinsic_curvature", 0.0)
    kappa = np.full(nv, float(k or 0.0))
    c0 = np.full(nv, float(c or 0.0))
    getter = getattr(mesh, "get_vertex_parameter_array", None)
    if getter is not None:
        for key in (f"bending_modulus_{leaflet}", "bending_modulus"):
            arr = getter(key)
            if arr is not None:
                kappa = np.asarray(arr, dtype=np.float64)
                break
        for key in (f"spontaneous_curvature_{leaflet}", "spontaneous_curvature"):
            arr = getter(key)
            if arr is not None:
                c0 = np.asarray(arr, dtype=np.float64)
                break
    elif isinstance(getattr(mesh, "vertices", None), dict):
        rows = mesh.vertex_index_to_row
        for vid, vertex in mesh.vertices.items():
            row = rows.get(int(vid))
            opts = getattr(vertex, "options", None) or {}
            if row is None:
                continue
            for key in (f"bending_modulus_{leaflet}", "bending_modulus"):
                if key in opts:
                    try:
                        kappa[row] = float(opts[key])
                    except (TypeError, ValueError):
                        pass
                    break
            for key in (f"spontaneous_curvature_{leaflet}", "spontaneous_curvature", "intrinsic_curvature"):
                if opts.get(key) is not None:
                    try:
                        c0[row] = float(opts[key])
                    except (TypeError, ValueError):
                        pass
                    break
    return kappa, c0


def disk_target_rows(mesh, leaflet: str, group: str) -> np.ndarray:
    """Rows tagged ``tilt_disk_target_group_<leaflet> == group`` (tilt_disk_target_in.py:137-145): vertex options of
    a reference Mesh, or the ``disk_rows_<leaflet>`` attribute (mask / row list) of an array mesh."""
    nv = len(mesh.vertex_ids)
    own = getattr(mesh, f"disk_rows_{leaflet}", None)
    if own is not None:
        own = np.asarray(own)
        return np.flatnonzero(own) if own.dtype == bool else own.astype(np.int64)
    verts = getattr(mesh, "vertices", None)
    if isinstance(verts, dict):
        rows = []
        key = f"tilt_disk_target_group_{leaflet}"
        for vid in mesh.vertex_ids:
            opts = getattr(verts[int(vid)], "options", None) or {}
            if opts.get(key) == group:
                row = mesh.vertex_index_to_row.get(int(vid))
                if row is not None:
                    rows.append(int(row))
        return np.asarray(rows, dtype=np.int64)
    return np.zeros(0, dtype=np.int64) if nv >= 0 else None


def disk_target_params(mesh, param_resolver, global_params, leaflet: str):
    """Resolved parameters of tilt_disk_target_<leaflet> (tilt_disk_target_in.py:38-134) as kwargs of
    DeviceMesh.set_leaflet_disk_target, or None when the module contributes nothing (:175-191)."""

    def pick(name):
        v = _get(param_resolver, global_params, f"tilt_disk_target_{name}_{leaflet}")
        return _get(param_resolver, global_params, f"tilt_disk_target_{name}") if v is None else v

    raw = _get(param_resolver, global_params, f"tilt_disk_target_group_{leaflet}")
    group = None if raw is None else str(raw).strip()
    if not group:
        return None
    k = float(_get(param_resolver, global_params, f"tilt_disk_target_strength_{leaflet}") or 0.0)
    theta_b = float(pick("theta_B") or 0.0)
    if k == 0.0 or theta_b == 0.0:
        return None
    rows = disk_target_rows(mesh, leaflet, group)
    if rows.size == 0:
        return None
    normal = pick("normal")
    if normal is None or float(np.linalg.norm(np.asarray(normal, dtype=float))) < 1e-15:
        raise L.MembraneHipError("tilt_disk_target without tilt_disk_target_normal (SVD plane fit of the disk rows) "
                                 "is outside the HIP hot path")
    center = pick("center")
    radius = pick("radius")
    try:
        radius = float(radius) if radius is not None and float(radius) > 0.0 else None
    except (TypeError, ValueError):
        radius = None
    lam = pick("lambda")
    if lam is not None:
        try:
            lam = float(lam)
        except (TypeError, ValueError):
            lam = 0.0
    else:
        kt = _get(param_resolver, global_params, f"tilt_modulus_{leaflet}")
        if kt is None and leaflet == "in":
            kt = _get(param_resolver, global_params, "tilt_modolus_in")
        kap = _get(param_resolver, global_params, f"bending_modulus_{leaflet}")
        if kap is None:
            kap = _get(param_resolver, global_params, "bending_modulus")
        lam = 0.0
        try:
            if kt is not None and kap is not None and float(kt) > 0.0 and float(kap) > 0.0:
                lam = float(np.sqrt(float(kt) / float(kap)))
        except (TypeError, ValueError):
            lam = 0.0
    return {"disk_rows": rows, "strength": k, "theta_b": theta_b, "lam": lam,
            "center": tuple(np.asarray([0.0, 0.0, 0.0] if center is None else center, dtype=float).reshape(3)),
            "normal": tuple(np.asarray(normal, dtype=float).reshape(3)), "radius": radius}


class _Options:
    """Stand-in for an entity of the reference (``.options``) when the options come from an ArrayMesh's tables."""

    __slots__ = ("options",)

    def __init__(self, options):
        self.options = options or {}


def pin_to_circle_group(options):
    """tilt_rim_source_in.py:50-54, as the reference has it: a vertex without options (None or empty) has no group;
    options whose ``pin_to_circle_group`` is None -- the key absent from non-empty options included, the reference
    reads ``options.get`` -- mean "default"."""
    if not options:
        return None
    group = options.get("pin_to_circle_group")
    return "default" if group is None else str(group)


def contact_line_strength(param_resolver, obj, leaflet: str) -> float:
    """gamma of one rim edge (modules/energy/contact_mapping.py:36-131): the strength key from the edge's options and
    then the global, else ``contact_gamma``, else ``h * delta_epsilon_over_a`` (or ``delta_epsilon / a``), each with
    the leaflet's suffix first and then without, then the si / physical unit conversion.  ``leaflet`` None: the bilayer
    module's suffix-free keys (tilt_rim_source_bilayer.py:129-136, contact_suffix "")."""
    key = f"tilt_rim_source_strength_{leaflet}" if leaflet else "tilt_rim_source_strength"
    val = param_resolver.get(obj, key)
    if val is None:
        val = param_resolver.get(None, key)
    if val is not None:
        return float(val)
    suffix = f"_{leaflet}" if leaflet else ""

    def get_key(base):
        got = param_resolver.get(obj, base + suffix)
        if got is None:
            got = param_resolver.get(None, base + suffix)
        if got is not None:
            return got
        got = param_resolver.get(obj, base)
        if got is None:
            got = param_resolver.get(None, base)
        return got

    def convert(raw):
        units = str(param_resolver.get(None, "tilt_rim_source_contact_units") or "solver").strip().lower()
        if units not in {"si", "physical", "physical_si"}:
            return float(raw)
        length = param_resolver.get(None, "tilt_rim_source_contact_length_unit_m")
        kappa = param_resolver.get(None, "tilt_rim_source_contact_kappa_ref_J")
        if length is None or kappa is None or abs(float(length)) < 1e-30 or abs(float(kappa)) < 1e-30:
            return float(raw)
        return float(raw) * float(length) / float(kappa)

    direct = get_key("tilt_rim_source_contact_gamma")
    if direct is not None:
        return convert(float(direct))
    h = get_key("tilt_rim_source_contact_h")
    if h is None:
        return 0.0
    ratio = get_key("tilt_rim_source_contact_delta_epsilon_over_a")
    if ratio is None:
        de, a = get_key("tilt_rim_source_contact_delta_epsilon"), get_key("tilt_rim_source_contact_a")
        if de is None or a is None:
            return 0.0
        ratio = float(de) / float(a)
    return convert(float(h) * float(ratio))


def _rim_entities(mesh):
    """-> (options per row {row: dict}, edges [(tail row, head row, options)]) of a reference Mesh or an ArrayMesh."""
    row_of = mesh.vertex_index_to_row
    if isinstance(getattr(mesh, "vertices", None), dict):
        vopts = {}
        for vid, v in mesh.vertices.items():
            row = row_of.get(int(vid))
            if row is not None:
                vopts[int(row)] = getattr(v, "options", None) or {}
        edges = []
        for e in mesh.edges.values():
            t, h = row_of.get(int(e.tail_index)), row_of.get(int(e.head_index))
            if t is not None and h is not None:
                edges.append((int(t), int(h), getattr(e, "options", None) or {}))
        return vopts, edges
    er = getattr(mesh, "edge_rows", None)
    if er is None:
        raise L.MembraneHipError("tilt_rim_source on a mesh without an edge table (ArrayMesh(edges=, edge_options=)) "
                                 "is outside the HIP hot path")
    vopts = {int(r): (o or {}) for r, o in (getattr(mesh, "vertex_options", None) or {}).items()}
    eo = getattr(mesh, "edge_options", None) or {}
    return vopts, [(int(er[k, 0]), int(er[k, 1]), eo.get(k) or {}) for k in range(len(er))]


def _side_counts(mesh, tail, head):
    """How many triangles each edge is a side of (the reference's len(edge_to_facets[edge]))."""
    tri, _f = mesh.triangle_row_cache()
    nv = len(mesh.vertex_ids)
    if tri is None or len(tri) == 0 or len(tail) == 0:
        return np.zeros(len(tail), dtype=np.int64)
    tri = np.asarray(tri, dtype=np.int64).reshape(-1, 3)
    a = np.concatenate([tri[:, 0], tri[:, 1], tri[:, 2]])
    b = np.concatenate([tri[:, 1], tri[:, 2], tri[:, 0]])
    keys, cnt = np.unique(np.minimum(a, b) * nv + np.maximum(a, b), return_counts=True)
    t, h = np.asarray(tail, dtype=np.int64), np.asarray(head, dtype=np.int64)
    want = np.minimum(t, h) * nv + np.maximum(t, h)
    pos = np.searchsorted(keys, want)
    pos[pos >= len(keys)] = 0
    return np.where(keys[pos] == want, cnt[pos], 0)


def rim_source_selection(mesh, param_resolver, global_params, leaflet: str | None = None):
    """-> (options per row, the selected rim edges [(tail row, head row, options)]) of a rim source; no group, or no
    edge with both ends in it (boundary mode: and on the boundary), selects nothing."""
    raw = _get(param_resolver, global_params, f"tilt_rim_source_group_{leaflet}" if leaflet else "tilt_rim_source_group")
    group = None if raw is None else str(raw).strip()
    if not group:
        return {}, []
    mode = str(_get(param_resolver, global_params, "tilt_rim_source_edge_mode") or "boundary").strip().lower()
    mode = "all" if mode == "all" else "boundary"
    vopts, edges = _rim_entities(mesh)
    member = {row for row, o in vopts.items() if pin_to_circle_group(o) == group}
    sel = [(t, h, o) for (t, h, o) in edges if t in member and h in member]
    if sel and mode == "boundary":
        cnt = _side_counts(mesh, [s[0] for s in sel], [s[1] for s in sel])
        # (tilt_rim_source_bilayer.py:67 keeps the edges with fewer than two triangles)
        sel = [s for s, n in zip(sel, cnt) if (n == 1 if leaflet else n < 2)]
    return vopts, sel


def rim_source_params(mesh, param_resolver, global_params, leaflet: str | None = None):
    """Resolved tables of tilt_rim_source_<leaflet> (tilt_rim_source_in.py:57-336) as kwargs of
    DeviceMesh.set_leaflet_rim_source, or None when the module contributes nothing (no group, no rim edge, every gamma
    0: :386-404).  Rim edges: both ends carry ``pin_to_circle_group == tilt_rim_source_group_<leaflet>``; with
    ``tilt_rim_source_edge_mode`` boundary (the default) only sides of exactly one triangle.  Frame: fixed center
    ``tilt_rim_source_center`` and the ``pin_to_circle_normal`` of the first rim row (row order) that carries one, else
    (0,0,1); follow (center = mean of the rim rows) when a rim row resolves ``pin_to_circle_mode`` to fit -- then a
    ``pin_to_circle_normal`` is required (the reference's SVD plane fit is host work).

    ``leaflet`` None resolves tilt_rim_source_bilayer (tilt_rim_source_bilayer.py:58-255, :431-479), as kwargs of
    DeviceMesh.set_rim_source_bilayer: the group is ``tilt_rim_source_group`` and the strength chain is read without a
    leaflet suffix; boundary mode keeps the edges with FEWER THAN TWO triangles (:67); the fixed frame's normal is
    always (0,0,1), whatever the rows carry (:478-479).  The stage-A restriction to the outermost midpoint chain needs
    ``theory_parity_lane: stage_a_emergent``, which check_supported refuses: it is not built."""
    name = f"tilt_rim_source_{leaflet}" if leaflet else "tilt_rim_source_bilayer"
    vopts, sel = rim_source_selection(mesh, param_resolver, global_params, leaflet)
    if not sel:
        return None
    resolver = param_resolver if param_resolver is not None else _GlobalOnly(global_params)
    gamma = np.array([contact_line_strength(resolver, _Options(o), leaflet) for (_t, _h, o) in sel], dtype=np.float64)
    if not np.any(gamma):
        return None
    tail = np.array([s[0] for s in sel], dtype=np.int32)
    head = np.array([s[1] for s in sel], dtype=np.int32)
    rim_rows = np.unique(np.concatenate([tail, head]))

    def opt(row, key):
        o = vopts.get(int(row)) or {}
        val = o.get(key)
        return global_params.get(key) if val is None and global_params is not None else val

    follow = any(str(opt(r, "pin_to_circle_mode") or "fixed").strip().lower() == "fit" for r in rim_rows)
    normal = None
    for r in rim_rows:
        rawn = opt(r, "pin_to_circle_normal")
        if rawn is None:
            continue
        vec = np.asarray(rawn, dtype=float).reshape(3)
        if float(np.linalg.norm(vec)) >= 1e-15:
            normal = vec / float(np.linalg.norm(vec))
            break
    if normal is None:
        if follow:
            raise L.MembraneHipError(f"{name} in follow mode (pin_to_circle_mode: fit) without "
                                     "pin_to_circle_normal on a rim vertex (SVD plane fit of the rim rows) is outside "
                                     "the HIP hot path")
        normal = np.array([0.0, 0.0, 1.0])
    if leaflet != "in" and not follow:
        # tilt_rim_source_out.py:311-312, tilt_rim_source_bilayer.py:478-479: their fixed frame never reads the rows' normal
        normal = np.array([0.0, 0.0, 1.0])
    center = _get(param_resolver, global_params, "tilt_rim_source_center")
    center = np.asarray([0.0, 0.0, 0.0] if center is None else center, dtype=float).reshape(3)
    return {"tail": tail, "head": head, "gamma": gamma, "center": tuple(float(v) for v in center),
            "normal": tuple(float(v) for v in normal), "follow": bool(follow)}


class _GlobalOnly:
    def __init__(self, gp):
        self.gp = gp

    def get(self, obj, name):
        opts = getattr(obj, "options", None) if obj is not None else None
        if opts and name in opts:
            return opts[name]
        return self.gp.get(name) if self.gp is not None else None


def rim_source_key(prm):
    """Hashable identity of rim_source_params' result (the Minimizer re-uploads when it changes)."""
    if prm is None:
        return None
    return (prm["tail"].tobytes(), prm["head"].tobytes(), prm["gamma"].tobytes(), prm["center"], prm["normal"],
            prm["follow"])


def rim_source_host_tables(nv: int, iperm, tail, head, gamma):
    """The row -> rim edge CSR as the library builds it (ms_rim_source_tables_host: the code
    ms_set_leaflet_rim_source runs), rows in the library's order (``iperm``: external row -> library row)."""
    ip = np.ascontiguousarray(np.asarray(iperm, dtype=np.int32).reshape(-1))
    t = np.ascontiguousarray(np.asarray(tail, dtype=np.int32).reshape(-1))
    h = np.ascontiguousarray(np.asarray(head, dtype=np.int32).reshape(-1))
    g = np.ascontiguousarray(np.asarray(gamma, dtype=np.float64).reshape(-1))
    n = len(t)
    cnt = np.zeros(2, dtype=np.int32)
    vrow, off = np.zeros(2 * n + 1, np.int32), np.zeros(2 * n + 2, np.int32)
    other, og = np.zeros(2 * n + 1, np.int32), np.zeros(2 * n + 1)
    i32 = lambda a: a.ctypes.data_as(L._I32)  # noqa: E731
    rc = L.lib().ms_rim_source_tables_host(int(nv), i32(ip), n, i32(t), i32(h), g.ctypes.data_as(L._D), i32(cnt),
                                           i32(vrow), i32(off), i32(other), og.ctypes.data_as(L._D))
    L.check(rc, None, "ms_rim_source_tables_host")
    ne, nt = int(cnt[0]), int(cnt[1])
    return {"n_edges": ne, "vrow": vrow[:nt].copy(), "off": off[:nt + 1].copy(), "other": other[:2 * ne].copy(),
            "csr_gamma": og[:2 * ne].copy()}


_COUPLING_MODES = {"difference": -1, "diff": -1, "minus": -1, "sub": -1, "sum": 1, "add": 1, "plus": 1}


def coupling_params(param_resolver, global_params):
    """(k_c, sign) of tilt_coupling (modules/energy/tilt_coupling.py:24-40): ``tilt_coupling_modulus`` and
    ``tilt_coupling_mode`` with the misspelt ``tilt_couping_mode`` as fallback; sign -1 for difference / diff / minus /
    sub, +1 for sum / add / plus.  None when the module contributes nothing: unknown or absent mode, or k_c == 0."""
    mode = _get(param_resolver, global_params, "tilt_coupling_mode")
    if mode is None:
        mode = _get(param_resolver, global_params, "tilt_couping_mode")
    if mode is None:
        return None
    sign = _COUPLING_MODES.get(str(mode).strip().lower())
    k_c = float(_get(param_resolver, global_params, "tilt_coupling_modulus") or 0.0)
    if sign is None or k_c == 0.0:
        return None
    return k_c, sign


def evaluate_coupling(mesh, global_params, param_resolver, *, positions, tilts_in, tilts_out, grad_arr,
                      tilt_in_grad_arr, tilt_out_grad_arr) -> float:
    """tilt_coupling on caller arrays (H2D/D2H per call: the parity seam, not the hot loop): energy; shape gradient
    ADDED into ``grad_arr``, tilt gradients ADDED into ``tilt_in_grad_arr`` / ``tilt_out_grad_arr`` (each optional)."""
    prm = coupling_params(param_resolver, global_params)
    if prm is None:
        return 0.0
    tri, _f = mesh.triangle_row_cache()
    if tri is None or len(tri) == 0:
        return 0.0
    nv = len(mesh.vertex_ids)
    fields = {}
    for lf, t in (("in", tilts_in), ("out", tilts_out)):
        if t is None:
            t = mesh.tilts_in_view() if lf == "in" else mesh.tilts_out_view()
        t = np.ascontiguousarray(t, dtype=np.float64)
        if t.shape != (nv, 3):
            raise ValueError(f"tilts_{lf} must have shape (N_vertices, 3)")
        fields[lf] = t
    for name, arr in (("tilt_in_grad_arr", tilt_in_grad_arr), ("tilt_out_grad_arr", tilt_out_grad_arr)):
        if arr is not None and np.shape(arr) != (nv, 3):
            raise ValueError(f"{name} must have shape (N_vertices, 3)")
    mir = mirror_for(mesh)
    dm = mir.sync(positions=None if positions is mesh.positions_view() else positions)
    for lf in ("in", "out"):
        dm.set_leaflet_tilts(lf, fields[lf], tilt_modulus=0.0, smoothness=0.0)
    mir._leaflet_keys = {}  # foreign arrays were uploaded
    dm.set_tilt_coupling(*prm)
    dm.set_params(modules=L.MS_MOD_TILT_COUPLING)
    if grad_arr is not None:
        e, g = dm.energy_and_gradient(want_grad=True, raw=True)
        grad_arr += g
        E = float(e[3])
    else:
        E = float(dm.energy()[3])
    if tilt_in_grad_arr is not None or tilt_out_grad_arr is not None:
        _e, gi, go = dm.leaflet_tilt_energy_and_gradient(want_gradient=True)
        if tilt_in_grad_arr is not None:
            tilt_in_grad_arr += gi
        if tilt_out_grad_arr is not None:
            tilt_out_grad_arr += go
    return E


def evaluate_rim_bilayer(mesh, global_params, param_resolver, *, positions, tilts_in, tilts_out, tilt_in_grad_arr,
                         tilt_out_grad_arr) -> float:
    """tilt_rim_source_bilayer on caller arrays (H2D/D2H per call: the parity seam, not the hot loop): energy; the SAME
    coefficient rows ADDED into ``tilt_in_grad_arr`` and ``tilt_out_grad_arr`` (each optional).  No shape gradient: the
    caller's ``grad_arr`` is never touched.  The early returns keep the reference's order (:431-462): no group and no
    selected edge return 0.0 before the tilt shapes are looked at, a bad shape raises before gamma is."""
    check_supported(global_params if global_params is not None else {}, mesh)
    tri, _f = mesh.triangle_row_cache()
    if tri is None or len(tri) == 0:
        return 0.0
    nv = len(mesh.vertex_ids)
    if not rim_source_selection(mesh, param_resolver, global_params, None)[1]:
        return 0.0
    fields = {}
    for lf, t in (("in", tilts_in), ("out", tilts_out)):
        if t is None:
            t = mesh.tilts_in_view() if lf == "in" else mesh.tilts_out_view()
        t = np.ascontiguousarray(t, dtype=np.float64)
        if t.shape != (nv, 3):
            raise ValueError(f"tilts_{lf} must have shape (N_vertices, 3)")
        fields[lf] = t
    prm = rim_source_params(mesh, param_resolver, global_params, None)
    if prm is None:
        return 0.0
    for name, arr in (("tilt_in_grad_arr", tilt_in_grad_arr), ("tilt_out_grad_arr", tilt_out_grad_arr)):
        if arr is not None and np.shape(arr) != (nv, 3):
            raise ValueError(f"{name} must have shape (N_vertices, 3)")
    if prm["follow"]:
        # tilt_rim_source_bilayer.py:355: the followed center is read from the MESH, whatever `positions` the caller
        # evaluates on -- a fixed frame for this one call
        rows = np.unique(np.concatenate([prm["tail"], prm["head"]]))
        center = np.mean(np.asarray(mesh.positions_view(), dtype=np.float64)[rows], axis=0)
        prm = dict(prm, center=tuple(float(v) for v in center), follow=False)
    mir = mirror_for(mesh)
    dm = mir.sync(positions=None if positions is mesh.positions_view() else positions)
    for lf in ("in", "out"):
        dm.set_leaflet_tilts(lf, fields[lf], tilt_modulus=0.0, smoothness=0.0)
    mir._leaflet_keys = {}  # foreign arrays were uploaded
    dm.set_rim_source_bilayer(**prm)
    dm.set_params(modules=L.MS_MOD_TILT_RIM_SOURCE_BILAYER)
    if tilt_in_grad_arr is None and tilt_out_grad_arr is None:
        return float(dm.energy()[3])
    E, gi, go = dm.leaflet_tilt_energy_and_gradient(want_gradient=True)
    if tilt_in_grad_arr is not None:
        tilt_in_grad_arr += gi
    if tilt_out_grad_arr is not None:
        tilt_out_grad_arr += go
    return float(E)


def thetab_contact_group(param_resolver, global_params):
    """The ring's group (tilt_thetaB_contact_in.py:46-53): ``tilt_thetaB_group_in``, else
    ``rim_slope_match_disk_group``; None when neither names one."""
    raw = _get(param_resolver, global_params, "tilt_thetaB_group_in")
    if raw is None:
        raw = _get(param_resolver, global_params, "rim_slope_match_disk_group")
    if raw is None:
        return None
    group = str(raw).strip()
    return group if group else None


def thetab_contact_rows(mesh, group: str) -> np.ndarray:
    """Rows whose options carry ``rim_slope_match_group == group`` or ``tilt_thetaB_group == group``, in vertex_ids order
    (tilt_thetaB_contact_in.py:178-197): vertex options of a reference Mesh, or ``vertex_options`` of an array mesh."""
    tagged = lambda o: o.get("rim_slope_match_group") == group or o.get("tilt_thetaB_group") == group  # noqa: E731
    verts = getattr(mesh, "vertices", None)
    rows = []
    if isinstance(verts, dict):
        for vid in mesh.vertex_ids:
            if tagged(getattr(verts[int(vid)], "options", None) or {}):
                row = mesh.vertex_index_to_row.get(int(vid))
                if row is not None:
                    rows.append(int(row))
    else:
        vopts = getattr(mesh, "vertex_options", None) or {}
        row_of = mesh.vertex_index_to_row
        for vid in mesh.vertex_ids:
            row = row_of.get(int(vid))
            if row is not None and tagged(vopts.get(int(row)) or {}):
                rows.append(int(row))
    return np.asarray(rows, dtype=np.int64)


def thetab_contact_modes(global_params):
    """(work mode, penalty mode) of tilt_thetaB_contact_in (:150-175): ``field_linear`` or the default ``scalar``;
    ``legacy`` for legacy / on / true / 1, else ``off``."""
    raw = None if global_params is None else global_params.get("tilt_thetaB_contact_work_mode")
    work = "field_linear" if raw is not None and str(raw).strip().lower() == "field_linear" else "scalar"
    raw = None if global_params is None else global_params.get("tilt_thetaB_contact_penalty_mode")
    pen = "legacy" if raw is not None and str(raw).strip().lower() in {"legacy", "on", "true", "1"} else "off"
    return work, pen


def thetab_value(global_params) -> float:
    """theta_B (tilt_thetaB_contact_in.py:145-147)."""
    return float((global_params.get("tilt_thetaB_value") if global_params is not None else None) or 0.0)


def thetab_contact_params(mesh, param_resolver, global_params):
    """Resolved parameters of tilt_thetaB_contact_in as kwargs of DeviceMesh.set_thetab_contact, or None where the
    reference returns 0.0 before it looks at a position: no group (:351-353), no tagged row (:208-210), k == gamma == 0
    (:373-374).  The two 1e-12 returns depend on the positions: the device takes them.  Refused: a missing or zero
    ``tilt_thetaB_normal`` (the SVD plane fit of the ring, :70-91, stays host work), a ring above the device's size and
    non-finite parameters."""
    group = thetab_contact_group(param_resolver, global_params)
    if group is None:
        return None
    rows = thetab_contact_rows(mesh, group)
    if rows.size == 0:
        return None
    k = float(_get(param_resolver, global_params, "tilt_thetaB_strength_in") or 0.0)
    gamma = float(_get(param_resolver, global_params, "tilt_thetaB_contact_strength_in") or 0.0)
    if k == 0.0 and gamma == 0.0:  # (whatever the frame: the reference's result is 0.0 with a fitted normal as well)
        return None
    center = _get(param_resolver, global_params, "tilt_thetaB_center")
    center = np.asarray([0.0, 0.0, 0.0] if center is None else center, dtype=float).reshape(3)
    raw = _get(param_resolver, global_params, "tilt_thetaB_normal")
    normal = None if raw is None else np.asarray(raw, dtype=float).reshape(3)
    if normal is not None and not np.all(np.isfinite(normal)):
        raise L.MembraneHipError("tilt_thetaB_contact_in: tilt_thetaB_normal must be finite")
    if normal is None or float(np.linalg.norm(normal)) < 1e-15:
        raise L.MembraneHipError("tilt_thetaB_contact_in without a non-zero tilt_thetaB_normal (SVD plane fit of the "
                                 "ring rows) is outside the HIP hot path")
    if rows.size > L.MS_THETAB_MAX_ROWS:
        raise L.MembraneHipError(f"tilt_thetaB_contact_in: a ring of {rows.size} rows is above the "
                                 f"{L.MS_THETAB_MAX_ROWS} the device orders")
    if not (np.isfinite(k) and np.isfinite(gamma) and np.all(np.isfinite(center))
            and np.isfinite(thetab_value(global_params))):
        raise L.MembraneHipError("tilt_thetaB_contact_in: tilt_thetaB_strength_in, tilt_thetaB_contact_strength_in, "
                                 "tilt_thetaB_center and tilt_thetaB_value must be finite")
    work, pen = thetab_contact_modes(global_params)
    return {"rows": rows.astype(np.int32), "center": tuple(float(v) for v in center),
            "normal": tuple(float(v) for v in normal), "k": k, "gamma": gamma, "work_mode": work, "penalty_mode": pen}


def thetab_contact_key(prm):
    """Hashable identity of thetab_contact_params' result (the Minimizer re-uploads when it changes; theta_B is no part
    of it: it changes between steps and goes to the device by ms_set_thetab_value)."""
    if prm is None:
        return None
    return (prm["rows"].tobytes(), prm["center"], prm["normal"], prm["k"], prm["gamma"], prm["work_mode"],
            prm["penalty_mode"])


def _thetab_upload(mesh, global_params, param_resolver, positions, tilts_in):
    """The contact term alone on caller arrays -> (DeviceMesh, mirror), or None where the term contributes nothing."""
    check_supported(global_params if global_params is not None else {}, mesh)
    if thetab_contact_group(param_resolver, global_params) is None:
        return None
    nv = len(mesh.vertex_ids)
    if tilts_in is None:
        tilts_in = mesh.tilts_in_view()
    tilts_in = np.ascontiguousarray(tilts_in, dtype=np.float64)
    if tilts_in.shape != (nv, 3):
        raise ValueError("tilts_in must have shape (N_vertices, 3)")
    prm = thetab_contact_params(mesh, param_resolver, global_params)
    if prm is None:
        return None
    mir = mirror_for(mesh)
    dm = mir.sync(positions=None if positions is mesh.positions_view() else positions)
    dm.set_leaflet_tilts("in", tilts_in, tilt_modulus=0.0, smoothness=0.0)
    dm.set_leaflet_tilts("out", np.zeros((nv, 3)), tilt_modulus=0.0, smoothness=0.0)
    mir._leaflet_keys = {}  # foreign arrays were uploaded
    dm.set_thetab_contact(**prm)
    dm.set_thetab_value(thetab_value(global_params))
    dm.set_params(modules=L.MS_MOD_TILT_THETAB_CONTACT_IN)
    return dm, mir


def evaluate_thetab_contact(mesh, global_params, param_resolver, *, positions, tilts_in, tilt_in_grad_arr) -> float:
    """tilt_thetaB_contact_in on caller arrays (H2D/D2H per call: the parity seam, not the hot loop): energy; tilt
    gradient ADDED into ``tilt_in_grad_arr`` (optional).  No shape gradient and nothing for the outer leaflet.  0.0
    exactly where the reference returns early: no group, no rows, k == gamma == 0 and the two 1e-12 returns (the
    device's "contributes nothing" state: every sum is skipped)."""
    up = _thetab_upload(mesh, global_params, param_resolver, positions, tilts_in)
    if up is None:
        return 0.0
    dm, _mir = up
    if tilt_in_grad_arr is not None and np.shape(tilt_in_grad_arr) != (len(mesh.vertex_ids), 3):
        raise ValueError("tilt_in_grad_arr must have shape (N_vertices, 3)")
    if tilt_in_grad_arr is None:
        return float(dm.energy()[3])
    E, gi, _go = dm.leaflet_tilt_energy_and_gradient(want_gradient=True)
    tilt_in_grad_arr += gi
    return float(E)


def thetab_update_scalar(mesh, global_params, param_resolver) -> None:
    """update_scalar_params of tilt_thetaB_contact_in (:271-302) on the mesh's positions and inner tilts: legacy penalty
    mode with k > 0 only; theta_B = sum w theta / wsum + 2 pi R_eff gamma / (k wsum) written into
    ``tilt_thetaB_value``."""
    if thetab_contact_modes(global_params)[1] != "legacy":
        return
    up = _thetab_upload(mesh, global_params, param_resolver, mesh.positions_view(), None)
    if up is None:
        return
    tb, changed = up[0].update_thetab_value()
    if changed:
        _set_param(global_params, "tilt_thetaB_value", float(tb))


def _set_param(global_params, key, value) -> None:
    if hasattr(global_params, "set"):
        global_params.set(key, value)
    else:
        global_params[key] = value


# --- rim_slope_match_out ----------------------------------------------------------------------------------------------
_RIM_MATCH_MODES = ("pointwise_radial_v1", "ring_average_radial_v1", "shared_rim_staggered_v1",
                    "physical_edge_staggered_v1")
_RIM_MATCH_WARNED = False


def rim_match_group(param_resolver, global_params, key: str):
    """A group name of rim_slope_match_out (:78-83): stripped, None when absent or empty."""
    raw = _get(param_resolver, global_params, key)
    if raw is None:
        return None
    group = str(raw).strip()
    return group if group else None


def rim_match_sanitize_disk_group(rim_group, disk_group):
    """_sanitize_disk_group (:86-102): a disk group equal to the rim group is dropped, with one warning per process."""
    if rim_group is None or disk_group is None or disk_group != rim_group:
        return disk_group
    global _RIM_MATCH_WARNED
    if not _RIM_MATCH_WARNED:
        import logging

        logging.getLogger("membrane_solver").warning(
            "rim_slope_match_disk_group matches rim_slope_match_group (%s); skipping disk-side coupling to avoid "
            "degenerate constraints.", rim_group)
        _RIM_MATCH_WARNED = True
    return None


def rim_match_mode(param_resolver, global_params) -> str:
    """rim_slope_match_mode (:117-131): default pointwise_radial_v1, an unknown mode raises ValueError."""
    raw = _get(param_resolver, global_params, "rim_slope_match_mode")
    mode = "pointwise_radial_v1" if raw is None else str(raw).strip().lower()
    if mode not in _RIM_MATCH_MODES:
        raise ValueError("rim_slope_match_mode must be 'pointwise_radial_v1' or 'ring_average_radial_v1' or "
                         "'shared_rim_staggered_v1' or 'physical_edge_staggered_v1'.")
    return mode


def rim_match_strength(param_resolver, global_params) -> float:
    return float(_get(param_resolver, global_params, "rim_slope_match_strength") or 0.0)


def rim_match_rows(mesh, group: str) -> np.ndarray:
    """Rows whose options carry ``rim_slope_match_group == group``, in vertex_ids order (:160-169): vertex options of a
    reference Mesh, or ``vertex_options`` of an array mesh."""
    verts = getattr(mesh, "vertices", None)
    rows = []
    if isinstance(verts, dict):
        for vid in mesh.vertex_ids:
            if (getattr(verts[int(vid)], "options", None) or {}).get("rim_slope_match_group") == group:
                row = mesh.vertex_index_to_row.get(int(vid))
                if row is not None:
                    rows.append(int(row))
    else:
        vopts = getattr(mesh, "vertex_options", None) or {}
        row_of = mesh.vertex_index_to_row
        for vid in mesh.vertex_ids:
            row = row_of.get(int(vid))
            if row is not None and (vopts.get(int(row)) or {}).get("rim_slope_match_group") == group:
                rows.append(int(row))
    return np.asarray(rows, dtype=np.int64)


def rim_match_params(mesh, param_resolver, global_params):
    """Resolved parameters of rim_slope_match_out as kwargs of DeviceMesh.set_rim_match, or None where the reference
    returns 0.0 before it looks at a position: strength 0 (:380-382), no rim or outer group (:377-378), an empty rim or
    outer ring (:420-421).  The other early returns depend on the positions: the device takes them.  Refused, each with
    its own text: the staggered modes, a missing or zero ``rim_slope_match_normal`` (the SVD plane fit, :422-423), a ring
    above the device's size and non-finite parameters."""
    mode = rim_match_mode(param_resolver, global_params)
    k = rim_match_strength(param_resolver, global_params)
    if k == 0.0:
        return None
    if not np.isfinite(k):
        raise L.MembraneHipError("rim_slope_match_out: rim_slope_match_strength must be finite")
    if mode in ("shared_rim_staggered_v1", "physical_edge_staggered_v1"):
        raise L.MembraneHipError(f"rim_slope_match_out with rim_slope_match_mode={mode} and a non-zero "
                                 "rim_slope_match_strength (vertex normals and local interface shells) is outside the "
                                 "HIP hot path")
    group = rim_match_group(param_resolver, global_params, "rim_slope_match_group")
    outer_group = rim_match_group(param_resolver, global_params, "rim_slope_match_outer_group")
    disk_group = rim_match_sanitize_disk_group(group, rim_match_group(param_resolver, global_params,
                                                                      "rim_slope_match_disk_group"))
    if group is None or outer_group is None:
        return None
    rim, outer = rim_match_rows(mesh, group), rim_match_rows(mesh, outer_group)
    if rim.size == 0 or outer.size == 0:
        return None
    disk = rim_match_rows(mesh, disk_group) if disk_group is not None else np.zeros(0, np.int64)
    center = _get(param_resolver, global_params, "rim_slope_match_center")
    center = np.asarray([0.0, 0.0, 0.0] if center is None else center, dtype=float).reshape(3)
    raw = _get(param_resolver, global_params, "rim_slope_match_normal")
    normal = None if raw is None else np.asarray(raw, dtype=float).reshape(3)
    if not np.all(np.isfinite(center)) or (normal is not None and not np.all(np.isfinite(normal))):
        raise L.MembraneHipError("rim_slope_match_out: rim_slope_match_center and rim_slope_match_normal must be finite")
    if normal is None or float(np.linalg.norm(normal)) < 1e-15:
        raise L.MembraneHipError("rim_slope_match_out with a non-zero rim_slope_match_strength and without a non-zero "
                                 "rim_slope_match_normal (SVD plane fit of the rim rows) is outside the HIP hot path")
    for name, rows in (("a rim", rim), ("an outer", outer), ("a disk", disk)):
        if rows.size > L.MS_RIM_MATCH_MAX_ROWS:
            raise L.MembraneHipError(f"rim_slope_match_out: {name} ring of {rows.size} rows is above the "
                                     f"{L.MS_RIM_MATCH_MAX_ROWS} the device orders")
    return {"rim": rim.astype(np.int32), "outer": outer.astype(np.int32), "disk": disk.astype(np.int32),
            "center": tuple(float(v) for v in center), "normal": tuple(float(v) for v in normal), "strength": k}


def rim_match_key(prm):
    """Hashable identity of rim_match_params' result (the Minimizer re-uploads when it changes)."""
    if prm is None:
        return None
    return (prm["rim"].tobytes(), prm["outer"].tobytes(), prm["disk"].tobytes(), prm["center"], prm["normal"],
            prm["strength"])


def evaluate_rim_match(mesh, global_params, param_resolver, *, positions, tilts_in, tilts_out, grad_arr,
                       tilt_in_grad_arr, tilt_out_grad_arr) -> float:
    """rim_slope_match_out on caller arrays (H2D/D2H per call: the parity seam, not the hot loop): energy; shape gradient
    ADDED into ``grad_arr``, tilt gradients ADDED into ``tilt_in_grad_arr`` / ``tilt_out_grad_arr`` (each optional).
    0.0 with nothing written exactly where the reference returns early."""
    prm = rim_match_params(mesh, param_resolver, global_params)
    if prm is None:
        return 0.0
    nv = len(mesh.vertex_ids)
    fields = {}
    for lf, t in (("in", tilts_in), ("out", tilts_out)):
        if t is None:
            t = mesh.tilts_in_view() if lf == "in" else mesh.tilts_out_view()
        t = np.ascontiguousarray(t, dtype=np.float64)
        if t.shape != (nv, 3):
            raise ValueError(f"tilts_{lf} must have shape (N_vertices, 3)")
        fields[lf] = t
    for name, arr in (("tilt_in_grad_arr", tilt_in_grad_arr), ("tilt_out_grad_arr", tilt_out_grad_arr)):
        if arr is not None and np.shape(arr) != (nv, 3):
            raise ValueError(f"{name} must have shape (N_vertices, 3)")
    mir = mirror_for(mesh)
    dm = mir.sync(positions=None if positions is mesh.positions_view() else positions)
    for lf in ("in", "out"):
        dm.set_leaflet_tilts(lf, fields[lf], tilt_modulus=0.0, smoothness=0.0)
    mir._leaflet_keys = {}  # foreign arrays were uploaded
    dm.set_rim_match(**prm)
    dm.set_params(modules=L.MS_MOD_RIM_SLOPE_MATCH_OUT)
    if grad_arr is not None:
        e, g = dm.energy_and_gradient(want_grad=True, raw=True)
        grad_arr += g
        E = float(e[3])
    else:
        E = float(dm.energy()[3])
    if tilt_in_grad_arr is not None or tilt_out_grad_arr is not None:
        _e, gi, go = dm.leaflet_tilt_energy_and_gradient(want_gradient=True)
        if tilt_in_grad_arr is not None:
            tilt_in_grad_arr += gi
        if tilt_out_grad_arr is not None:
            tilt_out_grad_arr += go
    return E


def rim_match_numpy(positions, tilts_in, tilts_out, *, rim, outer, disk, center, normal, strength, shape_gradient=True):
    """The module's tables and sums restated in NumPy, the way k_rsm_geom / k_rsm_apply form them (rank-by-counting for
    the order, a binary search for the pairing, the first rim entry of every outer row, a row's terms added in np.add.at's
    order) -> dict with E, E_out, E_in, grad, tilt_in_grad, tilt_out_grad, the ordered rows and the record.  Host-side
    check of the device's scheme against the fixtures; not on any hot path."""
    x = np.asarray(positions, dtype=np.float64)
    c = np.asarray(center, dtype=np.float64).reshape(3)
    n = np.asarray(normal, dtype=np.float64).reshape(3)
    n = n / np.linalg.norm(n)
    trial = np.array([0.0, 1.0, 0.0]) if abs(n[0]) > 0.9 else np.array([1.0, 0.0, 0.0])
    u = trial - float(trial @ n) * n
    u = u / np.linalg.norm(u)
    v = np.cross(n, u)
    v = v / np.linalg.norm(v)

    def order(rows):
        rows = np.asarray(rows, dtype=np.int64)
        rel = x[rows] - c
        key = np.arctan2(rel @ v, rel @ u)
        idx = np.arange(len(rows))
        before = (key[None, :] < key[:, None]) | ((key[None, :] == key[:, None]) & (idx[None, :] < idx[:, None]))
        out = np.empty(len(rows), np.int64)
        out[before.sum(axis=1)] = rows
        return out

    def in_plane(p):
        r = p - c
        return r - (r @ n)[:, None] * n

    def arc_weight(p):
        return 0.5 * (np.linalg.norm(np.roll(p, -1, axis=0) - p, axis=1) + np.linalg.norm(p - np.roll(p, 1, axis=0), axis=1))

    def arc_params(p):
        seg = np.linalg.norm(np.roll(p, -1, axis=0) - p, axis=1)
        run, s = 0.0, np.zeros(len(p))
        for q in range(len(p)):
            s[q] = run
            run += seg[q]
        return (s / run if run > 0.0 else np.zeros(len(p))), run

    orim, oout = order(rim), order(outer)
    odisk = order(disk) if len(disk) else np.zeros(0, np.int64)
    nr, no, nd = len(orim), len(oout), len(odisk)
    nv = len(x)
    out = {"E": 0.0, "E_out": 0.0, "E_in": 0.0, "grad": np.zeros((nv, 3)), "tilt_in_grad": np.zeros((nv, 3)),
           "tilt_out_grad": np.zeros((nv, 3)), "rim_order": orim, "outer_order": oout, "disk_order": odisk,
           "n_valid": 0, "contributes": False, "local_disk": nd > 0 and nd == nr, "sum_wd": 0.0}
    p_rim, p_out = x[orim], x[oout]
    idx0, w0, w1 = np.arange(nr), np.ones(nr), np.zeros(nr)
    paired, interp = True, nr != no
    if interp:
        s_out, total_out = arc_params(p_out)
        s_rim, total_rim = arc_params(p_rim)
        paired = total_rim > 0.0 and total_out > 0.0 and no >= 2
        if paired:
            for q in range(nr):
                lo, hi = 0, no
                while lo < hi:
                    mid = (lo + hi) >> 1
                    if s_out[mid] <= s_rim[q]:
                        lo = mid + 1
                    else:
                        hi = mid
                i1 = lo % no
                i0 = (i1 + no - 1) % no
                s0, s1, st = s_out[i0], s_out[i1], s_rim[q]
                if s1 <= s0:
                    s1 += 1.0
                if st < s0:
                    st += 1.0
                t = (st - s0) / (s1 - s0) if s1 - s0 > 1e-12 else 0.0
                idx0[q], w0[q], w1[q] = i0, 1.0 - t, t
    if not paired:
        return out
    idx1 = (idx0 + 1) % no if interp else idx0
    po = p_out[idx0] * w0[:, None] + p_out[idx1] * w1[:, None] if interp else p_out[idx0]
    r = in_plane(p_rim)
    rl = np.linalg.norm(r, axis=1)
    good = rl > 1e-12
    rhat = np.where(good[:, None], r / np.where(good, rl, 1.0)[:, None], 0.0)
    dr = np.linalg.norm(in_plane(po), axis=1) - rl
    ok = np.abs(dr) > 1e-8
    phi = np.where(ok, ((po - c) @ n - (p_rim - c) @ n) / np.where(ok, dr, 1.0), 0.0)
    valid = ok & good & np.isfinite(phi)
    out["n_valid"] = int(valid.sum())
    if not valid.any():
        return out
    out["contributes"] = True
    w = np.where(valid, arc_weight(p_rim), 0.0)
    phi = np.where(valid, phi, 0.0)
    inv_dr = np.where(valid, 1.0 / np.where(valid, dr, 1.0), 0.0)
    k = float(strength)
    tin, tout = np.asarray(tilts_in, dtype=np.float64), np.asarray(tilts_out, dtype=np.float64)
    dif = np.where(valid, np.einsum("ij,ij->i", tout[orim], rhat) - phi, 0.0)
    dif_in = np.zeros(nr)
    has_in = False
    if nd:
        rd = in_plane(x[odisk])
        rdl = np.linalg.norm(rd, axis=1)
        gd = rdl > 1e-12
        rhat_d = np.where(gd[:, None], rd / np.where(gd, rdl, 1.0)[:, None], 0.0)
        th_d = np.einsum("ij,ij->i", tin[odisk], rhat_d)
        if out["local_disk"]:
            theta, has_in = th_d, True
        else:
            w_d = np.where(gd, arc_weight(x[odisk]), 0.0)
            out["sum_wd"] = float(w_d.sum())
            if out["sum_wd"] > 0.0:
                theta, has_in = float((w_d * th_d).sum() / out["sum_wd"]), True
        if has_in:
            dif_in = np.where(valid, np.einsum("ij,ij->i", tin[orim], rhat) - (theta - phi), 0.0)
    out["E_out"] = 0.5 * k * float((w * dif * dif).sum())
    out["E_in"] = 0.5 * k * float((w * dif_in * dif_in).sum()) if has_in else 0.0
    out["E"] = out["E_out"] + out["E_in"]
    out["tilt_out_grad"][orim] += (k * w * dif)[:, None] * rhat
    if has_in:
        out["tilt_in_grad"][orim] += (k * w * dif_in)[:, None] * rhat
        if out["local_disk"]:
            out["tilt_in_grad"][odisk] += (-k * w * dif_in)[:, None] * rhat_d
        else:
            out["tilt_in_grad"][odisk] += (-k * float((w * dif_in).sum())) * (w_d / out["sum_wd"])[:, None] * rhat_d
    if shape_gradient:
        gc = k * w * (dif - dif_in) * inv_dr
        out["grad"][orim] += gc[:, None] * n
        first0 = np.searchsorted(idx0, np.arange(no + 1), side="left")  # idx0 is monotone
        assert np.all(np.diff(idx0) >= 0)
        for j in range(no):
            for ps in range(2 if interp else 1):
                jj = j if ps == 0 else (j + no - 1) % no
                for q in range(first0[jj], first0[jj + 1]):
                    out["grad"][oout[j]] += (-gc[q] * n) * (w0[q] if ps == 0 else w1[q])
    return out


def splay_twist_params(param_resolver, global_params):
    """(k_splay, k_twist, divergence mode) of tilt_splay_twist_in (modules/energy/tilt_splay_twist_in.py:16-50), in the
    reference's order: ``tilt_splay_modulus_in`` else ``bending_modulus_in`` else ``bending_modulus`` (the fallback is
    taken on None only: an explicit 0.0 stays 0); ``tilt_twist_modulus_in`` else ``tilt_twist_modulus`` else 0; a
    negative modulus raises ValueError; ``tilt_divergence_mode_in`` else ``tilt_divergence_mode``, default native,
    anything but native / vertex_recovered raises ValueError."""
    val = _get(param_resolver, global_params, "tilt_splay_modulus_in")
    if val is None:
        val = _get(param_resolver, global_params, "bending_modulus_in")
    if val is None:
        val = _get(param_resolver, global_params, "bending_modulus")
    k_splay = float(val or 0.0)
    if k_splay < 0.0:
        raise ValueError("tilt_splay_modulus_in must be non-negative.")
    val = _get(param_resolver, global_params, "tilt_twist_modulus_in")
    if val is None:
        val = _get(param_resolver, global_params, "tilt_twist_modulus")
    k_twist = float(val or 0.0)
    if k_twist < 0.0:
        raise ValueError("tilt_twist_modulus_in must be non-negative.")
    val = _get(param_resolver, global_params, "tilt_divergence_mode_in")
    if val is None:
        val = _get(param_resolver, global_params, "tilt_divergence_mode")
    mode = str(val or "native").strip().lower()
    if mode not in {"native", "vertex_recovered"}:
        raise ValueError("tilt_divergence_mode_in must be 'native' or 'vertex_recovered'.")
    return k_splay, k_twist, mode


def splay_twist_device_params(param_resolver, global_params, mesh=None):
    """(k_splay, k_twist) for DeviceMesh.set_tilt_splay_twist, or None when the module contributes nothing (both moduli
    0: tilt_splay_twist_in.py:134-135).  Everything is resolved before that early return, as in the reference (:128-133):
    a bad mode or transport model raises with both moduli 0 as well.  The vertex_recovered divergence is not on the
    device path."""
    k_splay, k_twist, mode = splay_twist_params(param_resolver, global_params)
    check_supported(global_params if global_params is not None else {}, mesh)
    if k_splay == 0.0 and k_twist == 0.0:
        return None
    if mode != "native":
        raise L.MembraneHipError(f"tilt_splay_twist_in with tilt_divergence_mode {mode!r} is outside the HIP hot path "
                                 "(only the native divergence is on the device)")
    return k_splay, k_twist


def evaluate_splay_twist(mesh, global_params, param_resolver, *, positions, tilts_in, tilt_in_grad_arr) -> float:
    """tilt_splay_twist_in on caller arrays (H2D/D2H per call: the parity seam, not the hot loop): energy; tilt gradient
    ADDED into ``tilt_in_grad_arr`` (optional).  No shape gradient: the caller's ``grad_arr`` is never touched."""
    prm = splay_twist_device_params(param_resolver, global_params, mesh)
    if prm is None:
        return 0.0
    tri, _f = mesh.triangle_row_cache()
    if tri is None or len(tri) == 0:
        return 0.0
    nv = len(mesh.vertex_ids)
    if tilts_in is None:
        tilts_in = mesh.tilts_in_view()
    tilts_in = np.ascontiguousarray(tilts_in, dtype=np.float64)
    if tilts_in.shape != (nv, 3):
        raise ValueError("tilts_in must have shape (N_vertices, 3)")
    if tilt_in_grad_arr is not None and np.shape(tilt_in_grad_arr) != (nv, 3):
        raise ValueError("tilt_in_grad_arr must have shape (N_vertices, 3)")
    mir = mirror_for(mesh)
    dm = mir.sync(positions=None if positions is mesh.positions_view() else positions)
    dm.set_leaflet_tilts("in", tilts_in, tilt_modulus=0.0, smoothness=0.0)
    dm.set_leaflet_tilts("out", np.zeros((nv, 3)), tilt_modulus=0.0, smoothness=0.0)
    mir._leaflet_keys = {}  # foreign arrays were uploaded
    dm.set_tilt_splay_twist(*prm)
    dm.set_params(modules=L.MS_MOD_TILT_SPLAY_TWIST_IN)
    if tilt_in_grad_arr is None:
        return float(dm.energy()[3])
    E, gi, _go = dm.leaflet_tilt_energy_and_gradient(want_gradient=True)
    tilt_in_grad_arr += gi
    return float(E)


def check_bt_supported(global_params) -> None:
    mode = str(global_params.get("bending_gradient_mode", "analytic") or "analytic").strip().lower()
    if mode != "analytic":
        raise L.MembraneHipError("bending_tilt_in/out: only bending_gradient_mode=analytic is on the HIP hot path")


def device_params(param_resolver, global_params, leaflet: str) -> dict:
    return {"tilt_modulus": tilt_modulus(param_resolver, global_params, leaflet),
            "mass_mode": tilt_mass_mode(param_resolver, global_params, leaflet),
            "smoothness": smoothness_rigidity(param_resolver, global_params, leaflet),
            "precond_smoothness": precond_smoothness(param_resolver, global_params, leaflet)}


def evaluate(mesh, global_params, param_resolver, *, kind: str, leaflet: str, positions, tilts, grad_arr,
             tilt_grad_arr) -> float:
    """One leaflet module on caller arrays (H2D/D2H per call: the parity seam, not the hot loop)."""
    check_supported(global_params, mesh)
    absent = absent_out_rows(mesh, global_params)
    if kind == "bt" and leaflet == "out" and absent is not None:
        raise L.MembraneHipError(BT_OUT_ABSENT_MESSAGE)
    tri, _f = mesh.triangle_row_cache()
    if tri is None or len(tri) == 0:
        return 0.0
    nv = len(mesh.vertex_ids)
    if tilts is None:
        tilts = mesh.tilts_in_view() if leaflet == "in" else mesh.tilts_out_view()
    tilts = np.ascontiguousarray(tilts, dtype=np.float64)
    if tilts.shape != (nv, 3):
        raise ValueError(f"tilts for leaflet '{leaflet}' must have shape (N_vertices, 3)")
    if tilt_grad_arr is not None and np.shape(tilt_grad_arr) != (nv, 3):
        raise ValueError(f"tilt_grad_arr for leaflet '{leaflet}' must have shape (N_vertices, 3)")
    params = device_params(param_resolver, global_params, leaflet)
    mir = mirror_for(mesh)
    dm = mir.sync(positions=None if positions is mesh.positions_view() else positions)
    other = "out" if leaflet == "in" else "in"
    dm.set_leaflet_tilts(leaflet, tilts, **params)
    dm.set_leaflet_tilts(other, np.zeros((nv, 3)), tilt_modulus=0.0, smoothness=0.0)
    mir._leaflet_keys = {}  # foreign arrays were uploaded
    if leaflet == "out":
        mir.set_absent_out(absent)  # (tilt_out and tilt_smoothness_out read it; a mask of an earlier call is cleared)
    if kind == "bt":
        check_bt_supported(global_params)
        dm.set_leaflet_bending(leaflet, *bending_params(mesh, global_params, leaflet))
    if kind == "disk":
        prm = disk_target_params(mesh, param_resolver, global_params, leaflet)
        if prm is None:
            return 0.0
        dm.set_leaflet_disk_target(leaflet, **prm)
    if kind == "rim":
        prm = rim_source_params(mesh, param_resolver, global_params, leaflet)
        if prm is None:
            return 0.0
        if prm["follow"]:
            # tilt_rim_source_in.py:318: the followed center is read from the MESH, whatever `positions` the caller
            # evaluates on -- a fixed frame for this one call
            rows = np.unique(np.concatenate([prm["tail"], prm["head"]]))
            center = np.mean(np.asarray(mesh.positions_view(), dtype=np.float64)[rows], axis=0)
            prm = dict(prm, center=tuple(float(v) for v in center), follow=False)
        dm.set_leaflet_rim_source(leaflet, **prm)
        dm.set_params(modules=LEAFLET_BITS[(kind, leaflet)])
        # no shape gradient (grad_arr stays as it is); the tilt gradient is the coefficient field itself
        E = float(dm.energy()[3])
        if tilt_grad_arr is not None:
            _e, gi, go = dm.leaflet_tilt_energy_and_gradient(want_gradient=True)
            tilt_grad_arr += gi if leaflet == "in" else go
        return E
    dm.set_params(modules=LEAFLET_BITS[(kind, leaflet)])
    if kind == "disk":
        if grad_arr is not None:
            e, g = dm.energy_and_gradient(want_grad=True, raw=True)
            grad_arr += g
            E = float(e[3])
        else:
            E = float(dm.energy()[3])
    elif kind == "bt":
        if grad_arr is not None:
            e, g = dm.energy_and_gradient(want_grad=True, raw=True)
            grad_arr += g
            E = float(e[1])
        else:
            E = float(dm.energy()[1])
    elif grad_arr is not None and kind == "tilt":
        e, g = dm.energy_and_gradient(want_grad=True, raw=True)
        grad_arr += g
        E = float(e[3])
    else:
        E = float(dm.energy()[3])
    if tilt_grad_arr is not None:
        # the module's own mass mode (tilt_leaflet.py:116-150): lumped k A/3 t_k or consistent k A/12 (2 t_k + t_a + t_b)
        _e, gi, go = dm.leaflet_tilt_energy_and_gradient(want_gradient=True, module_form=(kind == "tilt"))
        tilt_grad_arr += gi if leaflet == "in" else go
    return E


# --- leaflet absence: the masked modules restated in NumPy -------------------------------------------------------------
BT_OUT_ABSENT_MESSAGE = ("bending_tilt_out next to a non-empty leaflet_out_absent_presets mask is outside the HIP hot "
                         "path (the follow-up to the mask: masked normals and effective areas in the energy pass's "
                         "per-vertex record and in the leaflet shape-gradient instance)")


def _facet_geometry(positions, tri):
    x = np.asarray(positions, dtype=np.float64)
    tri = np.asarray(tri, dtype=np.int64).reshape(-1, 3)
    v0, v1, v2 = x[tri[:, 0]], x[tri[:, 1]], x[tri[:, 2]]
    n = np.cross(v1 - v0, v2 - v0)
    return tri, v0, v1, v2, n, np.linalg.norm(n, axis=1)


def masked_vertex_areas(positions, tri, absent=None) -> np.ndarray:
    """Barycentric vertex areas over the kept facets (tilt_relaxation.py:31-45, :681-697): what a relaxation hands the
    outer leaflet's magnitude term and the k_t A_v part of its Jacobi diagonal."""
    tri, _v0, _v1, _v2, _n, nn = _facet_geometry(positions, tri)
    out = np.zeros(len(np.asarray(positions)), dtype=np.float64)
    if absent is not None and np.any(absent):
        keep = kept_facets(tri, absent)
        tri, nn = tri[keep], nn[keep]
    a3 = (0.5 * nn) / 3.0
    for k in range(3):
        np.add.at(out, tri[:, k], a3)
    return out


def tilt_leaflet_numpy(positions, tri, tilts, *, k_tilt, mass_mode="lumped", absent=None):
    """tilt_in / tilt_out (tilt_leaflet.py:41-169) on the facets kept by ``absent`` -> dict with E, grad (shape
    gradient) and tilt_grad.  Host-side statement of what k_tilt sums under a mask; not on any hot path."""
    tri, v0, v1, v2, n, nn = _facet_geometry(positions, tri)
    t = np.asarray(tilts, dtype=np.float64)
    nv = len(t)
    out = {"E": 0.0, "grad": np.zeros((nv, 3)), "tilt_grad": np.zeros((nv, 3))}
    if k_tilt == 0.0 or len(tri) == 0:
        return out
    keep = nn >= 1e-12
    if absent is not None and np.any(absent):
        keep &= kept_facets(tri, absent)
    if not np.any(keep):
        return out
    tri, v0, v1, v2, n, nn = tri[keep], v0[keep], v1[keep], v2[keep], n[keep], nn[keep]
    area = 0.5 * nn
    t0, t1, t2 = t[tri[:, 0]], t[tri[:, 1]], t[tri[:, 2]]
    dot = lambda a, b: np.einsum("ij,ij->i", a, b)  # noqa: E731
    sq = dot(t0, t0) + dot(t1, t1) + dot(t2, t2)
    if mass_mode == "consistent":
        coeff = (k_tilt / 12.0) * (sq + dot(t0, t1) + dot(t1, t2) + dot(t2, t0))
        f = (k_tilt * area / 12.0)[:, None]
        rows = (f * (2.0 * t0 + t1 + t2), f * (2.0 * t1 + t2 + t0), f * (2.0 * t2 + t0 + t1))
    else:
        coeff = 0.5 * k_tilt * (sq / 3.0)
        f = (k_tilt * area / 3.0)[:, None]
        rows = (f * t0, f * t1, f * t2)
    out["E"] = float(np.dot(coeff, area))
    nh = n / nn[:, None]
    shape = (0.5 * np.cross(nh, v2 - v1), 0.5 * np.cross(nh, v0 - v2), 0.5 * np.cross(nh, v1 - v0))
    for k in range(3):
        np.add.at(out["tilt_grad"], tri[:, k], rows[k])
        np.add.at(out["grad"], tri[:, k], coeff[:, None] * shape[k])
    return out


def tilt_smoothness_numpy(positions, tri, tilts, *, k_smooth, absent=None):
    """tilt_smoothness_in / _out (tilt_smoothness.py:84-198 with the weights of tilt_smoothness_utils.py:17-76): the
    cotangent Dirichlet energy over the facets kept by ``absent`` -> dict with E and tilt_grad (no shape gradient)."""
    tri, v0, v1, v2, _n, nn = _facet_geometry(positions, tri)
    t = np.asarray(tilts, dtype=np.float64)
    out = {"E": 0.0, "tilt_grad": np.zeros((len(t), 3))}
    if k_smooth == 0.0 or len(tri) == 0:
        return out
    if absent is not None and np.any(absent):
        keep = kept_facets(tri, absent)
        tri, v0, v1, v2, nn = tri[keep], v0[keep], v1[keep], v2[keep], nn[keep]
    if len(tri) == 0:
        return out
    dot = lambda a, b: np.einsum("ij,ij->i", a, b)  # noqa: E731
    ad = np.maximum(nn, 1e-12)  # (compute_curvature_data: area_doubled clamped)
    c0, c1, c2 = dot(v1 - v0, v2 - v0) / ad, dot(v2 - v1, v0 - v1) / ad, dot(v0 - v2, v1 - v2) / ad
    t0, t1, t2 = t[tri[:, 0]], t[tri[:, 1]], t[tri[:, 2]]
    d12, d20, d01 = t1 - t2, t2 - t0, t0 - t1
    out["E"] = float(0.25 * k_smooth * np.sum(c0 * dot(d12, d12) + c1 * dot(d20, d20) + c2 * dot(d01, d01)))
    hk = 0.5 * k_smooth
    np.add.at(out["tilt_grad"], tri[:, 0], hk * (c2[:, None] * d01 - c1[:, None] * d20))
    np.add.at(out["tilt_grad"], tri[:, 1], hk * (c0[:, None] * d12 - c2[:, None] * d01))
    np.add.at(out["tilt_grad"], tri[:, 2], hk * (c1[:, None] * d20 - c0[:, None] * d12))
    return out
