"""``tilt_thetaB_boundary_in``: the hard boundary condition ``t_in . d = theta_B`` on an inclusion's ring of vertices.

Drop-in for the reference's modules/constraints/tilt_thetaB_boundary_in.py.  The ring is the set of vertices whose option
``rim_slope_match_group``, ``tilt_thetaB_group`` or ``tilt_thetaB_group_in`` equals the group ``tilt_thetaB_group_in``
(fallback ``rim_slope_match_disk_group``), in ``vertex_ids`` order.  Per row, on the positions handed in::

    r = (p - c) - ((p - c) . n) n          c = tilt_thetaB_center, n = tilt_thetaB_normal normalised
    d = r_hat - (r_hat . N_v) N_v          N_v the unit vertex normal; d normalised

a row with ``|r| <= 1e-12`` or ``|d| <= 1e-12`` is dropped.  The projection ``t_in <- t_in + (theta_B - t_in . d) d``
(``theta_B = tilt_thetaB_value or 0``) acts on the kept rows that are not ``tilt_fixed_in``; the same rows give one sparse
constraint row ``(row, d)`` each, against which the relaxation projects the inner tilt gradient.  The module has no
``enforce_constraint``: alone it never makes the line search enforce anything.

The functions below are the NumPy restatement on host arrays (the parity seam).  On the device the ring, the frame and a
ring row -> facet table go up once (``device_params`` -> ``DeviceMesh.set_thetab_boundary``); k_tbb_geom forms ``d`` and
k_tbb_apply enforces or projects (csrc/ms_thetab_bnd.hip).  Outside the device path: a missing ``tilt_thetaB_normal``
(the reference fits a plane to the ring), the group ``"disk"`` without ``parity_trace_layer_radius`` (the reference then
grows the ring from the positions of every call) and ``tilt_thetaB_optimize``.
"""

from __future__ import annotations

import numpy as np

from ... import _lib as L
from ...geometry.mesh import tilt_fixed_mask

NAME = "tilt_thetaB_boundary_in"
_TAG_KEYS = ("rim_slope_match_group", "tilt_thetaB_group", "tilt_thetaB_group_in")


def _gp(global_params, key):
    return None if global_params is None else global_params.get(key)


def resolve_group(global_params):
    raw = _gp(global_params, "tilt_thetaB_group_in")
    if raw is None:
        raw = _gp(global_params, "rim_slope_match_disk_group")
    if raw is None:
        return None
    group = str(raw).strip()
    return group if group else None


def group_rows(mesh, group: str) -> np.ndarray:
    """Rows tagged with ``group`` by any of the three keys, in vertex_ids order: vertex options of a reference Mesh, or
    ``vertex_options`` of an array mesh."""
    tagged = lambda o: any(o.get(k) == group for k in _TAG_KEYS)  # noqa: E731
    verts = getattr(mesh, "vertices", None)
    row_of = mesh.vertex_index_to_row
    rows = []
    if isinstance(verts, dict):
        for vid in mesh.vertex_ids:
            if tagged(getattr(verts[int(vid)], "options", None) or {}):
                row = row_of.get(int(vid))
                if row is not None:
                    rows.append(int(row))
    else:
        vopts = getattr(mesh, "vertex_options", None) or {}
        for vid in mesh.vertex_ids:
            row = row_of.get(int(vid))
            if row is not None and tagged(vopts.get(int(row)) or {}):
                rows.append(int(row))
    return np.asarray(rows, dtype=np.int64)


def thetab_value(global_params) -> float:
    return float(_gp(global_params, "tilt_thetaB_value") or 0.0)


def frame(global_params):
    """-> (center (3,), unit normal (3,)); the refusals every lane shares"""
    center = _gp(global_params, "tilt_thetaB_center")
    center = np.asarray([0.0, 0.0, 0.0] if center is None else center, dtype=float).reshape(3)
    raw = _gp(global_params, "tilt_thetaB_normal")
    normal = None if raw is None else np.asarray(raw, dtype=float).reshape(3)
    if not np.all(np.isfinite(center)) or (normal is not None and not np.all(np.isfinite(normal))) \
            or not np.isfinite(thetab_value(global_params)):
        raise L.MembraneHipError(f"{NAME}: tilt_thetaB_center, tilt_thetaB_normal and tilt_thetaB_value must be finite")
    if normal is None or float(np.linalg.norm(normal)) < 1e-15:
        raise L.MembraneHipError(f"{NAME} without a non-zero tilt_thetaB_normal (SVD plane fit of the ring rows) is "
                                 "outside the HIP hot path")
    return center, normal / float(np.linalg.norm(normal))


def ring(mesh, global_params):
    """-> the ring's rows, or None where the module does nothing (no group, no tagged row).  Refused: the group "disk"
    without parity_trace_layer_radius, tilt_thetaB_optimize."""
    group = resolve_group(global_params)
    if group is None:
        return None
    rows = group_rows(mesh, group)
    if rows.size == 0:
        return None
    if group == "disk" and _gp(global_params, "parity_trace_layer_radius") is None:
        raise L.MembraneHipError(f"{NAME} with the group 'disk' and no parity_trace_layer_radius (the ring is then grown "
                                 "from the positions of every call) is outside the HIP hot path")
    if bool(_gp(global_params, "tilt_thetaB_optimize") or False):
        raise L.MembraneHipError(f"{NAME} with tilt_thetaB_optimize is outside the HIP hot path")
    return rows


def unit_vertex_normals(positions: np.ndarray, tri: np.ndarray) -> np.ndarray:
    tn = np.cross(positions[tri[:, 1]] - positions[tri[:, 0]], positions[tri[:, 2]] - positions[tri[:, 0]])
    normals = np.zeros_like(positions)
    for k in range(3):
        np.add.at(normals, tri[:, k], tn)
    lens = np.linalg.norm(normals, axis=1)
    mask = lens >= 1e-12
    normals[mask] /= lens[mask][:, None]
    return normals


def directions(mesh, global_params, *, positions: np.ndarray):
    """-> (rows (n,), d (n,3), keep (n,) bool) of every ring row on ``positions`` (d is 0 where the row is dropped), or
    None where the module does nothing."""
    rows = ring(mesh, global_params)
    if rows is None:
        return None
    center, normal = frame(global_params)
    positions = np.asarray(positions, dtype=float)
    rel = positions[rows] - center[None, :]
    r = rel - (rel @ normal)[:, None] * normal[None, :]
    r_len = np.linalg.norm(r, axis=1)
    good = r_len > 1e-12
    r_hat = np.zeros_like(r)
    r_hat[good] = r[good] / r_len[good][:, None]
    tri = np.asarray(mesh.triangle_row_cache()[0])
    nrm = unit_vertex_normals(positions, tri)[rows]
    d = r_hat - np.einsum("ij,ij->i", r_hat, nrm)[:, None] * nrm
    d_len = np.linalg.norm(d, axis=1)
    keep = good & (d_len > 1e-12)
    d[keep] /= d_len[keep][:, None]
    d[~keep] = 0.0
    return rows, d, keep


def _free_rows(mesh, global_params, positions):
    data = directions(mesh, global_params, positions=positions)
    if data is None:
        return None
    rows, d, keep = data
    free = keep & ~tilt_fixed_mask(mesh, "tilt_fixed_in")[rows]
    if not np.any(free):
        return None
    return rows[free], d[free]


def constraint_gradients(mesh, global_params=None) -> None:
    """No shape constraint: the module acts on the tilts only."""
    return None


def constraint_gradients_array(mesh, global_params=None, *, positions=None, index_map=None) -> None:
    """No shape constraint: the module acts on the tilts only."""
    return None


def constraint_gradients_tilt_rows_array(mesh, global_params, *, positions, index_map=None, tilts_in=None,
                                         tilts_out=None):
    """One sparse row ``((rows [1], vecs [1,3]), None)`` per kept ring row that is not tilt_fixed_in, or None."""
    data = _free_rows(mesh, global_params, positions)
    if data is None:
        return None
    return [((np.asarray([int(r)], dtype=int), np.asarray(v, dtype=float).reshape(1, 3)), None) for r, v in zip(*data)]


def constraint_gradients_tilt_array(mesh, global_params, *, positions, index_map=None, tilts_in=None, tilts_out=None):
    """The same rows as dense ``(g_in, None)`` pairs."""
    sparse = constraint_gradients_tilt_rows_array(mesh, global_params, positions=positions, index_map=index_map,
                                                  tilts_in=tilts_in, tilts_out=tilts_out)
    if not sparse:
        return None
    out = []
    for (rows, vecs), _none in sparse:
        g = np.zeros_like(np.asarray(positions, dtype=float))
        g[rows] += vecs
        out.append((g, None))
    return out


def project_gradient(tilt_in_grad_arr: np.ndarray, mesh, global_params, *, positions) -> None:
    """g_i <- g_i - ((g_i . d_i) / (d_i . d_i)) d_i on the constraint's rows, in place: C^T (C C^T)^-1 C with disjoint
    rows."""
    data = _free_rows(mesh, global_params, positions)
    if data is None:
        return
    rows, d = data
    g = tilt_in_grad_arr[rows]
    coef = np.einsum("ij,ij->i", g, d) / np.einsum("ij,ij->i", d, d)
    tilt_in_grad_arr[rows] = g - coef[:, None] * d


def enforce_tilt_constraint(mesh, global_params=None, **_kwargs) -> None:
    """t_in <- t_in + (theta_B - t_in . d) d on the kept, free ring rows of the mesh's positions, in place."""
    data = _free_rows(mesh, global_params, mesh.positions_view())
    if data is None:
        return
    rows, d = data
    tilts_in = mesh.tilts_in_view()
    t = tilts_in[rows]
    new = t + (thetab_value(global_params) - np.einsum("ij,ij->i", t, d))[:, None] * d
    full = np.array(tilts_in, copy=True)
    full[rows] = new
    mesh.set_tilts_in_from_array(full)


# -- the device path ----------------------------------------------------------------------------------------------------
def device_params(mesh, global_params):
    """kwargs of DeviceMesh.set_thetab_boundary, or None where the module does nothing."""
    rows = ring(mesh, global_params)
    if rows is None:
        return None
    center, normal = frame(global_params)
    return {"rows": rows.astype(np.int32), "center": tuple(float(v) for v in center),
            "normal": tuple(float(v) for v in normal)}


def device_key(prm):
    """Hashable identity of device_params' result (theta_B is no part of it: it goes up with every configuration)."""
    return None if prm is None else (prm["rows"].tobytes(), prm["center"], prm["normal"])


def projection_schedule(global_params):
    """(cadence, interval) of tilt_projection_cadence / tilt_projection_interval, as the reference reads and rejects
    them."""
    cadence = str(_gp(global_params, "tilt_projection_cadence") or "per_step").strip().lower()
    if cadence not in {"per_step", "per_pass"}:
        raise ValueError("tilt_projection_cadence must be 'per_step' or 'per_pass'.")
    interval = int(_gp(global_params, "tilt_projection_interval") or 1)
    if interval < 1:
        raise ValueError("tilt_projection_interval must be >= 1.")
    return cadence, interval


def tables_host(nv: int, iperm, tri, rows):
    """The ring row -> incident facet CSR as the library builds it (ms_thetab_boundary_tables_host) -> (off, fv)"""
    i32 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.int32).reshape(-1))  # noqa: E731
    ptr = lambda a: (a if len(a) else np.zeros(1, np.int32)).ctypes.data_as(L._I32)  # noqa: E731
    ip, t, r = i32(iperm), i32(tri), i32(rows)
    off = np.zeros(len(r) + 1, np.int32)
    args = (int(nv), ptr(ip), len(t) // 3, ptr(t), len(r), ptr(r))
    L.check(L.lib().ms_thetab_boundary_tables_host(*args, off.ctypes.data_as(L._I32), None), None,
            "ms_thetab_boundary_tables_host")
    fv = np.zeros(max(3 * int(off[-1]), 1), np.int32)
    L.check(L.lib().ms_thetab_boundary_tables_host(*args, off.ctypes.data_as(L._I32), fv.ctypes.data_as(L._I32)), None,
            "ms_thetab_boundary_tables_host")
    return off, fv[:3 * int(off[-1])].reshape(-1, 3)


__all__ = ["constraint_gradients", "constraint_gradients_array", "constraint_gradients_tilt_array",
           "constraint_gradients_tilt_rows_array", "enforce_tilt_constraint"]
