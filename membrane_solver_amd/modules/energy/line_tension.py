"""Line-tension energy plugin on the HIP path.

Drop-in for modules/energy/line_tension.py:24-140: E = sum over the tagged edges of gamma |e|, gradient
-/+ gamma (x_h - x_t) / |e| at the tail / head, an edge shorter than 1e-15 contributing nothing.  On the device the
energy is added into the surface slot behind the energy pass and the gradient into G behind the gradient pass
(MS_MOD_LINE_TENSION, ms_set_line_tension).
"""

from __future__ import annotations

from typing import Dict

import numpy as np

from ... import _lib as L
from ...geometry.mesh import mirror_for
from ..constraints.pins import _entities


def edge_is_tagged(opts) -> bool:
    """line_tension.py:24-34: the edge's ``energy`` option is the string "line_tension", or a list / tuple that
    contains it, or the key ``line_tension`` is present in its options."""
    opts = opts or {}
    energy = opts.get("energy")
    has_line = False
    if isinstance(energy, str):
        has_line = energy == "line_tension"
    elif isinstance(energy, (list, tuple)):
        has_line = "line_tension" in energy
    return bool(has_line or "line_tension" in opts)


def has_edge_table(mesh) -> bool:
    """Whether the mesh carries edges at all: the reference's meshes always do (mesh.edges), an ArrayMesh only when
    it was built with ``edges=``.  Without them no edge can be tagged, and a deck that lists the module would run
    with a line energy of zero; the Minimizer refuses that deck instead."""
    if hasattr(mesh, "vertices") and isinstance(mesh.vertices, dict):
        return hasattr(mesh, "edges")
    return getattr(mesh, "edge_rows", None) is not None


def tagged_edges(mesh, global_params):
    """-> (tail rows, head rows, gamma, edge numbers) of the edges the reference's loop charges, in its iteration
    order: gamma is the edge's own ``line_tension`` option or else the global parameter (line_tension.py:117-122), a
    falsy gamma skips the edge (:123-124), an end without a row skips it (:125-128)."""
    _verts, edges, row_of, _fixed_of = _entities(mesh)
    default_gamma = float(global_params.get("line_tension", 0.0) or 0.0)
    tail, head, gam, num = [], [], [], []
    for k, (t, h, opts) in enumerate(edges):
        if not edge_is_tagged(opts):
            continue
        gamma = (opts or {}).get("line_tension", default_gamma)
        if not gamma:
            continue
        tr, hr = row_of.get(t), row_of.get(h)
        if tr is None or hr is None:
            continue
        tail.append(int(tr))
        head.append(int(hr))
        gam.append(float(gamma))
        num.append(k)
    return (np.asarray(tail, dtype=np.int32), np.asarray(head, dtype=np.int32), np.asarray(gam, dtype=np.float64),
            np.asarray(num, dtype=np.int64))


def check_triangle_sides(tri_rows, nv: int, tail, head, numbers=None) -> None:
    """A tagged edge must be a side of some triangle: the reference's minimum edge length (the line search's safe
    step) runs over all edges, the device's over triangle sides, so an edge outside the triangulation would change
    the search silently."""
    if len(tail) == 0:
        return
    tri = np.asarray(tri_rows, dtype=np.int64).reshape(-1, 3)
    a = np.concatenate([tri[:, 0], tri[:, 1], tri[:, 2]])
    b = np.concatenate([tri[:, 1], tri[:, 2], tri[:, 0]])
    sides = np.unique(np.minimum(a, b) * int(nv) + np.maximum(a, b))
    t, h = np.asarray(tail, dtype=np.int64), np.asarray(head, dtype=np.int64)
    bad = np.flatnonzero(~np.isin(np.minimum(t, h) * int(nv) + np.maximum(t, h), sides))
    if len(bad):
        k = int(bad[0])
        which = k if numbers is None else int(numbers[k])
        raise L.MembraneHipError(f"line_tension: tagged edge {which} (rows {int(t[k])}, {int(h[k])}) is not a side of "
                                 "any triangle; edges outside the triangulation are outside the HIP hot path")


def host_tables(nv: int, iperm, tail, head, gamma):
    """The device tables as the library builds them (ms_line_tables_host: the code ms_set_line_tension runs), for
    inspection: the edge table {tail, head, gamma} and the vertex -> edge CSR {vrow, off, other, gamma}, rows in the
    library's order (``iperm``: external row -> library row)."""
    ip = np.ascontiguousarray(np.asarray(iperm, dtype=np.int32).reshape(-1))
    t = np.ascontiguousarray(np.asarray(tail, dtype=np.int32).reshape(-1))
    h = np.ascontiguousarray(np.asarray(head, dtype=np.int32).reshape(-1))
    g = np.ascontiguousarray(np.asarray(gamma, dtype=np.float64).reshape(-1))
    n = len(t)
    cnt = np.zeros(2, dtype=np.int32)
    et, eh, eg = np.zeros(n + 1, np.int32), np.zeros(n + 1, np.int32), np.zeros(n + 1)
    vrow, off = np.zeros(2 * n + 1, np.int32), np.zeros(2 * n + 2, np.int32)
    other, og = np.zeros(2 * n + 1, np.int32), np.zeros(2 * n + 1)
    i32 = lambda a: a.ctypes.data_as(L._I32)  # noqa: E731
    d = lambda a: a.ctypes.data_as(L._D)  # noqa: E731
    rc = L.lib().ms_line_tables_host(int(nv), i32(ip), n, i32(t), i32(h), d(g), i32(cnt), i32(et), i32(eh), d(eg),
                                     i32(vrow), i32(off), i32(other), d(og))
    L.check(rc, None, "ms_line_tables_host")
    ne, nt = int(cnt[0]), int(cnt[1])
    return {"tail": et[:ne].copy(), "head": eh[:ne].copy(), "gamma": eg[:ne].copy(), "vrow": vrow[:nt].copy(),
            "off": off[:nt + 1].copy(), "other": other[:2 * ne].copy(), "csr_gamma": og[:2 * ne].copy()}


def upload(mesh, global_params, dm) -> bool:
    """Resolve the tagged edges and hand them to the device; False (tables cleared) when nothing is charged."""
    tail, head, gamma, num = tagged_edges(mesh, global_params)
    if len(tail) == 0:
        dm.set_line_tension()
        return False
    tri, _ = mesh.triangle_row_cache()
    check_triangle_sides(tri if tri is not None else np.zeros((0, 3), np.int32), dm.nv, tail, head, num)
    dm.set_line_tension(tail, head, gamma)
    return True


def compute_energy_and_gradient_array(mesh, global_params, param_resolver, *, positions: np.ndarray,
                                      index_map: Dict[int, int], grad_arr: np.ndarray) -> float:
    _ = index_map, param_resolver
    mir = mirror_for(mesh)
    dm = mir.sync(positions=None if positions is mesh.positions_view() else positions)
    if not upload(mesh, global_params, dm):
        return 0.0  # line_tension.py:113-115
    dm.set_params(modules=L.MS_MOD_LINE_TENSION)
    if grad_arr is not None:
        e, g = dm.energy_and_gradient(want_grad=True, raw=True)
        np.add(grad_arr, g, out=grad_arr)
    else:
        e = dm.energy()
    return float(e[0])


def compute_energy_and_gradient(mesh, global_params, param_resolver, *, compute_gradient: bool = True):
    positions = mesh.positions_view()
    grad_arr = np.zeros_like(positions) if compute_gradient else None
    E = compute_energy_and_gradient_array(mesh, global_params, param_resolver, positions=positions,
                                          index_map=mesh.vertex_index_to_row, grad_arr=grad_arr)
    if not compute_gradient:
        return float(E), {}
    return float(E), {int(vid): grad_arr[row].copy() for row, vid in enumerate(mesh.vertex_ids)
                      if np.any(grad_arr[row])}


__all__ = ["compute_energy_and_gradient", "compute_energy_and_gradient_array", "tagged_edges", "edge_is_tagged",
           "has_edge_table", "check_triangle_sides", "host_tables", "upload"]
