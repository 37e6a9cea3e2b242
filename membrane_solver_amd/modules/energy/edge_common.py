"""What the edge-energy plugins (line_tension, edge_length_penalty) share on the HIP path: the triangle-side check of
their edges, the marshalling of the library's table builders, and the plugin entry points' bodies."""

from __future__ import annotations

import numpy as np

from ... import _lib as L
from ...geometry.mesh import mirror_for


def check_triangle_sides(name: str, noun: str, tri_rows, nv: int, tail, head, numbers=None) -> None:
    """An edge the module ``name`` charges (``noun``: "tagged" / "charged") must be a side of some triangle: the
    reference's minimum edge length (the line search's safe step) runs over all edges, the device's over triangle
    sides, so an edge outside the triangulation would change the search silently."""
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
        raise L.MembraneHipError(f"{name}: {noun} edge {which} (rows {int(t[k])}, {int(h[k])}) is not a side of "
                                 "any triangle; edges outside the triangulation are outside the HIP hot path")


def host_tables(entry: str, col_key: str, nv: int, iperm, tail, head, col, *extra):
    """The device tables as the library's ``entry`` (ms_line_tables_host / ms_edge_penalty_tables_host) builds them:
    the edge table {tail, head, <col_key>} and the vertex -> edge CSR {vrow, off, other, csr_<col_key>}, rows in the
    library's order (``iperm``: external row -> library row).  ``extra`` goes to the entry point behind the column."""
    ip = np.ascontiguousarray(np.asarray(iperm, dtype=np.int32).reshape(-1))
    t = np.ascontiguousarray(np.asarray(tail, dtype=np.int32).reshape(-1))
    h = np.ascontiguousarray(np.asarray(head, dtype=np.int32).reshape(-1))
    c = np.ascontiguousarray(np.asarray(col, dtype=np.float64).reshape(-1))
    n = len(t)
    cnt = np.zeros(2, dtype=np.int32)
    et, eh, ec = np.zeros(n + 1, np.int32), np.zeros(n + 1, np.int32), np.zeros(n + 1)
    vrow, off = np.zeros(2 * n + 1, np.int32), np.zeros(2 * n + 2, np.int32)
    other, oc = np.zeros(2 * n + 1, np.int32), np.zeros(2 * n + 1)
    i32 = lambda a: a.ctypes.data_as(L._I32)  # noqa: E731
    d = lambda a: a.ctypes.data_as(L._D)  # noqa: E731
    rc = getattr(L.lib(), entry)(int(nv), i32(ip), n, i32(t), i32(h), d(c), *extra, i32(cnt), i32(et), i32(eh), d(ec),
                                 i32(vrow), i32(off), i32(other), d(oc))
    L.check(rc, None, entry)
    ne, nt = int(cnt[0]), int(cnt[1])
    return {"tail": et[:ne].copy(), "head": eh[:ne].copy(), col_key: ec[:ne].copy(), "vrow": vrow[:nt].copy(),
            "off": off[:nt + 1].copy(), "other": other[:2 * ne].copy(), "csr_" + col_key: oc[:2 * ne].copy()}


def compute_energy_and_gradient_array(upload, module_bit: int, mesh, global_params, positions, grad_arr) -> float:
    """The module alone on the device: ``upload(mesh, global_params, dm)`` hands its edges over (False: nothing is
    charged, the energy is 0.0 as in the reference), then one evaluation with ``module_bit``; the raw gradient is added
    into ``grad_arr`` when one is given."""
    mir = mirror_for(mesh)
    dm = mir.sync(positions=None if positions is mesh.positions_view() else positions)
    if not upload(mesh, global_params, dm):
        return 0.0
    dm.set_params(modules=module_bit)
    if grad_arr is not None:
        e, g = dm.energy_and_gradient(want_grad=True, raw=True)
        np.add(grad_arr, g, out=grad_arr)
    else:
        e = dm.energy()
    return float(e[0])


def compute_energy_and_gradient(array_fn, mesh, global_params, param_resolver, compute_gradient: bool):
    """The dict-returning plugin entry point over a module's ``compute_energy_and_gradient_array``."""
    positions = mesh.positions_view()
    grad_arr = np.zeros_like(positions) if compute_gradient else None
    E = array_fn(mesh, global_params, param_resolver, positions=positions, index_map=mesh.vertex_index_to_row,
                 grad_arr=grad_arr)
    if not compute_gradient:
        return float(E), {}
    return float(E), {int(vid): grad_arr[row].copy() for row, vid in enumerate(mesh.vertex_ids)
                      if np.any(grad_arr[row])}
