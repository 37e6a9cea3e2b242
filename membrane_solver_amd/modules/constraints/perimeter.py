"""Perimeter constraint plugin on the HIP path (modules/constraints/perimeter.py).

``enforce_constraint`` (:27-74) holds the total length of each edge list of the global ``perimeter_constraints`` at its
``target_perimeter``: the entries in list order, per entry up to ``max_iter`` passes x_v -= ((P - target) / (sum |g_v|^2 +
1e-18)) g_v on movable rows, g_v the listed edges' -dir at the tail and +dir at the head (:9-24), until |P - target| < tol
or sum |g_v|^2 < 1e-18.  All of it is one launch of one workgroup on the device (ms_project_perimeter).  The module has no
KKT row: it takes no part in the gradient projection (the reference's manager warns about that once).

Signed edge indices: on a reference ``Mesh`` index i is ``mesh.edges[abs(i)]``, reversed when negative (mesh.get_edge);
on an ``ArrayMesh`` +-(k + 1) is row k of ``edges=`` (the reference's ids start at 1).  The sign changes nothing.
"""

from __future__ import annotations

import math

import numpy as np

from ... import _lib as L
from ...geometry.mesh import mirror_for
from ..energy import edge_common as _edge
from ..energy.line_tension import has_edge_table
from .body_area import _write_back

NAME = "perimeter"


def _edge_rows(mesh, signed_idx):
    """(tail row, head row) of one signed edge index (mesh.get_edge: geometry/mesh.py:321-326)."""
    try:
        i = int(signed_idx)
    except (TypeError, ValueError):
        raise L.MembraneHipError(f"perimeter: edge index {signed_idx!r} is not an integer") from None
    if i == 0:
        raise L.MembraneHipError("perimeter: edge index 0 is invalid (signed indices start at 1)")
    row_of = mesh.vertex_index_to_row
    if hasattr(mesh, "vertices") and isinstance(mesh.vertices, dict):
        e = mesh.edges.get(abs(i))
        if e is None:
            raise L.MembraneHipError(f"perimeter: unknown edge index {i}")
        t, h = row_of[int(e.tail_index)], row_of[int(e.head_index)]
    else:
        er = mesh.edge_rows
        if abs(i) > len(er):
            raise L.MembraneHipError(f"perimeter: unknown edge index {i} (the mesh has {len(er)} edges)")
        t, h = int(er[abs(i) - 1, 0]), int(er[abs(i) - 1, 1])
    return (int(h), int(t)) if i < 0 else (int(t), int(h))


def loops(mesh, global_params=None):
    """-> (entry numbers, loop_off, tail rows, head rows, targets) of the entries of ``perimeter_constraints`` that do
    something, in list order: an entry without ``edges`` or without ``target_perimeter`` is skipped (perimeter.py:39-42)."""
    gp = global_params if global_params is not None else getattr(mesh, "global_parameters", None)
    cons = (gp.get("perimeter_constraints") if gp is not None else None) or []
    num, off, tail, head, target = [], [0], [], [], []
    for k, con in enumerate(cons):
        edges = con.get("edges")
        t = con.get("target_perimeter")
        if not edges or t is None:
            continue
        t = float(t)
        if not math.isfinite(t):
            raise L.MembraneHipError(f"perimeter: target_perimeter of entry {k} must be finite (got {t!r})")
        if not has_edge_table(mesh):
            raise L.MembraneHipError("perimeter: the mesh has no edge table (ArrayMesh(edges=...)); its signed edge "
                                     "indices cannot be resolved")
        for s in edges:
            a, b = _edge_rows(mesh, s)
            tail.append(a)
            head.append(b)
        num.append(k)
        off.append(len(tail))
        target.append(t)
    return (num, np.asarray(off, dtype=np.int32), np.asarray(tail, dtype=np.int32), np.asarray(head, dtype=np.int32),
            np.asarray(target, dtype=np.float64))


def host_tables(nv: int, iperm, loop_off, tail, head):
    """The device tables as the library builds them (ms_perimeter_tables_host: the code ms_set_perimeter runs), for
    inspection: the entries {tail, head} in library rows, the distinct vertices per loop {vert_off, vrow} and the
    vertex -> entry CSR {csr_off, csr_ent} whose items are -(entry + 1) at a tail and +(entry + 1) at a head."""
    ip = np.ascontiguousarray(np.asarray(iperm, dtype=np.int32).reshape(-1))
    lo = np.ascontiguousarray(np.asarray(loop_off, dtype=np.int32).reshape(-1))
    t = np.ascontiguousarray(np.asarray(tail, dtype=np.int32).reshape(-1))
    h = np.ascontiguousarray(np.asarray(head, dtype=np.int32).reshape(-1))
    n, nl = len(t), len(lo) - 1
    cnt = np.zeros(2, dtype=np.int32)
    et, eh = np.zeros(n + 1, np.int32), np.zeros(n + 1, np.int32)
    vo, vrow = np.zeros(nl + 2, np.int32), np.zeros(2 * n + 1, np.int32)
    co, ce = np.zeros(2 * n + 2, np.int32), np.zeros(2 * n + 1, np.int32)
    i32 = lambda a: a.ctypes.data_as(L._I32)  # noqa: E731
    rc = L.lib().ms_perimeter_tables_host(int(nv), i32(ip), nl, i32(lo), i32(t), i32(h), i32(cnt), i32(et), i32(eh),
                                          i32(vo), i32(vrow), i32(co), i32(ce))
    L.check(rc, None, "ms_perimeter_tables_host")
    ne, nd = int(cnt[0]), int(cnt[1])
    return {"tail": et[:ne].copy(), "head": eh[:ne].copy(), "vert_off": vo[:nl + 1].copy(), "vrow": vrow[:nd].copy(),
            "csr_off": co[:nd + 1].copy(), "csr_ent": ce[:2 * ne].copy()}


def upload(mesh, global_params, dm):
    """Resolve the loops and hand them to the device -> the entry numbers of the loops set ([]: tables cleared)."""
    num, off, tail, head, target = loops(mesh, global_params)
    if not num:
        dm.set_perimeter()
        return num
    tri, _ = mesh.triangle_row_cache()
    _edge.check_triangle_sides(NAME, "listed", tri if tri is not None else np.zeros((0, 3), np.int32), dm.nv, tail, head)
    dm.set_perimeter(off, tail, head, target)
    return num


def enforce_constraint(mesh, tol: float = 1e-10, max_iter: int = 3, **_kwargs) -> None:
    mir = mirror_for(mesh)
    dm = mir.sync()
    if not upload(mesh, None, dm):
        return
    passes, _p = dm.project_perimeter(tol=tol, max_iter=max_iter)
    if int(np.sum(passes)) > 0:
        _write_back(mesh, dm, mir)


__all__ = ["enforce_constraint", "loops", "upload", "host_tables", "NAME"]
