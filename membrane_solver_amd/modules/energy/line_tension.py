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
from ..constraints.pins import _entities
from . import edge_common as _edge


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
    """A tagged edge must be a side of some triangle (edge_common.check_triangle_sides)."""
    _edge.check_triangle_sides("line_tension", "tagged", tri_rows, nv, tail, head, numbers)


def host_tables(nv: int, iperm, tail, head, gamma):
    """The device tables as the library builds them (ms_line_tables_host: the code ms_set_line_tension runs), for
    inspection: the edge table {tail, head, gamma} and the vertex -> edge CSR {vrow, off, other, csr_gamma}, rows in
    the library's order (``iperm``: external row -> library row)."""
    return _edge.host_tables("ms_line_tables_host", "gamma", nv, iperm, tail, head, gamma)


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
    return _edge.compute_energy_and_gradient_array(upload, L.MS_MOD_LINE_TENSION, mesh, global_params, positions,
                                                   grad_arr)  # (0.0 without a charged edge: line_tension.py:113-115)


def compute_energy_and_gradient(mesh, global_params, param_resolver, *, compute_gradient: bool = True):
    return _edge.compute_energy_and_gradient(compute_energy_and_gradient_array, mesh, global_params, param_resolver,
                                             compute_gradient)


__all__ = ["compute_energy_and_gradient", "compute_energy_and_gradient_array", "tagged_edges", "edge_is_tagged",
           "has_edge_table", "check_triangle_sides", "host_tables", "upload"]
