"""Edge-length penalty energy plugin on the HIP path.

Drop-in for modules/energy/edge_length_penalty.py:16-69: E = sum over the edges that carry a target length of
0.5 k (|e| - L0)^2, gradient -/+ k (|e| - L0) (x_h - x_t) / |e| at the tail / head, an edge shorter than 1e-15
contributing nothing.  k is the global ``edge_stiffness`` alone (default 100).  On the device the energy is added into
the surface slot behind the energy pass and the gradient into G behind the gradient pass, each behind line_tension's
launch when both modules are on (MS_MOD_EDGE_LENGTH_PENALTY, ms_set_edge_length_penalty).
"""

from __future__ import annotations

from typing import Dict

import numpy as np

from ... import _lib as L
from ..constraints.pins import _entities
from . import edge_common as _edge

NAME = "edge_length_penalty"


def stiffness(global_params) -> float:
    """edge_length_penalty.py:35: the global parameter alone, 100.0 when the key is absent; never the edge's own
    option, never through the resolver."""
    return float(global_params.get("edge_stiffness", 100.0))


def edge_is_selected(opts) -> bool:
    """edge_length_penalty.py:16-22: ``"edge_length_penalty" in opts.get("energy", [])`` or the key ``target_length``
    is present.  ``energy`` may be a string, a list or absent; whatever else it holds selects nothing (the edge is
    then charged, or not, by its target alone) and does not raise."""
    opts = opts or {}
    if "target_length" in opts:
        return True
    energy = opts.get("energy", [])
    try:
        return NAME in energy
    except TypeError:
        return False


def charged_edges(mesh, global_params):
    """-> (tail rows, head rows, target lengths, edge numbers) of the edges the reference's loop charges, in its
    iteration order: a selected edge whose ``target_length`` is not None (edge_length_penalty.py:40-42 -- so a tag
    without a target charges nothing, and a target without a tag does), both ends with a row (:44-47)."""
    _ = global_params  # (k is global and applies to every edge: see stiffness())
    _verts, edges, row_of, _fixed_of = _entities(mesh)
    tail, head, tgt, num = [], [], [], []
    for k, (t, h, opts) in enumerate(edges):
        if not edge_is_selected(opts):
            continue
        target = (opts or {}).get("target_length")
        if target is None:
            continue
        tr, hr = row_of.get(t), row_of.get(h)
        if tr is None or hr is None:
            continue
        tail.append(int(tr))
        head.append(int(hr))
        tgt.append(float(target))
        num.append(k)
    return (np.asarray(tail, dtype=np.int32), np.asarray(head, dtype=np.int32), np.asarray(tgt, dtype=np.float64),
            np.asarray(num, dtype=np.int64))


def check_triangle_sides(tri_rows, nv: int, tail, head, numbers=None) -> None:
    """A charged edge must be a side of some triangle (edge_common.check_triangle_sides)."""
    _edge.check_triangle_sides(NAME, "charged", tri_rows, nv, tail, head, numbers)


def host_tables(nv: int, iperm, tail, head, target_length, k: float):
    """The device tables as the library builds them (ms_edge_penalty_tables_host: the code ms_set_edge_length_penalty
    runs), for inspection: the edge table {tail, head, l0} and the vertex -> edge CSR {vrow, off, other, csr_l0}, rows
    in the library's order (``iperm``: external row -> library row).  k == 0 keeps no edge."""
    return _edge.host_tables("ms_edge_penalty_tables_host", "l0", nv, iperm, tail, head, target_length, float(k))


def upload(mesh, global_params, dm, charged=None) -> bool:
    """Resolve the charged edges (or take them as ``charged_edges`` returned them) and hand them to the device;
    False (tables cleared) when nothing is charged or k == 0 (the reference adds zeros there)."""
    tail, head, target, num = charged if charged is not None else charged_edges(mesh, global_params)
    k = stiffness(global_params)
    if not np.isfinite(k) or not np.all(np.isfinite(target)):
        raise L.MembraneHipError(NAME + ": edge_stiffness and every target_length must be finite")
    if len(tail) == 0 or k == 0.0:
        dm.set_edge_length_penalty()
        return False
    tri, _ = mesh.triangle_row_cache()
    check_triangle_sides(tri if tri is not None else np.zeros((0, 3), np.int32), dm.nv, tail, head, num)
    dm.set_edge_length_penalty(tail, head, target, k)
    return True


def compute_energy_and_gradient_array(mesh, global_params, param_resolver, *, positions: np.ndarray,
                                      index_map: Dict[int, int], grad_arr: np.ndarray) -> float:
    _ = index_map, param_resolver
    return _edge.compute_energy_and_gradient_array(upload, L.MS_MOD_EDGE_LENGTH_PENALTY, mesh, global_params,
                                                   positions, grad_arr)


def compute_energy_and_gradient(mesh, global_params, param_resolver, *, compute_gradient: bool = True):
    return _edge.compute_energy_and_gradient(compute_energy_and_gradient_array, mesh, global_params, param_resolver,
                                             compute_gradient)


__all__ = ["compute_energy_and_gradient", "compute_energy_and_gradient_array", "charged_edges", "edge_is_selected",
           "stiffness", "check_triangle_sides", "host_tables", "upload"]
