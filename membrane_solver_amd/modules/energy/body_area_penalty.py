"""Soft body-area penalty energy plugin on the HIP path.

Drop-in for modules/energy/body_area_penalty.py:100-145: E = 1/2 k (A - A0)^2 over the body's facets, gradient
k (A - A0) dA/dx with the facet area and its gradient of geometry/facet.py:168-249.  On the device that gradient is
an effective surface tension k (A - A0) on the facets that carry the body flag (MS_MOD_AREA_PENALTY).  One body per
mesh.
"""

from __future__ import annotations

from typing import Dict

import numpy as np

from ... import _lib as L
from ...geometry.mesh import mirror_for


def body_area_params(mesh, global_params, param_resolver):
    """(k, A0) of the mesh's single body as body_area_penalty.py:111-123 resolves them, or None when the module
    contributes nothing: no body, no ``area_target`` in the body's options, or a stiffness that is absent or zero
    (there is no default stiffness)."""
    bodies = getattr(mesh, "bodies", None) or {}
    if not bodies:
        return None
    body = next(iter(bodies.values()))
    target = (getattr(body, "options", None) or {}).get("area_target")
    if target is None:
        return None
    k = param_resolver.get(body, "area_stiffness") if param_resolver is not None else None
    if k is None:
        k = float(global_params.get("area_stiffness", 0.0) or 0.0)
    k = float(k)
    if k == 0.0:
        return None
    return k, float(target)


def compute_energy_and_gradient_array(mesh, global_params, param_resolver, *, positions: np.ndarray,
                                      index_map: Dict[int, int], grad_arr: np.ndarray) -> float:
    _ = index_map
    mir = mirror_for(mesh)
    dm = mir.sync(positions=None if positions is mesh.positions_view() else positions)  # validates the single body
    ka = body_area_params(mesh, global_params, param_resolver)
    if ka is None:
        return 0.0
    dm.set_area_penalty(*ka)
    dm.set_params(modules=L.MS_MOD_AREA_PENALTY)
    if grad_arr is not None:
        e, g = dm.energy_and_gradient(want_grad=True, raw=True)
        np.add(grad_arr, g, out=grad_arr)
    else:
        e = dm.energy()
    return float(e[2])


def compute_energy_and_gradient(mesh, global_params, param_resolver, *, compute_gradient: bool = True):
    positions = mesh.positions_view()
    grad_arr = np.zeros_like(positions)
    E = compute_energy_and_gradient_array(mesh, global_params, param_resolver, positions=positions,
                                          index_map=mesh.vertex_index_to_row, grad_arr=grad_arr)
    if not compute_gradient:
        return float(E), {}
    return float(E), {int(vid): grad_arr[row].copy() for row, vid in enumerate(mesh.vertex_ids)
                      if np.any(grad_arr[row])}


__all__ = ["compute_energy_and_gradient", "compute_energy_and_gradient_array", "body_area_params"]
