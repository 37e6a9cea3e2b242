"""Outer-leaflet rim source (soft contact term on an inclusion rim) plugin on the HIP path.

Drop-in for the reference's modules/energy/tilt_rim_source_out.py (the mirror of tilt_rim_source_in.py:339-519).
    E = -sum over the rim edges of gamma L 1/2 (t_tail + t_head) . r_hat,
r_hat the in-plane unit vector from the circle's center to the edge's midpoint (0 when the midpoint lies on the axis),
L the edge's length; tilt gradient -1/2 gamma L r_hat at both ends into ``tilt_out_grad_arr``; no shape gradient, so
``grad_arr`` is left as it is.  Rim edges, gamma (modules/energy/contact_mapping.py) and the frame are resolved by
leaflet_common.rim_source_params.  Follow mode (a rim vertex with ``pin_to_circle_mode: fit``) needs a
``pin_to_circle_normal``: the reference's SVD plane fit raises here.
"""

from __future__ import annotations

from typing import Dict

import numpy as np

from . import leaflet_common as _lc

USES_TILT_LEAFLETS = True
IS_EXTERNAL_WORK = True
_LEAFLET = "out"
_KIND = "rim"


def compute_energy_and_gradient_array(mesh, global_params, param_resolver, *, positions: np.ndarray,
                                      index_map: Dict[int, int], grad_arr: np.ndarray | None, ctx=None,
                                      tilts_in: np.ndarray | None = None, tilts_out: np.ndarray | None = None,
                                      tilt_in_grad_arr: np.ndarray | None = None,
                                      tilt_out_grad_arr: np.ndarray | None = None) -> float:
    _ = (index_map, ctx, grad_arr)
    return _lc.evaluate(mesh, global_params, param_resolver, kind=_KIND, leaflet=_LEAFLET, positions=positions,
                        tilts=tilts_in if _LEAFLET == "in" else tilts_out, grad_arr=None,
                        tilt_grad_arr=tilt_in_grad_arr if _LEAFLET == "in" else tilt_out_grad_arr)


def compute_energy_array(mesh, global_params, param_resolver, *, positions: np.ndarray, index_map: Dict[int, int],
                         tilts_in: np.ndarray | None = None, tilts_out: np.ndarray | None = None, ctx=None) -> float:
    return compute_energy_and_gradient_array(mesh, global_params, param_resolver, positions=positions,
                                             index_map=index_map, grad_arr=None, ctx=ctx, tilts_in=tilts_in,
                                             tilts_out=tilts_out)


def compute_energy_and_gradient(mesh, global_params, param_resolver, *, compute_gradient: bool = True):
    """Dict API of the reference: (E, {}, tilt_grad) with the non-zero rows of the tilt gradient only (:363-368)."""
    positions = mesh.positions_view()
    tg = np.zeros_like(positions) if compute_gradient else None
    kw = {"tilt_in_grad_arr": tg} if _LEAFLET == "in" else {"tilt_out_grad_arr": tg}
    E = compute_energy_and_gradient_array(mesh, global_params, param_resolver, positions=positions,
                                          index_map=mesh.vertex_index_to_row, grad_arr=None, **kw)
    if not compute_gradient:
        return float(E), {}
    return float(E), {}, {int(v): tg[r].copy() for r, v in enumerate(mesh.vertex_ids) if np.any(tg[r])}


__all__ = ["compute_energy_and_gradient", "compute_energy_and_gradient_array", "compute_energy_array"]
