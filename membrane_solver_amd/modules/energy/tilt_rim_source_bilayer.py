"""Bilayer rim source (soft contact term driving theta_B = theta_in + theta_out on an inclusion rim) on the HIP path.

Drop-in for the reference's modules/energy/tilt_rim_source_bilayer.py:376-603.
    E = -sum over the rim edges of gamma L (1/2 (t_in,tail + t_in,head) + 1/2 (t_out,tail + t_out,head)) . r_hat,
r_hat the in-plane unit vector from the circle's center to the edge's midpoint (0 when the midpoint lies on the axis),
L the edge's length; the same vector -1/2 gamma L r_hat at both ends goes into ``tilt_in_grad_arr`` AND
``tilt_out_grad_arr``; no shape gradient, so ``grad_arr`` is left as it is.  The keys carry no leaflet suffix
(``tilt_rim_source_group``, ``tilt_rim_source_strength`` and the contact-parameter chain), the fixed frame's normal is
always (0,0,1) and boundary mode keeps edges with fewer than two triangles: leaflet_common.rim_source_params with
``leaflet=None``.  Follow mode (a rim vertex with ``pin_to_circle_mode: fit``) needs a ``pin_to_circle_normal``: the
reference's SVD plane fit raises here.  On the device one table, one coefficient array and one apply kernel serve both
fields (ms_set_rim_source_bilayer).
"""

from __future__ import annotations

from typing import Dict

import numpy as np

from . import leaflet_common as _lc

USES_TILT_LEAFLETS = True
IS_EXTERNAL_WORK = True


def compute_energy_and_gradient(mesh, global_params, param_resolver, *, compute_gradient: bool = True):
    """Dict API of the reference (:376-413): (E, {}, tilt_in_grad, tilt_out_grad) with the non-zero rows of the tilt
    gradients only; (E, {}) without the gradient."""
    positions = mesh.positions_view()
    gi = np.zeros_like(positions) if compute_gradient else None
    go = np.zeros_like(positions) if compute_gradient else None
    E = compute_energy_and_gradient_array(mesh, global_params, param_resolver, positions=positions,
                                          index_map=mesh.vertex_index_to_row, grad_arr=None, tilts_in=None,
                                          tilts_out=None, tilt_in_grad_arr=gi, tilt_out_grad_arr=go)
    if not compute_gradient:
        return float(E), {}
    rows = lambda tg: {int(v): tg[r].copy() for r, v in enumerate(mesh.vertex_ids) if np.any(tg[r])}  # noqa: E731
    return float(E), {}, rows(gi), rows(go)


def compute_energy_and_gradient_array(mesh, global_params, param_resolver, *, positions: np.ndarray,
                                      index_map: Dict[int, int], grad_arr: np.ndarray | None,
                                      tilts_in: np.ndarray | None = None, tilts_out: np.ndarray | None = None,
                                      tilt_in_grad_arr: np.ndarray | None = None,
                                      tilt_out_grad_arr: np.ndarray | None = None) -> float:
    _ = (index_map, grad_arr)
    return _lc.evaluate_rim_bilayer(mesh, global_params, param_resolver, positions=positions, tilts_in=tilts_in,
                                    tilts_out=tilts_out, tilt_in_grad_arr=tilt_in_grad_arr,
                                    tilt_out_grad_arr=tilt_out_grad_arr)


def compute_energy_array(mesh, global_params, param_resolver, *, positions: np.ndarray, index_map: Dict[int, int],
                         tilts_in: np.ndarray | None = None, tilts_out: np.ndarray | None = None) -> float:
    return compute_energy_and_gradient_array(mesh, global_params, param_resolver, positions=positions,
                                             index_map=index_map, grad_arr=None, tilts_in=tilts_in,
                                             tilts_out=tilts_out)


__all__ = ["compute_energy_and_gradient", "compute_energy_and_gradient_array", "compute_energy_array"]
