"""Rim slope matching energy plugin (outer leaflet) on the HIP path.

Drop-in for the reference's modules/energy/rim_slope_match_out.py:352-629 in its modes ``pointwise_radial_v1`` (the
default) and ``ring_average_radial_v1`` (the same code there).  Three rings of vertices tagged ``rim_slope_match_group``
-- ``rim_slope_match_group`` (rim), ``rim_slope_match_outer_group`` (outer), optionally ``rim_slope_match_disk_group``
(disk; dropped with a warning when it names the rim group) -- are ordered by angle in the frame
(``rim_slope_match_center``, ``rim_slope_match_normal``) from the positions of the evaluation; rim and outer entries are
paired by index, or with unequal counts the outer positions are interpolated at the rim's arc-length parameters:
    phi_i = (h_out - h_rim) / (r_out - r_rim),   w_i = 1/2 (l_next + l_prev) on the ordered rim, 0 where not valid
    E = 1/2 k sum w (t_out . r_hat - phi)^2  [+ 1/2 k sum w (t_in . r_hat - (theta_disk - phi))^2 with a disk ring]
theta_disk per entry when the disk ring has the rim's count, else the arc-length weighted mean of t_in . r_hat_disk.
Tilt gradients on the rim rows (both leaflets) and the disk rows (inner); a shape gradient along the normal on the rim
and outer rows.  On the device one workgroup orders the rings and forms the tables (k_rsm_geom) and k_rsm_apply forms the
sums and scatters without atomics (ms_set_rim_match).  Strength 0 and a missing rim or outer group stay a host constant
0.0.  Refused: the staggered modes, a missing ``rim_slope_match_normal`` (the reference's SVD plane fit), a ring above
the device's size.
"""

from __future__ import annotations

from typing import Dict

import numpy as np

from . import leaflet_common as _lc

USES_TILT_LEAFLETS = True


def compute_energy_and_gradient_array(mesh, global_params, param_resolver, *, positions: np.ndarray,
                                      index_map: Dict[int, int], grad_arr: np.ndarray | None,
                                      tilts_in: np.ndarray | None = None, tilts_out: np.ndarray | None = None,
                                      tilt_in_grad_arr: np.ndarray | None = None,
                                      tilt_out_grad_arr: np.ndarray | None = None) -> float:
    _ = index_map
    return _lc.evaluate_rim_match(mesh, global_params, param_resolver, positions=positions, tilts_in=tilts_in,
                                  tilts_out=tilts_out, grad_arr=grad_arr, tilt_in_grad_arr=tilt_in_grad_arr,
                                  tilt_out_grad_arr=tilt_out_grad_arr)


def compute_energy_array(mesh, global_params, param_resolver, *, positions: np.ndarray, index_map: Dict[int, int],
                         tilts_in: np.ndarray | None = None, tilts_out: np.ndarray | None = None) -> float:
    return compute_energy_and_gradient_array(mesh, global_params, param_resolver, positions=positions,
                                             index_map=index_map, grad_arr=None, tilts_in=tilts_in, tilts_out=tilts_out)


def compute_energy_and_gradient(mesh, global_params, param_resolver, *, compute_gradient: bool = True):
    """Dict API of the reference (:303-349): (E, shape_grad, tilt_in_grad, tilt_out_grad) with the non-zero rows only;
    (E, {}) without the gradient."""
    positions = mesh.positions_view()
    g = np.zeros_like(positions)
    gi = np.zeros_like(positions) if compute_gradient else None
    go = np.zeros_like(positions) if compute_gradient else None
    E = compute_energy_and_gradient_array(mesh, global_params, param_resolver, positions=positions,
                                          index_map=mesh.vertex_index_to_row, grad_arr=g, tilts_in=None, tilts_out=None,
                                          tilt_in_grad_arr=gi, tilt_out_grad_arr=go)
    if not compute_gradient:
        return float(E), {}
    rows = lambda a: {int(v): a[r].copy() for r, v in enumerate(mesh.vertex_ids) if np.any(a[r])}  # noqa: E731
    return float(E), rows(g), rows(gi), rows(go)


__all__ = ["compute_energy_and_gradient", "compute_energy_and_gradient_array", "compute_energy_array"]
