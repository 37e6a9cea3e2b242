"""Inner-leaflet theta_B contact work term (Kozlov-style scalar boundary mode) on the HIP path.

Drop-in for the reference's modules/energy/tilt_thetaB_contact_in.py:271-466.  The ring of vertices tagged
``rim_slope_match_group`` / ``tilt_thetaB_group`` == ``tilt_thetaB_group_in`` (fallback ``rim_slope_match_disk_group``) is
ordered by angle in the frame (``tilt_thetaB_center``, ``tilt_thetaB_normal``) from the positions of the evaluation,
w_i = 1/2 (|p_next - p_i| + |p_i - p_prev|) around the closed ring, theta_i = t_in,i . r_hat_i, R_eff = sum w |r| / wsum:
    scalar work mode (default)   E = -2 pi R_eff gamma theta_B, no gradient;
    field_linear                 E = -2 pi R_eff gamma (sum w theta / wsum), tilt gradient -(2 pi R_eff gamma / wsum) w r_hat;
    legacy penalty mode, k != 0  E += 1/2 k sum w (theta - theta_B)^2, tilt gradient k w (theta - theta_B) r_hat.
No shape gradient (``grad_arr`` is left as it is) and nothing for the outer leaflet.  On the device one workgroup orders
the ring (k_thetab_geom) and k_thetab_apply forms the sums (ms_set_thetab_contact).  A missing ``tilt_thetaB_normal``
(the reference's SVD plane fit) is refused.
"""

from __future__ import annotations

from typing import Dict

import numpy as np

from . import leaflet_common as _lc

USES_TILT_LEAFLETS = True
IS_EXTERNAL_WORK = True


def update_scalar_params(mesh, global_params, param_resolver) -> None:
    """theta_B <- sum w theta / wsum + 2 pi R_eff gamma / (k wsum) in the legacy penalty mode with k > 0 (:271-302)."""
    _lc.thetab_update_scalar(mesh, global_params, param_resolver)


def compute_energy_and_gradient(mesh, global_params, param_resolver, *, compute_gradient: bool = True):
    """Dict API of the reference (:305-333): (E, {}, tilt_in_grad) with the non-zero rows of the tilt gradient only;
    (E, {}) without the gradient."""
    positions = mesh.positions_view()
    gi = np.zeros_like(positions) if compute_gradient else None
    E = compute_energy_and_gradient_array(mesh, global_params, param_resolver, positions=positions,
                                          index_map=mesh.vertex_index_to_row, grad_arr=None, tilts_in=None,
                                          tilt_in_grad_arr=gi)
    if not compute_gradient:
        return float(E), {}
    return float(E), {}, {int(v): gi[r].copy() for r, v in enumerate(mesh.vertex_ids) if np.any(gi[r])}


def compute_energy_and_gradient_array(mesh, global_params, param_resolver, *, positions: np.ndarray,
                                      index_map: Dict[int, int], grad_arr: np.ndarray | None,
                                      tilts_in: np.ndarray | None = None, tilts_out: np.ndarray | None = None,
                                      tilt_in_grad_arr: np.ndarray | None = None,
                                      tilt_out_grad_arr: np.ndarray | None = None) -> float:
    _ = (index_map, grad_arr, tilts_out, tilt_out_grad_arr)
    return _lc.evaluate_thetab_contact(mesh, global_params, param_resolver, positions=positions, tilts_in=tilts_in,
                                       tilt_in_grad_arr=tilt_in_grad_arr)


def compute_energy_array(mesh, global_params, param_resolver, *, positions: np.ndarray, index_map: Dict[int, int],
                         tilts_in: np.ndarray | None = None, tilts_out: np.ndarray | None = None) -> float:
    return compute_energy_and_gradient_array(mesh, global_params, param_resolver, positions=positions,
                                             index_map=index_map, grad_arr=None, tilts_in=tilts_in, tilts_out=tilts_out)


__all__ = ["update_scalar_params", "compute_energy_and_gradient", "compute_energy_and_gradient_array",
           "compute_energy_array"]
