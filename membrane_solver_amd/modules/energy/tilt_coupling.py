"""Inter-leaflet tilt coupling plugin on the HIP path.

Drop-in for the reference's modules/energy/tilt_coupling.py:43-262.
    E = 1/2 k_c int |t_out + s t_in|^2 dA,   s = -1 ("difference", tracking) or +1 ("sum", anti-tracking),
lumped per facet with |n| >= 1e-12: coeff_f = 0.5 k_c ((q_0 + q_1 + q_2) / 3), q_v = |t_out,v + s t_in,v|^2.
Shape gradient coeff_f dA_f/dv_k into ``grad_arr``; tilt gradients k_c d_v A_v into ``tilt_out_grad_arr`` and
k_c s d_v A_v into ``tilt_in_grad_arr`` (A_v the barycentric area over the same facets).  ``tilt_coupling_modulus`` is
k_c; the mode is ``tilt_coupling_mode`` (fallback: the misspelt ``tilt_couping_mode``), resolved by
leaflet_common.coupling_params.  An unknown or absent mode, or k_c == 0, contributes exactly nothing.
"""

from __future__ import annotations

from typing import Dict, Tuple

import numpy as np

from . import leaflet_common as _lc

USES_TILT_LEAFLETS = True


def compute_energy_and_gradient(mesh, global_params, param_resolver) -> Tuple[float, Dict[int, np.ndarray],
                                                                                Dict[int, np.ndarray]]:
    """Dict API of the reference (:43-111): (E, shape_grad, tilt_grad) with a row for every vertex; ``tilt_grad`` is
    the OUTER leaflet's gradient k_c d_v A_v (:109)."""
    positions = mesh.positions_view()
    nv = len(mesh.vertex_ids)
    g = np.zeros((nv, 3))
    tg = np.zeros((nv, 3))
    E = compute_energy_and_gradient_array(mesh, global_params, param_resolver, positions=positions,
                                          index_map=mesh.vertex_index_to_row, grad_arr=g, tilt_out_grad_arr=tg)
    shape_grad = {int(v): g[r].copy() for r, v in enumerate(mesh.vertex_ids)}
    tilt_grad = {int(v): tg[r].copy() for r, v in enumerate(mesh.vertex_ids)}
    return float(E), shape_grad, tilt_grad


def compute_energy_and_gradient_array(mesh, global_params, param_resolver, *, positions: np.ndarray,
                                      index_map: Dict[int, int], grad_arr: np.ndarray | None,
                                      tilts_in: np.ndarray | None = None, tilts_out: np.ndarray | None = None,
                                      tilt_in_grad_arr: np.ndarray | None = None,
                                      tilt_out_grad_arr: np.ndarray | None = None) -> float:
    _ = index_map
    return _lc.evaluate_coupling(mesh, global_params, param_resolver, positions=positions, tilts_in=tilts_in,
                                 tilts_out=tilts_out, grad_arr=grad_arr, tilt_in_grad_arr=tilt_in_grad_arr,
                                 tilt_out_grad_arr=tilt_out_grad_arr)


def compute_energy_array(mesh, global_params, param_resolver, *, positions: np.ndarray, index_map: Dict[int, int],
                         tilts_in: np.ndarray | None = None, tilts_out: np.ndarray | None = None) -> float:
    return compute_energy_and_gradient_array(mesh, global_params, param_resolver, positions=positions,
                                             index_map=index_map, grad_arr=None, tilts_in=tilts_in,
                                             tilts_out=tilts_out)


__all__ = ["compute_energy_and_gradient", "compute_energy_and_gradient_array", "compute_energy_array"]
