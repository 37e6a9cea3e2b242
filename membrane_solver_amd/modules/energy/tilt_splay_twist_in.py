"""Inner-leaflet split splay / twist tilt-gradient energy plugin on the HIP path.

Drop-in for the reference's modules/energy/tilt_splay_twist_in.py:76-276 (ambient_v1 transport, native divergence).
    E = 1/2 sum_f A_f (k_splay div^2 + k_twist curl_n^2),
    div = sum_k t_k . g_k,  curl_n = (sum_k g_k x t_k) . n_hat,  g_k = (n x e_k) / max(n.n, 1e-20),
tilt gradient A_f k_splay div g_k + A_f k_twist curl_n (n_hat x g_k) into ``tilt_in_grad_arr``; no shape gradient
(``grad_arr`` is never touched).  ``k_splay`` is ``tilt_splay_modulus_in`` else ``bending_modulus_in`` else
``bending_modulus``; ``k_twist`` is ``tilt_twist_modulus_in`` else ``tilt_twist_modulus`` else 0, resolved by
leaflet_common.splay_twist_params.  Both moduli 0 contribute exactly nothing.
"""

from __future__ import annotations

from typing import Dict, Tuple

import numpy as np

from . import leaflet_common as _lc

USES_TILT_LEAFLETS = True


def compute_energy_and_gradient(
    mesh, global_params, param_resolver, *, compute_gradient: bool = True
) -> (Tuple[float, Dict[int, np.ndarray]] | Tuple[float, Dict[int, np.ndarray], Dict[int, np.ndarray]]):
    """Dict API of the reference (:76-110): ``(E, shape_grad, tilt_grad)`` listing the non-zero rows only (the shape
    gradient is therefore empty), or ``(E, {})`` when ``compute_gradient`` is False."""
    positions = mesh.positions_view()
    grad_arr = np.zeros_like(positions)
    tilt_grad_arr = np.zeros_like(positions) if compute_gradient else None
    energy = compute_energy_and_gradient_array(mesh, global_params, param_resolver, positions=positions,
                                               index_map=mesh.vertex_index_to_row, grad_arr=grad_arr, tilts_in=None,
                                               tilt_in_grad_arr=tilt_grad_arr)
    if not compute_gradient:
        return float(energy), {}
    shape_grad = {int(vid): grad_arr[row].copy() for row, vid in enumerate(mesh.vertex_ids) if np.any(grad_arr[row])}
    tilt_grad = {int(vid): tilt_grad_arr[row].copy() for row, vid in enumerate(mesh.vertex_ids)
                 if np.any(tilt_grad_arr[row])}
    return float(energy), shape_grad, tilt_grad


def compute_energy_and_gradient_array(
    mesh,
    global_params,
    param_resolver,
    *,
    positions: np.ndarray,
    index_map: Dict[int, int],
    grad_arr: np.ndarray,
    tilts_in: np.ndarray | None = None,
    tilts_out: np.ndarray | None = None,
    tilt_in_grad_arr: np.ndarray | None = None,
    tilt_out_grad_arr: np.ndarray | None = None,
) -> float:
    _ = index_map, grad_arr, tilts_out, tilt_out_grad_arr
    return _lc.evaluate_splay_twist(mesh, global_params, param_resolver, positions=positions, tilts_in=tilts_in,
                                    tilt_in_grad_arr=tilt_in_grad_arr)


def compute_energy_array(
    mesh,
    global_params,
    param_resolver,
    *,
    positions: np.ndarray,
    index_map: Dict[int, int],
    tilts_in: np.ndarray | None = None,
    tilts_out: np.ndarray | None = None,
) -> float:
    _ = tilts_out
    return compute_energy_and_gradient_array(mesh, global_params, param_resolver, positions=positions,
                                             index_map=index_map, grad_arr=np.zeros_like(positions),
                                             tilts_in=tilts_in, tilt_in_grad_arr=None)


__all__ = ["compute_energy_and_gradient", "compute_energy_and_gradient_array", "compute_energy_array"]
