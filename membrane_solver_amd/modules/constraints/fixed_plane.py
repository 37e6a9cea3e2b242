"""Fixed-plane constraint plugin on the HIP path (modules/constraints/fixed_plane.py).

``enforce_constraint`` (:25-53) puts every vertex that is not fixed onto the plane {``fixed_plane_normal`` (default
(0, 0, 1), divided by its norm), ``fixed_plane_point`` (default the origin)}: x - ((x - point) . n) n, one pass, on the
device (ms_enforce_fixed_plane).  A normal below 1e-15 gives the reference's warning and no projection.  The module has
no KKT row: it takes no part in the gradient projection.
"""

from __future__ import annotations

import logging

import numpy as np

from ... import _lib as L
from ...geometry.mesh import mirror_for
from .body_area import _write_back

logger = logging.getLogger("membrane_solver")

NAME = "fixed_plane"


def plane(mesh, global_params=None):
    """(normal, point) as the globals give them (fixed_plane.py:32-48), or None where the module warns and does nothing
    (|normal| < 1e-15).  The library normalises the normal."""
    gp = global_params if global_params is not None else getattr(mesh, "global_parameters", None)
    n = gp.get("fixed_plane_normal") if gp is not None else None
    q = gp.get("fixed_plane_point") if gp is not None else None
    try:
        normal = np.array([0.0, 0.0, 1.0]) if n is None else np.asarray(n, dtype=float).reshape(3).copy()
        point = np.zeros(3) if q is None else np.asarray(q, dtype=float).reshape(3).copy()
    except (TypeError, ValueError):
        raise L.MembraneHipError("fixed_plane: fixed_plane_normal / fixed_plane_point must be three numbers") from None
    if not (np.all(np.isfinite(normal)) and np.all(np.isfinite(point))):
        raise L.MembraneHipError("fixed_plane: fixed_plane_normal / fixed_plane_point must be finite")
    if float(np.linalg.norm(normal)) < 1e-15:
        logger.warning("fixed_plane: normal is near zero; skipping projection.")
        return None
    return normal, point


def upload(mesh, global_params, dm) -> bool:
    """Hand the plane to the device; False (plane cleared) where the module does nothing."""
    pl = plane(mesh, global_params)
    if pl is None:
        dm.set_fixed_plane()
        return False
    dm.set_fixed_plane(*pl)
    return True


def enforce_constraint(mesh, tol: float = 0.0, max_iter: int = 1, **_kwargs) -> None:
    _ = (tol, max_iter)
    mir = mirror_for(mesh)
    dm = mir.sync()
    if not upload(mesh, None, dm):
        return
    dm.enforce_fixed_plane()
    _write_back(mesh, dm, mir)


__all__ = ["enforce_constraint", "plane", "upload", "NAME"]
