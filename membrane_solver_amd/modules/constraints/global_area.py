"""Hard global-area constraint plugin on the HIP path (modules/constraints/global_area.py).

``enforce_constraint`` (:8-51) is the projection loop x -= (dA / (|dA/dx|^2 + 1e-18)) dA/dx over every facet on movable
rows, up to 3 steps, run on the device.  The target is the global ``target_surface_area``.  The module has no KKT row:
it takes no part in the gradient projection (the reference's manager warns about that once).
"""

from __future__ import annotations

import math

from ... import _lib as L
from ...geometry.mesh import mirror_for
from .body_area import _write_back


def target_area(mesh, global_params=None):
    """The global ``target_surface_area``, or None when the module does nothing (global_area.py:11-15)."""
    gp = global_params if global_params is not None else getattr(mesh, "global_parameters", None)
    t = gp.get("target_surface_area") if gp is not None else None
    if t is None:
        return None
    t = float(t)
    if not (math.isfinite(t) and t > 0.0):
        raise L.MembraneHipError(f"global_area: target_surface_area must be finite and positive (got {t!r})")
    return t


def enforce_constraint(mesh, tol: float = 1e-12, max_iter: int = 3, **_kwargs) -> None:
    target = target_area(mesh)
    if target is None:
        return
    mir = mirror_for(mesh)
    dm = mir.sync()
    dm.set_area_constraint(L.MS_AREA_GLOBAL, target)
    iters, _a = dm.project_area(tol=tol, max_iter=max_iter)
    if iters > 0:
        _write_back(mesh, dm, mir)


__all__ = ["enforce_constraint", "target_area"]
