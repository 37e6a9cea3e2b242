"""Hard body-area constraint plugin on the HIP path (modules/constraints/body_area.py).

``constraint_gradients_array`` (:28-84) returns the dense KKT row dA/dx over the body's facets (facets with
|n| < 1e-12 skipped, fixed rows not masked); ``enforce_constraint`` (:87-139) is the projection loop
x -= (dA / (|dA/dx|^2 + 1e-18)) dA/dx on movable rows, up to 20 steps, run on the device.  The target is
``body.options["target_area"]`` (not the penalty's ``area_target``).  One body per mesh.
"""

from __future__ import annotations

import math

import numpy as np

from ... import _lib as L
from ...geometry.mesh import mirror_for


def target_area(mesh):
    """``target_area`` of the mesh's single body, or None when the module does nothing: no body, or no target in the
    body's options (body_area.py:40-41, :102-104).  A target the device does not take is refused."""
    bodies = getattr(mesh, "bodies", None) or {}
    if not bodies:
        return None
    if len(bodies) > 1:
        raise L.MembraneHipError("body_area: the HIP path supports one body per mesh (SURVEY 8a row a7); "
                                 f"this mesh has {len(bodies)}")
    body = next(iter(bodies.values()))
    t = (getattr(body, "options", None) or {}).get("target_area")
    if t is None:
        return None
    t = float(t)
    if not (math.isfinite(t) and t > 0.0):
        raise L.MembraneHipError(f"body_area: target_area must be finite and positive (got {t!r})")
    return t


def _write_back(mesh, dm, mir):
    mesh.positions_view()[...] = dm.get_positions()
    if hasattr(mesh, "vertices"):  # reference Mesh: write the objects back
        pos = mesh.positions_view()
        for row, vid in enumerate(mesh.vertex_ids):
            mesh.vertices[int(vid)].position[:] = pos[row]
    mesh.increment_version()
    mir.mark_device_positions_current()


def constraint_gradients_array(mesh, global_params, *, positions: np.ndarray, index_map) -> list | None:
    _ = (global_params, index_map)
    target = target_area(mesh)
    if target is None:
        return None
    mir = mirror_for(mesh)
    dm = mir.sync(positions=None if positions is mesh.positions_view() else positions)
    dm.set_area_constraint(L.MS_AREA_BODY, target)
    row, _area, _n2 = dm.area_row()
    return [row]


def enforce_constraint(mesh, tol: float = 1e-12, max_iter: int = 20, **_kwargs) -> None:
    target = target_area(mesh)
    if target is None:
        return
    mir = mirror_for(mesh)
    dm = mir.sync()
    dm.set_area_constraint(L.MS_AREA_BODY, target)
    iters, _a = dm.project_area(tol=tol, max_iter=max_iter)
    if iters > 0:
        _write_back(mesh, dm, mir)


__all__ = ["enforce_constraint", "constraint_gradients_array", "target_area"]
