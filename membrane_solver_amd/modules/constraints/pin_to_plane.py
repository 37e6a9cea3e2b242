"""pin_to_plane on the HIP path (modules/constraints/pin_to_plane.py of the reference).

Tagged vertices, and both endpoints of tagged edges, are projected onto a plane: per entity (``fixed`` mode) or
onto the plane of the given normal through the centroid of the group's current positions (``slide``).  The tag
resolution lives in ``pins`` (shared with ``pin_to_circle``); the device runs the same program in k_pin_enforce.
"""

from __future__ import annotations

from . import pins


def enforce_constraint(mesh, **_kwargs) -> None:
    """Project the tagged rows of ``mesh.positions_view()`` in place (NumPy restatement)."""
    _project(mesh, pins.PLANE)


def constraint_gradients_rows_array(mesh, _global_params, *, positions, index_map=None):
    """Sparse rows ``[(rows, (m, 3) vectors)]``: the unit normal per pinned, non-fixed vertex."""
    _ = index_map
    return pins.rows(positions, pins.programs(mesh, [pins.PLANE])) or None


def _project(mesh, name):
    progs = pins.programs(mesh, [name])
    X = mesh.positions_view()
    pins.enforce(X, progs)
    if hasattr(mesh, "vertices") and isinstance(mesh.vertices, dict):  # reference Mesh: write the objects back
        for row, vid in enumerate(mesh.vertex_ids):
            mesh.vertices[int(vid)].position[:] = X[row]
    if hasattr(mesh, "increment_version") and not hasattr(mesh, "vertices"):
        mesh.increment_version()
