"""pin_to_circle on the HIP path (modules/constraints/pin_to_circle.py of the reference).

Tagged vertices, and both endpoints of tagged edges, are projected onto a circle: per entity (``fixed`` mode) or
onto the group's circle whose centre slides along the given normal by the members' mean offset, with the given
radius or else their mean radial distance (``slide``).  ``fit`` mode and the preserve-normal option raise.
"""

from __future__ import annotations

from . import pins
from .pin_to_plane import _project


def enforce_constraint(mesh, **_kwargs) -> None:
    """Project the tagged rows of ``mesh.positions_view()`` in place (NumPy restatement)."""
    _project(mesh, pins.CIRCLE)


def constraint_gradients_rows_array(mesh, _global_params, *, positions, index_map=None):
    """Sparse rows: fixed circles the normal and the radial unit vector per vertex; slide circles
    ``{first member: -n, v: +n}`` per other member plus the radial unit vector per member (fixed vertices: none)."""
    _ = index_map
    return pins.rows(positions, pins.programs(mesh, [pins.CIRCLE])) or None
