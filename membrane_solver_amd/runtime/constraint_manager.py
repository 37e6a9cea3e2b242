"""Constraint plugin loader (runtime/constraint_manager.py, reduced to the
in-scope ``volume``, ``body_area``, ``global_area``, ``pin_to_plane``, ``pin_to_circle``,
``tilt_thetaB_boundary_in`` and the enforce-only ``fixed_plane`` / ``perimeter`` modules, which have no row and take no
part in it), the KKT projection of the gradient (:174-315): the k == 1 dense row alone, the
volume and area rows together, or the mixed dense + sparse-row solve with the pins -- and the two tilt-space seams
(:651-841) for
constraints that act on the leaflet tilts only."""

from __future__ import annotations

import importlib
import logging

import numpy as np

from ..modules.constraints import pins as _pins

logger = logging.getLogger("membrane_solver")

_PACKAGE = "membrane_solver_amd.modules.constraints"


class ConstraintModuleManager:
    def __init__(self, module_names):
        self.modules = {}
        for name in module_names:
            try:
                self.modules[name] = importlib.import_module(f"{_PACKAGE}.{name}")
            except ImportError as e:
                logger.error("Could not load constraint module '%s': %s", name, e)
                raise

    def get_constraint(self, name):
        if name not in self.modules:
            raise KeyError(f"Constraint module '{name}' not found.")
        return self.modules[name]

    def __contains__(self, name):
        return name in self.modules

    def __getitem__(self, name):
        return self.modules[name]

    def apply_gradient_modifications_array(self, grad_arr, mesh, global_params):
        """Host-array variant of constraint_manager.py:174-315 (the device path's CPU restatement)."""
        positions = mesh.positions_view()
        if any(hasattr(m, "constraint_gradients_rows_array") for m in self.modules.values()):
            dense, sparse = [], []
            for module in self.modules.values():
                fr = getattr(module, "constraint_gradients_rows_array", None)
                if fr is not None:
                    sparse.extend(fr(mesh, global_params, positions=positions,
                                     index_map=mesh.vertex_index_to_row) or [])
                    continue
                fn = getattr(module, "constraint_gradients_array", None)
                if fn is not None:
                    dense.extend(fn(mesh, global_params, positions=positions,
                                    index_map=mesh.vertex_index_to_row) or [])
            _pins.project_gradient(grad_arr, dense, sparse)
            return
        rows = []
        for module in self.modules.values():
            fn = getattr(module, "constraint_gradients_array", None)
            if fn is None:
                continue
            g_list = fn(mesh, global_params, positions=positions, index_map=mesh.vertex_index_to_row)
            if g_list:
                rows.extend(g_list)
        if not rows:
            return
        if len(rows) == 2:
            # the dense KKT solve (constraint_projection.py:101-129) on C = [volume row; area row], in the listed order
            C = np.stack([np.asarray(r, dtype=float).reshape(-1) for r in rows])
            g = grad_arr.reshape(-1)
            A = C @ C.T
            A[np.diag_indices_from(A)] += 1e-18
            b = C @ g
            try:
                lam = np.linalg.solve(np.linalg.cholesky(A).T, np.linalg.solve(np.linalg.cholesky(A), b))
            except np.linalg.LinAlgError:
                try:
                    lam = np.linalg.solve(A, b)
                except np.linalg.LinAlgError:
                    return
            g -= C.T @ lam
            return
        if len(rows) != 1:
            raise NotImplementedError("only one dense constraint row (volume or body_area) or the two together are in scope")
        gC = rows[0]
        norm_sq = float(np.sum(gC * gC))
        if norm_sq > 1e-18:
            lam = float(np.sum(grad_arr * gC)) / norm_sq
            grad_arr -= lam * gC

    def apply_tilt_gradient_modifications_array(self, tilt_in_grad_arr, tilt_out_grad_arr, mesh, global_params, *,
                                                positions=None, tilts_in=None, tilts_out=None):
        """Host-array variant of constraint_manager.py:651-828: the leaflet tilt gradients projected against the sparse
        rows of every module that has ``constraint_gradients_tilt_rows_array``.  In scope: rows that touch one vertex
        of one leaflet each and are pairwise disjoint (tilt_thetaB_boundary_in), so C C^T is diagonal and the
        projection is g_i <- g_i - ((g_i . d_i) / (d_i . d_i)) d_i row by row.  (On the device the relaxation does
        this itself: ms_relax_leaflet_tilts with a table set, DeviceMesh.thetab_boundary_projected_gradient.)"""
        if tilt_in_grad_arr.shape != tilt_out_grad_arr.shape:
            raise ValueError("tilt gradient arrays must have matching shapes")
        if positions is None:
            positions = mesh.positions_view()
        seen = [set(), set()]
        for module in self.modules.values():
            fn = getattr(module, "constraint_gradients_tilt_rows_array", None)
            if fn is None:
                continue
            payload = fn(mesh, global_params, positions=positions, index_map=mesh.vertex_index_to_row,
                         tilts_in=tilts_in, tilts_out=tilts_out)
            for parts in payload or []:
                for leaflet, (part, grad) in enumerate(zip(parts, (tilt_in_grad_arr, tilt_out_grad_arr))):
                    if part is None:
                        continue
                    rows, vecs = np.asarray(part[0], dtype=int), np.asarray(part[1], dtype=float)
                    if len(rows) != 1 or int(rows[0]) in seen[leaflet] or sum(p is not None for p in parts) != 1:
                        raise NotImplementedError("only disjoint one-vertex, one-leaflet tilt constraint rows are in scope")
                    seen[leaflet].add(int(rows[0]))
                    d = vecs.reshape(3)
                    g = grad[int(rows[0])]
                    grad[int(rows[0])] = g - (float(g @ d) / float(d @ d)) * d

    def enforce_tilt_constraints(self, mesh, *, device=None, **kwargs):
        """Tilt-only projections of every loaded module that has ``enforce_tilt_constraint``
        (constraint_manager.py:830-841), on the mesh's arrays -- or, with ``device`` (a DeviceMesh whose table is set),
        on the device's positions and stored inner tilts (ms_thetab_boundary_enforce)."""
        for module in self.modules.values():
            fn = getattr(module, "enforce_tilt_constraint", None)
            if fn is None:
                continue
            if device is not None:
                device.thetab_boundary_enforce()
            else:
                fn(mesh, **kwargs)

    def enforce_all(self, mesh, *, context="minimize", global_params=None, **options):
        """Hard projection of every loaded constraint that has one -- here: ``volume`` -- onto its target
        (interface of constraint_manager.py:843-905).

        Inside a minimisation step (``context == "minimize"``) the volume projection only runs when
        ``volume_projection_during_minimization`` is on; with it off the optimizer holds the volume through the
        KKT projection of the gradient alone.  After mesh operations and at the end of ``minimize`` (the other
        contexts) it always runs, with ``force_projection=True``."""
        during_step = context == "minimize"
        step_projection = True if global_params is None else bool(
            global_params.get("volume_projection_during_minimization", True))
        options.pop("force_projection", None)
        for name, module in self.modules.items():  # in the listed order (:857-905); the pins in every context
            if not hasattr(module, "enforce_constraint"):  # (a tilt-only module: enforce_tilt_constraints)
                continue
            if name != "volume":
                module.enforce_constraint(mesh, context=context, global_params=global_params, **options)
            elif not (during_step and not step_projection):
                module.enforce_constraint(mesh, force_projection=True, context=context, global_params=global_params,
                                          **options)
