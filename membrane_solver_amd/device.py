"""DeviceMesh: the HBM-resident mirror of what the hot path reads from the
reference's ``Mesh`` (positions_view, triangle_row_cache, fixed_mask,
boundary_vertex_ids, per-facet / per-vertex parameter arrays:
geometry/mesh.py:372-389, :597-624, :210-232, :304-319, :234-265).

Thin object wrapper over the C ABI (include/membrane_hip.h).  All arithmetic
runs in libmembrane_hip.so on the GPU; every error raises MembraneHipError.
"""

from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np

from . import _lib as L


def _f64(a, shape=None, name="array"):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None and a.shape != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)}, got {a.shape}")
    return a


def _pd(a):
    return None if a is None else a.ctypes.data_as(L._D)


def _pu8(a):
    return None if a is None else a.ctypes.data_as(L._U8)


def _vec3(v):
    return (ctypes.c_double * 3)(*map(float, v))


def _i32_table(a):
    """-> (rows as a flat contiguous int32 array, a pointer to them); a table that holds nothing hands the library a
    one-element dummy: a non-NULL pointer (NULL clears a setter's tables)."""
    a = np.ascontiguousarray(np.asarray(a, dtype=np.int32).reshape(-1))
    return a, (a if len(a) else np.zeros(1, np.int32)).ctypes.data_as(L._I32)


@dataclass(slots=True)
class StepResult:
    success: bool
    converged: bool
    trials: int
    guard_rejects: int
    next_step: float
    energy: float
    alpha: float
    energy_eval: float
    grad_norm: float
    g_dot_d: float
    volume: float


class DeviceMesh:
    """One mesh resident on one GPU (or one shard of it)."""

    def __init__(self, positions, tri_rows, *, fixed=None, boundary=None, body_facets=None,
                 device: int = 0, tile_vertices: int = 0, shard_rank: int = 0, shard_count: int = 1):
        lib = L.lib()
        pos = _f64(positions, name="positions")
        if pos.ndim != 2 or pos.shape[1] != 3:
            raise ValueError("positions must be (nv,3)")
        tri = np.ascontiguousarray(tri_rows, dtype=np.int32)
        if tri.size and (tri.ndim != 2 or tri.shape[1] != 3):
            raise ValueError("tri_rows must be (nf,3)")
        self.nv = int(pos.shape[0])
        self._tri_for_tests = tri
        self.nf = int(tri.shape[0]) if tri.size else 0
        fx = None if fixed is None else np.ascontiguousarray(fixed, dtype=np.uint8)
        bd = None if boundary is None else np.ascontiguousarray(boundary, dtype=np.uint8)
        bf = None if body_facets is None else np.ascontiguousarray(body_facets, dtype=np.uint8)
        for arr, n, nm in ((fx, self.nv, "fixed"), (bd, self.nv, "boundary"), (bf, self.nf, "body_facets")):
            if arr is not None and arr.shape != (n,):
                raise ValueError(f"{nm} must have shape ({n},)")
        self._h = ctypes.c_void_p()
        rc = lib.ms_create(ctypes.byref(self._h), int(device), self.nv, self.nf, _pd(pos),
                           tri.ctypes.data_as(L._I32) if tri.size else None, _pu8(fx), _pu8(bd),
                           _pu8(bf), int(tile_vertices), int(shard_rank), int(shard_count))
        L.check(rc, None, "ms_create")
        self.device = int(device)
        self.shard_rank, self.shard_count = int(shard_rank), int(shard_count)
        self._params = L.ms_params(L.MS_MOD_SURFACE, L.MS_BEND_HELFRICH, L.MS_GRAD_ANALYTIC, 1000.0, 0.0)

    # -- lifetime -------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            L.lib().ms_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        L.check(rc, self._h, what)

    # -- parameters -----------------------------------------------------------
    def set_stream(self, hip_stream: int | None):
        self._chk(L.lib().ms_set_stream(self._h, ctypes.c_void_p(hip_stream or 0)), "ms_set_stream")

    def set_surface_tension(self, gamma):
        g = _f64(gamma, (self.nf,), "gamma")
        self._chk(L.lib().ms_set_surface_tension(self._h, _pd(g)), "ms_set_surface_tension")

    def set_bending_params(self, kappa, c0):
        k = _f64(kappa, (self.nv,), "kappa")
        z = _f64(c0, (self.nv,), "c0")
        self._chk(L.lib().ms_set_bending_params(self._h, _pd(k), _pd(z)), "ms_set_bending_params")

    def set_params(self, *, modules: int, bending_model: int = L.MS_BEND_HELFRICH,
                   bending_grad_mode: int = L.MS_GRAD_ANALYTIC, volume_stiffness: float = 1000.0,
                   target_volume: float = 0.0):
        self._params = L.ms_params(int(modules), int(bending_model), int(bending_grad_mode),
                                   float(volume_stiffness), float(target_volume))
        self._chk(L.lib().ms_set_params(self._h, ctypes.byref(self._params)), "ms_set_params")

    def set_area_penalty(self, stiffness: float, target_area: float):
        """k and A0 of the body_area_penalty module (used while MS_MOD_AREA_PENALTY is in the module mask)."""
        self._area_penalty = (float(stiffness), float(target_area))
        self._chk(L.lib().ms_set_area_penalty(self._h, float(stiffness), float(target_area)), "ms_set_area_penalty")

    def set_area_constraint(self, kind: int, target_area: float = 0.0):
        """body_area (L.MS_AREA_BODY: the body's facets) or global_area (L.MS_AREA_GLOBAL: every facet) with its target;
        L.MS_AREA_NONE clears it (ms_set_area_constraint)."""
        self._chk(L.lib().ms_set_area_constraint(self._h, int(kind), float(target_area)), "ms_set_area_constraint")
        self._area_constraint = (int(kind), float(target_area)) if kind != L.MS_AREA_NONE else None

    @property
    def area_constraint(self):
        """(kind, target) of the area constraint that is set, or None."""
        return self.__dict__.get("_area_constraint")

    def project_area(self, tol: float = 1e-12, max_iter: int = 20, first_step_cached: bool = False):
        """enforce_constraint of the area constraint that is set, on the device positions; ``first_step_cached``: Body's
        cached-area quirk (include/membrane_hip.h, ms_project_area_cached).  -> (steps taken, area of the last evaluation)"""
        it = ctypes.c_int(0)
        a = ctypes.c_double(0.0)
        self._chk(L.lib().ms_project_area_cached(self._h, float(tol), int(max_iter), int(bool(first_step_cached)),
                                                 ctypes.byref(it), ctypes.byref(a)), "ms_project_area_cached")
        return int(it.value), float(a.value)

    def area_row(self):
        """dA/dx of the area constraint that is set at the device positions -> (row (nv,3), area, <gA,gA>)."""
        row = np.zeros((self.nv, 3))
        a = ctypes.c_double(0.0)
        n2 = ctypes.c_double(0.0)
        self._chk(L.lib().ms_area_row(self._h, _pd(row), ctypes.byref(a), ctypes.byref(n2)), "ms_area_row")
        return row, float(a.value), float(n2.value)

    def area_stats(self) -> dict:
        """Launch counts of the area lane's kernels (ms_area_stats)."""
        s = np.zeros(4)
        self._chk(L.lib().ms_area_stats(self._h, _pd(s)), "ms_area_stats")
        return {"row": int(s[0]), "dots": int(s[1]), "fold": int(s[2]), "apply": int(s[3])}

    def body_area(self) -> float:
        """Area of the body's facets as the last energy pass folded it (MS_S_AREA)."""
        a = ctypes.c_double(0.0)
        self._chk(L.lib().ms_get_body_area(self._h, ctypes.byref(a)), "ms_get_body_area")
        return float(a.value)

    def area_penalty_energy(self) -> float:
        """1/2 k (A - A0)^2 of the last energy pass, the reference's expression (body_area_penalty.py:136-137)."""
        k, a0 = getattr(self, "_area_penalty", (0.0, 0.0))
        delta = self.body_area() - a0
        return 0.5 * k * delta * delta

    def _set_edge_term(self, entry, what, tail, head, col, *extra):
        """One setter of the edge lane: external rows with their column, or no arguments to clear the tables."""
        fn = getattr(L.lib(), entry)
        if tail is None:
            self._chk(fn(self._h, 0, None, None, None, *[0.0 for _ in extra]), entry)
            return
        (t, pt), (h, ph) = _i32_table(tail), _i32_table(head)
        c = np.ascontiguousarray(np.asarray(col, dtype=np.float64).reshape(-1))
        if not (len(t) == len(h) == len(c)):
            raise ValueError(f"{entry[3:]}: tail, head and {what} must have the same length")
        self._chk(fn(self._h, len(t), pt, ph, _pd(c if len(c) else np.zeros(1)), *extra), entry)

    def _edge_term_energy(self, entry) -> float:
        e = ctypes.c_double(0.0)
        self._chk(getattr(L.lib(), entry)(self._h, ctypes.byref(e)), entry)
        return float(e.value)

    def _edge_term_stats(self, entry):
        v = np.zeros(4)
        self._chk(getattr(L.lib(), entry)(self._h, _pd(v)), entry)
        return {"energy_launches": int(v[0]), "grad_launches": int(v[1]), "energy_us": float(v[2]),
                "grad_us": float(v[3])}

    def set_line_tension(self, tail=None, head=None, gamma=None):
        """Tagged edges of the line_tension module as external rows with their gamma, in ascending edge order (used
        while MS_MOD_LINE_TENSION is in the module mask); no arguments clear the tables."""
        self._set_edge_term("ms_set_line_tension", "gamma", tail, head, gamma)

    def line_energy(self) -> float:
        """The line_tension module's own energy as the last energy pass summed it (ms_get_line_energy)."""
        return self._edge_term_energy("ms_get_line_energy")

    def line_stats(self):
        """Launch counts of the two line_tension kernels and their event-timed microseconds (ms_line_stats)."""
        return self._edge_term_stats("ms_line_stats")

    def set_edge_length_penalty(self, tail=None, head=None, target_length=None, k=100.0):
        """Charged edges of the edge_length_penalty module as external rows with their target lengths, in ascending
        edge order, and the one stiffness k (used while MS_MOD_EDGE_LENGTH_PENALTY is in the module mask); no
        arguments clear the tables."""
        self._set_edge_term("ms_set_edge_length_penalty", "target_length", tail, head, target_length, float(k))

    def edge_penalty_energy(self) -> float:
        """The edge_length_penalty module's own energy as the last energy pass summed it
        (ms_get_edge_penalty_energy)."""
        return self._edge_term_energy("ms_get_edge_penalty_energy")

    def edge_penalty_stats(self):
        """Launch counts of the two edge_length_penalty kernels and their event-timed microseconds
        (ms_edge_penalty_stats)."""
        return self._edge_term_stats("ms_edge_penalty_stats")

    @property
    def modules(self) -> int:
        return int(self._params.modules)

    # -- host <-> HBM ---------------------------------------------------------
    def set_positions(self, positions):
        p = _f64(positions, (self.nv, 3), "positions")
        self._chk(L.lib().ms_set_positions(self._h, _pd(p)), "ms_set_positions")

    def get_positions(self) -> np.ndarray:
        out = np.empty((self.nv, 3), dtype=np.float64)
        self._chk(L.lib().ms_get_positions(self._h, _pd(out)), "ms_get_positions")
        return out

    def get_gradient(self) -> np.ndarray:
        out = np.empty((self.nv, 3), dtype=np.float64)
        self._chk(L.lib().ms_get_gradient(self._h, _pd(out)), "ms_get_gradient")
        return out

    def get_vertex_buffer(self, buffer: int) -> np.ndarray:
        ncomp = 2 if buffer == L.MS_BUF_FA else 3
        out = np.empty((self.nv, ncomp), dtype=np.float64)
        self._chk(L.lib().ms_get_vertex_buffer(self._h, int(buffer), _pd(out)), "ms_get_vertex_buffer")
        return out

    # -- evaluation -----------------------------------------------------------
    def set_tilts(self, tilts, tilt_rigidity: float):
        t = _f64(tilts, (self.nv, 3), "tilts")
        self._chk(L.lib().ms_set_tilts(self._h, _pd(t), float(tilt_rigidity)), "ms_set_tilts")

    def get_tilts(self) -> np.ndarray:
        out = np.empty((self.nv, 3), dtype=np.float64)
        self._chk(L.lib().ms_get_tilts(self._h, _pd(out)), "ms_get_tilts")
        return out

    def get_tilt_gradient(self) -> np.ndarray:
        out = np.empty((self.nv, 3), dtype=np.float64)
        self._chk(L.lib().ms_get_tilt_gradient(self._h, _pd(out)), "ms_get_tilt_gradient")
        return out

    def set_tilt_fixed(self, tilt_fixed=None):
        """vertex.tilt_fixed flags of the reference (None clears them)."""
        if tilt_fixed is None:
            ptr = None
        else:
            arr = np.ascontiguousarray(np.asarray(tilt_fixed, dtype=bool).astype(np.uint8))
            if arr.shape != (self.nv,):
                raise ValueError("tilt_fixed must have shape (nv,)")
            ptr = arr.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
        self._chk(L.lib().ms_set_tilt_fixed(self._h, ptr), "ms_set_tilt_fixed")

    def set_deterministic(self, on: bool = True):
        """Fixed-order (bitwise reproducible) per-vertex sums instead of LDS atomics (~20 % slower)."""
        self._chk(L.lib().ms_set_deterministic(self._h, int(bool(on))), "ms_set_deterministic")

    def set_tilt_smoothness(self, k_smooth: float):
        self._chk(L.lib().ms_set_tilt_smoothness(self._h, float(k_smooth)), "ms_set_tilt_smoothness")

    def tilt_energy_and_gradient(self, want_gradient: bool = True):
        """-> (energy of the tilt-reading modules, dE/dt (nv,3) or None) at the stored tilts."""
        e = ctypes.c_double(0.0)
        out = np.empty((self.nv, 3), dtype=np.float64) if want_gradient else None
        self._chk(L.lib().ms_tilt_energy_and_gradient(self._h, ctypes.byref(e), _pd(out) if want_gradient else None),
                  "ms_tilt_energy_and_gradient")
        return float(e.value), out

    def relax_tilts(self, *, solver: str = "cg", max_iters: int, step_size: float, tol: float = 0.0,
                    jacobi: bool = True):
        """TiltRelaxationManager.relax_tilts on the device -> (iterations, energy evaluations)."""
        rp = L.ms_tilt_relax_params(1 if solver == "cg" else 0, int(max_iters), float(step_size), float(tol),
                                    1 if jacobi else 0)
        it, ev = ctypes.c_int(0), ctypes.c_int(0)
        self._chk(L.lib().ms_relax_tilts(self._h, ctypes.byref(rp), ctypes.byref(it), ctypes.byref(ev)),
                  "ms_relax_tilts")
        return int(it.value), int(ev.value)

    # -- two-leaflet tilt fields (tilts_in / tilts_out) ----------------------------
    def set_leaflet_tilts(self, leaflet: str, tilts, *, tilt_fixed=None, tilt_modulus: float = 0.0,
                          mass_mode: str = "lumped", smoothness: float = 0.0,
                          precond_smoothness: float | None = None):
        """Mesh.tilts_in_view()/tilts_out_view() + the leaflet's module parameters."""
        lf = {"in": L.MS_LEAFLET_IN, "out": L.MS_LEAFLET_OUT}[leaflet]
        arr = _f64(tilts, (self.nv, 3), f"tilts_{leaflet}")
        if tilt_fixed is None:
            ptr = None
        else:
            fx = np.ascontiguousarray(np.asarray(tilt_fixed, dtype=bool).astype(np.uint8))
            if fx.shape != (self.nv,):
                raise ValueError("tilt_fixed must have shape (nv,)")
            ptr = fx.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
        if mass_mode not in ("lumped", "consistent"):
            raise ValueError(f"tilt_mass_mode_{leaflet} must be 'lumped' or 'consistent'.")
        lp = L.ms_leaflet_params(float(tilt_modulus), 1 if mass_mode == "consistent" else 0, float(smoothness),
                                 float(smoothness if precond_smoothness is None else precond_smoothness))
        self._chk(L.lib().ms_set_leaflet_tilts(self._h, lf, _pd(arr), ptr, ctypes.byref(lp)), "ms_set_leaflet_tilts")

    def set_leaflet_absent(self, leaflet: str, absent=None):
        """Rows the leaflet is absent on (leaflet_presence.py:34-122; None clears them): tilt_out and
        tilt_smoothness_out skip every facet that touches one, a relaxation's outer vertex areas are the kept facets'.
        Only the outer leaflet has a mask on the device (include/membrane_hip.h, ms_set_leaflet_absent)."""
        lf = {"in": L.MS_LEAFLET_IN, "out": L.MS_LEAFLET_OUT}[leaflet]
        if absent is None:
            ptr = None
        else:
            arr = np.ascontiguousarray(np.asarray(absent, dtype=bool).astype(np.uint8))
            if arr.shape != (self.nv,):
                raise ValueError("absent must have shape (nv,)")
            ptr = arr.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
        self._chk(L.lib().ms_set_leaflet_absent(self._h, lf, ptr), "ms_set_leaflet_absent")

    def set_leaflet_bending(self, leaflet: str, kappa, c0):
        """Per-vertex (kappa, c0) of bending_tilt_in / bending_tilt_out."""
        lf = {"in": L.MS_LEAFLET_IN, "out": L.MS_LEAFLET_OUT}[leaflet]
        k = _f64(np.broadcast_to(np.asarray(kappa, dtype=np.float64), (self.nv,)), (self.nv,), "kappa")
        c = _f64(np.broadcast_to(np.asarray(c0, dtype=np.float64), (self.nv,)), (self.nv,), "c0")
        self._chk(L.lib().ms_set_leaflet_bending(self._h, lf, _pd(k), _pd(c)), "ms_set_leaflet_bending")

    def set_leaflet_disk_target(self, leaflet: str, disk_rows, *, strength: float, theta_b: float, lam: float,
                                center=(0.0, 0.0, 0.0), normal=(0.0, 0.0, 1.0), radius: float | None = None):
        """tilt_disk_target_in/out: tagged rows (bool mask or row indices) and the profile parameters."""
        lf = {"in": L.MS_LEAFLET_IN, "out": L.MS_LEAFLET_OUT}[leaflet]
        rows = np.asarray(disk_rows)
        if rows.dtype == bool:
            mask = rows.astype(np.uint8)
        else:
            mask = np.zeros(self.nv, dtype=np.uint8)
            mask[rows.astype(np.int64)] = 1
        if mask.shape != (self.nv,):
            raise ValueError("disk_rows must be a (nv,) mask or a list of rows")
        mask = np.ascontiguousarray(mask)
        p = L.ms_disk_target_params(float(strength), float(theta_b), float(lam), _vec3(center), _vec3(normal),
                                    float(radius or 0.0))
        self._chk(L.lib().ms_set_leaflet_disk_target(self._h, lf, mask.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                                     ctypes.byref(p)), "ms_set_leaflet_disk_target")

    def _set_rim_source(self, entry, lead, tail, head, gamma, center, normal, follow):
        """One setter of the rim tables (``lead``: the entry point's arguments in front of the edge count): external rows
        with their gamma and the circle's frame, or no edges to clear the tables."""
        fn = getattr(L.lib(), entry)
        if tail is None:
            self._chk(fn(self._h, *lead, 0, None, None, None, None), entry)
            return
        (t, pt), (h, ph) = _i32_table(tail), _i32_table(head)
        g = np.ascontiguousarray(np.asarray(gamma, dtype=np.float64).reshape(-1))
        if not (len(t) == len(h) == len(g)):
            raise ValueError(f"{entry[3:]}: tail, head and gamma must have the same length")
        p = L.ms_rim_source_params(_vec3(center), _vec3(normal), 1 if follow else 0)
        self._chk(fn(self._h, *lead, len(t), pt, ph, _pd(g if len(g) else np.zeros(1)), ctypes.byref(p)), entry)

    def set_leaflet_rim_source(self, leaflet: str, tail=None, head=None, gamma=None, *, center=(0.0, 0.0, 0.0),
                               normal=(0.0, 0.0, 1.0), follow: bool = False):
        """tilt_rim_source_in/out: the rim edges as external rows with their strength gamma, and the circle's frame
        (``follow``: the center is the mean of the rim rows of the evaluated positions); no edges clear the tables."""
        lf = {"in": L.MS_LEAFLET_IN, "out": L.MS_LEAFLET_OUT}[leaflet]
        self._set_rim_source("ms_set_leaflet_rim_source", (lf,), tail, head, gamma, center, normal, follow)

    def leaflet_rim_source_energy(self, leaflet: str) -> float:
        """The rim source's own energy as the last evaluation summed it (ms_get_leaflet_rim_source_energy)."""
        lf = {"in": L.MS_LEAFLET_IN, "out": L.MS_LEAFLET_OUT}[leaflet]
        e = ctypes.c_double(0.0)
        self._chk(L.lib().ms_get_leaflet_rim_source_energy(self._h, lf, ctypes.byref(e)),
                  "ms_get_leaflet_rim_source_energy")
        return float(e.value)

    def leaflet_rim_source_stats(self, leaflet: str):
        """Launch counts of the rim source's three kernels (ms_leaflet_rim_source_stats)."""
        lf = {"in": L.MS_LEAFLET_IN, "out": L.MS_LEAFLET_OUT}[leaflet]
        v = np.zeros(3)
        self._chk(L.lib().ms_leaflet_rim_source_stats(self._h, lf, _pd(v)), "ms_leaflet_rim_source_stats")
        return {"frame_launches": int(v[0]), "coef_launches": int(v[1]), "apply_launches": int(v[2])}

    def set_rim_source_bilayer(self, tail=None, head=None, gamma=None, *, center=(0.0, 0.0, 0.0),
                               normal=(0.0, 0.0, 1.0), follow: bool = False):
        """tilt_rim_source_bilayer: set_leaflet_rim_source's tables, kept once for both leaflet fields
        (ms_set_rim_source_bilayer); no edges clear them."""
        self._set_rim_source("ms_set_rim_source_bilayer", (), tail, head, gamma, center, normal, follow)

    def rim_source_bilayer_energy(self) -> float:
        """The bilayer rim source's own energy as the last evaluation summed it (ms_get_rim_source_bilayer_energy)."""
        e = ctypes.c_double(0.0)
        self._chk(L.lib().ms_get_rim_source_bilayer_energy(self._h, ctypes.byref(e)), "ms_get_rim_source_bilayer_energy")
        return float(e.value)

    def rim_source_bilayer_stats(self):
        """Launch counts of the bilayer rim source's three kernels (ms_rim_source_bilayer_stats)."""
        v = np.zeros(3)
        self._chk(L.lib().ms_rim_source_bilayer_stats(self._h, _pd(v)), "ms_rim_source_bilayer_stats")
        return {"frame_launches": int(v[0]), "coef_launches": int(v[1]), "apply_launches": int(v[2])}

    def set_tilt_coupling(self, modulus: float, sign: int):
        """tilt_coupling: modulus k_c and sign -1 ("difference"), +1 ("sum") or 0 (off) (ms_set_tilt_coupling)."""
        self._chk(L.lib().ms_set_tilt_coupling(self._h, float(modulus), int(sign)), "ms_set_tilt_coupling")

    def tilt_coupling_energy(self) -> float:
        """The coupling's own energy as its last launch summed it, whatever that launch evaluated
        (ms_get_tilt_coupling_energy); call energy() first to read it for the stored state."""
        e = ctypes.c_double(0.0)
        self._chk(L.lib().ms_get_tilt_coupling_energy(self._h, ctypes.byref(e)), "ms_get_tilt_coupling_energy")
        return float(e.value)

    def tilt_coupling_stats(self):
        """Launch counts of the coupling's kernels (ms_tilt_coupling_stats)."""
        v = np.zeros(3)
        self._chk(L.lib().ms_tilt_coupling_stats(self._h, _pd(v)), "ms_tilt_coupling_stats")
        return {"energy_launches": int(v[0]), "gradient_launches": int(v[1]), "vec_launches": int(v[2])}

    def set_tilt_splay_twist(self, k_splay: float, k_twist: float):
        """tilt_splay_twist_in: the splay and twist moduli, finite and non-negative (ms_set_tilt_splay_twist)."""
        self._chk(L.lib().ms_set_tilt_splay_twist(self._h, float(k_splay), float(k_twist)), "ms_set_tilt_splay_twist")

    def tilt_splay_twist_energy(self) -> float:
        """The splay / twist term's own energy as its last launch summed it, whatever that launch evaluated
        (ms_get_tilt_splay_twist_energy); call energy() first to read it for the stored state."""
        e = ctypes.c_double(0.0)
        self._chk(L.lib().ms_get_tilt_splay_twist_energy(self._h, ctypes.byref(e)), "ms_get_tilt_splay_twist_energy")
        return float(e.value)

    def tilt_splay_twist_stats(self):
        """Launch counts of the splay / twist kernels (ms_tilt_splay_twist_stats)."""
        v = np.zeros(2)
        self._chk(L.lib().ms_tilt_splay_twist_stats(self._h, _pd(v)), "ms_tilt_splay_twist_stats")
        return {"energy_launches": int(v[0]), "gradient_launches": int(v[1])}

    def set_thetab_contact(self, rows=None, *, center=(0.0, 0.0, 0.0), normal=(0.0, 0.0, 1.0), k: float = 0.0,
                           gamma: float = 0.0, work_mode: str = "scalar", penalty_mode: str = "off"):
        """tilt_thetaB_contact_in: the ring's rows (external, in vertex_ids order), frame and strengths
        (ms_set_thetab_contact); no rows clear the tables."""
        if rows is None:
            self._chk(L.lib().ms_set_thetab_contact(self._h, 0, None, None), "ms_set_thetab_contact")
            return
        r, pr = _i32_table(rows)
        work = {"scalar": L.MS_THETAB_WORK_SCALAR, "field_linear": L.MS_THETAB_WORK_FIELD_LINEAR}
        penalty = {"off": 0, "legacy": 1}
        if work_mode not in work or penalty_mode not in penalty:  # (leaflet_common.thetab_contact_modes resolves the aliases)
            raise ValueError("set_thetab_contact: work_mode must be 'scalar' or 'field_linear' and penalty_mode 'off' or "
                             f"'legacy', not {work_mode!r} / {penalty_mode!r}")
        p = L.ms_thetab_contact_params(_vec3(center), _vec3(normal), float(k), float(gamma), work[work_mode],
                                       penalty[penalty_mode])
        self._chk(L.lib().ms_set_thetab_contact(self._h, len(r), pr, ctypes.byref(p)), "ms_set_thetab_contact")

    def set_thetab_value(self, theta_b: float):
        """theta_B of the contact term (tilt_thetaB_value, ms_set_thetab_value)."""
        self._chk(L.lib().ms_set_thetab_value(self._h, float(theta_b)), "ms_set_thetab_value")

    def thetab_contact_energy(self) -> float:
        """The contact term's own energy as the last evaluation summed it (ms_get_thetab_contact_energy)."""
        e = ctypes.c_double(0.0)
        self._chk(L.lib().ms_get_thetab_contact_energy(self._h, ctypes.byref(e)), "ms_get_thetab_contact_energy")
        return float(e.value)

    def thetab_contact_scalars(self):
        """{sum w theta / wsum, R_eff, wsum} of the last evaluation (ms_get_thetab_contact_scalars)."""
        v = np.zeros(3)
        self._chk(L.lib().ms_get_thetab_contact_scalars(self._h, _pd(v)), "ms_get_thetab_contact_scalars")
        return {"theta_mean": float(v[0]), "r_eff": float(v[1]), "wsum": float(v[2])}

    def update_thetab_value(self):
        """update_scalar_params on the device's positions and stored inner tilts (ms_update_thetab_value): the stored
        theta_B and whether the call replaced it."""
        tb, ch = ctypes.c_double(0.0), ctypes.c_int(0)
        self._chk(L.lib().ms_update_thetab_value(self._h, ctypes.byref(tb), ctypes.byref(ch)), "ms_update_thetab_value")
        return float(tb.value), bool(ch.value)

    def thetab_contact_stats(self):
        """Launch counts of the contact term's two kernels (ms_thetab_contact_stats)."""
        v = np.zeros(2)
        self._chk(L.lib().ms_thetab_contact_stats(self._h, _pd(v)), "ms_thetab_contact_stats")
        return {"geom_launches": int(v[0]), "apply_launches": int(v[1])}

    def set_rim_match(self, rim=None, outer=None, disk=None, *, center=(0.0, 0.0, 0.0), normal=(0.0, 0.0, 1.0),
                      strength: float = 0.0):
        """rim_slope_match_out: the rim, outer and optional disk rows (external, each in vertex_ids order), frame and
        strength (ms_set_rim_match); no rim rows clear the tables (ms_clear_rim_match)."""
        if self.shard_count != 1:  # (the library refuses it as well)
            raise L.MembraneHipError("the rim_slope_match_out module is not sharded (single GPU only)")
        if rim is None:
            self._chk(L.lib().ms_clear_rim_match(self._h), "ms_clear_rim_match")
            return
        (r, p_r), (o, p_o), (d, p_d) = (_i32_table([] if t is None else t) for t in (rim, outer, disk))
        p = L.ms_rim_match_params(_vec3(center), _vec3(normal), float(strength))
        self._chk(L.lib().ms_set_rim_match(self._h, len(r), p_r, len(o), p_o, len(d), p_d, ctypes.byref(p)), "ms_set_rim_match")

    def rim_match_energy(self) -> float:
        """The rim matching term's own energy as the last evaluation summed it (ms_get_rim_match_energy)."""
        return self.rim_match_energies()[0]

    def rim_match_energies(self):
        """(E, E_out, E_in) of the last evaluation: the module's energy and its outer- and inner-leaflet terms."""
        v = np.zeros(3)
        self._chk(L.lib().ms_get_rim_match_energy(self._h, _pd(v)), "ms_get_rim_match_energy")
        return float(v[0]), float(v[1]), float(v[2])

    def rim_match_stats(self):
        """Launch counts of the rim matching term's two kernels (ms_rim_match_stats)."""
        v = np.zeros(2)
        self._chk(L.lib().ms_rim_match_stats(self._h, _pd(v)), "ms_rim_match_stats")
        return {"geom_launches": int(v[0]), "apply_launches": int(v[1])}

    def set_thetab_boundary(self, rows=None, *, center=(0.0, 0.0, 0.0), normal=(0.0, 0.0, 1.0)):
        """tilt_thetaB_boundary_in: the constraint's ring (external rows, in vertex_ids order) and frame
        (ms_set_thetab_boundary); no rows clear the table.  theta_B is set_thetab_value's."""
        if self.shard_count != 1:  # (the library refuses it as well)
            raise L.MembraneHipError("the tilt_thetaB_boundary_in constraint is not sharded (single GPU only)")
        if rows is None:
            self._chk(L.lib().ms_set_thetab_boundary(self._h, 0, None, None), "ms_set_thetab_boundary")
            self._thetab_boundary_rows = 0
            return
        r, pr = _i32_table(rows)
        p = L.ms_thetab_boundary_params(_vec3(center), _vec3(normal))
        self._chk(L.lib().ms_set_thetab_boundary(self._h, len(r), pr, ctypes.byref(p)), "ms_set_thetab_boundary")
        self._thetab_boundary_rows = len(r)

    def set_tilt_projection(self, cadence: str = "per_step", interval: int = 1):
        """tilt_projection_cadence / tilt_projection_interval of the leaflet relaxation (ms_set_tilt_projection)."""
        codes = {"per_step": L.MS_TILT_PROJECTION_PER_STEP, "per_pass": L.MS_TILT_PROJECTION_PER_PASS}
        if cadence not in codes:
            raise ValueError("tilt_projection_cadence must be 'per_step' or 'per_pass'.")
        if int(interval) < 1:
            raise ValueError("tilt_projection_interval must be >= 1.")
        self._chk(L.lib().ms_set_tilt_projection(self._h, codes[cadence], int(interval)), "ms_set_tilt_projection")

    def thetab_boundary_enforce(self):
        """t_in <- t_in + (theta_B - t_in . d) d on the ring's kept, free rows, on the context's positions and stored
        inner tilts (ms_thetab_boundary_enforce)."""
        self._chk(L.lib().ms_thetab_boundary_enforce(self._h), "ms_thetab_boundary_enforce")

    def thetab_boundary_directions(self):
        """-> (d (n_rows,3), keep (n_rows,) bool) of the table's rows on the context's positions
        (ms_thetab_boundary_directions)."""
        n = int(getattr(self, "_thetab_boundary_rows", 0))
        d, keep = np.zeros((max(n, 1), 3)), np.zeros(max(n, 1), dtype=np.uint8)
        self._chk(L.lib().ms_thetab_boundary_directions(self._h, _pd(d), keep.ctypes.data_as(L._U8)),
                  "ms_thetab_boundary_directions")
        return d[:n], keep[:n].astype(bool)

    def thetab_boundary_projected_gradient(self):
        """-> (tilt-dependent energy, dE/dt_in, dE/dt_out) as the relaxation sees them: the inner gradient projected
        against the constraint's rows, fixed rows zeroed (ms_thetab_boundary_projected_gradient)."""
        e = ctypes.c_double(0.0)
        gi, go = np.empty((self.nv, 3), dtype=np.float64), np.empty((self.nv, 3), dtype=np.float64)
        self._chk(L.lib().ms_thetab_boundary_projected_gradient(self._h, ctypes.byref(e), _pd(gi), _pd(go)),
                  "ms_thetab_boundary_projected_gradient")
        return float(e.value), gi, go

    def thetab_boundary_stats(self):
        """Launch counts of the constraint's kernels (ms_thetab_boundary_stats)."""
        v = np.zeros(3)
        self._chk(L.lib().ms_thetab_boundary_stats(self._h, _pd(v)), "ms_thetab_boundary_stats")
        return {"geom_launches": int(v[0]), "enforce_launches": int(v[1]), "project_launches": int(v[2])}

    def get_leaflet_tilts(self, leaflet: str) -> np.ndarray:
        out = np.empty((self.nv, 3), dtype=np.float64)
        lf = {"in": L.MS_LEAFLET_IN, "out": L.MS_LEAFLET_OUT}[leaflet]
        self._chk(L.lib().ms_get_leaflet_tilts(self._h, lf, _pd(out)), "ms_get_leaflet_tilts")
        return out

    def leaflet_tilt_energy_and_gradient(self, want_gradient: bool = True, module_form: bool = False):
        """-> (tilt-dependent energy, dE/dt_in, dE/dt_out) at frozen positions, magnitude modules
        in their vertex-area form (evaluation_manager.py:630-742 with tilt_vertex_areas); with
        ``module_form`` in their own mass mode, as the plugin API evaluates them
        (tilt_leaflet.py:101-150: lumped, or consistent k A/12 (2 t_k + t_a + t_b))."""
        e = ctypes.c_double(0.0)
        gi = np.empty((self.nv, 3), dtype=np.float64) if want_gradient else None
        go = np.empty((self.nv, 3), dtype=np.float64) if want_gradient else None
        self._chk(L.lib().ms_leaflet_tilt_energy_and_gradient_ex(
            self._h, 1 if module_form else 0, ctypes.byref(e), _pd(gi) if want_gradient else None,
            _pd(go) if want_gradient else None), "ms_leaflet_tilt_energy_and_gradient_ex")
        return float(e.value), gi, go

    def relax_leaflet_tilts(self, *, solver: str = "cg", max_iters: int, step_size: float, tol: float = 0.0,
                            jacobi: bool = True):
        """TiltRelaxationManager.relax_leaflet_tilts on the device -> (iterations, energy evaluations)."""
        rp = L.ms_tilt_relax_params(1 if solver == "cg" else 0, int(max_iters), float(step_size), float(tol),
                                    1 if jacobi else 0)
        it, ev = ctypes.c_int(0), ctypes.c_int(0)
        self._chk(L.lib().ms_relax_leaflet_tilts(self._h, ctypes.byref(rp), ctypes.byref(it), ctypes.byref(ev)),
                  "ms_relax_leaflet_tilts")
        return int(it.value), int(ev.value)

    def leaflet_relax_geometry(self, leaflet: str):
        """-> (vertex areas (nv,), clamped inverse Jacobi diagonal (nv,)) the last relax_leaflet_tilts left for this
        leaflet (include/membrane_hip.h, ms_get_leaflet_relax_geometry)."""
        lf = {"in": L.MS_LEAFLET_IN, "out": L.MS_LEAFLET_OUT}[leaflet]
        va, minv = np.empty(self.nv, dtype=np.float64), np.empty(self.nv, dtype=np.float64)
        self._chk(L.lib().ms_get_leaflet_relax_geometry(self._h, lf, _pd(va), _pd(minv)), "ms_get_leaflet_relax_geometry")
        return va, minv

    def angle_defects(self) -> np.ndarray:
        """Per-vertex angle defects (integrated Gaussian curvature) at the current positions."""
        out = np.empty(self.nv, dtype=np.float64)
        self._chk(L.lib().ms_angle_defects(self._h, _pd(out)), "ms_angle_defects")
        return out

    def curvature_fields(self) -> dict:
        """geometry/curvature.compute_curvature_fields at the context's positions (ms_curvature_fields) + the raw
        per-vertex angle sums."""
        a, b, c, d = (np.empty((self.nv, 3), dtype=np.float64) for _ in range(4))
        self._chk(L.lib().ms_curvature_fields(self._h, _pd(a), _pd(b), _pd(c), _pd(d)), "ms_curvature_fields")
        return {"mean_curvature_normal": a, "mean_curvature": b[:, 0].copy(), "mixed_area": b[:, 1].copy(),
                "angle_sum": b[:, 2].copy(), "angle_defect": c[:, 0].copy(), "gaussian_curvature": c[:, 1].copy(),
                "principal_curvatures": d[:, :2].copy()}

    def project_tilts_to_tangent(self):
        self._chk(L.lib().ms_project_tilts_to_tangent(self._h), "ms_project_tilts_to_tangent")

    def energy_and_gradient(self, want_grad: bool = True, raw: bool = False):
        """-> (energies[surface, bending, volume_penalty, tilt], grad (nv,3) | None).  ``raw``: the module loop's
        plain sum as an energy-module plugin accumulates it -- fixed rows not zeroed, no constraint projection."""
        e = np.zeros(4)
        g = np.empty((self.nv, 3), dtype=np.float64) if want_grad else None
        if raw:
            self._chk(L.lib().ms_energy_and_raw_gradient(self._h, _pd(e), _pd(g)), "ms_energy_and_raw_gradient")
        else:
            self._chk(L.lib().ms_energy_and_gradient(self._h, _pd(e), _pd(g)), "ms_energy_and_gradient")
        return e, g

    def energy(self) -> np.ndarray:
        e = np.zeros(4)
        self._chk(L.lib().ms_energy(self._h, _pd(e)), "ms_energy")
        return e

    # -- stepping -------------------------------------------------------------
    def step(self, *, stepper: int, step_size: float, tol: float = 1e-6, max_iter: int = 10,
             beta: float = 0.7, c: float = 1e-4, gamma: float = 1.5, alpha_max_factor: float = 10.0,
             restart_interval: int = 10, edge_fraction: float = 0.0,
             reuse_energy0: int = 0, enforce_volume: int = 0, precondition: int = 0,
             enforce_pins: int = 0, enforce_area: int = 0, enforce_fixed_plane: int = 0,
             enforce_perimeter: int = 0) -> StepResult:
        # the parameter block and the result struct are reused between calls: at ~140 us per
        # step every microsecond of ctypes marshalling shows
        key = (stepper, max_iter, beta, c, gamma, alpha_max_factor, restart_interval, edge_fraction,
               reuse_energy0, enforce_volume, precondition, enforce_pins, enforce_area, enforce_fixed_plane,
               enforce_perimeter)
        cache = self.__dict__.get("_step_cache")
        if cache is None or cache[0] != key:
            sp = L.ms_stepper_params(int(stepper), int(max_iter), float(beta), float(c), float(gamma),
                                     float(alpha_max_factor), int(restart_interval), float(edge_fraction),
                                     int(reuse_energy0), int(enforce_volume), int(precondition),
                                     int(enforce_pins), int(bool(enforce_fixed_plane)), int(bool(enforce_perimeter)),
                                     int(enforce_area > 0), int(enforce_area))
            r = L.ms_step_result()
            cache = (key, sp, r, ctypes.byref(sp), ctypes.byref(r), L.lib().ms_step)
            self._step_cache = cache
        _k, sp, r, sp_ref, r_ref, fn = cache
        rc = fn(self._h, sp_ref, step_size, tol, r_ref)
        if rc != 0:
            self._chk(rc, "ms_step")
        return StepResult(r.success != 0, r.converged != 0, r.trials, r.guard_rejects, r.next_step, r.energy,
                          r.alpha, r.energy_eval, r.grad_norm, r.g_dot_d, r.volume)

    def minimize(self, params: "L.ms_minimize_params", n_steps: int, want_log: bool = False):
        """ms_minimize: n_steps iterations of the minimizer loop inside the library.
        -> (ms_minimize_result, step_log (iterations,8) | None)"""
        out = L.ms_minimize_result()
        log = np.zeros((int(n_steps), 8)) if want_log else None
        self._chk(L.lib().ms_minimize(self._h, ctypes.byref(params), int(n_steps), ctypes.byref(out),
                                      _pd(log) if want_log else None), "ms_minimize")
        return out, (log[: out.iterations] if want_log else None)

    def reset_stepper(self):
        self._chk(L.lib().ms_reset_stepper(self._h), "ms_reset_stepper")

    def project_volume(self, target: float, tol: float = 1e-12, max_iter: int = 3, first_step_cached: bool = False):
        """volume.enforce_constraint's projection loop; ``first_step_cached``: Body's cached-gradient quirk
        (include/membrane_hip.h, ms_project_volume_cached)."""
        it = ctypes.c_int(0)
        v = ctypes.c_double(0.0)
        self._chk(L.lib().ms_project_volume_cached(self._h, float(target), float(tol), int(max_iter),
                                                   int(bool(first_step_cached)), ctypes.byref(it), ctypes.byref(v)),
                  "ms_project_volume_cached")
        return int(it.value), float(v.value)

    # -- phase API (multi-GPU drivers) ----------------------------------------
    def phase_energy(self, *, use_direction=False, alpha=0.0, write_trial=False, guard=False,
                     write_bending_factors=False):
        self._chk(L.lib().ms_phase_energy(self._h, int(use_direction), float(alpha), int(write_trial),
                                          int(guard), int(write_bending_factors)), "ms_phase_energy")

    def phase_gradient(self):
        self._chk(L.lib().ms_phase_gradient(self._h), "ms_phase_gradient")

    def phase_direction(self, stepper: int, use_history: bool):
        self._chk(L.lib().ms_phase_direction(self._h, int(stepper), int(use_history)), "ms_phase_direction")

    def phase_accept(self, keep_history: bool):
        self._chk(L.lib().ms_phase_accept(self._h, int(keep_history)), "ms_phase_accept")

    def phase_commit_trial(self, alpha: float, keep_history: bool):
        self._chk(L.lib().ms_phase_commit_trial(self._h, float(alpha), int(keep_history)),
                  "ms_phase_commit_trial")

    def phase_gradient_direction(self, stepper: int, use_history: bool):
        self._chk(L.lib().ms_phase_gradient_direction(self._h, int(stepper), int(use_history)),
                  "ms_phase_gradient_direction")

    def phase_set_factors_valid(self, valid: bool):
        self._chk(L.lib().ms_phase_set_factors_valid(self._h, int(valid)), "ms_phase_set_factors_valid")

    # -- library-side sharded driver ----------------------------------------------
    @staticmethod
    def shard_unique_id() -> bytes:
        buf = ctypes.create_string_buffer(128)
        L.check(L.lib().ms_shard_unique_id(buf), None, "ms_shard_unique_id")
        return buf.raw

    def shard_comm_init(self, unique_id: bytes):
        if len(unique_id) != 128:
            raise ValueError("ncclUniqueId is 128 bytes")
        self._chk(L.lib().ms_shard_comm_init(self._h, ctypes.create_string_buffer(unique_id, 128)),
                  "ms_shard_comm_init")

    def shard_set_allgather(self, fn):
        """fn(send_ptr, recv_ptr, bytes_per_rank) -> None: in-process stand-in for ncclAllGather."""
        def thunk(_user, send, recv, nbytes):
            try:
                fn(int(send), int(recv), int(nbytes))
                return 0
            except Exception:  # pragma: no cover - surfaced as MS_ERR_STATE
                import traceback

                traceback.print_exc()
                return 1

        self._allgather_cb = L.ALLGATHER_FN(thunk)  # keep the trampoline alive
        self._chk(L.lib().ms_shard_set_allgather(self._h, self._allgather_cb, None), "ms_shard_set_allgather")

    # peer-to-peer exchange of the library driver (include/membrane_hip.h, ms_shard_peer_*)
    def shard_peer_local(self):
        """-> (slab pointer, flag-word pointer) of this rank, as integers (contexts of one process exchange these)."""
        a, b = ctypes.c_void_p(), ctypes.c_void_p()
        self._chk(L.lib().ms_shard_peer_local(self._h, ctypes.byref(a), ctypes.byref(b)), "ms_shard_peer_local")
        return int(a.value or 0), int(b.value or 0)

    def shard_peer_set_pointers(self, slabs, flags):
        n = len(slabs)
        a = (ctypes.c_void_p * n)(*[ctypes.c_void_p(int(x)) for x in slabs])
        b = (ctypes.c_void_p * n)(*[ctypes.c_void_p(int(x)) for x in flags])
        self._chk(L.lib().ms_shard_peer_set_pointers(self._h, a, b), "ms_shard_peer_set_pointers")

    def shard_peer_set_barrier(self, fn):
        """fn() -> None: returns once every rank of this process has raised its flags (host-side wait)."""
        def thunk(_user):
            try:
                fn()
                return 0
            except Exception:  # pragma: no cover - surfaced as MS_ERR_STATE
                import traceback

                traceback.print_exc()
                return 1

        self._peer_barrier_cb = L.BARRIER_FN(thunk)  # keep the trampoline alive
        self._chk(L.lib().ms_shard_peer_set_barrier(self._h, ctypes.cast(self._peer_barrier_cb, ctypes.c_void_p), None),
                  "ms_shard_peer_set_barrier")

    def shard_peer_export(self) -> bytes:
        buf = ctypes.create_string_buffer(128)
        self._chk(L.lib().ms_shard_peer_export(self._h, buf), "ms_shard_peer_export")
        return bytes(buf.raw)

    def shard_peer_open(self, handles_all: bytes):
        buf = ctypes.create_string_buffer(bytes(handles_all), len(handles_all))
        self._chk(L.lib().ms_shard_peer_open(self._h, buf), "ms_shard_peer_open")

    def shard_step(self, *, stepper: int, step_size: float, tol: float = 1e-6, max_iter: int = 10,
                   beta: float = 0.7, c: float = 1e-4, gamma: float = 1.5, alpha_max_factor: float = 10.0,
                   restart_interval: int = 10, edge_fraction: float = 0.0, reuse_energy0: int = 2) -> StepResult:
        sp = L.ms_stepper_params(int(stepper), int(max_iter), float(beta), float(c), float(gamma),
                                 float(alpha_max_factor), int(restart_interval), float(edge_fraction),
                                 int(reuse_energy0))
        r = L.ms_step_result()
        self._chk(L.lib().ms_shard_step(self._h, ctypes.byref(sp), float(step_size), float(tol), ctypes.byref(r)),
                  "ms_shard_step")
        return StepResult(r.success != 0, r.converged != 0, r.trials, r.guard_rejects, r.next_step, r.energy,
                          r.alpha, r.energy_eval, r.grad_norm, r.g_dot_d, r.volume)

    def shard_comm_ranks(self) -> int:
        """Ranks of the context's RCCL communicator (ncclCommCount); 0 without one."""
        return int(L.lib().ms_shard_comm_ranks(self._h))

    def shard_exchange_count(self) -> int:
        return int(L.lib().ms_shard_exchange_count(self._h))

    def shard_chain_stats(self):
        """Device-side trial decisions of ms_shard_step and the passes chained behind them (ms_shard_chain_stats)."""
        v = np.zeros(8, dtype=np.int64)
        self._chk(L.lib().ms_shard_chain_stats(self._h, v.ctypes.data_as(L._I64)), "ms_shard_chain_stats")
        return {"queued": int(v[0]), "ran": int(v[1]), "adopted": int(v[2]), "dropped": int(v[3])}

    def peer_memory_kind(self) -> str:
        """Memory kind of the peer exchange's slabs / flag words (ms_shard_peer_memory_kind)."""
        k = int(L.lib().ms_shard_peer_memory_kind(self._h))
        return {0: "uncached device memory", 1: "fine-grained device memory",
                2: "plain hipMalloc (coarse-grained)"}.get(k, "not allocated")

    # -- shard boundary exchange ------------------------------------------------
    def boundary_info(self):
        v = np.zeros(4, dtype=np.int64)
        self._chk(L.lib().ms_boundary_info(self._h, v.ctypes.data_as(L._I64)), "ms_boundary_info")
        return {"max_rows": int(v[0]), "my_rows": int(v[1]), "halo_rows": int(v[2]), "world": int(v[3])}

    @staticmethod
    def _ids(buffers):
        return (ctypes.c_int * max(1, len(buffers)))(*[int(b) for b in buffers])

    def exchange_bytes(self, buffers) -> int:
        return int(L.lib().ms_exchange_bytes(self._h, len(buffers), self._ids(buffers)))

    def pack_boundary(self, buffers, send_ptr: int, send_bytes: int):
        self._chk(L.lib().ms_pack_boundary(self._h, len(buffers), self._ids(buffers),
                                           ctypes.c_void_p(send_ptr), int(send_bytes)), "ms_pack_boundary")

    def unpack_boundary(self, buffers, recv_ptr: int, stride_bytes: int, world: int) -> np.ndarray:
        out = np.zeros((world, L.MS_NSCAL))
        self._chk(L.lib().ms_unpack_boundary(self._h, len(buffers), self._ids(buffers),
                                             ctypes.c_void_p(recv_ptr), int(stride_bytes), _pd(out)),
                  "ms_unpack_boundary")
        return out

    def state_bytes(self) -> int:
        return int(L.lib().ms_state_bytes(self._h))

    def rebind_state(self, device_ptr: int, nbytes: int):
        self._chk(L.lib().ms_rebind_state(self._h, ctypes.c_void_p(device_ptr), int(nbytes)),
                  "ms_rebind_state")

    def fetch_scalars(self) -> np.ndarray:
        out = np.zeros(L.MS_NSCAL)
        self._chk(L.lib().ms_fetch_scalars(self._h, _pd(out)), "ms_fetch_scalars")
        return out

    def store_scalars(self, values):
        v = _f64(values, (L.MS_NSCAL,), "scalars")
        self._chk(L.lib().ms_store_scalars(self._h, _pd(v)), "ms_store_scalars")

    def device_buffer(self, buffer: int):
        p = ctypes.c_void_p()
        n = ctypes.c_size_t(0)
        self._chk(L.lib().ms_device_buffer(self._h, int(buffer), ctypes.byref(p), ctypes.byref(n)),
                  "ms_device_buffer")
        return int(p.value or 0), int(n.value)

    def profile_enable(self, on: bool = True):
        self._chk(L.lib().ms_profile_enable(self._h, int(on)), "ms_profile_enable")

    def profile_read(self):
        """-> {kind: (total_ms, launches)} per kernel kind (include/membrane_hip.h, ms_profile_read)."""
        ms = np.zeros(13)
        n = np.zeros(13, dtype=np.int64)
        self._chk(L.lib().ms_profile_read(self._h, _pd(ms), n.ctypes.data_as(L._I64)), "ms_profile_read")
        names = ("energy", "gradient", "direction", "reduce", "tilt", "bending_tilt", "tilt_vec", "energy_pair", "energy_triple",
                 "gradient_lean", "energy_multi", "tilt_smoothness", "tilt_search")
        return {k: (float(ms[i]), int(n[i])) for i, k in enumerate(names)}

    def queue_stats(self):
        """Line-search queue statistics (include/membrane_hip.h, ms_queue_stats)."""
        v = np.zeros(8, dtype=np.int64)
        self._chk(L.lib().ms_queue_stats(self._h, v.ctypes.data_as(L._I64)), "ms_queue_stats")
        return {"rounds": int(v[0]), "multi_launches": int(v[1]), "wasted_evaluations": int(v[2]),
                "side_accepts": int(v[3]), "mismatches": int(v[4]), "ahead": int(v[5]), "adopted": int(v[6]),
                "dropped": int(v[7])}

    def search_trials(self):
        """Trial log of the most recent step (include/membrane_hip.h, ms_search_trials):
        -> {alpha, energy, rhs (float arrays), launch, slot (int arrays), behind, guard (bool arrays), one entry per
        logged trial in ladder order; first_launch_hist: {trials of a round's first launch: rounds since creation}}."""
        lib = L.lib()
        n = ctypes.c_int(0)
        hist = np.zeros(8, dtype=np.int64)
        self._chk(lib.ms_search_trials(self._h, None, 0, ctypes.byref(n), hist.ctypes.data_as(L._I64)),
                  "ms_search_trials")
        rows = np.zeros((max(n.value, 1), L.MS_TRIAL_COLS))
        self._chk(lib.ms_search_trials(self._h, _pd(rows), rows.shape[0], ctypes.byref(n), None), "ms_search_trials")
        rows = rows[: n.value]
        flags = rows[:, 5].astype(np.int64)
        return {"alpha": rows[:, 0].copy(), "energy": rows[:, 1].copy(), "rhs": rows[:, 2].copy(),
                "launch": rows[:, 3].astype(np.int64), "slot": rows[:, 4].astype(np.int64),
                "behind": (flags & L.MS_TRIAL_BEHIND) != 0, "guard": (flags & L.MS_TRIAL_GUARD) != 0,
                "first_launch_hist": {k + 1: int(hist[k]) for k in range(8)}}

    def direction_stats(self):
        """Fused direction passes that left D unstored, and directions written out afterwards (ms_direction_stats)."""
        v = np.zeros(2, dtype=np.int64)
        self._chk(L.lib().ms_direction_stats(self._h, v[0:1].ctypes.data_as(L._I64), v[1:2].ctypes.data_as(L._I64)),
                  "ms_direction_stats")
        return {"skipped": int(v[0]), "materialized": int(v[1])}

    def energy_stats(self):
        """Energy launches that ran the lean instance and the general one (include/membrane_hip.h, ms_energy_stats)."""
        v = np.zeros(2, dtype=np.int64)
        self._chk(L.lib().ms_energy_stats(self._h, v[0:1].ctypes.data_as(L._I64), v[1:2].ctypes.data_as(L._I64)),
                  "ms_energy_stats")
        return {"lean": int(v[0]), "general": int(v[1])}

    def exec_stats(self):
        """One-workgroup interpreter of one-tile meshes (include/membrane_hip.h, ms_exec_stats)."""
        v = np.zeros(4, dtype=np.int64)
        self._chk(L.lib().ms_exec_stats(self._h, v.ctypes.data_as(L._I64)), "ms_exec_stats")
        return {"active": bool(v[0]), "packs": int(v[1]), "launches_recorded": int(v[2]), "wanted": bool(v[3] & 1),
                "relax_programs": int((v[3] >> 8) & 0xffffff), "relax_fused": int(v[3] >> 32)}

    def set_pins(self, tables):
        """Upload pin tables (modules/constraints/pins.DeviceTables; None clears them)."""
        if tables is None:
            self._chk(L.lib().ms_set_pins(self._h, 0, None, 0, None, None, None, None, None, 0, 0, None, None, None,
                                          0, None, None, None), "ms_set_pins")
            return

        prm = np.ascontiguousarray(np.asarray(tables.params, dtype=np.float64).reshape(-1, 7))
        arrs, p = zip(*[_i32_table(v) for v in (
            tables.stage_kind, tables.stage_param, tables.stage_off, tables.item_row, tables.item_arg, tables.grad_row,
            tables.grad_kind, tables.grad_param, tables.avg_param, tables.avg_off, tables.avg_row)])
        lane = L.MS_PIN_LANE_PROJECT if tables.lane == "project" else L.MS_PIN_LANE_SKIP
        self._chk(L.lib().ms_set_pins(self._h, prm.shape[0], prm.ctypes.data_as(L._D), len(tables.stage_kind),
                                      p[0], p[1], p[2], p[3], p[4], lane, len(tables.grad_row), p[5], p[6], p[7],
                                      len(tables.avg_param), p[8], p[9], p[10]), "ms_set_pins")
        self._pin_arrays = (prm, arrs)

    def enforce_pins(self):
        """pin_to_plane / pin_to_circle enforce_constraint on the device positions (ms_enforce_pins)."""
        self._chk(L.lib().ms_enforce_pins(self._h), "ms_enforce_pins")

    def pin_stats(self):
        v = np.zeros(4, dtype=np.int64)
        self._chk(L.lib().ms_pin_stats(self._h, v.ctypes.data_as(L._I64)), "ms_pin_stats")
        return {"lane": int(v[0]), "enforce_launches": int(v[1]), "grad_launches": int(v[2]), "trials": int(v[3])}

    def set_fixed_plane(self, normal=None, point=None):
        """fixed_plane's plane {normal (the library normalises it), point}; no normal clears it (ms_set_fixed_plane)."""
        if normal is None:
            self._chk(L.lib().ms_set_fixed_plane(self._h, None, None), "ms_set_fixed_plane")
            self._fixed_plane = None
            return
        n = np.ascontiguousarray(np.asarray(normal, dtype=np.float64).reshape(3))
        q = np.ascontiguousarray(np.zeros(3) if point is None else np.asarray(point, dtype=np.float64).reshape(3))
        self._chk(L.lib().ms_set_fixed_plane(self._h, _pd(n), _pd(q)), "ms_set_fixed_plane")
        self._fixed_plane = (tuple(n.tolist()), tuple(q.tolist()))

    @property
    def fixed_plane(self):
        """(normal, point) as handed to set_fixed_plane, or None."""
        return self.__dict__.get("_fixed_plane")

    def enforce_fixed_plane(self):
        """fixed_plane.enforce_constraint on the device positions (ms_enforce_fixed_plane)."""
        self._chk(L.lib().ms_enforce_fixed_plane(self._h), "ms_enforce_fixed_plane")

    def set_perimeter(self, loop_off=None, tail=None, head=None, target=None):
        """perimeter's loops: entries loop_off[l] .. loop_off[l + 1) of tail / head (external rows, list order) and the
        target length of each; nothing clears them (ms_set_perimeter).  The same tables are not uploaded twice."""
        if loop_off is None or len(loop_off) <= 1:
            if self.__dict__.get("_perimeter_key") is not None:
                self._chk(L.lib().ms_set_perimeter(self._h, 0, None, None, None, None), "ms_set_perimeter")
            self._perimeter_key = None
            return
        (lo, p_lo), (t, p_t), (h, p_h) = _i32_table(loop_off), _i32_table(tail), _i32_table(head)
        tg = np.ascontiguousarray(np.asarray(target, dtype=np.float64).reshape(-1))
        if len(tg) != len(lo) - 1 or len(t) != len(h) or (len(lo) and int(lo[-1]) != len(t)):
            raise L.MembraneHipError("set_perimeter: loop_off, tail / head and target do not fit together")
        key = (lo.tobytes(), t.tobytes(), h.tobytes(), tg.tobytes())
        if key == self.__dict__.get("_perimeter_key"):
            return
        self._perimeter_key = None
        self._chk(L.lib().ms_set_perimeter(self._h, len(lo) - 1, p_lo, p_t, p_h, _pd(tg)), "ms_set_perimeter")
        self._perimeter_key = key

    @property
    def perimeter_key(self):
        """What identifies the tables set_perimeter uploaded last (None: none)."""
        return self.__dict__.get("_perimeter_key")

    @property
    def perimeter_loops(self) -> int:
        """Loops set by set_perimeter (0: none)."""
        key = self.__dict__.get("_perimeter_key")
        return 0 if key is None else len(key[3]) // 8

    def project_perimeter(self, tol: float = 1e-10, max_iter: int = 3, fetch: bool = True):
        """perimeter.enforce_constraint on the device positions, one launch (ms_project_perimeter) -> (passes per loop that
        moved something, P per loop at its last evaluation); ``fetch=False``: nothing comes back, no synchronise."""
        if not fetch:
            self._chk(L.lib().ms_project_perimeter(self._h, float(tol), int(max_iter), None, None), "ms_project_perimeter")
            return None, None
        n = max(1, self.perimeter_loops)
        passes = np.zeros(n, dtype=np.int32)
        per = np.zeros(n)
        self._chk(L.lib().ms_project_perimeter(self._h, float(tol), int(max_iter), passes.ctypes.data_as(L._I32), _pd(per)),
                  "ms_project_perimeter")
        return passes[: self.perimeter_loops], per[: self.perimeter_loops]

    def enforce_only_stats(self) -> dict:
        """Launch counts of fixed_plane's and perimeter's kernels (ms_enforce_only_stats)."""
        v = np.zeros(4, dtype=np.int64)
        self._chk(L.lib().ms_enforce_only_stats(self._h, v.ctypes.data_as(L._I64)), "ms_enforce_only_stats")
        return {"fixed_plane_launches": int(v[0]), "perimeter_launches": int(v[1]), "trials": int(v[2]), "loops": int(v[3])}

    def padded_positions(self) -> np.ndarray:
        """The padding rows nv .. nvp of the position buffer (ms_get_padded_rows): no kernel may move them."""
        n = ctypes.c_int64(0)
        self._chk(L.lib().ms_get_padded_rows(self._h, ctypes.byref(n), None), "ms_get_padded_rows")
        out = np.zeros((max(int(n.value), 0), 3))
        if len(out):
            self._chk(L.lib().ms_get_padded_rows(self._h, ctypes.byref(n), _pd(out)), "ms_get_padded_rows")
        return out

    def resident_stats(self):
        """The resident step kernel (include/membrane_hip.h, ms_resident_stats)."""
        v = np.zeros(4, dtype=np.int64)
        self._chk(L.lib().ms_resident_stats(self._h, v.ctypes.data_as(L._I64)), "ms_resident_stats")
        return {"co_resident": int(v[0]), "launches": int(v[1]), "steps": int(v[2]), "declined": int(v[3])}

    def tsearch_stats(self):
        """Search passes of the tilt relaxations (include/membrane_hip.h, ms_tsearch_stats)."""
        v = np.zeros(2, dtype=np.int64)
        self._chk(L.lib().ms_tsearch_stats(self._h, v.ctypes.data_as(L._I64)), "ms_tsearch_stats")
        return {"passes": int(v[0]), "step_sizes": int(v[1])}

    @staticmethod
    def _tilt_lanes(v) -> dict:
        fits = lambda k: {"search": bool(v[k]), "gradient": bool(v[k + 1]), "energy_only": bool(v[k + 2])}  # noqa: E731
        return {"cap": int(v[0]), "max_ent": int(v[1]), 1: fits(2), 2: fits(5), "leaflet_gradient_lds": int(v[8]),
                "leaflet_gradient_fits": bool(v[9]), "threads": int(v[10]), "own": int(v[11])}

    def tilt_lane_stats(self) -> dict:
        """Which lane the tilt family takes on this context (include/membrane_hip.h, ms_tilt_lane_stats): the patch size
        ``cap``, per number of fields (keys 1 and 2) whether the search, gradient and energy-only passes fit, and the
        leaflet bending_tilt gradient instance's LDS bytes in the current summation mode."""
        v = np.zeros(12, dtype=np.int64)
        self._chk(L.lib().ms_tilt_lane_stats(self._h, v.ctypes.data_as(L._I64)), "ms_tilt_lane_stats")
        return self._tilt_lanes(v)

    @classmethod
    def plan_tilt_lanes(cls, positions, tri_rows, tile_vertices: int = 0, fixed_order: bool = False) -> dict:
        """The same for a mesh, on the host (ms_plan_tilt_lanes: no GPU needed)."""
        pos = _f64(positions, name="positions")
        tri = np.ascontiguousarray(tri_rows, dtype=np.int32)
        v = np.zeros(12, dtype=np.int64)
        L.check(L.lib().ms_plan_tilt_lanes(len(pos), len(tri), _pd(pos), tri.ctypes.data_as(L._I32), int(tile_vertices),
                                           1 if fixed_order else 0, v.ctypes.data_as(L._I64)), None, "ms_plan_tilt_lanes")
        return cls._tilt_lanes(v)

    @classmethod
    def tilt_lane_plan(cls, threads: int, cap: int, max_ent: int, fixed_order: bool = False) -> dict:
        """... and for a patch of ``cap`` rows outright (ms_tilt_lane_plan): where the thresholds lie."""
        v = np.zeros(12, dtype=np.int64)
        L.check(L.lib().ms_tilt_lane_plan(int(threads), int(cap), int(max_ent), 1 if fixed_order else 0,
                                          v.ctypes.data_as(L._I64)), None, "ms_tilt_lane_plan")
        return cls._tilt_lanes(v)

    EXEC_KINDS = {1: "energy", 2: "gradient", 3: "tilt", 4: "bt", 5: "tsmooth", 6: "tvec", 7: "disk_target", 8: "reduce",
                  9: "direction", 10: "row_dot", 11: "axpy_masked", 12: "memset", 13: "relax", 14: "relax_fused", 15: "tsearch"}

    def exec_trace(self, on: bool = True):
        """Per-record durations of the one-workgroup interpreter since the last call (ms_exec_trace):
        -> list of {kind, mode, inst, count, total_us, avg_us}."""
        rows = np.zeros((256, 4), dtype=np.float64)
        n = ctypes.c_int(0)
        self._chk(L.lib().ms_exec_trace(self._h, 1 if on else 0, _pd(rows), 256, ctypes.byref(n)), "ms_exec_trace")
        out = []
        for k in range(n.value):
            kind, mi, cnt, tot = int(rows[k, 0]), int(rows[k, 1]), int(rows[k, 2]), float(rows[k, 3])
            out.append({"kind": self.EXEC_KINDS.get(kind, str(kind)), "mode": mi & 0xffff, "inst": mi >> 16, "count": cnt,
                        "total_us": tot, "avg_us": tot / max(cnt, 1)})
        return out

    def shard_info(self):
        v = [ctypes.c_int64(0) for _ in range(4)]
        self._chk(L.lib().ms_shard_info(self._h, *[ctypes.byref(x) for x in v]), "ms_shard_info")
        return {"nvp": v[0].value, "row0": v[1].value, "row1": v[2].value, "rows_per_shard": v[3].value}

    def tile_stats(self):
        v = [ctypes.c_int64(0) for _ in range(5)]
        self._chk(L.lib().ms_tile_stats(self._h, *[ctypes.byref(x) for x in v]), "ms_tile_stats")
        lo = np.zeros(2, dtype=np.int64)
        self._chk(L.lib().ms_lane_order_stats(self._h, lo.ctypes.data_as(L._I64)), "ms_lane_order_stats")
        return {"n_tiles": v[0].value, "facet_instances": v[1].value, "max_halo": v[2].value,
                "lds_bytes_energy": v[3].value, "lds_bytes_gradient": v[4].value,
                "lane_order": bool(lo[0]), "lane_halo": bool(lo[1])}
