"""Device-resident Minimizer with the reference's entry points.

Mirrors ``runtime/minimizer.py`` of the reference for the hot-path scope:
``Minimizer(mesh, global_params, stepper, energy_manager, constraint_manager,
energy_modules=None, constraint_modules=None, step_size=1e-3, tol=1e-6,
quiet=False)`` with ``minimize(n_steps, callback=None) -> dict``,
``compute_energy()``, ``compute_energy_and_gradient_array()``,
``compute_energy_breakdown()``, ``refresh_modules()``, ``reset_soa_caches()``
and the attributes ``step_size``, ``stepper``, ``mesh``.

One iteration (minimizer.py:1230-1515) =
  energy + gradient over all modules            (:1314, evaluation_manager.py:134-151)
  volume-constraint KKT projection, fixed rows  (:982-990, constraint_manager.py:293-301)
  convergence test |g| < tol                    (:1324)
  stepper.step: direction + Armijo line search  (:1374, line_search.py:267-426)
  zero-step / reset bookkeeping                 (:1439-1464)
  Lagrange volume-drift check -> projection     (:1478-1513)
All array work runs in libmembrane_hip.so with positions, gradient, direction,
CG history and trial positions resident in HBM; the host sees a handful of
scalars per step.  ``Vertex.position`` objects / the mesh position array are
written back once at the end (or before each ``callback``).

On the device as well: the tilt relaxation at the top of every iteration
(``tilt_solve_mode`` nested / coupled, single field and two leaflets:
ms_relax_tilts / ms_relax_leaflet_tilts, minimizer.py:1237-1307), the tilt
modules (``tilt``, ``bending_tilt``, ``tilt_smoothness`` and their ``_in`` /
``_out`` leaflet forms, ``tilt_disk_target_in/out``), ``rim_slope_match_out`` with a
non-zero strength (k_rsm_geom / k_rsm_apply), and ``gaussian_curvature`` and the
switched-off ``rim_slope_match_out`` as host-side constants.

Constraints: ``volume``, the hard area constraints ``body_area`` (its row in the KKT projection next to the volume row,
its projection on every line-search trial and in every enforce context) and ``global_area`` (the projection alone), and
the pins (``pin_to_plane`` / ``pin_to_circle``: the pin program on every
line-search trial and in every enforce context, their rows removed from the gradient in the project lane).  Next to
the tilt modules, single field or leaflets, a trial is: positions, pin program, the stored tilts projected onto the
pinned surface, energy there; a rejected trial puts the tilts back with the positions.  The enforce-only constraints
``fixed_plane`` (every movable vertex onto a plane; next to the tilt modules it takes the pins' lane) and ``perimeter``
(listed edge loops held at a target length) have no row: they run on every trial and in every enforce context, in the
device's one order fixed_plane -> pins -> perimeter -> volume -> area.

Out of scope here (raises MembraneHipError): every other energy module,
constraints other than ``volume``, ``body_area``, ``global_area``, ``pin_to_plane``, ``pin_to_circle``,
``tilt_thetaB_boundary_in``, ``fixed_plane`` and ``perimeter``, a listed order of the enforcers other than the device's,
``perimeter`` next to tilt modules, ``volume``, ``global_area`` or a ``body_area`` whose facets its loops touch,
``fixed_plane`` next to ``volume`` or the area constraints, the area constraints next to tilt modules, pins or ``body_area_penalty``, pins next to tilt modules together with the
``volume`` constraint, the benchmark toggles of the leaflet modules
(modules/energy/leaflet_common._UNSUPPORTED_KEYS), the reference's auto
mesh-quality repair hook.
"""

from __future__ import annotations

import logging
from typing import Callable, Dict, List, NamedTuple, Optional, Tuple

import numpy as np

from .. import _lib as L
from ..core.parameters import ParameterResolver
from .steppers.base import BaseStepper
from ..geometry.mesh import _body_facet_mask, mirror_for
from ..modules.energy import leaflet_common as _lc
from ..modules.energy._common import bending_gradient_mode, bending_model
from ..modules.constraints import pins as _pins
from ..modules.constraints import tilt_thetaB_boundary_in as _tbb
from ..modules.constraints import body_area as _body_area
from ..modules.constraints import global_area as _global_area
from ..modules.constraints import fixed_plane as _fplane
from ..modules.constraints import perimeter as _perimeter
from ..modules.energy.body_area_penalty import body_area_params
from ..modules.energy import edge_length_penalty as _edgepen
from ..modules.energy import line_tension as _line
from ..modules.energy.volume import body_penalty_params
from .steppers.base import write_back_positions

logger = logging.getLogger("membrane_solver")

_RIM_MATCH = "rim_slope_match_out"
_EDGE_MODULES = ("line_tension", "edge_length_penalty")  # they share the lane behind the energy and the gradient pass


class _Module(NamedTuple):
    """What the Minimizer knows of one energy module.  A new module adds its record here, the refusals that are its own
    in Minimizer._check() and, where it has a table on the device, one keyed upload in Minimizer._apply()."""

    bit: int                            # its bit of the module mask (0: a host-side constant, no kernel)
    slot: Optional[int]                 # its entry of energies[]; None: it reports its own energy, or a host constant
    scalar: Optional[int] = None        # its scalar slot, where it shares energies[3] / energies[1] with others
    field: Optional[str] = None         # the tilt field(s) it reads and relaxes: "single", or the leaflets "in" / "out" / "both"
    edges: bool = False                 # it selects edges: refused on a mesh without an edge table
    # resolve(...) -> its parameters; falsy: switched off; absent: always on.  Called by ``reads``: "params" (param_resolver,
    # global_params, *args) or "mesh" (mesh, the same), leaflet_common's forms; else (minimizer, mirror, device or None)
    resolve: Optional[Callable] = None
    reads: str = ""
    args: tuple = ()
    # a ride-along module: its sums ride in the scalar slots of ``hosts``, it reports its own energy and each host
    # reports its slot without it.  (device) -> that energy; a tuple where the hosts' parts differ: (own, part per host)
    energy: Optional[Callable] = None
    hosts: Tuple[str, ...] = ()


def _gp_nonzero(key):
    return lambda mz, mir, dm: float(mz.global_params.get(key, 0.0) or 0.0) != 0.0


def _gaussian_constant(mz, mir, dm):
    from ..modules.energy import gaussian_curvature as _gc

    mz._const_energy["gaussian_curvature"] = _gc.constant_energy(mz.mesh, mz.global_params)  # gaussian_curvature.py:117-134


def _rim_match_gate(mz, mir, dm):
    """rim_slope_match_out.py:380-382: strength 0 is 0.0 whatever else is set.  With a strength the module is on for now:
    _check() resolves its tables once the other modules' bits are known; no group or ring puts it back to this constant."""
    mz._const_energy[_RIM_MATCH] = 0.0
    return _lc.rim_match_strength(mz.param_resolver, mz.global_params) != 0.0


# The order counts: the refusal of an unknown module lists the names in it, and the ride-along energies are taken out of
# their hosts in it (floating-point sums).
_MODULES = {
    "surface": _Module(L.MS_MOD_SURFACE, 0),
    "bending": _Module(L.MS_MOD_BENDING, 1, L.MS_S_EBEND),
    "volume": _Module(L.MS_MOD_VOLUME_PENALTY, 2,
                      resolve=lambda mz, mir, dm: (mz.global_params.get("volume_constraint_mode", "lagrange") == "penalty"
                                               and bool(getattr(mz.mesh, "bodies", None)))),
    "tilt": _Module(L.MS_MOD_TILT, 3, L.MS_S_ETILT, "single", resolve=_gp_nonzero("tilt_rigidity")),  # tilt.py:110-112
    "bending_tilt": _Module(L.MS_MOD_BENDING_TILT, 1, L.MS_S_EBT, "single"),
    "tilt_smoothness": _Module(L.MS_MOD_TILT_SMOOTH, 3, L.MS_S_ETS, "single",
                               resolve=_gp_nonzero("tilt_smoothness_rigidity")),  # tilt_smoothness.py:258-260
    # tilt_leaflet.py:41-43, tilt_smoothness_leaflet.py:32-34: a zero modulus switches the module off
    "tilt_in": _Module(L.MS_MOD_TILT_IN, 3, L.MS_S_ETILT_IN, "in", False, _lc.tilt_modulus, "params", ("in",)),
    "tilt_out": _Module(L.MS_MOD_TILT_OUT, 3, L.MS_S_ETILT_OUT, "out", False, _lc.tilt_modulus, "params", ("out",)),
    "tilt_smoothness_in": _Module(L.MS_MOD_TILT_SMOOTH_IN, 3, L.MS_S_ETS_IN, "in", False, _lc.smoothness_rigidity, "params", ("in",)),
    "tilt_smoothness_out": _Module(L.MS_MOD_TILT_SMOOTH_OUT, 3, L.MS_S_ETS_OUT, "out", False, _lc.smoothness_rigidity, "params", ("out",)),
    "bending_tilt_in": _Module(L.MS_MOD_BENDING_TILT_IN, 1, L.MS_S_EBT_IN, "in"),
    "bending_tilt_out": _Module(L.MS_MOD_BENDING_TILT_OUT, 1, L.MS_S_EBT_OUT, "out"),
    # tilt_disk_target_in.py:175-191: no group, no row, k or theta_B zero
    "tilt_disk_target_in": _Module(L.MS_MOD_TILT_DISK_TARGET_IN, 3, L.MS_S_EDT_IN, "in", False, _lc.disk_target_params, "mesh", ("in",)),
    "tilt_disk_target_out": _Module(L.MS_MOD_TILT_DISK_TARGET_OUT, 3, L.MS_S_EDT_OUT, "out", False, _lc.disk_target_params, "mesh", ("out",)),
    "body_area_penalty": _Module(L.MS_MOD_AREA_PENALTY, 2,  # body_area_penalty.py:114-123
                                 resolve=lambda mz, mir, dm: body_area_params(mz.mesh, mz.global_params, mz.param_resolver)),
    # the edge modules resolve on the device, which _device() synchronises first for them: their tables go up and say
    # whether any edge is charged (k != 0)
    "line_tension": _Module(L.MS_MOD_LINE_TENSION, 0, edges=True,
                            resolve=lambda mz, mir, dm: mz._upload_line(mir, dm)),
    "edge_length_penalty": _Module(L.MS_MOD_EDGE_LENGTH_PENALTY, 0, edges=True,
                                   resolve=lambda mz, mir, dm: mz._upload_edge_penalty(mir, dm)),
    # tilt_rim_source_in.py:386-404: no group, no rim edge, every gamma 0; in the leaflet's tilt-magnitude slot
    "tilt_rim_source_in": _Module(L.MS_MOD_TILT_RIM_SOURCE_IN, None, None, "in", True, _lc.rim_source_params, "mesh", ("in",),
                                  lambda dm: dm.leaflet_rim_source_energy("in"), ("tilt_in",)),
    "tilt_rim_source_out": _Module(L.MS_MOD_TILT_RIM_SOURCE_OUT, None, None, "out", True, _lc.rim_source_params, "mesh", ("out",),
                                   lambda dm: dm.leaflet_rim_source_energy("out"), ("tilt_out",)),
    # tilt_coupling.py:129-132: unknown or absent mode, or k_c == 0; in the outer leaflet's tilt-magnitude slot
    "tilt_coupling": _Module(L.MS_MOD_TILT_COUPLING, None, None, "both", False, _lc.coupling_params, "params", (),
                             lambda dm: dm.tilt_coupling_energy(), ("tilt_out",)),
    # tilt_splay_twist_in.py:134-135: both moduli 0; in the inner leaflet's smoothness slot
    "tilt_splay_twist_in": _Module(L.MS_MOD_TILT_SPLAY_TWIST_IN, None, None, "in", False,
                                   lambda mz, mir, dm: _lc.splay_twist_device_params(mz.param_resolver, mz.global_params, mz.mesh),
                                   "", (), lambda dm: dm.tilt_splay_twist_energy(), ("tilt_smoothness_in",)),
    # tilt_rim_source_bilayer.py:431-462: one table for both leaflet fields; in the outer leaflet's tilt-magnitude slot
    "tilt_rim_source_bilayer": _Module(L.MS_MOD_TILT_RIM_SOURCE_BILAYER, None, None, "both", True,
                                       _lc.rim_source_params, "mesh", (None,),
                                       lambda dm: dm.rim_source_bilayer_energy(), ("tilt_out",)),
    # tilt_thetaB_contact_in.py:351-374: no group, no tagged row, k == gamma == 0; in the inner leaflet's tilt-magnitude slot
    "tilt_thetaB_contact_in": _Module(L.MS_MOD_TILT_THETAB_CONTACT_IN, None, None, "in", False, _lc.thetab_contact_params,
                                      "mesh", (), lambda dm: dm.thetab_contact_energy(), ("tilt_in",)),
    # (no field of its own: the module is admitted only next to leaflet modules that relax the fields it couples; one part
    # in each leaflet's tilt-magnitude slot)
    _RIM_MATCH: _Module(L.MS_MOD_RIM_SLOPE_MATCH_OUT, None, resolve=_rim_match_gate,
                        energy=lambda dm: dm.rim_match_energies(), hosts=("tilt_out", "tilt_in")),
    # host-side constant, no kernel: a topological constant on closed surfaces
    "gaussian_curvature": _Module(0, None, resolve=_gaussian_constant),
}
__doc__ += "\nEnergy modules on the device path: " + ", ".join(_MODULES) + ".\n"


def _bits(*fields):
    return sum(m.bit for m in _MODULES.values() if m.field in fields)  # (distinct bits: the sum is their union)


_WALK = {n: (m.bit, m.resolve, m.reads, m.args) for n, m in _MODULES.items()}  # what Minimizer._resolve() reads, unpacked
_ENERGY_BITS = {n: m.bit for n, m in _MODULES.items()}
_ENERGY_SLOT = {n: m.slot for n, m in _MODULES.items()}
_TILT_SCALAR = {n: m.scalar for n, m in _MODULES.items() if m.slot == 3}  # scalar slot of every module that shares energies[3]
_BEND_SCALAR = {n: m.scalar for n, m in _MODULES.items() if m.slot == 1}
_SINGLE_TILT_BITS = _bits("single")
_LEAFLET_BITS = _bits("in", "out", "both")
_TILT_BITS = _SINGLE_TILT_BITS | _LEAFLET_BITS
_INNER_LEAFLET_BITS = _bits("in", "both")  # every module that reads the inner leaflet's field (a relaxation with one relaxes it)
_OUTER_RELAX_BITS = _bits("out", "both")   # the modules whose tilt gradient relaxes the outer leaflet's field
_LEAFLET_BT_BITS = L.MS_MOD_BENDING_TILT_IN | L.MS_MOD_BENDING_TILT_OUT
_BEND_BITS = L.MS_MOD_BENDING | L.MS_MOD_BENDING_TILT
_PIN_MODULES = ("pin_to_plane", "pin_to_circle")
_AREA_CONSTRAINTS = ("body_area", "global_area")  # the area lane: the row (body_area) and the enforcer on every trial
# The reference's fixed_plane and perimeter write vertex.position without Mesh.increment_version(), and volume.py:109 /
# body_area.py:98 / global_area take their first evaluation from Mesh.positions_view(), a copy keyed on that version: right
# behind an enforce-only module their first pass is evaluated at the positions from BEFORE it and applied to the moved
# ones.  The device evaluates where it applies; the reference's trajectories of these pairs differ from it by 1e-5 .. 1e-1
# in the accepted energies, so the pairs are refused until that first pass is reproduced.
_STALE_CACHE = ("the reference evaluates that module's first pass at the positions cached before the enforce-only module "
                "moved them (Mesh.positions_view is not invalidated), which the device path does not reproduce")
_ENFORCE_ONLY = (_fplane.NAME, _perimeter.NAME)  # no KKT row: they only move the positions of a trial / an enforce context


def _keyed_upload(keys, slot, key, dm, setter, args=(), kwargs=None):
    """Call the device's ``setter`` unless the table under ``slot`` of the mirror's ``keys`` went up with the same key."""
    if keys.get(slot) != key:
        getattr(dm, setter)(*args, **(kwargs or {}))
        keys[slot] = key


class GradientRows:
    """Lazy stand-in for the reference's ``{vertex_id: grad_row}`` dict of non-zero rows
    (minimizer.py:1067-1073); materialised on first dict-style access."""

    def __init__(self, mesh, grad_arr):
        """grad_arr: the (nv,3) array, or a zero-argument callable that downloads it on first use
        (minimize(sync_mesh=False) keeps the 24 B/vertex D2H copy out of the loop that way; read
        it before stepping again: it fetches the gradient then resident on the device)."""
        self._array = None if callable(grad_arr) else grad_arr
        self._fetch = grad_arr if callable(grad_arr) else None
        self._mesh = mesh
        self._dict = None

    @property
    def array(self) -> np.ndarray:
        if self._array is None:
            self._array = self._fetch()
            self._fetch = None
        return self._array

    def _materialise(self):
        if self._dict is None:
            nz = np.flatnonzero(np.any(self.array != 0.0, axis=1))
            ids = self._mesh.vertex_ids
            self._dict = {int(ids[r]): self.array[r].copy() for r in nz}
        return self._dict

    def __getitem__(self, k):
        return self._materialise()[k]

    def __iter__(self):
        return iter(self._materialise())

    def __len__(self):
        return len(self._materialise())

    def items(self):
        return self._materialise().items()

    def keys(self):
        return self._materialise().keys()

    def values(self):
        return self._materialise().values()

    def __contains__(self, k):
        return k in self._materialise()


class Minimizer:
    """Coordinate the optimisation loop for a mesh, on the GPU."""

    def __init__(self, mesh, global_params, stepper, energy_manager, constraint_manager,
                 energy_modules: Optional[List[str]] = None,
                 constraint_modules: Optional[List[str]] = None, step_size: float = 1e-3,
                 tol: float = 1e-6, quiet: bool = False, *, device: int = 0, tile_vertices: int = 0,
                 deterministic: Optional[bool] = None):
        self.mesh = mesh
        self.global_params = global_params
        self.energy_manager = energy_manager
        self.constraint_manager = constraint_manager
        self.stepper = stepper
        self.step_size = step_size
        self.tol = tol
        self.quiet = quiet
        self.device = device
        self.tile_vertices = tile_vertices
        # None: library default (LDS-atomic vertex sums unless MS_DETERMINISTIC=1); True: fixed-order
        # sums, bitwise reproducible run to run (ms_set_deterministic)
        self.deterministic = deterministic
        self.max_zero_steps = int(global_params.get("max_zero_steps", 10))
        self.step_size_floor = float(global_params.get("step_size_floor", 1e-8))
        self.param_resolver = ParameterResolver(global_params)
        module_list = energy_modules if energy_modules is not None else mesh.energy_modules
        self.energy_module_names = list(module_list)
        constraint_list = constraint_modules if constraint_modules is not None else mesh.constraint_modules
        self.constraint_module_names = list(constraint_list)
        self.refresh_modules()

    # -- module wiring (minimizer.py:100-118, :235-243) -----------------------
    def refresh_modules(self):
        self.energy_modules = [self.energy_manager.get_module(m) for m in self.energy_module_names]
        for name, mod in zip(self.energy_module_names, self.energy_modules):
            if not hasattr(mod, "compute_energy_and_gradient_array"):
                raise TypeError(f"energy module {name!r} lacks compute_energy_and_gradient_array")
            # an edge module on a mesh built without edges stays refused: nothing could be tagged or given a target,
            # and the deck would run with that module's energy at zero
            # (the rim sources select edges as well: without an edge table nothing could be a rim edge)
            no_edges = name in _MODULES and _MODULES[name].edges and not _line.has_edge_table(self.mesh)
            if name not in _MODULES or no_edges:
                where = " on a mesh without an edge table (ArrayMesh(edges=, edge_options=))" if no_edges else ""
                raise L.MembraneHipError(f"energy module {name!r}{where} is outside the HIP hot path "
                                         f"({', '.join(_MODULES)})")
        if "body_area_penalty" in self.energy_module_names and any(
                _ENERGY_BITS[n] & _TILT_BITS for n in self.energy_module_names):  # (not rim_slope_match_out: see its record)
            raise L.MembraneHipError("body_area_penalty together with tilt modules is outside the HIP hot path")
        for edge_mod in _EDGE_MODULES:
            if edge_mod in self.energy_module_names and any(
                    _ENERGY_BITS[n] & _TILT_BITS for n in self.energy_module_names):
                raise L.MembraneHipError(f"{edge_mod} together with tilt modules is outside the HIP hot path")
        listed = list(dict.fromkeys(self.energy_module_names))
        self._edge_listed = any(n in _EDGE_MODULES for n in listed)  # (_device() then synchronises before it resolves)
        self._disk_order, self._rim_order = ([n[len(pre):] for n in listed if n in (pre + "in", pre + "out")]
                                             for pre in ("tilt_disk_target_", "tilt_rim_source_"))
        self._line_key = None
        self._absent_key = None
        _lc.clear_absent_cache(self.mesh)
        self._edgepen_key = None
        self.constraint_modules = [self.constraint_manager.get_constraint(c)
                                   for c in self.constraint_module_names]
        for name in self.constraint_module_names:
            if name not in ("volume", _tbb.NAME) + _PIN_MODULES + _AREA_CONSTRAINTS + _ENFORCE_ONLY:
                raise L.MembraneHipError(f"constraint module {name!r} is outside the HIP hot path "
                                         "(volume, body_area, global_area, pin_to_plane, pin_to_circle, "
                                         "tilt_thetaB_boundary_in, fixed_plane, perimeter)")
        self._pin_names = [n for n in self.constraint_module_names if n in _PIN_MODULES]
        if self._pin_names and "volume" in self.constraint_module_names and \
                self.constraint_module_names.index("volume") < self.constraint_module_names.index(self._pin_names[0]):
            # enforce_all runs the modules in their listed order; the device runs the pins first
            raise L.MembraneHipError("constraint_modules lists volume before pin_to_plane / pin_to_circle: the HIP "
                                     "path enforces the pins first; list the pin modules before volume")
        self._check_area_constraints()
        self._check_enforce_only()
        self._fplane_active = False  # (set by _device(): fixed_plane is listed and its normal is not zero)
        self._perim_active = False   # (set by _device(): perimeter is listed and some entry has edges and a target)
        self._perim_key = None
        self._area_con = None  # (set by _device(): (kind, target) of the area constraint that is listed and has a target)
        self._pin_key = None
        self._pins_active = False
        self._tbb_active = False  # (set by _device(): tilt_thetaB_boundary_in is listed and has a ring)
        # (tilt_thetaB_boundary_in has no enforce_constraint: alone it switches no enforcer on, minimizer.py:1103-1106)
        self._has_enforceable_constraints = any(hasattr(m, "enforce_constraint")
                                                for m in self.constraint_modules)
        self._configured_key = None
        self._device_ahead = False

    def _check_area_constraints(self):
        """What the area lane does not take, by the names alone (the targets are checked by _device()): the lane enforces
        pins -> volume -> area and has no fixture next to the tilt families, the pins or the soft penalty."""
        names = self.constraint_module_names
        area = [n for n in names if n in _AREA_CONSTRAINTS]
        if not area:
            return
        if len(area) > 1:
            raise L.MembraneHipError("body_area and global_area together are outside the HIP hot path: the device "
                                     "holds one area constraint")
        what = area[0]
        if "volume" in names and names.index("volume") > names.index(what):
            raise L.MembraneHipError(f"constraint_modules lists volume after {what}: the HIP path enforces the volume "
                                     f"first; list volume before {what}")
        if len(getattr(self.mesh, "bodies", None) or {}) > 1:
            raise L.MembraneHipError(f"{what} on a mesh with more than one body is outside the HIP hot path "
                                     "(one body per mesh, SURVEY 8a row a7)")
        if any(_ENERGY_BITS[n] & _TILT_BITS for n in self.energy_module_names) or _tbb.NAME in names:
            raise L.MembraneHipError(f"{what} together with tilt modules is outside the HIP hot path")
        if "body_area_penalty" in self.energy_module_names:
            raise L.MembraneHipError(f"{what} together with body_area_penalty is outside the HIP hot path: hold the area "
                                     "with the constraint or with the penalty")
        if self._pin_names:
            raise L.MembraneHipError(f"{what} next to pin_to_plane / pin_to_circle is outside the HIP hot path")

    def _check_enforce_only(self):
        """What the lane of fixed_plane / perimeter does not take, by the names alone.  The device enforces in ONE order,
        fixed_plane -> pin program -> perimeter -> volume -> area: enforce_all's listed order for the lists the
        reference's decks and parser produce (explicitly listed modules first, body_area / volume appended from the
        bodies last); a list whose relative order differs is refused."""
        names = self.constraint_module_names
        enforcers = [n for n in names if n in ("volume",) + _PIN_MODULES + _AREA_CONSTRAINTS + _ENFORCE_ONLY]
        tilt = any(_ENERGY_BITS[n] & _TILT_BITS for n in self.energy_module_names)
        if _fplane.NAME in names:
            if enforcers[0] != _fplane.NAME:
                raise L.MembraneHipError(f"constraint_modules lists fixed_plane after {enforcers[0]}: the HIP path "
                                         "enforces fixed_plane first; list fixed_plane before every other enforcer")
            for other in ("volume",) + _AREA_CONSTRAINTS:
                if other in names:
                    raise L.MembraneHipError(f"fixed_plane next to {other} is outside the HIP hot path: " + _STALE_CACHE)
        if _perimeter.NAME in names:
            at = names.index(_perimeter.NAME)
            later_pins = [n for n in names[at + 1:] if n in _PIN_MODULES]
            if later_pins:
                raise L.MembraneHipError(f"constraint_modules lists perimeter before {later_pins[0]}: the HIP path "
                                         "enforces the pins first; list the pin modules before perimeter")
            earlier = [n for n in names[:at] if n in ("volume",) + _AREA_CONSTRAINTS]
            if earlier:
                raise L.MembraneHipError(f"constraint_modules lists perimeter after {earlier[0]}: the HIP path enforces "
                                         f"perimeter first; list perimeter before {earlier[0]}")
            if tilt or _tbb.NAME in names:
                raise L.MembraneHipError("perimeter together with tilt modules is outside the HIP hot path")
            for other in ("volume", "global_area"):
                if other in names:
                    raise L.MembraneHipError(f"perimeter next to {other} is outside the HIP hot path: " + _STALE_CACHE)
            # (body_area behind perimeter: where the loops touch no vertex of the body's facets, checked at upload)
            if not _line.has_edge_table(self.mesh):
                raise L.MembraneHipError("perimeter is listed but the mesh has no edge table (ArrayMesh(edges=...)): its "
                                         "signed edge indices cannot be resolved")

    def _upload_enforce_only(self, mir, dm):
        """fixed_plane's plane and perimeter's loops on the device, keyed like the pins: resolved once per mesh topology,
        context and parameter values (call refresh_modules() after changing them).  A module that is not listed leaves
        nothing set: a plane or loops that the module's own ``enforce_constraint`` (or another minimizer) left on the
        mesh's context are cleared, so that the lanes that decline with them (the resident kernel) stay open."""
        names = self.constraint_module_names
        gp = self.global_params
        if _fplane.NAME not in names and dm.fixed_plane is not None:
            dm.set_fixed_plane()
        if _perimeter.NAME not in names and dm.perimeter_loops:
            dm.set_perimeter()
        if _fplane.NAME in names:
            pl = _fplane.plane(self.mesh, gp)
            want = None if pl is None else (tuple(pl[0].tolist()), tuple(pl[1].tolist()))
            if want != dm.fixed_plane:
                dm.set_fixed_plane(*(pl if pl is not None else ()))
            self._fplane_active = pl is not None
        if _perimeter.NAME in names:
            cons = gp.get("perimeter_constraints") or []
            key = (mir._topo_key, id(dm), repr([(list(c.get("edges") or []), c.get("target_perimeter")) for c in cons]))
            # (the tables this minimizer uploaded must still be the context's: the module's own entry point may have
            # replaced them in between)
            if self._perim_key is None or self._perim_key[:3] != key or self._perim_key[3] != dm.perimeter_key:
                self._perim_active = bool(_perimeter.upload(self.mesh, gp, dm))
                self._perim_key = key + (dm.perimeter_key,)
                if self._perim_active and "body_area" in names:
                    # body_area.py:98 reads the cached positions: exact only where perimeter moved no vertex of the body
                    tri, _ = self.mesh.triangle_row_cache()
                    mask, body = _body_facet_mask(self.mesh, len(tri))
                    rows = np.asarray(tri)[np.flatnonzero(mask)] if mask is not None else np.asarray(tri)
                    _n, _off, tail, head, _t = _perimeter.loops(self.mesh, gp)
                    if body is not None and np.intersect1d(np.concatenate([tail, head]), rows.reshape(-1)).size:
                        self._perim_key = None  # (refused again on the next call)
                        raise L.MembraneHipError("perimeter next to body_area with a listed edge on the body's facets is "
                                                 "outside the HIP hot path: " + _STALE_CACHE)

    def _area_constraint_params(self):
        """(kind, target, max_iter) of the listed area constraint, or None where it does nothing (no body, no
        ``target_area`` / ``target_surface_area``: body_area.py:40-41, global_area.py:11-15).  A target that is not finite
        and positive is refused by the module's ``target_area``."""
        names = self.constraint_module_names
        if "body_area" in names:
            t = _body_area.target_area(self.mesh)
            return None if t is None else (L.MS_AREA_BODY, t, 20)
        if "global_area" in names:
            t = _global_area.target_area(self.mesh, self.global_params)
            return None if t is None else (L.MS_AREA_GLOBAL, t, 3)
        return None

    def sync_mesh_from_device(self):
        """Write device positions back into the mesh (after minimize(sync_mesh=False))."""
        mir, dm = self._device_nosync()
        write_back_positions(self.mesh, dm, mir)
        self._device_ahead = False

    def _device_nosync(self):
        mir = mirror_for(self.mesh, device=self.device, tile_vertices=self.tile_vertices)
        if mir.dm is None:
            mir.sync()
        return mir, mir.dm

    def reset_soa_caches(self):
        """Forget the device mirror (call after topology surgery, minimizer.py:208)."""
        mir = getattr(self.mesh, "_hip_mirror", None)
        if mir is not None and mir.dm is not None:
            mir.dm.close()
        self.mesh._hip_mirror = None
        self._configured_key = None

    # -- device configuration --------------------------------------------------
    def _device(self):
        """-> (mirror, device) in this minimizer's configuration, in three steps: resolve every listed module's parameters
        and the module mask, run every refusal that needs nothing from the device, then synchronise and upload."""
        mir = mirror_for(self.mesh, device=self.device, tile_vertices=self.tile_vertices)
        area_con = self._area_constraint_params()
        dm = None
        if self._edge_listed:  # an edge module resolves by uploading: synchronise first; else _apply() does, after the checks
            dm = mir.sync()
            if self.deterministic is not None:
                dm.set_deterministic(self.deterministic)
        mods, p = self._resolve(mir, dm)
        return mir, self._apply(mir, dm, p, area_con, self._check(mir, mods, p, area_con))

    def _resolve(self, mir, dm):
        """Walk the listed energy modules through the table -> (module mask, {name: parameters}) of the modules that are
        switched on; the host-side constants go to ``_const_energy``."""
        self._const_energy = {}
        mesh, pr, gp = self.mesh, self.param_resolver, self.global_params
        mods, p = 0, {}
        for name in self.energy_module_names:
            bit, resolve, reads, args = _WALK[name]
            if resolve is None:
                prm = True
            elif reads == "params":
                prm = resolve(pr, gp, *args)
            elif reads == "mesh":
                prm = resolve(mesh, pr, gp, *args)
            else:
                prm = resolve(self, mir, dm)
            if prm:  # (None, False, a zero modulus: switched off)
                mods |= bit
                p[name] = prm
        return mods, p

    def _check(self, mir, mods, p, area_con):
        """Every refusal that reads only names, parameters and the mesh, in one order, with what is resolved on the way
        (the two modules admitted by the other modules' bits, the constraint bits, the bending model, the leaflets'
        parameters) -> (module mask, bending model, gradient mode, volume stiffness, target volume, tilt_thetaB_boundary_in's
        tables, (leaflet parameters, absent outer rows or None) or None).  Nothing here touches the device: no upload precedes a refusal."""
        gp, names, cons = self.global_params, self.energy_module_names, self.constraint_module_names
        rim_bilayer, thetab = p.get("tilt_rim_source_bilayer"), p.get("tilt_thetaB_contact_in")
        if rim_bilayer is not None:
            if mods & _SINGLE_TILT_BITS:
                raise L.MembraneHipError("tilt_rim_source_bilayer together with a single-field tilt module is outside "
                                         "the HIP hot path")
            if rim_bilayer["follow"] and (self._pin_names or "volume" in cons):
                raise L.MembraneHipError("tilt_rim_source_bilayer in follow mode (pin_to_circle_mode: fit) next to "
                                         "pin_to_plane / pin_to_circle or the volume constraint's enforcer on the line "
                                         "search is outside the HIP hot path")
            if not (np.all(np.isfinite(rim_bilayer["gamma"])) and np.all(np.isfinite(rim_bilayer["center"]))
                    and np.all(np.isfinite(rim_bilayer["normal"]))):
                raise L.MembraneHipError("tilt_rim_source_bilayer: gamma, tilt_rim_source_center and the frame's normal "
                                         "must be finite")
        if thetab is not None and mods & _SINGLE_TILT_BITS:
            raise L.MembraneHipError("tilt_thetaB_contact_in together with a single-field tilt module is outside the "
                                     "HIP hot path")
        self._thetab_update = thetab is not None and thetab["penalty_mode"] == "legacy" and thetab["k"] > 0.0
        if _RIM_MATCH in p:  # (a non-zero strength)
            p[_RIM_MATCH] = self._rim_match_params(mods)
            if p[_RIM_MATCH] is None:
                del p[_RIM_MATCH]
                mods &= ~_MODULES[_RIM_MATCH].bit
            else:
                del self._const_energy[_RIM_MATCH]
        tbb = self._thetab_boundary_params(mods) if _tbb.NAME in cons else None
        self._tbb_active = tbb is not None
        vol_mode = gp.get("volume_constraint_mode", "lagrange")
        target_volume = self._target_volume() if getattr(self.mesh, "bodies", None) else None
        target = 0.0 if target_volume is None else target_volume
        stiffness = float(gp.get("volume_stiffness") or 0.0)
        if mods & L.MS_MOD_VOLUME_PENALTY:
            stiffness, target = body_penalty_params(self.mesh, gp, self.param_resolver)
        if "volume" in cons and vol_mode == "lagrange" and target_volume is not None:
            mods |= L.MS_CON_VOLUME
        if target_volume is not None and vol_mode == "lagrange" and not gp.get("volume_projection_during_minimization", True):
            mods |= L.MS_TRACK_VOLUME  # drift check of minimizer.py:1478-1513
        if area_con is not None and area_con[0] == L.MS_AREA_BODY:
            mods |= L.MS_CON_BODY_AREA  # its row takes part in the KKT projection (global_area has none)
        self._area_con = area_con
        model = bending_model(gp)
        if (mods & L.MS_MOD_BENDING) and (mods & L.MS_MOD_BENDING_TILT):
            raise L.MembraneHipError("bending and bending_tilt together are outside the HIP hot path")
        if mods & L.MS_MOD_BENDING_TILT:
            model = "helfrich"  # bending_tilt.py:212-215
        any_bend = mods & _BEND_BITS
        mode = bending_gradient_mode(gp) if any_bend else "analytic"
        if mode == "approx" and (mods & L.MS_MOD_BENDING_TILT) and np.any(_boundary(self.mesh)) \
                and names.index("bending_tilt") != len(names) - 1:
            raise L.MembraneHipError(
                "bending_gradient_mode=approx with modules listed AFTER bending_tilt on an open mesh is "
                "not on the fused device path (bending_tilt.py:297-299 zeroes boundary rows of what was "
                "accumulated so far); list bending_tilt last")
        for edge_mod in _EDGE_MODULES:
            if mode == "approx" and edge_mod in p and np.any(_boundary(self.mesh)):
                # (bending.py:165-166 / bending_tilt.py:297-299 zero the boundary rows of what the modules listed before
                # them accumulated; the device adds the edge modules' rows behind the whole gradient pass)
                raise L.MembraneHipError(f"{edge_mod} with bending_gradient_mode=approx on an open mesh is outside the "
                                         "HIP hot path")
        if mode == "approx" and (mods & L.MS_MOD_BENDING):
            if names.index("bending") != len(names) - 1 and np.any(_boundary(self.mesh)):
                raise L.MembraneHipError(
                    "bending_gradient_mode=approx with energy modules listed AFTER bending on an "
                    "open mesh is not on the fused device path (bending.py:165-166 zeroes boundary "
                    "rows of what was accumulated so far); list bending last")
        if "tilt_splay_twist_in" in p:
            if mods & _SINGLE_TILT_BITS:
                raise L.MembraneHipError("tilt_splay_twist_in together with a single-field tilt module is outside the "
                                         "HIP hot path")
            if self._pin_names:
                raise L.MembraneHipError("tilt_splay_twist_in next to pin_to_plane / pin_to_circle is outside the HIP "
                                         "hot path")
            if _fplane.NAME in cons:
                raise L.MembraneHipError("tilt_splay_twist_in next to fixed_plane is outside the HIP hot path")
            if "volume" in cons:
                raise L.MembraneHipError("tilt_splay_twist_in next to the volume constraint's enforcer is outside the "
                                         "HIP hot path")
        if (mods & _SINGLE_TILT_BITS) and (mods & _LEAFLET_BITS):
            raise L.MembraneHipError("single-field and leaflet tilt modules together are outside the HIP hot path")
        leaflet = None
        if mods & _LEAFLET_BITS:
            _lc.check_supported(gp, self.mesh)
            if gp.get("line_search_reduced_energy", False):
                raise L.MembraneHipError("line_search_reduced_energy is outside the HIP hot path")
            # leaflet_out_absent_presets: the rows and validate_leaflet_absence_topology once per topology (as the mirror
            # keys it) and preset list (refresh_modules() after the vertex presets change); what cannot read the mask is refused
            absent = None
            presets = gp.get("leaflet_out_absent_presets")
            if presets and (presets := _lc.normalize_preset_list(presets)):
                akey = (mir._topology_key(), tuple(sorted(presets)),
                        str(gp.get("leaflet_out_absence_mode", "strict") or "strict").strip().lower())
                if getattr(self, "_absent_key", None) != akey:
                    _lc.validate_absence_topology(self.mesh, gp)
                    self._absent_rows = _lc.absent_out_rows(self.mesh, gp)
                    self._absent_key = akey
                absent = self._absent_rows
                if mods & L.MS_MOD_BENDING_TILT_OUT:
                    raise L.MembraneHipError(_lc.BT_OUT_ABSENT_MESSAGE)
            leaflet = ({lf: _lc.device_params(self.param_resolver, gp, lf) for lf in ("in", "out")}, absent)
            if mods & _LEAFLET_BT_BITS:
                _lc.check_bt_supported(gp)
                if mods & _BEND_BITS:
                    raise L.MembraneHipError("bending / bending_tilt together with bending_tilt_in/out is outside "
                                             "the HIP hot path")
        if mods & _SINGLE_TILT_BITS:
            if gp.get("line_search_reduced_energy", False):
                raise L.MembraneHipError("line_search_reduced_energy (inner tilt relaxation inside every "
                                         "line-search trial, minimizer.py:568-608) is outside the HIP hot path")
            if str(gp.get("tilt_transport_model", "ambient_v1") or "ambient_v1").strip().lower() != "ambient_v1":
                raise L.MembraneHipError("tilt_transport_model other than ambient_v1 is outside the HIP hot path")
        if _fplane.NAME in cons:
            if mods & _TILT_BITS and ((mods & L.MS_CON_VOLUME) or "volume" in cons):
                raise L.MembraneHipError("fixed_plane next to tilt modules together with the volume constraint is "
                                         "outside the HIP hot path")
            if rim_bilayer is not None and rim_bilayer["follow"]:  # (ms_step refuses the one-leaflet sources' follow mode)
                raise L.MembraneHipError("tilt_rim_source_bilayer in follow mode (pin_to_circle_mode: fit) next to "
                                         "fixed_plane's enforcer on the line search is outside the HIP hot path")
        return mods, model, mode, stiffness, target, tbb, leaflet

    def _apply(self, mir, dm, p, area_con, checked):
        """Synchronise the mirror and upload what _resolve() and _check() made: the per-module tables where their key
        changed, what goes with every configuration, the constraints' tables, and set_params behind ``_configured_key``."""
        mods, model, mode, stiffness, target, tbb, leaflet = checked
        gp = self.global_params
        if dm is None:
            dm = mir.sync()
            if self.deterministic is not None:
                dm.set_deterministic(self.deterministic)
        topo, keys = mir._topo_key, mir._leaflet_keys
        if mods & L.MS_MOD_SURFACE:
            mir.upload_surface_tension()
        if mods & _BEND_BITS:
            mir.upload_bending_params(gp, model)
        if mods & _LEAFLET_BITS:
            if leaflet[1] is None:
                mir.upload_leaflets(leaflet[0])  # (clears the mask of an earlier configuration)
            else:
                mir.upload_leaflets(leaflet[0], absent_out=leaflet[1])
            # the modules' tables ("bend_": no tilt upload, mark_device_leaflets_current leaves the key): keyed on topology
            # and parameters, and on the context where the table is its own; the leaflets' in the modules' listed order
            for lf in self._disk_order:
                if (prm := p.get("tilt_disk_target_" + lf)) is not None:
                    key = (topo, prm["disk_rows"].tobytes(), tuple([kv for kv in prm.items() if kv[0] != "disk_rows"]))
                    _keyed_upload(keys, "bend_disk_" + lf, key, dm, "set_leaflet_disk_target", (lf,), prm)
            for lf in self._rim_order:
                if (prm := p.get("tilt_rim_source_" + lf)) is not None:
                    _keyed_upload(keys, "bend_rim_" + lf, (topo, _lc.rim_source_key(prm)), dm, "set_leaflet_rim_source", (lf,), prm)
            if (prm := p.get("tilt_rim_source_bilayer")) is not None:
                _keyed_upload(keys, "bend_rim_bilayer", (topo, _lc.rim_source_key(prm)), dm, "set_rim_source_bilayer", (), prm)
            if (prm := p.get("tilt_thetaB_contact_in")) is not None:  # (theta_B goes with every configuration)
                _keyed_upload(keys, "bend_thetab", (topo, id(dm), _lc.thetab_contact_key(prm)), dm, "set_thetab_contact", (), prm)
                dm.set_thetab_value(_lc.thetab_value(gp))
            if (prm := p.get(_RIM_MATCH)) is not None:
                _keyed_upload(keys, "bend_rim_match", (topo, id(dm), _lc.rim_match_key(prm)), dm, "set_rim_match", (), prm)
            # tilt_thetaB_boundary_in: keyed like the other ring tables; theta_B and the relaxation's cadence go with every
            # configuration; a table of an earlier configuration is cleared
            key = None if tbb is None else (topo, id(dm), _tbb.device_key(tbb))
            old = keys.get("bend_tbb")
            if old != key:
                if tbb is not None:
                    dm.set_thetab_boundary(**tbb)
                elif old is not None and old[1] == id(dm):
                    dm.set_thetab_boundary(None)
                keys["bend_tbb"] = key
            if tbb is not None:
                dm.set_thetab_value(_lc.thetab_value(gp))
                dm.set_tilt_projection(*_tbb.projection_schedule(gp))
            if (prm := p.get("tilt_coupling")) is not None:  # modulus and sign
                _keyed_upload(keys, "bend_coupling", (id(dm), prm), dm, "set_tilt_coupling", prm)
            if (prm := p.get("tilt_splay_twist_in")) is not None:  # the two moduli
                _keyed_upload(keys, "bend_splay_twist", (id(dm), prm), dm, "set_tilt_splay_twist", prm)
            for lf in ("in", "out"):
                if "bending_tilt_" + lf in p:
                    kappa, c0 = _lc.bending_params(self.mesh, gp, lf)
                    _keyed_upload(keys, "bend_" + lf, (topo, kappa.tobytes(), c0.tobytes()), dm, "set_leaflet_bending",
                                  (lf, kappa, c0))
        if mods & _SINGLE_TILT_BITS:
            mir.upload_tilts(gp)
            mir.upload_tilt_fixed()
            dm.set_tilt_smoothness(float(gp.get("tilt_smoothness_rigidity", 0.0) or 0.0))
        if self._pin_names:
            self._upload_pins(mir, dm, mods)
        self._upload_enforce_only(mir, dm)
        if area_con is not None or getattr(self, "_area_set_on", None) is dm:
            # (the constraint of an earlier configuration of this minimizer is replaced or cleared)
            if (None if area_con is None else area_con[:2]) != dm.area_constraint:
                dm.set_area_constraint(*(area_con[:2] if area_con is not None else (L.MS_AREA_NONE, 0.0)))
            self._area_set_on = dm if area_con is not None else None
        area_params = p.get("body_area_penalty")
        key = (mods, model, mode, stiffness, target, area_params, self._line_key, self._edgepen_key, id(dm))
        if key != self._configured_key:
            if area_params is not None:
                dm.set_area_penalty(*area_params)
            dm.set_params(modules=mods,
                          bending_model=L.MS_BEND_HELFRICH if model == "helfrich" else L.MS_BEND_WILLMORE,
                          bending_grad_mode=L.MS_GRAD_ANALYTIC if mode == "analytic" else L.MS_GRAD_APPROX,
                          volume_stiffness=stiffness, target_volume=target)
            self._configured_key = key
        return dm

    def _upload_line(self, mir, dm) -> bool:
        """Resolve the tagged edges and their gamma (modules/energy/line_tension.py) once per mesh topology and
        parameter value (call refresh_modules() after changing the tags) and upload the device tables; True when
        some edge is charged.  A re-tiled mesh is a new context: its tables start empty."""
        key = (mir._topo_key, id(dm), float(self.global_params.get("line_tension", 0.0) or 0.0))
        if self._line_key is None or self._line_key[:3] != key:
            self._line_key = key + (_line.upload(self.mesh, self.global_params, dm),)
        return self._line_key[3]

    def _upload_edge_penalty(self, mir, dm) -> bool:
        """Resolve the charged edges and their targets (modules/energy/edge_length_penalty.py) once per mesh topology,
        edge_stiffness and set of targets (they are hashed: the "fix edges" command rewrites them in place) and
        upload the device tables; True when some edge is charged with k != 0."""
        tail, head, target, num = _edgepen.charged_edges(self.mesh, self.global_params)
        key = (mir._topo_key, id(dm), _edgepen.stiffness(self.global_params), num.tobytes(), target.tobytes())
        if self._edgepen_key is None or self._edgepen_key[:5] != key:
            self._edgepen_key = key + (_edgepen.upload(self.mesh, self.global_params, dm, (tail, head, target, num)),)
        return self._edgepen_key[5]

    def _rim_match_params(self, mods):
        """rim_slope_match_out with a non-zero strength: kwargs of DeviceMesh.set_rim_match, or None where the module is
        a constant 0.0 (no rim / outer group, an empty ring).  Refused here: no active outer-leaflet tilt module -- checked
        first, whatever the groups hold --, a single-field tilt module next to it, a disk ring without an active
        inner-leaflet module (the sharded drivers refuse the bit themselves); in leaflet_common.rim_match_params: the staggered modes, a missing
        normal, a ring above the device's size, non-finite parameters."""
        if not mods & _OUTER_RELAX_BITS:
            raise L.MembraneHipError("rim_slope_match_out with a non-zero rim_slope_match_strength and without an active "
                                     "outer-leaflet tilt module (tilt_out, bending_tilt_out, tilt_smoothness_out, "
                                     "tilt_disk_target_out, tilt_rim_source_out, tilt_coupling, tilt_rim_source_bilayer) is "
                                     "outside the HIP hot path: nothing relaxes the field it couples")
        if mods & _SINGLE_TILT_BITS:
            raise L.MembraneHipError("rim_slope_match_out with a non-zero rim_slope_match_strength together with a "
                                     "single-field tilt module is outside the HIP hot path")
        prm = _lc.rim_match_params(self.mesh, self.param_resolver, self.global_params)
        if prm is None:
            return None
        if len(prm["disk"]) and not mods & _INNER_LEAFLET_BITS:
            raise L.MembraneHipError("rim_slope_match_out with a non-zero rim_slope_match_strength and a disk group, "
                                     "without an active inner-leaflet tilt module (tilt_in, bending_tilt_in, "
                                     "tilt_smoothness_in, ...), is outside the HIP hot path: nothing relaxes the inner field "
                                     "it couples")
        return prm

    def _thetab_boundary_params(self, mods):
        """tilt_thetaB_boundary_in: kwargs of DeviceMesh.set_thetab_boundary, or None where the module is not listed or
        does nothing (no group, no tagged row).  Everything the device path does not take is refused here, before
        anything is uploaded."""
        if _tbb.NAME not in self.constraint_module_names:
            return None
        gp = self.global_params
        prm = _tbb.device_params(self.mesh, gp)  # (a missing normal, non-finite parameters, the grown "disk" ring,
        if prm is None:                          # tilt_thetaB_optimize: refused there)
            return None
        _tbb.projection_schedule(gp)  # ValueError on the values the reference rejects
        if mods & _SINGLE_TILT_BITS:
            raise L.MembraneHipError("tilt_thetaB_boundary_in together with a single-field tilt module is outside the "
                                     "HIP hot path")
        if not mods & _INNER_LEAFLET_BITS:
            raise L.MembraneHipError("tilt_thetaB_boundary_in without an active inner-leaflet tilt module (tilt_in, "
                                     "bending_tilt_in, ...) is outside the HIP hot path: nothing relaxes the field it "
                                     "constrains")
        if "volume" in self.constraint_module_names:
            raise L.MembraneHipError("tilt_thetaB_boundary_in next to the volume constraint's enforcer is outside the "
                                     "HIP hot path")
        if self._pin_names:
            X = np.asarray(self.mesh.positions_view(), dtype=np.float64)
            if not _pins.device_tables(X, _pins.programs(self.mesh, self._pin_names), []).params:
                # the reference's line search then has an enforcer that moves nothing but the ring's tilts; the device
                # switches its enforcer lane on with the pin program
                raise L.MembraneHipError("tilt_thetaB_boundary_in next to a pin module that pins nothing is outside the "
                                         "HIP hot path")
            if self._target_volume() is not None and gp.get("volume_constraint_mode", "lagrange") == "lagrange" \
                    and not gp.get("volume_projection_during_minimization", True):
                # the volume drift check of a step (minimizer.py:1478-1513) then runs the mesh-operation enforcement
                # inside ms_minimize, whose lane does not run the tilt constraint between the pins and the projection
                raise L.MembraneHipError("tilt_thetaB_boundary_in next to pins and the volume drift check of a body with "
                                         "a target volume is outside the HIP hot path")
        return prm

    def _upload_pins(self, mir, dm, mods):
        """Resolve the pin tags once per mesh topology, fixed mask and row set (call refresh_modules() after
        changing the tags or the pin parameters) and upload the device tables; an empty program (nothing tagged, or
        only slide circles of fewer than three members, which the reference skips) clears them; the project-or-skip decision is the reference's KKT solve on C = [volume row;
        pin rows] at the current positions (runtime/constraint_projection.py:101-129)."""
        volrow = bool(mods & L.MS_CON_VOLUME)
        if mods & _TILT_BITS and (volrow or "volume" in self.constraint_module_names):
            raise L.MembraneHipError("pin_to_plane / pin_to_circle next to tilt modules together with the volume "
                                     "constraint are outside the HIP hot path")
        key = (mir._topo_key, id(dm), volrow, np.asarray(self.mesh.fixed_mask, dtype=bool).tobytes())
        if key == self._pin_key:
            return
        X = np.asarray(self.mesh.positions_view(), dtype=np.float64)
        dense = [_volume_gradient(self.mesh, X)] if volrow else []
        self.pin_tables = _pins.device_tables(X, _pins.programs(self.mesh, self._pin_names), dense)
        self._pins_active = bool(self.pin_tables.params)
        dm.set_pins(self.pin_tables if self._pins_active else None)
        self._pin_key = key

    def _target_volume(self):
        bodies = getattr(self.mesh, "bodies", None) or {}
        if not bodies:
            return None
        body = next(iter(bodies.values()))
        t = body.target_volume
        if t is None:
            t = (body.options or {}).get("target_volume")
        return None if t is None else float(t)

    # -- evaluation entry points ------------------------------------------------
    def compute_energy_and_gradient_array(self):
        """Total energy and dense gradient (minimizer.py:941-992)."""
        _mir, dm = self._device()
        e, g = dm.energy_and_gradient(want_grad=True)
        return float(e.sum()) + self._energy_offset, g

    def compute_energy_and_gradient(self):
        E, g = self.compute_energy_and_gradient_array()
        return E, GradientRows(self.mesh, g)

    def compute_energy(self) -> float:
        """minimizer.py:1051-1054."""
        _mir, dm = self._device()
        return float(dm.energy().sum()) + self._energy_offset

    def compute_energy_breakdown(self) -> Dict[str, float]:
        """Per-module energies (minimizer.py:1056-1065)."""
        _mir, dm = self._device()
        e = dm.energy()
        out = {}
        for name in self.energy_module_names:
            out[name] = self._const_energy.get(name, 0.0) if _ENERGY_SLOT[name] is None else float(e[_ENERGY_SLOT[name]])
        if "body_area_penalty" in out:  # energies[2] is volume penalty + area penalty: each module reports its own
            area_e = dm.area_penalty_energy() if dm.modules & L.MS_MOD_AREA_PENALTY else 0.0
            out["body_area_penalty"] = area_e
            if "volume" in out and dm.modules & L.MS_MOD_AREA_PENALTY:
                k, v0 = body_penalty_params(self.mesh, self.global_params, self.param_resolver) \
                    if dm.modules & L.MS_MOD_VOLUME_PENALTY else (0.0, 0.0)
                dv = float(dm.fetch_scalars()[L.MS_S_VOL]) - v0
                out["volume"] = 0.5 * k * (dv * dv)
        if any(n in out for n in _EDGE_MODULES):
            # energies[0] is surface + line tension + edge length penalty: each module reports its own
            line_e = dm.line_energy() if dm.modules & L.MS_MOD_LINE_TENSION else 0.0
            pen_e = dm.edge_penalty_energy() if dm.modules & L.MS_MOD_EDGE_LENGTH_PENALTY else 0.0
            if "line_tension" in out:
                out["line_tension"] = line_e
            if "edge_length_penalty" in out:
                out["edge_length_penalty"] = pen_e
            if "surface" in out:
                out["surface"] = float(e[0]) - line_e - pen_e if dm.modules & L.MS_MOD_SURFACE else 0.0
        # the ride-along modules: each reports its own energy, and whoever reports the slot its sums ride in, or
        # energies[3], reports it without that part
        own, parts = [], {}
        for name, rec in _MODULES.items():
            if rec.energy is None:
                continue
            v = rec.energy(dm) if dm.modules & rec.bit else 0.0
            own.append(v[0] if isinstance(v, tuple) else v)
            for k, host in enumerate(rec.hosts):
                parts.setdefault(host, []).append(v[1 + k] if isinstance(v, tuple) else v)
            if name in out and dm.modules & rec.bit:
                out[name] = own[-1]
        for table in (_TILT_SCALAR, _BEND_SCALAR):
            sharing = [n for n in out if n in table]
            if len(sharing) > 1:  # they share one entry of the energy vector: split via the scalars
                sc = dm.fetch_scalars()
                for n in sharing:
                    out[n] = float(sc[table[n]]) if dm.modules & _ENERGY_BITS[n] else 0.0
                    if n in parts and dm.modules & _ENERGY_BITS[n]:
                        out[n] -= parts[n][0] + sum(parts[n][1:])
            elif len(sharing) == 1 and table is _TILT_SCALAR and any(own):
                out[sharing[0]] = float(e[3])
                for v in own:
                    out[sharing[0]] -= v
        return out

    # -- constraint enforcement (minimizer.py:1103-1188) ---------------------------
    def _enforce(self, dm, context: str, first_step_cached: bool = False) -> bool:
        """Volume projection on the device.  Returns True if positions moved.  ``first_step_cached``: the
        reference's Body still holds the volume gradient of its previous projection and a compute_volume at the
        current mesh version has made that cache look current (ms_project_volume_cached)."""
        if not self._has_enforceable_constraints:
            return False
        self._vol_ended_on_eval = False
        moved = self._enforce_pins_volume(dm, context, first_step_cached)
        if self._area_con is not None:
            # body_area / global_area behind them, in every context (enforce_all's order; body_area.py:87, global_area.py:8:
            # tol 1e-12, max_iter 20 / 3 whatever the context).  A volume projection that ended on an evaluation leaves
            # Body's cache looking current: body_area's first pass then reads the cached area (ms_project_area_cached)
            iters, _a = dm.project_area(tol=1e-12, max_iter=self._area_con[2],
                                        first_step_cached=self._vol_ended_on_eval)
            moved = moved or iters > 0
        return moved

    def _enforce_pins_volume(self, dm, context: str, first_step_cached: bool = False) -> bool:
        moved = False
        if self._fplane_active:  # fixed_plane.py:25-53: in every context, listed in front of every other enforcer
            dm.enforce_fixed_plane()
            moved = True
        if self._pins_active:  # constraint_manager.enforce_all: the pins in every context, listed before volume
            dm.enforce_pins()
            moved = True
        if self._perim_active:  # perimeter.py:27-74: tol 1e-10, 3 passes whatever the context; behind the pins
            passes, _p = dm.project_perimeter(tol=1e-10, max_iter=3)
            moved = moved or int(passes.sum()) > 0
        if self._tbb_active:
            # minimizer.py:1112-1120, :1165-1171: enforce_tilt_constraints behind enforce_all, on the pinned surface; the
            # tangent projection of the finalize / mesh-operation contexts below comes after it
            dm.thetab_boundary_enforce()
            moved = True
        gp = self.global_params
        if context == "minimize" and not gp.get("volume_projection_during_minimization", True):
            return moved
        target = self._target_volume()
        if target is None or "volume" not in self.constraint_module_names:
            if (self._pin_names or _fplane.NAME in self.constraint_module_names) \
                    and context in ("finalize", "mesh_operation") and dm.modules & _TILT_BITS:
                # minimizer.py:1186, :1224: the pins alone are an enforcer as well -- the tilts go onto the tangent
                # planes of the pinned surface before the next evaluation reads them.  Keyed on the LISTED pin modules,
                # not on _pins_active: the reference projects whenever a constraint module with enforce_constraint is
                # loaded (_has_enforceable_constraints), an empty pin program included
                dm.project_tilts_to_tangent()
                moved = True
            return moved
        max_iter = 12 if context in ("finalize", "mesh_operation") else 3
        iters, _v = dm.project_volume(target, tol=1e-12, max_iter=max_iter, first_step_cached=first_step_cached)
        self._vol_ended_on_eval = iters < max_iter
        moved = moved or iters > 0
        if context in ("finalize", "mesh_operation") and dm.modules & _TILT_BITS:
            # minimizer.py:1186, :1224, :1506: every enforce outside the line search is followed by
            # mesh.project_tilts_to_tangent() -- the tilts must be tangent to the PROJECTED surface before the
            # next energy / gradient evaluation reads them
            dm.project_tilts_to_tangent()
            moved = True
        return moved

    # -- tilt relaxation (runtime/steppers/tilt_relaxation.py:237-300 parameter handling) --
    def _tilt_relax_params(self):
        """Resolved relaxation parameters or None when tilt_solve_mode leaves the tilts alone."""
        gp = self.global_params
        mode = str(gp.get("tilt_solve_mode", "fixed") or "").strip().lower()
        if mode in ("", "none", "off", "false", "fixed"):
            return None
        if mode not in ("nested", "coupled"):
            logger.warning("Unknown tilt_solve_mode=%r; treating as 'fixed'.", mode)
            return None
        step = float(gp.get("tilt_step_size", 0.0) or 0.0)
        if step <= 0.0:
            return None
        tol = float(gp.get("tilt_tol", 0.0) or 0.0)
        if mode == "nested":
            n_inner = int(gp.get("tilt_inner_steps", 0) or 0)
        else:
            n_inner = int(gp.get("tilt_coupled_steps", gp.get("tilt_inner_steps", 0)) or 0)
        if n_inner <= 0:
            return None
        solver = str(gp.get("tilt_solver", "cg") or "cg").strip().lower()
        if solver not in ("gd", "cg"):
            logger.warning("Unknown tilt_solver=%r; using gradient descent.", solver)
            solver = "gd"
        max_iters = int(gp.get("tilt_cg_max_iters", n_inner) or 0) if solver == "cg" else n_inner
        if max_iters <= 0:
            return None
        pre = str(gp.get("tilt_cg_preconditioner", "jacobi") or "jacobi").strip().lower()
        return {"solver": solver, "max_iters": max_iters, "step_size": step, "tol": max(tol, 0.0),
                "jacobi": pre == "jacobi"}

    def _relax_tilts(self, dm) -> bool:
        rp = self._tilt_relax_params()
        if rp is None:
            return False
        if dm.modules & _LEAFLET_BITS:
            dm.relax_leaflet_tilts(**rp)  # minimizer.py:1240-1305 (no energy guard)
        else:
            dm.relax_tilts(**rp)
        return True

    def _update_scalar_params(self, dm) -> None:
        """minimizer.py:1234, :1309 -> tilt_thetaB_contact_in.update_scalar_params (:271-302): theta_B of the legacy
        penalty mode from the ring's three scalars on the device's positions and stored inner tilts
        (ms_update_thetab_value), written back into ``tilt_thetaB_value``.  Skipped when the penalty mode is off."""
        if not getattr(self, "_thetab_update", False) or not dm.modules & L.MS_MOD_TILT_THETAB_CONTACT_IN:
            return
        tb, changed = dm.update_thetab_value()
        if changed:
            _lc._set_param(self.global_params, "tilt_thetaB_value", float(tb))

    @property
    def _energy_offset(self) -> float:
        """Sum of the host-side constant modules (set by _device())."""
        return float(sum(getattr(self, "_const_energy", {}).values()))

    def _write_back_tilts(self, dm, mir):
        """Device tilt fields -> mesh (the reference leaves relaxed / projected tilts on the mesh)."""
        if dm.modules & _SINGLE_TILT_BITS:
            self.mesh.set_tilts_from_array(dm.get_tilts())
            mir.mark_device_tilts_current()
        if dm.modules & _LEAFLET_BITS:
            self.mesh.set_tilts_in_from_array(dm.get_leaflet_tilts("in"))
            self.mesh.set_tilts_out_from_array(dm.get_leaflet_tilts("out"))
            mir.mark_device_leaflets_current()

    def _fast_path_ok(self, callback) -> bool:
        """The whole loop can run inside the library (ms_minimize) when nothing on the Python side
        wants to see individual steps: no callback, quiet, and the stepper's device_step is the
        stock one (tests and tools wrap it to log steps)."""
        st = self.stepper
        if getattr(self, "_thetab_update", False):
            # theta_B is updated twice per step from the device's scalars (_update_scalar_params): the Python loop's work
            return False
        return (callback is None and self.quiet and isinstance(st, BaseStepper)
                and "device_step" not in vars(st) and type(st).device_step is BaseStepper.device_step)

    def _minimize_in_library(self, mir, dm, n_steps, sync_mesh):
        gp = self.global_params
        st = self.stepper
        st._dm = dm
        edge_fraction = float(gp.get("shape_step_edge_fraction", 0.0) or 0.0)
        extra = st._extra()
        mp = L.ms_minimize_params()
        mp.stepper = L.ms_stepper_params(int(st.stepper_id), int(st._max_iter_for(self.mesh)), float(st.beta),
                                         float(st.c), float(st.gamma), float(st.alpha_max_factor),
                                         int(extra.get("restart_interval", 10)), edge_fraction,
                                         int(st.reuse_energy0), int(getattr(st, "enforce_volume", 0)),
                                         int(extra.get("precondition", 0)), int(getattr(st, "enforce_pins", 0)),
                                         int(getattr(st, "enforce_fixed_plane", 0)),
                                         int(getattr(st, "enforce_perimeter", 0)),
                                         int(getattr(st, "enforce_area", 0) > 0), int(getattr(st, "enforce_area", 0)))
        step_mode = str(gp.get("step_size_mode", "adaptive") or "adaptive").lower()
        mp.step_size = float(self.step_size)
        mp.tol = float(self.tol)
        mp.fixed_step_mode = 1 if step_mode == "fixed" else 0
        mp.fixed_step = float(gp.get("step_size", self.step_size) or self.step_size)
        mp.max_zero_steps = int(self.max_zero_steps)
        mp.step_size_floor = float(self.step_size_floor)
        target = self._target_volume()
        mp.drift_check = 1 if (gp.get("volume_constraint_mode", "lagrange") == "lagrange"
                               and not gp.get("volume_projection_during_minimization", True)
                               and target is not None) else 0
        mp.target_volume = float(target) if target is not None else 0.0
        mp.volume_tolerance = float(gp.get("volume_tolerance", 1e-3))
        mp.project_on_drift = 1 if self._has_enforceable_constraints else 0
        rp = self._tilt_relax_params() if dm.modules & (_TILT_BITS) else None
        mp.relax_tilts = 0 if rp is None else 1
        if rp is not None:
            mp.relax = L.ms_tilt_relax_params(1 if rp["solver"] == "cg" else 0, rp["max_iters"], rp["step_size"],
                                              rp["tol"], 1 if rp["jacobi"] else 0)
        out, log = dm.minimize(mp, n_steps, want_log=True)
        self.step_size = float(out.step_size)
        self.last_run = {"accepted": out.accepted, "trials": out.trials, "guard_rejects": out.guard_rejects,
                         "iterations": out.iterations, "step_log": log}
        return out

    # -- the loop -------------------------------------------------------------------
    def minimize(self, n_steps: int = 1, callback: Optional[Callable] = None, *, sync_mesh: bool = True):
        """Run ``n_steps`` iterations (minimizer.py:1189-1535).

        ``sync_mesh=False`` leaves the new positions in HBM only (the mesh object is
        refreshed by the next call that uses ``sync_mesh=True`` or by
        ``sync_mesh_from_device()``); benchmarks use it to keep PCIe out of the loop."""
        mir, dm = self._device()
        gp = self.global_params
        # minimizer.py:1379: the stepper gets Minimizer._enforce_constraints as its constraint enforcer; with
        # volume_projection_during_minimization on (the programmatic default) that projects every trial onto the
        # target volume before its energy is taken (line_search.py:428-487) -- on the device: ms_stepper_params.enforce_volume
        self.stepper.enforce_volume = int(bool(
            self._has_enforceable_constraints and gp.get("volume_projection_during_minimization", True)
            and gp.get("volume_constraint_mode", "lagrange") == "lagrange" and self._target_volume() is not None
            and (dm.modules & L.MS_CON_VOLUME)))
        self.stepper.enforce_pins = int(self._pins_active)  # (pins always have enforce_constraint)
        # (so do body_area / global_area: the projection on every trial, with the module's own max_iter)
        self.stepper.enforce_area = int(self._area_con[2]) if self._area_con is not None else 0
        # (fixed_plane / perimeter have enforce_constraint as well: minimizer.py:114-116 switches the enforcer lane on)
        self.stepper.enforce_fixed_plane = int(self._fplane_active)
        self.stepper.enforce_perimeter = int(self._perim_active)
        if n_steps <= 0:
            E, g = self.compute_energy_and_gradient_array()
            moved = self._enforce(dm, "minimize")
            if moved:
                write_back_positions(self.mesh, dm, mir)
            return {"energy": float(self.compute_energy()), "gradient": GradientRows(self.mesh, g),
                    "mesh": self.mesh, "step_success": True, "iterations": 0, "terminated_early": True}

        dirty = False
        if self._has_enforceable_constraints:
            dirty |= self._enforce(dm, "mesh_operation")

        if self._fast_path_ok(callback):
            out = self._minimize_in_library(mir, dm, n_steps, sync_mesh)
            moved = bool(out.moved) or dirty
            early = bool(out.converged or out.zero_step_exit)
            if out.converged:
                logger.info("Converged in %d iterations; |grad E|=%.3e", out.iterations - 1, out.grad_norm)
            moved_by_finalize = False
            if not out.zero_step_exit:  # minimizer.py:1324-1337 / :1516-1535 finalize the constraints
                moved_by_finalize = self._enforce(dm, "finalize", first_step_cached=bool(out.volume_cache_current))
                moved |= moved_by_finalize
            if out.converged:
                energy = float(out.energy_eval) + self._energy_offset
            elif out.energy_current_valid and not moved_by_finalize:
                # the step logic already holds the energies of the positions the loop ended at (reuse level 2: a pass
                # whose result is on the device is not repeated)
                energy = float(out.energy_current) + self._energy_offset
            else:
                energy = float(dm.energy().sum()) + self._energy_offset
            if moved or self._device_ahead:
                if sync_mesh:
                    write_back_positions(self.mesh, dm, mir)
                    if dm.modules & (_TILT_BITS):
                        self._write_back_tilts(dm, mir)
                    self._device_ahead = False
                else:
                    self._device_ahead = True
            return {"energy": energy, "gradient": GradientRows(self.mesh, dm.get_gradient() if sync_mesh
                                                               else dm.get_gradient),
                    "mesh": self.mesh, "step_success": bool(out.step_success) if not out.zero_step_exit else False,
                    "iterations": int(out.iterations), "terminated_early": early,
                    "steps_accepted": int(out.accepted), "line_search_trials": int(out.trials)}

        zero_step_counter = 0
        step_success = True
        # Body's cached volume is current (minimizer.py:1492 ran at this mesh version and nothing has bumped it since)
        vol_cache_current = False
        proj_flag = gp.get("volume_projection_during_minimization", True)
        vol_tol = float(gp.get("volume_tolerance", 1e-3))
        vol_mode = gp.get("volume_constraint_mode", "lagrange")
        target = self._target_volume()
        have_grad = False

        def finish(result):
            if dirty_box[0] or self._device_ahead:
                if sync_mesh:
                    write_back_positions(self.mesh, dm, mir)
                    if dm.modules & (_TILT_BITS):  # tilts changed on the device
                        self._write_back_tilts(dm, mir)
                    self._device_ahead = False
                else:
                    self._device_ahead = True
            return result

        dirty_box = [dirty]
        for i in range(n_steps):
            if callback:
                if dirty_box[0]:  # the callback sees the mesh as the reference's does: positions and tilt fields
                    write_back_positions(self.mesh, dm, mir)
                    if dm.modules & (_TILT_BITS):
                        self._write_back_tilts(dm, mir)
                    dirty_box[0] = False
                callback(self.mesh, i)
                mir, dm = self._device()
            self._update_scalar_params(dm)  # minimizer.py:1234
            if dm.modules & (_TILT_BITS):
                if self._relax_tilts(dm):  # minimizer.py:1237-1307, before the convergence check
                    dirty_box[0] = True
            self._update_scalar_params(dm)  # minimizer.py:1309
            step_mode = str(gp.get("step_size_mode", "adaptive") or "adaptive").lower()
            fixed_step = float(gp.get("step_size", self.step_size) or self.step_size)
            step_size_in = fixed_step if step_mode == "fixed" else self.step_size
            r = self.stepper.device_step(dm, self.mesh, step_size_in, tol=self.tol)
            have_grad = True
            if r.converged:  # minimizer.py:1324-1337
                logger.info("Converged in %d iterations; |grad E|=%.3e", i, r.grad_norm)
                dirty_box[0] |= self._enforce(dm, "finalize", first_step_cached=vol_cache_current)
                return finish({"energy": r.energy_eval + self._energy_offset,
                               "gradient": GradientRows(self.mesh, dm.get_gradient()),
                               "mesh": self.mesh, "step_success": True, "iterations": i + 1,
                               "terminated_early": True})
            step_success = r.success
            vol_cache_current = False  # minimizer.py:1415-1416: project_tilts_to_tangent + increment_version
            self.step_size = r.next_step
            if r.success:
                dirty_box[0] = True
            if not self.quiet:
                print(f"Step {i:4d}: Energy = {r.energy:.5f}, Step Size  = {step_size_in:.2e}")
            if step_mode == "fixed":
                self.step_size = fixed_step
            if not step_success:
                if self.step_size <= self.step_size_floor:
                    zero_step_counter += 1
                    if zero_step_counter >= self.max_zero_steps:
                        logger.info("Terminating early after %d consecutive zero-steps", zero_step_counter)
                        return finish({"energy": float(dm.energy().sum()) + self._energy_offset,
                                       "gradient": GradientRows(self.mesh, dm.get_gradient()),
                                       "mesh": self.mesh, "step_success": False, "iterations": i + 1,
                                       "terminated_early": True})
                else:
                    zero_step_counter = 0
                self.stepper.reset()
            else:
                zero_step_counter = 0
                # Lagrange volume drift check (minimizer.py:1478-1513)
                if vol_mode == "lagrange" and not proj_flag and target is not None:
                    vol_cache_current = True  # body.compute_volume at the current mesh version
                    denom = max(abs(target), 1.0)
                    if abs(r.volume - target) / denom > vol_tol:
                        dirty_box[0] |= self._enforce(dm, "mesh_operation", first_step_cached=True)
                        vol_cache_current = False  # enforce_constraints_after_mesh_ops: increment_version
                        self.stepper.reset()
        dirty_box[0] |= self._enforce(dm, "finalize", first_step_cached=vol_cache_current)
        final_energy = float(dm.energy().sum()) + self._energy_offset
        grad = GradientRows(self.mesh, dm.get_gradient() if sync_mesh else dm.get_gradient) if have_grad else {}
        return finish({"energy": final_energy, "gradient": grad, "mesh": self.mesh,
                       "step_success": step_success, "iterations": n_steps, "terminated_early": False})


def _volume_gradient(mesh, X):
    """dV/dx of the (single, whole-mesh) body: sum over facets of cross(x_j, x_k) / 6 at corner i."""
    tri, _ = mesh.triangle_row_cache()
    tri = np.asarray(tri, dtype=np.int64)
    g = np.zeros_like(X)
    a, b, c = X[tri[:, 0]], X[tri[:, 1]], X[tri[:, 2]]
    np.add.at(g, tri[:, 0], np.cross(b, c) / 6.0)
    np.add.at(g, tri[:, 1], np.cross(c, a) / 6.0)
    np.add.at(g, tri[:, 2], np.cross(a, b) / 6.0)
    return g


def _boundary(mesh):
    from ..geometry.mesh import _boundary_mask_of

    return _boundary_mask_of(mesh, len(mesh.vertex_ids))
