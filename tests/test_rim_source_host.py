"""Host side of tilt_rim_source_in / tilt_rim_source_out (no GPU): rim edge selection on an ArrayMesh, the strength
resolution of modules/energy/contact_mapping.py, the frame, the refusals, the library's table builder against a NumPy
construction, and the C ABI."""

import os
import re

import numpy as np
import pytest

from membrane_solver_amd import _lib as L
from membrane_solver_amd import meshgen
from membrane_solver_amd.core.parameters import GlobalParameters, ParameterResolver
from membrane_solver_amd.geometry.mesh import ArrayMesh
from membrane_solver_amd.modules.energy import leaflet_common as lc


def _ring_rows(r):
    start = 1 + 3 * r * (r - 1)
    return list(range(start, start + 6 * r))


def _edge_table(T):
    seen, rows = set(), []
    for a, b, c in np.asarray(T):
        for u, v in ((a, b), (b, c), (c, a)):
            k = (min(u, v), max(u, v))
            if k not in seen:
                seen.add(k)
                rows.append((int(u), int(v)))
    return np.array(rows, dtype=np.int64)


def _mesh(gp, vopts, eopts=None, n=4):
    P, T, B = meshgen.disk_patch(n)
    edges = _edge_table(T)
    return ArrayMesh(P, T, global_parameters=dict(gp), vertex_options=vopts, edges=edges, edge_options=eopts or {}), edges, B


def _params(mesh, leaflet="in"):
    gp = mesh.global_parameters
    return lc.rim_source_params(mesh, ParameterResolver(gp), gp, leaflet)


def _pairs(prm):
    return sorted((min(int(t), int(h)), max(int(t), int(h))) for t, h in zip(prm["tail"], prm["head"]))


# -- edge selection ---------------------------------------------------------------------------------------------------
def test_boundary_mode_selects_the_boundary_ring_only():
    P, T, B = meshgen.disk_patch(4)
    rows = [int(r) for r in np.flatnonzero(B)] + _ring_rows(2)  # the interior ring is tagged as well
    mesh, edges, _ = _mesh({"tilt_rim_source_group_in": "rim", "tilt_rim_source_strength_in": 2.0},
                           {r: {"pin_to_circle_group": "rim"} for r in rows})
    prm = _params(mesh)
    bset = set(int(r) for r in np.flatnonzero(B))
    want = sorted((min(int(t), int(h)), max(int(t), int(h))) for t, h in edges if int(t) in bset and int(h) in bset)
    assert len(want) == 24 and _pairs(prm) == want
    assert np.all(prm["gamma"] == 2.0) and prm["follow"] is False
    assert prm["center"] == (0.0, 0.0, 0.0) and prm["normal"] == (0.0, 0.0, 1.0)


def test_all_mode_selects_interior_ring_and_boundary_mode_finds_nothing_there():
    rows = _ring_rows(3)
    gp = {"tilt_rim_source_group_in": "rim", "tilt_rim_source_strength_in": 2.0, "tilt_rim_source_edge_mode": "ALL "}
    mesh, edges, _ = _mesh(gp, {r: {"pin_to_circle_group": "rim"} for r in rows})
    prm = _params(mesh)
    rs = set(rows)
    assert len(prm["tail"]) == 18
    assert all(int(t) in rs and int(h) in rs for t, h in zip(prm["tail"], prm["head"]))
    mesh.global_parameters.set("tilt_rim_source_edge_mode", "boundary")
    assert _params(mesh) is None
    mesh.global_parameters.set("tilt_rim_source_edge_mode", "something else")  # (anything but "all" is boundary)
    assert _params(mesh) is None


def test_group_rules():
    """The reference's _pin_to_circle_group: no options -> no group; options whose pin_to_circle_group is None (the
    key absent from non-empty options included) -> "default"; anything else -> its string."""
    assert lc.pin_to_circle_group(None) is None and lc.pin_to_circle_group({}) is None
    assert lc.pin_to_circle_group({"pin_to_circle_group": None}) == "default"
    assert lc.pin_to_circle_group({"constraints": ["pin_to_circle"]}) == "default"
    assert lc.pin_to_circle_group({"pin_to_circle_group": 7}) == "7"
    P, T, B = meshgen.disk_patch(4)
    brows = [int(r) for r in np.flatnonzero(B)]
    vo = {r: ({"pin_to_circle_group": None} if j % 2 else {"pin_to_circle_group": "default"}) for j, r in enumerate(brows)}
    mesh, _e, _ = _mesh({"tilt_rim_source_group_in": "default", "tilt_rim_source_strength_in": 1.0}, vo)
    assert len(_params(mesh)["tail"]) == 24
    # one vertex without any options breaks the ring in two places
    vo.pop(brows[3])
    mesh, _e, _ = _mesh({"tilt_rim_source_group_in": "default", "tilt_rim_source_strength_in": 1.0}, vo)
    assert len(_params(mesh)["tail"]) == 22
    # the other leaflet's group key is its own
    assert _params(mesh, "out") is None


def test_nothing_to_do_gives_none():
    P, T, B = meshgen.disk_patch(4)
    vo = {int(r): {"pin_to_circle_group": "rim"} for r in np.flatnonzero(B)}
    assert _params(_mesh({"tilt_rim_source_strength_in": 2.0}, vo)[0]) is None  # no group
    assert _params(_mesh({"tilt_rim_source_group_in": "  ", "tilt_rim_source_strength_in": 2.0}, vo)[0]) is None
    assert _params(_mesh({"tilt_rim_source_group_in": "other", "tilt_rim_source_strength_in": 2.0}, vo)[0]) is None
    assert _params(_mesh({"tilt_rim_source_group_in": "rim"}, vo)[0]) is None  # every gamma 0
    assert _params(_mesh({"tilt_rim_source_group_in": "rim", "tilt_rim_source_strength_in": 0.0}, vo)[0]) is None


# -- gamma ------------------------------------------------------------------------------------------------------------
class _Edge:
    def __init__(self, **options):
        self.options = options


def _gamma(gp, leaflet="in", **edge_options):
    return lc.contact_line_strength(ParameterResolver(GlobalParameters(gp)), _Edge(**edge_options), leaflet)


def test_contact_line_strength_every_branch():
    assert _gamma({}) == 0.0
    # 1: the strength key, the edge's before the global; it wins over every contact key
    assert _gamma({"tilt_rim_source_strength_in": 3.0, "tilt_rim_source_contact_gamma": 9.0}) == 3.0
    assert _gamma({"tilt_rim_source_strength_in": 3.0}, tilt_rim_source_strength_in=4.5) == 4.5
    assert _gamma({"tilt_rim_source_strength_in": 3.0}, tilt_rim_source_strength_in=None) == 3.0
    assert _gamma({"tilt_rim_source_strength_in": 3.0}, "out") == 0.0
    assert _gamma({"tilt_rim_source_strength_in": 0.0, "tilt_rim_source_contact_gamma": 9.0}) == 0.0  # (0 is a value)
    # 2: contact_gamma, suffixed before unsuffixed, edge before global
    assert _gamma({"tilt_rim_source_contact_gamma": 2.0}) == 2.0
    assert _gamma({"tilt_rim_source_contact_gamma": 2.0, "tilt_rim_source_contact_gamma_in": 5.0}) == 5.0
    assert _gamma({"tilt_rim_source_contact_gamma": 2.0, "tilt_rim_source_contact_gamma_in": 5.0}, "out") == 2.0
    assert _gamma({"tilt_rim_source_contact_gamma_in": 5.0}, tilt_rim_source_contact_gamma_in=6.0) == 6.0
    assert _gamma({"tilt_rim_source_contact_gamma_in": 5.0}, tilt_rim_source_contact_gamma=7.0) == 5.0
    # 3: h * (delta_epsilon / a), either spelling; anything missing gives 0
    assert _gamma({"tilt_rim_source_contact_h": 0.5, "tilt_rim_source_contact_delta_epsilon_over_a": 4.0}) == 2.0
    assert _gamma({"tilt_rim_source_contact_h_in": 0.5, "tilt_rim_source_contact_delta_epsilon": 3.0,
                   "tilt_rim_source_contact_a_in": 2.0}) == 0.75
    assert _gamma({"tilt_rim_source_contact_h": 0.5}) == 0.0
    assert _gamma({"tilt_rim_source_contact_h": 0.5, "tilt_rim_source_contact_delta_epsilon": 3.0}) == 0.0
    assert _gamma({"tilt_rim_source_contact_delta_epsilon_over_a": 4.0}) == 0.0
    # 4: units
    si = {"tilt_rim_source_contact_gamma": 2.0, "tilt_rim_source_contact_units": " SI ",
          "tilt_rim_source_contact_length_unit_m": 1e-8, "tilt_rim_source_contact_kappa_ref_J": 4e-20}
    assert _gamma(si) == 2.0 * 1e-8 / 4e-20
    assert _gamma(dict(si, tilt_rim_source_contact_units="physical")) == 2.0 * 1e-8 / 4e-20
    assert _gamma(dict(si, tilt_rim_source_contact_units="solver")) == 2.0
    assert _gamma(dict(si, tilt_rim_source_contact_units="furlongs")) == 2.0
    assert _gamma(dict(si, tilt_rim_source_contact_kappa_ref_J=None)) == 2.0
    assert _gamma(dict(si, tilt_rim_source_contact_length_unit_m=0.0)) == 2.0
    assert _gamma(dict(si, tilt_rim_source_strength_in=3.0)) == 3.0  # (the strength key is never converted)


def test_per_edge_strength_on_the_mesh():
    rows = _ring_rows(3)
    P, T, _B = meshgen.disk_patch(4)
    edges = _edge_table(T)
    ring = [k for k, (t, h) in enumerate(edges) if int(t) in set(rows) and int(h) in set(rows)]
    eo = {ring[0]: {"tilt_rim_source_strength_in": 4.0}, ring[1]: {"tilt_rim_source_strength_in": 0.0}}
    gp = {"tilt_rim_source_group_in": "rim", "tilt_rim_source_edge_mode": "all", "tilt_rim_source_contact_gamma": 1.5}
    mesh, _e, _ = _mesh(gp, {r: {"pin_to_circle_group": "rim"} for r in rows}, eo)
    prm = _params(mesh)
    assert len(prm["gamma"]) == 18
    assert sorted(prm["gamma"].tolist()) == [0.0] + [1.5] * 16 + [4.0]


# -- frame ------------------------------------------------------------------------------------------------------------
def test_frame_resolution():
    rows = _ring_rows(3)
    gp = {"tilt_rim_source_group_in": "rim", "tilt_rim_source_group_out": "rim", "tilt_rim_source_edge_mode": "all",
          "tilt_rim_source_strength_in": 1.0, "tilt_rim_source_strength_out": 1.0, "tilt_rim_source_center": [0.1, 0.2, 0.3]}
    vo = {r: {"pin_to_circle_group": "rim"} for r in rows}
    vo[rows[4]]["pin_to_circle_normal"] = [0.0, 0.0, 0.0]  # (a zero vector is no normal)
    vo[rows[5]]["pin_to_circle_normal"] = [0.0, 3.0, 4.0]  # the first rim row, in row order, that carries one
    vo[rows[9]]["pin_to_circle_normal"] = [1.0, 0.0, 0.0]
    mesh, _e, _ = _mesh(gp, vo)
    prm = _params(mesh)
    assert prm["center"] == (0.1, 0.2, 0.3) and prm["follow"] is False
    assert np.allclose(prm["normal"], (0.0, 0.6, 0.8), rtol=0, atol=1e-16)
    # the outer module's fixed frame never reads the rows' normal (tilt_rim_source_out.py:311-312)
    assert _params(mesh, "out")["normal"] == (0.0, 0.0, 1.0)
    # the global pin_to_circle_normal serves rows without one of their own
    mesh, _e, _ = _mesh(dict(gp, pin_to_circle_normal=[2.0, 0.0, 0.0]), {r: {"pin_to_circle_group": "rim"} for r in rows})
    assert _params(mesh)["normal"] == (1.0, 0.0, 0.0)
    # follow: one rim row (or the global) resolving pin_to_circle_mode to fit
    vo2 = {r: {"pin_to_circle_group": "rim", "pin_to_circle_normal": [0.0, 0.0, 2.0]} for r in rows}
    vo2[rows[7]]["pin_to_circle_mode"] = " Fit"
    mesh, _e, _ = _mesh(gp, vo2)
    assert _params(mesh)["follow"] is True and _params(mesh)["normal"] == (0.0, 0.0, 1.0)
    assert _params(mesh, "out")["follow"] is True
    mesh, _e, _ = _mesh(dict(gp, pin_to_circle_mode="fit", pin_to_circle_normal=[0, 0, 1]), vo)
    assert _params(mesh)["follow"] is True
    mesh, _e, _ = _mesh(dict(gp, pin_to_circle_mode="fixed"), vo)
    assert _params(mesh)["follow"] is False


# -- refusals ---------------------------------------------------------------------------------------------------------
def test_follow_mode_needs_a_normal():
    rows = _ring_rows(3)
    gp = {"tilt_rim_source_group_in": "rim", "tilt_rim_source_edge_mode": "all", "tilt_rim_source_strength_in": 1.0,
          "pin_to_circle_mode": "fit"}
    mesh, _e, _ = _mesh(gp, {r: {"pin_to_circle_group": "rim"} for r in rows})
    with pytest.raises(L.MembraneHipError, match="pin_to_circle_normal"):
        _params(mesh)


def test_array_mesh_without_edges_is_refused():
    from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager
    from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager
    from membrane_solver_amd.runtime.minimizer import Minimizer
    from membrane_solver_amd.runtime.steppers import GradientDescent

    P, T, _B = meshgen.disk_patch(3)
    for name in ("tilt_rim_source_in", "tilt_rim_source_out"):
        mods = ["tilt_in", name]
        mesh = ArrayMesh(P, T, global_parameters={"tilt_rim_source_group_in": "rim"}, energy_modules=mods)
        with pytest.raises(L.MembraneHipError, match="without an edge table"):
            Minimizer(mesh, mesh.global_parameters, GradientDescent(), EnergyModuleManager(mods),
                      ConstraintModuleManager([]), quiet=True)
    mesh = ArrayMesh(P, T, global_parameters={"tilt_rim_source_group_in": "rim", "tilt_rim_source_strength_in": 1.0})
    with pytest.raises(L.MembraneHipError, match="without an edge table"):
        _params(mesh)


def test_modules_load_with_the_reference_interface():
    from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager
    from membrane_solver_amd.runtime import minimizer as mzr

    em = EnergyModuleManager(["tilt_rim_source_in", "tilt_rim_source_out"])
    for name in ("tilt_rim_source_in", "tilt_rim_source_out"):
        mod = em.get_module(name)
        assert mod.USES_TILT_LEAFLETS and mod.IS_EXTERNAL_WORK
        for fn in ("compute_energy_and_gradient", "compute_energy_and_gradient_array", "compute_energy_array"):
            assert callable(getattr(mod, fn))
        assert mzr._ENERGY_SLOT[name] is None and mzr._ENERGY_BITS[name] & mzr._LEAFLET_BITS
    assert mzr._ENERGY_BITS["tilt_rim_source_in"] == L.MS_MOD_TILT_RIM_SOURCE_IN == 524288
    assert mzr._ENERGY_BITS["tilt_rim_source_out"] == L.MS_MOD_TILT_RIM_SOURCE_OUT == 1048576


# -- the library's tables ---------------------------------------------------------------------------------------------
def _numpy_tables(nv, iperm, tail, head, gamma):
    """The documented layout: rim rows ascending (library order), each row's edges in ascending edge order with the other
    end and the edge's gamma; an edge with gamma == 0 is kept."""
    t, h = np.asarray(iperm)[tail], np.asarray(iperm)[head]
    per_row = {}
    for e in range(len(t)):
        per_row.setdefault(int(t[e]), []).append((int(h[e]), float(gamma[e])))
        per_row.setdefault(int(h[e]), []).append((int(t[e]), float(gamma[e])))
    vrow = sorted(per_row)
    off, other, cg = [0], [], []
    for v in vrow:
        other += [o for o, _g in per_row[v]]
        cg += [g_ for _o, g_ in per_row[v]]
        off.append(len(other))
    return np.array(vrow, np.int32), np.array(off, np.int32), np.array(other, np.int32), np.array(cg)


def test_tables_host_matches_numpy_with_a_permutation():
    P, T, B = meshgen.disk_patch(5)
    nv = len(P)
    edges = _edge_table(T)
    rs = set(_ring_rows(3)) | set(int(r) for r in np.flatnonzero(B))
    sel = np.array([k for k, (t, h) in enumerate(edges) if int(t) in rs and int(h) in rs])
    tail, head = edges[sel, 0], edges[sel, 1]
    rng = np.random.default_rng(3)
    gamma = rng.normal(size=len(sel))
    gamma[::4] = 0.0
    iperm = rng.permutation(nv).astype(np.int32)
    got = lc.rim_source_host_tables(nv, iperm, tail, head, gamma)
    vrow, off, other, cg = _numpy_tables(nv, iperm, tail, head, gamma)
    assert got["n_edges"] == len(sel)
    assert np.array_equal(got["vrow"], vrow) and np.array_equal(got["off"], off)
    assert np.array_equal(got["other"], other) and np.array_equal(got["csr_gamma"], cg)
    # nothing: empty tables
    empty = lc.rim_source_host_tables(nv, iperm, [], [], [])
    assert empty["n_edges"] == 0 and len(empty["vrow"]) == 0 and empty["off"].tolist() == [0]
    for bad_tail, bad_gamma in (([nv], [1.0]), ([-1], [1.0]), ([0], [np.nan])):
        with pytest.raises(L.MembraneHipError):
            lc.rim_source_host_tables(nv, iperm, bad_tail, [1], bad_gamma)


def test_c_abi_declares_the_module():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "membrane_hip.h")).read()
    assert re.search(r"#define MS_MOD_TILT_RIM_SOURCE_IN 524288u", hdr)
    assert re.search(r"#define MS_MOD_TILT_RIM_SOURCE_OUT 1048576u", hdr)
    assert re.search(r"MS_NSCAL = 31\b", hdr)  # (no new reduction slot)
    names = {"ms_set_leaflet_rim_source", "ms_get_leaflet_rim_source_energy", "ms_leaflet_rim_source_stats",
             "ms_rim_source_tables_host"}
    for n in names:
        assert re.search(r"\bint %s\(" % n, hdr) and hasattr(L.lib(), n)
    assert names <= set(L.SIGNATURES)
    assert [f[0] for f in L.ms_rim_source_params._fields_] == ["center", "normal", "follow"]
