"""rim_slope_match_out with a non-zero strength, host side (no GPU): group, row and parameter resolution against the
fixtures of tools/gen_golden_rim_slope_match.py, the disk-group rule, every refusal text, the strength-0 path, and the
NumPy restatement of the device's tables (leaflet_common.rim_match_numpy: rank-by-counting, binary-search pairing, one
owner per target row) against every case of the reference.  Bars: energies 1e-12 relative, every gradient entry within
1e-10 of the largest."""

import json
import logging

import numpy as np
import pytest

from conftest import load_golden
from membrane_solver_amd import _lib as L
from membrane_solver_amd import meshgen
from membrane_solver_amd.core.parameters import GlobalParameters, ParameterResolver
from membrane_solver_amd.geometry.mesh import ArrayMesh
from membrane_solver_amd.modules.energy import leaflet_common as lc

NAME = "rim_slope_match_out"
CASES = load_golden("rim_slope_match_cases.npz")
NAMES = [str(n) for n in CASES["names"]]
K, G, GO, GD = "rim_slope_match_strength", "rim_slope_match_group", "rim_slope_match_outer_group", "rim_slope_match_disk_group"
OFF = ("outer_empty", "rim_empty", "no_outer_group", "strength_zero")  # a host constant 0.0: no table, no module bit


def case_mesh(name):
    """The case's mesh as the generator built it: meshgen.disk_patch rotated about z, renumbered by a seeded
    permutation, the rings' rows moved to the recorded positions -> (positions, triangles, tilts_in, tilts_out, gp,
    vertex options)"""
    g = CASES
    spec = json.loads(str(g[name + "__mesh"]))
    P, T, _B = meshgen.disk_patch(spec["n_rings"], bulge=spec["bulge"])
    c, s = np.cos(spec["rot"]), np.sin(spec["rot"])
    P = np.asarray(P, dtype=float) @ np.array([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]])
    perm = np.random.default_rng(spec["perm_seed"]).permutation(len(P))
    P2 = np.empty_like(P)
    P2[perm] = P
    T2 = perm[np.asarray(T)].astype(np.int32)
    rows = g[name + "__rows"].astype(np.int64)
    P2[rows] = g[name + "__positions"]
    tin, tout = np.zeros_like(P2), np.zeros_like(P2)
    tin[rows] = g[name + "__tilts_in"]
    tout[rows] = g[name + "__tilts_out"]
    vo = {int(r): {"rim_slope_match_group": key} for key in ("rim", "outer", "disk") for r in g[name + "__" + key]}
    vo[int(g[name + "__elsewhere"])] = {"rim_slope_match_group": "elsewhere"}
    return P2, T2, tin, tout, json.loads(str(g[name + "__gp"])), vo


def expected(name, nv):
    g = CASES
    rows = g[name + "__rows"].astype(np.int64)
    out = {}
    for key in ("grad", "tilt_in_grad", "tilt_out_grad"):
        a = np.zeros((nv, 3))
        a[rows] = g[name + "__" + key]
        out[key] = a
    return float(g[name + "__E"]), out


def close(got, ref):
    big = float(np.max(np.abs(ref)))
    return not got.any() if big == 0.0 else float(np.max(np.abs(got - ref))) <= 1e-10 * big


def test_fixture_covers_what_the_issue_lists():
    g = CASES
    sizes = {len(g[n + "__rim"]) for n in NAMES}
    assert {1, 2, 3, 4, 63, 64, 65, 255, 256, 257} <= sizes
    for n in NAMES:
        if len(g[n + "__rim"]) >= 255:
            assert json.loads(str(g[n + "__mesh"]))["n_rings"] == 43  # 5677 vertices
    rel_counts = set()
    for n in NAMES:
        r, o = len(g[n + "__rim"]), len(g[n + "__outer"])
        if r and o:
            rel_counts.add("eq" if o == r else "2x" if o == 2 * r else "plus1" if o == r + 1 else "less" if o < r else "more")
    assert {"eq", "2x", "plus1", "less"} <= rel_counts
    assert json.loads(str(g["reference_flags"])) == {"USES_TILT_LEAFLETS": True}


def test_module_keeps_the_reference_names_and_signatures():
    import inspect

    from membrane_solver_amd.modules.energy import rim_slope_match_out as module

    ref = json.loads(str(CASES["reference_signatures"]))
    for fn, params in ref.items():
        assert [p for p in inspect.signature(getattr(module, fn)).parameters] == params, fn
    assert module.USES_TILT_LEAFLETS is True


@pytest.mark.parametrize("name", NAMES)
def test_resolution_matches_fixture(name):
    """Groups, rows in vertex_ids order, frame and strength as the reference resolved them; None where it returns 0.0
    before it looks at a position."""
    P, T, _tin, _tout, gp, vo = case_mesh(name)
    mesh = ArrayMesh(P, T, global_parameters=gp, vertex_options=vo)
    prm = lc.rim_match_params(mesh, ParameterResolver(GlobalParameters(gp)), gp)
    if name in OFF:
        assert prm is None and float(CASES[name + "__E"]) == 0.0
        return
    assert np.array_equal(prm["rim"], CASES[name + "__rim"]) and np.array_equal(prm["outer"], CASES[name + "__outer"])
    disk = CASES[name + "__disk"] if gp.get(GD) == "disk" else np.zeros(0, np.int32)  # (disk == rim group: dropped)
    assert np.array_equal(prm["disk"], disk)
    assert prm["strength"] == gp[K] and prm["normal"] == tuple(gp["rim_slope_match_normal"])
    assert prm["center"] == tuple(gp.get("rim_slope_match_center", [0.0, 0.0, 0.0]))
    assert lc.rim_match_key(prm) == lc.rim_match_key(dict(prm)) and lc.rim_match_key(None) is None


@pytest.mark.parametrize("name", NAMES)
def test_numpy_restatement_matches_reference(name):
    """The device's scheme, restated: the same energy and the same three gradients as the reference's module."""
    P, T, tin, tout, gp, vo = case_mesh(name)
    mesh = ArrayMesh(P, T, global_parameters=gp, vertex_options=vo)
    prm = lc.rim_match_params(mesh, None, gp)
    E_ref, ref = expected(name, len(P))
    if prm is None:
        assert E_ref == 0.0 and not any(a.any() for a in ref.values())
        return
    got = lc.rim_match_numpy(P, tin, tout, **prm)
    print(name, "E", got["E"], "ref", E_ref, "n_valid", got["n_valid"], "local_disk", got["local_disk"])
    assert abs(got["E"] - E_ref) <= 1e-12 * abs(E_ref)
    for key, a in ref.items():
        assert close(got[key], a), key
    if E_ref == 0.0:
        assert not any(got[k].any() for k in ref)
    without = lc.rim_match_numpy(P, tin, tout, shape_gradient=False, **prm)
    assert without["E"] == got["E"] and not without["grad"].any()
    assert np.array_equal(without["tilt_out_grad"], got["tilt_out_grad"])
    if name == "invalid_dr_zero":
        assert got["n_valid"] == len(prm["rim"]) - 1
    if name == "invalid_row_on_center":
        assert 0 < got["n_valid"] < len(prm["rim"])
    if name in ("all_invalid", "rim_without_length", "outer_one_row"):
        assert not got["contributes"]


def test_disk_group_equal_to_the_rim_group_is_dropped_with_one_warning(caplog):
    lc._RIM_MATCH_WARNED = False
    with caplog.at_level(logging.WARNING, logger="membrane_solver"):
        assert lc.rim_match_sanitize_disk_group("rim", "rim") is None
        assert lc.rim_match_sanitize_disk_group("rim", "rim") is None
    assert len([r for r in caplog.records if "rim_slope_match_disk_group matches" in r.getMessage()]) == 1
    assert lc.rim_match_sanitize_disk_group("rim", "disk") == "disk"
    assert lc.rim_match_sanitize_disk_group(None, "disk") == "disk" and lc.rim_match_sanitize_disk_group("rim", None) is None
    assert lc.rim_match_group(None, {G: "  rim "}, G) == "rim" and lc.rim_match_group(None, {G: "  "}, G) is None


def _mesh(gp, tag=True):
    P, T, _B = meshgen.disk_patch(6)
    vo = {}
    if tag:
        for key, ring in (("rim", 3), ("outer", 4), ("disk", 2)):
            start = 1 + 3 * ring * (ring - 1)
            for r in range(start, start + 6 * ring):
                vo[r] = {"rim_slope_match_group": key}
    return ArrayMesh(P, T, global_parameters=dict(gp), vertex_options=vo)


BASE = {G: "rim", GO: "outer", GD: "disk", K: 2.0, "rim_slope_match_normal": [0.0, 0.0, 1.0]}


@pytest.mark.parametrize("change, text", [
    ({"rim_slope_match_mode": "shared_rim_staggered_v1"}, "rim_slope_match_mode=shared_rim_staggered_v1"),
    ({"rim_slope_match_mode": "physical_edge_staggered_v1"}, "rim_slope_match_mode=physical_edge_staggered_v1"),
    ({"rim_slope_match_normal": None}, "without a non-zero rim_slope_match_normal"),
    ({"rim_slope_match_normal": [0.0, 0.0, 0.0]}, "without a non-zero rim_slope_match_normal"),
    ({"rim_slope_match_normal": [0.0, np.nan, 1.0]}, "must be finite"),
    ({"rim_slope_match_center": [np.inf, 0.0, 0.0]}, "must be finite"),
    ({K: np.nan}, "rim_slope_match_strength must be finite"),
])
def test_parameter_refusals(change, text):
    gp = {k: v for k, v in dict(BASE, **change).items() if v is not None}
    with pytest.raises(L.MembraneHipError, match=text):
        lc.rim_match_params(_mesh(gp), None, gp)


def test_unknown_mode_and_oversized_ring():
    gp = dict(BASE, rim_slope_match_mode="nearest")
    with pytest.raises(ValueError, match="rim_slope_match_mode must be"):
        lc.rim_match_params(_mesh(gp), None, gp)
    P, T, _B = meshgen.disk_patch(38)  # 4447 vertices
    vo = {r: {"rim_slope_match_group": "rim"} for r in range(L.MS_RIM_MATCH_MAX_ROWS + 1)}
    vo[len(P) - 1] = {"rim_slope_match_group": "outer"}
    mesh = ArrayMesh(P, T, global_parameters=dict(BASE), vertex_options=vo)
    with pytest.raises(L.MembraneHipError, match="a rim ring of 4097 rows is above the 4096"):
        lc.rim_match_params(mesh, None, BASE)


def _minimizer(gp, mods, cons=(), tag=True):
    from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager
    from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager
    from membrane_solver_amd.runtime.minimizer import Minimizer
    from membrane_solver_amd.runtime.steppers import GradientDescent

    mesh = _mesh(gp, tag)
    mesh.energy_modules, mesh.constraint_modules = list(mods), list(cons)
    return Minimizer(mesh, mesh.global_parameters, GradientDescent(), EnergyModuleManager(list(mods)),
                     ConstraintModuleManager(list(cons)), quiet=True)


def test_minimizer_refusals_that_need_no_device():
    """The checks the Minimizer makes before anything is uploaded (its _rim_match_params), on the module bits alone."""
    out_bits = L.MS_MOD_TILT_OUT
    gp = dict(BASE, tilt_modulus_out=1.0, tilt_modulus_in=1.0)
    mz = _minimizer(gp, ["tilt_out", NAME])
    with pytest.raises(L.MembraneHipError, match="rim_slope_match_strength and without an active outer-leaflet"):
        mz._rim_match_params(L.MS_MOD_SURFACE)
    with pytest.raises(L.MembraneHipError, match="rim_slope_match_strength and without an active outer-leaflet"):
        mz._rim_match_params(L.MS_MOD_TILT_IN)  # (an inner-leaflet module alone does not relax the outer field)
    with pytest.raises(L.MembraneHipError, match="single-field tilt module"):
        mz._rim_match_params(out_bits | L.MS_MOD_TILT)
    with pytest.raises(L.MembraneHipError, match="a disk group, without an active inner-leaflet"):
        mz._rim_match_params(out_bits)
    prm = mz._rim_match_params(out_bits | L.MS_MOD_TILT_IN)
    assert len(prm["rim"]) == 18 and len(prm["outer"]) == 24 and len(prm["disk"]) == 12
    # without a disk group the inner leaflet is not needed
    mz2 = _minimizer({k: v for k, v in gp.items() if k != GD}, ["tilt_out", NAME])
    assert len(mz2._rim_match_params(out_bits)["disk"]) == 0
    # nobody tagged: the constant 0.0 -- but only behind the outer-leaflet check
    mz3 = _minimizer(gp, ["tilt_out", NAME], tag=False)
    assert mz3._rim_match_params(out_bits) is None
    with pytest.raises(L.MembraneHipError, match="rim_slope_match_strength"):
        mz3._rim_match_params(L.MS_MOD_SURFACE)


def test_listed_in_the_hot_path_text_and_in_the_module_bits():
    from membrane_solver_amd.runtime import minimizer as M

    assert M._ENERGY_BITS[NAME] == L.MS_MOD_RIM_SLOPE_MATCH_OUT == 1 << 26
    assert not M._ENERGY_BITS[NAME] & M._TILT_BITS  # (body_area_penalty next to the switched-off module stays accepted)
    with pytest.raises(L.MembraneHipError, match="tilt_thetaB_contact_in, rim_slope_match_out, "):
        _minimizer({}, ["line_tension"])  # (an edge module on a mesh without an edge table: the list text)


def test_strength_zero_is_a_host_constant():
    for gp in (dict(BASE, **{K: 0.0}), {k: v for k, v in BASE.items() if k != K},
               dict(BASE, **{K: 0.0, "rim_slope_match_mode": "shared_rim_staggered_v1"}),
               {k: v for k, v in BASE.items() if k != G}, {k: v for k, v in BASE.items() if k != GO}):
        assert lc.rim_match_params(_mesh(gp), None, gp) is None
        from membrane_solver_amd.modules.energy import rim_slope_match_out as module

        mesh = _mesh(gp)
        sentinel = np.arange(mesh.positions_view().size, dtype=float).reshape(-1, 3)
        g, gi, go = sentinel.copy(), sentinel.copy(), sentinel.copy()
        E = module.compute_energy_and_gradient_array(mesh, gp, None, positions=mesh.positions_view(), index_map={},
                                                     grad_arr=g, tilt_in_grad_arr=gi, tilt_out_grad_arr=go)
        assert E == 0.0 and all(np.array_equal(a, sentinel) for a in (g, gi, go))
        assert module.compute_energy_and_gradient(mesh, gp, None) == (0.0, {}, {}, {})


def test_sharded_drivers_refuse_the_module():
    """Every sharded entry refuses the bit with its own text: parallel.HipShardBackend.configure, ms_set_params and
    ms_set_rim_match on a sharded context (read in the library's source: a sharded context needs GPUs), and
    DeviceMesh.set_rim_match."""
    import os
    import re
    import types

    from membrane_solver_amd.device import DeviceMesh
    from membrane_solver_amd.parallel import HipShardBackend

    with pytest.raises(L.MembraneHipError, match="rim_slope_match_out module with a non-zero rim_slope_match_strength is not"):
        HipShardBackend.configure(types.SimpleNamespace(), modules=L.MS_MOD_SURFACE | L.MS_MOD_RIM_SLOPE_MATCH_OUT)
    with pytest.raises(L.MembraneHipError, match="the rim_slope_match_out module is not sharded"):
        DeviceMesh.set_rim_match(types.SimpleNamespace(shard_count=2), [1], [2])
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "membrane_solver_amd", "csrc")
    src = open(os.path.join(csrc, "ms_api_context.inc")).read()
    sp = src[src.index("int ms_set_params("):]
    assert re.search(r"MS_MOD_RIM_SLOPE_MATCH_OUT\) && c->shard_count != 1\)\s*return fail\(c, MS_ERR_STATE, "
                     r"\"the rim_slope_match_out module is not sharded", sp)
    assert re.search(r"MS_MOD_RIM_SLOPE_MATCH_OUT\) && \(p->modules & MS_TILT_MODS\)", sp)
    setter = open(os.path.join(csrc, "ms_api_rimmatch.inc")).read()
    setter = setter[setter.index("int ms_set_rim_match("):]
    assert re.search(r"if \(c->shard_count != 1\)\s*return fail\(c, MS_ERR_STATE, \"ms_set_rim_match: the "
                     r"rim_slope_match_out module is not sharded", setter)
