"""tilt_splay_twist_in, host side (no GPU): parameter resolution as modules/energy/tilt_splay_twist_in.py:16-50 resolves
it and in its order, the plugin's interface against the reference module's (recorded as names in
splay_twist_cases.npz), the properties the fixtures are named for, a NumPy restatement of the term against every case's
reference outputs, the Minimizer's wiring, refusals and breakdown arithmetic, and the C ABI."""

import inspect
import json
import os
import re
import types

import numpy as np
import pytest

from membrane_solver_amd import _lib as L
from membrane_solver_amd import meshgen
from membrane_solver_amd.core.parameters import GlobalParameters, ParameterResolver
from membrane_solver_amd.geometry.mesh import ArrayMesh
from membrane_solver_amd.modules.energy import leaflet_common as lc
from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager
from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager
from membrane_solver_amd.runtime.minimizer import Minimizer
from membrane_solver_amd.runtime.steppers import GradientDescent

from conftest import load_golden
from minimizer_stub import install_stub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = load_golden("splay_twist_cases.npz")
NAMES = [str(n) for n in CASES["names"]]
TRAJ = ["traj_disk6_cg_splaytwist_coupled_gd.npz", "traj_disk6_gd_splaytwist_nested_cg.npz",
        "traj_ico4_gd_splaytwist_surface_backtrack.npz"]


def _params(gp):
    gp = GlobalParameters(gp)
    return lc.splay_twist_params(ParameterResolver(gp), gp)


def _device_params(gp):
    gp = GlobalParameters(gp)
    return lc.splay_twist_device_params(ParameterResolver(gp), gp)


def test_every_fixture_case_resolves_as_the_reference_did():
    for name in NAMES:
        gp = json.loads(str(CASES[name + "__gp"]))
        want = (float(CASES[name + "__k_splay"]), float(CASES[name + "__k_twist"]))
        assert _params(gp) == want + ("native",), name
        if str(CASES[name + "__what"]) == "off":
            assert want == (0.0, 0.0) and _device_params(gp) is None
        else:
            assert _device_params(gp) == want


def test_fallback_keys_and_explicit_zero():
    assert _params({"tilt_splay_modulus_in": 0.9, "bending_modulus_in": 5.0, "bending_modulus": 7.0})[:2] == (0.9, 0.0)
    assert _params({"bending_modulus_in": 0.6, "bending_modulus": 7.0})[:2] == (0.6, 0.0)
    assert _params({"bending_modulus": 0.45})[:2] == (0.45, 0.0)
    assert _params({})[:2] == (0.0, 0.0)
    # the fallback is taken on None only: an explicit 0.0 is 0
    assert _params({"tilt_splay_modulus_in": 0.0, "bending_modulus_in": 0.6, "bending_modulus": 7.0})[:2] == (0.0, 0.0)
    assert _params({"tilt_splay_modulus_in": None, "bending_modulus_in": 0.0, "bending_modulus": 7.0})[:2] == (0.0, 0.0)
    assert _params({"tilt_twist_modulus_in": 0.8, "tilt_twist_modulus": 3.0})[1] == 0.8
    assert _params({"tilt_twist_modulus": 0.3})[1] == 0.3
    assert _params({"tilt_twist_modulus_in": 0.0, "tilt_twist_modulus": 3.0})[1] == 0.0
    assert _params({"tilt_divergence_mode_in": " Vertex_Recovered ", "tilt_divergence_mode": "native"})[2] == "vertex_recovered"
    assert _params({"tilt_divergence_mode": "NATIVE"})[2] == "native"


@pytest.mark.parametrize("gp,text", [({"tilt_splay_modulus_in": -1.0}, "tilt_splay_modulus_in must be non-negative"),
                                     ({"bending_modulus": -0.5}, "tilt_splay_modulus_in must be non-negative"),
                                     ({"tilt_twist_modulus_in": -1.0}, "tilt_twist_modulus_in must be non-negative"),
                                     ({"tilt_twist_modulus": -2.0}, "tilt_twist_modulus_in must be non-negative"),
                                     ({"tilt_divergence_mode_in": "recovered"}, "tilt_divergence_mode_in must be"),
                                     ({"tilt_divergence_mode": "p1"}, "tilt_divergence_mode_in must be")])
def test_bad_parameters_raise_value_error(gp, text):
    with pytest.raises(ValueError, match=text):
        _params(gp)
    with pytest.raises(ValueError, match=text):
        _device_params(gp)


def test_everything_is_resolved_before_the_early_return():
    """tilt_splay_twist_in.py:128-135: a bad mode (or transport model) raises with both moduli 0 as well."""
    off = {"tilt_splay_modulus_in": 0.0}
    assert _device_params(off) is None
    with pytest.raises(ValueError, match="tilt_divergence_mode_in must be"):
        _device_params(dict(off, tilt_divergence_mode="bad"))
    with pytest.raises(L.MembraneHipError, match="tilt_transport_model other than ambient_v1"):
        _device_params(dict(off, tilt_transport_model="connection_v1"))
    with pytest.raises(L.MembraneHipError, match="tilt_transport_model other than ambient_v1"):
        _device_params({"tilt_splay_modulus_in": 1.0, "tilt_transport_model": "connection_v1"})
    # the splay modulus is looked at first, the twist modulus second, the mode third
    with pytest.raises(ValueError, match="tilt_splay_modulus_in"):
        _device_params({"tilt_splay_modulus_in": -1.0, "tilt_twist_modulus_in": -1.0, "tilt_divergence_mode": "bad"})
    with pytest.raises(ValueError, match="tilt_twist_modulus_in"):
        _device_params({"tilt_twist_modulus_in": -1.0, "tilt_divergence_mode": "bad"})
    # a valid mode the device does not carry: named, and only where the module would do something
    assert _device_params(dict(off, tilt_divergence_mode="vertex_recovered")) is None
    with pytest.raises(L.MembraneHipError, match="'vertex_recovered'"):
        _device_params({"tilt_splay_modulus_in": 1.0, "tilt_divergence_mode_in": "vertex_recovered"})


def test_plugin_has_the_reference_interface():
    mod = EnergyModuleManager(["tilt_splay_twist_in"]).get_module("tilt_splay_twist_in")
    assert mod.USES_TILT_LEAFLETS is True and bool(CASES["uses_tilt_leaflets"])
    ref = json.loads(str(CASES["signatures"]))
    assert sorted(ref) == sorted(mod.__all__) == ["compute_energy_and_gradient", "compute_energy_and_gradient_array",
                                                 "compute_energy_array"]
    for fn, params in ref.items():
        mine = [[p.name, str(p.kind), p.default is not inspect.Parameter.empty]
                for p in inspect.signature(getattr(mod, fn)).parameters.values()]
        assert mine == params, fn


def _case_arrays(n):
    g = CASES
    mesh, what = str(g[n + "__mesh"]), str(g[n + "__what"])
    pos = g[n + "__eval_positions"] if what == "moved" else g["mesh__" + mesh + "__positions"]
    return mesh, what, pos, g["mesh__" + mesh + "__tri"], g[n + "__tilts_in"]


def _areas(pos, tri):
    return 0.5 * np.linalg.norm(np.cross(pos[tri[:, 1]] - pos[tri[:, 0]], pos[tri[:, 2]] - pos[tri[:, 0]]), axis=1)


def test_fixture_has_the_named_properties():
    g = CASES
    whats = {n: str(g[n + "__what"]) for n in NAMES}
    assert {"", "moved", "off", "zero_area", "rotation", "rotation_zero", "mesh_tilts"} == set(whats.values())
    sizes = {m: len(g["mesh__" + m + "__positions"]) for m in ("disk4", "disk6", "ico4", "disk6z")}
    assert sizes == {"disk4": 61, "disk6": 127, "ico4": 162, "disk6z": 127}  # one tile of 64; two; three, closed
    for m in ("disk4", "disk6", "ico4", "disk6z"):
        assert np.ptp(g["mesh__" + m + "__positions"][:, 2]) > 0.1  # warped out of plane
    assert not g["mesh__flat6__positions"][:, 2].any() and len(g["mesh__flat6__positions"]) == 127
    gps = {n: json.loads(str(g[n + "__gp"])) for n in NAMES}
    splay_keys = ("tilt_splay_modulus_in", "bending_modulus_in", "bending_modulus")
    # splay only through each of the three keys: the first key present is the one that counts
    for k, key in enumerate(splay_keys):
        assert any(float(g[n + "__k_twist"]) == 0.0 and float(g[n + "__k_splay"]) == gp[key] > 0.0
                   and not any(q in gp for q in splay_keys[:k]) for n, gp in gps.items()), key
    # an explicit zero that does not fall back
    assert any(gp.get("tilt_splay_modulus_in") == 0.0 and gp.get("bending_modulus_in", 0.0) > 0.0
               and float(g[n + "__k_splay"]) == 0.0 and float(g[n + "__k_twist"]) > 0.0 for n, gp in gps.items())
    # twist only through each of its two keys
    assert any(float(g[n + "__k_splay"]) == 0.0 and float(g[n + "__k_twist"]) == gp.get("tilt_twist_modulus_in", -1.0) > 0.0
               for n, gp in gps.items())
    assert any(float(g[n + "__k_splay"]) == 0.0 and "tilt_twist_modulus_in" not in gp
               and float(g[n + "__k_twist"]) == gp.get("tilt_twist_modulus", -1.0) > 0.0 for n, gp in gps.items())
    for n in NAMES:
        mesh, what, pos, tri, tin = _case_arrays(n)
        E, tg, area = float(g[n + "__E"]), g[n + "__tilt_grad_in"], _areas(pos, tri)
        E_scale, row_scale = float(g[n + "__E_scale"]), g[n + "__row_scale"]
        assert row_scale.shape == (len(pos),) and tg.shape == pos.shape
        if what == "moved":
            assert not np.array_equal(pos, g["mesh__" + mesh + "__positions"])
        if what == "off":
            assert E == 0.0 and not tg.any() and E_scale == 0.0 and not row_scale.any()
        elif what == "rotation_zero":
            # div (omega z x r) = 0: energy and gradient are rounding noise; the scales are the uncancelled field's
            assert float(g[n + "__k_twist"]) == 0.0 and E_scale > 0.1 and abs(E) <= 1e-24 * E_scale
            assert np.max(np.abs(tg)) <= 1e-13 * row_scale.max()
        else:
            assert E > 0.0 and tg.any() and E_scale == pytest.approx(E, rel=1e-13)  # (the sum does not cancel)
        if what == "rotation":
            w = tin[:, 1] / pos[:, 0]  # t = omega z x r
            omega = float(np.median(w[np.abs(pos[:, 0]) > 0.1]))
            assert float(g[n + "__k_splay"]) == 0.0
            assert E == pytest.approx(0.5 * float(g[n + "__k_twist"]) * (2.0 * omega) ** 2 * area.sum(), rel=1e-12)
        if what == "zero_area":
            assert (area == 0.0).sum() == 1 and (area[area != 0.0] > 1e-6).all()  # one facet, exactly 0
        else:
            assert (area > 1e-6).all()
    tri = g["mesh__ico4__tri"]
    edges = np.sort(np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]]), axis=1)
    assert (np.unique(edges, axis=0, return_counts=True)[1] == 2).all()  # closed


def _numpy_term(pos, tri, t, k_splay, k_twist):
    """The issue's formulas, expression for expression."""
    v0, v1, v2 = pos[tri[:, 0]], pos[tri[:, 1]], pos[tri[:, 2]]
    n = np.cross(v1 - v0, v2 - v0)
    n2 = np.einsum("ij,ij->i", n, n)
    denom = np.maximum(n2, 1e-20)
    e = (v2 - v1, v0 - v2, v1 - v0)
    g = [np.cross(n, e[k]) / denom[:, None] for k in range(3)]
    area = 0.5 * np.sqrt(np.maximum(n2, 0.0))
    nn = np.sqrt(n2)
    n_hat = np.zeros_like(n)
    ok = nn > 1e-20
    n_hat[ok] = n[ok] / nn[ok, None]
    tk = [t[tri[:, k]] for k in range(3)]
    div = sum(np.einsum("ij,ij->i", tk[k], g[k]) for k in range(3))
    curl = sum(np.cross(g[k], tk[k]) for k in range(3))
    curl_n = np.einsum("ij,ij->i", curl, n_hat)
    E = 0.5 * np.sum(area * (k_splay * div ** 2 + k_twist * curl_n ** 2))
    grad = np.zeros_like(pos)
    for k in range(3):
        np.add.at(grad, tri[:, k], (area * k_splay * div)[:, None] * g[k]
                  + (area * k_twist * curl_n)[:, None] * np.cross(n_hat, g[k]))
    return float(E), grad


@pytest.mark.parametrize("name", NAMES)
def test_numpy_restatement_agrees_with_the_reference(name):
    g = CASES
    _mesh, what, pos, tri, tin = _case_arrays(name)
    E, grad = _numpy_term(pos, tri, tin, float(g[name + "__k_splay"]), float(g[name + "__k_twist"]))
    E_scale, row_scale = float(g[name + "__E_scale"]), g[name + "__row_scale"]
    assert abs(E - float(g[name + "__E"])) <= 1e-13 * E_scale
    assert np.all(np.max(np.abs(grad - g[name + "__tilt_grad_in"]), axis=1) <= 1e-13 * row_scale)
    if what == "off":
        assert E == 0.0 and not grad.any()


def test_relaxation_fixture_has_the_named_properties():
    g = load_golden("splay_twist_relax.npz")
    gp = json.loads(str(g["gp_json"]))
    assert [str(m) for m in g["modules"]] == ["tilt_in", "tilt_smoothness_in", "tilt_splay_twist_in"]
    assert _params(gp) == (0.7, 0.4, "native") and len(g["positions"]) == 127
    assert str(gp["tilt_solver"]) == "cg" and str(gp["tilt_cg_preconditioner"]) == "jacobi"
    n_it, n_g, n_e = int(g["n_iterations"]), int(g["n_gradient_evaluations"]), int(g["n_energy_evaluations"])
    # CG: one gradient evaluation more than line searches, and some search backtracked
    assert 0 < n_it <= int(gp["tilt_inner_steps"]) and n_g == n_it + 1 and n_e > n_it and int(g["n_evaluations"]) == n_g + n_e
    assert str(g["stop_reason"]) in ("converged", "completed_max_iters")
    fin = g["tilt_fixed_in"]
    assert 0 < fin.sum() < len(fin)
    assert np.max(np.abs(g["tilts_in_final"][fin] - g["tilts_in0"][fin])) <= 1e-15  # clamped rows stay
    assert np.max(np.abs(g["tilts_in_final"][~fin] - g["tilts_in0"][~fin])) > 1e-3
    assert 0.0 < float(g["E_splay_twist"]) < float(g["E_total"])


def test_trajectory_fixtures_have_the_named_properties():
    for fname in TRAJ:
        g = load_golden(fname)
        mods = [str(m) for m in g["modules"]]
        gp = json.loads(str(g["gp_json"]))
        assert "tilt_splay_twist_in" in mods and "surface" in mods and _device_params(gp) == (0.7, 0.4)
        log = g["step_log"]
        assert len(log) == int(g["n_steps"]) and (log[:, 0] > 0).sum() >= 3
        assert float(g["E_splay_twist_final"]) > 0.0
        for k in ("noise_energy", "noise_positions", "noise_tilts"):  # what a 1e-13 perturbation of the start does
            assert 0.0 < float(g[k]) < 1e-9, (fname, k, float(g[k]))
    g = load_golden("traj_disk6_gd_splaytwist_nested_cg.npz")  # the DEFINE lane
    gp = json.loads(str(g["gp_json"]))
    assert "tilt_smoothness_in" not in {str(m) for m in g["modules"]} and str(g["stepper"]) == "GradientDescent"
    assert (gp["tilt_solve_mode"], gp["tilt_solver"]) == ("nested", "cg") and len(g["positions0"]) == 127
    # (plain CG: the reference's leaflet Jacobi diagonal reads a stale curvature cache in this deck, see the generator)
    assert gp["tilt_cg_preconditioner"] == "none"
    g = load_golden("traj_disk6_cg_splaytwist_coupled_gd.npz")  # the ADD lane, next to tilt_out
    gp = json.loads(str(g["gp_json"]))
    assert {"tilt_smoothness_in", "tilt_out"} <= {str(m) for m in g["modules"]} and str(g["stepper"]) == "ConjugateGradient"
    assert (gp["tilt_solve_mode"], gp["tilt_solver"]) == ("coupled", "gd") and len(g["positions0"]) == 127
    g = load_golden("traj_ico4_gd_splaytwist_surface_backtrack.npz")
    log = g["step_log"]
    assert len(g["positions0"]) == 162
    given = np.concatenate([[float(g["step_size0"])], log[:-1, 1]])
    # an accepted step whose alpha lies below the step size it was given: the search backtracked, a trial was rejected
    assert np.any((log[:, 0] > 0) & (log[:, 1] < 1.5 * given * 0.999))


# -- Minimizer wiring -------------------------------------------------------------------------------------------------
P3, T3, _B3 = meshgen.disk_patch(3)
ON = {"tilt_splay_modulus_in": 0.7, "tilt_twist_modulus_in": 0.4}
BIT = 4194304


def _minimizer(gp, energy, constraints=()):
    mesh = ArrayMesh(P3, T3, global_parameters=dict(gp), energy_modules=energy)
    return Minimizer(mesh, mesh.global_parameters, GradientDescent(), EnergyModuleManager(energy),
                     ConstraintModuleManager(list(constraints)), energy_modules=energy,
                     constraint_modules=list(constraints), quiet=True)


def test_minimizer_knows_the_module():
    from membrane_solver_amd.runtime import minimizer as mzr

    assert mzr._ENERGY_BITS["tilt_splay_twist_in"] == L.MS_MOD_TILT_SPLAY_TWIST_IN == BIT
    assert mzr._ENERGY_SLOT["tilt_splay_twist_in"] is None and BIT & mzr._LEAFLET_BITS and BIT & mzr._TILT_BITS
    _minimizer(ON, ["tilt_in", "tilt_splay_twist_in"])  # accepted by the wiring
    # the refusal of an unknown module lists every module the path takes
    plugin = types.SimpleNamespace(compute_energy_and_gradient_array=None)  # (a module some plugin could load)
    mesh = ArrayMesh(P3, T3, global_parameters=dict(ON))
    with pytest.raises(L.MembraneHipError, match="energy module 'no_such_module' is outside the HIP hot path") as exc:
        Minimizer(mesh, mesh.global_parameters, GradientDescent(), types.SimpleNamespace(get_module=lambda name: plugin),
                  ConstraintModuleManager([]), energy_modules=["tilt_in", "no_such_module"], constraint_modules=[], quiet=True)
    listed = str(exc.value).split("(", 1)[1].rstrip(")").split(", ")
    assert listed == list(mzr._ENERGY_BITS) and "tilt_splay_twist_in" in listed and "gaussian_curvature" in listed


def _with_stub(monkeypatch, gp, energy, constraints=()):
    dm, mir = install_stub(monkeypatch)
    return _minimizer(gp, energy, constraints), dm, mir


def test_minimizer_sets_the_bit_and_uploads_the_moduli_once(monkeypatch):
    mz, dm, _mir = _with_stub(monkeypatch, dict(ON, tilt_modulus_in=1.0), ["tilt_in", "tilt_splay_twist_in"])
    mz._device()
    mz._device()
    assert [c[1] for c in dm.calls if c[0] == "set_tilt_splay_twist"] == [(0.7, 0.4)]
    assert dm.modules == L.MS_MOD_TILT_IN | BIT
    assert any(c[0] == "upload_leaflets" and sorted(c[1][0]) == ["in", "out"] for c in dm.calls)
    mz.global_params.update({"tilt_twist_modulus_in": 0.9})  # the key is the two moduli
    mz._device()
    assert [c[1] for c in dm.calls if c[0] == "set_tilt_splay_twist"] == [(0.7, 0.4), (0.7, 0.9)]


def test_module_alone_brings_the_leaflet_field_up(monkeypatch):
    mz, dm, _mir = _with_stub(monkeypatch, ON, ["surface", "tilt_splay_twist_in"])
    mz._device()
    assert dm.modules == L.MS_MOD_SURFACE | BIT
    assert any(c[0] == "upload_leaflets" for c in dm.calls) and any(c[0] == "set_tilt_splay_twist" for c in dm.calls)


def test_switched_off_module_leaves_its_bit_off(monkeypatch):
    mz, dm, _mir = _with_stub(monkeypatch, {"tilt_splay_modulus_in": 0.0, "bending_modulus": 3.0, "tilt_modulus_in": 1.0},
                              ["tilt_in", "tilt_splay_twist_in"])
    mz._device()
    assert dm.modules == L.MS_MOD_TILT_IN and not [c for c in dm.calls if c[0] == "set_tilt_splay_twist"]


@pytest.mark.parametrize("single,gp", [("tilt", {"tilt_rigidity": 1.0}), ("tilt_smoothness", {"tilt_smoothness_rigidity": 1.0}),
                                       ("bending_tilt", {"bending_modulus": 1.0})])
def test_minimizer_refuses_the_module_next_to_single_field_modules(monkeypatch, single, gp):
    mz, dm, _mir = _with_stub(monkeypatch, dict(ON, **gp), [single, "tilt_splay_twist_in"])
    with pytest.raises(L.MembraneHipError, match="tilt_splay_twist_in together with a single-field tilt module"):
        mz._device()
    assert not [c for c in dm.calls if c[0] in ("set_params", "set_tilt_splay_twist")]


@pytest.mark.parametrize("constraints,text", [(["pin_to_plane"], "tilt_splay_twist_in next to pin_to_plane / pin_to_circle"),
                                              (["pin_to_circle"], "tilt_splay_twist_in next to pin_to_plane / pin_to_circle"),
                                              (["volume"], "tilt_splay_twist_in next to the volume constraint's enforcer")])
def test_minimizer_refuses_pins_and_the_volume_enforcer_next_to_the_module(monkeypatch, constraints, text):
    mz, dm, _mir = _with_stub(monkeypatch, dict(ON, tilt_modulus_in=1.0), ["surface", "tilt_in", "tilt_splay_twist_in"],
                              constraints)
    with pytest.raises(L.MembraneHipError, match=text):
        mz._device()
    assert not [c for c in dm.calls if c[0] in ("set_params", "set_tilt_splay_twist")]


def test_minimizer_refuses_other_transport_and_divergence(monkeypatch):
    mz, _dm, _mir = _with_stub(monkeypatch, dict(ON, tilt_transport_model="connection_v1"), ["tilt_splay_twist_in"])
    with pytest.raises(L.MembraneHipError, match="tilt_transport_model other than ambient_v1"):
        mz._device()
    mz, _dm, _mir = _with_stub(monkeypatch, dict(ON, tilt_divergence_mode="vertex_recovered"), ["tilt_splay_twist_in"])
    with pytest.raises(L.MembraneHipError, match="'vertex_recovered'"):
        mz._device()
    mz, _dm, _mir = _with_stub(monkeypatch, dict(ON, tilt_splay_modulus_in=-1.0), ["tilt_splay_twist_in"])
    with pytest.raises(ValueError, match="non-negative"):
        mz._device()


def test_sharded_drivers_refuse_the_module():
    from membrane_solver_amd.parallel import HipShardBackend

    with pytest.raises(L.MembraneHipError, match="tilt_splay_twist_in module is not sharded"):
        HipShardBackend.configure(types.SimpleNamespace(), modules=L.MS_MOD_SURFACE | BIT)
    src = open(os.path.join(ROOT, "membrane_solver_amd", "csrc", "ms_api_context.inc")).read()
    sp = src[src.index("int ms_set_params("):]
    assert re.search(r"MS_MOD_TILT_SPLAY_TWIST_IN\) && c->shard_count != 1", sp), "ms_set_params must refuse it on a sharded context"
    assert re.search(r"MS_MOD_TILT_SPLAY_TWIST_IN\) && \(p->modules & MS_TILT_MODS\)", sp), "and next to a single-field module"
    assert "the tilt_splay_twist_in module is not sharded (single GPU only)" in sp


class _FakeDevice:
    """what compute_energy_breakdown reads of a DeviceMesh"""

    def __init__(self, modules, e3, scal, st):
        self.modules, self._e, self._sc, self._st = modules, np.array([1.0, 0.0, 0.0, e3]), scal, st

    def energy(self):
        return self._e

    def fetch_scalars(self):
        sc = np.zeros(L.MS_NSCAL)
        for k, v in self._sc.items():
            sc[k] = v
        return sc

    def tilt_splay_twist_energy(self):
        return self._st


def test_breakdown_arithmetic(monkeypatch):
    """The term's sums ride in the inner leaflet's smoothness slot: it reports its own energy, tilt_smoothness_in reports
    the slot without it, and a lone sharer of energies[3] reports that entry without it."""
    gp = dict(ON, tilt_modulus_in=1.0, bending_modulus_in=1.0)
    names = ["surface", "tilt_in", "tilt_smoothness_in", "tilt_splay_twist_in"]
    mz = _minimizer(gp, names)
    mz._const_energy = {}
    bits = L.MS_MOD_SURFACE | L.MS_MOD_TILT_IN | L.MS_MOD_TILT_SMOOTH_IN | BIT
    dev = _FakeDevice(bits, 0.25 + 0.5 + 0.125, {L.MS_S_ETILT_IN: 0.25, L.MS_S_ETS_IN: 0.5 + 0.125}, 0.125)
    monkeypatch.setattr(mz, "_device", lambda: (None, dev))
    assert mz.compute_energy_breakdown() == {"surface": 1.0, "tilt_in": 0.25, "tilt_smoothness_in": 0.5,
                                             "tilt_splay_twist_in": 0.125}
    # tilt_smoothness_in switched off (rigidity 0): the slot holds the term alone
    dev = _FakeDevice(bits & ~L.MS_MOD_TILT_SMOOTH_IN, 0.25 + 0.125, {L.MS_S_ETILT_IN: 0.25, L.MS_S_ETS_IN: 0.125}, 0.125)
    monkeypatch.setattr(mz, "_device", lambda: (None, dev))
    assert mz.compute_energy_breakdown() == {"surface": 1.0, "tilt_in": 0.25, "tilt_smoothness_in": 0.0,
                                             "tilt_splay_twist_in": 0.125}
    # one sharer of energies[3] next to the term
    mz2 = _minimizer(gp, ["surface", "tilt_in", "tilt_splay_twist_in"])
    mz2._const_energy = {}
    dev = _FakeDevice(L.MS_MOD_SURFACE | L.MS_MOD_TILT_IN | BIT, 0.25 + 0.125, {}, 0.125)
    monkeypatch.setattr(mz2, "_device", lambda: (None, dev))
    assert mz2.compute_energy_breakdown() == {"surface": 1.0, "tilt_in": 0.25, "tilt_splay_twist_in": 0.125}
    # the bit off: 0, and the getter is not asked
    dev = _FakeDevice(L.MS_MOD_SURFACE | L.MS_MOD_TILT_IN, 0.25, {}, None)
    dev.tilt_splay_twist_energy = lambda: pytest.fail("tilt_splay_twist_in is off: its energy is not read")
    monkeypatch.setattr(mz2, "_device", lambda: (None, dev))
    assert mz2.compute_energy_breakdown() == {"surface": 1.0, "tilt_in": 0.25, "tilt_splay_twist_in": 0.0}


def test_c_abi_declares_the_module():
    hdr = open(os.path.join(ROOT, "include", "membrane_hip.h")).read()
    m = re.search(r"#define MS_MOD_TILT_SPLAY_TWIST_IN (\d+)u", hdr)
    assert m and int(m.group(1)) == L.MS_MOD_TILT_SPLAY_TWIST_IN == BIT == 2 * L.MS_MOD_TILT_COUPLING  # the next free bit
    assert re.search(r"MS_NSCAL = 31\b", hdr)  # (no new reduction slot)
    bits = [int(v) for v in re.findall(r"#define MS_(?:MOD|CON|TRACK)_[A-Z_]+ (\d+)u", hdr)]
    assert len(bits) == len(set(bits)) and all(b & (b - 1) == 0 for b in bits)
    names = {"ms_set_tilt_splay_twist", "ms_get_tilt_splay_twist_energy", "ms_tilt_splay_twist_stats"}
    for n in names:
        assert re.search(r"\bint %s\(" % n, hdr) and hasattr(L.lib(), n)
    assert names <= set(L.SIGNATURES)


def test_one_list_says_what_lands_in_the_smoothness_slot():
    """TiltField::ets_mods() feeds every reader of the slot; the passes that cannot carry the term decline."""
    csrc = os.path.join(ROOT, "membrane_solver_amd", "csrc")
    ctx = open(os.path.join(csrc, "ms_api_ctx.inc")).read()
    # the list is the slot-writer table's: the smoothness module and the add-ons whose row names the field's slot
    import slot_writer_cases as sw

    assert re.search(r"uint32_t ets_mods\(\) const \{ return mod_smooth \| \(mod_addons & slot_writers\(s_ets, true\)\); \}", ctx)
    assert sw.row("MS_MOD_TILT_SPLAY_TWIST_IN") == {"bit": "MS_MOD_TILT_SPLAY_TWIST_IN", "slot": "MS_S_ETS_IN", "slot_disk": None,
                                                    "reads": {"RD_IN"}, "base": False, "shape_grad": False}
    assert sw.writers_in_front("MS_MOD_TILT_SPLAY_TWIST_IN", "MS_S_ETS_IN") == ["MS_MOD_TILT_SMOOTH_IN"]
    tilt = open(os.path.join(csrc, "ms_api_tilt.inc")).read()
    phases = open(os.path.join(csrc, "ms_api_phases.inc")).read()
    assert tilt.count("f.ets_mods()") >= 2 and phases.count("f.ets_mods()") >= 1
    assert not re.search(r"modules & f\.mod_smooth\) e(\[3\])? \+=", tilt + phases)  # no reader left on the old list
    sw.assert_lanes_decline_every_addon("MS_MOD_TILT_SPLAY_TWIST_IN")  # tsearch_plan among them
    m = re.search(r"constexpr uint32_t MS_TILT_SHAPE_MODS = ([^;]*);", phases)
    assert m and "MS_MOD_TILT_SPLAY_TWIST_IN" not in m.group(1)  # no shape gradient
