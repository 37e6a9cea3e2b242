"""tilt_coupling, host side (no GPU): parameter resolution as modules/energy/tilt_coupling.py:24-40 resolves it, the
plugin's interface against the reference module's (recorded as names in tilt_coupling_cases.npz), the properties the
fixtures are named for, the Minimizer's wiring, refusals and breakdown arithmetic, and the C ABI."""

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
CASES = load_golden("tilt_coupling_cases.npz")
NAMES = [str(n) for n in CASES["names"]]
TRAJ = ["traj_disk6_cg_coupling_coupled_gd.npz", "traj_disk6_gd_coupling_nested_cg.npz",
        "traj_ico4_gd_coupling_surface_backtrack.npz"]


def _params(gp):
    gp = GlobalParameters(gp)
    return lc.coupling_params(ParameterResolver(gp), gp)


@pytest.mark.parametrize("mode,sign", [("difference", -1), ("diff", -1), ("minus", -1), ("sub", -1), ("sum", 1),
                                       ("add", 1), ("plus", 1), ("  Difference ", -1), ("SUM", 1)])
def test_mode_aliases(mode, sign):
    assert _params({"tilt_coupling_modulus": 2.5, "tilt_coupling_mode": mode}) == (2.5, sign)


def test_misspelt_key_is_the_fallback_only():
    assert _params({"tilt_coupling_modulus": 1.0, "tilt_couping_mode": "sum"}) == (1.0, 1)
    # the right key wins, even when its value is unknown
    assert _params({"tilt_coupling_modulus": 1.0, "tilt_coupling_mode": "diff", "tilt_couping_mode": "sum"}) == (1.0, -1)
    assert _params({"tilt_coupling_modulus": 1.0, "tilt_coupling_mode": "product", "tilt_couping_mode": "sum"}) is None


@pytest.mark.parametrize("gp", [{"tilt_coupling_modulus": 2.0}, {"tilt_coupling_modulus": 2.0, "tilt_coupling_mode": "times"},
                                {"tilt_coupling_modulus": 0.0, "tilt_coupling_mode": "sum"}, {"tilt_coupling_mode": "sum"},
                                {"tilt_coupling_modulus": None, "tilt_coupling_mode": "difference"}, {}])
def test_nothing_to_do_gives_none(gp):
    assert _params(gp) is None


def test_every_fixture_case_resolves_as_the_reference_did():
    for name in NAMES:
        prm = _params(json.loads(str(CASES[name + "__gp"])))
        sign, k_c = int(CASES[name + "__sign"]), float(CASES[name + "__k_c"])
        if str(CASES[name + "__what"]) == "off":
            assert prm is None and (sign == 0 or k_c == 0.0)
        else:
            assert prm == (k_c, sign)


def test_plugin_has_the_reference_interface():
    mod = EnergyModuleManager(["tilt_coupling"]).get_module("tilt_coupling")
    assert mod.USES_TILT_LEAFLETS is True and bool(CASES["uses_tilt_leaflets"])
    ref = json.loads(str(CASES["signatures"]))
    assert sorted(ref) == sorted(mod.__all__) == ["compute_energy_and_gradient", "compute_energy_and_gradient_array",
                                                 "compute_energy_array"]
    for fn, params in ref.items():
        mine = [[p.name, str(p.kind), p.default is not inspect.Parameter.empty]
                for p in inspect.signature(getattr(mod, fn)).parameters.values()]
        assert mine == params, fn


def test_fixture_has_the_named_properties():
    g = CASES
    whats = {n: str(g[n + "__what"]) for n in NAMES}
    assert {"", "moved", "off", "cancel", "zero_area"} == set(whats.values())
    assert {-1, 1} <= {int(g[n + "__sign"]) for n in NAMES}
    gps = [json.loads(str(g[n + "__gp"])) for n in NAMES]
    assert any("tilt_couping_mode" in gp and "tilt_coupling_mode" not in gp for gp in gps)
    assert any(str(gp.get("tilt_coupling_mode", "")).strip().lower() in ("plus", "add") for gp in gps)
    assert any(str(gp.get("tilt_coupling_mode", "")).strip().lower() in ("sub", "minus", "diff") for gp in gps)
    sizes = {m: len(g["mesh__" + m + "__positions"]) for m in ("disk4", "disk6", "ico4", "disk6z")}
    assert sizes == {"disk4": 61, "disk6": 127, "ico4": 162, "disk6z": 127}  # one tile of 64; two; three, closed
    for n in NAMES:
        mesh = str(g[n + "__mesh"])
        pos = g[n + "__eval_positions"] if whats[n] == "moved" else g["mesh__" + mesh + "__positions"]
        tri, tin, tout = g["mesh__" + mesh + "__tri"], g[n + "__tilts_in"], g[n + "__tilts_out"]
        E, gr, tgo = float(g[n + "__E"]), g[n + "__grad"], g[n + "__tilt_grad_out"]
        nn = np.linalg.norm(np.cross(pos[tri[:, 1]] - pos[tri[:, 0]], pos[tri[:, 2]] - pos[tri[:, 0]]), axis=1)
        if whats[n] == "moved":
            assert not np.array_equal(pos, g["mesh__" + mesh + "__positions"])
        if whats[n] == "off":
            assert E == 0.0 and not gr.any() and not tgo.any() and float(g[n + "__E_scale"]) == 0.0
        elif whats[n] == "cancel":
            assert np.array_equal(tout, -int(g[n + "__sign"]) * tin)
            assert E == 0.0 and not gr.any() and not tgo.any()
            # (the scales are the uncancelled field's)
            assert float(g[n + "__E_scale"]) > 0 and float(g[n + "__grad_scale"]) > 0 and float(g[n + "__tilt_grad_scale"]) > 0
        else:
            assert E > 0.0 and float(g[n + "__E_scale"]) == pytest.approx(E, rel=1e-13)  # (the sum does not cancel)
            assert float(g[n + "__grad_scale"]) == np.max(np.abs(gr)) and float(g[n + "__tilt_grad_scale"]) == np.max(np.abs(tgo))
        if whats[n] == "zero_area":
            assert (nn == 0.0).sum() == 2 and (nn[nn != 0.0] >= 1e-12).all()  # exactly 0: both area rules agree
        else:
            assert (nn >= 1e-12).all()
    # closed mesh with irregular valence
    tri = g["mesh__ico4__tri"]
    val = np.bincount(tri.ravel())
    assert set(val.tolist()) == {5, 6}
    edges = np.sort(np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]]), axis=1)
    assert (np.unique(edges, axis=0, return_counts=True)[1] == 2).all()


def test_trajectory_fixtures_have_the_named_properties():
    for fname in TRAJ:
        g = load_golden(fname)
        mods = [str(m) for m in g["modules"]]
        gp = json.loads(str(g["gp_json"]))
        assert "tilt_coupling" in mods and _params(gp) is not None
        log = g["step_log"]
        assert len(log) == int(g["n_steps"]) and (log[:, 0] > 0).sum() >= 3
        assert float(g["E_coupling_final"]) > 0.0
    g = load_golden("traj_disk6_gd_coupling_nested_cg.npz")
    assert {"tilt_rim_source_in", "tilt_in", "tilt_out", "tilt_smoothness_in", "tilt_smoothness_out"} <= {str(m) for m in g["modules"]}
    assert _params(json.loads(str(g["gp_json"])))[1] == -1
    g = load_golden("traj_ico4_gd_coupling_surface_backtrack.npz")
    log = g["step_log"]
    given = np.concatenate([[float(g["step_size0"])], log[:-1, 1]])
    # an accepted step whose alpha lies below the step size it was given: a trial before it was rejected
    assert np.any((log[:, 0] > 0) & (log[:, 1] < 1.5 * given * 0.999))


def test_milestone_b_fixture_tracks():
    g = load_golden("tilt_coupling_milestone_b.npz")
    gp = json.loads(str(g["gp_json"]))
    assert _params(gp) == (10.0, -1) and int(gp["tilt_inner_steps"]) == 1000
    assert not g["positions"][:, 2].any()  # flat
    # CG that ends on the tolerance: one gradient evaluation more than line searches, at least one trial per search
    n_it, n_g, n_e = int(g["n_iterations"]), int(g["n_gradient_evaluations"]), int(g["n_energy_evaluations"])
    assert 0 < n_it < 1000 and n_g == n_it + 1 and n_e >= n_it and int(g["n_evaluations"]) == n_g + n_e
    assert [str(m) for m in g["modules"]] == ["tilt_smoothness_in", "tilt_in", "tilt_coupling"]
    tin, tout = g["tilts_in_final"], g["tilts_out_final"]
    assert not g["tilts_out0"].any()
    assert np.mean(np.linalg.norm(tin - tout, axis=1)) < 0.1 and np.max(np.linalg.norm(tout, axis=1)) > 0.9
    ring = g["tilt_fixed_in"]
    assert ring.sum() == 24 and np.array_equal(tin[ring], g["tilts_in0"][ring])  # the hard source stays what it was


# -- Minimizer wiring -------------------------------------------------------------------------------------------------
P4, T4, _B4 = meshgen.disk_patch(3)
ON = {"tilt_coupling_modulus": 2.0, "tilt_coupling_mode": "difference"}


def _minimizer(gp, energy):
    mesh = ArrayMesh(P4, T4, global_parameters=dict(gp), energy_modules=energy)
    return Minimizer(mesh, mesh.global_parameters, GradientDescent(), EnergyModuleManager(energy),
                     ConstraintModuleManager([]), energy_modules=energy, constraint_modules=[], quiet=True)


def test_minimizer_knows_the_module():
    from membrane_solver_amd.runtime import minimizer as mzr

    assert mzr._ENERGY_BITS["tilt_coupling"] == L.MS_MOD_TILT_COUPLING == 2097152
    assert mzr._ENERGY_SLOT["tilt_coupling"] is None and L.MS_MOD_TILT_COUPLING & mzr._LEAFLET_BITS
    _minimizer(ON, ["tilt_in", "tilt_out", "tilt_coupling"])  # accepted by the wiring


def _with_stub(monkeypatch, gp, energy):
    dm, mir = install_stub(monkeypatch)
    return _minimizer(gp, energy), dm, mir


@pytest.mark.parametrize("single,gp", [("tilt", {"tilt_rigidity": 1.0}), ("tilt_smoothness", {"tilt_smoothness_rigidity": 1.0}),
                                       ("bending_tilt", {"bending_modulus": 1.0})])
def test_minimizer_refuses_the_module_next_to_single_field_modules(monkeypatch, single, gp):
    mz, dm, _mir = _with_stub(monkeypatch, dict(ON, **gp), [single, "tilt_coupling"])
    with pytest.raises(L.MembraneHipError, match="single-field and leaflet tilt modules together"):
        mz._device()
    assert not [c for c in dm.calls if c[0] in ("set_params", "set_tilt_coupling")]


def test_minimizer_uploads_modulus_and_sign_once(monkeypatch):
    mz, dm, mir = _with_stub(monkeypatch, dict(ON, tilt_modulus_in=1.0), ["tilt_in", "tilt_coupling"])
    mz._device()
    mz._device()
    assert [c[1] for c in dm.calls if c[0] == "set_tilt_coupling"] == [(2.0, -1)]
    assert dm.modules == L.MS_MOD_TILT_IN | L.MS_MOD_TILT_COUPLING
    assert any(c[0] == "upload_leaflets" and sorted(c[1][0]) == ["in", "out"] for c in dm.calls)  # both fields go up
    mz.global_params.update({"tilt_coupling_mode": "sum"})  # the key is (modulus, sign)
    mz._device()
    assert [c[1] for c in dm.calls if c[0] == "set_tilt_coupling"] == [(2.0, -1), (2.0, 1)]


def test_switched_off_module_leaves_its_bit_off(monkeypatch):
    mz, dm, _mir = _with_stub(monkeypatch, {"tilt_coupling_modulus": 2.0, "tilt_coupling_mode": "times", "tilt_modulus_in": 1.0},
                              ["tilt_in", "tilt_coupling"])
    mz._device()
    assert dm.modules == L.MS_MOD_TILT_IN and not [c for c in dm.calls if c[0] == "set_tilt_coupling"]


def test_sharded_driver_refuses_the_module():
    from membrane_solver_amd.parallel import HipShardBackend

    with pytest.raises(L.MembraneHipError, match="tilt_coupling module is not sharded"):
        HipShardBackend.configure(types.SimpleNamespace(), modules=L.MS_MOD_SURFACE | L.MS_MOD_TILT_COUPLING)
    src = open(os.path.join(ROOT, "membrane_solver_amd", "csrc", "ms_api_context.inc")).read()
    sp = src[src.index("int ms_set_params("):]
    assert re.search(r"MS_MOD_TILT_COUPLING\) && c->shard_count != 1", sp), "ms_set_params must refuse it on a sharded context"
    assert re.search(r"MS_MOD_TILT_COUPLING\) && \(p->modules & MS_TILT_MODS\)", sp), "and next to a single-field module"


class _FakeDevice:
    """what compute_energy_breakdown reads of a DeviceMesh"""

    def __init__(self, modules, e3, scal, cpl, rim_in=0.0):
        self.modules, self._e, self._sc, self._cpl, self._rim = modules, np.array([1.0, 0.0, 0.0, e3]), scal, cpl, rim_in

    def energy(self):
        return self._e

    def fetch_scalars(self):
        sc = np.zeros(L.MS_NSCAL)
        for k, v in self._sc.items():
            sc[k] = v
        return sc

    def tilt_coupling_energy(self):
        return self._cpl

    def leaflet_rim_source_energy(self, lf):
        return self._rim if lf == "in" else 0.0


def test_breakdown_arithmetic(monkeypatch):
    """The coupling's sums ride in the outer leaflet's tilt-magnitude slot: it reports its own energy, tilt_out reports the
    slot without it, and a lone sharer of energies[3] reports that entry without it."""
    gp = dict(ON, tilt_modulus_in=1.0, tilt_modulus_out=1.0)
    mz = _minimizer(gp, ["surface", "tilt_in", "tilt_out", "tilt_coupling"])
    mz._const_energy = {}
    bits = L.MS_MOD_SURFACE | L.MS_MOD_TILT_IN | L.MS_MOD_TILT_OUT | L.MS_MOD_TILT_COUPLING
    dev = _FakeDevice(bits, 0.25 + 0.5 + 0.125, {L.MS_S_ETILT_IN: 0.25, L.MS_S_ETILT_OUT: 0.5 + 0.125}, 0.125)
    monkeypatch.setattr(mz, "_device", lambda: (None, dev))
    assert mz.compute_energy_breakdown() == {"surface": 1.0, "tilt_in": 0.25, "tilt_out": 0.5, "tilt_coupling": 0.125}
    # tilt_out switched off (modulus 0): the slot holds the coupling alone
    dev = _FakeDevice(bits & ~L.MS_MOD_TILT_OUT, 0.25 + 0.125, {L.MS_S_ETILT_IN: 0.25, L.MS_S_ETILT_OUT: 0.125}, 0.125)
    monkeypatch.setattr(mz, "_device", lambda: (None, dev))
    assert mz.compute_energy_breakdown() == {"surface": 1.0, "tilt_in": 0.25, "tilt_out": 0.0, "tilt_coupling": 0.125}
    # one sharer of energies[3] next to the coupling
    mz2 = _minimizer(gp, ["surface", "tilt_in", "tilt_coupling"])
    mz2._const_energy = {}
    dev = _FakeDevice(L.MS_MOD_SURFACE | L.MS_MOD_TILT_IN | L.MS_MOD_TILT_COUPLING, 0.25 + 0.125, {}, 0.125)
    monkeypatch.setattr(mz2, "_device", lambda: (None, dev))
    assert mz2.compute_energy_breakdown() == {"surface": 1.0, "tilt_in": 0.25, "tilt_coupling": 0.125}
    # the bit off: 0, and the getter is not asked
    dev = _FakeDevice(L.MS_MOD_SURFACE | L.MS_MOD_TILT_IN, 0.25, {}, None)
    dev.tilt_coupling_energy = lambda: pytest.fail("tilt_coupling is off: its energy is not read")
    monkeypatch.setattr(mz2, "_device", lambda: (None, dev))
    assert mz2.compute_energy_breakdown() == {"surface": 1.0, "tilt_in": 0.25, "tilt_coupling": 0.0}


def test_c_abi_declares_the_module():
    hdr = open(os.path.join(ROOT, "include", "membrane_hip.h")).read()
    assert re.search(r"#define MS_MOD_TILT_COUPLING 2097152u", hdr)
    assert L.MS_MOD_TILT_COUPLING == 2 * L.MS_MOD_TILT_RIM_SOURCE_OUT  # the next free bit
    assert re.search(r"MS_NSCAL = 31\b", hdr)  # (no new reduction slot)
    bits = [int(v) for v in re.findall(r"#define MS_(?:MOD|CON|TRACK)_[A-Z_]+ (\d+)u", hdr)]
    assert len(bits) == len(set(bits)) and all(b & (b - 1) == 0 for b in bits)
    names = {"ms_set_tilt_coupling", "ms_get_tilt_coupling_energy", "ms_tilt_coupling_stats"}
    for n in names:
        assert re.search(r"\bint %s\(" % n, hdr) and hasattr(L.lib(), n)
    assert names <= set(L.SIGNATURES)
