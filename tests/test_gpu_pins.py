"""pin_to_plane / pin_to_circle on the device: k_pin_enforce and the project lane's k_pin_grad against the
reference's outputs, and reference trajectories through Minimizer (Python loop and ms_minimize, multi-tile and
one-tile contexts)."""

import ast
import os

import numpy as np
import pytest

from membrane_solver_amd.geometry.mesh import ArrayMesh
from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager
from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager
from membrane_solver_amd.runtime.minimizer import Minimizer
from membrane_solver_amd.runtime.steppers import ConjugateGradient, GradientDescent

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
MODS = ["pin_to_plane", "pin_to_circle"]


def _case_mesh(z, name, energy):
    gp = dict(ast.literal_eval(str(z[name + "__gp"])), surface_tension=1.0)
    return ArrayMesh(z[name + "__positions0"], z["tri"], fixed=z[name + "__fixed"], global_parameters=gp,
                     vertex_options=ast.literal_eval(str(z[name + "__vopts"])), edges=z[name + "__edges"],
                     edge_options=ast.literal_eval(str(z[name + "__eopts"])), energy_modules=energy,
                     constraint_modules=MODS)


def _mz(mesh, cons, stepper=None, tile=0, step_size=1e-3):
    return Minimizer(mesh, mesh.global_parameters, stepper or GradientDescent(),
                     EnergyModuleManager(mesh.energy_modules), ConstraintModuleManager(cons),
                     energy_modules=mesh.energy_modules, constraint_modules=cons, quiet=True,
                     step_size=step_size, tile_vertices=tile)


@pytest.mark.parametrize("tile", [64, 256])
def test_enforce_pins_matches_reference(tile):
    z = np.load(os.path.join(GOLD, "pin_cases.npz"))
    for name in [str(n) for n in z["names"]]:
        mesh = _case_mesh(z, name, ["surface"])
        mz = _mz(mesh, MODS, tile=tile)
        _mir, dm = mz._device()
        dm.enforce_pins()
        np.testing.assert_allclose(dm.get_positions(), z[name + "__positions1"], rtol=0, atol=1e-12, err_msg=name)
        assert dm.pin_stats()["enforce_launches"] == 1


@pytest.mark.parametrize("tile", [64, 256])
def test_projected_gradient_matches_host(tile):
    z = np.load(os.path.join(GOLD, "pin_cases.npz"))
    for name in [str(n) for n in z["names"]]:
        mesh = _case_mesh(z, name, ["surface"])
        # the gradient the KKT solve sees: fixed rows NOT zeroed yet (minimizer.py:982-990 zeroes them after)
        _e, g_raw = _mz(mesh, [], tile=tile)._device()[1].energy_and_gradient(raw=True)
        mesh._hip_mirror = None
        mz = _mz(mesh, MODS, tile=tile)
        _e, g = mz.compute_energy_and_gradient_array()
        ref = g_raw.copy()
        ConstraintModuleManager(MODS).apply_gradient_modifications_array(ref, mesh, mesh.global_parameters)
        ref[np.asarray(mesh.fixed_mask)] = 0.0
        np.testing.assert_allclose(g, ref, rtol=0, atol=1e-12 * max(1.0, np.abs(ref).max()), err_msg=name)
        lane = mz.pin_tables.lane
        assert mz._device()[1].pin_stats()["lane"] == (1 if lane == "project" else 0)


def _traj_mesh(z):
    """The fixture's deck as an ArrayMesh: the reference's global parameters, tags, fixed mask and body."""
    from membrane_solver_amd.geometry.mesh import ArrayBody

    vo = ast.literal_eval(str(z["vopts_rows"] if "vopts_rows" in z else z["vopts"]))
    eo = ast.literal_eval(str(z["eopts_rows"] if "eopts_rows" in z else z["eopts"]))
    bodies = [ArrayBody(target_volume=float(z["target_volume"]))] if "target_volume" in z else None
    return ArrayMesh(z["positions0"], z["tri"], fixed=z["fixed"], global_parameters=ast.literal_eval(str(z["gp"])),
                     vertex_options=vo, edges=z["edge_rows"] if "edge_rows" in z else z["edges"], edge_options=eo,
                     bodies=bodies, energy_modules=[str(s) for s in z["energy_modules"]],
                     constraint_modules=[str(s) for s in z["constraint_modules"]])


TRAJ = ["traj_disk5_gd_pins_circle_fixed.npz",        # project lane, surface + bending
        "traj_disk5_cg_pins_slide_skip.npz",          # skip lane (plane + circle slide on one ring), CG
        "traj_ico8_gd_pins_volume_kkt.npz",           # pins + volume row in the KKT (projection off, drift check)
        "traj_ico8_gd_pins_volume_enforcer.npz",      # pins then the volume projection on every trial
        "traj_catenoid_gd_pins_fixed_rings.npz",      # reference decks: pinned rings that are also fixed
        "traj_good_min_cap_gd_pins_fixed_rings.npz"]


@pytest.mark.parametrize("fname", TRAJ)
@pytest.mark.parametrize("tile", [64, 256])
@pytest.mark.parametrize("in_library", [False, True])
def test_trajectory_matches_reference(fname, tile, in_library):
    z = np.load(os.path.join(GOLD, fname))
    mesh = _traj_mesh(z)
    stepper = ConjugateGradient() if str(z["stepper"]) == "ConjugateGradient" else GradientDescent()
    mz = _mz(mesh, list(mesh.constraint_modules), stepper, tile=tile, step_size=float(z["step_size0"]))
    n = int(z["n_steps"])
    ref = np.asarray(z["step_log"]).reshape(-1, 3)
    log = []
    if not in_library:
        orig = stepper.device_step

        def logged(dm, m, step_size, tol=0.0):
            r = orig(dm, m, step_size, tol=tol)
            if not r.converged:  # (the reference's stepper.step is not reached on convergence)
                log.append((float(bool(r.success)), float(r.next_step), float(r.energy)))
            return r

        stepper.device_step = logged
    res = mz.minimize(n)
    if in_library:
        got = np.asarray(mz.last_run["step_log"])[: len(ref), :3]
    else:
        got = np.array(log).reshape(-1, 3)
    assert got.shape == ref.shape
    np.testing.assert_array_equal(got[:, 0], ref[:, 0])
    np.testing.assert_array_equal(got[:, 1], ref[:, 1])
    if "good_min_cap" not in fname:
        # (good_min_cap: the reference's first volume projection after the pins reads Body's volume cached before
        # the pins moved the ring -- enforce_constraint does not bump the mesh version -- so its start state is one
        # projection behind; the device projects from the fresh volume.  Both end at the same finalized state.)
        np.testing.assert_allclose(got[:, 2], ref[:, 2], rtol=0, atol=1e-10)
    assert float(mz.step_size) == float(z["step_size_final"])
    assert abs(res["energy"] - float(z["E_final"])) <= 1e-10
    np.testing.assert_allclose(mesh.positions_view(), z["positions_final"], rtol=0, atol=1e-8)


@pytest.mark.parametrize("tile", [64, 256])
def test_volume_cases_enforce_and_gradient(tile):
    """k_pin_enforce, and k_pin_grad with the volume row (GC projected, <g,gC> / <gC,gC> corrected), against the
    reference's mixed KKT (tests/golden/pin_volume_cases.npz) applied to the device's raw gradient."""
    from membrane_solver_amd.geometry.mesh import ArrayBody
    from membrane_solver_amd.modules.constraints import pins
    from membrane_solver_amd.runtime.minimizer import _volume_gradient

    z = np.load(os.path.join(GOLD, "pin_volume_cases.npz"))
    for name in [str(n) for n in z["names"]]:
        def mk():
            return ArrayMesh(z[name + "__positions0"], z["tri"], fixed=z[name + "__fixed"],
                             global_parameters=dict(ast.literal_eval(str(z[name + "__gp"])), surface_tension=1.0),
                             vertex_options=ast.literal_eval(str(z[name + "__vopts"])), edges=z[name + "__edges"],
                             edge_options=ast.literal_eval(str(z[name + "__eopts"])), energy_modules=["surface"],
                             constraint_modules=MODS + ["volume"], bodies=[ArrayBody(target_volume=1.0)])
        mesh = mk()
        cons = MODS + ["volume"]
        _e, g_raw = _mz(mesh, [], tile=tile)._device()[1].energy_and_gradient(raw=True)
        mesh = mk()
        mz = _mz(mesh, cons, tile=tile)
        _e, g = mz.compute_energy_and_gradient_array()
        X = mesh.positions_view()
        ref = g_raw.copy()
        lane = pins.project_gradient(ref, [_volume_gradient(mesh, X)], pins.rows(X, pins.programs(mesh, MODS)))
        assert lane == mz.pin_tables.lane
        np.testing.assert_allclose(g, ref, rtol=0, atol=1e-12 * max(1.0, np.abs(ref).max()), err_msg=name)
        dm = mz._device()[1]
        dm.enforce_pins()
        np.testing.assert_allclose(dm.get_positions(), z[name + "__positions1"], rtol=0, atol=1e-12, err_msg=name)


def test_pinned_band_multitile_deterministic_and_not_resident(monkeypatch):
    """About 50 k facets, many tiles: k_pin_enforce and the projected gradient (volume row included) against the
    host path; two runs bitwise equal in MS_DETERMINISTIC=1; a pinned surface + volume-row GD run at the default
    settings takes the kernel-per-phase path (no resident steps)."""
    from membrane_solver_amd import meshgen
    from membrane_solver_amd.geometry.mesh import ArrayBody
    from membrane_solver_amd.modules.constraints import pins
    from membrane_solver_amd.runtime.minimizer import _volume_gradient

    monkeypatch.setenv("MS_DETERMINISTIC", "1")
    P, T = meshgen.icosphere(50)
    P = meshgen.smooth_displace(P, 0.03)
    band = np.flatnonzero(np.abs(P[:, 2]) < 0.01)
    assert len(T) > 45000 and len(band) > 50

    def mk():
        return ArrayMesh(P, T, global_parameters={"surface_tension": 1.0},
                         vertex_options={int(i): {"constraints": ["pin_to_plane"]} for i in band},
                         bodies=[ArrayBody(target_volume=4.1)], energy_modules=["surface"],
                         constraint_modules=["pin_to_plane", "volume"])

    def run():
        mesh = mk()
        _e, g_raw = _mz(mesh, [], tile=256)._device()[1].energy_and_gradient(raw=True)
        mesh = mk()
        mz = _mz(mesh, ["pin_to_plane", "volume"], tile=256, step_size=1e-3)
        _e, g = mz.compute_energy_and_gradient_array()
        X = mesh.positions_view().copy()
        ref = g_raw.copy()
        assert pins.project_gradient(ref, [_volume_gradient(mesh, X)],
                                     pins.rows(X, pins.programs(mesh, ["pin_to_plane"]))) == "project"
        np.testing.assert_allclose(g, ref, rtol=0, atol=1e-12 * max(1.0, np.abs(ref).max()))
        dm = mz._device()[1]
        dm.enforce_pins()
        host = X.copy()
        pins.enforce(host, pins.programs(mesh, ["pin_to_plane"]))
        np.testing.assert_allclose(dm.get_positions(), host, rtol=0, atol=1e-12)
        dm.set_positions(X)
        res = mz.minimize(5)
        return mesh.positions_view().copy(), res["energy"], dm.resident_stats()["steps"], mz.last_run["accepted"]

    a, b = run(), run()
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]
    assert a[2] == 0 and a[3] > 0
