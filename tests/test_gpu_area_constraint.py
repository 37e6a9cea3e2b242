"""body_area / global_area on the device against the reference (tests/golden/area_con_cases.npz, traj_*_areacon_*.npz):
the row and the area, the one- and two-row projection of the gradient, the enforcer, trajectories through Minimizer
(Python loop and ms_minimize), the summation modes, and the lanes that must not notice the feature."""

import ast
import os

import numpy as np
import pytest

from membrane_solver_amd import _lib as L
from membrane_solver_amd.device import DeviceMesh
from membrane_solver_amd.geometry.mesh import ArrayBody, ArrayMesh
from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager
from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager
from membrane_solver_amd.runtime.minimizer import Minimizer
from membrane_solver_amd.runtime.steppers import ConjugateGradient, GradientDescent

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
TRAJ = ["traj_ico4_gd_areacon_bending.npz",            # 1: bending, target 3 % below
        "traj_ico4_gd_areacon_fixed_rows.npz",         # 2: every 7th row fixed
        "traj_ico4_gd_areacon_surface_subset.npz",     # 3: surface tension, the body owns the upper facets
        "traj_ico4_gd_areacon_volume_rows.npz",        # 4: volume + area rows, the volume projection off
        "traj_ico4_cg_areacon_volume_rows.npz",
        "traj_ico4_gd_areacon_volume_enforcers.npz",   # 5: both enforcers on every trial
        "traj_ico4_cg_areacon_volume_enforcers.npz",
        "traj_ico4_gd_areacon_volume_subset.npz",      # 6: surface + bending, both rows, a subset body
        "traj_ico8_cg_areacon_bending.npz",            # 7: several tiles, CG, 4 of 8 accepted
        "traj_ico4_gd_areacon_global.npz"]             # 8: global_area
ONE_TILE = ["traj_ico4_gd_areacon_bending.npz", "traj_ico4_cg_areacon_volume_enforcers.npz",
            "traj_ico4_gd_areacon_volume_subset.npz", "traj_ico4_gd_areacon_global.npz"]


def _cases():
    return np.load(os.path.join(GOLD, "area_con_cases.npz"))


def _body(rows, nf, options, target_volume=None):
    return ArrayBody(facet_rows=None if len(rows) == nf else np.asarray(rows), target_volume=target_volume,
                     options=dict(options))


def _mz(mesh, stepper=None, tile=0, step_size=1e-3, deterministic=None):
    cons = list(mesh.constraint_modules)
    return Minimizer(mesh, mesh.global_parameters, stepper or GradientDescent(), EnergyModuleManager(mesh.energy_modules),
                     ConstraintModuleManager(cons), energy_modules=mesh.energy_modules, constraint_modules=cons, quiet=True,
                     step_size=step_size, tile_vertices=tile, deterministic=deterministic)


def _case_mesh(z, name):
    P, T = z[name + "__positions"], z[name + "__tri"]
    tv = float(z[name + "__target_volume"])
    return ArrayMesh(P, T, fixed=z[name + "__fixed"], global_parameters=ast.literal_eval(str(z[name + "__gp"])),
                     bodies=[_body(z[name + "__body_facets"], len(T), {"target_area": float(z[name + "__area"])},
                                   None if np.isnan(tv) else tv)],
                     energy_modules=[str(s) for s in z[name + "__energy_modules"]],
                     constraint_modules=[str(s) for s in z[name + "__constraint_modules"]])


@pytest.mark.parametrize("tile", [64, 256])
@pytest.mark.parametrize("fixed_order", [False, True])
def test_row_area_and_projected_gradient_match_reference(tile, fixed_order):
    """Through the C ABI (ms_area_row, ms_energy_and_gradient with MS_CON_BODY_AREA): area to 1e-12 relative, row to 1e-10
    of max|gA|, projected gradient of the one- and two-row cases to 1e-10 of max|g|, fixed rows exactly zero; the open
    disk and the degenerate facet (which contributes nothing) included."""
    z = _cases()
    for name in [str(n) for n in z["names"]]:
        mesh = _case_mesh(z, name)
        mz = _mz(mesh, tile=tile, deterministic=fixed_order)
        _E, g = mz.compute_energy_and_gradient_array()
        dm = mz._device()[1]
        assert dm.modules & L.MS_CON_BODY_AREA
        assert bool(dm.modules & L.MS_CON_VOLUME) == ("volume" in mesh.constraint_modules)
        row, A, n2 = dm.area_row()
        gA, A_ref, fixed = z[name + "__gA"], float(z[name + "__area"]), z[name + "__fixed"]
        scale = np.abs(z[name + "__g_before"]).max()
        print(f"{name} tile={tile} fixed_order={fixed_order}: dA/A={abs(A - A_ref) / A_ref:.3e} "
              f"drow={np.abs(row - gA).max() / np.abs(gA).max():.3e} dg={np.abs(g - z[name + '__g_after']).max() / scale:.3e}")
        assert abs(A - A_ref) <= 1e-12 * A_ref, name
        assert np.abs(row - gA).max() <= 1e-10 * np.abs(gA).max(), name
        assert abs(n2 - float(np.sum(gA * gA))) <= 1e-12 * n2, name
        assert np.abs(g - z[name + "__g_after"]).max() <= 1e-10 * scale, name
        assert not g[fixed].any(), name
        # the module's own entry point returns the same row
        from membrane_solver_amd.modules.constraints import body_area

        rows = body_area.constraint_gradients_array(mesh, mesh.global_parameters, positions=mesh.positions_view(),
                                                    index_map=mesh.vertex_index_to_row)
        assert len(rows) == 1 and np.abs(rows[0] - gA).max() <= 1e-10 * np.abs(gA).max()
        if name == "ico4_degenerate_area":
            # the merged pair's facets contribute nothing: the row equals the row of the body without them
            T = z[name + "__tri"]
            P = z[name + "__positions"]
            n = np.cross(P[T[:, 1]] - P[T[:, 0]], P[T[:, 2]] - P[T[:, 0]])
            good = np.linalg.norm(n, axis=1) >= 1e-12
            keep = np.array([f for f in z[name + "__body_facets"] if good[f]])
            assert len(keep) < len(z[name + "__body_facets"])
            dm2 = DeviceMesh(P, T, body_facets=np.isin(np.arange(len(T)), keep), tile_vertices=tile)
            dm2.set_area_constraint(L.MS_AREA_BODY, 1.0)
            row2, A2, _n = dm2.area_row()
            assert np.array_equal(row2, row) or np.abs(row2 - row).max() <= 1e-15
            assert abs(A2 - A) <= 1e-15 * A
            dm2.close()


@pytest.mark.parametrize("tile", [64, 256])
def test_enforcer_matches_reference(tile):
    """Same number of steps, |A - A0| < 1e-12 where the reference reaches it, positions to 1e-10, fixed rows bitwise
    unmoved: through ms_project_area and through the modules' enforce_constraint."""
    from membrane_solver_amd.modules.constraints import body_area, global_area

    z = _cases()
    for name in [str(n) for n in z["enforcer_names"]]:
        P, T, facets, fixed = z[name + "__positions"], z[name + "__tri"], z[name + "__body_facets"], z[name + "__fixed"]
        module, target, iters_ref = str(z[name + "__module"]), float(z[name + "__target"]), int(z[name + "__iters"])
        max_iter = 20 if module == "body_area" else 3
        dm = DeviceMesh(P, T, fixed=fixed, tile_vertices=tile,
                        body_facets=None if len(facets) == len(T) else np.isin(np.arange(len(T)), facets))
        dm.set_area_constraint(L.MS_AREA_BODY if module == "body_area" else L.MS_AREA_GLOBAL, target)
        iters, _A = dm.project_area(tol=1e-12, max_iter=max_iter)
        X = dm.get_positions()
        _row, A1, _n2 = dm.area_row()
        print(f"{name} tile={tile}: steps {iters} (reference {iters_ref}) |A-A0|={abs(A1 - target):.3e} "
              f"max|dx|={np.abs(X - z[name + '__positions_final']).max():.3e}")
        assert iters == iters_ref, name
        if abs(float(z[name + "__area_final"]) - target) < 1e-12:
            assert abs(A1 - target) < 1e-12, name
        np.testing.assert_allclose(X, z[name + "__positions_final"], rtol=0, atol=1e-10)
        assert np.array_equal(X[fixed], P[fixed]), name
        dm.close()
        # the Python module on a mesh: same result, written back
        gp = {"target_surface_area": target} if module == "global_area" else {}
        mesh = ArrayMesh(P, T, fixed=fixed, global_parameters=gp,
                         bodies=[_body(facets, len(T), {"target_area": target} if module == "body_area" else {})])
        (body_area if module == "body_area" else global_area).enforce_constraint(mesh)
        np.testing.assert_allclose(mesh.positions_view(), z[name + "__positions_final"], rtol=0, atol=1e-10)


def _traj_mesh(z):
    nf = len(z["tri"])
    tv = float(z["target_volume"]) if "target_volume" in z else None
    return ArrayMesh(z["positions0"], z["tri"], fixed=z["fixed"], global_parameters=ast.literal_eval(str(z["gp"])),
                     bodies=[_body(z["body_facets"], nf, ast.literal_eval(str(z["body_options"])), tv)],
                     energy_modules=[str(s) for s in z["energy_modules"]],
                     constraint_modules=[str(s) for s in z["constraint_modules"]])


def _run(fname, tile, in_library, reuse=2, deterministic=None):
    """-> (fixture, step log (n,3), final positions, final energy, final step size, device, minimizer)"""
    z = np.load(os.path.join(GOLD, fname))
    mesh = _traj_mesh(z)
    stepper = ConjugateGradient() if str(z["stepper"]) == "ConjugateGradient" else GradientDescent()
    stepper.reuse_energy0 = reuse
    mz = _mz(mesh, stepper, tile=tile, step_size=float(z["step_size0"]), deterministic=deterministic)
    log = []
    if not in_library:
        orig = stepper.device_step

        def logged(dm, m, step_size, tol=0.0):
            r = orig(dm, m, step_size, tol=tol)
            if not r.converged:  # (the reference's stepper.step is not reached on convergence)
                log.append((float(bool(r.success)), float(r.next_step), float(r.energy)))
            return r

        stepper.device_step = logged
    res = mz.minimize(int(z["n_steps"]))
    got = np.asarray(mz.last_run["step_log"])[:, :3] if in_library else np.array(log).reshape(-1, 3)
    return z, got, mesh.positions_view().copy(), res["energy"], float(mz.step_size), mz._device()[1], mz


def test_minimizer_takes_volume_and_body_area():
    """What the parent refused with "outside the HIP hot path"."""
    z = np.load(os.path.join(GOLD, "traj_ico4_gd_areacon_volume_rows.npz"))
    mz = _mz(_traj_mesh(z))
    assert mz.constraint_module_names == ["volume", "body_area"]
    res = mz.minimize(1)
    assert np.isfinite(res["energy"])


@pytest.mark.parametrize("fname", TRAJ)
@pytest.mark.parametrize("tile", [64, 256])
@pytest.mark.parametrize("in_library", [False, True])
def test_trajectory_matches_reference(fname, tile, in_library):
    """Accept / reject flags and step sizes identical (an accepted step's next step size is gamma times the alpha of the
    trial that was accepted, a failed search's is its last alpha times beta: equal step sizes are equal trial counts),
    accepted energies to 1e-10, final positions to 1e-8, the final area at the reference's (the bars of
    tests/test_gpu_area.py)."""
    z, got, X, E, step, dm, _m = _run(fname, tile, in_library)
    ref = np.asarray(z["step_log"]).reshape(-1, 3)
    got = got[: len(ref)]
    assert got.shape == ref.shape
    print(f"{fname} tile={tile} in_library={in_library}: max|dE|={np.abs(got[:, 2] - ref[:, 2]).max():.3e} "
          f"|dE_final|={abs(E - float(z['E_final'])):.3e} max|dx|={np.abs(X - z['positions_final']).max():.3e}")
    np.testing.assert_array_equal(got[:, 0], ref[:, 0])
    np.testing.assert_array_equal(got[:, 1], ref[:, 1])
    np.testing.assert_allclose(got[:, 2], ref[:, 2], rtol=0, atol=1e-10)
    assert step == float(z["step_size_final"])
    assert abs(E - float(z["E_final"])) <= 1e-10
    np.testing.assert_allclose(X, z["positions_final"], rtol=0, atol=1e-8)
    qs = dm.queue_stats()
    assert qs["rounds"] == 0 and qs["mismatches"] == 0, qs  # (every Armijo decision of the lane is the host's)
    st = dm.area_stats()
    assert st["row"] > 0 and st["fold"] > 0
    has_row = "body_area" in [str(s) for s in z["constraint_modules"]]
    assert (st["dots"] > 0) == has_row and (st["apply"] > 0) == has_row  # (global_area has no row)


def test_two_runs_are_bitwise_equal(deterministic):
    a = _run("traj_ico4_gd_areacon_volume_enforcers.npz", 256, True)
    b = _run("traj_ico4_gd_areacon_volume_enforcers.npz", 256, True)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3] and a[4] == b[4]
    a = _run("traj_ico8_cg_areacon_bending.npz", 64, False)
    b = _run("traj_ico8_cg_areacon_bending.npz", 64, False)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3] and a[4] == b[4]


@pytest.mark.parametrize("fname", ["traj_ico4_cg_areacon_volume_rows.npz", "traj_ico8_cg_areacon_bending.npz"])
def test_evaluation_reuse_levels_are_bitwise_identical(fname, deterministic):
    runs = [_run(fname, 256, True, reuse=r) for r in (0, 1, 2)]
    for r in runs[1:]:
        assert np.array_equal(r[1], runs[0][1]) and np.array_equal(r[2], runs[0][2])
        assert r[3] == runs[0][3] and r[4] == runs[0][4]


@pytest.mark.parametrize("fname", ONE_TILE)
@pytest.mark.parametrize("in_library", [False, True])
def test_one_workgroup_interpreter_is_bitwise_the_launch_per_kernel_path(fname, in_library, deterministic, monkeypatch):
    monkeypatch.setenv("MS_EXEC", "0")
    ref = _run(fname, 256, in_library)
    assert not ref[5].exec_stats()["active"]
    monkeypatch.setenv("MS_EXEC", "1")
    got = _run(fname, 256, in_library)
    assert got[5].exec_stats()["active"] and got[5].exec_stats()["packs"] > 0
    assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2])
    assert got[3] == ref[3] and got[4] == ref[4]


def test_tile_sizes_agree_in_default_mode():
    a = _run("traj_ico8_cg_areacon_bending.npz", 64, True)
    b = _run("traj_ico8_cg_areacon_bending.npz", 256, True)
    assert a[5].tile_stats()["n_tiles"] > b[5].tile_stats()["n_tiles"] > 1
    np.testing.assert_array_equal(a[1][:, :2], b[1][:, :2])
    np.testing.assert_allclose(a[1][:, 2], b[1][:, 2], rtol=0, atol=1e-11)
    np.testing.assert_allclose(a[2], b[2], rtol=0, atol=1e-11)


def test_existing_lanes_do_not_notice_the_feature():
    """With no area constraint set, a context that has seen area calls (set, row, projection on a copy of the positions,
    clear) behaves as one that never has: queue statistics, chosen kernel instances and a 6-step surface + bending CG
    trajectory on ico8."""
    from membrane_solver_amd import meshgen

    P, T = meshgen.icosphere(8)
    P = meshgen.smooth_displace(P, 0.05)
    gp = {"surface_tension": 1.0, "bending_modulus": 1.0, "spontaneous_curvature": 0.2}

    def run(touch):
        mesh = ArrayMesh(P, T, global_parameters=dict(gp), energy_modules=["surface", "bending"])
        mz = _mz(mesh, ConjugateGradient(), tile=64, deterministic=True)
        dm = mz._device()[1]
        if touch:
            dm.set_area_constraint(L.MS_AREA_GLOBAL, 12.0)
            dm.area_row()
            dm.project_area(max_iter=2)
            dm.set_positions(P)
            dm.set_area_constraint(L.MS_AREA_NONE)
            assert dm.area_stats()["row"] > 0
        res = mz.minimize(6)
        log = np.asarray(mz.last_run["step_log"])
        return log, mesh.positions_view().copy(), res["energy"], dm.queue_stats(), dm.energy_stats(), dm.area_stats()

    a, b = run(False), run(True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    assert a[3] == b[3] and a[4] == b[4]
    assert a[5] == {"row": 0, "dots": 0, "fold": 0, "apply": 0}
    assert a[3]["rounds"] > 0  # (the headline lane did queue rounds: the comparison means something)


def test_c_abi_refusals():
    from membrane_solver_amd import meshgen

    P, T = meshgen.icosphere(4)
    dm = DeviceMesh(P, T)
    dm.set_deterministic(True)  # (fixed-order sums: the gradients below are compared bit for bit)
    dm.set_surface_tension(np.ones(len(T)))
    for bad in (float("nan"), float("inf"), 0.0, -1.0):
        with pytest.raises(L.MembraneHipError, match="target area must be finite and positive"):
            dm.set_area_constraint(L.MS_AREA_BODY, bad)
    with pytest.raises(L.MembraneHipError, match="kind is MS_AREA_NONE, MS_AREA_BODY or MS_AREA_GLOBAL"):
        dm.set_area_constraint(7, 1.0)
    with pytest.raises(L.MembraneHipError, match="no area constraint"):
        dm.project_area()
    with pytest.raises(L.MembraneHipError, match="no area constraint"):
        dm.area_row()
    dm.set_params(modules=L.MS_MOD_SURFACE)
    with pytest.raises(L.MembraneHipError, match="enforce_area without an area constraint"):
        dm.step(stepper=L.MS_STEPPER_GD, step_size=1e-3, enforce_area=20)
    with pytest.raises(L.MembraneHipError, match="row together with body_area_penalty"):
        dm.set_params(modules=L.MS_MOD_SURFACE | L.MS_MOD_AREA_PENALTY | L.MS_CON_BODY_AREA)
    with pytest.raises(L.MembraneHipError, match="row together with a tilt-family module"):
        dm.set_params(modules=L.MS_MOD_SURFACE | L.MS_MOD_TILT | L.MS_CON_BODY_AREA)
    # the bit without a body_area target does nothing: the gradient is the plain one
    dm.set_params(modules=L.MS_MOD_SURFACE)
    _e, g0 = dm.energy_and_gradient(want_grad=True)
    dm.set_params(modules=L.MS_MOD_SURFACE | L.MS_CON_BODY_AREA)
    _e, g1 = dm.energy_and_gradient(want_grad=True)
    assert np.array_equal(g0, g1) and dm.area_stats()["dots"] == 0
    # with the target the whole-mesh row removes the surface gradient (it is gamma times the row)
    dm.set_area_constraint(L.MS_AREA_BODY, 12.0)
    _e, g2 = dm.energy_and_gradient(want_grad=True)
    assert np.abs(g2).max() <= 1e-12 * np.abs(g0).max() and dm.area_stats()["dots"] == 1
    dm.set_area_constraint(L.MS_AREA_NONE)
    _e, g3 = dm.energy_and_gradient(want_grad=True)
    assert np.array_equal(g0, g3)
    dm.close()
