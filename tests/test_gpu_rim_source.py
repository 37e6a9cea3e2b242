"""tilt_rim_source_in / tilt_rim_source_out on the HIP path (csrc/ms_rim.hip): the plugins against the reference's
module on every case of rim_source_cases.npz, the milestone-C leaflet relaxation, and three reference trajectories
(tools/gen_golden_rim_source.py).  Tolerances are the leaflet tests': |E - E_ref| <= 1e-12 E_scale with
E_scale = sum |gamma L dots| (the energy is a signed sum that may cancel), relerr(tilt gradient) < 1e-10."""

import json

import numpy as np
import pytest

from conftest import load_golden, relerr

pytestmark = pytest.mark.gpu

CASES = load_golden("rim_source_cases.npz")
NAMES = [str(n) for n in CASES["names"]]
TRAJ = {"traj_disk6_gd_rimsource_nested_cg.npz": "gd", "traj_disk6_cg_rimsource_coupled_gd.npz": "cg",
        "traj_disk5_gd_rimsource_follow_fastpath.npz": "gd"}


def _opts(text):
    return {int(k): v for k, v in json.loads(str(text)).items()}


def _case_mesh(name, tile=0):
    from membrane_solver_amd.core.parameters import GlobalParameters
    from membrane_solver_amd.geometry.mesh import ArrayMesh, mirror_for

    g = CASES
    gp = GlobalParameters(json.loads(str(g[name + "__gp"])))
    mesh = ArrayMesh(g[name + "__positions"], g[name + "__tri"], global_parameters=gp, tilts_in=g[name + "__tilts_in"],
                     tilts_out=g[name + "__tilts_out"], edges=g[name + "__edges"], vertex_options=_opts(g[name + "__vopts"]),
                     edge_options=_opts(g[name + "__eopts"]))
    if tile:
        mirror_for(mesh, tile_vertices=tile)  # (stashed on the mesh: the plugins evaluate on this mirror)
    return mesh, gp


def _check_case(name, tile):
    from membrane_solver_amd.core.parameters import ParameterResolver
    from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager

    g = CASES
    lf = str(g[name + "__leaflet"])
    mesh, gp = _case_mesh(name, tile)
    res = ParameterResolver(gp)
    module = EnergyModuleManager([f"tilt_rim_source_{lf}"]).get_module(f"tilt_rim_source_{lf}")
    assert module.USES_TILT_LEAFLETS
    pos, tin, tout = g[name + "__eval_positions"], g[name + "__tilts_in"], g[name + "__tilts_out"]
    E_ref, tg_ref, scale = float(g[name + "__E"]), g[name + "__tilt_grad"], float(g[name + "__E_scale"])
    sentinel = np.arange(pos.size, dtype=np.float64).reshape(pos.shape)
    grad = sentinel.copy()
    tg = np.zeros_like(pos)
    kw = {"tilt_in_grad_arr": tg} if lf == "in" else {"tilt_out_grad_arr": tg}
    E = module.compute_energy_and_gradient_array(mesh, gp, res, positions=pos, index_map=mesh.vertex_index_to_row,
                                                 grad_arr=grad, tilts_in=tin, tilts_out=tout, **kw)
    E2 = module.compute_energy_array(mesh, gp, res, positions=pos, index_map=mesh.vertex_index_to_row, tilts_in=tin,
                                     tilts_out=tout)
    print(name, "E", E, "ref", E_ref, "|dE|/scale", abs(E - E_ref) / max(scale, 1e-300), "relerr tg", relerr(tg, tg_ref))
    assert np.array_equal(grad, sentinel), "the module has no shape gradient: grad_arr must stay as it is"
    assert abs(E - E_ref) <= 1e-12 * scale
    assert abs(E2 - E_ref) <= 1e-12 * scale
    if tg_ref.any():
        assert relerr(tg, tg_ref) < 1e-10
        assert np.array_equal(np.any(tg != 0.0, axis=1), np.any(tg_ref != 0.0, axis=1))
    else:
        assert not tg.any()
    if tile and len(pos) > tile:  # (disk4 has 61 vertices: one tile of 64; disk6's 127 make two)
        assert mesh._hip_mirror.dm.tile_stats()["n_tiles"] > 1
    if np.array_equal(pos, g[name + "__positions"]):  # the dict API evaluates the mesh's own positions and tilts
        Ed, gd, tgd = module.compute_energy_and_gradient(mesh, gp, res)
        assert abs(Ed - E_ref) <= 1e-12 * scale and gd == {}
        assert sorted(tgd) == [int(r) for r in np.flatnonzero(np.any(tg_ref != 0.0, axis=1))]
        for r, row in tgd.items():
            assert np.max(np.abs(row - tg_ref[r])) <= 1e-10 * np.max(np.abs(tg_ref))
        assert module.compute_energy_and_gradient(mesh, gp, res, compute_gradient=False) == (Ed, {})


@pytest.mark.parametrize("name", NAMES)
def test_rim_source_plugins_match_reference(name):
    _check_case(name, tile=0)


@pytest.mark.parametrize("name", NAMES)
def test_rim_source_plugins_with_small_tiles(name):
    """64-vertex tiles: several tiles, the rim ring crossing tile boundaries, the row permutation."""
    _check_case(name, tile=64)


@pytest.mark.parametrize("name", ["disk6_b_ring3_all_per_edge", "disk6_g_out_leaflet"])
@pytest.mark.parametrize("tile", [0, 64])
def test_leaflet_evaluation_differs_by_the_rim_source(name, tile):
    """leaflet_tilt_energy_and_gradient() with and without the module differs by exactly the module's contribution,
    next to tilt_in/out (the sums are ADDED behind the magnitude pass) and without them (the slot is DEFINED)."""
    from membrane_solver_amd import _lib as L
    from membrane_solver_amd.core.parameters import ParameterResolver
    from membrane_solver_amd.device import DeviceMesh
    from membrane_solver_amd.modules.energy import leaflet_common as lc

    g = CASES
    lf = str(g[name + "__leaflet"])
    mesh, gp = _case_mesh(name)
    prm = lc.rim_source_params(mesh, ParameterResolver(gp), gp, lf)
    dm = DeviceMesh(g[name + "__positions"], g[name + "__tri"], tile_vertices=tile)
    dm.set_leaflet_tilts("in", g[name + "__tilts_in"], tilt_modulus=1.3, smoothness=0.7)
    dm.set_leaflet_tilts("out", g[name + "__tilts_out"], tilt_modulus=0.9, smoothness=0.4)
    dm.set_leaflet_rim_source(lf, **prm)
    bit = L.MS_MOD_TILT_RIM_SOURCE_IN if lf == "in" else L.MS_MOD_TILT_RIM_SOURCE_OUT
    scale, tg_ref, E_ref = float(g[name + "__E_scale"]), g[name + "__tilt_grad"], float(g[name + "__E"])
    for base in (L.MS_MOD_TILT_IN | L.MS_MOD_TILT_OUT | L.MS_MOD_TILT_SMOOTH_IN | L.MS_MOD_TILT_SMOOTH_OUT,
                 L.MS_MOD_TILT_SMOOTH_IN | L.MS_MOD_TILT_SMOOTH_OUT):
        dm.set_params(modules=base)
        E0, gi0, go0 = dm.leaflet_tilt_energy_and_gradient()
        e0 = dm.energy()
        dm.set_params(modules=base | bit)
        E1, gi1, go1 = dm.leaflet_tilt_energy_and_gradient()
        e1 = dm.energy()
        own = dm.leaflet_rim_source_energy(lf)
        tol = 1e-12 * (scale + abs(E0))
        assert abs((E1 - E0) - E_ref) <= tol and abs((e1[3] - e0[3]) - E_ref) <= tol
        assert abs(own - E_ref) <= 1e-12 * scale
        d_in, d_out = gi1 - gi0, go1 - go0
        mine, other = (d_in, d_out) if lf == "in" else (d_out, d_in)
        assert np.max(np.abs(mine - tg_ref)) <= 1e-10 * np.max(np.abs(tg_ref)) + 1e-15 * np.max(np.abs(gi0))
        assert not other.any()
        assert np.array_equal(e1[:3], e0[:3])
    dm.close()


# ---------------------------------------------------------------------------------------------------------------------
def _minimizer(g, kind, observe, tile=0, deterministic=None):
    from membrane_solver_amd.geometry.mesh import ArrayMesh
    from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager
    from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager
    from membrane_solver_amd.runtime.minimizer import Minimizer
    from membrane_solver_amd.runtime.steppers import ConjugateGradient, GradientDescent

    mods = [str(m) for m in g["modules"]]
    mesh = ArrayMesh(g["positions0"], g["tri"], fixed=g["fixed"], surface_tension=g["gamma"], tilts_in=g["tilts_in0"],
                     tilts_out=g["tilts_out0"], tilt_fixed_in=g["tilt_fixed_in"], tilt_fixed_out=g["tilt_fixed_out"],
                     global_parameters=json.loads(str(g["gp_json"])), energy_modules=mods, constraint_modules=[],
                     edges=g["edges"], vertex_options=_opts(g["vopts"]))
    stepper = GradientDescent() if kind == "gd" else ConjugateGradient()
    log = []
    if observe:
        orig = stepper.device_step

        def logged(dm, m, step_size, tol=0.0):
            r = orig(dm, m, step_size, tol=tol)
            log.append((float(r.success), r.next_step, r.energy))
            return r

        stepper.device_step = logged
    mz = Minimizer(mesh, mesh.global_parameters, stepper, EnergyModuleManager(mods), ConstraintModuleManager([]),
                   quiet=True, step_size=float(g["step_size0"]), tile_vertices=tile, deterministic=deterministic)
    return mesh, mz, log


def _check_finals(mesh, res, g):
    assert relerr(mesh.positions_view(), g["positions_final"]) < 1e-8
    assert relerr(mesh.tilts_in_view(), g["tilts_in_final"]) < 1e-8
    assert relerr(mesh.tilts_out_view(), g["tilts_out_final"]) < 1e-8
    assert abs(res["energy"] - g["E_final"]) <= 1e-9 * abs(g["E_final"])


@pytest.mark.parametrize("fname", sorted(TRAJ))
def test_minimizer_reproduces_rim_source_trajectory(fname):
    """The assertions of test_minimizer_reproduces_disk_target_trajectory (tests/test_gpu_leaflet.py)."""
    g = load_golden(fname)
    for observe in (True, False):
        mesh, mz, log = _minimizer(g, TRAJ[fname], observe=observe)
        if observe:
            E0, grad0 = mz.compute_energy_and_gradient_array()
            assert abs(E0 - g["E0"]) <= 1e-12 * abs(g["E0"])
            assert relerr(grad0, g["grad0"]) < 1e-10
        res = mz.minimize(int(g["n_steps"]))
        if observe:
            got, ref = np.array(log), g["step_log"]
            print(fname, "got", got.tolist(), "ref", ref.tolist())
            assert got.shape == ref.shape
            assert np.array_equal(got[:, 0], ref[:, 0]), "accept/reject sequence differs from the reference"
            assert np.allclose(got[:, 1], ref[:, 1], rtol=1e-12, atol=0)
            assert np.allclose(got[:, 2], ref[:, 2], rtol=1e-9, atol=0)
            bd = mz.compute_energy_breakdown()
            assert abs(sum(bd.values()) - res["energy"]) <= 1e-12 * abs(res["energy"])
            assert bd["tilt_rim_source_in"] != 0.0
        _check_finals(mesh, res, g)


def test_rim_source_trajectory_with_small_tiles():
    g = load_golden("traj_disk6_cg_rimsource_coupled_gd.npz")
    mesh, mz, _ = _minimizer(g, "cg", observe=False, tile=64)
    E0, grad0 = mz.compute_energy_and_gradient_array()
    assert mesh._hip_mirror.dm.tile_stats()["n_tiles"] > 1
    assert abs(E0 - g["E0"]) <= 1e-12 * abs(g["E0"])
    assert relerr(grad0, g["grad0"]) < 1e-10
    res = mz.minimize(int(g["n_steps"]))
    _check_finals(mesh, res, g)


def _run_final(g, kind, **kw):
    mesh, mz, _ = _minimizer(g, kind, observe=False, **kw)
    res = mz.minimize(int(g["n_steps"]))
    return (mesh.positions_view().copy(), np.array(mesh.tilts_in_view()).copy(), np.array(mesh.tilts_out_view()).copy(),
            res["energy"])


def test_rim_source_trajectory_is_bitwise_reproducible_deterministic(monkeypatch):
    monkeypatch.setenv("MS_DETERMINISTIC", "1")
    g = load_golden("traj_disk6_gd_rimsource_nested_cg.npz")
    a = _run_final(g, "gd", tile=64)
    b = _run_final(g, "gd", tile=64)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_rim_source_trajectory_without_the_interpreter_is_bitwise_equal(monkeypatch):
    """MS_EXEC=0 (launch per kernel) against the default (one-tile interpreter, flushed before every rim launch)."""
    g = load_golden("traj_disk5_gd_rimsource_follow_fastpath.npz")
    monkeypatch.setenv("MS_DETERMINISTIC", "1")
    a = _run_final(g, "gd")
    monkeypatch.setenv("MS_EXEC", "0")
    b = _run_final(g, "gd")
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


# ---------------------------------------------------------------------------------------------------------------------
def _milestone_mesh(g, mods=None):
    from membrane_solver_amd.geometry.mesh import ArrayMesh

    mods = [str(m) for m in g["modules"]] if mods is None else mods
    return ArrayMesh(g["positions"], g["tri"], tilts_in=g["tilts_in0"], tilts_out=g["tilts_out0"],
                     tilt_fixed_in=g["tilt_fixed_in"], tilt_fixed_out=g["tilt_fixed_out"],
                     global_parameters=json.loads(str(g["gp_json"])), energy_modules=mods, constraint_modules=[],
                     edges=g["edges"], vertex_options=_opts(g["vopts"])), mods


def _milestone_relax(g, mods=None):
    from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager
    from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager
    from membrane_solver_amd.runtime.minimizer import Minimizer
    from membrane_solver_amd.runtime.steppers import GradientDescent

    mesh, mods = _milestone_mesh(g, mods)
    mz = Minimizer(mesh, mesh.global_parameters, GradientDescent(), EnergyModuleManager(mods), ConstraintModuleManager([]),
                   quiet=True)
    _mir, dm = mz._device()
    iters, evals = dm.relax_leaflet_tilts(**mz._tilt_relax_params())
    return mz, dm, iters, evals


def test_milestone_c_relaxation_matches_reference():
    """One nested leaflet relaxation on the reference's milestone-C annulus (24 vertices, 8 rim edges, follow mode), the
    benchmark's setup: 50 inner steps, step 0.05, tilt_tol 0."""
    g = load_golden("rim_source_milestone_c.npz")
    mz, dm, iters, evals = _milestone_relax(g)
    tin, tout = dm.get_leaflet_tilts("in"), dm.get_leaflet_tilts("out")
    E = float(dm.energy().sum())
    print("evals", evals, "ref", int(g["n_evaluations"]), "E", E, "ref", float(g["E_total"]), "relerr",
          relerr(tin, g["tilts_in_final"]), relerr(tout, g["tilts_out_final"]))
    assert evals == int(g["n_evaluations"])
    assert relerr(tin, g["tilts_in_final"]) < 1e-8
    # (the annulus is flat: nothing drives the outer leaflet, the reference's tilts_out stay 0)
    assert not g["tilts_out_final"].any() and np.max(np.abs(tout)) <= 1e-8 * np.max(np.abs(g["tilts_in_final"]))
    assert abs(E - g["E_total"]) <= 1e-9 * abs(g["E_total"])
    assert abs(dm.leaflet_rim_source_energy("in") - g["E_rim"]) <= 1e-9 * abs(g["E_rim"])
    st = dm.exec_stats()
    assert st["relax_fused"] == 0 and st["relax_programs"] == 0
    rs = dm.leaflet_rim_source_stats("in")
    # the coefficients (and the followed center) once for the whole relaxation, one apply per evaluation of it; the
    # evaluation that leaves the bending_tilt record before the loop and dm.energy() above form theirs in the apply launch
    assert rs["coef_launches"] == 1 and rs["frame_launches"] <= 3
    assert evals + 1 <= rs["apply_launches"] <= evals + 2


def test_context_without_the_module_keeps_its_fast_lanes():
    """The same deck without tilt_rim_source_in: the fused evaluator runs the relaxation as before."""
    g = load_golden("rim_source_milestone_c.npz")
    mods = [str(m) for m in g["modules"] if str(m) != "tilt_rim_source_in"]
    _mz, dm, _iters, evals = _milestone_relax(g, mods)
    st = dm.exec_stats()
    assert evals > 0 and st["relax_fused"] > 0 and st["relax_programs"] > 0
    assert dm.leaflet_rim_source_stats("in")["apply_launches"] == 0


def test_search_passes_still_run_without_the_module():
    """A multi-tile leaflet relaxation without the module still takes the search / gradient passes of ms_tsearch.inc;
    with it they decline."""
    from membrane_solver_amd import _lib as L

    g = load_golden("traj_disk6_gd_rimsource_nested_cg.npz")
    counts = {}
    for with_module in (False, True):
        g2 = dict(g)
        if not with_module:
            g2["modules"] = np.array([m for m in g["modules"] if not str(m).startswith("tilt_rim_source")])
        _mesh, mz, _ = _minimizer(g2, "gd", observe=False, tile=64)
        _mir, dm = mz._device()
        assert bool(dm.modules & L.MS_MOD_TILT_RIM_SOURCE_IN) == with_module
        before = dm.tsearch_stats()["passes"]
        dm.relax_leaflet_tilts(**mz._tilt_relax_params())
        counts[with_module] = dm.tsearch_stats()["passes"] - before
    assert counts[False] > 0 and counts[True] == 0


def test_follow_mode_with_the_volume_enforcer_raises():
    from membrane_solver_amd import _lib as L
    from membrane_solver_amd import meshgen
    from membrane_solver_amd.device import DeviceMesh

    P, T = meshgen.icosphere(3)
    dm = DeviceMesh(P, T)
    dm.set_leaflet_tilts("in", np.zeros_like(P), tilt_modulus=1.0)
    dm.set_leaflet_tilts("out", np.zeros_like(P))
    dm.set_leaflet_rim_source("in", [0, 1], [1, 2], [1.0, 1.0], normal=(0.0, 0.0, 1.0), follow=True)
    dm.set_params(modules=L.MS_MOD_SURFACE | L.MS_CON_VOLUME | L.MS_MOD_TILT_IN | L.MS_MOD_TILT_RIM_SOURCE_IN,
                  target_volume=4.0)
    with pytest.raises(L.MembraneHipError, match="follow mode"):
        dm.step(stepper=L.MS_STEPPER_GD, step_size=1e-3, tol=0.0, enforce_volume=1)
    r = dm.step(stepper=L.MS_STEPPER_GD, step_size=1e-3, tol=0.0)  # (without the enforcer the step runs)
    assert np.isfinite(r.energy)
    dm.close()
