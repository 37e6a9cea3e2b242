"""pin_to_plane / pin_to_circle next to the tilt modules on the device: three reference trajectories
(tools/gen_golden_pins_tilt.py) through the Python loop and ms_minimize, one-tile and two-tile contexts; the tilt
restore of a rejected search; the project lane behind the tilt modules' shape gradients; reproducibility; refusals.

Bars of the trajectories are those of tests/test_gpu_rim_source.py: E0 to 1e-12 relative, relerr(grad0) < 1e-10, per
step the same trial count, alpha to rtol 1e-12 and energy to rtol 1e-9, final positions and tilt fields relerr < 1e-8."""

import json

import numpy as np
import pytest

from conftest import load_golden, relerr

pytestmark = pytest.mark.gpu

SOFT = "traj_softsource_deck_gd_pins.npz"
DISK6 = "traj_disk6_cg_coupling_pins_slide.npz"
ICO4 = "traj_ico4_gd_bt_pins_plane.npz"
TRAJ = [SOFT, DISK6, ICO4]
_CACHE = {}
# two iterations of the soft_source deck without constraints, on the parent build (test_context_without_pins_keeps_its_lanes)
PIN_FREE_COUNTERS = {"packs": 290, "records": 1155, "relax_programs": 0, "relax_fused": 0, "tsearch_passes": 0, "trials": 11}


def _gold(fname):
    if fname not in _CACHE:
        _CACHE[fname] = load_golden(fname)
    return _CACHE[fname]


def _opts(text):
    return {int(k): v for k, v in json.loads(str(text)).items()}


def _single(g):
    return "tilt" in [str(m) for m in g["modules"]]


def _minimizer(g, observe=False, tile=0, deterministic=None, constraints=None, modules=None):
    from membrane_solver_amd.geometry.mesh import ArrayMesh
    from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager
    from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager
    from membrane_solver_amd.runtime.minimizer import Minimizer
    from membrane_solver_amd.runtime.steppers import ConjugateGradient, GradientDescent

    mods = [str(m) for m in g["modules"]] if modules is None else modules
    cons = [str(m) for m in g["constraint_modules"]] if constraints is None else constraints
    fields = ({"tilts": g["tilts0"], "tilt_fixed": g["tilt_fixed"]} if _single(g) else
              {"tilts_in": g["tilts_in0"], "tilts_out": g["tilts_out0"], "tilt_fixed_in": g["tilt_fixed_in"],
               "tilt_fixed_out": g["tilt_fixed_out"]})
    mesh = ArrayMesh(g["positions0"], g["tri"], fixed=g["fixed"], surface_tension=g["gamma"],
                     global_parameters=json.loads(str(g["gp_json"])), energy_modules=mods, constraint_modules=cons,
                     edges=g["edges"], vertex_options=_opts(g["vopts"]), edge_options=_opts(g["eopts"]), **fields)
    stepper = ConjugateGradient() if str(g["stepper"]) == "ConjugateGradient" else GradientDescent()
    log = []
    if observe:
        orig = stepper.device_step

        def logged(dm, m, step_size, tol=0.0):
            r = orig(dm, m, step_size, tol=tol)
            log.append((float(r.success), r.next_step, r.energy, r.trials, r.guard_rejects, r.alpha))
            return r

        stepper.device_step = logged
    mz = Minimizer(mesh, mesh.global_parameters, stepper, EnergyModuleManager(mods), ConstraintModuleManager(cons),
                   quiet=True, step_size=float(g["step_size0"]), tile_vertices=tile, deterministic=deterministic)
    return mesh, mz, log


def _fields(mesh, g):
    if _single(g):
        return [(np.array(mesh.tilts_view()), g["tilts_final"])]
    return [(np.array(mesh.tilts_in_view()), g["tilts_in_final"]), (np.array(mesh.tilts_out_view()), g["tilts_out_final"])]


def _accepted_alphas(g):
    """per step: the alpha of the accepted trial (0.0 when the search failed or never started)"""
    tl = g["trial_log"]
    out = np.zeros(int(g["n_steps"]))
    for row in tl[tl[:, 4] == 1.0]:
        out[int(row[0])] = row[1]
    return out


@pytest.mark.parametrize("in_library", [False, True])
@pytest.mark.parametrize("tile", [256, 64])
@pytest.mark.parametrize("fname", TRAJ)
def test_trajectory_matches_reference(fname, tile, in_library):
    g = _gold(fname)
    mesh, mz, log = _minimizer(g, observe=not in_library, tile=tile)
    E0, grad0 = mz.compute_energy_and_gradient_array()
    dm = mesh._hip_mirror.dm
    n_tiles = dm.tile_stats()["n_tiles"]
    assert n_tiles == 1 if tile == 256 else n_tiles >= 2  # (84, 127 and 162 vertices: the pin pass crosses tiles at 64)
    print(fname, tile, "E0", E0, "ref", float(g["E0"]), "relerr grad0", relerr(grad0, g["grad0"]))
    assert abs(E0 - g["E0"]) <= 1e-12 * abs(g["E0"])
    assert relerr(grad0, g["grad0"]) < 1e-10
    res = mz.minimize(int(g["n_steps"]))
    ref, sl = g["step_log"], g["search_log"]
    if in_library:
        full = np.asarray(mz.last_run["step_log"])
        got = full[:, :3]
        trials, alphas = full[:, 7], full[:, 6]
    else:
        full = np.array(log)
        got = full[:, :3]
        trials, alphas = full[:, 3], full[:, 5]
        # (every rejected ladder position is either an evaluated trial or a guard rejection)
        assert np.array_equal(full[:, 4], sl[:, 4]), "guard rejections differ from the reference"
    print(fname, "got", got.tolist(), "trials", trials.tolist(), "ref", ref.tolist(), sl[:, 3].tolist())
    assert got.shape == ref.shape
    assert np.array_equal(got[:, 0], ref[:, 0]), "accept/reject sequence differs from the reference"
    assert np.array_equal(trials, sl[:, 3]), "trial counts differ from the reference"
    assert np.allclose(got[:, 1], ref[:, 1], rtol=1e-12, atol=0)
    assert np.allclose(alphas, _accepted_alphas(g), rtol=1e-12, atol=0)
    assert np.allclose(got[:, 2], ref[:, 2], rtol=1e-9, atol=0)
    assert relerr(mesh.positions_view(), g["positions_final"]) < 1e-8
    for got_t, ref_t in _fields(mesh, g):
        assert relerr(got_t, ref_t) < 1e-8
    assert abs(res["energy"] - g["E_final"]) <= 1e-9 * abs(g["E_final"])
    assert dm.pin_stats()["trials"] == int(sl[:, 3].sum())


@pytest.mark.parametrize("deterministic", [False, True])
def test_exhausted_search_leaves_the_tilts_of_x(deterministic):
    """Every trial of the search rejected: the tilts afterwards are, bit for bit, the stored tilts after ONE projection
    at x -- not their projection onto the last rejected surface (the lane without an enforcer keeps that one).  Both
    contexts start from the same uploaded state (with LDS-atomic sums a relaxation is not bitwise repeatable)."""
    g = _gold(SOFT)
    _mesh, mz, _ = _minimizer(g, deterministic=deterministic)
    _mir, dm = mz._device()
    mz._enforce(dm, "mesh_operation")  # minimize()'s start: the pins, then the tilts onto the pinned surface
    dm.relax_leaflet_tilts(**mz._tilt_relax_params())  # the iteration's top: the state the fixture's first search sees
    state = dict(g, positions0=dm.get_positions(), tilts_in0=dm.get_leaflet_tilts("in"),
                 tilts_out0=dm.get_leaflet_tilts("out"))
    assert relerr(state["positions0"], g["positions_at_x"][0]) < 1e-12
    assert relerr(state["tilts_in0"], g["tilts_in_at_x"][0]) < 1e-9
    got = {}
    for what in ("project", "step"):
        _mesh, mz, _ = _minimizer(state, deterministic=deterministic)
        _mir, dm = mz._device()
        x = dm.get_positions()
        if what == "project":
            dm.project_tilts_to_tangent()
        else:
            # the fixture's first search is in this state; its first evaluated trial passed the guard and missed its
            # Armijo bound by more than 1e-9 |E0|: a search of that one trial runs out
            alpha = float(g["trial_log"][0, 1])
            assert g["trial_log"][0, 0] == 0.0 and g["trial_log"][0, 4] == 0.0
            before = dm.pin_stats()["trials"]
            r = dm.step(stepper=0, step_size=alpha, tol=0.0, max_iter=1, enforce_pins=1)
            print("exhausted search: alpha", alpha, "trials", r.trials, "guard", r.guard_rejects, "success", r.success)
            assert not r.success and r.trials == 1 and r.guard_rejects == 0
            assert dm.pin_stats()["trials"] - before == 1
            assert np.array_equal(dm.get_positions(), x)
        got[what] = (dm.get_leaflet_tilts("in"), dm.get_leaflet_tilts("out"))
    print("max |step - project|", [float(np.max(np.abs(a - b))) for a, b in zip(got["step"], got["project"])])
    assert np.array_equal(got["step"][0], got["project"][0])
    assert np.array_equal(got["step"][1], got["project"][1])
    # the fixture's own record: a rejected trial's projection moves the stored tilts by far more than rounding
    tl = g["trial_log"]
    assert tl[tl[:, 4] == 0.0][:, 5].max() > 1e-9


@pytest.mark.parametrize("tile", [256, 64])
def test_project_lane_behind_the_tilt_shape_gradients(tile):
    g = _gold(DISK6)
    _mesh, mz, _ = _minimizer(g, tile=tile)
    _mir, dm = mz._device()
    assert mz.pin_tables.lane == "project" and dm.pin_stats()["lane"] == 1
    before = dm.pin_stats()["grad_launches"]
    for k in range(2):
        _E, grad = mz.compute_energy_and_gradient_array()
        assert dm.pin_stats()["grad_launches"] == before + k + 1
    print("relerr", relerr(grad, g["grad0"]), "against the unprojected gradient", relerr(g["grad0_raw"], g["grad0"]))
    assert relerr(grad, g["grad0"]) < 1e-10
    assert relerr(g["grad0_raw"], g["grad0"]) > 1e-6  # (the pins' rows carry part of the gradient here)


def _run_final(g, **kw):
    mesh, mz, _ = _minimizer(g, **kw)
    res = mz.minimize(int(g["n_steps"]))
    return [mesh.positions_view().copy(), np.float64(res["energy"]), np.asarray(mz.last_run["step_log"])] + \
        [t for t, _ in _fields(mesh, g)]


@pytest.mark.parametrize("fname", TRAJ)
def test_trajectory_is_bitwise_reproducible_deterministic(fname, monkeypatch):
    """MS_DETERMINISTIC=1: two runs bitwise equal, and MS_EXEC=0 (a launch per kernel) equal to the default (the
    one-tile interpreter, flushed around the pin kernels)."""
    monkeypatch.setenv("MS_DETERMINISTIC", "1")
    g = _gold(fname)
    a = _run_final(g)
    b = _run_final(g)
    monkeypatch.setenv("MS_EXEC", "0")
    c = _run_final(g)
    for x, y, z in zip(a, b, c):
        assert np.array_equal(x, y)
        assert np.array_equal(x, z)


def _disk5_final():
    """traj_disk5_gd_pins_circle_fixed.npz (the shape-only pin lane: surface + bending, project lane) through ms_minimize"""
    import ast

    from membrane_solver_amd.geometry.mesh import ArrayMesh
    from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager
    from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager
    from membrane_solver_amd.runtime.minimizer import Minimizer
    from membrane_solver_amd.runtime.steppers import GradientDescent

    z = _gold("traj_disk5_gd_pins_circle_fixed.npz")
    mods, cons = [str(m) for m in z["energy_modules"]], [str(m) for m in z["constraint_modules"]]
    mesh = ArrayMesh(z["positions0"], z["tri"], fixed=z["fixed"], global_parameters=ast.literal_eval(str(z["gp"])),
                     vertex_options=ast.literal_eval(str(z["vopts"])), edges=z["edges"],
                     edge_options=ast.literal_eval(str(z["eopts"])), energy_modules=mods, constraint_modules=cons)
    mz = Minimizer(mesh, mesh.global_parameters, GradientDescent(), EnergyModuleManager(mods), ConstraintModuleManager(cons),
                   energy_modules=mods, constraint_modules=cons, quiet=True, step_size=float(z["step_size0"]))
    res = mz.minimize(int(z["n_steps"]))
    dm = mesh._hip_mirror.dm
    return [mesh.positions_view().copy(), np.float64(res["energy"]), np.asarray(mz.last_run["step_log"])], dm.exec_stats(), dm.pin_stats()


@pytest.mark.parametrize("fname", TRAJ + ["traj_disk5_gd_pins_circle_fixed.npz"])
def test_recorded_pin_kernels_are_bitwise_the_launched_ones(fname, monkeypatch):
    """MS_EXEC_PINS=0 (both pin kernels flush the one-workgroup interpreter and run as launches) against the default
    (CK_PIN_ENFORCE / CK_PIN_GRAD records of the pack): same bits, same program-run counters, fewer k_exec launches."""
    monkeypatch.setenv("MS_DETERMINISTIC", "1")

    def run():
        if fname not in TRAJ:
            return _disk5_final()
        g = _gold(fname)
        mesh, mz, _ = _minimizer(g)
        res = mz.minimize(int(g["n_steps"]))
        dm = mesh._hip_mirror.dm
        out = [mesh.positions_view().copy(), np.float64(res["energy"]), np.asarray(mz.last_run["step_log"])]
        return out + [t for t, _ in _fields(mesh, g)], dm.exec_stats(), dm.pin_stats()

    a, ex_a, pin_a = run()
    monkeypatch.setenv("MS_EXEC_PINS", "0")
    b, ex_b, pin_b = run()
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert ex_a["active"] and ex_b["active"]
    assert pin_a == pin_b and pin_a["enforce_launches"] > 0  # (program runs, recorded or launched)
    print(fname, "k_exec launches", ex_a["packs"], "recorded /", ex_b["packs"], "flushed; pin runs", pin_a)
    assert ex_a["packs"] < ex_b["packs"]


def test_no_flush_between_the_records_of_a_trial(monkeypatch):
    """One safe-small trial of the icosphere deck (tilt + bending_tilt under a fixed plane; no kernel of its own that
    flushes, as the rim source's do) is one pack with recording on -- positions, pin program, projection, energy passes
    and the fold reach the device together -- and two with MS_EXEC_PINS=0 (the pin kernel cuts it)."""
    g = _gold(ICO4)
    packs = {}
    for pins_recorded in (True, False):
        monkeypatch.setenv("MS_EXEC_PINS", "1" if pins_recorded else "0")
        _mesh, mz, _ = _minimizer(g, deterministic=True)
        _mir, dm = mz._device()
        mz._enforce(dm, "mesh_operation")
        counts = []
        for max_iter in (1, 2):  # the searches differ by exactly one trial: alpha = 1e-5 and 0.7e-5, far below the guard's range
            dm.set_positions(dm.get_positions())
            p0, t0 = dm.exec_stats()["packs"], dm.pin_stats()["trials"]
            r = dm.step(stepper=0, step_size=1e-5, tol=0.0, max_iter=max_iter, c=2.0, enforce_pins=1)
            assert not r.success and r.guard_rejects == 0 and r.trials == max_iter  # (c = 2: no trial can pass Armijo)
            assert dm.pin_stats()["trials"] - t0 == max_iter
            counts.append(dm.exec_stats()["packs"] - p0)
        packs[pins_recorded] = counts[1] - counts[0]
    print("k_exec launches per trial: recorded", packs[True], "flushed", packs[False])
    assert packs[True] == 1 and packs[False] == 2


def test_pins_tilt_and_volume_are_refused():
    from membrane_solver_amd import _lib as L

    g = _gold(ICO4)
    _mesh, mz, _ = _minimizer(g, constraints=["pin_to_plane", "volume"])
    with pytest.raises(L.MembraneHipError, match="together with the volume constraint"):
        mz.minimize(1)
    # the library's own refusal: the volume row next to pins on a trial, a tilt family active
    _mesh, mz, _ = _minimizer(g)
    _mir, dm = mz._device()
    dm.set_params(modules=dm.modules | L.MS_CON_VOLUME, target_volume=4.0)
    with pytest.raises(L.MembraneHipError, match="together with the volume constraint"):
        dm.step(stepper=L.MS_STEPPER_GD, step_size=1e-3, tol=0.0, enforce_pins=1)


def test_follow_mode_rim_source_with_pins_is_refused():
    from membrane_solver_amd import _lib as L

    g = _gold(SOFT)
    _mesh, mz, _ = _minimizer(g)
    _mir, dm = mz._device()
    assert dm.pin_stats()["lane"] >= 0
    rim = np.flatnonzero(np.abs(np.linalg.norm(g["positions0"][:, :2], axis=1) - 1.0) < 1e-6)
    dm.set_leaflet_rim_source("in", rim[:-1], rim[1:], np.ones(len(rim) - 1), normal=(0.0, 0.0, 1.0), follow=True)
    with pytest.raises(L.MembraneHipError, match="follow mode"):
        dm.step(stepper=L.MS_STEPPER_GD, step_size=1e-3, tol=0.0, enforce_pins=1)


def test_sharded_context_refuses_pins():
    from membrane_solver_amd import _lib as L
    from membrane_solver_amd.device import DeviceMesh

    g = _gold(ICO4)
    _mesh, mz, _ = _minimizer(g)
    mz._device()
    d2 = DeviceMesh(g["positions0"], g["tri"], shard_rank=0, shard_count=2)
    with pytest.raises(L.MembraneHipError, match="single-shard only"):
        d2.set_pins(mz.pin_tables)
    d2.close()


def test_context_without_pins_keeps_its_lanes():
    """The soft_source deck with its constraint list emptied: no pin tables, no pin program, no pin trial; the
    interpreter's launch and record counts and the tilt search counters of two iterations are those of the build before
    pins could run next to tilt modules (measured on that build: they move when the pin-free lane changes)."""
    g = _gold(SOFT)
    _mesh, mz, _ = _minimizer(g, constraints=[], deterministic=True)
    _mir, dm = mz._device()
    assert not mz._pins_active and dm.pin_stats()["lane"] == -1
    st0, ts0 = dm.exec_stats(), dm.tsearch_stats()
    res = mz.minimize(2)
    st1, ts1 = dm.exec_stats(), dm.tsearch_stats()
    assert res["iterations"] == 2 and mz.stepper.enforce_pins == 0
    assert st1["active"] and st1["wanted"]
    got = {"packs": st1["packs"] - st0["packs"], "records": st1["launches_recorded"] - st0["launches_recorded"],
           "relax_programs": st1["relax_programs"] - st0["relax_programs"], "relax_fused": st1["relax_fused"] - st0["relax_fused"],
           "tsearch_passes": ts1["passes"] - ts0["passes"], "trials": int(mz.last_run["trials"])}
    print("pin-free lane counters", got)
    assert got == PIN_FREE_COUNTERS
    assert dm.pin_stats() == {"lane": -1, "enforce_launches": 0, "grad_launches": 0, "trials": 0}
