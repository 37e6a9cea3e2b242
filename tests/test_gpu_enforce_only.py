"""fixed_plane / perimeter on the device against the reference (tests/golden/enforce_only_cases.npz, traj_*_perim_*.npz,
traj_*_fplane_*.npz): the two enforcers through the C ABI and through the modules, trajectories through Minimizer (Python
loop and ms_minimize), reproducibility, the one-tile interpreter, the evaluation-reuse levels, the resident kernel
declining, and the lanes that must not notice the feature.  The bars are those of tests/test_gpu_area_constraint.py."""

import ast
import json
import os

import numpy as np
import pytest

from membrane_solver_amd import _lib as L
from membrane_solver_amd import meshgen
from membrane_solver_amd.device import DeviceMesh
from membrane_solver_amd.geometry.mesh import ArrayBody, ArrayMesh, mirror_for
from membrane_solver_amd.modules.constraints import fixed_plane, perimeter
from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager
from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager
from membrane_solver_amd.runtime.minimizer import Minimizer
from membrane_solver_amd.runtime.steppers import ConjugateGradient, GradientDescent

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
PERIM = ["traj_disk%d_%s_perim_%s.npz" % (n, s, w) for n in (5, 12) for s in ("gd", "cg") for w in ("alone", "area")]
FPLANE = ["traj_disk%d_%s_fplane_%s.npz" % (n, s, w) for n in (5, 12) for s in ("gd", "cg") for w in ("default", "oblique")]
# fixed_plane in front of perimeter
FPLANE_PERIM = ["traj_disk5_%s_fplane_perim.npz" % s for s in ("gd", "cg")]
TRAJ = PERIM + FPLANE + FPLANE_PERIM
ONE_TILE = ["traj_disk5_gd_perim_alone.npz", "traj_disk5_cg_perim_area.npz", "traj_disk5_gd_fplane_oblique.npz"]
_CACHE = {}


def _load(fname):
    if fname not in _CACHE:
        _CACHE[fname] = dict(np.load(os.path.join(GOLD, fname)))
    return _CACHE[fname]


def _cases():
    return _load("enforce_only_cases.npz")


def _mz(mesh, stepper=None, tile=0, step_size=1e-3, deterministic=None):
    cons = list(mesh.constraint_modules)
    return Minimizer(mesh, mesh.global_parameters, stepper or GradientDescent(), EnergyModuleManager(mesh.energy_modules),
                     ConstraintModuleManager(cons), energy_modules=mesh.energy_modules, constraint_modules=cons, quiet=True,
                     step_size=step_size, tile_vertices=tile, deterministic=deterministic)


@pytest.mark.parametrize("tile", [64, 256])
def test_perimeter_enforcer_matches_reference(tile):
    """Through ms_project_perimeter and through the module: passes per loop equal, P of the last evaluation to 1e-12,
    positions to 1e-10, rows the reference left alone (the fixed ones among them) bitwise unmoved, the padded rows
    untouched, the zero-pass cases bitwise unchanged."""
    z = _cases()
    for name in [str(n) for n in z["perimeter_names"]]:
        P, fixed = z[name + "__positions"], z[name + "__fixed"]
        touched = z[name + "__touched"]
        want = P.copy()
        want[touched] = z[name + "__positions_touched"]
        if name + "__tri" in z:
            T = z[name + "__tri"]
        else:
            T = meshgen.disk_patch(48)[1]
        dm = DeviceMesh(P, T, fixed=fixed, tile_vertices=tile)
        pad0 = dm.padded_positions()
        dm.set_perimeter(z[name + "__loop_off"], z[name + "__tail"], z[name + "__head"], z[name + "__target"])
        assert dm.enforce_only_stats()["loops"] == len(z[name + "__target"])
        passes, per = dm.project_perimeter(tol=1e-10, max_iter=3)
        X = dm.get_positions()
        rest = np.setdiff1d(np.arange(len(P)), touched)
        print(f"{name} tile={tile}: passes {passes.tolist()} (reference {z[name + '__passes'].tolist()}) "
              f"max|dP|={np.abs(per - z[name + '__perimeter']).max():.3e} max|dx|={np.abs(X - want).max():.3e}")
        assert np.array_equal(passes, z[name + "__passes"]), name
        np.testing.assert_allclose(per, z[name + "__perimeter"], rtol=0, atol=1e-12, err_msg=name)
        np.testing.assert_allclose(X, want, rtol=0, atol=1e-10, err_msg=name)
        assert np.array_equal(X[rest], P[rest]) and np.array_equal(X[fixed], P[fixed]), name
        assert np.array_equal(dm.padded_positions(), pad0), name
        if not passes.any():
            assert np.array_equal(X, P), name
        assert dm.enforce_only_stats()["perimeter_launches"] == 1  # (one launch, however many loops and passes)
        dm.project_perimeter(fetch=False)  # (nothing comes back; a second call moves what the reference's would)
        dm.set_perimeter()
        with pytest.raises(L.MembraneHipError, match="no loops"):
            dm.project_perimeter()
        dm.close()
        if name + "__edges" not in z:
            continue
        # the Python module on a mesh, with the signed indices of the reference's own list: same result, written back
        cons = ast.literal_eval(str(z[name + "__constraints"]))
        mesh = ArrayMesh(P, T, fixed=fixed, edges=z[name + "__edges"], global_parameters={"perimeter_constraints": cons})
        mirror_for(mesh, tile_vertices=tile)  # (the module works on the mesh's own context: this one, at this tile size)
        perimeter.enforce_constraint(mesh)
        assert mesh._hip_mirror.dm.enforce_only_stats()["perimeter_launches"] == 1
        np.testing.assert_allclose(mesh.positions_view(), want, rtol=0, atol=1e-10, err_msg=name)
        assert np.array_equal(mesh.positions_view()[rest], P[rest]), name


@pytest.mark.parametrize("tile", [64, 256])
def test_fixed_plane_enforcer_matches_reference(tile):
    """Through ms_enforce_fixed_plane and through the module: positions to 1e-10, fixed rows bitwise unmoved, the padded rows
    untouched, and on the default plane exact zeros in z with x, y bit for bit."""
    z = _cases()
    for name in [str(n) for n in z["fixed_plane_names"]]:
        P, T, fixed = z[name + "__positions"], z[name + "__tri"], z[name + "__fixed"]
        gp = ast.literal_eval(str(z[name + "__gp"]))
        want = z[name + "__positions_final"]
        dm = DeviceMesh(P, T, fixed=fixed, tile_vertices=tile)
        pad0 = dm.padded_positions()
        assert len(pad0) > 0 and len(P) % 256 != 0
        dm.set_fixed_plane(gp.get("fixed_plane_normal", (0.0, 0.0, 1.0)), gp.get("fixed_plane_point"))
        dm.enforce_fixed_plane()
        X = dm.get_positions()
        print(f"{name} tile={tile}: max|dx|={np.abs(X - want).max():.3e}")
        np.testing.assert_allclose(X, want, rtol=0, atol=1e-10, err_msg=name)
        assert np.array_equal(X[fixed], P[fixed]), name
        assert np.array_equal(dm.padded_positions(), pad0), name
        if "fixed_plane_normal" not in gp:
            assert not X[~fixed, 2].any() and np.array_equal(X[:, :2], P[:, :2]), name
        assert dm.enforce_only_stats()["fixed_plane_launches"] == 1
        dm.set_fixed_plane()
        with pytest.raises(L.MembraneHipError, match="no plane"):
            dm.enforce_fixed_plane()
        dm.close()
        mesh = ArrayMesh(P, T, fixed=fixed, global_parameters=dict(gp))
        mirror_for(mesh, tile_vertices=tile)
        fixed_plane.enforce_constraint(mesh)
        assert mesh._hip_mirror.dm.enforce_only_stats()["fixed_plane_launches"] == 1
        np.testing.assert_allclose(mesh.positions_view(), want, rtol=0, atol=1e-10, err_msg=name)
        assert np.array_equal(mesh.positions_view()[fixed], P[fixed]), name
    # a zero normal: the reference's warning, nothing set, nothing moved
    mesh = ArrayMesh(P, T, global_parameters={"fixed_plane_normal": [0.0, 0.0, 0.0]})
    fixed_plane.enforce_constraint(mesh)
    assert np.array_equal(mesh.positions_view(), P)


def _traj_mesh(z):
    bodies = None
    if "body_facets" in z:
        rows, nf = z["body_facets"], len(z["tri"])
        bodies = [ArrayBody(facet_rows=None if len(rows) == nf else np.asarray(rows),
                            target_volume=float(z["target_volume"]) if "target_volume" in z else None,
                            options=ast.literal_eval(str(z["body_options"])))]
    return ArrayMesh(z["positions0"], z["tri"], fixed=z["fixed"], edges=z["edges"],
                     global_parameters=ast.literal_eval(str(z["gp"])), bodies=bodies,
                     energy_modules=[str(s) for s in z["energy_modules"]],
                     constraint_modules=[str(s) for s in z["constraint_modules"]])


def _run(fname, tile, in_library, reuse=2, deterministic=None):
    """-> (fixture, step log (n,3), final positions, final energy, final step size, device, minimizer)"""
    z = _load(fname)
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


def test_perimeter_on_the_bodys_facets_is_refused_next_to_body_area():
    """The fixtures' body owns the inner facets and the loop is the rim: no vertex in common.  With the body over every
    facet the reference's body_area would take its first pass from positions cached before perimeter moved the rim."""
    z = _load("traj_disk5_gd_perim_area.npz")
    mesh = _traj_mesh(z)
    mesh.bodies[next(iter(mesh.bodies))].facet_rows = None
    with pytest.raises(L.MembraneHipError, match="with a listed edge on the body's facets"):
        _mz(mesh).minimize(1)


def test_minimizer_takes_perimeter_and_fixed_plane():
    """What the parent refused with "outside the HIP hot path"."""
    for fname in ("traj_disk5_gd_perim_area.npz", "traj_disk5_gd_fplane_oblique.npz"):
        mz = _mz(_traj_mesh(_load(fname)))
        assert np.isfinite(mz.minimize(1)["energy"])


@pytest.mark.parametrize("fname", TRAJ)
@pytest.mark.parametrize("tile", [64, 256])
@pytest.mark.parametrize("in_library", [False, True])
def test_trajectory_matches_reference(fname, tile, in_library):
    """Accept / reject flags and step sizes identical, accepted energies to 1e-10, final positions to 1e-8; every Armijo
    decision of the lane is the host's; the launches show in ms_enforce_only_stats."""
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
    assert qs["rounds"] == 0 and qs["mismatches"] == 0, qs
    st = dm.enforce_only_stats()
    cons = [str(s) for s in z["constraint_modules"]]
    assert st["trials"] >= int(ref[:, 0].sum())  # (an accepted step ran at least one trial through the enforcers)
    if "perimeter" in cons:
        assert st["perimeter_launches"] > st["trials"] and st["loops"] == 1
    else:
        assert st["perimeter_launches"] == 0 and st["loops"] == 0
    if "fixed_plane" not in cons:
        assert st["fixed_plane_launches"] == 0
    else:
        assert st["fixed_plane_launches"] > st["trials"]
        fixed = z["fixed"]
        gp = ast.literal_eval(str(z["gp"]))
        n = np.asarray(gp.get("fixed_plane_normal", (0.0, 0.0, 1.0)), dtype=float)
        d = (X - np.asarray(gp.get("fixed_plane_point", (0.0, 0.0, 0.0)))) @ (n / np.linalg.norm(n))
        if cons == ["fixed_plane"]:  # (an enforcer behind it moves the rows it holds off the plane again)
            assert np.abs(d[~fixed]).max() < 1e-15
        if "fixed_plane_normal" in gp:  # (the fixed rim rows stay off the oblique plane; the disk's rim lies in z = 0)
            assert np.abs(d[fixed]).max() > 0.1


DECKS = ["traj_annulus_flat_no_tilt_gd_fplane_pins.npz", "traj_kozlov_annulus_flat_soft_source_gd_fplane_pins.npz",
         "traj_kozlov_annulus_flat_hard_source_gd_fplane_pins.npz"]


def _deck_minimizer(g, observe, tile):
    opts = lambda text: {int(k): v for k, v in json.loads(str(text)).items()}  # noqa: E731
    mods = [str(m) for m in g["energy_modules"]]
    cons = [str(m) for m in g["constraint_modules"]]
    mesh = ArrayMesh(g["positions0"], g["tri"], fixed=g["fixed"], surface_tension=g["gamma"],
                     global_parameters=json.loads(str(g["gp_json"])), energy_modules=mods, constraint_modules=cons,
                     edges=g["edges"], vertex_options=opts(g["vopts"]), edge_options=opts(g["eopts"]),
                     tilts_in=g["tilts_in0"], tilts_out=g["tilts_out0"], tilt_fixed_in=g["tilt_fixed_in"],
                     tilt_fixed_out=g["tilt_fixed_out"])
    stepper = GradientDescent()
    log = []
    if observe:
        orig = stepper.device_step

        def logged(dm, m, step_size, tol=0.0):
            r = orig(dm, m, step_size, tol=tol)
            if not r.converged:
                log.append((float(bool(r.success)), float(r.next_step), float(r.energy)))
            return r

        stepper.device_step = logged
    mz = Minimizer(mesh, mesh.global_parameters, stepper, EnergyModuleManager(mods), ConstraintModuleManager(cons),
                   quiet=True, step_size=float(g["step_size0"]), tile_vertices=tile)
    return mesh, mz, log


@pytest.mark.parametrize("fname", DECKS)
@pytest.mark.parametrize("tile", [64, 256])
@pytest.mark.parametrize("in_library", [False, True])
def test_deck_trajectory_matches_reference(fname, tile, in_library):
    """The three annulus decks that list fixed_plane next to pin_to_circle, their free vertices lifted off the plane: 5 GD
    steps (the tilt decks relax the inner leaflet's tilts in every step; the deck without tilt modules carries a seeded
    surface tension per facet, its uniform one being constant on the flat annulus).  Same bars as the other trajectories; the tilts to 1e-8 relative."""
    g = _load(fname)
    mesh, mz, log = _deck_minimizer(g, not in_library, tile)
    assert mz.constraint_module_names == ["fixed_plane", "pin_to_circle"]
    res = mz.minimize(int(g["n_steps"]))
    dm = mz._device()[1]
    ref = np.asarray(g["step_log"]).reshape(-1, 3)
    assert len(ref) == 5 and ref[:, 0].sum() >= 3
    if in_library:
        got = np.asarray(mz.last_run["step_log"])[:, :3][: len(ref)]
    else:
        got = np.array(log).reshape(-1, 3)
    X = mesh.positions_view()
    print(f"{fname} tile={tile} in_library={in_library}: steps {len(got)} (reference {len(ref)}) "
          f"|dE_final|={abs(res['energy'] - float(g['E_final'])):.3e} max|dx|={np.abs(X - g['positions_final']).max():.3e} "
          f"max|dt_in|={np.abs(np.array(mesh.tilts_in_view()) - g['tilts_in_final']).max():.3e}")
    assert got.shape == ref.shape
    print("   max|dE|=%.3e" % np.abs(got[:, 2] - ref[:, 2]).max())
    np.testing.assert_array_equal(got[:, 0], ref[:, 0])
    np.testing.assert_array_equal(got[:, 1], ref[:, 1])
    np.testing.assert_allclose(got[:, 2], ref[:, 2], rtol=0, atol=1e-10)
    assert float(mz.step_size) == float(g["step_size_final"])
    assert abs(res["energy"] - float(g["E_final"])) <= 1e-10
    np.testing.assert_allclose(X, g["positions_final"], rtol=0, atol=1e-8)
    t_ref = g["tilts_in_final"]  # (the tilt fields' bar of tests/test_gpu_pins_tilt.py: 1e-8 of the largest component)
    assert np.abs(np.array(mesh.tilts_in_view()) - t_ref).max() <= 1e-8 * max(np.abs(t_ref).max(), 1e-300)
    free = ~g["fixed"]
    assert np.abs(g["positions0"][free, 2]).max() > 0.01 and not X[free, 2].any()  # (lifted at the start, exactly flat at the end)
    st = dm.enforce_only_stats()
    assert st["fixed_plane_launches"] >= 1 + len(ref) and st["trials"] >= int(ref[:, 0].sum())
    assert dm.pin_stats()["enforce_launches"] >= 1 + len(ref)
    assert dm.queue_stats()["rounds"] == 0


@pytest.mark.parametrize("fname", ["traj_disk5_gd_fplane_oblique.npz", "traj_disk5_cg_fplane_perim.npz",
                                   "traj_kozlov_annulus_flat_hard_source_gd_fplane_pins.npz"])
def test_position_buffers_that_are_only_8_byte_aligned(fname):
    """131 rows per tile and one tile: nvp = 131, the context's buffers are slices at multiples of 3 * 131 doubles, so every
    second one -- the line search's trial buffer among them -- starts 8 bytes off a 16-byte boundary.  k_fixed_plane takes
    its rows one by one there; the trajectory is the reference's all the same."""
    z = _load(fname)
    if "annulus" in fname:
        mesh, mz, _log = _deck_minimizer(z, False, 131)
        mz.minimize(int(z["n_steps"]))
        got = np.asarray(mz.last_run["step_log"])[:, :3]
        X, dm = mesh.positions_view(), mz._device()[1]
    else:
        z, got, X, _E, _step, dm, _m = _run(fname, 131, True)
    assert (len(dm.padded_positions()) + len(X)) % 2 == 1  # (nvp odd: every second buffer starts 8 bytes off)
    ref = np.asarray(z["step_log"]).reshape(-1, 3)
    got = got[: len(ref)]
    np.testing.assert_array_equal(got[:, :2], ref[:, :2])
    np.testing.assert_allclose(got[:, 2], ref[:, 2], rtol=0, atol=1e-10)
    np.testing.assert_allclose(X, z["positions_final"], rtol=0, atol=1e-8)
    assert dm.enforce_only_stats()["fixed_plane_launches"] > len(ref)


@pytest.mark.parametrize("fixed_order", [False, True])
def test_two_runs_are_bitwise_equal(fixed_order, monkeypatch):
    """In both summation modes: the enforcers' sums have one order; the energies' sums are fixed-order on request and the
    one-tile meshes have no atomics to race."""
    if fixed_order:
        monkeypatch.setenv("MS_DETERMINISTIC", "1")
    for fname, tile, lib in (("traj_disk12_cg_perim_area.npz", 64, True), ("traj_disk12_gd_fplane_oblique.npz", 64, False)):
        if not fixed_order:
            # default mode: the energy kernels' LDS atomics may reorder; the enforcers alone must still be reproducible
            z = _load(fname)
            outs = []
            for _ in range(2):
                dm = DeviceMesh(z["positions0"], z["tri"], fixed=z["fixed"], tile_vertices=tile)
                if "perim" in fname:
                    mesh = _traj_mesh(z)
                    _n, off, tail, head, target = perimeter.loops(mesh)
                    dm.set_perimeter(off, tail, head, target)
                    dm.project_perimeter()
                else:
                    gp = ast.literal_eval(str(z["gp"]))
                    dm.set_fixed_plane(gp["fixed_plane_normal"], gp["fixed_plane_point"])
                    dm.enforce_fixed_plane()
                outs.append(dm.get_positions())
                dm.close()
            assert np.array_equal(outs[0], outs[1]) and not np.array_equal(outs[0], z["positions0"])
            continue
        a = _run(fname, tile, lib)
        b = _run(fname, tile, lib)
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3] and a[4] == b[4]


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


@pytest.mark.parametrize("fname", ["traj_disk12_cg_perim_area.npz", "traj_disk12_cg_fplane_oblique.npz"])
def test_evaluation_reuse_levels_are_bitwise_identical(fname, deterministic):
    runs = [_run(fname, 64, True, reuse=r) for r in (0, 1, 2)]
    for r in runs[1:]:
        assert np.array_equal(r[1], runs[0][1]) and np.array_equal(r[2], runs[0][2])
        assert r[3] == runs[0][3] and r[4] == runs[0][4]


def _resident_params(target):
    mp = L.ms_minimize_params()  # (the block of tests/test_gpu_resident.py)
    mp.stepper = L.ms_stepper_params(int(L.MS_STEPPER_GD), 10, 0.7, 1e-4, 1.5, 10.0, 10, 0.0, 2, 0, 0)
    mp.step_size, mp.tol, mp.fixed_step = 1e-3, 1e-9, 1e-3
    mp.max_zero_steps, mp.step_size_floor = 10, 1e-8
    mp.drift_check, mp.target_volume, mp.volume_tolerance = 1, float(target), 1e-3
    return mp


def test_resident_kernel_declines_with_a_plane_set(monkeypatch):
    """A surface + volume-row GD context is the resident kernel's own case; with a plane set the kernel would drop the
    projection without a word, so it must not run."""
    monkeypatch.setenv("MS_RESIDENT", "1")
    P, T = meshgen.icosphere(16)
    P = meshgen.smooth_displace(P, 0.05)

    def run(plane):
        dm = DeviceMesh(P, T, body_facets=np.ones(len(T), dtype=np.uint8))
        dm.set_surface_tension(np.ones(len(T)))
        mods = L.MS_MOD_SURFACE | L.MS_CON_VOLUME
        dm.set_params(modules=mods)
        dm.energy()
        V0 = float(dm.fetch_scalars()[L.MS_S_VOL])
        dm.set_params(modules=mods, target_volume=V0)
        if plane:
            dm.set_fixed_plane([0.0, 0.0, 1.0], [0.0, 0.0, -5.0])
        dm.minimize(_resident_params(V0), 6)
        st = dm.resident_stats()
        dm.close()
        return st

    assert run(False)["steps"] > 0  # (the kernel's own case: it runs without the plane ...)
    assert run(True)["steps"] == 0  # (... and never with it)


def test_existing_lanes_do_not_notice_the_feature():
    """A context that has seen both setters, both enforcers (on positions put back afterwards) and cleared them behaves,
    bit for bit, as one that never has: queue statistics and a 6-step surface + bending CG trajectory on ico8."""
    P, T = meshgen.icosphere(8)
    P = meshgen.smooth_displace(P, 0.05)
    gp = {"surface_tension": 1.0, "bending_modulus": 1.0, "spontaneous_curvature": 0.2}

    def run(touch):
        mesh = ArrayMesh(P, T, global_parameters=dict(gp), energy_modules=["surface", "bending"])
        mz = _mz(mesh, ConjugateGradient(), tile=64, deterministic=True)
        dm = mz._device()[1]
        if touch:
            dm.set_fixed_plane([0.0, 1.0, 1.0], [0.0, 0.0, 0.3])
            dm.enforce_fixed_plane()
            dm.set_perimeter([0, 3], T[0], np.roll(T[0], -1), [1.0])
            dm.project_perimeter()
            dm.set_positions(P)
            dm.set_fixed_plane()
            dm.set_perimeter()
            st = dm.enforce_only_stats()
            assert st["fixed_plane_launches"] == 1 and st["perimeter_launches"] == 1 and st["loops"] == 0
        res = mz.minimize(6)
        log = np.asarray(mz.last_run["step_log"])
        return log, mesh.positions_view().copy(), res["energy"], dm.queue_stats(), dm.energy_stats()

    a, b = run(False), run(True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    assert a[3] == b[3] and a[4] == b[4]
    assert a[3]["rounds"] > 0  # (the headline lane did queue rounds: the comparison means something)


def test_c_abi_refusals():
    P, T = meshgen.icosphere(4)
    dm = DeviceMesh(P, T)
    dm.set_surface_tension(np.ones(len(T)))
    dm.set_params(modules=L.MS_MOD_SURFACE)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(L.MembraneHipError, match="the normal and the point must be finite"):
            dm.set_fixed_plane([0.0, bad, 1.0])
        with pytest.raises(L.MembraneHipError, match="the normal and the point must be finite"):
            dm.set_fixed_plane([0.0, 0.0, 1.0], [bad, 0.0, 0.0])
        with pytest.raises(L.MembraneHipError, match="a target perimeter is not finite"):
            dm.set_perimeter([0, 1], [0], [1], [bad])
    with pytest.raises(L.MembraneHipError, match=r"\|normal\| < 1e-15"):
        dm.set_fixed_plane([0.0, 0.0, 1e-16])
    for t, h in (([0], [len(P)]), ([-1], [0])):
        with pytest.raises(L.MembraneHipError, match="edge row out of range"):
            dm.set_perimeter([0, 1], t, h, [1.0])
    with pytest.raises(L.MembraneHipError, match="enforce_fixed_plane without a plane"):
        dm.step(stepper=L.MS_STEPPER_GD, step_size=1e-3, enforce_fixed_plane=1)
    with pytest.raises(L.MembraneHipError, match="enforce_perimeter without loops"):
        dm.step(stepper=L.MS_STEPPER_GD, step_size=1e-3, enforce_perimeter=1)
    # an empty loop is legal and does nothing
    dm.set_perimeter([0, 0], [], [], [1.0])
    passes, per = dm.project_perimeter()
    assert passes.tolist() == [0] and per.tolist() == [0.0] and np.array_equal(dm.get_positions(), P)
    # perimeter next to a tilt family is refused by the step
    dm.set_perimeter([0, 1], [0], [1], [1.0])
    dm.set_tilts(np.zeros_like(P), 1.0)
    dm.set_params(modules=L.MS_MOD_SURFACE | L.MS_MOD_TILT)
    with pytest.raises(L.MembraneHipError, match="perimeter together with tilt modules is outside the device path"):
        dm.step(stepper=L.MS_STEPPER_GD, step_size=1e-3, enforce_perimeter=1)
    dm.close()
    # sharded contexts refuse both setters
    sh = DeviceMesh(P, T, shard_rank=0, shard_count=2)
    with pytest.raises(L.MembraneHipError, match="fixed_plane is not sharded"):
        sh.set_fixed_plane([0.0, 0.0, 1.0])
    with pytest.raises(L.MembraneHipError, match="perimeter is not sharded"):
        sh.set_perimeter([0, 1], [0], [1], [1.0])
    sh.close()
