"""edge_length_penalty on the device: module energy and gradient against the reference's
(tests/golden/edge_penalty_cases.npz), reference trajectories through Minimizer (Python loop and ms_minimize, multi-tile
and one-tile contexts), bitwise reproducibility in the fixed-order mode, and the lanes and refusals the module selects.
The bars are those of tests/test_gpu_line.py."""

import ast
import os

import numpy as np
import pytest

from membrane_solver_amd import _lib as L
from membrane_solver_amd.core.parameters import ParameterResolver
from membrane_solver_amd.device import DeviceMesh
from membrane_solver_amd.geometry.mesh import ArrayBody, ArrayMesh, mirror_for
from membrane_solver_amd.modules.energy import edge_length_penalty as mod
from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager
from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager
from membrane_solver_amd.runtime.minimizer import Minimizer
from membrane_solver_amd.runtime.steppers import ConjugateGradient, GradientDescent

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
TRAJ = ["traj_strip_gd_bending_edgepen.npz",                          # a: the folding deck's sheet, no surface module
        "traj_ico4_gd_edgepen_surface_backtrack.npz",                 # b: the first search rejects trials
        "traj_ico4_cg_edgepen_bending_volume_row.npz",                # c: bending, volume row in the KKT, CG
        "traj_ico8_cg_edgepen_bending_volume_row.npz",                # d: the same on a mesh of several tiles
        "traj_ico4_gd_edgepen_bending_volume_enforcer.npz",           # e: volume projected on every trial
        "traj_disk5_gd_edgepen_linetension_surface_pins_plane.npz"]   # f: both edge modules, rim on pin_to_plane
ONE_TILE = [f for f in TRAJ if "ico8" not in f]                       # <= 256 vertices: the one-workgroup interpreter
BOTH = TRAJ[5]


def _mz(mesh, stepper=None, tile=0, step_size=1e-3, deterministic=None):
    cons = list(mesh.constraint_modules)
    return Minimizer(mesh, mesh.global_parameters, stepper or GradientDescent(),
                     EnergyModuleManager(mesh.energy_modules), ConstraintModuleManager(cons),
                     energy_modules=mesh.energy_modules, constraint_modules=cons, quiet=True,
                     step_size=step_size, tile_vertices=tile, deterministic=deterministic)


def _case_mesh(z, name, energy_modules=("edge_length_penalty",)):
    return ArrayMesh(z[name + "__positions"], z[name + "__tri"], global_parameters=ast.literal_eval(str(z[name + "__gp"])),
                     edges=z[name + "__edges"], edge_options=ast.literal_eval(str(z[name + "__eopts"])),
                     energy_modules=list(energy_modules))


@pytest.mark.parametrize("tile", [64, 256])
@pytest.mark.parametrize("fixed_order", [False, True])
def test_module_energy_and_gradient_match_reference(tile, fixed_order):
    """The module alone through its plugin signatures: energy and ms_get_edge_penalty_energy to 1e-12 relative,
    gradient to 1e-10 of max|g|; edge_stiffness 0 gives exactly 0."""
    z = np.load(os.path.join(GOLD, "edge_penalty_cases.npz"))
    for name in [str(n) for n in z["names"]]:
        mesh = _case_mesh(z, name)
        res = ParameterResolver(mesh.global_parameters)
        mir = mirror_for(mesh, tile_vertices=tile)
        mir.sync().set_deterministic(fixed_order)
        g = np.zeros_like(mesh.positions_view())
        E = mod.compute_energy_and_gradient_array(mesh, mesh.global_parameters, res, positions=mesh.positions_view(),
                                                  index_map=mesh.vertex_index_to_row, grad_arr=g)
        E_ref, g_ref = float(z[name + "__energy"]), z[name + "__grad"]
        scale = np.abs(g_ref).max()
        E_own = mir.dm.edge_penalty_energy()
        st = mir.dm.tile_stats()
        print(f"{name} tile={tile} tiles={st['n_tiles']} fixed_order={fixed_order}: "
              f"dE/E={abs(E - E_ref) / max(abs(E_ref), 1e-300):.3e} dE_own/E={abs(E_own - E_ref) / max(abs(E_ref), 1e-300):.3e} "
              f"dg/max|g|={np.abs(g - g_ref).max() / max(scale, 1e-300):.3e}")
        if E_ref == 0.0:  # k == 0: energy 0, no gradient, the bit off
            assert E == 0.0 and not g.any() and E_own == 0.0, name
            assert mir.dm.edge_penalty_stats()["energy_launches"] == 0
            continue
        assert abs(E - E_ref) <= 1e-12 * abs(E_ref), (name, E, E_ref)
        assert np.abs(g - g_ref).max() <= 1e-10 * scale, name
        assert abs(E_own - E_ref) <= 1e-12 * abs(E_ref), (name, E_own, E_ref)
        if name == "ico8_all_edges" and tile == 256:
            assert st["n_tiles"] < (1920 + 255) // 256  # the grid is capped at the tiles and strides
        # the energy-only signature and the dictionary form agree with the array form
        E1, none = mod.compute_energy_and_gradient(mesh, mesh.global_parameters, res, compute_gradient=False)
        assert abs(E1 - E_ref) <= 1e-12 * abs(E_ref) and none == {}
        E2, rows = mod.compute_energy_and_gradient(mesh, mesh.global_parameters, res)
        assert abs(E2 - E_ref) <= 1e-12 * abs(E_ref)
        assert sorted(rows) == np.flatnonzero(np.any(g != 0.0, axis=1)).tolist()


@pytest.mark.parametrize("tile", [64, 256])
@pytest.mark.parametrize("fixed_order", [False, True])
def test_both_edge_modules_on_the_same_edges(tile, fixed_order):
    """line_tension and edge_length_penalty on the same edges, through the Minimizer: the sum of the reference's two
    modules, and each module's own energy."""
    z = np.load(os.path.join(GOLD, "edge_penalty_cases.npz"))
    name = "ico4_both_edge_modules"
    mesh = _case_mesh(z, name, ("line_tension", "edge_length_penalty"))
    mz = _mz(mesh, tile=tile, deterministic=fixed_order)
    E, g = mz.compute_energy_and_gradient_array()
    E_pen, E_line = float(z[name + "__energy"]), float(z[name + "__energy_line"])
    g_ref = z[name + "__grad"] + z[name + "__grad_line"]
    dm = mz._device()[1]
    assert dm.modules & L.MS_MOD_LINE_TENSION and dm.modules & L.MS_MOD_EDGE_LENGTH_PENALTY
    print(f"tile={tile} fixed_order={fixed_order}: dE/E={abs(E - E_pen - E_line) / (E_pen + E_line):.3e} "
          f"dg/max|g|={np.abs(g - g_ref).max() / np.abs(g_ref).max():.3e}")
    assert abs(E - (E_pen + E_line)) <= 1e-12 * (E_pen + E_line)
    assert np.abs(g - g_ref).max() <= 1e-10 * np.abs(g_ref).max()
    assert abs(dm.edge_penalty_energy() - E_pen) <= 1e-12 * E_pen
    assert abs(dm.line_energy() - E_line) <= 1e-12 * E_line
    out = mz.compute_energy_breakdown()
    assert abs(out["edge_length_penalty"] - E_pen) <= 1e-12 * E_pen and abs(out["line_tension"] - E_line) <= 1e-12 * E_line


def _traj_mesh(z):
    bodies = None
    if "body_options" in z:
        tv = float(z["target_volume"]) if "target_volume" in z else None
        bodies = [ArrayBody(target_volume=tv, options=ast.literal_eval(str(z["body_options"])))]
    return ArrayMesh(z["positions0"], z["tri"], fixed=z["fixed"], global_parameters=ast.literal_eval(str(z["gp"])),
                     vertex_options=ast.literal_eval(str(z["vopts"])), edges=z["edges"],
                     edge_options=ast.literal_eval(str(z["eopts"])), bodies=bodies,
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


@pytest.mark.parametrize("fname", TRAJ)
@pytest.mark.parametrize("tile", [64, 256])
@pytest.mark.parametrize("in_library", [False, True])
def test_trajectory_matches_reference(fname, tile, in_library):
    """Accept / reject sequence and step sizes identical, energies to 1e-10, final positions to 1e-8."""
    z, got, X, E, step, dm, _mz_ = _run(fname, tile, in_library)
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
    assert dm.modules & L.MS_MOD_EDGE_LENGTH_PENALTY
    assert bool(dm.modules & L.MS_MOD_LINE_TENSION) == (fname == BOTH)
    assert dm.queue_stats()["mismatches"] == 0
    ps = dm.edge_penalty_stats()
    assert ps["energy_launches"] > 0 and ps["grad_launches"] > 0
    if "ico8" in fname:
        assert dm.tile_stats()["n_tiles"] > 1


@pytest.mark.parametrize("fname", TRAJ)
@pytest.mark.parametrize("in_library", [False, True])
def test_evaluation_reuse_levels_are_bitwise_identical(fname, in_library, deterministic):
    """Fixed-order sums: skipping the passes whose result is on the device changes no double."""
    runs = [_run(fname, 256, in_library, reuse=r) for r in (0, 1, 2)]
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


@pytest.mark.parametrize("fname", TRAJ)
@pytest.mark.parametrize("tile", [64, 256])
def test_two_runs_are_bitwise_identical(fname, tile, deterministic):
    a = _run(fname, tile, True)
    b = _run(fname, tile, True)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3] and a[4] == b[4]


@pytest.mark.parametrize("tile", [64, 256])
def test_module_energy_is_bitwise_reproducible_in_both_modes(tile):
    """The two kernels have no atomics on data: with no other module on (nothing else adds into G or the slot) energy,
    gradient and the module's own energy repeat bit for bit in the default mode too."""
    z = np.load(os.path.join(GOLD, "edge_penalty_cases.npz"))
    mesh = _case_mesh(z, "ico8_all_edges")
    tail, head, target, _n = mod.charged_edges(mesh, mesh.global_parameters)
    out = []
    for _ in range(2):
        dm = DeviceMesh(mesh.positions_view(), z["ico8_all_edges__tri"], tile_vertices=tile)
        dm.set_edge_length_penalty(tail, head, target, 25.0)
        dm.set_params(modules=L.MS_MOD_EDGE_LENGTH_PENALTY)
        e, g = dm.energy_and_gradient(raw=True)
        out.append((e.copy(), g.copy(), dm.edge_penalty_energy()))
        dm.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and out[0][2] == out[1][2]
    # slot 0 carries the penalty alone: the fold of the tiles' partials against the workgroup-order sum, two fixed
    # orders over at most 11 values of one sign (11 roundings of 1.1e-16 each at the most)
    assert out[0][2] > 0.0 and abs(out[0][0][0] - out[0][2]) <= 11 * 1.2e-16 * out[0][2]


@pytest.mark.parametrize("tile", [64, 256])
def test_host_decided_lane_on_multi_tile_mesh(tile, deterministic):
    """ico8 (several tiles): with the module on the host takes every Armijo decision -- no round of the
    device-decided queue is queued -- and no decision differs."""
    z, _got, _X, _E, _s, dm, mz = _run("traj_ico8_cg_edgepen_bending_volume_row.npz", tile, True)
    qs = dm.queue_stats()
    assert dm.tile_stats()["n_tiles"] > 1
    assert qs["rounds"] == 0 and qs["mismatches"] == 0, qs
    assert mz.last_run["accepted"] > 0
    # the plain lane of the same mesh does queue rounds (so the counter above means something)
    gp = dict(ast.literal_eval(str(z["gp"])), surface_tension=1.0)
    mesh = ArrayMesh(z["positions0"], z["tri"], global_parameters=gp, energy_modules=["surface", "bending"])
    mz2 = _mz(mesh, ConjugateGradient(), tile=tile, step_size=1e-3)
    mz2.minimize(4)
    assert mz2._device()[1].queue_stats()["rounds"] > 0


def _all_sides(T):
    """(tail, head) of every triangle side once, in a fixed order"""
    a = np.concatenate([T[:, 0], T[:, 1], T[:, 2]]).astype(np.int64)
    b = np.concatenate([T[:, 1], T[:, 2], T[:, 0]]).astype(np.int64)
    n = int(T.max()) + 1
    key = np.unique(np.minimum(a, b) * n + np.maximum(a, b))
    return key // n, key % n


def test_module_keeps_the_resident_step_off():
    """A size at which the plain surface + GD lane runs its steps in the resident kernel: with the module on none does."""
    from membrane_solver_amd import meshgen

    P, T = meshgen.icosphere(50)
    P = meshgen.smooth_displace(P, 0.03)
    t, h = _all_sides(T)
    t, h = t[::7], h[::7]
    ln = np.linalg.norm(P[h] - P[t], axis=1)
    assert len(t) > 100

    def run(with_module):
        mods = ["surface", "edge_length_penalty"] if with_module else ["surface"]
        mesh = ArrayMesh(P, T, global_parameters={"surface_tension": 1.0, "edge_stiffness": 5.0},
                         edges=np.stack([t, h], axis=1), edge_options=[{"target_length": float(x)} for x in 0.95 * ln],
                         energy_modules=mods)
        mz = _mz(mesh, GradientDescent(), tile=256, step_size=1e-4)
        mz.minimize(5)
        dm = mz._device()[1]
        return dm.resident_stats(), dm.queue_stats(), mz.last_run["accepted"]

    plain, _q0, acc0 = run(False)
    pen, q1, acc1 = run(True)
    assert plain["steps"] > 0 and acc0 > 0, plain
    assert pen["steps"] == 0 and pen["launches"] == 0 and acc1 > 0, pen
    assert q1["rounds"] == 0 and q1["mismatches"] == 0, q1


def test_breakdown_reports_the_three_modules_on_their_own():
    z = np.load(os.path.join(GOLD, BOTH))
    mesh = _traj_mesh(z)
    mz = _mz(mesh)
    out = mz.compute_energy_breakdown()
    P, T, edges = z["positions0"], z["tri"], z["edges"]
    gp, eo = ast.literal_eval(str(z["gp"])), ast.literal_eval(str(z["eopts"]))
    A = 0.5 * np.linalg.norm(np.cross(P[T[:, 1]] - P[T[:, 0]], P[T[:, 2]] - P[T[:, 0]]), axis=1).sum()
    rim = sorted(eo)
    ln = np.linalg.norm(P[edges[rim, 1]] - P[edges[rim, 0]], axis=1)
    e_line = gp["line_tension"] * ln.sum()
    e_pen = float(np.sum(0.5 * gp["edge_stiffness"] * (ln - np.array([eo[k]["target_length"] for k in rim])) ** 2))
    tot = A + e_line + e_pen
    assert set(out) == {"surface", "line_tension", "edge_length_penalty"}
    assert abs(out["line_tension"] - e_line) <= 1e-12 * e_line
    assert abs(out["edge_length_penalty"] - e_pen) <= 1e-12 * e_pen
    assert abs(out["surface"] - A) <= 1e-12 * tot
    assert abs(mz.compute_energy() - tot) <= 1e-12 * tot


def test_c_abi_refusals_and_module_off_is_unchanged():
    from membrane_solver_amd import meshgen

    P, T = meshgen.icosphere(4)
    t, h = _all_sides(T)
    t, h = t[::3], h[::3]
    l0 = 0.9 * np.linalg.norm(P[h] - P[t], axis=1)
    k = 35.0
    dm = DeviceMesh(P, T)
    dm.set_deterministic(True)  # (the surface gradient repeats bit for bit only with fixed-order sums)
    dm.set_surface_tension(np.ones(len(T)))
    dm.set_params(modules=L.MS_MOD_SURFACE)
    e0, g0 = dm.energy_and_gradient(raw=True)
    dm.set_edge_length_penalty(t, h, l0, k)
    e1, g1 = dm.energy_and_gradient(raw=True)
    assert np.array_equal(e1, e0) and np.array_equal(g1, g0)  # tables alone switch nothing on
    assert dm.edge_penalty_stats()["energy_launches"] == 0
    for bad in (-1, len(P)):
        with pytest.raises(L.MembraneHipError, match="out of range"):
            dm.set_edge_length_penalty(np.array([0, bad]), np.array([1, 2]), np.array([1.0, 1.0]), k)
        with pytest.raises(L.MembraneHipError, match="out of range"):
            dm.set_edge_length_penalty(np.array([0, 1]), np.array([1, bad]), np.array([1.0, 1.0]), k)
    with pytest.raises(L.MembraneHipError, match="target_length must be finite"):
        dm.set_edge_length_penalty(np.array([0]), np.array([1]), np.array([np.inf]), k)
    with pytest.raises(L.MembraneHipError, match="edge_stiffness must be finite"):
        dm.set_edge_length_penalty(np.array([0]), np.array([1]), np.array([1.0]), np.nan)
    # (a refused call leaves no tables behind)
    dm.set_params(modules=L.MS_MOD_SURFACE | L.MS_MOD_EDGE_LENGTH_PENALTY)
    e2, g2 = dm.energy_and_gradient(raw=True)
    assert np.array_equal(e2, e0) and np.array_equal(g2, g0) and dm.edge_penalty_energy() == 0.0
    with pytest.raises(L.MembraneHipError, match="edge_length_penalty together with a tilt-family module"):
        dm.set_params(modules=L.MS_MOD_SURFACE | L.MS_MOD_EDGE_LENGTH_PENALTY | L.MS_MOD_TILT)
    dm.set_params(modules=L.MS_MOD_SURFACE | L.MS_MOD_EDGE_LENGTH_PENALTY)
    with pytest.raises(L.MembraneHipError, match="edge_length_penalty module is not sharded"):
        dm.shard_step(stepper=L.MS_STEPPER_GD, step_size=1e-3)
    dm.set_edge_length_penalty(t, h, l0, k)
    e3, g3 = dm.energy_and_gradient(raw=True)
    vec = P[h] - P[t]
    ln = np.linalg.norm(vec, axis=1)
    e_pen = float(np.sum(0.5 * k * (ln - l0) ** 2))
    g_pen = np.zeros_like(P)
    f = (k * (ln - l0) / ln)[:, None] * vec
    np.add.at(g_pen, h, f)
    np.add.at(g_pen, t, -f)
    assert abs(dm.edge_penalty_energy() - e_pen) <= 1e-12 * e_pen
    assert abs(e3[0] - (e0[0] + e_pen)) <= 1e-12 * e3[0]
    np.testing.assert_allclose(g3, g0 + g_pen, rtol=0, atol=1e-10 * np.abs(g3).max())
    # targets above the lengths: the force changes sign with L - L0
    dm.set_edge_length_penalty(t, h, 1.1 * ln, k)
    _e, g_up = dm.energy_and_gradient(raw=True)
    f = (k * (-0.1 * ln) / ln)[:, None] * vec
    g_pen = np.zeros_like(P)
    np.add.at(g_pen, h, f)
    np.add.at(g_pen, t, -f)
    np.testing.assert_allclose(g_up, g0 + g_pen, rtol=0, atol=1e-10 * np.abs(g_up).max())
    dm.set_edge_length_penalty(t, h, l0, 0.0)  # k == 0: tables that hold no edge
    e5, g5 = dm.energy_and_gradient(raw=True)
    assert np.array_equal(e5, e0) and np.array_equal(g5, g0) and dm.edge_penalty_energy() == 0.0
    dm.set_edge_length_penalty(t, h, l0, k)
    dm.set_edge_length_penalty()  # cleared (NULL tail): the module bit alone contributes nothing
    e4, g4 = dm.energy_and_gradient(raw=True)
    assert np.array_equal(e4, e0) and np.array_equal(g4, g0)
    dm.close()
    d2 = DeviceMesh(P, T, shard_rank=0, shard_count=2)
    try:
        with pytest.raises(L.MembraneHipError, match="edge_length_penalty module is not sharded"):
            d2.set_params(modules=L.MS_MOD_SURFACE | L.MS_MOD_EDGE_LENGTH_PENALTY)
        with pytest.raises(L.MembraneHipError, match="edge_length_penalty module is not sharded"):
            d2.set_edge_length_penalty(t, h, l0, k)
    finally:
        d2.close()


def test_retiled_mesh_starts_without_tables():
    """Refinement re-uploads the mesh into a new context: the old tables are gone, and the Minimizer resolves the
    targets again for the new topology (here: none left, so the module contributes nothing)."""
    z = np.load(os.path.join(GOLD, "traj_ico4_gd_edgepen_surface_backtrack.npz"))
    mesh = _traj_mesh(z)
    mz = _mz(mesh)
    E0 = mz.compute_energy()
    assert mz._device()[1].modules & L.MS_MOD_EDGE_LENGTH_PENALTY
    mesh.edge_rows, mesh.edge_options = np.zeros((0, 2), dtype=np.int64), {}
    mesh.replace_topology(z["positions0"], z["tri"])
    mz.refresh_modules()
    E1 = mz.compute_energy()
    dm = mz._device()[1]
    assert not dm.modules & L.MS_MOD_EDGE_LENGTH_PENALTY and dm.edge_penalty_stats()["energy_launches"] == 0
    assert E1 < E0


def test_changed_targets_are_uploaded_again():
    """The upload is keyed on the targets: rewriting them in place (what the "fix edges" command does) reaches the
    device at the next evaluation without refresh_modules()."""
    z = np.load(os.path.join(GOLD, "traj_ico4_gd_edgepen_surface_backtrack.npz"))
    mesh = _traj_mesh(z)
    mz = _mz(mesh)
    before = mz.compute_energy_breakdown()["edge_length_penalty"]
    assert before > 0.0
    P, edges = z["positions0"], z["edges"]
    for k, o in mesh.edge_options.items():
        o["target_length"] = float(np.linalg.norm(P[edges[k, 1]] - P[edges[k, 0]]))
    after = mz.compute_energy_breakdown()["edge_length_penalty"]
    assert after <= 1e-24 * before  # every edge at its target
    mz.global_params.set("edge_stiffness", 0.0)
    mz.compute_energy()
    assert not mz._device()[1].modules & L.MS_MOD_EDGE_LENGTH_PENALTY


def _np_edge_terms(P, t, h, coef_of_len):
    """-> (lengths, gradient (nv,3)) of sum f(|e|) over the edges, coef_of_len(len) = f'(len)."""
    vec = P[h] - P[t]
    ln = np.linalg.norm(vec, axis=1)
    g = np.zeros_like(P)
    np.add.at(g, t, -(coef_of_len(ln) / ln)[:, None] * vec)
    np.add.at(g, h, (coef_of_len(ln) / ln)[:, None] * vec)
    return ln, g


@pytest.mark.parametrize("fixed_order", [False, True])
def test_the_two_edge_terms_keep_their_own_tables(fixed_order):
    """line_tension on edges 0..299 and edge_length_penalty on edges 250..479 of a several-tile icosphere (two
    workgroups of k_line_energy, one of k_edgepen_energy): each term's own energy to 1e-12 relative and the two terms'
    gradient to 1e-10 of max|g| against NumPy (the bars of test_module_energy_and_gradient_match_reference); clearing one
    term leaves the other's energy and gradient bit for bit; each term's statistics count its own launches."""
    from membrane_solver_amd import meshgen

    P0, T = meshgen.icosphere(4)
    P = meshgen.smooth_displace(P0)
    tri = np.asarray(T, dtype=np.int64)
    a = np.concatenate([tri[:, 0], tri[:, 1], tri[:, 2]])
    b = np.concatenate([tri[:, 1], tri[:, 2], tri[:, 0]])
    key = np.unique(np.minimum(a, b) * len(P) + np.maximum(a, b))
    et, eh = (key // len(P)).astype(np.int32), (key % len(P)).astype(np.int32)
    assert len(P) == 162 and len(et) == 480
    lt, lh, gam = et[:300], eh[:300], 0.5 + 0.01 * np.arange(300)
    pt, ph, l0, k = et[250:], eh[250:], 0.2 + 0.001 * np.arange(230), 3.0
    ln_l, g_line = _np_edge_terms(P, lt, lh, lambda ln: gam)
    ln_p, g_pen = _np_edge_terms(P, pt, ph, lambda ln: k * (ln - l0))
    e_line, e_pen = float((gam * ln_l).sum()), float((0.5 * k * (ln_p - l0) ** 2).sum())
    both = L.MS_MOD_LINE_TENSION | L.MS_MOD_EDGE_LENGTH_PENALTY

    def fresh():
        dm = DeviceMesh(P, T, tile_vertices=64)
        dm.set_deterministic(fixed_order)
        dm.set_surface_tension(np.ones(len(T)))
        return dm

    def alone(dm, bit):
        dm.set_params(modules=bit)
        e, g = dm.energy_and_gradient(raw=True)
        return e.copy(), g.copy()

    # a run where the other term was never set
    dm = fresh()
    dm.set_edge_length_penalty(pt, ph, l0, k)
    pen_only = alone(dm, L.MS_MOD_EDGE_LENGTH_PENALTY) + (dm.edge_penalty_energy(),)
    dm.close()
    dm = fresh()
    dm.set_line_tension(lt, lh, gam)
    line_only = alone(dm, L.MS_MOD_LINE_TENSION) + (dm.line_energy(),)
    dm.close()

    dm = fresh()
    assert dm.tile_stats()["n_tiles"] > 1
    dm.set_params(modules=L.MS_MOD_SURFACE)
    e0, g0 = dm.energy_and_gradient(raw=True)
    dm.set_line_tension(lt, lh, gam)
    dm.set_edge_length_penalty(pt, ph, l0, k)
    assert dm.line_stats()["energy_launches"] == 0 and dm.edge_penalty_stats()["energy_launches"] == 0
    dm.set_params(modules=L.MS_MOD_SURFACE | both)
    e1, g1 = dm.energy_and_gradient(raw=True)
    E_line, E_pen = dm.line_energy(), dm.edge_penalty_energy()
    scale = np.abs(g_line + g_pen).max()
    print(f"fixed_order={fixed_order}: dE_line/E={abs(E_line - e_line) / e_line:.3e} dE_pen/E={abs(E_pen - e_pen) / e_pen:.3e} "
          f"dg/max|g|={np.abs(g1 - g0 - g_line - g_pen).max() / scale:.3e}")
    assert abs(E_line - e_line) <= 1e-12 * e_line
    assert abs(E_pen - e_pen) <= 1e-12 * e_pen
    assert abs(e1[0] - (e0[0] + e_line + e_pen)) <= 1e-12 * abs(e1[0])
    assert np.abs((g1 - g0) - (g_line + g_pen)).max() <= 1e-10 * scale
    # each term counts the launches of its own lane
    count = lambda st: (st["energy_launches"], st["grad_launches"])  # noqa: E731
    n_line, n_pen = count(dm.line_stats()), count(dm.edge_penalty_stats())
    assert n_line == n_pen and min(n_line) >= 1
    alone(dm, L.MS_MOD_LINE_TENSION)
    assert count(dm.line_stats()) == (2 * n_line[0], 2 * n_line[1]) and count(dm.edge_penalty_stats()) == n_pen
    # line_tension cleared: the penalty's tables are untouched
    dm.set_line_tension()
    e, g = alone(dm, L.MS_MOD_EDGE_LENGTH_PENALTY)
    assert np.array_equal(e, pen_only[0]) and np.array_equal(g, pen_only[1])
    assert dm.edge_penalty_energy() == pen_only[2] and dm.line_energy() == 0.0
    e, g = alone(dm, both)  # (the cleared term's bit contributes nothing)
    assert np.array_equal(e, pen_only[0]) and np.array_equal(g, pen_only[1])
    # and the other way round
    dm.set_line_tension(lt, lh, gam)
    dm.set_edge_length_penalty()
    e, g = alone(dm, L.MS_MOD_LINE_TENSION)
    assert np.array_equal(e, line_only[0]) and np.array_equal(g, line_only[1])
    assert dm.line_energy() == line_only[2] and dm.edge_penalty_energy() == 0.0
    e, g = alone(dm, both)
    assert np.array_equal(e, line_only[0]) and np.array_equal(g, line_only[1])
    dm.close()
