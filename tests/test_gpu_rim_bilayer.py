"""tilt_rim_source_bilayer on the HIP path (csrc/ms_rim.hip, k_rim_apply2): the plugin against the reference's module on
every case of rim_bilayer_cases.npz and the 264-row rim, the device equivalence with tilt_rim_source_in + _out, the slot
rules next to tilt_out / tilt_rim_source_out / tilt_coupling, the deck's leaflet relaxation and three reference
trajectories (tools/gen_golden_rim_bilayer.py).  Tolerances are the rim source tests': |E - E_ref| <= 1e-12 E_scale with
E_scale = sum |gamma L dots| (the energy is a signed sum that may cancel), every tilt-gradient entry within 1e-10 of the
largest; relaxation and trajectories within max(1e-12, 10 x noise), noise being what a 1e-13 perturbation of the start
moves in the reference's own run (the fixtures record it)."""

import json

import numpy as np
import pytest

from conftest import load_golden, relerr

pytestmark = pytest.mark.gpu

NAME = "tilt_rim_source_bilayer"
CASES = load_golden("rim_bilayer_cases.npz")
NAMES = [str(n) for n in CASES["names"]]
TRAJ = {"traj_disk6_gd_rimbilayer_nested_cg.npz": "gd", "traj_disk6_cg_rimbilayer_coupled_gd.npz": "cg",
        "traj_disk5_gd_rimbilayer_follow_fastpath.npz": "gd"}


def _opts(text):
    return {int(k): v for k, v in json.loads(str(text)).items()}


def _bar(g, key):
    return max(1e-12, 10.0 * float(g[key]))


def _case_mesh(name, tile=0):
    from membrane_solver_amd.core.parameters import GlobalParameters
    from membrane_solver_amd.geometry.mesh import ArrayMesh, mirror_for

    g = CASES
    gp = GlobalParameters(json.loads(str(g[name + "__gp"])))
    mesh = ArrayMesh(g[name + "__positions"], g[name + "__tri"], global_parameters=gp, tilts_in=g[name + "__tilts_in"],
                     tilts_out=g[name + "__tilts_out"], edges=g[name + "__edges"], vertex_options=_opts(g[name + "__vopts"]),
                     edge_options=_opts(g[name + "__eopts"]))
    if tile:
        mirror_for(mesh, tile_vertices=tile)  # (stashed on the mesh: the plugin evaluates on this mirror)
    return mesh, gp


def _module():
    from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager

    return EnergyModuleManager([NAME]).get_module(NAME)


@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("tile", [0, 64])
@pytest.mark.parametrize("name", NAMES)
def test_plugin_matches_reference(name, tile, deterministic, monkeypatch):
    """Array, energy-only and dict APIs; default tiles and 64-vertex tiles (several tiles, the rim crossing tile
    boundaries, the row permutation); LDS-atomic and fixed-order sums."""
    from membrane_solver_amd.core.parameters import ParameterResolver

    if deterministic:
        monkeypatch.setenv("MS_DETERMINISTIC", "1")
    g = CASES
    mesh, gp = _case_mesh(name, tile)
    res = ParameterResolver(gp)
    module = _module()
    pos, tin, tout = g[name + "__eval_positions"], g[name + "__tilts_in"], g[name + "__tilts_out"]
    E_ref, tg_ref, scale = float(g[name + "__E"]), g[name + "__tilt_grad"], float(g[name + "__E_scale"])
    sentinel = np.arange(pos.size, dtype=np.float64).reshape(pos.shape)
    grad = sentinel.copy()
    gi, go = np.zeros_like(pos), np.zeros_like(pos)
    E = module.compute_energy_and_gradient_array(mesh, gp, res, positions=pos, index_map=mesh.vertex_index_to_row,
                                                 grad_arr=grad, tilts_in=tin, tilts_out=tout, tilt_in_grad_arr=gi,
                                                 tilt_out_grad_arr=go)
    E2 = module.compute_energy_array(mesh, gp, res, positions=pos, index_map=mesh.vertex_index_to_row, tilts_in=tin,
                                     tilts_out=tout)
    print(name, "E", E, "ref", E_ref, "|dE|/scale", abs(E - E_ref) / max(scale, 1e-300), "relerr tg", relerr(gi, tg_ref))
    assert np.array_equal(grad, sentinel), "the module has no shape gradient: grad_arr must stay as it is"
    assert abs(E - E_ref) <= 1e-12 * scale
    assert abs(E2 - E_ref) <= 1e-12 * scale
    assert np.array_equal(gi, go), "both leaflets get the same coefficient rows"
    if tg_ref.any():
        assert np.max(np.abs(gi - tg_ref)) <= 1e-10 * np.max(np.abs(tg_ref))
        assert np.array_equal(np.any(gi != 0.0, axis=1), np.any(tg_ref != 0.0, axis=1))
    else:  # the off cases: exact zeros, nothing written
        assert E == 0.0 and E2 == 0.0 and not gi.any() and not go.any()
    if tile and len(pos) > tile and tg_ref.any():  # (an off case returns before it touches the device)
        assert mesh._hip_mirror.dm.tile_stats()["n_tiles"] > 1
    if np.array_equal(pos, g[name + "__positions"]):  # the dict API evaluates the mesh's own positions and tilts
        Ed, gd, tgi, tgo = module.compute_energy_and_gradient(mesh, gp, res)
        assert abs(Ed - E_ref) <= 1e-12 * scale and gd == {}
        assert sorted(tgi) == sorted(tgo) == [int(r) for r in np.flatnonzero(np.any(tg_ref != 0.0, axis=1))]
        for r, row in tgi.items():
            assert np.max(np.abs(row - tg_ref[r])) <= 1e-10 * np.max(np.abs(tg_ref))
            assert np.array_equal(row, tgo[r])
        assert module.compute_energy_and_gradient(mesh, gp, res, compute_gradient=False) == (Ed, {})


@pytest.mark.parametrize("deterministic", [False, True])
def test_large_rim_uses_a_second_workgroup(deterministic):
    """264 rim rows on ~23 tiles: grid = min(tiles, ceil(264 / 256)) = 2.  The slot is DEFINED: an evaluation with
    tilt_out before it leaves every cell of the slot non-zero, and the cells past the grid must be zeroed."""
    from membrane_solver_amd import _lib as L
    from membrane_solver_amd import meshgen
    from membrane_solver_amd.device import DeviceMesh

    g = load_golden("rim_bilayer_large.npz")
    P, T, B = meshgen.disk_patch(int(g["rings"]))
    rows = g["rim_rows"].astype(np.int64)
    assert np.array_equal(np.flatnonzero(B), rows) and len(rows) == 264
    gp = json.loads(str(g["gp"]))
    tin, tout = np.zeros_like(P), np.zeros_like(P)
    tin[rows], tout[rows] = g["tilts_in_rim"], g["tilts_out_rim"]
    on_ring = set(map(int, rows))
    tri = np.asarray(T)
    edges = {tuple(sorted((int(a), int(b)))) for f in tri for a, b in ((f[0], f[1]), (f[1], f[2]), (f[2], f[0]))
             if int(a) in on_ring and int(b) in on_ring}
    # boundary edges only: both ends on the ring and a side of exactly one triangle
    cnt = {}
    for f in tri:
        for a, b in ((f[0], f[1]), (f[1], f[2]), (f[2], f[0])):
            k = tuple(sorted((int(a), int(b))))
            cnt[k] = cnt.get(k, 0) + 1
    bnd = sorted(k for k in edges if cnt[k] == 1)
    assert len(bnd) == 264
    dm = DeviceMesh(P, T)
    dm.set_deterministic(deterministic)
    assert dm.tile_stats()["n_tiles"] >= 2  # (so the launch has min(tiles, 2) = 2 workgroups)
    dm.set_leaflet_tilts("in", tin, tilt_modulus=1.0)
    dm.set_leaflet_tilts("out", tout + 0.1, tilt_modulus=1.0)  # every tile's cell of the outer slot non-zero
    dm.set_params(modules=L.MS_MOD_TILT_IN | L.MS_MOD_TILT_OUT)
    assert dm.energy()[3] > 0.0
    dm.set_leaflet_tilts("out", tout, tilt_modulus=1.0)
    dm.set_rim_source_bilayer([k[0] for k in bnd], [k[1] for k in bnd], np.full(len(bnd), gp["tilt_rim_source_strength"]),
                              center=gp["tilt_rim_source_center"])
    dm.set_params(modules=L.MS_MOD_TILT_RIM_SOURCE_BILAYER)
    scale, E_ref = float(g["E_scale"]), float(g["E"])
    e = dm.energy()
    E, gi, go = dm.leaflet_tilt_energy_and_gradient()
    print("large rim: E", E, e[3], "ref", E_ref, "own", dm.rim_source_bilayer_energy())
    assert abs(e[3] - E_ref) <= 1e-12 * scale and abs(E - E_ref) <= 1e-12 * scale
    assert abs(dm.rim_source_bilayer_energy() - E_ref) <= 1e-12 * scale
    assert np.array_equal(gi, go)
    assert np.max(np.abs(gi[rows] - g["tilt_grad_rim"])) <= 1e-10 * np.max(np.abs(g["tilt_grad_rim"]))
    rest = np.ones(len(P), bool)
    rest[rows] = False
    assert not gi[rest].any()
    assert dm.rim_source_bilayer_stats()["apply_launches"] == 2
    dm.close()


@pytest.mark.parametrize("name", ["disk6_b_ring3_all_per_edge", "disk6_a_boundary_global", "annulus_deck"])
@pytest.mark.parametrize("tile", [0, 64])
@pytest.mark.parametrize("with_tilt", [False, True])
def test_device_equivalence_with_the_two_leaflet_modules(name, tile, with_tilt):
    """One context with the bilayer tables against one with tilt_rim_source_in and _out loaded with the same gamma and
    frame: both tilt gradients bitwise equal, the energies equal to 1e-12 of scale, half the apply launches."""
    from membrane_solver_amd import _lib as L
    from membrane_solver_amd.core.parameters import ParameterResolver
    from membrane_solver_amd.device import DeviceMesh
    from membrane_solver_amd.modules.energy import leaflet_common as lc

    g = CASES
    mesh, gp = _case_mesh(name)
    prm = lc.rim_source_params(mesh, ParameterResolver(gp), gp, None)
    assert prm["normal"] == (0.0, 0.0, 1.0) and not prm["follow"]
    base = (L.MS_MOD_TILT_IN | L.MS_MOD_TILT_OUT) if with_tilt else 0
    got = {}
    for kind in ("bilayer", "pair"):
        dm = DeviceMesh(g[name + "__positions"], g[name + "__tri"], tile_vertices=tile)
        dm.set_deterministic(True)
        dm.set_leaflet_tilts("in", g[name + "__tilts_in"], tilt_modulus=1.3)
        dm.set_leaflet_tilts("out", g[name + "__tilts_out"], tilt_modulus=0.9)
        if kind == "bilayer":
            dm.set_rim_source_bilayer(**prm)
            dm.set_params(modules=base | L.MS_MOD_TILT_RIM_SOURCE_BILAYER)
        else:
            dm.set_leaflet_rim_source("in", **prm)
            dm.set_leaflet_rim_source("out", **prm)
            dm.set_params(modules=base | L.MS_MOD_TILT_RIM_SOURCE_IN | L.MS_MOD_TILT_RIM_SOURCE_OUT)
        E, gi, go = dm.leaflet_tilt_energy_and_gradient()
        launches = (dm.rim_source_bilayer_stats()["apply_launches"] if kind == "bilayer" else
                    dm.leaflet_rim_source_stats("in")["apply_launches"] + dm.leaflet_rim_source_stats("out")["apply_launches"])
        got[kind] = (E, gi, go, launches)
        dm.close()
    scale = float(g[name + "__E_scale"])
    (Eb, gib, gob, nb), (Ep, gip, gop, npair) = got["bilayer"], got["pair"]
    print(name, "E bilayer", Eb, "pair", Ep, "launches", nb, npair)
    assert np.array_equal(gib, gip) and np.array_equal(gob, gop)
    assert abs(Eb - Ep) <= 1e-12 * (scale + abs(Ep))
    assert nb == 1 and npair == 2


_LANES = {  # (base modules, what the bilayer pass finds in the outer slot's cells)
    "tilt_out_on": (["TILT_IN", "TILT_OUT", "TILT_SMOOTH_IN", "TILT_SMOOTH_OUT"], "add"),
    "tilt_out_off": (["TILT_IN", "TILT_SMOOTH_IN", "TILT_SMOOTH_OUT"], "define"),
    "rim_out_add": (["TILT_IN", "TILT_OUT", "TILT_RIM_SOURCE_OUT"], "add"),
    "rim_out_defines": (["TILT_SMOOTH_IN", "TILT_RIM_SOURCE_OUT"], "add"),
    "coupling_add": (["TILT_IN", "TILT_OUT", "TILT_COUPLING"], "add"),
    "coupling_define": (["TILT_IN", "TILT_COUPLING"], "define"),
}


@pytest.mark.parametrize("lane", sorted(_LANES))
@pytest.mark.parametrize("tile", [0, 64])
def test_evaluations_differ_by_the_module(lane, tile):
    """With and without the bit: energies[:3] bit-identical; energies[3], the leaflet evaluation and the module's own
    energy differ by the reference's energy; both tilt gradients by the reference's rows."""
    from membrane_solver_amd import _lib as L
    from membrane_solver_amd.core.parameters import ParameterResolver
    from membrane_solver_amd.device import DeviceMesh
    from membrane_solver_amd.modules.energy import leaflet_common as lc

    name = "disk6_b_ring3_all_per_edge"
    g = CASES
    mesh, gp = _case_mesh(name)
    prm = lc.rim_source_params(mesh, ParameterResolver(gp), gp, None)
    dm = DeviceMesh(g[name + "__positions"], g[name + "__tri"], tile_vertices=tile)
    dm.set_leaflet_tilts("in", g[name + "__tilts_in"], tilt_modulus=1.3, smoothness=0.7)
    dm.set_leaflet_tilts("out", g[name + "__tilts_out"], tilt_modulus=0.9, smoothness=0.4)
    dm.set_rim_source_bilayer(**prm)
    dm.set_leaflet_rim_source("out", **dict(prm, gamma=0.5 * prm["gamma"], center=(0.1, 0.0, 0.0)))
    dm.set_tilt_coupling(0.8, -1)
    base = 0
    for m in _LANES[lane][0]:
        base |= getattr(L, "MS_MOD_" + m)
    bit = L.MS_MOD_TILT_RIM_SOURCE_BILAYER
    scale, tg_ref, E_ref = float(g[name + "__E_scale"]), g[name + "__tilt_grad"], float(g[name + "__E"])
    dm.set_params(modules=base)
    E0, gi0, go0 = dm.leaflet_tilt_energy_and_gradient()
    e0, g0 = dm.energy_and_gradient(want_grad=True, raw=True)
    dm.set_params(modules=base | bit)
    E1, gi1, go1 = dm.leaflet_tilt_energy_and_gradient()
    own_t = dm.rim_source_bilayer_energy()
    e1, g1 = dm.energy_and_gradient(want_grad=True, raw=True)  # (phase_gradient rewrites the slot behind k_tilt<1>)
    own = dm.rim_source_bilayer_energy()
    e2 = dm.energy()
    tol = 1e-12 * (scale + abs(E0))
    print(lane, tile, "dE", E1 - E0, e1[3] - e0[3], e2[3] - e0[3], "own", own, "ref", E_ref)
    assert abs((E1 - E0) - E_ref) <= tol and abs((e1[3] - e0[3]) - E_ref) <= tol and abs((e2[3] - e0[3]) - E_ref) <= tol
    assert abs(own - E_ref) <= 1e-12 * scale and abs(own_t - E_ref) <= 1e-12 * scale
    assert np.array_equal(e1[:3], e0[:3]) and np.array_equal(e2[:3], e0[:3])
    assert np.array_equal(g1, g0), "no shape gradient"
    big = max(np.max(np.abs(gi0)), np.max(np.abs(go0)))
    for d in (gi1 - gi0, go1 - go0):
        assert np.max(np.abs(d - tg_ref)) <= 1e-10 * np.max(np.abs(tg_ref)) + 1e-15 * big
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
    print("    finals: x", relerr(mesh.positions_view(), g["positions_final"]), "bar", _bar(g, "noise_positions"),
          "t", relerr(mesh.tilts_in_view(), g["tilts_in_final"]), relerr(mesh.tilts_out_view(), g["tilts_out_final"]),
          "bar", _bar(g, "noise_tilts"), "E", abs(res["energy"] - float(g["E_final"])) / abs(float(g["E_final"])),
          "bar", _bar(g, "noise_energy"))
    assert relerr(mesh.positions_view(), g["positions_final"]) <= _bar(g, "noise_positions")
    assert relerr(mesh.tilts_in_view(), g["tilts_in_final"]) <= _bar(g, "noise_tilts")
    assert relerr(mesh.tilts_out_view(), g["tilts_out_final"]) <= _bar(g, "noise_tilts")
    assert abs(res["energy"] - float(g["E_final"])) <= _bar(g, "noise_energy") * abs(float(g["E_final"]))


@pytest.mark.parametrize("fname", sorted(TRAJ))
def test_minimizer_reproduces_trajectory(fname):
    """The Python loop (observed steps) and ms_minimize: the reference's decisions and step sizes, energies and finals
    within the fixture's noise bar; the breakdown reports the module's own energy and sums to the total."""
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
            assert np.allclose(got[:, 2], ref[:, 2], rtol=_bar(g, "noise_energy"), atol=0)
            bd = mz.compute_energy_breakdown()
            assert abs(sum(bd.values()) - res["energy"]) <= 1e-12 * abs(res["energy"])
            assert abs(bd[NAME] - float(g["E_rim_final"])) <= _bar(g, "noise_energy") * abs(float(g["E_final"]))
        _check_finals(mesh, res, g)


def test_trajectory_with_small_tiles():
    g = load_golden("traj_disk6_cg_rimbilayer_coupled_gd.npz")
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


@pytest.mark.parametrize("fname", sorted(TRAJ))
def test_trajectory_is_bitwise_reproducible_in_fixed_order_mode(fname, monkeypatch):
    monkeypatch.setenv("MS_DETERMINISTIC", "1")
    g = load_golden(fname)
    a = _run_final(g, TRAJ[fname], tile=64)
    b = _run_final(g, TRAJ[fname], tile=64)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("fname", sorted(TRAJ))
def test_trajectory_without_the_interpreter_is_bitwise_equal(fname, monkeypatch):
    """MS_EXEC=0 (launch per kernel) against the default (one-tile interpreter, flushed before every rim launch)."""
    g = load_golden(fname)
    monkeypatch.setenv("MS_DETERMINISTIC", "1")
    a = _run_final(g, TRAJ[fname])
    monkeypatch.setenv("MS_EXEC", "0")
    b = _run_final(g, TRAJ[fname])
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


# ---------------------------------------------------------------------------------------------------------------------
def _relax(g, mods=None):
    from membrane_solver_amd.geometry.mesh import ArrayMesh
    from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager
    from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager
    from membrane_solver_amd.runtime.minimizer import Minimizer
    from membrane_solver_amd.runtime.steppers import GradientDescent

    mods = [str(m) for m in g["modules"]] if mods is None else mods
    cons = [str(m) for m in g["constraint_modules"]]
    mesh = ArrayMesh(g["positions"], g["tri"], fixed=g["fixed"], tilts_in=g["tilts_in0"], tilts_out=g["tilts_out0"],
                     tilt_fixed_in=g["tilt_fixed_in"], tilt_fixed_out=g["tilt_fixed_out"],
                     global_parameters=json.loads(str(g["gp_json"])), energy_modules=mods, constraint_modules=cons,
                     edges=g["edges"], vertex_options=_opts(g["vopts"]))
    mz = Minimizer(mesh, mesh.global_parameters, GradientDescent(), EnergyModuleManager(mods), ConstraintModuleManager(cons),
                   quiet=True)
    _mir, dm = mz._device()
    iters, evals = dm.relax_leaflet_tilts(**mz._tilt_relax_params())
    return mz, dm, iters, evals


def test_deck_relaxation_matches_reference():
    """The nested leaflet relaxation of kozlov_1disk_3d_tensionless_bilayer_source.yaml with its module list and its pins
    (84 vertices, 12 rim edges, gamma 50), tilt_inner_steps capped where the reference's counts are stable."""
    g = load_golden("rim_bilayer_relax.npz")
    mz, dm, iters, evals = _relax(g)
    assert dm.modules & mz_bit()
    tin, tout = dm.get_leaflet_tilts("in"), dm.get_leaflet_tilts("out")
    E = float(dm.energy().sum())
    own = dm.rim_source_bilayer_energy()
    bar_t, bar_e = _bar(g, "noise_tilts"), _bar(g, "noise_energy")
    print("iters", iters, "evals", evals, "ref", int(g["n_gradient_evaluations"]), int(g["n_energy_evaluations"]), "E", E,
          "ref", float(g["E_total"]), "relerr", relerr(tin, g["tilts_in_final"]), relerr(tout, g["tilts_out_final"]),
          "bars", bar_t, bar_e, "own", own, float(g["E_rim"]))
    assert iters == int(g["n_gradient_evaluations"]) - 1 == int(g["tilt_inner_steps"])
    assert evals == int(g["n_evaluations"])
    assert relerr(tin, g["tilts_in_final"]) <= bar_t and relerr(tout, g["tilts_out_final"]) <= bar_t
    assert abs(E - float(g["E_total"])) <= bar_e * abs(float(g["E_total"]))
    assert abs(own - float(g["E_rim"])) <= bar_e * abs(float(g["E_rim"]))
    st = dm.exec_stats()
    assert st["relax_fused"] == 0 and st["relax_programs"] == 0
    rs = dm.rim_source_bilayer_stats()
    # the coefficients once for the whole relaxation, one apply per evaluation of it; the evaluation that leaves the
    # bending_tilt record before the loop and dm.energy() above form theirs in the apply launch
    assert rs["coef_launches"] == 1 and rs["frame_launches"] == 0
    assert evals + 1 <= rs["apply_launches"] <= evals + 2
    bd = mz.compute_energy_breakdown()
    assert abs(bd[NAME] - float(g["E_rim"])) <= bar_e * abs(float(g["E_rim"]))
    assert abs(sum(bd.values()) - float(g["E_total"])) <= bar_e * abs(float(g["E_total"]))


def mz_bit():
    from membrane_solver_amd import _lib as L

    return L.MS_MOD_TILT_RIM_SOURCE_BILAYER


def test_context_without_the_module_keeps_its_fast_lanes():
    """The same deck without the module: the fused evaluator and the relaxation program run as before."""
    g = load_golden("rim_bilayer_relax.npz")
    mods = [str(m) for m in g["modules"] if str(m) != NAME]
    _mz, dm, _iters, evals = _relax(g, mods)
    st = dm.exec_stats()
    assert evals > 0 and st["relax_fused"] > 0 and st["relax_programs"] > 0
    assert dm.rim_source_bilayer_stats()["apply_launches"] == 0


def test_search_passes_still_run_without_the_module():
    """A multi-tile leaflet relaxation without the module still takes the search / gradient passes of ms_tsearch.inc;
    with it they decline."""
    g = load_golden("traj_disk6_gd_rimbilayer_nested_cg.npz")
    counts = {}
    for with_module in (False, True):
        g2 = dict(g)
        if not with_module:
            g2["modules"] = np.array([m for m in g["modules"] if str(m) != NAME])
        _mesh, mz, _ = _minimizer(g2, "gd", observe=False, tile=64)
        _mir, dm = mz._device()
        assert bool(dm.modules & mz_bit()) == with_module
        before = dm.tsearch_stats()["passes"]
        dm.relax_leaflet_tilts(**mz._tilt_relax_params())
        counts[with_module] = dm.tsearch_stats()["passes"] - before
    assert counts[False] > 0 and counts[True] == 0


def test_refusals():
    from membrane_solver_amd import _lib as L
    from membrane_solver_amd import meshgen
    from membrane_solver_amd.device import DeviceMesh

    P, T = meshgen.icosphere(3)
    dm = DeviceMesh(P, T)
    dm.set_leaflet_tilts("in", np.zeros_like(P), tilt_modulus=1.0)
    dm.set_leaflet_tilts("out", np.zeros_like(P))
    bit = L.MS_MOD_TILT_RIM_SOURCE_BILAYER
    with pytest.raises(L.MembraneHipError, match="never called"):  # the bit without tables
        dm.set_params(modules=L.MS_MOD_TILT_IN | bit)
        dm.energy()
    for bad in ({"gamma": [1.0, np.nan]}, {"center": (0.0, np.inf, 0.0)}, {"normal": (0.0, 0.0, 0.0)},
                {"normal": (np.nan, 0.0, 1.0)}, {"tail": [0, len(P)]}):
        kw = dict({"tail": [0, 1], "head": [1, 2], "gamma": [1.0, 1.0]}, **bad)
        with pytest.raises(L.MembraneHipError, match="ms_set_rim_source_bilayer"):
            dm.set_rim_source_bilayer(**kw)
    dm.set_rim_source_bilayer([0, 1], [1, 2], [1.0, 1.0], normal=(0.0, 0.0, 1.0), follow=True)
    with pytest.raises(L.MembraneHipError, match="single-field"):
        dm.set_params(modules=L.MS_MOD_TILT | bit)
    dm.set_params(modules=L.MS_MOD_SURFACE | L.MS_CON_VOLUME | L.MS_MOD_TILT_IN | bit, target_volume=4.0)
    with pytest.raises(L.MembraneHipError, match="tilt_rim_source_bilayer in follow mode"):
        dm.step(stepper=L.MS_STEPPER_GD, step_size=1e-3, tol=0.0, enforce_volume=1)
    r = dm.step(stepper=L.MS_STEPPER_GD, step_size=1e-3, tol=0.0)  # (without the enforcer the step runs)
    assert np.isfinite(r.energy)
    dm.set_rim_source_bilayer(None)  # cleared: the bit is refused again
    with pytest.raises(L.MembraneHipError, match="never called"):
        dm.energy()
    dm.close()
