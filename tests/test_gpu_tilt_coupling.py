"""tilt_coupling on the HIP path (csrc/ms_couple.hip): the plugin against the reference's module on every case of
tilt_coupling_cases.npz, the leaflet evaluation with and without the module, the frozen (k_couple_vec) against the tile
form (k_couple<1>) of the same relaxation, the milestone-B tracking relaxation and three reference trajectories
(tools/gen_golden_tilt_coupling.py).  Tolerances are the leaflet tests': |E - E_ref| <= 1e-12 E_scale with
E_scale = sum |coeff_f| A_f, relerr < 1e-10 for the shape gradient and both tilt gradients (for the cancelling cases
against the scales of the uncancelled field), exact zeros where the reference has exact zeros."""

import json

import numpy as np
import pytest

from conftest import load_golden, relerr

pytestmark = pytest.mark.gpu

CASES = load_golden("tilt_coupling_cases.npz")
NAMES = [str(n) for n in CASES["names"]]
TRAJ = {"traj_disk6_gd_coupling_nested_cg.npz": "gd", "traj_disk6_cg_coupling_coupled_gd.npz": "cg",
        "traj_ico4_gd_coupling_surface_backtrack.npz": "gd"}


def _case(name):
    g = CASES
    mesh = str(g[name + "__mesh"])
    what = str(g[name + "__what"])
    P, T = g["mesh__" + mesh + "__positions"], g["mesh__" + mesh + "__tri"]
    pos = g[name + "__eval_positions"] if what == "moved" else P
    sign = int(g[name + "__sign"])
    tgo = g[name + "__tilt_grad_out"]
    return {"P": P, "T": T, "pos": pos, "what": what, "gp": json.loads(str(g[name + "__gp"])), "sign": sign,
            "k_c": float(g[name + "__k_c"]), "tin": g[name + "__tilts_in"], "tout": g[name + "__tilts_out"],
            "E": float(g[name + "__E"]), "grad": g[name + "__grad"], "tgo": tgo, "tgi": sign * tgo,
            "E_scale": float(g[name + "__E_scale"]), "g_scale": float(g[name + "__grad_scale"]),
            "tg_scale": float(g[name + "__tilt_grad_scale"])}


def _case_mesh(c, tile=0):
    from membrane_solver_amd.core.parameters import GlobalParameters
    from membrane_solver_amd.geometry.mesh import ArrayMesh, mirror_for

    gp = GlobalParameters(c["gp"])
    mesh = ArrayMesh(c["P"], c["T"], global_parameters=gp, tilts_in=c["tin"], tilts_out=c["tout"])
    if tile:
        mirror_for(mesh, tile_vertices=tile)  # (stashed on the mesh: the plugin evaluates on this mirror)
    return mesh, gp


def _close(got, ref, scale, what=""):
    """relerr < 1e-10 against the reference's own scale -- for a cancelling case, the uncancelled field's"""
    err = float(np.max(np.abs(got - ref))) / max(scale, 1e-300)
    print("   ", what, "max|d| / scale", err)
    return err < 1e-10


def _check_case(name, tile):
    from membrane_solver_amd.core.parameters import ParameterResolver
    from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager

    c = _case(name)
    mesh, gp = _case_mesh(c, tile)
    res = ParameterResolver(gp)
    module = EnergyModuleManager(["tilt_coupling"]).get_module("tilt_coupling")
    assert module.USES_TILT_LEAFLETS
    pos, tin, tout = c["pos"], c["tin"], c["tout"]
    kw = dict(positions=pos, index_map=mesh.vertex_index_to_row, tilts_in=tin, tilts_out=tout)
    grad, tgi, tgo = np.zeros_like(pos), np.zeros_like(pos), np.zeros_like(pos)
    E = module.compute_energy_and_gradient_array(mesh, gp, res, grad_arr=grad, tilt_in_grad_arr=tgi,
                                                 tilt_out_grad_arr=tgo, **kw)
    E2 = module.compute_energy_array(mesh, gp, res, **kw)
    print(name, "tile", tile, "E", E, "ref", c["E"], "|dE|/scale", abs(E - c["E"]) / max(c["E_scale"], 1e-300))
    if c["what"] == "off":  # exactly nothing
        assert E == 0.0 and E2 == 0.0 and not grad.any() and not tgi.any() and not tgo.any()
    else:
        assert abs(E - c["E"]) <= 1e-12 * c["E_scale"]
        assert abs(E2 - c["E"]) <= 1e-12 * c["E_scale"]
        assert _close(grad, c["grad"], c["g_scale"], "shape gradient")
        assert _close(tgo, c["tgo"], c["tg_scale"], "tilt gradient out")
        assert _close(tgi, c["tgi"], c["tg_scale"], "tilt gradient in")
        if tile and len(pos) > tile:  # (disk4 has 61 vertices: one tile of 64; disk6's 127 make two, ico4's 162 three)
            assert mesh._hip_mirror.dm.tile_stats()["n_tiles"] > 1
    # every output is optional: an array that is not handed over is not touched, the others are ADDED into
    sentinel = np.arange(pos.size, dtype=np.float64).reshape(pos.shape)
    only_in = sentinel.copy()
    E3 = module.compute_energy_and_gradient_array(mesh, gp, res, grad_arr=None, tilt_in_grad_arr=only_in, **kw)
    assert E3 == E2
    assert np.max(np.abs((only_in - sentinel) - tgi)) <= 1e-12 * max(c["tg_scale"], 1.0) + 4e-16 * sentinel.max()
    only_g = sentinel.copy()
    module.compute_energy_and_gradient_array(mesh, gp, res, grad_arr=only_g, tilt_out_grad_arr=None, **kw)
    assert np.max(np.abs((only_g - sentinel) - grad)) <= 1e-12 * max(c["g_scale"], 1.0) + 4e-16 * sentinel.max()
    if c["what"] == "off":
        assert np.array_equal(only_in, sentinel) and np.array_equal(only_g, sentinel)
    if c["what"] != "moved":  # the dict API evaluates the mesh's own positions and tilts; its tilt gradient is the OUT one
        Ed, gd, tgd = module.compute_energy_and_gradient(mesh, gp, res)
        assert sorted(gd) == sorted(tgd) == list(range(len(pos)))
        assert abs(Ed - c["E"]) <= 1e-12 * c["E_scale"]
        assert _close(np.array([gd[i] for i in range(len(pos))]), c["grad"], c["g_scale"], "dict shape gradient")
        assert _close(np.array([tgd[i] for i in range(len(pos))]), c["tgo"], c["tg_scale"], "dict tilt gradient (out)")
        if c["what"] == "off":
            assert Ed == 0.0 and not any(v.any() for v in gd.values()) and not any(v.any() for v in tgd.values())


@pytest.mark.parametrize("name", NAMES)
def test_plugin_matches_reference(name):
    _check_case(name, tile=0)


@pytest.mark.parametrize("name", NAMES)
def test_plugin_with_small_tiles(name):
    """64-vertex tiles: several tiles, halo rows of both tilt fields, the row permutation."""
    _check_case(name, tile=64)


def _device(c, tile, k_in=1.3, k_out=0.9):
    from membrane_solver_amd.device import DeviceMesh

    dm = DeviceMesh(c["pos"], c["T"], tile_vertices=tile)
    dm.set_leaflet_tilts("in", c["tin"], tilt_modulus=k_in, smoothness=0.7)
    dm.set_leaflet_tilts("out", c["tout"], tilt_modulus=k_out, smoothness=0.4)
    dm.set_tilt_coupling(c["k_c"], c["sign"])
    return dm


@pytest.mark.parametrize("name", ["disk6_difference", "ico4_sum_moved"])
@pytest.mark.parametrize("tile", [0, 64])
def test_leaflet_evaluation_differs_by_the_coupling(name, tile):
    """leaflet_tilt_energy_and_gradient() with and without the module differs by exactly the module's contribution, next
    to tilt_out (the sums are ADDED behind the magnitude pass) and without it (the cells are DEFINED)."""
    from membrane_solver_amd import _lib as L

    c = _case(name)
    dm = _device(c, tile)
    bit = L.MS_MOD_TILT_COUPLING
    for base in (L.MS_MOD_TILT_IN | L.MS_MOD_TILT_OUT | L.MS_MOD_TILT_SMOOTH_IN | L.MS_MOD_TILT_SMOOTH_OUT,
                 L.MS_MOD_TILT_IN | L.MS_MOD_TILT_SMOOTH_IN | L.MS_MOD_TILT_SMOOTH_OUT,
                 L.MS_MOD_TILT_SMOOTH_IN):
        dm.set_params(modules=base)
        E0, gi0, go0 = dm.leaflet_tilt_energy_and_gradient()
        e0, g0 = dm.energy_and_gradient(want_grad=True, raw=True)
        dm.set_params(modules=base | bit)
        E1, gi1, go1 = dm.leaflet_tilt_energy_and_gradient()
        own1 = dm.tilt_coupling_energy()
        e1, g1 = dm.energy_and_gradient(want_grad=True, raw=True)
        own2 = dm.tilt_coupling_energy()
        e2 = dm.energy()
        tol = 1e-12 * (c["E_scale"] + abs(E0))
        print(name, tile, hex(base), "dE", (E1 - E0) - c["E"], (e1[3] - e0[3]) - c["E"], "own", own1 - c["E"], own2 - c["E"])
        assert abs((E1 - E0) - c["E"]) <= tol and abs((e1[3] - e0[3]) - c["E"]) <= tol and abs((e2[3] - e0[3]) - c["E"]) <= tol
        assert abs(own1 - c["E"]) <= 1e-12 * c["E_scale"] and abs(own2 - c["E"]) <= 1e-12 * c["E_scale"]
        assert np.array_equal(e1[:3], e0[:3]) and np.array_equal(e2[:3], e0[:3])
        floor_i, floor_o, floor_g = (4e-16 * max(float(np.max(np.abs(a))), 0.0) for a in (gi0, go0, g0))
        assert np.max(np.abs((gi1 - gi0) - c["tgi"])) <= 1e-10 * c["tg_scale"] + floor_i
        assert np.max(np.abs((go1 - go0) - c["tgo"])) <= 1e-10 * c["tg_scale"] + floor_o
        assert np.max(np.abs((g1 - g0) - c["grad"])) <= 1e-10 * c["g_scale"] + floor_g
    dm.close()


def _relax_through(monkeypatch, c, tile, vec, mods, **rp):
    monkeypatch.setenv("MS_COUPLE_VEC", "1" if vec else "0")  # (read by ms_set_tilt_coupling)
    dm = _device(c, tile)
    dm.set_params(modules=mods)
    before = dm.tilt_coupling_stats()
    iters, evals = dm.relax_leaflet_tilts(**rp)
    st = dm.tilt_coupling_stats()
    tin, tout = dm.get_leaflet_tilts("in"), dm.get_leaflet_tilts("out")
    E, gi, go = dm.leaflet_tilt_energy_and_gradient()  # (outside the relaxation: the tile kernel)
    dm.close()
    return {"iters": iters, "evals": evals, "tin": tin, "tout": tout, "E": E, "gi": gi, "go": go,
            "launches": {k: st[k] - before[k] for k in st}}


@pytest.mark.parametrize("name", ["disk6_difference", "disk6z_zero_area_difference", "ico4_difference"])
@pytest.mark.parametrize("tile", [0, 64])
def test_frozen_form_agrees_with_the_tile_kernel(monkeypatch, name, tile):
    """The evaluations of one relaxation through k_couple_vec (positions frozen, the set-up launch's vertex areas) and
    the same ones forced through k_couple<1>: same decisions, tilts within the module tolerances.  On the case with two
    facets of area exactly 0 the unmasked vertex areas are the masked ones."""
    from membrane_solver_amd import _lib as L

    c = _case(name)
    both = L.MS_MOD_TILT_IN | L.MS_MOD_TILT_OUT
    # next to both magnitude modules (the cells are added to), alone (they are defined; the vertex areas come from the
    # set-up launch all the same), and -- away from the collapsed facets -- next to a smoothness module
    mods_list = [both | L.MS_MOD_TILT_COUPLING, L.MS_MOD_TILT_COUPLING]
    if c["what"] != "zero_area":
        mods_list.append(both | L.MS_MOD_TILT_SMOOTH_IN | L.MS_MOD_TILT_COUPLING)
    for mods in mods_list:
        rp = dict(solver="gd", max_iters=3, step_size=0.05, tol=0.0)
        a = _relax_through(monkeypatch, c, tile, True, mods, **rp)
        b = _relax_through(monkeypatch, c, tile, False, mods, **rp)
        print(name, tile, hex(mods), a["iters"], a["evals"], a["launches"], b["launches"], relerr(a["tin"], b["tin"]),
              relerr(a["tout"], b["tout"]), abs(a["E"] - b["E"]))
        assert (a["iters"], a["evals"]) == (b["iters"], b["evals"]) and a["iters"] == 3
        # inside the relaxation: only the streaming kernel / only the tile kernel
        assert a["launches"] == {"energy_launches": 0, "gradient_launches": 0, "vec_launches": a["evals"]}
        assert b["launches"]["vec_launches"] == 0
        assert b["launches"]["gradient_launches"] + b["launches"]["energy_launches"] == b["evals"]
        assert not np.array_equal(a["tin"], c["tin"]) and not np.array_equal(a["tout"], c["tout"])
        assert relerr(a["tin"], b["tin"]) < 1e-10 and relerr(a["tout"], b["tout"]) < 1e-10
        assert abs(a["E"] - b["E"]) <= 1e-12 * (c["E_scale"] + abs(b["E"]))
        assert relerr(a["gi"], b["gi"]) < 1e-10 and relerr(a["go"], b["go"]) < 1e-10


# ---------------------------------------------------------------------------------------------------------------------
def _milestone(g, tile=0):
    from membrane_solver_amd.geometry.mesh import ArrayMesh
    from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager
    from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager
    from membrane_solver_amd.runtime.minimizer import Minimizer
    from membrane_solver_amd.runtime.steppers import GradientDescent

    mods = [str(m) for m in g["modules"]]
    mesh = ArrayMesh(g["positions"], g["tri"], fixed=g["fixed"], tilts_in=g["tilts_in0"], tilts_out=g["tilts_out0"],
                     tilt_fixed_in=g["tilt_fixed_in"], tilt_fixed_out=g["tilt_fixed_out"],
                     global_parameters=json.loads(str(g["gp_json"])), energy_modules=mods, constraint_modules=[])
    mz = Minimizer(mesh, mesh.global_parameters, GradientDescent(), EnergyModuleManager(mods), ConstraintModuleManager([]),
                   quiet=True, tile_vertices=tile)
    return mz


def test_milestone_b_relaxation_matches_reference():
    """The shape of the reference's milestone-B tracking test: flat annulus, hard tilt_in source on the inner rim,
    k_c = 10 "difference", one nested relaxation of up to 1000 inner steps; the outer leaflet has no module but the
    coupling (its cells are DEFINED by the coupling, the vertex areas come from the set-up launch all the same)."""
    g = load_golden("tilt_coupling_milestone_b.npz")
    mz = _milestone(g)
    _mir, dm = mz._device()
    iters, evals = dm.relax_leaflet_tilts(**mz._tilt_relax_params())
    tin, tout = dm.get_leaflet_tilts("in"), dm.get_leaflet_tilts("out")
    E = float(dm.energy().sum())  # (outside the relaxation: one launch of k_couple<0>)
    st = dm.tilt_coupling_stats()
    print("iters", iters, "ref", int(g["n_iterations"]), "evals", evals, "ref", int(g["n_evaluations"]), "E", E, "ref", float(g["E_total"]), "relerr",
          relerr(tin, g["tilts_in_final"]), relerr(tout, g["tilts_out_final"]), st)
    assert iters == int(g["n_iterations"]) and evals == int(g["n_evaluations"])
    assert int(g["n_evaluations"]) == int(g["n_gradient_evaluations"]) + int(g["n_energy_evaluations"])
    assert relerr(tin, g["tilts_in_final"]) < 1e-8 and relerr(tout, g["tilts_out_final"]) < 1e-8
    assert abs(E - g["E_total"]) <= 1e-9 * abs(g["E_total"])
    assert np.mean(np.linalg.norm(tin - tout, axis=1)) < 0.1 and np.max(np.linalg.norm(tout, axis=1)) > 0.9  # it tracks
    assert abs(dm.tilt_coupling_energy() - g["E_coupling"]) <= 1e-9 * abs(g["E_total"])
    # launch counts: the streaming kernel for every evaluation of the relaxation, the tile kernel for none of them
    assert st["vec_launches"] == evals and st["gradient_launches"] == 0 and st["energy_launches"] == 1
    ex = dm.exec_stats()
    assert ex["relax_fused"] == 0 and ex["relax_programs"] == 0  # (the lanes that cannot carry it declined)
    assert dm.tsearch_stats()["passes"] == 0


def test_context_without_the_module_keeps_its_fast_lanes():
    g = dict(load_golden("tilt_coupling_milestone_b.npz"))
    g["modules"] = np.array(["tilt_smoothness_in", "tilt_in"])
    mz = _milestone(g)
    _mir, dm = mz._device()
    _iters, evals = dm.relax_leaflet_tilts(**mz._tilt_relax_params())
    assert evals > 0 and dm.exec_stats()["relax_programs"] > 0
    assert dm.tilt_coupling_stats() == {"energy_launches": 0, "gradient_launches": 0, "vec_launches": 0}


# ---------------------------------------------------------------------------------------------------------------------
def _opts(text):
    return {int(k): v for k, v in json.loads(str(text)).items()}


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
def test_minimizer_reproduces_coupling_trajectory(fname):
    """The acceptance rule of the rim-source trajectories (tests/test_gpu_rim_source.py): success flags and step sizes
    equal, energies to their tolerance; the Python loop (observe) and the C ms_minimize path, both in fixed-order mode,
    give identical finals."""
    g = load_golden(fname)
    finals = []
    for observe in (True, False):
        mesh, mz, log = _minimizer(g, TRAJ[fname], observe=observe, deterministic=True)
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
            assert abs(bd["tilt_coupling"] - g["E_coupling_final"]) <= 1e-8 * abs(g["E_final"])
            assert bd["tilt_coupling"] > 0.0
        _check_finals(mesh, res, g)
        finals.append((mesh.positions_view().copy(), np.array(mesh.tilts_in_view()).copy(),
                       np.array(mesh.tilts_out_view()).copy(), res["energy"]))
    for x, y in zip(*finals):  # observe on / off: the same launches in the same order, the same bits
        assert np.array_equal(x, y)


@pytest.mark.parametrize("fname", sorted(TRAJ))
def test_coupling_trajectory_with_small_tiles(fname):
    g = load_golden(fname)
    mesh, mz, _ = _minimizer(g, TRAJ[fname], observe=False, tile=64)
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


@pytest.mark.parametrize("fname", ["traj_disk6_gd_coupling_nested_cg.npz", "traj_ico4_gd_coupling_surface_backtrack.npz"])
def test_coupling_trajectory_is_bitwise_reproducible_in_fixed_order_mode(monkeypatch, fname):
    monkeypatch.setenv("MS_DETERMINISTIC", "1")
    g = load_golden(fname)
    a = _run_final(g, TRAJ[fname], tile=64)
    b = _run_final(g, TRAJ[fname], tile=64)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("tile", [0, 64])
def test_own_sums_are_bitwise_reproducible_in_default_mode(monkeypatch, tile):
    """The coupling's kernels use no atomics: with the module alone every output is the same bits run after run in the
    default (LDS-atomic) mode as well -- the tile form and, inside a relaxation, the streaming form."""
    from membrane_solver_amd import _lib as L

    monkeypatch.delenv("MS_DETERMINISTIC", raising=False)
    c = _case("ico4_difference")
    runs = []
    for _ in range(2):
        dm = _device(c, tile)
        dm.set_params(modules=L.MS_MOD_TILT_COUPLING)
        E, gi, go = dm.leaflet_tilt_energy_and_gradient()
        e, g = dm.energy_and_gradient(want_grad=True, raw=True)
        own = dm.tilt_coupling_energy()
        dm.relax_leaflet_tilts(solver="cg", max_iters=4, step_size=0.05, tol=0.0)
        assert dm.tilt_coupling_stats()["vec_launches"] > 0
        runs.append((np.array(E), gi, go, e, g, np.array(own), dm.get_leaflet_tilts("in"), dm.get_leaflet_tilts("out"),
                     np.array(dm.tilt_coupling_energy())))
        dm.close()
    for x, y in zip(*runs):
        assert np.array_equal(x, y)
    assert abs(float(runs[0][0]) - c["E"]) <= 1e-12 * c["E_scale"] and abs(float(runs[0][5]) - c["E"]) <= 1e-12 * c["E_scale"]


def test_search_passes_decline_with_the_module():
    """A multi-tile leaflet relaxation without the module takes the search / gradient passes of ms_tsearch.inc; with it
    they decline and the streaming kernel carries the coupling."""
    from membrane_solver_amd import _lib as L

    g = load_golden("traj_disk6_gd_coupling_nested_cg.npz")
    counts = {}
    for with_module in (False, True):
        g2 = dict(g)
        drop = ("tilt_rim_source",) if with_module else ("tilt_rim_source", "tilt_coupling")
        g2["modules"] = np.array([m for m in g["modules"] if not str(m).startswith(drop)])
        _mesh, mz, _ = _minimizer(g2, "gd", observe=False, tile=64)
        _mir, dm = mz._device()
        assert bool(dm.modules & L.MS_MOD_TILT_COUPLING) == with_module
        before = dm.tsearch_stats()["passes"]
        _iters, evals = dm.relax_leaflet_tilts(**mz._tilt_relax_params())
        counts[with_module] = dm.tsearch_stats()["passes"] - before
        st = dm.tilt_coupling_stats()
        assert st["vec_launches"] == (evals if with_module else 0) and st["gradient_launches"] == 0
    assert counts[False] > 0 and counts[True] == 0


def test_refusals_on_the_device():
    from membrane_solver_amd import _lib as L
    from membrane_solver_amd import meshgen
    from membrane_solver_amd.device import DeviceMesh

    P, T = meshgen.icosphere(3)
    dm = DeviceMesh(P, T)
    for k, s in ((1.0, 2), (1.0, -2), (float("nan"), 1), (float("inf"), -1)):
        with pytest.raises(L.MembraneHipError):
            dm.set_tilt_coupling(k, s)
    dm.set_leaflet_tilts("in", np.zeros_like(P), tilt_modulus=1.0)
    dm.set_leaflet_tilts("out", np.zeros_like(P))
    dm.set_params(modules=L.MS_MOD_TILT_IN | L.MS_MOD_TILT_COUPLING)
    with pytest.raises(L.MembraneHipError, match="ms_set_tilt_coupling was never called"):
        dm.energy()
    dm.set_tilt_coupling(2.0, -1)
    assert dm.energy()[3] == 0.0 and dm.tilt_coupling_energy() == 0.0  # (zero tilts)
    dm.set_tilt_coupling(2.0, 0)  # off: the bit is refused again
    with pytest.raises(L.MembraneHipError, match="switched it off"):
        dm.energy()
    dm.set_tilts(np.zeros_like(P), 1.0)
    with pytest.raises(L.MembraneHipError, match="single-field tilt module"):
        dm.set_params(modules=L.MS_MOD_TILT | L.MS_MOD_TILT_COUPLING)
    dm.close()
    d2 = DeviceMesh(P, T, shard_rank=0, shard_count=2)  # a sharded context: the setter and ms_set_params both refuse
    try:
        with pytest.raises(L.MembraneHipError, match="tilt_coupling module is not sharded"):
            d2.set_tilt_coupling(2.0, -1)
        with pytest.raises(L.MembraneHipError, match="tilt_coupling module is not sharded"):
            d2.set_params(modules=L.MS_MOD_TILT_IN | L.MS_MOD_TILT_COUPLING)
        d2.set_tilt_coupling(2.0, 0)  # (switching it off is no use of the module)
    finally:
        d2.close()
