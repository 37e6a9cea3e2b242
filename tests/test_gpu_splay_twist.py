"""tilt_splay_twist_in on the HIP path (csrc/ms_splay.hip): the plugin against the reference's module on every case of
splay_twist_cases.npz, the slot protocol (sums ADDED behind tilt_smoothness_in's pass or DEFINING the cells), one
reference relaxation and three reference trajectories (tools/gen_golden_splay_twist.py), the one-tile interpreter and the
refusals.  Bars: |E - E_ref| <= 1e-12 E_scale with E_scale = sum |facet term|, every tilt-gradient row within 1e-10 of
its scale sum |corner term| (for the rotation field whose divergence vanishes: the scales of the uncancelled field), exact
zeros where the reference has exact zeros; trajectories within max(1e-12, 10 x noise) relative, noise being what a 1e-13
perturbation of the start does to the reference's own run."""

import json

import numpy as np
import pytest

from conftest import load_golden, relerr

pytestmark = pytest.mark.gpu

CASES = load_golden("splay_twist_cases.npz")
NAMES = [str(n) for n in CASES["names"]]
TRAJ = {"traj_disk6_gd_splaytwist_nested_cg.npz": "gd", "traj_disk6_cg_splaytwist_coupled_gd.npz": "cg",
        "traj_ico4_gd_splaytwist_surface_backtrack.npz": "gd"}


def _case(name):
    g = CASES
    mesh = str(g[name + "__mesh"])
    what = str(g[name + "__what"])
    P, T = g["mesh__" + mesh + "__positions"], g["mesh__" + mesh + "__tri"]
    pos = g[name + "__eval_positions"] if what == "moved" else P
    return {"P": P, "T": T, "pos": pos, "what": what, "gp": json.loads(str(g[name + "__gp"])),
            "k_splay": float(g[name + "__k_splay"]), "k_twist": float(g[name + "__k_twist"]), "tin": g[name + "__tilts_in"],
            "E": float(g[name + "__E"]), "tg": g[name + "__tilt_grad_in"], "E_scale": float(g[name + "__E_scale"]),
            "row_scale": g[name + "__row_scale"]}


def _set_mode(monkeypatch, fixed_order):
    if fixed_order:
        monkeypatch.setenv("MS_DETERMINISTIC", "1")
    else:
        monkeypatch.delenv("MS_DETERMINISTIC", raising=False)


def _rows_close(got, ref, row_scale, what=""):
    """every row within 1e-10 of its own scale"""
    err = np.max(np.abs(got - ref), axis=1)
    worst = float(np.max(err / np.maximum(row_scale, 1e-300))) if len(err) else 0.0
    print("   ", what, "max row |d| / scale", worst)
    return bool(np.all(err <= 1e-10 * row_scale))


def _check_case(monkeypatch, name, tile, fixed_order):
    from membrane_solver_amd.core.parameters import GlobalParameters, ParameterResolver
    from membrane_solver_amd.geometry.mesh import ArrayMesh, mirror_for
    from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager

    _set_mode(monkeypatch, fixed_order)
    c = _case(name)
    gp = GlobalParameters(c["gp"])
    mesh = ArrayMesh(c["P"], c["T"], global_parameters=gp, tilts_in=c["tin"], tilts_out=np.zeros_like(c["P"]))
    if tile:
        mirror_for(mesh, tile_vertices=tile)  # (stashed on the mesh: the plugin evaluates on this mirror)
    res = ParameterResolver(gp)
    module = EnergyModuleManager(["tilt_splay_twist_in"]).get_module("tilt_splay_twist_in")
    assert module.USES_TILT_LEAFLETS
    pos, tin = c["pos"], c["tin"]
    kw = dict(positions=pos, index_map=mesh.vertex_index_to_row)
    t_arg = None if c["what"] == "mesh_tilts" else tin
    sentinel = np.arange(pos.size, dtype=np.float64).reshape(pos.shape)
    grad, tg = sentinel.copy(), np.zeros_like(pos)
    E = module.compute_energy_and_gradient_array(mesh, gp, res, grad_arr=grad, tilts_in=t_arg, tilt_in_grad_arr=tg, **kw)
    E2 = module.compute_energy_array(mesh, gp, res, tilts_in=t_arg, **kw)
    E3 = module.compute_energy_and_gradient_array(mesh, gp, res, grad_arr=grad, tilts_in=t_arg, **kw)  # no tilt_in_grad_arr
    print(name, "tile", tile, "fixed order", fixed_order, "E", E, "ref", c["E"], "|dE|/scale",
          abs(E - c["E"]) / max(c["E_scale"], 1e-300))
    assert np.array_equal(grad, sentinel)  # the shape-gradient array comes back bit-identical
    if c["what"] == "off":  # exactly nothing
        assert E == 0.0 and E2 == 0.0 and E3 == 0.0 and not tg.any()
    else:
        for e in (E, E2, E3):
            assert abs(e - c["E"]) <= 1e-12 * c["E_scale"]
        assert _rows_close(tg, c["tg"], c["row_scale"], "tilt gradient")
        if tile and len(pos) > tile:  # (disk4 has 61 vertices: one tile of 64; disk6's 127 make two, ico4's 162 three)
            assert mesh._hip_mirror.dm.tile_stats()["n_tiles"] > 1
    # the tilt gradient is ADDED into what it is handed
    added = sentinel.copy()
    module.compute_energy_and_gradient_array(mesh, gp, res, grad_arr=grad, tilts_in=t_arg, tilt_in_grad_arr=added, **kw)
    assert np.all(np.max(np.abs((added - sentinel) - c["tg"]), axis=1) <= 1e-10 * c["row_scale"] + 4e-16 * sentinel.max())
    if c["what"] == "off":
        assert np.array_equal(added, sentinel)
    if c["what"] != "moved":  # the dict API evaluates the mesh's own positions and tilts and lists the non-zero rows
        Ed, gd, tgd = module.compute_energy_and_gradient(mesh, gp, res)
        assert gd == {} and abs(Ed - c["E"]) <= 1e-12 * c["E_scale"]
        dense = np.zeros_like(pos)
        for vid, row in tgd.items():
            assert row.any()
            dense[mesh.vertex_index_to_row[vid]] = row
        assert _rows_close(dense, c["tg"], c["row_scale"], "dict tilt gradient")
        Ee, none = module.compute_energy_and_gradient(mesh, gp, res, compute_gradient=False)  # (k_splay<0>, not <1>)
        assert none == {} and abs(Ee - c["E"]) <= 1e-12 * c["E_scale"]
        if c["what"] == "off":
            assert Ed == 0.0 and tgd == {}


@pytest.mark.parametrize("fixed_order", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_plugin_matches_reference(monkeypatch, name, fixed_order):
    _check_case(monkeypatch, name, 0, fixed_order)


@pytest.mark.parametrize("fixed_order", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_plugin_with_small_tiles(monkeypatch, name, fixed_order):
    """64-vertex tiles: every tile takes at least two facet chunks with a partial last one, the 127- and 162-row meshes
    have halo rows and a last tile with few owned rows."""
    _check_case(monkeypatch, name, 64, fixed_order)


def _device(c, tile, k_in=1.3, k_out=0.9):
    from membrane_solver_amd.device import DeviceMesh

    dm = DeviceMesh(c["pos"], c["T"], tile_vertices=tile)
    dm.set_leaflet_tilts("in", c["tin"], tilt_modulus=k_in, smoothness=0.7)
    dm.set_leaflet_tilts("out", 0.5 * c["tin"][::-1].copy(), tilt_modulus=k_out, smoothness=0.4)
    dm.set_tilt_splay_twist(c["k_splay"], c["k_twist"])
    return dm


@pytest.mark.parametrize("fixed_order", [False, True])
@pytest.mark.parametrize("name", ["disk6_both", "ico4_moved", "disk6z_zero_area_both"])
@pytest.mark.parametrize("tile", [0, 64])
def test_slot_protocol(monkeypatch, name, tile, fixed_order):
    """With and without the bit, next to tilt_smoothness_in (the sums are ADDED behind its pass) and without it (the cells
    are DEFINED): energies[:3] bit-identical, energies[3] and the leaflet evaluation differ by the module's own energy
    and gradient; the module reports its own energy."""
    from membrane_solver_amd import _lib as L

    _set_mode(monkeypatch, fixed_order)
    c = _case(name)
    dm = _device(c, tile)
    bit = L.MS_MOD_TILT_SPLAY_TWIST_IN
    for base in (L.MS_MOD_SURFACE | L.MS_MOD_TILT_IN | L.MS_MOD_TILT_OUT | L.MS_MOD_TILT_SMOOTH_IN | L.MS_MOD_TILT_SMOOTH_OUT,
                 L.MS_MOD_TILT_SMOOTH_IN,                                       # ADD lanes
                 L.MS_MOD_SURFACE | L.MS_MOD_TILT_IN | L.MS_MOD_TILT_SMOOTH_OUT, L.MS_MOD_TILT_OUT):  # DEFINE lanes
        dm.set_params(modules=base)
        E0, gi0, go0 = dm.leaflet_tilt_energy_and_gradient()
        e0, g0 = dm.energy_and_gradient(want_grad=True, raw=True)
        dm.set_params(modules=base | bit)
        E1, gi1, go1 = dm.leaflet_tilt_energy_and_gradient()
        own1 = dm.tilt_splay_twist_energy()
        e1, g1 = dm.energy_and_gradient(want_grad=True, raw=True)
        own2 = dm.tilt_splay_twist_energy()
        e2 = dm.energy()
        own3 = dm.tilt_splay_twist_energy()
        tol = 1e-12 * (c["E_scale"] + abs(E0))
        print(name, tile, hex(base), "dE", (E1 - E0) - c["E"], (e1[3] - e0[3]) - c["E"], "own", own1 - c["E"], own2 - c["E"])
        assert abs((E1 - E0) - c["E"]) <= tol and abs((e1[3] - e0[3]) - c["E"]) <= tol and abs((e2[3] - e0[3]) - c["E"]) <= tol
        for own in (own1, own2, own3):
            assert abs(own - c["E"]) <= 1e-12 * c["E_scale"]
        assert np.array_equal(e1[:3], e0[:3]) and np.array_equal(e2[:3], e0[:3])
        # no shape gradient and nothing of the outer leaflet's (the other modules' own vertex sums are LDS atomics in
        # the default setting: their order, and so their last bits, may differ from run to run)
        if fixed_order:
            assert np.array_equal(g1, g0) and np.array_equal(go1, go0)
        else:
            assert relerr(g1, g0) < 1e-13 and relerr(go1, go0) < 1e-13
        floor = 4e-16 * float(np.max(np.abs(gi0)))
        assert np.all(np.max(np.abs((gi1 - gi0) - c["tg"]), axis=1) <= 1e-10 * c["row_scale"] + floor)
    dm.close()


@pytest.mark.parametrize("fixed_order", [False, True])
@pytest.mark.parametrize("tile", [0, 64])
def test_own_outputs_are_bitwise_reproducible(monkeypatch, tile, fixed_order):
    """No atomics, the gather in ascending facet order: with the module alone every output is the same bits run after
    run, in both summation settings -- and the same bits in one setting as in the other."""
    from membrane_solver_amd import _lib as L

    c = _case("ico4_both")
    runs = []
    for mode in (fixed_order, fixed_order, not fixed_order):
        _set_mode(monkeypatch, mode)
        dm = _device(c, tile)
        dm.set_params(modules=L.MS_MOD_TILT_SPLAY_TWIST_IN)
        E, gi, _go = dm.leaflet_tilt_energy_and_gradient()
        e = dm.energy()
        own = dm.tilt_splay_twist_energy()
        dm.relax_leaflet_tilts(solver="cg", max_iters=4, step_size=0.01, tol=0.0)
        runs.append((np.array(E), gi, e, np.array(own), dm.get_leaflet_tilts("in"), np.array(dm.tilt_splay_twist_energy())))
        st = dm.tilt_splay_twist_stats()
        assert st["energy_launches"] > 0 and st["gradient_launches"] > 0
        dm.close()
    for x, y, z in zip(*runs):
        assert np.array_equal(x, y) and np.array_equal(x, z)
    assert abs(float(runs[0][0]) - c["E"]) <= 1e-12 * c["E_scale"] and abs(float(runs[0][3]) - c["E"]) <= 1e-12 * c["E_scale"]
    assert not np.array_equal(runs[0][4], c["tin"])  # the relaxation moved the field


# ---------------------------------------------------------------------------------------------------------------------
def _relax_minimizer(g, tile=0, deterministic=None):
    from membrane_solver_amd.geometry.mesh import ArrayMesh
    from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager
    from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager
    from membrane_solver_amd.runtime.minimizer import Minimizer
    from membrane_solver_amd.runtime.steppers import GradientDescent

    mods = [str(m) for m in g["modules"]]
    mesh = ArrayMesh(g["positions"], g["tri"], fixed=g["fixed"], tilts_in=g["tilts_in0"], tilts_out=g["tilts_out0"],
                     tilt_fixed_in=g["tilt_fixed_in"], tilt_fixed_out=g["tilt_fixed_out"],
                     global_parameters=json.loads(str(g["gp_json"])), energy_modules=mods, constraint_modules=[])
    return Minimizer(mesh, mesh.global_parameters, GradientDescent(), EnergyModuleManager(mods), ConstraintModuleManager([]),
                     quiet=True, tile_vertices=tile, deterministic=deterministic)


@pytest.mark.parametrize("tile", [0, 64])
def test_relaxation_matches_reference(tile):
    """One relax_leaflet_tilts run of tilt_in + tilt_smoothness_in + tilt_splay_twist_in (the ADD lane), CG with the
    Jacobi preconditioner: the reference's iteration and evaluation counts exactly, tilts within the bar of
    test_gpu_relax_onetile.py, clamped rows unchanged, and every pass that cannot carry the term declined."""
    g = load_golden("splay_twist_relax.npz")
    mz = _relax_minimizer(g, tile)
    _mir, dm = mz._device()
    iters, evals = dm.relax_leaflet_tilts(**mz._tilt_relax_params())
    tin = dm.get_leaflet_tilts("in")
    E = float(dm.energy().sum())
    st = dm.tilt_splay_twist_stats()
    print("tile", tile, "iters", iters, "ref", int(g["n_iterations"]), "evals", evals, "ref", int(g["n_evaluations"]), "E", E,
          "ref", float(g["E_total"]), "relerr", relerr(tin, g["tilts_in_final"]), st)
    assert iters == int(g["n_iterations"]) and evals == int(g["n_evaluations"])
    assert relerr(tin, g["tilts_in_final"]) < 1e-9
    fin = g["tilt_fixed_in"]
    assert np.max(np.abs(tin[fin] - g["tilts_in0"][fin])) <= 1e-15  # (projected once onto the plane they lay in)
    assert abs(E - float(g["E_total"])) <= 1e-9 * abs(float(g["E_total"]))
    assert abs(dm.tilt_splay_twist_energy() - float(g["E_splay_twist"])) <= 1e-9 * abs(float(g["E_total"]))
    # one launch per evaluation of the relaxation: k_splay<1> for the gradient evaluations, k_splay<0> for the trials
    # (+ the energy() above)
    assert st["gradient_launches"] == int(g["n_gradient_evaluations"])
    assert st["energy_launches"] == int(g["n_energy_evaluations"]) + 1
    ex = dm.exec_stats()
    assert ex["relax_fused"] == 0 and ex["relax_programs"] == 0  # (the lanes that cannot carry it declined)
    assert dm.tsearch_stats()["passes"] == 0


def test_context_without_the_module_keeps_its_fast_lanes():
    g = dict(load_golden("splay_twist_relax.npz"))
    g["modules"] = np.array(["tilt_in", "tilt_smoothness_in"])
    mz = _relax_minimizer(g)
    _mir, dm = mz._device()
    _iters, evals = dm.relax_leaflet_tilts(**mz._tilt_relax_params())
    assert evals > 0 and dm.exec_stats()["relax_programs"] > 0
    assert dm.tilt_splay_twist_stats() == {"energy_launches": 0, "gradient_launches": 0}
    mz = _relax_minimizer(g, tile=64)  # several tiles: the search passes
    _mir, dm = mz._device()
    dm.relax_leaflet_tilts(**mz._tilt_relax_params())
    assert dm.tsearch_stats()["passes"] > 0


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
                     edges=g["edges"])
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


def _bar(g, key):
    """The device differs from the reference by summation order only: a perturbation of the kind the generator measured
    (noise_*: a 1e-13 perturbation of the start); the factor 10 is the margin for its size being a few ulps."""
    return max(1e-12, 10.0 * float(g[key]))


def _check_finals(mesh, res, g):
    print("    finals: x", relerr(mesh.positions_view(), g["positions_final"]), "bar", _bar(g, "noise_positions"),
          "t_in", relerr(mesh.tilts_in_view(), g["tilts_in_final"]), "bar", _bar(g, "noise_tilts"),
          "E", abs(res["energy"] - float(g["E_final"])) / abs(float(g["E_final"])), "bar", _bar(g, "noise_energy"))
    assert relerr(mesh.positions_view(), g["positions_final"]) <= _bar(g, "noise_positions")
    assert relerr(mesh.tilts_in_view(), g["tilts_in_final"]) <= _bar(g, "noise_tilts")
    if any(str(m).endswith("_out") for m in g["modules"]):
        assert relerr(mesh.tilts_out_view(), g["tilts_out_final"]) <= _bar(g, "noise_tilts")
    else:  # (nobody reads the outer leaflet: it starts at zero and stays there)
        assert not np.any(g["tilts_out_final"]) and not np.any(mesh.tilts_out_view())
    assert abs(res["energy"] - float(g["E_final"])) <= _bar(g, "noise_energy") * abs(float(g["E_final"]))


@pytest.mark.parametrize("tile", [0, 64])
@pytest.mark.parametrize("fname", sorted(TRAJ))
def test_minimizer_reproduces_splay_twist_trajectory(fname, tile):
    """Accept / reject sequence and step sizes equal the reference's, energies and finals within the measured noise; the
    Python loop (observe) and the C ms_minimize path, both in fixed-order mode, give identical finals."""
    g = load_golden(fname)
    finals = []
    for observe in (True, False):
        mesh, mz, log = _minimizer(g, TRAJ[fname], observe=observe, tile=tile, deterministic=True)
        if observe:
            E0, grad0 = mz.compute_energy_and_gradient_array()
            assert abs(E0 - g["E0"]) <= 1e-12 * abs(g["E0"])
            assert relerr(grad0, g["grad0"]) < 1e-10
        res = mz.minimize(int(g["n_steps"]))
        if observe:
            got, ref = np.array(log), g["step_log"]
            print(fname, "tile", tile, "got", got.tolist(), "ref", ref.tolist())
            assert got.shape == ref.shape
            assert np.array_equal(got[:, 0], ref[:, 0]), "accept/reject sequence differs from the reference"
            assert np.allclose(got[:, 1], ref[:, 1], rtol=1e-12, atol=0)
            assert np.allclose(got[:, 2], ref[:, 2], rtol=_bar(g, "noise_energy"), atol=0)
            bd = mz.compute_energy_breakdown()
            assert abs(sum(bd.values()) - res["energy"]) <= 1e-12 * abs(res["energy"])
            assert abs(bd["tilt_splay_twist_in"] - float(g["E_splay_twist_final"])) <= _bar(g, "noise_energy") * abs(float(g["E_final"]))
            assert bd["tilt_splay_twist_in"] > 0.0
        _check_finals(mesh, res, g)
        finals.append((mesh.positions_view().copy(), np.array(mesh.tilts_in_view()).copy(),
                       np.array(mesh.tilts_out_view()).copy(), res["energy"]))
    for x, y in zip(*finals):  # observe on / off: the same launches in the same order, the same bits
        assert np.array_equal(x, y)


def _run_final(g, kind, **kw):
    mesh, mz, _ = _minimizer(g, kind, observe=False, **kw)
    res = mz.minimize(int(g["n_steps"]))
    ex = mesh._hip_mirror.dm.exec_stats()
    return (mesh.positions_view().copy(), np.array(mesh.tilts_in_view()).copy(), np.array(mesh.tilts_out_view()).copy(),
            res["energy"]), ex


@pytest.mark.parametrize("fname", sorted(TRAJ))
def test_interpreter_on_and_off_give_the_same_bits(monkeypatch, fname):
    """One-tile contexts run their launches through the one-workgroup interpreter; the splay / twist pass flushes the
    recorder and launches on its own, so the rest of the pack is as before: MS_EXEC=0 and the default give bitwise equal
    trajectories in fixed-order mode."""
    g = load_golden(fname)
    monkeypatch.delenv("MS_EXEC", raising=False)
    a, ex_a = _run_final(g, TRAJ[fname], deterministic=True)
    monkeypatch.setenv("MS_EXEC", "0")
    b, ex_b = _run_final(g, TRAJ[fname], deterministic=True)
    print(fname, ex_a, ex_b)
    assert ex_a["active"] and ex_a["packs"] > 0 and not ex_b["active"]
    assert ex_a["relax_programs"] == 0 and ex_a["relax_fused"] == 0
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_refusals_on_the_device():
    from membrane_solver_amd import _lib as L
    from membrane_solver_amd import meshgen
    from membrane_solver_amd.device import DeviceMesh
    from membrane_solver_amd.geometry.mesh import ArrayMesh
    from membrane_solver_amd.modules.constraints import pins

    P, T = meshgen.icosphere(3)
    dm = DeviceMesh(P, T)
    for ks, kt in ((-1.0, 0.0), (0.0, -1e-300), (float("nan"), 1.0), (1.0, float("inf")), (-float("inf"), 0.0)):
        with pytest.raises(L.MembraneHipError, match="ms_set_tilt_splay_twist: the moduli must be"):
            dm.set_tilt_splay_twist(ks, kt)
    dm.set_leaflet_tilts("in", np.zeros_like(P), tilt_modulus=1.0)
    dm.set_leaflet_tilts("out", np.zeros_like(P))
    dm.set_params(modules=L.MS_MOD_TILT_IN | L.MS_MOD_TILT_SPLAY_TWIST_IN)
    with pytest.raises(L.MembraneHipError, match="ms_set_tilt_splay_twist was never called"):
        dm.energy()
    dm.set_tilt_splay_twist(2.0, 1.0)
    assert dm.energy()[3] == 0.0 and dm.tilt_splay_twist_energy() == 0.0  # (zero tilts)
    # both moduli 0: the bit contributes exactly nothing
    rng = np.random.default_rng(3)
    dm.set_leaflet_tilts("in", 0.2 * rng.normal(size=P.shape), tilt_modulus=1.0)
    dm.set_params(modules=L.MS_MOD_TILT_IN)
    E0, gi0, _go = dm.leaflet_tilt_energy_and_gradient()
    e0 = dm.energy()
    dm.set_tilt_splay_twist(0.0, 0.0)
    dm.set_params(modules=L.MS_MOD_TILT_IN | L.MS_MOD_TILT_SPLAY_TWIST_IN)
    E1, gi1, _go = dm.leaflet_tilt_energy_and_gradient()
    assert E1 == E0 and np.array_equal(gi1, gi0) and np.array_equal(dm.energy(), e0) and dm.tilt_splay_twist_energy() == 0.0
    # a single-field tilt module next to it
    dm.set_tilts(np.zeros_like(P), 1.0)
    with pytest.raises(L.MembraneHipError, match="tilt_splay_twist_in together with a single-field tilt module"):
        dm.set_params(modules=L.MS_MOD_TILT | L.MS_MOD_TILT_SPLAY_TWIST_IN)
    # pins, or the volume enforcer, next to it on the line search
    dm.set_tilt_splay_twist(2.0, 1.0)
    dm.set_params(modules=L.MS_MOD_SURFACE | L.MS_MOD_TILT_IN | L.MS_MOD_TILT_SPLAY_TWIST_IN)
    opts = {0: {"constraints": ["pin_to_plane"], "pin_to_plane_normal": [0.0, 0.0, 1.0],
                "pin_to_plane_point": [0.0, 0.0, float(P[0, 2])]}}
    mesh = ArrayMesh(P, T, vertex_options=opts)
    dm.set_pins(pins.device_tables(P, pins.programs(mesh, ["pin_to_plane"])))
    with pytest.raises(L.MembraneHipError, match="tilt_splay_twist_in together with pin_to_plane / pin_to_circle or the volume enforcer"):
        dm.step(stepper=L.MS_STEPPER_GD, step_size=1e-3, enforce_pins=1)
    dm.set_pins(None)
    with pytest.raises(L.MembraneHipError, match="tilt_splay_twist_in together with pin_to_plane / pin_to_circle or the volume enforcer"):
        dm.step(stepper=L.MS_STEPPER_GD, step_size=1e-3, enforce_volume=1)
    r = dm.step(stepper=L.MS_STEPPER_GD, step_size=1e-3)  # (without an enforcer the step runs)
    assert r.success
    dm.close()
    d2 = DeviceMesh(P, T, shard_rank=0, shard_count=2)  # a sharded context: the setter and ms_set_params both refuse
    try:
        with pytest.raises(L.MembraneHipError, match="tilt_splay_twist_in module is not sharded"):
            d2.set_tilt_splay_twist(2.0, 1.0)
        with pytest.raises(L.MembraneHipError, match="tilt_splay_twist_in module is not sharded"):
            d2.set_params(modules=L.MS_MOD_TILT_IN | L.MS_MOD_TILT_SPLAY_TWIST_IN)
    finally:
        d2.close()
