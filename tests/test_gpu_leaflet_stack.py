"""The leaflet add-on modules TOGETHER on the HIP path: several of them behind each other in one partial-sum cell and in
the same rows of the tilt-gradient buffers (tools/gen_golden_leaflet_stack.py).  tilt_rim_source_in and
tilt_thetaB_contact_in ride in the inner leaflet's tilt-magnitude cell, tilt_rim_source_out, tilt_rim_source_bilayer and
tilt_coupling in the outer one's, tilt_splay_twist_in in the inner smoothness cell; every pass decides from the module mask
whether it defines its cell or adds behind an earlier pass, and the gradient pass re-adds behind k_tilt<1>.  A cell defined
twice, an add left out of the re-adds or a part subtracted twice in compute_energy_breakdown shows here; a decision that
forgets one add-on of a chain (tilt_thetaB_contact_in behind tilt_rim_source_in without tilt_in) shows nowhere else.

Bars.  Energies within 1e-12 E_scale (E_scale: the sum over the active modules of the module's energy where every term is
>= 0, of sum |term| for the rim sources and the contact term); gradients within the project's 1e-10 of the reference
array's largest entry, exact zeros where the reference has exact zeros; every add-on of every case moves E or a tilt
gradient by >= 1e-4 of those scales when it is dropped (test_leaflet_stack_host.py).  Relaxation and trajectories: counts,
decisions and step sizes exact, fields and energies within max(1e-12, 10 x noise), noise being what a 1e-13 perturbation
of the start does to the reference's own run."""

import json

import numpy as np
import pytest

from conftest import load_golden, relerr
from test_leaflet_stack_host import ADDONS, CASES, CONSTRAINT, NAMES, RELAX_FILE, TRAJ, bar, case

pytestmark = pytest.mark.gpu

INNER_ONLY = ["tilt_rim_source_in", "tilt_thetaB_contact_in", "tilt_splay_twist_in"]


def _set_mode(monkeypatch, fixed_order):
    if fixed_order:
        monkeypatch.setenv("MS_DETERMINISTIC", "1")
    else:
        monkeypatch.delenv("MS_DETERMINISTIC", raising=False)


def _opts(text):
    return {int(k): v for k, v in json.loads(str(text)).items()}


def _case_minimizer(mods, gp, tile):
    from membrane_solver_amd.geometry.mesh import ArrayMesh
    from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager
    from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager
    from membrane_solver_amd.runtime.minimizer import Minimizer
    from membrane_solver_amd.runtime.steppers import GradientDescent

    g = CASES
    mesh = ArrayMesh(g["positions"], g["tri"], fixed=g["fixed"], tilts_in=g["tilts_in"], tilts_out=g["tilts_out"],
                     global_parameters=dict(gp), energy_modules=list(mods), constraint_modules=[], edges=g["edges"],
                     vertex_options=_opts(g["vopts"]))
    mz = Minimizer(mesh, mesh.global_parameters, GradientDescent(), EnergyModuleManager(list(mods)),
                   ConstraintModuleManager([]), quiet=True, tile_vertices=tile)
    _mir, dm = mz._device()
    if tile:
        assert dm.tile_stats()["n_tiles"] == 2  # (127 rows: two tiles of 64, halo rows on both)
    return mz, dm


def _own_energies(dm):
    """every add-on's own energy as its getter reports it"""
    from membrane_solver_amd import _lib as L

    on = lambda bit: bool(dm.modules & bit)  # noqa: E731
    return {"tilt_rim_source_in": dm.leaflet_rim_source_energy("in") if on(L.MS_MOD_TILT_RIM_SOURCE_IN) else 0.0,
            "tilt_rim_source_out": dm.leaflet_rim_source_energy("out") if on(L.MS_MOD_TILT_RIM_SOURCE_OUT) else 0.0,
            "tilt_rim_source_bilayer": dm.rim_source_bilayer_energy() if on(L.MS_MOD_TILT_RIM_SOURCE_BILAYER) else 0.0,
            "tilt_coupling": dm.tilt_coupling_energy() if on(L.MS_MOD_TILT_COUPLING) else 0.0,
            "tilt_thetaB_contact_in": dm.thetab_contact_energy() if on(L.MS_MOD_TILT_THETAB_CONTACT_IN) else 0.0,
            "tilt_splay_twist_in": dm.tilt_splay_twist_energy() if on(L.MS_MOD_TILT_SPLAY_TWIST_IN) else 0.0}


def _close(got, ref, what):
    """within 1e-10 of the reference array's largest entry, exact zeros where the reference has exact zeros"""
    big = float(np.max(np.abs(ref)))
    err = float(np.max(np.abs(got - ref)))
    print("   ", what, "max |d| / largest entry", err / max(big, 1e-300))
    zero = ~np.any(ref != 0.0, axis=1)
    return err <= 1e-10 * big and not got[zero].any()


def _check_evaluation(mz, dm, c, fixed_order, label):
    tol = 1e-12 * c["E_scale"]
    # -- the total by the three routes
    e_first = dm.energy()
    e_grad, _g_raw = dm.energy_and_gradient(want_grad=True, raw=True)
    e_after = dm.energy()
    E_tilt, gi, go = dm.leaflet_tilt_energy_and_gradient()
    e_last = dm.energy()
    print(label, "E", float(e_first.sum()), "ref", c["E"], "|dE|/scale", abs(float(e_first.sum()) - c["E"]) / c["E_scale"],
          "after the gradient", abs(float(e_grad.sum()) - c["E"]) / c["E_scale"], "tilt route",
          abs(E_tilt - c["E_tilt"]) / c["E_scale"])
    assert abs(float(e_first.sum()) - c["E"]) <= tol
    assert abs(float(e_grad.sum()) - c["E"]) <= tol
    assert abs(E_tilt - c["E_tilt"]) <= tol
    # -- the energy vector after the gradient pass rewrote and re-added the cells
    print(label, "energy vector: first", e_first.tolist(), "gradient", e_grad.tolist(), "after", e_after.tolist())
    for e in (e_grad, e_after, e_last):
        if fixed_order:
            assert np.array_equal(e, e_first), "the energy vector changed across a gradient evaluation"
        else:
            assert np.all(np.abs(e - e_first) <= 1e-13 * np.abs(e_first))
    # -- gradients
    E_arr, grad = mz.compute_energy_and_gradient_array()
    assert abs(E_arr - c["E"]) <= tol
    assert _close(gi, c["gi"], "inner tilt gradient") and _close(go, c["go"], "outer tilt gradient")
    assert _close(grad, c["grad"], "shape gradient")
    # -- breakdown
    bd = mz.compute_energy_breakdown()
    own = _own_energies(dm)
    E_now = float(dm.energy().sum())
    print(label, "breakdown deviations / scale", {m: abs(bd[m] - c["breakdown"][m]) / c["E_scale"] for m in c["modules"]})
    assert list(bd) == c["modules"]
    for m in c["modules"]:
        assert abs(bd[m] - c["breakdown"][m]) <= tol, m
        if m in ADDONS:
            assert abs(own[m] - bd[m]) <= tol, m
    assert abs(sum(bd.values()) - E_now) <= tol and abs(E_now - c["E"]) <= tol
    for m in c["empty"]:
        assert bd[m] == 0.0


@pytest.mark.parametrize("fixed_order", [False, True])
@pytest.mark.parametrize("tile", [0, 64])
@pytest.mark.parametrize("name", NAMES)
def test_case_matches_reference(monkeypatch, name, tile, fixed_order):
    """Every subset of one chain next to the two others in full, the add-ons alone (every cell DEFINED by an add-on, the
    gradient pass leaves the cells alone) and the listed modules whose group selects no edge: total energy by
    energy(), energy_and_gradient(raw) and leaflet_tilt_energy_and_gradient(), the energy vector across the gradient
    pass, the three gradients and the breakdown."""
    _set_mode(monkeypatch, fixed_order)
    c = case(name)
    mz, dm = _case_minimizer(c["modules"], c["gp"], tile)
    _check_evaluation(mz, dm, c, fixed_order, "%s tile %d fixed order %s" % (name, tile, fixed_order))
    dm.close()


EMPTY_TABLES = {"empty_rsi_then_tbc": ("in", "MS_MOD_TILT_RIM_SOURCE_IN"),
                "empty_rso_then_rb_cpl": ("out", "MS_MOD_TILT_RIM_SOURCE_OUT"),
                "empty_rb_then_cpl": (None, "MS_MOD_TILT_RIM_SOURCE_BILAYER")}


@pytest.mark.parametrize("fixed_order", [False, True])
@pytest.mark.parametrize("tile", [0, 64])
@pytest.mark.parametrize("name", sorted(EMPTY_TABLES))
def test_empty_table_in_front_of_a_populated_pass(monkeypatch, name, tile, fixed_order):
    """The Minimizer leaves a module without a rim edge out of the mask.  Here the module's bit is SET and its table holds
    no edge: its pass zeroes the cells it would define, and the populated passes behind it add into them -- the same
    energies, gradients and breakdown as before."""
    from membrane_solver_amd import _lib as L

    _set_mode(monkeypatch, fixed_order)
    c = case(name)
    mz, dm = _case_minimizer(c["modules"], c["gp"], tile)
    leaflet, bit = EMPTY_TABLES[name]
    assert not dm.modules & getattr(L, bit)
    none = np.zeros(0, np.int32)
    if leaflet is None:
        dm.set_rim_source_bilayer(none, none, np.zeros(0))
    else:
        dm.set_leaflet_rim_source(leaflet, none, none, np.zeros(0))
    p = dm._params
    dm.set_params(modules=p.modules | getattr(L, bit), bending_model=p.bending_model, bending_grad_mode=p.bending_grad_mode,
                  volume_stiffness=p.volume_stiffness, target_volume=p.target_volume)
    tol = 1e-12 * c["E_scale"]
    e_first = dm.energy()
    e_grad, _g = dm.energy_and_gradient(want_grad=True, raw=True)
    e_after = dm.energy()
    E_tilt, gi, go = dm.leaflet_tilt_energy_and_gradient()
    print(name, tile, fixed_order, "|dE|/scale", abs(float(e_first.sum()) - c["E"]) / c["E_scale"],
          abs(float(e_grad.sum()) - c["E"]) / c["E_scale"], abs(E_tilt - c["E_tilt"]) / c["E_scale"])
    for e in (e_first, e_grad, e_after):
        assert abs(float(e.sum()) - c["E"]) <= tol
    assert abs(E_tilt - c["E_tilt"]) <= tol
    if fixed_order:
        assert np.array_equal(e_grad, e_first) and np.array_equal(e_after, e_first)
    assert _close(gi, c["gi"], "inner tilt gradient") and _close(go, c["go"], "outer tilt gradient")
    own = _own_energies(dm)
    for m in c["modules"]:
        if m in ADDONS:
            assert abs(own[m] - c["breakdown"][m]) <= tol, m
    assert own[c["empty"][0]] == 0.0
    dm.close()


@pytest.mark.parametrize("tile", [0, 64])
@pytest.mark.parametrize("addon", INNER_ONLY)
def test_outer_gradient_ignores_an_inner_addon(monkeypatch, addon, tile):
    """Fixed-order mode: the outer leaflet's tilt gradient of the full stack is the same bits with and without an add-on
    that reads the inner field only; the inner one moves by that add-on's own gradient."""
    _set_mode(monkeypatch, True)
    c = case("full")
    seen = []
    for mods in (c["modules"], [m for m in c["modules"] if m != addon]):
        _mz, dm = _case_minimizer(mods, c["gp"], tile)
        seen.append(dm.leaflet_tilt_energy_and_gradient())
        dm.close()
    (E1, gi1, go1), (E0, gi0, go0) = seen
    own_gi = CASES["alone__" + addon + "__tilt_grad_in"]
    assert not CASES["alone__" + addon + "__tilt_grad_out"].any()
    assert np.array_equal(go1, go0)
    assert abs((E1 - E0) - float(CASES["alone__" + addon + "__E"])) <= 1e-12 * c["E_scale"]
    assert np.max(np.abs((gi1 - gi0) - own_gi)) <= 1e-10 * float(np.max(np.abs(c["gi"])))
    assert np.max(np.abs(gi1 - gi0)) >= 1e-4 * float(np.max(np.abs(c["gi"])))


# -- the relaxation --------------------------------------------------------------------------------------------------------
def _launches(dm):
    return {"rim_in": dm.leaflet_rim_source_stats("in")["apply_launches"],
            "rim_out": dm.leaflet_rim_source_stats("out")["apply_launches"],
            "rim_bilayer": dm.rim_source_bilayer_stats()["apply_launches"],
            "coupling": sum(dm.tilt_coupling_stats().values()),
            "contact": dm.thetab_contact_stats()["apply_launches"],
            "splay_energy": dm.tilt_splay_twist_stats()["energy_launches"],
            "splay_gradient": dm.tilt_splay_twist_stats()["gradient_launches"],
            "project": dm.thetab_boundary_stats()["project_launches"]}


@pytest.mark.parametrize("fixed_order", [False, True])
@pytest.mark.parametrize("tile", [0, 64])
def test_relaxation_matches_reference(monkeypatch, tile, fixed_order):
    """One nested relaxation of the twelve tilt-dependent modules next to the tilt_thetaB_boundary_in constraint on the
    84-vertex annulus, CG with the Jacobi preconditioner: the reference's evaluation counts, one launch of every add-on
    per evaluation, its fields and energy, and every lane that cannot carry the stack declined."""
    from membrane_solver_amd.geometry.mesh import ArrayMesh
    from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager
    from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager
    from membrane_solver_amd.runtime.minimizer import Minimizer
    from membrane_solver_amd.runtime.steppers import GradientDescent

    _set_mode(monkeypatch, fixed_order)
    g = load_golden(RELAX_FILE)
    mods = [str(m) for m in g["modules"]]
    mesh = ArrayMesh(g["positions"], g["tri"], fixed=g["fixed"], tilts_in=g["tilts_in0"], tilts_out=g["tilts_out0"],
                     tilt_fixed_in=g["tilt_fixed_in"], global_parameters=json.loads(str(g["gp_json"])), energy_modules=mods,
                     constraint_modules=[CONSTRAINT], edges=g["edges"], vertex_options=_opts(g["vopts"]))
    mz = Minimizer(mesh, mesh.global_parameters, GradientDescent(), EnergyModuleManager(mods),
                   ConstraintModuleManager([CONSTRAINT]), quiet=True, tile_vertices=tile)
    _mir, dm = mz._device()
    assert mz._tbb_active
    if tile:
        assert dm.tile_stats()["n_tiles"] == 2
    dm.energy()  # (leaves the bending_tilt record the relaxation would otherwise take first)
    before = _launches(dm)
    iters, evals = dm.relax_leaflet_tilts(**mz._tilt_relax_params())
    after = _launches(dm)
    d = {k: after[k] - before[k] for k in after}
    tin, tout = dm.get_leaflet_tilts("in"), dm.get_leaflet_tilts("out")
    E = float(dm.energy().sum())
    n_grad, n_en = int(g["n_gradient_evaluations"]), int(g["n_energy_evaluations"])
    print("tile", tile, "fixed order", fixed_order, "iters", iters, "accepted", int(g["accepted_steps"]), "evals", evals, "ref",
          n_grad, n_en, "E", E, "ref", float(g["E_total"]), "fields", relerr(tin, g["tilts_in_final"]),
          relerr(tout, g["tilts_out_final"]), "bars", bar(g, "noise_tilts"), bar(g, "noise_energy"), "launches", d)
    assert evals == n_grad + n_en
    # (the reference stops in its 36th iteration, whose search finds no descent: one gradient evaluation per iteration begun)
    assert iters == n_grad == int(g["accepted_steps"]) + 1 and str(g["stop_reason"]) == "line_search_rejected"
    assert d == {"rim_in": evals, "rim_out": evals, "rim_bilayer": evals, "coupling": evals, "contact": evals,
                 "splay_energy": n_en, "splay_gradient": n_grad, "project": n_grad}
    assert relerr(tin, g["tilts_in_final"]) <= bar(g, "noise_tilts")
    assert relerr(tout, g["tilts_out_final"]) <= bar(g, "noise_tilts")
    assert abs(E - float(g["E_total"])) <= bar(g, "noise_energy") * abs(float(g["E_total"]))
    bd = mz.compute_energy_breakdown()
    scale = float(np.sum(np.abs(g["breakdown"])))
    for m, ref in zip(mods, g["breakdown"].tolist()):
        assert abs(bd[m] - ref) <= bar(g, "noise_energy") * scale, m
    st = dm.exec_stats()
    assert st["relax_fused"] == 0 and st["relax_programs"] == 0 and dm.tsearch_stats()["passes"] == 0
    fin = g["tilt_fixed_in"]
    assert np.max(np.abs(tin[fin] - g["tilts_in0"][fin])) <= 1e-15
    dm.close()


# -- trajectories ----------------------------------------------------------------------------------------------------------
def _minimizer(g, kind, observe, tile=0, deterministic=None):
    from membrane_solver_amd.geometry.mesh import ArrayMesh
    from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager
    from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager
    from membrane_solver_amd.runtime.minimizer import Minimizer
    from membrane_solver_amd.runtime.steppers import ConjugateGradient, GradientDescent

    mods = [str(m) for m in g["modules"]]
    cons = [str(m) for m in g["constraint_modules"]]
    mesh = ArrayMesh(g["positions0"], g["tri"], fixed=g["fixed"], surface_tension=g["gamma"], tilts_in=g["tilts_in0"],
                     tilts_out=g["tilts_out0"], tilt_fixed_in=g["tilt_fixed_in"], tilt_fixed_out=g["tilt_fixed_out"],
                     global_parameters=json.loads(str(g["gp_json"])), energy_modules=mods, constraint_modules=cons,
                     edges=g["edges"], vertex_options=_opts(g["vopts"]))
    stepper = GradientDescent() if kind == "gd" else ConjugateGradient()
    log, trials = [], []
    mz = Minimizer(mesh, mesh.global_parameters, stepper, EnergyModuleManager(mods), ConstraintModuleManager(cons),
                   quiet=True, step_size=float(g["step_size0"]), tile_vertices=tile, deterministic=deterministic)
    if observe:
        orig = stepper.device_step

        def logged(dm, m, step_size, tol=0.0):
            r = orig(dm, m, step_size, tol=tol)
            log.append((float(r.success), r.next_step, r.energy))
            trials.append(r.trials)
            return r

        stepper.device_step = logged
    mz.step_trials = trials
    return mesh, mz, log


def _finals(mesh, res):
    return (mesh.positions_view().copy(), np.array(mesh.tilts_in_view()).copy(), np.array(mesh.tilts_out_view()).copy(),
            res["energy"])


@pytest.mark.parametrize("fixed_order", [False, True])
@pytest.mark.parametrize("tile", [0, 64])
@pytest.mark.parametrize("fname", sorted(TRAJ))
def test_minimizer_reproduces_trajectory(monkeypatch, fname, tile, fixed_order):
    """The observed Python loop and ms_minimize against the reference: its accept / reject sequence and step sizes exactly,
    its energies and finals within the noise bar; in fixed-order mode the two loops give the same bits."""
    _set_mode(monkeypatch, fixed_order)
    g = load_golden(fname)
    pinned = "pin_to_circle" in [str(c) for c in g["constraint_modules"]]
    finals = []
    for observe in (True, False):
        mesh, mz, log = _minimizer(g, TRAJ[fname], observe=observe, tile=tile)
        if observe:
            E0, grad0 = mz.compute_energy_and_gradient_array()
            assert abs(E0 - g["E0"]) <= 1e-12 * abs(g["E0"]) and relerr(grad0, g["grad0"]) < 1e-10
        res = mz.minimize(int(g["n_steps"]))
        assert mz._has_enforceable_constraints == pinned and mz._pins_active == pinned
        assert mz._tbb_active == (CONSTRAINT in [str(c) for c in g["constraint_modules"]])
        if observe:
            got, ref = np.array(log), g["step_log"]
            print(fname, "tile", tile, "fixed order", fixed_order, "got", got.tolist(), "ref", ref.tolist())
            print(fname, "energy deviations", (np.abs(got[:, 2] - ref[:, 2]) / np.abs(ref[:, 2])).tolist(), "bar",
                  bar(g, "noise_energy"))
            assert got.shape == ref.shape
            assert np.array_equal(got[:, 0], ref[:, 0]), "accept/reject sequence differs from the reference"
            assert np.allclose(got[:, 1], ref[:, 1], rtol=1e-12, atol=0), "step sizes differ from the reference"
            assert np.allclose(got[:, 2], ref[:, 2], rtol=bar(g, "noise_energy"), atol=0)
            assert np.array_equal(np.array(mz.step_trials) + 1, g["line_search_evals"])
            bd = mz.compute_energy_breakdown()
            assert abs(sum(bd.values()) - res["energy"]) <= 1e-12 * sum(abs(v) for v in bd.values())
        else:
            assert mz._fast_path_ok(None) and mz.last_run["iterations"] == int(g["n_steps"])
            assert mz.last_run["trials"] + int(g["n_steps"]) == int(g["line_search_evals"].sum())
        print(fname, "observe", observe, "finals x", relerr(mesh.positions_view(), g["positions_final"]), "t",
              relerr(mesh.tilts_in_view(), g["tilts_in_final"]), relerr(mesh.tilts_out_view(), g["tilts_out_final"]), "E",
              abs(res["energy"] - float(g["E_final"])) / abs(float(g["E_final"])), "bars", bar(g, "noise_positions"),
              bar(g, "noise_tilts"), bar(g, "noise_energy"))
        assert relerr(mesh.positions_view(), g["positions_final"]) <= bar(g, "noise_positions")
        assert relerr(mesh.tilts_in_view(), g["tilts_in_final"]) <= bar(g, "noise_tilts")
        assert relerr(mesh.tilts_out_view(), g["tilts_out_final"]) <= bar(g, "noise_tilts")
        assert abs(res["energy"] - float(g["E_final"])) <= bar(g, "noise_energy") * abs(float(g["E_final"]))
        finals.append(_finals(mesh, res))
    if fixed_order:
        for x, y in zip(*finals):  # the same launches in the same order: the same bits
            assert np.array_equal(x, y)


@pytest.mark.parametrize("fname", sorted(TRAJ))
def test_interpreter_on_and_off_give_the_same_bits(monkeypatch, fname):
    """One tile, fixed-order mode: MS_EXEC=0 and the default give bitwise equal trajectories -- the add-ons' passes flush
    the one-workgroup interpreter's recorder and launch on their own, so the rest of a pack is as without them."""
    _set_mode(monkeypatch, True)
    g = load_golden(fname)
    runs = []
    for exec_off in (False, True):
        if exec_off:
            monkeypatch.setenv("MS_EXEC", "0")
        else:
            monkeypatch.delenv("MS_EXEC", raising=False)
        mesh, mz, _log = _minimizer(g, TRAJ[fname], observe=False)
        res = mz.minimize(int(g["n_steps"]))
        ex = mesh._hip_mirror.dm.exec_stats()
        runs.append((_finals(mesh, res), ex))
    (a, ex_a), (b, ex_b) = runs
    print(fname, ex_a, ex_b)
    assert ex_a["active"] and not ex_b["active"]
    assert ex_a["relax_programs"] == 0 and ex_a["relax_fused"] == 0
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
