"""tilt_thetaB_boundary_in on the HIP path (csrc/ms_thetab_bnd.hip: k_tbb_geom, k_tbb_apply): every case of
thetab_boundary_cases.npz through the C ABI, the twelve leaflet relaxations on the annulus and the two reference
trajectories (tools/gen_golden_thetab_boundary.py).

Bars.  d within 1e-11, keep exact: N_v carries a few ulp, d = r_hat - (r_hat . N_v) N_v is divided by |d| >= 1e-3 (the
generator asserts that margin), so a few 1e-16 / 1e-3 with a tenfold margin.  Enforced rows and |t . d - theta_B| within
1e-10; projected gradients within the project's 1e-10 of the largest entry; relaxations: counts exact, fields within
1e-11; trajectories: decisions and step sizes exact, energies within 1e-12."""

import json

import numpy as np
import pytest

from conftest import load_golden, relerr
from test_thetab_boundary_host import CASES, NAME, NAMES, TRAJ, case_mesh

pytestmark = pytest.mark.gpu

ACTIVE = [n for n in NAMES if n not in ("no_group", "no_rows")]
KIND = {TRAJ[0]: "cg", TRAJ[1]: "gd", TRAJ[2]: "cg"}
RELAX = load_golden("thetab_boundary_relax.npz")
LABELS = [str(x) for x in RELAX["labels"]]


def _device(name, tile=0, deterministic=False):
    from membrane_solver_amd import _lib as L
    from membrane_solver_amd.device import DeviceMesh

    P, T, tin, tout, fin, fout, gp, _vo = case_mesh(name)
    dm = DeviceMesh(P, T, tile_vertices=tile)
    dm.set_deterministic(deterministic)
    dm.set_leaflet_tilts("in", tin, tilt_fixed=fin, tilt_modulus=gp["tilt_modulus_in"])
    dm.set_leaflet_tilts("out", tout, tilt_fixed=fout, tilt_modulus=gp["tilt_modulus_out"])
    dm.set_thetab_boundary(CASES[name + "__rows"], center=gp.get("tilt_thetaB_center", (0.0, 0.0, 0.0)),
                           normal=gp["tilt_thetaB_normal"])
    dm.set_thetab_value(float(gp.get("tilt_thetaB_value") or 0.0))
    dm.set_params(modules=L.MS_MOD_TILT_IN | L.MS_MOD_TILT_OUT)
    return dm, P, tin, tout, fin, fout, gp


@pytest.mark.parametrize("name", ["no_group", "no_rows"])
def test_cases_that_do_nothing(name):
    """No group, or nobody carries it: the Python layer uploads no table; a table without a row does nothing."""
    from membrane_solver_amd.device import DeviceMesh
    from membrane_solver_amd.geometry.mesh import ArrayMesh
    from membrane_solver_amd.modules.constraints import tilt_thetaB_boundary_in as module

    P, T, tin, tout, _fin, _fout, gp, vo = case_mesh(name)
    assert module.device_params(ArrayMesh(P, T, global_parameters=gp, vertex_options=vo), gp) is None
    assert not CASES[name + "__keep"].any()
    dm = DeviceMesh(P, T)
    dm.set_leaflet_tilts("in", tin, tilt_modulus=1.0)
    dm.set_leaflet_tilts("out", tout, tilt_modulus=1.0)
    dm.set_thetab_boundary([], normal=(0.0, 0.0, 1.0))
    dm.thetab_boundary_enforce()
    d, keep = dm.thetab_boundary_directions()
    assert d.shape == (0, 3) and keep.shape == (0,)
    assert np.array_equal(dm.get_leaflet_tilts("in"), tin)
    assert dm.thetab_boundary_stats() == {"geom_launches": 0, "enforce_launches": 0, "project_launches": 0}
    dm.close()


@pytest.mark.parametrize("tile", [0, 64])
@pytest.mark.parametrize("name", ACTIVE)
def test_directions_enforcement_and_projection(name, tile):
    """The three new entry points against the reference, default tiles and 64-vertex tiles (the ring's rows spread over
    tiles, the row permutation)."""
    g = CASES
    dm, P, tin, tout, fin, fout, gp = _device(name, tile)
    rows = g[name + "__rows"].astype(np.int64)
    keep_ref, d_ref = g[name + "__keep"], g[name + "__d"]
    theta = float(gp.get("tilt_thetaB_value") or 0.0)
    if len(P) > 5000:
        assert dm.tile_stats()["n_tiles"] >= 2
    d, keep = dm.thetab_boundary_directions()
    print(name, tile, "d", float(np.max(np.abs(d - d_ref))), "kept", int(keep.sum()), "of", len(rows))
    assert np.array_equal(keep, keep_ref)
    assert np.max(np.abs(d - d_ref)) <= 1e-11 and not d[~keep].any()
    # -- the projected gradient of the stored (not yet enforced) tilts, next to the raw one
    E_raw, gi_raw, go_raw = dm.leaflet_tilt_energy_and_gradient()
    E, gi, go = dm.thetab_boundary_projected_gradient()
    raw_ref, prj_ref = g[name + "__ring_grad_raw"], g[name + "__ring_grad_projected"]
    big = float(np.max(np.abs(raw_ref)))
    print(name, tile, "E", E, "ref", float(g[name + "__E"]), "raw", float(np.max(np.abs(gi_raw[rows] - raw_ref))) / big,
          "projected", float(np.max(np.abs(gi[rows] - prj_ref))) / big)
    assert E == E_raw and abs(E - float(g[name + "__E"])) <= 1e-12 * abs(float(g[name + "__E"]))
    assert np.max(np.abs(gi_raw[rows] - raw_ref)) <= 1e-10 * big
    assert np.max(np.abs(gi[rows] - prj_ref)) <= 1e-10 * big
    free = keep_ref & ~fin[rows]
    expect = gi_raw.copy()
    expect[fin] = 0.0
    off = np.ones(len(P), bool)
    off[rows[free]] = False
    assert np.array_equal(gi[off], expect[off]), "rows the constraint does not own: the raw gradient, fixed rows zeroed"
    expect_o = go_raw.copy()
    expect_o[fout] = 0.0
    assert np.array_equal(go, expect_o)
    if free.any():
        assert np.max(np.abs(np.einsum("ij,ij->i", gi[rows], d_ref)[free])) <= 1e-10 * big
    # -- the enforcement
    dm.thetab_boundary_enforce()
    got, got_o = dm.get_leaflet_tilts("in"), dm.get_leaflet_tilts("out")
    resid = np.einsum("ij,ij->i", got[rows], d_ref)[free] - theta
    print(name, tile, "enforced", float(np.max(np.abs(got[rows] - g[name + "__ring_enforced"]))), "residual",
          float(np.max(np.abs(resid))) if free.any() else 0.0)
    assert np.max(np.abs(got[rows] - g[name + "__ring_enforced"])) <= 1e-10
    if free.any():
        assert np.max(np.abs(resid)) <= 1e-10
    assert np.array_equal(got[off], tin[off]), "non-ring rows, fixed rows and dropped rows: bitwise unchanged"
    assert np.array_equal(got_o, tout) and np.array_equal(dm.get_positions(), P)
    st = dm.thetab_boundary_stats()
    assert st == {"geom_launches": 3, "enforce_launches": 1, "project_launches": 1}  # (x is not frozen: every call forms d)
    dm.close()


@pytest.mark.parametrize("name", ["n001", "n065", "n257", "fixed_rows", "flat_d_zero"])
def test_both_deterministic_modes_give_the_same_bits(name):
    """Rows are distinct and nothing is summed: the three entry points are bitwise equal in both modes of
    ms_set_deterministic and from one context to the next.  The projection's INPUT, the raw gradient, carries the tile
    kernels' vertex-area sums, which are ordered in fixed-order mode only; so every context evaluates raw and projected
    gradient in its own mode, and the projected rows are compared wherever the raw rows agree bit for bit -- which has to
    be the case on the ring's free rows of the two fixed-order contexts at least."""
    rows = CASES[name + "__rows"].astype(np.int64)
    seen = []
    for det in (False, True, True):
        dm, _P, _tin, _tout, fin, *_rest = _device(name, 64, det)
        d, keep = dm.thetab_boundary_directions()
        dm.thetab_boundary_enforce()
        t = dm.get_leaflet_tilts("in")
        _E, raw, _go = dm.leaflet_tilt_energy_and_gradient()
        _E, gi, _go = dm.thetab_boundary_projected_gradient()
        seen.append((d, keep, t, raw, gi))
        dm.close()
    free = rows[seen[0][1] & ~fin[rows]]
    for k, other in enumerate(seen[1:], 1):
        for a, b in zip(seen[0][:3], other[:3]):
            assert np.array_equal(a, b)
        same_in = np.all(seen[0][3] == other[3], axis=1)
        print(name, "context", k, "raw gradient rows equal bit for bit", int(same_in.sum()), "of", len(same_in),
              "free ring rows among them", int(same_in[free].sum()), "of", len(free))
        assert np.array_equal(seen[0][4][same_in], other[4][same_in])
    same_det = np.all(seen[1][3] == seen[2][3], axis=1)
    assert same_det.all() and np.array_equal(seen[1][4], seen[2][4])
    # the projection changed those rows in every mode
    for d, keep, t, raw, gi in seen:
        if len(free):
            assert np.any(gi[free] != raw[free])


def test_setter_refusals_and_clearing():
    from membrane_solver_amd import _lib as L

    dm, P, tin, *_rest = _device("n003")
    d0, _k = dm.thetab_boundary_directions()
    ok = {"rows": [1, 2, 3]}
    for bad, why in (({"rows": [1, 2, 1]}, "listed twice"), ({"rows": [1, len(P)]}, "out of range"),
                     ({"rows": [-1, 2]}, "out of range"), ({"center": (0.0, np.inf, 0.0)}, "must be finite"),
                     ({"normal": (np.nan, 0.0, 1.0)}, "must be finite"), ({"normal": (0.0, 0.0, 0.0)}, "non-zero plane normal")):
        with pytest.raises(L.MembraneHipError, match=why):
            dm.set_thetab_boundary(**dict(ok, **bad))
        d1, _k = dm.thetab_boundary_directions()
        assert np.array_equal(d1, d0), "a refused call leaves the table in use as it was"
    with pytest.raises(ValueError, match="tilt_projection_cadence"):
        dm.set_tilt_projection("sometimes", 1)
    with pytest.raises(ValueError, match="tilt_projection_interval"):
        dm.set_tilt_projection("per_step", 0)
    for args, why in (((2, 1), "cadence must be"), ((0, 0), "interval must be >= 1")):
        assert L.lib().ms_set_tilt_projection(dm._h, *args) != 0 and why in L.lib().ms_last_error(dm._h).decode()
    dm.set_thetab_boundary(None)
    with pytest.raises(L.MembraneHipError, match="never called"):
        dm.thetab_boundary_enforce()
    dm.set_thetab_boundary(np.arange(len(P)))  # every vertex a ring row: no size limit
    dm.thetab_boundary_enforce()
    assert np.all(np.isfinite(dm.get_leaflet_tilts("in")))
    dm.close()


# -- relaxations -----------------------------------------------------------------------------------------------------------
def _opts(text):
    return {int(k): v for k, v in json.loads(str(text)).items()}


def _relax(label, deterministic=None):
    from membrane_solver_amd.geometry.mesh import ArrayMesh
    from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager
    from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager
    from membrane_solver_amd.runtime.minimizer import Minimizer
    from membrane_solver_amd.runtime.steppers import GradientDescent

    g = RELAX
    mods = [str(m) for m in g[label + "__modules"]]
    mesh = ArrayMesh(g["positions"], g["tri"], fixed=g["fixed"], tilts_in=g[label + "__tilts_in0"],
                     tilts_out=g[label + "__tilts_out0"], tilt_fixed_in=g[label + "__tilt_fixed_in"],
                     global_parameters=json.loads(str(g[label + "__gp_json"])), energy_modules=mods,
                     constraint_modules=[NAME], edges=g["edges"], vertex_options=_opts(g["vopts"]))
    mz = Minimizer(mesh, mesh.global_parameters, GradientDescent(), EnergyModuleManager(mods),
                   ConstraintModuleManager([NAME]), quiet=True, deterministic=deterministic)
    _mir, dm = mz._device()
    dm.energy()  # (leaves the bending_tilt record the relaxation would otherwise take first)
    before = dm.thetab_boundary_stats()
    iters, evals = dm.relax_leaflet_tilts(**mz._tilt_relax_params())
    after = dm.thetab_boundary_stats()
    return mz, dm, iters, evals, {k: after[k] - before[k] for k in after}


@pytest.mark.parametrize("label", LABELS)
def test_relaxation_matches_reference(label):
    """40 iterations on the 84-vertex annulus, GD and Jacobi CG, the three projection schedules, with and without the
    contact module: the reference's counts, its fields, and the launches the code makes -- one geometry launch (x is
    frozen), an enforcement at the start and at the end and one per scheduled refresh, one projection per gradient."""
    g = RELAX
    mz, dm, iters, evals, d = _relax(label)
    assert mz._tbb_active and not mz._has_enforceable_constraints
    tin, tout = dm.get_leaflet_tilts("in"), dm.get_leaflet_tilts("out")
    E = float(dm.energy().sum())
    n_grad, n_en = int(g[label + "__n_gradient_evaluations"]), int(g[label + "__n_energy_evaluations"])
    accepted, refreshes = int(g[label + "__accepted_steps"]), int(g[label + "__projection_apply_count"])
    print(label, "iters", iters, "evals", evals, "ref", n_grad, n_en, "E", E, "ref", float(g[label + "__E_total"]), "fields",
          relerr(tin, g[label + "__tilts_in_final"]), relerr(tout, g[label + "__tilts_out_final"]), "launches", d)
    assert iters == int(g[label + "__tilt_inner_steps"]) == accepted
    assert evals == n_grad + n_en
    assert relerr(tin, g[label + "__tilts_in_final"]) <= 1e-11 and relerr(tout, g[label + "__tilts_out_final"]) <= 1e-11
    assert abs(E - float(g[label + "__E_total"])) <= 1e-11 * abs(float(g[label + "__E_total"]))
    st = dm.exec_stats()
    assert st["relax_fused"] == 0 and st["relax_programs"] == 0, "the one-tile programs decline the constraint"
    assert d == {"geom_launches": 1, "enforce_launches": 2 + refreshes, "project_launches": n_grad}
    ring = g["ring"].astype(np.int64)
    free = ~g[label + "__tilt_fixed_in"][ring]
    dirs, keep = dm.thetab_boundary_directions()
    assert keep.all() and np.max(np.abs(np.einsum("ij,ij->i", tin[ring], dirs)[free] - 0.15)) <= 1e-10


@pytest.mark.parametrize("label", ["gd_step2_plain", "cg_step1_contact"])
def test_relaxation_without_the_search_pass_is_the_same(label, monkeypatch):
    """MS_TSEARCH=0 (every trial a pass of its own): the same counts and, in fixed-order mode, the same bits -- the trial
    rows are the same doubles at every site that forms them."""
    _mz, dm, iters, evals, d = _relax(label, deterministic=True)
    a = (dm.get_leaflet_tilts("in"), dm.get_leaflet_tilts("out"))
    monkeypatch.setenv("MS_TSEARCH", "0")
    _mz2, dm2, iters2, evals2, d2 = _relax(label, deterministic=True)
    assert dm2 is not dm and dm2.tsearch_stats()["passes"] == 0
    assert (iters2, evals2, d2) == (iters, evals, d)
    assert np.array_equal(dm2.get_leaflet_tilts("in"), a[0]) and np.array_equal(dm2.get_leaflet_tilts("out"), a[1])


def test_relaxation_without_the_constraint_keeps_its_fast_lanes():
    """The same context with the table cleared: the fused evaluator / the relaxation program run as before."""
    mz, dm, _iters, _evals, _d = _relax("cg_step1_plain")
    dm.set_thetab_boundary(None)
    before = dm.thetab_boundary_stats()
    _it, evals = dm.relax_leaflet_tilts(**mz._tilt_relax_params())
    st = dm.exec_stats()
    assert evals > 0 and st["relax_fused"] + st["relax_programs"] > 0
    assert dm.thetab_boundary_stats() == before


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
    log, counts = [], []
    mz = Minimizer(mesh, mesh.global_parameters, stepper, EnergyModuleManager(mods), ConstraintModuleManager(cons),
                   quiet=True, step_size=float(g["step_size0"]), tile_vertices=tile, deterministic=deterministic)
    if observe:
        orig = stepper.device_step

        def logged(dm, m, step_size, tol=0.0):
            before = dm.thetab_boundary_stats()
            r = orig(dm, m, step_size, tol=tol)
            after = dm.thetab_boundary_stats()
            log.append((float(r.success), r.next_step, r.energy))
            counts.append((r.trials, r.guard_rejects) + tuple(after[k] - before[k] for k in
                                                              ("geom_launches", "enforce_launches", "project_launches")))
            return r

        stepper.device_step = logged
    mz.step_counts = counts
    return mesh, mz, log


@pytest.mark.parametrize("fname", TRAJ)
def test_minimizer_reproduces_trajectory(fname):
    """The Python loop (observed steps) and ms_minimize: the reference's decisions and step sizes exactly, its energies
    within 1e-12.  Next to the pins every evaluated trial of a search gets the pin program, one geometry launch on the
    enforced trial and one P(enforce(t)) launch -- a trial the step-length guard refuses is never enforced; alone the
    constraint launches nothing inside a search."""
    g = load_golden(fname)
    pinned = "pin_to_circle" in [str(c) for c in g["constraint_modules"]]
    for observe in (True, False):
        mesh, mz, log = _minimizer(g, KIND[fname], observe=observe)
        if observe:
            E0, grad0 = mz.compute_energy_and_gradient_array()
            assert abs(E0 - g["E0"]) <= 1e-12 * abs(g["E0"]) and relerr(grad0, g["grad0"]) < 1e-10
        res = mz.minimize(int(g["n_steps"]))
        assert mz._tbb_active and mz._has_enforceable_constraints == pinned
        if observe:
            got, ref = np.array(log), g["step_log"]
            print(fname, "got", got.tolist(), "ref", ref.tolist())
            print(fname, "energy deviations", (np.abs(got[:, 2] - ref[:, 2]) / np.abs(ref[:, 2])).tolist())
            assert got.shape == ref.shape
            assert np.array_equal(got[:, 0], ref[:, 0]), "accept/reject sequence differs from the reference"
            assert np.array_equal(got[:, 1], ref[:, 1]), "step sizes differ from the reference"
            assert np.allclose(got[:, 2], ref[:, 2], rtol=1e-12, atol=0)
            cnt = np.array(mz.step_counts)
            print(fname, "trials, guard rejects, geom, enforce, project per step", cnt.tolist(), "ref evals",
                  g["line_search_evals"].tolist())
            assert np.array_equal(cnt[:, 0] + 1, g["line_search_evals"])
            want = cnt[:, 0] if pinned else 0 * cnt[:, 0]
            assert np.array_equal(cnt[:, 2], want) and np.array_equal(cnt[:, 3], want) and not cnt[:, 4].any()
        else:
            assert mz._fast_path_ok(None) and mz.last_run["iterations"] == int(g["n_steps"])
            assert mz.last_run["trials"] + int(g["n_steps"]) == int(g["line_search_evals"].sum())
        print(fname, observe, "finals x", relerr(mesh.positions_view(), g["positions_final"]), "t",
              relerr(mesh.tilts_in_view(), g["tilts_in_final"]), relerr(mesh.tilts_out_view(), g["tilts_out_final"]), "E",
              abs(res["energy"] - float(g["E_final"])) / abs(float(g["E_final"])))
        assert abs(res["energy"] - float(g["E_final"])) <= 1e-12 * abs(float(g["E_final"]))
        bar = max(1e-12, 10.0 * float(g["noise_tilts"]), 10.0 * float(g["noise_positions"]))  # (the fixture's own spread)
        assert relerr(mesh.positions_view(), g["positions_final"]) <= bar
        assert relerr(mesh.tilts_in_view(), g["tilts_in_final"]) <= bar
        assert relerr(mesh.tilts_out_view(), g["tilts_out_final"]) <= bar


@pytest.mark.parametrize("fname", TRAJ)
def test_library_loop_against_the_python_loop(fname, monkeypatch):
    """ms_minimize against the Python loop stepping the same context calls: in fixed-order mode the same bits."""
    monkeypatch.setenv("MS_DETERMINISTIC", "1")
    g = load_golden(fname)
    mesh_p, mz_p, _log = _minimizer(g, KIND[fname], observe=True)
    res_p = mz_p.minimize(int(g["n_steps"]))
    assert not mz_p._fast_path_ok(None)  # (the observed stepper)
    mesh_l, mz_l, _log2 = _minimizer(g, KIND[fname], observe=False)
    res_l = mz_l.minimize(int(g["n_steps"]))
    assert mz_l._fast_path_ok(None) and mz_l.last_run["iterations"] == int(g["n_steps"])
    assert np.array_equal(mesh_p.positions_view(), mesh_l.positions_view())
    assert np.array_equal(mesh_p.tilts_in_view(), mesh_l.tilts_in_view())
    assert np.array_equal(mesh_p.tilts_out_view(), mesh_l.tilts_out_view())
    assert res_p["energy"] == res_l["energy"]
    assert mz_l.last_run["trials"] == sum(c[0] for c in mz_p.step_counts)


def test_rejected_trials_leave_the_tilts_of_x_untouched():
    """A pinned search whose every trial is rejected (an Armijo constant no trial can meet): each trial was enforced --
    pins, geometry, P(enforce(t)) into the trial buffer -- and the stored fields are bit for bit what the same search
    leaves on a context without the constraint: the tilts of x as the search's own projection at x wrote them."""
    from membrane_solver_amd import _lib as L

    g = load_golden(TRAJ[0])
    fields = []
    for with_table in (True, False):
        mesh, mz, _log = _minimizer(g, "cg", observe=False, deterministic=True)
        _mir, dm = mz._device()
        assert mz._pins_active
        if not with_table:
            dm.set_thetab_boundary(None)
        x0 = dm.get_positions()
        before = dm.thetab_boundary_stats()
        r = dm.step(stepper=L.MS_STEPPER_CG, step_size=1e-3, tol=0.0, max_iter=3, c=1e9, enforce_pins=1)
        after = dm.thetab_boundary_stats()
        assert not r.success and r.trials == 3 and r.guard_rejects == 0
        delta = {k: after[k] - before[k] for k in after}
        assert delta == ({"geom_launches": 3, "enforce_launches": 3, "project_launches": 0} if with_table else
                         {"geom_launches": 0, "enforce_launches": 0, "project_launches": 0})
        assert np.array_equal(dm.get_positions(), x0)
        fields.append((dm.get_leaflet_tilts("in"), dm.get_leaflet_tilts("out")))
    assert np.array_equal(fields[0][0], fields[1][0]) and np.array_equal(fields[0][1], fields[1][1])
