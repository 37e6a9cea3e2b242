"""tilt_thetaB_contact_in on the HIP path (csrc/ms_thetab.hip: k_thetab_geom, k_thetab_apply): every case of
thetab_contact_cases.npz through the C ABI and through the plugin against the reference's module, the slot rules next to
tilt_in, the two leaflet relaxations and the three reference trajectories (tools/gen_golden_thetab_contact.py).
Bars: energies and the three scalars to 1e-12 relative, every tilt-gradient entry within 1e-10 of the largest;
relaxations and trajectories within max(1e-12, 10 x noise), noise being what a 1e-13 perturbation of the start moves in
the reference's own run (the fixtures record it)."""

import json

import numpy as np
import pytest

from conftest import load_golden, relerr
from test_thetab_contact_host import GA, K, TB, TRAJ, case_mesh

pytestmark = pytest.mark.gpu

NAME = "tilt_thetaB_contact_in"
CASES = load_golden("thetab_contact_cases.npz")
NAMES = [str(n) for n in CASES["names"]]
KIND = {TRAJ[0]: "gd", TRAJ[1]: "cg", TRAJ[2]: "gd"}


def _bar(g, key):
    return max(1e-12, 10.0 * float(g[key]))


def _abi_params(name, gp):
    """kwargs of DeviceMesh.set_thetab_contact straight from the case's parameters (k == gamma == 0 included: the
    Python layer would switch the module off)"""
    from membrane_solver_amd.modules.energy import leaflet_common as lc

    work, pen = lc.thetab_contact_modes(gp)
    return {"rows": CASES[name + "__rows"], "center": gp.get("tilt_thetaB_center", [0.0, 0.0, 0.0]),
            "normal": gp["tilt_thetaB_normal"], "k": float(gp.get(K) or 0.0), "gamma": float(gp.get(GA) or 0.0),
            "work_mode": work, "penalty_mode": pen}


def _device(name, tile, deterministic, modules=None, tilt_modulus=0.0):
    from membrane_solver_amd import _lib as L
    from membrane_solver_amd.device import DeviceMesh

    P, T, tin, gp, _vo = case_mesh(name)
    dm = DeviceMesh(P, T, tile_vertices=tile)
    dm.set_deterministic(deterministic)
    dm.set_leaflet_tilts("in", tin, tilt_modulus=tilt_modulus)
    dm.set_leaflet_tilts("out", 0.1 + np.zeros_like(P), tilt_modulus=tilt_modulus)
    dm.set_thetab_contact(**_abi_params(name, gp))
    dm.set_thetab_value(gp[TB])
    dm.set_params(modules=L.MS_MOD_TILT_THETAB_CONTACT_IN if modules is None else modules)
    return dm, P, tin, gp


def _tagged(name):
    _P, _T, _tin, gp, vo = case_mesh(name)
    from membrane_solver_amd.modules.energy import leaflet_common as lc

    group = lc.thetab_contact_group(None, gp)
    return group is not None and any(group in (o.get("rim_slope_match_group"), o.get("tilt_thetaB_group")) for o in vo.values())


@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("tile", [0, 64])
@pytest.mark.parametrize("name", NAMES)
def test_case_through_the_c_abi(name, tile, deterministic):
    """Energy, energy-only == gradient call bit for bit, gradient rows, the outer gradient and the shape gradient
    untouched, the three scalars, the module's own energy, two runs bitwise equal -- default tiles and 64-vertex tiles
    (the ring's rows spread over tiles, the row permutation), both modes of ms_set_deterministic."""
    g = CASES
    if not _tagged(name):  # no group / nobody carries it: the plugin's business (test_plugin_matches_reference)
        from membrane_solver_amd.modules.energy import leaflet_common as lc
        from membrane_solver_amd.geometry.mesh import ArrayMesh

        P, T, _tin, gp, vo = case_mesh(name)
        assert lc.thetab_contact_params(ArrayMesh(P, T, global_parameters=gp, vertex_options=vo), None, gp) is None
        assert float(g[name + "__E"]) == 0.0
        return
    dm, P, _tin, _gp = _device(name, tile, deterministic)
    rows = g[name + "__rows"].astype(np.int64)
    E_ref, grad_ref, scal_ref = float(g[name + "__E"]), g[name + "__ring_grad"], g[name + "__scalars"]
    if len(P) > 5000:
        assert dm.tile_stats()["n_tiles"] >= 2
    e = dm.energy()
    own_e = dm.thetab_contact_energy()
    scal_e = dm.thetab_contact_scalars()
    E, gi, go = dm.leaflet_tilt_energy_and_gradient()
    own = dm.thetab_contact_energy()
    scal = dm.thetab_contact_scalars()
    e2, gshape = dm.energy_and_gradient(want_grad=True, raw=True)
    E_again, gi_again, _go = dm.leaflet_tilt_energy_and_gradient()
    big = max(float(np.max(np.abs(grad_ref))), 1e-300)
    print(name, tile, deterministic, "E", E, "ref", E_ref, "rel", abs(E - E_ref) / max(abs(E_ref), 1e-300), "grad",
          float(np.max(np.abs(gi[rows] - grad_ref))) / big, "scalars", scal, scal_ref.tolist())
    assert abs(E - E_ref) <= 1e-12 * abs(E_ref)
    assert e[3] == E == own == own_e == e2[3] == E_again, "energy-only, the gradient call and the getter: the same double"
    assert not e[:3].any()
    assert np.max(np.abs(gi[rows] - grad_ref)) <= 1e-10 * big
    rest = np.ones(len(P), bool)
    rest[rows] = False
    assert not gi[rest].any() and not go.any() and not gshape.any()
    assert np.array_equal(gi, gi_again) and scal == scal_e
    got = np.array([scal["theta_mean"], scal["r_eff"], scal["wsum"]])
    if scal_ref.any():
        assert np.max(np.abs(got - scal_ref) / np.abs(scal_ref)) <= 1e-12
    else:  # the ring contributes nothing (one row: no weight)
        assert not got.any() and E == 0.0 and not gi.any()
    st = dm.thetab_contact_stats()
    # x is not frozen: every evaluation orders the ring (energy_and_gradient may reuse the energy pass before it)
    assert st["geom_launches"] == st["apply_launches"] and 3 <= st["geom_launches"] <= 4
    dm.close()
    # a second context: the same bits
    dm2, _P, _t, _g = _device(name, tile, deterministic)
    E2, gi2, _go2 = dm2.leaflet_tilt_energy_and_gradient()
    assert E2 == E and np.array_equal(gi2, gi)
    dm2.close()


@pytest.mark.parametrize("name", NAMES)
def test_plugin_matches_reference(name):
    """Array, energy-only and dict APIs and update_scalar_params of the drop-in module."""
    from membrane_solver_amd.core.parameters import GlobalParameters, ParameterResolver
    from membrane_solver_amd.geometry.mesh import ArrayMesh
    from membrane_solver_amd.modules.energy import tilt_thetaB_contact_in as module

    g = CASES
    P, T, tin, gpd, vo = case_mesh(name)
    gp = GlobalParameters(gpd)
    mesh = ArrayMesh(P, T, global_parameters=gp, tilts_in=tin, vertex_options=vo)
    res = ParameterResolver(gp)
    rows = g[name + "__rows"].astype(np.int64)
    E_ref, grad_ref = float(g[name + "__E"]), g[name + "__ring_grad"]
    sentinel = np.arange(P.size, dtype=np.float64).reshape(P.shape)
    grad, go = sentinel.copy(), sentinel.copy()
    gi = np.zeros_like(P)
    kw = dict(positions=P.copy(), index_map=mesh.vertex_index_to_row)
    E = module.compute_energy_and_gradient_array(mesh, gp, res, grad_arr=grad, tilts_in=tin, tilts_out=np.zeros_like(P),
                                                 tilt_in_grad_arr=gi, tilt_out_grad_arr=go, **kw)
    E2 = module.compute_energy_array(mesh, gp, res, tilts_in=tin, **kw)
    assert np.array_equal(grad, sentinel) and np.array_equal(go, sentinel)
    assert abs(E - E_ref) <= 1e-12 * abs(E_ref) and E2 == E
    if E_ref == 0.0:
        assert E == 0.0 and not gi.any()
    else:
        assert np.max(np.abs(gi[rows] - grad_ref)) <= 1e-10 * np.max(np.abs(grad_ref))
    Ed, gd, tgi = module.compute_energy_and_gradient(mesh, gp, res)
    assert Ed == E and gd == {} and sorted(tgi) == [int(r) for r in np.flatnonzero(np.any(gi != 0.0, axis=1))]
    assert module.compute_energy_and_gradient(mesh, gp, res, compute_gradient=False) == (Ed, {})
    module.update_scalar_params(mesh, gp, res)
    tb_ref = float(g[name + "__thetaB_updated"])
    assert abs(float(gp.get(TB)) - tb_ref) <= 1e-12 * abs(tb_ref)


@pytest.mark.parametrize("tile", [0, 64])
@pytest.mark.parametrize("with_tilt_in", [False, True])
@pytest.mark.parametrize("name", ["n065", "mode_scalar_off", "n257"])
def test_define_versus_add(name, with_tilt_in, tile):
    """With tilt_in in front of it the term ADDS into the inner leaflet's cells, without it DEFINES them (every other
    cell zeroed: an evaluation with tilt_in before it left them all non-zero).  With and without the bit: energies[:3],
    the outer tilt gradient and the shape gradient bit-identical; energies[3] and the inner gradient differ by the
    reference's."""
    from membrane_solver_amd import _lib as L

    g = CASES
    bit = L.MS_MOD_TILT_THETAB_CONTACT_IN
    base = (L.MS_MOD_TILT_IN if with_tilt_in else 0) | L.MS_MOD_TILT_OUT | L.MS_MOD_SURFACE
    dm, P, tin, _gp = _device(name, tile, True, modules=L.MS_MOD_TILT_IN | L.MS_MOD_TILT_OUT | L.MS_MOD_SURFACE,
                              tilt_modulus=1.3)
    tin_all = tin + 0.05  # every tile's cell of the inner slot non-zero
    dm.set_leaflet_tilts("in", tin_all, tilt_modulus=1.3)
    assert dm.energy()[3] > 0.0
    dm.set_leaflet_tilts("in", tin, tilt_modulus=1.3)
    dm.set_params(modules=base)
    E0, gi0, go0 = dm.leaflet_tilt_energy_and_gradient()
    e0, g0 = dm.energy_and_gradient(want_grad=True, raw=True)
    dm.set_params(modules=base | bit)
    E1, gi1, go1 = dm.leaflet_tilt_energy_and_gradient()
    own_t = dm.thetab_contact_energy()
    e1, g1 = dm.energy_and_gradient(want_grad=True, raw=True)  # (phase_gradient rewrites the slot behind k_tilt<1>)
    own = dm.thetab_contact_energy()
    e2 = dm.energy()
    E_ref, grad_ref = float(g[name + "__E"]), g[name + "__ring_grad"]
    rows = g[name + "__rows"].astype(np.int64)
    tol = 1e-12 * (abs(E_ref) + abs(E0))
    print(name, with_tilt_in, tile, "dE", E1 - E0, e1[3] - e0[3], e2[3] - e0[3], "own", own, "ref", E_ref)
    assert abs((E1 - E0) - E_ref) <= tol and abs((e1[3] - e0[3]) - E_ref) <= tol and abs((e2[3] - e0[3]) - E_ref) <= tol
    assert abs(own - E_ref) <= 1e-12 * abs(E_ref) and own_t == own
    assert np.array_equal(e1[:3], e0[:3]) and np.array_equal(e2[:3], e0[:3])
    assert np.array_equal(g1, g0), "no shape gradient"
    assert np.array_equal(go1, go0), "the outer leaflet is not touched"
    d = gi1 - gi0
    big = float(np.max(np.abs(gi0))) if gi0.any() else 0.0
    if grad_ref.any():
        assert np.max(np.abs(d[rows] - grad_ref)) <= 1e-10 * np.max(np.abs(grad_ref)) + 4e-16 * big
    else:
        assert not d.any()
    dm.close()


def test_refusals():
    from membrane_solver_amd import _lib as L
    from membrane_solver_amd import meshgen
    from membrane_solver_amd.device import DeviceMesh

    P, T, _B = meshgen.disk_patch(38)  # 4447 vertices
    dm = DeviceMesh(P, T)
    dm.set_leaflet_tilts("in", np.zeros_like(P), tilt_modulus=1.0)
    dm.set_leaflet_tilts("out", np.zeros_like(P))
    bit = L.MS_MOD_TILT_THETAB_CONTACT_IN
    with pytest.raises(L.MembraneHipError, match="never called"):  # the bit without tables
        dm.set_params(modules=L.MS_MOD_TILT_IN | bit)
        dm.energy()
    ok = {"rows": [1, 2, 3], "k": 1.0, "gamma": 1.0}
    for bad, why in (({"rows": np.arange(4097)}, "a ring of 4097 rows is above the 4096"), ({"rows": [1, 2, 1]}, "listed twice"),
                     ({"rows": [1, len(P)]}, "out of range"), ({"rows": [-1, 2]}, "out of range"),
                     ({"k": np.nan}, "must be finite"), ({"gamma": np.inf}, "must be finite"),
                     ({"center": (0.0, np.inf, 0.0)}, "must be finite"), ({"normal": (np.nan, 0.0, 1.0)}, "must be finite"),
                     ({"normal": (0.0, 0.0, 0.0)}, "non-zero plane normal")):
        with pytest.raises(L.MembraneHipError, match=why):
            dm.set_thetab_contact(**dict(ok, **bad))
    with pytest.raises(L.MembraneHipError, match="must be finite"):
        dm.set_thetab_value(np.nan)
    dm.set_thetab_contact(np.arange(4096), k=1.0, gamma=1.0)  # the largest ring runs
    dm.set_params(modules=bit)
    E_big = dm.energy()[3]
    assert np.isfinite(E_big)
    with pytest.raises(L.MembraneHipError, match="listed twice"):  # a refused call leaves the table in use as it was
        dm.set_thetab_contact([1, 2, 1], k=1.0, gamma=1.0)
    assert dm.energy()[3] == E_big
    for bad in ({"work_mode": "linear"}, {"penalty_mode": "on"}):  # (the aliases are leaflet_common's to resolve)
        with pytest.raises(ValueError, match="set_thetab_contact"):
            dm.set_thetab_contact(**dict(ok, **bad))
    assert dm.energy()[3] == E_big
    with pytest.raises(L.MembraneHipError, match="single-field"):
        dm.set_params(modules=L.MS_MOD_TILT | bit)
    dm.set_thetab_contact(None)  # cleared: the bit is refused again
    dm.set_params(modules=bit)
    with pytest.raises(L.MembraneHipError, match="never called"):
        dm.energy()
    dm.close()


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
    cons = [str(m) for m in g["constraint_modules"]]
    mesh = ArrayMesh(g["positions0"], g["tri"], fixed=g["fixed"], surface_tension=g["gamma"], tilts_in=g["tilts_in0"],
                     tilts_out=g["tilts_out0"], tilt_fixed_in=g["tilt_fixed_in"], tilt_fixed_out=g["tilt_fixed_out"],
                     global_parameters=json.loads(str(g["gp_json"])), energy_modules=mods, constraint_modules=cons,
                     edges=g["edges"], vertex_options=_opts(g["vopts"]))
    stepper = GradientDescent() if kind == "gd" else ConjugateGradient()
    log, thetas, counts = [], [], []
    mz = Minimizer(mesh, mesh.global_parameters, stepper, EnergyModuleManager(mods), ConstraintModuleManager(cons),
                   quiet=True, step_size=float(g["step_size0"]), tile_vertices=tile, deterministic=deterministic)
    if observe:
        orig = stepper.device_step

        def logged(dm, m, step_size, tol=0.0):
            before = dm.thetab_contact_stats()
            r = orig(dm, m, step_size, tol=tol)
            after = dm.thetab_contact_stats()
            log.append((float(r.success), r.next_step, r.energy))
            counts.append((r.trials, r.guard_rejects, after["geom_launches"] - before["geom_launches"],
                           after["apply_launches"] - before["apply_launches"]))
            return r

        stepper.device_step = logged
    orig_u = mz._update_scalar_params

    def upd(dm):
        orig_u(dm)
        thetas.append(float(mesh.global_parameters.get(TB) or 0.0))

    mz._update_scalar_params = upd
    mz.step_counts = counts
    return mesh, mz, log, thetas


def _check_finals(mesh, res, g):
    print("    finals: x", relerr(mesh.positions_view(), g["positions_final"]), "bar", _bar(g, "noise_positions"),
          "t", relerr(mesh.tilts_in_view(), g["tilts_in_final"]), relerr(mesh.tilts_out_view(), g["tilts_out_final"]),
          "bar", _bar(g, "noise_tilts"), "E", abs(res["energy"] - float(g["E_final"])) / abs(float(g["E_final"])),
          "bar", _bar(g, "noise_energy"))
    assert relerr(mesh.positions_view(), g["positions_final"]) <= _bar(g, "noise_positions")
    assert relerr(mesh.tilts_in_view(), g["tilts_in_final"]) <= _bar(g, "noise_tilts")
    assert relerr(mesh.tilts_out_view(), g["tilts_out_final"]) <= _bar(g, "noise_tilts")
    assert abs(res["energy"] - float(g["E_final"])) <= _bar(g, "noise_energy") * abs(float(g["E_final"]))


@pytest.mark.parametrize("fname", TRAJ)
def test_minimizer_reproduces_trajectory(fname):
    """Observed steps (the Python loop) and unobserved ones (ms_minimize, or the Python loop again where theta_B is
    updated between steps): the reference's decisions, step sizes and theta_B sequence; energies and finals within the
    fixture's noise bar; the breakdown reports the module's own energy and sums to the total."""
    g = load_golden(fname)
    for observe in (True, False):
        mesh, mz, log, thetas = _minimizer(g, KIND[fname], observe=observe)
        if observe:
            E0, grad0 = mz.compute_energy_and_gradient_array()
            assert abs(E0 - g["E0"]) <= 1e-12 * abs(g["E0"])
            assert relerr(grad0, g["grad0"]) < 1e-10
        res = mz.minimize(int(g["n_steps"]))
        legacy = bool(mz._thetab_update)
        if not observe:
            assert mz._fast_path_ok(None) == (not legacy)
            if not legacy:  # ms_minimize: the same count over the whole run
                assert mz.last_run["trials"] + int(g["n_steps"]) == int(g["line_search_evals"].sum())
        if observe or legacy:
            tb = np.array(thetas)
            print(fname, "theta_B", tb.tolist(), "ref", g["thetaB_log"].tolist())
            assert tb.shape == g["thetaB_log"].shape
            assert np.allclose(tb, g["thetaB_log"], rtol=_bar(g, "noise_thetaB"), atol=0)
        assert abs(float(mesh.global_parameters.get(TB)) - float(g["thetaB_final"])) <= \
            _bar(g, "noise_thetaB") * abs(float(g["thetaB_final"]))
        if observe:
            got, ref = np.array(log), g["step_log"]
            print(fname, "got", got.tolist(), "ref", ref.tolist())
            assert got.shape == ref.shape
            assert np.array_equal(got[:, 0], ref[:, 0]), "accept/reject sequence differs from the reference"
            assert np.allclose(got[:, 1], ref[:, 1], rtol=1e-12, atol=0)
            assert np.allclose(got[:, 2], ref[:, 2], rtol=_bar(g, "noise_energy"), atol=0)
            # evaluation counts.  The reference's line search takes the module's energy once at x and once per trial it
            # puts to the Armijo test (the fixture's line_search_evals); a trial its step-length guard refuses is not
            # evaluated there, while the device has taken its energy pass by then (guard_rejects): trials + 1 is the
            # count both sides share.  Every evaluation of the step orders the ring: the trials, the guarded ones, the
            # energy at x, the re-add behind k_tilt<1> of the gradient pass and the accepted trial's commit.
            cnt = np.array(mz.step_counts)
            print(fname, "trials, guard rejects, geom, apply per step", cnt.tolist(), "ref", g["line_search_evals"].tolist())
            assert np.array_equal(cnt[:, 0] + 1, g["line_search_evals"])
            assert np.array_equal(cnt[:, 2], cnt[:, 0] + cnt[:, 1] + 3) and np.array_equal(cnt[:, 3], cnt[:, 2])
            bd = mz.compute_energy_breakdown()
            assert abs(sum(bd.values()) - res["energy"]) <= 1e-12 * abs(res["energy"])
            assert abs(bd[NAME] - float(g["E_own_final"])) <= _bar(g, "noise_energy") * abs(float(g["E_final"]))
        _check_finals(mesh, res, g)


def _run_final(g, kind, observe=False, **kw):
    mesh, mz, _log, thetas = _minimizer(g, kind, observe=observe, **kw)
    res = mz.minimize(int(g["n_steps"]))
    return (mesh.positions_view().copy(), np.array(mesh.tilts_in_view()).copy(), np.array(mesh.tilts_out_view()).copy(),
            res["energy"], float(mesh.global_parameters.get(TB)))


@pytest.mark.parametrize("fname", TRAJ)
def test_trajectory_is_bitwise_reproducible_in_both_modes(fname):
    g = load_golden(fname)
    for det in (False, True):
        a = _run_final(g, KIND[fname], tile=64, deterministic=det)
        b = _run_final(g, KIND[fname], tile=64, deterministic=det)
        if det:
            for x, y in zip(a, b):
                assert np.array_equal(x, y)
        else:  # (the tile kernels' LDS-atomic sums are not ordered; the module's own sums are: see the case tests)
            assert relerr(a[0], b[0]) < 1e-9


def test_observed_and_unobserved_loops_agree_on_the_legacy_trajectory(monkeypatch):
    """The run whose theta_B moves is handed to the Python loop whether its steps are observed or not: the same bits."""
    monkeypatch.setenv("MS_DETERMINISTIC", "1")
    g = load_golden(TRAJ[0])
    a = _run_final(g, "gd", observe=True)
    b = _run_final(g, "gd", observe=False)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("fname", TRAJ[1:])
def test_library_loop_against_the_python_loop(fname, monkeypatch):
    """ms_minimize (the trajectories whose theta_B does not move: field_linear next to the pins, scalar next to surface)
    against the Python loop stepping the same context calls: in fixed-order mode the same bits."""
    monkeypatch.setenv("MS_DETERMINISTIC", "1")
    g = load_golden(fname)
    mesh_p, mz_p, _log, _th = _minimizer(g, KIND[fname], observe=True)
    res_p = mz_p.minimize(int(g["n_steps"]))
    assert not mz_p._fast_path_ok(None)  # (the observed stepper)
    mesh_l, mz_l, _log2, _th2 = _minimizer(g, KIND[fname], observe=False)
    res_l = mz_l.minimize(int(g["n_steps"]))
    assert mz_l._fast_path_ok(None) and mz_l.last_run["iterations"] == int(g["n_steps"])
    assert np.array_equal(mesh_p.positions_view(), mesh_l.positions_view())
    assert np.array_equal(mesh_p.tilts_in_view(), mesh_l.tilts_in_view())
    assert np.array_equal(mesh_p.tilts_out_view(), mesh_l.tilts_out_view())
    assert res_p["energy"] == res_l["energy"]
    assert mz_l.last_run["trials"] == sum(c[0] for c in mz_p.step_counts)
    assert mz_l.last_run["guard_rejects"] == sum(c[1] for c in mz_p.step_counts)


def test_geometry_runs_once_per_trial_of_a_shape_search():
    """stats: every evaluation of a shape step orders the ring on the positions it is handed."""
    g = load_golden(TRAJ[2])
    _mesh, mz, _log, _th = _minimizer(g, "gd", observe=False)
    _mir, dm = mz._device()
    from membrane_solver_amd import _lib as L

    before = dm.thetab_contact_stats()
    r = dm.step(stepper=L.MS_STEPPER_GD, step_size=float(g["step_size0"]), tol=0.0)
    after = dm.thetab_contact_stats()
    d_geom = after["geom_launches"] - before["geom_launches"]
    d_apply = after["apply_launches"] - before["apply_launches"]
    n = r.trials + r.guard_rejects  # (a trial the edge guard rejects has had its energy pass as well)
    print("trials", r.trials, "guard rejects", r.guard_rejects, "geom", d_geom, "apply", d_apply)
    assert n >= 2, "the fixture's first search backtracks"
    # one per trial; besides them the energy at x, the re-add behind k_tilt<1> of the gradient pass (it rewrites the
    # cells) and the accepted trial's commit
    assert d_geom == d_apply == n + 3


# ---------------------------------------------------------------------------------------------------------------------
def _relax(g, label, with_module=True):
    from membrane_solver_amd.geometry.mesh import ArrayMesh
    from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager
    from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager
    from membrane_solver_amd.runtime.minimizer import Minimizer
    from membrane_solver_amd.runtime.steppers import GradientDescent

    mods = [str(m) for m in g["modules"] if with_module or str(m) != NAME]
    mesh = ArrayMesh(g["positions"], g["tri"], fixed=g["fixed"], tilts_in=g[label + "__tilts_in0"],
                     tilts_out=g[label + "__tilts_out0"], global_parameters=json.loads(str(g[label + "__gp_json"])),
                     energy_modules=mods, constraint_modules=[], edges=g["edges"], vertex_options=_opts(g["vopts"]))
    mz = Minimizer(mesh, mesh.global_parameters, GradientDescent(), EnergyModuleManager(mods), ConstraintModuleManager([]),
                   quiet=True)
    _mir, dm = mz._device()
    dm.energy()  # (leaves the bending_tilt record the relaxation would otherwise take first, on positions not yet frozen)
    before = dm.thetab_contact_stats()
    iters, evals = dm.relax_leaflet_tilts(**mz._tilt_relax_params())
    after = dm.thetab_contact_stats()
    return mz, dm, iters, evals, {k: after[k] - before[k] for k in after}


@pytest.mark.parametrize("label", ["legacy", "linear"])
def test_relaxation_matches_reference(label):
    """One nested CG relaxation on the one-tile disk with both leaflets' tilt and bending_tilt modules and this one,
    tilt_inner_steps capped where the reference's counts are stable.  The ring is ordered ONCE: positions are frozen."""
    from membrane_solver_amd import _lib as L

    g = load_golden("thetab_contact_relax.npz")
    mz, dm, iters, evals, d = _relax(g, label)
    assert dm.modules & L.MS_MOD_TILT_THETAB_CONTACT_IN
    tin, tout = dm.get_leaflet_tilts("in"), dm.get_leaflet_tilts("out")
    E = float(dm.energy().sum())
    own = dm.thetab_contact_energy()
    bar_t, bar_e = _bar(g, label + "__noise_tilts"), _bar(g, label + "__noise_energy")
    n_grad, n_en = int(g[label + "__n_gradient_evaluations"]), int(g[label + "__n_energy_evaluations"])
    print(label, "iters", iters, "evals", evals, "ref", n_grad, n_en, "E", E, "ref", float(g[label + "__E_total"]), "relerr",
          relerr(tin, g[label + "__tilts_in_final"]), relerr(tout, g[label + "__tilts_out_final"]), "bars", bar_t, bar_e,
          "own", own, float(g[label + "__E_own"]), "launches", d)
    assert iters == n_grad - 1 == int(g[label + "__tilt_inner_steps"])
    assert evals == n_grad + n_en
    assert relerr(tin, g[label + "__tilts_in_final"]) <= bar_t and relerr(tout, g[label + "__tilts_out_final"]) <= bar_t
    assert abs(E - float(g[label + "__E_total"])) <= bar_e * abs(float(g[label + "__E_total"]))
    assert abs(own - float(g[label + "__E_own"])) <= bar_e * abs(float(g[label + "__E_total"]))
    st = dm.exec_stats()
    assert st["relax_fused"] == 0 and st["relax_programs"] == 0
    assert d["geom_launches"] == 1, "the geometry pass runs once per relaxation"
    assert d["apply_launches"] == evals
    bd = mz.compute_energy_breakdown()
    assert abs(bd[NAME] - float(g[label + "__E_own"])) <= bar_e * abs(float(g[label + "__E_total"]))
    assert abs(sum(bd.values()) - float(g[label + "__E_total"])) <= bar_e * abs(float(g[label + "__E_total"]))


def test_context_without_the_module_keeps_its_fast_lanes():
    """The same relaxation without the module: the fused evaluator and the relaxation program run as before."""
    g = load_golden("thetab_contact_relax.npz")
    _mz, dm, _iters, evals, d = _relax(g, "legacy", with_module=False)
    st = dm.exec_stats()
    assert evals > 0 and st["relax_fused"] > 0 and st["relax_programs"] > 0
    assert d["geom_launches"] == 0 and d["apply_launches"] == 0
