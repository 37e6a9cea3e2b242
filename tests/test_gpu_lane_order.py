"""The lean k_energy instances' own lane order (Tiling::tile_facets_lean, csrc/ms_tiles.cpp step 4) on the device.

The lean k_energy instances read each tile's facet records in an order of their own (the records themselves are the
common ones); MS_LANE_ORDER=0 at ms_create makes them read the common array, as every other kernel does.  The facet
arithmetic is the same in either order; what differs is which lane sums which facets' scalars and the order in which
the LDS atomics arrive, so the two orders are held to the bars each of them meets against the oracle (1e-12 relative
on energies, 1e-10 of max |row| on rows: test_gpu_kernels.py), and test_gpu_energy_lean.py goes on holding the default
context to the general instance's own run-to-run scatter.  Every other instance (general, fixed-order) reads what it
read before and must not change by a bit; the gradient pass sees the lean order only through the factor rows fK / fA
it is handed.

Meshes, contexts and oracle values are those of test_gpu_energy_lean.py: icosphere f = 6, 8, 13 (2, 3, 7 tiles) and the
pulled sliver mesh, default tile, surface + Helfrich bending, uniform parameters."""

import functools

import numpy as np
import pytest

import multi_trial_cases as mt
import test_gpu_energy_lean as tl
from conftest import relerr

pytestmark = pytest.mark.gpu

E_TOL, F_TOL = tl.E_TOL, tl.F_TOL
OFF = {"MS_LANE_ORDER": "0"}
ALPHA = 2.0e-3


def _context(P, T, monkeypatch, env=None, **kw):
    monkeypatch.delenv("MS_LANE_ORDER", raising=False)
    return tl._context(P, T, monkeypatch, env, **kw)


def _mt_context(cs, monkeypatch, env, fixed=False):
    monkeypatch.delenv("MS_LANE_ORDER", raising=False)
    return tl._mt_context(cs, monkeypatch, env, fixed=fixed)


def _oracle_at(P, T, fixed=None):
    """oracle.ms_oracle at P: (E_surface, E_bending, fK, fA, gradient with the fixed rows zeroed)"""
    from oracle import ms_oracle as orc

    nv, nf = len(P), len(T)
    g = np.zeros_like(P)
    Es = orc.surface_energy_and_gradient(P, T, np.full(nf, tl.GP["surface_tension"]), g)
    Eb, fK, fAe, fAv = orc.bending_energy_and_gradient(
        P, T, np.full(nv, tl.GP["bending_modulus"]), np.full(nv, tl.GP["spontaneous_curvature"]), np.zeros(nv, bool),
        grad=g, want_factors=True)
    if fixed is not None:
        g[fixed.astype(bool)] = 0.0
    return float(Es), float(Eb), fK, np.stack([fAe, fAv], axis=1), g


@functools.lru_cache(maxsize=None)
def _oracle_x(name):
    P, T = tl._mesh(name)
    fixed = np.zeros(len(P), dtype=np.uint8)
    fixed[::5] = 1
    out = _oracle_at(P, T, fixed)
    for a in out[2:]:
        a.setflags(write=False)
    return out


def _fixed(P):
    fixed = np.zeros(len(P), dtype=np.uint8)
    fixed[::5] = 1
    return fixed


def _check_against_oracle(tag, got, grad, ref, P, T):
    Es, Eb, fK, fA, g = ref
    errs = {"e_surf": abs(got["e_surf"] - Es) / abs(Es), "e_bend": abs(got["e_bend"] - Eb) / abs(Eb),
            "fK": relerr(got["fK"], fK), "fA": relerr(got["fA"], fA), "grad": relerr(grad, g)}
    print(tag, " ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    assert errs["e_surf"] <= E_TOL and errs["e_bend"] <= E_TOL, (tag, errs)
    assert errs["fK"] <= F_TOL and errs["fA"] <= F_TOL and errs["grad"] <= F_TOL, (tag, errs)
    e = np.concatenate([P[T[:, 1]] - P[T[:, 0]], P[T[:, 2]] - P[T[:, 1]], P[T[:, 0]] - P[T[:, 2]]])
    L2 = float(np.einsum("ij,ij->i", e, e).min())
    assert abs(got["min_e2"] - L2) <= 4.0 * np.spacing(L2), (tag, got["min_e2"], L2)


# -- selection -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("freq", sorted(tl.TILES))
def test_selection(freq, monkeypatch):
    """Default: tile_stats() reports the lean order and the energy launches are lean ones; MS_LANE_ORDER=0: off, still
    lean launches; fixed-order mode launches the general instance whatever the flag says."""
    from membrane_solver_amd import _lib as L

    P, T = tl._ico(freq)
    for env, want in ((None, True), (OFF, False)):
        dm = _context(P, T, monkeypatch, env)
        ts = dm.tile_stats()
        assert ts["n_tiles"] == tl.TILES[freq] and ts["lane_order"] is want and ts["lane_halo"] is False, ts
        dm.energy()
        dm.energy_and_gradient()
        dm.step(stepper=L.MS_STEPPER_CG, step_size=1e-3, reuse_energy0=2)
        st = dm.energy_stats()
        assert st["lean"] >= 3 and st["general"] == 0, st
        tl._fixed_order_direction(dm)  # (asserts one general launch, no lean one)
        assert dm.tile_stats()["lane_order"] is want
        dm.close()


# -- against the oracle, and against the common order ---------------------------------------------------------------

@pytest.mark.parametrize("name", [6, 8, 13, "pulled"])
def test_lean_order_matches_the_oracle_and_the_common_order(name, monkeypatch):
    """Every 5th row fixed.  At x and at x + alpha d (d = -g of fixed-order sums, the same doubles in both contexts):
    energies within 1e-12 relative, fK / fA rows and the gradient within 1e-10 of max |row| of oracle.ms_oracle, min_e2
    within 4 ulp of the NumPy minimum; xt bitwise the MS_LANE_ORDER=0 context's; and the two orders against each other
    by the same bars (differences printed)."""
    P, T = tl._mesh(name)
    fixed = _fixed(P)
    res = {}
    for which, env in (("lean", None), ("common", OFF)):
        dm = _context(P, T, monkeypatch, env, fixed=fixed)
        assert dm.tile_stats()["lane_order"] is (which == "lean")
        d = tl._fixed_order_direction(dm)
        at_x, n0 = tl._evaluate(dm)
        at_t, n1 = tl._evaluate(dm, ALPHA)
        assert n0 == n1 == {"lean": 1, "general": 0}
        _e, g_x = dm.energy_and_gradient()  # (after the trial: a gradient call leaves its own direction in D)
        dm.close()
        # the gradient at the trial positions: a context of its own created there
        xt = np.ascontiguousarray(at_t["xt"])
        dm = _context(xt, T, monkeypatch, env, fixed=fixed)
        _e, g_t = dm.energy_and_gradient()
        assert dm.energy_stats()["general"] == 0
        dm.close()
        res[which] = (d, at_x, g_x, at_t, g_t)
    d, at_x, g_x, at_t, g_t = res["lean"]
    dc, cx, gcx, ct, gct = res["common"]
    assert np.array_equal(d, dc) and np.abs(d).max() > 0.0
    assert np.array_equal(at_t["xt"], ct["xt"])
    assert np.array_equal(at_t["xt"][::5], P[::5]) and not np.array_equal(at_t["xt"], P)
    _check_against_oracle(f"{name} at x:", at_x, g_x, _oracle_x(name), P, T)
    xt = np.ascontiguousarray(at_t["xt"])
    _check_against_oracle(f"{name} at x + alpha d:", at_t, g_t, _oracle_at(xt, T, fixed), xt, T)
    for tag, a, ga, b, gb in (("x", at_x, g_x, cx, gcx), ("x + alpha d", at_t, g_t, ct, gct)):
        de = {k: abs(a[k] - b[k]) / abs(b[k]) for k in ("e_surf", "e_bend")}
        dr = {"fK": relerr(a["fK"], b["fK"]), "fA": relerr(a["fA"], b["fA"]), "grad": relerr(ga, gb)}
        print(f"{name} at {tag}: lean order - common order:", " ".join(f"{k} {v:.3e}" for k, v in {**de, **dr}.items()))
        assert a["min_e2"] == b["min_e2"]
        assert all(v <= E_TOL for v in de.values()), de
        assert all(v <= F_TOL for v in dr.values()), dr


# -- multi-trial launches ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("freq", [8, 13])
def test_multi_trial_energies_match_the_oracle(freq, monkeypatch):
    """One gradient-descent step with multi_trial_cases.py's strict Armijo parameters, MS_ESCALATE in {1, 3, 5}: every
    logged trial energy within 1e-12 of mt.ladder; alphas, launch sizes, slots and the step result equal the
    MS_LANE_ORDER=0 run's; no queue mismatch."""
    from membrane_solver_amd import _lib as L

    cs = tl._mt_case(freq)
    dm = _mt_context(cs, monkeypatch, {}, fixed=True)
    _e, g = dm.energy_and_gradient()
    dm.close()
    d = -g
    for esc in ("1", "3", "5"):
        logs = {}
        for which, extra in (("lean", {}), ("common", OFF)):
            dm = _mt_context(cs, monkeypatch, dict({"MS_ESCALATE": esc}, **extra))
            assert dm.tile_stats()["lane_order"] is (which == "lean")
            r = dm.step(stepper=L.MS_STEPPER_GD, step_size=cs.alpha0, tol=1e-9, max_iter=mt.MAX_ITER, beta=cs.beta,
                        c=mt.C1, gamma=mt.GAMMA, alpha_max_factor=mt.ALPHA_MAX_FACTOR, reuse_energy0=2)
            logs[which] = (r, dm.search_trials(), dm.energy_stats(), dm.queue_stats())
            dm.close()
        r, log, st, qs = logs["lean"]
        rc, log_c, st_c, qs_c = logs["common"]
        assert st["general"] == 0 and st["lean"] > 0 and st_c["general"] == 0 and st_c["lean"] > 0, (st, st_c)
        assert qs["mismatches"] == 0 and qs_c["mismatches"] == 0 and r.success and not log["guard"].any()
        E_ref = mt.ladder(cs, d, log["alpha"])
        err = np.abs(log["energy"] - E_ref) / np.abs(E_ref)
        print(f"f={freq} MS_ESCALATE={esc}: {len(err)} trials, max |E - E_oracle|/|E| {err.max():.3e}")
        assert (err <= 1e-12).all(), err
        for k in ("alpha", "launch", "slot", "behind", "guard"):
            assert np.array_equal(log[k], log_c[k]), k
        assert np.max(np.abs(log["energy"] - log_c["energy"]) / np.abs(log_c["energy"])) <= 1e-12
        assert (r.success, r.trials, r.alpha, r.next_step) == (rc.success, rc.trials, rc.alpha, rc.next_step)


def _minimize(dm, steps):
    from membrane_solver_amd import _lib as L

    prm = L.ms_minimize_params()
    prm.stepper = L.ms_stepper_params(L.MS_STEPPER_CG, 10, 0.7, 1e-4, 1.5, 10.0, 10, 0.0, 2)
    prm.step_size, prm.tol = 1e-3, 1e-9
    prm.fixed_step_mode, prm.fixed_step = 0, 1e-3
    prm.max_zero_steps, prm.step_size_floor = 10, 1e-8
    _out, log = dm.minimize(prm, steps, want_log=True)
    return np.array(log)


def test_cg_trajectory_equals_the_common_order_run(monkeypatch):
    """Twelve CG steps of ms_minimize at f = 8: success flags, trial counts and step sizes equal the MS_LANE_ORDER=0
    run's, accepted energies within rtol 1e-10."""
    P, T = tl._ico(8)
    runs = {}
    for which, env in (("common", OFF), ("lean", None)):
        dm = _context(P, T, monkeypatch, env)
        runs[which] = (_minimize(dm, 12), dm.energy_stats())
        dm.close()
    want, st_c = runs["common"]
    got, st = runs["lean"]
    assert len(want) == 12 and want[:, 0].sum() >= 6
    assert st["general"] == 0 and st["lean"] > 0 and st_c["general"] == 0
    assert np.array_equal(got[:, 0], want[:, 0])   # success flags
    assert np.array_equal(got[:, 7], want[:, 7])   # trial counts
    assert np.array_equal(got[:, 1], want[:, 1])   # step sizes
    assert np.allclose(got[:, 2], want[:, 2], rtol=1e-10, atol=0)


# -- lanes that must not change by a bit ---------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["fixed_order", "general"])
def test_other_instances_are_untouched(mode, monkeypatch):
    """Fixed-order mode: energy, gradient and three CG steps are bitwise equal between a default context and an
    MS_LANE_ORDER=0 one.  The general instance (MS_KA_LEAN=0), one evaluation: its factor rows, trial positions and
    scalars likewise -- compared in fixed-order mode too for the sums, as LDS-atomic sums do not repeat run to run;
    min_e2 and xt of the LDS-atomic general launch are bitwise equal."""
    from membrane_solver_amd import _lib as L

    P, T = tl._ico(8)
    out = {}
    for which, env in (("default", {}), ("off", OFF)):
        if mode == "general":
            env = dict(env, MS_KA_LEAN="0")
        dm = _context(P, T, monkeypatch, env)
        assert dm.tile_stats()["lane_order"] is (which == "default")
        if mode == "fixed_order":
            dm.set_deterministic(True)
            e, g = dm.energy_and_gradient()
            steps = []
            for _ in range(3):
                s = dm.step(stepper=L.MS_STEPPER_CG, step_size=1e-3, reuse_energy0=2)
                steps.append((s.success, s.trials, s.alpha, s.energy, s.next_step))
            out[which] = [np.asarray(e), g, np.array(steps, dtype=float),
                          dm.get_vertex_buffer(L.MS_BUF_X)]
            assert dm.energy_stats()["lean"] == 0
        else:
            d = tl._fixed_order_direction(dm)
            got, n = tl._evaluate(dm, ALPHA)  # (LDS-atomic general launch)
            assert n == {"lean": 0, "general": 1}
            dm.set_deterministic(True)
            det, n = tl._evaluate(dm, ALPHA)
            assert n == {"lean": 0, "general": 1}
            out[which] = [d, got["xt"], np.float64(got["min_e2"]), det["fK"], det["fA"],
                          np.array([det["e_surf"], det["e_bend"], det["min_e2"]])]
        dm.close()
    for a, b in zip(out["default"], out["off"]):
        assert np.array_equal(a, b)
