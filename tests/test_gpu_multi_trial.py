"""Line-search launches of four to eight trials (k_energy<..., MULTI == 8>, the block -> (tile, trial) map of
energy_body, the side sets, the one k_reduce launch that folds them and decides) against the CPU oracle.

The host replays every Armijo decision from the folded doubles the device decided on, so a wrong partial of an early
trial -- the wrong alpha_side[j], the wrong side set, a tile the block map dropped -- replays without a mismatch.
These tests read the trial log (ms_search_trials) and compare every trial's energy with an independent evaluation at
that alpha, put the acceptance at every slot of a launch, and run the launches at tile counts that leave idle blocks
(grid n0 * 8 * ceil(tiles / 8): 2, 7 and 9 tiles) and at one that leaves none (8).

The searches are long because the Armijo constant is strict (multi_trial_cases.py); test_host_logic.py checks on the
CPU that every ladder rejects at least twenty alphas inside the queued regime, accepts monotonically behind the first
accepted alpha and decides nothing within rounding.  The direction of a search is taken from a context of its own in
fixed-order mode (d = -g of ms_energy_and_gradient: after an accepted step the gradient pass queued behind it has
replaced G and D); the oracle evaluates at x + alpha d with that d, so the energy launch alone is under test.  The
default mode's direction differs from it in the last bits of its sums, which moves a trial energy by some 1e-16 |E|."""

import dataclasses
import functools

import numpy as np
import pytest

import multi_trial_cases as mt

pytestmark = pytest.mark.gpu

ESCALATE = ("1", "3", "5", "7")
QUEUE_ENV = ("MS_ESCALATE", "MS_PAIR", "MS_SPECULATE", "MS_PAIR_LEAN", "MS_AHEAD", "MS_DETERMINISTIC")


def _context(cs, monkeypatch, *, fixed, env=None, volume=None):
    from membrane_solver_amd import _lib as L
    from membrane_solver_amd.device import DeviceMesh

    for k in QUEUE_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    nv, nf = len(cs.P), len(cs.T)
    dm = DeviceMesh(cs.P, cs.T, tile_vertices=cs.tile)
    dm.set_deterministic(fixed)
    dm.set_surface_tension(np.full(nf, mt.GP["surface_tension"]))
    dm.set_bending_params(np.full(nv, mt.GP["bending_modulus"]), np.full(nv, mt.GP["spontaneous_curvature"]))
    mods = L.MS_MOD_SURFACE | L.MS_MOD_BENDING
    if volume is None:
        dm.set_params(modules=mods)
    else:
        dm.set_params(modules=mods | L.MS_CON_VOLUME, target_volume=volume)
    assert dm.tile_stats()["n_tiles"] == cs.tiles
    return dm


def _step(dm, cs, step_size, *, stepper=None, max_iter=mt.MAX_ITER):
    from membrane_solver_amd import _lib as L

    return dm.step(stepper=L.MS_STEPPER_GD if stepper is None else stepper, step_size=step_size, tol=1e-9,
                   max_iter=max_iter, beta=cs.beta, c=mt.C1, gamma=mt.GAMMA, alpha_max_factor=mt.ALPHA_MAX_FACTOR,
                   reuse_energy0=2)


@functools.lru_cache(maxsize=None)
def _device_direction(name):
    """d = -g of the device's gradient at the case's positions, fixed-order sums (bitwise repeatable)."""
    from membrane_solver_amd import _lib as L
    from membrane_solver_amd.device import DeviceMesh

    cs = mt.case(name)
    nv, nf = len(cs.P), len(cs.T)
    dm = DeviceMesh(cs.P, cs.T, tile_vertices=cs.tile)
    dm.set_deterministic(True)
    dm.set_surface_tension(np.full(nf, mt.GP["surface_tension"]))
    dm.set_bending_params(np.full(nv, mt.GP["bending_modulus"]), np.full(nv, mt.GP["spontaneous_curvature"]))
    dm.set_params(modules=L.MS_MOD_SURFACE | L.MS_MOD_BENDING)
    e, g = dm.energy_and_gradient()
    dm.close()
    assert abs(e.sum() - cs.E0) <= 1e-12 * abs(cs.E0)
    assert np.max(np.abs(g - cs.g)) <= 1e-10 * np.max(np.abs(cs.g))
    d = -g
    d.setflags(write=False)
    return d


def _oracle_search(cs, d, step_size, max_iter=mt.MAX_ITER):
    from oracle import minimizer_port as mp

    return mp.line_search(mt.problem(cs), d, -d, step_size, max_iter=max_iter, beta=cs.beta, c=mt.C1, gamma=mt.GAMMA,
                          alpha_max_factor=mt.ALPHA_MAX_FACTOR)


def _check_search(cs, d, dm, r, step_size, max_iter=mt.MAX_ITER, label=""):
    """One step's trial log against the oracle: alphas, every trial's energy, the right-hand sides, the outcome.
    -> (the log, largest |E_hip - E_oracle| / |E_oracle| over its trials, the oracle's energies)."""
    log, st = dm.search_trials(), dm.queue_stats()
    n = len(log["alpha"])
    search = ~log["behind"]
    assert n >= 1 and not log["guard"].any(), "every alpha of these ladders lies below the guard range"
    # the trials behind an accepted slot continue the ladder: all n alphas are step_size * beta^j
    assert np.array_equal(log["alpha"], mt.alphas_from(step_size, n, cs.beta))
    assert search[: int(search.sum())].all(), "a trial behind the accepted slot was logged in front of the search"
    E_ref = mt.ladder(cs, d, log["alpha"])
    err = np.abs(log["energy"] - E_ref) / np.abs(E_ref)
    print(f"{label} trials {int(search.sum())} (+{int(log['behind'].sum())} behind) launches "
          f"{[int(v) for v in log['launch'][log['slot'] == 0]]} max |E_hip - E_oracle|/|E| {err.max():.3e}")
    assert (err <= 1e-12).all(), (label, err)
    # the right-hand sides, from the device's own scalars in the order ms_step forms them
    assert np.array_equal(log["rhs"], r.energy_eval + mt.C1 * log["alpha"] * r.g_dot_d)
    # launches: slots count up inside a launch, and nothing follows an accepted slot but the rest of its launch
    pos = 0
    while pos < n:
        size = int(log["launch"][pos])
        m = min(size, n - pos)
        assert 1 <= size <= 8 and np.array_equal(log["slot"][pos:pos + m], np.arange(m))
        assert (log["launch"][pos:pos + m] == size).all()
        assert m == size or pos + m == n
        pos += m
    ls = _oracle_search(cs, d, step_size, max_iter)
    assert r.success == ls.success and r.trials == ls.trials == int(search.sum()) and r.guard_rejects == 0
    assert r.next_step == ls.next_step
    if ls.success:
        k = ls.trials - 1
        assert r.alpha == ls.alpha == log["alpha"][k]
        assert log["energy"][k] <= log["rhs"][k] and (log["energy"][:k] > log["rhs"][:k]).all()
        assert r.energy == log["energy"][k] and abs(r.energy - ls.energy) <= 1e-12 * abs(ls.energy)
        assert int(log["behind"].sum()) == int(log["launch"][k]) - 1 - int(log["slot"][k])
    else:
        assert r.alpha == 0.0 and not log["behind"].any() and (log["energy"] > log["rhs"]).all()
    assert st["mismatches"] == 0
    return log, float(err.max()), E_ref


def _truth_energies(cs, d, alphas):
    from oracle import truth

    nv, nf = len(cs.P), len(cs.T)
    out = []
    for a in alphas:
        E, _ = truth.surface_bending_energy_and_gradient(
            cs.P + a * d, cs.T, np.full(nf, mt.GP["surface_tension"]), np.full(nv, mt.GP["bending_modulus"]),
            np.full(nv, mt.GP["spontaneous_curvature"]), np.zeros(nv, dtype=bool))
        out.append(E)
    return np.array(out, dtype=np.longdouble)


@pytest.mark.parametrize("mode", ["fixed", "atomic"])
@pytest.mark.parametrize("name", list(mt.MESHES))
def test_every_trial_energy_matches_the_oracle(name, mode, monkeypatch):
    """One gradient-descent step from 0.9 x the safe limit on a fresh context, for MS_ESCALATE in {1, 3, 5, 7}: every
    logged trial energy within 1e-12 |E| of minimizer_port.energy_total at x + alpha_j d_device, the alphas
    alpha0 beta^j exactly, the right-hand sides from the device's own scalars, and trial count, accepted alpha,
    next_step and accepted energy those of minimizer_port.line_search.  Over the four settings the first launches of
    the rounds cover every size 2 ... 8 (with today's plan_round 1,1,2,4,8,8 / 1,1,1,3,6,8 / 1x5,5,8 / 1x7,7,8: a
    prediction, only the coverage is asserted).  On ico6 the HIP error of each trial energy against the long-double
    evaluation is at most twice the fp64 oracle's own, plus 1e-13 |E| (the margin of
    test_full_size_energy_and_gradient_match_oracle for a differently ordered sum)."""
    from oracle import truth

    cs = mt.case(name)
    lad = mt.check_preconditions(name)
    d = _device_direction(name)
    hist = np.zeros(9, dtype=np.int64)
    for esc in ESCALATE:
        dm = _context(cs, monkeypatch, fixed=(mode == "fixed"), env={"MS_ESCALATE": esc})
        r = _step(dm, cs, cs.alpha0)
        log, err, E_ref = _check_search(cs, d, dm, r, cs.alpha0, label=f"{name} {mode} MS_ESCALATE={esc}:")
        h = dm.search_trials()["first_launch_hist"]
        dm.close()
        assert r.success and r.trials == lad.R + 1, "the device direction gives the ladder of the oracle's own"
        for size in range(2, 9):  # (a launch of one trial in the log is a round's first launch or a gated stage)
            assert h[size] == int(np.sum((log["launch"] == size) & (log["slot"] == 0))), (h, log["launch"])
        assert h[1] <= int(np.sum(log["launch"] == 1))
        hist[1:] += [h[s] for s in range(1, 9)]
        if name == "ico6" and truth.available():
            E_ld = _truth_energies(cs, d, log["alpha"])
            e_hip = np.abs(log["energy"].astype(np.longdouble) - E_ld).astype(np.float64)
            e_orc = np.abs(E_ref.astype(np.longdouble) - E_ld).astype(np.float64)
            print(f"{name} {mode} MS_ESCALATE={esc}: against the long-double evaluation, relative to |E|: HIP max "
                  f"{np.max(e_hip / np.abs(E_ref)):.3e}, fp64 oracle max {np.max(e_orc / np.abs(E_ref)):.3e}")
            assert (e_hip <= 2.0 * e_orc + 1e-13 * np.abs(E_ref)).all(), (e_hip, e_orc)
    print(f"{name} {mode}: first launches by size {dict(enumerate(hist.tolist()))}")
    assert (hist[2:] >= 1).all(), f"first-launch sizes 2 ... 8 are not all covered: {hist[1:]}"


@pytest.mark.parametrize("name", ["ico6", "ico15"])
def test_acceptance_at_every_slot(name, monkeypatch):
    """MS_ESCALATE=1, fixed-order sums, CG: the search starts k alphas above the accepted one for k = 0 ... 15, so the
    acceptance lands in a single-trial launch (k = 0, 1), at both slots of a pair (2, 3), at every slot of a 4-launch
    (4 ... 7) and of an 8-launch (8 ... 15) -- which slots were the accepted one is asserted from the log, the launch
    sizes are plan_round's.  An early slot is DEC_ACCEPT_SIDE: the accepted trial is evaluated again alone and the
    gated gradient pass stays out.  What that leaves behind is pinned three ways: the positions are x + alpha d to one
    ulp, energy and gradient at the new point match the oracle (1e-12, 1e-10), and a second step gives the doubles of
    the same two steps with one trial per launch (MS_PAIR=0 MS_SPECULATE=0), every StepResult field and position."""
    from membrane_solver_amd import _lib as L
    from oracle import minimizer_port as mp

    cs = mt.case(name)
    lad = mt.check_preconditions(name)
    d = _device_direction(name)
    a_acc = lad.alphas[lad.R]
    starts, expect = [], []
    for k in range(16):
        a0 = a_acc / cs.beta ** k
        assert a0 < cs.safe, "the start of the ladder must stay in the queued regime"
        ls = _oracle_search(cs, d, a0)
        assert ls.success and ls.trials == k + 1
        starts.append(a0)
        expect.append(ls)
    seen = set()
    for k, (a0, ls) in enumerate(zip(starts, expect)):
        def two_steps(env, between=None):
            dm = _context(cs, monkeypatch, fixed=True, env=env)
            r1 = _step(dm, cs, a0, stepper=L.MS_STEPPER_CG)
            info = between(dm, r1) if between else None
            x1 = dm.get_positions()
            r2 = _step(dm, cs, r1.next_step, stepper=L.MS_STEPPER_CG)
            x2 = dm.get_positions()
            dm.close()
            return dataclasses.astuple(r1), x1, dataclasses.astuple(r2), x2, info

        def after_first(dm, r1):
            log, _err, _E = _check_search(cs, d, dm, r1, a0, label=f"{name} k={k}:")
            return log, dm.queue_stats()

        plain = two_steps({"MS_PAIR": "0", "MS_SPECULATE": "0"})
        queue = two_steps({"MS_ESCALATE": "1"}, after_first)
        log, st = queue[4]
        r1 = queue[0]
        assert r1[2] == k + 1 and r1[6] == ls.alpha, (k, r1)  # (trials, alpha)
        n0, slot = int(log["launch"][k]), int(log["slot"][k])
        seen.add((n0, slot))
        if slot < n0 - 1:
            assert st["side_accepts"] == 1 and st["wasted_evaluations"] == n0 - 1 - slot, (k, st)
        else:
            assert st["side_accepts"] == 0 and st["wasted_evaluations"] == 0, (k, st)
        x_want = cs.P + ls.alpha * d
        assert (np.abs(queue[1] - x_want) <= np.spacing(np.abs(x_want))).all(), k
        assert plain[0] == queue[0] and np.array_equal(plain[1], queue[1]), (k, plain[0], queue[0])
        assert plain[2] == queue[2] and np.array_equal(plain[3], queue[3]), (k, plain[2], queue[2])
        # energy and gradient at the accepted point, on a context that has just taken the step
        dm = _context(cs, monkeypatch, fixed=True, env={"MS_ESCALATE": "1"})
        r1b = _step(dm, cs, a0, stepper=L.MS_STEPPER_CG)
        e, g = dm.energy_and_gradient()
        x1b = dm.get_positions()
        dm.close()
        assert dataclasses.astuple(r1b) == r1 and np.array_equal(x1b, queue[1])
        E_ref, g_ref = mp.energy_and_gradient(cs.p, x1b)
        assert abs(e.sum() - E_ref) <= 1e-12 * abs(E_ref), (k, e.sum(), E_ref)
        assert np.max(np.abs(g - g_ref)) <= 1e-10 * np.max(np.abs(g_ref)), k
    print(f"{name}: accepted (launch size, slot) pairs {sorted(seen)}")
    want = {(n0, s) for n0 in (2, 4, 8) for s in range(n0)}
    assert want <= seen, f"never the accepted slot: {sorted(want - seen)}"


@pytest.mark.parametrize("mode", ["fixed", "atomic"])
@pytest.mark.parametrize("name", ["ico6", "ico14", "ico15"])
def test_search_that_opens_with_a_multi_trial_launch(name, mode, monkeypatch):
    """The cold branch of plan_round: the previous search along -g ran out of its max_iter = 10 trials, so the next
    one (same max_iter, no history of accepted alphas) opens with as many trials as there are sets.  Its first launch
    has more than three trials by the histogram, and its log matches the oracle as above with the acceptance at the
    launch's first slot, in its middle, at its last slot, and behind it (start k alphas above the accepted one)."""
    cs = mt.case(name)
    lad = mt.check_preconditions(name)
    d = _device_direction(name)
    a_acc = lad.alphas[lad.R]
    for k in (0, 3, 7, 9):
        dm = _context(cs, monkeypatch, fixed=(mode == "fixed"))
        r0 = _step(dm, cs, cs.alpha0, max_iter=10)
        _check_search(cs, d, dm, r0, cs.alpha0, max_iter=10, label=f"{name} {mode} exhausted:")
        assert not r0.success and r0.trials == 10
        h0 = dm.search_trials()["first_launch_hist"]
        assert np.array_equal(dm.get_positions(), cs.P)
        a0 = a_acc / cs.beta ** k
        r = _step(dm, cs, a0, max_iter=10)
        log, _err, _E = _check_search(cs, d, dm, r, a0, max_iter=10, label=f"{name} {mode} k={k}:")
        h1 = dm.search_trials()["first_launch_hist"]
        dm.close()
        assert r.success and r.trials == k + 1
        first = int(log["launch"][0])
        assert first > 3 and h1[first] == h0[first] + 1, (first, h0, h1)


@pytest.mark.parametrize("volume_row", [False, True])
@pytest.mark.parametrize("kind", ["gd", "cg"])
@pytest.mark.parametrize("name", ["ico13", "ico14", "ico15", "ico24"])
def test_multi_trial_launches_do_not_change_the_trajectory(name, kind, volume_row, monkeypatch):
    """Twelve ms_minimize steps with the strict Armijo parameters and fixed-order sums, without and with the volume
    row (target: the mesh's own volume): for MS_ESCALATE in {0, 1, 3, 5, 7} the step log and the final positions are
    those of the one-trial-per-launch run (MS_PAIR=0 MS_SPECULATE=0) bit for bit, no decision was replayed
    differently, and every setting but MS_ESCALATE=0 launched four or more trials at once.  The plain run itself
    follows minimizer_port.minimize by the rule of test_minimizer_reproduces_reference_trajectory: equal success
    flags and trial counts, step sizes to 1e-12, energies to 1e-10."""
    from membrane_solver_amd import _lib as L
    from oracle import minimizer_port as mp
    from oracle import ms_oracle as orc

    cs = mt.case(name)
    mt.check_preconditions(name)
    n_steps = 12
    V0 = float(orc.volume(cs.P, cs.T, None))
    runs = {}
    for esc in (None, "0", "1", "3", "5", "7"):
        env = {"MS_PAIR": "0", "MS_SPECULATE": "0"} if esc is None else {"MS_ESCALATE": esc}
        dm = _context(cs, monkeypatch, fixed=True, env=env, volume=V0 if volume_row else None)
        prm = L.ms_minimize_params()
        prm.stepper = L.ms_stepper_params(L.MS_STEPPER_CG if kind == "cg" else L.MS_STEPPER_GD, mt.MAX_ITER, cs.beta,
                                          mt.C1, mt.GAMMA, mt.ALPHA_MAX_FACTOR, 10, 0.0, 2)
        prm.step_size, prm.tol = cs.alpha0, 1e-9
        prm.fixed_step_mode, prm.fixed_step = 0, cs.alpha0
        prm.max_zero_steps, prm.step_size_floor = 10, 1e-8
        _out, log = dm.minimize(prm, n_steps, want_log=True)
        runs[esc] = (np.array(log), dm.get_positions(), dm.queue_stats(), dm.search_trials()["first_launch_hist"])
        dm.close()
    plain, x_plain, st_plain, _h = runs[None]
    assert len(plain) == n_steps and st_plain["rounds"] == 0 and st_plain["mismatches"] == 0
    assert plain[:, 0].sum() >= 4 and plain[:, 7].max() >= mt.MIN_REJECTED, "the run is meant to accept after long searches"
    for esc in ("0", "1", "3", "5", "7"):
        log, x, st, h = runs[esc]
        print(f"{name} {kind} volume_row={volume_row} MS_ESCALATE={esc}: first launches by size {h} {st}")
        assert np.array_equal(log, plain), f"MS_ESCALATE={esc} changed the trajectory"
        assert np.array_equal(x, x_plain)
        assert st["mismatches"] == 0 and st["rounds"] > 0
        if esc != "0":
            assert sum(h[s] for s in range(4, 9)) >= 1, (esc, h)
    # the plain run against the oracle's minimizer
    gp = dict(mt.GP)
    if volume_row:  # (the row alone: no projection of the trials, and no drift check -- the device run has none either)
        gp.update(volume_constraint_mode="lagrange", volume_projection_during_minimization=False, volume_tolerance=1e30)
    p = mp.Problem(positions=cs.P, tri=cs.T, energy_modules=["surface", "bending"],
                   constraint_modules=["volume"] if volume_row else [], gp=gp, target_volume=V0 if volume_row else None)
    stepper = (mp.ConjugateGradient if kind == "cg" else mp.GradientDescent)(
        max_iter=mt.MAX_ITER, beta=cs.beta, c=mt.C1, gamma=mt.GAMMA, alpha_max_factor=mt.ALPHA_MAX_FACTOR)
    ref = mp.minimize(p, stepper, n_steps, step_size=cs.alpha0, tol=1e-9)
    want = np.array([[float(t["success"]), t["next_step"], t["E_accepted"], t["trials"]] for t in ref["trace"]])
    got = plain[:, [0, 1, 2, 7]]
    assert got.shape == want.shape
    assert np.array_equal(got[:, 0], want[:, 0]), (got, want)
    assert np.array_equal(got[:, 3], want[:, 3]), (got, want)
    assert np.allclose(got[:, 1], want[:, 1], rtol=1e-12, atol=0)
    assert np.allclose(got[:, 2], want[:, 2], rtol=1e-10, atol=0)
