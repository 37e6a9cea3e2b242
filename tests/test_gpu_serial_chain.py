"""The deciding workgroup of a fold loads everything its decision can need in one round trip (fold_decide: the direction
scalars of a merged fold and every trial set's energies, then the comparisons in order).  That may not change a
decision or a double: trajectories with long line searches -- pair, triple and four-or-more-trial launches, every one
folded and decided by k_reduce's last workgroup or, on one tile, by reduce_one_tile in k_exec -- against the oracle port.

Meshes: meshgen.icosphere(f) with smooth_displace and the noise of multi_trial_cases.py; nv = 10 f^2 + 2, 256 rows per
tile: f = 8 -> 642 vertices, 3 tiles; f = 15 -> 2 252, 9 tiles; f = 24 -> 5 762, 23 tiles (around the NXCD = 8 edge of
the multi-trial block map); f = 4 -> 162 vertices, one tile (the interpreter k_exec and reduce_one_tile).

The trajectories use the strict Armijo parameters of multi_trial_cases.py (c = 0.9, beta = 0.9) so that the searches are
long; test_searches_are_long_on_the_cpu checks that on the CPU with the oracle alone.  Tolerances are those of
test_gpu_multi_trial.py: equal success flags and trial counts, step sizes to 1e-12, energies to 1e-10 (trajectories);
energy 1e-12, gradient 1e-10 of its largest entry (evaluations)."""
from __future__ import annotations

import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import multi_trial_cases as mt

TILES = {8: 3, 15: 9, 24: 23, 4: 1}
BETA = 0.9
N_STEPS = 12
QUEUE_ENV = ("MS_ESCALATE", "MS_PAIR", "MS_SPECULATE", "MS_PAIR_LEAN", "MS_AHEAD", "MS_DETERMINISTIC", "MS_EXEC")


@functools.lru_cache(maxsize=None)
def _case(freq):
    """The mesh of multi_trial_cases.case for any frequency, with the oracle's energy, gradient and safe step."""
    from membrane_solver_amd import meshgen
    from oracle import minimizer_port as mp

    P, T = meshgen.icosphere(freq)
    P = meshgen.smooth_displace(P, 0.05)
    P = P + 2.0e-3 * np.random.default_rng(3).standard_normal(P.shape)
    P, T = np.ascontiguousarray(P, dtype=np.float64), np.ascontiguousarray(T, dtype=np.int32)
    assert len(P) == 10 * freq * freq + 2
    p = mp.Problem(positions=P, tri=T, energy_modules=["surface", "bending"], gp=dict(mt.GP))
    E0, g = mp.energy_and_gradient(p, P)
    safe = 0.3 * mp.min_edge_length(P, T) / float(np.max(np.linalg.norm(g, axis=1)))
    for a in (P, T, g):
        a.setflags(write=False)
    return SimpleNamespace(freq=freq, P=P, T=T, E0=E0, g=g, safe=safe, alpha0=0.9 * safe)


def _problem(cs, fixed=None):
    from oracle import minimizer_port as mp

    return mp.Problem(positions=cs.P, tri=cs.T, fixed=fixed, energy_modules=["surface", "bending"], gp=dict(mt.GP))


@functools.lru_cache(maxsize=None)
def _oracle_trajectory(freq, n_steps, fixed_row=-1):
    """minimizer_port.minimize with CG and the strict Armijo parameters -> rows (success, next_step, E, trials), x."""
    from oracle import minimizer_port as mp

    cs = _case(freq)
    fixed = None
    if fixed_row >= 0:
        fixed = np.zeros(len(cs.P), dtype=bool)
        fixed[fixed_row] = True
    p = _problem(cs, fixed)
    stepper = mp.ConjugateGradient(max_iter=mt.MAX_ITER, beta=BETA, c=mt.C1, gamma=mt.GAMMA,
                                   alpha_max_factor=mt.ALPHA_MAX_FACTOR)
    ref = mp.minimize(p, stepper, n_steps, step_size=cs.alpha0, tol=1e-9)
    rows = np.array([[float(t["success"]), t["next_step"], t["E_accepted"], t["trials"]] for t in ref["trace"]])
    x = np.array(p.positions)
    rows.setflags(write=False)
    x.setflags(write=False)
    return rows, x


def _tiles(cs):
    """-> (tile count, tile of every caller row) from the host-only tiling pass ms_create runs."""
    from membrane_solver_amd import _lib as L

    st = (ctypes.c_int64 * 8)()
    perm = np.zeros(len(cs.P), dtype=np.int32)
    assert L.lib().ms_plan_tiling(len(cs.P), len(cs.T), cs.P.ctypes.data_as(L._D), cs.T.ctypes.data_as(L._I32), 0, 1, st,
                                  perm.ctypes.data_as(L._I32)) == 0
    tile_of = np.empty(len(cs.P), dtype=np.int64)
    tile_of[perm] = np.arange(len(cs.P)) // 256  # (perm: patch row -> caller row; a tile owns 256 consecutive patch rows)
    return int(st[0]), tile_of


@functools.lru_cache(maxsize=None)
def _halo_row(freq):
    """A vertex that some tile stages as a halo row while its neighbour owns it: an end of the first edge whose ends
    lie in different tiles (every facet at an owned vertex belongs to the tile, its other corners are halo rows)."""
    cs = _case(freq)
    _n, tile_of = _tiles(cs)
    for a, b, c in cs.T:
        for u, v in ((a, b), (b, c), (c, a)):
            if tile_of[u] != tile_of[v]:
                return int(u), int(tile_of[u]), int(tile_of[v])
    raise AssertionError("the mesh has one tile")


# ---- CPU: what the GPU tests rest on ---------------------------------------------------------------------------------
@pytest.mark.parametrize("freq", [8, 15, 24, 4])
def test_tile_counts(freq):
    cs = _case(freq)
    n, tile_of = _tiles(cs)
    assert n == TILES[freq] == -(-len(cs.P) // 256) and tile_of.max() == n - 1


@pytest.mark.parametrize("freq", [8, 15, 24])
def test_searches_are_long_on_the_cpu(freq):
    """Twelve CG steps of the oracle: the run accepts after searches of nine and more trials -- under the default plan
    (MS_ESCALATE=3: launches of 1, 1, 1, 3, 6 trials) a seventh trial lies behind a triple, under MS_ESCALATE=1
    (1, 1, 2, 4, 8) a ninth behind a pair and a four-trial launch -- and every first alpha lies below the safe limit
    (the queued regime)."""
    cs = _case(freq)
    rows, _x = _oracle_trajectory(freq, N_STEPS)
    assert len(rows) == N_STEPS and cs.alpha0 < cs.safe
    print(f"f={freq}: trials per step {rows[:, 3].astype(int).tolist()} accepted {int(rows[:, 0].sum())}")
    assert rows[:, 0].sum() >= 4
    assert rows[rows[:, 0] > 0, 3].max() >= 9


def test_the_fixed_row_is_a_halo_row_owned_by_a_neighbour():
    row, owner, reader = _halo_row(15)
    cs = _case(15)
    _n, tile_of = _tiles(cs)
    assert tile_of[row] == owner != reader
    assert any(tile_of[v] == reader for f in cs.T if row in f for v in f), "no facet of the reading tile holds the row"


# ---- GPU -------------------------------------------------------------------------------------------------------------
def _context(cs, monkeypatch, *, deterministic, env=None, fixed=None):
    from membrane_solver_amd import _lib as L
    from membrane_solver_amd.device import DeviceMesh

    for k in QUEUE_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    P, T = cs.P, cs.T
    dm = DeviceMesh(P, T, fixed=fixed)
    dm.set_deterministic(deterministic)
    dm.set_surface_tension(np.full(len(T), mt.GP["surface_tension"]))
    dm.set_bending_params(np.full(len(P), mt.GP["bending_modulus"]), np.full(len(P), mt.GP["spontaneous_curvature"]))
    dm.set_params(modules=L.MS_MOD_SURFACE | L.MS_MOD_BENDING)
    return dm


def _minimize(dm, cs, n_steps):
    from membrane_solver_amd import _lib as L

    prm = L.ms_minimize_params()
    prm.stepper = L.ms_stepper_params(L.MS_STEPPER_CG, mt.MAX_ITER, BETA, mt.C1, mt.GAMMA, mt.ALPHA_MAX_FACTOR, 10, 0.0, 2)
    prm.step_size, prm.tol = cs.alpha0, 1e-9
    prm.fixed_step_mode, prm.fixed_step = 0, cs.alpha0
    prm.max_zero_steps, prm.step_size_floor = 10, 1e-8
    _out, log = dm.minimize(prm, n_steps, want_log=True)
    return np.array(log)


def _check_trajectory(log, want, label):
    got = log[:, [0, 1, 2, 7]]
    print(f"{label}: trials {got[:, 3].astype(int).tolist()}, max |dE|/|E| "
          f"{np.max(np.abs(got[:, 2] - want[:, 2]) / np.abs(want[:, 2])):.3e}, max |d step|/step "
          f"{np.max(np.abs(got[:, 1] - want[:, 1]) / np.abs(want[:, 1])):.3e}")
    assert got.shape == want.shape
    assert np.array_equal(got[:, 0], want[:, 0]), (got, want)
    assert np.array_equal(got[:, 3], want[:, 3]), (got, want)
    assert np.allclose(got[:, 1], want[:, 1], rtol=1e-12, atol=0)
    assert np.allclose(got[:, 2], want[:, 2], rtol=1e-10, atol=0)


def _check_evaluation(dm, p, x, label, fixed_row=None):
    from oracle import minimizer_port as mp

    e, g = dm.energy_and_gradient()
    E_ref, g_ref = mp.energy_and_gradient(p, x)
    print(f"{label}: |dE|/|E| {abs(e.sum() - E_ref) / abs(E_ref):.3e}, max |dg|/max|g| "
          f"{np.max(np.abs(g - g_ref)) / np.max(np.abs(g_ref)):.3e}")
    assert abs(e.sum() - E_ref) <= 1e-12 * abs(E_ref)
    assert np.max(np.abs(g - g_ref)) <= 1e-10 * np.max(np.abs(g_ref))
    if fixed_row is not None:
        assert (g[fixed_row] == 0.0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("freq", [8, 15, 24])
def test_trajectories_are_unchanged(freq, monkeypatch):
    """Twelve CG steps through ms_minimize with fixed-order sums, under the default launch plan and under
    MS_ESCALATE=1: the step log is the oracle port's by the rule above, no decision was replayed differently, and the
    two plans together launched pairs, triples and four or more trials at once (every one of them folded and decided
    by k_reduce's last workgroup from batched loads)."""
    cs = _case(freq)
    want, _x = _oracle_trajectory(freq, N_STEPS)
    hist = np.zeros(9, dtype=np.int64)
    xs = []
    for esc in (None, "1"):
        dm = _context(cs, monkeypatch, deterministic=True, env={} if esc is None else {"MS_ESCALATE": esc})
        assert dm.tile_stats()["n_tiles"] == TILES[freq]
        log = _minimize(dm, cs, N_STEPS)
        st, h = dm.queue_stats(), dm.search_trials()["first_launch_hist"]
        xs.append(dm.get_positions())
        dm.close()
        print(f"f={freq} MS_ESCALATE={esc}: first launches by size {h} {st}")
        _check_trajectory(log, want, f"f={freq} MS_ESCALATE={esc}")
        assert st["mismatches"] == 0 and st["rounds"] > 0
        hist[1:] += [int(h[s]) for s in range(1, 9)]
    assert np.array_equal(xs[0], xs[1]), "the launch plan changed the trajectory"
    assert hist[2] >= 1 and hist[3] >= 1 and hist[4:].sum() >= 1, hist


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["fixed", "atomic"])
def test_trajectory_with_a_fixed_halo_row(mode, monkeypatch):
    """f = 15 with one fixed vertex that a tile stages as a halo row while its neighbour owns it: energy and gradient
    are the oracle's before and after six steps, and (fixed-order sums) so is the step log; the fixed row has a zero
    gradient and does not move, bit for bit."""
    cs = _case(15)
    row, _owner, _reader = _halo_row(15)
    mask = np.zeros(len(cs.P), dtype=bool)
    mask[row] = True
    dm = _context(cs, monkeypatch, deterministic=(mode == "fixed"), fixed=mask)
    _check_evaluation(dm, _problem(cs, mask), cs.P, f"fixed row {mode}", row)
    log = _minimize(dm, cs, 6)
    x = dm.get_positions()
    assert dm.queue_stats()["mismatches"] == 0
    if mode == "fixed":
        want, _x = _oracle_trajectory(15, 6, row)
        _check_trajectory(log, want, f"fixed row {mode}")
    assert log[:, 0].sum() >= 1 and not np.array_equal(x, cs.P)
    assert np.array_equal(x[row], cs.P[row])
    _check_evaluation(dm, _problem(cs, mask), x, f"fixed row {mode} after the steps", row)
    dm.close()


@pytest.mark.gpu
def test_one_tile_interpreter_trajectory(monkeypatch):
    """f = 4, one tile: the library runs its launches in one workgroup (k_exec); every fold is reduce_one_tile, whose
    thread 0 decides with the batched loads.  Ten CG steps against the oracle port."""
    cs = _case(4)
    want, _x = _oracle_trajectory(4, 10)
    dm = _context(cs, monkeypatch, deterministic=True, env={"MS_EXEC": "1"})
    assert dm.tile_stats()["n_tiles"] == 1
    log = _minimize(dm, cs, 10)
    st, ex = dm.queue_stats(), dm.exec_stats()
    x = dm.get_positions()
    dm.close()
    print(f"f=4: {st} {ex}")
    assert ex["active"] and ex["packs"] > 0
    _check_trajectory(log, want, "f=4 k_exec")
    assert st["mismatches"] == 0
