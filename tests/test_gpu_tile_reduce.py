"""The per-tile scalars of the default-mode (LDS-atomic) headline instances are folded one value per wave out of LDS
columns (block_reduce_store_staged, csrc/ms_kernels.hip); every other instance -- the fixed-order mode among them -- keeps
block_reduce_store.  The two modes compute the same per-thread values on the same context, so their scalars are the
checks of one another: a minimum does not depend on the order and must be EQUAL (a staging or identity mistake shows
there first), the sums agree to the rounding of a differently ordered sum, and a maximum is never below any row's value.

Meshes: displaced icospheres (as bench.py displaces its own), surface + Helfrich bending.
  ico5          252 vertices: one tile with four idle lanes, run by the one-workgroup interpreter
  ico6          362 vertices: tiles of 256 and 106 owned rows
  ico12         1442 vertices: six tiles, the last with 162 rows
  ico12_fixed   the same with every 7th row fixed
  ico12_tile64  the same at tile_vertices=64: runtime-size instances, which keep block_reduce_store in both modes

Tolerances.  Sums of n <= 2 900 positive terms of either order differ by at most ~n eps/2 relative in the worst case and
~sqrt(n) eps typically: 1e-13 for the energies (the project's energy bar is 1e-12).  The gradient rows themselves are
sums of LDS atomics whose order changes their last bits, and |g|^2, <g,d> and the row maxima inherit that twice over:
1e-11."""

import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ALPHA = 1e-3
E_RTOL = 1e-13
G_RTOL = 1e-11
# name -> (icosphere frequency, tile_vertices (0: the library's 256), every k-th row fixed (0: none))
MESHES = {
    "ico5": (5, 0, 0),
    "ico6": (6, 0, 0),
    "ico12": (12, 0, 0),
    "ico12_fixed": (12, 0, 7),
    "ico12_tile64": (12, 64, 0),
}


@functools.lru_cache(maxsize=None)
def _mesh_arrays(freq, fixed_every):
    """(positions, rows, fixed mask): built once per mesh, shared by the tests, never written to"""
    from membrane_solver_amd import meshgen

    P, T = meshgen.icosphere(freq)
    P = meshgen.smooth_displace(P, 0.05)
    fixed = np.zeros(len(P), dtype=np.uint8)
    if fixed_every:
        fixed[::fixed_every] = 1
    for a in (P, T, fixed):
        a.setflags(write=False)
    return P, T, fixed


def _device(name):
    from membrane_solver_amd import _lib as L
    from membrane_solver_amd.device import DeviceMesh

    freq, tile, fixed_every = MESHES[name]
    P, T, fixed = _mesh_arrays(freq, fixed_every)
    dm = DeviceMesh(P, T, fixed=fixed, tile_vertices=tile)
    dm.set_surface_tension(np.ones(len(T)))
    dm.set_bending_params(np.ones(len(P)), np.zeros(len(P)))
    dm.set_params(modules=L.MS_MOD_SURFACE | L.MS_MOD_BENDING)
    return dm


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


def _check_tiles(name, dm):
    nv = len(_mesh_arrays(MESHES[name][0], MESHES[name][2])[0])
    n_tiles = dm.tile_stats()["n_tiles"]
    assert nv == {5: 252, 6: 362, 12: 1442}[MESHES[name][0]]
    assert n_tiles == -(-nv // (MESHES[name][1] or 256)), (name, n_tiles)
    if name == "ico5":
        st = dm.exec_stats()
        assert st["active"] and st["packs"] > 0, st  # (one tile: the launches went through k_exec)


def _energy_scalars(dm, deterministic, **kw):
    dm.set_deterministic(deterministic)
    dm.phase_energy(**kw)
    return dm.fetch_scalars()


@pytest.mark.parametrize("name", sorted(MESHES))
def test_energy_scalars_of_both_modes_agree(name):
    """ms_phase_energy at x and at x + alpha d (one trial): MS_S_MINEDGE2 equal, MS_S_ESURF / MS_S_EBEND to 1e-13; the
    fixed-order scalars repeat bit for bit."""
    from membrane_solver_amd import _lib as L

    dm = _device(name)
    at_x = dict(write_bending_factors=True)
    trial = dict(use_direction=True, alpha=ALPHA, write_trial=True, write_bending_factors=True)
    fx = _energy_scalars(dm, True, **at_x)
    # a direction for the trial passes: d = -g at x, computed once (fixed order) and read by both modes
    dm.phase_gradient_direction(L.MS_STEPPER_CG, False)
    for what, kw in (("x", at_x), ("x + alpha d", trial)):
        fixed = _energy_scalars(dm, True, **kw)
        again = _energy_scalars(dm, True, **kw)
        atomic = _energy_scalars(dm, False, **kw)
        keys = (L.MS_S_ESURF, L.MS_S_EBEND, L.MS_S_MINEDGE2)
        print(name, what, "fixed", [fixed[k] for k in keys], "atomic", [atomic[k] for k in keys],
              "rel", [_rel(atomic[k], fixed[k]) for k in keys])
        assert np.array_equal(fixed, again), what
        if what == "x":
            assert np.array_equal(fixed[list(keys)], fx[list(keys)])
        assert fixed[L.MS_S_ESURF] > 0.0 and fixed[L.MS_S_EBEND] > 0.0 and 0.0 < fixed[L.MS_S_MINEDGE2] < 1.0
        assert atomic[L.MS_S_MINEDGE2] == fixed[L.MS_S_MINEDGE2], what
        assert _rel(atomic[L.MS_S_ESURF], fixed[L.MS_S_ESURF]) <= E_RTOL, what
        assert _rel(atomic[L.MS_S_EBEND], fixed[L.MS_S_EBEND]) <= E_RTOL, what
    _check_tiles(name, dm)
    dm.close()


def _direction_scalars(dm, deterministic, use_history):
    """One fused gradient + direction pass -> (scalars, max_i |g_i|^2, max_i |d_i|^2 of the stored rows)"""
    from membrane_solver_amd import _lib as L

    dm.set_deterministic(deterministic)
    dm.phase_set_factors_valid(True)
    dm.phase_gradient_direction(L.MS_STEPPER_CG, use_history)
    sc = dm.fetch_scalars()
    g, d = dm.get_gradient(), dm.get_vertex_buffer(L.MS_BUF_D)
    return sc, float(np.max(np.einsum("ij,ij->i", g, g))), float(np.max(np.einsum("ij,ij->i", d, d)))


@pytest.mark.parametrize("name", sorted(MESHES))
def test_direction_scalars_of_both_modes_agree(name):
    """ms_phase_gradient_direction (CG) without and with history: MS_S_GNORM2 / MS_S_GDOTD / MS_S_MAXD2 / MS_S_MAXG2 of
    the two modes within 1e-11, the maxima never below the rows' own (NumPy) maximum less 1e-11; the fixed-order
    scalars repeat bit for bit."""
    from membrane_solver_amd import _lib as L

    dm = _device(name)
    dm.set_deterministic(True)
    dm.phase_energy(write_bending_factors=True)
    for use_history in (False, True):
        if use_history:
            # accept a trial point along d = -g: x moves, the CG history becomes (g, d), the factors are the new x's
            dm.set_deterministic(True)
            dm.phase_set_factors_valid(True)
            dm.phase_gradient_direction(L.MS_STEPPER_CG, False)
            dm.phase_energy(use_direction=True, alpha=ALPHA, write_trial=True, write_bending_factors=True)
            dm.phase_accept(True)
        fixed, _g2, _d2 = _direction_scalars(dm, True, use_history)
        again, _g2, _d2 = _direction_scalars(dm, True, use_history)
        assert np.array_equal(fixed, again), use_history
        atomic, g2_rows, d2_rows = _direction_scalars(dm, False, use_history)
        keys = (L.MS_S_GNORM2, L.MS_S_GDOTD, L.MS_S_MAXD2, L.MS_S_MAXG2)
        print(name, "history" if use_history else "no history", "fixed", [fixed[k] for k in keys],
              "atomic", [atomic[k] for k in keys], "rel", [_rel(atomic[k], fixed[k]) for k in keys],
              "rows", g2_rows, d2_rows)
        assert fixed[L.MS_S_GNORM2] > 0.0 and fixed[L.MS_S_GDOTD] < 0.0
        for k in keys:
            assert _rel(atomic[k], fixed[k]) <= G_RTOL, (use_history, k)
        assert atomic[L.MS_S_MAXG2] >= g2_rows * (1.0 - G_RTOL), use_history
        assert atomic[L.MS_S_MAXD2] >= d2_rows * (1.0 - G_RTOL), use_history
        if use_history:
            assert atomic[L.MS_S_GDOTD] != -atomic[L.MS_S_GNORM2]  # (some row is a Polak-Ribiere row, not -g)
    _check_tiles(name, dm)
    dm.close()


def test_multi_trial_launches_replay_without_mismatch():
    """20 CG steps of ms_minimize on ico12 in the default mode: the host replays every decision the device took from the
    same doubles, so a wrong partial of a multi-trial launch shows as a mismatch."""
    from membrane_solver_amd import _lib as L

    dm = _device("ico12")
    dm.set_deterministic(False)
    mp = L.ms_minimize_params()
    mp.stepper = L.ms_stepper_params(L.MS_STEPPER_CG, 10, 0.7, 1e-4, 1.5, 10.0, 10, 0.0, 2, 0, 0, 0)
    mp.step_size, mp.tol = 1e-3, 1e-6
    mp.fixed_step_mode, mp.fixed_step = 0, 1e-3
    mp.max_zero_steps, mp.step_size_floor = 10, 1e-8
    out, _log = dm.minimize(mp, 20)
    qs = dm.queue_stats()
    print(qs, out.iterations, out.accepted, out.trials)
    dm.close()
    assert out.iterations == 20 and out.accepted > 0
    assert qs["mismatches"] == 0, qs
    assert qs["multi_launches"] >= 1, qs
