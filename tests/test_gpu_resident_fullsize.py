"""The resident step kernel (csrc/ms_resident.inc) at the size it is on for -- BASELINE config 2, icosphere f = 81,
65 612 vertices, 257 tiles on 256 CUs -- and at the tile counts where its index arithmetic changes behaviour: the
barrier's group sizes (nwg / 8 and the remainder), the second half of res_fold_n (tiles >= 256), a last tile with one
owned row and one that is exactly full, the first CU with two workgroups, the co-residency limit of resident_fits
and one tile past it, and ms_minimize's RES_CHUNK steps-per-launch boundary.  The meshes are in resident_meshes.py
(what the cuts leave is checked on the CPU in test_host_logic.py).

Three kinds of check: against the oracle's minimizer port (an independent CPU restatement of the loop), bit for bit
against the kernel-per-phase path (MS_RESIDENT=0) with fixed-order vertex sums, and the resident lane against itself
over thousands of grid barriers.

Every decline of a step by the kernel costs the ordinary path at most nine iterations (the declined one and a cooldown
of eight), and a single remaining step is never given to the kernel: a run of n iterations that does not converge has
at least n - 9 * declined - 1 resident steps.  The tests hold the lane to that, so a lane that quietly stops running
fails them.

Figures of one MI355X run (gfx950, 256 CUs) are in the docstrings below and in DESIGN.md 4d; every test prints its
own (pytest -s)."""
from __future__ import annotations

import functools

import numpy as np
import pytest

from resident_meshes import CUT_TABLE, _cut_icosphere
from test_gpu_resident import _params

pytestmark = pytest.mark.gpu

SIZES = sorted(CUT_TABLE, key=lambda fk: (CUT_TABLE[fk][1], CUT_TABLE[fk][0]))  # by tile count, then vertex count
CLOSED = [fk for fk in SIZES if fk[1] == 0]
RES_CHUNK = 4096  # csrc/ms_api_step.inc

def _record(section, key, value):
    """The figures of a run, on the test's output."""
    print(f"\n[resident_fullsize] {section} {key}: {value}")


@functools.lru_cache(maxsize=None)
def _mesh(freq, k):
    P, T = _cut_icosphere(freq, k)
    P.setflags(write=False)
    T.setflags(write=False)
    return P, T


_TILE_STATS_SEEN = set()


def _note_tiles(dm, freq, k, nv):
    """tile_stats() of a mesh, once: the smallest tile is the last one, min(256, nv - 256 * tile) rows (tile_ctx)."""
    if (freq, k) in _TILE_STATS_SEEN:
        return
    _TILE_STATS_SEEN.add((freq, k))
    ts = dm.tile_stats()
    ts["last_tile_rows"] = nv - 256 * (ts["n_tiles"] - 1)
    _record("tile_stats", f"f{freq}_k{k}", ts)
    if (freq, k) in CUT_TABLE:
        assert ts["n_tiles"] == CUT_TABLE[(freq, k)][1] and ts["last_tile_rows"] == CUT_TABLE[(freq, k)][2]


def _run(monkeypatch, resident, *, freq, k=0, volume, n_steps, step_size, fixed_every=0, noise=0.0, tol=0.0):
    """tests/test_gpu_resident.py::_run on a mesh of the table."""
    from membrane_solver_amd import _lib as L
    from membrane_solver_amd.device import DeviceMesh

    monkeypatch.setenv("MS_RESIDENT", "1" if resident else "0")
    pos, tri = _mesh(freq, k)
    if noise:
        pos = pos + noise * np.random.default_rng(5).standard_normal(pos.shape)
    fixed = None
    if fixed_every:
        fixed = np.zeros(len(pos), dtype=np.uint8)
        fixed[::fixed_every] = 1
    dm = DeviceMesh(pos, tri, fixed=fixed, body_facets=np.ones(len(tri), dtype=np.uint8) if volume else None)
    try:
        _note_tiles(dm, freq, k, len(pos))
        dm.set_surface_tension(np.full(len(tri), 1.0))
        mods = L.MS_MOD_SURFACE | (L.MS_CON_VOLUME if volume else 0)
        V0 = 0.0
        dm.set_params(modules=mods)
        if volume:
            dm.energy()
            V0 = float(dm.fetch_scalars()[L.MS_S_VOL])
            dm.set_params(modules=mods, target_volume=V0)
        mp = _params(L, step_size=step_size, drift=volume, target=V0, tol=tol)
        out, log = dm.minimize(mp, n_steps, want_log=True)
        return {"log": log.copy(), "x": dm.get_positions(), "stats": dm.resident_stats(), "accepted": out.accepted,
                "trials": out.trials, "iterations": out.iterations, "step_size": out.step_size,
                "converged": out.converged, "n": n_steps}
    finally:
        dm.close()


def _check_lane(res):
    """The verdict is the device's; what follows from it is not: a co-resident mesh runs its steps in the kernel (all
    but nine per declined step and a last single one), a refused one never launches it."""
    st, n = res["stats"], res["n"]
    assert st["co_resident"] in (0, 1), st
    if st["co_resident"] == 1:
        assert st["launches"] > 0 and st["steps"] > 0, st
        assert 0 <= n - st["steps"] <= 9 * st["declined"] + 1, (st, n)
    else:
        assert st["launches"] == 0 and st["steps"] == 0 and st["declined"] == 0, st


def _same(got, ref):
    assert got["iterations"] == ref["iterations"] and got["accepted"] == ref["accepted"]
    assert got["trials"] == ref["trials"] and got["converged"] == ref["converged"]
    assert got["log"].shape == ref["log"].shape and got["log"].shape[1] == 8
    for col in range(8):
        assert np.array_equal(got["log"][:, col], ref["log"][:, col]), \
            (col, np.flatnonzero(got["log"][:, col] != ref["log"][:, col])[:5])
    assert np.array_equal(got["x"], ref["x"]), int((got["x"] != ref["x"]).any(axis=1).sum())
    assert got["step_size"] == ref["step_size"]


# ---- 1. against the independent reference -----------------------------------------------------------------------------
ORACLE_CASES = {
    # BASELINE config 2: closed, surface + Lagrange volume row (projection off), searches that backtrack
    "A_f81_closed_volume_row": dict(freq=81, k=0, volume=True, step_size=3.0, n=40),
    # one owned row in the 257th tile, open surface, surface tension only
    "B_f81_cut75_surface": dict(freq=81, k=75, volume=False, step_size=1e-3, n=20),
}


@pytest.mark.parametrize("name", sorted(ORACLE_CASES))
def test_resident_trajectory_matches_oracle_port_at_full_size(name, monkeypatch):
    """Minimizer.minimize(n) with the stock stepper: ms_minimize runs the steps, the resident kernel takes them (257
    workgroups, default LDS-atomic vertex sums, default tile size).  The oracle's minimizer port runs the same steps
    on the CPU: equal success flags and trial counts, step sizes to 1e-12, accepted energies and the final energy to
    1e-10, positions to 1e-8 of the distance the run moved them -- the bars of
    test_gpu_minimizer.py::test_full_size_trajectory_matches_oracle_port, which the Python step loop meets.

    The oracle accepts every step of both cases (A: 40 steps of 1-3 trials; B: 20 steps of one trial).

    MI355X (largest deviation from the port over the run; the kernel declines a step when a search reaches the
    guard range, the ordinary path then takes that step and the next eight):
      A: 31 of 40 steps resident in 2 launches, 1 declined (9 outside); accepted energies 1.3e-14, final energy
         2.7e-15, step sizes equal, positions 2.3e-13 of the 2.586 the run moved them;
      B: 13 of 20 steps resident in 1 launch, 1 declined (7 outside); energies 1.8e-15, final energy 1.9e-15, step
         sizes equal, positions 5.1e-14 of 0.1188.  tile_stats: 257 tiles, 148 584 facet instances, longest halo 82,
         ONE owned row in the last tile."""
    from membrane_solver_amd.geometry.mesh import ArrayBody, ArrayMesh
    from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager
    from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager
    from membrane_solver_amd.runtime.minimizer import Minimizer
    from membrane_solver_amd.runtime.steppers import GradientDescent
    from oracle import minimizer_port as mp
    from oracle import ms_oracle as orc

    case = ORACLE_CASES[name]
    n = case["n"]
    monkeypatch.delenv("MS_RESIDENT", raising=False)
    monkeypatch.delenv("MS_DETERMINISTIC", raising=False)
    P, T = _mesh(case["freq"], case["k"])
    if case["volume"]:
        mods, cons = ["surface"], ["volume"]
        gp = {"surface_tension": 1.0, "volume_constraint_mode": "lagrange",
              "volume_projection_during_minimization": False}
    else:
        mods, cons, gp = ["surface"], [], {"surface_tension": 1.0}
    orc.use_openmp(True)  # (the checker may use the host's cores; the serial build gives the same trajectory)
    try:
        V0 = 0.97 * orc.volume(P, T, None) if case["volume"] else None
        p = mp.Problem(positions=P, tri=T, energy_modules=list(mods), constraint_modules=list(cons), gp=dict(gp),
                       target_volume=V0)
        ref = mp.minimize(p, mp.GradientDescent(), n, step_size=case["step_size"])
    finally:
        orc.use_openmp(False)
    bodies = [ArrayBody(0, None, float(V0))] if V0 is not None else []
    mesh = ArrayMesh(np.array(P), np.array(T), bodies=bodies, global_parameters=dict(gp), energy_modules=list(mods),
                     constraint_modules=list(cons))
    mz = Minimizer(mesh, mesh.global_parameters, GradientDescent(), EnergyModuleManager(mods),
                   ConstraintModuleManager(cons), quiet=True, step_size=case["step_size"])
    res = mz.minimize(n)
    dm = mz._device()[1]
    _note_tiles(dm, case["freq"], case["k"], len(P))
    stats = dm.resident_stats()
    got = np.asarray(mz.last_run["step_log"])
    want = np.array([[float(t["success"]), t["next_step"], t["E_accepted"], t["trials"]] for t in ref["trace"]])
    assert want.shape == (n, 4) and want[:, 0].all(), "the oracle is expected to accept every step of this case"
    assert got.shape == (n, 8) and mz.last_run["iterations"] == n
    moved = float(np.linalg.norm(p.positions - P))
    dx = float(np.linalg.norm(mesh.positions_view() - p.positions))
    figures = {"resident_stats": stats, "steps_outside": n - stats["steps"],
               "max_energy_rel": float(np.max(np.abs(got[:, 2] - want[:, 2]) / np.abs(want[:, 2]))),
               "max_step_size_rel": float(np.max(np.abs(got[:, 1] - want[:, 1]) / np.abs(want[:, 1]))),
               "final_energy_rel": float(abs(res["energy"] - ref["energy"]) / abs(ref["energy"])),
               "position_dev_over_moved": dx / moved, "moved": moved,
               "trials_hip": got[:, 7].astype(int).tolist(), "trials_oracle": want[:, 3].astype(int).tolist()}
    _record("oracle", name, figures)
    assert stats["co_resident"] == 1, stats
    assert stats["steps"] > 0 and stats["launches"] > 0, stats
    assert 0 <= n - stats["steps"] <= 9 * stats["declined"] + 1, stats  # steps + (steps taken outside) == n
    assert np.array_equal(got[:, 0], want[:, 0]), (got[:, 0], want[:, 0])
    assert np.array_equal(got[:, 7], want[:, 3]), (got[:, 7], want[:, 3])
    assert np.allclose(got[:, 1], want[:, 1], rtol=1e-12, atol=0)
    assert np.allclose(got[:, 2], want[:, 2], rtol=1e-10, atol=0)
    assert abs(res["energy"] - ref["energy"]) <= 1e-10 * abs(ref["energy"])
    assert moved > 0.0
    assert dx <= 1e-8 * moved


# ---- 2. bitwise against the kernel-per-phase path, at size and at the edges ------------------------------------------
BITWISE = {f"surface_f{f}_k{k}": dict(freq=f, k=k, volume=False, n_steps=60, step_size=1e-3) for f, k in SIZES}
BITWISE.update({f"volume_row_f{f}": dict(freq=f, k=0, volume=True, n_steps=60, step_size=1e-3) for f, k in CLOSED})
BITWISE["fixed_rows_f81"] = dict(freq=81, k=0, volume=True, n_steps=60, step_size=1e-3, fixed_every=7)
# an over-long first step on a noisy mesh: the first searches backtrack, some run into the guard range (declined steps)
BITWISE["backtracking_and_guard_f81"] = dict(freq=81, k=0, volume=True, n_steps=60, step_size=0.3, noise=2e-3)


@pytest.mark.parametrize("name", sorted(BITWISE))
def test_resident_steps_equal_the_kernel_per_phase_path_at_size(name, deterministic, monkeypatch):
    """60 steps with fixed-order vertex sums: all 8 columns of the step log, the positions, iterations, accepted,
    trials and the final step size are those of MS_RESIDENT=0, bit for bit -- at 255, 256, 257, 508, 512, 513 and 517
    tiles, with last tiles of 1, 255 and 256 rows.  Whether a size is co-resident is the device's answer
    (resident_stats); what the lane then has to do is not (see _check_lane).

    MI355X: co-resident up to 512 tiles (two workgroups per CU), refused at 513 (one owned row in the last tile; 297 162
    facet instances, longest halo 84) and 517.  With the volume row all 60 steps run in one launch (f = 81, f = 114);
    surface tension alone grows the step into the guard range: 13-26 of 60 steps resident, 4-6 declined; fixed rows
    19 resident steps and 5 declined; the over-long noisy start 5 resident steps and 7 declined.  With res_fold_n's
    h = 1 half switched off (a throw-away build) every co-resident case above 256 tiles fails here and no case of
    test_gpu_resident.py does."""
    case = BITWISE[name]
    ref = _run(monkeypatch, False, **case)
    got = _run(monkeypatch, True, **case)
    _record("bitwise", name, {"tiles": CUT_TABLE[(case["freq"], case["k"])][1], "resident_stats": got["stats"],
                              "accepted": int(got["accepted"]), "trials": int(got["trials"])})
    assert ref["stats"]["launches"] == 0 and ref["stats"]["steps"] == 0
    assert ref["iterations"] == case["n_steps"] and not ref["converged"]
    if case["freq"] == 81:
        assert got["stats"]["co_resident"] == 1, got["stats"]  # the size the lane is on for
    _check_lane(got)
    _same(got, ref)


_VERDICTS = []


def _verdicts(monkeypatch):
    """-> [(tiles, nv, (freq, k), co_resident)] over the table, by tile count: two surface steps each (asked once)."""
    if _VERDICTS:
        return list(_VERDICTS)
    rows = _VERDICTS
    for f, k in SIZES:
        r = _run(monkeypatch, True, freq=f, k=k, volume=False, n_steps=2, step_size=1e-3)
        _check_lane(r)
        rows.append((CUT_TABLE[(f, k)][1], CUT_TABLE[(f, k)][0], (f, k), r["stats"]["co_resident"]))
    return list(rows)


def test_coresidency_verdict_switches_off_once(deterministic, monkeypatch):
    """resident_fits over the table's sizes in the order of their tile counts: co-resident up to some count, refused
    from there on, never back.  f = 81 is co-resident, some size above 257 tiles is, and some size is refused: the
    sizes on both sides of the limit are really among those the bitwise test runs.  (The table was enough: no larger
    mesh had to be added.)"""
    rows = _verdicts(monkeypatch)
    verdict = {f"{tiles}_tiles_f{f}_k{k}": co for tiles, _nv, (f, k), co in rows}
    _record("co_residency", "by_tile_count", verdict)
    cos = [co for *_rest, co in rows]
    assert all(a >= b for a, b in zip(cos, cos[1:])), verdict
    assert all(co == 1 for _t, _nv, (f, _k), co in rows if f == 81), verdict
    assert any(co == 1 and tiles > 257 for tiles, _nv, _fk, co in rows), verdict
    assert any(co == 0 for co in cos), verdict


# ---- 3. long run and repeatability -----------------------------------------------------------------------------------
def _long_run_three_ways(monkeypatch, freq, k, n_steps=2000):
    """The resident lane twice (two runs, not a loop) and the kernel-per-phase path once; the volume row is on where
    the mesh is closed."""
    case = dict(freq=freq, k=k, volume=(k == 0), n_steps=n_steps, step_size=1e-3, tol=0.0)
    first = _run(monkeypatch, True, **case)
    second = _run(monkeypatch, True, **case)
    ref = _run(monkeypatch, False, **case)
    _record("long_run", f"f{freq}_k{k}", {"tiles": CUT_TABLE[(freq, k)][1], "first": first["stats"],
                                          "second": second["stats"], "accepted": int(ref["accepted"])})
    assert ref["iterations"] == n_steps and not ref["converged"] and ref["stats"]["launches"] == 0
    assert first["stats"]["co_resident"] == 1, first["stats"]
    _check_lane(first)
    _check_lane(second)
    _same(second, first)
    _same(first, ref)
    return first


def test_resident_long_run_repeats_itself_and_the_kernel_per_phase_path(deterministic, monkeypatch):
    """f = 81 closed with the volume row, 2000 steps that do not converge (tol = 0), fixed-order sums: the resident
    lane twice and MS_RESIDENT=0 once give the same log and positions, bit for bit.  A difference between the two
    resident runs would point at res_barrier's ordering (relaxed atomics, no release between a workgroup's st_agent
    stores and its arrival).

    MI355X: all 2000 steps accepted, all of them in ONE launch of 257 workgroups, none declined (a grid barrier behind
    the gradient and one behind every search phase: 4000 or more per run), both resident runs and the
    kernel-per-phase path equal in every bit."""
    _long_run_three_ways(monkeypatch, 81, 0)


def test_resident_long_run_at_the_largest_coresident_sizes(deterministic, monkeypatch):
    """The same three runs at the largest size of the table that resident_fits accepts, and at the largest CLOSED one
    when that is another mesh: two workgroups on (nearly) every CU.  A cut mesh runs surface tension only (a volume
    row on an open surface stalls the search within a few hundred steps); its free rim takes the searches into the
    guard range again and again, so that run is many short launches; the closed one is the long launch.

    MI355X: 512 tiles (f = 115 without 1180 vertices, surface only): 112 of 2000 steps resident in 210 launches, 210
    declined, 1014 accepted; 508 tiles (f = 114 closed, volume row): 2000 steps in one launch, none declined.  All
    three runs of each equal in every bit."""
    co = [(tiles, nv, fk) for tiles, nv, fk, c in _verdicts(monkeypatch) if c == 1]
    assert co, "no co-resident size"
    tiles, _nv, largest = max(co)
    assert tiles > 257, "the largest co-resident size is expected beyond one workgroup per CU"
    _long_run_three_ways(monkeypatch, *largest)
    closed = [(t, nv, fk) for t, nv, fk in co if fk[1] == 0]
    if max(closed)[2] != largest:
        assert max(closed)[0] > 257
        _long_run_three_ways(monkeypatch, *max(closed)[2])


# ---- 4. launch-chunk edge --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_steps", [RES_CHUNK + 1, RES_CHUNK + 2, 4100])
def test_resident_launch_is_cut_at_the_chunk(n_steps, deterministic, monkeypatch):
    """f = 12 closed (6 tiles), volume row with V0 = V, step size 1e-3, tol = 0: the oracle port accepts all 4100 steps
    in one unbroken run.  A launch takes at most RES_CHUNK = 4096 steps; one remaining step goes through the ordinary
    path (4097: one launch, 4096 resident steps), two or more start a second launch (4098, 4100: every step
    resident).  Bit for bit the kernel-per-phase path's.  MI355X: the kernel declines no step of this run, so the
    launch and step counts are asserted exactly."""
    case = dict(freq=12, k=0, volume=True, n_steps=n_steps, step_size=1e-3, tol=0.0)
    ref = _run(monkeypatch, False, **case)
    got = _run(monkeypatch, True, **case)
    st = got["stats"]
    _record("chunk", f"n{n_steps}", st)
    assert ref["iterations"] == n_steps and ref["accepted"] == n_steps and not ref["converged"]
    assert st["co_resident"] == 1 and st["declined"] == 0, st
    if n_steps == RES_CHUNK + 1:
        assert st["launches"] == 1 and st["steps"] == RES_CHUNK, st
    else:
        assert st["launches"] == 2 and st["steps"] == n_steps, st
    _same(got, ref)
