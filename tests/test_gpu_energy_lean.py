"""The lean instances of the energy kernel (energy_body's LEANE, csrc/ms_kernels.hip) against the general instance and
against the CPU oracle.

The lean instance runs where the headline does: surface + Helfrich bending, uniform parameters, closed surface, default
(LDS-atomic) mode, more than one tile.  MS_KA_LEAN=0 at ms_create forces the general instance.  The lean instance is the
general arithmetic operation for operation, so it is compared with the general instance at the level of the atomic
sums' own run-to-run scatter, and held to the bars of test_gpu_kernels.py against oracle.ms_oracle.

Meshes: icosphere f = 6 (362 vertices, 2 tiles), 8 (642, 3 tiles), 13 (1 692, 7 tiles: an idle block in the multi-trial
grid), smooth_displace 0.05, default tile of 256 rows; and an f = 8 mesh with 20 vertices pulled along an edge until
that edge is 1e-3 of the mean edge (slivers: where cotangents and mixed areas lose the most digits)."""

import functools
from types import SimpleNamespace

import numpy as np
import pytest

import multi_trial_cases as mt
from conftest import load_golden, relerr

pytestmark = pytest.mark.gpu

E_TOL = 1e-12   # energies, relative (test_gpu_kernels.py)
F_TOL = 1e-10   # factor rows, of max |row| (test_gpu_kernels.py)
GP = {"surface_tension": 1.0, "bending_modulus": 1.0, "spontaneous_curvature": 0.2}
TILES = {6: 2, 8: 3, 13: 7}
LEAN_ENV = ("MS_KA_LEAN",)
QUEUE_ENV = ("MS_ESCALATE", "MS_PAIR", "MS_SPECULATE", "MS_PAIR_LEAN", "MS_AHEAD", "MS_DETERMINISTIC", "MS_EXEC")
GENERAL = {"MS_KA_LEAN": "0"}


@functools.lru_cache(maxsize=None)
def _ico(freq):
    from membrane_solver_amd import meshgen

    P, T = meshgen.icosphere(freq)
    P = np.ascontiguousarray(meshgen.smooth_displace(P, 0.05), dtype=np.float64)
    T = np.ascontiguousarray(T, dtype=np.int32)
    assert len(P) == {6: 362, 8: 642, 13: 1692}[freq]
    for a in (P, T):
        a.setflags(write=False)
    return P, T


def _edge_lengths(P, T):
    e = np.concatenate([P[T[:, 1]] - P[T[:, 0]], P[T[:, 2]] - P[T[:, 1]], P[T[:, 0]] - P[T[:, 2]]])
    return np.linalg.norm(e, axis=1)


@functools.lru_cache(maxsize=None)
def _pulled(ratio=1e-3, count=20):
    """f = 8 with `count` vertices, no two of them neighbours or neighbours of one vertex, each pulled along one of its
    edges towards the other end until the edge is `ratio` of the mesh's mean edge."""
    P0, T = _ico(8)
    P = P0.copy()
    nbrs = [set() for _ in range(len(P))]
    for a, b, c in T:
        nbrs[a] |= {int(b), int(c)}
        nbrs[b] |= {int(a), int(c)}
        nbrs[c] |= {int(a), int(b)}
    mean = float(_edge_lengths(P0, T).mean())
    used, moved = set(), 0
    for i in range(0, len(P), 7):
        ring = {i} | nbrs[i]
        two_ring = set().union(*(nbrs[j] for j in ring)) | ring
        if two_ring & used:
            continue
        j = min(nbrs[i])
        u = P0[i] - P0[j]
        P[i] = P0[j] + u * (ratio * mean / np.linalg.norm(u))
        used |= ring
        moved += 1
        if moved == count:
            break
    assert moved == count
    L = _edge_lengths(P, T)
    assert abs(L.min() / L.mean() - ratio) < 0.05 * ratio
    P.setflags(write=False)
    return P, T


def _mesh(name):
    return _pulled() if name == "pulled" else _ico(name)


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """oracle.ms_oracle at the mesh's positions: (E_surface, E_bending, fK, fA (nv, 2)), serial build, never written to"""
    from oracle import ms_oracle as orc

    P, T = _mesh(name)
    nv, nf = len(P), len(T)
    Es = orc.surface_energy_and_gradient(P, T, np.full(nf, GP["surface_tension"]), np.zeros_like(P))
    Eb, fK, fAe, fAv = orc.bending_energy_and_gradient(
        P, T, np.full(nv, GP["bending_modulus"]), np.full(nv, GP["spontaneous_curvature"]), np.zeros(nv, bool),
        grad=np.zeros_like(P), want_factors=True)
    fA = np.stack([fAe, fAv], axis=1)
    for a in (fK, fA):
        a.setflags(write=False)
    return float(Es), float(Eb), fK, fA


def _context(P, T, monkeypatch, env=None, *, fixed=None, boundary=None, kappa=None, gamma=None, modules=None,
             model=None, target_volume=0.0):
    from membrane_solver_amd import _lib as L
    from membrane_solver_amd.device import DeviceMesh

    for k in LEAN_ENV + QUEUE_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    nv, nf = len(P), len(T)
    dm = DeviceMesh(P, T, fixed=fixed, boundary=boundary)
    dm.set_surface_tension(np.full(nf, GP["surface_tension"]) if gamma is None else gamma)
    dm.set_bending_params(np.full(nv, GP["bending_modulus"]) if kappa is None else kappa,
                          np.full(nv, GP["spontaneous_curvature"]))
    dm.set_params(modules=(L.MS_MOD_SURFACE | L.MS_MOD_BENDING) if modules is None else modules,
                  bending_model=L.MS_BEND_HELFRICH if model is None else model, target_volume=target_volume)
    return dm


def _delta(dm, before):
    st = dm.energy_stats()
    return {k: st[k] - before[k] for k in st}


def _evaluate(dm, alpha=None):
    """One energy launch that writes factors (and trial positions): its scalars and rows, and what the stats counted."""
    from membrane_solver_amd import _lib as L

    before = dm.energy_stats()
    if alpha is None:
        dm.phase_energy(write_bending_factors=True)
    else:
        dm.phase_energy(use_direction=True, alpha=alpha, write_trial=True, write_bending_factors=True)
    sc = dm.fetch_scalars()
    out = {"e_surf": float(sc[L.MS_S_ESURF]), "e_bend": float(sc[L.MS_S_EBEND]), "min_e2": float(sc[L.MS_S_MINEDGE2]),
           "fK": dm.get_vertex_buffer(L.MS_BUF_FK), "fA": dm.get_vertex_buffer(L.MS_BUF_FA)}
    if alpha is not None:
        out["xt"] = dm.get_vertex_buffer(L.MS_BUF_XT)
    return out, _delta(dm, before)


def _fixed_order_direction(dm):
    """D = -g at x from fixed-order sums (the general instance, bitwise repeatable): the same doubles in every context"""
    from membrane_solver_amd import _lib as L

    dm.set_deterministic(True)
    before = dm.energy_stats()
    dm.phase_energy(write_bending_factors=True)
    assert _delta(dm, before) == {"lean": 0, "general": 1}, "fixed-order mode never selects the lean instance"
    dm.phase_gradient_direction(L.MS_STEPPER_GD, False)
    d = dm.get_vertex_buffer(L.MS_BUF_D)
    dm.set_deterministic(False)
    return d


# -- selection -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("freq", sorted(TILES))
def test_headline_case_selects_lean(freq, monkeypatch):
    """Surface + Helfrich bending with uniform parameters: every default-mode energy launch of an evaluation, of a
    gradient call and of three CG steps is a lean one; fixed-order mode (ms_set_deterministic) selects none."""
    from membrane_solver_amd import _lib as L

    P, T = _ico(freq)
    dm = _context(P, T, monkeypatch)
    assert dm.tile_stats()["n_tiles"] == TILES[freq]
    before = dm.energy_stats()
    assert before == {"lean": 0, "general": 0}
    dm.energy()
    dm.energy_and_gradient()
    for _ in range(3):
        dm.step(stepper=L.MS_STEPPER_CG, step_size=1e-3, reuse_energy0=2)
    st = dm.energy_stats()
    assert st["lean"] >= 5 and st["general"] == 0, st
    _fixed_order_direction(dm)  # (asserts one general launch, no lean one)
    dm.close()


@pytest.mark.parametrize("case", ["kappa_array", "boundary", "volume", "willmore", "switch"])
def test_other_cases_select_general(case, monkeypatch):
    """One launch condition broken at a time: only general launches."""
    from membrane_solver_amd import _lib as L
    from oracle import ms_oracle as orc

    P, T = _ico(8)
    kw, env = {}, None
    if case == "kappa_array":
        kw["kappa"] = 1.0 + 0.1 * np.random.default_rng(1).random(len(P))
    elif case == "boundary":
        g = load_golden("mesh_disk5.npz")
        P, T = g["positions"], g["tri"]
        assert g["is_boundary"].any()
        kw["boundary"] = g["is_boundary"]
    elif case == "volume":
        kw["modules"] = L.MS_MOD_SURFACE | L.MS_MOD_BENDING | L.MS_CON_VOLUME
        kw["target_volume"] = float(orc.volume(P, T, None))
    elif case == "willmore":
        kw["model"] = L.MS_BEND_WILLMORE
    else:
        env = GENERAL
    dm = _context(P, T, monkeypatch, env, **kw)
    dm.energy()
    dm.energy_and_gradient()
    dm.step(stepper=L.MS_STEPPER_CG, step_size=1e-3, reuse_energy0=2)
    st = dm.energy_stats()
    dm.close()
    assert st["general"] >= 3 and st["lean"] == 0, (case, st)


# -- the lean instance against the general one --------------------------------------------------------------------

def _ulp_floor(a):
    return 4.0 * np.spacing(float(np.max(np.abs(a))))


@pytest.mark.parametrize("alpha", [None, 2.0e-3])
@pytest.mark.parametrize("freq", sorted(TILES))
def test_lean_equals_general(freq, alpha, monkeypatch):
    """The default against MS_KA_LEAN=0, every 5th row fixed, at x and at x + alpha d (d = -g of fixed-order sums,
    the same doubles in both contexts).  The LDS-atomic sums are not bitwise repeatable, so the yardstick is measured
    here: twice the largest difference between two runs of the general instance on the same input, floored at 4 ulp of
    the array's largest magnitude, for e_surf, e_bend and every fK / fA row.  min_e2 and xt are bitwise equal."""
    P, T = _ico(freq)
    fixed = np.zeros(len(P), dtype=np.uint8)
    fixed[::5] = 1
    dm_g = _context(P, T, monkeypatch, GENERAL, fixed=fixed)
    dm_l = _context(P, T, monkeypatch, fixed=fixed)
    if alpha is not None:
        d_g, d_l = _fixed_order_direction(dm_g), _fixed_order_direction(dm_l)
        assert np.array_equal(d_g, d_l) and np.abs(d_g).max() > 0.0
    g1, n1 = _evaluate(dm_g, alpha)
    g2, n2 = _evaluate(dm_g, alpha)
    le, n3 = _evaluate(dm_l, alpha)
    dm_g.close()
    dm_l.close()
    assert n1 == n2 == {"lean": 0, "general": 1} and n3 == {"lean": 1, "general": 0}
    assert le["min_e2"] == g1["min_e2"] == g2["min_e2"]
    if alpha is not None:
        assert np.array_equal(le["xt"], g1["xt"]) and np.array_equal(g1["xt"], g2["xt"])
        assert np.array_equal(le["xt"][::5], P[::5]) and not np.array_equal(le["xt"], P)
    for key in ("e_surf", "e_bend", "fK", "fA"):
        a1, a2, b = (np.asarray(r[key]) for r in (g1, g2, le))
        scatter = float(np.max(np.abs(a1 - a2)))
        bound = max(2.0 * scatter, _ulp_floor(a1))
        diff = float(np.max(np.abs(b - a1)))
        print(f"f={freq} alpha={alpha} {key}: general run to run {scatter:.3e}, lean - general {diff:.3e}, bound {bound:.3e}")
        assert diff <= bound, (key, diff, bound)


# -- against the oracle -------------------------------------------------------------------------------------------

def test_pulled_mesh_is_within_the_oracle_s_own_reach():
    """On the CPU: the oracle's serial and OpenMP builds meet the bars of the device test on the pulled mesh (if they did
    not, the pull would have to be relaxed, never the bars)."""
    from oracle import ms_oracle as orc

    Es, Eb, fK, fA = _oracle("pulled")
    P, T = _pulled()
    nv, nf = len(P), len(T)
    orc.use_openmp(True)
    try:
        Es2 = orc.surface_energy_and_gradient(P, T, np.full(nf, GP["surface_tension"]), np.zeros_like(P))
        Eb2, fK2, fAe2, fAv2 = orc.bending_energy_and_gradient(
            P, T, np.full(nv, GP["bending_modulus"]), np.full(nv, GP["spontaneous_curvature"]), np.zeros(nv, bool),
            grad=np.zeros_like(P), want_factors=True)
    finally:
        orc.use_openmp(False)
    assert abs(Es2 - Es) <= E_TOL * abs(Es) and abs(Eb2 - Eb) <= E_TOL * abs(Eb)
    assert relerr(fK2, fK) <= F_TOL and relerr(np.stack([fAe2, fAv2], axis=1), fA) <= F_TOL


@pytest.mark.parametrize("name", [6, 8, 13, "pulled"])
def test_lean_matches_the_oracle(name, monkeypatch):
    """Energies within 1e-12 relative and factor rows within 1e-10 of max |row| of oracle.ms_oracle (the bars of
    test_gpu_kernels.py), on the three meshes and on the pulled one, lean launches only."""
    P, T = _mesh(name)
    Es, Eb, fK, fA = _oracle(name)
    dm = _context(P, T, monkeypatch)
    got, n = _evaluate(dm)
    dm.close()
    assert n == {"lean": 1, "general": 0}
    errs = (abs(got["e_surf"] - Es) / abs(Es), abs(got["e_bend"] - Eb) / abs(Eb), relerr(got["fK"], fK), relerr(got["fA"], fA))
    print(f"{name}: relative errors e_surf {errs[0]:.3e} e_bend {errs[1]:.3e} fK {errs[2]:.3e} fA {errs[3]:.3e}")
    assert errs[0] <= E_TOL and errs[1] <= E_TOL
    assert errs[2] <= F_TOL and errs[3] <= F_TOL
    # min_e2: the smallest of the facets' own three-term inner products e.e (each within 3 ulp of its value)
    e = np.concatenate([P[T[:, 1]] - P[T[:, 0]], P[T[:, 2]] - P[T[:, 1]], P[T[:, 0]] - P[T[:, 2]]])
    L2 = float(np.einsum("ij,ij->i", e, e).min())
    assert abs(got["min_e2"] - L2) <= 4.0 * np.spacing(L2)


# -- multi-trial launches ------------------------------------------------------------------------------------------

def _mt_context(cs, monkeypatch, env, fixed=False):
    from membrane_solver_amd import _lib as L
    from membrane_solver_amd.device import DeviceMesh

    for k in LEAN_ENV + QUEUE_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    dm = DeviceMesh(cs.P, cs.T, tile_vertices=cs.tile)
    dm.set_deterministic(fixed)
    dm.set_surface_tension(np.full(len(cs.T), mt.GP["surface_tension"]))
    dm.set_bending_params(np.full(len(cs.P), mt.GP["bending_modulus"]), np.full(len(cs.P), mt.GP["spontaneous_curvature"]))
    dm.set_params(modules=L.MS_MOD_SURFACE | L.MS_MOD_BENDING)
    return dm


@functools.lru_cache(maxsize=None)
def _mt_case(freq):
    """multi_trial_cases.py's ico13, and at f = 8 (not one of its meshes) the same construction and parameters"""
    from membrane_solver_amd import meshgen
    from oracle import minimizer_port as mp

    if freq == 13:
        return mt.case("ico13")
    P, T = meshgen.icosphere(freq)
    P = meshgen.smooth_displace(P, 0.05)
    P = P + 2.0e-3 * np.random.default_rng(3).standard_normal(P.shape)
    P, T = np.ascontiguousarray(P, dtype=np.float64), np.ascontiguousarray(T, dtype=np.int32)
    p = mp.Problem(positions=P, tri=T, energy_modules=["surface", "bending"], gp=dict(mt.GP))
    E0, g = mp.energy_and_gradient(p, P)
    safe = 0.3 * mp.min_edge_length(P, T) / float(np.max(np.linalg.norm(g, axis=1)))
    for a in (P, T, g):
        a.setflags(write=False)
    return SimpleNamespace(name=f"ico{freq}", P=P, T=T, tile=0, tiles=TILES[freq], p=p, E0=E0, g=g, safe=safe,
                           alpha0=0.9 * safe, beta=0.9)


@pytest.mark.parametrize("freq", [8, 13])
def test_multi_trial_energies_match_the_oracle(freq, monkeypatch):
    """One gradient-descent step with multi_trial_cases.py's strict Armijo parameters for MS_ESCALATE in {1, 3, 5}:
    launches of 2, 3 and 5 (and more) trials.  Every logged trial energy within 1e-12 |E| of minimizer_port.energy_total
    at x + alpha_j d (d = -g of fixed-order sums), every energy launch a lean one; and the step result and the log's
    alphas, launches and slots are those of the MS_KA_LEAN=0 run, its energies within 1e-12."""
    from membrane_solver_amd import _lib as L

    cs = _mt_case(freq)
    dm = _mt_context(cs, monkeypatch, {}, fixed=True)
    _e, g = dm.energy_and_gradient()
    dm.close()
    d = -g
    sizes = set()
    for esc in ("1", "3", "5"):
        logs = {}
        for which, extra in (("lean", {}), ("general", GENERAL)):
            dm = _mt_context(cs, monkeypatch, dict({"MS_ESCALATE": esc}, **extra))
            r = dm.step(stepper=L.MS_STEPPER_GD, step_size=cs.alpha0, tol=1e-9, max_iter=mt.MAX_ITER, beta=cs.beta,
                        c=mt.C1, gamma=mt.GAMMA, alpha_max_factor=mt.ALPHA_MAX_FACTOR, reuse_energy0=2)
            logs[which] = (r, dm.search_trials(), dm.energy_stats(), dm.queue_stats())
            dm.close()
        r, log, st, qs = logs["lean"]
        rg, log_g, st_g, _qs = logs["general"]
        assert st["general"] == 0 and st["lean"] > 0 and st_g["lean"] == 0 and st_g["general"] > 0, (st, st_g)
        assert qs["mismatches"] == 0 and r.success and not log["guard"].any()
        E_ref = mt.ladder(cs, d, log["alpha"])
        err = np.abs(log["energy"] - E_ref) / np.abs(E_ref)
        first = sorted({int(v) for v in log["launch"][log["slot"] == 0]})
        print(f"f={freq} MS_ESCALATE={esc}: {len(err)} trials, launch sizes {first}, max |E - E_oracle|/|E| {err.max():.3e}")
        assert (err <= 1e-12).all(), err
        sizes |= set(first)
        for k in ("alpha", "launch", "slot", "behind", "guard"):
            assert np.array_equal(log[k], log_g[k]), k
        assert np.max(np.abs(log["energy"] - log_g["energy"]) / np.abs(log_g["energy"])) <= 1e-12
        assert (r.success, r.trials, r.alpha, r.next_step) == (rg.success, rg.trials, rg.alpha, rg.next_step)
    assert {2, 3, 5} <= sizes, sizes


def test_cg_trajectory_equals_the_general_run(monkeypatch):
    """Twelve CG steps of ms_minimize at f = 8 in the default mode: success flags, trial counts and step sizes of the
    lean run equal the MS_KA_LEAN=0 run's, accepted energies within 1e-10."""
    from membrane_solver_amd import _lib as L

    P, T = _ico(8)
    runs = {}
    for which, env in (("general", GENERAL), ("lean", None)):
        dm = _context(P, T, monkeypatch, env)
        prm = L.ms_minimize_params()
        prm.stepper = L.ms_stepper_params(L.MS_STEPPER_CG, 10, 0.7, 1e-4, 1.5, 10.0, 10, 0.0, 2)
        prm.step_size, prm.tol = 1e-3, 1e-9
        prm.fixed_step_mode, prm.fixed_step = 0, 1e-3
        prm.max_zero_steps, prm.step_size_floor = 10, 1e-8
        _out, log = dm.minimize(prm, 12, want_log=True)
        runs[which] = (np.array(log), dm.energy_stats())
        dm.close()
    want, st_g = runs["general"]
    assert len(want) == 12 and want[:, 0].sum() >= 6 and st_g["lean"] == 0
    for which in ("lean",):
        got, st = runs[which]
        assert st["general"] == 0 and st["lean"] > 0, st
        assert np.array_equal(got[:, 0], want[:, 0]), which   # success flags
        assert np.array_equal(got[:, 7], want[:, 7]), which   # trial counts
        assert np.array_equal(got[:, 1], want[:, 1]), which   # step sizes
        assert np.allclose(got[:, 2], want[:, 2], rtol=1e-10, atol=0), which
