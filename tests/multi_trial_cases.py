"""Line searches long enough to reach energy launches of four to eight trials (k_energy<..., MULTI == 8>): the meshes,
the strict Armijo parameters and the CPU oracle's view of each ladder.  Shared by test_multi_trial_host.py (the ladders'
preconditions, on the CPU) and test_gpu_multi_trial.py (the launches against them).

With the reference's c = 1e-4, beta = 0.7 a search on a small mesh rejects three or four alphas below the guard range;
with c = 0.9 and beta = 0.9 (0.92 on the largest mesh) the ladder from 0.9 x the safe limit rejects twenty and more,
every one of them in the queued regime (above the safe limit 0.3 min_edge / max|d| the step decides on the host and
queues no round)."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

# name -> (icosphere frequency, tile_vertices (0: the default 256), tiles, seed of the noise, beta of the ladder)
MESHES = {
    "ico6": (6, 0, 2, 3, 0.9),           # 362 vertices: 256 + 106 rows, six idle blocks per trial
    "ico13": (13, 0, 7, 3, 0.9),         # 1 692 vertices: one idle block per trial
    "ico14": (14, 0, 8, 3, 0.9),         # 1 962 vertices: no idle block
    "ico15": (15, 0, 9, 3, 0.9),         # 2 252 vertices: seven idle blocks per trial
    # the mesh of test_pair_launch_does_not_change_the_trajectory; beta 0.9 rejects 19 alphas only, 0.92 rejects 24
    "ico24": (24, 0, 23, 3, 0.92),
    "ico12_t64": (12, 64, 23, 3, 0.9),   # 1 442 vertices in tiles of 64 rows: the runtime-size instances
}
GP = {"surface_tension": 1.0, "bending_modulus": 1.0, "spontaneous_curvature": 0.2}
C1, MAX_ITER = 0.9, 48
GAMMA, ALPHA_MAX_FACTOR = 1.5, 10.0
MIN_REJECTED = 20  # a ladder must reject this many alphas, and leave four trials of max_iter unused


def alphas_from(alpha0, n, beta):
    """alpha0 * beta^j by repeated multiplication, as the loop of line_search.py forms them."""
    out = np.empty(n)
    a = float(alpha0)
    for j in range(n):
        out[j] = a
        a *= beta
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    """-> the mesh, the oracle's problem, energy, gradient, safe limit and first alpha (0.9 x the safe limit)."""
    from membrane_solver_amd import meshgen
    from oracle import minimizer_port as mp

    freq, tile, tiles, seed, beta = MESHES[name]
    P, T = meshgen.icosphere(freq)
    P = meshgen.smooth_displace(P, 0.05)
    P = P + 2.0e-3 * np.random.default_rng(seed).standard_normal(P.shape)
    P, T = np.ascontiguousarray(P, dtype=np.float64), np.ascontiguousarray(T, dtype=np.int32)
    p = mp.Problem(positions=P, tri=T, energy_modules=["surface", "bending"], gp=dict(GP))
    E0, g = mp.energy_and_gradient(p, P)
    safe = 0.3 * mp.min_edge_length(P, T) / float(np.max(np.linalg.norm(g, axis=1)))
    for a in (P, T, g):
        a.setflags(write=False)
    return SimpleNamespace(name=name, P=P, T=T, tile=tile, tiles=tiles, p=p, E0=E0, g=g, safe=safe, alpha0=0.9 * safe,
                           beta=beta)


def problem(cs):
    """A fresh oracle problem at the case's positions (line_search and minimize move theirs)."""
    from oracle import minimizer_port as mp

    return mp.Problem(positions=cs.P, tri=cs.T, energy_modules=["surface", "bending"], gp=dict(GP))


def ladder(cs, d, alphas):
    """The fp64 oracle's total energy at x + alpha d for every alpha."""
    from oracle import minimizer_port as mp

    return np.array([mp.energy_total(cs.p, cs.P + a * d) for a in alphas])


@functools.lru_cache(maxsize=None)
def oracle_ladder(name):
    """The ladder from alpha0 along d = -g of the oracle, three alphas past the first accepted one.
    -> alphas, energies, right-hand sides, R (alphas rejected), smallest slack |E_t - rhs_t| / |E0|."""
    cs = case(name)
    d = -cs.g
    gdd = float(np.sum(cs.g * d))
    alphas = alphas_from(cs.alpha0, MAX_ITER, cs.beta)
    rhs = cs.E0 + C1 * alphas * gdd
    E = np.full(MAX_ITER, np.nan)
    R = None
    for j in range(MAX_ITER):
        E[j] = ladder(cs, d, alphas[j:j + 1])[0]
        if R is None and E[j] <= rhs[j]:
            R = j
        if R is not None and j >= R + 3:
            break
    n = j + 1
    slack = float(np.min(np.abs(E[:n] - rhs[:n])) / abs(cs.E0))
    return SimpleNamespace(alphas=alphas[:n], E=E[:n], rhs=rhs[:n], R=R, slack=slack, gdd=gdd)


def check_preconditions(name):
    """What every device assertion on this mesh rests on: a long ladder inside max_iter, monotone acceptance behind
    the first accepted alpha, and no decision that hinges on rounding."""
    lad = oracle_ladder(name)
    assert lad.R is not None and MIN_REJECTED <= lad.R <= MAX_ITER - 4, (name, lad.R)
    assert len(lad.E) == lad.R + 4 and (lad.E[lad.R:] <= lad.rhs[lad.R:]).all(), (name, "acceptance is not monotone")
    assert (lad.E[:lad.R] > lad.rhs[:lad.R]).all()
    assert lad.slack > 1e-9, (name, lad.slack)
    return lad
