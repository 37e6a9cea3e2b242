"""The problems the sharded step is run on, shared by test_gpu_sharded.py (HIP shards against the single context and
against the oracle's minimizer port) and test_parallel_gloo.py (parallel.ShardedStepper on the NumPy stand-in backend
against the same port, no GPU).  A plain module, not a conftest: a case is data (mesh, masks, parameter arrays, module
bits, stepper, reuse level, world, tile, steps), `materialize` builds its arrays and `run_port` runs
oracle.minimizer_port on it -- the anchor that is independent of both sharded drivers and of ms_step.

The `note` of every new case is what `run_port` measured for it on a CPU (accepted steps / failed searches / trials /
guard rejections over the case's steps); test_parallel_gloo.py::test_port_anchor_takes_its_lane asserts the lane
conditions on exactly those runs."""
from __future__ import annotations

from dataclasses import dataclass, field
from types import SimpleNamespace

import numpy as np

from membrane_solver_amd import _lib as L

S, B, PEN, ROW = L.MS_MOD_SURFACE, L.MS_MOD_BENDING, L.MS_MOD_VOLUME_PENALTY, L.MS_CON_VOLUME
GD, CG = L.MS_STEPPER_GD, L.MS_STEPPER_CG


@dataclass(frozen=True)
class ShardCase:
    id: str
    mesh: tuple  # ("sphere", freq, amplitude) | ("disk", rings, bulge, jitter, seed)
    modules: int
    stepper: int
    level: int = 2  # reuse_energy0 of the sharded run
    world: int = 2
    tile: int = 64
    n_steps: int = 9
    step0: float = 1e-3
    params: dict = field(default_factory=dict)  # stepper parameters other than the defaults (edge_fraction, ...)
    fixed: str = "every29"  # "every29" | "rim" (the boundary rows)
    nonuniform: bool = False  # kappa = 0.8+0.4U, c0 = 0.3U per vertex, gamma = 1+0.2U per facet (seed 7)
    body: str | None = None  # "upper": the volume is taken over the facets whose centroid has z > 0
    stiffness: float = 0.0  # volume_stiffness of the penalty
    v0_factor: float | None = None  # target volume = factor * V(start); None: the legacy cases' 4.0
    deterministic: bool = False
    deterministic_why: str = ""
    anchor: bool = True  # compare the single-context log with oracle.minimizer_port as well
    note: str = ""

    @property
    def constraint(self):
        return bool(self.modules & ROW)

    @property
    def penalty(self):
        return bool(self.modules & PEN)

    @property
    def bending(self):
        return bool(self.modules & B)


def legacy_case(with_volume, world, level, freq, tile):
    """The problem test_shards_match_single_context has always run: displaced closed icosphere, uniform parameters,
    every 29th row fixed, CG; the two sizes near the headline compare fixed-order sums."""
    big = freq >= 100
    return ShardCase(
        id=f"legacy-{int(with_volume)}-{world}-{level}-{freq}-{tile}", mesh=("sphere", freq, 0.06),
        modules=S | B | (ROW if with_volume else 0), stepper=CG, level=level, world=world, tile=tile,
        n_steps=6 if big else 9, step0=1e-6 if big else 1e-3, deterministic=big,
        deterministic_why="six CG steps on 512k facets amplify last-bit differences beyond the tolerances; the big "
                          "case compares fixed-order sums, the small ones run the default atomic mode",
        anchor=False)


_SPHERE = ("sphere", 16, 0.06)  # 2 562 vertices, 5 120 facets
_DISK = ("disk", 40, 0.3, 0.15, 1)  # 4 921 vertices, 9 600 facets, 240 boundary rows

# None of the new cases needs MS_DETERMINISTIC: at a few thousand vertices nine steps of the default atomic mode stay
# inside the tolerances (the legacy cases of this size run the default mode for the same reason).
NEW_CASES = [
    ShardCase("pen_gd", _SPHERE, S | PEN, GD, step0=3.0, stiffness=30.0, v0_factor=0.97,
              note="9 accepted; trials 2 1 1 2 2 2 2 2 2, guard rejections 3 2 2 0 1 0 0 0 0"),
    ShardCase("pen_cg_bend-l2", _SPHERE, S | B | PEN, CG, level=2, stiffness=30.0, v0_factor=0.97,
              note="5 accepted; trials 1 1 6 4 0 4 0 3 0, guard rejections 0 0 4 0 0 0 0 0 0 (step 3 fails after 10 "
                   "iterations, steps 5 7 9 fail on a non-descent direction)"),
    ShardCase("pen_cg_bend-l1", _SPHERE, S | B | PEN, CG, level=1, stiffness=30.0, v0_factor=0.97,
              note="as pen_cg_bend-l2 (the reuse level does not change the trajectory)"),
    ShardCase("row_gd_guard", _SPHERE, S | ROW, GD, step0=3.0, v0_factor=0.97,
              note="9 accepted; trials 1 4 3 3 2 2 2 2 2, guard rejections 0 3 0 0 0 0 0 0 0"),
    ShardCase("surf_cg", _SPHERE, S, CG, note="9 accepted, 1 trial each"),
    ShardCase("open_cg-w2-t64", _DISK, S | B, CG, world=2, tile=64, fixed="rim", nonuniform=True,
              note="3 accepted (steps 4 6 8); steps 1-3 fail after 2 3 4 trials and 8 7 6 guard rejections; steps "
                   "5 7 9 fail on a non-descent direction with 0 trials; trials 2 3 4 5 0 4 0 2 0, guards "
                   "8 7 6 5 0 2 0 0 0"),
    ShardCase("open_cg-w3-t200", _DISK, S | B, CG, world=3, tile=200, fixed="rim", nonuniform=True,
              note="as open_cg-w2-t64 (the same problem, other shards)"),
    ShardCase("open_gd_nonuniform", _DISK, S | B, GD, fixed="rim", nonuniform=True,
              note="6 accepted of 9; trials 2 3 4 5 4 2 2 3 1, guard rejections 8 7 6 5 2 0 0 0 0"),
    ShardCase("open_body_row", _SPHERE, S | ROW, CG, body="upper", v0_factor=0.97,
              note="9 accepted, 1 trial each; the row's volume is 2.1367 of the sphere's 4.3104"),
    ShardCase("edge_fraction", _SPHERE, S | B, CG, params={"edge_fraction": 0.1}, step0=1.0,
              note="5 accepted; trials 9 0 10 0 3 0 3 0 3, no guard rejection; step 1 starts at 0.378 instead of "
                   "1.0, steps 2 4 6 8 fail on a non-descent direction"),
]
BY_ID = {c.id: c for c in NEW_CASES}
OPEN_IDS = ("open_cg-w2-t64", "open_cg-w3-t200", "open_gd_nonuniform")


def TILT_BITS(L):
    """Every module bit of the tilt family: none of them is sharded."""
    return (L.MS_MOD_TILT, L.MS_MOD_BENDING_TILT, L.MS_MOD_TILT_SMOOTH, L.MS_MOD_TILT_IN, L.MS_MOD_TILT_OUT,
            L.MS_MOD_TILT_SMOOTH_IN, L.MS_MOD_TILT_SMOOTH_OUT, L.MS_MOD_BENDING_TILT_IN, L.MS_MOD_BENDING_TILT_OUT,
            L.MS_MOD_TILT_DISK_TARGET_IN, L.MS_MOD_TILT_DISK_TARGET_OUT)


def materialize(case):
    """-> namespace(P, T, fixed, boundary, body_facets, body_rows, gamma, kappa, c0, V_start, V0)"""
    from membrane_solver_amd import meshgen

    boundary = None
    if case.mesh[0] == "sphere":
        _k, freq, amp = case.mesh
        P, T = meshgen.icosphere(freq)
        P = meshgen.smooth_displace(P, amp)
    else:
        _k, rings, bulge, jitter, seed = case.mesh
        P, T, boundary = meshgen.disk_patch(rings, bulge=bulge, jitter=jitter, seed=seed)
    nv, nf = P.shape[0], T.shape[0]
    fixed = np.zeros(nv, bool)
    if case.fixed == "every29":
        fixed[::29] = True
    else:
        fixed[boundary] = True
    if case.nonuniform:
        rng = np.random.default_rng(7)
        kappa, c0, gamma = 0.8 + 0.4 * rng.random(nv), 0.3 * rng.random(nv), 1.0 + 0.2 * rng.random(nf)
    else:
        kappa, c0, gamma = np.full(nv, 0.9), np.full(nv, 0.1), np.full(nf, 1.1)
    body_facets = body_rows = None
    if case.body == "upper":
        body_facets = P[T].mean(axis=1)[:, 2] > 0.0
        body_rows = np.flatnonzero(body_facets).astype(np.int32)
    Tb = T if body_rows is None else T[body_rows]
    V = float(np.einsum("ij,ij->i", np.cross(P[Tb[:, 1]], P[Tb[:, 2]]), P[Tb[:, 0]]).sum() / 6.0)
    V0 = 4.0 if case.v0_factor is None else case.v0_factor * V
    return SimpleNamespace(P=P, T=T, fixed=fixed, boundary=boundary, body_facets=body_facets, body_rows=body_rows,
                           gamma=gamma, kappa=kappa, c0=c0, V_start=V, V0=V0)


def configure_kwargs(case, a):
    """Keyword arguments of HipShardBackend.configure / DeviceMesh.set_params for the case."""
    kw = {"target_volume": a.V0}
    if case.penalty:
        kw["volume_stiffness"] = case.stiffness
    return kw


def port_problem(case, a):
    """-> (oracle.minimizer_port.Problem, stepper) for the case: the module names and global parameters the module
    bits stand for."""
    from oracle import minimizer_port as mp

    mods = ["surface"] + (["bending"] if case.bending else []) + (["volume"] if case.penalty else [])
    gp = {"volume_constraint_mode": "penalty" if case.penalty else "lagrange",
          "volume_projection_during_minimization": False, "volume_stiffness": case.stiffness,
          "shape_step_edge_fraction": float(case.params.get("edge_fraction", 0.0))}
    p = mp.Problem(positions=a.P, tri=a.T, gamma=a.gamma, kappa=a.kappa, c0=a.c0, is_boundary=a.boundary,
                   fixed=a.fixed, energy_modules=mods, constraint_modules=["volume"] if case.constraint else [],
                   body_rows=a.body_rows, target_volume=a.V0, gp=gp)
    return p, (mp.ConjugateGradient() if case.stepper == CG else mp.GradientDescent())


def run_port(case, a=None):
    """The loop of test_parallel_gloo._worker on oracle.minimizer_port: energy_and_gradient + stepper.step, stepper
    reset on failure.  The port's line search does not report its guard rejections: they are counted where it takes
    them, as the calls of check_max_normal_change_positions that return False.
    -> namespace(log (n,3) [success, next_step, energy], trials, guards, alpha, step_in, x)"""
    from oracle import minimizer_port as mp

    a = materialize(case) if a is None else a
    p, stepper = port_problem(case, a)
    rejected = [0]
    check = mp.check_max_normal_change_positions

    def counting(tri, old, new, limit_radians=0.5):
        ok = check(tri, old, new, limit_radians)
        rejected[0] += 0 if ok else 1
        return ok

    log, trials, guards, alphas, step_in, step = [], [], [], [], [], case.step0
    mp.check_max_normal_change_positions = counting
    try:
        for _ in range(case.n_steps):
            rejected[0] = 0
            _E, g = mp.energy_and_gradient(p, p.positions)
            res = stepper.step(p, g, step)
            log.append((float(res.success), res.next_step, res.energy))
            trials.append(int(res.trials))
            guards.append(rejected[0])
            alphas.append(float(res.alpha))
            step_in.append(step)
            step = res.next_step
            if not res.success:
                stepper.reset()
    finally:
        mp.check_max_normal_change_positions = check
    return SimpleNamespace(log=np.array(log), trials=trials, guards=guards, alpha=alphas, step_in=step_in,
                           x=p.positions.copy())


def clamped_steps(success, trials, guards, alpha, step_in, beta=0.7):
    """Steps whose search provably started below the step size asked for.  Every rejected iteration (trial or guard)
    multiplies alpha by beta, so an accepted alpha is alpha_start * beta^(trials + guards - 1); a start below
    step_size is the edge_fraction clamp -- nothing else lowers it."""
    out = []
    for i in range(len(success)):
        if success[i] and trials[i] >= 1:
            start = alpha[i] / beta ** (trials[i] + guards[i] - 1)
            if start < step_in[i] * (1.0 - 1e-9):
                out.append(i)
    return out


def lane_report(case, success, trials, guards, alpha, step_in):
    """The conditions under which the case takes the lane it is in the table for, checked on a comparison run (the
    single context's or the port's).  -> list of what is missing (empty: the lane is taken)."""
    success = [bool(s) for s in success]
    n = len(success)
    missing = []
    if sum(success) < 2:
        missing.append("fewer than 2 accepted steps")
    if case.id == "row_gd_guard" and not any(g >= 1 for g in guards):
        missing.append("no step with a guard rejection")
    if case.id.startswith("open_cg"):
        if not any((not success[i]) and trials[i] > 0 for i in range(n)):
            missing.append("no failed search with trials")
        if not any((not success[i]) and trials[i] + guards[i] == 0 and success[i + 1] for i in range(n - 1)):
            missing.append("no 0-trial failure followed by an accepted step")
    if case.id == "edge_fraction" and not clamped_steps(success, trials, guards, alpha, step_in):
        missing.append("no step with a clamped alpha")
    if case.id == "pen_gd" and not any(t >= 2 for t in trials):
        missing.append("no search that backtracks")
    return missing
