"""GPU parity of the device-resident Minimizer (reference-shaped API) against
the reference's own trajectories (tests/golden/traj_*.npz) and the CPU oracle.

Trajectory tolerance: accept/reject sequence and step sizes identical; accepted
energies 1e-10 relative; final positions 1e-8 relative (SURVEY 7.3 item 5:
trajectories are compared per step, not bitwise)."""

import numpy as np
import pytest

from conftest import ROOT, load_golden, relerr

pytestmark = pytest.mark.gpu


def _build(g, mods, cons, gp, with_body):
    from membrane_solver_amd.geometry.mesh import ArrayBody, ArrayMesh

    bodies = []
    if with_body:
        bodies = [ArrayBody(0, None, float(g["target_volume"]))]
    return ArrayMesh(g["positions0"], g["tri"], fixed=g["fixed"], surface_tension=g["gamma"],
                     tilts=g["tilts0"] if "tilts0" in g else None,
                     bodies=bodies, global_parameters=gp, energy_modules=mods, constraint_modules=cons)


BASE = {"volume_constraint_mode": "lagrange", "volume_projection_during_minimization": False}
CASES = {
    "traj_cube_gd.npz": (["surface", "volume"], [], "gd",
                         {"volume_constraint_mode": "penalty", "volume_projection_during_minimization": True}),
    "traj_ico8_gd_surface_volume.npz": (["surface"], ["volume"], "gd", dict(BASE)),
    "traj_ico8_cg_surface_bending.npz": (["surface", "bending"], [], "cg", dict(BASE, bending_modulus=1.0)),
    "traj_ico8_cg_surface_bending_volume.npz": (["surface", "bending"], ["volume"], "cg",
                                                dict(BASE, bending_modulus=1.0, spontaneous_curvature=0.3)),
    "traj_disk5_gd_surface_bending_fixed.npz": (["surface", "bending"], [], "gd",
                                                dict(BASE, bending_modulus=1.0)),
    # vertex tilts: energy + shape gradient each step, tilts re-projected to the tangent
    # planes (trial energies use tilts projected on the trial surface)
    "traj_ico4_gd_surface_tilt.npz": (["surface", "tilt"], [], "gd", dict(BASE, tilt_rigidity=2.5)),
    # reference-generated: the normal-rotation guard decides trials (72 of its 73 answers reject) and searches run out
    # of their ten trials (topology.py:13-48, line_search.py:362-384, :425-426)
    "traj_ico6_cg_guard.npz": (["surface", "bending"], [], "cg", dict(BASE, bending_modulus=0.5)),
    "traj_ico6_gd_exhaust.npz": (["surface", "bending"], [], "gd", dict(BASE, bending_modulus=0.5)),
    # the Lagrange drift check fires after every accepted step (volume_tolerance 1e-11): volume.enforce_constraint
    # through ms_project_volume_cached (Body's cached-gradient first step), then project_tilts_to_tangent
    "traj_ico8_gd_volume_drift.npz": (["surface"], ["volume"], "gd", dict(BASE, volume_tolerance=1.0e-11)),
    "traj_ico4_gd_tilt_volume_drift.npz": (["surface", "tilt"], ["volume"], "gd",
                                           dict(BASE, tilt_rigidity=2.5, volume_tolerance=1.0e-11)),
    # the enforcer lane (ms_stepper_params.enforce_volume): GlobalParameters()'s own defaults -- Lagrange row and
    # volume_projection_during_minimization on -- project every line-search trial onto the target volume
    "traj_ico8_gd_volume_enforcer.npz": (["surface"], ["volume"], "gd",
                                         dict(BASE, volume_projection_during_minimization=True)),
    "traj_ico8_cg_bending_volume_enforcer.npz": (["surface", "bending"], ["volume"], "cg",
                                                 dict(BASE, bending_modulus=1.0, spontaneous_curvature=0.3,
                                                      volume_projection_during_minimization=True)),
    # ConjugateGradient(precondition=True) (ms_stepper_params.precondition): backtracking, a restart, exhausted
    # searches; with the row, non-descent directions every other step
    "traj_ico8_cg_precondition.npz": (["surface", "bending"], [], "cgp", dict(BASE, bending_modulus=1.0)),
    "traj_ico8_cg_precondition_volume.npz": (["surface", "bending"], ["volume"], "cgp",
                                             dict(BASE, bending_modulus=1.0, spontaneous_curvature=0.3)),
}
# positions against the reference: the drift cases resolve the 1 % effect of the cached-gradient first projection
# step on a 7e-7 displacement, so they are held to a tighter bound than the historical 1e-8
POS_TOL = {"traj_ico8_gd_volume_drift.npz": 2e-11, "traj_ico4_gd_tilt_volume_drift.npz": 2e-10}


@pytest.mark.parametrize("fname", sorted(CASES))
def test_minimizer_reproduces_reference_trajectory(fname):
    from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager
    from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager
    from membrane_solver_amd.runtime.minimizer import Minimizer
    from membrane_solver_amd.runtime.steppers import ConjugateGradient, GradientDescent

    mods, cons, kind, gp = CASES[fname]
    g = load_golden(fname)
    gp = dict(gp)
    if "gp_volume_stiffness" in g:
        gp["volume_stiffness"] = float(g["gp_volume_stiffness"])
        gp["surface_tension"] = float(g["gp_surface_tension"])
    mesh = _build(g, mods, cons, gp, "target_volume" in g)
    stepper = GradientDescent() if kind == "gd" else ConjugateGradient(precondition=(kind == "cgp"))
    log = []
    orig = stepper.device_step

    def logged(dm, m, step_size, tol=0.0):
        r = orig(dm, m, step_size, tol=tol)
        log.append((float(r.success), r.next_step, r.energy))
        return r

    stepper.device_step = logged
    mz = Minimizer(mesh, mesh.global_parameters, stepper, EnergyModuleManager(mods),
                   ConstraintModuleManager(cons), quiet=True, step_size=float(g["step_size0"]))
    E0, grad0 = mz.compute_energy_and_gradient_array()
    assert abs(E0 - g["E0"]) <= 1e-12 * abs(g["E0"])
    assert relerr(grad0, g["grad0"]) < 1e-10
    snaps = []
    res = mz.minimize(int(g["n_steps"]), callback=lambda m, i: snaps.append(m.positions_view().copy()))
    got, ref = np.array(log), g["step_log"]
    assert got.shape == ref.shape
    assert np.array_equal(got[:, 0], ref[:, 0]), "accept/reject sequence differs from the reference"
    assert np.allclose(got[:, 1], ref[:, 1], rtol=1e-12, atol=0)
    assert np.allclose(got[:, 2], ref[:, 2], rtol=1e-10, atol=0)
    ptol = POS_TOL.get(fname, 1e-8)
    assert relerr(np.array(snaps), g["positions_iter"]) < ptol
    assert relerr(mesh.positions_view(), g["positions_final"]) < ptol
    assert abs(res["energy"] - g["E_final"]) <= 1e-10 * abs(g["E_final"])
    assert abs(mz.step_size - g["step_size_final"]) <= 1e-12 * g["step_size_final"]
    assert res["iterations"] == int(g["iterations"])
    if "tilts_final" in g:
        assert relerr(mesh.tilts_view(), g["tilts_final"]) < 1e-9
    if "guard_rejects" in g:
        assert int(g["guard_rejects"]) > 0  # the fixture does exercise the guard in the reference


def test_config1_cube_g5_energies():
    """cube.json, g5 -> 5.98402, 5.96632, 5.94183, 5.92462, 5.92118;
    final 5.9211760891123495."""
    from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager
    from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager
    from membrane_solver_amd.runtime.minimizer import Minimizer
    from membrane_solver_amd.runtime.steppers import GradientDescent

    g = load_golden("traj_cube_gd.npz")
    gp = {"volume_constraint_mode": "penalty", "volume_projection_during_minimization": True,
          "volume_stiffness": float(g["gp_volume_stiffness"]), "surface_tension": float(g["gp_surface_tension"])}
    mesh = _build(g, ["surface", "volume"], [], gp, True)
    mz = Minimizer(mesh, mesh.global_parameters, GradientDescent(), EnergyModuleManager(["surface", "volume"]),
                   ConstraintModuleManager([]), quiet=True, step_size=1e-3)
    energies = []
    for _ in range(5):
        mz.minimize(1)
        energies.append(mz.compute_energy())
    assert np.allclose(energies, [5.98402, 5.96632, 5.94183, 5.92462, 5.92118], atol=5e-6)
    assert abs(energies[-1] - 5.9211760891123495) < 1e-10


def test_guard_and_failure_paths_match_oracle():
    """Huge initial step: the normal-rotation guard (topology.py:13-48) and the
    zero-step bookkeeping must follow the oracle's minimizer port step for step."""
    from membrane_solver_amd import meshgen
    from membrane_solver_amd.geometry.mesh import ArrayMesh
    from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager
    from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager
    from membrane_solver_amd.runtime.minimizer import Minimizer
    from membrane_solver_amd.runtime.steppers import ConjugateGradient
    from oracle import minimizer_port as mp

    P, T = meshgen.icosphere(6)
    P = meshgen.smooth_displace(P, 0.1)
    gp = {"bending_modulus": 0.5, "surface_tension": 1.0}
    p = mp.Problem(positions=P, tri=T, energy_modules=["surface", "bending"], gp=dict(gp))
    ref = mp.minimize(p, mp.ConjugateGradient(), 8, step_size=5.0)
    mesh = ArrayMesh(P, T, global_parameters=dict(gp), energy_modules=["surface", "bending"])
    stepper = ConjugateGradient()
    log = []
    orig = stepper.device_step

    def logged(dm, m, step_size, tol=0.0):
        r = orig(dm, m, step_size, tol=tol)
        log.append((float(r.success), r.next_step, r.energy, r.guard_rejects))
        return r

    stepper.device_step = logged
    mz = Minimizer(mesh, mesh.global_parameters, stepper, EnergyModuleManager(["surface", "bending"]),
                   ConstraintModuleManager([]), quiet=True, step_size=5.0)
    res = mz.minimize(8)
    got = np.array(log)
    want = np.array([[float(t["success"]), t["next_step"], t["E_accepted"]] for t in ref["trace"]])
    assert got[:, 3].sum() > 0, "the guard was expected to trigger in this case"
    assert np.array_equal(got[:, 0], want[:, 0])
    assert np.allclose(got[:, 1], want[:, 1], rtol=1e-12)
    assert np.allclose(got[:, 2], want[:, 2], rtol=1e-10)
    assert relerr(mesh.positions_view(), p.positions) < 1e-8
    assert abs(res["energy"] - ref["energy"]) <= 1e-10 * abs(ref["energy"])


def test_plugin_api_host_arrays_match_reference():
    """modules.energy.* called the way EvaluationManager calls them (accumulate into grad_arr)."""
    from membrane_solver_amd.core.parameters import ParameterResolver
    from membrane_solver_amd.geometry.mesh import ArrayBody, ArrayMesh
    from membrane_solver_amd.modules.constraints import volume as cvolume
    from membrane_solver_amd.modules.energy import bending, surface
    from membrane_solver_amd.modules.energy import volume as evolume

    g = load_golden("mesh_disk5.npz")
    gp = {"bending_modulus": 0.8, "spontaneous_curvature": 0.5, "volume_constraint_mode": "lagrange"}
    mesh = ArrayMesh(g["positions"], g["tri"], surface_tension=g["gamma"], global_parameters=gp,
                     bodies=[ArrayBody(0, None, float(g["volpen_target"]))])
    pr = ParameterResolver(mesh.global_parameters)
    pos, im = mesh.positions_view(), mesh.vertex_index_to_row
    grad = np.ones_like(pos)  # accumulate semantics: pre-filled array
    Es = surface.compute_energy_and_gradient_array(mesh, mesh.global_parameters, pr, positions=pos,
                                                   index_map=im, grad_arr=grad)
    Eb = bending.compute_energy_and_gradient_array(mesh, mesh.global_parameters, pr, positions=pos,
                                                   index_map=im, grad_arr=grad)
    assert abs(Es - g["E_surface"]) <= 1e-12 * abs(g["E_surface"])
    assert abs(Eb - g["E_bend_helfrich_c5_analytic"]) <= 1e-12 * abs(g["E_bend_helfrich_c5_analytic"])
    assert relerr(grad - 1.0, g["grad_surface"] + g["grad_bend_helfrich_c5_analytic"]) < 1e-10
    assert abs(bending.compute_energy_array(mesh, mesh.global_parameters, pos, im)
               - float(np.sum(g["Earr_bend_helfrich_c5"]))) <= 1e-12 * abs(Eb)
    gC = cvolume.constraint_gradients_array(mesh, mesh.global_parameters, positions=pos, index_map=im)
    assert relerr(gC[0], g["grad_volume"]) < 1e-10
    mesh.global_parameters.set("volume_constraint_mode", "penalty")
    mesh.global_parameters.set("volume_stiffness", float(g["volpen_k"]))
    gv = np.zeros_like(pos)
    Ev = evolume.compute_energy_and_gradient_array(mesh, mesh.global_parameters, pr, positions=pos,
                                                   index_map=im, grad_arr=gv)
    assert abs(Ev - g["E_volpen"]) <= 1e-12 * abs(g["E_volpen"])
    assert relerr(gv, g["grad_volpen"]) < 1e-10
    # tilt module (modules/energy/tilt.py): shape gradient accumulated, tilt gradient optional
    from membrane_solver_amd.modules.energy import tilt as etilt

    mesh.global_parameters.set("tilt_rigidity", float(g["k_tilt"]))
    mesh.set_tilts_from_array(g["tilts"])
    gs, gt = np.full_like(pos, 2.0), np.full_like(pos, -1.0)
    Et = etilt.compute_energy_and_gradient_array(mesh, mesh.global_parameters, pr, positions=pos, index_map=im,
                                                 grad_arr=gs, tilt_grad_arr=gt)
    assert abs(Et - g["E_tilt"]) <= 1e-12 * abs(g["E_tilt"])
    assert relerr(gs - 2.0, g["grad_tilt_shape"]) < 1e-10
    assert relerr(gt + 1.0, g["grad_tilt_tilt"]) < 1e-10
    assert abs(etilt.compute_energy_array(mesh, mesh.global_parameters, pr, positions=pos, index_map=im)
               - g["E_tilt"]) <= 1e-12 * abs(g["E_tilt"])
    # a foreign positions array (not the mesh's cache) is honoured
    pos2 = pos * 1.01
    g2 = np.zeros_like(pos)
    E2 = surface.compute_energy_and_gradient_array(mesh, mesh.global_parameters, pr, positions=pos2,
                                                   index_map=im, grad_arr=g2)
    assert abs(E2 - 1.0201 * g["E_surface"]) <= 1e-11 * abs(g["E_surface"])


@pytest.mark.parametrize("freq,kind", [(81, "gd"), (320, "cg")])
def test_full_size_properties(freq, kind):
    """BASELINE sizes (configs 2 and 3; nf = 131 220 / 2 048 000): size-independent
    properties instead of an oracle run.
    - patch-order round trip of positions is bit exact;
    - fixed rows of the gradient are exactly zero;
    - KKT: the volume-projected gradient is orthogonal to dV/dx;
    - translation invariance of E and grad; closed-surface gradient rows sum to 0;
    - linearity: doubling gamma doubles E_surface and its gradient;
    - accepted steps satisfy Armijo decrease and the alpha_max growth cap."""
    from membrane_solver_amd import _lib as L
    from membrane_solver_amd import meshgen
    from membrane_solver_amd.device import DeviceMesh

    P, T = meshgen.icosphere(freq)
    P = meshgen.smooth_displace(P, 0.05)
    nv, nf = P.shape[0], T.shape[0]
    assert nf == 20 * freq * freq
    mods = L.MS_MOD_SURFACE | (L.MS_MOD_BENDING if kind == "cg" else 0)
    dm = DeviceMesh(P, T)
    assert np.array_equal(dm.get_positions(), P)
    dm.set_surface_tension(np.ones(nf))
    dm.set_bending_params(np.ones(nv), np.full(nv, 0.2))
    # KKT orthogonality
    dm.set_params(modules=mods | L.MS_CON_VOLUME, target_volume=4.0)
    e1, g1 = dm.energy_and_gradient()
    gC = dm.get_vertex_buffer(L.MS_BUF_GC)
    assert abs(np.sum(g1 * gC)) <= 1e-10 * np.linalg.norm(g1) * np.linalg.norm(gC)
    # unprojected gradient, translation invariance, zero row-sum of the surface part
    dm.set_params(modules=mods)
    e0, g0 = dm.energy_and_gradient()
    assert abs(e0.sum() - e1.sum()) <= 1e-13 * abs(e0.sum())
    lam = np.sum(g0 * gC) / np.sum(gC * gC)
    # Two evaluations of the bending gradient agree to ~1e-16 * (1/h^2): the back-prop
    # differences fK_i - fK_j of neighbouring vertices amplify last-bit noise of H by
    # 1/(h * |grad H|), so at nf = 2 048 000 (h ~ 3e-3) any two summation orders -- the
    # reference's own Fortran vs NumPy paths included -- differ at the 1e-9 level.
    assert relerr(g1, g0 - lam * gC) < (1e-10 if freq <= 81 else 5e-8)
    dm.set_positions(P + np.array([0.3, -0.2, 0.1]))
    e2, g2 = dm.energy_and_gradient()
    assert abs(e2.sum() - e0.sum()) <= 1e-11 * abs(e0.sum())
    # (how far the gradient may move under the translation is MEASURED against the oracle's own sensitivity in
    # test_full_size_energy_and_gradient_match_oracle; here only a gross bound)
    assert relerr(g2, g0) < 1e-5
    dm.set_positions(P)
    dm.set_params(modules=L.MS_MOD_SURFACE)
    es, gs = dm.energy_and_gradient()
    assert np.max(np.abs(gs.sum(axis=0))) < 1e-12
    dm.set_surface_tension(np.full(nf, 2.0))
    es2, gs2 = dm.energy_and_gradient()
    assert abs(es2[0] - 2.0 * es[0]) <= 1e-14 * es2[0]
    assert relerr(gs2, 2.0 * gs) < 1e-13
    dm.close()
    # fixed rows + a few real steps
    fixed = np.zeros(nv, dtype=bool)
    fixed[:: max(1, nv // 97)] = True
    dm = DeviceMesh(P, T, fixed=fixed)
    dm.set_surface_tension(np.ones(nf))
    dm.set_bending_params(np.ones(nv), np.zeros(nv))
    dm.set_params(modules=mods)
    _, g = dm.energy_and_gradient()
    assert np.all(g[fixed] == 0.0) and np.any(g[~fixed] != 0.0)
    step, e_prev = 1e-6, dm.energy().sum()
    stepper = L.MS_STEPPER_CG if kind == "cg" else L.MS_STEPPER_GD
    accepted = 0
    for _ in range(8):
        r = dm.step(stepper=stepper, step_size=step)
        if r.success:
            accepted += 1
            assert r.energy <= e_prev + 1e-4 * r.alpha * r.g_dot_d + 1e-15
            assert r.next_step <= 10.0 * step * (1 + 1e-15)
            e_prev = r.energy
        else:
            dm.reset_stepper()
        step = r.next_step
    assert accepted >= 1
    x = dm.get_positions()
    assert np.array_equal(x[fixed], P[fixed])
    dm.close()


@pytest.mark.parametrize("freq", [81, 320])
def test_full_size_rotation_and_scaling_laws(freq):
    """Size-independent laws at BASELINE sizes (131 220 / 2 048 000 facets), none of which the kernels know about:
    - a rigid rotation leaves every energy unchanged and rotates the gradient;
    - scaling the surface by s: E_surface ~ s^2 (gradient ~ s), the Willmore energy (c0 = 0) does not change
      (gradient ~ 1/s), the enclosed volume ~ s^3 (read through the penalty energy k/2 (V - V0)^2 with V0 = 0, k = 2).
    The gradient bounds are gross (the bending back-propagation amplifies rounding by ~1/h^2: measured against the
    oracle in test_full_size_energy_and_gradient_match_oracle); the energies are held to 1e-11."""
    from membrane_solver_amd import _lib as L
    from membrane_solver_amd import meshgen
    from membrane_solver_amd.device import DeviceMesh

    P, T = meshgen.icosphere(freq)
    P = meshgen.smooth_displace(P, 0.05)
    nv, nf = P.shape[0], T.shape[0]
    dm = DeviceMesh(P, T)
    dm.set_surface_tension(np.ones(nf))
    dm.set_bending_params(np.ones(nv), np.zeros(nv))
    both = L.MS_MOD_SURFACE | L.MS_MOD_BENDING
    # (rotating / scaling the INPUT rounds every coordinate anew: 1e-16 in x is ~1e-16 / h^2 in the curvature and more
    # in its differences -- 3e-8 of max|g| at 131 220 facets)
    gtol = 1e-6 if freq <= 81 else 1e-4

    def evaluate(X, modules, **kw):
        dm.set_positions(X)
        dm.set_params(modules=modules, **kw)
        return dm.energy_and_gradient()

    e0, g0 = evaluate(P, both)
    es0, gs0 = evaluate(P, L.MS_MOD_SURFACE)
    ev0, _ = evaluate(P, L.MS_MOD_VOLUME_PENALTY, volume_stiffness=2.0, target_volume=0.0)
    V0 = np.sqrt(ev0.sum())
    assert abs(V0 - 4.0 * np.pi / 3.0) < 0.3  # (a displaced unit sphere)
    # rotation (a proper one, from a QR factorisation)
    Q, _r = np.linalg.qr(np.random.default_rng(5).normal(size=(3, 3)))
    if np.linalg.det(Q) < 0:
        Q[:, 0] = -Q[:, 0]
    e1, g1 = evaluate(P @ Q.T, both)
    assert np.allclose(e1, e0, rtol=1e-11, atol=0)
    assert relerr(g1, g0 @ Q.T) < gtol
    # scaling
    s = 1.7
    e2, g2 = evaluate(s * P, both)
    es2, gs2 = evaluate(s * P, L.MS_MOD_SURFACE)
    assert abs(es2[0] - s * s * es0[0]) <= 1e-12 * es2[0]
    assert relerr(gs2, s * gs0) < 1e-10  # (per-vertex sums of facet terms that cancel to ~h of their size)
    assert abs(e2[0] - s * s * e0[0]) <= 1e-12 * e2[0]
    assert abs(e2[1] - e0[1]) <= 1e-11 * e0[1]  # Willmore: scale-invariant
    gb0, gb2 = g0 - gs0, g2 - gs2
    assert relerr(gb2, gb0 / s) < gtol
    ev2, _ = evaluate(s * P, L.MS_MOD_VOLUME_PENALTY, volume_stiffness=2.0, target_volume=0.0)
    assert abs(np.sqrt(ev2.sum()) - s ** 3 * V0) <= 1e-12 * s ** 3 * V0
    dm.close()


@pytest.mark.parametrize("fname", sorted(CASES))
def test_evaluation_reuse_levels_are_bitwise_identical(fname, deterministic):
    """ms_stepper_params.reuse_energy0 = 0 (re-evaluate everything the reference re-evaluates),
    1 (reuse energy0) and 2 (an accepted trial is the next step's energy/factor pass) must give
    the SAME doubles: the skipped passes are the same kernel on the same inputs."""
    from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager
    from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager
    from membrane_solver_amd.runtime.minimizer import Minimizer
    from membrane_solver_amd.runtime.steppers import ConjugateGradient, GradientDescent

    mods, cons, kind, gp = CASES[fname]
    g = load_golden(fname)
    gp = dict(gp)
    if "gp_volume_stiffness" in g:
        gp["volume_stiffness"] = float(g["gp_volume_stiffness"])
        gp["surface_tension"] = float(g["gp_surface_tension"])
    runs = []
    for level in (0, 1, 2):
        mesh = _build(g, mods, cons, gp, "target_volume" in g)
        stepper = GradientDescent() if kind == "gd" else ConjugateGradient()
        stepper.reuse_energy0 = level
        log = []
        orig = stepper.device_step

        def logged(dm, m, step_size, tol=0.0, _orig=orig, _log=log):
            r = _orig(dm, m, step_size, tol=tol)
            _log.append((float(r.success), r.next_step, r.energy, r.energy_eval, r.grad_norm,
                         r.g_dot_d, r.alpha, r.volume))
            return r

        stepper.device_step = logged
        mz = Minimizer(mesh, mesh.global_parameters, stepper, EnergyModuleManager(mods),
                       ConstraintModuleManager(cons), quiet=True, step_size=float(g["step_size0"]))
        mz.minimize(int(g["n_steps"]) + 7)
        runs.append((np.array(log), mesh.positions_view().copy()))
    for log, pos in runs[1:]:
        assert np.array_equal(log, runs[0][0])
        assert np.array_equal(pos, runs[0][1])


def test_reuse_levels_bitwise_identical_multitile_with_rejections(deterministic):
    """Same, straight on DeviceMesh.step for a multi-tile noisy sphere with an over-long first
    step (forces backtracking / failed searches, i.e. the carried state must be invalidated)."""
    from membrane_solver_amd import _lib as L
    from membrane_solver_amd import meshgen
    from membrane_solver_amd.device import DeviceMesh

    pos, tri = meshgen.icosphere(24)
    pos = meshgen.smooth_displace(pos, 0.05)
    pos = pos + 2.0e-3 * np.random.default_rng(3).standard_normal(pos.shape)
    nv = pos.shape[0]
    outs = []
    for level in (0, 1, 2):
        dm = DeviceMesh(pos, tri)
        dm.set_surface_tension(np.full(tri.shape[0], 1.0))
        dm.set_bending_params(np.full(nv, 1.0), np.full(nv, 0.2))
        dm.set_params(modules=L.MS_MOD_SURFACE | L.MS_MOD_BENDING)
        step, rows = 5.0e-2, []
        for _ in range(25):
            r = dm.step(stepper=L.MS_STEPPER_CG, step_size=step, reuse_energy0=level)
            rows.append((r.success, r.trials, r.energy, r.energy_eval, r.grad_norm, r.g_dot_d, r.alpha))
            step = r.next_step
            if not r.success:
                dm.reset_stepper()
        outs.append((np.array(rows, dtype=np.float64), dm.get_positions()))
        dm.close()
    assert outs[0][0][:, 1].max() > 1, "the case is meant to exercise backtracking"
    assert (outs[0][0][:, 0] == 0).any(), "the case is meant to exercise failed searches"
    for rows, x in outs[1:]:
        assert np.array_equal(outs[0][0], rows)
        assert np.array_equal(outs[0][1], x)


@pytest.mark.parametrize("fname", ["traj_ico8_cg_surface_bending_volume.npz", "traj_cube_gd.npz",
                                   "traj_ico8_gd_volume_drift.npz", "traj_ico4_gd_tilt_volume_drift.npz",
                                   "traj_ico6_cg_guard.npz", "traj_ico8_cg_precondition.npz",
                                   "traj_ico8_cg_precondition_volume.npz",
                                   "traj_ico4_gd_surface_tilt.npz"])
def test_library_loop_equals_python_loop(fname, deterministic):
    """Minimizer.minimize runs the loop inside the library (ms_minimize) when nobody watches the
    individual steps; wrapping stepper.device_step (as the parity tests do) selects the Python
    loop.  Both must leave bit-identical state."""
    from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager
    from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager
    from membrane_solver_amd.runtime.minimizer import Minimizer
    from membrane_solver_amd.runtime.steppers import ConjugateGradient, GradientDescent

    mods, cons, kind, gp = CASES[fname]
    g = load_golden(fname)
    gp = dict(gp, volume_tolerance=1e-9)  # make the Lagrange drift check fire
    if "gp_volume_stiffness" in g:
        gp["volume_stiffness"] = float(g["gp_volume_stiffness"])
        gp["surface_tension"] = float(g["gp_surface_tension"])
    outs = []
    for watched in (False, True):
        mesh = _build(g, mods, cons, gp, "target_volume" in g)
        stepper = GradientDescent() if kind == "gd" else ConjugateGradient(precondition=(kind == "cgp"))
        if watched:
            orig = stepper.device_step
            stepper.device_step = lambda dm, m, step_size, tol=0.0, _o=orig: _o(dm, m, step_size, tol=tol)
        mz = Minimizer(mesh, mesh.global_parameters, stepper, EnergyModuleManager(mods),
                       ConstraintModuleManager(cons), quiet=True, step_size=float(g["step_size0"]))
        assert mz._fast_path_ok(None) == (not watched)
        res = mz.minimize(int(g["n_steps"]) + 5)
        res2 = mz.minimize(3)
        outs.append((mesh.positions_view().copy(), mz.step_size, res["energy"], res2["energy"], res["iterations"],
                     res["step_success"], mesh.tilts_view().copy()))
    a, b = outs
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[6], b[6])
    assert a[1:6] == b[1:6]


def test_topology_change_rebuilds_the_device_mirror(deterministic):
    """SURVEY 8(f)-3, the refinement re-upload hook: after the mesh's topology counters change the
    next call re-tiles and re-uploads; the run continues exactly like a fresh Minimizer on the new mesh."""
    from membrane_solver_amd import meshgen
    from membrane_solver_amd.geometry.mesh import ArrayMesh
    from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager
    from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager
    from membrane_solver_amd.runtime.minimizer import Minimizer
    from membrane_solver_amd.runtime.steppers import ConjugateGradient

    gp = {"surface_tension": 1.0, "bending_modulus": 0.8, "spontaneous_curvature": 0.1,
          "volume_constraint_mode": "lagrange", "volume_projection_during_minimization": False}
    mods = ["surface", "bending"]
    P4, T4 = meshgen.icosphere(4)
    P4 = meshgen.smooth_displace(P4, 0.06)
    P9, T9 = meshgen.icosphere(9)
    P9 = meshgen.smooth_displace(P9, 0.06)

    def make(P, T):
        mesh = ArrayMesh(P, T, global_parameters=dict(gp), energy_modules=mods, constraint_modules=[])
        return mesh, Minimizer(mesh, mesh.global_parameters, ConjugateGradient(), EnergyModuleManager(mods),
                               ConstraintModuleManager([]), quiet=True, step_size=1e-3)

    mesh, mz = make(P4, T4)
    mz.minimize(4)
    first_dm = mesh._hip_mirror.dm
    mesh.replace_topology(P9, T9)       # "refine"
    mz.stepper.reset()
    mz.step_size = 1e-3
    res = mz.minimize(5)
    assert mesh._hip_mirror.dm is not first_dm and mesh._hip_mirror.dm.nv == P9.shape[0]
    mesh_b, mz_b = make(P9, T9)
    res_b = mz_b.minimize(5)
    assert np.array_equal(mesh.positions_view(), mesh_b.positions_view())
    assert res["energy"] == res_b["energy"] and mz.step_size == mz_b.step_size


@pytest.mark.parametrize("mode,lean", [("1", "1"), ("2", "1"), ("3", "1"), ("4", "1"), ("2", "0"), ("4", "0")])
def test_pair_launch_does_not_change_the_trajectory(mode, lean, monkeypatch):
    """Two trial evaluations in one launch (k_energy<PAIR>, ms_step): MS_PAIR=1 lets the line-search history decide,
    MS_PAIR=2 pairs whenever it can (so trial 0 is accepted inside a pair now and then: the re-evaluation path, or with
    MS_PAIR_LEAN=0 the copy-back path), MS_PAIR=3 also queues a gated third trial behind every pair, MS_PAIR=4 evaluates
    three trials per launch whenever it can -- all must give the doubles of the one-trial-per-launch search, bit for
    bit with fixed-order sums.  `lean`: the early trials of a launch are evaluated for their energies only (default)
    or write their positions and factors into side sets."""
    from membrane_solver_amd import _lib as L
    from membrane_solver_amd import meshgen
    from membrane_solver_amd.device import DeviceMesh

    pos, tri = meshgen.icosphere(24)
    pos = meshgen.smooth_displace(pos, 0.05)
    pos = pos + 2.0e-3 * np.random.default_rng(3).standard_normal(pos.shape)
    nv = pos.shape[0]

    def run(pair, speculate="1"):
        monkeypatch.setenv("MS_PAIR", pair)
        monkeypatch.setenv("MS_SPECULATE", speculate)
        monkeypatch.setenv("MS_PAIR_LEAN", lean)
        dm = DeviceMesh(pos, tri)
        dm.set_deterministic(True)
        dm.set_surface_tension(np.full(tri.shape[0], 1.0))
        dm.set_bending_params(np.full(nv, 1.0), np.full(nv, 0.2))
        dm.set_params(modules=L.MS_MOD_SURFACE | L.MS_MOD_BENDING)
        dm.profile_enable(True)
        step, rows = 5.0e-2, []
        for _ in range(70):
            r = dm.step(stepper=L.MS_STEPPER_CG, step_size=step, reuse_energy0=2)
            rows.append((r.success, r.trials, r.energy, r.energy_eval, r.grad_norm, r.g_dot_d, r.alpha))
            step = r.next_step
            if not r.success:
                dm.reset_stepper()
        prof = dm.profile_read()
        x = dm.get_positions()
        dm.close()
        return np.array(rows, dtype=np.float64), x, prof

    ref_rows, ref_x, ref_prof = run("0", "0")
    assert ref_prof.get("energy_pair", (0.0, 0))[1] == 0
    rows, x, prof = run(mode)
    assert prof["energy_triple" if mode == "4" else "energy_pair"][1] > 0, "the case is meant to exercise the pair launch"
    assert np.array_equal(rows, ref_rows)
    assert np.array_equal(x, ref_x)
    acc = ref_rows[ref_rows[:, 0] == 1]
    assert (acc[:, 1] == 1).any() and (acc[:, 1] == 2).any() and (acc[:, 1] >= 3).any(), \
        "needs acceptances at the first, second and a later trial"


def test_project_volume_matches_oracle_including_the_cached_gradient_step():
    """modules/constraints/volume.py:69-149 through ms_project_volume / ms_project_volume_cached against the oracle
    port's restatement (itself pinned to 1e-15 by the reference's drift trajectories): a fresh projection, then --
    after moving the surface -- one whose first step uses the gradient cached by the first (geometry/body.py:386-407)."""
    from membrane_solver_amd import _lib as L
    from membrane_solver_amd import meshgen
    from membrane_solver_amd.device import DeviceMesh
    from oracle import minimizer_port as mp
    from oracle import ms_oracle as orc

    P, T = meshgen.icosphere(8)
    P = meshgen.smooth_displace(P, 0.05)
    V0 = float(orc.volume(P, T, None))
    target = V0 * 1.0005
    p = mp.Problem(positions=P, tri=T, energy_modules=["surface"], constraint_modules=["volume"],
                   target_volume=target, gp={"surface_tension": 1.0})
    dm = DeviceMesh(P, T, tile_vertices=64)
    dm.set_params(modules=L.MS_MOD_SURFACE | L.MS_CON_VOLUME, target_volume=target)
    it, v = dm.project_volume(target, tol=1e-12, max_iter=12)
    x1 = mp.project_volume(p, P.copy(), tol=1e-12, max_iter=12)
    assert it >= 2 and abs(v - target) < 1e-12
    assert relerr(dm.get_positions(), x1) < 1e-13
    # move the surface, then project with the first step along the CACHED gradient
    x2 = x1 * (1.0 + 5e-3 * np.sin(3.0 * x1[:, [0]]))
    dm.set_positions(x2)
    it, v = dm.project_volume(target, tol=1e-12, max_iter=12, first_step_cached=True)
    x3 = mp.project_volume(p, x2.copy(), tol=1e-12, max_iter=12, first_cached=True)
    x3_fresh = mp.project_volume(mp.Problem(positions=P, tri=T, energy_modules=["surface"],
                                            constraint_modules=["volume"], target_volume=target,
                                            gp={"surface_tension": 1.0}), x2.copy(), tol=1e-12, max_iter=12)
    assert relerr(dm.get_positions(), x3) < 1e-13
    assert relerr(x3, x3_fresh) > 1e-9, "the cached first step must be distinguishable from a fresh one here"
    dm.close()


@pytest.mark.parametrize("freq", [81, 320])
def test_full_size_energy_and_gradient_match_oracle(freq):
    """BASELINE configs 2 and 3 at their FULL sizes (131 220 and 2 048 000 facets) against the CPU oracle
    (libms_oracle.so, ~2 s of CPU at f = 320): energies to 1e-12; the gradient in max-norm against a tolerance that is
    MEASURED here, not asserted from an argument: the same oracle source built with another summation order
    (libms_oracle_omp.so: facet loops split over threads, vertex sums by atomics) differs from the serial build by
    `noise`; the HIP gradient has to stay within 5 x that (and never worse than 2e-8; measured on MI355X: 1.05e-10
    against a noise of 8.6e-11 at f = 81, 3.6e-9 against 2.1e-9 at f = 320).  The bending back-propagation
    differences fK_i - fK_j of neighbouring vertices amplify last-bit noise of H by ~1/h^2, which is what `noise`
    shows growing with the mesh."""
    import json
    import os

    from membrane_solver_amd import _lib as L
    from membrane_solver_amd import meshgen
    from membrane_solver_amd.device import DeviceMesh
    from oracle import ms_oracle as orc

    P, T = meshgen.icosphere(freq)
    P = meshgen.smooth_displace(P, 0.05)
    nv, nf = len(P), len(T)
    assert nf == 20 * freq * freq
    kappa, c0 = np.ones(nv), np.full(nv, 0.2)
    dm = DeviceMesh(P, T)
    dm.set_surface_tension(np.ones(nf))
    dm.set_bending_params(kappa, c0)
    dm.set_params(modules=L.MS_MOD_SURFACE | L.MS_MOD_BENDING)
    e, g = dm.energy_and_gradient(raw=True)
    shift = np.array([0.3, -0.2, 0.1])
    dm.set_positions(P + shift)
    e_t, g_t = dm.energy_and_gradient(raw=True)
    dm.set_positions(P)
    dm.set_params(modules=L.MS_MOD_SURFACE)
    _es, g_surf = dm.energy_and_gradient(raw=True)
    dm.close()

    def oracle(omp, X=P):
        orc.use_openmp(omp)
        try:
            gs = np.zeros_like(X)
            Es = orc.surface_energy_and_gradient(X, T, np.ones(nf), gs)
            gb = np.zeros_like(X)
            Eb = orc.bending_energy_and_gradient(X, T, kappa, c0, np.zeros(nv, bool), grad=gb)
        finally:
            orc.use_openmp(False)
        return Es, Eb, gs, gb

    Es, Eb, gs, gb = oracle(False)
    _Es2, _Eb2, gs2, gb2 = oracle(True)
    _Es3, _Eb3, gs3, gb3 = oracle(False, P + shift)
    noise = relerr(gs2 + gb2, gs + gb)
    err = relerr(g, gs + gb)
    err_surf = relerr(g_surf, gs)
    # translation invariance, measured on both sides: the oracle's own gradient moves by `oracle_shift` when every
    # coordinate is re-rounded at the shifted origin; the HIP gradient may move by a small multiple of that
    oracle_shift = relerr(gs3 + gb3, gs + gb)
    hip_shift = relerr(g_t, g)
    tol = max(2e-10, 5.0 * noise)
    # Which of the two is closer to the exact gradient?  The same oracle source in x87 extended precision (every
    # double a long double: 2^-11 of fp64's rounding unit, oracle/truth.py) is the reference for both.
    from oracle import truth

    E_ld, g_ld = truth.surface_bending_energy_and_gradient(P, T, np.ones(nf), kappa, c0, np.zeros(nv, bool))
    g_true = g_ld.astype(np.float64)
    gmax = np.max(np.abs(g_true))
    hip_vs_truth = float(np.max(np.abs(g - g_true)) / gmax)
    oracle_vs_truth = float(np.max(np.abs((gs + gb) - g_true)) / gmax)
    omp_vs_truth = float(np.max(np.abs((gs2 + gb2) - g_true)) / gmax)
    report_truth = {"hip_grad_error": hip_vs_truth, "fp64_oracle_grad_error": oracle_vs_truth,
                    "fp64_oracle_omp_grad_error": omp_vs_truth,
                    "hip_energy_error": float(abs(np.longdouble(e[0] + e[1]) - E_ld) / abs(E_ld)),
                    "fp64_oracle_energy_error": float(abs(np.longdouble(Es + Eb) - E_ld) / abs(E_ld))}
    report = {"freq": freq, "nf": nf, "E_surface_rel": abs(e[0] - Es) / Es, "E_bending_rel": abs(e[1] - Eb) / Eb,
              "grad_rel_maxnorm": err, "surface_grad_rel_maxnorm": err_surf,
              "oracle_summation_order_noise": noise, "tolerance_used": tol,
              "against_extended_precision": report_truth,
              "translation": {"hip_grad_change": hip_shift, "oracle_grad_change": oracle_shift,
                              "hip_energy_change": abs(e_t.sum() - e.sum()) / abs(e.sum())}}
    out_dir = os.path.join(ROOT, "gpurun_out")
    if os.path.isdir(out_dir):
        with open(os.path.join(out_dir, f"fullsize_parity_f{freq}.json"), "w") as fh:
            json.dump(report, fh, indent=1)
    assert abs(e[0] - Es) <= 1e-12 * Es, report
    assert abs(e[1] - Eb) <= 1e-12 * Eb, report
    assert err_surf < 1e-12, report                      # no cancellation in the surface term
    assert err < tol and err < 2e-8, report
    # against the extended-precision gradient the HIP path may be at most twice as far off as the fp64 oracle itself
    # (the worse of its two summation orders), and never further than the 1e-10 bar allows at the sizes where fp64
    # arithmetic can meet it at all
    assert hip_vs_truth <= 2.0 * max(oracle_vs_truth, omp_vs_truth), report
    assert hip_vs_truth < max(1e-10, 2.0 * max(oracle_vs_truth, omp_vs_truth)), report
    assert hip_shift < max(1e-9, 5.0 * oracle_shift), report
    assert abs(e_t.sum() - e.sum()) <= 1e-11 * abs(e.sum()), report


@pytest.mark.parametrize("freq,kind,n_steps", [(81, "gd", 10), (320, "cg", 5)])
def test_full_size_trajectory_matches_oracle_port(freq, kind, n_steps):
    """BASELINE configs 2 and 3 at their full sizes, as trajectories: icosphere f = 81 (131 220 facets), surface +
    Lagrange volume constraint, gradient descent; f = 320 (2 048 000 facets), surface + Helfrich bending, CG.  The
    oracle's minimizer port (C energy / gradient kernels under the restated control flow, itself pinned by the
    reference's trajectories at small sizes) runs the same steps on the CPU: same accept / reject sequence, same
    trial counts, same step sizes, energies to 1e-10.  Default (LDS-atomic) vertex sums, default line-search queue."""
    from membrane_solver_amd import meshgen
    from membrane_solver_amd.geometry.mesh import ArrayMesh
    from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager
    from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager
    from membrane_solver_amd.runtime.minimizer import Minimizer
    from membrane_solver_amd.runtime.steppers import ConjugateGradient, GradientDescent
    from oracle import minimizer_port as mp
    from oracle import ms_oracle as orc

    orc.use_openmp(True)  # (the checker may use the host's cores; the serial build gives the same trajectory)
    P, T = meshgen.icosphere(freq)
    P = meshgen.smooth_displace(P, 0.05)
    if kind == "gd":
        mods, cons = ["surface"], ["volume"]
        gp = {"surface_tension": 1.0, "volume_constraint_mode": "lagrange",
              "volume_projection_during_minimization": False}
        V0 = 0.97 * orc.volume(P, T, None)
    else:
        mods, cons = ["surface", "bending"], []
        gp = {"surface_tension": 1.0, "bending_modulus": 1.0}
        V0 = None
    # step sizes that make the searches backtrack (and, for config 2, run into the normal-rotation guard)
    step0 = 3.0 if kind == "gd" else 4e-6
    p = mp.Problem(positions=P, tri=T, energy_modules=list(mods), constraint_modules=list(cons), gp=dict(gp),
                   target_volume=V0)
    ref = mp.minimize(p, mp.GradientDescent() if kind == "gd" else mp.ConjugateGradient(), n_steps, step_size=step0)
    orc.use_openmp(False)
    from membrane_solver_amd.geometry.mesh import ArrayBody

    bodies = [ArrayBody(0, None, float(V0))] if V0 is not None else []
    mesh = ArrayMesh(P, T, bodies=bodies, global_parameters=dict(gp), energy_modules=list(mods),
                     constraint_modules=list(cons))
    stepper = GradientDescent() if kind == "gd" else ConjugateGradient()
    log = []
    orig = stepper.device_step

    def logged(dm, m, step_size, tol=0.0):
        r = orig(dm, m, step_size, tol=tol)
        log.append((float(r.success), r.next_step, r.energy, r.trials))
        return r

    stepper.device_step = logged
    mz = Minimizer(mesh, mesh.global_parameters, stepper, EnergyModuleManager(mods), ConstraintModuleManager(cons),
                   quiet=True, step_size=step0)
    res = mz.minimize(n_steps)
    got = np.array(log)
    want = np.array([[float(t["success"]), t["next_step"], t["E_accepted"], t["trials"]] for t in ref["trace"]])
    assert got.shape == want.shape
    assert want[:, 0].sum() >= 2 and want[:, 3].max() >= 2, "the case is expected to accept steps after backtracking"
    assert np.array_equal(got[:, 0], want[:, 0]), (got, want)
    assert np.array_equal(got[:, 3], want[:, 3]), (got, want)
    assert np.allclose(got[:, 1], want[:, 1], rtol=1e-12)
    assert np.allclose(got[:, 2], want[:, 2], rtol=1e-10)
    assert abs(res["energy"] - ref["energy"]) <= 1e-10 * abs(ref["energy"])
    # positions: the displacement of the run, not the positions themselves, is what the steps produced
    moved = np.linalg.norm(p.positions - P)
    assert moved > 0.0
    assert np.linalg.norm(mesh.positions_view() - p.positions) <= (1e-8 if kind == "gd" else 1e-5) * moved


def test_default_mode_ladder_at_full_size(monkeypatch):
    """The speculative line-search ladder (queued trials, pair / triple launches, gated gradient pass) where it is
    actually used: the headline workload at FULL size (2 048 000 facets) in the DEFAULT LDS-atomic mode.  Against the
    plain one-trial-per-launch search (MS_PAIR=0, MS_SPECULATE=0) the accept/reject sequence, the trial counts and the
    step sizes must be equal and the energies agree to 1e-10 (atomic sums are not bitwise repeatable)."""
    from membrane_solver_amd import _lib as L
    from membrane_solver_amd import meshgen
    from membrane_solver_amd.device import DeviceMesh

    P, T = meshgen.icosphere(320)
    P = meshgen.smooth_displace(P, 0.05)
    nv, nf = len(P), len(T)
    logs = []
    for env in ({"MS_PAIR": "0", "MS_SPECULATE": "0"}, {}):
        for k in ("MS_PAIR", "MS_SPECULATE"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        dm = DeviceMesh(P, T)
        dm.set_surface_tension(np.ones(nf))
        dm.set_bending_params(np.ones(nv), np.zeros(nv))
        dm.set_params(modules=L.MS_MOD_SURFACE | L.MS_MOD_BENDING)
        step, rows = 1e-6, []
        for _ in range(40):
            r = dm.step(stepper=L.MS_STEPPER_CG, step_size=step, reuse_energy0=2)  # (level 2: the queue's precondition)
            rows.append((float(r.success), float(r.trials), r.next_step, r.energy, r.alpha))
            step = r.next_step
            if not r.success:
                dm.reset_stepper()
        logs.append(np.array(rows))
        dm.close()
    plain, ladder = logs
    assert plain[:, 0].sum() >= 15 and plain[:, 1].max() >= 2, "the run is meant to exercise multi-trial searches"
    assert np.array_equal(plain[:, 0], ladder[:, 0]), "accept/reject sequence differs"
    assert np.array_equal(plain[:, 1], ladder[:, 1]), "trial counts differ"
    assert np.allclose(plain[:, 2], ladder[:, 2], rtol=1e-12, atol=0)
    assert np.allclose(plain[:, 4], ladder[:, 4], rtol=1e-12, atol=0)
    assert np.allclose(plain[:, 3], ladder[:, 3], rtol=1e-10, atol=0)


@pytest.mark.parametrize("volume_row", [False, True])
def test_rounds_queued_ahead_do_not_change_the_trajectory(volume_row, monkeypatch):
    """ms_minimize at FULL size (2 048 000 facets, fixed-order sums so that runs are bitwise comparable), three ways:
    without the line-search queue (MS_SPECULATE=0: every decision on the host), with the queue but without rounds queued
    ahead of their step (MS_AHEAD=0), and the default.  The step logs -- success, next step size, energies, |g|, <g,d>,
    accepted alpha, trial counts of every step -- must be equal bit for bit; the queue's own book-keeping must show
    that the device's decisions were replayed without a single difference and that rounds were adopted."""
    from membrane_solver_amd import _lib as L
    from membrane_solver_amd import meshgen
    from membrane_solver_amd.device import DeviceMesh

    P, T = meshgen.icosphere(320)
    P = meshgen.smooth_displace(P, 0.05)
    nv, nf = len(P), len(T)
    v0, v1, v2 = P[T[:, 0]], P[T[:, 1]], P[T[:, 2]]
    V0 = float(np.einsum("ij,ij->i", np.cross(v1, v2), v0).sum() / 6.0)
    logs, stats = [], []
    for env in ({"MS_SPECULATE": "0"}, {"MS_AHEAD": "0"}, {}):
        for k in ("MS_SPECULATE", "MS_AHEAD"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        dm = DeviceMesh(P, T)
        dm.set_deterministic(True)
        dm.set_surface_tension(np.ones(nf))
        dm.set_bending_params(np.ones(nv), np.zeros(nv))
        dm.set_params(modules=L.MS_MOD_SURFACE | L.MS_MOD_BENDING | (L.MS_CON_VOLUME if volume_row else 0),
                      target_volume=V0)
        mp = L.ms_minimize_params()
        mp.stepper = L.ms_stepper_params(L.MS_STEPPER_CG, 10, 0.7, 1e-4, 1.5, 10.0, 10, 0.0, 2)
        mp.step_size, mp.tol = 1e-6, 1e-9
        mp.fixed_step_mode, mp.fixed_step = 0, 1e-6
        mp.max_zero_steps, mp.step_size_floor = 10, 1e-8
        out, log = dm.minimize(mp, 36, want_log=True)
        logs.append(np.array(log))
        stats.append(dm.queue_stats())
        x = dm.get_positions()
        logs[-1] = (logs[-1], x)
        dm.close()
    (plain, x_plain), (queue, x_queue), (ahead, x_ahead) = logs
    assert plain[:, 0].sum() >= 12 and plain[:, 7].max() >= 2, "the run is meant to accept steps after backtracking"
    assert np.array_equal(plain, queue), "the queue changed the trajectory"
    assert np.array_equal(plain, ahead), "rounds queued ahead changed the trajectory"
    assert np.array_equal(x_plain, x_queue) and np.array_equal(x_plain, x_ahead)
    for st in stats:
        assert st["mismatches"] == 0, stats
    assert stats[0]["rounds"] == 0 and stats[1]["rounds"] > 0 and stats[1]["ahead"] == 0
    assert stats[2]["ahead"] > 0 and stats[2]["adopted"] >= stats[2]["ahead"] - stats[2]["dropped"] > 0, stats


def _small_ahead_meshes():
    from membrane_solver_amd import meshgen

    pos, tri = meshgen.icosphere(24)  # (the mesh of test_pair_launch_does_not_change_the_trajectory: 23 tiles)
    pos = meshgen.smooth_displace(pos, 0.05)
    pos = pos + 2.0e-3 * np.random.default_rng(3).standard_normal(pos.shape)
    g = load_golden("mesh_ico4.npz")  # (one tile: the launches go through the one-workgroup interpreter)
    return {"ico24": (pos, tri), "ico4": (np.ascontiguousarray(g["positions"]), np.ascontiguousarray(g["tri"]))}


@pytest.mark.parametrize("volume_row", [False, True])
@pytest.mark.parametrize("kind", ["gd", "cg"])
@pytest.mark.parametrize("mesh_name", ["ico24", "ico4"])
def test_rounds_queued_ahead_do_not_change_the_trajectory_small(mesh_name, kind, volume_row, monkeypatch):
    """test_rounds_queued_ahead_do_not_change_the_trajectory at small size (a 23-tile and a one-tile mesh), gradient
    descent as well as CG: ms_minimize with fixed-order sums without the line-search queue (MS_SPECULATE=0), without
    rounds queued ahead (MS_AHEAD=0) and by default gives the same step log and positions bit for bit; no decision was
    replayed differently; rounds were queued ahead and adopted in the default run only.  (Step size 1e-2 and 40 steps:
    every combination queues and adopts rounds, and the 23-tile mesh and one-tile CG also drop some.)"""
    from membrane_solver_amd import _lib as L
    from membrane_solver_amd.device import DeviceMesh

    P, T = _small_ahead_meshes()[mesh_name]
    nv, nf = len(P), len(T)
    v0, v1, v2 = P[T[:, 0]], P[T[:, 1]], P[T[:, 2]]
    V0 = float(np.einsum("ij,ij->i", np.cross(v1, v2), v0).sum() / 6.0)
    runs = []
    for env in ({"MS_SPECULATE": "0"}, {"MS_AHEAD": "0"}, {}):
        for k in ("MS_SPECULATE", "MS_AHEAD"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        dm = DeviceMesh(P, T)
        dm.set_deterministic(True)
        dm.set_surface_tension(np.ones(nf))
        dm.set_bending_params(np.ones(nv), np.full(nv, 0.2))
        dm.set_params(modules=L.MS_MOD_SURFACE | L.MS_MOD_BENDING | (L.MS_CON_VOLUME if volume_row else 0),
                      target_volume=V0)
        mp = L.ms_minimize_params()
        mp.stepper = L.ms_stepper_params(L.MS_STEPPER_CG if kind == "cg" else L.MS_STEPPER_GD, 10, 0.7, 1e-4, 1.5,
                                         10.0, 10, 0.0, 2)
        mp.step_size, mp.tol = 1e-2, 1e-9
        mp.fixed_step_mode, mp.fixed_step = 0, 1e-2
        mp.max_zero_steps, mp.step_size_floor = 10, 1e-8
        out, log = dm.minimize(mp, 40, want_log=True)
        runs.append((np.array(log), dm.get_positions(), dm.queue_stats()))
        dm.close()
    (plain, x_plain, st_plain), (queue, x_queue, st_queue), (ahead, x_ahead, st_ahead) = runs
    print(mesh_name, kind, volume_row, st_plain, st_queue, st_ahead)
    assert len(plain) == 40 and plain[:, 0].sum() >= 12 and plain[:, 7].max() >= 2, \
        "the run is meant to accept steps after backtracking"
    assert np.array_equal(plain, queue), "the queue changed the trajectory"
    assert np.array_equal(plain, ahead), "rounds queued ahead changed the trajectory"
    assert np.array_equal(x_plain, x_queue) and np.array_equal(x_plain, x_ahead)
    for st in (st_plain, st_queue, st_ahead):
        assert st["mismatches"] == 0, (st_plain, st_queue, st_ahead)
    assert st_plain["rounds"] == 0 and st_queue["rounds"] > 0 and st_queue["ahead"] == 0
    assert st_ahead["ahead"] > 0 and st_ahead["adopted"] >= st_ahead["ahead"] - st_ahead["dropped"] > 0, st_ahead
