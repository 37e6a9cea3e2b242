"""body_area / global_area without a GPU: the reference fixtures against a NumPy restatement of the row and of the one- and
two-row KKT projection, the ABI's symbols, the names Minimizer accepts and everything it refuses."""

import ast
import os
import types

import numpy as np
import pytest

from membrane_solver_amd import _lib as L
from membrane_solver_amd import meshgen
from membrane_solver_amd.geometry.mesh import ArrayBody, ArrayMesh
from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager
from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager
from membrane_solver_amd.runtime.minimizer import Minimizer
from membrane_solver_amd.runtime.steppers import GradientDescent

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TRAJ = ["traj_ico4_gd_areacon_bending.npz", "traj_ico4_gd_areacon_fixed_rows.npz", "traj_ico4_gd_areacon_surface_subset.npz",
        "traj_ico4_gd_areacon_volume_rows.npz", "traj_ico4_cg_areacon_volume_rows.npz",
        "traj_ico4_gd_areacon_volume_enforcers.npz", "traj_ico4_cg_areacon_volume_enforcers.npz",
        "traj_ico4_gd_areacon_volume_subset.npz", "traj_ico8_cg_areacon_bending.npz", "traj_ico4_gd_areacon_global.npz"]


def area_row(P, T, facets):
    """body_area.py:51-63 restated: n = (v1 - v0) x (v2 - v0), |n| < 1e-12 skipped, g0 = 1/2 (v1 - v2) x n_hat, cyclic."""
    t = np.asarray(T)[np.asarray(facets)]
    v0, v1, v2 = P[t[:, 0]], P[t[:, 1]], P[t[:, 2]]
    n = np.cross(v1 - v0, v2 - v0)
    A2 = np.linalg.norm(n, axis=1)
    keep = A2 >= 1e-12
    nh = n[keep] / A2[keep][:, None]
    g = np.zeros_like(P)
    np.add.at(g, t[keep, 0], 0.5 * np.cross(v1[keep] - v2[keep], nh))
    np.add.at(g, t[keep, 1], 0.5 * np.cross(v2[keep] - v0[keep], nh))
    np.add.at(g, t[keep, 2], 0.5 * np.cross(v0[keep] - v1[keep], nh))
    return g, 0.5 * A2.sum(), keep


def volume_row(P, T):
    g = np.zeros_like(P)
    a, b, c = P[T[:, 0]], P[T[:, 1]], P[T[:, 2]]
    np.add.at(g, T[:, 0], np.cross(b, c) / 6.0)
    np.add.at(g, T[:, 1], np.cross(c, a) / 6.0)
    np.add.at(g, T[:, 2], np.cross(a, b) / 6.0)
    return g


def project(g, rows):
    """constraint_manager.py:293-301 (one row) / constraint_projection.py:101-129 (two rows), restated."""
    g = g.copy()
    if len(rows) == 1:
        nn = float(np.sum(rows[0] * rows[0]))
        if nn > 1e-18:
            g -= (float(np.sum(g * rows[0])) / nn) * rows[0]
        return g
    C = np.stack([r.reshape(-1) for r in rows])
    A = C @ C.T + 1e-18 * np.eye(len(rows))
    lam = np.linalg.solve(A, C @ g.reshape(-1))
    return g - (C.T @ lam).reshape(g.shape)


def test_fixtures_are_self_consistent_and_numpy_reproduces_them():
    z = np.load(os.path.join(GOLD, "area_con_cases.npz"))
    names = [str(n) for n in z["names"]]
    assert {"ico4_whole_area", "ico4_whole_vol_area", "ico4_subset_area", "ico4_fixed_vol_area", "ico8_whole_vol_area",
            "ico8_subset_area", "ico8_subset_fixed_area", "disk5_whole_area", "ico4_degenerate_area"} == set(names)
    for name in names:
        P, T, facets = z[name + "__positions"], z[name + "__tri"], z[name + "__body_facets"]
        fixed = z[name + "__fixed"]
        cmods = [str(s) for s in z[name + "__constraint_modules"]]
        gA, A, keep = area_row(P, T, facets)
        ref = z[name + "__gA"]
        assert np.abs(gA - ref).max() <= 1e-13 * np.abs(ref).max(), name
        assert abs(A - float(z[name + "__area"])) <= 1e-13 * A, name
        rows = ([volume_row(P, T)] if "volume" in cmods else []) + [gA]
        assert len(rows) == len(cmods)
        after = project(z[name + "__g_before"], rows)
        after[fixed] = 0.0  # minimizer.py:982-990: after the projection
        scale = np.abs(z[name + "__g_before"]).max()
        assert np.abs(after - z[name + "__g_after"]).max() <= 1e-12 * scale, name
        assert not z[name + "__g_after"][fixed].any()
        if "fixed" in name:
            assert fixed[::7].all() and fixed.sum() == len(range(0, len(P), 7))
            assert np.abs(ref[fixed]).max() > 0.0  # (the row itself is not masked)
        if name == "ico4_degenerate_area":
            f = int(z[name + "__degenerate_facet"])
            assert f in set(facets.tolist()) and not keep.all() and not keep[list(facets).index(f)]
    # the subsets straddle tile borders on ico8: the body owns part of the facets of more than one 64-row tile
    f8 = z["ico8_subset_area__body_facets"]
    assert 0 < len(f8) < len(z["ico8_subset_area__tri"])
    enf = [str(n) for n in z["enforcer_names"]]
    assert len(enf) == 6
    for name in enf:
        module, target = str(z[name + "__module"]), float(z[name + "__target"])
        assert module in ("body_area", "global_area")
        iters = int(z[name + "__iters"])
        assert 1 <= iters <= (20 if module == "body_area" else 3)
        fixed = z[name + "__fixed"]
        assert np.array_equal(z[name + "__positions_final"][fixed], z[name + "__positions"][fixed])
        _g, A1, _k = area_row(z[name + "__positions_final"], z[name + "__tri"], z[name + "__body_facets"])
        assert abs(A1 - float(z[name + "__area_final"])) <= 1e-12 * A1
        if iters < (20 if module == "body_area" else 3):  # it stopped on the tolerance
            assert abs(A1 - target) < 1e-12


@pytest.mark.parametrize("fname", TRAJ)
def test_reference_accepted_at_least_half_of_every_trajectory(fname):
    z = np.load(os.path.join(GOLD, fname))
    log = np.asarray(z["step_log"]).reshape(-1, 3)
    assert len(log) == int(z["n_steps"]) and 2 * int(log[:, 0].sum()) >= len(log)
    cm = [str(s) for s in z["constraint_modules"]]
    assert cm in (["body_area"], ["volume", "body_area"], ["global_area"])


def test_abi_symbols_and_constants():
    for sym in ("ms_set_area_constraint", "ms_clear_area_constraint", "ms_project_area", "ms_project_area_cached",
                "ms_area_row", "ms_area_stats"):
        assert sym in L.SIGNATURES, sym
    hdr = open(os.path.join(ROOT, "include", "membrane_hip.h")).read()
    for sym in ("ms_set_area_constraint", "ms_clear_area_constraint", "ms_project_area", "ms_project_area_cached",
                "ms_area_row", "ms_area_stats", "MS_CON_BODY_AREA 33554432u", "int enforce_area;", "int enforce_area_iters;"):
        assert sym in hdr, sym
    assert L.MS_CON_BODY_AREA == 1 << 25 and (L.MS_AREA_NONE, L.MS_AREA_BODY, L.MS_AREA_GLOBAL) == (0, 1, 2)
    fields = [f[0] for f in L.ms_stepper_params._fields_]
    assert fields[-2:] == ["enforce_area", "enforce_area_iters"]
    # the bit collides with no module bit
    others = [v for k, v in vars(L).items() if k.startswith(("MS_MOD_", "MS_CON_", "MS_TRACK_")) and k != "MS_CON_BODY_AREA"]
    assert all(isinstance(v, int) and not (v & L.MS_CON_BODY_AREA) for v in others)


def _mz(emods=("bending",), cons=("body_area",), bodies=None, gp=None, vopts=None, mesh_fn=None):
    P, T = meshgen.icosphere(2)
    if bodies is None:
        bodies = [ArrayBody(options={"target_area": 12.0})]
    mesh = ArrayMesh(P, T, global_parameters=dict(gp or {"bending_modulus": 1.0}), bodies=bodies, vertex_options=vopts,
                     energy_modules=list(emods), constraint_modules=list(cons))
    return Minimizer(mesh, mesh.global_parameters, GradientDescent(), EnergyModuleManager(list(emods)),
                     ConstraintModuleManager(list(cons)), quiet=True)


def test_minimizer_accepts_the_names_and_resolves_the_targets():
    mz = _mz(cons=("volume", "body_area"))
    assert mz._has_enforceable_constraints
    assert mz._area_constraint_params() == (L.MS_AREA_BODY, 12.0, 20)
    mz = _mz(cons=("global_area",), gp={"bending_modulus": 1.0, "target_surface_area": 11.5})
    assert mz._area_constraint_params() == (L.MS_AREA_GLOBAL, 11.5, 3)
    # no-ops, as in the reference: no body, no target_area in the body's options (the penalty's area_target is another
    # key), no target_surface_area
    assert _mz(bodies=[])._area_constraint_params() is None
    assert _mz(bodies=[ArrayBody(options={"area_target": 12.0})])._area_constraint_params() is None
    assert _mz(cons=("global_area",))._area_constraint_params() is None
    # the module list order rule: pins -> volume -> area is the device's order
    _mz(cons=("volume", "body_area"))
    _mz(cons=("volume", "global_area"))
    with pytest.raises(L.MembraneHipError, match="lists volume after body_area"):
        _mz(cons=("body_area", "volume"))
    with pytest.raises(L.MembraneHipError, match="lists volume after global_area"):
        _mz(cons=("global_area", "volume"))


def test_every_refusal_has_its_own_text():
    with pytest.raises(L.MembraneHipError, match="body_area and global_area together"):
        _mz(cons=("body_area", "global_area"))
    with pytest.raises(L.MembraneHipError, match="more than one body"):
        _mz(bodies=[ArrayBody(index=0, options={"target_area": 1.0}), ArrayBody(index=1)])
    for tilt in ("tilt", "tilt_in", "bending_tilt_out"):
        with pytest.raises(L.MembraneHipError, match="body_area together with tilt modules"):
            _mz(emods=("surface", tilt))
    with pytest.raises(L.MembraneHipError, match="global_area together with tilt modules"):
        _mz(emods=("surface", "tilt_in"), cons=("global_area", "tilt_thetaB_boundary_in"))
    with pytest.raises(L.MembraneHipError, match="body_area together with body_area_penalty"):
        _mz(emods=("surface", "body_area_penalty"))
    for pin in ("pin_to_plane", "pin_to_circle"):
        with pytest.raises(L.MembraneHipError, match="body_area next to pin_to_plane / pin_to_circle"):
            _mz(cons=(pin, "body_area"))
    for bad in (float("nan"), float("inf"), 0.0, -3.0):
        with pytest.raises(L.MembraneHipError, match="target_area must be finite and positive"):
            _mz(bodies=[ArrayBody(options={"target_area": bad})])._area_constraint_params()
        with pytest.raises(L.MembraneHipError, match="target_surface_area must be finite and positive"):
            _mz(cons=("global_area",), gp={"target_surface_area": bad})._area_constraint_params()
    # the sharded drivers, and the library's own texts (raised on a GPU: tests/test_gpu_area_constraint.py)
    from membrane_solver_amd.parallel import HipShardBackend

    with pytest.raises(L.MembraneHipError, match="body_area constraint is not sharded"):
        HipShardBackend.configure(types.SimpleNamespace(), modules=L.MS_MOD_SURFACE | L.MS_CON_BODY_AREA)
    src = "".join(open(os.path.join(ROOT, "membrane_solver_amd", "csrc", f)).read()
                  for f in ("ms_api_area_con.inc", "ms_api_step.inc", "ms_api_shard.inc", "ms_api_context.inc"))
    for text in ("the target area must be finite and positive", "the area constraints are not sharded (single GPU only)",
                 "the body_area / global_area constraints are not sharded (single GPU only)",
                 "the body_area / global_area constraints together with a tilt-family module are outside the device path",
                 "the body_area / global_area constraints next to pin_to_plane / pin_to_circle are outside the device path",
                 "the body_area / global_area constraints together with body_area_penalty are outside the device path",
                 "the body_area constraint row together with a tilt-family module is outside the device path",
                 "ms_stepper_params.enforce_area without an area constraint"):
        assert text in src, text


def test_unknown_constraint_names_stay_refused():
    with pytest.raises(L.MembraneHipError, match="outside the HIP hot path"):
        _mz(cons=("body_area", "pins"))  # (a module of the package that is no constraint of the path)


def test_trajectory_fixture_options_parse():
    for fname in TRAJ:
        z = np.load(os.path.join(GOLD, fname))
        opts = ast.literal_eval(str(z["body_options"]))
        gp = ast.literal_eval(str(z["gp"]))
        if "global_area" in [str(s) for s in z["constraint_modules"]]:
            assert gp["target_surface_area"] == 12.0 and "target_area" not in opts
        else:
            assert opts["target_area"] > 0.0
