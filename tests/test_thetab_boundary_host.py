"""tilt_thetaB_boundary_in on the host: the NumPy restatement of the constraint against the reference's fixture
(tools/gen_golden_thetab_boundary.py), the two tilt seams of ConstraintModuleManager, the Minimizer's refusals and table
key, the C ABI's declarations and the ring row -> facet CSR builder.  No GPU."""

import inspect
import json
import os
import re
import types

import numpy as np
import pytest

from conftest import load_golden
from membrane_solver_amd import _lib as L
from membrane_solver_amd import meshgen
from membrane_solver_amd.core.parameters import GlobalParameters
from membrane_solver_amd.geometry.mesh import ArrayMesh
from membrane_solver_amd.modules.constraints import tilt_thetaB_boundary_in as module
from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "tilt_thetaB_boundary_in"
CASES = load_golden("thetab_boundary_cases.npz")
NAMES = [str(n) for n in CASES["names"]]
TRAJ = ("traj_disk6_cg_thetab_boundary_pins.npz", "traj_disk6_gd_thetab_boundary_alone.npz",
        "traj_disk6_cg_thetab_boundary_pins_apart.npz")


def case_mesh(name):
    """The case as the generator built it: meshgen.disk_patch renumbered by a seeded permutation (laid into the plane
    y = 0 for the flat case), the ring's rows at the recorded positions, the seeded tilt fields and fixed flags
    -> (positions, triangles, tilts_in, tilts_out, tilt_fixed_in, tilt_fixed_out, gp, vertex options)"""
    g = CASES
    spec = json.loads(str(g[name + "__mesh"]))
    P, T, _B = meshgen.disk_patch(spec["n_rings"], bulge=spec["bulge"])
    perm = np.random.default_rng(spec["perm_seed"]).permutation(len(P))
    P2 = np.empty_like(P)
    P2[perm] = P
    if spec["flat_y"]:
        P2 = np.stack([P2[:, 0], np.zeros(len(P2)), P2[:, 1]], axis=1)
    T2 = perm[np.asarray(T)].astype(np.int32)
    rows = g[name + "__rows"].astype(np.int64)
    P2[rows] = g[name + "__ring_positions"]
    rng = np.random.default_rng(spec["field_seed"])
    tin = rng.uniform(-1.0, 1.0, size=P2.shape) / np.sqrt(3.0)
    tout = rng.uniform(-1.0, 1.0, size=P2.shape) / np.sqrt(3.0)
    assert np.array_equal(tin[rows], g[name + "__ring_tilts"]), "the seeded field is not the generator's"
    fin, fout = np.zeros(len(P2), bool), np.zeros(len(P2), bool)
    fin[::7] = True
    fout[3::11] = True
    fin[rows] = g[name + "__ring_fixed_in"]
    vo = {int(k): v for k, v in json.loads(str(g[name + "__vopts"])).items()}
    return P2, T2, tin, tout, fin, fout, json.loads(str(g[name + "__gp"])), vo


def array_mesh(name):
    P, T, tin, tout, fin, fout, gp, vo = case_mesh(name)
    mesh = ArrayMesh(P, T, global_parameters=GlobalParameters(gp), tilts_in=tin, tilts_out=tout, tilt_fixed_in=fin,
                     tilt_fixed_out=fout, vertex_options=vo)
    return mesh, mesh.global_parameters


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_reference(name):
    """Directions and keep flags, the enforcement and the gradient projection of the host module, through the manager's
    two seams."""
    g = CASES
    mesh, gp = array_mesh(name)
    P, tin, tout = mesh.positions_view().copy(), mesh.tilts_in_view().copy(), mesh.tilts_out_view().copy()
    rows = g[name + "__rows"].astype(np.int64)
    keep_ref, d_ref = g[name + "__keep"], g[name + "__d"]
    data = module.directions(mesh, gp, positions=P)
    if name in ("no_group", "no_rows"):
        assert data is None and not keep_ref.any()
    else:
        r, d, keep = data
        assert np.array_equal(r, rows) and np.array_equal(keep, keep_ref)
        assert np.max(np.abs(d - d_ref)) <= 1e-12 and not d[~keep].any()
    cm = ConstraintModuleManager([NAME])
    free = keep_ref & ~g[name + "__ring_fixed_in"]
    sparse = module.constraint_gradients_tilt_rows_array(mesh, gp, positions=P, index_map=mesh.vertex_index_to_row)
    dense = module.constraint_gradients_tilt_array(mesh, gp, positions=P, index_map=mesh.vertex_index_to_row)
    if free.any():
        assert [int(p[0][0][0]) for p in sparse] == [int(x) for x in rows[free]] and all(p[1] is None for p in sparse)
        assert len(dense) == len(sparse) and all(np.count_nonzero(np.any(gd[0] != 0.0, axis=1)) == 1 for gd in dense)
    else:
        assert sparse is None and dense is None
    assert module.constraint_gradients(mesh, gp) is None
    assert module.constraint_gradients_array(mesh, gp, positions=P, index_map=mesh.vertex_index_to_row) is None
    # enforce: the free kept ring rows move, nothing else does
    cm.enforce_tilt_constraints(mesh, global_params=gp)
    got = np.array(mesh.tilts_in_view())
    assert np.max(np.abs(got[rows] - g[name + "__ring_enforced"])) <= 1e-12
    rest = np.ones(len(P), bool)
    rest[rows[free]] = False
    assert np.array_equal(got[rest], tin[rest]) and np.array_equal(mesh.tilts_out_view(), tout)
    assert np.array_equal(mesh.positions_view(), P)
    theta = float(gp.get("tilt_thetaB_value") or 0.0)
    if free.any():
        assert np.max(np.abs(np.einsum("ij,ij->i", got[rows], d_ref)[free] - theta)) <= 1e-14
    # gradient seam: the recorded raw rows in, the recorded projected rows out (then the fixed rows' zeroing)
    gi, go = np.zeros_like(P), np.full_like(P, 0.25)
    gi[rows] = g[name + "__ring_grad_raw"]
    cm.apply_tilt_gradient_modifications_array(gi, go, mesh, gp, positions=P, tilts_in=tin, tilts_out=tout)
    gi[mesh.tilt_fixed_in] = 0.0
    assert np.max(np.abs(gi[rows] - g[name + "__ring_grad_projected"])) <= 1e-12
    off_ring = np.ones(len(P), bool)
    off_ring[rows] = False
    assert not gi[off_ring].any() and np.all(go == 0.25)
    untouched = rows[~free & ~g[name + "__ring_fixed_in"]]  # dropped rows keep their raw gradient
    assert np.array_equal(gi[untouched], g[name + "__ring_grad_raw"][~free & ~g[name + "__ring_fixed_in"]])


def test_manager_seams():
    mesh, gp = array_mesh("fixed_rows")
    cm = ConstraintModuleManager(["pin_to_circle", NAME])
    assert hasattr(cm, "enforce_tilt_constraints") and hasattr(cm, "apply_tilt_gradient_modifications_array")
    assert not hasattr(module, "enforce_constraint")  # (alone it switches no enforcer on)
    assert sorted(module.__all__) == ["constraint_gradients", "constraint_gradients_array", "constraint_gradients_tilt_array",
                                      "constraint_gradients_tilt_rows_array", "enforce_tilt_constraint"]
    P, tin = mesh.positions_view().copy(), mesh.tilts_in_view().copy()
    cm.enforce_all(mesh, context="minimize", global_params=gp)  # the tilt-only module is not asked for a shape projection
    assert np.array_equal(mesh.positions_view(), P) and np.array_equal(mesh.tilts_in_view(), tin)
    calls = []
    cm.enforce_tilt_constraints(mesh, global_params=gp, device=types.SimpleNamespace(
        thetab_boundary_enforce=lambda: calls.append("device")))
    assert calls == ["device"] and np.array_equal(mesh.tilts_in_view(), tin), "with a device the mesh's arrays stay"
    with pytest.raises(ValueError, match="matching shapes"):
        cm.apply_tilt_gradient_modifications_array(np.zeros((3, 3)), np.zeros((4, 3)), mesh, gp)
    # a manager without a tilt module: both seams do nothing
    cm0 = ConstraintModuleManager(["pin_to_circle"])
    gi = np.ones_like(P)
    cm0.apply_tilt_gradient_modifications_array(gi, gi.copy(), mesh, gp)
    cm0.enforce_tilt_constraints(mesh, global_params=gp)
    assert np.all(gi == 1.0) and np.array_equal(mesh.tilts_in_view(), tin)


# -- the Minimizer: refusals, the table key --------------------------------------------------------------------------------
def _minimizer(gp_extra=None, energy=("tilt_in", "tilt_out"), cons=(NAME,), name="n003"):
    from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager
    from membrane_solver_amd.runtime.minimizer import Minimizer
    from membrane_solver_amd.runtime.steppers import GradientDescent

    P, T, tin, tout, fin, fout, gp, vo = case_mesh(name)
    gp = dict(gp, **(gp_extra or {}))
    gp = {k: v for k, v in gp.items() if v is not None}
    mesh = ArrayMesh(P, T, global_parameters=GlobalParameters(gp), tilts_in=tin, tilts_out=tout, tilt_fixed_in=fin,
                     tilt_fixed_out=fout, vertex_options=vo, energy_modules=list(energy), constraint_modules=list(cons))
    return Minimizer(mesh, mesh.global_parameters, GradientDescent(), EnergyModuleManager(list(energy)),
                     ConstraintModuleManager(list(cons)), quiet=True)


INNER = L.MS_MOD_TILT_IN | L.MS_MOD_TILT_OUT


def test_minimizer_accepts_the_module_and_keeps_the_enforcer_off():
    mz = _minimizer()
    assert mz._has_enforceable_constraints is False  # alone: no line-search enforcer, no tilt restore
    prm = mz._thetab_boundary_params(INNER)
    assert np.array_equal(prm["rows"], CASES["n003__rows"]) and prm["normal"] == (0.0, 0.0, 1.0)
    assert prm["center"] == (0.03, -0.02, 0.01)
    assert _minimizer(cons=("pin_to_circle", NAME))._has_enforceable_constraints is True
    assert _minimizer(cons=())._thetab_boundary_params(INNER) is None
    assert _minimizer(name="no_group")._thetab_boundary_params(INNER) is None
    assert _minimizer(name="no_rows")._thetab_boundary_params(INNER) is None


@pytest.mark.parametrize("extra,mods,cons,exc,why", [
    ({}, L.MS_MOD_TILT_OUT, (NAME,), L.MembraneHipError, "without an active inner-leaflet tilt module"),
    ({}, INNER | L.MS_MOD_TILT, (NAME,), L.MembraneHipError, "together with a single-field tilt module"),
    ({"tilt_thetaB_normal": None}, INNER, (NAME,), L.MembraneHipError, "without a non-zero tilt_thetaB_normal"),
    ({"tilt_thetaB_normal": [0.0, 0.0, 0.0]}, INNER, (NAME,), L.MembraneHipError, "without a non-zero tilt_thetaB_normal"),
    ({"tilt_thetaB_group_in": "disk"}, INNER, (NAME,), L.MembraneHipError, "group 'disk' and no parity_trace_layer_radius"),
    ({"tilt_thetaB_optimize": True}, INNER, (NAME,), L.MembraneHipError, "with tilt_thetaB_optimize"),
    ({"tilt_projection_cadence": "per_eval"}, INNER, (NAME,), ValueError, "tilt_projection_cadence must be"),
    ({"tilt_projection_interval": -2}, INNER, (NAME,), ValueError, "tilt_projection_interval must be >= 1"),
    ({"tilt_thetaB_center": [0.0, float("nan"), 0.0]}, INNER, (NAME,), L.MembraneHipError, "must be finite"),
    ({"tilt_thetaB_normal": [0.0, float("inf"), 1.0]}, INNER, (NAME,), L.MembraneHipError, "must be finite"),
    ({"tilt_thetaB_value": float("inf")}, INNER, (NAME,), L.MembraneHipError, "must be finite"),
    ({}, INNER, ("volume", NAME), L.MembraneHipError, "next to the volume constraint"),
])
def test_refusals(extra, mods, cons, exc, why):
    name = "n003"
    if extra.get("tilt_thetaB_group_in") == "disk":  # tag the rows with that group
        mz = _minimizer(extra, cons=cons)
        mz.mesh.vertex_options = {r: {"tilt_thetaB_group": "disk"} for r in mz.mesh.vertex_options}
    else:
        mz = _minimizer(extra, cons=cons, name=name)
    with pytest.raises(exc, match=why):
        mz._thetab_boundary_params(mods)


def test_refusals_next_to_pins():
    """A listed pin module whose program is empty (nothing is tagged), and pins together with the volume drift check of a
    body with a target volume: both refused before anything is uploaded (the method runs without a device)."""
    mz = _minimizer(cons=("pin_to_circle", NAME))
    with pytest.raises(L.MembraneHipError, match="next to a pin module that pins nothing"):
        mz._thetab_boundary_params(INNER)
    assert mz._tbb_active is False
    pin = {"constraints": ["pin_to_circle"], "pin_to_circle_group": "g", "pin_to_circle_mode": "slide",
           "pin_to_circle_normal": [0.0, 0.0, 1.0]}
    mz = _minimizer(cons=("pin_to_circle", NAME))
    ring = sorted(mz.mesh.vertex_options)
    mz.mesh.vertex_options = {r: dict(o, **(pin if r in ring[:3] else {})) for r, o in mz.mesh.vertex_options.items()}
    assert mz._thetab_boundary_params(INNER) is not None  # pins that pin something, no body: taken
    mz.mesh.bodies = {0: types.SimpleNamespace(target_volume=1.0, options={})}
    mz.global_params.set("volume_projection_during_minimization", False)
    with pytest.raises(L.MembraneHipError, match="volume drift check"):
        mz._thetab_boundary_params(INNER)
    mz.global_params.set("volume_projection_during_minimization", True)
    assert mz._thetab_boundary_params(INNER) is not None


def test_disk_group_with_an_explicit_trace_radius_is_taken():
    mz = _minimizer({"tilt_thetaB_group_in": "disk", "parity_trace_layer_radius": 0.4})
    mz.mesh.vertex_options = {r: {"tilt_thetaB_group": "disk"} for r in mz.mesh.vertex_options}
    assert mz._thetab_boundary_params(INNER) is not None


def test_device_layer_refusals_without_a_device():
    from membrane_solver_amd.device import DeviceMesh

    with pytest.raises(L.MembraneHipError, match="tilt_thetaB_boundary_in constraint is not sharded"):
        DeviceMesh.set_thetab_boundary(types.SimpleNamespace(shard_count=2), [1, 2, 3])
    for bad, why in ((("per_eval", 1), "tilt_projection_cadence must be"), (("per_step", 0), "tilt_projection_interval must be")):
        with pytest.raises(ValueError, match=why):
            DeviceMesh.set_tilt_projection(types.SimpleNamespace(), *bad)
    src = open(os.path.join(ROOT, "membrane_solver_amd", "csrc", "ms_api_thetab_bnd.inc")).read()
    for text in ("is not sharded (single GPU only)", "interval must be >= 1",
                 "cadence must be MS_TILT_PROJECTION_PER_STEP or MS_TILT_PROJECTION_PER_PASS"):
        assert text in src, text
    # the ring's and the plane's refusals are worded once for every ring setter (ms_api_tables.inc); this one hands them
    # its name and its nouns, which makes "ms_set_thetab_boundary: ring row out of range" and so on
    shared = open(os.path.join(ROOT, "membrane_solver_amd", "csrc", "ms_api_tables.inc")).read()
    for text in ('": " + noun + " row out of range"', '": " + a_noun + " row is listed twice"',
                 '": center and normal must be finite"', '": a non-zero plane normal is required"'):
        assert text in shared, text
    assert 'const char* who = "ms_set_thetab_boundary";' in src
    assert re.search(r'ring_rows\(c, who, "ring", "a ring", nv, c->til\.iperm\.data\(\), n_rows, rows, seen, lib\.data\(\)\)', src)
    assert "plane_finite(c, who, p->center, p->normal)" in src and "plane_frame(c, who, p->normal, unit)" in src
    # an unknown constraint module
    with pytest.raises(L.MembraneHipError, match="outside the HIP hot path"):
        _minimizer(cons=(NAME, "pins"))


def test_table_key():
    prm = _minimizer()._thetab_boundary_params(INNER)
    key = module.device_key(prm)
    assert module.device_key(None) is None and key == module.device_key(dict(prm))
    assert key == module.device_key(_minimizer({"tilt_thetaB_value": 0.4})._thetab_boundary_params(INNER)), \
        "theta_B is no part of the table"
    assert key != module.device_key(dict(prm, rows=prm["rows"][::-1].copy()))
    assert key != module.device_key(dict(prm, center=(0.0, 0.0, 0.0)))
    assert key != module.device_key(_minimizer({"tilt_thetaB_normal": [0.0, 1.0, 1.0]})._thetab_boundary_params(INNER))
    assert module.projection_schedule({}) == ("per_step", 1)
    assert module.projection_schedule({"tilt_projection_cadence": " Per_Pass ", "tilt_projection_interval": 3}) == ("per_pass", 3)


# -- C ABI and sources ------------------------------------------------------------------------------------------------------
ABI = ("ms_set_thetab_boundary", "ms_set_tilt_projection", "ms_thetab_boundary_enforce", "ms_thetab_boundary_directions",
       "ms_thetab_boundary_projected_gradient", "ms_thetab_boundary_stats", "ms_thetab_boundary_tables_host")


def test_abi_is_declared_bound_and_built():
    header = open(os.path.join(ROOT, "include", "membrane_hip.h")).read()
    for fn in ABI:
        assert re.search(r"\bint %s\(" % fn, header), fn
        assert fn in L.SIGNATURES and hasattr(L.lib(), fn), fn
    assert "ms_tilt_relax_params" in header and "tilt_projection" not in \
        header[header.index("typedef struct ms_tilt_relax_params"):header.index("} ms_tilt_relax_params;")]
    mk = open(os.path.join(ROOT, "membrane_solver_amd", "csrc", "Makefile")).read()
    assert "ms_thetab_bnd.hip" in mk and "$(BUILD)/ms_thetab_bnd.o" in mk
    kern = open(os.path.join(ROOT, "membrane_solver_amd", "csrc", "ms_thetab_bnd.hip")).read()
    assert "k_tbb_geom" in kern and "k_tbb_apply" in kern and not re.search(r"atomic\w*\(", kern)
    assert "__launch_bounds__(LB)" in kern
    from membrane_solver_amd.device import DeviceMesh
    for meth in ("set_thetab_boundary", "set_tilt_projection", "thetab_boundary_enforce", "thetab_boundary_directions",
                 "thetab_boundary_projected_gradient", "thetab_boundary_stats"):
        assert inspect.isfunction(getattr(DeviceMesh, meth)), meth


@pytest.mark.parametrize("name", ["n001", "n065", "n257", "no_rows"])
def test_csr_builder_against_numpy(name):
    """ms_thetab_boundary_tables_host: per ring row its incident facets in ascending facet order, every entry the facet's
    three rows in its own order, mapped through the row permutation."""
    P, T, *_rest = case_mesh(name)
    rows = CASES[name + "__rows"].astype(np.int64) if name != "no_rows" else np.zeros(0, np.int64)
    nv = len(P)
    iperm = np.random.default_rng(5).permutation(nv).astype(np.int32)
    off, fv = module.tables_host(nv, iperm, T, rows)
    counts = np.bincount(T.reshape(-1), minlength=nv)[rows]
    assert off[0] == 0 and np.array_equal(np.diff(off), counts) and fv.shape == (int(counts.sum()), 3)
    for i, r in enumerate(rows):
        facets = np.flatnonzero(np.any(T == r, axis=1))  # ascending
        assert np.array_equal(fv[off[i]:off[i + 1]], iperm[T[facets]])
    bad = np.array([0, nv], np.int64)
    with pytest.raises(L.MembraneHipError, match="ring row out of range"):
        module.tables_host(nv, iperm, T, bad)
    with pytest.raises(L.MembraneHipError, match="listed twice"):
        module.tables_host(nv, iperm, T, np.array([3, 3]))


def test_fixtures_hold_what_the_issue_asks_for():
    g = CASES
    assert {"n001", "n002", "n003", "n063", "n064", "n065", "n255", "n256", "n257"} <= set(NAMES)
    assert int((~g["row_on_center__keep"]).sum()) == 1 and int((~g["flat_d_zero__keep"]).sum()) == 2
    assert g["fixed_rows__ring_fixed_in"].sum() >= 6
    assert "tilt_thetaB_value" not in json.loads(str(g["theta_zero__gp"]))
    rel = load_golden("thetab_boundary_relax.npz")
    labels = [str(x) for x in rel["labels"]]
    assert len(labels) == 12 and len(rel["positions"]) == 84
    assert all(int(rel[lb + "__tilt_inner_steps"]) == 40 for lb in labels)
    pins, alone, apart = (load_golden(f) for f in TRAJ)
    assert int(pins["n_steps"]) == int(alone["n_steps"]) == int(apart["n_steps"]) == 5
    assert [str(c) for c in pins["constraint_modules"]] == ["pin_to_circle", NAME]
    assert [str(c) for c in alone["constraint_modules"]] == [NAME]
    # the run with the pins ON the ring is kept inside the reference's safe-step limit, where its directions are not stale
    # (the generator's docstring): no search of it backtracks.  The run with the pins APART from the ring holds the
    # rejected trials: an accepted search behind rejected trials and a search that accepts nothing
    assert np.all(pins["step_log"][:, 0] > 0) and np.all(pins["line_search_evals"] == 2)
    assert [str(c) for c in apart["constraint_modules"]] == ["pin_to_circle", NAME]
    assert np.any((apart["step_log"][:, 0] > 0) & (apart["line_search_evals"] >= 3)), "no rejected trial"
    assert np.any((apart["step_log"][:, 0] == 0) & (apart["line_search_evals"] >= 3)), "no search that rejects every trial"
    vo = {int(k): v for k, v in json.loads(str(apart["vopts"])).items()}
    ring = {r for r, o in vo.items() if o.get("tilt_thetaB_group") == "ring"}
    pinned = {r for r, o in vo.items() if "pin_to_circle" in (o.get("constraints") or [])}
    touching = {int(v) for t in apart["tri"] if ring & set(int(x) for x in t) for v in t}
    assert ring and pinned and not (pinned & touching), "a pinned row is a facet neighbour of the ring"
    for f in os.listdir(os.path.join(ROOT, "tests", "golden")):
        if "thetab_boundary" in f:
            assert os.path.getsize(os.path.join(ROOT, "tests", "golden", f)) < 1 << 20
