"""pin_to_plane / pin_to_circle: the tag resolver and the host restatement of enforce_all and the KKT projection
against the reference's own outputs (tests/golden/pin_cases.npz, tools/gen_golden_pins.py).  CPU only."""

import ast
import os

import numpy as np
import pytest

from membrane_solver_amd import _lib as L
from membrane_solver_amd.geometry.mesh import ArrayMesh
from membrane_solver_amd.modules.constraints import pins
from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager

GOLD = os.path.join(os.path.dirname(__file__), "golden", "pin_cases.npz")
MODS = ["pin_to_plane", "pin_to_circle"]


def _case(name):
    z = np.load(GOLD)
    gp = ast.literal_eval(str(z[name + "__gp"]))
    mesh = ArrayMesh(z[name + "__positions0"], z["tri"], fixed=z[name + "__fixed"], global_parameters=dict(gp),
                     vertex_options=ast.literal_eval(str(z[name + "__vopts"])), edges=z[name + "__edges"],
                     edge_options=ast.literal_eval(str(z[name + "__eopts"])), constraint_modules=MODS)
    return z, mesh


def _names():
    return [str(n) for n in np.load(GOLD)["names"]]


@pytest.mark.parametrize("name", _names())
def test_enforce_all_matches_reference(name):
    z, mesh = _case(name)
    ConstraintModuleManager(MODS).enforce_all(mesh, global_params=mesh.global_parameters, context="minimize")
    np.testing.assert_allclose(mesh.positions_view(), z[name + "__positions1"], rtol=0, atol=1e-13)


@pytest.mark.parametrize("name", _names())
def test_gradient_projection_matches_reference(name):
    z, mesh = _case(name)
    g = z[name + "__grad0"].copy()
    ConstraintModuleManager(MODS).apply_gradient_modifications_array(g, mesh, mesh.global_parameters)
    np.testing.assert_allclose(g, z[name + "__grad1"], rtol=0, atol=1e-13)


@pytest.mark.parametrize("name", _names())
def test_device_tables_lane_and_closed_form(name):
    """The lane the tables carry is the reference's outcome (untouched gradient = skip), and in the project lane
    the device's closed form (per-row directions, then the slide supports' normal means) gives the reference's
    projected gradient."""
    z, mesh = _case(name)
    X = mesh.positions_view()
    t = pins.device_tables(X, pins.programs(mesh, MODS))
    untouched = np.array_equal(z[name + "__grad0"], z[name + "__grad1"])
    assert t.lane == ("skip" if untouched else "project"), (t.lane, t.n_rows, t.rank)
    if t.lane != "project":
        assert t.rank < t.n_rows
        return
    g = z[name + "__grad0"].copy()
    P = np.asarray(t.params).reshape(-1, 7)
    for row, kind, k in zip(t.grad_row, t.grad_kind, t.grad_param):
        n, c = P[k, :3], P[k, 3:6]
        if kind != pins.GRAD_RADIAL:
            g[row] -= np.dot(g[row], n) * n
        if kind != pins.GRAD_PLANE:
            rh = pins._radial_hat(X[row], n, c)
            g[row] -= np.dot(g[row], rh) * rh
    for s, k in enumerate(t.avg_param):
        rows = t.avg_row[t.avg_off[s]:t.avg_off[s + 1]]
        n = P[k, :3]
        m = np.mean(g[rows] @ n)
        g[rows] += (m - g[rows] @ n)[:, None] * n[None, :]
    fixed = z[name + "__fixed"]
    ref = z[name + "__grad1"].copy()
    g[fixed] = ref[fixed] = 0.0  # (the minimizer zeroes fixed rows after the projection)
    np.testing.assert_allclose(g, ref, rtol=0, atol=1e-12)


def test_fixed_segment_levels_touch_a_row_once():
    z, mesh = _case("plane_fixed_edges")
    t = pins.device_tables(mesh.positions_view(), pins.programs(mesh, MODS))
    for s in range(len(t.stage_kind)):
        rows = t.item_row[t.stage_off[s]:t.stage_off[s + 1]]
        assert len(rows) == len(set(rows))
    assert len(t.stage_kind) == 2  # every ring vertex ends two edges
    assert t.lane == "skip"  # (the two rows of such a vertex are equal)


@pytest.mark.parametrize("gp,msg", [
    ({"pin_to_plane_mode": "fit"}, "fit"),
    ({"pin_to_circle_mode": "fit"}, "fit"),
    ({"pin_to_plane_normal": [0, 1, 1]}, "coordinate axis"),
    ({"pin_to_circle_mesh_operation_preserve_normal_groups": ["a"]}, "preserve_normal"),
    ({"pin_to_circle_mode": "slide"}, "fitted normal"),
])
def test_out_of_scope_settings_raise(gp, msg):
    z, mesh = _case("plane_and_circle_same_vertex")
    mesh.global_parameters.update(gp) if hasattr(mesh.global_parameters, "update") else [
        mesh.global_parameters.set(k, v) for k, v in gp.items()]
    with pytest.raises(L.MembraneHipError, match=msg):
        pins.programs(mesh, MODS)


# ---- pins with the Lagrange volume row (tests/golden/pin_volume_cases.npz) ----------------------------------------
VGOLD = os.path.join(os.path.dirname(__file__), "golden", "pin_volume_cases.npz")


def _vcase(name):
    z = np.load(VGOLD)
    mesh = ArrayMesh(z[name + "__positions0"], z["tri"], fixed=z[name + "__fixed"],
                     global_parameters=ast.literal_eval(str(z[name + "__gp"])),
                     vertex_options=ast.literal_eval(str(z[name + "__vopts"])), edges=z[name + "__edges"],
                     edge_options=ast.literal_eval(str(z[name + "__eopts"])))
    return z, mesh


@pytest.mark.parametrize("name", [str(n) for n in np.load(VGOLD)["names"]])
def test_volume_row_with_pins_matches_reference(name):
    """Mixed KKT of the volume row (dense, first) and the pin rows: the reference's projection, or its skip."""
    z, mesh = _vcase(name)
    X = mesh.positions_view().copy()
    progs = pins.programs(mesh, MODS)
    g = z[name + "__grad0"].copy()
    lane = pins.project_gradient(g, [z[name + "__vgrad"]], pins.rows(X, progs))
    np.testing.assert_allclose(g, z[name + "__grad1"], rtol=0, atol=1e-13)
    untouched = np.array_equal(z[name + "__grad0"], z[name + "__grad1"])
    assert lane == ("skip" if untouched else "project")
    # the decision the device takes, with the host's own volume gradient as the dense row
    from membrane_solver_amd.runtime.minimizer import _volume_gradient

    vg = _volume_gradient(mesh, X)
    np.testing.assert_allclose(vg, z[name + "__vgrad"], rtol=0, atol=1e-14)
    t = pins.device_tables(X, progs, [vg])
    assert t.lane == lane
    if t.lane == "project":
        # device closed form: the pin null-space projector on g and on the volume row, then the k = 1 row
        P = np.asarray(t.params).reshape(-1, 7)

        def proj(v):
            v = v.copy()
            for row, kind, k in zip(t.grad_row, t.grad_kind, t.grad_param):
                n = P[k, :3]
                if kind != pins.GRAD_RADIAL:
                    v[row] -= np.dot(v[row], n) * n
                if kind != pins.GRAD_PLANE:
                    rh = pins._radial_hat(X[row], n, P[k, 3:6])
                    v[row] -= np.dot(v[row], rh) * rh
            return v

        pg, pc = proj(z[name + "__grad0"]), proj(vg)
        pg -= (np.sum(pg * pc) / np.sum(pc * pc)) * pc
        np.testing.assert_allclose(pg, z[name + "__grad1"], rtol=0, atol=1e-12)
    ConstraintModuleManager(MODS).enforce_all(mesh, global_params=mesh.global_parameters, context="minimize")
    np.testing.assert_allclose(mesh.positions_view(), z[name + "__positions1"], rtol=0, atol=1e-13)


# ---- every reference deck that uses pins (tests/golden/pin_deck_decisions.npz) ------------------------------------
DGOLD = os.path.join(os.path.dirname(__file__), "golden", "pin_deck_decisions.npz")


@pytest.mark.parametrize("key", [str(k) for k in np.load(DGOLD)["keys"]])
def test_deck_decision_matches_reference(key):
    """Row count, rank and project-or-skip of the reference on each deck, repeated by the resolver on the deck's
    pinned vertices (the volume row's part elsewhere folded into one extra row of the same norm)."""
    z = np.load(DGOLD)
    X = z[key + "__positions"]
    mesh = ArrayMesh(X, np.zeros((0, 3), np.int32), fixed=z[key + "__fixed"],
                     global_parameters=ast.literal_eval(str(z[key + "__gp"])),
                     vertex_options=ast.literal_eval(str(z[key + "__vopts"])), edges=z[key + "__edges"],
                     edge_options=ast.literal_eval(str(z[key + "__eopts"])))
    cons = [str(c) for c in z[key + "__cons"] if str(c) != "volume"]
    dense = [z[key + "__vgrad"]] if bool(z[key + "__has_volume"]) else []
    try:
        t = pins.device_tables(X, pins.programs(mesh, cons), dense)
    except L.MembraneHipError as e:
        # out of scope on the device by design (fit mode, a fitted slide normal) -- never the full-rank raise
        assert "two constraints" not in str(e), (str(z[key + "__name"]), e)
        assert "fit" in str(e), (str(z[key + "__name"]), e)
        return
    assert (t.lane, t.n_rows, t.rank) == (str(z[key + "__decision"]), int(z[key + "__n_rows"]),
                                          int(z[key + "__rank"])), str(z[key + "__name"])


def test_deck_decisions_cover_the_issue_table():
    z = np.load(DGOLD)
    got = {str(z[k + "__name"]): (str(z[k + "__decision"]), int(z[k + "__n_rows"]), int(z[k + "__rank"]))
           for k in (str(k) for k in z["keys"])}
    assert got["meshes/caveolin/kozlov_1disk_3d_tensionless_single_leaflet_profile_hard_rim_R12.yaml"] == ("skip", 96, 72)
    assert got["meshes/caveolin/annulus_flat_no_tilt.yaml"][0] == "project"
    assert got["meshes/catenoid.json"][0] == "none"


def test_volume_listed_before_pins_raises():
    from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager
    from membrane_solver_amd.runtime.minimizer import Minimizer
    from membrane_solver_amd.runtime.steppers import GradientDescent

    z, mesh = _vcase("volume_plane_fixed")
    with pytest.raises(L.MembraneHipError, match="before"):
        Minimizer(mesh, mesh.global_parameters, GradientDescent(), EnergyModuleManager(["surface"]),
                  ConstraintModuleManager(["volume", "pin_to_plane"]), energy_modules=["surface"],
                  constraint_modules=["volume", "pin_to_plane"])
