"""edge_length_penalty, host side (no GPU): the edges are selected and charged as modules/energy/edge_length_penalty.py
:16-22 and :35-47 do it (the reference's energies of tests/golden/edge_penalty_cases.npz are reproduced from
``charged_edges`` and a NumPy sum written here), the device tables come out in the stated order with the target length
on both ends, line_tension's tables are what they were, the module is refused where the device path does not run it,
and the header, the library and the Python signatures agree on the new entry points."""

import ast
import ctypes
import glob
import os
import re
import types

import numpy as np
import pytest

from membrane_solver_amd import _lib as L
from membrane_solver_amd.geometry.mesh import ArrayMesh
from membrane_solver_amd.modules.energy import edge_length_penalty as mod
from membrane_solver_amd.modules.energy import line_tension as line
from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager
from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager
from membrane_solver_amd.runtime.minimizer import Minimizer
from membrane_solver_amd.runtime.steppers import GradientDescent

from minimizer_stub import install_stub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TRAJ = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLD, "traj_*edgepen*.npz")))
CASES = ["ico4_third_untargeted", "ico8_all_edges", "disk5_rim_target_zero", "ico4_tag_and_target_mixed",
         "ico4_default_stiffness", "ico4_zero_stiffness", "ico4_one_edge_collapsed", "ico4_both_edge_modules"]

# a tetrahedron: six edges
P4 = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
T4 = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], dtype=np.int32)
E4 = np.array([[0, 2], [2, 1], [1, 0], [1, 3], [3, 0], [2, 3]])


def _mesh(gp, eopts, edges=E4, positions=P4):
    return ArrayMesh(positions, T4, global_parameters=gp, edges=edges, edge_options=eopts,
                     energy_modules=["edge_length_penalty"])


@pytest.mark.parametrize("opts,selected", [
    ({"energy": "edge_length_penalty"}, True),
    ({"energy": ["edge_length_penalty"]}, True),
    ({"energy": ["surface", "edge_length_penalty"]}, True),
    ({"energy": "surface"}, False),
    ({"energy": []}, False),
    ({"target_length": 1.0}, True),                          # the key alone
    ({"target_length": None}, True),                         # ... whatever its value: selected, then not charged
    ({"energy": "surface", "target_length": 0.0}, True),
    ({"energy": 3}, False),                                  # nothing that can hold the name: no error
    ({"constraints": ["pin_to_plane"]}, False),
    ({}, False),
    (None, False),
])
def test_edge_selection(opts, selected):
    assert mod.edge_is_selected(opts) is selected


def test_charged_edges_follow_the_target_not_the_tag():
    eo = {0: {"energy": "edge_length_penalty"},                            # tagged, no target: not charged
          1: {"energy": ["edge_length_penalty"], "target_length": None},   # target None: not charged
          2: {"target_length": 0.5},                                       # a target and no tag: charged
          3: {"energy": ["surface", "edge_length_penalty"], "target_length": 0.0},  # L0 = 0 is a target
          4: {"energy": "edge_length_penalty", "target_length": 2, "edge_stiffness": 7.0},
          5: {"energy": "surface"}}
    m = _mesh({"edge_stiffness": 12.5}, eo)
    tail, head, target, num = mod.charged_edges(m, m.global_parameters)
    assert num.tolist() == [2, 3, 4]
    assert tail.tolist() == [1, 1, 3] and head.tolist() == [0, 3, 0]
    assert target.tolist() == [0.5, 0.0, 2.0] and target.dtype == np.float64
    # k: the global parameter alone, 100 when absent; the edge's own option is not read
    assert mod.stiffness(m.global_parameters) == 12.5
    assert mod.stiffness({}) == 100.0 and mod.stiffness({"edge_stiffness": 0}) == 0.0
    # nothing targeted, or no edge table at all: nothing charged
    assert len(mod.charged_edges(_mesh({}, {}), {})[0]) == 0
    bare = ArrayMesh(P4, T4, global_parameters={})
    assert len(mod.charged_edges(bare, {})[0]) == 0


def test_reference_style_mesh_resolves_the_same_way():
    """a mesh with .vertices / .edges dictionaries (the reference's entities) goes through the same selection; an end
    without a row skips the edge"""
    V = {i: types.SimpleNamespace(options={}, fixed=False) for i in (10, 11, 12, 13)}
    E = {1: types.SimpleNamespace(tail_index=10, head_index=11, options={"energy": ["edge_length_penalty"],
                                                                         "target_length": 1.5}),
         2: types.SimpleNamespace(tail_index=11, head_index=12, options={"target_length": 0.25}),
         3: types.SimpleNamespace(tail_index=12, head_index=10, options={"energy": "edge_length_penalty"}),
         4: types.SimpleNamespace(tail_index=12, head_index=13, options={"target_length": 1.0}),
         5: types.SimpleNamespace(tail_index=10, head_index=12, options=None)}
    m = types.SimpleNamespace(vertices=V, edges=E, vertex_index_to_row={10: 0, 11: 1, 12: 2},
                              fixed_mask=np.zeros(3, bool))
    tail, head, target, num = mod.charged_edges(m, {})
    assert tail.tolist() == [0, 1] and head.tolist() == [1, 2] and target.tolist() == [1.5, 0.25]
    assert num.tolist() == [0, 1]


def _penalty_numpy(P, tail, head, target, k):
    """edge_length_penalty.py:49-67 over the charged edges, in NumPy"""
    vec = P[head] - P[tail]
    ln = np.linalg.norm(vec, axis=1)
    ok = ln >= 1e-15
    delta = ln[ok] - target[ok]
    E = float(np.sum(0.5 * k * delta ** 2))
    g = np.zeros_like(P)
    force = (k * delta / ln[ok])[:, None] * vec[ok]
    np.add.at(g, head[ok], force)
    np.add.at(g, tail[ok], -force)
    return E, g, int((~ok).sum())


def test_cases_reproduce_the_reference_from_charged_edges():
    """The selection, the default k and the skip rules: ``charged_edges`` plus the sum above gives the reference's
    energy of every case to 1e-12 relative (and its gradient to 1e-12 of max|g|)."""
    z = np.load(os.path.join(GOLD, "edge_penalty_cases.npz"))
    assert [str(n) for n in z["names"]] == CASES
    skipped = {}
    for name in CASES:
        P, T, edges = z[name + "__positions"], z[name + "__tri"], z[name + "__edges"]
        eo, gp = ast.literal_eval(str(z[name + "__eopts"])), ast.literal_eval(str(z[name + "__gp"]))
        mesh = ArrayMesh(P, T, global_parameters=gp, edges=edges, edge_options=eo,
                         energy_modules=["edge_length_penalty"])
        tail, head, target, num = mod.charged_edges(mesh, mesh.global_parameters)
        assert len(tail) == int(z[name + "__n_charged"]), name
        mod.check_triangle_sides(T, len(P), tail, head, num)
        E, g, skipped[name] = _penalty_numpy(P, tail, head, target, mod.stiffness(mesh.global_parameters))
        E_ref, g_ref = float(z[name + "__energy"]), z[name + "__grad"]
        assert abs(E - E_ref) <= 1e-12 * abs(E_ref), (name, E, E_ref)
        assert np.abs(g - g_ref).max() <= 1e-12 * max(np.abs(g_ref).max(), 1e-300), name
    assert int(z["ico4_third_untargeted__n_charged"]) == 320 < len(z["ico4_third_untargeted__edges"]) == 480
    assert int(z["ico8_all_edges__n_charged"]) == 1920 > 256 * 5  # more 256-edge blocks than tiles at tile 256
    assert int(z["disk5_rim_target_zero__n_charged"]) == 30
    eo = ast.literal_eval(str(z["disk5_rim_target_zero__eopts"]))
    assert all(o["target_length"] == 0.0 for o in eo.values())
    mixed = ast.literal_eval(str(z["ico4_tag_and_target_mixed__eopts"]))
    tagged_no_target = [k for k, o in mixed.items() if mod.edge_is_selected(o) and o.get("target_length") is None]
    target_no_tag = [k for k, o in mixed.items() if "energy" not in o and o.get("target_length") is not None]
    assert len(tagged_no_target) >= 100 and len(target_no_tag) >= 50
    assert int(z["ico4_tag_and_target_mixed__n_charged"]) == sum(o.get("target_length") is not None for o in mixed.values())
    assert "edge_stiffness" not in ast.literal_eval(str(z["ico4_default_stiffness__gp"]))
    assert float(z["ico4_zero_stiffness__energy"]) == 0.0 and not z["ico4_zero_stiffness__grad"].any()
    assert skipped["ico4_one_edge_collapsed"] == 1 and sum(skipped.values()) == 1
    both = ast.literal_eval(str(z["ico4_both_edge_modules__eopts"]))
    assert all(line.edge_is_tagged(o) and mod.edge_is_selected(o) for o in both.values())
    assert float(z["ico4_both_edge_modules__energy_line"]) > 0.0


def test_device_tables_order_and_permutation():
    """The library's own table builder (the code ms_set_edge_length_penalty runs): edges in ascending order, iperm
    applied to both ends, CSR rows ascending with each row's edges in ascending edge order and the edge's L0 on both
    of its ends; L0 == 0 is kept; k == 0 and nothing targeted give empty tables."""
    L.build()
    nv = 6
    iperm = np.array([3, 5, 0, 1, 4, 2], dtype=np.int32)  # external row -> library row
    tail = np.array([0, 1, 2, 3, 0], dtype=np.int32)
    head = np.array([1, 2, 0, 4, 3], dtype=np.int32)
    l0 = np.array([1.0, 2.0, 0.0, 4.0, 5.0])
    t = mod.host_tables(nv, iperm, tail, head, l0, 30.0)
    assert t["tail"].tolist() == iperm[tail].tolist() == [3, 5, 0, 1, 3]
    assert t["head"].tolist() == iperm[head].tolist() == [5, 0, 3, 4, 1]
    assert t["l0"].tolist() == [1.0, 2.0, 0.0, 4.0, 5.0]
    assert t["vrow"].tolist() == [0, 1, 3, 4, 5]
    assert np.all(np.diff(t["vrow"]) > 0)
    assert t["off"].tolist() == [0, 2, 4, 7, 8, 10]
    # row 0: edges 1, 2 (others 5, 3); row 1: edges 3, 4 (4, 3); row 3: edges 0, 2, 4 (5, 0, 1); row 4: edge 3 (1);
    # row 5: edges 0, 1 (3, 0)
    assert t["other"].tolist() == [5, 3, 4, 3, 5, 0, 1, 1, 3, 0]
    assert t["csr_l0"].tolist() == [2.0, 0.0, 4.0, 5.0, 1.0, 0.0, 5.0, 4.0, 1.0, 2.0]
    # every edge appears once from each end, with its own L0
    assert sorted(t["csr_l0"].tolist()) == sorted(2 * l0.tolist())
    zero_k = mod.host_tables(nv, iperm, tail, head, l0, 0.0)
    assert len(zero_k["tail"]) == 0 and len(zero_k["vrow"]) == 0 and zero_k["off"].tolist() == [0]
    empty = mod.host_tables(nv, iperm, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0), 30.0)
    assert len(empty["tail"]) == 0 and empty["off"].tolist() == [0]
    one = np.array([0], np.int32)
    for bad in (-1, nv):
        with pytest.raises(L.MembraneHipError, match="out of range"):
            mod.host_tables(nv, iperm, np.array([bad], np.int32), one, np.array([1.0]), 30.0)
        with pytest.raises(L.MembraneHipError, match="out of range"):
            mod.host_tables(nv, iperm, one, np.array([bad], np.int32), np.array([1.0]), 30.0)
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(L.MembraneHipError, match="target_length must be finite"):
            mod.host_tables(nv, iperm, one, np.array([1], np.int32), np.array([bad]), 30.0)
        with pytest.raises(L.MembraneHipError, match="edge_stiffness must be finite"):
            mod.host_tables(nv, iperm, one, np.array([1], np.int32), np.array([1.0]), bad)
    with pytest.raises(L.MembraneHipError, match="target_length must be finite"):  # (refused with k == 0 as well)
        mod.host_tables(nv, iperm, one, np.array([1], np.int32), np.array([np.nan]), 0.0)


def test_tables_of_the_fixtures_match_a_numpy_construction():
    """On the all-edges fixture under a scrambled row permutation: the edge table is the input in order, and the CSR
    is the stable sort of the (row, edge) incidences."""
    L.build()
    z = np.load(os.path.join(GOLD, "edge_penalty_cases.npz"))
    name = "ico8_all_edges"
    P, edges = z[name + "__positions"], z[name + "__edges"]
    mesh = ArrayMesh(P, z[name + "__tri"], global_parameters=ast.literal_eval(str(z[name + "__gp"])), edges=edges,
                     edge_options=ast.literal_eval(str(z[name + "__eopts"])))
    tail, head, target, _num = mod.charged_edges(mesh, mesh.global_parameters)
    nv = len(P)
    iperm = np.random.default_rng(3).permutation(nv).astype(np.int32)
    t = mod.host_tables(nv, iperm, tail, head, target, 25.0)
    a, b = iperm[tail], iperm[head]
    assert np.array_equal(t["tail"], a) and np.array_equal(t["head"], b) and np.array_equal(t["l0"], target)
    row = np.stack([a, b], axis=1).reshape(-1)         # incidences in edge order, tail end first
    oth = np.stack([b, a], axis=1).reshape(-1)
    col = np.repeat(target, 2)
    order = np.argsort(row, kind="stable")
    assert np.array_equal(t["vrow"], np.unique(row))
    assert np.array_equal(t["off"], np.concatenate([[0], np.cumsum(np.bincount(row)[np.unique(row)])]))
    assert np.array_equal(t["other"], oth[order]) and np.array_equal(t["csr_l0"], col[order])


def test_line_tension_tables_are_unchanged():
    """The shared builder still gives line_tension exactly its tables: on every line fixture, under a scrambled row
    permutation, ms_line_tables_host equals a NumPy construction of the documented layout (gamma == 0 dropped)."""
    L.build()
    z = np.load(os.path.join(GOLD, "line_cases.npz"))
    for name in [str(n) for n in z["names"]]:
        P = z[name + "__positions"]
        mesh = ArrayMesh(P, z[name + "__tri"], global_parameters=ast.literal_eval(str(z[name + "__gp"])),
                         edges=z[name + "__edges"], edge_options=ast.literal_eval(str(z[name + "__eopts"])))
        tail, head, gamma, _n = line.tagged_edges(mesh, mesh.global_parameters)
        if len(tail):  # (one uncharged edge among them: the builder drops it)
            gamma = gamma.copy()
            gamma[len(gamma) // 2] = 0.0
        nv = len(P)
        iperm = np.random.default_rng(5).permutation(nv).astype(np.int32)
        t = line.host_tables(nv, iperm, tail, head, gamma)
        keep = gamma != 0.0
        a, b, gk = iperm[tail[keep]], iperm[head[keep]], gamma[keep]
        assert np.array_equal(t["tail"], a) and np.array_equal(t["head"], b) and np.array_equal(t["gamma"], gk)
        row = np.stack([a, b], axis=1).reshape(-1)
        oth = np.stack([b, a], axis=1).reshape(-1)
        order = np.argsort(row, kind="stable")
        assert np.array_equal(t["vrow"], np.unique(row)), name
        assert np.array_equal(t["other"], oth[order]) and np.array_equal(t["csr_gamma"], np.repeat(gk, 2)[order]), name
        assert t["off"][-1] == 2 * len(a) and len(t["off"]) == len(t["vrow"]) + 1
        assert set(t) == {"tail", "head", "gamma", "vrow", "off", "other", "csr_gamma"}


def test_edge_outside_the_triangulation_is_refused():
    mod.check_triangle_sides(T4, 4, E4[:, 0], E4[:, 1])
    mod.check_triangle_sides(T4, 4, E4[:, 1], E4[:, 0])  # either orientation
    P = np.vstack([P4, [[2.0, 2, 2]]])
    with pytest.raises(L.MembraneHipError, match="edge_length_penalty: charged edge 9 .* not a side of any triangle"):
        mod.check_triangle_sides(T4, 5, [0, 1], [2, 4], numbers=[7, 9])
    mesh = ArrayMesh(P, T4, global_parameters={}, edges=[[1, 4]], edge_options={0: {"target_length": 1.0}},
                     energy_modules=["edge_length_penalty"])
    dm = types.SimpleNamespace(nv=5, set_edge_length_penalty=lambda *a: pytest.fail("must not reach the device"))
    with pytest.raises(L.MembraneHipError, match="edge_length_penalty: charged edge 0"):
        mod.upload(mesh, mesh.global_parameters, dm)


@pytest.mark.parametrize("gp,target", [({"edge_stiffness": np.inf}, 1.0), ({"edge_stiffness": np.nan}, 1.0),
                                       ({}, np.nan), ({"edge_stiffness": 0.0}, np.inf)])
def test_non_finite_input_is_refused_before_the_device(gp, target):
    mesh = _mesh(gp, {0: {"target_length": target}})
    dm = types.SimpleNamespace(nv=4, set_edge_length_penalty=lambda *a: pytest.fail("must not reach the device"))
    with pytest.raises(L.MembraneHipError, match="must be finite"):
        mod.upload(mesh, mesh.global_parameters, dm)


def test_upload_clears_the_tables_when_nothing_is_charged():
    calls = []
    dm = types.SimpleNamespace(nv=4, set_edge_length_penalty=lambda *a: calls.append(a))
    assert mod.upload(_mesh({}, {0: {"energy": "edge_length_penalty"}}), {}, dm) is False  # a tag and no target
    assert mod.upload(_mesh({"edge_stiffness": 0.0}, {0: {"target_length": 1.0}}), {"edge_stiffness": 0.0}, dm) is False
    assert calls == [(), ()]
    m = _mesh({}, {0: {"target_length": 1.0}, 4: {"target_length": 0.0}})
    assert mod.upload(m, m.global_parameters, dm) is True
    t, h, l0, k = calls[2]
    assert t.tolist() == [0, 3] and h.tolist() == [2, 0] and l0.tolist() == [1.0, 0.0] and k == 100.0


@pytest.mark.parametrize("fname", TRAJ)
def test_trajectory_fixtures_load(fname):
    z = np.load(os.path.join(GOLD, fname))
    assert os.path.getsize(os.path.join(GOLD, fname)) <= 250 * 1024
    log = np.asarray(z["step_log"]).reshape(-1, 3)
    assert len(log) == int(z["n_steps"]) and log[:, 0].sum() >= 3
    mods = [str(s) for s in z["energy_modules"]]
    assert "edge_length_penalty" in mods
    eo = ast.literal_eval(str(z["eopts"]))
    assert eo and max(eo) < len(z["edges"]) and all(o["target_length"] is not None for o in eo.values())
    assert z["positions_final"].shape == z["positions0"].shape
    acc = log[log[:, 0] > 0, 2]
    assert np.all(np.diff(acc) <= 0.0)  # the accepted energies of a line search never rise
    if "backtrack" in fname:
        assert log[0, 1] < 1.5 * float(z["step_size0"])  # the first search did not accept its first trial
    if "strip" in fname:  # the folding deck's sheet: every edge at its target before the perturbation, no surface module
        assert mods == ["bending", "edge_length_penalty"] and int(z["fixed"].sum()) == 2
        assert len(eo) == len(z["edges"]) and str(z["stepper"]) == "GradientDescent"
        assert ast.literal_eval(str(z["gp"]))["spontaneous_curvature"] == 2.0
    if "linetension" in fname:
        assert mods == ["surface", "line_tension", "edge_length_penalty"]
        assert [str(s) for s in z["constraint_modules"]] == ["pin_to_plane"]
        assert all(line.edge_is_tagged(o) for o in eo.values())


def test_there_are_six_trajectories():
    assert TRAJ == ["traj_disk5_gd_edgepen_linetension_surface_pins_plane.npz",
                    "traj_ico4_cg_edgepen_bending_volume_row.npz",
                    "traj_ico4_gd_edgepen_bending_volume_enforcer.npz",
                    "traj_ico4_gd_edgepen_surface_backtrack.npz",
                    "traj_ico8_cg_edgepen_bending_volume_row.npz",
                    "traj_strip_gd_bending_edgepen.npz"]


def _minimizer(mesh, energy):
    return Minimizer(mesh, mesh.global_parameters, GradientDescent(), EnergyModuleManager(energy),
                     ConstraintModuleManager([]), energy_modules=energy, constraint_modules=[], quiet=True)


@pytest.mark.parametrize("tilt", ["tilt", "bending_tilt", "tilt_smoothness", "tilt_in", "tilt_smoothness_out",
                                  "bending_tilt_in", "tilt_disk_target_out"])
def test_minimizer_refuses_the_module_next_to_tilt_modules(tilt):
    mesh = _mesh({}, {0: {"target_length": 1.0}})
    with pytest.raises(L.MembraneHipError, match="edge_length_penalty together with tilt"):
        _minimizer(mesh, ["surface", "edge_length_penalty", tilt])
    # accepted by the wiring, next to the other edge module as well
    _minimizer(mesh, ["surface", "bending", "volume", "body_area_penalty", "line_tension", "edge_length_penalty"])


def test_minimizer_refuses_the_module_on_a_mesh_without_edges():
    """An ArrayMesh built without edges= cannot carry a target: the deck stays refused, as it was before the module
    reached the device, and is not run with a penalty of zero.  An edge table with nothing targeted is the reference's
    "energy 0, no gradient" and is accepted."""
    bare = ArrayMesh(P4, T4, global_parameters={}, energy_modules=["edge_length_penalty"])
    with pytest.raises(L.MembraneHipError, match="'edge_length_penalty' on a mesh without an edge table"):
        _minimizer(bare, ["bending", "edge_length_penalty"])
    _minimizer(_mesh({}, {}), ["bending", "edge_length_penalty"])
    _minimizer(_mesh({}, {}, edges=np.zeros((0, 2), dtype=np.int64)), ["bending", "edge_length_penalty"])


def test_minimizer_refuses_approx_bending_gradient_on_an_open_mesh(monkeypatch):
    """bending.py:165-166 zeroes the boundary rows of what the modules listed before it accumulated; the device adds
    the penalty's rows behind the whole gradient pass, so the combination is refused (as it is for line_tension).  The
    device is stood in for: the refusal is taken before anything but the tables is handed to it."""
    dm, _mir = install_stub(monkeypatch)
    gp = {"bending_modulus": 1.0, "bending_gradient_mode": "approx"}
    eo = {0: {"target_length": 0.5}}
    open_mesh = ArrayMesh(P4, T4[:3], global_parameters=gp, edges=E4, edge_options=eo,
                          energy_modules=["edge_length_penalty", "bending"])
    mz = _minimizer(open_mesh, ["edge_length_penalty", "bending"])
    with pytest.raises(L.MembraneHipError, match="edge_length_penalty with bending_gradient_mode=approx on an open"):
        mz._device()
    uploads = [c[1] for c in dm.calls if c[0] == "set_edge_length_penalty"]
    assert len(uploads) == 1 and len(uploads[0]) == 4  # (the edge was charged: the bit was on when it was refused)
    assert not [c for c in dm.calls if c[0] not in ("sync", "set_edge_length_penalty")]  # (nothing but the tables)
    # nothing charged: the module's bit stays off and there is nothing to refuse on its account
    idle = ArrayMesh(P4, T4[:3], global_parameters=gp, edges=E4, edge_options={0: {"energy": "edge_length_penalty"}},
                     energy_modules=["edge_length_penalty", "bending"])
    mz = _minimizer(idle, ["edge_length_penalty", "bending"])
    try:
        mz._device()
    except L.MembraneHipError as exc:
        pytest.fail(f"refused with nothing charged: {exc}")
    assert dm.modules == L.MS_MOD_BENDING  # (past the refusals: the parameters were set, without the module's bit)


class _FakeDevice:
    """what compute_energy_breakdown and the approx-mode refusal read of a DeviceMesh"""

    def __init__(self, modules, e0, line_e, pen_e):
        self.modules, self._e, self._line, self._pen = modules, np.array([e0, 2.0, 0.0, 0.0]), line_e, pen_e

    def energy(self):
        return self._e

    def line_energy(self):
        return self._line

    def edge_penalty_energy(self):
        return self._pen


def test_breakdown_arithmetic(monkeypatch):
    """energies[0] is surface + line tension + edge length penalty: each module reports its own share, a module whose
    bit is off reports 0 and is not asked for its energy."""
    mesh = _mesh({"line_tension": 1.0}, {0: {"target_length": 1.0, "energy": ["line_tension"]}})
    mz = _minimizer(mesh, ["surface", "bending", "line_tension", "edge_length_penalty"])
    S, LT, EP = L.MS_MOD_SURFACE | L.MS_MOD_BENDING, L.MS_MOD_LINE_TENSION, L.MS_MOD_EDGE_LENGTH_PENALTY
    mz._const_energy = {}
    monkeypatch.setattr(mz, "_device", lambda: (None, _FakeDevice(S | LT | EP, 10.0, 3.0, 0.5)))
    assert mz.compute_energy_breakdown() == {"surface": 6.5, "bending": 2.0, "line_tension": 3.0,
                                             "edge_length_penalty": 0.5}
    off = _FakeDevice(S | EP, 10.0, None, 0.5)
    off.line_energy = lambda: pytest.fail("line_tension is off: its energy is not read")
    monkeypatch.setattr(mz, "_device", lambda: (None, off))
    assert mz.compute_energy_breakdown() == {"surface": 9.5, "bending": 2.0, "line_tension": 0.0,
                                             "edge_length_penalty": 0.5}
    mz2 = _minimizer(mesh, ["bending", "edge_length_penalty"])  # no surface module: slot 0 is the penalty alone
    mz2._const_energy = {}
    monkeypatch.setattr(mz2, "_device", lambda: (None, _FakeDevice(L.MS_MOD_BENDING | EP, 0.5, 0.0, 0.5)))
    assert mz2.compute_energy_breakdown() == {"bending": 2.0, "edge_length_penalty": 0.5}


def test_energy_manager_finds_the_plugin():
    m = EnergyModuleManager(["edge_length_penalty"]).get_module("edge_length_penalty")
    assert m is mod and callable(m.compute_energy_and_gradient) and callable(m.compute_energy_and_gradient_array)


def test_sharded_driver_refuses_the_module():
    from membrane_solver_amd.parallel import HipShardBackend

    with pytest.raises(L.MembraneHipError, match="edge_length_penalty module is not sharded"):
        HipShardBackend.configure(types.SimpleNamespace(), modules=L.MS_MOD_SURFACE | L.MS_MOD_EDGE_LENGTH_PENALTY)
    src = open(os.path.join(ROOT, "membrane_solver_amd", "csrc", "ms_api_shard.inc")).read()
    step = src[src.index("int ms_shard_step("):]
    assert "MS_MOD_EDGE_LENGTH_PENALTY" in step[:1600], "ms_shard_step must refuse the module before it queues anything"


def test_header_library_and_signatures_agree():
    L.build()
    hdr = open(os.path.join(ROOT, "include", "membrane_hip.h")).read()
    assert int(re.search(r"#define MS_MOD_EDGE_LENGTH_PENALTY (\d+)u", hdr).group(1)) == L.MS_MOD_EDGE_LENGTH_PENALTY == 262144
    assert L.MS_MOD_EDGE_LENGTH_PENALTY == 2 * L.MS_MOD_LINE_TENSION  # the next free bit
    assert int(re.search(r"MS_NSCAL = (\d+)", hdr).group(1)) == L.MS_NSCAL == 31  # no new reduction slot
    bits = [int(v) for v in re.findall(r"#define MS_(?:MOD|CON|TRACK)_[A-Z_]+ (\d+)u", hdr)]
    assert len(bits) == len(set(bits)) and all(b & (b - 1) == 0 for b in bits)
    L.lib()
    cd = ctypes.CDLL(L.LIB_PATH)
    new = {"ms_set_edge_length_penalty", "ms_get_edge_penalty_energy", "ms_edge_penalty_stats",
           "ms_edge_penalty_tables_host"}
    for name in new - {"ms_edge_penalty_tables_host"}:
        assert re.search(r"\bint %s\(ms_ctx \*ctx" % name, hdr), name
    assert re.search(r"\bint ms_edge_penalty_tables_host\(int nv", hdr)
    # each cites the reference routine it replaces (or says that it has none)
    for name in new:
        decl = hdr.index("int %s(" % name)
        comment = hdr[hdr.rindex("/*", 0, decl):decl]
        assert "edge_length_penalty.py:" in comment or "No reference counterpart" in comment, name
    # every exported ms_* symbol is declared in the header and has a ctypes signature, and the other way round
    declared = set(re.findall(r"^(?:int|void|const char \*|ms_ctx \*)\s*(ms_[a-z0-9_]+)\(", hdr, flags=re.M))
    assert new <= declared <= set(L.SIGNATURES)
    for name in declared:
        assert hasattr(cd, name), name
