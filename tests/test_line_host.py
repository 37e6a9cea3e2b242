"""line_tension, host side (no GPU): the tags and gamma resolve as modules/energy/line_tension.py:24-34 and :117-124
resolve them, the device tables come out in the stated order with the row permutation applied, the reference fixtures
are self-consistent, the module is refused where the device path does not run it, and the header, the library and
the Python signatures agree on the new entry points."""

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
from membrane_solver_amd.modules.energy import line_tension as mod
from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager
from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager
from membrane_solver_amd.runtime.minimizer import Minimizer
from membrane_solver_amd.runtime.steppers import GradientDescent

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TRAJ = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLD, "traj_*_line_*.npz")))

# a tetrahedron: six edges
P4 = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
T4 = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], dtype=np.int32)
E4 = np.array([[0, 2], [2, 1], [1, 0], [1, 3], [3, 0], [2, 3]])


def _mesh(gp, eopts, edges=E4):
    return ArrayMesh(P4, T4, global_parameters=gp, edges=edges, edge_options=eopts, energy_modules=["line_tension"])


@pytest.mark.parametrize("opts,tagged", [
    ({"energy": "line_tension"}, True),
    ({"energy": "surface"}, False),
    ({"energy": ["surface", "line_tension"]}, True),
    ({"energy": ("line_tension",)}, True),
    ({"energy": ["surface"]}, False),
    ({"line_tension": 2.0}, True),            # the key alone
    ({"line_tension": 0.0}, True),            # ... whatever its value: tagged, then skipped for its gamma
    ({"energy": {"line_tension"}}, False),    # a set is neither a string nor a list / tuple
    ({"constraints": ["pin_to_plane"]}, False),
    ({}, False),
    (None, False),
])
def test_edge_tag(opts, tagged):
    assert mod.edge_is_tagged(opts) is tagged


def test_gamma_resolution_and_order():
    eo = {0: {"energy": "line_tension"},                         # global gamma
          1: {"energy": "line_tension", "line_tension": 2.5},   # per-edge override
          2: {"line_tension": 0.75},                            # key alone
          3: {"energy": "line_tension", "line_tension": 0.0},   # gamma 0: skipped
          4: {"energy": "line_tension", "line_tension": None},  # falsy: skipped
          5: {"energy": "surface"}}                             # not tagged
    m = _mesh({"line_tension": 1.5}, eo)
    tail, head, gamma, num = mod.tagged_edges(m, m.global_parameters)
    assert num.tolist() == [0, 1, 2]
    assert tail.tolist() == [0, 2, 1] and head.tolist() == [2, 1, 0]
    assert gamma.tolist() == [1.5, 2.5, 0.75]
    # no global parameter: only the edges with a gamma of their own are charged
    m = _mesh({}, eo)
    assert mod.tagged_edges(m, m.global_parameters)[3].tolist() == [1, 2]
    m = _mesh({"line_tension": 0.0}, eo)
    assert mod.tagged_edges(m, m.global_parameters)[3].tolist() == [1, 2]
    # nothing tagged, or no edge table at all: nothing charged
    m = _mesh({"line_tension": 1.0}, {})
    assert len(mod.tagged_edges(m, m.global_parameters)[0]) == 0
    m = ArrayMesh(P4, T4, global_parameters={"line_tension": 1.0})
    assert len(mod.tagged_edges(m, m.global_parameters)[0]) == 0


def test_reference_style_mesh_resolves_the_same_way():
    """a mesh with .vertices / .edges dictionaries (the reference's entities) goes through the same resolution"""
    V = {i: types.SimpleNamespace(options={}, fixed=False) for i in (10, 11, 12)}
    E = {1: types.SimpleNamespace(tail_index=10, head_index=11, options={"energy": "line_tension"}),
         2: types.SimpleNamespace(tail_index=11, head_index=12, options={"line_tension": 3.0}),
         3: types.SimpleNamespace(tail_index=12, head_index=10, options={})}
    m = types.SimpleNamespace(vertices=V, edges=E, vertex_index_to_row={10: 0, 11: 1, 12: 2},
                              fixed_mask=np.zeros(3, bool))
    tail, head, gamma, _num = mod.tagged_edges(m, {"line_tension": 0.5})
    assert tail.tolist() == [0, 1] and head.tolist() == [1, 2] and gamma.tolist() == [0.5, 3.0]


def test_device_tables_order_and_permutation():
    """The library's own table builder (the code ms_set_line_tension runs): gamma == 0 dropped, edges in ascending
    order, iperm applied to both ends, CSR rows ascending with each row's edges in ascending edge order."""
    L.build()
    nv = 6
    iperm = np.array([3, 5, 0, 1, 4, 2], dtype=np.int32)  # external row -> library row
    tail = np.array([0, 1, 2, 3, 0], dtype=np.int32)
    head = np.array([1, 2, 0, 4, 3], dtype=np.int32)
    gamma = np.array([1.0, 2.0, 0.0, 4.0, 5.0])
    t = mod.host_tables(nv, iperm, tail, head, gamma)
    keep = [0, 1, 3, 4]
    assert t["tail"].tolist() == iperm[tail[keep]].tolist() == [3, 5, 1, 3]
    assert t["head"].tolist() == iperm[head[keep]].tolist() == [5, 0, 4, 1]
    assert t["gamma"].tolist() == [1.0, 2.0, 4.0, 5.0]
    assert t["vrow"].tolist() == [0, 1, 3, 4, 5]
    assert t["off"].tolist() == [0, 1, 3, 5, 6, 8]
    # row 0: edge 1 (other 5); row 1: edges 2, 3 (others 4, 3); row 3: edges 0, 3 (5, 1); row 4: edge 2 (1);
    # row 5: edges 0, 1 (3, 0)
    assert t["other"].tolist() == [5, 4, 3, 5, 1, 1, 3, 0]
    assert t["csr_gamma"].tolist() == [2.0, 4.0, 5.0, 1.0, 5.0, 4.0, 1.0, 2.0]
    # every kept edge appears once from each end
    assert len(t["other"]) == 2 * len(keep)
    for bad_tail in (-1, nv):
        with pytest.raises(L.MembraneHipError, match="out of range"):
            mod.host_tables(nv, iperm, np.array([bad_tail], np.int32), np.array([0], np.int32), np.array([1.0]))
    with pytest.raises(L.MembraneHipError, match="out of range"):
        mod.host_tables(nv, iperm, np.array([0], np.int32), np.array([nv], np.int32), np.array([1.0]))
    with pytest.raises(L.MembraneHipError, match="finite"):
        mod.host_tables(nv, iperm, np.array([0], np.int32), np.array([1], np.int32), np.array([np.nan]))
    empty = mod.host_tables(nv, iperm, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0))
    assert len(empty["tail"]) == 0 and empty["off"].tolist() == [0]


def test_edge_outside_the_triangulation_is_refused():
    mod.check_triangle_sides(T4, 4, E4[:, 0], E4[:, 1])
    mod.check_triangle_sides(T4, 4, E4[:, 1], E4[:, 0])  # either orientation
    P = np.vstack([P4, [[2.0, 2, 2]]])
    with pytest.raises(L.MembraneHipError, match="not a side of any triangle"):
        mod.check_triangle_sides(T4, 5, [0, 1], [2, 4], numbers=[7, 9])
    mesh = ArrayMesh(P, T4, global_parameters={"line_tension": 1.0}, edges=[[1, 4]],
                     edge_options={0: {"energy": "line_tension"}}, energy_modules=["line_tension"])
    dm = types.SimpleNamespace(nv=5, set_line_tension=lambda *a: pytest.fail("must not reach the device"))
    with pytest.raises(L.MembraneHipError, match="edge 0"):
        mod.upload(mesh, mesh.global_parameters, dm)


def _line_energy_numpy(P, edges, eopts, gp):
    """line_tension.py:117-138 in NumPy"""
    E, g = 0.0, np.zeros_like(P)
    for k, (t, h) in enumerate(edges):
        o = eopts.get(k)
        if not mod.edge_is_tagged(o):
            continue
        gamma = o.get("line_tension", float(gp.get("line_tension", 0.0) or 0.0))
        if not gamma:
            continue
        vec = P[h] - P[t]
        ln = float(np.linalg.norm(vec))
        if ln < 1e-15:
            continue
        E += float(gamma) * ln
        g[t] -= float(gamma) * vec / ln
        g[h] += float(gamma) * vec / ln
    return E, g


def test_line_cases_are_self_consistent():
    z = np.load(os.path.join(GOLD, "line_cases.npz"))
    names = [str(n) for n in z["names"]]
    assert names == ["disk5_rim_global", "ico4_loop_mixed", "ico4_all_edges", "ico8_all_edges",
                     "ico4_loop_coincident", "ico4_nothing_tagged"]
    for name in names:
        P, T, edges = z[name + "__positions"], z[name + "__tri"], z[name + "__edges"]
        eo, gp = ast.literal_eval(str(z[name + "__eopts"])), ast.literal_eval(str(z[name + "__gp"]))
        mesh = ArrayMesh(P, T, global_parameters=gp, edges=edges, edge_options=eo, energy_modules=["line_tension"])
        tail, head, gamma, num = mod.tagged_edges(mesh, mesh.global_parameters)
        assert len(tail) == int(z[name + "__n_charged"]), name
        mod.check_triangle_sides(T, len(P), tail, head, num)
        E, g = _line_energy_numpy(P, edges, eo, gp)
        E_ref, g_ref = float(z[name + "__energy"]), z[name + "__grad"]
        assert abs(E - E_ref) <= 1e-13 * max(abs(E_ref), 1.0), name
        assert np.abs(g - g_ref).max() <= 1e-13 * max(np.abs(g_ref).max(), 1.0), name
    assert int(z["disk5_rim_global__n_charged"]) == 30
    assert int(z["ico4_loop_mixed__n_charged"]) == 21 and len(ast.literal_eval(str(z["ico4_loop_mixed__eopts"]))) == 22
    assert int(z["ico8_all_edges__n_charged"]) == 1920 > 256 * 5  # more 256-edge blocks than tiles at tile 256
    # the coincident pair: one edge of zero length among the charged ones
    P, edges = z["ico4_loop_coincident__positions"], z["ico4_loop_coincident__edges"]
    m = ArrayMesh(P, z["ico4_loop_coincident__tri"], global_parameters={"line_tension": 0.75}, edges=edges,
                  edge_options=ast.literal_eval(str(z["ico4_loop_coincident__eopts"])))
    t, h, _g, _n = mod.tagged_edges(m, m.global_parameters)
    assert int((np.linalg.norm(P[h] - P[t], axis=1) < 1e-15).sum()) == 1


@pytest.mark.parametrize("fname", TRAJ)
def test_trajectory_fixtures_load(fname):
    z = np.load(os.path.join(GOLD, fname))
    assert os.path.getsize(os.path.join(GOLD, fname)) <= 250 * 1024
    log = np.asarray(z["step_log"]).reshape(-1, 3)
    assert len(log) == int(z["n_steps"]) and log[:, 0].sum() >= 1
    assert "line_tension" in [str(s) for s in z["energy_modules"]]
    eo = ast.literal_eval(str(z["eopts"]))
    assert eo and max(eo) < len(z["edges"]) and all(mod.edge_is_tagged(o) for o in eo.values())
    assert float(ast.literal_eval(str(z["gp"]))["line_tension"]) > 0.0
    assert z["positions_final"].shape == z["positions0"].shape
    acc = log[log[:, 0] > 0, 2]
    assert np.all(np.diff(acc) <= 0.0)  # the accepted energies of a line search never rise
    if "cg_line" in fname:
        assert (log[:, 0] == 0).any()   # a non-descent restart
    if "backtrack" in fname:
        assert log[0, 1] < 1.5 * float(z["step_size0"])  # the first search did not accept its first trial


def test_there_are_six_trajectories():
    assert len(TRAJ) == 6, TRAJ


def _minimizer(mesh, energy):
    return Minimizer(mesh, mesh.global_parameters, GradientDescent(), EnergyModuleManager(energy),
                     ConstraintModuleManager([]), energy_modules=energy, constraint_modules=[], quiet=True)


@pytest.mark.parametrize("tilt", ["tilt", "bending_tilt", "tilt_smoothness", "tilt_in", "tilt_smoothness_out",
                                  "bending_tilt_in", "tilt_disk_target_out"])
def test_minimizer_refuses_the_module_next_to_tilt_modules(tilt):
    mesh = _mesh({"line_tension": 1.0}, {0: {"energy": "line_tension"}})
    with pytest.raises(L.MembraneHipError, match="line_tension together with tilt"):
        _minimizer(mesh, ["surface", "line_tension", tilt])
    _minimizer(mesh, ["surface", "bending", "volume", "body_area_penalty", "line_tension"])  # accepted by the wiring


def test_minimizer_refuses_the_module_on_a_mesh_without_edges():
    """An ArrayMesh built without edges= cannot tag anything: the deck stays refused, as it was before the module
    reached the device, and is not run with a line energy of zero.  An edge table with nothing tagged is the
    reference's "energy 0, no gradient" and is accepted."""
    bare = ArrayMesh(P4, T4, global_parameters={"line_tension": 1.0}, energy_modules=["line_tension"])
    assert not mod.has_edge_table(bare) and mod.has_edge_table(_mesh({}, {}))
    with pytest.raises(L.MembraneHipError, match="'line_tension' on a mesh without an edge table"):
        _minimizer(bare, ["surface", "line_tension"])
    _minimizer(_mesh({"line_tension": 1.0}, {}), ["surface", "line_tension"])
    _minimizer(_mesh({"line_tension": 1.0}, {}, edges=np.zeros((0, 2), dtype=np.int64)), ["surface", "line_tension"])


def test_energy_manager_finds_the_plugin():
    m = EnergyModuleManager(["line_tension"]).get_module("line_tension")
    assert m is mod and callable(m.compute_energy_and_gradient) and callable(m.compute_energy_and_gradient_array)


def test_sharded_driver_refuses_the_module():
    from membrane_solver_amd.parallel import HipShardBackend

    with pytest.raises(L.MembraneHipError, match="line_tension module is not sharded"):
        HipShardBackend.configure(types.SimpleNamespace(), modules=L.MS_MOD_SURFACE | L.MS_MOD_LINE_TENSION)
    src = open(os.path.join(ROOT, "membrane_solver_amd", "csrc", "ms_api_shard.inc")).read()
    step = src[src.index("int ms_shard_step("):]
    assert "MS_MOD_LINE_TENSION" in step[:1400], "ms_shard_step must refuse the module before it queues anything"


def test_header_library_and_signatures_agree():
    L.build()
    hdr = open(os.path.join(ROOT, "include", "membrane_hip.h")).read()
    assert int(re.search(r"#define MS_MOD_LINE_TENSION (\d+)u", hdr).group(1)) == L.MS_MOD_LINE_TENSION == 131072
    assert int(re.search(r"MS_NSCAL = (\d+)", hdr).group(1)) == L.MS_NSCAL == 31  # no new reduction slot
    bits = [int(v) for v in re.findall(r"#define MS_(?:MOD|CON|TRACK)_[A-Z_]+ (\d+)u", hdr)]
    assert len(bits) == len(set(bits)) and all(b & (b - 1) == 0 for b in bits)
    L.lib()
    cd = ctypes.CDLL(L.LIB_PATH)
    for name in ("ms_set_line_tension", "ms_get_line_energy", "ms_line_stats"):
        assert re.search(r"\bint %s\(ms_ctx \*ctx" % name, hdr), name
        assert hasattr(cd, name) and name in L.SIGNATURES, name
    assert re.search(r"\bint ms_line_tables_host\(int nv", hdr) and hasattr(cd, "ms_line_tables_host")
    # every exported ms_* symbol is declared in the header and has a ctypes signature, and the other way round
    declared = set(re.findall(r"^(?:int|void|const char \*|ms_ctx \*)\s*(ms_[a-z0-9_]+)\(", hdr, flags=re.M))
    assert {"ms_set_line_tension", "ms_get_line_energy", "ms_line_stats", "ms_line_tables_host"} <= declared
    assert {"ms_set_line_tension", "ms_get_line_energy", "ms_line_stats", "ms_line_tables_host"} <= set(L.SIGNATURES)
