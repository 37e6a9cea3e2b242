"""fixed_plane / perimeter without a GPU: a NumPy restatement of both reference modules against the enforcer fixtures
(tests/golden/enforce_only_cases.npz), the library's perimeter tables against a NumPy build of them, the ABI, the names
the Minimizer accepts, every refusal with its text, and the signed edge indices on both mesh kinds."""

import ast
import os
import re
import types

import numpy as np
import pytest

from membrane_solver_amd import _lib as L
from membrane_solver_amd import meshgen
from membrane_solver_amd.geometry.mesh import ArrayBody, ArrayMesh
from membrane_solver_amd.modules.constraints import fixed_plane, perimeter
from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager
from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager
from membrane_solver_amd.runtime.minimizer import Minimizer
from membrane_solver_amd.runtime.steppers import GradientDescent

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SYMBOLS = ("ms_set_fixed_plane", "ms_enforce_fixed_plane", "ms_set_perimeter", "ms_perimeter_tables_host",
           "ms_project_perimeter", "ms_enforce_only_stats")


@pytest.fixture(scope="module")
def cases():
    return dict(np.load(os.path.join(GOLD, "enforce_only_cases.npz")))


def np_perimeter(X, fixed, loop_off, tail, head, target, tol=1e-10, max_iter=3):
    """perimeter.enforce_constraint (perimeter.py:27-74) on arrays -> (positions, passes per loop, P per loop)."""
    X = np.array(X, dtype=float, copy=True)
    passes, per = [], []
    for l in range(len(target)):
        t, h = tail[loop_off[l]:loop_off[l + 1]], head[loop_off[l]:loop_off[l + 1]]
        n, P = 0, 0.0
        for _ in range(max_iter):
            vec = X[h] - X[t]
            ln = np.sqrt(np.einsum("ij,ij->i", vec, vec))
            P = 0.0
            for v in ln:
                P += v
            delta = P - target[l]
            if abs(delta) < tol:
                break
            g = {}
            for a, b, v, l_ in zip(t, h, vec, ln):
                if l_ < 1e-12:
                    continue
                g.setdefault(int(a), np.zeros(3))
                g.setdefault(int(b), np.zeros(3))
                g[int(a)] += -(v / l_)
                g[int(b)] += v / l_
            norm_sq = sum(float(np.dot(v, v)) for v in g.values())
            if norm_sq < 1e-18:
                break
            lam = delta / (norm_sq + 1e-18)
            for r, v in g.items():
                if not fixed[r]:
                    X[r] -= lam * v
            n += 1
        passes.append(n)
        per.append(P)
    return X, np.array(passes), np.array(per)


def np_fixed_plane(X, fixed, gp):
    """fixed_plane.enforce_constraint (fixed_plane.py:25-53) on arrays."""
    n = np.asarray(gp.get("fixed_plane_normal", (0.0, 0.0, 1.0)), dtype=float)
    q = np.asarray(gp.get("fixed_plane_point", (0.0, 0.0, 0.0)), dtype=float)
    n = n / np.linalg.norm(n)
    out = np.array(X, dtype=float, copy=True)
    free = ~np.asarray(fixed, dtype=bool)
    out[free] = X[free] - ((X[free] - q) @ n)[:, None] * n
    return out


def test_numpy_restatement_reproduces_every_perimeter_case(cases):
    z = cases
    names = [str(n) for n in z["perimeter_names"]]
    assert len(names) == 9
    for name in names:
        P, fixed = z[name + "__positions"], z[name + "__fixed"]
        X, passes, per = np_perimeter(P, fixed, z[name + "__loop_off"], z[name + "__tail"], z[name + "__head"], z[name + "__target"])
        assert np.array_equal(passes, z[name + "__passes"]), name
        np.testing.assert_allclose(per, z[name + "__perimeter"], rtol=0, atol=1e-12, err_msg=name)
        touched = z[name + "__touched"]
        np.testing.assert_allclose(X[touched], z[name + "__positions_touched"], rtol=0, atol=1e-13, err_msg=name)
        rest = np.setdiff1d(np.arange(len(P)), touched)
        assert np.array_equal(X[rest], P[rest]), name
        assert np.array_equal(X[fixed], P[fixed]), name
    # what the cases are there for
    assert z["perim_disk5_exhaust__passes"].tolist() != [0] and z["perim_disk5_zero_pass__passes"].tolist() == [0]
    assert len(z["perim_disk5_zero_pass__touched"]) == 0 and len(z["perim_disk5_single_zero__touched"]) == 0
    assert z["perim_disk48_rim__loop_off"][-1] == 288 > 256 and len(z["perim_disk48_rim__positions"]) == 7057
    assert len(z["perim_disk5_two_loops__target"]) == 2  # (the entry without a target is not a loop)
    assert "'target_perimeter'" in str(z["perim_disk5_two_loops__constraints"])
    t, h = z["perim_disk5_two_loops__tail"], z["perim_disk5_two_loops__head"]
    o = z["perim_disk5_two_loops__loop_off"]
    assert set(t[o[0]:o[1]]) & (set(t[o[1]:o[2]]) | set(h[o[1]:o[2]]))  # (the two loops share vertices)
    assert z["perim_disk12_rim_fixed7__fixed"].sum() == 67
    t, h = z["perim_disk5_duplicate__tail"], z["perim_disk5_duplicate__head"]
    assert len(set(zip(t.tolist(), h.tolist()))) == len(t) - 1
    P, t, h = z["perim_disk5_merged__positions"], z["perim_disk5_merged__tail"], z["perim_disk5_merged__head"]
    assert (np.linalg.norm(P[h] - P[t], axis=1) == 0.0).sum() == 1
    assert any(int(s) < 0 for s in ast.literal_eval(str(z["perim_disk5_rim__constraints"]))[0]["edges"])


def test_numpy_restatement_reproduces_every_fixed_plane_case(cases):
    z = cases
    names = [str(n) for n in z["fixed_plane_names"]]
    assert len(names) == 5
    for name in names:
        P, fixed, gp = z[name + "__positions"], z[name + "__fixed"], ast.literal_eval(str(z[name + "__gp"]))
        X = np_fixed_plane(P, fixed, gp)
        np.testing.assert_allclose(X, z[name + "__positions_final"], rtol=0, atol=1e-15, err_msg=name)
        assert np.array_equal(z[name + "__positions_final"][fixed], P[fixed]), name
        assert len(P) % 256 != 0
        if "fixed_plane_normal" not in gp:  # the default plane: exact zeros in z, x and y bit for bit
            F = z[name + "__positions_final"]
            assert not F[~fixed, 2].any() and np.array_equal(F[:, :2], P[:, :2]), name
    assert abs(np.linalg.norm(ast.literal_eval(str(z["fplane_disk12_oblique__gp"]))["fixed_plane_normal"]) - 1.0) > 0.01
    assert z["fplane_disk12_oblique_fixed__fixed"].any()


def np_tables(nv, iperm, loop_off, tail, head):
    """The layout include/membrane_hip.h documents for ms_perimeter_tables_host, built independently."""
    et, eh = iperm[tail], iperm[head]
    vert_off, vrow, csr_off, csr_ent = [0], [], [0], []
    for l in range(len(loop_off) - 1):
        seen, items = [], {}
        for i in range(loop_off[l], loop_off[l + 1]):
            for r, s in ((int(et[i]), -(i + 1)), (int(eh[i]), i + 1)):
                if r not in items:
                    seen.append(r)
                    items[r] = []
                items[r].append(s)
        for r in seen:
            vrow.append(r)
            csr_ent.extend(items[r])
            csr_off.append(len(csr_ent))
        vert_off.append(len(vrow))
    return {"tail": et, "head": eh, "vert_off": np.array(vert_off), "vrow": np.array(vrow, dtype=np.int64),
            "csr_off": np.array(csr_off), "csr_ent": np.array(csr_ent, dtype=np.int64)}


def test_perimeter_tables_match_a_numpy_build(cases):
    z = cases
    rng = np.random.default_rng(5)
    for name in ("perim_disk5_two_loops", "perim_disk5_duplicate", "perim_disk5_rim", "perim_disk48_rim", "perim_disk5_single_zero"):
        nv = len(z[name + "__positions"])
        off, tail, head = z[name + "__loop_off"], z[name + "__tail"], z[name + "__head"]
        for iperm in (np.arange(nv, dtype=np.int32), rng.permutation(nv).astype(np.int32)):
            got = perimeter.host_tables(nv, iperm, off, tail, head)
            want = np_tables(nv, iperm, off, tail, head)
            for k in want:
                assert np.array_equal(got[k], want[k]), (name, k)
    # an empty loop between two others, and no loop at all
    got = perimeter.host_tables(6, np.arange(6), [0, 2, 2, 3], [0, 1, 4], [1, 2, 5])
    assert got["vert_off"].tolist() == [0, 3, 3, 5] and got["csr_ent"].tolist() == [-1, 1, -2, 2, -3, 3]
    got = perimeter.host_tables(6, np.arange(6), [0], [], [])
    assert got["vert_off"].tolist() == [0] and len(got["vrow"]) == 0
    for bad_tail, bad_off, text in (([0, 6], [0, 2], "edge row out of range"), ([0, -1], [0, 2], "edge row out of range"),
                                    ([0, 1], [1, 2], r"loop_off\[0\] != 0"), ([0, 1], [0, 2, 1], "loop offsets decrease")):
        with pytest.raises(L.MembraneHipError, match=text):
            perimeter.host_tables(6, np.arange(6), bad_off, bad_tail, [1, 2])
    with pytest.raises(L.MembraneHipError, match="row permutation out of range"):
        perimeter.host_tables(6, [0, 1, 2, 3, 4, 9], [0, 1], [5], [0])


def test_abi_symbols():
    cd = L.lib()
    hdr = open(os.path.join(ROOT, "include", "membrane_hip.h")).read()
    for sym in SYMBOLS:
        assert hasattr(cd, sym) and sym in L.SIGNATURES, sym
        assert re.search(r"\bint %s\(" % sym, hdr), sym
    block = re.search(r"typedef struct ms_stepper_params \{(.*?)\} ms_stepper_params;", hdr, re.S).group(1)
    names = re.findall(r"^\s*(?:int|double)\s+(\w+);", block, re.M)
    assert "enforce_fixed_plane" in names and "enforce_perimeter" in names
    assert names == [f[0] for f in L.ms_stepper_params._fields_]
    sp = L.ms_stepper_params()
    assert sp.enforce_fixed_plane == 0 and sp.enforce_perimeter == 0  # (zero-initialised callers keep today's behaviour)


def _disk(n=3, edges=True, **kw):
    P, T, B = meshgen.disk_patch(n)
    e = None
    if edges:
        a = np.concatenate([T[:, 0], T[:, 1], T[:, 2]])
        b = np.concatenate([T[:, 1], T[:, 2], T[:, 0]])
        e = np.unique(np.stack([np.minimum(a, b), np.maximum(a, b)], axis=1), axis=0)
    return P, T, B, e, kw


def _mz(emods=("surface",), cons=("perimeter",), gp=None, edges=True, bodies=None):
    P, T, _B, e, _ = _disk(edges=edges)
    gp = dict({"surface_tension": 1.0}, **(gp or {}))
    mesh = ArrayMesh(P, T, global_parameters=gp, edges=e, bodies=bodies, energy_modules=list(emods),
                     constraint_modules=list(cons))
    return Minimizer(mesh, mesh.global_parameters, GradientDescent(), EnergyModuleManager(list(emods)),
                     ConstraintModuleManager(list(cons)), quiet=True)


def test_minimizer_accepts_the_names():
    for cons in (("perimeter",), ("fixed_plane",), ("fixed_plane", "pin_to_circle"), ("pin_to_circle", "perimeter"),
                 ("perimeter", "body_area"), ("fixed_plane", "perimeter"), ("fixed_plane", "pin_to_plane", "perimeter")):
        mz = _mz(cons=cons, bodies=[ArrayBody(options={"target_area": 3.0})] if "body_area" in cons else None)
        assert mz.constraint_module_names == list(cons) and mz._has_enforceable_constraints
    for tilt in ("tilt", "tilt_in"):
        _mz(emods=("surface", tilt), cons=("fixed_plane",))
        _mz(emods=("surface", tilt), cons=("fixed_plane", "pin_to_circle"))


def test_every_refusal_has_its_own_text():
    with pytest.raises(L.MembraneHipError, match="lists fixed_plane after pin_to_circle"):
        _mz(cons=("pin_to_circle", "fixed_plane"))
    with pytest.raises(L.MembraneHipError, match="lists fixed_plane after perimeter"):
        _mz(cons=("perimeter", "fixed_plane"))
    with pytest.raises(L.MembraneHipError, match="lists fixed_plane after volume"):
        _mz(cons=("volume", "fixed_plane"))
    with pytest.raises(L.MembraneHipError, match="lists perimeter before pin_to_plane"):
        _mz(cons=("perimeter", "pin_to_plane"))
    for first in ("volume", "body_area", "global_area"):
        with pytest.raises(L.MembraneHipError, match="lists perimeter after " + first):
            _mz(cons=(first, "perimeter"))
    for tilt in ("tilt", "tilt_in", "bending_tilt_out"):
        with pytest.raises(L.MembraneHipError, match="perimeter together with tilt modules is outside the HIP hot path"):
            _mz(emods=("surface", tilt))
    with pytest.raises(L.MembraneHipError, match="perimeter together with tilt modules is outside the HIP hot path"):
        _mz(cons=("perimeter", "tilt_thetaB_boundary_in"))
    # the pairs whose reference trajectories hinge on Mesh.positions_view not being invalidated by the enforce-only modules
    for cons in (("perimeter", "volume"), ("perimeter", "volume", "body_area"), ("perimeter", "global_area"),
                 ("fixed_plane", "volume"), ("fixed_plane", "body_area"), ("fixed_plane", "global_area")):
        with pytest.raises(L.MembraneHipError, match=f"{cons[0]} next to {cons[1]} is outside the HIP hot path: the reference "
                                                     "evaluates that module's first pass at the positions cached before"):
            _mz(cons=cons)
    # ... and the fixtures the reference gave for them (kept for the change that reproduces that first pass) are refused
    for fname in sorted(os.listdir(GOLD)):
        if re.match(r"traj_ico\d_(gd|cg)_perim_volume_|traj_disk5_(gd|cg)_fplane_area", fname):
            z = np.load(os.path.join(GOLD, fname))
            with pytest.raises(L.MembraneHipError, match="positions cached before"):
                _mz(cons=tuple(str(c) for c in z["constraint_modules"]))
    with pytest.raises(L.MembraneHipError, match="no edge table"):
        _mz(edges=False)
    with pytest.raises(L.MembraneHipError, match=r"outside the HIP hot path \(.*fixed_plane, perimeter\)"):
        _mz(cons=("pins",))
    # the library's own texts (raised on a GPU: tests/test_gpu_enforce_only.py)
    src = "".join(open(os.path.join(ROOT, "membrane_solver_amd", "csrc", f)).read()
                  for f in ("ms_api_enforce.inc", "ms_api_step.inc", "ms_api_shard.inc"))
    for text in ("ms_set_fixed_plane: fixed_plane is not sharded (single GPU only)",
                 "ms_set_perimeter: perimeter is not sharded (single GPU only)",
                 "the fixed_plane / perimeter constraints are not sharded (single GPU only)",
                 "ms_set_fixed_plane: the normal and the point must be finite", "ms_set_fixed_plane: |normal| < 1e-15",
                 "ms_set_perimeter: edge row out of range", "ms_set_perimeter: a target perimeter is not finite",
                 "ms_stepper_params.enforce_fixed_plane without a plane", "ms_stepper_params.enforce_perimeter without loops",
                 "perimeter together with tilt modules is outside the device path",
                 "tilt_splay_twist_in together with fixed_plane"):
        assert text in src, text


def test_signed_edge_indices_on_both_mesh_kinds():
    P, T, _B, e, _ = _disk()
    mesh = ArrayMesh(P, T, edges=e, global_parameters={"perimeter_constraints": [
        {"edges": [1, -2, 3], "target_perimeter": 1.0}, {"edges": [2]}, {"edges": [], "target_perimeter": 2.0},
        {"edges": [-len(e)], "target_perimeter": 0.5}]})
    num, off, tail, head, target = perimeter.loops(mesh)
    assert num == [0, 3] and off.tolist() == [0, 3, 4] and target.tolist() == [1.0, 0.5]
    assert tail.tolist() == [e[0, 0], e[1, 1], e[2, 0], e[-1, 1]] and head.tolist() == [e[0, 1], e[1, 0], e[2, 1], e[-1, 0]]
    for bad in (0, len(e) + 1, -(len(e) + 1), "x"):
        mesh.global_parameters.set("perimeter_constraints", [{"edges": [1, bad], "target_perimeter": 1.0}])
        with pytest.raises(L.MembraneHipError, match="perimeter: .*edge index"):
            perimeter.loops(mesh)
    mesh.global_parameters.set("perimeter_constraints", [{"edges": [1], "target_perimeter": float("nan")}])
    with pytest.raises(L.MembraneHipError, match="must be finite"):
        perimeter.loops(mesh)
    # a reference-style mesh: dicts of vertex / edge objects with ids of their own, ids != rows
    ids = [10 * (i + 1) for i in range(len(P))]
    ref = types.SimpleNamespace(
        vertices={v: types.SimpleNamespace(position=P[i].copy()) for i, v in enumerate(ids)},
        edges={k + 1: types.SimpleNamespace(tail_index=ids[a], head_index=ids[b]) for k, (a, b) in enumerate(e)},
        vertex_index_to_row={v: i for i, v in enumerate(ids)},
        global_parameters={"perimeter_constraints": [{"edges": [3, -1], "target_perimeter": 1.0}]})
    num, off, tail, head, target = perimeter.loops(ref)
    assert tail.tolist() == [e[2, 0], e[0, 1]] and head.tolist() == [e[2, 1], e[0, 0]]
    ref.global_parameters = {"perimeter_constraints": [{"edges": [len(e) + 1], "target_perimeter": 1.0}]}
    with pytest.raises(L.MembraneHipError, match="unknown edge index"):
        perimeter.loops(ref)


def test_fixed_plane_parameters(caplog):
    mesh = types.SimpleNamespace(global_parameters={})
    n, q = fixed_plane.plane(mesh)
    assert n.tolist() == [0.0, 0.0, 1.0] and q.tolist() == [0.0, 0.0, 0.0]
    n, q = fixed_plane.plane(mesh, {"fixed_plane_normal": [0.2, -0.1, 1.0], "fixed_plane_point": [0, 0, 0.1]})
    assert n.tolist() == [0.2, -0.1, 1.0] and q.tolist() == [0.0, 0.0, 0.1]  # (the library normalises)
    with caplog.at_level("WARNING", logger="membrane_solver"):
        assert fixed_plane.plane(mesh, {"fixed_plane_normal": [0.0, 0.0, 1e-16]}) is None
    assert "normal is near zero" in caplog.text
    with pytest.raises(L.MembraneHipError, match="must be finite"):
        fixed_plane.plane(mesh, {"fixed_plane_normal": [0.0, float("nan"), 1.0]})
    with pytest.raises(L.MembraneHipError, match="three numbers"):
        fixed_plane.plane(mesh, {"fixed_plane_normal": [0.0, 1.0]})
