"""body_area_penalty, host side (no GPU): the reference fixtures are self-consistent, the parameters resolve as
modules/energy/body_area_penalty.py:111-123 resolves them, the module is refused where the device path does not run
it, and the header, the library and the Python signatures agree on the new entry points."""

import ast
import ctypes
import glob
import os
import re
import types

import numpy as np
import pytest

from membrane_solver_amd import _lib as L
from membrane_solver_amd.core.parameters import GlobalParameters, ParameterResolver
from membrane_solver_amd.geometry.mesh import ArrayBody, ArrayMesh
from membrane_solver_amd.modules.energy.body_area_penalty import body_area_params
from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager
from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager
from membrane_solver_amd.runtime.minimizer import Minimizer
from membrane_solver_amd.runtime.steppers import GradientDescent

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TRAJ = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLD, "traj_*_area_*.npz")))


def _facet_areas(P, T):
    n = np.cross(P[T[:, 1]] - P[T[:, 0]], P[T[:, 2]] - P[T[:, 0]])
    return 0.5 * np.linalg.norm(n, axis=1)


def case_mesh(z, name, energy=("body_area_penalty",)):
    T = z[name + "__tri"]
    rows = z[name + "__body_facets"]
    body = ArrayBody(facet_rows=None if len(rows) == len(T) else rows,
                     options=ast.literal_eval(str(z[name + "__body_options"])))
    return ArrayMesh(z[name + "__positions"], T, global_parameters=ast.literal_eval(str(z[name + "__gp"])),
                     bodies=[body], energy_modules=list(energy))


def test_area_cases_are_self_consistent():
    z = np.load(os.path.join(GOLD, "area_cases.npz"))
    names = [str(n) for n in z["names"]]
    assert {"ico4_no_target", "ico4_subset_above", "ico8_subset_below", "disk5_global_above"} <= set(names)
    above = below = 0
    for name in names:
        mesh = case_mesh(z, name)
        P, T, rows = z[name + "__positions"], z[name + "__tri"], z[name + "__body_facets"]
        A = float(z[name + "__area"])
        assert abs(_facet_areas(P, T)[rows].sum() - A) <= 1e-12 * A, name
        ka = body_area_params(mesh, mesh.global_parameters, ParameterResolver(mesh.global_parameters))
        E, g = float(z[name + "__energy"]), z[name + "__grad"]
        if ka is None:
            assert E == 0.0 and not g.any(), name
            continue
        k, a0 = ka
        assert abs(E - 0.5 * k * (A - a0) ** 2) <= 1e-12 * abs(E), name
        above += A > a0
        below += A < a0
        # factor * dA/dx vanishes off the body, and translations leave the area alone
        off_body = np.setdiff1d(np.arange(len(P)), np.unique(T[rows]))
        assert not g[off_body].any(), name
        assert np.abs(g.sum(axis=0)).max() <= 1e-12 * np.abs(g).max(), name
    assert above >= 2 and below >= 2


@pytest.mark.parametrize("fname", TRAJ)
def test_trajectory_fixtures_load(fname):
    z = np.load(os.path.join(GOLD, fname))
    assert os.path.getsize(os.path.join(GOLD, fname)) <= 250 * 1024
    log = np.asarray(z["step_log"]).reshape(-1, 3)
    assert len(log) == int(z["n_steps"]) and log[:, 0].sum() >= 1
    assert "body_area_penalty" in [str(s) for s in z["energy_modules"]]
    T, rows = z["tri"], z["body_facets"]
    assert rows.min() >= 0 and rows.max() < len(T) and len(np.unique(rows)) == len(rows)
    opts = ast.literal_eval(str(z["body_options"]))
    gp = ast.literal_eval(str(z["gp"]))
    assert float(z["area_target"]) == float(opts["area_target"]) > 0.0
    assert float(z["area_stiffness"]) == float(opts.get("area_stiffness", gp.get("area_stiffness")))
    assert z["positions_final"].shape == z["positions0"].shape
    # the accepted energies of a line search never rise
    acc = log[log[:, 0] > 0, 2]
    assert np.all(np.diff(acc) <= 0.0)


def test_there_are_seven_trajectories():
    assert len(TRAJ) == 7, TRAJ


def _mesh(gp, options):
    P = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
    T = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], dtype=np.int32)
    return ArrayMesh(P, T, global_parameters=gp, bodies=[ArrayBody(options=dict(options))],
                     energy_modules=["body_area_penalty"])


def test_parameter_resolution():
    def resolve(gp, options):
        m = _mesh(gp, options)
        return body_area_params(m, m.global_parameters, ParameterResolver(m.global_parameters))

    assert resolve({"area_stiffness": 5.0}, {"area_target": 2.0}) == (5.0, 2.0)                      # global
    assert resolve({"area_stiffness": 5.0}, {"area_target": 2.0, "area_stiffness": 7.0}) == (7.0, 2.0)  # per body
    assert resolve({}, {"area_target": 2.0, "area_stiffness": 7.0}) == (7.0, 2.0)
    assert resolve({"area_stiffness": 5.0}, {}) is None                   # absent target: the module returns 0
    assert resolve({}, {"area_target": 2.0}) is None                      # no default stiffness
    assert resolve({"area_stiffness": 0.0}, {"area_target": 2.0}) is None  # zero stiffness switches it off
    assert resolve({"area_stiffness": 5.0}, {"area_target": 2.0, "area_stiffness": 0.0}) is None
    m = ArrayMesh(np.zeros((3, 3)), np.array([[0, 1, 2]], dtype=np.int32), global_parameters={"area_stiffness": 1.0})
    assert body_area_params(m, m.global_parameters, ParameterResolver(m.global_parameters)) is None  # no body
    assert "area_stiffness" not in GlobalParameters().to_dict()


def _minimizer(mesh, energy):
    return Minimizer(mesh, mesh.global_parameters, GradientDescent(), EnergyModuleManager(energy),
                     ConstraintModuleManager([]), energy_modules=energy, constraint_modules=[], quiet=True)


@pytest.mark.parametrize("tilt", ["tilt", "bending_tilt", "tilt_smoothness", "tilt_in", "tilt_smoothness_out",
                                  "bending_tilt_in", "tilt_disk_target_out"])
def test_minimizer_refuses_the_module_next_to_tilt_modules(tilt):
    mesh = _mesh({"area_stiffness": 5.0}, {"area_target": 2.0})
    with pytest.raises(L.MembraneHipError, match="body_area_penalty together with tilt"):
        _minimizer(mesh, ["surface", "body_area_penalty", tilt])
    _minimizer(mesh, ["surface", "bending", "volume", "body_area_penalty"])  # accepted by the module wiring


def test_unsupported_module_message_names_it():
    mesh = _mesh({}, {})
    stub = types.SimpleNamespace(get_module=lambda name: types.SimpleNamespace(
        compute_energy_and_gradient_array=lambda *a, **k: 0.0))
    with pytest.raises(L.MembraneHipError, match="body_area_penalty"):
        Minimizer(mesh, mesh.global_parameters, GradientDescent(), stub, ConstraintModuleManager([]),
                  energy_modules=["surface", "line_tension"], constraint_modules=[], quiet=True)


def test_sharded_driver_refuses_the_module():
    from membrane_solver_amd.parallel import HipShardBackend

    with pytest.raises(L.MembraneHipError, match="body_area_penalty module is not sharded"):
        HipShardBackend.configure(types.SimpleNamespace(), modules=L.MS_MOD_SURFACE | L.MS_MOD_AREA_PENALTY)
    src = open(os.path.join(ROOT, "membrane_solver_amd", "csrc", "ms_api_shard.inc")).read()
    step = src[src.index("int ms_shard_step("):]
    assert "MS_MOD_AREA_PENALTY" in step[:1200], "ms_shard_step must refuse the module before it queues anything"


def test_header_library_and_signatures_agree():
    L.build()
    hdr = open(os.path.join(ROOT, "include", "membrane_hip.h")).read()
    assert int(re.search(r"#define MS_MOD_AREA_PENALTY (\d+)u", hdr).group(1)) == L.MS_MOD_AREA_PENALTY == 65536
    assert int(re.search(r"MS_S_AREA = (\d+)", hdr).group(1)) == L.MS_S_AREA == 30
    assert int(re.search(r"MS_NSCAL = (\d+)", hdr).group(1)) == L.MS_NSCAL == 31
    bits = [int(v) for v in re.findall(r"#define MS_(?:MOD|CON|TRACK)_[A-Z_]+ (\d+)u", hdr)]
    assert len(bits) == len(set(bits)) and all(b & (b - 1) == 0 for b in bits)
    L.lib()
    cd = ctypes.CDLL(L.LIB_PATH)
    for name in ("ms_set_area_penalty", "ms_get_body_area"):
        assert re.search(r"\bint %s\(ms_ctx \*ctx" % name, hdr), name
        assert hasattr(cd, name) and name in L.SIGNATURES, name
    # ms_params keeps its layout: the new parameters have an entry point of their own
    assert [f[0] for f in L.ms_params._fields_] == ["modules", "bending_model", "bending_grad_mode",
                                                    "volume_stiffness", "target_volume"]
    assert ctypes.sizeof(L.ms_params) == 32
