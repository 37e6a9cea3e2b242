"""pin_to_plane / pin_to_circle next to the tilt modules, CPU side: the fixtures of tools/gen_golden_pins_tilt.py are
consistent with themselves, Minimizer._upload_pins accepts tilt modules and refuses the volume constraint next to them,
_enforce projects the tilts after a pins-only enforcement, and the library's step carries the lane and its refusal."""

import json
import os
import re

import numpy as np
import pytest

from conftest import load_golden

from membrane_solver_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAJ = ["traj_softsource_deck_gd_pins.npz", "traj_disk6_cg_coupling_pins_slide.npz", "traj_ico4_gd_bt_pins_plane.npz"]


@pytest.mark.parametrize("fname", TRAJ)
def test_fixture_is_self_consistent(fname):
    """The recorded trial energies give the recorded accept / reject log: every trial against its own Armijo bound, the
    alphas on the backtracking ladder, the step log's energy and next step size from the trial that ended the search."""
    g = load_golden(fname)
    tl, sl, log = g["trial_log"], g["search_log"], g["step_log"]
    c1, beta, n = float(g["armijo_c"]), float(g["beta"]), int(g["n_steps"])
    assert len(sl) == len(log) == n and len(g["tilts_in_steps"]) == n and len(g["tilts_out_steps"]) == n
    given = float(g["step_size0"])
    fixed_mode = json.loads(str(g["gp_json"])).get("step_size_mode") == "fixed"
    for s in range(n):
        E0, gdd, step, n_tr, n_guard = sl[s]
        assert step == given
        rows = tl[tl[:, 0] == s]
        assert len(rows) == int(n_tr)
        ladder = [step]
        for _ in range(12):
            ladder.append(ladder[-1] * beta)
        for row in rows:
            _s, alpha, E, rhs, acc, _move = row
            assert alpha in ladder
            assert rhs == E0 + c1 * alpha * gdd
            assert bool(acc) == (E <= rhs)
            assert abs(E - rhs) >= 1e-9 * abs(E0)  # (a thousand times the energy bar: no decision hangs on rounding)
        assert not rows[:-1, 4].any(), "a trial after an accepted one"
        success = len(rows) > 0 and rows[-1, 4] == 1.0
        assert bool(log[s, 0]) == success
        if success:
            assert log[s, 2] == rows[-1, 2]
            assert log[s, 1] == min(rows[-1, 1] * 1.5, 10.0 * step)
        else:
            assert log[s, 2] == E0
            assert gdd >= 0.0 or len(rows) + int(n_guard) == 10  # no descent direction, or the search ran out
        given = float(g["step_size0"]) if fixed_mode else float(log[s, 1])


def test_fixtures_have_the_properties_they_are_named_for():
    g = load_golden(TRAJ[0])
    tl, sl, log = g["trial_log"], g["search_log"], g["step_log"]
    assert len(g["positions0"]) == 84 and len(g["tri"]) == 144
    assert log[:, 0].tolist() == [1.0, 1.0, 1.0, 0.0]
    for s in range(3):
        assert (tl[tl[:, 0] == s][:, 4] == 0.0).any(), "steps 1-3 carry rejected trials"
    assert (tl[:, 0] == 3).sum() + int(sl[3, 4]) == 10, "step 4 runs out of its 10 ladder positions"
    # a lane that forgets the restore would differ: rejected trials moved tilt rows by far more than rounding
    assert tl[tl[:, 4] == 0.0][:, 5].max() > 1e-9
    g = load_golden(TRAJ[1])
    assert len(g["positions0"]) == 127 and (g["trial_log"][:, 4] == 0.0).any()
    assert np.max(np.abs(g["grad0"] - g["grad0_raw"])) > 1e-6 * np.max(np.abs(g["grad0_raw"]))  # the KKT solve projects
    assert [str(m) for m in g["modules"]] == ["surface", "tilt_in", "tilt_out", "tilt_coupling", "bending_tilt_in"]
    g = load_golden(TRAJ[2])
    assert len(g["positions0"]) == 162 and [str(m) for m in g["modules"]] == ["tilt", "bending_tilt"]
    for f in TRAJ:
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", f)) < (1 << 20)


class _StubDevice:
    def __init__(self):
        self.tables, self.calls, self.modules = "unset", [], 0

    def set_pins(self, tables):
        self.tables = tables

    def enforce_pins(self):
        self.calls.append("enforce_pins")

    def project_tilts_to_tangent(self):
        self.calls.append("project_tilts_to_tangent")


class _StubMirror:
    _topo_key = ("stub",)


def _minimizer(fname, constraints=None):
    from membrane_solver_amd.geometry.mesh import ArrayMesh
    from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager
    from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager
    from membrane_solver_amd.runtime.minimizer import Minimizer
    from membrane_solver_amd.runtime.steppers import GradientDescent

    g = load_golden(fname)
    mods = [str(m) for m in g["modules"]]
    cons = [str(m) for m in g["constraint_modules"]] if constraints is None else constraints
    opts = lambda t: {int(k): v for k, v in json.loads(str(t)).items()}  # noqa: E731
    mesh = ArrayMesh(g["positions0"], g["tri"], fixed=g["fixed"], global_parameters=json.loads(str(g["gp_json"])),
                     energy_modules=mods, constraint_modules=cons, edges=g["edges"], vertex_options=opts(g["vopts"]),
                     edge_options=opts(g["eopts"]), tilts_in=g["tilts_in0"], tilts_out=g["tilts_out0"])
    return Minimizer(mesh, mesh.global_parameters, GradientDescent(), EnergyModuleManager(mods),
                     ConstraintModuleManager(cons), quiet=True)


TILT_MODS = L.MS_MOD_TILT_IN | L.MS_MOD_TILT_OUT | L.MS_MOD_BENDING_TILT_IN | L.MS_MOD_TILT_RIM_SOURCE_IN


def test_upload_pins_accepts_tilt_modules():
    mz = _minimizer(TRAJ[0])
    dm = _StubDevice()
    mz._upload_pins(_StubMirror(), dm, TILT_MODS)
    assert mz._pins_active and dm.tables is mz.pin_tables and len(dm.tables.stage_kind) > 0
    for bits in (L.MS_MOD_TILT | L.MS_MOD_BENDING_TILT, L.MS_MOD_TILT_COUPLING | L.MS_MOD_TILT_OUT):
        mz._pin_key = None
        mz._upload_pins(_StubMirror(), dm, bits)  # single field, coupling: no refusal either


def test_upload_pins_refuses_tilt_modules_with_the_volume_constraint():
    mz = _minimizer(TRAJ[0])
    with pytest.raises(L.MembraneHipError, match="next to tilt modules together with the volume constraint"):
        mz._upload_pins(_StubMirror(), _StubDevice(), TILT_MODS | L.MS_CON_VOLUME)
    mz = _minimizer(TRAJ[0], constraints=["pin_to_plane", "pin_to_circle", "volume"])
    with pytest.raises(L.MembraneHipError, match="next to tilt modules together with the volume constraint"):
        mz._upload_pins(_StubMirror(), _StubDevice(), TILT_MODS)
    mz._upload_pins(_StubMirror(), _StubDevice(), L.MS_MOD_SURFACE)  # (pins + volume without a tilt family: as before)


@pytest.mark.parametrize("context,projects", [("mesh_operation", True), ("finalize", True), ("minimize", False)])
def test_enforce_projects_the_tilts_after_the_pins(context, projects):
    mz = _minimizer(TRAJ[0])
    dm = _StubDevice()
    mz._upload_pins(_StubMirror(), dm, TILT_MODS)
    dm.modules = TILT_MODS
    assert mz._enforce(dm, context) is True
    assert dm.calls == ["enforce_pins"] + (["project_tilts_to_tangent"] if projects else [])
    dm2 = _StubDevice()
    dm2.modules = L.MS_MOD_SURFACE  # no tilt family: nothing to project
    assert mz._enforce(dm2, context) is True and dm2.calls == ["enforce_pins"]


def test_enforce_projects_with_an_empty_pin_program():
    """A listed pin module whose program is empty (nothing tagged) is still an enforcer in the reference: no pin launch,
    but the tilts are projected in the mesh-operation context."""
    mz = _minimizer(TRAJ[0])
    mz._pins_active = False
    dm = _StubDevice()
    dm.modules = TILT_MODS
    assert mz._enforce(dm, "mesh_operation") is True and dm.calls == ["project_tilts_to_tangent"]


def test_header_and_lib_agree_on_the_stepper_block():
    hdr = open(os.path.join(ROOT, "include", "membrane_hip.h")).read()
    block = re.search(r"typedef struct ms_stepper_params \{(.*?)\} ms_stepper_params;", hdr, re.S).group(1)
    names = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", block, flags=re.S))
    assert names == [f[0] for f in L.ms_stepper_params._fields_]
    assert "pins next to tilt modules together with the volume constraint" in " ".join(hdr.split())


def test_ms_exec_pins_is_parsed_and_documented():
    """MS_EXEC_PINS=0 is read where the other interpreter switches are, the two record kinds exist on both sides of the
    pack, and README's row names the bitwise test."""
    csrc = os.path.join(ROOT, "membrane_solver_amd", "csrc")
    ctx = open(os.path.join(csrc, "ms_api_context.inc")).read()
    assert re.search(r'exec_pins\s*=\s*!\(getenv\("MS_EXEC_PINS"\) != nullptr && atoi\(getenv\("MS_EXEC_PINS"\)\) == 0\)', ctx)
    internal = open(os.path.join(csrc, "ms_internal.h")).read()
    interp = open(os.path.join(csrc, "ms_exec.inc")).read()
    for kind in ("CK_PIN_ENFORCE", "CK_PIN_GRAD"):
        assert kind in internal and ("case " + kind) in interp
    row = [ln for ln in open(os.path.join(ROOT, "README.md")) if ln.startswith("| `MS_EXEC_PINS=0`")]
    assert len(row) == 1 and "test_gpu_pins_tilt.py::test_recorded_pin_kernels_are_bitwise_the_launched_ones" in row[0]
