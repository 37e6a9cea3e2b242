"""One-tile tilt relaxations on the device against the oracle port, on the cases of tests/relax_cases.py: meshes at the
tile's capacity and at the facet-list edges of the fused relaxation (csrc/ms_relax_fused.inc), one leaflet only, both
solvers, ladders that halve or reject everything, a tolerance that ends the loop, clamp bits, the disk target.  Every
case runs on the four implementations a one-tile context can take (and on the launch-per-kernel path with fixed-order
sums, the bitwise partner of the generic program):

    launch         MS_EXEC=0                       the host-driven loop of relax_fields, one launch per kernel
    launch_fixed   MS_EXEC=0, fixed-order sums
    generic_fixed  MS_EXEC=1, fixed-order sums     the generic device program (ms_exec.inc: exec_relax)
    generic        MS_EXEC_FUSED=0                 the same with the default LDS-atomic sums
    fused          defaults                        exec_relax_fused (leaflet fields; the single field has no fused form)

The bars are the project's own: counts equal to the port's, fields to 1e-9 relative max-norm
(test_gpu_leaflet.py::test_leaflet_midsize_matches_oracle), clamped rows to 1e-12, generic_fixed bit for bit
launch_fixed (test_gpu_exec.py), fused within 1e-11 of the field scale of generic (test_gpu_exec.py), and an evaluation
after the relaxation to 1e-11 / 1e-10 of the port's at its relaxed fields.

Measured on an MI355X when the table was written (the port's iterations / evaluations, which every path reproduced;
largest relative difference of a relaxed field from the port's per path, bar 1e-9; fused against generic in units of
the field scale, bar 1e-11); the evaluation afterwards was within 3e-16 (energy) and 1.4e-15 (gradients) everywhere:

    case                      it/ev   launch   generic_fixed  generic  fused    fused-generic
    all-closed256             6/13    5.7e-16  5.7e-16        4.3e-16  4.3e-16  1.7e-16
    all-closed255_odd         6/13    4.0e-16  5.3e-16        4.0e-16  4.0e-16  1.1e-16
    all-disk256               6/13    6.0e-16  6.0e-16        6.0e-16  4.5e-16  1.1e-16
    all-closed130             6/13    6.9e-16  5.3e-16        5.3e-16  5.3e-16  1.1e-16
    all-closed131             6/13    4.3e-16  3.6e-16        3.6e-16  3.9e-16  1.2e-16
    all-small92               6/13    5.3e-16  5.3e-16        6.2e-16  5.3e-16  7.0e-17
    all-hub                   6/13    2.6e-16  3.7e-16        3.1e-16  3.1e-16  8.1e-17
    gd-closed256              6/12    2.9e-16  2.3e-16        2.9e-16  2.9e-16  1.1e-16
    gd-disk256                6/12    3.5e-16  3.5e-16        3.5e-16  3.5e-16  5.4e-17
    nojacobi-closed131        6/13    5.2e-16  3.6e-16        4.3e-16  4.5e-16  1.0e-16
    step40-closed255_odd      6/50    1.3e-15  1.2e-15        1.2e-15  1.2e-15  1.4e-16
    step40gd-closed131        6/58    8.2e-16  7.5e-16        7.8e-16  6.5e-16  9.7e-17
    allrej-closed256          1/13    1.1e-16  1.1e-16        1.1e-16  1.1e-16  0.0e+00
    allrej-gd-small92         1/13    1.1e-16  1.1e-16        1.1e-16  1.1e-16  0.0e+00
    tol-closed131             4/9     2.6e-16  2.6e-16        2.6e-16  2.6e-16  1.1e-16
    tolgd-closed130           3/7     1.6e-16  1.6e-16        1.6e-16  1.6e-16  1.1e-16
    in_only-closed256         6/13    2.3e-16  2.3e-16        2.3e-16  2.3e-16  1.1e-16
    out_only-disk256          6/13    4.6e-16  4.6e-16        3.4e-16  3.4e-16  4.7e-17
    clampall_in-closed130     6/13    4.6e-16  3.8e-16        3.8e-16  3.8e-16  1.1e-16
    clampall_out-hub          6/13    2.2e-16  2.2e-16        2.2e-16  2.2e-16  1.1e-16
    disktarget-disk256        6/13    5.1e-16  5.1e-16        5.1e-16  5.1e-16  5.4e-17
    disktarget_off-disk256    6/13    3.8e-16  3.8e-16        3.8e-16  3.8e-16  0.0e+00
    precond_param-closed256   6/13    3.4e-16  3.4e-16        3.4e-16  3.4e-16  1.1e-16
    single-closed256          6/13    2.3e-16  2.3e-16        2.3e-16  2.3e-16  -
"""
from __future__ import annotations

import numpy as np
import pytest

import relax_cases as rc
from conftest import relerr

pytestmark = pytest.mark.gpu

PORT_PATHS = ("launch", "generic_fixed", "generic", "fused")
_ENV = {"launch": {"MS_EXEC": "0"}, "launch_fixed": {"MS_EXEC": "0"}, "generic_fixed": {"MS_EXEC": "1"},
        "generic": {"MS_EXEC_FUSED": "0"}, "fused": {}}
_RESULTS = {}


def _context(case, m):
    from membrane_solver_amd.geometry.mesh import ArrayMesh
    from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager
    from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager
    from membrane_solver_amd.runtime.minimizer import Minimizer
    from membrane_solver_amd.runtime.steppers import GradientDescent

    mods = list(case.modules)
    if case.kind == "single":
        mesh = ArrayMesh(m.P, m.T, tilts=m.tilts, tilt_fixed=m.fixed_in, global_parameters=dict(case.gp),
                         energy_modules=mods, constraint_modules=[])
    else:
        mesh = ArrayMesh(m.P, m.T, tilts_in=m.tilts_in, tilts_out=m.tilts_out, tilt_fixed_in=m.fixed_in,
                         tilt_fixed_out=m.fixed_out, disk_rows_in=m.disk_rows, disk_rows_out=m.disk_rows,
                         global_parameters=dict(case.gp), energy_modules=mods, constraint_modules=[])
    mz = Minimizer(mesh, mesh.global_parameters, GradientDescent(), EnergyModuleManager(mods),
                   ConstraintModuleManager([]), quiet=True)
    _mir, dm = mz._device()
    return mz, dm


def _relax(case, dm, rp):
    return dm.relax_tilts(**rp) if case.kind == "single" else dm.relax_leaflet_tilts(**rp)


def _fields(case, dm):
    return (dm.get_tilts(),) if case.kind == "single" else (dm.get_leaflet_tilts("in"), dm.get_leaflet_tilts("out"))


def _run(cid, path, monkeypatch):
    """One relaxation of the case in a fresh context of the path (cached: the cross-path tests share the runs) ->
    dict(counts, fields, stats, start = the device's own projected start fields, E / grads of an evaluation
    afterwards)"""
    if (cid, path) in _RESULTS:
        return _RESULTS[cid, path]
    case = rc.BY_ID[cid]
    m = rc.materialize(case)
    for var in ("MS_EXEC", "MS_EXEC_FUSED", "MS_DETERMINISTIC"):
        monkeypatch.delenv(var, raising=False)
    if path.endswith("_fixed"):  # (what the `deterministic` fixture sets; a test here creates contexts of both kinds)
        monkeypatch.setenv("MS_DETERMINISTIC", "1")
    for var, val in _ENV[path].items():
        monkeypatch.setenv(var, val)
    # the device's projected start fields: a call that stops at its first norm test (no iteration, one evaluation)
    mz, dm = _context(case, m)
    rp = mz._tilt_relax_params()
    assert rp is not None
    assert dm.tile_stats()["n_tiles"] == 1 and dm.tile_stats()["facet_instances"] == m.nf
    assert _relax(case, dm, dict(rp, tol=1e300)) == (0, 1)
    start = _fields(case, dm)
    mz.reset_soa_caches()
    mz, dm = _context(case, m)
    counts = _relax(case, dm, rp)
    fields = _fields(case, dm)
    stats = dm.exec_stats()
    if case.kind == "single":
        E, g = dm.tilt_energy_and_gradient()
        grads = (g,)
    else:
        E, gi, go = dm.leaflet_tilt_energy_and_gradient()
        grads = (gi, go)
    mz.reset_soa_caches()
    _RESULTS[cid, path] = out = {"counts": counts, "fields": fields, "stats": stats, "start": start, "E": E,
                                 "grads": grads}
    return out


def _port_evaluation(case, p):
    from oracle import minimizer_port as mp
    from oracle import ms_oracle as orc

    if case.kind == "single":
        E, g = mp.energy_and_tilt_gradient(p, p.positions, p.tilts)
        return E, (g,)
    va = orc.barycentric_vertex_areas(p.positions, p.tri)
    E, gi, go = mp.energy_and_leaflet_tilt_gradients(p, p.positions, p.tilts_in, p.tilts_out, va)
    return E, (gi, go)


@pytest.mark.parametrize("path", PORT_PATHS)
@pytest.mark.parametrize("cid", rc.CASE_IDS)
def test_relaxation_matches_the_port(cid, path, monkeypatch):
    case = rc.BY_ID[cid]
    p, port_counts, _trace = rc.port_result(cid)
    m = rc.materialize(case)
    r = _run(cid, path, monkeypatch)
    st = r["stats"]
    if path == "launch":
        assert not st["active"] and st["relax_programs"] == 0, st
    elif path == "fused" and case.kind == "leaflet":
        assert st["relax_fused"] > 0, st
    else:  # (the single field has no fused form: the defaults run the generic program)
        assert st["relax_programs"] > 0 and st["relax_fused"] == 0, st
    want = rc.fields_of(case, p)
    errs = [relerr(a, b) for a, b in zip(r["fields"], want)]
    print(f"RELAX_FIG port {cid} {path} counts={r['counts']} port={port_counts} "
          f"relerr={' '.join('%.3e' % e for e in errs)} bar=1e-9")
    assert r["counts"] == port_counts, f"{cid} on {path}: (iterations, evaluations) differ from the port's"
    for name, e in zip(("in", "out"), errs):
        assert e < 1e-9, f"{cid} on {path}: relaxed field {name} off by {e:.3e}"
    masks = (m.fixed_in,) if case.kind == "single" else (m.fixed_in, m.fixed_out)
    for got, start, mask in zip(r["fields"], r["start"], masks):
        assert np.abs(got[mask] - start[mask]).max(initial=0.0) <= 1e-12, f"{cid} on {path}: a clamped row moved"
        # (every implementation copies a clamped row's projected value into each trial: not a bit changes either)
        assert np.array_equal(got[mask], start[mask]), f"{cid} on {path}: a clamped row was recomputed"
    # (the device's projected start rows are the uploaded tangent rows to rounding)
    starts = (m.tilts,) if case.kind == "single" else (m.tilts_in, m.tilts_out)
    for start, given in zip(r["start"], starts):
        assert np.abs(start - given).max() <= 1e-12
    if case.all_rejected:
        for got, start in zip(r["fields"], r["start"]):
            assert np.array_equal(got, start), f"{cid} on {path}: a rejected ladder moved the fields"
    # the context is usable afterwards: an evaluation at the relaxed fields is the port's
    E_ref, g_ref = _port_evaluation(case, p)
    e_err = abs(r["E"] - E_ref) / abs(E_ref)
    g_errs = [relerr(a, b) if np.any(b) else float(np.abs(a).max()) for a, b in zip(r["grads"], g_ref)]
    print(f"RELAX_FIG after {cid} {path} E={e_err:.3e} bar=1e-11 "
          f"grads={' '.join('%.3e' % e for e in g_errs)} bar=1e-10")
    assert e_err <= 1e-11, f"{cid} on {path}: energy after the relaxation off by {e_err:.3e}"
    for e in g_errs:
        assert e < 1e-10, f"{cid} on {path}: tilt gradient after the relaxation off by {e:.3e}"


@pytest.mark.parametrize("cid", rc.CASE_IDS)
def test_generic_program_is_bitwise_the_launch_per_kernel_path(cid, monkeypatch):
    ref = _run(cid, "launch_fixed", monkeypatch)
    got = _run(cid, "generic_fixed", monkeypatch)
    assert not ref["stats"]["active"] and ref["stats"]["relax_programs"] == 0
    assert got["stats"]["relax_programs"] > 0 and got["stats"]["relax_fused"] == 0
    assert got["counts"] == ref["counts"] == rc.COUNTS[cid]
    for a, b in zip(got["fields"], ref["fields"]):
        assert np.array_equal(a, b), f"{cid}: generic program off launch per kernel by {np.abs(a - b).max():.3e}"
    for a, b in zip(got["start"], ref["start"]):
        assert np.array_equal(a, b)
    if rc.BY_ID[cid].all_rejected:
        for a, b in zip(ref["fields"], ref["start"]):
            assert np.array_equal(a, b), f"{cid} on launch_fixed: a rejected ladder moved the fields"


@pytest.mark.parametrize("cid", [c.id for c in rc.CASES if c.kind == "leaflet"])
def test_fused_relaxation_agrees_with_the_generic_program(cid, monkeypatch):
    ref = _run(cid, "generic", monkeypatch)
    got = _run(cid, "fused", monkeypatch)
    assert ref["stats"]["relax_fused"] == 0 and got["stats"]["relax_fused"] > 0
    assert got["counts"] == ref["counts"]
    scale = max(max(np.abs(f).max() for f in ref["fields"]), 1e-30)
    diffs = [float(np.abs(a - b).max()) / scale for a, b in zip(got["fields"], ref["fields"])]
    print(f"RELAX_FIG fused_vs_generic {cid} {' '.join('%.3e' % d for d in diffs)} bar=1e-11")
    for d in diffs:
        assert d <= 1e-11, f"{cid}: fused differs from the generic program by {d:.3e} of the field scale"
