"""rim_slope_match_out with a non-zero strength on the HIP path (csrc/ms_rimmatch.hip: k_rsm_geom, k_rsm_apply): every
case of rim_slope_match_cases.npz through the C ABI and through the plugin against the reference's module, the slot
rules next to tilt_in / tilt_out, the module next to tilt_coupling and tilt_thetaB_contact_in, the lanes that decline,
and the 40-iteration leaflet relaxation (tools/gen_golden_rim_slope_match.py).
Bars: energies to 1e-12 relative, every gradient entry within 1e-10 of the largest; the relaxation within
max(1e-12, 10 x noise), noise being what a 1e-13 perturbation of the start moves in the reference's own run (the fixture
records it)."""

import json

import numpy as np
import pytest

from conftest import load_golden, relerr
from test_rim_slope_match_host import CASES, NAME, NAMES, OFF, case_mesh, expected

pytestmark = pytest.mark.gpu

ON = [n for n in NAMES if n not in OFF]


def _bar(g, key):
    return max(1e-12, 10.0 * float(g[key]))


def _abi_params(name, gp):
    """kwargs of DeviceMesh.set_rim_match straight from the case's rows and parameters"""
    disk = CASES[name + "__disk"] if gp.get("rim_slope_match_disk_group") == "disk" else None
    return {"rim": CASES[name + "__rim"], "outer": CASES[name + "__outer"], "disk": disk,
            "center": gp.get("rim_slope_match_center", [0.0, 0.0, 0.0]), "normal": gp["rim_slope_match_normal"],
            "strength": float(gp["rim_slope_match_strength"])}


def _device(name, tile, deterministic, modules=None, tilt_modulus=0.0):
    from membrane_solver_amd import _lib as L
    from membrane_solver_amd.device import DeviceMesh

    P, T, tin, tout, gp, _vo = case_mesh(name)
    dm = DeviceMesh(P, T, tile_vertices=tile)
    dm.set_deterministic(deterministic)
    dm.set_leaflet_tilts("in", tin, tilt_modulus=tilt_modulus)
    dm.set_leaflet_tilts("out", tout, tilt_modulus=tilt_modulus)
    dm.set_rim_match(**_abi_params(name, gp))
    dm.set_params(modules=L.MS_MOD_RIM_SLOPE_MATCH_OUT if modules is None else modules)
    return dm, P, tin, tout, gp


def _close(got, ref, what):
    big = float(np.max(np.abs(ref)))
    err = float(np.max(np.abs(got - ref)))
    print("   ", what, "max abs err", err, "largest", big)
    if big == 0.0:
        assert not got.any(), what
    else:
        assert err <= 1e-10 * big, what


@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("tile", [0, 64])
@pytest.mark.parametrize("name", ON)
def test_case_through_the_c_abi(name, tile, deterministic):
    """Energy, energy-only == gradient call bit for bit, the three gradients, rows outside the rings untouched, the
    module's own energy and its two terms, two contexts bitwise equal -- default tiles and 64-vertex tiles (the rings'
    rows spread over tiles, the row permutation), both modes of ms_set_deterministic."""
    dm, P, _tin, _tout, gp = _device(name, tile, deterministic)
    E_ref, ref = expected(name, len(P))
    if len(P) > 5000:
        assert dm.tile_stats()["n_tiles"] >= 2
    e = dm.energy()
    own_e = dm.rim_match_energies()
    E, gi, go = dm.leaflet_tilt_energy_and_gradient()
    own = dm.rim_match_energies()
    e2, gshape = dm.energy_and_gradient(want_grad=True, raw=True)
    E_again, gi_again, go_again = dm.leaflet_tilt_energy_and_gradient()
    print(name, tile, deterministic, "E", E, "ref", E_ref, "rel", abs(E - E_ref) / max(abs(E_ref), 1e-300), "own", own)
    assert abs(E - E_ref) <= 1e-12 * abs(E_ref)
    assert e[3] == E == e2[3] == E_again, "energy-only, the gradient call and the shape-gradient call: the same double"
    assert own == own_e and abs(own[0] - E_ref) <= 1e-12 * abs(E_ref) and own[0] == own[1] + own[2]
    assert abs(own[0] - E) <= 4e-16 * (abs(own[1]) + abs(own[2]))  # (E is the fold of the two cells)
    assert not e[:3].any()
    has_disk = gp.get("rim_slope_match_disk_group") == "disk" and len(CASES[name + "__disk"]) > 0
    if not has_disk:
        assert own[2] == 0.0
    _close(gi, ref["tilt_in_grad"], "tilt_in_grad")
    _close(go, ref["tilt_out_grad"], "tilt_out_grad")
    _close(gshape, ref["grad"], "shape grad")
    rest = np.ones(len(P), bool)
    rest[CASES[name + "__rows"].astype(np.int64)] = False
    assert not gi[rest].any() and not go[rest].any() and not gshape[rest].any()
    assert np.array_equal(gi, gi_again) and np.array_equal(go, go_again)
    if E_ref == 0.0:  # an early return: nothing is written
        assert E == 0.0 and not gi.any() and not go.any() and not gshape.any()
    st = dm.rim_match_stats()
    # x is not frozen: every evaluation orders the rings (energy_and_gradient may reuse the energy pass before it)
    assert st["geom_launches"] == st["apply_launches"] and 3 <= st["geom_launches"] <= 5
    dm.close()
    dm2, _P, _a, _b, _g = _device(name, tile, deterministic)  # a second context: the same bits
    E2, gi2, go2 = dm2.leaflet_tilt_energy_and_gradient()
    _e, gshape2 = dm2.energy_and_gradient(want_grad=True, raw=True)
    assert E2 == E and np.array_equal(gi2, gi) and np.array_equal(go2, go) and np.array_equal(gshape2, gshape)
    dm2.close()


@pytest.mark.parametrize("name", NAMES)
def test_plugin_matches_reference(name):
    """Array API (with and without grad_arr), energy-only API and dict API of the drop-in module; arrays are ADDED to."""
    from membrane_solver_amd.core.parameters import GlobalParameters, ParameterResolver
    from membrane_solver_amd.geometry.mesh import ArrayMesh
    from membrane_solver_amd.modules.energy import rim_slope_match_out as module

    P, T, tin, tout, gpd, vo = case_mesh(name)
    gp = GlobalParameters(gpd)
    mesh = ArrayMesh(P, T, global_parameters=gp, tilts_in=tin, tilts_out=tout, vertex_options=vo)
    res = ParameterResolver(gp)
    E_ref, ref = expected(name, len(P))
    base = np.arange(P.size, dtype=np.float64).reshape(P.shape) / P.size
    g, gi, go = base.copy(), base.copy(), base.copy()
    kw = dict(positions=P.copy(), index_map=mesh.vertex_index_to_row)
    E = module.compute_energy_and_gradient_array(mesh, gp, res, grad_arr=g, tilts_in=tin, tilts_out=tout,
                                                 tilt_in_grad_arr=gi, tilt_out_grad_arr=go, **kw)
    gi2, go2 = np.zeros_like(P), np.zeros_like(P)
    E_nog = module.compute_energy_and_gradient_array(mesh, gp, res, grad_arr=None, tilts_in=tin, tilts_out=tout,
                                                     tilt_in_grad_arr=gi2, tilt_out_grad_arr=go2, **kw)
    E2 = module.compute_energy_array(mesh, gp, res, tilts_in=tin, tilts_out=tout, **kw)
    assert abs(E - E_ref) <= 1e-12 * abs(E_ref) and E2 == E == E_nog
    for got, key in ((g, "grad"), (gi, "tilt_in_grad"), (go, "tilt_out_grad")):
        big = float(np.max(np.abs(ref[key])))
        assert np.max(np.abs((got - base) - ref[key])) <= 1e-10 * big + 4e-16
        if big == 0.0:
            assert np.array_equal(got, base)
    _close(gi2, ref["tilt_in_grad"], "tilt_in_grad without grad_arr")
    _close(go2, ref["tilt_out_grad"], "tilt_out_grad without grad_arr")
    Ed, gd, tgi, tgo = module.compute_energy_and_gradient(mesh, gp, res)
    assert Ed == E and sorted(tgo) == [int(r) for r in np.flatnonzero(np.any(ref["tilt_out_grad"] != 0.0, axis=1))]
    assert sorted(gd) == [int(r) for r in np.flatnonzero(np.any(ref["grad"] != 0.0, axis=1))]
    assert sorted(tgi) == [int(r) for r in np.flatnonzero(np.any(ref["tilt_in_grad"] != 0.0, axis=1))]
    assert module.compute_energy_and_gradient(mesh, gp, res, compute_gradient=False) == (Ed, {})


@pytest.mark.parametrize("tile", [0, 64])
@pytest.mark.parametrize("others", ["none", "out", "both"])
@pytest.mark.parametrize("name", ["disk_mean_outer_plus1", "disk_local", "n257_outer_less_disk_mean"])
def test_define_versus_add(name, others, tile):
    """Behind tilt_out / tilt_in the two terms are ADDED into the leaflets' cells, without them they DEFINE the cells
    (every other cell zeroed: an evaluation with the magnitude modules before it left them all non-zero).  With and
    without the bit: energies[:3] bit-identical; energies[3] and the three gradients differ by the reference's."""
    from membrane_solver_amd import _lib as L

    bit = L.MS_MOD_RIM_SLOPE_MATCH_OUT
    full = L.MS_MOD_TILT_IN | L.MS_MOD_TILT_OUT | L.MS_MOD_SURFACE
    base = L.MS_MOD_SURFACE | {"none": 0, "out": L.MS_MOD_TILT_OUT, "both": L.MS_MOD_TILT_IN | L.MS_MOD_TILT_OUT}[others]
    dm, P, tin, tout, _gp = _device(name, tile, True, modules=full, tilt_modulus=1.3)
    dm.set_leaflet_tilts("in", tin + 0.05, tilt_modulus=1.3)  # every tile's cell of both slots non-zero
    dm.set_leaflet_tilts("out", tout + 0.05, tilt_modulus=1.3)
    assert dm.energy()[3] > 0.0
    dm.set_leaflet_tilts("in", tin, tilt_modulus=1.3)
    dm.set_leaflet_tilts("out", tout, tilt_modulus=1.3)
    dm.set_params(modules=base)
    if others == "none":
        e0, g0 = dm.energy_and_gradient(want_grad=True, raw=True)
        E0, gi0, go0 = 0.0, np.zeros_like(P), np.zeros_like(P)
    else:
        E0, gi0, go0 = dm.leaflet_tilt_energy_and_gradient()
        e0, g0 = dm.energy_and_gradient(want_grad=True, raw=True)
    dm.set_params(modules=base | bit)
    E1, gi1, go1 = dm.leaflet_tilt_energy_and_gradient()
    own_t = dm.rim_match_energies()
    e1, g1 = dm.energy_and_gradient(want_grad=True, raw=True)  # (phase_gradient rewrites the slots behind k_tilt<1>)
    own = dm.rim_match_energies()
    e2 = dm.energy()
    E_ref, ref = expected(name, len(P))
    tol = 1e-12 * (abs(E_ref) + abs(E0) + abs(e0[3]))
    print(name, others, tile, "dE", E1 - E0, e1[3] - e0[3], e2[3] - e0[3], "own", own, "ref", E_ref)
    assert abs((E1 - E0) - E_ref) <= tol and abs((e1[3] - e0[3]) - E_ref) <= tol and abs((e2[3] - e0[3]) - E_ref) <= tol
    assert abs(own[0] - E_ref) <= 1e-12 * abs(E_ref) and own_t == own
    assert np.array_equal(e1[:3], e0[:3]) and np.array_equal(e2[:3], e0[:3])
    for d, key, other in ((gi1 - gi0, "tilt_in_grad", gi0), (go1 - go0, "tilt_out_grad", go0), (g1 - g0, "grad", g0)):
        big = float(np.max(np.abs(other))) if other.any() else 0.0
        assert np.max(np.abs(d - ref[key])) <= 1e-10 * np.max(np.abs(ref[key])) + 4e-16 * big, key
    dm.close()


def test_refusals():
    from membrane_solver_amd import _lib as L
    from membrane_solver_amd import meshgen
    from membrane_solver_amd.device import DeviceMesh

    P, T, _B = meshgen.disk_patch(44)  # 5941 vertices
    dm = DeviceMesh(P, T)
    dm.set_leaflet_tilts("in", np.zeros_like(P), tilt_modulus=1.0)
    dm.set_leaflet_tilts("out", np.zeros_like(P), tilt_modulus=1.0)
    bit = L.MS_MOD_RIM_SLOPE_MATCH_OUT
    with pytest.raises(L.MembraneHipError, match="never called"):  # the bit without tables
        dm.set_params(modules=L.MS_MOD_TILT_OUT | bit)
        dm.energy()
    ok = {"rim": [1, 2, 3], "outer": [7, 8, 9, 10], "disk": [4, 5], "strength": 1.0}
    for bad, why in (({"rim": np.arange(4097)}, "a rim ring of 4097 rows is above the 4096"),
                     ({"outer": np.arange(100, 4197)}, "an outer ring of 4097 rows is above the 4096"),
                     ({"disk": np.arange(100, 4197)}, "a disk ring of 4097 rows is above the 4096"),
                     ({"rim": [1, 2, 1]}, "listed twice"), ({"outer": [7, 8, 3]}, "listed twice"),
                     ({"disk": [4, 7]}, "listed twice"), ({"rim": [1, len(P)]}, "out of range"),
                     ({"outer": [-1, 8]}, "out of range"), ({"rim": []}, "at least one row"), ({"outer": []}, "at least one row"),
                     ({"strength": np.nan}, "must be finite"), ({"center": (0.0, np.inf, 0.0)}, "must be finite"),
                     ({"normal": (np.nan, 0.0, 1.0)}, "must be finite"), ({"normal": (0.0, 0.0, 0.0)}, "non-zero plane normal")):
        with pytest.raises(L.MembraneHipError, match=why):
            dm.set_rim_match(**dict(ok, **bad))
    # the largest rings run: 4096 rim rows against 1845 outer rows (interpolated), no disk
    dm.set_rim_match(np.arange(4096), np.arange(4096, len(P)), None, strength=1.0)
    dm.set_params(modules=bit)
    E_big = dm.energy()[3]
    assert np.isfinite(E_big)
    with pytest.raises(L.MembraneHipError, match="listed twice"):  # a refused call leaves the tables in use as they were
        dm.set_rim_match(**dict(ok, rim=[1, 2, 1]))
    assert dm.energy()[3] == E_big
    with pytest.raises(L.MembraneHipError, match="single-field"):
        dm.set_params(modules=L.MS_MOD_TILT | bit)
    dm.set_rim_match(None)  # cleared: the bit is refused again
    dm.set_params(modules=bit)
    with pytest.raises(L.MembraneHipError, match="never called"):
        dm.energy()
    dm.close()


@pytest.mark.parametrize("tile", [0, 64])
def test_next_to_tilt_coupling_and_thetab_contact(tile):
    """Added next to tilt_coupling and tilt_thetaB_contact_in: each module's gradient rows and own energy are unchanged by
    the others' presence, and the sum is the sum."""
    from membrane_solver_amd import _lib as L

    name = "disk_mean_outer_plus1"
    dm, P, _tin, _tout, gp = _device(name, tile, True, modules=0, tilt_modulus=1.1)
    dm.set_tilt_coupling(0.8, -1)
    dm.set_thetab_contact(CASES[name + "__disk"], center=gp["rim_slope_match_center"], normal=(0.0, 0.0, 1.0), k=2.0,
                          gamma=0.4, work_mode="field_linear", penalty_mode="legacy")
    dm.set_thetab_value(0.07)
    base = L.MS_MOD_TILT_IN | L.MS_MOD_TILT_OUT
    bits = {"rsm": L.MS_MOD_RIM_SLOPE_MATCH_OUT, "cpl": L.MS_MOD_TILT_COUPLING, "tb": L.MS_MOD_TILT_THETAB_CONTACT_IN}

    def run(extra):
        dm.set_params(modules=base | extra)
        E, gi, go = dm.leaflet_tilt_energy_and_gradient()
        e, g = dm.energy_and_gradient(want_grad=True, raw=True)
        assert e[3] == E
        return E, gi, go, g

    E0, gi0, go0, g0 = run(0)
    alone = {k: run(b) for k, b in bits.items()}
    own_alone = dm.rim_match_energies()  # ("tb" ran last without the bit: the getter keeps the last evaluation's)
    Ea, gia, goa, ga = run(bits["rsm"] | bits["cpl"] | bits["tb"])
    own = dm.rim_match_energies()
    E_ref, ref = expected(name, len(P))
    assert own == own_alone and abs(own[0] - E_ref) <= 1e-12 * abs(E_ref)
    assert abs((alone["rsm"][0] - E0) - E_ref) <= 1e-12 * (abs(E_ref) + abs(E0))
    dE = sum(alone[k][0] - E0 for k in bits)
    assert abs((Ea - E0) - dE) <= 1e-12 * (abs(Ea) + abs(E0))
    for idx, key in ((1, "tilt_in_grad"), (2, "tilt_out_grad"), (3, "grad")):
        big = float(np.max(np.abs(alone["rsm"][idx]))) + float(np.max(np.abs(ga if idx == 3 else gia)))
        # the rim matching term's rows, with and without the others
        d_alone = alone["rsm"][idx] - (E0, gi0, go0, g0)[idx]
        assert np.max(np.abs(d_alone - ref[key])) <= 1e-10 * np.max(np.abs(ref[key])) + 4e-16 * big
        d_all = (Ea, gia, goa, ga)[idx] - (E0, gi0, go0, g0)[idx]
        d_sum = sum(alone[k][idx] - (E0, gi0, go0, g0)[idx] for k in bits)
        assert np.max(np.abs(d_all - d_sum)) <= 8e-16 * big, key
    dm.close()


# ---------------------------------------------------------------------------------------------------------------------
def _opts(text):
    return {int(k): v for k, v in json.loads(str(text)).items()}


def _relax(g, with_module=True, tile=0, deterministic=None, exec_off=False):
    from membrane_solver_amd.geometry.mesh import ArrayMesh
    from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager
    from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager
    from membrane_solver_amd.runtime.minimizer import Minimizer
    from membrane_solver_amd.runtime.steppers import GradientDescent

    mods = [str(m) for m in g["modules"] if with_module or str(m) != NAME]
    mesh = ArrayMesh(g["positions"], g["tri"], fixed=g["fixed"], tilts_in=g["tilts_in0"], tilts_out=g["tilts_out0"],
                     global_parameters=json.loads(str(g["gp_json"])), energy_modules=mods, constraint_modules=[],
                     edges=g["edges"], vertex_options=_opts(g["vopts"]))
    mz = Minimizer(mesh, mesh.global_parameters, GradientDescent(), EnergyModuleManager(mods), ConstraintModuleManager([]),
                   quiet=True, tile_vertices=tile, deterministic=deterministic)
    _mir, dm = mz._device()
    dm.energy()  # (leaves the bending_tilt record the relaxation would otherwise take first, on positions not yet frozen)
    before = dm.rim_match_stats()
    iters, evals = dm.relax_leaflet_tilts(**mz._tilt_relax_params())
    after = dm.rim_match_stats()
    return mz, dm, iters, evals, {k: after[k] - before[k] for k in after}


@pytest.mark.parametrize("tile", [0, 64])
def test_relaxation_matches_reference(tile):
    """One nested CG relaxation of 40 iterations with both leaflets' tilt and bending_tilt modules and this one (rim 18,
    outer 24: interpolated; disk 12: the mean variant), on one tile and on several.  The rings are ordered ONCE:
    positions are frozen; every evaluation applies the tables: 1 geometry launch and as many applies as evaluations."""
    from membrane_solver_amd import _lib as L

    g = load_golden("rim_slope_match_relax.npz")
    mz, dm, iters, evals, d = _relax(g, tile=tile)
    assert dm.modules & L.MS_MOD_RIM_SLOPE_MATCH_OUT
    assert (dm.tile_stats()["n_tiles"] == 1) == (tile == 0)
    tin, tout = dm.get_leaflet_tilts("in"), dm.get_leaflet_tilts("out")
    E = float(dm.energy().sum())
    own = dm.rim_match_energy()
    bar_t, bar_e = _bar(g, "noise_tilts"), _bar(g, "noise_energy")
    n_grad, n_en = int(g["n_gradient_evaluations"]), int(g["n_energy_evaluations"])
    print("tile", tile, "iters", iters, "evals", evals, "ref", n_grad, n_en, "E", E, "ref", float(g["E_total"]), "relerr",
          relerr(tin, g["tilts_in_final"]), relerr(tout, g["tilts_out_final"]), "bars", bar_t, bar_e, "own", own,
          float(g["E_own"]), "launches", d)
    assert iters == n_grad - 1 == int(g["tilt_inner_steps"]) == 40
    assert evals == n_grad + n_en
    assert relerr(tin, g["tilts_in_final"]) <= bar_t and relerr(tout, g["tilts_out_final"]) <= bar_t
    assert abs(E - float(g["E_total"])) <= bar_e * abs(float(g["E_total"]))
    assert abs(own - float(g["E_own"])) <= bar_e * abs(float(g["E_total"]))
    st = dm.exec_stats()
    assert st["relax_fused"] == 0 and st["relax_programs"] == 0  # (the one-tile lanes decline)
    assert dm.tsearch_stats()["passes"] == 0  # (and so does the multi-trial search pass of multi-tile meshes)
    assert d["geom_launches"] == 1, "the geometry pass runs once per relaxation"
    assert d["apply_launches"] == evals == 1 + 2 * 40 + 1
    bd = mz.compute_energy_breakdown()
    assert abs(bd[NAME] - float(g["E_own"])) <= bar_e * abs(float(g["E_total"]))
    assert abs(sum(bd.values()) - float(g["E_total"])) <= bar_e * abs(float(g["E_total"]))


def test_relaxation_repeats_bitwise_in_fixed_order_mode_and_closely_in_default_mode():
    g = load_golden("rim_slope_match_relax.npz")
    for det in (False, True):
        runs = []
        for _ in range(2):
            _mz, dm, _i, _e, _d = _relax(g, tile=64, deterministic=det)
            runs.append((dm.get_leaflet_tilts("in"), dm.get_leaflet_tilts("out"), dm.rim_match_energies()))
        if det:
            assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
            assert runs[0][2] == runs[1][2]
        else:  # (the tile kernels' LDS-atomic sums are not ordered; the module's own sums are: see the case tests)
            assert relerr(runs[0][0], runs[1][0]) < 1e-9 and relerr(runs[0][1], runs[1][1]) < 1e-9


def test_context_without_the_module_keeps_its_fast_lanes():
    """The same relaxation without the module: the fused evaluator and the relaxation program run as before on one
    tile, the search pass on several."""
    g = load_golden("rim_slope_match_relax.npz")
    _mz, dm, _iters, evals, d = _relax(g, with_module=False)
    st = dm.exec_stats()
    assert evals > 0 and st["relax_fused"] > 0 and st["relax_programs"] > 0
    assert d["geom_launches"] == 0 and d["apply_launches"] == 0
    _mz, dm, _iters, evals, d = _relax(g, with_module=False, tile=64)
    assert evals > 0 and dm.tsearch_stats()["passes"] > 0 and d["geom_launches"] == 0


def _step_minimizer(g, strength, mods=("surface", "tilt_in", "tilt_out", NAME), **gp_extra):
    from membrane_solver_amd.geometry.mesh import ArrayMesh
    from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager
    from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager
    from membrane_solver_amd.runtime.minimizer import Minimizer
    from membrane_solver_amd.runtime.steppers import GradientDescent

    gp = dict(json.loads(str(g["gp_json"])), surface_tension=1.0, rim_slope_match_strength=strength, tilt_inner_steps=3,
              mesh_quality_auto_repair_enabled=False, **gp_extra)
    mods = list(mods)
    mesh = ArrayMesh(g["positions"], g["tri"], fixed=g["fixed"], tilts_in=g["tilts_in0"], tilts_out=g["tilts_out0"],
                     global_parameters=gp, energy_modules=mods, constraint_modules=[], edges=g["edges"],
                     vertex_options=_opts(g["vopts"]))
    return mesh, Minimizer(mesh, mesh.global_parameters, GradientDescent(), EnergyModuleManager(mods),
                           ConstraintModuleManager([]), quiet=True, step_size=1e-2, deterministic=True)


def test_shape_step_orders_the_rings_at_every_evaluation_and_declines_the_resident_lanes():
    """A shape step of the Minimizer's context: one geometry launch per evaluation (the trials, the energy at x, the
    re-add behind k_tilt<1> of the gradient pass, the accepted trial's commit); the one-tile recorder's programs and
    the resident step stay unused; ms_minimize against the Python loop: the same bits."""
    from membrane_solver_amd import _lib as L

    g = load_golden("rim_slope_match_relax.npz")
    _mesh, mz = _step_minimizer(g, 0.1)
    _mir, dm = mz._device()
    assert dm.modules & L.MS_MOD_RIM_SLOPE_MATCH_OUT
    before = dm.rim_match_stats()
    r = dm.step(stepper=L.MS_STEPPER_GD, step_size=1e-2, tol=0.0)
    after = dm.rim_match_stats()
    d_geom = after["geom_launches"] - before["geom_launches"]
    d_apply = after["apply_launches"] - before["apply_launches"]
    n = r.trials + r.guard_rejects
    print("trials", r.trials, "guard rejects", r.guard_rejects, "geom", d_geom, "apply", d_apply, "success", r.success)
    assert r.success and n >= 1
    assert d_geom == d_apply == n + 3
    rs_ = dm.resident_stats()
    assert rs_["launches"] == 0 and rs_["steps"] == 0  # (the resident step declines every tilt-family module)
    # the library's loop against the Python loop stepping the same context calls
    finals = []
    for observe in (True, False):
        mesh2, mz2 = _step_minimizer(g, 0.1)
        if observe:
            orig = mz2.stepper.device_step
            mz2.stepper.device_step = lambda *a, **k: orig(*a, **k)
        res = mz2.minimize(3)
        assert mz2._fast_path_ok(None) == (not observe)
        finals.append((mesh2.positions_view().copy(), np.array(mesh2.tilts_in_view()).copy(),
                       np.array(mesh2.tilts_out_view()).copy(), res["energy"]))
    for x, y in zip(*finals):
        assert np.array_equal(x, y)
    assert np.max(np.abs(finals[0][0] - g["positions"])) > 0.0


def test_minimizer_refuses_what_the_issue_lists():
    """Through Minimizer._device(): no outer-leaflet module, a single-field tilt module next to it, a disk group without
    an inner-leaflet module, a staggered mode, a missing normal -- each with its own text, before anything runs; and a
    non-zero strength next to tilt_out alone, without the disk group, runs."""
    from membrane_solver_amd import _lib as L

    g = load_golden("rim_slope_match_relax.npz")
    for kw, text in ((dict(mods=("surface", NAME)), "without an active outer-leaflet tilt module"),
                     (dict(mods=("surface", "tilt_in", NAME)), "without an active outer-leaflet tilt module"),
                     (dict(mods=("surface", "tilt", "tilt_out", NAME), tilt_rigidity=1.0), "single-field tilt module"),
                     (dict(mods=("surface", "tilt_out", NAME)), "a disk group, without an active inner-leaflet"),
                     (dict(rim_slope_match_mode="shared_rim_staggered_v1"), "rim_slope_match_mode=shared_rim_staggered_v1"),
                     (dict(rim_slope_match_normal=None), "without a non-zero rim_slope_match_normal")):
        _mesh, mz = _step_minimizer(g, 2.0, **kw)
        with pytest.raises(L.MembraneHipError, match=text):
            mz.compute_energy()
    _mesh, mz = _step_minimizer(g, 2.0, mods=("surface", "tilt_out", NAME), rim_slope_match_disk_group=None)
    bd = mz.compute_energy_breakdown()
    assert bd[NAME] > 0.0 and abs(sum(bd.values()) - mz.compute_energy()) <= 1e-12 * abs(mz.compute_energy())
    _mir, dm = mz._device()
    assert dm.rim_match_energies()[2] == 0.0


# ---------------------------------------------------------------------------------------------------------------------
TRAJ = ("traj_disk6_gd_rsm_weak_unequal.npz", "traj_disk6_cg_rsm_strong_pins.npz", "traj_deck_gd_rsm_profile.npz")
KIND = {TRAJ[0]: "gd", TRAJ[1]: "cg", TRAJ[2]: "gd"}


def _traj_minimizer(g, kind, observe, tile=0, deterministic=None):
    from membrane_solver_amd.geometry.mesh import ArrayMesh
    from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager
    from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager
    from membrane_solver_amd.runtime.minimizer import Minimizer
    from membrane_solver_amd.runtime.steppers import ConjugateGradient, GradientDescent

    mods = [str(m) for m in g["modules"]]
    cons = [str(m) for m in g["constraint_modules"]]
    vo, gp = _opts(g["vopts"]), json.loads(str(g["gp_json"]))
    # (an array mesh carries the disk target's rows as an attribute, not in its vertex options)
    disk = {lf: sorted(r for r, o in vo.items() if gp.get("tilt_disk_target_group_" + lf) is not None
                       and o.get("tilt_disk_target_group_" + lf) == gp["tilt_disk_target_group_" + lf]) for lf in ("in", "out")}
    disk = {"disk_rows_" + lf: np.array(rows, dtype=np.int64) for lf, rows in disk.items() if rows}
    mesh = ArrayMesh(g["positions0"], g["tri"], fixed=g["fixed"], surface_tension=g["gamma"], tilts_in=g["tilts_in0"], **disk,
                     tilts_out=g["tilts_out0"], tilt_fixed_in=g["tilt_fixed_in"], tilt_fixed_out=g["tilt_fixed_out"],
                     global_parameters=gp, energy_modules=mods, constraint_modules=cons, edges=g["edges"], vertex_options=vo)
    stepper = GradientDescent() if kind == "gd" else ConjugateGradient()
    log, counts = [], []
    mz = Minimizer(mesh, mesh.global_parameters, stepper, EnergyModuleManager(mods), ConstraintModuleManager(cons),
                   quiet=True, step_size=float(g["step_size0"]), tile_vertices=tile, deterministic=deterministic)
    if observe:
        orig = stepper.device_step

        def logged(dm, m, step_size, tol=0.0):
            before = dm.rim_match_stats()
            r = orig(dm, m, step_size, tol=tol)
            after = dm.rim_match_stats()
            log.append((float(r.success), r.next_step, r.energy))
            counts.append((r.trials, r.guard_rejects, after["geom_launches"] - before["geom_launches"],
                           after["apply_launches"] - before["apply_launches"]))
            return r

        stepper.device_step = logged
    return mesh, mz, log, counts


@pytest.mark.parametrize("tile", [0, 64])
@pytest.mark.parametrize("fname", TRAJ)
def test_minimizer_reproduces_trajectory(fname, tile):
    """Five steps with unequal counts and the mean-disk variant next to tilt_in + tilt_out (the first: and surface) -- GD with strength
    0.1 and a nested relaxation; CG with strength 200, a coupled relaxation and the rim pinned to its circle (searches
    that backtrack, steps that fail); and the reference's own kozlov_1disk_3d_tensionless_single_leaflet_profile deck
    (its mesh turned off atan2's branch cut, its eight energy modules, pin_to_plane and fixed pin_to_circle on rim and
    outer ring, strength 200, coupled relaxation of 40 steps, fixed step mode) -- on one tile and on several: observed steps (the Python loop) and unobserved ones (ms_minimize) give the reference's
    decisions and step sizes exactly, energies and finals within the fixture's noise bar, the reference's evaluation
    count per line search and one geometry launch per evaluation of a shape step; the breakdown reports the module's own
    energy and sums to the total.

    The pinned trajectory lists no surface module, as the deck it stands in for: the reference's relaxation accepts a tilt
    step on E_tilt-dependent(trial) <= E_total(x) (runtime/steppers/tilt_relaxation.py:894, :954-962), the device compares
    tilt-dependent energies on both sides, and the two differ once a relaxation step backtracks next to a tilt-independent
    module."""
    g = load_golden(fname)
    for observe in (True, False):
        mesh, mz, log, counts = _traj_minimizer(g, KIND[fname], observe, tile=tile)
        if observe:
            E0, grad0 = mz.compute_energy_and_gradient_array()
            print("E0", E0, float(g["E0"]), "grad0", relerr(grad0, g["grad0"]))
            assert abs(E0 - g["E0"]) <= 1e-12 * abs(g["E0"])
            assert relerr(grad0, g["grad0"]) < 1e-10
        res = mz.minimize(int(g["n_steps"]))
        assert mz._fast_path_ok(None) == (not observe)
        if observe:
            got, ref = np.array(log), g["step_log"]
            cnt = np.array(counts)
            print(fname, tile, "got", got.tolist(), "ref", ref.tolist(), "trials, guard rejects, geom, apply", cnt.tolist(),
                  "ref evals per search", g["line_search_evals"].tolist())
            assert got.shape == ref.shape
            assert np.array_equal(got[:, 0], ref[:, 0]), "accept/reject sequence differs from the reference"
            assert np.allclose(got[:, 1], ref[:, 1], rtol=1e-12, atol=0)
            assert np.allclose(got[:, 2], ref[:, 2], rtol=_bar(g, "noise_energy"), atol=0)
            # the reference takes the module once at x and once per trial it puts to the Armijo test; a trial its
            # step-length guard refuses is not evaluated there, while the device has taken its energy pass by then
            assert np.array_equal(cnt[:, 0] + 1, g["line_search_evals"])
            # one geometry launch per evaluation of the step: the trials, the guarded ones, the energy at x, the gradient
            # pass and -- where the step succeeds -- the accepted trial's commit
            ok = got[:, 0] > 0
            assert np.array_equal(cnt[ok, 2], cnt[ok, 0] + cnt[ok, 1] + 3) and np.array_equal(cnt[:, 3], cnt[:, 2])
            assert np.all(cnt[~ok, 2] >= 2)  # (a step that fails: at least the energy at x and the gradient pass)
            bd = mz.compute_energy_breakdown()
            assert abs(sum(bd.values()) - res["energy"]) <= 1e-12 * abs(res["energy"])
            assert abs(bd[NAME] - float(g["E_own_final"])) <= _bar(g, "noise_energy") * abs(float(g["E_final"]))
        else:
            assert mz.last_run["trials"] + int(g["n_steps"]) == int(g["line_search_evals"].sum())
        print("    finals: x", relerr(mesh.positions_view(), g["positions_final"]), "bar", _bar(g, "noise_positions"),
              "t", relerr(mesh.tilts_in_view(), g["tilts_in_final"]), relerr(mesh.tilts_out_view(), g["tilts_out_final"]),
              "bar", _bar(g, "noise_tilts"), "E", abs(res["energy"] - float(g["E_final"])) / abs(float(g["E_final"])),
              "bar", _bar(g, "noise_energy"))
        assert relerr(mesh.positions_view(), g["positions_final"]) <= _bar(g, "noise_positions")
        assert relerr(mesh.tilts_in_view(), g["tilts_in_final"]) <= _bar(g, "noise_tilts")
        assert relerr(mesh.tilts_out_view(), g["tilts_out_final"]) <= _bar(g, "noise_tilts")
        assert abs(res["energy"] - float(g["E_final"])) <= _bar(g, "noise_energy") * abs(float(g["E_final"]))


@pytest.mark.parametrize("fname", TRAJ)
def test_trajectory_repeats_bitwise_in_fixed_order_mode_and_closely_in_default_mode(fname):
    g = load_golden(fname)
    for det in (False, True):
        runs = []
        for _ in range(2):
            mesh, mz, _log, _c = _traj_minimizer(g, KIND[fname], False, tile=64, deterministic=det)
            res = mz.minimize(int(g["n_steps"]))
            runs.append((mesh.positions_view().copy(), np.array(mesh.tilts_in_view()).copy(),
                         np.array(mesh.tilts_out_view()).copy(), res["energy"]))
        if det:
            for x, y in zip(*runs):
                assert np.array_equal(x, y)
        else:  # (the tile kernels' LDS-atomic sums are not ordered; the module's own sums are: see the case tests)
            assert relerr(runs[0][0], runs[1][0]) < 1e-9
