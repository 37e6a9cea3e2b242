"""leaflet_out_absent_presets on the device: tilt_out and tilt_smoothness_out with the outer leaflet absent on some rows
(ms_set_leaflet_absent, VF_ABSENT_OUT) against the reference's golden vectors (tools/gen_golden_leaflet_absent.py): the
modules' energies and gradients, the relaxation's masked vertex areas and Jacobi diagonal, a 40-iteration relaxation, a
6-step trajectory, the lanes that honour the mask against each other and the lanes that step aside under one.

Bounds: energies 1e-12 relative, gradients 1e-10 of their largest entry (the device bounds of every module here);
relaxed fields 1e-9 and trajectory finals 1e-8 (what test_gpu_leaflet.py asks of the same drivers; the fixtures'
own noise under a 1e-13 perturbation is asserted below 1e-9 when they are written)."""

import json
import os

import numpy as np
import pytest

from conftest import load_golden, relerr

pytestmark = pytest.mark.gpu

G = load_golden("leaflet_absent_cases.npz")
NAMES = [str(n) for n in G["names"]]
MODS = ("tilt_in", "tilt_out", "tilt_smoothness_in", "tilt_smoothness_out")


class _Env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            os.environ[k] = v

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _opts(text):
    return {int(k): v for k, v in json.loads(str(text)).items()}


def _case(name, masked=True):
    from membrane_solver_amd.geometry.mesh import ArrayMesh

    mname = str(G[name + "__mesh"])
    P, T = G["mesh__" + mname + "__positions"], G["mesh__" + mname + "__tri"]
    gp = json.loads(str(G[name + "__gp"]))
    if not masked:
        gp["leaflet_out_absent_presets"] = []
    mesh = ArrayMesh(P, T, global_parameters=gp, tilts_in=G[name + "__tilts_in"], tilts_out=G[name + "__tilts_out"],
                     vertex_options=_opts(G[name + "__vopts"]), tilt_fixed_out=G[name + "__tilt_fixed_out"])
    return mesh, P, T, gp


def _plugin(mesh, mod, P, tin, tout):
    from membrane_solver_amd.core.parameters import ParameterResolver
    from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager

    module = EnergyModuleManager([mod]).get_module(mod)
    grad, tg = np.zeros_like(P), np.zeros_like(P)
    kw = {"tilt_in_grad_arr": tg} if mod.endswith("_in") else {"tilt_out_grad_arr": tg}
    E = module.compute_energy_and_gradient_array(mesh, mesh.global_parameters, ParameterResolver(mesh.global_parameters),
                                                 positions=P, index_map=mesh.vertex_index_to_row, grad_arr=grad,
                                                 tilts_in=tin, tilts_out=tout, **kw)
    return float(E), grad, tg


@pytest.mark.parametrize("name", NAMES)
def test_modules_match_reference(name, deterministic):
    """Each module through the reference's plugin signature: the outer modules against the masked goldens, the inner
    ones against theirs and BITWISE what they are on the same mesh without a mask."""
    mesh, P, _T, _gp = _case(name)
    bare, _P, _T2, _gp2 = _case(name, masked=False)
    tin, tout = G[name + "__tilts_in"], G[name + "__tilts_out"]
    key = {"tilt_out": "tilt_out", "tilt_smoothness_out": "smooth_out", "tilt_in": "tilt_in", "tilt_smoothness_in": "smooth_in"}
    for mod in MODS:
        E, grad, tg = _plugin(mesh, mod, P, tin, tout)
        k = key[mod]
        want_E = float(G[f"{name}__E_{k}"])
        want_tg = G[f"{name}__tilt_grad_{k}"]
        want_g = G[f"{name}__grad_{k}"] if "smooth" not in k else np.zeros_like(P)
        print(name, mod, "E", E, want_E, "grad", relerr(grad, want_g) if want_g.any() else 0.0, "tilt grad",
              relerr(tg, want_tg) if want_tg.any() else 0.0)
        assert abs(E - want_E) <= 1e-12 * abs(want_E)
        for got, want in ((grad, want_g), (tg, want_tg)):
            if want.any():
                assert relerr(got, want) <= 1e-10
            else:
                assert not got.any()
        if mod.endswith("_in"):
            E0, g0, t0 = _plugin(bare, mod, P, tin, tout)
            assert E == E0 and np.array_equal(grad, g0) and np.array_equal(tg, t0)
    if str(G[name + "__what"]) == "all":  # no kept facet: energy 0, gradients 0
        for mod in ("tilt_out", "tilt_smoothness_out"):
            E, grad, tg = _plugin(mesh, mod, P, tin, tout)
            assert E == 0.0 and not grad.any() and not tg.any()


def _context(name, absent="golden", tile=0, env=None, mass=None):
    """A context with both fields, the four modules and (unless ``absent`` is None) the mask set by hand."""
    from membrane_solver_amd import _lib as L
    from membrane_solver_amd.device import DeviceMesh

    mname = str(G[name + "__mesh"])
    P, T = G["mesh__" + mname + "__positions"], G["mesh__" + mname + "__tri"]
    gp = json.loads(str(G[name + "__gp"]))
    with _Env(**(env or {})):
        dm = DeviceMesh(P, T, tile_vertices=tile)
    fout = G[name + "__tilt_fixed_out"]
    dm.set_leaflet_tilts("in", G[name + "__tilts_in"], tilt_modulus=gp["tilt_modulus_in"], mass_mode=gp["tilt_mass_mode_in"],
                         smoothness=gp["bending_modulus_in"])
    dm.set_leaflet_tilts("out", G[name + "__tilts_out"], tilt_fixed=fout if fout.any() else None,
                         tilt_modulus=gp["tilt_modulus_out"], mass_mode=mass or gp["tilt_mass_mode_out"],
                         smoothness=gp["bending_modulus_out"])
    if isinstance(absent, str):
        absent = G[name + "__absent"]
    if absent is not None:
        dm.set_leaflet_absent("out", absent)
    dm.set_params(modules=L.MS_MOD_TILT_IN | L.MS_MOD_TILT_OUT | L.MS_MOD_TILT_SMOOTH_IN | L.MS_MOD_TILT_SMOOTH_OUT)
    return dm


@pytest.mark.parametrize("name", NAMES)
def test_relaxation_geometry_matches_reference(name):
    """The outer leaflet's vertex areas are the kept facets' thirds, its diagonal k_t A_v(masked) + the unmasked smoothness
    part, clamped; the inner leaflet's are what they are without a mask."""
    dm = _context(name)
    dm.relax_leaflet_tilts(solver="cg", max_iters=1, step_size=0.05, jacobi=True)
    va_out, minv_out = dm.leaflet_relax_geometry("out")
    va_in, minv_in = dm.leaflet_relax_geometry("in")
    dm.close()
    scale = float(np.max(G[name + "__va_in"]))
    for got, key in ((va_out, "va_out"), (va_in, "va_in")):
        print(name, key, float(np.max(np.abs(got - G[f"{name}__{key}"]))) / scale)
        assert np.max(np.abs(got - G[f"{name}__{key}"])) <= 1e-12 * scale
    absent = G[name + "__absent"]
    assert not va_out[absent].any()
    for got, key in ((minv_out, "minv_out"), (minv_in, "minv_in")):
        print(name, key, relerr(got, G[f"{name}__{key}"]))
        assert relerr(got, G[f"{name}__{key}"]) <= 1e-10
    assert np.all(minv_out[G[name + "__tilt_fixed_out"]] == 1.0)


def _evaluate_all(dm):
    from membrane_solver_amd import _lib as L

    e, g = dm.energy_and_gradient()
    sc = dm.fetch_scalars()
    E, gi, go = dm.leaflet_tilt_energy_and_gradient()
    it, ev = dm.relax_leaflet_tilts(solver="cg", max_iters=4, step_size=0.05, jacobi=True)
    return (e.copy(), g.copy(), float(sc[L.MS_S_ETILT_OUT]), float(sc[L.MS_S_ETS_OUT]), E, gi, go, it, ev,
            dm.get_leaflet_tilts("in").copy(), dm.get_leaflet_tilts("out").copy()) + dm.leaflet_relax_geometry("out")


@pytest.mark.parametrize("tile", [0, 64])
def test_no_mask_control(tile, deterministic):
    """With the mask unset -- cleared, or set to no row -- every result is bitwise that of a context on which
    ms_set_leaflet_absent was never called; with it set, the results differ."""
    name = "disk4_ring2_consistent"
    runs = []
    for how in ("never", "cleared", "empty", "set"):
        dm = _context(name, absent=None if how == "never" else "golden", tile=tile)
        if how == "cleared":
            dm.set_leaflet_absent("out", None)
        if how == "empty":
            dm.set_leaflet_absent("out", np.zeros(dm.nv, bool))
        runs.append(_evaluate_all(dm))
        dm.close()
    for other in runs[1:3]:
        for a, b in zip(runs[0], other):
            assert np.array_equal(a, b)
    assert runs[3][2] != runs[0][2] and runs[3][3] != runs[0][3]


def test_absent_rows_leave_no_trace(deterministic):
    """The reference's test_outer_leaflet_absent_disk restated: t_out of an absent row changes no outer energy (here: not
    a bit of it, nor of any gradient row but its own projection), t_out of a present row does."""
    from membrane_solver_amd import _lib as L

    name = "disk12_cross_lumped"
    absent = G[name + "__absent"]
    tout = G[name + "__tilts_out"].copy()
    gp = json.loads(str(G[name + "__gp"]))

    def energies(t):
        dm = _context(name)
        dm.set_leaflet_tilts("out", t, tilt_modulus=gp["tilt_modulus_out"], smoothness=gp["bending_modulus_out"])
        dm.energy()
        sc = dm.fetch_scalars()
        E, _gi, go = dm.leaflet_tilt_energy_and_gradient()
        dm.close()
        return float(sc[L.MS_S_ETILT_OUT]), float(sc[L.MS_S_ETS_OUT]), E, go

    base = energies(tout)
    t1 = tout.copy()
    t1[np.flatnonzero(absent)[3]] += [0.25, -0.1, 0.05]
    moved = energies(t1)
    assert moved[:3] == base[:3] and np.array_equal(moved[3], base[3])
    assert not base[3][absent].any()
    t2 = tout.copy()
    t2[np.flatnonzero(~absent)[40]] += [0.25, -0.1, 0.05]
    other = energies(t2)
    assert other[0] != base[0] and other[1] != base[1]


def _relax(tag, tile=0, env=None, deterministic=None):
    g = load_golden("leaflet_absent_relax.npz")
    return _relax_with(tag, json.loads(str(g[tag + "__gp_json"])), tile, env, deterministic)


@pytest.mark.parametrize("tag", ["disk4", "disk12"])
def test_relaxation_matches_reference(tag):
    """A nested CG relaxation of 40 iterations, the outer leaflet absent on the inner rings, an absent and a present row
    clamped: on one tile (the interpreter's relaxation program replays the masked bodies) and on two (the mask edge
    crosses the tile boundary).  Fields, iterations, evaluations (accepted steps = gradient evaluations - 1); the fused
    lanes stepped aside."""
    from membrane_solver_amd.modules.energy import leaflet_common as lc

    g, mz, dm, iters, evals = _relax(tag)
    n_grad, n_en = int(g[tag + "__n_gradient_evaluations"]), int(g[tag + "__n_energy_evaluations"])
    tin, tout = dm.get_leaflet_tilts("in"), dm.get_leaflet_tilts("out")
    absent = g[tag + "__absent"]
    E = float(dm.energy().sum())
    print(tag, "iters", iters, "evals", evals, "ref", n_grad, n_en, "relerr", relerr(tin, g[tag + "__tilts_in_final"]),
          relerr(tout, g[tag + "__tilts_out_final"]), "E", E, float(g[tag + "__E_total"]), "tiles", dm.tile_stats()["n_tiles"])
    assert (dm.tile_stats()["n_tiles"] == 1) == (tag == "disk4")
    assert iters == n_grad - 1 == int(g[tag + "__n_accepted"]) == 40
    assert evals == n_grad + n_en
    assert relerr(tin, g[tag + "__tilts_in_final"]) <= 1e-9 and relerr(tout, g[tag + "__tilts_out_final"]) <= 1e-9
    assert abs(E - float(g[tag + "__E_total"])) <= 1e-9 * abs(float(g[tag + "__E_total"]))
    va_out, _minv = dm.leaflet_relax_geometry("out")
    want = lc.masked_vertex_areas(g[tag + "__positions"], g[tag + "__tri"], absent)
    assert np.max(np.abs(va_out - want)) <= 1e-12 * np.max(want) and not va_out[absent].any()
    # the fallbacks: no fused evaluator run, no search / gradient pass
    st = dm.exec_stats()
    assert st["relax_fused"] == 0 and dm.tsearch_stats()["passes"] == 0
    if tag == "disk4":
        assert st["relax_programs"] > 0  # (the one-tile program replays k_tilt / k_tsmooth / k_tvec: it inherits the mask)
    dm.close()


@pytest.mark.parametrize("tag", ["disk4c", "disk12c"])
@pytest.mark.parametrize("vec", ["1", "0"])
def test_relaxation_with_tilt_coupling_matches_reference(tag, vec):
    """The same relaxations with tilt_coupling in the list.  The coupling is not masked (tilt_coupling.py:160-203 takes
    every facet): its frozen-surface lane k_couple_vec reads the INNER leaflet's vertex areas while the outer leaflet's
    array holds the kept facets' (vec "1"; the tile kernel k_couple with MS_COUPLE_VEC=0).  With the masked areas the
    absent rows' t_out would stay where the projection put them; the reference moves them."""
    g, mz, dm, iters, evals = _relax(tag, env={"MS_COUPLE_VEC": vec})
    n_grad, n_en = int(g[tag + "__n_gradient_evaluations"]), int(g[tag + "__n_energy_evaluations"])
    tin, tout = dm.get_leaflet_tilts("in"), dm.get_leaflet_tilts("out")
    absent = g[tag + "__absent"]
    E = float(dm.energy().sum())
    st = dm.tilt_coupling_stats()
    print(tag, vec, "iters", iters, "evals", evals, "ref", n_grad, n_en, "relerr", relerr(tin, g[tag + "__tilts_in_final"]),
          relerr(tout, g[tag + "__tilts_out_final"]), "absent rows", relerr(tout[absent], g[tag + "__tilts_out_final"][absent]),
          "E", E, float(g[tag + "__E_total"]), st)
    assert "tilt_coupling" in [str(m) for m in g[tag + "__modules"]]
    assert (st["vec_launches"] > 0) == (vec == "1")
    assert iters == n_grad - 1 == 40 and evals == n_grad + n_en
    assert relerr(tin, g[tag + "__tilts_in_final"]) <= 1e-9 and relerr(tout, g[tag + "__tilts_out_final"]) <= 1e-9
    assert relerr(tout[absent], g[tag + "__tilts_out_final"][absent]) <= 1e-9
    assert abs(E - float(g[tag + "__E_total"])) <= 1e-9 * abs(float(g[tag + "__E_total"]))
    # the outer leaflet's own areas are still the kept facets'
    va_out, _m = dm.leaflet_relax_geometry("out")
    assert not va_out[absent].any()
    dm.close()


def test_lanes_without_a_mask_keep_their_fast_paths():
    """The control of the fallback checks: the same relaxations with the preset list empty run the fused evaluator (one
    tile) and the search pass (two tiles)."""
    for tag, tile in (("disk4", 0), ("disk12", 0)):
        g = load_golden("leaflet_absent_relax.npz")
        gp = dict(json.loads(str(g[tag + "__gp_json"])), leaflet_out_absent_presets=[])
        g2, mz, dm, iters, evals = _relax_with(tag, gp, tile)
        st = dm.exec_stats()
        if tag == "disk4":
            assert st["relax_fused"] > 0
        else:
            assert dm.tsearch_stats()["passes"] > 0
        assert evals > 0
        dm.close()


def _relax_with(tag, gp, tile=0, env=None, deterministic=None):
    from membrane_solver_amd.geometry.mesh import ArrayMesh
    from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager
    from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager
    from membrane_solver_amd.runtime.minimizer import Minimizer
    from membrane_solver_amd.runtime.steppers import GradientDescent

    g = load_golden("leaflet_absent_relax.npz")
    mods = [str(m) for m in g[tag + "__modules"]]
    P = g[tag + "__positions"]
    mesh = ArrayMesh(P, g[tag + "__tri"], fixed=np.ones(len(P), bool), tilts_in=g[tag + "__tilts_in0"],
                     tilts_out=g[tag + "__tilts_out0"], tilt_fixed_out=g[tag + "__tilt_fixed_out"], global_parameters=gp,
                     energy_modules=mods, constraint_modules=[], edges=g[tag + "__edges"],
                     vertex_options=_opts(g[tag + "__vopts"]))
    with _Env(**(env or {})):
        mz = Minimizer(mesh, mesh.global_parameters, GradientDescent(), EnergyModuleManager(mods),
                       ConstraintModuleManager([]), quiet=True, tile_vertices=tile, deterministic=deterministic)
        _mir, dm = mz._device()
    dm.energy()
    iters, evals = dm.relax_leaflet_tilts(**mz._tilt_relax_params())
    return g, mz, dm, iters, evals


def _fields(dm):
    return dm.get_leaflet_tilts("in").copy(), dm.get_leaflet_tilts("out").copy()


def test_interpreter_replays_the_masked_bodies_bit_for_bit():
    """MS_EXEC: the one-workgroup interpreter runs tilt_body / ts_body themselves, so it honours the mask; in fixed-order
    mode its relaxation equals the launch-per-kernel one bit for bit."""
    res = []
    for ex in ("1", "0"):
        _g, _mz, dm, iters, evals = _relax("disk4", env={"MS_EXEC": ex, "MS_DETERMINISTIC": "1"}, deterministic=True)
        assert dm.exec_stats()["active"] == (ex == "1")
        res.append((iters, evals) + _fields(dm) + (dm.energy().copy(),))
        dm.close()
    assert res[0][:2] == res[1][:2]
    for a, b in zip(res[0][2:], res[1][2:]):
        assert np.array_equal(a, b)


def test_fused_evaluator_steps_aside_under_a_mask():
    """MS_EXEC_FUSED: the one-tile fused relaxation evaluator does not read the mask and is not selected while one is set
    (exec_stats: no fused run, the captured program instead); the result agrees with the launch-per-kernel path to 1e-11."""
    _g, _mz, dm, iters, evals = _relax("disk4", env={"MS_EXEC_FUSED": "1"})
    st = dm.exec_stats()
    assert st["active"] and st["relax_fused"] == 0 and st["relax_programs"] > 0
    a = (iters, evals) + _fields(dm)
    dm.close()
    _g, _mz, dm2, iters2, evals2 = _relax("disk4", env={"MS_EXEC": "0"})
    b = (iters2, evals2) + _fields(dm2)
    dm2.close()
    assert a[:2] == b[:2]
    assert relerr(a[2], b[2]) <= 1e-11 and relerr(a[3], b[3]) <= 1e-11


def test_search_and_gradient_passes_step_aside_under_a_mask():
    """MS_TSEARCH: k_tsearch / k_tgrad do not read the mask and are not selected while one is set (tsearch_stats: no
    pass); switching them off changes nothing then -- bit for bit in fixed-order mode."""
    res = []
    for ts in ("1", "0"):
        _g, _mz, dm, iters, evals = _relax("disk12", env={"MS_TSEARCH": ts, "MS_DETERMINISTIC": "1"}, deterministic=True)
        assert dm.tile_stats()["n_tiles"] >= 2 and dm.tsearch_stats()["passes"] == 0
        res.append((iters, evals) + _fields(dm))
        dm.close()
    assert res[0][:2] == res[1][:2]
    assert np.array_equal(res[0][2], res[1][2]) and np.array_equal(res[0][3], res[1][3])


def test_energy_only_pass_steps_aside_under_a_mask():
    """The one-launch energy pass of an energy-only evaluation (k_tsearch with one step size) is not selected while a mask
    is set: the profile counts k_tilt<0> / k_tsmooth<0> launches and no search-kernel launch; without a mask it runs."""
    name = "disk12_cross_lumped"
    for absent, fused in (("golden", False), (None, True)):
        dm = _context(name, absent=absent)
        dm.energy()
        dm.profile_enable(True)
        e = dm.energy()
        prof = dm.profile_read()
        dm.profile_enable(False)
        dm.close()
        print("mask" if absent is not None else "no mask", {k: v[1] for k, v in prof.items() if v[1]})
        if fused:
            assert prof["tilt_search"][1] > 0 and prof["tilt"][1] == 0 and prof["tilt_smoothness"][1] == 0
        else:
            assert prof["tilt_search"][1] == 0 and prof["tilt"][1] >= 2 and prof["tilt_smoothness"][1] >= 2
            want = sum(float(G[f"{name}__E_{k}"]) for k in ("tilt_in", "tilt_out", "smooth_in", "smooth_out"))
            assert abs(e[3] - want) <= 1e-12 * abs(want)


TRAJ = "traj_disk6_gd_leaflet_absent_pins.npz"


def _traj_minimizer(g, observe, tile=0):
    from membrane_solver_amd.geometry.mesh import ArrayMesh
    from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager
    from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager
    from membrane_solver_amd.runtime.minimizer import Minimizer
    from membrane_solver_amd.runtime.steppers import GradientDescent

    mods = [str(m) for m in g["modules"]]
    cons = [str(m) for m in g["constraint_modules"]]
    mesh = ArrayMesh(g["positions0"], g["tri"], fixed=g["fixed"], surface_tension=g["gamma"], tilts_in=g["tilts_in0"],
                     tilts_out=g["tilts_out0"], tilt_fixed_in=g["tilt_fixed_in"], tilt_fixed_out=g["tilt_fixed_out"],
                     global_parameters=json.loads(str(g["gp_json"])), energy_modules=mods, constraint_modules=cons,
                     edges=g["edges"], vertex_options=_opts(g["vopts"]))
    stepper = GradientDescent()
    log = []
    mz = Minimizer(mesh, mesh.global_parameters, stepper, EnergyModuleManager(mods), ConstraintModuleManager(cons),
                   quiet=True, step_size=float(g["step_size0"]), tile_vertices=tile)
    if observe:
        orig = stepper.device_step

        def logged(dm, m, step_size, tol=0.0):
            r = orig(dm, m, step_size, tol=tol)
            log.append((float(r.success), r.next_step, r.energy))
            return r

        stepper.device_step = logged
    return mesh, mz, log


@pytest.mark.parametrize("tile", [0, 64])
def test_minimizer_reproduces_trajectory(tile):
    """Six GD steps: tilt_in, tilt_out, tilt_smoothness_in / _out and bending_tilt_in, the outer leaflet absent on rings
    0-2, slide-mode pin_to_circle on the boundary and fixed-mode pin_to_plane on ring 3, a nested CG relaxation per step:
    the reference's accept / reject sequence and step sizes exactly, observed (the Python loop) and unobserved
    (ms_minimize), on one tile and on several."""
    g = load_golden(TRAJ)
    for observe in (True, False):
        mesh, mz, log = _traj_minimizer(g, observe, tile=tile)
        if observe:
            E0, grad0 = mz.compute_energy_and_gradient_array()
            print("E0", E0, float(g["E0"]), "grad0", relerr(grad0, g["grad0"]))
            assert abs(E0 - g["E0"]) <= 1e-12 * abs(g["E0"])
            assert relerr(grad0, g["grad0"]) < 1e-10
        res = mz.minimize(int(g["n_steps"]))
        if observe:
            got, ref = np.array(log), g["step_log"]
            print(tile, "got", got.tolist(), "ref", ref.tolist())
            assert got.shape == ref.shape
            assert np.array_equal(got[:, 0], ref[:, 0]), "accept/reject sequence differs from the reference"
            assert np.array_equal(got[:, 1], ref[:, 1]), "step sizes differ from the reference"
            assert np.allclose(got[:, 2], ref[:, 2], rtol=1e-9, atol=0)
            bd = mz.compute_energy_breakdown()
            assert abs(sum(bd.values()) - res["energy"]) <= 1e-12 * abs(res["energy"])
            assert abs(bd["tilt_out"] - float(g["E_tilt_out_final"])) <= 1e-9 * abs(float(g["E_final"]))
            assert abs(bd["tilt_smoothness_out"] - float(g["E_smooth_out_final"])) <= 1e-9 * abs(float(g["E_final"]))
        print("    finals: x", relerr(mesh.positions_view(), g["positions_final"]), "t",
              relerr(mesh.tilts_in_view(), g["tilts_in_final"]), relerr(mesh.tilts_out_view(), g["tilts_out_final"]))
        assert relerr(mesh.positions_view(), g["positions_final"]) < 1e-8
        assert relerr(mesh.tilts_in_view(), g["tilts_in_final"]) < 1e-8
        assert relerr(mesh.tilts_out_view(), g["tilts_out_final"]) < 1e-8
        assert abs(res["energy"] - g["E_final"]) <= 1e-9 * abs(g["E_final"])
        mesh._hip_mirror.dm.close()


def test_refusals_through_the_minimizer_and_the_abi():
    """What the Minimizer refuses before anything runs, and the ABI call's own refusals."""
    from membrane_solver_amd import _lib as L
    from membrane_solver_amd.geometry.mesh import ArrayMesh
    from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager
    from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager
    from membrane_solver_amd.runtime.minimizer import Minimizer
    from membrane_solver_amd.runtime.steppers import GradientDescent

    mesh, P, T, gp = _case("disk4_ring1_lumped")
    vo = _opts(G["disk4_ring1_lumped__vopts"])

    def minimizer(m, mods):
        return Minimizer(m, m.global_parameters, GradientDescent(), EnergyModuleManager(mods), ConstraintModuleManager([]),
                         quiet=True)

    with pytest.raises(L.MembraneHipError, match="selects no row.*outside the HIP hot path"):
        minimizer(ArrayMesh(P, T, global_parameters=dict(gp), energy_modules=["tilt_in", "tilt_out"]),
                  ["tilt_in", "tilt_out"]).compute_energy()
    m2 = ArrayMesh(P, T, global_parameters=dict(gp, bending_modulus=0.6), vertex_options=vo,
                   energy_modules=["tilt_out", "bending_tilt_out"])
    with pytest.raises(L.MembraneHipError, match="bending_tilt_out next to a non-empty.*outside the HIP hot path.*follow-up"):
        minimizer(m2, ["tilt_out", "bending_tilt_out"]).compute_energy()
    m3 = ArrayMesh(P, T, global_parameters=dict(gp, leaflet_out_absence_mode="strict"), vertex_options=vo,
                   energy_modules=["tilt_in", "tilt_out"])
    with pytest.raises(ValueError, match="Leaflet absence topology invalid"):
        minimizer(m3, ["tilt_in", "tilt_out"]).compute_energy()
    m4 = ArrayMesh(P, T, global_parameters=dict(gp, leaflet_in_absent_presets=["disk"]), vertex_options=vo,
                   energy_modules=["tilt_in", "tilt_out"])
    with pytest.raises(L.MembraneHipError, match="leaflet_in_absent_presets.*outside the HIP hot path"):
        minimizer(m4, ["tilt_in", "tilt_out"]).compute_energy()
    # accepted: the energy is the masked goldens' sum
    m5 = ArrayMesh(P, T, global_parameters=dict(gp), vertex_options=vo, tilts_in=G["disk4_ring1_lumped__tilts_in"],
                   tilts_out=G["disk4_ring1_lumped__tilts_out"], energy_modules=list(MODS))
    E = minimizer(m5, list(MODS)).compute_energy()
    m5._hip_mirror.dm.close()
    want = sum(float(G[f"disk4_ring1_lumped__E_{k}"]) for k in ("tilt_in", "tilt_out", "smooth_in", "smooth_out"))
    assert abs(E - want) <= 1e-12 * abs(want)
    dm = _context("disk4_ring1_lumped", absent=None)
    with pytest.raises(L.MembraneHipError, match="MS_ERR_UNSUPPORTED.*inner leaflet"):
        dm.set_leaflet_absent("in", G["disk4_ring1_lumped__absent"])
    with pytest.raises(ValueError):
        dm.set_leaflet_absent("out", np.zeros(3, bool))
    dm.close()
