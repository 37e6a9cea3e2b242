"""Host side of tilt_rim_source_bilayer (no GPU): the suffix-free keys and their order, every early return, the frame
rules, the plugin interface against the reference's recorded names, a NumPy restatement of the term against every case of
rim_bilayer_cases.npz, the Minimizer's wiring, refusals and breakdown arithmetic, and the C ABI."""

import ctypes
import inspect
import json
import os
import re

import numpy as np
import pytest

from conftest import load_golden
from minimizer_stub import Refused, install_stub
from membrane_solver_amd import _lib as L
from membrane_solver_amd import meshgen
from membrane_solver_amd.core.parameters import GlobalParameters, ParameterResolver
from membrane_solver_amd.geometry.mesh import ArrayMesh
from membrane_solver_amd.modules.energy import leaflet_common as lc
from membrane_solver_amd.modules.energy import tilt_rim_source_bilayer as plugin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "tilt_rim_source_bilayer"
BIT = L.MS_MOD_TILT_RIM_SOURCE_BILAYER
CASES = load_golden("rim_bilayer_cases.npz")
NAMES = [str(n) for n in CASES["names"]]
G, S = "tilt_rim_source_group", "tilt_rim_source_strength"
MS_ERR_INVALID = -1  # (include/membrane_hip.h)


def _opts(text):
    return {int(k): v for k, v in json.loads(str(text)).items()}


def _ring_rows(r):
    start = 1 + 3 * r * (r - 1)
    return list(range(start, start + 6 * r))


def _edge_table(T):
    seen, rows = set(), []
    for a, b, c in np.asarray(T):
        for u, v in ((a, b), (b, c), (c, a)):
            k = (min(u, v), max(u, v))
            if k not in seen:
                seen.add(k)
                rows.append((int(u), int(v)))
    return np.array(rows, dtype=np.int64)


def _mesh(gp, vopts, eopts=None, n=4, **kw):
    P, T, B = meshgen.disk_patch(n)
    edges = _edge_table(T)
    return ArrayMesh(P, T, global_parameters=dict(gp), vertex_options=vopts, edges=edges, edge_options=eopts or {}, **kw), edges, B


def _params(mesh):
    gp = mesh.global_parameters
    return lc.rim_source_params(mesh, ParameterResolver(gp), gp, None)


def _boundary(n=4):
    return [int(r) for r in np.flatnonzero(meshgen.disk_patch(n)[2])]


def _tag(rows, **extra):
    return {int(r): dict({"pin_to_circle_group": "rim"}, **extra) for r in rows}


# -- keys -------------------------------------------------------------------------------------------------------------
def test_keys_carry_no_leaflet_suffix():
    mesh, _e, _b = _mesh({G: "rim", S: 2.0, "tilt_rim_source_strength_in": 7.0, "tilt_rim_source_group_in": "other",
                          "tilt_rim_source_contact_gamma_out": 9.0}, _tag(_boundary()))
    prm = _params(mesh)
    assert len(prm["tail"]) == 24 and np.all(prm["gamma"] == 2.0)
    # the leaflet modules do not read the suffix-free group either
    gp = mesh.global_parameters
    assert lc.rim_source_params(mesh, ParameterResolver(gp), gp, "out") is None
    mesh2, _e, _b = _mesh({"tilt_rim_source_group_in": "rim", "tilt_rim_source_group_out": "rim", S: 2.0}, _tag(_boundary()))
    assert _params(mesh2) is None  # no suffix-free group: off


def test_strength_resolution_order():
    """edge option, then the global strength, then contact_gamma, then h * ratio, then h * (de / a); the unit conversion."""
    rows = _boundary()
    base = {G: "rim"}
    chain = {"tilt_rim_source_contact_h": 0.5, "tilt_rim_source_contact_delta_epsilon": 6.0, "tilt_rim_source_contact_a": 2.0}
    m, _e, _b = _mesh(dict(base, **chain), _tag(rows))
    assert np.all(_params(m)["gamma"] == 0.5 * (6.0 / 2.0))
    m, _e, _b = _mesh(dict(base, **chain, tilt_rim_source_contact_delta_epsilon_over_a=4.0), _tag(rows))
    assert np.all(_params(m)["gamma"] == 0.5 * 4.0)
    m, _e, _b = _mesh(dict(base, **chain, tilt_rim_source_contact_gamma=0.9), _tag(rows))
    assert np.all(_params(m)["gamma"] == 0.9)
    m, edges, _b = _mesh(dict(base, **chain, tilt_rim_source_contact_gamma=0.9, **{S: 1.5}), _tag(rows))
    assert np.all(_params(m)["gamma"] == 1.5)
    bset = set(rows)
    k0 = next(k for k, (t, h) in enumerate(edges) if int(t) in bset and int(h) in bset)
    m, edges, _b = _mesh(dict(base, **{S: 1.5}), _tag(rows), eopts={k0: {S: 3.5}})
    prm = _params(m)
    hit = [(int(t), int(h)) == tuple(int(v) for v in edges[k0]) for t, h in zip(prm["tail"], prm["head"])]
    assert sum(hit) == 1 and np.all(prm["gamma"][np.array(hit)] == 3.5) and np.all(prm["gamma"][~np.array(hit)] == 1.5)
    si = {"tilt_rim_source_contact_units": "si", "tilt_rim_source_contact_length_unit_m": 1e-8,
          "tilt_rim_source_contact_kappa_ref_J": 4e-20, "tilt_rim_source_contact_gamma": 2e-12}
    m, _e, _b = _mesh(dict(base, **si), _tag(rows))
    assert np.allclose(_params(m)["gamma"], 2e-12 * 1e-8 / 4e-20, rtol=1e-15)


# -- early returns ----------------------------------------------------------------------------------------------------
def _call(mesh, **kw):
    gp = mesh.global_parameters
    nv = len(mesh.vertex_ids)
    args = dict(positions=mesh.positions_view(), index_map=mesh.vertex_index_to_row, grad_arr=None,
                tilts_in=np.zeros((nv, 3)), tilts_out=np.zeros((nv, 3)))
    args.update(kw)
    return plugin.compute_energy_and_gradient_array(mesh, gp, ParameterResolver(gp), **args)


@pytest.mark.parametrize("gp, tagged", [({S: 2.0}, "boundary"), ({G: " ", S: 2.0}, "boundary"), ({G: "rim", S: 2.0}, "ring2"),
                                        ({G: "rim", S: 0.0}, "boundary"), ({G: "rim"}, "boundary")])
def test_early_returns_write_nothing_and_need_no_device(gp, tagged):
    """No group, a blank group, no selected edge (an interior ring in boundary mode), every gamma 0: 0.0 and untouched
    arrays, before any device work (this test has no GPU)."""
    rows = _boundary() if tagged == "boundary" else _ring_rows(2)
    mesh, _e, _b = _mesh(gp, _tag(rows))
    nv = len(mesh.vertex_ids)
    gi, go = np.full((nv, 3), 3.0), np.full((nv, 3), 4.0)
    assert _call(mesh, tilt_in_grad_arr=gi, tilt_out_grad_arr=go) == 0.0
    assert np.all(gi == 3.0) and np.all(go == 4.0)
    res = ParameterResolver(mesh.global_parameters)
    assert plugin.compute_energy_and_gradient(mesh, mesh.global_parameters, res) == (0.0, {}, {}, {})
    assert plugin.compute_energy_and_gradient(mesh, mesh.global_parameters, res, compute_gradient=False) == (0.0, {})


def test_bad_tilt_shape_raises_before_gamma_is_looked_at():
    """:440-462: with a group and a selected edge the tilt shapes are checked before gamma -- every gamma 0 still raises;
    without a selected edge the shapes are never looked at."""
    mesh, _e, _b = _mesh({G: "rim", S: 0.0}, _tag(_boundary()))
    with pytest.raises(ValueError, match="tilts_in must have shape"):
        _call(mesh, tilts_in=np.zeros((3, 3)))
    with pytest.raises(ValueError, match="tilts_out must have shape"):
        _call(mesh, tilts_out=np.zeros((3, 3)))
    mesh2, _e, _b = _mesh({G: "rim", S: 2.0}, _tag(_ring_rows(2)))
    assert _call(mesh2, tilts_in=np.zeros((3, 3))) == 0.0


# -- frame and selection ----------------------------------------------------------------------------------------------
def test_fixed_frame_never_reads_the_rows_normal():
    mesh, _e, _b = _mesh({G: "rim", S: 2.0, "tilt_rim_source_center": [0.1, 0.2, 0.3]},
                         _tag(_boundary(), pin_to_circle_normal=[0.2, -0.1, 1.0]))
    prm = _params(mesh)
    assert prm["normal"] == (0.0, 0.0, 1.0) and prm["center"] == (0.1, 0.2, 0.3) and prm["follow"] is False


def test_follow_frame_takes_the_rows_normal_and_needs_one():
    mesh, _e, _b = _mesh({G: "rim", S: 2.0}, _tag(_boundary(), pin_to_circle_mode="fit", pin_to_circle_normal=[0.0, 3.0, 4.0]))
    prm = _params(mesh)
    assert prm["follow"] is True and np.allclose(prm["normal"], (0.0, 0.6, 0.8), rtol=1e-15)
    mesh2, _e, _b = _mesh({G: "rim", S: 2.0}, _tag(_boundary(), pin_to_circle_mode="fit"))
    with pytest.raises(L.MembraneHipError, match="tilt_rim_source_bilayer in follow mode.*SVD plane fit"):
        _params(mesh2)


def test_edge_modes():
    rows = _boundary() + _ring_rows(2)
    mesh, edges, _b = _mesh({G: "rim", S: 2.0}, _tag(rows))
    assert len(_params(mesh)["tail"]) == 24  # boundary mode: the boundary ring only
    mesh, edges, _b = _mesh({G: "rim", S: 2.0, "tilt_rim_source_edge_mode": "ALL "}, _tag(rows))
    rset = set(rows)
    assert len(_params(mesh)["tail"]) == sum(1 for t, h in edges if int(t) in rset and int(h) in rset) > 24


def test_boundary_mode_keeps_an_edge_with_no_triangle():
    """:67 keeps the edges with FEWER THAN two facets; the leaflet modules' resolver wants exactly one."""
    P, T, _B = meshgen.disk_patch(2)
    edges = np.vstack([_edge_table(T), [[7, 13]]])  # two boundary rows that share no triangle: a dangling edge
    assert not any({7, 13} <= set(map(int, f)) for f in np.asarray(T))
    vo = {7: {"pin_to_circle_group": "rim"}, 13: {"pin_to_circle_group": "rim"}}
    gp = {G: "rim", S: 2.0, "tilt_rim_source_group_in": "rim", "tilt_rim_source_strength_in": 2.0}
    mesh = ArrayMesh(P, T, global_parameters=gp, vertex_options=vo, edges=edges)
    prm = _params(mesh)
    assert prm is not None and sorted((int(prm["tail"][0]), int(prm["head"][0]))) == [7, 13]
    assert lc.rim_source_params(mesh, ParameterResolver(gp), gp, "in") is None


def test_stage_a_lane_is_refused():
    mesh, _e, _b = _mesh({G: "disk", S: 2.0, "tilt_rim_source_edge_mode": "all", "theory_parity_lane": "stage_a_emergent"},
                         {int(r): {"pin_to_circle_group": "disk"} for r in _boundary()})
    with pytest.raises(L.MembraneHipError):
        _call(mesh)


# -- plugin interface -------------------------------------------------------------------------------------------------
def test_plugin_interface_matches_the_reference_names():
    sigs = json.loads(str(CASES["reference_signatures"]))
    for fn, names in sigs.items():
        assert [p for p in inspect.signature(getattr(plugin, fn)).parameters] == names, fn
    flags = json.loads(str(CASES["reference_flags"]))
    assert plugin.USES_TILT_LEAFLETS is flags["USES_TILT_LEAFLETS"] is True
    assert plugin.IS_EXTERNAL_WORK is flags["IS_EXTERNAL_WORK"] is True
    from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager

    assert EnergyModuleManager([NAME]).get_module(NAME) is plugin


# -- the term restated in NumPy -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_numpy_restatement_of_the_term(name):
    g = CASES
    gp = GlobalParameters(json.loads(str(g[name + "__gp"])))
    mesh = ArrayMesh(g[name + "__positions"], g[name + "__tri"], global_parameters=gp, edges=g[name + "__edges"],
                     vertex_options=_opts(g[name + "__vopts"]), edge_options=_opts(g[name + "__eopts"]))
    prm = lc.rim_source_params(mesh, ParameterResolver(gp), gp, None)
    E_ref, tg_ref = float(g[name + "__E"]), g[name + "__tilt_grad"]
    if prm is None:
        assert E_ref == 0.0 and not tg_ref.any() and float(g[name + "__E_scale"]) == 0.0
        return
    assert len(prm["tail"]) == int(g[name + "__n_rim_edges"])
    x, tin, tout = g[name + "__eval_positions"], g[name + "__tilts_in"], g[name + "__tilts_out"]
    t, h, gamma = prm["tail"].astype(int), prm["head"].astype(int), prm["gamma"]
    center, n = np.array(prm["center"]), np.array(prm["normal"])
    if prm["follow"]:  # the mean of the rim rows of the MESH's positions, whatever is evaluated
        center = np.mean(g[name + "__positions"][np.unique(np.concatenate([t, h]))], axis=0)
    r = 0.5 * (x[t] + x[h]) - center
    r = r - (r @ n)[:, None] * n
    rn = np.linalg.norm(r, axis=1)
    r_hat = np.zeros_like(r)
    r_hat[rn > 1e-12] = r[rn > 1e-12] / rn[rn > 1e-12][:, None]
    Lk = np.linalg.norm(x[h] - x[t], axis=1)
    terms = gamma * Lk * np.einsum("ij,ij->i", 0.5 * (tin[t] + tin[h]) + 0.5 * (tout[t] + tout[h]), r_hat)
    scale = float(g[name + "__E_scale"])
    assert abs(np.abs(terms).sum() - scale) <= 1e-12 * scale
    assert abs(-terms.sum() - E_ref) <= 1e-12 * scale
    tg = np.zeros_like(x)
    contrib = (-0.5 * gamma * Lk)[:, None] * r_hat
    np.add.at(tg, t, contrib)
    np.add.at(tg, h, contrib)
    assert np.max(np.abs(tg - tg_ref)) <= 1e-12 * np.max(np.abs(tg_ref))


# -- Minimizer ----------------------------------------------------------------------------------------------------------
def _minimizer(gp, vopts, mods, cons=(), **kw):
    from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager
    from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager
    from membrane_solver_amd.runtime.minimizer import Minimizer
    from membrane_solver_amd.runtime.steppers import GradientDescent

    mesh, _e, _b = _mesh(gp, vopts, energy_modules=list(mods), constraint_modules=list(cons), **kw)
    return Minimizer(mesh, mesh.global_parameters, GradientDescent(), EnergyModuleManager(list(mods)),
                     ConstraintModuleManager(list(cons)), quiet=True)


def test_minimizer_knows_the_module():
    from membrane_solver_amd.runtime import minimizer as mzr

    assert mzr._ENERGY_BITS[NAME] == BIT and mzr._ENERGY_SLOT[NAME] is None and mzr._LEAFLET_BITS & BIT
    mz = _minimizer({G: "rim", S: 2.0}, _tag(_boundary()), ["tilt_in", "tilt_out", NAME])
    assert mz.energy_module_names[-1] == NAME
    P, T, _B = meshgen.disk_patch(4)
    from membrane_solver_amd.runtime.constraint_manager import ConstraintModuleManager
    from membrane_solver_amd.runtime.energy_manager import EnergyModuleManager
    from membrane_solver_amd.runtime.steppers import GradientDescent

    bare = ArrayMesh(P, T, global_parameters={G: "rim", S: 2.0}, energy_modules=[NAME])
    with pytest.raises(L.MembraneHipError, match="without an edge table"):
        mzr.Minimizer(bare, bare.global_parameters, GradientDescent(), EnergyModuleManager([NAME]), ConstraintModuleManager([]),
                      quiet=True)


def _no_device(monkeypatch):
    """The refusals come before anything is uploaded: any upload or set_params in these tests is an error."""
    install_stub(monkeypatch, refuse=True)


def test_minimizer_refusals_come_before_any_upload(monkeypatch):
    _no_device(monkeypatch)
    rows = _boundary()
    mz = _minimizer({G: "rim", S: 2.0, "tilt_rigidity": 1.0}, _tag(rows), ["tilt", NAME])
    with pytest.raises(L.MembraneHipError, match="tilt_rim_source_bilayer together with a single-field tilt module"):
        mz._device()
    fit = _tag(rows, pin_to_circle_mode="fit", pin_to_circle_normal=[0.0, 0.0, 1.0])
    for cons in (["pin_to_circle"], ["volume"]):
        mz = _minimizer({G: "rim", S: 2.0}, fit, ["tilt_in", NAME], cons)
        with pytest.raises(L.MembraneHipError, match="tilt_rim_source_bilayer in follow mode"):
            mz._device()
    for bad in ({S: float("nan")}, {S: 2.0, "tilt_rim_source_center": [0.0, float("inf"), 0.0]}):
        mz = _minimizer(dict({G: "rim"}, **bad), _tag(rows), ["tilt_in", NAME])
        with pytest.raises(L.MembraneHipError, match="must be finite"):
            mz._device()
    # without a refusal the next thing IS an upload (fixed mode next to pins is allowed)
    mz = _minimizer({G: "rim", S: 2.0}, _tag(rows, pin_to_circle_mode="fixed"), ["tilt_in", NAME])
    with pytest.raises(Refused):
        mz._device()


def test_breakdown_reports_the_module_and_takes_it_out_of_tilt_out(monkeypatch):
    mz = _minimizer({G: "rim", S: 2.0}, _tag(_boundary()), ["surface", "tilt_in", "tilt_out", NAME, "tilt_coupling"])

    class Dev:
        modules = L.MS_MOD_SURFACE | L.MS_MOD_TILT_IN | L.MS_MOD_TILT_OUT | BIT | L.MS_MOD_TILT_COUPLING

        def energy(self):
            return np.array([1.0, 0.0, 0.0, 0.25 + (0.5 - 3.0 + 0.125)])

        def fetch_scalars(self):
            sc = np.zeros(L.MS_NSCAL)
            sc[L.MS_S_ETILT_IN], sc[L.MS_S_ETILT_OUT] = 0.25, 0.5 - 3.0 + 0.125
            return sc

        def rim_source_bilayer_energy(self):
            return -3.0

        def tilt_coupling_energy(self):
            return 0.125

    monkeypatch.setattr(mz, "_device", lambda: (None, Dev()))
    mz._const_energy = {}
    assert mz.compute_energy_breakdown() == {"surface": 1.0, "tilt_in": 0.25, "tilt_out": 0.5, NAME: -3.0,
                                             "tilt_coupling": 0.125}
    # one module left on energies[3]: it reports energies[3] without the riders
    mz2 = _minimizer({G: "rim", S: 2.0}, _tag(_boundary()), ["surface", "tilt_out", NAME])

    class Dev2(Dev):
        modules = L.MS_MOD_SURFACE | L.MS_MOD_TILT_OUT | BIT

        def energy(self):
            return np.array([1.0, 0.0, 0.0, 0.5 - 3.0])

    monkeypatch.setattr(mz2, "_device", lambda: (None, Dev2()))
    mz2._const_energy = {}
    assert mz2.compute_energy_breakdown() == {"surface": 1.0, "tilt_out": 0.5, NAME: -3.0}
    # the module switched off (no group): its entry is 0.0 and nobody is asked for its energy
    class Dev3(Dev2):
        modules = L.MS_MOD_SURFACE | L.MS_MOD_TILT_OUT

        def energy(self):
            return np.array([1.0, 0.0, 0.0, 0.5])

        def rim_source_bilayer_energy(self):
            raise AssertionError("not asked when the bit is off")

    monkeypatch.setattr(mz2, "_device", lambda: (None, Dev3()))
    assert mz2.compute_energy_breakdown() == {"surface": 1.0, "tilt_out": 0.5, NAME: 0.0}


def test_sharded_driver_refuses_the_module():
    src = open(os.path.join(ROOT, "membrane_solver_amd", "parallel.py")).read()
    assert re.search(r"modules & L\.MS_MOD_TILT_RIM_SOURCE_BILAYER:\s*\n\s*raise L\.MembraneHipError\(\"the tilt_rim_source_bilayer "
                     r"module is not sharded", src)


# -- C ABI ---------------------------------------------------------------------------------------------------------------
def test_c_abi_declares_the_module():
    hdr = open(os.path.join(ROOT, "include", "membrane_hip.h")).read()
    m = re.search(r"#define MS_MOD_TILT_RIM_SOURCE_BILAYER (\d+)u", hdr)
    assert m and int(m.group(1)) == BIT == 8388608 == 2 * L.MS_MOD_TILT_SPLAY_TWIST_IN  # the next free bit
    assert re.search(r"MS_NSCAL = 31\b", hdr)  # (no new reduction slot)
    bits = [int(v) for v in re.findall(r"#define MS_(?:MOD|CON|TRACK)_[A-Z_]+ (\d+)u", hdr)]
    assert len(bits) == len(set(bits)) and all(b & (b - 1) == 0 for b in bits)
    names = {"ms_set_rim_source_bilayer", "ms_get_rim_source_bilayer_energy", "ms_rim_source_bilayer_stats"}
    for n in names:
        assert re.search(r"\bint %s\(" % n, hdr) and hasattr(L.lib(), n)
    assert names <= set(L.SIGNATURES)


def test_c_abi_argument_checks_without_a_device():
    lib = L.lib()
    e = ctypes.c_double(1.0)
    v = (ctypes.c_double * 3)()
    assert lib.ms_set_rim_source_bilayer(None, 0, None, None, None, None) == MS_ERR_INVALID
    assert lib.ms_get_rim_source_bilayer_energy(None, ctypes.byref(e)) == MS_ERR_INVALID
    assert b"ms_get_rim_source_bilayer_energy: bad argument" in lib.ms_last_error(None)
    assert lib.ms_rim_source_bilayer_stats(None, v) == MS_ERR_INVALID


def test_one_helper_uploads_both_kinds_of_tables():
    """ms_set_leaflet_rim_source and ms_set_rim_source_bilayer share rim_upload; the lanes that decline a rim source name
    the bilayer bit; the slot list and the coupling's cell rule count it."""
    csrc = os.path.join(ROOT, "membrane_solver_amd", "csrc")
    rim = open(os.path.join(csrc, "ms_api_rim.inc")).read()
    # (one allocation for both: the table builder's upload, called once, and no allocation of the file's own)
    assert rim.count("upload_table(") == 1 and rim.count("hipMalloc(") == 0
    assert len(re.findall(r"return rim_upload\(c, \"ms_set_", rim)) == 2
    # the slot list: the module's row of the slot-writer table rides in the outer leaflet's tilt-magnitude slot, reads
    # both fields (TiltField::mods() of either) and has no shape gradient
    import slot_writer_cases as sw

    r = sw.row("MS_MOD_TILT_RIM_SOURCE_BILAYER")
    assert r == {"bit": "MS_MOD_TILT_RIM_SOURCE_BILAYER", "slot": "MS_S_ETILT_OUT", "slot_disk": None,
                 "reads": {"RD_IN", "RD_OUT"}, "base": False, "shape_grad": False}
    assert sw.writers_in_front("MS_MOD_TILT_RIM_SOURCE_BILAYER", "MS_S_ETILT_OUT") == ["MS_MOD_TILT_OUT", "MS_MOD_TILT_RIM_SOURCE_OUT"]
    # the coupling's cell rule counts it: tilt_out, tilt_rim_source_out and this module are the writers in front of it
    assert sw.writers_in_front("MS_MOD_TILT_COUPLING", "MS_S_ETILT_OUT") == [
        "MS_MOD_TILT_OUT", "MS_MOD_TILT_RIM_SOURCE_OUT", "MS_MOD_TILT_RIM_SOURCE_BILAYER"]
    sw.assert_lanes_decline_every_addon("MS_MOD_TILT_RIM_SOURCE_BILAYER")  # tsearch_plan, the fused evaluator, the relaxation program
    phases = open(os.path.join(csrc, "ms_api_phases.inc")).read()
    m = re.search(r"constexpr uint32_t MS_TILT_SHAPE_MODS = ([^;]*);", phases)
    assert m and "MS_MOD_TILT_RIM_SOURCE_BILAYER" not in m.group(1)  # no shape gradient
