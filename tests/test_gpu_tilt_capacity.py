"""The tilt family on the device where the size of a tile's vertex patch decides the lane (tests/capacity_cases.py:
five meshes with a pole of valence 640 ... 1450, cap = 706 ... 1709 rows, 17 ... 68 tiles): on every band the lanes
`tilt_lane_stats()` reports are the band's, and every evaluation and relaxation agrees with `oracle.ms_oracle` / the
oracle port by the project's usual bars -- energies 1e-12, shape and tilt gradients 1e-10 (relative max-norm), counts
equal, relaxed fields 1e-10, clamped rows within 1e-12 of the projected start -- in both summation modes; fixed-order
results repeat bit for bit and equal those of a context created under MS_TSEARCH=0.  test_capacity_cases_host.py shows
on the CPU that the oracle's own noise on these meshes is below a tenth of these bars.

On the tile-256 mesh the leaflet bending_tilt instance of the shape-gradient kernel needs 168 / 186 KiB of LDS: an
evaluation that needs it is refused with MS_ERR_TILE_CAPACITY before anything is launched, and everything else on the
context works.

Measured on an MI355X when the file was written (60 tests, 3.7 s), worst over bands and modes:
energies 4.1e-16; tilt gradients 8.5e-15; shape gradients 1.2e-13 (single field) and 3.3e-12 (leaflets: 5.8e-13 at cap
706 growing to 3.3e-12 at cap 1515); relaxed fields 2.2e-14 with the port's
counts everywhere; coupling 4.3e-15, splay / twist rows 6.7e-15.  A scratch library whose search pass takes trial j at
trial j + 1's step size when cap > 900 fails test_relaxation_matches_the_port[search1-single-cg40] ((2, 21) against
(6, 50)) and passes every `fused` case."""
from __future__ import annotations

import os

import numpy as np
import pytest

import capacity_cases as cc
from conftest import relerr

pytestmark = pytest.mark.gpu

MODES = [False, True]
MODE_IDS = ["atomic", "fixed"]


class _Env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _mods(names):
    from membrane_solver_amd import _lib as L

    bits = {"tilt": L.MS_MOD_TILT, "bending_tilt": L.MS_MOD_BENDING_TILT, "tilt_smoothness": L.MS_MOD_TILT_SMOOTH,
            "tilt_in": L.MS_MOD_TILT_IN, "tilt_out": L.MS_MOD_TILT_OUT, "tilt_smoothness_in": L.MS_MOD_TILT_SMOOTH_IN,
            "tilt_smoothness_out": L.MS_MOD_TILT_SMOOTH_OUT, "bending_tilt_in": L.MS_MOD_BENDING_TILT_IN,
            "bending_tilt_out": L.MS_MOD_BENDING_TILT_OUT}
    out = 0
    for n in names:
        out |= bits[n]
    return out


def _context(row, kind, fixed_order, tsearch=True, modules=None):
    """A context of the row with the parameters of relax_cases._GP_SINGLE / _GP_ALL (what capacity_cases.problem hands
    the oracle)."""
    from membrane_solver_amd.device import DeviceMesh

    m = cc.materialize(row, kind)
    with _Env(MS_TSEARCH="1" if tsearch else "0", MS_DETERMINISTIC="1" if fixed_order else "0"):
        dm = DeviceMesh(m.P, m.T, tile_vertices=cc.ROWS[row][1])
    if kind == "single":
        dm.set_bending_params(np.full(m.nv, 0.5), np.full(m.nv, 0.08))
        dm.set_tilts(m.tilts, 1.1)
        dm.set_tilt_smoothness(0.3)
        dm.set_tilt_fixed(m.fixed_in)
        dm.set_params(modules=_mods(modules or cc.SINGLE_MODULES))
    else:
        dm.set_leaflet_tilts("in", m.tilts_in, tilt_fixed=m.fixed_in, tilt_modulus=1.3, smoothness=0.6)
        dm.set_leaflet_tilts("out", m.tilts_out, tilt_modulus=0.7, mass_mode="consistent", smoothness=0.4)
        dm.set_leaflet_bending("in", 0.6, 0.05)
        dm.set_leaflet_bending("out", 0.4, -0.1)
        dm.set_params(modules=_mods(modules or cc.LEAFLET_ALL))
    return dm


def _lanes(st):
    return {nf: tuple(st[nf][k] for k in ("search", "gradient", "energy_only")) for nf in (1, 2)}


def _rel(a, b):
    return abs(a - b) / abs(b)


@pytest.mark.parametrize("fixed_order", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("row", list(cc.ROWS))
def test_lane_stats_report_the_band(row, fixed_order):
    from membrane_solver_amd.device import DeviceMesh

    dm = _context(row, "leaflet", fixed_order)
    st = dm.tilt_lane_stats()
    m = cc.materialize(row, "leaflet")
    assert st == DeviceMesh.plan_tilt_lanes(m.P, m.T, cc.ROWS[row][1], fixed_order)  # the host-only plan is the context's
    want, leaf = cc.BANDS[row]
    assert _lanes(st) == want and st["leaflet_gradient_fits"] == leaf
    assert st["cap"] == cc.ROWS[row][1] + dm.tile_stats()["max_halo"] and st["cap"] > cc.ROWS[row][0]
    dm.set_deterministic(not fixed_order)  # the figure follows the summation mode
    assert dm.tilt_lane_stats() == DeviceMesh.plan_tilt_lanes(m.P, m.T, cc.ROWS[row][1], not fixed_order)
    dm.close()


@pytest.mark.parametrize("fixed_order", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("row", list(cc.ROWS))  # (the tile-256 row as well: everything single-field works there)
def test_single_field_evaluations_match_the_oracle(row, fixed_order):
    ref = cc.oracle_eval(row, "single")
    dm = _context(row, "single", fixed_order)
    runs = []
    for _ in range(2):
        e, g = dm.energy_and_gradient()
        Et, tg = dm.tilt_energy_and_gradient()
        e_only = dm.energy()
        runs.append((e.copy(), g, Et, tg, e_only.copy()))
    e, g, Et, tg, e_only = runs[0]
    figs = (_rel(e.sum(), ref.E), relerr(g, ref.grad), _rel(Et, ref.E_tilt), relerr(tg, ref.tgrads[0]),
            _rel(e_only.sum(), ref.E))
    print("CAP_FIG single %s %s E=%.2e grad=%.2e E_tilt=%.2e tilt_grad=%.2e E_only=%.2e" %
          ((row, "fixed" if fixed_order else "atomic") + figs))
    assert figs[0] <= 1e-12 and figs[2] <= 1e-12 and figs[4] <= 1e-12
    assert figs[1] < 1e-10 and figs[3] < 1e-10
    assert _rel(e_only.sum(), e.sum()) <= 1e-12
    if fixed_order:
        for a, b in zip(runs[0], runs[1]):
            assert np.array_equal(a, b), "fixed-order sums must repeat bit for bit"
    dm.close()


@pytest.mark.parametrize("fixed_order", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("row", cc.WORKING)
def test_leaflet_evaluations_match_the_oracle(row, fixed_order):
    ref = cc.oracle_eval(row, "leaflet")
    dm = _context(row, "leaflet", fixed_order)
    assert dm.tilt_lane_stats()["leaflet_gradient_fits"]
    runs = []
    for _ in range(2):
        e, g = dm.energy_and_gradient()
        Et, gi, go = dm.leaflet_tilt_energy_and_gradient()
        Em, mi, mo = dm.leaflet_tilt_energy_and_gradient(module_form=True)
        e_only = dm.energy()
        runs.append((e.copy(), g, Et, gi, go, Em, mi, mo, e_only.copy()))
    e, g, Et, gi, go, Em, mi, mo, e_only = runs[0]
    e_figs = (_rel(e.sum(), ref.E), _rel(Et, ref.E_tilt), _rel(Em, ref.E_module), _rel(e_only.sum(), ref.E))
    g_figs = (relerr(g, ref.grad), relerr(gi, ref.tgrads[0]), relerr(go, ref.tgrads[1]),
              relerr(mi, ref.tgrads_module[0]), relerr(mo, ref.tgrads_module[1]))
    print("CAP_FIG leaflet %s %s energies %s gradients %s" % (row, "fixed" if fixed_order else "atomic",
          " ".join("%.2e" % v for v in e_figs), " ".join("%.2e" % v for v in g_figs)))
    assert max(e_figs) <= 1e-12
    assert max(g_figs) < 1e-10
    # the energy-only evaluation (one fused launch where it fits, the per-module kernels where it does not) gives the
    # energies of the evaluation with gradients
    assert _rel(e_only.sum(), e.sum()) <= 1e-12 and np.abs(e_only - e).max() <= 1e-12 * np.abs(e).max()
    if fixed_order:
        for a, b in zip(runs[0], runs[1]):
            assert np.array_equal(a, b), "fixed-order sums must repeat bit for bit"
    dm.close()


def _relax(row, kind, solver, fixed_order, tsearch=True):
    gp = cc.SOLVERS[solver]
    dm = _context(row, kind, fixed_order, tsearch)
    rp = dict(solver=gp["tilt_solver"], max_iters=6, step_size=gp["tilt_step_size"], jacobi=True)
    # the device's projected start rows: a call that stops at its first norm test
    start_call = dict(rp, tol=1e300)
    if kind == "single":
        assert dm.relax_tilts(**start_call) == (0, 1)
        start = (dm.get_tilts(),)
        counts = dm.relax_tilts(**rp)
        fields = (dm.get_tilts(),)
    else:
        assert dm.relax_leaflet_tilts(**start_call) == (0, 1)
        start = (dm.get_leaflet_tilts("in"), dm.get_leaflet_tilts("out"))
        counts = dm.relax_leaflet_tilts(**rp)
        fields = (dm.get_leaflet_tilts("in"), dm.get_leaflet_tilts("out"))
    passes = dm.tsearch_stats()["passes"]
    dm.close()
    return counts, fields, start, passes


@pytest.mark.parametrize("row,kind,solver", cc.RELAX, ids=cc.RELAX_IDS)
def test_relaxation_matches_the_port(row, kind, solver):
    import relax_cases as rc

    cid = f"{row}-{kind}-{solver}"
    c = cc.case(row, kind, solver)
    p, port_counts, _trace = cc.port_result(row, kind, solver)
    assert port_counts == cc.COUNTS[cid]
    m = cc.materialize(row, kind)
    want = rc.fields_of(c, p)
    masks = (m.fixed_in, m.fixed_out)
    given = (m.tilts,) if kind == "single" else (m.tilts_in, m.tilts_out)
    search_fits = cc.BANDS[row][0][1 if kind == "single" else 2][0]
    results = {}
    for fixed_order in MODES:
        counts, fields, start, passes = _relax(row, kind, solver, fixed_order)
        results[fixed_order] = (counts, fields)
        errs = [relerr(a, b) for a, b in zip(fields, want)]
        print("CAP_FIG relax %s %s counts=%s port=%s passes=%d relerr=%s" %
              (cid, "fixed" if fixed_order else "atomic", counts, port_counts, passes, " ".join("%.2e" % e for e in errs)))
        assert (passes > 0) == search_fits, "the search pass ran where it does not fit, or stepped aside where it does"
        assert counts == port_counts, f"{cid}: (iterations, evaluations) differ from the port's"
        assert max(errs) < 1e-10
        for got, st, giv, mask in zip(fields, start, given, masks):
            assert np.abs(st - giv).max() <= 1e-12  # (the start fields are tangent: the projection moves nothing)
            assert np.abs(got[mask] - st[mask]).max(initial=0.0) <= 1e-12, f"{cid}: a clamped row moved"
            if solver == "gd40":  # (every call projects once more: rounding, nothing else)
                assert np.abs(got - st).max() <= 1e-14, f"{cid}: a rejected ladder moved the field"
    # fixed-order sums: bit for bit the launch-per-module-and-trial path
    counts0, fields0, _start0, passes0 = _relax(row, kind, solver, True, tsearch=False)
    assert passes0 == 0 and counts0 == results[True][0]
    for a, b in zip(results[True][1], fields0):
        assert np.array_equal(a, b), f"{cid}: differs from the MS_TSEARCH=0 context by {np.abs(a - b).max():.3e}"


@pytest.mark.parametrize("fixed_order", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("row", ["fused", "no_epass"])
def test_coupling_and_splay_twist_on_large_patches(row, fixed_order):
    """k_couple and k_splay: tilt_coupling is k_tilt's lumped arithmetic on d = t_out - t_in, so
    the oracle's tilt module evaluates it; tilt_splay_twist_in against its NumPy restatement.  Bars of
    test_gpu_tilt_coupling.py / test_gpu_splay_twist.py: energies 1e-12 of sum |facet term|, gradients 1e-10."""
    from membrane_solver_amd import _lib as L
    from membrane_solver_amd.device import DeviceMesh
    from oracle import ms_oracle as orc

    m = cc.materialize(row, "leaflet")
    k_c, sign = 0.9, -1
    d = m.tilts_out + sign * m.tilts_in
    g_ref, tg_ref = np.zeros_like(m.P), np.zeros_like(m.P)
    E_ref = orc.tilt_energy_and_gradient(m.P, d, m.T, k_c, g_ref, tg_ref)
    with _Env(MS_DETERMINISTIC="1" if fixed_order else "0"):
        dm = DeviceMesh(m.P, m.T, tile_vertices=cc.ROWS[row][1])
    for lf, t in (("in", m.tilts_in), ("out", m.tilts_out)):
        dm.set_leaflet_tilts(lf, t, tilt_modulus=0.0, smoothness=0.0)
    dm.set_tilt_coupling(k_c, sign)
    dm.set_params(modules=L.MS_MOD_TILT_COUPLING)
    e, g = dm.energy_and_gradient(raw=True)
    Et, gi, go = dm.leaflet_tilt_energy_and_gradient()
    e_only = dm.energy()
    figs = (_rel(e[3], E_ref), _rel(Et, E_ref), _rel(e_only[3], E_ref), relerr(g, g_ref), relerr(go, tg_ref),
            relerr(gi, sign * tg_ref))
    print("CAP_FIG coupling %s %s %s" % (row, "fixed" if fixed_order else "atomic", " ".join("%.2e" % v for v in figs)))
    assert max(figs[:3]) <= 1e-12 and max(figs[3:]) < 1e-10  # (every facet term is >= 0: E is its own scale)
    # tilt_splay_twist_in on the same context
    k_s, k_t = 0.7, 0.4
    E_ref, tg_ref, E_scale, row_scale = cc.splay_twist_reference(m.P, m.T, m.tilts_in, k_s, k_t)
    dm.set_leaflet_tilts("out", np.zeros_like(m.P), tilt_modulus=0.0, smoothness=0.0)
    dm.set_tilt_splay_twist(k_s, k_t)
    dm.set_params(modules=L.MS_MOD_TILT_SPLAY_TWIST_IN)
    E, gi, go = dm.leaflet_tilt_energy_and_gradient()
    E_only = float(dm.energy()[3])
    rows = np.max(np.abs(gi - tg_ref), axis=1) / row_scale
    print("CAP_FIG splay %s %s E=%.2e E_only=%.2e rows=%.2e" % (row, "fixed" if fixed_order else "atomic",
          abs(E - E_ref) / E_scale, abs(E_only - E_ref) / E_scale, rows.max()))
    assert abs(E - E_ref) <= 1e-12 * E_scale and abs(E_only - E_ref) <= 1e-12 * E_scale
    assert rows.max() <= 1e-10 and not go.any()
    dm.close()


@pytest.mark.parametrize("fixed_order", MODES, ids=MODE_IDS)
def test_oversized_leaflet_gradient_instance_is_refused_before_any_launch(fixed_order):
    """Tile 256, cap 1709: the leaflet bending_tilt instance of k_gradient (12 doubles per patch row) is over the
    160 KiB of a CU in both summation modes.  The evaluation that needs it is refused -- MS_ERR_TILE_CAPACITY, the text
    names tile_vertices, nothing was launched -- and everything else on the context works."""
    from membrane_solver_amd import _lib as L

    row = "tile256"
    ref = cc.oracle_eval(row, "leaflet")
    dm = _context(row, "leaflet", fixed_order)
    st = dm.tilt_lane_stats()
    assert not st["leaflet_gradient_fits"] and st["leaflet_gradient_lds"] > 160 * 1024
    dm.profile_enable(True)
    dm.profile_read()
    for call in (dm.energy_and_gradient, lambda: dm.energy_and_gradient(raw=True)):
        with pytest.raises(L.MembraneHipError) as err:
            call()
        text = str(err.value)
        assert "MS_ERR_TILE_CAPACITY" in text and "tile_vertices" in text and "MS_ERR_HIP" not in text, text
        assert sum(n for _ms, n in dm.profile_read().values()) == 0, "a kernel was launched before the refusal"
    # what does not need the instance: the energies, the tilt gradients in both forms ...
    e_only = dm.energy()
    assert sum(n for _ms, n in dm.profile_read().values()) > 0  # (the counter counts)
    dm.profile_enable(False)
    Et, gi, go = dm.leaflet_tilt_energy_and_gradient()
    Em, mi, mo = dm.leaflet_tilt_energy_and_gradient(module_form=True)
    e_figs = (_rel(e_only.sum(), ref.E), _rel(Et, ref.E_tilt), _rel(Em, ref.E_module))
    g_figs = (relerr(gi, ref.tgrads[0]), relerr(go, ref.tgrads[1]), relerr(mi, ref.tgrads_module[0]),
              relerr(mo, ref.tgrads_module[1]))
    print("CAP_FIG tile256 %s energies %s gradients %s" % ("fixed" if fixed_order else "atomic",
          " ".join("%.2e" % v for v in e_figs), " ".join("%.2e" % v for v in g_figs)))
    assert max(e_figs) <= 1e-12 and max(g_figs) < 1e-10
    # ... a leaflet set without bending_tilt_in/out, shape gradient included ...
    ref_nb = cc.oracle_eval(row, "leaflet", cc.LEAFLET_NO_BT)
    dm.set_params(modules=_mods(cc.LEAFLET_NO_BT))
    e, g = dm.energy_and_gradient()
    assert _rel(e.sum(), ref_nb.E) <= 1e-12 and relerr(g, ref_nb.grad) < 1e-10
    assert _rel(dm.energy().sum(), ref_nb.E) <= 1e-12
    # ... and the surface alone
    from oracle import ms_oracle as orc

    m = cc.materialize(row, "leaflet")
    dm.set_surface_tension(np.ones(m.nf))
    dm.set_params(modules=L.MS_MOD_SURFACE)
    g_ref = np.zeros_like(m.P)
    E_ref = orc.surface_energy_and_gradient(m.P, m.T, np.ones(m.nf), g_ref)
    e, g = dm.energy_and_gradient()
    assert _rel(e[0], E_ref) <= 1e-12 and relerr(g, g_ref) < 1e-10
    dm.close()
