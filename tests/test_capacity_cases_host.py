"""The case table of tests/capacity_cases.py, on the CPU: every mesh lies in the band of patch sizes it is named for,
at least 40 rows from the nearest threshold of the library's own LDS formulas; ms_create's admission formula admits all
five; the oracle port's relaxations have the recorded counts, decide nothing near a knife edge and do not notice a
perturbation of the start fields in the last bit; and the oracle's own noise on these meshes (smallest facet angle
0.2-0.5 degrees) is a tenth of the bars test_gpu_tilt_capacity.py holds the device to.

Measured when the table was written (x86-64, gcc; the same in both summation modes unless noted):

    row       cap   max_ent  nearest threshold (rows)                      smallest angle  leaflet gradient LDS
    fused     706   956      144  (two-field search, 850)                  0.51 deg        75528 / 70544 B
    search1   967   1216     116  (two-field search, 850)                  0.36            101360 / 95856
    unfused   1407  1656     52   (two-field energy-only pass, 1459)       0.25            144912 / 138528
    no_epass  1515  1764     55   (the same; leaflet instance 84 / 152)    0.23            155608 / 149008
    tile256   1709  2784     249 / 88 (energy-only pass / leaflet, 1620)   0.23            190288 / 172432 (> 163840)

    port: counts as in capacity_cases.COUNTS; smallest decision margin |E1 - E0| / |E0| 1.6e-3 (unfused-leaflet-cg40),
    2.1e-1 on every first-step accept, >= 9.7 on the rejected ladders; a 1e-15 perturbation changes no count and no
    accept / reject string.
    oracle noise (worst over the OpenMP build and a permuted facet order): energies 2.1e-16 (bar 1e-13); gradients
    single field 8.5e-16, leaflets 8.0e-15 (bar 1e-12).
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import capacity_cases as cc
import relax_cases as rc
from conftest import relerr

ROWS = list(cc.ROWS)
LANES = [(nf, k) for nf in (1, 2) for k in ("search", "gradient", "energy_only")]


def _plan(row, fixed_order):
    from membrane_solver_amd.device import DeviceMesh

    P, T = cc.build_mesh(row)
    return DeviceMesh.plan_tilt_lanes(P, T, cc.ROWS[row][1], fixed_order)


def _largest_fitting_cap(read, threads, max_ent, fixed_order):
    """The largest patch at which ``read(stats)`` still says "fits", by bisection over ms_tilt_lane_plan."""
    from membrane_solver_amd.device import DeviceMesh

    fits = lambda cap: read(DeviceMesh.tilt_lane_plan(threads, cap, max_ent, fixed_order))  # noqa: E731
    lo, hi = 1, 1 << 14
    assert fits(lo) and not fits(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if fits(mid) else (lo, mid)
    return lo


@pytest.mark.parametrize("fixed_order", [False, True], ids=["atomic", "fixed"])
@pytest.mark.parametrize("row", ROWS)
def test_mesh_lies_in_its_band(row, fixed_order):
    from membrane_solver_amd import _lib as L

    P, T = cc.build_mesh(row)
    m, tile = cc.ROWS[row]
    assert (len(P), len(T)) == (3 * m + 2, 6 * m)
    st = _plan(row, fixed_order)
    # the patch is what ms_plan_tiling reports: owned rows + the largest halo
    plan = np.zeros(8, dtype=np.int64)
    assert L.lib().ms_plan_tiling(len(P), len(T), P.ctypes.data_as(L._D), T.ctypes.data_as(L._I32), tile, 1,
                                  plan.ctypes.data_as(L._I64), None) == 0
    assert st["own"] == st["threads"] == tile and st["cap"] == tile + int(plan[2])
    assert rc.valences(len(P), T).max() == m and st["cap"] > m
    want, leaf = cc.BANDS[row]
    got = {nf: tuple(st[nf][k] for k in ("search", "gradient", "energy_only")) for nf in (1, 2)}
    assert got == want and st["leaflet_gradient_fits"] == leaf, (st, want, leaf)
    # ... and not by a hair: 40 rows to every threshold, each found from the library's formula at this mesh's max_ent
    dist = {}
    for nf, k in LANES:
        thr = _largest_fitting_cap(lambda s, nf=nf, k=k: s[nf][k], tile, st["max_ent"], fixed_order)
        dist[nf, k] = (thr - st["cap"]) if st[nf][k] else (st["cap"] - (thr + 1))
    thr = _largest_fitting_cap(lambda s: s["leaflet_gradient_fits"], tile, st["max_ent"], fixed_order)
    dist["leaflet"] = (thr - st["cap"]) if leaf else (st["cap"] - (thr + 1))
    print(f"CAP_FIG band {row} {'fixed' if fixed_order else 'atomic'} cap={st['cap']} max_ent={st['max_ent']} "
          f"leaflet_lds={st['leaflet_gradient_lds']} nearest={min(dist.values())} {dist}")
    assert min(dist.values()) >= cc.MARGIN_ROWS, dist


def test_thresholds_are_the_documented_ones():
    """The rows of the table in capacity_cases.py (tile 64, the `no_epass` mesh's corner lists)."""
    st = _plan("no_epass", False)
    thr = {(nf, k): _largest_fitting_cap(lambda s, nf=nf, k=k: s[nf][k], 64, st["max_ent"], False) for nf, k in LANES}
    assert thr[1, "search"] == thr[1, "gradient"] == 1345 and thr[2, "search"] == thr[2, "gradient"] == 850
    assert thr[1, "energy_only"] == 2360 and thr[2, "energy_only"] == 1459
    assert _largest_fitting_cap(lambda s: s["leaflet_gradient_fits"], 64, st["max_ent"], False) == 1667
    assert _largest_fitting_cap(lambda s: s["leaflet_gradient_fits"], 64, st["max_ent"], True) == 1599


@pytest.mark.parametrize("row", ROWS)
def test_ms_create_admits_the_mesh(row):
    """ms_create admits a context when the plain energy and gradient instances fit 160 KiB; the gradient formula (the
    larger one: bending, a constraint row, fixed-order sums) is what ms_plan_tiling reports."""
    from membrane_solver_amd import _lib as L

    P, T = cc.build_mesh(row)
    plan = np.zeros(8, dtype=np.int64)
    rc_ = L.lib().ms_plan_tiling(len(P), len(T), P.ctypes.data_as(L._D), T.ctypes.data_as(L._I32), cc.ROWS[row][1], 1,
                                 plan.ctypes.data_as(L._I64), None)
    assert rc_ == 0
    assert 0 < int(plan[7]) <= 160 * 1024 and int(plan[4]) == 0  # fits; no facet dropped
    assert int(plan[0]) == -(-len(P) // cc.ROWS[row][1])
    if row == "tile256":  # the instance nothing admits: over the limit in both summation modes
        assert min(_plan(row, False)["leaflet_gradient_lds"], _plan(row, True)["leaflet_gradient_lds"]) > 160 * 1024


def test_case_table_is_complete():
    assert set(cc.RELAX_IDS) == set(cc.COUNTS) and len(cc.RELAX_IDS) == len(cc.RELAX) == 26
    for row in cc.WORKING:
        assert {(k, s) for r, k, s in cc.RELAX if r == row} == {(k, s) for k in ("single", "leaflet") for s in cc.SOLVERS}
    m = cc.materialize("fused", "leaflet")
    assert m.fixed_in[::13].all() and m.fixed_in.sum() == len(range(0, m.nv, 13)) and not m.fixed_out.any()
    c = cc.case("fused", "leaflet")
    assert c.gp["tilt_mass_mode_out"] == "consistent" and set(c.modules) == set(rc._LEAFLET_ALL)


@pytest.mark.parametrize("row,kind,solver", cc.RELAX, ids=cc.RELAX_IDS)
def test_port_counts_and_decision_margins(row, kind, solver):
    cid = f"{row}-{kind}-{solver}"
    c = cc.case(row, kind, solver)
    p, counts, trace = cc.port_result(row, kind, solver)
    assert counts == cc.COUNTS[cid], "the port's (iterations, evaluations) changed"
    trials = [t for t in trace if t[0] == "trial"]
    assert len(trials) + len([t for t in trace if t[0] == "gnorm"]) == counts[1]
    margin = min(abs(E1 - E0) / abs(E0) for _k, E0, E1 in trials)
    accepted = "".join("A" if E1 <= E0 else "r" for _k, E0, E1 in trials)
    print(f"CAP_FIG port {cid} counts={counts} margin={margin:.2e} {accepted}")
    assert margin >= 1e-8
    if solver == "cg005":
        assert accepted == "A" * 6
    elif solver == "cg40":
        assert accepted.count("A") == 6 and accepted.count("r") >= 6 * 6, "the ladder halves six times and more"
    else:
        assert accepted == "r" * 12 and counts == (1, 13)  # the whole ladder rejected: nothing may move
    m = cc.materialize(row, kind)
    start = (m.tilts,) if kind == "single" else (m.tilts_in, m.tilts_out)
    for got, given, mask in zip(rc.fields_of(c, p), start, (m.fixed_in, m.fixed_out)):
        assert np.abs(got[mask] - given[mask]).max(initial=0.0) <= 1e-15
        if solver == "gd40":
            assert np.abs(got - given).max() <= 1e-15


@pytest.mark.parametrize("row,kind,solver", cc.RELAX, ids=cc.RELAX_IDS)
def test_port_is_insensitive_to_last_bit_perturbations(row, kind, solver):
    c = cc.case(row, kind, solver)
    p, counts, trace = cc.port_result(row, kind, solver)
    m = cc.materialize(row, kind)
    rng = np.random.default_rng(1234)
    scale = (1.0 + 1e-15 * rng.normal(size=m.tilts_in.shape), 1.0 + 1e-15 * rng.normal(size=m.tilts_out.shape))
    q, counts_q, trace_q = rc.run_port(c, m, scale=scale)
    assert counts_q == counts
    acc = lambda tr: [E1 <= E0 for k, E0, E1 in (t for t in tr if t[0] == "trial")]  # noqa: E731
    assert acc(trace_q) == acc(trace)
    for a, b in zip(rc.fields_of(c, q), rc.fields_of(c, p)):
        assert np.abs(a - b).max() < 1e-11 * np.abs(b).max()


def _noise(ref, other, kind):
    e = [abs(other.E - ref.E) / abs(ref.E), abs(other.E_tilt - ref.E_tilt) / abs(ref.E_tilt)]
    g = [relerr(other.grad, ref.grad)] + [relerr(a, b) for a, b in zip(other.tgrads, ref.tgrads)]
    if kind == "leaflet":
        e.append(abs(other.E_module - ref.E_module) / abs(ref.E_module))
        g += [relerr(a, b) for a, b in zip(other.tgrads_module, ref.tgrads_module)]
    return max(e), max(g)


@pytest.mark.parametrize("kind", ["single", "leaflet"])
@pytest.mark.parametrize("row", [r for r in ROWS if r != "tile256"])  # (tile256 is the `no_epass` mesh)
def test_oracle_noise_is_a_tenth_of_the_device_bars(row, kind):
    """The oracle against itself on the mesh: the OpenMP build (other summation order, vertex sums by atomics) and a
    random permutation of the facet rows.  Energies within 1e-13, gradients within 1e-12 (relative max-norm)."""
    from oracle import ms_oracle as orc

    ref = cc.oracle_eval(row, kind)
    p = cc.problem(row, kind)
    perm = np.random.default_rng(99).permutation(len(p.tri))
    p.tri = np.ascontiguousarray(p.tri[perm])
    p.gamma = p.gamma[perm]
    permuted = cc.evaluate(p, kind)
    orc.use_openmp(True)
    try:
        omp = cc.evaluate(cc.problem(row, kind), kind)
    finally:
        orc.use_openmp(False)
    for name, other in (("permuted", permuted), ("openmp", omp)):
        e, g = _noise(ref, other, kind)
        print(f"CAP_FIG noise {row} {kind} {name} energies={e:.2e} gradients={g:.2e}")
        assert e <= 1e-13 and g <= 1e-12, (name, e, g)
