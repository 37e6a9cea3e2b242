"""The case table of tests/relax_cases.py, on the CPU: the meshes have the sizes and edges the one-tile relaxation
programs branch on, and every case is a FAIR test of a loop that branches on E1 <= E0 and |g| < tol -- the port itself
is nowhere near a knife edge, its counts are the recorded ones, and a perturbation of the start fields in the last bit
changes neither the counts nor (beyond 1e-11) the result.  test_gpu_relax_onetile.py compares the device with these
runs."""
from __future__ import annotations

import numpy as np
import pytest

import relax_cases as rc

T = rc.TILE


@pytest.mark.parametrize("name", sorted(rc.MESHES))
def test_mesh_has_the_documented_shape(name):
    P, tri, bnd = rc.build_mesh(name)
    nv, nf = len(P), len(tri)
    assert (nv, nf) == rc.EXPECT[name]
    assert nv <= T, "one tile at T = 256"
    assert tri.min() == 0 and tri.max() == nv - 1 and len(np.unique(tri)) == nv  # every row is a corner of some facet
    assert rc.facet_min_angle_deg(P, tri) >= 2.0
    areas = rc.facet_areas(P, tri)
    assert areas.min() >= 1e-6 * areas.mean()
    # manifold: an edge has one or two facets, boundary edges only where the table says so
    e = np.sort(np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]]), axis=1)
    _u, cnt = np.unique(e[:, 0].astype(np.int64) * nv + e[:, 1], return_counts=True)
    assert cnt.max() == 2
    chunks = [min(T, nf - c0) for c0 in range(0, nf, T)]
    val = rc.valences(nv, tri)
    if name == "closed256":
        assert nv == T and chunks == [256, 252] and not bnd.any()
    elif name == "closed255_odd":
        assert nv == T - 1 and nf % 2 == 1 and ((nf + 1) & ~1) == nf + 1 and int(bnd.sum()) == 3 and len(chunks) == 2
    elif name == "disk256":
        assert nv == T and nf % 2 == 0 and int(bnd.sum()) == 48 and len(chunks) == 2
        assert bnd.any() and not bnd.all()
        per_facet = bnd[tri].sum(axis=1)  # facets with 1 or 2 boundary corners: the redistribution of the corner areas
        assert (per_facet == 1).any() and (per_facet == 2).any() and (per_facet == 0).any()
    elif name == "closed130":
        assert chunks == [256]
    elif name == "closed131":
        assert chunks == [256, 2]
    elif name == "small92":
        assert chunks == [180]
    elif name == "hub":
        assert val.max() >= 32 and int((val >= 32).sum()) == 2 and nf > T + val.max() and len(chunks) == 2
    if name != "disk256" and name != "closed255_odd":
        assert not bnd.any() and cnt.min() == 2


def test_case_table_covers_the_rows():
    ids = set(rc.CASE_IDS)
    assert len(ids) == len(rc.CASES) and ids == set(rc.COUNTS)
    assert {f"all-{m}" for m in rc.MESHES} <= ids
    by = rc.BY_ID
    assert by["gd-closed256"].gp["tilt_solver"] == "gd" and by["gd-disk256"].gp["tilt_solver"] == "gd"
    assert by["nojacobi-closed131"].gp["tilt_cg_preconditioner"] == "none"
    assert by["in_only-closed256"].modules and all(m.endswith("_in") for m in by["in_only-closed256"].modules)
    assert all(m.endswith("_out") for m in by["out_only-disk256"].modules)
    assert by["clampall_in-closed130"].clamp_in == "all" and by["clampall_out-hub"].clamp_out == "all"
    assert not any("smoothness" in m for m in by["precond_param-closed256"].modules)
    assert by["precond_param-closed256"].gp["bending_modulus"] != 0.0
    m = rc.materialize(by["disktarget-disk256"])
    assert 0 < len(m.disk_rows) < m.nv and len(m.disk_rows) == m.nv // 2
    # the switched-off profile: the module is loaded and parameterised, its only tagged row has radius 0
    from oracle import minimizer_port as mp

    off = rc.problem(by["disktarget_off-disk256"])
    for lf in ("in", "out"):
        assert mp.disk_target_params(off, lf) is not None
        assert mp._disk_target(off, off.positions, mp.leaflet_tilts(off, lf), lf) == 0.0
    on = rc.problem(by["disktarget-disk256"])
    assert mp._disk_target(on, on.positions, on.tilts_in, "in") > 0.0
    for c in rc.CASES:
        if c.kind == "leaflet" and "bending_tilt_in" in c.modules and "bending_tilt_out" in c.modules:
            gp = c.gp
            assert gp["bending_modulus_in"] != gp["bending_modulus"] and gp["spontaneous_curvature"] != 0.0
            assert gp["spontaneous_curvature_out"] != 0.0


@pytest.mark.parametrize("cid", rc.CASE_IDS)
def test_port_counts_and_decision_margins(cid):
    case = rc.BY_ID[cid]
    p, counts, trace = rc.port_result(cid)
    assert counts == rc.COUNTS[cid], "the port's (iterations, evaluations) changed"
    trials = [t for t in trace if t[0] == "trial"]
    gnorms = [t[1] for t in trace if t[0] == "gnorm"]
    assert len(trials) + len(gnorms) == counts[1]
    for _k, E0, E1 in trials:
        assert abs(E1 - E0) >= 1e-8 * abs(E0), (E0, E1)
    tol = float(case.gp.get("tilt_tol", 0.0) or 0.0)
    if tol > 0.0:
        for g in gnorms:
            assert abs(g - tol) >= 1e-6 * tol
        # the tolerance ends the loop between two iterations of the run without it
        lo, hi = rc.TOL_BRACKET[cid]
        _p, free_counts, free_trace = rc.run_port(case, gp_over={"tilt_tol": 0.0})
        free = [t[1] for t in free_trace if t[0] == "gnorm"]
        assert free[hi] < tol < free[lo]
        assert gnorms == free[:hi + 1] and counts[0] == hi and counts[0] < free_counts[0]
    accepted = ["A" if E1 <= E0 else "r" for _k, E0, E1 in trials]
    if case.all_rejected:
        assert accepted == ["r"] * 12 and counts == (1, 13)
    if "step40" in cid:
        assert accepted.count("r") >= 3 * counts[0], "the ladder halves several times in every search"
        assert accepted.count("A") == counts[0]
    # the start fields are tangent: what the relaxation clamps is what the table uploads
    m = rc.materialize(case)
    for name, mask in (("in", m.fixed_in), ("out", m.fixed_out)):
        if case.kind == "single" and name == "out":
            continue
        got = p.tilts if case.kind == "single" else getattr(p, "tilts_" + name)
        start = m.tilts if case.kind == "single" else getattr(m, "tilts_" + name)
        assert np.abs(got[mask] - start[mask]).max(initial=0.0) <= 1e-15


@pytest.mark.parametrize("cid", rc.CASE_IDS)
def test_port_is_insensitive_to_last_bit_perturbations(cid):
    case = rc.BY_ID[cid]
    p, counts, _trace = rc.port_result(cid)
    m = rc.materialize(case)
    rng = np.random.default_rng(1234)
    scale = (1.0 + 1e-15 * rng.normal(size=m.tilts_in.shape), 1.0 + 1e-15 * rng.normal(size=m.tilts_out.shape))
    q, counts_q, _t = rc.run_port(case, m, scale=scale)
    assert counts_q == counts
    for a, b in zip(rc.fields_of(case, q), rc.fields_of(case, p)):
        assert np.abs(a - b).max() < 1e-11 * np.abs(b).max()
