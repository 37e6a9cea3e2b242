"""The meshes on which the size of a tile's vertex patch, cap = owned rows + largest halo, decides which lane the tilt
family runs (k_tilt, k_bt, k_tsmooth, k_tsearch, k_tgrad, the leaflet instance of k_gradient, k_couple, k_splay), shared
by test_capacity_cases_host.py (bands, the port's counts and margins, the oracle's own noise; no GPU) and
test_gpu_tilt_capacity.py (the device against the oracle on every band).  A plain module in the style of
relax_cases.py, not a conftest.

A mesh is `relax_cases.uv_sphere(m, 3)` -- two poles of valence m, three rings -- displaced by
`meshgen.smooth_displace(., 0.05)`: a pole's tile stages the whole first ring as its halo, so cap grows with m and
nothing else about the mesh changes.  Smallest facet angle 0.2-0.4 degrees (the pole fan), no degenerate facet.

The bands (LDS limits: csrc/ms_internal.h, MS_LDS_TILT_PASS = 150 KiB for the fused tilt passes, MS_LDS_CU = 160 KiB
for any launch; thresholds in patch rows, from `DeviceMesh.tilt_lane_plan`):

    row         m     tile  cap    8-step search, 1 / 2 fields   energy-only pass, 2 fields   leaflet gradient instance
    fused       640   64    706    fits / fits                   fits                         fits
    search1     900   64    967    fits / no  (> 850)            fits                         fits
    unfused     1340  64    1407   no (> 1345) / no              fits                         fits
    no_epass    1450  64    1515   no / no                       no  (> 1459)                 fits (152 / 146 KiB)
    tile256     1450  256   1709   no / no                       no                           NO: 186 / 168 KiB > 160 KiB

(LDS bytes: fixed-order / LDS-atomic summation mode.  The leaflet gradient instance fits up to 1599 / 1667 rows with
the tile-64 meshes' corner lists and up to 1436 / 1620 rows with the tile-256 one's; the one-field energy-only pass fits
up to 2360 rows, beyond every mesh here.  With m = 1300 and 1500, the first probe, `unfused` sat 20 rows above the
one-field search threshold and `no_epass` 32 rows below the fixed-order threshold of the leaflet instance: both were
moved.)

COUNTS holds the port's (iterations, evaluations) per relaxation as measured on a CPU; test_capacity_cases_host.py
asserts them together with the decision margins."""
from __future__ import annotations

from functools import lru_cache
from types import SimpleNamespace

import numpy as np

import relax_cases as rc
from membrane_solver_amd import meshgen

# row -> (meridians, tile_vertices)
ROWS = {"fused": (640, 64), "search1": (900, 64), "unfused": (1340, 64), "no_epass": (1450, 64), "tile256": (1450, 256)}
WORKING = ("fused", "search1", "unfused", "no_epass")  # every lane has a form that fits
# row -> what tilt_lane_stats must say: {fields: (search, gradient pass, energy-only pass)}, leaflet gradient instance
BANDS = {
    "fused": ({1: (True, True, True), 2: (True, True, True)}, True),
    "search1": ({1: (True, True, True), 2: (False, False, True)}, True),
    "unfused": ({1: (False, False, True), 2: (False, False, True)}, True),
    "no_epass": ({1: (False, False, True), 2: (False, False, False)}, True),
    "tile256": ({1: (False, False, True), 2: (False, False, False)}, False),
}
MARGIN_ROWS = 40  # a mesh's cap keeps this distance from every threshold

SINGLE_MODULES = ("tilt", "bending_tilt", "tilt_smoothness")
LEAFLET_ALL = tuple(rc._LEAFLET_ALL)
LEAFLET_NO_BT = ("tilt_in", "tilt_out", "tilt_smoothness_in", "tilt_smoothness_out")
# solver settings of the relaxations: the first step size passes / the ladder halves several times in every search
SOLVERS = {"cg005": {"tilt_solver": "cg", "tilt_step_size": 0.05}, "cg40": {"tilt_solver": "cg", "tilt_step_size": 40.0},
           "gd40": {"tilt_solver": "gd", "tilt_step_size": 40.0}}


@lru_cache(maxsize=None)
def build_mesh(row: str):
    """-> (positions, tri rows), read-only."""
    m, _tile = ROWS[row]
    P, T = rc.uv_sphere(m, 3)
    P = meshgen.smooth_displace(P, 0.05)
    for a in (P, T):
        a.setflags(write=False)
    return P, T


def case(row: str, kind: str, solver: str = "cg005", modules=None) -> rc.RelaxCase:
    """The relaxation of a row as a relax_cases.RelaxCase (every 13th row of the single / the inner field clamped)."""
    if kind == "single":
        return rc.RelaxCase(f"{row}-single-{solver}", row, modules=tuple(modules or SINGLE_MODULES),
                            gp=dict(rc._GP_SINGLE, **SOLVERS[solver]), kind="single", seed=5)
    return rc.RelaxCase(f"{row}-leaflet-{solver}", row, modules=tuple(modules or LEAFLET_ALL),
                        gp=dict(rc._GP_ALL, **SOLVERS[solver]), kind="leaflet", seed=7)


@lru_cache(maxsize=None)
def materialize(row: str, kind: str):
    """The arrays of a row's cases, as relax_cases.materialize makes them (shared, read-only)."""
    P, T = build_mesh(row)
    nv = len(P)
    rng = np.random.default_rng(5 if kind == "single" else 7)
    a = rc.tangent_field(P, T, 0.2, rng)
    b = rc.tangent_field(P, T, 0.15, rng)
    for arr in (a, b):
        arr.setflags(write=False)
    return SimpleNamespace(P=P, T=T, boundary=np.zeros(nv, dtype=bool), nv=nv, nf=len(T), tilts_in=a, tilts_out=b, tilts=a,
                           fixed_in=rc._clamp("every13", nv), fixed_out=rc._clamp("none", nv), disk_rows=None)


# the relaxations the GPU file runs: rows 1-4 both kinds x three solver settings; the tile-256 row one of each
RELAX = [(row, kind, s) for row in WORKING for kind in ("single", "leaflet") for s in SOLVERS]
RELAX += [("tile256", "single", "cg005"), ("tile256", "leaflet", "cg005")]
RELAX_IDS = [f"{r}-{k}-{s}" for r, k, s in RELAX]

# (iterations, evaluations) of the port, measured on a CPU
COUNTS = {
    "fused-single-cg005": (6, 13), "fused-single-cg40": (6, 54), "fused-single-gd40": (1, 13),
    "fused-leaflet-cg005": (6, 13), "fused-leaflet-cg40": (6, 51), "fused-leaflet-gd40": (1, 13),
    "search1-single-cg005": (6, 13), "search1-single-cg40": (6, 50), "search1-single-gd40": (1, 13),
    "search1-leaflet-cg005": (6, 13), "search1-leaflet-cg40": (6, 53), "search1-leaflet-gd40": (1, 13),
    "unfused-single-cg005": (6, 13), "unfused-single-cg40": (6, 50), "unfused-single-gd40": (1, 13),
    "unfused-leaflet-cg005": (6, 13), "unfused-leaflet-cg40": (6, 52), "unfused-leaflet-gd40": (1, 13),
    "no_epass-single-cg005": (6, 13), "no_epass-single-cg40": (6, 50), "no_epass-single-gd40": (1, 13),
    "no_epass-leaflet-cg005": (6, 13), "no_epass-leaflet-cg40": (6, 53), "no_epass-leaflet-gd40": (1, 13),
    "tile256-single-cg005": (6, 13), "tile256-leaflet-cg005": (6, 13),
}


@lru_cache(maxsize=None)
def port_result(row: str, kind: str, solver: str):
    """The port's relaxation, computed once per process and shared (treat as read-only)."""
    c = case(row, kind, solver)
    p, counts, trace = rc.run_port(c, materialize(row, kind))
    for f in rc.fields_of(c, p):
        f.setflags(write=False)
    return p, counts, tuple(trace)


def problem(row: str, kind: str, modules=None):
    """The port's Problem of a row (start fields, clamp masks, parameters of the kind)."""
    return rc.problem(case(row, kind, "cg005", modules), materialize(row, kind))


def evaluate(p, kind: str):
    """Every evaluation the GPU file compares, by oracle.ms_oracle through the port's module loops -> namespace:
    E / grad (energy and shape gradient of the module list), E_tilt / tgrads (tilt-dependent energy and tilt gradients
    at frozen positions: the leaflets' magnitude modules in the vertex-area form), and for the leaflets E_module /
    tgrads_module (the same with every module in its own mass mode)."""
    from oracle import minimizer_port as mp
    from oracle import ms_oracle as orc

    pos = p.positions
    E, grad = mp.energy_and_gradient(p, pos)
    if kind == "single":
        Et, tg = mp.energy_and_tilt_gradient(p, pos, p.tilts)
        return SimpleNamespace(E=E, grad=grad, E_tilt=Et, tgrads=(tg,))
    va = orc.barycentric_vertex_areas(pos, p.tri)
    Et, gi, go = mp.energy_and_leaflet_tilt_gradients(p, pos, p.tilts_in, p.tilts_out, va)
    # module form: the magnitude modules as modules/energy/tilt_leaflet.py evaluates them, the others as above
    Em, tgm = 0.0, {"in": np.zeros_like(pos), "out": np.zeros_like(pos)}
    for name in p.energy_modules:
        lf = name.rsplit("_", 1)[1]
        t = mp.leaflet_tilts(p, lf)
        if name in ("tilt_in", "tilt_out"):
            Em += orc.tilt_leaflet_energy_and_gradient(pos, t, p.tri, mp.tilt_modulus(p, lf), mp.tilt_mass_mode(p, lf),
                                                       None, tgm[lf])
        elif name.startswith("tilt_smoothness_"):
            Em += mp._smoothness_leaflet(p, pos, t, lf, tgm[lf])
        elif name.startswith("bending_tilt_"):
            Em += mp._bending_tilt_leaflet(p, pos, t, lf, tilt_grad=tgm[lf])
        else:
            raise ValueError(name)
    return SimpleNamespace(E=E, grad=grad, E_tilt=Et, tgrads=(gi, go), E_module=float(Em), tgrads_module=(tgm["in"], tgm["out"]))


@lru_cache(maxsize=None)
def oracle_eval(row: str, kind: str, modules=None):
    """`evaluate` at a row's start fields, computed once per process and shared (treat as read-only)."""
    return evaluate(problem(row, kind, modules), kind)


def splay_twist_reference(pos, tri, t, k_splay, k_twist):
    """tilt_splay_twist_in in plain NumPy (the restatement test_splay_twist_host.py checks against the reference's
    vectors) -> (E, tilt gradient, E_scale = sum |facet term|, row_scale = sum |corner term| per row)."""
    v0, v1, v2 = pos[tri[:, 0]], pos[tri[:, 1]], pos[tri[:, 2]]
    n = np.cross(v1 - v0, v2 - v0)
    n2 = np.einsum("ij,ij->i", n, n)
    denom = np.maximum(n2, 1e-20)
    e = (v2 - v1, v0 - v2, v1 - v0)
    g = [np.cross(n, e[k]) / denom[:, None] for k in range(3)]
    area = 0.5 * np.sqrt(np.maximum(n2, 0.0))
    n_hat = n / np.sqrt(n2)[:, None]
    tk = [t[tri[:, k]] for k in range(3)]
    div = sum(np.einsum("ij,ij->i", tk[k], g[k]) for k in range(3))
    curl_n = np.einsum("ij,ij->i", sum(np.cross(g[k], tk[k]) for k in range(3)), n_hat)
    terms = 0.5 * area * (k_splay * div ** 2 + k_twist * curl_n ** 2)
    grad, row_scale = np.zeros_like(pos), np.zeros(len(pos))
    for k in range(3):
        corner = (area * k_splay * div)[:, None] * g[k] + (area * k_twist * curl_n)[:, None] * np.cross(n_hat, g[k])
        np.add.at(grad, tri[:, k], corner)
        np.add.at(row_scale, tri[:, k], np.abs(corner).max(axis=1))
    return float(terms.sum()), grad, float(np.abs(terms).sum()), row_scale
