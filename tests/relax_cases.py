"""The problems the one-tile tilt relaxation programs are pinned on, shared by test_relax_cases_host.py (mesh
properties, decision margins and the port's counts, no GPU) and test_gpu_relax_onetile.py (the four device paths
against oracle.minimizer_port).  A plain module, not a conftest: a case is data (mesh, module list, one parameter dict,
seeds, clamp / disk-row selections), `materialize` builds its arrays, `problem` the port's Problem and `run_port`
runs the port's relaxation on it.

Meshes: every mesh is ONE tile at T = 256 (nv <= 256) and irregular, not degenerate: geodesic icospheres / a ring
disk refined by centroid insertion (1 facet -> 3, +1 vertex, +2 facets; the largest of a few sampled facets is split,
seeded), then `meshgen.smooth_displace`.  `build_mesh` asserts a smallest facet angle >= 2 degrees and a smallest facet
area >= 1e-6 of the mean.  The facet counts are what the fused relaxation (csrc/ms_relax_fused.inc) branches on: its
facet loops run in chunks of 256 lanes and its per-facet arrays have the stride (nf + 1) & ~1.

The library orders the facets of a tile itself (ms_tiles.cpp: a stride permutation, then a bank-aware fill), so which
vertex -> corner CSR runs cross local facet 256 is not the input order's to choose: on the two-chunk meshes the stride
permutation spreads the facets of every vertex over the whole list, and the `hub` mesh has two vertices of valence 32
whose runs therefore straddle the chunk boundary.

COUNTS holds the port's (iterations, evaluations) per case as measured on a CPU; test_relax_cases_host.py asserts them
together with the decision margins, so a later change of the port (or of a builder) is noticed."""
from __future__ import annotations

from dataclasses import dataclass, field
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

from membrane_solver_amd import meshgen

TILE = 256

# name -> (base, insertions, facets removed, displace amplitude, seed)
MESHES = {
    "closed256": (("sphere", 4), 94, 0, 0.05, 11),      # 256 / 508: capacity, chunks of 256 + 252 facets
    "closed255_odd": (("sphere", 4), 93, 1, 0.05, 12),  # 255 / 505: odd facet count, three boundary vertices
    "disk256": (("disk", 8), 39, 0, 0.03, 13),          # 256 / 462: open surface at capacity, boundary ring of 48
    "closed130": (("sphere", 3), 38, 0, 0.05, 14),      # 130 / 256: exactly one full chunk
    "closed131": (("sphere", 3), 39, 0, 0.05, 15),      # 131 / 258: a second chunk of two facets
    "small92": (("sphere", 3), 0, 0, 0.05, 16),         # 92 / 180: one partial chunk
    "hub": (("uv", 32, 7), 0, 0, 0.05, 17),             # 226 / 448: both poles have valence 32
}
EXPECT = {"closed256": (256, 508), "closed255_odd": (255, 505), "disk256": (256, 462), "closed130": (130, 256),
          "closed131": (131, 258), "small92": (92, 180), "hub": (226, 448)}


def uv_sphere(n_meridians: int, n_rings: int):
    """Latitude / longitude sphere: two poles of valence ``n_meridians``, outward facets."""
    m, r = int(n_meridians), int(n_rings)
    pts = [(0.0, 0.0, 1.0)]
    for i in range(1, r + 1):
        th = np.pi * i / (r + 1)
        for j in range(m):
            ph = 2.0 * np.pi * j / m
            pts.append((np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)))
    pts.append((0.0, 0.0, -1.0))
    P = np.array(pts, dtype=np.float64)
    ring = lambda i, j: 1 + (i - 1) * m + (j % m)  # noqa: E731
    tris = [(0, ring(1, j), ring(1, j + 1)) for j in range(m)]
    for i in range(1, r):
        for j in range(m):
            a, b, c, d = ring(i, j), ring(i, j + 1), ring(i + 1, j), ring(i + 1, j + 1)
            tris += [(a, c, d), (a, d, b)] if (i + j) % 2 else [(a, c, b), (b, c, d)]  # alternating diagonals
    south = len(P) - 1
    tris += [(south, ring(r, j + 1), ring(r, j)) for j in range(m)]
    T = np.array(tris, dtype=np.int32)
    v0, v1, v2 = P[T[:, 0]], P[T[:, 1]], P[T[:, 2]]
    flip = np.einsum("ij,ij->i", np.cross(v1 - v0, v2 - v0), v0 + v1 + v2) < 0.0
    T[flip] = T[flip][:, [0, 2, 1]]
    return P, np.ascontiguousarray(T)


def facet_areas(P, T):
    return 0.5 * np.linalg.norm(np.cross(P[T[:, 1]] - P[T[:, 0]], P[T[:, 2]] - P[T[:, 0]]), axis=1)


def facet_min_angle_deg(P, T) -> float:
    best = 180.0
    for k in range(3):
        a, b, c = P[T[:, k]], P[T[:, (k + 1) % 3]], P[T[:, (k + 2) % 3]]
        u, v = b - a, c - a
        cs = np.einsum("ij,ij->i", u, v) / (np.linalg.norm(u, axis=1) * np.linalg.norm(v, axis=1))
        best = min(best, float(np.degrees(np.arccos(np.clip(cs, -1.0, 1.0))).min()))
    return best


def valences(nv, T):
    return np.bincount(np.asarray(T).reshape(-1), minlength=nv)


def insert_centroids(P, T, n: int, rng):
    """``n`` centroid insertions: of five sampled facets the largest is split into three around its centroid."""
    P, T = [tuple(p) for p in P], [tuple(int(v) for v in t) for t in T]
    for _ in range(n):
        cand = rng.choice(len(T), size=min(5, len(T)), replace=False)
        arr = np.array(P)
        f = int(cand[int(np.argmax(facet_areas(arr, np.array([T[c] for c in cand]))))])
        a, b, c = T[f]
        d = len(P)
        P.append(tuple((arr[a] + arr[b] + arr[c]) / 3.0))
        T[f] = (a, b, d)
        T += [(b, c, d), (c, a, d)]
    return np.array(P, dtype=np.float64), np.array(T, dtype=np.int32)


@lru_cache(maxsize=None)
def build_mesh(name: str):
    """-> (positions, tri rows, boundary mask), read-only arrays."""
    base, n_ins, n_drop, amp, seed = MESHES[name]
    rng = np.random.default_rng(seed)
    if base[0] == "sphere":
        P, T = meshgen.icosphere(base[1])
    elif base[0] == "uv":
        P, T = uv_sphere(base[1], base[2])
    else:
        P, T, _b = meshgen.disk_patch(base[1], jitter=0.1, seed=seed)
    P, T = insert_centroids(P, T, n_ins, rng)
    if n_drop:
        T = np.ascontiguousarray(np.delete(T, rng.choice(len(T), size=n_drop, replace=False), axis=0))
    P = meshgen.smooth_displace(P, amp)
    bnd = meshgen.boundary_mask_from_triangles(len(P), T)
    areas = facet_areas(P, T)
    assert len(P) <= TILE, name
    assert facet_min_angle_deg(P, T) >= 2.0, (name, facet_min_angle_deg(P, T))
    assert areas.min() >= 1e-6 * areas.mean(), name
    for a in (P, T, bnd):
        a.setflags(write=False)
    return P, T, bnd


_LEAFLET_ALL = ["tilt_in", "tilt_out", "tilt_smoothness_in", "tilt_smoothness_out", "bending_tilt_in",
                "bending_tilt_out"]
# kappa_in != kappa_out, c0 != 0 per leaflet, one consistent mass mode (the relaxation evaluates the vertex-area form
# whatever the mode), Jacobi CG with six inner steps of 0.05
_GP_ALL = {"tilt_modulus_in": 1.3, "tilt_modulus_out": 0.7, "tilt_mass_mode_out": "consistent", "bending_modulus": 0.4,
           "bending_modulus_in": 0.6, "spontaneous_curvature": 0.05, "spontaneous_curvature_out": -0.1,
           "tilt_solve_mode": "nested", "tilt_solver": "cg", "tilt_step_size": 0.05, "tilt_inner_steps": 6}
_GP_DISK = {"tilt_disk_target_group_in": "disk", "tilt_disk_target_strength_in": 15.0,
            "tilt_disk_target_group_out": "disk", "tilt_disk_target_strength_out": 10.0,
            "tilt_disk_target_theta_B": 0.5, "tilt_disk_target_theta_B_out": -0.4, "tilt_disk_target_lambda": 1.0,
            "tilt_disk_target_center": [0.02, -0.01, 0.1], "tilt_disk_target_normal": [0.0, 0.1, 1.0]}
_GP_SINGLE = {"tilt_rigidity": 1.1, "bending_modulus": 0.5, "spontaneous_curvature": 0.08,
              "tilt_smoothness_rigidity": 0.3, "tilt_solve_mode": "nested", "tilt_solver": "cg",
              "tilt_step_size": 0.05, "tilt_inner_steps": 6}


@dataclass(frozen=True)
class RelaxCase:
    id: str
    mesh: str
    modules: tuple = tuple(_LEAFLET_ALL)
    gp: dict = field(default_factory=dict)  # one dict for mp.Problem and ArrayMesh / Minimizer
    kind: str = "leaflet"  # "leaflet": relax_leaflet_tilts; "single": relax_tilts (one field, the generic program only)
    seed: int = 3
    clamp_in: str = "every13"  # "none" | "every13" | "all"
    clamp_out: str = "none"
    disk_rows: str = ""  # rows tagged for tilt_disk_target_in/out: "half" every second row, "row0" row 0 alone
    all_rejected: bool = False  # the first ladder is rejected twelve times: nothing may move
    note: str = ""


def _gp(**over):
    return dict(_GP_ALL, **over)


CASES = [RelaxCase(f"all-{m}", m, gp=_gp(), note="row 1: every module, both leaflets") for m in MESHES]
CASES += [
    RelaxCase("gd-closed256", "closed256", gp=_gp(tilt_solver="gd"), note="row 2"),
    RelaxCase("gd-disk256", "disk256", gp=_gp(tilt_solver="gd"), note="row 2"),
    RelaxCase("nojacobi-closed131", "closed131", gp=_gp(tilt_cg_preconditioner="none"), note="row 3: minv == 1"),
    RelaxCase("step40-closed255_odd", "closed255_odd", gp=_gp(tilt_step_size=40.0), note="row 4: the ladder halves"),
    RelaxCase("step40gd-closed131", "closed131", gp=_gp(tilt_step_size=40.0, tilt_solver="gd"),
              note="row 4: the ladder halves in every gradient-descent iteration"),
    RelaxCase("allrej-closed256", "closed256", gp=_gp(tilt_step_size=1.0e7), all_rejected=True,
              note="row 4: twelve rejections, (1, 13), fields unchanged"),
    RelaxCase("allrej-gd-small92", "small92", gp=_gp(tilt_step_size=1.0e7, tilt_solver="gd"), all_rejected=True,
              note="row 4: the same through gradient descent"),
    # row 5: tilt_tol between the port's gradient norms after the third and the fourth accepted step (TOL_BRACKET)
    RelaxCase("tol-closed131", "closed131", gp=_gp(tilt_tol=8.5), note="row 5: the norm test ends the loop"),
    RelaxCase("tolgd-closed130", "closed130", gp=_gp(tilt_tol=8.5, tilt_solver="gd"),
              note="row 5 through gradient descent: the norm test at the top of an iteration"),
    RelaxCase("in_only-closed256", "closed256", modules=("tilt_in", "tilt_smoothness_in", "bending_tilt_in"), gp=_gp(),
              note="row 6: one field (the outer leaflet has no module)"),
    RelaxCase("out_only-disk256", "disk256", modules=("tilt_out", "tilt_smoothness_out", "bending_tilt_out"),
              gp=_gp(), clamp_in="none", clamp_out="every13", note="row 6, mirrored, on the open surface"),
    RelaxCase("clampall_in-closed130", "closed130", gp=_gp(), clamp_in="all", note="row 7"),
    RelaxCase("clampall_out-hub", "hub", gp=_gp(), clamp_out="all", note="row 7, mirrored"),
    RelaxCase("disktarget-disk256", "disk256",
              modules=("tilt_in", "tilt_out", "tilt_smoothness_in", "tilt_smoothness_out", "tilt_disk_target_in",
                       "tilt_disk_target_out"), gp=_gp(**_GP_DISK), disk_rows="half",
              note="row 8: tagged and untagged rows on one mesh"),
    # the only tagged row sits on the disk's center: radius 0, the profile is switched off (tilt_disk_target_in.py:
    # 219-220) and the frozen-surface cache holds NaN for it -- the loaded module must contribute nothing
    RelaxCase("disktarget_off-disk256", "disk256",
              modules=("tilt_in", "tilt_out", "tilt_smoothness_in", "tilt_smoothness_out", "tilt_disk_target_in",
                       "tilt_disk_target_out"),
              gp=_gp(**dict(_GP_DISK, tilt_disk_target_normal=[0.0, 0.0, 1.0], tilt_disk_target_center="row0")),
              disk_rows="row0", note="row 8, edge: the target profile switched off"),
    RelaxCase("precond_param-closed256", "closed256",
              modules=("tilt_in", "tilt_out", "bending_tilt_in", "bending_tilt_out"), gp=_gp(),
              note="row 9: no smoothness module, its rigidity still enters the Jacobi diagonal"),
    RelaxCase("single-closed256", "closed256", modules=("tilt", "bending_tilt", "tilt_smoothness"), gp=dict(_GP_SINGLE),
              kind="single", note="row 10: one field, the generic program alone"),
]
for _c in CASES:  # ("row0": the center is that row's position, to the bit)
    if _c.gp.get("tilt_disk_target_center") == "row0":
        _c.gp["tilt_disk_target_center"] = [float(v) for v in build_mesh(_c.mesh)[0][0]]
CASE_IDS = [c.id for c in CASES]
BY_ID = {c.id: c for c in CASES}

# case -> two consecutive gradient evaluations of the port's run with tilt_tol = 0: the case's tilt_tol lies between
# their norms (asserted on the CPU)
TOL_BRACKET = {"tol-closed131": (3, 4), "tolgd-closed130": (2, 3)}

# (iterations, evaluations) of the port, measured on a CPU
COUNTS = {
    "all-closed256": (6, 13), "all-closed255_odd": (6, 13), "all-disk256": (6, 13), "all-closed130": (6, 13),
    "all-closed131": (6, 13), "all-small92": (6, 13), "all-hub": (6, 13),
    "gd-closed256": (6, 12), "gd-disk256": (6, 12), "nojacobi-closed131": (6, 13),
    "step40-closed255_odd": (6, 50), "step40gd-closed131": (6, 58),
    "allrej-closed256": (1, 13), "allrej-gd-small92": (1, 13), "tol-closed131": (4, 9), "tolgd-closed130": (3, 7),
    "in_only-closed256": (6, 13), "out_only-disk256": (6, 13), "clampall_in-closed130": (6, 13),
    "clampall_out-hub": (6, 13), "disktarget-disk256": (6, 13), "disktarget_off-disk256": (6, 13),
    "precond_param-closed256": (6, 13),
    "single-closed256": (6, 13),
}


def _clamp(spec: str, nv: int):
    m = np.zeros(nv, dtype=bool)
    if spec == "every13":
        m[::13] = True
    elif spec == "all":
        m[:] = True
    return m


def tangent_field(P, T, amplitude, rng):
    from oracle import minimizer_port as mp

    nrm = mp.unit_vertex_normals(P, T)
    t = amplitude * rng.normal(size=P.shape)
    return t - np.einsum("ij,ij->i", t, nrm)[:, None] * nrm


def materialize(case: RelaxCase):
    """-> namespace of the case's arrays: P, T, boundary, tilts_in / tilts_out (or tilts), clamp masks, disk rows."""
    P, T, bnd = build_mesh(case.mesh)
    nv = len(P)
    rng = np.random.default_rng(case.seed)
    a = tangent_field(P, T, 0.2, rng)
    b = tangent_field(P, T, 0.15, rng)
    rows = {"": None, "half": np.arange(0, nv, 2), "row0": np.arange(1)}[case.disk_rows]
    return SimpleNamespace(P=P, T=T, boundary=bnd, nv=nv, nf=len(T), tilts_in=a, tilts_out=b, tilts=a,
                           fixed_in=_clamp(case.clamp_in, nv), fixed_out=_clamp(case.clamp_out, nv), disk_rows=rows)


def problem(case: RelaxCase, m=None, scale=None):
    """The port's Problem of the case; ``scale`` = (s_a, s_b): element-wise factors on the two start fields."""
    from oracle import minimizer_port as mp

    m = materialize(case) if m is None else m
    sa, sb = (1.0, 1.0) if scale is None else scale
    if case.kind == "single":
        return mp.Problem(positions=m.P, tri=m.T, is_boundary=m.boundary, tilts=m.tilts * sa, tilt_fixed=m.fixed_in,
                          energy_modules=list(case.modules), gp=dict(case.gp))
    return mp.Problem(positions=m.P, tri=m.T, is_boundary=m.boundary, tilts_in=m.tilts_in * sa,
                      tilts_out=m.tilts_out * sb, tilt_fixed_in=m.fixed_in, tilt_fixed_out=m.fixed_out,
                      disk_rows_in=m.disk_rows, disk_rows_out=m.disk_rows, energy_modules=list(case.modules),
                      gp=dict(case.gp))


def run_port(case: RelaxCase, m=None, scale=None, gp_over=None):
    """-> (problem after the relaxation, (iterations, evaluations), trace)"""
    from oracle import minimizer_port as mp

    p = problem(case, m, scale)
    if gp_over:
        p.gp.update(gp_over)
    trace = []
    fn = mp.relax_tilts if case.kind == "single" else mp.relax_leaflet_tilts
    st = fn(p, p.positions, trace=trace)
    return p, (st["iters"], st["evals"]), trace


def fields_of(case: RelaxCase, p):
    return (p.tilts,) if case.kind == "single" else (p.tilts_in, p.tilts_out)


@lru_cache(maxsize=None)
def port_result(case_id: str):
    """The port's relaxation of a case, computed once per process and shared (treat as read-only)."""
    case = BY_ID[case_id]
    p, counts, trace = run_port(case)
    for f in fields_of(case, p):
        f.setflags(write=False)
    return p, counts, tuple(trace)
