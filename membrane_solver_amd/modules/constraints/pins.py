"""Shared resolver of the ``pin_to_plane`` / ``pin_to_circle`` tags (modules/constraints/pin_to_plane.py,
pin_to_circle.py of the reference) for both mesh kinds.

A vertex or an edge is pinned when its ``options["constraints"]`` names the module; an edge pins both endpoints.
Parameters resolve per entity, then from the mesh's global parameters, then from the defaults.  ``resolve`` turns
the tags into one ordered *program* per module:

* ``("fixed", [(row, param), ...])``: per-entity planes / circles, vertices first, then edges (tail, head);
* ``("plane_group", param, [(row, skip_fixed), ...])``: a slide plane through the group's centroid;
* ``("circle_group", param, [row, ...])``: a slide circle (centre moved along the normal by the mean offset).

``params`` rows are ``(nx, ny, nz, px, py, pz, radius)``; a circle group's radius is < 0 when it is the mean radial
distance of the members.  The same tables feed the NumPy restatement (``enforce``, ``rows``) and the device
(``device_tables``).
"""

from __future__ import annotations

import numpy as np

from ... import _lib as L

PLANE, CIRCLE = "pin_to_plane", "pin_to_circle"
_SLIDE = {"slide", "normal", "normal_only", "slide_normal"}

# device stage kinds (include/membrane_hip.h MS_PIN_*)
STAGE_FIXED, STAGE_PLANE_GROUP, STAGE_CIRCLE_GROUP = 0, 1, 2
OP_PLANE, OP_CIRCLE = 0, 1
GRAD_PLANE, GRAD_CIRCLE, GRAD_RADIAL = 0, 1, 2


def _tagged(opts, name):
    if not opts:
        return False
    c = opts.get("constraints")
    if isinstance(c, str):
        return c == name
    if isinstance(c, (list, tuple)):
        return name in c
    return False


def _entities(mesh):
    """-> (vertices [(vid, opts)], edges [(tail_vid, head_vid, opts)], row_of, fixed_of) in the reference's
    iteration order (mesh.vertices / mesh.edges dicts, or the ArrayMesh's tables)."""
    row_of = mesh.vertex_index_to_row
    fixed_mask = np.asarray(mesh.fixed_mask, dtype=bool)
    if hasattr(mesh, "vertices") and isinstance(mesh.vertices, dict):
        verts = [(int(vid), getattr(v, "options", None)) for vid, v in mesh.vertices.items()]
        edges = [(int(e.tail_index), int(e.head_index), getattr(e, "options", None)) for e in mesh.edges.values()]

        def fixed_of(vid):
            return bool(getattr(mesh.vertices[vid], "fixed", False))
    else:
        vopts = getattr(mesh, "vertex_options", None) or {}
        ids = mesh.vertex_ids
        verts = [(int(ids[r]), o) for r, o in sorted(vopts.items()) if o]
        er = getattr(mesh, "edge_rows", None)
        eo = getattr(mesh, "edge_options", None) or {}
        edges = [] if er is None else [(int(ids[er[k, 0]]), int(ids[er[k, 1]]), eo.get(k)) for k in range(len(er))]

        def fixed_of(vid):
            return bool(fixed_mask[row_of[vid]])
    return verts, edges, row_of, fixed_of


def _axis_unit(vec, what):
    v = np.asarray(vec, dtype=float).reshape(3)
    nrm = float(np.linalg.norm(v))
    if nrm < 1e-15:
        raise L.MembraneHipError(f"{what}: zero normal is outside the HIP path")
    u = v / nrm
    if int(np.count_nonzero(u)) != 1:
        raise L.MembraneHipError(f"{what}: normal {list(v)} is not along a coordinate axis; only axis-aligned "
                                 "normals are on the HIP path (the project-or-skip decision is taken once)")
    return u


def _mode(opts, gp, key):
    raw = None
    if opts and opts.get(key) is not None:
        raw = opts.get(key)
    elif gp is not None and gp.get(key) is not None:
        raw = gp.get(key)
    m = str(raw or "fixed").lower()
    if m == "fit":
        raise L.MembraneHipError(f"{key}=fit is outside the HIP path (fixed and slide only)")
    return "slide" if m in _SLIDE else "fixed"


def _pick(opts, gp, key, default):
    if opts and opts.get(key) is not None:
        return opts.get(key)
    if gp is not None and gp.get(key) is not None:
        return gp.get(key)
    return default


class PinProgram:
    """Ordered tags of one module: ``program`` (see module doc), ``params`` (k, 7), ``fixed`` (vertex ids)."""

    def __init__(self, name):
        self.name = name
        self.program = []
        self.params = []
        self.row_vid = {}

    def param(self, n, p, r=0.0):
        self.params.append(tuple(float(x) for x in n) + tuple(float(x) for x in p) + (float(r),))
        return len(self.params) - 1


def _plane_program(mesh):
    gp = getattr(mesh, "global_parameters", None)
    verts, edges, row_of, fixed_of = _entities(mesh)
    prog = PinProgram(PLANE)
    fixed_ops, groups = [], {}

    def normal_of(opts, default):
        n = _pick(opts, gp, "pin_to_plane_normal", None)
        return default if n is None else _axis_unit(n, "pin_to_plane")

    def entity_param(opts):
        n = normal_of(opts, np.array([0.0, 0.0, 1.0]))
        p = _pick(opts, gp, "pin_to_plane_point", [0.0, 0.0, 0.0])
        return prog.param(n, np.asarray(p, dtype=float).reshape(3))

    def note(opts, vid):
        g = "default" if not opts or opts.get("pin_to_plane_group") is None else str(opts["pin_to_plane_group"])
        e = groups.setdefault(g, {"vids": set(), "normal": None})
        e["vids"].add(vid)
        if e["normal"] is None:
            e["normal"] = normal_of(opts, None)

    for vid, opts in verts:
        if not _tagged(opts, PLANE):
            continue
        if _mode(opts, gp, "pin_to_plane_mode") == "fixed":
            fixed_ops.append((row_of[vid], entity_param(opts), vid))
        else:
            note(opts, vid)
    for t, h, opts in edges:
        if not _tagged(opts, PLANE):
            continue
        if _mode(opts, gp, "pin_to_plane_mode") == "fixed":
            k = entity_param(opts)
            fixed_ops += [(row_of[t], k, t), (row_of[h], k, h)]
        else:
            note(opts, t)
            note(opts, h)
    if fixed_ops:
        prog.program.append(("fixed", [(r, k) for r, k, _v in fixed_ops], [v for _r, _k, v in fixed_ops]))
    for g, e in groups.items():
        n = e["normal"] if e["normal"] is not None else np.array([0.0, 0.0, 1.0])
        k = prog.param(n, (0.0, 0.0, 0.0))
        vids = sorted(e["vids"])
        prog.program.append(("plane_group", k, [(row_of[v], fixed_of(v)) for v in vids], vids))
    return prog, fixed_of


def _circle_program(mesh):
    gp = getattr(mesh, "global_parameters", None)
    if gp is not None and gp.get("pin_to_circle_mesh_operation_preserve_normal_groups") is not None:
        raise L.MembraneHipError("pin_to_circle_mesh_operation_preserve_normal_groups is outside the HIP path")
    verts, edges, row_of, fixed_of = _entities(mesh)
    prog = PinProgram(CIRCLE)
    fixed_ops, groups = [], {}

    def entity_param(opts):
        n = _axis_unit(_pick(opts, gp, "pin_to_circle_normal", [0.0, 0.0, 1.0]), "pin_to_circle")
        c = np.asarray(_pick(opts, gp, "pin_to_circle_point", [0.0, 0.0, 0.0]), dtype=float).reshape(3)
        r = float(_pick(opts, gp, "pin_to_circle_radius", 1.0))
        if r <= 0.0:
            raise L.MembraneHipError("pin_to_circle: radius must be positive")
        return prog.param(n, c, r)

    def note(opts, vid):
        g = "default" if not opts or opts.get("pin_to_circle_group") is None else opts["pin_to_circle_group"]
        e = groups.setdefault(g, {"vids": set(), "opts": []})
        e["vids"].add(vid)
        if opts:
            e["opts"].append(opts)

    for vid, opts in verts:
        if not _tagged(opts, CIRCLE):
            continue
        if _mode(opts, gp, "pin_to_circle_mode") == "fixed":
            fixed_ops.append((row_of[vid], entity_param(opts), vid))
        else:
            note(opts, vid)
    for t, h, opts in edges:
        if not _tagged(opts, CIRCLE):
            continue
        if _mode(opts, gp, "pin_to_circle_mode") == "fixed":
            k = entity_param(opts)
            fixed_ops += [(row_of[t], k, t), (row_of[h], k, h)]
        else:
            note(opts, t)
            note(opts, h)
    if fixed_ops:
        prog.program.append(("fixed", [(r, k) for r, k, _v in fixed_ops], [v for _r, _k, v in fixed_ops]))
    for g, e in groups.items():
        vids = sorted(e["vids"])
        if len(vids) < 3:  # the reference skips such a group (no projection, no rows)
            continue

        def first(key):
            for o in e["opts"]:
                if o and o.get(key) is not None:
                    return o.get(key)
            return None if gp is None else gp.get(key)

        n = first("pin_to_circle_normal")
        if n is None:
            raise L.MembraneHipError("pin_to_circle slide group without a normal (a fitted normal) is outside the "
                                     "HIP path")
        n = _axis_unit(n, "pin_to_circle")
        base = first("pin_to_circle_point")
        base = np.zeros(3) if base is None else np.asarray(base, dtype=float).reshape(3)
        r = first("pin_to_circle_radius")
        r = -1.0 if r is None or float(r) <= 0.0 else float(r)  # (a non-positive radius: the fitted one)
        k = prog.param(n, base, r)
        prog.program.append(("circle_group", k, [row_of[v] for v in vids], vids))
    return prog, fixed_of


def programs(mesh, module_names):
    """The pin programs of ``module_names`` in their order (other names are skipped)."""
    out = []
    for name in module_names:
        if name == PLANE:
            out.append(_plane_program(mesh))
        elif name == CIRCLE:
            out.append(_circle_program(mesh))
    return out


# ---- NumPy restatement ---------------------------------------------------------------------------------------------
def _default_tangent(n):
    t = np.array([1.0, 0.0, 0.0])
    if abs(float(np.dot(t, n))) > 0.9:
        t = np.array([0.0, 1.0, 0.0])
    t = t - np.dot(t, n) * n
    nrm = float(np.linalg.norm(t))
    return t / nrm if nrm >= 1e-15 else np.array([1.0, 0.0, 0.0])


def _onto_plane(x, n, p):
    return x - np.dot(x - p, n) * n


def _onto_circle(x, n, c, r):
    off = (x - np.dot(x - c, n) * n) - c
    nrm = float(np.linalg.norm(off))
    t = off / nrm if nrm >= 1e-15 else _default_tangent(n)
    return c + r * t


def _radial_hat(x, n, c):
    rad = (x - np.dot(x - c, n) * n) - c
    nrm = float(np.linalg.norm(rad))
    return rad / nrm if nrm >= 1e-15 else _default_tangent(n)


def _circle_group_frame(X, rows, n, base, r):
    pts = X[rows]
    t = float(np.mean((pts - base[None, :]) @ n))
    c = base + t * n
    if r < 0.0:
        pp = pts - ((pts - c[None, :]) @ n)[:, None] * n[None, :]
        rad = pp - c[None, :]
        rad = rad - (rad @ n)[:, None] * n[None, :]
        r = float(np.mean(np.linalg.norm(rad, axis=1)))
    return c, r


def enforce(X, progs):
    """Project positions ``X`` (nv, 3) in place, module by module in the reference's order."""
    for prog, _fx in progs:
        P = np.asarray(prog.params, dtype=float).reshape(-1, 7)
        for seg in prog.program:
            if seg[0] == "fixed":
                for row, k in seg[1]:
                    n, p, r = P[k, :3], P[k, 3:6], P[k, 6]
                    X[row] = _onto_plane(X[row], n, p) if prog.name == PLANE else _onto_circle(X[row], n, p, r)
            elif seg[0] == "plane_group":
                n = P[seg[1], :3]
                rows = [r for r, _s in seg[2]]
                centroid = np.mean(X[rows], axis=0)
                for row, skip in seg[2]:
                    if not skip:
                        X[row] = _onto_plane(X[row], n, centroid)
            else:
                n, base, r = P[seg[1], :3], P[seg[1], 3:6], P[seg[1], 6]
                c, r = _circle_group_frame(X, seg[2], n, base, r)
                if not np.isfinite(r) or r <= 0.0:
                    continue
                for row in seg[2]:
                    X[row] = _onto_circle(X[row], n, c, r)


def rows(X, progs):
    """Sparse constraint rows ``[(rows, vecs)]`` in the reference's order (constraint_gradients_rows_array)."""
    out = []
    for prog, fixed_of in progs:
        P = np.asarray(prog.params, dtype=float).reshape(-1, 7)
        for seg in prog.program:
            if seg[0] == "fixed":
                for (row, k), vid in zip(seg[1], seg[2]):
                    if fixed_of(vid):
                        continue
                    n = P[k, :3]
                    out.append((np.array([row]), n.reshape(1, 3).copy()))
                    if prog.name == CIRCLE:
                        out.append((np.array([row]), _radial_hat(X[row], n, P[k, 3:6]).reshape(1, 3)))
            elif seg[0] == "plane_group":
                n = P[seg[1], :3]
                for (row, _s), vid in zip(seg[2], seg[3]):
                    if not fixed_of(vid):
                        out.append((np.array([row]), n.reshape(1, 3).copy()))
            else:
                n, base, r = P[seg[1], :3], P[seg[1], 3:6], P[seg[1], 6]
                c, r = _circle_group_frame(X, seg[2], n, base, r)
                if not np.isfinite(r) or r <= 0.0:
                    continue
                ref = seg[2][0]
                for row, vid in zip(seg[2], seg[3]):
                    if fixed_of(vid):
                        continue
                    if row != ref:
                        out.append((np.array([ref, row]), np.stack([-n, n])))
                    out.append((np.array([row]), _radial_hat(X[row], n, c).reshape(1, 3)))
    return out


def _coalesce(r, v):
    if r.size <= 1:
        return r.reshape(-1), v.reshape(-1, 3)
    order = np.argsort(r, kind="stable")
    r, v = r[order], v[order]
    u, inv = np.unique(r, return_inverse=True)
    if u.size == r.size:
        return r, v
    w = np.zeros((u.size, 3))
    np.add.at(w, inv, v)
    return u, w


def _solve(A, b):
    try:
        Lc = np.linalg.cholesky(A)
        return np.linalg.solve(Lc.T, np.linalg.solve(Lc, b))
    except np.linalg.LinAlgError:
        try:
            return np.linalg.solve(A, b)
        except np.linalg.LinAlgError:
            return None


def stacked(grad_shape, dense, sparse):
    """C (k, 3 nv) of the dense rows, then the sparse rows (runtime/constraint_projection.py:101-129)."""
    n = int(np.prod(grad_shape))
    C = np.zeros((len(dense) + len(sparse), n))
    for i, g in enumerate(dense):
        C[i] = np.asarray(g, dtype=float).reshape(-1)
    for j, (r, v) in enumerate(sparse):
        np.add.at(C[len(dense) + j].reshape(-1, 3), r, v)
    return C


def project_gradient(grad, dense, sparse):
    """The reference's apply_gradient_modifications_array on row lists (constraint_manager.py:174-315): one
    sparse row or one dense row alone by its closed form, more rows by the mixed KKT solve; a system that neither
    Cholesky nor LU can solve leaves ``grad`` untouched.  Returns "project", "skip" or "none"."""
    sparse = [_coalesce(np.asarray(r, dtype=int).reshape(-1), np.asarray(v, dtype=float)) for r, v in sparse]
    sparse = [(r, v) for r, v in sparse if r.size]
    if len(dense) + len(sparse) == 0:
        return "none"
    if len(dense) + len(sparse) == 1:
        if dense:
            g = dense[0]
            nsq = float(np.sum(g * g))
            if nsq > 1e-18:
                grad -= (float(np.sum(grad * g)) / nsq) * g
            return "project"
        r, v = sparse[0]
        nsq = float(np.sum(v * v))
        if nsq > 1e-18:
            upd = np.zeros_like(grad)
            np.add.at(upd, r, v)
            grad -= (float(np.sum(grad[r] * v)) / nsq) * upd
        return "project"
    C = stacked(grad.shape, dense, sparse)
    A = C @ C.T
    A[np.diag_indices_from(A)] += 1e-18
    lam = _solve(A, C @ grad.reshape(-1))
    if lam is None:
        return "skip"
    grad.reshape(-1)[:] -= C.T @ lam
    return "project"


def gram(dense, sparse):
    """C Cᵀ of the stacked rows without forming C (C is k x 3 nv; the pin rows touch a rim)."""
    k = len(dense) + len(sparse)
    A = np.zeros((k, k))
    flat = [np.asarray(d, dtype=float).reshape(-1, 3) for d in dense]
    for i, d in enumerate(flat):
        for j in range(i, len(flat)):
            A[i, j] = A[j, i] = float(np.sum(d * flat[j]))
    by_row = {}
    for j, (r, v) in enumerate(sparse):
        jj = len(dense) + j
        for i, d in enumerate(flat):
            A[i, jj] = A[jj, i] = float(np.sum(d[r] * v))
        for rr, vv in zip(np.asarray(r).reshape(-1), np.asarray(v).reshape(-1, 3)):
            by_row.setdefault(int(rr), []).append((jj, vv))
    for entries in by_row.values():
        for a, (ja, va) in enumerate(entries):
            for jb, vb in entries[a:]:
                d = float(np.dot(va, vb))
                A[ja, jb] += d
                if jb != ja:
                    A[jb, ja] += d
    return A


def decision(X, progs, dense_rows=()):
    """Project-or-skip decision of the KKT solve the rows take ("project", "skip" or "none") and the row count /
    rank of C (that of C Cᵀ)."""
    sparse = [_coalesce(np.asarray(r), np.asarray(v)) for r, v in rows(X, progs)]
    k = len(dense_rows) + len(sparse)
    if k == 0:
        return "none", 0, 0
    A = gram(list(dense_rows), sparse)
    # (a diagnostic: the eigen-decomposition is skipped for long rims, rank -1 then)
    rank = int(np.linalg.matrix_rank(A, hermitian=True)) if k <= 2048 else -1
    if k == 1:
        return "project", 1, rank
    A[np.diag_indices_from(A)] += 1e-18
    return ("project" if _solve(A, np.zeros(k)) is not None else "skip"), k, rank


class DeviceTables:
    """What ms_set_pins uploads (external rows; the library maps them to its row order)."""

    def __init__(self):
        self.params = []        # (k, 7) rows of every module, concatenated
        self.stage_kind = []    # STAGE_*
        self.stage_param = []   # group stages: the group's param row, else -1
        self.stage_off = [0]    # into items
        self.item_row = []
        self.item_arg = []      # fixed stages: OP_* << 24 | param row; plane groups: 1 = member is fixed (kept)
        self.lane = "none"      # "project", "skip" or "none": the KKT decision of pins (+ volume row)
        self.grad_row = []      # project lane: rows with their own directions
        self.grad_kind = []     # GRAD_*
        self.grad_param = []
        self.avg_param = []     # slide-circle groups: the normal-component mean over the rows' support
        self.avg_off = [0]
        self.avg_row = []
        self.n_rows = 0
        self.rank = 0

    def _stage(self, kind, param, items):
        self.stage_kind.append(kind)
        self.stage_param.append(param)
        for r, a in items:
            self.item_row.append(int(r))
            self.item_arg.append(int(a))
        self.stage_off.append(len(self.item_row))


def device_tables(X, progs, dense_rows=()):
    """Stages of the enforcement kernel and the project lane's gradient tables.  A fixed segment is cut into
    levels (level j holds the j-th op of every row), so a stage touches a row at most once and the ops of one row
    keep their order; each group is a stage of its own."""
    t = DeviceTables()
    for prog, fixed_of in progs:
        base = len(t.params)
        t.params += prog.params
        op = OP_PLANE if prog.name == PLANE else OP_CIRCLE
        for seg in prog.program:
            if seg[0] == "fixed":
                levels, seen = [], {}
                for row, k in seg[1]:
                    j = seen.get(row, 0)
                    seen[row] = j + 1
                    if j == len(levels):
                        levels.append([])
                    levels[j].append((row, (op << 24) | (base + k)))
                for lv in levels:
                    t._stage(STAGE_FIXED, -1, lv)
            elif seg[0] == "plane_group":
                t._stage(STAGE_PLANE_GROUP, base + seg[1], [(r, int(s)) for r, s in seg[2]])
            else:
                t._stage(STAGE_CIRCLE_GROUP, base + seg[1], [(r, 0) for r in seg[2]])
    t.lane, t.n_rows, t.rank = decision(X, progs, dense_rows)
    if t.lane != "project":
        return t
    owner = {}

    def claim(row, what):
        if row in owner and owner[row] != what:
            raise L.MembraneHipError(
                "pin rows of two constraints on one vertex with a full-rank KKT system are outside the HIP path")
        owner[row] = what

    off = 0
    for prog, fixed_of in progs:
        for seg in prog.program:
            if seg[0] == "fixed":
                kind = GRAD_PLANE if prog.name == PLANE else GRAD_CIRCLE
                for (row, k), vid in zip(seg[1], seg[2]):
                    if fixed_of(vid) or (row in owner and owner[row] == ("f", off + k)):
                        continue
                    claim(row, ("f", off + k))
                    t.grad_row.append(row)
                    t.grad_kind.append(kind)
                    t.grad_param.append(off + k)
            elif seg[0] == "plane_group":
                for (row, _s), vid in zip(seg[2], seg[3]):
                    if fixed_of(vid):
                        continue
                    claim(row, ("p", off + seg[1]))
                    t.grad_row.append(row)
                    t.grad_kind.append(GRAD_PLANE)
                    t.grad_param.append(off + seg[1])
            else:
                ref = seg[2][0]
                support = []
                for row, vid in zip(seg[2], seg[3]):
                    if row == ref or not fixed_of(vid):
                        support.append(row)
                        claim(row, ("c", off + seg[1]))
                    if not fixed_of(vid):
                        t.grad_row.append(row)
                        t.grad_kind.append(GRAD_RADIAL)
                        t.grad_param.append(off + seg[1])
                if len(support) > 1:
                    t.avg_param.append(off + seg[1])
                    t.avg_row += support
                    t.avg_off.append(len(t.avg_row))
        off += len(prog.params)
    return t
