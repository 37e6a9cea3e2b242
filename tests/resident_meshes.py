"""Meshes whose vertex counts sit at the tile-count edges of the resident step kernel (csrc/ms_resident.inc): the
displaced icosphere with its last k vertices cut out.  Shared by test_host_logic.py (what the cut leaves, on the CPU)
and test_gpu_resident_fullsize.py (the kernel on those meshes)."""
from __future__ import annotations

import numpy as np

# (freq, k) -> (nv, tiles of 256 rows, owned rows of the last tile).  f = 81, k = 0 is BASELINE config 2 itself.
CUT_TABLE = {
    (81, 0): (65612, 257, 76),
    (81, 75): (65537, 257, 1),
    (81, 76): (65536, 256, 256),
    (81, 77): (65535, 256, 255),
    (81, 332): (65280, 255, 256),
    (115, 1180): (131072, 512, 256),
    (115, 1179): (131073, 513, 1),
    (114, 0): (129962, 508, 170),
    (115, 0): (132252, 517, 156),
}


def _cut_icosphere(freq, k):
    """meshgen.icosphere(freq) displaced by smooth_displace(., 0.05), without its last k vertices and every facet that
    touches one of them, relabelled to the vertices still in use.  -> (positions float64, rows int32), C-contiguous."""
    from membrane_solver_amd import meshgen

    P, T = meshgen.icosphere(freq)
    P = meshgen.smooth_displace(P, 0.05)
    if k:
        nv = len(P) - k
        T = T[(T < nv).all(axis=1)]
        used = np.zeros(len(P), dtype=bool)
        used[T.ravel()] = True
        new_id = np.cumsum(used) - 1
        P, T = P[used], new_id[T]
    return np.ascontiguousarray(P, dtype=np.float64), np.ascontiguousarray(T, dtype=np.int32)


def edge_report(nv, T):
    """-> (boundary loops, largest number of facets on one edge, vertices on no facet).  A vertex met by more than two
    boundary edges (a pinched hole) is reported as -1 loops."""
    t = np.asarray(T, dtype=np.int64)
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]], axis=0)
    e.sort(axis=1)
    uniq, counts = np.unique(e[:, 0] * np.int64(nv) + e[:, 1], return_counts=True)
    isolated = int(nv - np.unique(t).size)
    b = uniq[counts == 1]
    ba, bb = (b // nv).astype(np.int64), (b % nv).astype(np.int64)
    nbr = {}
    for u, v in zip(ba.tolist(), bb.tolist()):
        nbr.setdefault(u, []).append(v)
        nbr.setdefault(v, []).append(u)
    if any(len(n) != 2 for n in nbr.values()):
        return -1, int(counts.max()), isolated
    loops, seen = 0, set()
    for start in nbr:
        if start in seen:
            continue
        loops += 1
        prev, cur = None, start
        while cur not in seen:
            seen.add(cur)
            a, c = nbr[cur]
            prev, cur = cur, (c if a == prev else a)
    return loops, int(counts.max()), isolated
