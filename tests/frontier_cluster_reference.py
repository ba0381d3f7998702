"""A restatement of the frontier clusters' definition (include/isdf_accel.h, "frontier clusters") that shares nothing with the product's
header: a flood fill with a deque over a boolean array instead of a union-find over list positions, the neighbour offsets enumerated
by the rule, the statistics from NumPy over each component's argwhere, the representative by an explicit lexsort on (d2, voxel)."""
from collections import deque
from itertools import product

import numpy as np

ROW = 16


def offsets(connectivity):
    """the offsets in {-1, 0, 1}^3 with 1, at most 2 or at most 3 non-zero entries"""
    most = {6: 1, 18: 2, 26: 3}[connectivity]
    out = [d for d in product((-1, 0, 1), repeat=3) if 1 <= sum(v != 0 for v in d) <= most]
    assert len(out) == connectivity
    return out


def components(mask, connectivity):
    """the connected components of a boolean [X, Y, Z] array as lists of (x, y, z), in ascending order of their lowest voxel index"""
    mask = np.asarray(mask, dtype=bool)
    nx, ny, nz = mask.shape
    offs = offsets(connectivity)
    seen = np.zeros(mask.shape, dtype=bool)
    out = []
    for start in map(tuple, np.argwhere(mask)):                 # argwhere is in C order: ascending voxel index
        if seen[start]:
            continue
        seen[start] = True
        queue, members = deque([start]), []
        while queue:
            p = queue.popleft()
            members.append(p)
            for d in offs:
                q = (p[0] + d[0], p[1] + d[1], p[2] + d[2])
                if 0 <= q[0] < nx and 0 <= q[1] < ny and 0 <= q[2] < nz and mask[q] and not seen[q]:
                    seen[q] = True
                    queue.append(q)
        out.append(members)
    return out


def clusters(mask, connectivity=26, min_size=1):
    """(voxels int64 ascending, labels int32, rows int64 [n_rows, 16], counts) as the definition states them"""
    mask = np.asarray(mask, dtype=bool)
    nx, ny, nz = mask.shape
    vox = np.flatnonzero(mask.reshape(-1)).astype(np.int64)
    comp_of = np.full(mask.shape, -1, dtype=np.int64)
    rows, sizes, labels_of = [], [], []
    comps = components(mask, connectivity)
    for c, members in enumerate(comps):
        p = np.array(members, dtype=np.int64).reshape(-1, 3)
        comp_of[p[:, 0], p[:, 1], p[:, 2]] = c
        idx = (p[:, 0] * ny + p[:, 1]) * nz + p[:, 2]
        size = len(p)
        s = p.sum(axis=0)
        cell = s // size
        d2 = ((p - cell) ** 2).sum(axis=1)
        j = np.lexsort((idx, d2))[0]                            # least d2, ties to the lowest voxel index
        label = int(idx.min())
        row = [label, size] + p.min(axis=0).tolist() + p.max(axis=0).tolist() + s.tolist() + [int(idx[j]), int(d2[j]), int(np.searchsorted(vox, label)), 0, 0]
        rows.append(row)
        sizes.append(size)
        labels_of.append(label)
    assert labels_of == sorted(labels_of)
    kept = [c for c in range(len(comps)) if sizes[c] >= min_size]
    row_of = np.full(len(comps), -1, dtype=np.int32)
    row_of[kept] = np.arange(len(kept), dtype=np.int32)
    labels = row_of[comp_of.reshape(-1)[vox]].astype(np.int32) if len(vox) else np.zeros(0, dtype=np.int32)
    out = np.array([rows[c] for c in kept], dtype=np.int64).reshape(-1, ROW)
    big = max(range(len(comps)), key=lambda c: (sizes[c], -labels_of[c])) if comps else None
    counts = {"n_voxels": len(vox), "n_clusters": len(comps), "n_rows": len(kept), "n_voxels_dropped": int(sum(s for s in sizes if s < min_size)),
              "largest_size": 0 if big is None else sizes[big], "largest_label": -1 if big is None else labels_of[big]}
    return vox, labels, out, counts
