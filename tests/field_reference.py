"""The tests' own reference of the cost-to-go field (include/isdf_accel.h, isdf_frontend_field_*), written from the definition and not
from the C++: d[goal] = 0, d[v] = min over free 26-neighbours u of d[u] + w with w = math.sqrt(i*i + j*j + k*k), the least fixed point
from +inf - a heapq Dijkstra.  Python floats are IEEE doubles and `+` is one rounded addition, so the bytes are those of the definition.
Also the small maps the CPU and the GPU tests share (occupancy: 1 = occupied)."""
import heapq
import math

import numpy as np

NEIGHBOURS = [(i, j, k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1) if (i, j, k) != (0, 0, 0)]     # the A*'s i, j, k loop order
EDGE = [math.sqrt(q) for q in range(4)]


def field(free, goal):
    """free: bool [X, Y, Z]; goal: voxel index (may lie outside the map).  Returns d, float64 [X, Y, Z]."""
    X, Y, Z = free.shape
    d = np.full((X, Y, Z), np.inf)
    gx, gy, gz = (int(v) for v in goal)
    if not (0 <= gx < X and 0 <= gy < Y and 0 <= gz < Z) or not free[gx, gy, gz]:
        return d
    fr = free.tolist()
    dd = [[[math.inf] * Z for _ in range(Y)] for _ in range(X)]
    dd[gx][gy][gz] = 0.0
    heap = [(0.0, gx, gy, gz)]
    while heap:
        key, x, y, z = heapq.heappop(heap)
        if key > dd[x][y][z]:
            continue
        for i, j, k in NEIGHBOURS:
            vx, vy, vz = x + i, y + j, z + k
            if vx < 0 or vx >= X or vy < 0 or vy >= Y or vz < 0 or vz >= Z or not fr[vx][vy][vz]:
                continue
            cand = key + EDGE[i * i + j * j + k * k]
            if cand < dd[vx][vy][vz]:
                dd[vx][vy][vz] = cand
                heapq.heappush(heap, (cand, vx, vy, vz))
    return np.array(dd, dtype=np.float64)


def same_bytes(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def open_map(dims=(9, 7, 5)):
    return np.zeros(dims, dtype=np.uint8)


def wall_with_gap(dims=(9, 7, 5)):
    occ = np.zeros(dims, dtype=np.uint8)
    occ[4, :, :] = 1
    occ[4, 3, 2] = 0
    return occ


def sealed_pocket(dims=(9, 7, 5)):
    """a one-voxel shell around the 3 x 3 x 3 cells [4:7, 2:5, 1:4]"""
    occ = np.zeros(dims, dtype=np.uint8)
    occ[3:8, 1:6, 0:5] = 1
    occ[4:7, 2:5, 1:4] = 0
    return occ


POCKET_CELL = (5, 3, 2)


def serpentine(dims):
    """walls on every odd row y, each with a gap at alternating ends of x: one corridor that runs the length of x again and again"""
    occ = np.zeros(dims, dtype=np.uint8)
    for y in range(1, dims[1], 2):
        occ[:, y, :] = 1
        occ[dims[0] - 1 if (y // 2) % 2 == 0 else 0, y, :] = 0
    return occ


def table_from_free(free, n_att=121):
    """a configuration-space table (uint32 [X, Y, Z, 4 * ceil(n_att / 128)]) whose free voxels each have ONE attitude bit set, spread over the words"""
    X, Y, Z = free.shape
    nw = 4 * ((n_att + 127) // 128)
    t = np.zeros((X, Y, Z, nw), dtype=np.uint32)
    x, y, z = np.nonzero(free)
    a = (x + 3 * y + 5 * z) % n_att
    t[x, y, z, a // 32] = np.uint32(1) << (a % 32).astype(np.uint32)
    return t
