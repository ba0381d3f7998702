"""Exact references of the device map products (csrc/map_build.hip) in plain numpy, for the host and the device tests of
tests/mapbuild_cases.py.  Integers until the one final square root; no knowledge of how the kernels find their answers.

exact_d2          occupancy -> squared voxel distance to the nearest occupied voxel (int64), a separable min-plus over z, y, x
esdf_from_d2      res * sqrt(d2) in float64, the double the reference stores (GridMap3D::generateESDF3d)
brute_d2          the same integer as a minimum over all occupied voxels, O(n^2): what exact_d2 is itself held to
gather_reference  the rule of oracle/pyoracle.py::gather_points with box slices in place of its triple loop"""
import numpy as np

NONE = 1 << 40                                   # "nothing here": above every squared distance of a 4096^3 grid, far below int64's end
DBL_MAX = float(np.finfo(np.float64).max)


def _minplus(f, axis):
    """out(q) = min over p of (q - p)^2 + f(p) along one axis: for every offset r, out = min(out, f shifted by +-r, + r^2)."""
    f = np.ascontiguousarray(np.moveaxis(f, axis, 0))
    out = f.copy()
    for r in range(1, f.shape[0]):
        rr = r * r
        np.minimum(out[r:], f[:-r] + rr, out=out[r:])
        np.minimum(out[:-r], f[r:] + rr, out=out[:-r])
    return np.moveaxis(out, 0, axis)            # out starts as f, so NONE + r^2 never survives: out <= NONE


def exact_d2(occ):
    """int64 [X][Y][Z]: the squared index distance to the nearest occupied voxel; NONE everywhere on a map without one."""
    f = np.where(np.asarray(occ) != 0, 0, NONE).astype(np.int64)
    for axis in (2, 1, 0):
        f = _minplus(f, axis)
    return np.ascontiguousarray(f)


def esdf_from_d2(d2, res):
    """float64: res * sqrt(d2); a map with no occupied voxel gives res * sqrt(DBL_MAX) (fillESDF's start value never lowered)."""
    v = d2.astype(np.float64)
    v[d2 >= NONE] = DBL_MAX
    return res * np.sqrt(v)


def brute_d2(occ):
    """exact_d2 by its definition: per voxel the minimum over ALL occupied voxels (small grids only)."""
    occ = np.asarray(occ)
    P = np.argwhere(occ != 0).astype(np.int64)
    Q = np.argwhere(np.ones(occ.shape, dtype=bool)).astype(np.int64)
    if P.shape[0] == 0:
        return np.full(occ.shape, NONE, dtype=np.int64)
    d = ((Q[:, None, :] - P[None, :, :]) ** 2).sum(axis=2)
    return d.min(axis=1).reshape(occ.shape)


def gather_indices(occ, bmin, bmax, res, waypoints, half, offset=None):
    """int64 [M][3], sorted by (ix, iy, iz): the occupied voxels of every waypoint's index box [w - half + offset, w + half + offset]
    (corners clamped into the map, floor-indexed) that lie outside the PREVIOUS waypoint's box without offset; the first previous
    waypoint is (999, 999, 999)."""
    occ = np.asarray(occ)
    dims = np.array(occ.shape, dtype=np.int64)
    bmin = np.asarray(bmin, dtype=np.float64); bmax = np.asarray(bmax, dtype=np.float64)
    half = np.asarray(half, dtype=np.float64) * np.ones(3)
    off = np.zeros(3) if offset is None else np.asarray(offset, dtype=np.float64)

    def corner(p):
        q = np.minimum(np.maximum(p, bmin), bmax)
        return np.clip(np.floor((q - bmin) / res).astype(np.int64), 0, dims - 1)
    mark = np.zeros(occ.shape, dtype=bool)
    last = np.array([999.0, 999.0, 999.0])
    for w in np.asarray(waypoints, dtype=np.float64).reshape(-1, 3):
        lo, hi = corner(w - half + off), corner(w + half + off)
        llo, lhi = corner(last - half), corner(last + half)
        box = np.ones(tuple(np.maximum(hi - lo + 1, 0)), dtype=bool)
        a, b = np.maximum(llo, lo) - lo, np.minimum(lhi, hi) - lo          # the previous box, cut to this one, in its coordinates
        if np.all(a <= b):
            box[a[0]:b[0] + 1, a[1]:b[1] + 1, a[2]:b[2] + 1] = False
        mark[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1] |= box
        last = w
    mark &= occ != 0
    return np.argwhere(mark).astype(np.int64)


def gather_reference(occ, bmin, bmax, res, waypoints, half, offset=None):
    """float64 [M][3]: the centres (i + 0.5) * res + bmin of gather_indices, product and sum rounded separately (getGridCubeCenter)."""
    I = gather_indices(occ, bmin, bmax, res, waypoints, half, offset)
    return (I.astype(np.float64) + 0.5) * res + np.asarray(bmin, dtype=np.float64)
