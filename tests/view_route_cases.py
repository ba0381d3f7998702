"""The scenes of the routed view selection's tests (tests/test_view_route_host.py, tests/test_gpu_view_route.py).  Nothing here calls
the library.

CPU: tests/view_select_cases.py's base case with travel costs chosen against its gains, and a known grid cut so that two views have the
marginals 4 and 2 exactly.

GPU: tests/test_gpu_field_known.py's map (tests/test_gpu_map_update.py's 24 x 20 x 70 voxels at 0.5 m, kernel_size 5, 3 x 3 attitudes): a
wall across x = 16 with one gap, a baffle across x = 8 over z 14 .. 39, the half z < 35 seen.  The robot stands at START = (3, 10, 30);
the eyes, as voxels:
  0  NEAR     (5, 10, 29) looking up: two cells from the robot, three unknown layers in range
  1  FAR      (21, 10, 32) looking up, beyond the wall: more unknown layers in range, a long way through the gap
  2  BAFFLED  (12, 10, 30) looking up, behind the baffle: nine cells from the robot in a straight line, under the baffle by the field
  3  CLOSED   (15, 3, 30) looking up, against the wall: free in the occupancy, closed for every attitude in the configuration space
  4  UNSEEN   (5, 4, 40) looking along +x, in unseen space: reached by the ungated field only
  5  OUTSIDE  outside the map: status 1, cost +inf
  6  BAD      NEAR's eye with a NaN in the rotation: status 1, a finite cost
  7  NEAR again, to the byte: ties with 0 on utility, adds nothing once 0 is picked
  8  LOW      (3, 10, 12) looking down: eighteen cells below the robot in the open, nothing unknown in range (gain 0)
  9  FAR2     (21, 4, 32) looking up
  10 MID      (5, 16, 31) looking up"""
import numpy as np

from view_select_cases import _look

START = (3, 10, 30)
RANGE_M = 4.0
EYES = [(5, 10, 29), (21, 10, 32), (12, 10, 30), (15, 3, 30), (5, 4, 40), None, (5, 10, 29), (5, 10, 29), (3, 10, 12), (21, 4, 32), (5, 16, 31)]
NEAR, FAR, BAFFLED, CLOSED, UNSEEN, OUTSIDE, BAD, NEAR2, LOW, FAR2, MID = range(11)


def centre(cell, bmin, res):
    return (np.asarray(cell, dtype=np.float64) + 0.5) * res + np.asarray(bmin, dtype=np.float64)


def cells_of(xyz, bmin, res, dims):
    """the cell of each point as the field takes it, and whether the point lies in the map's box (points on the upper faces included)"""
    p = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    bmin = np.asarray(bmin, dtype=np.float64)
    bmax = bmin + np.asarray(dims) * res
    inside = ~((p < bmin).any(axis=1) | (p > bmax).any(axis=1))
    idx = np.clip(np.floor((np.where(inside[:, None], p, bmin) - bmin) / res).astype(np.int64), 0, np.asarray(dims) - 1)
    return idx, inside


def field_at(d, xyz, bmin, res):
    """what isdf_frontend_field_value answers for a field d: d at the point's cell, +inf outside the map"""
    idx, inside = cells_of(xyz, bmin, res, d.shape)
    return np.where(inside, d[tuple(idx.T)], np.inf)


def gpu_poses(bmin, res):
    """[11, 12] poses for the eyes above"""
    out = []
    for i, cell in enumerate(EYES):
        if cell is None:
            eye = np.asarray(bmin, dtype=np.float64) - 1.0
            out.append(_look(eye, eye + (1.0, 0.0, 0.0)))
            continue
        eye = centre(cell, bmin, res)
        if i == UNSEEN:
            out.append(_look(eye, eye + (4.0, 0.0, 0.0)))
        elif i == LOW:
            out.append(_look(eye, eye - (0.0, 0.0, 4.0), up=(1.0, 0.0, 0.0)))
        else:
            out.append(_look(eye, eye + (0.0, 0.0, 4.0), up=(1.0, 0.0, 0.0)))
    out[BAD][6] = np.nan
    return np.array(out)


def eyes_of(poses):
    return np.ascontiguousarray(np.asarray(poses).reshape(-1, 3, 4)[:, :, 3])


def tie_known(sets_a, sets_b, dims):
    """K all known but four voxels only view a sees and two only view b sees (the first of each in index order)"""
    only_a, only_b = np.flatnonzero(sets_a & ~sets_b), np.flatnonzero(sets_b & ~sets_a)
    assert len(only_a) >= 4 and len(only_b) >= 2
    k = np.ones(int(np.prod(dims)), dtype=bool)
    k[only_a[:4]] = False
    k[only_b[:2]] = False
    return k.reshape(dims)
