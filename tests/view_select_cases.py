"""The scenes of the view selection's tests (tests/test_view_select_host.py, tests/test_gpu_view_select.py) on the known grid's three
grids, with the view gain's small camera.  `base_case` is built on the largest grid so that the NumPy restatement alone
(tests/view_select_reference.py) meets the five conditions of `conditions`; the two smaller grids, too small to hold them, carry the
view gain's poses with two of them repeated.  Nothing here calls the library."""
import numpy as np

import known_reference as kr

RES = 0.5
BASE_DIMS = (24, 20, 70)
BASE_RANGE = 4.0


def _look(eye, target, up=(0.0, 0.0, 1.0)):
    """engine.look_at's pose for an axis that is not parallel to `up`"""
    eye, target, up = (np.asarray(v, dtype=np.float64) for v in (eye, target, up))
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(z, up)
    x = x / np.linalg.norm(x)
    return np.ascontiguousarray(np.column_stack([x, np.cross(z, x), z, eye]).reshape(12))


def base_case():
    """(occupied bool [X, Y, Z], K's fills as map_known_fill takes them, poses [8, 12])
    The half x < 6 m is seen; beyond it everything is unknown but one box in front of view 2.  A piece of wall stands in view 0's way.
      0, 1   two nearly identical views down +x at z = 8 m: the two largest gains
      2      the same direction at z = 14 m, looking elsewhere; the known box takes some of its gain
      3      a pose with a NaN: status 1
      4      view 2 again, to the byte
      5      looks back into the seen half: scored, gain 0
      6      near view 2 and further back: it reaches little of the unknown half
      7      straight up under the ceiling at the far end: unknown space of its own, a small gain"""
    X, Y, Z = BASE_DIMS
    occ = np.zeros(BASE_DIMS, dtype=bool)
    occ[17, 6:12, 14:19] = True
    fills = [((0, 0, 0, 11, Y - 1, Z - 1), 1), ((12, 0, 24, 14, Y - 1, 30), 1)]
    poses = [_look((5.0, 5.0, 8.0), (9.0, 5.0, 8.0)), _look((5.0, 5.05, 8.02), (9.0, 5.05, 8.02)), _look((5.0, 5.0, 14.0), (9.0, 5.0, 14.0)),
             _look((5.0, 5.0, 8.0), (9.0, 5.0, 8.0)), _look((5.0, 5.0, 14.0), (9.0, 5.0, 14.0)), _look((4.0, 5.0, 20.0), (0.0, 5.0, 20.0)),
             _look((3.5, 5.5, 14.2), (7.5, 5.5, 14.2)), _look((11.0, 2.0, 33.6), (11.0, 2.0, 34.6), up=(1.0, 0.0, 0.0))]
    poses[3][6] = np.nan
    return occ, fills, np.array(poses)


def generic_case(dims, look_at, seed=3):
    """(occupied, fills, poses [9, 12]) on any grid: the view gain's six candidates (two inside, one in an occupied voxel, one straight
    down, one outside, one with a NaN), the first two again, and the first looking the other way"""
    rng = np.random.default_rng(seed)
    occ = rng.uniform(size=dims) < 0.2
    occ[0, 0, 0] = False
    ext = np.array(dims) * RES
    cell = np.argwhere(occ)
    cell = cell[len(cell) // 2]
    poses = [look_at(0.4 * ext, ext * (0.9, 0.6, 0.5)), look_at((0.25, 0.25, 0.25), ext - 0.25), look_at((cell + 0.5) * RES, 0.5 * ext + 0.01),
             look_at(ext * (0.6, 0.5, 0.9), ext * (0.6, 0.5, 0.0)), look_at(ext + 1.0, 0.5 * ext), look_at(0.4 * ext, ext * (0.1, 0.6, 0.5))]
    poses[5][5] = np.nan
    poses += [poses[0].copy(), poses[1].copy(), look_at(0.4 * ext, ext * (0.1, 0.4, 0.5))]
    fills = []
    for i in range(8):
        lo = [int(rng.integers(0, d)) for d in dims]
        hi = [int(rng.integers(l, min(d, l + max(2, d // 2)))) for l, d in zip(lo, dims)]
        fills.append((tuple(lo + hi), 0 if i % 3 == 2 else 1))
    return occ, fills, np.array(poses)


def known_of(dims, fills):
    k = np.zeros(dims, dtype=bool)
    for box, value in fills:
        k = kr.fill(k, box, value)
    return k


def conditions(ref, k):
    """what the base case must meet on the restatement alone (ref = view_select_reference.select with k_select = n_views, min_gain = 1),
    before anything is compared"""
    import view_select_reference as sr
    rows, sel, rnd = ref["rows"], ref["select"], ref["round"]
    n, n_selected = len(rows), ref["info"][2]
    picked = sel[:n_selected, 0].tolist()
    # 1: the greedy set is not the top k by solo gain - two nearly identical poses hold the two largest gains, a third with a smaller
    #    one, looking elsewhere, is picked second
    top = sr.top_k_by_solo_gain(rows, 3)
    assert sorted(top[:2]) == [0, 1] and picked[0] in (0, 1) and picked[1] == 2 and rows[2, 1] < min(rows[0, 1], rows[1, 1]), (rows[:, 1], picked)
    assert picked[:2] != top[:2] and sel[1, 3] == 0                                # view 2 shares nothing with the first pick
    # 2: round 1 has a tie, broken to the lower index: views 2 and 4 are the same pose
    assert np.array_equal(rows[2], rows[4]) and rnd[2] == 1 and rnd[4] == -1
    # 3: the duplicate's marginal falls to 0, and with min_gain = 1 the selection ends early
    assert not (ref["sets"][4] & ~ref["claimed_mask"]).any() and n_selected < n == len(sel) and (sel[n_selected:] == [-1, 0, 0, 0]).all()
    # 4: one view has status 1 and one scored view has gain 0
    assert rows[3].tolist() == [1, 0, 0, 0, 0, 0, 0, 0] and rows[5, 0] == 0 and rows[5, 1] == 0 and rnd[3] == rnd[5] == -1
    # 5: marginals never increase; the last cumulative is what was claimed beyond K and is below the sum of the picked views' own gains
    assert n_selected >= 3 and (np.diff(sel[:n_selected, 1]) <= 0).all() and (sel[:n_selected, 1] >= 1).all()
    claimed = kr.unpack(ref["claimed"], k.shape)
    assert sel[n_selected - 1, 2] == int((claimed & ~k).sum()) == ref["info"][3] < ref["info"][4] and (claimed & k).sum() == k.sum()
