"""The scenes of the candidate views' tests (tests/test_view_cand_host.py, tests/test_gpu_view_cand.py): per grid an occupancy of one
wall over half the room's width, a K of a few box fills, eight targets and sixteen offsets chosen so that the NumPy restatement alone
meets every status, a target with more kept candidates than k_best, a target with none, and a tie in gain.  Nothing here calls the library."""
import numpy as np

import known_reference as kr

RES = 0.5
JIT = np.array([0.01, -0.02, 0.03])     # the targets are not at voxel centres


def scene(dims):
    """(occupied bool [X, Y, Z], K's fills as map_known_fill takes them, targets [8, 3], offsets [16, 3])
    A room x < a, all free and seen but for one unknown corner voxel; a wall at x = a over the lower half of y; behind it unknown
    space with one known strip."""
    X, Y, Z = dims
    a = X // 2
    occ = np.zeros(dims, dtype=bool)
    occ[a, :max(1, Y // 2), :] = True
    fills = [((0, 0, 0, a, Y - 1, Z - 1), 1), ((0, Y - 1, Z - 1, 0, Y - 1, Z - 1), 0), ((a + 1, 0, 0, X - 1, 0, Z // 2), 1)]
    c = lambda *v: (np.array(v) + 0.5) * RES                   # noqa: E731
    targets = np.array([
        c(a - 1, Y // 2, Z // 2) + JIT,         # 0: beside the wall, in the room: many eyes keep it
        c(a, 0, Z // 2) + JIT,                  # 1: a voxel of the wall: a hit at the target's own voxel is visible
        c(X - 1, 0, Z // 2) + JIT,              # 2: behind the wall
        [np.nan, 1.0, 1.0],                     # 3: keeps none
        c(a - 1, Y // 2, Z // 2) + JIT,         # 4: target 0 again
        [-1.0, 0.5, 0.5],                       # 5: outside the map
        c(1, Y // 2, Z // 2),                   # 6: a voxel centre: the offset straight down looks straight up
        c(1, 1, 1),                             # 7: the offset (-0.5, -0.5, -0.5) puts the eye into the corner voxel
    ])
    offsets = np.array([
        [-0.5, 0.0, 0.0], [-1.0, 0.0, 0.0], [-1.0, 0.0, 0.5], [-1.0, 0.0, -0.5], [-1.0, 0.5, 0.0], [-1.0, -0.5, 0.0],
        [0.0, 0.0, 0.0],                        # the eye is the target
        [0.0, 0.0, -0.5],                       # straight below: beside the wall for target 0 (close), inside it for target 1 (occupied), the pose's second branch for target 6
        [0.5, 0.0, 0.0],                        # target 0: in the opening beside the wall's edge
        [1.0, 0.0, 0.0],                        # target 0: beyond the wall's plane, unknown
        [np.nan, 0.0, 0.0], [100.0, 0.0, 0.0],
        [-1.0, 0.0, 0.0],                       # offset 1 again: a tie in gain
        [-(X - 2) * RES, 0.0, 0.0],             # target 2: an eye in the room, the wall between
        [-0.5, -0.5, -0.5],
        [-0.5, 0.5, 0.0],
    ])
    return occ, fills, targets, offsets


def random_scene(dims, seed, n_targets=24, n_offsets=20):
    """(occupied bool, K's fills, targets, offsets): an occupancy of a few small boxes and a K of boxes set and cleared in turn, as
    tests/test_gpu_map_known.py's _random_fills makes them, over a known lower half - K's words have structure at every alignment, so
    the clearance cube's columns start at every bit of a word and many cross into the next.  Targets anywhere in the map, offsets up to
    1.5 m."""
    rng = np.random.default_rng(seed)
    occ = np.zeros(dims, dtype=bool)
    for _ in range(6):
        lo = [int(rng.integers(0, d)) for d in dims]
        occ[tuple(slice(l, min(d, l + int(rng.integers(1, max(2, d // 6) + 1)))) for l, d in zip(lo, dims))] = True
    fills = [((0, 0, 0, dims[0] - 1, dims[1] - 1, dims[2] // 2), 1)]
    for i in range(24):
        lo = [int(rng.integers(0, d)) for d in dims]
        hi = [int(rng.integers(l, min(d, l + max(2, d // 2)))) for l, d in zip(lo, dims)]
        fills.append((tuple(lo + hi), 0 if i % 3 == 2 else 1))
    targets = rng.uniform(0.02, 0.98, (n_targets, 3)) * np.array(dims) * RES
    return occ, fills, targets, rng.uniform(-1.5, 1.5, (n_offsets, 3))


def cube_columns_crossing_words(cand, dims, radius):
    """of the candidates that reached the clearance test: how many of their cubes hold a column whose z run crosses a word of K"""
    n = 0
    for status, voxel in cand[cand[:, 0] != 1][:, :2]:
        if status in (2, 3):
            continue
        x, y, z = voxel // (dims[1] * dims[2]), voxel // dims[2] % dims[1], voxel % dims[2]
        z0, z1 = max(z - radius, 0), min(z + radius, dims[2] - 1)
        starts = [((cx * dims[1] + cy) * dims[2] + z0) & 31 for cx in range(max(x - radius, 0), min(x + radius, dims[0] - 1) + 1)
                  for cy in range(max(y - radius, 0), min(y + radius, dims[1] - 1) + 1)]
        n += any(s + (z1 - z0) > 31 for s in starts)
    return n


def known_of(dims, fills):
    k = np.zeros(dims, dtype=bool)
    for box, value in fills:
        k = kr.fill(k, box, value)
    return k


def conditions(cand, rows_t, best, n_offsets, k_best):
    """what every base case must meet on the restatement, before anything is compared"""
    assert sorted(set(cand[:, 0].tolist())) == [0, 1, 2, 3, 4, 5], np.bincount(cand[:, 0], minlength=6)
    assert (rows_t[:, 0] > k_best).any(), rows_t[:, 0]
    assert (rows_t[:, 0] == 0).any()
    tie = False
    for i in range(len(rows_t)):
        g = cand[i * n_offsets:(i + 1) * n_offsets]
        g = g[g[:, 0] == 0, 3]
        tie = tie or len(np.unique(g[g >= 1])) < (g >= 1).sum()
    assert tie, "no two kept candidates of one target tie at a gain >= 1"
