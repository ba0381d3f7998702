"""NumPy restatement of the eroded known grid's definition (include/isdf_accel.h, "planning through observed space only") on boolean
[X, Y, Z] arrays: K padded by r with `border`, the AND of the (2 r + 1)^3 shifted slices.  The bit layout is known_reference's.  Nothing
here calls the library, and nothing here is separable."""
import numpy as np

import known_reference as kr


def erode(mask, r, border):
    """E[v] = 1 iff every u with max |u - v| <= r is (inside and known) or (outside and border = 1)"""
    mask = np.asarray(mask, dtype=bool)
    r = int(r)
    padded = np.pad(mask, r, mode="constant", constant_values=bool(border))
    out = np.ones(mask.shape, dtype=bool)
    nx, ny, nz = mask.shape
    for i in range(2 * r + 1):
        for j in range(2 * r + 1):
            for k in range(2 * r + 1):
                out &= padded[i:i + nx, j:j + ny, k:k + nz]
    return out


def erode_by_count(mask, r, border):
    """the same set for a radius at which (2 r + 1)^3 slices are too many: the number of unseen voxels in each cube, from one
    summed-volume table of the padded grid, is 0.  The tests hold it to `erode` at the small radii."""
    mask = np.asarray(mask, dtype=bool)
    r = int(r)
    unseen = ~np.pad(mask, r, mode="constant", constant_values=bool(border))
    s = np.zeros(tuple(d + 1 for d in unseen.shape), dtype=np.int64)
    s[1:, 1:, 1:] = unseen.cumsum(0).cumsum(1).cumsum(2)
    nx, ny, nz = mask.shape
    w = 2 * r + 1
    lo, hi = (slice(0, nx), slice(0, ny), slice(0, nz)), (slice(w, w + nx), slice(w, w + ny), slice(w, w + nz))
    total = np.zeros(mask.shape, dtype=np.int64)
    for a in (0, 1):
        for b in (0, 1):
            for c in (0, 1):
                sign = 1 if (a + b + c) % 2 == 1 else -1          # + for the far corner, alternating
                total += sign * s[(hi if a else lo)[0], (hi if b else lo)[1], (hi if c else lo)[2]]
    return total == 0


def erode_words(words, dims, r, border):
    return kr.pack(erode(kr.unpack(words, dims), r, border))


def cleared_cube(dims, v, r):
    """the voxels one unknown voxel v clears: the cube of 2 r + 1 a side round it, clipped to the grid"""
    out = np.zeros(dims, dtype=bool)
    out[tuple(slice(max(0, c - r), min(d, c + r + 1)) for c, d in zip(v, dims))] = True
    return out
