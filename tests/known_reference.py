"""NumPy restatement of the known grid's four definitions (include/isdf_accel.h, "observed space in the map") on boolean [X, Y, Z]
arrays: the bit layout by np.packbits(..., bitorder="little"), the shift by slicing, the fill by slicing, the frontier by six shifted
ANDs.  Nothing here calls the library."""
import numpy as np


def pack(mask):
    """voxel a = (x * ny + y) * nz + z is bit a & 31 of uint32 word a >> 5; ceil(n / 32) words, the tail bits 0"""
    m = np.ascontiguousarray(mask, dtype=bool).reshape(-1)
    b = np.packbits(m, bitorder="little")
    out = np.zeros(4 * ((m.size + 31) // 32), dtype=np.uint8)
    out[:b.size] = b
    return out.view("<u4").astype(np.uint32)


def unpack(words, dims):
    n = int(np.prod(dims))
    b = np.ascontiguousarray(words, dtype=np.uint32).astype("<u4").view(np.uint8)
    bits = np.unpackbits(b, bitorder="little")
    assert not bits[n:].any(), "a bit beyond the last voxel is set"
    return bits[:n].astype(bool).reshape(tuple(int(v) for v in dims))


def shift(mask, s):
    """K'[v] = K[v + s] where v + s lies in the grid, else 0"""
    out = np.zeros_like(mask)
    src, dst = [], []
    for d, sa in zip(mask.shape, s):
        sa = int(sa)
        if abs(sa) >= d:
            return out
        dst.append(slice(max(0, -sa), min(d, d - sa)))
        src.append(slice(max(0, sa), min(d, d + sa)))
    out[tuple(dst)] = mask[tuple(src)]
    return out


def fill(mask, box, value):
    out = mask.copy()
    if box is None:
        out[...] = bool(value)
    else:
        out[box[0]:box[3] + 1, box[1]:box[4] + 1, box[2]:box[5] + 1] = bool(value)
    return out


def merge(mask, free, hits):
    return mask | (np.asarray(free) != 0) | (np.asarray(hits) > 0)


def frontier(mask, occ):
    """K = 1, occupancy byte 0, some 6-neighbour inside the grid with K = 0"""
    unknown = ~mask
    nb = np.zeros_like(mask)
    for axis in range(3):
        for step in (1, -1):
            moved = np.zeros_like(mask)             # moved[v] = unknown[v + step e_axis], False outside the grid
            a, b = [slice(None)] * 3, [slice(None)] * 3
            if step == 1:
                a[axis], b[axis] = slice(0, -1), slice(1, None)
            else:
                a[axis], b[axis] = slice(1, None), slice(0, -1)
            moved[tuple(a)] = unknown[tuple(b)]
            nb |= moved
    return mask & (np.asarray(occ) == 0) & nb


def box_of(mask):
    """(lo, hi) of the set voxels; ([0, 0, 0], [-1, -1, -1]) for none"""
    idx = np.argwhere(mask)
    if len(idx) == 0:
        return [0, 0, 0], [-1, -1, -1]
    return idx.min(axis=0).tolist(), idx.max(axis=0).tolist()
