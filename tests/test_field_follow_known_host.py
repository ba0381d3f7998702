"""The gated field's follow without a device: the new ABI's symbols, sizes and null-ctx status codes, and the direction
argument the follow rests on, checked with the NumPy erosion (tests/known_erode_reference.py) and the plain host forms of the field, its
repair and its reopen: a K that grows moves free' = free & E(K) in the opening direction only and only inside the changed box grown by
the radius, a K that shrinks in the closing direction only, and the host reopen / repair on the gated free set then give the bytes of the
host Dijkstra on it.  Grid: 13 x 11 x 9 voxels, a wall with a gap, 121 attitudes."""
import ctypes as C

import numpy as np
import pytest

import field_reference as fr
import known_erode_reference as er
import known_reference as kr

DIMS = (13, 11, 9)
GOAL = (10, 5, 2)
N_ATT = 121
SYMBOLS = ("isdf_frontend_field_set_known_follow", "isdf_frontend_field_follow_info", "isdf_frontend_field_follow_sizes")


def test_symbols_sizes_and_null_ctx(pkg, product_lib):
    capi = pkg.capi
    for name in SYMBOLS:
        assert hasattr(product_lib, name)
    sz = (C.c_int * 1)(-1)
    product_lib.isdf_frontend_field_follow_sizes(sz)
    assert sz[0] == C.sizeof(capi.IsdfFieldFollowInfo) == 88
    product_lib.isdf_frontend_field_follow_sizes(None)           # null-safe
    assert product_lib.isdf_frontend_field_set_known_follow(None, 1) == capi.ISDF_ERR_INVALID_ARG
    assert product_lib.isdf_frontend_field_follow_info(None, C.byref(capi.IsdfFieldFollowInfo())) == capi.ISDF_ERR_INVALID_ARG
    assert (capi.FIELD_KNOWN_FOLLOW_DROP, capi.FIELD_KNOWN_FOLLOW_FOLLOW) == (0, 1)


def _scene():
    free = np.ones(DIMS, dtype=bool)
    free[6, :, :] = False                       # a wall across x = 6 ...
    free[6, 4:7, 1:4] = True                    # ... with a gap
    k = kr.fill(np.zeros(DIMS, dtype=bool), (0, 0, 0, DIMS[0] - 1, DIMS[1] - 1, 5), 1)
    return free, k


def _grown(box, r):
    lo = [max(box[a] - r, 0) for a in range(3)]
    hi = [min(box[3 + a] + r, DIMS[a] - 1) for a in range(3)]
    m = np.zeros(DIMS, dtype=bool)
    m[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1] = True
    return m


@pytest.mark.parametrize("r,border", [(0, 0), (1, 0), (1, 1), (2, 1)])
def test_a_growing_k_opens_and_a_shrinking_k_closes_inside_the_grown_box(pkg, product_lib, r, border):
    free, k0 = _scene()
    assert free[GOAL]
    table = fr.table_from_free(free, N_ATT)
    gate = lambda k: table * er.erode(k, r, border)[..., None].astype(np.uint32)
    d0, reach0 = pkg.frontend_field_host(gate(k0), GOAL, N_ATT, lib=product_lib)
    assert reach0
    # K grows: opening only, inside the box grown by r; the host reopen from d0 has the bytes of the host build
    box = (2, 1, 6, 10, 9, 7)
    k1 = kr.fill(k0, box, 1)
    e0, e1 = er.erode(k0, r, border), er.erode(k1, r, border)
    assert not (e0 & ~e1).any() and (e1 & ~e0).any() and not ((e1 ^ e0) & ~_grown(box, r)).any()
    d1, reach1 = pkg.frontend_field_host(gate(k1), GOAL, N_ATT, lib=product_lib)
    assert not fr.same_bytes(d1, d0)
    got, _, info = pkg.frontend_field_reopen_host(gate(k1), GOAL, N_ATT, d0, lib=product_lib)
    assert fr.same_bytes(got, d1) and info.opened_voxels > 0
    # K shrinks: closing only, inside the grown box; the host repair from d1 has the bytes of the host build
    hole = (4, 3, 2, 8, 7, 4)
    k2 = kr.fill(k1, hole, 0)
    e2 = er.erode(k2, r, border)
    assert not (e2 & ~e1).any() and (e1 & ~e2).any() and not ((e1 ^ e2) & ~_grown(hole, r)).any()
    d2, _ = pkg.frontend_field_host(gate(k2), GOAL, N_ATT, lib=product_lib)
    assert not fr.same_bytes(d2, d1)
    got, _, info = pkg.frontend_field_repair_host(gate(k2), GOAL, N_ATT, d1, lib=product_lib)
    assert fr.same_bytes(got, d2) and info.closed_reached > 0
