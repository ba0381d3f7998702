"""The frontier clusters on the device (csrc/frontier_cluster.hip: isdf_map_frontier_clusters) against the plain host form
isdf_known_clusters_host, which tests/test_frontier_cluster_host.py holds to the restatement of the definition
(tests/frontier_cluster_reference.py).  Every comparison of lists, labels, rows and integer info words is == on bytes; the only
floating-point values are the three times.  Grids, random sets, the plane and the serpentine are the host tests'; the ctx is
tests/test_gpu_map_known.py's."""
import ctypes as C

import numpy as np
import pytest

import known_reference as kr
import test_frontier_cluster_host as fh
import test_gpu_map_scan as ms
import test_gpu_map_update as mu
from test_gpu_map_known import RES, _grid_engine, _random_fills
from test_map_known_host import GRIDS, IDS

pytestmark = pytest.mark.gpu
INFO = fh.INFO


def _same(got, want, what=""):
    for a, b, name in zip(got[:3], want[:3], ("vox", "labels", "rows")):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), (what, name)
    assert {k: getattr(got[3], k) for k in INFO} == {k: getattr(want[3], k) for k in INFO}, what
    assert all(getattr(got[3], k) >= 0.0 for k in ("frontier_ms", "label_ms", "stats_ms"))


def _frontier_mask(pkg, lib, eng):
    """the frontier of the ctx's K and occupancy by the host form (held to the restatement by tests/test_map_known_host.py)"""
    occ = eng.get_grid(pkg.capi.GRID_OCCUPANCY)[0]
    bits, vox, _ = pkg.engine.known_frontier_host(eng.map_known()[0], occ, lib=lib)
    return kr.unpack(bits, occ.shape), vox


def _same_frontier_clusters(pkg, lib, eng, cases=((6, 1), (18, 1), (26, 1), (26, 3))):
    front, hvox = _frontier_mask(pkg, lib, eng)
    list_ = eng.map_frontier()[1]
    assert np.array_equal(list_, hvox)
    out = None
    for conn, min_size in cases:
        got = eng.map_frontier_clusters(connectivity=conn, min_size=min_size)
        _same(got, fh.host(pkg, lib, front, conn, min_size), (conn, min_size))
        assert np.array_equal(got[0], list_)                    # the call's list is isdf_map_frontier's
        out = got
    return out


@pytest.mark.parametrize("dims", GRIDS, ids=IDS)
def test_frontier_mode_equals_the_host_form(pkg, product_lib, dims):
    eng, _ = _grid_engine(pkg, dims)
    with pytest.raises(pkg.engine.IsdfError) as e:              # mode off
        eng.map_frontier_clusters()
    assert e.value.code == pkg.capi.ISDF_ERR_STATE
    eng.map_known_enable(True)
    vox, labels, rows, info = _same_frontier_clusters(pkg, product_lib, eng)          # all unknown
    assert len(vox) == 0 and rows.shape == (0, 16) and (info.n_clusters, info.largest_label) == (0, -1)
    for box, value in _random_fills(dims):
        eng.map_known_fill(box, value)
    vox, labels, rows, info = _same_frontier_clusters(pkg, product_lib, eng)
    assert info.n_voxels > 0 and info.n_clusters >= 1
    eng.shift_map((2, -3, 5))
    _same_frontier_clusters(pkg, product_lib, eng)
    eng.map_known_fill(None, 1)                                 # all known
    assert _same_frontier_clusters(pkg, product_lib, eng)[3].n_voxels == 0


def _empty_engine(pkg, dims):
    """_grid_engine's map without an occupied voxel: one point in voxel 0, below the threshold of two"""
    eng = pkg.Engine(pkg.synth.default_config(pkg.capi.V1_SWEPT))
    assert eng.set_pointcloud(np.full((1, 3), 0.5 * RES, dtype=np.float32), RES, 2, np.zeros(3), np.array(dims) * RES) == tuple(dims)
    assert not eng.get_grid(pkg.capi.GRID_OCCUPANCY)[0].any()
    eng.map_known_enable(True)
    return eng


def _boxes_of(mask):
    """a mask made of z columns and single voxels as box fills: one box per run along z"""
    out = []
    for x, y in np.argwhere(mask.any(axis=2)):
        z = np.flatnonzero(mask[x, y])
        for run in np.split(z, np.flatnonzero(np.diff(z) > 1) + 1):
            out.append((int(x), int(y), int(run[0]), int(x), int(y), int(run[-1])))
    return out


def test_the_plane_and_the_serpentine_from_box_fills(pkg, product_lib):
    dims = GRIDS[2]
    eng = _empty_engine(pkg, dims)
    eng.map_known_fill((0, 0, 37, dims[0] - 1, dims[1] - 1, 37), 1)         # one known slab in unknown space: every voxel of it is frontier
    assert np.array_equal(_frontier_mask(pkg, product_lib, eng)[0], fh.plane(dims, 37))
    for conn in fh.CONNS:                                       # every lane of the statistics kernel hits one row
        vox, labels, rows, info = _same_frontier_clusters(pkg, product_lib, eng, ((conn, 1),))
        assert info.n_clusters == 1 and rows[0, 1] == 480 and (labels == 0).all()
    eng.map_known_fill(None, 0)
    snake = fh.serpentine(dims)
    for box in _boxes_of(snake):
        eng.map_known_fill(box, 1)
    assert np.array_equal(_frontier_mask(pkg, product_lib, eng)[0], snake)   # one voxel wide: all of it is frontier
    for conn in fh.CONNS:                                       # the longest parent chains; one component already at 6
        vox, labels, rows, info = _same_frontier_clusters(pkg, product_lib, eng, ((conn, 1),))
        assert info.n_clusters == 1 and rows[0, 0] == 0 and rows[0, 1] == snake.sum() and info.largest_size == snake.sum()


@pytest.mark.parametrize("density", fh.DENSITIES)
@pytest.mark.parametrize("dims", GRIDS, ids=IDS)
def test_bits_in_mode_equals_the_host_form(pkg, product_lib, dims, density):
    eng, _ = _grid_engine(pkg, dims)
    eng.map_known_enable(True)
    mask = fh.random_set(tuple(dims), density)
    for conn in fh.CONNS:
        for min_size in (1, 2):
            got = eng.map_frontier_clusters(kr.pack(mask), conn, min_size)
            _same(got, fh.host(pkg, product_lib, mask, conn, min_size), (conn, min_size))
    assert got[3].n_voxels == mask.sum() > 0


def _raw(pkg, eng, words=None, conn=26, min_size=1, nv=0, nr=0, vox=None, labels=None, rows=None):
    p = pkg.capi.IsdfFrontierClusterParams(conn, 0, min_size)
    info = pkg.capi.IsdfFrontierClusterInfo()
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = eng.lib.isdf_map_frontier_clusters(eng.h, ptr(words), C.byref(p), ptr(vox), ptr(labels), nv, ptr(rows), nr, C.byref(info))
    return rc, info


def test_sizing_overflow_and_what_the_call_leaves_alone(pkg, product_lib):
    from test_gpu_map_clear import CM, MARGIN, T
    capi = pkg.capi
    old, ends, hit = ms._scene()
    eng = mu._engine(pkg, old)
    eng.map_known_enable(True)
    eng.integrate_scan(ms.ORIGIN, ends, hit, miss_weight=ms.MISS)
    rep = eng.traj_check(T, CM, margin=MARGIN)
    kept = eng.traj_check_points().tobytes()
    k0, kinfo0 = eng.map_known()
    occ0 = eng.get_grid(capi.GRID_OCCUPANCY)[0].copy()
    bits0, list0, finfo0 = eng.map_frontier()
    front = kr.unpack(bits0, ms.DIMS)
    want = fh.host(pkg, product_lib, front, 6, 2)
    n, r = int(want[3].n_voxels), int(want[3].n_rows)
    assert kinfo0.merges == 1 and n > 100 and r >= 2
    rc, info = _raw(pkg, eng, conn=6, min_size=2)               # the sizing call
    assert rc == 0 and {k: getattr(info, k) for k in INFO} == {k: getattr(want[3], k) for k in INFO}

    def fresh():
        return np.full(n, -7, dtype=np.int64), np.full(n, -7, dtype=np.int32), np.full((r, 16), -7, dtype=np.int64)
    for nv, nr, use in ((n - 1, r, "vlr"), (n, r - 1, "vlr"), (n - 1, r, "l"), (n, r - 1, "r"), (0, 0, "vlr")):
        vox, labels, rows = fresh()
        rc, info = _raw(pkg, eng, conn=6, min_size=2, nv=nv, nr=nr, vox=vox if "v" in use else None, labels=labels if "l" in use else None,
                        rows=rows if "r" in use else None)
        assert rc == capi.ISDF_ERR_OVERFLOW, (nv, nr, use)
        assert {k: getattr(info, k) for k in INFO} == {k: getattr(want[3], k) for k in INFO}      # the info is filled
        assert (vox == -7).all() and (labels == -7).all() and (rows == -7).all()                   # every output untouched
    vox, labels, rows = fresh()                                 # exactly the sizes the sizing call reported
    rc, info = _raw(pkg, eng, conn=6, min_size=2, nv=n, nr=r, vox=vox, labels=labels, rows=rows)
    assert rc == 0
    _same((vox, labels, rows, info), want)
    assert _raw(pkg, eng, conn=5)[0] == capi.ISDF_ERR_INVALID_ARG and _raw(pkg, eng, min_size=0)[0] == capi.ISDF_ERR_INVALID_ARG
    assert _raw(pkg, eng, nv=-1)[0] == capi.ISDF_ERR_INVALID_ARG and _raw(pkg, eng, nr=-1)[0] == capi.ISDF_ERR_INVALID_ARG
    # two calls give the same bytes; a second call of a size allocates nothing
    a = eng.map_frontier_clusters(connectivity=6, min_size=2)
    eng.map_frontier_clusters(kr.pack(front), 26, 1)
    live = mu._live(product_lib)
    b = eng.map_frontier_clusters(connectivity=6, min_size=2)
    eng.map_frontier_clusters(kr.pack(front), 26, 1)
    assert mu._live(product_lib) == live
    _same(a, want)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3]))
    # read-only: K, the occupancy, merges, the kept report; isdf_map_frontier returns what it returned before
    k1, kinfo1 = eng.map_known()
    assert np.array_equal(k1, k0) and (kinfo1.merges, kinfo1.newly_known, kinfo1.n_known) == (kinfo0.merges, kinfo0.newly_known, kinfo0.n_known)
    assert np.array_equal(eng.get_grid(capi.GRID_OCCUPANCY)[0], occ0)
    assert eng.traj_check_points().tobytes() == kept
    bits1, list1, finfo1 = eng.map_frontier()
    assert np.array_equal(bits1, bits0) and np.array_equal(list1, list0) and finfo1.n_frontier == finfo0.n_frontier
    assert rep["n_below_margin"] >= 0


def test_status_codes(pkg, product_lib):
    capi = pkg.capi
    dims = GRIDS[0]
    eng = pkg.Engine(pkg.synth.default_config(capi.V1_SWEPT))
    eng.map_known_enable(True)
    eng.set_grid(np.ones(dims, dtype=np.float32), (0, 0, 0), RES, capi.GRID_ESDF)      # a map with a known grid and no occupancy grid
    with pytest.raises(pkg.engine.IsdfError) as e:
        eng.map_frontier()
    assert e.value.code == capi.ISDF_ERR_STATE
    with pytest.raises(pkg.engine.IsdfError) as e:
        eng.map_frontier_clusters()
    assert e.value.code == capi.ISDF_ERR_STATE
    mask = fh.random_set(tuple(dims), 0.5)                      # a caller's set needs no occupancy
    _same(eng.map_frontier_clusters(kr.pack(mask), 6), fh.host(pkg, product_lib, mask, 6))
    dirty = kr.pack(mask)                                       # 105 voxels: bits 9 .. 31 of the last word lie beyond the grid
    dirty[-1] |= np.uint32(1 << 9)
    assert _raw(pkg, eng, words=dirty)[0] == capi.ISDF_ERR_INVALID_ARG
    eng.map_known_enable(False)
    with pytest.raises(pkg.engine.IsdfError) as e:              # ... but the known grid's mode
        eng.map_frontier_clusters(kr.pack(mask), 6)
    assert e.value.code == capi.ISDF_ERR_STATE
    multi = pkg.Engine(pkg.synth.default_config(capi.V3_ESDF_TILE), devices=[0, 0])
    multi.set_grid(np.zeros(dims, dtype=np.uint8), (0, 0, 0), RES, capi.GRID_OCCUPANCY)
    with pytest.raises(pkg.engine.IsdfError) as e:
        multi.map_frontier_clusters()
    assert e.value.code == capi.ISDF_ERR_UNSUPPORTED
    with pytest.raises(pkg.engine.IsdfError) as e:
        multi.map_frontier_clusters(kr.pack(mask), 6)
    assert e.value.code == capi.ISDF_ERR_UNSUPPORTED
