"""The known grid on the device (csrc/map_known.hip: isdf_map_known_enable / _fill / _get, isdf_map_frontier, the merge inside
isdf_integrate_scan / isdf_integrate_depth and the translation inside isdf_shift_map) against the plain host forms, which
tests/test_map_known_host.py holds to the NumPy restatement (tests/known_reference.py).  Every comparison of grids, lists and integer
info words is == on bytes.  Grids, shifts, boxes and frontier cases are the host tests'; the scan scene is tests/test_gpu_map_scan.py's,
the corridor loop tests/test_gpu_depth_cam.py's."""
import ctypes as C

import numpy as np
import pytest

import known_reference as kr
import test_gpu_depth_cam as dc
import test_gpu_map_scan as ms
import test_gpu_map_update as mu
from test_map_known_host import GRIDS, IDS, bad_boxes, fill_boxes, shifts_of

pytestmark = pytest.mark.gpu
RES = 0.5


def _grid_engine(pkg, dims, seed=3):
    """a map of exactly dims voxels from a cloud: two points in every occupied voxel (sta_threshold 2), one in voxel 0"""
    rng = np.random.default_rng(seed)
    occ = rng.uniform(size=dims) < 0.2
    occ[0, 0, 0] = False
    cells = np.concatenate([np.repeat(np.argwhere(occ), 2, axis=0), [[0, 0, 0]]])
    cloud = ((cells + 0.5) * RES).astype(np.float32)
    eng = pkg.Engine(pkg.synth.default_config(pkg.capi.V1_SWEPT))
    assert eng.set_pointcloud(cloud, RES, 2, np.zeros(3), np.array(dims) * RES) == tuple(dims)
    assert np.array_equal(eng.get_grid(pkg.capi.GRID_OCCUPANCY)[0] != 0, occ)
    return eng, cloud


def _random_fills(dims, seed=11, n=24):
    """a K with structure at every alignment: boxes set and cleared in turn"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        lo = [int(rng.integers(0, d)) for d in dims]
        hi = [int(rng.integers(l, min(d, l + max(2, d // 2)))) for l, d in zip(lo, dims)]
        out.append((tuple(lo + hi), 0 if i % 3 == 2 else 1))
    return out


def _apply(pkg, lib, eng, k, fills):
    """the fills on the device and on the restatement; after each the grid, newly_known and the info equal the host form's"""
    dims = k.shape
    for box, value in fills:
        eng.map_known_fill(box, value)
        want, newly = pkg.engine.known_fill_host(kr.pack(k), dims, box, value, lib=lib)
        k = kr.fill(k, box, value)
        assert np.array_equal(want, kr.pack(k))
        _same_known(eng, k, newly=newly)
    return k


def _same_known(eng, k, newly=None, merges=None):
    bits, info = eng.map_known()
    assert bits.dtype == np.uint32 and np.array_equal(bits, kr.pack(k))
    lo, hi = kr.box_of(k)
    assert (info.n_known, info.n_unknown, list(info.lo), list(info.hi)) == (int(k.sum()), int(k.size - k.sum()), lo, hi)
    if newly is not None:
        assert info.newly_known == newly
    if merges is not None:
        assert info.merges == merges
    return info


def _same_frontier(pkg, lib, eng, k):
    occ = eng.get_grid(pkg.capi.GRID_OCCUPANCY)[0]
    bits, vox, info = eng.map_frontier()
    hbits, hvox, hinfo = pkg.engine.known_frontier_host(kr.pack(k), occ, lib=lib)
    want = kr.frontier(k, occ)
    assert np.array_equal(hbits, kr.pack(want))
    assert np.array_equal(bits, hbits) and vox.dtype == np.int64 and np.array_equal(vox, hvox)
    assert (info.n_frontier, list(info.lo), list(info.hi)) == (hinfo.n_frontier, list(hinfo.lo), list(hinfo.hi)) and info.kernel_ms >= 0.0
    bits2, none, info2 = eng.map_frontier(want_list=False)
    assert none is None and np.array_equal(bits2, bits) and info2.n_frontier == info.n_frontier
    return int(info.n_frontier)


@pytest.mark.parametrize("dims", GRIDS, ids=IDS)
def test_fill_get_and_frontier_equal_the_host_form(pkg, product_lib, dims):
    eng, _ = _grid_engine(pkg, dims)
    with pytest.raises(pkg.engine.IsdfError) as e:
        eng.map_known()
    assert e.value.code == pkg.capi.ISDF_ERR_STATE
    with pytest.raises(pkg.engine.IsdfError) as e:
        eng.map_frontier()
    assert e.value.code == pkg.capi.ISDF_ERR_STATE
    eng.map_known_enable(True)
    k = np.zeros(dims, dtype=bool)
    _same_known(eng, k, newly=0, merges=0)
    assert _same_frontier(pkg, product_lib, eng, k) == 0        # all unknown
    for box in fill_boxes(dims):
        for value in (1, 0):
            k = _apply(pkg, product_lib, eng, k, [(box, value)])
    for box in bad_boxes(dims):
        with pytest.raises(pkg.engine.IsdfError) as e:
            eng.map_known_fill(box, 1)
        assert e.value.code == pkg.capi.ISDF_ERR_INVALID_ARG
    _same_known(eng, k)                                         # nothing changed
    k = _apply(pkg, product_lib, eng, k, [(None, 1)])
    assert _same_frontier(pkg, product_lib, eng, k) == 0        # all known
    nx, ny, nz = dims
    cases = {"block": [(None, 0), ((1, 1, 1, nx - 2, ny - 2, nz - 2), 1)],
             "faces": [(None, 0), ((0, 0, 0, max(nx - 3, 0), max(ny - 2, 0), max(nz - 3, 0)), 1)],
             "hole": [(None, 1), ((nx // 2, ny // 2, nz // 2) * 2, 0)],
             "random": [(None, 0)] + _random_fills(dims)}
    for name, fills in cases.items():
        k = _apply(pkg, product_lib, eng, k, fills)
        n = _same_frontier(pkg, product_lib, eng, k)
        assert n > 0, name
    # a short list: ISDF_ERR_OVERFLOW, the info filled, the list untouched
    vox = np.full(max(n - 1, 1), -7, dtype=np.int64)
    info = pkg.capi.IsdfMapFrontierInfo()
    rc = product_lib.isdf_map_frontier(eng.h, None, vox.ctypes.data_as(C.c_void_p), n - 1, C.byref(info))
    assert rc == pkg.capi.ISDF_ERR_OVERFLOW and (vox == -7).all() and info.n_frontier == n


@pytest.mark.parametrize("path", [1, 2], ids=["incremental", "full"])
@pytest.mark.parametrize("dims", GRIDS, ids=IDS)
def test_shift_equals_the_host_form(pkg, product_lib, dims, path):
    eng, _ = _grid_engine(pkg, dims)
    eng.map_known_enable(True)
    fills = _random_fills(dims)
    k = np.zeros(dims, dtype=bool)
    for s in shifts_of(dims):
        if not k.any():
            k = _apply(pkg, product_lib, eng, k, [(None, 0)] + fills)
        info = eng.shift_map(s, force_path=path)
        assert info.path == (0 if s == (0, 0, 0) else (2 if any(abs(a) >= d for a, d in zip(s, dims)) else path))
        want = pkg.engine.known_shift_host(kr.pack(k), dims, s, lib=product_lib)
        k = kr.shift(k, s)
        assert np.array_equal(want, kr.pack(k)), s
        _same_known(eng, k)
        _same_frontier(pkg, product_lib, eng, k)


def _scan_engines(pkg):
    old = ms._scene()[0]
    a, b = mu._engine(pkg, old), mu._engine(pkg, old)
    a.map_known_enable(True)                                    # a map with kept counts exists: allocated now, all unknown
    return a, b


def test_the_scan_merges_and_changes_nothing_else(pkg, product_lib):
    _, ends, hit = ms._scene()
    free, hits, _ = ms._sets(pkg, product_lib, ends, hit)
    a, b = _scan_engines(pkg)
    k = np.zeros(ms.DIMS, dtype=bool)
    _same_known(a, k, newly=0, merges=0)
    ia, ib = a.integrate_scan(ms.ORIGIN, ends, hit, miss_weight=ms.MISS), b.integrate_scan(ms.ORIGIN, ends, hit, miss_weight=ms.MISS)
    want, newly = pkg.engine.known_merge_host(kr.pack(k), ms.DIMS, free, hits, lib=product_lib)
    k = kr.merge(k, free, hits)
    assert np.array_equal(want, kr.pack(k)) and newly == int(k.sum()) > 1000
    _same_known(a, k, newly=newly, merges=1)
    assert ms._fields(ia) == ms._fields(ib)                     # the scan's info but the times
    mu._same(mu._products(pkg, a), mu._products(pkg, b))        # counts, occupancy, ESDF, bit map, table: as with the mode off
    ia, ib = a.integrate_scan(ms.ORIGIN, ends, hit, miss_weight=ms.MISS), b.integrate_scan(ms.ORIGIN, ends, hit, miss_weight=ms.MISS)
    _same_known(a, k, newly=0, merges=2)                        # a second identical scan: nothing new
    assert ms._fields(ia) == ms._fields(ib)
    a.map_known_fill(None, 0)
    a.integrate_scan(ms.ORIGIN, ends, hit, miss_weight=0)       # miss_weight 0 still merges
    b.integrate_scan(ms.ORIGIN, ends, hit, miss_weight=0)
    _same_known(a, k, newly=int(k.sum()), merges=3)
    a.map_known_fill((0, 0, 0, 3, 3, 3), 0)
    k = kr.fill(k, (0, 0, 0, 3, 3, 3), 0)
    a.integrate_scan(ms.ORIGIN, np.zeros((0, 3), dtype=np.float32), np.zeros(0, dtype=np.uint8))       # n_rays 0 merges nothing
    b.integrate_scan(ms.ORIGIN, np.zeros((0, 3), dtype=np.float32), np.zeros(0, dtype=np.uint8))
    _same_known(a, k, newly=0, merges=3)
    with pytest.raises(pkg.engine.IsdfError):                   # refused before anything moves: K stays
        a.integrate_scan(np.array(ms.BMAX) + 5.0, ends, hit)
    _same_known(a, k, merges=3)
    mu._same(mu._products(pkg, a), mu._products(pkg, b))
    _same_frontier(pkg, product_lib, a, k)


def test_the_depth_loop_keeps_the_known_grid(pkg, product_lib):
    truth = dc._corridor()
    old = ms._scene()[0]
    a = mu._engine(pkg, old, esdf=False, frontend=False)
    a.map_known_enable(True)
    cam = dc._cam(pkg, dc.WIDE)
    params = {"max_range_m": 9.0, "no_return_is_free": True, "min_range_m": 0.3}
    k = np.zeros(ms.DIMS, dtype=bool)
    moved = False
    for step, z in enumerate((14.0, 17.0, 20.5)):
        p12 = dc.ref.pose(dc.ref.rot(0.05, 0.1, -0.2), [5.2, 7.1, z])
        origin = p12.reshape(3, 4)[:, 3]
        image, _ = a.depth_render(cam, p12, truth, splat_m=0.15)
        _, bmin, bmax = a.get_grid(pkg.capi.GRID_OCCUPANCY)
        a.integrate_depth(cam, p12, image, **params)
        ends, hit, _ = dc._host_rays(pkg, product_lib, image, p12=p12, bmin=bmin, bmax=bmax, **params)
        free, hits, _ = pkg.engine.scan_sets_host(bmin, bmax, ms.RES, ms.DIMS, origin, ends, hit, lib=product_lib)
        want, newly = pkg.engine.known_merge_host(kr.pack(k), ms.DIMS, free, hits, lib=product_lib)
        k = kr.merge(k, free, hits)
        assert np.array_equal(want, kr.pack(k))
        _same_known(a, k, newly=newly, merges=step + 1)
        s, _ = a.map_follow(origin)
        moved = moved or s != (0, 0, 0)
        want = pkg.engine.known_shift_host(kr.pack(k), ms.DIMS, s, lib=product_lib)
        k = kr.shift(k, s)
        assert np.array_equal(want, kr.pack(k))
        _same_known(a, k, merges=step + 1)
    assert moved and 0 < k.sum() < k.size
    assert _same_frontier(pkg, product_lib, a, k) > 0


def test_a_new_map_resets_and_the_callers_assertions_leave_alone(pkg, product_lib):
    old = ms._scene()[0]
    eng = mu._engine(pkg, old, esdf=False, frontend=False)
    eng.map_known_enable(True)
    box = (2, 3, 4, 9, 9, 40)
    k = kr.fill(np.zeros(ms.DIMS, dtype=bool), box, 1)
    eng.map_known_fill(box, 1)
    extra = ms._centres([[5, 5, 5], [5, 5, 5], [6, 5, 5], [6, 5, 5]])
    eng.update_pointcloud(extra)
    _same_known(eng, k)                                         # an assertion about occupancy is not an observation
    eng.clear_pointcloud(np.repeat(extra, 2, axis=0))
    _same_known(eng, k)
    eng.map_known_enable(True)                                  # a second enable: the grid stays
    _same_known(eng, k)
    eng.map_known_enable(False)
    with pytest.raises(pkg.engine.IsdfError) as e:
        eng.map_known_fill(box, 1)
    assert e.value.code == pkg.capi.ISDF_ERR_STATE
    eng.map_known_enable(True)
    _same_known(eng, np.zeros(ms.DIMS, dtype=bool), newly=0, merges=0)
    eng.map_known_fill(box, 1)
    assert eng.set_pointcloud(old, ms.RES, ms.THR, ms.BMIN, ms.BMAX) == ms.DIMS          # the mode outlives the map; the grid does not
    _same_known(eng, np.zeros(ms.DIMS, dtype=bool), newly=0, merges=0)
    small, _ = _grid_engine(pkg, GRIDS[0])
    small.map_known_enable(True)
    small.map_known_fill(None, 1)
    assert small.set_pointcloud(old, ms.RES, ms.THR, ms.BMIN, ms.BMAX) == ms.DIMS        # ... at the new size
    _same_known(small, np.zeros(ms.DIMS, dtype=bool))


def test_a_second_call_of_a_size_allocates_nothing(pkg, product_lib):
    old, ends, hit = ms._scene()
    eng = mu._engine(pkg, old, esdf=False, frontend=False)
    eng.map_known_enable(True)

    def round_():
        """the same K and the same occupancy at every call of every round: no ray ends on a surface and miss_weight is 0"""
        eng.map_known_fill(None, 0)
        eng.map_known_fill((1, 1, 1, 5, 5, 5), 1)
        eng.integrate_scan(ms.ORIGIN, ends, np.zeros_like(hit), miss_weight=0)
        eng.map_known()
        eng.map_frontier()
        eng.shift_map((1, 0, -2))
        eng.shift_map((-1, 0, 2))
        eng.map_frontier(want_list=False)
    round_()
    live = mu._live(product_lib)
    round_()
    assert mu._live(product_lib) == live
    eng.map_known_enable(False)
    assert mu._live(product_lib)[0] < live[0]


# ---- the known horizon of a trajectory: against the field query at the centres of ALL unknown voxels, reduced in NumPy
from test_gpu_map_clear import CM, MARGIN, N, T, _bits

HALF = (0, 0, 0, ms.DIMS[0] - 1, ms.DIMS[1] - 1, 34)            # known: the first half of the straight path (z from voxel 9 to 60)
INT_WORDS = ("qualified", "n_below_margin", "n_penetrating", "horizon_voxel", "horizon_piece", "min_voxel")


def _horizon_reference(pkg, eng, mode):
    """isdf_swept_sdf at (i + 0.5) * res + origin of every unknown voxel, filtered and reduced by the stated rules"""
    k = kr.unpack(eng.map_known()[0], ms.DIMS)
    _, bmin, _ = eng.get_grid(pkg.capi.GRID_OCCUPANCY)
    cells = np.argwhere(~k)
    vox = np.flatnonzero(~k.reshape(-1))                        # ascending, the order of `cells`
    want = {"qualified": 0, "n_below_margin": 0, "n_penetrating": 0, "horizon_t": -1.0, "horizon_voxel": -1, "horizon_value": 10.0,
            "horizon_piece": -1, "min_clearance": 10.0, "min_voxel": -1, "duration": float(np.sum(T)), "margin": MARGIN}
    if len(cells) == 0:
        return want
    assert len(cells) <= 33600
    centres = (cells + 0.5) * ms.RES + np.asarray(bmin)
    val, ts = eng.swept_sdf(T, CM, centres, mode=mode)
    q = val != 10.0
    below = q & (val < MARGIN)
    want.update(qualified=int(q.sum()), n_below_margin=int(below.sum()), n_penetrating=int((q & (val < 0.0)).sum()))
    if q.any():
        j = np.flatnonzero(q)[np.lexsort((vox[q], val[q]))[0]]
        want.update(min_clearance=float(val[j]), min_voxel=int(vox[j]))
    if below.any():
        j = np.flatnonzero(below)[np.lexsort((vox[below], ts[below]))[0]]
        t, piece = float(ts[j]), 0
        while piece < N and t > T[piece]:                       # locate_piece's rule
            t -= T[piece]
            piece += 1
        want.update(horizon_t=float(ts[j]), horizon_voxel=int(vox[j]), horizon_value=float(val[j]), horizon_piece=min(piece, N - 1))
        want["horizon_point"] = centres[j]
    return want


def _same_horizon(got, want):
    for key, v in want.items():
        if key in INT_WORDS:
            assert got[key] == v, (key, got[key], v)
        else:
            assert np.array_equal(_bits(got[key]), _bits(v)), (key, got[key], v)
    assert got["unknown_in_box"] >= got["candidates"] >= got["qualified"]


def _horizon_engine(pkg):
    eng = mu._engine(pkg, ms._scene()[0])
    eng.map_known_enable(True)
    return eng


@pytest.mark.parametrize("mode", ["PLANNER", "CLOSED"])
def test_horizon_equals_the_field_query_over_all_unknown_voxels(pkg, product_lib, mode):
    mode = getattr(pkg.capi, "SWEPT_FIELD_" + mode)
    eng = _horizon_engine(pkg)
    got = eng.traj_known_horizon(T, CM, margin=MARGIN, mode=mode)            # all unknown
    want = _horizon_reference(pkg, eng, mode)
    _same_horizon(got, want)
    assert got["n_below_margin"] > 50 and got["horizon_piece"] == 0 and got["horizon_t"] >= 0.0
    eng.map_known_fill(None, 1)                                 # all known
    got = eng.traj_known_horizon(T, CM, margin=MARGIN, mode=mode)
    _same_horizon(got, _horizon_reference(pkg, eng, mode))
    assert got["horizon_t"] == -1.0 and got["candidates"] == 0 and got["unknown_in_box"] == 0 and got["horizon_voxel"] == -1
    eng.map_known_fill(None, 0)
    eng.map_known_fill(HALF, 1)                                 # known around the first half of the path
    want = _horizon_reference(pkg, eng, mode)
    assert want["n_below_margin"] >= 50 and want["horizon_piece"] not in (0, N - 1)      # the case's condition, by the reference alone
    got = eng.traj_known_horizon(T, CM, margin=MARGIN, mode=mode)
    _same_horizon(got, want)
    again = eng.traj_known_horizon(T, CM, margin=MARGIN, mode=mode)            # two runs, the same bytes
    assert all(np.array_equal(_bits(again[k]), _bits(got[k])) for k in got if not k.endswith('_ms') and not isinstance(got[k], int))
    eng.shift_map((2, -3, 5))                                   # ... and again in the shifted window
    want2 = _horizon_reference(pkg, eng, mode)
    got2 = eng.traj_known_horizon(T, CM, margin=MARGIN, mode=mode)
    _same_horizon(got2, want2)
    assert got2["n_below_margin"] > 0 and got2["horizon_voxel"] != got["horizon_voxel"]


def test_horizon_device_form_on_a_side_stream(pkg, product_lib):
    import torch
    eng = _horizon_engine(pkg)
    eng.map_known_fill(HALF, 1)
    host = eng.traj_known_horizon(T, CM, margin=MARGIN)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        dT = torch.tensor(T, dtype=torch.float64, device="cuda")
        dC = torch.tensor(np.ascontiguousarray(CM).reshape(-1), dtype=torch.float64, device="cuda")
    side.synchronize()
    dev = eng.traj_known_horizon_device(N, dT.data_ptr(), dC.data_ptr(), margin=MARGIN, stream=side.cuda_stream)
    for key, v in host.items():
        if not key.endswith("_ms"):
            assert np.array_equal(_bits(dev[key]), _bits(v)) if not isinstance(v, int) else dev[key] == v, key
    assert host["horizon_t"] > 0.0


def test_horizon_leaves_the_kept_report_and_the_watch_alone(pkg, product_lib):
    eng = _horizon_engine(pkg)
    eng.map_known_fill(HALF, 1)
    eng.traj_check_set_watch(1)
    rep = eng.traj_check(T, CM, margin=MARGIN)
    rows = eng.traj_check_points()
    watch, last = eng.traj_check_watch_info()
    eng.traj_known_horizon(T, CM, margin=MARGIN)
    eng.traj_known_horizon(T, CM, margin=0.5, mode=pkg.capi.SWEPT_FIELD_CLOSED)
    assert eng.traj_check_points().tobytes() == rows.tobytes()
    watch2, last2 = eng.traj_check_watch_info()
    ms._same_report(watch2, watch, "watch")
    assert last2 == last
    extra = ms._centres([[5, 5, 5], [5, 5, 5]])                 # the watch is still armed: an update folds
    eng.update_pointcloud(extra)
    assert eng.traj_check_watch_info()[1]["updates_folded"] == last["updates_folded"] + 1
    ms._same_report(watch, rep, "report")


def test_horizon_status_codes(pkg, product_lib):
    eng = mu._engine(pkg, ms._scene()[0])
    with pytest.raises(pkg.engine.IsdfError) as e:
        eng.traj_known_horizon(T, CM, margin=MARGIN)
    assert e.value.code == pkg.capi.ISDF_ERR_STATE              # no known grid
    eng.map_known_enable(True)
    with pytest.raises(pkg.engine.IsdfError) as e:
        eng.traj_known_horizon(T, CM, margin=50.0)
    assert e.value.code == pkg.capi.ISDF_ERR_INVALID_ARG        # the check's rule for the margin
