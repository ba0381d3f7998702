"""Rays cast through the map on the device (csrc/map_raycast.hip: isdf_map_raycast / isdf_map_raycast_device) against the plain host
form (isdf_raycast_host, which tests/test_map_raycast_host.py holds to the definition) on the occupancy and the box read back with
isdf_get_grid - never against the device path itself.  Every comparison of rows is == on bytes.  Geometry of
tests/test_gpu_map_update.py: 24 x 20 x 70 voxels at 0.5 m; the world of the closed loop (sta_threshold 1, one point per occupied
voxel) and the named rays come from tests/test_map_raycast_host.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import test_block_sum_cases as bs
import test_gpu_map_update as mu
from test_gpu_map_clear import N, _same_report
from test_gpu_map_scan import _scene, _watched
from test_gpu_map_update import BMAX, BMIN, DIMS, RES, _products, _same
from test_map_raycast_host import BLOCK_ONLY_A, BLOCK_ONLY_B, FLAT, NAMED_ENDS, NAMED_ORIGINS, SENSOR, closed_loop_scene

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 63, 64, 65, 4097)


def _world(pkg, cloud=None):
    """a ctx holding the closed loop's world (or `cloud`) with sta_threshold 1 and no derived product"""
    eng = pkg.Engine(pkg.synth.default_config(pkg.capi.V1_SWEPT))
    assert eng.set_pointcloud(closed_loop_scene()[0] if cloud is None else cloud, RES, 1, BMIN, BMAX) == DIMS
    return eng


@functools.lru_cache(maxsize=None)
def _rays():
    """4 097 rays: the named rays first, then pairs of random points, the ends drawn a little beyond the box (some are skipped).
    The per-ray origins of the random pairs lie in the map; those of the named rays include three outside it."""
    rng = np.random.default_rng(3)
    n = SIZES[-1] - len(NAMED_ENDS)
    span = BMAX - BMIN
    origins = np.concatenate([NAMED_ORIGINS, rng.uniform(BMIN, BMAX, (n, 3))])
    ends = np.concatenate([NAMED_ENDS, rng.uniform(BMIN - 0.02 * span, BMAX + 0.02 * span, (n, 3)).astype(np.float32)])
    return origins, ends


def _host(pkg, lib, eng, origins, ends, test_origin=False):
    """the host form on what the ctx holds now: occupancy AND box"""
    occ, bmin, bmax = eng.get_grid(pkg.capi.GRID_OCCUPANCY)
    return pkg.engine.raycast_host(occ, bmin, bmax, RES, origins, ends, test_origin_voxel=test_origin, lib=lib)[0]


def _info_is_the_sum(info, rows):
    ok = rows[:, 0] < 2
    assert (info.n_rays, info.n_clear, info.n_hits, info.n_skipped, info.n_origin_outside, info.steps_total) == \
        (len(rows), (rows[:, 0] == 0).sum(), (rows[:, 0] == 1).sum(), (rows[:, 0] == 2).sum(), (rows[:, 0] == 3).sum(), rows[ok, 1].sum())
    assert info.cast_ms >= 0.0


# ---- 1. rows byte-equal to the host form
@pytest.mark.parametrize("test_origin", [False, True])
@pytest.mark.parametrize("per_ray", [False, True])
def test_rows_equal_the_host_form(pkg, product_lib, per_ray, test_origin):
    eng = _world(pkg)
    origins, ends = _rays()
    for n in SIZES:
        o = origins[:n] if per_ray else SENSOR
        want = _host(pkg, product_lib, eng, o, ends[:n], test_origin)
        rows, info = eng.map_raycast(o, ends[:n], test_origin_voxel=test_origin, per_ray_origin=per_ray)
        assert rows.shape == (n, 8) and rows.tobytes() == want.tobytes(), n
        _info_is_the_sum(info, rows)
    assert (want[:, 0] == 1).sum() > 500 and (want[:, 0] == 0).sum() > 500 and (want[:, 0] == 2).sum() > 50       # (the last, largest cast)
    assert ((want[:, 0] == 3).sum() == 3) == per_ray


def test_the_origin_voxel_is_tested_only_on_request(pkg, product_lib):
    cloud = closed_loop_scene()[0]
    eng = _world(pkg)
    inside = cloud[:200].astype(np.float64)                          # origins in occupied voxels
    ends = np.roll(cloud[:200], 1, axis=0)
    rows, info = eng.map_raycast(inside, ends, test_origin_voxel=True)
    assert (rows[:, :2] == [1, 0]).all() and (rows[:, 5:] == [-1, 0, 1]).all() and info.steps_total == 0
    rows, _ = eng.map_raycast(inside, ends)
    assert rows.tobytes() == _host(pkg, product_lib, eng, inside, ends).tobytes() and (rows[:, 1] > 0).sum() > 150


# ---- 2. the device-pointer form
@pytest.mark.parametrize("per_ray", [False, True])
def test_device_form_equals_the_host_pointer_form(pkg, product_lib, per_ray):
    import torch
    eng = _world(pkg)
    origins, ends = _rays()
    d_ends = torch.from_numpy(ends).cuda()
    o = torch.from_numpy(origins).cuda() if per_ray else SENSOR
    want, want_info = eng.map_raycast(origins if per_ray else SENSOR, ends)
    d_rows = torch.full((len(ends), 8), -7, dtype=torch.int32, device="cuda")
    info = eng.map_raycast_device(o, d_ends, d_rows)
    assert d_rows.cpu().numpy().tobytes() == want.tobytes()
    _info_is_the_sum(info, want)
    assert info.steps_total == want_info.steps_total
    # info_out = NULL: nothing handed over, no synchronisation - the test synchronises the stream
    d_rows.fill_(-7)
    assert eng.map_raycast_device(o, d_ends, d_rows, want_info=False) is None
    torch.cuda.current_stream().synchronize()
    assert d_rows.cpu().numpy().tobytes() == want.tobytes()
    d_none = torch.zeros((0, 8), dtype=torch.int32, device="cuda")
    info = eng.map_raycast_device(o[:0] if per_ray else o, d_ends[:0], d_none)
    assert (info.n_rays, info.n_hits, info.n_clear, info.steps_total) == (0, 0, 0, 0)


# ---- 3. other contexts and status codes
def test_other_contexts_and_status_codes(pkg, product_lib):
    capi = pkg.capi
    cloud, _, occ_a, _, _ = closed_loop_scene()
    origins, ends = _rays()
    want = pkg.engine.raycast_host(occ_a, BMIN, BMAX, RES, SENSOR, ends, lib=product_lib)[0]
    grid = pkg.Engine(pkg.synth.default_config(capi.V1_SWEPT))       # a map from isdf_set_grid: occupancy, no counts
    grid.set_grid(occ_a, BMIN, RES, capi.GRID_OCCUPANCY, bmax=BMAX)
    with pytest.raises(pkg.IsdfError) as err:
        grid.map_counts()
    assert err.value.code == capi.ISDF_ERR_STATE
    assert grid.map_raycast(SENSOR, ends)[0].tobytes() == want.tobytes()
    bare = pkg.Engine(pkg.synth.default_config(capi.V1_SWEPT))       # no map at all
    with pytest.raises(pkg.IsdfError) as err:
        bare.map_raycast(SENSOR, ends)
    assert err.value.code == capi.ISDF_ERR_STATE
    eng = _world(pkg)
    rows = np.full((len(ends), 8), -7, dtype=np.int32)
    fp, rp = ends.ctypes.data_as(C.POINTER(C.c_float)), rows.ctypes.data_as(C.c_void_p)
    dp = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
    for origin in (BMAX + [0.1, 0.0, 0.0], BMIN - [0.0, 1e-6, 0.0], [np.nan, 5.0, 5.0]):
        assert product_lib.isdf_map_raycast(eng.h, dp(origin), fp, len(ends), None, rp, None) == capi.ISDF_ERR_INVALID_ARG
    assert product_lib.isdf_map_raycast(eng.h, None, fp, 3, None, rp, None) == capi.ISDF_ERR_INVALID_ARG
    assert product_lib.isdf_map_raycast(eng.h, dp(SENSOR), None, 3, None, rp, None) == capi.ISDF_ERR_INVALID_ARG
    assert product_lib.isdf_map_raycast(eng.h, dp(SENSOR), fp, 3, None, None, None) == capi.ISDF_ERR_INVALID_ARG
    assert product_lib.isdf_map_raycast(eng.h, dp(SENSOR), fp, -1, None, rp, None) == capi.ISDF_ERR_INVALID_ARG
    assert (rows == -7).all()                                        # a refused call wrote nothing
    assert product_lib.isdf_map_raycast(eng.h, dp(SENSOR), None, 0, None, None, None) == capi.ISDF_OK          # n = 0; params and info_out may be NULL
    assert product_lib.isdf_map_raycast(eng.h, dp(SENSOR), fp, len(ends), None, rp, None) == capi.ISDF_OK and rows.tobytes() == want.tobytes()
    multi = pkg.Engine(pkg.synth.default_config(capi.V3_ESDF_TILE), devices=[0, 0])
    multi.set_pointcloud(cloud, RES, 1, BMIN, BMAX)
    with pytest.raises(pkg.IsdfError) as err:
        multi.map_raycast(SENSOR, ends)
    assert err.value.code == capi.ISDF_ERR_UNSUPPORTED


# ---- 4. the rows follow the map
def test_rows_follow_the_map(pkg, product_lib):
    cloud_a, cloud_b, occ_a, occ_b, _ = closed_loop_scene()
    origins, ends = _rays()
    ends = ends[:1500]
    eng = _world(pkg)
    seen = [eng.map_raycast(SENSOR, ends)[0]]
    assert seen[0].tobytes() == _host(pkg, product_lib, eng, SENSOR, ends).tobytes()
    only_b = cloud_b[occ_b[tuple(mu._bin(cloud_b)[0].T)] > occ_a[tuple(mu._bin(cloud_b)[0].T)]]
    only_a = cloud_a[occ_a[tuple(mu._bin(cloud_a)[0].T)] > occ_b[tuple(mu._bin(cloud_a)[0].T)]]
    assert len(only_a) == len(only_b) == 64
    steps = (lambda: eng.update_pointcloud(only_b, refresh_esdf=False, refresh_frontend=False),
             lambda: eng.clear_pointcloud(only_a, refresh_esdf=False, refresh_frontend=False),
             lambda: eng.shift_map((3, 0, -2)))
    for step in steps:
        step()
        rows, info = eng.map_raycast(SENSOR, ends)
        assert rows.tobytes() == _host(pkg, product_lib, eng, SENSOR, ends).tobytes()
        _info_is_the_sum(info, rows)
        assert rows.tobytes() != seen[-1].tobytes()                  # and the map did change what the rays see
        seen.append(rows)
    assert np.array_equal(eng.get_grid(pkg.capi.GRID_OCCUPANCY)[1], BMIN + np.array([3, 0, -2]) * RES)           # the new box


# ---- 5. the cast is read-only
def test_a_cast_changes_nothing(pkg, product_lib):
    origins, ends = _rays()
    eng, _ = _watched(pkg, _scene()[0], 1)                           # the scan tests' map: every product, a valid field, an armed watch, a kept report
    before = _products(pkg, eng)
    field, report_rows = eng.frontend_field(), eng.traj_check_points()
    rep_a, last_a = eng.traj_check_watch_info(N)
    for per_ray in (False, True):
        rows, _ = eng.map_raycast(origins if per_ray else SENSOR, ends, test_origin_voxel=per_ray)
        assert (rows[:, 0] == 1).sum() > 50
    _same(_products(pkg, eng), before)                               # counts, occupancy, ESDF, configuration space, bit map
    assert np.array_equal(eng.frontend_field().view(np.uint8), field.view(np.uint8))
    rep_b, last_b = eng.traj_check_watch_info(N)
    _same_report(rep_b, rep_a, "after the casts")
    assert last_b == last_a
    assert eng.traj_check_points().tobytes() == report_rows.tobytes()
    assert eng.points_merge_check()["n_added"] >= 0                # the kept report is not stale: the grid epoch did not move


def test_a_second_cast_of_the_same_size_allocates_nothing(pkg, product_lib):
    origins, ends = _rays()
    eng = _world(pkg)
    first, _ = eng.map_raycast(origins, ends)
    live = (C.c_longlong * 2)()
    product_lib.isdf_debug_live_bytes(live)
    before = list(live)
    again, _ = eng.map_raycast(origins, ends)
    fewer, _ = eng.map_raycast(SENSOR, ends[:100])
    product_lib.isdf_debug_live_bytes(live)
    assert list(live) == before and again.tobytes() == first.tobytes() and len(fewer) == 100


# ---- 6. rows_to_points
def test_entry_points_lie_on_their_faces(pkg, product_lib):
    eng = _world(pkg)
    origins, ends = _rays()
    rows, _ = eng.map_raycast(origins, ends)
    rng, point = pkg.engine.rows_to_points(rows, origins, ends, (BMIN, BMAX, RES, DIMS))
    hit = np.flatnonzero((rows[:, 0] == 1) & (rows[:, 1] > 0))
    assert len(hit) > 500
    a = rows[hit, 5]
    up = (ends[hit].astype(np.float64) > origins[hit])[np.arange(len(hit)), a]
    face = BMIN[a] + (rows[hit, 2 + a] + np.where(up, 0, 1)) * RES
    assert np.abs(point[hit, a] - face).max() <= 1e-9
    lo = BMIN + rows[hit, 2:5] * RES
    assert (point[hit] >= lo - 1e-9).all() and (point[hit] <= lo + RES + 1e-9).all()                 # in the closed voxel
    assert (rng[hit] > 0).all() and (rng[hit] <= np.linalg.norm(ends[hit] - origins[hit], axis=1) + 2e-3).all()


# ---- 7. the closed loop: a scan rendered from the world, integrated into the robot's map, read back
def test_closed_loop(pkg, product_lib):
    cloud_a, cloud_b, occ_a, occ_b, ends = closed_loop_scene()
    world, robot = _world(pkg, cloud_a), _world(pkg, cloud_b)
    assert np.array_equal(world.get_grid(pkg.capi.GRID_OCCUPANCY)[0], occ_a) and np.array_equal(robot.get_grid(pkg.capi.GRID_OCCUPANCY)[0], occ_b)
    scan_ends, hit, dropped = pkg.engine.scan_from_map(world, SENSOR, ends)
    on_host = pkg.engine.scan_from_map((occ_a, BMIN, BMAX, RES), SENSOR, ends, lib=product_lib)
    assert scan_ends.tobytes() == on_host[0].tobytes() and hit.tobytes() == on_host[1].tobytes() and dropped == on_host[2]
    rows_a, _ = world.map_raycast(SENSOR, scan_ends)
    assert np.array_equal(rows_a[:, 0], hit) and hit.sum() > 100 and (hit == 0).sum() > 20
    info = robot.integrate_scan(SENSOR, scan_ends, hit, miss_weight=1)
    assert info.n_rays_skipped == 0 and info.n_hits == hit.sum()
    rows_b, _ = robot.map_raycast(SENSOR, scan_ends)
    assert rows_b.tobytes() == rows_a.tobytes()
    # and not on an unchanged map: the scan freed voxels of the block only the robot's map had and occupied voxels of the other
    occ_after = robot.get_grid(pkg.capi.GRID_OCCUPANCY)[0]
    freed, born = (occ_b == 1) & (occ_after == 0), (occ_b == 0) & (occ_after == 1)
    print(f"\n{len(ends)} rays, {dropped} dropped, {hit.sum()} hits; the scan freed {freed.sum()} voxels and occupied {born.sum()}")
    assert freed[BLOCK_ONLY_B].sum() >= 5 and born[BLOCK_ONLY_A].sum() >= 5
    assert info.clear.n_cleared_voxels == freed.sum() and info.update.n_new_voxels == born.sum()


# ---- 8. the counters at the edges of the block sum: a lane, a wavefront, a workgroup of 128
@pytest.mark.parametrize("n", bs.CAST_SIZES)
def test_counters_equal_the_host_form_at_the_block_sums_edges(pkg, product_lib, n):
    g = FLAT
    occ, origins, ends = bs.cast_case()
    eng = pkg.Engine(pkg.synth.default_config(pkg.capi.V1_SWEPT))
    eng.set_grid(occ, g.bmin, g.res, pkg.capi.GRID_OCCUPANCY, bmax=g.bmax)
    want, want_hits = pkg.engine.raycast_host(occ, g.bmin, g.bmax, g.res, origins[:n], ends[:n], per_ray_origin=True, lib=product_lib)
    rows, info = eng.map_raycast(origins[:n], ends[:n], per_ray_origin=True)
    assert rows.shape == (n, 8) and rows.tobytes() == want.tobytes()
    got = {k: int(getattr(info, k)) for k in ("n_rays",) + bs.CAST_COUNTERS}
    print(f"\nn = {n}: {got}")
    assert got == bs.cast_counts(want) and info.n_hits == want_hits
