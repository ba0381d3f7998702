"""The view gain on the device (csrc/view_gain.hip: isdf_view_gain, isdf_view_gain_device) against the plain host form, which
tests/test_view_gain_host.py holds to the NumPy restatement.  Every comparison of rows and of the info's integer words is == on bytes.
Grids and engines are tests/test_gpu_map_known.py's, camera and poses the host test's; the closed loop holds the gain to what
isdf_integrate_depth then reports as newly known."""
import numpy as np
import pytest

import known_reference as kr
import test_block_sum_cases as bs
from test_gpu_map_known import RES, _grid_engine, _random_fills
from test_gpu_map_update import _live
from test_map_known_host import GRIDS, IDS
from test_view_gain_host import RANGES, STRIDES, cam_of, poses_of

pytestmark = pytest.mark.gpu
INT_WORDS = ("n_views", "n_scored", "n_rays_per_view", "best_view", "best_gain", "gain_total")


def _host(pkg, lib, eng, cam, poses, **params):
    """the host form on the ctx's own K, occupancy and box"""
    occ, bmin, bmax = eng.get_grid(pkg.capi.GRID_OCCUPANCY)
    params.pop("scratch_bytes", None)
    return pkg.engine.view_gain_host(eng.map_known()[0], occ, bmin, bmax, RES, cam, poses, lib=lib, **params)


def _same(pkg, lib, eng, cam, poses, chunks=1, **params):
    want, hinfo = _host(pkg, lib, eng, cam, poses, **params)
    got, info = eng.view_gain(cam, poses, **params)
    assert got.dtype == np.int64 and np.array_equal(got, want), (params, got, want)
    assert [getattr(info, w) for w in INT_WORDS] == [getattr(hinfo, w) for w in INT_WORDS]
    assert info.chunks == chunks and info.gain_ms >= 0.0
    return got, info


def _sweep(pkg, lib, eng, cam, poses):
    total = 0
    for stride in STRIDES:
        for rng_m in RANGES:
            total += int(_same(pkg, lib, eng, cam, poses, stride=stride, max_range_m=rng_m)[0][:, 1].sum())
    return total


@pytest.mark.parametrize("dims", GRIDS, ids=IDS)
def test_rows_equal_the_host_form(pkg, product_lib, dims):
    eng, _ = _grid_engine(pkg, dims)
    eng.map_known_enable(True)
    cam = cam_of(pkg)
    poses, _ = poses_of(pkg, eng.get_grid(pkg.capi.GRID_OCCUPANCY)[0])
    assert _sweep(pkg, product_lib, eng, cam, poses) > 0        # all unknown
    for box, value in _random_fills(dims):
        eng.map_known_fill(box, value)
    k = kr.unpack(eng.map_known()[0], dims)
    assert 0 < k.sum() < k.size
    assert _sweep(pkg, product_lib, eng, cam, poses) > 0
    ext = np.array(dims) * RES                                  # a scan from the first pose's eye: its merge makes what that pose sees known
    ends = (np.random.default_rng(5).uniform(0.05, 0.95, (200, 3)) * ext).astype(np.float32)
    eng.integrate_scan(poses[0].reshape(3, 4)[:, 3], ends, np.zeros(len(ends), dtype=np.uint8), miss_weight=0)
    assert eng.map_known()[1].merges == 1
    _sweep(pkg, product_lib, eng, cam, poses)
    eng.shift_map((2, -3, 5))
    _sweep(pkg, product_lib, eng, cam, poses)
    rows, info = _same(pkg, product_lib, eng, cam, poses[:0], chunks=0)     # no views
    assert rows.shape == (0, 8) and (info.best_view, info.chunks) == (-1, 0)


@pytest.mark.parametrize("dims", GRIDS, ids=IDS)
def test_the_chunk_size_does_not_change_a_byte(pkg, product_lib, dims):
    eng, _ = _grid_engine(pkg, dims)
    eng.map_known_enable(True)
    for box, value in _random_fills(dims)[:6]:
        eng.map_known_fill(box, value)
    cam = cam_of(pkg)
    poses = poses_of(pkg, eng.get_grid(pkg.capi.GRID_OCCUPANCY)[0])[0][:5]
    two_views = 2 * 4 * pkg.engine.known_words(dims)
    a, _ = _same(pkg, product_lib, eng, cam, poses, chunks=5, stride=1, max_range_m=40.0, scratch_bytes=0)
    b, _ = _same(pkg, product_lib, eng, cam, poses, chunks=3, stride=1, max_range_m=40.0, scratch_bytes=two_views)
    c, _ = _same(pkg, product_lib, eng, cam, poses, chunks=1, stride=1, max_range_m=40.0)
    assert a.tobytes() == b.tobytes() == c.tobytes() and a[:, 1].sum() > 0


def test_device_form_on_a_side_stream(pkg, product_lib):
    import torch
    dims = GRIDS[2]
    eng, _ = _grid_engine(pkg, dims)
    eng.map_known_enable(True)
    for box, value in _random_fills(dims)[:6]:
        eng.map_known_fill(box, value)
    cam = cam_of(pkg)
    poses, _ = poses_of(pkg, eng.get_grid(pkg.capi.GRID_OCCUPANCY)[0])
    want, hinfo = _host(pkg, product_lib, eng, cam, poses, stride=1, max_range_m=40.0)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d_poses = torch.tensor(poses, dtype=torch.float64, device="cuda")
        d_rows = torch.full((len(poses), 8), -7, dtype=torch.int64, device="cuda")
    side.synchronize()
    info = eng.view_gain_device(cam, d_poses, d_rows, stream=side.cuda_stream, stride=1, max_range_m=40.0)
    assert np.array_equal(d_rows.cpu().numpy(), want)           # the call synchronised the stream
    assert [getattr(info, w) for w in INT_WORDS] == [getattr(hinfo, w) for w in INT_WORDS] and info.chunks == 1
    with torch.cuda.stream(side):
        d_rows.fill_(-7)
    assert eng.view_gain_device(cam, d_poses, d_rows, want_info=False, stream=side.cuda_stream, stride=1, max_range_m=40.0) is None
    side.synchronize()
    assert np.array_equal(d_rows.cpu().numpy(), want)
    _same(pkg, product_lib, eng, cam, poses, stride=1, max_range_m=40.0)


def test_the_call_is_read_only_and_allocates_once(pkg, product_lib):
    dims = GRIDS[2]
    eng, _ = _grid_engine(pkg, dims)
    cam = cam_of(pkg)
    poses, _ = poses_of(pkg, eng.get_grid(pkg.capi.GRID_OCCUPANCY)[0])
    with pytest.raises(pkg.engine.IsdfError) as e:              # the mode is off
        eng.view_gain(cam, poses)
    assert e.value.code == pkg.capi.ISDF_ERR_STATE
    eng.map_known_enable(True)
    for box, value in _random_fills(dims)[:6]:
        eng.map_known_fill(box, value)
    ends = (np.random.default_rng(5).uniform(0.05, 0.95, (50, 3)) * np.array(dims) * RES).astype(np.float32)
    eng.integrate_scan(poses[0].reshape(3, 4)[:, 3], ends, np.zeros(len(ends), dtype=np.uint8), miss_weight=0)

    def state():
        bits, info = eng.map_known()
        return bits.tobytes(), eng.get_grid(pkg.capi.GRID_OCCUPANCY)[0].tobytes(), info.merges, info.newly_known
    before = state()
    first, _ = eng.view_gain(cam, poses, stride=1, max_range_m=40.0)
    live = _live(product_lib)
    second, _ = eng.view_gain(cam, poses, stride=1, max_range_m=40.0)
    assert _live(product_lib) == live and second.tobytes() == first.tobytes()
    assert state() == before and before[2] == 1
    for bad in ({"stride": 0}, {"max_range_m": float("nan")}, {"max_range_m": 0.0}, {"scratch_bytes": -1}):
        with pytest.raises(pkg.engine.IsdfError) as e:
            eng.view_gain(cam, poses, **bad)
        assert e.value.code == pkg.capi.ISDF_ERR_INVALID_ARG
    with pytest.raises(pkg.engine.IsdfError) as e:
        eng.view_gain(pkg.engine.depth_camera(8, 6, 0.0, 6.0, 3.5, 2.5), poses)
    assert e.value.code == pkg.capi.ISDF_ERR_INVALID_ARG
    other, _ = _grid_engine(pkg, GRIDS[0])                      # a second ctx with the mode off, while the first has a grid
    with pytest.raises(pkg.engine.IsdfError) as e:
        other.view_gain(cam, poses)
    assert e.value.code == pkg.capi.ISDF_ERR_STATE
    assert state() == before


def test_the_gain_is_what_integrating_the_view_then_makes_known(pkg, product_lib):
    """closed loop against isdf_integrate_depth: nothing occupied in the frustum, every occupied voxel behind the camera"""
    dims = GRIDS[2]
    rng = np.random.default_rng(3)
    occ = np.zeros(dims, dtype=bool)
    occ[:4] = rng.uniform(size=(4,) + dims[1:]) < 0.2
    cloud = ((np.repeat(np.argwhere(occ), 2, axis=0) + 0.5) * RES).astype(np.float32)
    eng = pkg.Engine(pkg.synth.default_config(pkg.capi.V1_SWEPT))
    assert eng.set_pointcloud(cloud, RES, 2, np.zeros(3), np.array(dims) * RES) == tuple(dims)
    assert np.array_equal(eng.get_grid(pkg.capi.GRID_OCCUPANCY)[0] != 0, occ)
    eng.map_known_enable(True)
    cam = cam_of(pkg, 32, 24, 20.0)
    eye = (np.array([6, 10, 35]) + 0.5) * RES
    pose = pkg.engine.look_at(eye, eye + (1.0, 0.1, -0.2))
    for stride, rng_m in (((1, 1), 4.0), ((3, 2), 40.0)):
        eng.map_known_fill(None, 0)
        rows, info = _same(pkg, product_lib, eng, cam, pose, stride=stride, max_range_m=rng_m)
        assert rows[0, 0] == 0 and rows[0, 4] == 0 and rows[0, 1] > 50      # scored, no walk ended by an occupied voxel
        image = np.zeros((cam.height, cam.width), dtype=np.uint16)
        eng.integrate_depth(cam, pose, image, stride=stride, max_range_m=rng_m, no_return_is_free=True)
        assert eng.map_known()[1].newly_known == rows[0, 1]
        again, _ = _same(pkg, product_lib, eng, cam, pose, stride=stride, max_range_m=rng_m)
        assert again[0].tolist() == [0, 0, rows[0, 2], rows[0, 3], 0, rows[0, 5], 0, 0]


def test_a_known_map_offers_nothing(pkg, product_lib):
    dims = GRIDS[1]
    eng, _ = _grid_engine(pkg, dims)
    eng.map_known_enable(True)
    eng.map_known_fill(None, 1)
    cam = cam_of(pkg)
    poses, _ = poses_of(pkg, eng.get_grid(pkg.capi.GRID_OCCUPANCY)[0])
    rows, info = _same(pkg, product_lib, eng, cam, poses[::-1], stride=1, max_range_m=40.0)     # reversed: the first two are not scored
    assert rows[:, 0].tolist() == [1, 1, 0, 0, 0, 0] and not rows[:, 1].any() and not rows[:, 6].any()
    assert (info.best_view, info.best_gain, info.gain_total, info.n_scored) == (2, 0, 0, 4)


# ---- the counters at the edges of the block sum: a lane, a wavefront, a workgroup of 128; the second view returns before it
@pytest.mark.parametrize("n_rays", sorted(bs.VG_STRIDES))
def test_counters_equal_the_host_form_at_the_block_sums_edges(pkg, product_lib, n_rays):
    eng, _ = _grid_engine(pkg, bs.VG_DIMS)
    eng.map_known_enable(True)
    eng.map_known_fill(bs.VG_KNOWN_BOX, 1)
    cam = pkg.engine.depth_camera(**bs.VG_CAM)
    rows, info = _same(pkg, product_lib, eng, cam, bs.vg_poses(pkg, bs.VG_DIMS, RES), stride=bs.VG_STRIDES[n_rays], max_range_m=bs.VG_RANGE)
    print(f"\n{n_rays} rays: {rows[0]}")
    assert rows[0, 2] == n_rays and rows[0, 1] > 0 and (rows[1] == [1, 0, 0, 0, 0, 0, 0, 0]).all() and info.n_scored == 1
    assert n_rays == 1 or (rows[0, 1:7] > 0).all()                  # every counter counts (tests/test_block_sum_cases.py, on the same map)
