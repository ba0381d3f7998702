"""The depth camera on the device (csrc/depth_cam.hip) against its plain host forms, which tests/test_depth_cam_host.py holds to the
definitions: images and rows byte for byte, counts equal.  isdf_integrate_depth on one ctx against isdf_integrate_scan of the host form's
rays on a second, from the same start: every product and every count of the scan's info.  Scenes of tests/depth_cam_reference.py and
of tests/test_gpu_map_scan.py (24 x 20 x 70 voxels at 0.5 m, sta_threshold 2, box robot)."""
import ctypes as C

import numpy as np
import pytest

import depth_cam_reference as ref
import test_block_sum_cases as bs
import test_gpu_map_scan as ms
import test_gpu_map_update as mu
from depth_cam_reference import AXIS_POSE, BMAX, BMIN, DIMS, MAP_POSE, RES, SMALL, WIDE
from test_depth_cam_host import PARAM_SETS, RAY_PARAMS, _bits, _cam

pytestmark = pytest.mark.gpu

WAVE_AREA = 64          # depth_cam.hip: windows above this many pixels are dealt out to the wavefront


def _bare(pkg):
    return pkg.Engine(pkg.synth.default_config(pkg.capi.V1_SWEPT))


def _render_both(pkg, lib, eng, camd, p12, xyz, **params):
    cam = _cam(pkg, camd)
    got, gi = eng.depth_render(cam, p12, xyz, **params)
    want, wi = pkg.engine.depth_render_host(cam, p12, xyz=xyz, lib=lib, **params)
    assert np.array_equal(got, want), (camd, params)
    assert ref.info_counts(gi, ref.RENDER_COUNTS) == ref.info_counts(wi, ref.RENDER_COUNTS), (camd, params)
    return got, gi


# ---- 1. the render
def test_render_equals_the_host_form(pkg, product_lib):
    eng = _bare(pkg)
    for camd in (SMALL, WIDE):
        for params in PARAM_SETS:
            _render_both(pkg, product_lib, eng, camd, AXIS_POSE, ref.crafted_cloud(AXIS_POSE), **params)
        img, info = _render_both(pkg, product_lib, eng, camd, AXIS_POSE, np.zeros((0, 3), dtype=np.float32))
        assert (img == ref.EMPTY).all() and info.n_points == 0


def test_render_of_a_random_cloud_across_the_wavefront_threshold(pkg, product_lib):
    camd = ref.scaled_fixture_camera()
    cloud = ref.random_cloud()
    w = ref.world2cam(MAP_POSE)
    areas = np.array([(win[1] - win[0] + 1) * (win[3] - win[2] + 1) for why, win in (ref.project(camd, w, p) for p in cloud) if why == "drawn"])
    assert (areas < WAVE_AREA).sum() > 100 and (areas == WAVE_AREA).sum() >= 4 and (areas == WAVE_AREA + 1).sum() + (areas > WAVE_AREA).sum() > 100
    assert areas.max() > 1000 and areas.min() == 1
    eng = _bare(pkg)
    for params in ({}, {"max_splat_px": 4}, {"min_depth_m": 0.3}):
        img, info = _render_both(pkg, product_lib, eng, camd, MAP_POSE, cloud, **params)
        print(f"\n{params}: {info.n_points} points, {info.n_splat_pixels} splat pixels, {info.n_pixels_set} set, {info.render_ms:.3f} ms")
    assert info.n_near > 0 and info.n_behind > 0 and info.n_outside > 0


def test_the_device_form_on_a_side_stream(pkg, product_lib):
    import torch
    camd = ref.scaled_fixture_camera()
    cam = _cam(pkg, camd)
    cloud = ref.random_cloud()
    want, wi = pkg.engine.depth_render_host(cam, MAP_POSE, xyz=cloud, lib=product_lib)
    eng = _bare(pkg)
    d_xyz = torch.from_numpy(cloud).cuda()
    d_img = torch.zeros((cam.height, cam.width), dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    assert eng.depth_render_device(cam, MAP_POSE, d_xyz, d_img, want_info=False, stream=side.cuda_stream) is None        # info_out == NULL: not synchronised
    side.synchronize()
    assert np.array_equal(d_img.cpu().numpy(), want)
    d_img.zero_()
    torch.cuda.synchronize()
    info = eng.depth_render_device(cam, MAP_POSE, d_xyz, d_img, stream=side.cuda_stream)
    assert np.array_equal(d_img.cpu().numpy(), want) and ref.info_counts(info, ref.RENDER_COUNTS) == ref.info_counts(wi, ref.RENDER_COUNTS)


def test_the_map_source_after_set_pointcloud(pkg, product_lib):
    old = ms._scene()[0]
    eng = mu._engine(pkg, old, esdf=False, frontend=False)
    occ = eng.get_grid(pkg.capi.GRID_OCCUPANCY)[0]
    assert 50 < occ.sum() < 400
    for camd in (WIDE, ref.scaled_fixture_camera()):
        cam = _cam(pkg, camd)
        for params in ({}, {"max_splat_px": 2}):
            got, gi = eng.depth_render(cam, MAP_POSE, None, **params)
            want, wi = pkg.engine.depth_render_host(cam, MAP_POSE, occ=occ, bmin=BMIN, res=RES, lib=product_lib, **params)
            assert np.array_equal(got, want) and ref.info_counts(gi, ref.RENDER_COUNTS) == ref.info_counts(wi, ref.RENDER_COUNTS)
            assert gi.n_points == occ.sum() and gi.n_pixels_set > 0
    with pytest.raises(pkg.IsdfError) as err:
        _bare(pkg).depth_render(cam, MAP_POSE, None)                # no occupancy grid
    assert err.value.code == pkg.capi.ISDF_ERR_STATE


def test_a_second_call_of_a_size_allocates_nothing(pkg, product_lib):
    eng = _bare(pkg)
    cloud = ref.random_cloud()
    small, large = _cam(pkg, SMALL), _cam(pkg, ref.scaled_fixture_camera())
    eng.depth_render(small, MAP_POSE, cloud[:500])
    eng.depth_render(large, MAP_POSE, cloud)
    before = ms._live(product_lib)
    a, _ = eng.depth_render(small, MAP_POSE, cloud[:500])
    b, _ = eng.depth_render(large, MAP_POSE, cloud)
    assert ms._live(product_lib) == before
    assert np.array_equal(a, pkg.engine.depth_render_host(small, MAP_POSE, xyz=cloud[:500], lib=product_lib)[0])
    assert np.array_equal(b, pkg.engine.depth_render_host(large, MAP_POSE, xyz=cloud, lib=product_lib)[0])


# ---- 2. the rays
@pytest.mark.parametrize("fmt", ["i32", "u16", "f32"])
def test_rays_equal_the_host_form(pkg, product_lib, fmt):
    eng = mu._engine(pkg, ms._scene()[0], esdf=False, frontend=False)           # the geometry is all the rays need
    image = ref.depth_scene()[fmt]
    cam = _cam(pkg, WIDE)
    for stride in ((1, 1), (2, 3), (5, 4)):
        for params in RAY_PARAMS:
            ends, hit, info = eng.depth_rays(cam, MAP_POSE, image, stride=stride, **params)
            want, want_hit, wi = pkg.engine.depth_rays_host(cam, MAP_POSE, image, BMIN, BMAX, RES, DIMS, lib=product_lib, stride=stride, **params)
            assert np.array_equal(_bits(ends), _bits(want)) and np.array_equal(hit, want_hit), (stride, params)             # NaN rows included
            assert ref.info_counts(info, ref.RAYS_COUNTS) == ref.info_counts(wi, ref.RAYS_COUNTS)
    outside = MAP_POSE.copy()
    outside[11] = BMAX[2] + 1.0
    with pytest.raises(pkg.IsdfError) as err:
        eng.depth_rays(cam, outside, image)
    assert err.value.code == pkg.capi.ISDF_ERR_INVALID_ARG


# ---- 3. a depth image integrated into the map
SCAN_POSE = ref.pose(ref.rot(0.1, -0.06, 0.4), ms.ORIGIN)
DEPTH_PARAMS = {"max_range_m": 7.0, "no_return_is_free": True, "min_range_m": 0.25}


def _depth_image(pkg, eng):
    """what the sensor at SCAN_POSE sees of the ctx's own map, with wide splats so that a good part of the image has a return"""
    img, info = eng.depth_render(_cam(pkg, WIDE), SCAN_POSE, None, splat_m=0.4)
    assert 30 < info.n_pixels_set < 33 * 17
    return img


def _host_rays(pkg, lib, image, p12=SCAN_POSE, bmin=BMIN, bmax=BMAX, **params):
    return pkg.engine.depth_rays_host(_cam(pkg, WIDE), p12, image, bmin, bmax, RES, DIMS, lib=lib, **params)


def test_integrate_depth_equals_the_scan_of_the_host_rays(pkg, product_lib):
    old = ms._scene()[0]
    a, b = mu._engine(pkg, old), mu._engine(pkg, old)
    image = _depth_image(pkg, a)
    incr = {"full_fraction": 1.0}
    dinfo, sinfo = a.integrate_depth(_cam(pkg, WIDE), SCAN_POSE, image, miss_weight=ms.MISS, **DEPTH_PARAMS, **incr)
    ends, hit, hinfo = _host_rays(pkg, product_lib, image, **DEPTH_PARAMS)
    want = b.integrate_scan(ms.ORIGIN, ends, hit, miss_weight=ms.MISS, **incr)
    assert ref.info_counts(dinfo, ref.RAYS_COUNTS) == ref.info_counts(hinfo, ref.RAYS_COUNTS)
    assert ms._fields(sinfo) == ms._fields(want)
    assert sinfo.n_rays == 33 * 17 and sinfo.n_hits == hinfo.n_hits > 10 and sinfo.n_free_voxels > 100 and sinfo.clear.n_cleared_voxels + sinfo.update.n_new_voxels > 0
    mu._same(mu._products(pkg, a), mu._products(pkg, b))
    # the staging split: the scan's own entry on the same ctx still gives its own bytes
    _, ends2, hit2 = ms._scene()
    ia, ib = a.integrate_scan(ms.ORIGIN, ends2, hit2, miss_weight=ms.MISS, **incr), b.integrate_scan(ms.ORIGIN, ends2, hit2, miss_weight=ms.MISS, **incr)
    assert ms._fields(ia) == ms._fields(ib)
    mu._same(mu._products(pkg, a), mu._products(pkg, b))
    # the other formats and a stride, from the same start again
    for img, params in ((np.where(image >= 65536, 0, image).astype(np.uint16), {"stride": (2, 1)}), ((np.where(image >= 500000, 0, image) / 1000.0).astype(np.float32), {})):
        a, b = mu._engine(pkg, old, frontend=False), mu._engine(pkg, old, frontend=False)
        dinfo, sinfo = a.integrate_depth(_cam(pkg, WIDE), SCAN_POSE, img, **DEPTH_PARAMS, **params)
        ends, hit, hinfo = _host_rays(pkg, product_lib, img, **DEPTH_PARAMS, **params)
        assert ms._fields(sinfo) == ms._fields(b.integrate_scan(ms.ORIGIN, ends, hit)) and ref.info_counts(dinfo, ref.RAYS_COUNTS) == ref.info_counts(hinfo, ref.RAYS_COUNTS)
        mu._same(mu._products(pkg, a, frontend=False), mu._products(pkg, b, frontend=False))


def test_integrate_depth_with_a_kept_field_and_an_armed_watch(pkg, product_lib):
    old = ms._scene()[0]
    a, _ = ms._watched(pkg, old, 1)
    b, _ = ms._watched(pkg, old, 1)
    image = _depth_image(pkg, a)
    incr = {"full_fraction": 1.0}
    dinfo, sinfo = a.integrate_depth(_cam(pkg, WIDE), SCAN_POSE, image, miss_weight=ms.MISS, **DEPTH_PARAMS, **incr)
    ends, hit, _ = _host_rays(pkg, product_lib, image, **DEPTH_PARAMS)
    want = b.integrate_scan(ms.ORIGIN, ends, hit, miss_weight=ms.MISS, **incr)
    assert ms._fields(sinfo) == ms._fields(want)
    fa, fb = ms._field_or_none(pkg, a), ms._field_or_none(pkg, b)
    assert (fa is None) == (fb is None)
    if fa is not None:
        assert np.array_equal(fa.view(np.uint8), fb.view(np.uint8))
    rep_a, last_a = a.traj_check_watch_info(ms.N)
    rep_b, last_b = b.traj_check_watch_info(ms.N)
    ms._same_report(rep_a, rep_b, "watch after the depth image")
    assert {k: v for k, v in last_a.items() if not k.endswith("_ms")} == {k: v for k, v in last_b.items() if not k.endswith("_ms")}
    assert a.traj_check_points().tobytes() == b.traj_check_points().tobytes()
    mu._same(mu._products(pkg, a), mu._products(pkg, b))


def test_status_codes(pkg, product_lib):
    capi = pkg.capi
    old = ms._scene()[0]
    eng = mu._engine(pkg, old, esdf=False, frontend=False)
    cam = _cam(pkg, WIDE)
    image = ref.depth_scene()["i32"]
    before = eng.map_counts()
    outside = SCAN_POSE.copy()
    outside[3] = BMIN[0] - 0.5
    for p12, cm, params in ((outside, cam, {}), (SCAN_POSE, _cam(pkg, {**WIDE, "fx": 0.0}), {}), (SCAN_POSE, cam, {"no_return_is_free": True}),
                            (SCAN_POSE, cam, {"miss_weight": -1}), (SCAN_POSE, cam, {"stride": 0})):
        with pytest.raises(pkg.IsdfError) as err:
            eng.integrate_depth(cm, p12, image if cm is cam else np.zeros((17, 33), dtype=np.int32), **params)
        assert err.value.code == capi.ISDF_ERR_INVALID_ARG, params
    assert np.array_equal(eng.map_counts(), before)                 # a refused call changed nothing
    with pytest.raises(pkg.IsdfError) as err:
        _bare(pkg).integrate_depth(cam, SCAN_POSE, image)
    assert err.value.code == capi.ISDF_ERR_STATE
    multi = pkg.Engine(pkg.synth.default_config(capi.V3_ESDF_TILE), devices=[0, 0])
    multi.set_pointcloud(old, RES, mu.THR, BMIN, BMAX)
    for call in (lambda: multi.integrate_depth(cam, SCAN_POSE, image), lambda: multi.depth_render(cam, SCAN_POSE, old), lambda: multi.depth_rays(cam, SCAN_POSE, image)):
        with pytest.raises(pkg.IsdfError) as err:
            call()
        assert err.value.code == capi.ISDF_ERR_UNSUPPORTED


# ---- 4. the loop: render -> integrate -> follow, from poses alone
def _corridor():
    """two walls along z at x = 2.2 and x = 7.8 and an end wall, sampled every 0.2 m"""
    y, z = np.meshgrid(np.arange(4.0, 10.0, 0.2), np.arange(3.0, 33.0, 0.2), indexing="ij")
    walls = [np.stack([np.full(y.size, x), y.ravel(), z.ravel()], axis=1) for x in (2.2, 7.8)]
    x, y = np.meshgrid(np.arange(2.2, 7.8, 0.2), np.arange(4.0, 10.0, 0.2), indexing="ij")
    return np.concatenate(walls + [np.stack([x.ravel(), y.ravel(), np.full(x.size, 32.0)], axis=1)]).astype(np.float32)


def test_the_loop_from_poses_alone(pkg, product_lib):
    truth = _corridor()
    old = ms._scene()[0]
    a, b = mu._engine(pkg, old), mu._engine(pkg, old)
    cam = _cam(pkg, WIDE)
    params = {"max_range_m": 9.0, "no_return_is_free": True, "min_range_m": 0.3}
    for z in (14.0, 17.0, 20.5):
        p12 = ref.pose(ref.rot(0.05, 0.1, -0.2), [5.2, 7.1, z])
        image, rinfo = a.depth_render(cam, p12, truth, splat_m=0.15)
        host_image, _ = pkg.engine.depth_render_host(cam, p12, xyz=truth, lib=product_lib, splat_m=0.15)
        assert np.array_equal(image, host_image) and rinfo.n_pixels_set > 50
        dinfo, sinfo = a.integrate_depth(cam, p12, image, **params)
        _, bmin, bmax = b.get_grid(pkg.capi.GRID_OCCUPANCY)
        ends, hit, _ = _host_rays(pkg, product_lib, host_image, p12=p12, bmin=bmin, bmax=bmax, **params)
        want = b.integrate_scan(p12.reshape(3, 4)[:, 3], ends, hit)
        assert ms._fields(sinfo) == ms._fields(want)
        assert all(v >= 0 for v in ref.info_counts(dinfo, ref.RAYS_COUNTS).values()) and sinfo.n_hits > 0 and min(sinfo.n_free_voxels, sinfo.n_rays_skipped) >= 0
        sa, _ = a.map_follow(p12.reshape(3, 4)[:, 3])
        sb, _ = b.map_follow(p12.reshape(3, 4)[:, 3])
        assert sa == sb
    assert sa != (0, 0, 0)
    mu._same(mu._products(pkg, a), mu._products(pkg, b))
    assert np.array_equal(a.get_grid(pkg.capi.GRID_OCCUPANCY)[1], b.get_grid(pkg.capi.GRID_OCCUPANCY)[1])


# ---- 5. the counters at the edges of the block sum: a lane, a wavefront, a workgroup of 256
@pytest.mark.parametrize("n", bs.DC_SIZES)
def test_render_counters_equal_the_host_form_at_the_block_sums_edges(pkg, product_lib, n):
    cloud = bs.dc_cloud()[:n]
    _, info = _render_both(pkg, product_lib, _bare(pkg), bs.DC_CAM, AXIS_POSE, cloud, **bs.DC_RENDER_PARAMS)
    print(f"\nn = {n}: {ref.info_counts(info, ref.RENDER_COUNTS)}")
    assert info.n_points == n and info.n_pixels_set > 0


@pytest.mark.parametrize("size", bs.DC_RAYS_IMAGES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_rays_counters_equal_the_host_form_at_the_block_sums_edges(pkg, product_lib, size):
    eng = _bare(pkg)
    eng.set_grid(np.zeros(DIMS, dtype=np.uint8), BMIN, RES, pkg.capi.GRID_OCCUPANCY, bmax=BMAX)          # the geometry is all the rays need
    cam = _cam(pkg, dict(bs.DC_CAM, width=size[0], height=size[1]))
    image = bs.dc_depth_image(*size)
    ends, hit, info = eng.depth_rays(cam, MAP_POSE, image, **bs.DC_RAYS_PARAMS)
    want, want_hit, wi = pkg.engine.depth_rays_host(cam, MAP_POSE, image, BMIN, BMAX, RES, DIMS, lib=product_lib, **bs.DC_RAYS_PARAMS)
    assert np.array_equal(_bits(ends), _bits(want)) and np.array_equal(hit, want_hit)
    print(f"\n{size}: {ref.info_counts(info, ref.RAYS_COUNTS)}")
    assert ref.info_counts(info, ref.RAYS_COUNTS) == ref.info_counts(wi, ref.RAYS_COUNTS) and info.n_pixels == size[0] * size[1]
