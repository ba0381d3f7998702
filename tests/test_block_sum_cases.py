"""The inputs on which the device tests hold the queries' counters to the host forms at the edges of dev_reduce.hpp's block sum - a
lane, a wavefront, a workgroup - and, here, the proof that the host forms count something in every counter on them: a counter that is 0
on the host would hold nothing.  Ray cast: tests/test_map_raycast_host.py's 9 x 1 x 13 grid.  Depth camera: a 17 x 13 camera at
tests/depth_cam_reference.py's poses (and, for the rays, the same intrinsics on images of exactly 1, 255 and 257 pixels, which 17 x 13
cannot give).  View gain: a 43 x 13 camera whose strides give 1, 65 and 129 rays per view."""
import numpy as np
import pytest

import depth_cam_reference as ref
from test_map_raycast_host import FLAT

# ---- the ray cast: MR_BLOCK = 128
CAST_SIZES = (0, 1, 63, 64, 65, 127, 129)
CAST_COUNTERS = ("n_skipped", "n_origin_outside", "n_hits", "n_clear", "steps_total")


def cast_case():
    """(occ, origins float64 [129, 3], ends float32 [129, 3]): the column x = 4 is occupied; ray i is of kind i % 4 - 0: a hit across the
    column, 1: clear on this side of it, 2: the end outside the map, 3: the origin outside"""
    g = FLAT
    occ = np.zeros(g.dims, dtype=np.uint8)
    occ[4, 0, :] = 1
    rng = np.random.default_rng(17)
    n = CAST_SIZES[-1]
    origins = np.array([g.centre((1, 0, rng.integers(0, 13))) + rng.uniform(-0.2, 0.2, 3) for _ in range(n)])
    ends = np.array([g.centre((7 if i % 4 == 0 else 3, 0, rng.integers(0, 13))) + rng.uniform(-0.2, 0.2, 3) for i in range(n)])
    ends[2::4] = g.bmax + 0.3
    origins[3::4] = g.bmin - 0.1
    return occ, origins, ends.astype(np.float32)


def cast_counts(rows):
    """the info's counters as the rows give them (mr_count_row)"""
    ok = rows[:, 0] < 2
    return {"n_rays": len(rows), "n_clear": int((rows[:, 0] == 0).sum()), "n_hits": int((rows[:, 0] == 1).sum()), "n_skipped": int((rows[:, 0] == 2).sum()),
            "n_origin_outside": int((rows[:, 0] == 3).sum()), "steps_total": int(rows[ok, 1].sum())}


def test_every_cast_counter_counts(pkg, product_lib):
    g = FLAT
    occ, origins, ends = cast_case()
    for n in CAST_SIZES:
        rows, hits = pkg.engine.raycast_host(occ, g.bmin, g.bmax, g.res, origins[:n], ends[:n], per_ray_origin=True, lib=product_lib)
        counts = cast_counts(rows)
        assert hits == counts["n_hits"] and counts["n_rays"] == n
        if n >= 63:
            assert all(counts[k] > 0 for k in CAST_COUNTERS), (n, counts)
    assert counts["n_hits"] == 33 and counts["n_origin_outside"] == 32         # (n = 129: kinds 0 and 3)
    first = cast_counts(pkg.engine.raycast_host(occ, g.bmin, g.bmax, g.res, origins[:1], ends[:1], per_ray_origin=True, lib=product_lib)[0])
    assert first["n_hits"] == 1 and first["steps_total"] >= 3          # (three steps in x to the column, and those in z)


# ---- the depth camera: DC_BLOCK = 256
DC_SIZES = (1, 255, 257)
DC_CAM = dict(width=17, height=13, fx=12.0, fy=12.0, cx=8.3, cy=5.7)
DC_RENDER_PARAMS = {"min_depth_m": 0.5}
DC_RAYS_PARAMS = {"min_range_m": 0.25, "max_range_m": 25.0}
DC_RAYS_IMAGES = ((1, 1), (17, 13), (17, 15), (257, 1))             # 1, 221, 255 and 257 pixels


def dc_cloud():
    """257 points, as camera-frame points taken to the world through the axis pose; point i is of kind i % 4 - 0: drawn, 1: behind, 2: outside
    the image, 3: nearer than min_depth_m"""
    rng = np.random.default_rng(23)
    pts = []
    for i in range(DC_SIZES[-1]):
        z = rng.uniform(1.0, 4.0)
        kind = i % 4
        if kind == 0:
            pts.append(((rng.uniform(1, 15) - 8.3) / 12.0 * z, (rng.uniform(1, 11) - 5.7) / 12.0 * z, z))
        elif kind == 1:
            pts.append((rng.uniform(-1, 1), rng.uniform(-1, 1), -z))
        elif kind == 2:
            pts.append((3.0 * z, rng.uniform(-0.2, 0.2), z))
        else:
            pts.append((0.0, 0.0, rng.uniform(0.1, 0.4)))
    return ref.cam_to_world(ref.AXIS_POSE, pts)


def dc_depth_image(width, height):
    """int32 millimetres; pixel k is of kind k % 5 - 0: a hit at 2 m, 1: no return, 2: below min_range_m, 3: beyond max_range_m, 4: 20 m, out
    of the 12 x 10 x 35 m map"""
    k = np.arange(width * height)
    return np.choose(k % 5, [2000, 0, 100, 30000, 20000]).astype(np.int32).reshape(height, width)


def test_every_depth_counter_counts(pkg, product_lib):
    cam = pkg.engine.depth_camera(**DC_CAM)
    cloud = dc_cloud()
    for n in DC_SIZES:
        info = pkg.engine.depth_render_host(cam, ref.AXIS_POSE, xyz=cloud[:n], lib=product_lib, **DC_RENDER_PARAMS)[1]
        counts = ref.info_counts(info, ref.RENDER_COUNTS)
        assert counts["n_points"] == n and counts["n_pixels_set"] > 0 and counts["n_splat_pixels"] > 0
        if n > 1:
            assert all(v > 0 for v in counts.values()), (n, counts)
    for width, height in DC_RAYS_IMAGES:
        c = pkg.engine.depth_camera(**dict(DC_CAM, width=width, height=height))
        info = pkg.engine.depth_rays_host(c, ref.MAP_POSE, dc_depth_image(width, height), ref.BMIN, ref.BMAX, ref.RES, ref.DIMS, lib=product_lib, **DC_RAYS_PARAMS)[2]
        counts = ref.info_counts(info, ref.RAYS_COUNTS)
        assert counts["n_pixels"] == width * height and counts["n_hits"] > 0
        if width * height > 1:
            assert all(v > 0 for v in counts.values()), ((width, height), counts)


# ---- the view gain: a workgroup of 128
VG_CAM = dict(width=43, height=13, fx=6.0, fy=6.0, cx=0.0, cy=6.0)
VG_STRIDES = {1: (43, 13), 65: (9, 1), 129: (1, 5)}                 # rays per view: (stride_u, stride_v)
VG_DIMS = (6, 5, 64)
VG_RANGE = 40.0
VG_KNOWN_BOX = (3, 0, 0, 5, 4, 63)                                  # the half x >= 3 of the map is known; the first view's eye is in the other


def vg_poses(pkg, dims, res):
    """two views: one inside the map, one outside it (status 1: every thread of its workgroups returns before the block sum).  The first
    view's x axis is scaled by 1e308 - finite, so the pose is scored -: its rays of column u = 0 (cx = 0) are ordinary, those further right
    overflow to an end point that is not finite and are skipped, which is the only way a ray of a scored view is skipped."""
    look = pkg.engine.look_at
    ext = np.array(dims) * res
    inside = look(0.4 * ext, ext * (0.9, 0.6, 0.5))
    inside[0::4] *= 1e308
    return np.array([inside, look(ext + 1.0, 0.5 * ext)])


def test_every_view_gain_counter_counts(pkg, product_lib):
    from test_view_gain_host import RES, occ_of
    cam = pkg.engine.depth_camera(**VG_CAM)
    occ = (occ_of(VG_DIMS) != 0).astype(np.uint8)                   # the occupancy of tests/test_gpu_map_known.py's _grid_engine
    occ[0, 0, 0] = 0
    known = np.zeros(VG_DIMS, dtype=bool)
    known[VG_KNOWN_BOX[0]:] = True
    bits = pkg.engine.known_pack(known)
    poses = vg_poses(pkg, VG_DIMS, RES)
    for n_rays, stride in VG_STRIDES.items():
        rows, info = pkg.engine.view_gain_host(bits, occ, np.zeros(3), np.array(VG_DIMS) * RES, RES, cam, poses, lib=product_lib, stride=stride, max_range_m=VG_RANGE)
        assert rows[0, 0] == 0 and rows[0, 2] == n_rays and (rows[1] == [1, 0, 0, 0, 0, 0, 0, 0]).all()
        assert rows[0, 1] > 0 and rows[0, 6] > 0, (n_rays, rows[0])
        if n_rays > 1:
            assert (rows[0, 1:7] > 0).all(), (n_rays, rows[0])      # gain, n_rays, n_skipped, n_hits, steps_total, n_rays_unknown
