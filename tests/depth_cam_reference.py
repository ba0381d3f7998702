"""The depth camera's two definitions (include/isdf_accel.h, "the depth camera") restated in Python from the header's text: the render with
NumPy float32 / float64 scalars and Python integers, the rays with Python floats (fp64) and math.sqrt.  Shared by tests/test_depth_cam_host.py
and tests/test_gpu_depth_cam.py, with the scenes both use.  Nothing here calls the library."""
import functools
import math
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAMERA_YAML = os.path.join(ROOT, "tests", "golden", "camera.yaml")
F = np.float32
EMPTY = 999999
NAN_BITS = 0x7FC00000

# the map tests' geometry
DIMS = (24, 20, 70)
RES = 0.5
BMIN = np.array([-1.0, 2.0, 0.5])
BMAX = BMIN + np.array(DIMS) * RES

SMALL = dict(width=16, height=12, fx=12.0, fy=12.0, cx=8.3, cy=5.7)
WIDE = dict(width=33, height=17, fx=12.0, fy=12.0, cx=8.3, cy=5.7)


def pose(R, t):
    return np.concatenate([np.asarray(R, dtype=np.float64), np.asarray(t, dtype=np.float64).reshape(3, 1)], axis=1).reshape(12)


# the camera looks along world +x from a point whose coordinates are binary fractions: world2cam is exact in float32
AXIS_POSE = pose([[0, 0, 1], [-1, 0, 0], [0, -1, 0]], [1.5, 2.25, 3.0])


def rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = math.cos(rx), math.sin(rx), math.cos(ry), math.sin(ry), math.cos(rz), math.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


# inside the map, looking along its long axis (+z), a little off it
MAP_POSE = pose(rot(0.07, -0.05, 0.3), [5.1, 7.3, 9.2])


def cam_to_world(p12, pts_cam):
    m = np.asarray(p12, dtype=np.float64).reshape(3, 4)
    return (np.asarray(pts_cam, dtype=np.float64) @ m[:, :3].T + m[:, 3]).astype(np.float32)


# ---- the render
def world2cam(p12):
    m = np.asarray(p12, dtype=np.float64).reshape(3, 4)
    w = np.zeros(12, dtype=np.float32)
    for i in range(3):
        for j in range(3):
            w[4 * i + j] = F(m[j, i])
        w[4 * i + 3] = F(-(m[0, i] * m[0, 3] + m[1, i] * m[1, 3] + m[2, i] * m[2, 3]))
    return w


def project(cam, w, point, splat_m=0.0573, min_depth_m=0.0, max_splat_px=0):
    """("behind" | "near" | "outside", None) or ("drawn", (x0, x1, y0, y1, dist_mm, px, py, r, pxd, pyd))"""
    x, y, z = (F(v) for v in point)
    fx, fy = F(cam["fx"]), F(cam["fy"])
    with np.errstate(all="ignore"):
        X = x * w[0] + y * w[1] + z * w[2] + w[3]
        Y = x * w[4] + y * w[5] + z * w[6] + w[7]
        Z = x * w[8] + y * w[9] + z * w[10] + w[11]
        if not Z > 0:
            return "behind", None
        if Z < F(min_depth_m):
            return "near", None
        pxd = float(X / Z * fx) + cam["cx"] + 0.5
        pyd = float(Y / Z * fy) + cam["cy"] + 0.5
        if not (-1.0 < pxd < cam["width"] and -1.0 < pyd < cam["height"]):
            return "outside", None
        px, py = int(pxd), int(pyd)                 # Python's int() truncates towards zero
        mm = Z * F(1000.0) + F(0.5)
        dist = int(mm) if mm < F(2147483648.0) else 0x7FFFFFFF
        rd = splat_m * float(fx) / float(Z) + 0.5
    r = int(rd) if rd < 4096.0 else 4096
    if max_splat_px > 0:
        r = min(r, max_splat_px)
    return "drawn", (max(px - r, 0), min(px + r, cam["width"] - 1), max(py - r, 0), min(py + r, cam["height"] - 1), dist, px, py, r, pxd, pyd)


def render(cam, p12, xyz, **params):
    """(image int32 [height, width], counts dict) of the cloud"""
    w = world2cam(p12)
    img = np.full((cam["height"], cam["width"]), EMPTY, dtype=np.int64)
    c = dict(n_points=0, n_behind=0, n_outside=0, n_near=0, n_splat_pixels=0, n_pixels_set=0)
    for pt in np.asarray(xyz, dtype=np.float32).reshape(-1, 3):
        c["n_points"] += 1
        why, win = project(cam, w, pt, **params)
        if why != "drawn":
            c["n_" + why] += 1
            continue
        x0, x1, y0, y1, dist = win[:5]
        c["n_splat_pixels"] += (x1 - x0 + 1) * (y1 - y0 + 1)
        img[y0:y1 + 1, x0:x1 + 1] = np.minimum(img[y0:y1 + 1, x0:x1 + 1], dist)
    c["n_pixels_set"] = int((img != EMPTY).sum())
    return img.astype(np.int32), c


def voxel_centres(occ, bmin=BMIN, res=RES):
    """the centres of the occupied voxels in index order: bmin + (v + 0.5) * res in fp64, rounded to float32"""
    v = np.argwhere(np.asarray(occ) != 0).astype(np.float64)
    return (np.asarray(bmin, dtype=np.float64) + (v + 0.5) * np.float64(res)).astype(np.float32)


def info_counts(info, names):
    return {k: int(getattr(info, k)) for k in names}


RENDER_COUNTS = ("n_points", "n_behind", "n_outside", "n_near", "n_splat_pixels", "n_pixels_set")
RAYS_COUNTS = ("n_pixels", "n_no_return", "n_below_min", "n_truncated", "n_clipped", "n_hits")


# ---- the rays
def depth_of(image, fmt, u, v):
    """metres as a Python float, or None: no return"""
    val = image[v, u]
    if fmt == "i32":
        return None if (val >= 500000 or val <= 0) else int(val) / 1000.0
    if fmt == "u16":
        return None if val == 0 else int(val) / 1000.0
    f = float(val)
    return f if (f > 0.0 and math.isfinite(f)) else None


def rays(cam, p12, image, fmt, stride=(1, 1), min_range_m=0.0, max_range_m=math.inf, no_return_is_free=False, bmin=BMIN, bmax=BMAX, res=RES):
    """(ends float32 [n, 3], hit uint8 [n], counts, outside-axes per ray: -1 for a ray that never reached the clip)"""
    m = [float(v) for v in np.asarray(p12, dtype=np.float64)]
    R = [m[0:3], m[4:7], m[8:11]]
    o = [m[3], m[7], m[11]]
    fx, fy, cx, cy = (float(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    lo = [float(bmin[a]) + 0.5 * res for a in range(3)]
    hi = [float(bmax[a]) - 0.5 * res for a in range(3)]
    su, sv = stride
    nu, nv = -(-cam["width"] // su), -(-cam["height"] // sv)
    ends = np.zeros((nu * nv, 3), dtype=np.float32)
    hits = np.zeros(nu * nv, dtype=np.uint8)
    axes = np.full(nu * nv, -1, dtype=np.int64)
    c = dict(n_pixels=nu * nv, n_no_return=0, n_below_min=0, n_truncated=0, n_clipped=0, n_hits=0)
    nan = np.array([NAN_BITS], dtype=np.uint32).view(np.float32)[0]
    for iv in range(nv):
        for iu in range(nu):
            k = iv * nu + iu
            u, v = iu * su, iv * sv
            d = depth_of(image, fmt, u, v)
            scale_to, hit = None, True
            if d is None:
                c["n_no_return"] += 1
                if not no_return_is_free:
                    ends[k] = nan
                    continue
                d, scale_to, hit = 1.0, max_range_m, False
            p = [(u - cx) * d / fx, (v - cy) * d / fy, d]
            e = [R[a][0] * p[0] + R[a][1] * p[1] + R[a][2] * p[2] + o[a] for a in range(3)]
            dv = [e[a] - o[a] for a in range(3)]
            rng = math.sqrt(dv[0] * dv[0] + dv[1] * dv[1] + dv[2] * dv[2])
            if scale_to is None:
                if rng < min_range_m:
                    c["n_below_min"] += 1
                    ends[k] = nan
                    continue
                if rng > max_range_m:
                    c["n_truncated"] += 1
                    scale_to, hit = max_range_m, False
            if scale_to is not None:
                kk = scale_to / rng
                e = [o[a] + dv[a] * kk for a in range(3)]
                dv = [e[a] - o[a] for a in range(3)]
            s, n_axes = None, 0
            for a in range(3):
                if e[a] < lo[a]:
                    bound = lo[a]
                elif e[a] > hi[a]:
                    bound = hi[a]
                else:
                    continue
                n_axes += 1
                sa = (bound - o[a]) / dv[a] if dv[a] != 0.0 else 0.0
                s = sa if s is None or sa < s else s
            axes[k] = n_axes
            if s is not None:
                s = min(max(s, 0.0), 1.0)
                e = [o[a] + dv[a] * s for a in range(3)]
                c["n_clipped"] += 1
                hit = False
            with np.errstate(over="ignore"):
                row = np.array(e, dtype=np.float64).astype(np.float32)
            if not np.isfinite(row).all():
                ends[k] = nan
                continue
            ends[k] = row
            hits[k] = 1 if hit else 0
            c["n_hits"] += int(hit)
    return ends, hits, c, axes


# ---- scenes
def crafted_cloud(p12):
    """the named cases of the render, as camera-frame points taken to the world through the (exact) axis pose; f = 12, cx = 8.3, cy = 5.7"""
    cam_pts = [
        (0.0, 0.0, -1.0), (0.25, 0.0, 0.0),                         # behind the camera, and in its plane
        (0.0, 0.0, float(np.nextafter(F(0.5), F(1.0)))),           # just above a min_depth_m of 0.5
        (0.0, 0.0, 0.5), (0.0, 0.0, 0.4375),                        # at it (kept) and below it
        (-0.775 * 4, 0.0, 4.0), (0.0, -0.55 * 4, 4.0),              # a projection in (-1, 0) on x, on y: column / row 0
        (0.55 * 4, 0.0, 4.0), (0.62 * 4, 0.0, 4.0),                 # column width - 1 of the 16-wide image, and column `width`: outside
        (-0.6 * 0.25, -0.4 * 0.25, 0.25), (0.5 * 0.25, 0.45 * 0.25, 0.25),      # r = 3: windows across the left / top and right / bottom edges
        (0.0, 0.0, 0.015625),                                       # r = 44: covers the whole image
        (0.125, 0.125, 2.0), (0.09375, 0.09375, 1.5),                # one pixel, r = 0: the nearer wins
        (0.0, -0.25, 2.5),                                          # r = 0
        (0.01875, 0.01875, 0.1875), (0.025, 0.025, 0.25),      # r = 4 and r = 3: a max_splat_px of 3 clamps the first only
    ]
    return cam_to_world(p12, cam_pts)


def scaled_fixture_camera():
    """the reference's camera (tests/golden/camera.yaml) scaled by 0.1: 64 x 48"""
    vals = {}
    for line in open(CAMERA_YAML):
        if ":" in line:
            k, v = line.split("#", 1)[0].split(":", 1)
            vals[k.strip()] = float(v)
    return dict(width=64, height=48, fx=vals["cam_fx"] * 0.1, fy=vals["cam_fy"] * 0.1, cx=vals["cam_cx"] * 0.1, cy=vals["cam_cy"] * 0.1)


@functools.lru_cache(maxsize=None)
def random_cloud(n=3000, seed=5):
    """points in front of MAP_POSE (and some behind and beside it) at 0.1 to 6 m: at the 64 x 48 camera, windows from 1 to several hundred
    pixels, so both sides of the 64-pixel threshold between the lane and the wavefront, plus eight points whose clipped window is exactly 8 x 8"""
    rng = np.random.default_rng(seed)
    z = rng.uniform(0.1, 6.0, n) * np.where(rng.uniform(size=n) < 0.05, -1.0, 1.0)
    xy = rng.uniform(-1.0, 1.0, (n, 2)) * np.abs(z)[:, None]
    pts = cam_to_world(MAP_POSE, np.concatenate([xy, z[:, None]], axis=1))
    cam = scaled_fixture_camera()
    w = world2cam(MAP_POSE)
    exact = []
    # r = 4 (9 x 9) at the image's corner, clipped to 8 x 8 = 64 pixels: the centre pixel is (3, 3)
    for zc in np.linspace(0.45, 0.6, 40):
        p = cam_to_world(MAP_POSE, [[(3.2 - cam["cx"]) / cam["fx"] * zc, (3.2 - cam["cy"]) / cam["fy"] * zc, zc]])[0]
        why, win = project(cam, w, p)
        if why == "drawn" and (win[1] - win[0] + 1) * (win[3] - win[2] + 1) == 64:
            exact.append(p)
    assert len(exact) >= 4
    return np.concatenate([pts, np.array(exact[:8], dtype=np.float32)])


@functools.lru_cache(maxsize=None)
def map_occupancy(n=40, seed=12):
    """about 40 occupied voxels of the 24 x 20 x 70 map, most of them in front of MAP_POSE"""
    rng = np.random.default_rng(seed)
    occ = np.zeros(DIMS, dtype=np.uint8)
    cells = np.stack([rng.integers(0, DIMS[0], n), rng.integers(0, DIMS[1], n), rng.integers(10, DIMS[2], n)], axis=1)
    occ[tuple(cells.T)] = 1
    occ[0, 0, 0] = occ[DIMS[0] - 1, DIMS[1] - 1, DIMS[2] - 1] = 1        # the grid's two ends
    return occ


@functools.lru_cache(maxsize=None)
def depth_scene(seed=9):
    """a 33 x 17 depth image for MAP_POSE in the three formats, depths multiples of 125 mm (exact in float32 metres, so the formats
    agree): 0.5 to 30 m - the far ones leave the 12 x 10 x 35 m map on one or two axes -, a tenth no return."""
    rng = np.random.default_rng(seed)
    h, w = WIDE["height"], WIDE["width"]
    mm = (rng.integers(4, 240, (h, w)) * 125).astype(np.int32)
    none = rng.uniform(size=(h, w)) < 0.1
    i32 = np.where(none, np.where(rng.uniform(size=(h, w)) < 0.5, EMPTY, 500000), mm).astype(np.int32)
    u16 = np.where(none, 0, mm).astype(np.uint16)
    f32 = np.where(none, 0.0, mm / 1000.0).astype(np.float32)
    bad = np.argwhere(none)
    f32[tuple(bad[0])] = np.nan
    f32[tuple(bad[1])] = -2.0
    f32[tuple(bad[2])] = np.inf
    return {"i32": i32, "u16": u16, "f32": f32}
