"""NumPy restatement of the view gain (include/isdf_accel.h, "the view gain") built only from host functions that are older than it:
per view engine.depth_rays_host on an all-zero uint16 image with no_return_is_free = 1, engine.raycast_host from the camera's position
with test_origin_voxel = False, per ray of status 0 or 1 the first steps + 1 voxels of engine.scan_ray_host, then a set union masked
by ~K.  Nothing here calls isdf_view_gain*.  The walks do not depend on K: `views` is computed once per (map, camera, poses, stride,
range) and `rows` masks it with each K."""
import numpy as np


def views(engine, lib, occ, bmin, bmax, res, cam, poses, stride, max_range_m):
    """per pose None (status 1) or {"walks": the flat voxel indices of V(ray) per ray that was not skipped, and the row's sums taken
    from the raycast rows}"""
    occ = np.ascontiguousarray(occ, dtype=np.uint8)
    dims = occ.shape
    image = np.zeros((cam.height, cam.width), dtype=np.uint16)
    out = []
    for pose in np.asarray(poses, dtype=np.float64).reshape(-1, 12):
        if not np.isfinite(pose).all():
            out.append(None)
            continue
        t = pose.reshape(3, 4)[:, 3]
        try:
            ends, _, _ = engine.depth_rays_host(cam, pose, image, bmin, bmax, res, dims, lib=lib, stride=stride, max_range_m=max_range_m, no_return_is_free=1)
        except engine.IsdfError:                                # the origin lies outside the map
            out.append(None)
            continue
        rc, _ = engine.raycast_host(occ, bmin, bmax, res, t, ends, test_origin_voxel=False, lib=lib)
        assert not (rc[:, 0] == 3).any()
        went = rc[:, 0] <= 1
        walks = []
        for e, steps in zip(ends[went], rc[went, 1]):
            w = engine.scan_ray_host(bmin, bmax, res, dims, t, e, lib=lib)[:int(steps) + 1].astype(np.int64)
            assert len(w) == steps + 1
            walks.append((w[:, 0] * dims[1] + w[:, 1]) * dims[2] + w[:, 2])
        out.append({"walks": walks, "n_rays": len(ends), "n_skipped": int((rc[:, 0] == 2).sum()), "n_hits": int((rc[:, 0] == 1).sum()),
                    "steps_total": int(rc[went, 1].astype(np.int64).sum())})
    return out


def seen(view, n_vox):
    """S_j as a flat boolean array"""
    s = np.zeros(n_vox, dtype=bool)
    for w in view["walks"]:
        s[w] = True
    return s


def rows(vs, k):
    """the call's rows, int64 [n, 8], for the known grid k (bool [X, Y, Z])"""
    unknown = ~np.asarray(k, dtype=bool).reshape(-1)
    out = np.zeros((len(vs), 8), dtype=np.int64)
    for j, v in enumerate(vs):
        if v is None:
            out[j, 0] = 1
            continue
        gain = int((seen(v, unknown.size) & unknown).sum())
        n_rays_unknown = sum(1 for w in v["walks"] if unknown[w].any())
        out[j] = [0, gain, v["n_rays"], v["n_skipped"], v["n_hits"], v["steps_total"], n_rays_unknown, 0]
    return out


def per_ray_unknown(view, k):
    """the sum over the rays of their unknown voxels: what the gain is NOT"""
    unknown = ~np.asarray(k, dtype=bool).reshape(-1)
    return int(sum(unknown[w].sum() for w in view["walks"]))


def best(r):
    """(n_scored, best_view, best_gain, gain_total) of rows"""
    scored = np.flatnonzero(r[:, 0] == 0)
    if len(scored) == 0:
        return 0, -1, 0, 0
    g = r[scored, 1]
    return len(scored), int(scored[np.argmax(g)]), int(g.max()), int(g.sum())        # argmax: the first of the largest
