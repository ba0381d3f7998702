"""NumPy restatement of the candidate views (include/isdf_accel.h, "candidate views") built only from code that is older than them:
engine._raycast_ticks for the quantisation, engine.raycast_host for the line of sight, known_reference.unpack for K, a NumPy slice for the
clearance cube, the pose formula in scalar np.float64 operations in the header's order, engine.view_gain_host for the gain rows and a
lexsort on (-gain, k) for the selection.  Nothing here calls isdf_view_candidates*."""
import numpy as np

import known_reference as kr

KEPT, BAD, OCCUPIED, UNKNOWN, CLOSE, BLOCKED = range(6)
INFO_WORDS = ("n_targets", "n_offsets", "n_candidates", "n_kept", "n_bad", "n_occupied", "n_unknown", "n_close", "n_blocked", "n_scored", "best_target",
              "best_candidate", "best_gain")


def pose_of(eye, target):
    """the header's formula, one np.float64 operation at a time"""
    f = np.float64
    ex, ey, ez = (f(v) for v in eye)
    dx, dy, dz = f(target[0]) - ex, f(target[1]) - ey, f(target[2]) - ez
    n2 = dx * dx + dy * dy + dz * dz
    n = np.sqrt(n2)
    zx, zy, zz = dx / n, dy / n, dz / n
    x0 = [zy, -zx, f(0.0)]
    h = np.sqrt(x0[0] * x0[0] + x0[1] * x0[1])
    second = bool(h <= f(1e-9))
    if second:
        x0 = [f(0.0), zz, -zy]
        h = np.sqrt(x0[1] * x0[1] + x0[2] * x0[2])
    xx, xy, xz = x0[0] / h, x0[1] / h, x0[2] / h
    yx, yy, yz = zy * xz - zz * xy, zz * xx - zx * xz, zx * xy - zy * xx
    return np.array([xx, yx, zx, ex, xy, yy, zy, ey, xz, yz, zz, ez], dtype=np.float64), second


def candidates(engine, lib, bits, occ, bmin, bmax, res, cam, targets, offsets, clearance_voxels=1, k_best=3, min_gain=1, **gain):
    """(cand int64 [n, 8], poses float64 [n, 12], target rows int64 [n_targets, 8], best int64 [n_targets, k_best], info dict of
    INFO_WORDS, the number of kept candidates that took the pose's second branch)"""
    occ = np.ascontiguousarray(occ, dtype=np.uint8)
    dims = occ.shape
    k = kr.unpack(bits, dims)
    bmin, bmax = np.asarray(bmin, dtype=np.float64), np.asarray(bmax, dtype=np.float64)
    T = np.asarray(targets, dtype=np.float64).reshape(-1, 3)
    O = np.asarray(offsets, dtype=np.float64).reshape(-1, 3)
    nt, no = len(T), len(O)
    n = nt * no
    cand = np.zeros((n, 8), dtype=np.int64)
    poses = np.zeros((n, 12), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        tgt = np.repeat(T, no, axis=0)
        eye = tgt + np.tile(O, (nt, 1))
        d = tgt - eye
        n2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        finite = np.isfinite(tgt).all(axis=1) & np.isfinite(eye).all(axis=1)
    qt, in_t = engine._raycast_ticks(np.where(finite[:, None], tgt, bmin - 1.0), bmin, bmax, res, dims)
    qe, in_e = engine._raycast_ticks(np.where(finite[:, None], eye, bmin - 1.0), bmin, bmax, res, dims)
    bad = ~finite | ~in_t | ~in_e | (n2 == 0.0) | ~np.isfinite(n2)
    ve, vt = qe >> 10, qt >> 10
    status = np.full(n, -1, dtype=np.int64)
    status[bad] = BAD
    cand[:, 1] = np.where(bad, -1, (ve[:, 0] * dims[1] + ve[:, 1]) * dims[2] + ve[:, 2])
    cand[:, 2] = -1
    r = int(clearance_voxels)
    for c in np.flatnonzero(~bad):
        v = tuple(int(a) for a in ve[c])
        if occ[v] != 0:
            status[c] = OCCUPIED
        elif not k[v]:
            status[c] = UNKNOWN
        else:
            box = tuple(slice(max(a - r, 0), min(a + r, m - 1) + 1) for a, m in zip(v, dims))
            if (occ[box] != 0).any() or not k[box].all():
                status[c] = CLOSE
    walk = np.flatnonzero(status == -1)
    if len(walk):
        # a float32 point at the centre of the target's tick: the older cast takes float32 ends, and this one has the target's ticks
        ends = (((qt[walk] + 0.5) / 1024.0) * np.float64(res) + bmin).astype(np.float32)
        again, inside = engine._raycast_ticks(ends.astype(np.float64), bmin, bmax, res, dims)
        assert inside.all() and np.array_equal(again, qt[walk]), "the tick centres are not float32 values on this map"
        rows, _ = engine.raycast_host(occ, bmin, bmax, res, eye[walk], ends, test_origin_voxel=False, per_ray_origin=True, lib=lib)
        assert (rows[:, 0] <= 1).all()
        cand[walk, 2] = rows[:, 1]
        blocked = (rows[:, 0] == 1) & (rows[:, 2:5] != vt[walk]).any(axis=1)
        status[walk] = np.where(blocked, BLOCKED, KEPT)
    cand[:, 0] = status
    kept = np.flatnonzero(status == KEPT)
    second = 0
    for c in kept:
        poses[c], br = pose_of(eye[c], tgt[c])
        second += br
        assert np.allclose(poses[c], engine.look_at(eye[c], tgt[c]), rtol=0.0, atol=1e-12)
    if len(kept):
        g, _ = engine.view_gain_host(bits, occ, bmin, bmax, res, cam, poses[kept], lib=lib, **gain)
        assert (g[:, 0] == 0).all()
        cand[kept, 3], cand[kept, 4], cand[kept, 5], cand[kept, 6] = g[:, 1], g[:, 4], g[:, 5], g[:, 6]
    cand[:, 7] = -1
    rows_t = np.zeros((nt, 8), dtype=np.int64)
    best = np.full((nt, int(k_best)), -1, dtype=np.int64)
    for i in range(nt):
        s = status[i * no:(i + 1) * no]
        rows_t[i, :6] = [(s == w).sum() for w in range(6)]
        gain_i = cand[i * no:(i + 1) * no, 3]
        q = np.flatnonzero((s == KEPT) & (gain_i >= int(min_gain)))
        q = q[np.lexsort((q, -gain_i[q]))][:int(k_best)]
        best[i, :len(q)] = i * no + q
        cand[i * no + q, 7] = np.arange(len(q))
        rows_t[i, 6:] = [i * no + q[0], gain_i[q[0]]] if len(q) else [-1, 0]
    info = {"n_targets": nt, "n_offsets": no, "n_candidates": n, "n_scored": len(kept), "best_target": -1, "best_candidate": -1, "best_gain": 0}
    for w, name in enumerate(("n_kept", "n_bad", "n_occupied", "n_unknown", "n_close", "n_blocked")):
        info[name] = int((status == w).sum())
    have = np.flatnonzero(rows_t[:, 6] >= 0)
    if len(have):
        i = have[np.lexsort((rows_t[have, 6], -rows_t[have, 7]))][0]
        info["best_target"], info["best_candidate"], info["best_gain"] = int(i), int(rows_t[i, 6]), int(rows_t[i, 7])
    return cand, poses, rows_t, best, info, second
