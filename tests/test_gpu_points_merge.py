"""The clearance report merged into the obstacle-point set on the device (isdf_points_merge_check) and the loop around it
(isdf_optimize_lbfgs_checked): optimise, check against the whole map, merge what the check found, again.

The merge must be what a user could do by hand before it existed - traj_check_points, a de-duplication by voxel id against
get_points in numpy, set_points - except that old points keep index, bytes and lastTstar and no point crosses PCIe.  The loop must
be the hand-written loop over the same four calls."""
import ctypes as C
import gc

import numpy as np
import pytest

from common import REL_TOL, assert_close, oracle_cost_function, small_world, traj

pytestmark = pytest.mark.gpu

SAFETY = 0.5
CONE = ((0.8, 0.3, 1.6), 1.9)                   # tests/test_gpu_swept_mesh.py
WORLD_SEED, TRAJ_SEED, TRAJ_N = 3, 43, 6        # the trajectory of tests/test_gpu_traj_check.py: it grazes obstacles
MERGE_MARGIN = 1.0                              # the merge tests' check margin (<= 2 safety_hor + 0.1): plenty of rows
ORIGIN = np.zeros(3)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _world(pkg):
    occ, esdf, res = small_world(pkg, seed=WORLD_SEED)
    T, cm = traj(pkg, occ, res, N=TRAJ_N, seed=TRAJ_SEED)
    return occ, esdf, res, T, cm


def _cfg(pkg, variant=None):
    capi = pkg.capi
    return pkg.synth.default_config(capi.V1_SWEPT if variant is None else variant, kernel_size=9, integral_intervs=16, safety_hor=SAFETY)


def _engine(pkg, occ, esdf, res, variant=None, devices=None):
    capi, synth = pkg.capi, pkg.synth
    eng = pkg.Engine(_cfg(pkg, variant), devices=devices)
    eng.set_shape(synth.make_shape("RoundedCone", params=CONE[0], bound_radius=CONE[1]))
    if esdf is not None:
        eng.set_grid(esdf, ORIGIN, res, capi.GRID_ESDF)
    eng.set_grid(occ, ORIGIN, res, capi.GRID_OCCUPANCY)
    return eng


def _voxel_ids(P, dims, res, origin=ORIGIN):
    """getGridIndex (Gridmap3D.cpp:135-175) restated: the voxel index (x * ny + y) * nz + z of every point, -1 outside the map"""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 3)
    dims = np.asarray(dims)
    bmax = origin + dims * res
    inside = np.all((P >= origin) & (P <= bmax), axis=1)
    idx = np.minimum(np.floor((P - origin) / res).astype(np.int64), dims - 1)
    ids = (idx[:, 0] * dims[1] + idx[:, 1]) * dims[2] + idx[:, 2]
    ids[~inside] = -1
    return ids


def _waypoints(cm, N):
    return np.asarray(cm).reshape(3, N, 6)[:, 1:, 0].T.copy()


def _ends(T, cm):
    """boundary states (3 x 3, columns pos / vel / acc) and inner waypoints of a trajectory given as (T, column-major coefficients)"""
    N = len(T)
    c = np.asarray(cm).reshape(3, N, 6)
    head = np.zeros((3, 3)); tail = np.zeros((3, 3))
    head[:, 0] = c[:, 0, 0]
    tail[:, 0] = sum(c[:, N - 1, p] * T[-1] ** p for p in range(6))
    return head, tail, _waypoints(cm, N)


def _restate(old, rows, dims, res, below=None):
    """the merge in numpy: (rows considered, rows appended, duplicates, points outside)"""
    keep = np.ones(len(rows), dtype=bool) if below is None else rows[:, 3] < below
    old_ids = _voxel_ids(old, dims, res)
    have = set(old_ids[old_ids >= 0].tolist())
    row_ids = _voxel_ids(rows[:, :3], dims, res)
    assert np.all(row_ids >= 0) and np.all(np.diff(row_ids) > 0)           # the report: in the map, ascending voxel index
    new = keep & ~np.isin(row_ids, list(have))
    return int(keep.sum()), rows[new, :3], int((keep & ~new).sum()), int((old_ids < 0).sum())


_SEQ = {}


def _sequence(pkg, fresh=False):
    """gathered points minus every third, a check at MERGE_MARGIN, one merge - run once and shared (fresh: run again on a new ctx)"""
    if "first" in _SEQ and not fresh:
        return _SEQ["first"]
    synth = pkg.synth
    occ, esdf, res, T, cm = _world(pkg)
    pts = synth.constraint_points(occ, ORIGIN, res, _waypoints(cm, TRAJ_N), half=4 * res * 1.5)
    old = np.ascontiguousarray(pts[np.arange(len(pts)) % 3 != 0])
    eng = _engine(pkg, occ, esdf, res)
    eng.set_points(old)
    rep = eng.traj_check(T, cm, margin=MERGE_MARGIN)
    rows = eng.traj_check_points()
    info = eng.points_merge_check()
    out = dict(eng=eng, occ=occ, esdf=esdf, res=res, T=T, cm=cm, old=old, rep=rep, rows=rows, info=info, merged=eng.get_points())
    _SEQ.setdefault("first", out)
    return out


# ---- 1. the merge equals its numpy restatement ---------------------------------------------------------------------------
def test_merge_equals_numpy_restatement(pkg, product_lib):
    s = _sequence(pkg)
    old, rows, info, merged = s["old"], s["rows"], s["info"], s["merged"]
    n_rows, tail, n_dup, n_out = _restate(old, rows, s["occ"].shape, s["res"])
    print(f"[points_merge] gathered-minus-a-third: M_before {info['M_before']} rows {info['n_rows']} added {info['n_added']} "
          f"duplicate {info['n_duplicate']} outside {info['n_outside']} M_after {info['M_after']} | numpy: rows {n_rows} added {len(tail)} "
          f"duplicate {n_dup} | {info['merge_ms']:.3f} ms")
    assert len(tail) > 0 and n_dup > 0, "the scenario must exercise both branches"
    assert info["M_before"] == len(old) and info["n_rows"] == n_rows == len(rows) == s["rep"]["n_below_margin"]
    assert info["n_added"] == len(tail) and info["n_duplicate"] == n_dup and info["n_outside"] == n_out == 0
    assert info["M_after"] == len(old) + len(tail) == len(merged)
    assert np.array_equal(_bits(merged[:len(old)]), _bits(old))
    assert np.array_equal(_bits(merged[len(old):]), _bits(tail))


# ---- 2. idempotent -------------------------------------------------------------------------------------------------------
def test_second_merge_adds_nothing(pkg, product_lib):
    s = _sequence(pkg)
    eng = s["eng"]
    again = eng.points_merge_check()
    assert again["n_added"] == 0 and again["n_duplicate"] == again["n_rows"] == s["info"]["n_rows"]
    assert again["M_before"] == again["M_after"] == s["info"]["M_after"]
    assert eng.get_points().tobytes() == s["merged"].tobytes()
    assert eng.traj_check_points().tobytes() == s["rows"].tobytes()          # the kept report stays


# ---- 3. the step after a merge is the step of that set ---------------------------------------------------------------------
def test_step_after_merge_is_the_step_of_the_merged_set(pkg, orc, product_lib):
    """Bitwise: both contexts take the same host path (asserted), so arithmetic and order are the same."""
    synth = pkg.synth
    occ, esdf, res, T, cm = _world(pkg)
    pts = synth.constraint_points(occ, ORIGIN, res, _waypoints(cm, TRAJ_N), half=4 * res * 1.5)
    old = np.ascontiguousarray(pts[np.arange(len(pts)) % 3 != 0])
    a = _engine(pkg, occ, esdf, res)
    a.set_points(old)
    ts_old = np.zeros(len(old))
    a.eval_single(T * 1.05, cm, tstar=ts_old)                # a step before the merge: scratch and lastTstar of the old set exist
    assert np.any(ts_old != 0.0)
    a.traj_check(T, cm, margin=MERGE_MARGIN)
    info = a.points_merge_check()
    assert info["n_added"] > 0
    merged = a.get_points()
    ts0 = np.concatenate([ts_old, np.zeros(info["n_added"])])
    b = _engine(pkg, occ, esdf, res)
    b.set_points(merged)
    # the ctx's own lastTstar (the callback's) survived the merge for the old points and is 0 for the new ones: a step that uses it
    # equals the fresh ctx's step given those values
    ci, gTi, gCi = a.eval_single(T, cm)
    ts_b = ts0.copy()
    cb, gTb, gCb = b.eval_single(T, cm, tstar=ts_b)
    assert a.host_path() == b.host_path()
    assert ci == cb and np.array_equal(_bits(gTi), _bits(gTb)) and np.array_equal(_bits(gCi), _bits(gCb))
    # ... and with the caller's array on both
    ts_a = ts0.copy()
    ca, gTa, gCa = a.eval_single(T, cm, tstar=ts_a)
    assert a.host_path() == b.host_path()
    print(f"[points_merge] step after merge: M {len(merged)} host path {a.host_path()} cost {ca!r} vs {cb!r} "
          f"max |dgradC| {np.abs(gCa - gCb).max():.3e} max |dt*| {np.abs(ts_a - ts_b).max():.3e}")
    assert ca == cb and np.array_equal(_bits(gTa), _bits(gTb)) and np.array_equal(_bits(gCa), _bits(gCb))
    assert np.array_equal(_bits(ts_a), _bits(ts_b))
    o = orc.Oracle(_cfg(pkg), threads=4)
    o.set_grid(occ, ORIGIN, res, pkg.capi.GRID_OCCUPANCY)
    o.set_shape(synth.make_shape("RoundedCone", params=CONE[0], bound_radius=CONE[1]))
    o.set_points(merged)
    c0, gT0, gC0, _ = o.eval(T, cm, tstar=ts0.copy())
    assert ca > 0 and abs(ca - c0) <= REL_TOL * abs(c0), (ca, c0)
    assert_close(gTa, gT0, "gradT after the merge"); assert_close(gCa, gC0, "gradC after the merge")


# ---- 4. empty start ------------------------------------------------------------------------------------------------------
def test_empty_start(pkg, orc, product_lib):
    capi, synth = pkg.capi, pkg.synth
    occ, esdf, res, T, cm = _world(pkg)
    eng = _engine(pkg, occ, esdf, res)
    eng.set_points(np.zeros((0, 3)))
    # a V1 step and the callback without a single obstacle point: no collision term
    c, gT, gC = eng.eval_single(T, cm)
    assert c == 0.0 and not gT.any() and not gC.any()
    ts = np.zeros(0)
    assert eng.eval_single(T, cm, tstar=ts)[0] == 0.0
    head, tail, way = _ends(T, cm)
    rho = 1.0
    eng.set_trajectory(TRAJ_N, head, tail, rho)
    x = eng.pack_variables(T * 0.5, way)
    cost, g = eng.cost_function(x)
    o2 = orc.Oracle(synth.default_config(capi.V3_ESDF_TILE, kernel_size=9, integral_intervs=16, safety_hor=SAFETY, enable_pos=0), threads=4)
    c0, g0 = oracle_cost_function(orc, [o2], head, tail, rho, x, TRAJ_N)
    assert np.isfinite(cost) and np.all(np.isfinite(g))
    assert abs(cost - c0) <= REL_TOL * abs(c0), (cost, c0)
    assert_close(g, g0, "g without obstacle points")
    assert eng.cost_parts()["swept"] == 0.0
    # check, merge: the set is the report
    rep = eng.traj_check(T, cm, margin=MERGE_MARGIN)
    rows = eng.traj_check_points()
    info = eng.points_merge_check()
    assert rep["n_below_margin"] == len(rows) > 0
    assert (info["M_before"], info["M_after"], info["n_rows"], info["n_added"], info["n_duplicate"], info["n_outside"]) == \
        (0, len(rows), len(rows), len(rows), 0, 0)
    assert np.array_equal(_bits(eng.get_points()), _bits(rows[:, :3]))
    assert eng.eval_single(T, cm)[0] > 0.0                  # and the step charges them


# ---- 5. arbitrary existing points, `below` ----------------------------------------------------------------------------------
def test_arbitrary_points_and_below(pkg, product_lib):
    occ, esdf, res, T, cm = _world(pkg)
    eng = _engine(pkg, occ, esdf, res)
    eng.set_points(np.zeros((0, 3)))
    eng.traj_check(T, cm, margin=MERGE_MARGIN)
    rows = eng.traj_check_points()
    vals = np.unique(rows[:, 3])
    assert len(vals) >= 4
    below = 0.5 * (vals[len(vals) // 2 - 1] + vals[len(vals) // 2])          # between two row values
    jmin = int(np.argmin(rows[:, 3]))                                       # a row that `below` includes
    old = np.array([rows[jmin, :3] + np.array([0.2, -0.2, 0.1]),            # off-centre inside that row's voxel
                    [-5.0, 3.0, 3.0],                                       # outside the grid: occupies no voxel
                    [3.0, 3.0, 1e6]])
    assert _voxel_ids(old[:1], occ.shape, res)[0] == _voxel_ids(rows[jmin:jmin + 1, :3], occ.shape, res)[0]
    eng.set_points(old)
    info = eng.points_merge_check(below=below)
    n_rows, tail, n_dup, n_out = _restate(old, rows, occ.shape, res, below=below)
    print(f"[points_merge] below {below!r}: rows {info['n_rows']} of {len(rows)} added {info['n_added']} duplicate {info['n_duplicate']} "
          f"outside {info['n_outside']}")
    assert 0 < n_rows < len(rows) and n_dup == 1 and n_out == 2
    assert n_rows == int((rows[:, 3] < below).sum())
    assert (info["n_rows"], info["n_added"], info["n_duplicate"], info["n_outside"]) == (n_rows, len(tail), 1, 2)
    got = eng.get_points()
    assert np.array_equal(_bits(got[:3]), _bits(old)) and np.array_equal(_bits(got[3:]), _bits(tail))
    want = rows[(rows[:, 3] < below) & (np.arange(len(rows)) != jmin), :3]
    assert np.array_equal(_bits(tail), _bits(want))
    # the rest of the report with the default: everything not yet in the set, the blocked voxel still blocked
    info2 = eng.points_merge_check()
    assert info2["n_rows"] == len(rows) and info2["n_added"] == len(rows) - n_rows and info2["n_duplicate"] == n_rows
    assert np.array_equal(_bits(eng.get_points()[3 + len(tail):]), _bits(rows[~(rows[:, 3] < below), :3]))


def test_points_outside_in_every_wavefront_of_two_workgroups(pkg, product_lib):
    """the mark kernel's count of the points outside the grid, past one workgroup: 300 points (256 + 44: the second workgroup's only
    wavefront is part filled), every third one outside, so every wavefront of both workgroups counts some"""
    occ, esdf, res, T, cm = _world(pkg)
    eng = _engine(pkg, occ, esdf, res)
    eng.set_points(np.zeros((0, 3)))
    eng.traj_check(T, cm, margin=MERGE_MARGIN)
    rows = eng.traj_check_points()
    old = np.random.default_rng(300).uniform(0.05, 0.95, (300, 3)) * np.array(occ.shape) * res + np.array(ORIGIN)
    old[::3, 0] = np.array(ORIGIN)[0] - 1.0 - old[::3, 0]
    eng.set_points(old)
    info = eng.points_merge_check()
    n_rows, tail, n_dup, n_out = _restate(old, rows, occ.shape, res)
    assert n_out == 100 and n_rows == len(rows) > 0
    assert (info["M_before"], info["n_rows"], info["n_added"], info["n_duplicate"], info["n_outside"]) == (300, n_rows, len(tail), n_dup, 100)
    got = eng.get_points()
    assert np.array_equal(_bits(got[:300]), _bits(old)) and np.array_equal(_bits(got[300:]), _bits(tail))


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------
def test_refusals(pkg, product_lib):
    capi = pkg.capi
    occ, esdf, res, T, cm = _world(pkg)
    eng = _engine(pkg, occ, esdf, res)

    def refused(e, code, word):
        with pytest.raises(pkg.IsdfError) as ei:
            e.points_merge_check()
        assert ei.value.code == code and word in str(ei.value), str(ei.value)
    refused(eng, capi.ISDF_ERR_STATE, "report")                              # never checked
    eng.traj_check(T, cm, margin=MERGE_MARGIN)
    eng.traj_check_release()
    refused(eng, capi.ISDF_ERR_STATE, "report")                              # released
    eng.traj_check(T, cm, margin=MERGE_MARGIN)
    eng.set_grid(occ, ORIGIN, res, capi.GRID_OCCUPANCY)
    refused(eng, capi.ISDF_ERR_STATE, "older")                               # the grid replaced after the check
    assert eng.get_points().shape[0] == 0
    eng.traj_check(T, cm, margin=MERGE_MARGIN)
    cloud = ((np.argwhere(occ != 0) + 0.5) * res).astype(np.float32)
    eng.set_pointcloud(cloud, res, sta_threshold=1, bmin=(0, 0, 0), bmax=np.array(occ.shape) * res)
    refused(eng, capi.ISDF_ERR_STATE, "older")
    eng.traj_check(T, cm, margin=MERGE_MARGIN)
    assert eng.points_merge_check()["n_added"] > 0                           # checked again: accepted
    with pytest.raises(pkg.IsdfError) as ei:
        eng.points_merge_check(below=float("nan"))
    assert ei.value.code == capi.ISDF_ERR_INVALID_ARG and "below" in str(ei.value)
    multi = _engine(pkg, occ, esdf, res, devices=[0, 0])
    refused(multi, capi.ISDF_ERR_UNSUPPORTED, "multi-device")
    # the driver: a V1 ctx, a trajectory, an occupancy grid
    head, tail, way = _ends(T, cm)
    v3 = _engine(pkg, occ, esdf, res, variant=capi.V3_ESDF_TILE)
    v3.set_trajectory(TRAJ_N, head, tail, 1.0)
    x0 = v3.pack_variables(T, way)
    with pytest.raises(pkg.IsdfError) as ei:
        v3.optimize_lbfgs_checked(x0)
    assert ei.value.code == capi.ISDF_ERR_UNSUPPORTED
    v1 = pkg.Engine(_cfg(pkg))
    v1.set_shape(pkg.synth.make_shape("RoundedCone", params=CONE[0], bound_radius=CONE[1]))
    with pytest.raises(pkg.IsdfError) as ei:
        v1.optimize_lbfgs_checked(x0)
    assert ei.value.code == capi.ISDF_ERR_STATE and "isdf_set_trajectory" in str(ei.value)
    v1.set_trajectory(TRAJ_N, head, tail, 1.0)
    with pytest.raises(pkg.IsdfError) as ei:
        v1.optimize_lbfgs_checked(x0)
    assert ei.value.code == capi.ISDF_ERR_STATE and "occupancy" in str(ei.value)
    for kw in (dict(max_rounds=0), dict(mode=2), dict(below=float("inf"))):
        with pytest.raises(pkg.IsdfError) as ei:
            eng.optimize_lbfgs_checked(x0, **kw)
        assert ei.value.code == capi.ISDF_ERR_INVALID_ARG


# ---- 7. two runs, same bytes ---------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bytes(pkg, product_lib):
    a, b = _sequence(pkg), _sequence(pkg, fresh=True)
    assert a["eng"] is not b["eng"]
    assert a["merged"].tobytes() == b["merged"].tobytes() and a["rows"].tobytes() == b["rows"].tobytes()
    for k in a["info"]:
        if k != "merge_ms":
            assert a["info"][k] == b["info"][k], k


# ---- 8. the driver equals the hand-written loop --------------------------------------------------------------------------------
LBFGS = dict(max_iterations=8, g_epsilon=0.0, past=0)


def _hand_loop(eng, x0, N, max_rounds, margin=None, below=None, lbfgs=LBFGS):
    x = np.array(x0, dtype=np.float64)
    out = dict(rounds=0, clear=False, stalled=False, M_round=[])
    for _ in range(max_rounds):
        out["M_round"].append(eng.get_points().shape[0])
        out["rounds"] += 1
        x, out["last_opt"] = eng.optimize_lbfgs(x, **lbfgs)
        T, cm = eng.unpack_variables(x)
        out["last_check"] = eng.traj_check(T, cm, margin=margin)
        if out["last_check"]["n_below_margin"] == 0:
            out["clear"] = True
            break
        if eng.points_merge_check(below=below)["n_added"] == 0:
            out["stalled"] = True
            break
    return x, out


def test_driver_equals_the_hand_written_loop(pkg, product_lib):
    """The final x is compared bitwise: the driver makes the same four calls in the same order."""
    synth = pkg.synth
    occ, esdf, res, T, cm = _world(pkg)
    head, tail, way = _ends(T, cm)
    pts = synth.constraint_points(occ, ORIGIN, res, way, half=4 * res * 1.5)
    old = np.ascontiguousarray(pts[np.arange(len(pts)) % 3 != 0])
    got = []
    for by_hand in (False, True):
        eng = _engine(pkg, occ, esdf, res)
        eng.set_points(old)
        eng.set_trajectory(TRAJ_N, head, tail, 1.0)
        x0 = eng.pack_variables(T, way)
        if by_hand:
            x, r = _hand_loop(eng, x0, TRAJ_N, 3, margin=MERGE_MARGIN)
        else:
            x, r = eng.optimize_lbfgs_checked(x0, lbfgs_params=LBFGS, max_rounds=3, margin=MERGE_MARGIN)
        got.append((x, r, eng.get_points(), eng.traj_check_points()))
    (xa, ra, pa, rowsa), (xb, rb, pb, rowsb) = got
    rel = np.abs(xa - xb).max() / max(np.abs(xb).max(), 1e-300)
    print(f"[points_merge] driver vs loop: rounds {ra['rounds']} / {rb['rounds']} M_round {ra['M_round']} / {rb['M_round']} "
          f"clear {ra['clear']} stalled {ra['stalled']} max rel |dx| {rel:.3e} final M {len(pa)}")
    assert ra["rounds"] == rb["rounds"] and ra["M_round"] == rb["M_round"] and ra["clear"] == rb["clear"] and ra["stalled"] == rb["stalled"]
    assert ra["rounds"] >= 2 and ra["M_round"][1] > ra["M_round"][0] == len(old), "the loop must have merged at least once"
    assert np.array_equal(_bits(xa), _bits(xb))
    assert pa.tobytes() == pb.tobytes() and rowsa.tobytes() == rowsb.tobytes()           # the last check's rows stay kept
    for k in ("f", "status", "iterations", "evaluations"):
        assert ra["last_opt"][k] == rb["last_opt"][k], k
    for k in ("n_below_margin", "n_penetrating", "min_clearance", "min_voxel", "candidates"):
        assert ra["last_check"][k] == rb["last_check"][k], k


# ---- 9. loop invariants, lazy start -------------------------------------------------------------------------------------------
def test_loop_invariants_on_the_random_world_lazy_start(pkg, product_lib):
    occ, esdf, res, T, cm = _world(pkg)
    head, tail, way = _ends(T, cm)
    eng = _engine(pkg, occ, esdf, res)
    eng.set_points(np.zeros((0, 3)))
    eng.set_trajectory(TRAJ_N, head, tail, 1.0)
    max_rounds = 4
    x, r = eng.optimize_lbfgs_checked(eng.pack_variables(T, way), lbfgs_params=LBFGS, max_rounds=max_rounds)
    rows = eng.traj_check_points()
    pts = eng.get_points()
    print(f"[points_merge] lazy start, random world: rounds {r['rounds']} M_round {r['M_round']} final M {len(pts)} clear {r['clear']} "
          f"stalled {r['stalled']} below {r['last_check']['n_below_margin']} penetrating {r['last_check']['n_penetrating']} "
          f"min {r['last_check']['min_clearance']!r}")
    assert r["M_round"][0] == 0 and len(r["M_round"]) == r["rounds"] and np.all(np.diff(r["M_round"]) >= 0)
    assert 1 <= r["rounds"] <= max_rounds
    assert not (r["clear"] and r["stalled"])
    assert r["clear"] or r["stalled"] or r["rounds"] == max_rounds
    assert len(rows) == r["last_check"]["n_below_margin"]
    if r["clear"]:
        T1, cm1 = eng.unpack_variables(x)
        assert eng.traj_check(T1, cm1)["n_below_margin"] == 0 and len(rows) == 0
    else:
        assert len(rows) > 0
    if r["stalled"] or (not r["clear"] and r["rounds"] == max_rounds):
        # the last merge ran (or found nothing to add): every last-check row's voxel is in the set
        have = _voxel_ids(pts, occ.shape, res)
        assert np.all(np.isin(_voxel_ids(rows[:, :3], occ.shape, res), have))


# ---- 10. the loop repairs a plan -------------------------------------------------------------------------------------------
BOX_LO, BOX_EDGE = (22, 23, 14), 5          # voxels: a cube of 5 voxels edge, its centre 1.5 voxels beside the straight line
LINE_Y, LINE_Z = 12.0, 8.25                 # metres: the straight line runs along x through (., 12.0, 8.25); the box centre is at y = 12.75


def _box_scene(pkg):
    synth = pkg.synth
    res = 0.5
    occ = np.zeros((48, 48, 32), dtype=np.uint8)
    occ[BOX_LO[0]:BOX_LO[0] + BOX_EDGE, BOX_LO[1]:BOX_LO[1] + BOX_EDGE, BOX_LO[2]:BOX_LO[2] + BOX_EDGE] = 1
    esdf = synth.esdf_from_occupancy(occ, res)
    N = 4
    head = np.zeros((3, 3)); tail = np.zeros((3, 3))
    head[:, 0] = (4.0, LINE_Y, LINE_Z); tail[:, 0] = (20.5, LINE_Y, LINE_Z)
    way = np.linspace(head[:, 0], tail[:, 0], N + 1)[1:-1]
    return occ, esdf, res, N, head, tail, way, np.full(N, 1.5)


REPAIR_LBFGS = dict(max_iterations=40, g_epsilon=1e-6, past=0)


def test_loop_repairs_a_plan(pkg, product_lib):
    occ, esdf, res, N, head, tail, way, T0 = _box_scene(pkg)
    rho = 1.0
    # precondition (no merge involved): optimised without a single obstacle point, the trajectory goes through the box
    pre = _engine(pkg, occ, esdf, res)
    pre.set_points(np.zeros((0, 3)))
    pre.set_trajectory(N, head, tail, rho)
    x0 = pre.pack_variables(T0, way)
    x1, _ = pre.optimize_lbfgs(x0, **REPAIR_LBFGS)
    first = pre.traj_check(*pre.unpack_variables(x1))
    assert first["n_penetrating"] > 0
    eng = _engine(pkg, occ, esdf, res)
    eng.set_points(np.zeros((0, 3)))
    eng.set_trajectory(N, head, tail, rho)
    x, r = eng.optimize_lbfgs_checked(x0, lbfgs_params=REPAIR_LBFGS, max_rounds=6)
    last = r["last_check"]
    print(f"[points_merge] repair: box {BOX_EDGE} voxels at {BOX_LO}, round 1 penetrating {first['n_penetrating']} min {first['min_clearance']!r} | "
          f"driver: rounds {r['rounds']} M_round {r['M_round']} clear {r['clear']} stalled {r['stalled']} penetrating {last['n_penetrating']} "
          f"below {last['n_below_margin']} min {last['min_clearance']!r} L-BFGS status {r['last_opt']['status']}")
    assert r["M_round"][0] == 0 and r["rounds"] >= 2
    assert last["n_penetrating"] == 0
    assert last["min_clearance"] > first["min_clearance"]


# ---- 11. lifetime --------------------------------------------------------------------------------------------------------------
def test_every_byte_comes_back(pkg, product_lib):
    lib = product_lib

    def live():
        out = (C.c_longlong * 2)()
        lib.isdf_debug_live_bytes(out)
        return int(out[0]), int(out[1])
    occ, esdf, res, T, cm = _world(pkg)
    head, tail, way = _ends(T, cm)
    _SEQ.clear()
    gc.collect()                                            # (engines other tests dropped go now, not in the middle of the count)
    before = live()
    eng = _engine(pkg, occ, esdf, res)
    eng.set_points(np.zeros((0, 3)))
    eng.traj_check(T, cm, margin=MERGE_MARGIN)
    assert eng.points_merge_check()["n_added"] > 0
    held = live()
    assert eng.points_merge_check()["n_added"] == 0
    assert live() == held, "a merge that adds nothing allocates nothing that stays"
    eng.set_trajectory(TRAJ_N, head, tail, 1.0)
    eng.optimize_lbfgs_checked(eng.pack_variables(T, way), lbfgs_params=LBFGS, max_rounds=2)
    assert live()[0] > before[0]
    eng.close()
    assert live() == before, "bytes still held after isdf_destroy (device, pinned)"
