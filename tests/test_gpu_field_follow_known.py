"""The gated cost-to-go field kept across fills, updates, clears, scans and depth images (isdf_frontend_field_set_known_follow, DESIGN
4.27) against references that are never the code under test: the expected field is the plain host Dijkstra (isdf_frontend_field_host) on a
table the TEST gates - table_new * E_ref, table_new as isdf_frontend_cspace_get gives it after the change, E_ref the NumPy erosion
(tests/known_erode_reference.py) of a K_ref evolved in NumPy (tests/known_reference.py) or merged from the scan's host sets
(isdf_scan_sets_host + isdf_known_merge_host).  Fields are compared byte for byte, and also with isdf_frontend_field_build_known on a
fresh ctx brought to the same map and K.  Every byte comparison is preceded by an assertion, on the references alone, that the expected
field differs from the expected field before the change (or, where nothing may change, that it does not).
The scene, the robot and the helpers are tests/test_gpu_field_known.py's: 24 x 20 x 70 voxels, kernel_size 5, 9 attitudes, the wall with
its gap, the baffle, K = the half z < 35."""
import ctypes as C

import numpy as np
import pytest

import field_reference as fr
import known_erode_reference as er
import known_reference as kr
import test_gpu_depth_cam as dc
import test_gpu_field_known as fk
import test_gpu_map_update as mu
from test_gpu_field_known import GOAL, GOAL_UNSEEN, N_ATT, SEEN, START
from test_gpu_map_update import BMAX, BMIN, DIMS, RES

pytestmark = pytest.mark.gpu

GROW = (0, 0, 0, 23, 19, 49)                    # case 1: the seen half grows to z < 50, over the baffle's top (z 14 .. 39)
UNSEE = (6, 0, 0, 10, 13, 13)                   # case 2: across the way under the baffle, y 0 .. 13 of it
SENSOR = fk._centre((3, 10, 30)) + np.array([0.11, -0.07, 0.13])       # the scans' origin: in the seen half, left of the baffle
INCR = mu.INCR


def _engine(pkg, follow=1):
    eng = fk._engine(pkg)
    eng.frontend_field_set_known_follow(follow)
    return eng


def _expect(pkg, lib, eng, k, r, border, goal=GOAL):
    """(free', d, reachable, E) of the ctx's table as it stands, gated by the test with the NumPy erosion of k"""
    table = eng.frontend_cspace_table()
    e = er.erode(k, fk._radius(r), border)
    d, reach = pkg.frontend_field_host(table * e[..., None].astype(np.uint32), goal, N_ATT, lib=lib)
    return table.any(axis=3) & e, d, reach, e


def _differs(a, b):
    return not fr.same_bytes(a, b)


def _follows(eng, want, k, opening, closing):
    """the followed field has the expected bytes and counts; the follow info names the stages"""
    free, d, reach, e = want
    assert fr.same_bytes(eng.frontend_field(), d)
    f = eng.frontend_field_follow_info()
    assert (f.opening, f.closing) == (opening, closing)
    assert (f.known_voxels, f.eroded_voxels, f.free_voxels, f.reached_voxels) == (int(k.sum()), int(e.sum()), int(free.sum()), int(np.isfinite(d).sum()))
    assert (f.reachable, f.status) == (int(reach), 0 if reach else 1) and f.erode_ms >= 0.0 and f.device_ms > 0.0
    assert np.array_equal(eng.map_known()[0], kr.pack(k))
    return f


def _fresh(pkg, steps, k, r, border, goal=GOAL):
    """frontend_field_build_known on a fresh ctx brought to the same map and K by the same calls, no field in their way"""
    eng = fk._engine(pkg)
    for step in steps:
        step(eng)
    assert np.array_equal(eng.map_known()[0], kr.pack(k))
    eng.frontend_field_build_known(fk._centre(goal), r, border)
    return eng


def _box_ends(lo, hi):
    """the centre of every cell of the inclusive box, as ray end points"""
    g = np.stack(np.meshgrid(*[np.arange(a, b + 1) for a, b in zip(lo, hi)], indexing="ij"), axis=-1).reshape(-1, 3)
    return fk._centre(g).astype(np.float32)


def _merged(pkg, lib, k, origin, ends, hit):
    """K after a scan, from the scan's host sets"""
    free, hits, _ = pkg.engine.scan_sets_host(BMIN, BMAX, RES, DIMS, origin, ends, hit, lib=lib)
    words, newly = pkg.engine.known_merge_host(kr.pack(k), DIMS, free, hits, lib=lib)
    return kr.unpack(words, DIMS), newly


# ---- case 1: a fill grows K
@pytest.mark.parametrize("r,border", fk.CASES)
def test_a_fill_that_grows_k_opens_the_field(pkg, product_lib, r, border):
    table, k0, fields, _ = fk.shared(pkg, product_lib)
    e0, d0, reach0 = fields[(r, border)]
    eng = _engine(pkg)
    info, _ = eng.frontend_field_build_known(fk._centre(GOAL), r, border)
    assert info.reachable == 1
    with pytest.raises(pkg.IsdfError) as err:
        eng.frontend_field_follow_info()
    assert err.value.code == pkg.capi.ISDF_ERR_STATE            # no followed change since the build
    eng.map_known_fill(GROW, 1)
    k1 = kr.fill(k0, GROW, 1)
    want = _expect(pkg, product_lib, eng, k1, r, border)
    free1, d1, reach1, e1 = want
    free0 = table.any(axis=3) & e0
    # on the references alone: the way over the baffle's top opens
    assert _differs(d1, d0) and d1[START] < d0[START] and (np.isinf(d0) & np.isfinite(d1)).sum() > 1000
    f = _follows(eng, want, k1, 1, 0)
    assert (f.opened_voxels, f.closed_voxels, f.radius_used, f.border) == (int((free1 & ~free0).sum()), 0, fk._radius(r), border)
    o = eng.frontend_field_reopen_info()
    assert (o.opened_voxels, o.goal_opened, o.reached_voxels) == (f.opened_voxels, 0, f.reached_voxels)
    assert eng.frontend_field_known_info() == (1, fk._radius(r), border)
    if (r, border) in (fk.CASES[0], fk.CASES[-1]):
        fresh = _fresh(pkg, [lambda e: e.map_known_fill(GROW, 1)], k1, r, border)
        assert fr.same_bytes(fresh.frontend_field(), eng.frontend_field())
    # a second fill that sets nothing new: no stage, the report of the last followed call stays
    eng.map_known_fill((0, 0, 0, 5, 5, 5), 1)
    assert fr.same_bytes(eng.frontend_field(), d1) and eng.frontend_field_follow_info().opened_voxels == f.opened_voxels


# ---- case 2: a fill shrinks K
@pytest.mark.parametrize("r,border", [(-1, 0), (0, 1)])
def test_a_fill_that_shrinks_k_closes_the_field(pkg, product_lib, r, border):
    table, k0, fields, _ = fk.shared(pkg, product_lib)
    e0, d0, reach0 = fields[(r, border)]
    eng = _engine(pkg)
    eng.frontend_field_build_known(fk._centre(GOAL), r, border)
    eng.map_known_fill(UNSEE, 0)
    k1 = kr.fill(k0, UNSEE, 0)
    want = _expect(pkg, product_lib, eng, k1, r, border)
    free1, d1, reach1, e1 = want
    free0 = table.any(axis=3) & e0
    closed = free0 & ~free1
    # on the references alone: the start's way under the baffle is longer or gone, and a reached voxel closed (tau is finite, the reset runs)
    assert _differs(d1, d0) and (d1[START] > d0[START] or np.isinf(d1[START])) and np.isfinite(d0[START]) and np.isfinite(d0[closed]).any()
    f = _follows(eng, want, k1, 0, 1)
    assert (f.opened_voxels, f.closed_voxels) == (0, int(closed.sum()))
    rep = eng.frontend_field_repair_info()
    assert rep.closed_voxels == f.closed_voxels and rep.closed_reached == int(np.isfinite(d0[closed]).sum()) and np.isfinite(rep.tau) and rep.reset_voxels > 0
    fresh = _fresh(pkg, [lambda e: e.map_known_fill(UNSEE, 0)], k1, r, border)
    assert fr.same_bytes(fresh.frontend_field(), eng.frontend_field())


# ---- case 3: the goal unseen at the build, revealed, unseen again
def test_a_goal_revealed_and_unseen_again(pkg, product_lib):
    _, k0, _, _ = fk.shared(pkg, product_lib)
    reveal, hide = (0, 0, 0, 23, 19, 57), (19, 8, 48, 23, 12, 52)
    eng = _engine(pkg)
    info, _ = eng.frontend_field_build_known(fk._centre(GOAL_UNSEEN))
    assert (info.reachable, info.status) == (0, 1)
    d0 = _expect(pkg, product_lib, eng, k0, -1, 0, GOAL_UNSEEN)[1]
    assert np.isinf(d0).all()
    eng.map_known_fill(reveal, 1)
    k1 = kr.fill(k0, reveal, 1)
    want = _expect(pkg, product_lib, eng, k1, -1, 0, GOAL_UNSEEN)
    assert _differs(want[1], d0) and want[2] and want[1][GOAL_UNSEEN] == 0.0 and np.isfinite(want[1][START])
    f = _follows(eng, want, k1, 1, 0)
    o = eng.frontend_field_reopen_info()
    assert (f.reachable, o.goal_opened, o.reachable, o.reached_before) == (1, 1, 1, 0)
    fresh = _fresh(pkg, [lambda e: e.map_known_fill(reveal, 1)], k1, -1, 0, GOAL_UNSEEN)
    assert fr.same_bytes(fresh.frontend_field(), eng.frontend_field())
    # the reverse: the goal's cube unseen
    eng.map_known_fill(hide, 0)
    k2 = kr.fill(k1, hide, 0)
    want2 = _expect(pkg, product_lib, eng, k2, -1, 0, GOAL_UNSEEN)
    assert _differs(want2[1], want[1]) and not want2[2] and np.isinf(want2[1]).all()
    f = _follows(eng, want2, k2, 0, 1)
    assert f.reachable == 0 and eng.frontend_field_paths(fk._centre(START)[None], 8)[0][0] == 0


# ---- case 4: the table changes, K fixed
def test_an_update_and_a_clear_are_followed_with_k_fixed(pkg, product_lib):
    _, k0, fields, _ = fk.shared(pkg, product_lib)
    d0 = fields[(-1, 0)][1]
    eng = _engine(pkg)
    eng.frontend_field_build_known(fk._centre(GOAL))
    words0 = eng.map_known()[0]
    gap = np.argwhere(np.ones((1, 4, 26), dtype=bool)) + (16, 6, 22)          # the wall's gap, y 6 .. 9 of it: closed
    hole = np.argwhere(np.ones((1, 5, 7), dtype=bool)) + (8, 8, 24)           # a hole in the baffle, in seen space: opened
    steps = []
    info = eng.update_voxels(gap, **INCR)
    steps.append(lambda e: e.update_voxels(gap, **INCR))
    want1 = _expect(pkg, product_lib, eng, k0, -1, 0)
    assert _differs(want1[1], d0) and (np.isfinite(d0) & np.isinf(want1[1])).any()
    assert (info.field_dropped, info.n_new_voxels) == (0, len(gap))
    f = _follows(eng, want1, k0, 0, 1)
    assert f.closed_voxels > 0 and eng.frontend_field_repair_info().closed_voxels == f.closed_voxels
    assert np.array_equal(eng.map_known()[0], words0)          # K is read, never written
    fresh = _fresh(pkg, steps, k0, -1, 0)
    assert fr.same_bytes(fresh.frontend_field(), eng.frontend_field())
    info = eng.clear_voxels(hole, **INCR)
    steps.append(lambda e: e.clear_voxels(hole, **INCR))
    want2 = _expect(pkg, product_lib, eng, k0, -1, 0)
    assert _differs(want2[1], want1[1]) and want2[1][START] < want1[1][START]
    assert (info.field_dropped, info.n_cleared_voxels) == (0, len(hole))
    f = _follows(eng, want2, k0, 1, 0)
    assert f.opened_voxels > 0 and eng.frontend_field_reopen_info().opened_voxels == f.opened_voxels
    assert np.array_equal(eng.map_known()[0], words0)
    fresh = _fresh(pkg, steps, k0, -1, 0)
    assert fr.same_bytes(fresh.frontend_field(), eng.frontend_field())


# ---- case 5: integrate_scan
def _scan_all_three():
    """(a): misses that fill a box of the unseen half above the sensor, misses that pass through the baffle (count 2, miss_weight 2: cleared),
    pairs of hits in free voxels of the seen half (threshold 2: newly occupied)"""
    up = _box_ends((0, 3, 35), (7, 16, 42))
    through = _box_ends((14, 8, 36), (14, 12, 44))
    cells = np.array([(6, 9, 33), (6, 10, 33), (6, 11, 33)])
    hits = np.concatenate([fk._centre(cells) - 0.05, fk._centre(cells) + 0.05]).astype(np.float32)
    ends = np.concatenate([up, through, hits])
    hit = np.concatenate([np.zeros(len(up) + len(through), dtype=np.uint8), np.ones(len(hits), dtype=np.uint8)])
    return ends, hit


def _scan_k_only():
    """(b): the misses into the unseen half alone - they pass and end in free voxels that no point was ever counted in"""
    up = _box_ends((0, 3, 35), (7, 16, 42))
    return up, np.zeros(len(up), dtype=np.uint8)


def _scan_inside():
    """(c): wholly inside known free space"""
    ends = _box_ends((1, 5, 20), (6, 15, 30))
    return ends, np.zeros(len(ends), dtype=np.uint8)


@pytest.mark.parametrize("r", [1, -1])
def test_scans_are_followed(pkg, product_lib, r):
    _, k0, fields, _ = fk.shared(pkg, product_lib)
    d0 = fields[(r, 0)][1]
    S = pkg.capi.ISDF_ERR_STATE
    # (c) and (d) first: nothing changes, the field is untouched and no stage is reported
    eng = _engine(pkg)
    eng.frontend_field_build_known(fk._centre(GOAL), r, 0)
    for ends, hit in (_scan_inside(), (np.zeros((0, 3), dtype=np.float32), np.zeros(0, dtype=np.uint8))):
        k1, newly = _merged(pkg, product_lib, k0, SENSOR, ends, hit)
        info = eng.integrate_scan(SENSOR, ends, hit, miss_weight=2, **INCR)
        want = _expect(pkg, product_lib, eng, k1, r, 0)
        assert newly == 0 and not _differs(want[1], d0)            # on the references alone: nothing to follow
        assert (info.clear.n_cleared_voxels, info.update.n_new_voxels, info.clear.field_dropped, info.update.field_dropped) == (0, 0, 0, 0)
        assert fr.same_bytes(eng.frontend_field(), d0) and eng.frontend_field_known_info() == (1, fk._radius(r), 0)
        with pytest.raises(pkg.IsdfError) as err:
            eng.frontend_field_follow_info()
        assert err.value.code == S
    # (b) on the same ctx: only K grows - the opening stage runs although no voxel was cleared
    ends, hit = _scan_k_only()
    k1, newly = _merged(pkg, product_lib, k0, SENSOR, ends, hit)
    info = eng.integrate_scan(SENSOR, ends, hit, miss_weight=2, **INCR)
    want = _expect(pkg, product_lib, eng, k1, r, 0)
    assert newly > 0 and _differs(want[1], d0) and (np.isinf(d0) & np.isfinite(want[1])).sum() > 0
    assert (info.clear.n_cleared_voxels, info.update.n_new_voxels, info.clear.field_dropped, info.update.field_dropped) == (0, 0, 0, 0)
    f = _follows(eng, want, k1, 1, 0)
    assert f.opened_voxels == int((want[0] & ~(fk.shared(pkg, product_lib)[0].any(axis=3) & fields[(r, 0)][0])).sum()) > 0
    fresh = _fresh(pkg, [lambda e: e.integrate_scan(SENSOR, ends, hit, miss_weight=2, **INCR)], k1, r, 0)
    assert fr.same_bytes(fresh.frontend_field(), eng.frontend_field())
    # (a) on a ctx of its own: K grows, baffle voxels are cleared, free voxels become occupied - an opening and a closing stage
    eng = _engine(pkg)
    eng.frontend_field_build_known(fk._centre(GOAL), r, 0)
    ends, hit = _scan_all_three()
    k1, newly = _merged(pkg, product_lib, k0, SENSOR, ends, hit)
    info = eng.integrate_scan(SENSOR, ends, hit, miss_weight=2, **INCR)
    want = _expect(pkg, product_lib, eng, k1, r, 0)
    assert newly > 0 and _differs(want[1], d0)
    assert info.clear.n_cleared_voxels > 0 and info.update.n_new_voxels == 3 and (info.clear.field_dropped, info.update.field_dropped) == (0, 0)
    f = _follows(eng, want, k1, 1, 1)
    assert f.opened_voxels > 0 and f.closed_voxels > 0
    assert eng.frontend_field_reopen_info().opened_voxels == f.opened_voxels and eng.frontend_field_repair_info().closed_voxels == f.closed_voxels
    fresh = _fresh(pkg, [lambda e: e.integrate_scan(SENSOR, ends, hit, miss_weight=2, **INCR)], k1, r, 0)
    assert fr.same_bytes(fresh.frontend_field(), eng.frontend_field())


# ---- case 6: a depth image
def test_a_depth_image_is_followed(pkg, product_lib):
    _, k0, fields, _ = fk.shared(pkg, product_lib)
    d0 = fields[(0, 0)][1]
    cam, p12, image = fk._empty_image(pkg)                          # no return anywhere: with no_return_is_free every pixel is a miss of max_range
    origin = np.array([5.2, 7.1, 14.0])
    eng = _engine(pkg)
    eng.frontend_field_build_known(fk._centre(GOAL), 0, 0)
    ends, hit, _ = dc._host_rays(pkg, product_lib, image, p12=p12, **dc.DEPTH_PARAMS)
    k1, newly = _merged(pkg, product_lib, k0, origin, ends, hit)
    _, info = eng.integrate_depth(cam, p12, image, **dc.DEPTH_PARAMS, **INCR)
    want = _expect(pkg, product_lib, eng, k1, 0, 0)
    assert newly > 0 and _differs(want[1], d0)
    assert (info.clear.field_dropped, info.update.field_dropped) == (0, 0)
    f = _follows(eng, want, k1, 1, 1 if info.update.n_new_voxels else 0)
    assert f.opened_voxels > 0
    fresh = _fresh(pkg, [lambda e: e.integrate_depth(cam, p12, image, **dc.DEPTH_PARAMS, **INCR)], k1, 0, 0)
    assert fr.same_bytes(fresh.frontend_field(), eng.frontend_field())


# ---- case 7: a sequence on one ctx
def test_a_sequence_of_changes_on_one_ctx(pkg, product_lib):
    _, k, fields, _ = fk.shared(pkg, product_lib)
    d_last = fields[(-1, 0)][1]
    eng = _engine(pkg)
    eng.frontend_field_build_known(fk._centre(GOAL))
    ends_a, hit_a = _scan_k_only()
    ends_b, hit_b = _scan_all_three()
    extra = mu._in_cells(np.array([(12, 10, 20), (12, 11, 20)]), 2, np.random.default_rng(9))      # two new occupied voxels between the baffle and the wall
    sensor_b = fk._centre((3, 10, 28)) + np.array([0.05, 0.02, -0.03])
    beside = (8, 0, 35, 15, 19, 40)          # the fill: above the seen half between the baffle and the wall, x 8 .. 15 - the first scan's rays stay in x 0 .. 7

    def scanned(k, sensor, ends, hit):
        k1, newly = _merged(pkg, product_lib, k, sensor, ends, hit)
        assert newly > 0                      # the scan follows a fill on this ctx and still has voxels of its own to make known
        return k1
    steps = [("fill", lambda e: e.map_known_fill(beside, 1), lambda k: kr.fill(k, beside, 1)),
             ("scan", lambda e: e.integrate_scan(SENSOR, ends_a, hit_a, miss_weight=2, **INCR), lambda k: scanned(k, SENSOR, ends_a, hit_a)),
             ("update", lambda e: e.update_pointcloud(extra, **INCR), lambda k: k),
             ("scan 2", lambda e: e.integrate_scan(sensor_b, ends_b, hit_b, miss_weight=2, **INCR), lambda k: scanned(k, sensor_b, ends_b, hit_b))]
    done = []
    for name, call, evolve in steps:
        call(eng)
        done.append(call)
        k = evolve(k)
        want = _expect(pkg, product_lib, eng, k, -1, 0)
        assert _differs(want[1], d_last), name          # on the references alone: every step has something to follow
        assert fr.same_bytes(eng.frontend_field(), want[1]), name
        assert np.array_equal(eng.map_known()[0], kr.pack(k)) and eng.frontend_field_known_info() == (1, mu.SIDE, 0), name
        d_last = want[1]
    fresh = _fresh(pkg, done, k, -1, 0)
    assert fr.same_bytes(fresh.frontend_field(), eng.frontend_field())
    rng = np.random.default_rng(5)
    reached = np.argwhere(np.isfinite(d_last) & (d_last > 0.0))
    starts = fk._centre(np.concatenate([[START], reached[rng.choice(len(reached), 10, replace=False)], [GOAL]]))
    assert fr.same_bytes(eng.frontend_field(starts), fresh.frontend_field(starts))
    got, want = eng.frontend_field_paths(starts, 256), fresh.frontend_field_paths(starts, 256)
    assert (got[0][:-1] > 1).all() and all(np.array_equal(a, b) for a, b in zip(got, want))


# ---- case 8: the drops and the modes
def test_what_still_drops_and_the_modes(pkg, product_lib):
    capi = pkg.capi
    goal_xyz = fk._centre(GOAL)
    extra = fk._centre([[5, 3, 5], [5, 3, 5]]).astype(np.float32)             # one new occupied voxel, in seen space
    eng = _engine(pkg)

    def build(**kw):
        info, _ = eng.frontend_field_build_known(goal_xyz, **kw)
        assert eng.frontend_field_known_info() == (1, mu.SIDE, 0)
        return info
    build()
    assert eng.shift_map((2, -3, 5)).field_dropped == 1
    fk._gone(pkg, eng)
    eng = _engine(pkg)
    build()
    assert eng.map_follow(fk._centre((14, 10, 36)))[1].field_dropped == 1
    fk._gone(pkg, eng)
    eng = _engine(pkg)
    build()
    assert eng.update_pointcloud(extra, refresh_frontend=False, **INCR).field_dropped == 1
    fk._gone(pkg, eng)
    eng = _engine(pkg)
    assert build(max_rounds=1).status == 2                        # not a fixed point: nothing to follow
    assert eng.update_pointcloud(extra, **INCR).field_dropped == 1
    fk._gone(pkg, eng)
    build()
    eng.map_known_enable(False)
    fk._gone(pkg, eng)
    # mode 0, set back, drops on a fill and on a scan
    eng = _engine(pkg)
    eng.frontend_field_set_known_follow(0)
    build()
    eng.map_known_fill(GROW, 1)
    fk._gone(pkg, eng)
    build()
    ends, hit = _scan_k_only()
    info = eng.integrate_scan(SENSOR, ends, hit, **INCR)
    assert (info.clear.field_dropped, info.update.field_dropped) == (1, 1)
    fk._gone(pkg, eng)
    # a bad mode, and the info before any follow
    for bad in (2, -1):
        assert eng.lib.isdf_frontend_field_set_known_follow(eng.h, bad) == capi.ISDF_ERR_INVALID_ARG
        assert "follow mode is 0 (drop) or 1 (follow in place)" in eng.lib.isdf_last_error(eng.h).decode()
    assert eng.lib.isdf_frontend_field_set_known_follow(None, 1) == capi.ISDF_ERR_INVALID_ARG
    eng.frontend_field_set_known_follow(1)
    build()
    with pytest.raises(pkg.IsdfError) as err:
        eng.frontend_field_follow_info()
    assert err.value.code == capi.ISDF_ERR_STATE
    assert eng.lib.isdf_frontend_field_follow_info(eng.h, None) == capi.ISDF_ERR_INVALID_ARG
    sz = (C.c_int * 1)()
    eng.lib.isdf_frontend_field_follow_sizes(sz)
    assert sz[0] == C.sizeof(capi.IsdfFieldFollowInfo)
    # an ungated field with follow mode 1 and the repair and reopen modes 0 is dropped on an update, as ever
    plain = _engine(pkg)
    assert plain.frontend_field_build(goal_xyz).reachable == 1
    assert plain.update_pointcloud(extra, **INCR).field_dropped == 1
    with pytest.raises(pkg.IsdfError) as err:
        plain.frontend_field()
    assert err.value.code == capi.ISDF_ERR_STATE
    # ... and the gated one beside it is followed whatever those modes say
    eng = _engine(pkg)
    build()
    k0 = fk.shared(pkg, product_lib)[1]
    d0 = fk.shared(pkg, product_lib)[2][(-1, 0)][1]
    assert eng.update_pointcloud(extra, **INCR).field_dropped == 0
    want = _expect(pkg, product_lib, eng, k0, -1, 0)
    assert _differs(want[1], d0)
    _follows(eng, want, k0, 0, 1)
