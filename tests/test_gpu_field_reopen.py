"""The cost-to-go field LOWERED in place by a map clear (isdf_frontend_field_set_reopen mode 1; csrc/frontend_field.hip, the rule in
include/isdf_accel.h and DESIGN 4.6.3) against a FRESH ctx that is given the map after the clear and builds its field from scratch - never
against the reopen itself.  Fields are compared BYTE FOR BYTE, paths node for node.  Set-up of tests/test_gpu_field_repair.py: 0.5 m
voxels, a ball smaller than a voxel (free = not occupied), kernel_size 5, 3 x 3 attitudes.  Shapes, the smallest at which each mechanism
can go wrong: 9 x 7 x 5 (less than one brick), 17 x 9 x 70 boxes (partial bricks in x and y, a second 64-lane z block; the opened voxels
straddle z = 63 / 64 and the brick edge x = 7 / 8, or touch the map's edge), the 24 x 24 x 3 serpentine (bricks left and re-entered)."""
import numpy as np
import pytest

import field_reference as fr
from test_gpu_field_repair import INCR, RES, MAX_ANG, ANG_RES, _boxes, _boxes_goal_low, _boxes_straddle, _centre, _live, _starts, _with

pytestmark = pytest.mark.gpu

FULL = {"max_cleared_voxels": 0}


def _prepare(pkg, eng, reopen, repair=None):
    eng.set_shape(pkg.synth.make_shape("Ball", params=(0.1,)))
    eng.frontend_build(pkg.capi.frontend_config(kernel_size=5, max_roll=MAX_ANG, max_pitch=MAX_ANG, ang_res=ANG_RES, safeh=0.0))
    if reopen is not None:
        eng.frontend_field_set_reopen(reopen)
    if repair is not None:
        eng.frontend_field_set_repair(repair)
    return eng


def _engine(pkg, occ, reopen=1, repair=None):
    eng = pkg.Engine(pkg.synth.default_config(pkg.capi.V1_SWEPT))
    eng.set_grid(np.ascontiguousarray(occ, dtype=np.uint8), (0, 0, 0), RES, pkg.capi.GRID_OCCUPANCY)
    return _prepare(pkg, eng, reopen, repair)


def _without(occ, cells):
    out = np.array(occ, dtype=np.uint8)
    for c in cells:
        assert out[tuple(c)] == 1, c
        out[tuple(c)] = 0
    return out


def _state_error(pkg, call):
    with pytest.raises(pkg.IsdfError) as err:
        call()
    assert err.value.code == pkg.capi.ISDF_ERR_STATE


def _hold_to_a_fresh_build(pkg, eng, occ_after, goal, clear_info, fresh=None):
    """the reopened ctx against a fresh one on the map after the clear: the field's bytes, 17 paths, the counts; returns (reopen info,
    field, the fresh build's info)"""
    fresh = fresh if fresh is not None else _engine(pkg, occ_after, reopen=None)
    finfo = fresh.frontend_field_build(_centre(goal))
    want = fresh.frontend_field()
    got = eng.frontend_field()
    r = eng.frontend_field_reopen_info()
    print(f"\nopened {r.opened_voxels} ({r.opened_reached} reached), goal opened {r.goal_opened}, reached {r.reached_before} -> {r.reached_voxels}, seeded {r.seeded_bricks}, "
          f"rounds {r.rounds} (build {finfo.rounds}), visits {r.brick_visits} (build {finfo.brick_visits}), {r.device_ms:.3f} ms (build {finfo.device_ms:.3f} ms)")
    assert clear_info.field_dropped == 0
    assert fr.same_bytes(got, want)
    assert np.isinf(got[np.asarray(occ_after) != 0]).all()
    assert (r.free_voxels, r.reached_voxels, r.reachable, r.status) == (finfo.free_voxels, finfo.reached_voxels, finfo.reachable, finfo.status)
    assert r.free_voxels == int((np.asarray(occ_after) == 0).sum()) and r.reached_voxels == int(np.isfinite(want).sum())
    starts = _starts(occ_after)
    cap = 48
    n, xyz, rp = eng.frontend_field_paths(starts, cap)
    n_f, xyz_f, rp_f = fresh.frontend_field_paths(starts, cap)
    assert np.array_equal(n, n_f) and np.array_equal(xyz, xyz_f) and np.array_equal(rp, rp_f)
    v = eng.frontend_field(starts)
    assert fr.same_bytes(v, fresh.frontend_field(starts))
    return r, got, finfo


# ---- 1. four voxels across the brick edge in x and the 64-lane split in z, both paths of the clear ------------------------------------
def test_opened_voxels_lower_a_part_only_on_both_paths(pkg, product_lib):
    occ = _boxes(pkg)
    goal = _boxes_goal_low(occ)
    four = _boxes_straddle(occ)
    before = _with(occ, four)
    fields = []
    for params, path in ((INCR, 1), (FULL, 2)):
        eng = _engine(pkg, before)
        binfo = eng.frontend_field_build(_centre(goal))
        _state_error(pkg, eng.frontend_field_reopen_info)            # no reopen since the build
        old = eng.frontend_field()
        assert all(np.isinf(old[c]) for c in four) and binfo.reachable == 1
        info = eng.clear_voxels(four, **params)
        assert info.path == path and info.n_cleared_voxels == 4
        r, got, finfo = _hold_to_a_fresh_build(pkg, eng, occ, goal, info)
        assert (r.opened_voxels, r.opened_reached, r.goal_opened) == (4, 4, 0) and r.reached_before == binfo.reached_voxels
        assert 0 < r.rounds and r.seeded_bricks == 4 and r.brick_visits >= r.seeded_bricks         # one brick on each side of x = 7 / 8 and of z = 63 / 64
        fin = np.isfinite(old)
        assert (old[fin] >= got[fin]).all()                          # every old finite value is an upper bound of the new one
        same = fin & (old.view(np.uint64) == got.view(np.uint64))
        assert same.sum() > 0 and got[goal] == 0.0                   # some values are the old ones: not a disguised rebuild
        fields.append(got)
        _state_error(pkg, eng.frontend_field_repair_info)            # a reopen is no repair
        eng.frontend_field_build(_centre(goal))                      # a new build forgets the reopen's report
        _state_error(pkg, eng.frontend_field_reopen_info)
    assert fr.same_bytes(fields[0], fields[1])


# ---- 2. the map's edge, and an opened voxel that nothing reaches ---------------------------------------------------------------------
def test_opened_voxel_at_the_maps_edge_and_one_with_only_inf_neighbours(pkg, product_lib):
    base = _boxes(pkg)
    base[10:13, 3:6, 30:33] = 1                                      # a solid 3 x 3 x 3 block: its centre's neighbours all stay occupied
    centre = (11, 4, 31)
    after = _without(base, [centre])
    goal = _boxes_goal_low(after)
    ref = fr.field(after == 0, goal)
    assert np.isinf(ref[centre]) and after[centre] == 0
    on_edge = np.zeros(after.shape, dtype=bool)
    on_edge[[0, -1], :, :] = on_edge[:, [0, -1], :] = on_edge[:, :, [0, -1]] = True
    cells = np.argwhere(on_edge & np.isfinite(ref))
    corner = tuple(int(v) for v in cells[np.argmax(cells.sum(axis=1))])          # the reached voxel of the map's faces nearest the far corner
    assert corner[2] >= 64 and corner != goal
    before = _with(after, [centre, corner])
    eng = _engine(pkg, before)
    eng.frontend_field_build(_centre(goal))
    old = eng.frontend_field()
    info = eng.clear_voxels([centre, corner], **INCR)
    assert info.path == 1 and info.n_cleared_voxels == 2
    r, got, _ = _hold_to_a_fresh_build(pkg, eng, after, goal, info)
    assert np.isinf(got[centre]) and np.isfinite(got[corner])
    assert (r.opened_voxels, r.opened_reached) == (2, 1)             # the centre opened, stays +inf and is not counted as reached
    assert r.reached_voxels >= r.reached_before + 1
    fin = np.isfinite(old)
    assert (old[fin] >= got[fin]).all()


# ---- 3. the serpentine: bricks left and re-entered -------------------------------------------------------------------------------------
def test_serpentine_shortcut_reactivates_bricks(pkg, product_lib):
    before = fr.serpentine((24, 24, 3))
    wall = (12, 11, 1)                                               # half-way along: the sixth of the eleven walls, far from its gap at x = 0
    after = _without(before, [wall])
    goal = (0, 0, 1)
    eng = _engine(pkg, before)
    binfo = eng.frontend_field_build(_centre(goal))
    old = eng.frontend_field()
    info = eng.clear_voxels([wall], **INCR)
    r, got, finfo = _hold_to_a_fresh_build(pkg, eng, after, goal, info)
    assert r.opened_voxels == r.opened_reached == 1 and r.reached_voxels == r.reached_before + 1 == binfo.reached_voxels + 1
    fell = (got < old) & np.isfinite(old)
    assert fell[:, 12:, :].any() and not fell[:, :11, :].any()       # the runs behind the wall get shorter, those before it keep their values
    assert fr.same_bytes(got[:, :11, :], old[:, :11, :])
    # every round relaxes a brick to its own fixed point, so the rounds count brick crossings of the lowered corridor (12 runs of 3
    # bricks), not voxels: more than two, and far below the bound of one round per free voxel
    assert 2 < r.rounds < r.free_voxels // 4 and r.brick_visits > r.seeded_bricks == 1
    assert fr.same_bytes(got, fr.field(after == 0, goal))


# ---- 4. less than one brick: the goal cell opens; or it does not -----------------------------------------------------------------------
def test_goal_cell_opened_and_goal_cell_kept_closed(pkg, product_lib):
    goal, other = (1, 5, 3), (4, 3, 2)
    before = _with(fr.open_map(), [goal, other])
    eng = _engine(pkg, before)
    binfo = eng.frontend_field_build(_centre(goal))
    assert (binfo.reachable, binfo.status, binfo.reached_voxels) == (0, 1, 0) and np.isinf(eng.frontend_field()).all()
    after = _without(before, [goal])
    info = eng.clear_voxels([goal], **INCR)
    r, got, _ = _hold_to_a_fresh_build(pkg, eng, after, goal, info)
    assert (r.goal_opened, r.reachable, r.status, r.opened_voxels, r.opened_reached, r.reached_before) == (1, 1, 0, 1, 1, 0)
    assert got[goal] == 0.0 and r.rounds >= 1 and fr.same_bytes(got, fr.field(after == 0, goal))
    n, _, _ = eng.frontend_field_paths([_centre((7, 1, 1))], 16)
    assert n[0] > 1
    # some other voxel instead: the field stays valid and all +inf, and nothing is relaxed
    eng = _engine(pkg, before)
    eng.frontend_field_build(_centre(goal))
    after = _without(before, [other])
    info = eng.clear_voxels([other], **INCR)
    r, got, _ = _hold_to_a_fresh_build(pkg, eng, after, goal, info)
    assert np.isinf(got).all() and (r.rounds, r.brick_visits, r.goal_opened, r.reachable, r.status) == (0, 0, 0, 0, 1)
    assert (r.opened_voxels, r.opened_reached, r.reached_voxels, r.seeded_bricks) == (1, 0, 0, 1)
    # ... and the goal after it: the reopen of a reopened field
    after = _without(after, [goal])
    info = eng.clear_voxels([goal], **INCR)
    r, got, _ = _hold_to_a_fresh_build(pkg, eng, after, goal, info)
    assert r.goal_opened == 1 and np.isfinite(got).all()


# ---- 5. a sealed pocket across the brick edge and the lane split --------------------------------------------------------------------------
def test_sealed_pocket_opened(pkg, product_lib):
    after = _boxes(pkg)
    after[4:9, 2:7, 60:67] = 1                                       # a closed one-voxel shell ...
    after[5:8, 3:6, 61:66] = 0                                       # ... around 3 x 3 x 5 cells on both sides of x = 7 / 8 and z = 63 / 64
    shell = (4, 4, 63)
    after[shell] = 0
    after[3, 4, 63] = 0                                              # the voxel outside the door is free
    before = _with(after, [shell])
    goal = _boxes_goal_low(after)
    eng = _engine(pkg, before)
    eng.frontend_field_build(_centre(goal))
    old = eng.frontend_field()
    assert np.isinf(old[5:8, 3:6, 61:66]).all() and np.isfinite(old[3, 4, 63])
    info = eng.clear_voxels([shell], **INCR)
    r, got, _ = _hold_to_a_fresh_build(pkg, eng, after, goal, info)
    assert np.isfinite(got[5:8, 3:6, 61:66]).all() and np.isfinite(got[shell])
    assert r.reached_voxels == r.reached_before + 46 and (r.opened_voxels, r.opened_reached) == (1, 1)
    fin = np.isfinite(old)
    assert fr.same_bytes(got[fin], old[fin])                         # a dead end: nothing outside gets shorter


# ---- 6. the point form -------------------------------------------------------------------------------------------------------------------
def test_pointcloud_form(pkg, product_lib):
    """the map from isdf_set_pointcloud with threshold 2, the door opened by isdf_clear_pointcloud taking one of its two points"""
    dims = (9, 7, 5)
    bmin, bmax = np.zeros(3), np.array(dims) * RES
    after = fr.wall_with_gap()
    door = (4, 3, 2)
    before = _with(after, [door])
    wall_cells = np.argwhere(after == 1)
    pts = lambda cells, dx: ((np.asarray(cells, dtype=np.float64).reshape(-1, 3) + 0.5) * RES + dx).astype(np.float32)
    wall_pts = np.concatenate([pts(wall_cells, -0.1), pts(wall_cells, 0.1), pts(wall_cells[:3], 0.0)])      # two points each, three of them a third
    door_pts = np.concatenate([pts([door], -0.1), pts([door], 0.1)])
    goal = (0, 0, 0)

    def engine(cloud, reopen):
        eng = pkg.Engine(pkg.synth.default_config(pkg.capi.V1_SWEPT))
        assert eng.set_pointcloud(cloud, RES, 2, bmin, bmax) == dims
        return _prepare(pkg, eng, reopen)

    eng = engine(np.concatenate([wall_pts, door_pts]), 1)
    assert np.array_equal(eng.get_grid(pkg.capi.GRID_OCCUPANCY)[0], before)
    eng.frontend_field_build(_centre(goal))
    old = eng.frontend_field()
    assert np.isinf(old[5:]).all() and np.isfinite(old[:4]).all()
    # points that free no voxel (a third point of a wall voxel, a voxel without points): the field and its validity stay, no reopen happened
    info = eng.clear_pointcloud(np.concatenate([pts(wall_cells[:1], 0.0), pts([(7, 1, 1)], 0.0)]))
    assert (info.n_cleared_voxels, info.n_points_ignored, info.field_dropped, info.path) == (0, 1, 0, 0)
    assert fr.same_bytes(eng.frontend_field(), old)
    _state_error(pkg, eng.frontend_field_reopen_info)
    # one of the door's two points: below the threshold
    info = eng.clear_pointcloud(door_pts[:1], **INCR)
    assert info.path == 1 and info.n_cleared_voxels == 1
    fresh = engine(np.concatenate([np.delete(wall_pts, 2 * len(wall_cells), axis=0), door_pts[1:]]), None)      # what is left, point for point
    assert np.array_equal(fresh.get_grid(pkg.capi.GRID_OCCUPANCY)[0], after)
    r, got, _ = _hold_to_a_fresh_build(pkg, eng, after, goal, info, fresh=fresh)
    assert np.isfinite(got[5:]).all() and (r.opened_voxels, r.opened_reached) == (1, 1) and r.reached_voxels > r.reached_before
    assert fr.same_bytes(got[:4], old[:4])


# ---- 7. door closes, door opens ---------------------------------------------------------------------------------------------------------
def test_door_closes_and_opens_twice_over(pkg, product_lib):
    occ = _boxes(pkg)
    goal = _boxes_goal_low(occ)
    door = _boxes_straddle(occ)
    closed = _with(occ, door)
    eng = _engine(pkg, occ, reopen=1, repair=1)
    eng.frontend_field_build(_centre(goal))
    original = eng.frontend_field()
    f_open, f_closed = _engine(pkg, occ, reopen=None), _engine(pkg, closed, reopen=None)
    f_open.frontend_field_build(_centre(goal)); f_closed.frontend_field_build(_centre(goal))
    want_open, want_closed = f_open.frontend_field(), f_closed.frontend_field()
    assert fr.same_bytes(original, want_open) and not fr.same_bytes(want_open, want_closed)
    live = None
    for rnd in range(2):
        u = eng.update_voxels(door, **INCR)
        assert u.field_dropped == 0 and u.n_new_voxels == 4 and fr.same_bytes(eng.frontend_field(), want_closed)
        c = eng.clear_voxels(door, **INCR)
        assert c.field_dropped == 0 and c.n_cleared_voxels == 4
        got = eng.frontend_field()
        assert fr.same_bytes(got, want_open) and fr.same_bytes(got, original)
        r, rep = eng.frontend_field_reopen_info(), eng.frontend_field_repair_info()
        assert r.opened_voxels == rep.closed_voxels == 4 and r.reached_voxels >= rep.reached_voxels + 4
        if rnd == 0:
            live = _live(eng)
    assert _live(eng) == live                                        # grow-only state: the second round allocates nothing
    starts = _starts(occ)
    n, xyz, rp = eng.frontend_field_paths(starts, 48)
    n_f, xyz_f, rp_f = f_open.frontend_field_paths(starts, 48)
    assert np.array_equal(n, n_f) and np.array_equal(xyz, xyz_f) and np.array_equal(rp, rp_f)


# ---- 8. what is still dropped, and the arguments ------------------------------------------------------------------------------------------
def test_dropped_cases_and_arguments(pkg, product_lib):
    capi = pkg.capi
    before = fr.serpentine((24, 24, 3))
    wall = (12, 11, 1)
    goal = (0, 0, 1)
    for mode in (0, None):                                # set explicitly, and the default
        for repair in (None, 1):                          # the repair's switch does not bear on a clear
            eng = _engine(pkg, before, reopen=mode, repair=repair)
            eng.frontend_field_build(_centre(goal))
            info = eng.clear_voxels([wall], **INCR)
            assert info.field_dropped == 1
            for call in (eng.frontend_field, eng.frontend_field_reopen_info, lambda: eng.frontend_field_paths([_centre(goal)], 8)):
                _state_error(pkg, call)
    # mode 1, but the field is only an upper bound (the round bound was hit): no fixed point to start from
    eng = _engine(pkg, before)
    part = eng.frontend_field_build(_centre(goal), max_rounds=1)
    assert part.status == 2
    assert eng.clear_voxels([wall], **INCR).field_dropped == 1
    _state_error(pkg, eng.frontend_field)
    # mode 1 and refresh_frontend = 0: the front end goes, the field with it
    eng = _engine(pkg, before)
    eng.frontend_field_build(_centre(goal))
    info = eng.clear_voxels([wall], refresh_frontend=False, **INCR)
    assert info.field_dropped == 1 and info.frontend_refreshed == 0
    # a field built under a round bound that it did not hit is a fixed point: it is lowered, under the same bound; a bound that the
    # reopen hits leaves a valid status-2 field, as the build does
    eng = _engine(pkg, before)
    full = eng.frontend_field_build(_centre(goal), max_rounds=500)
    assert full.status == 0 and 2 < full.rounds < 500
    info = eng.clear_voxels([wall], **INCR)
    r = eng.frontend_field_reopen_info()
    assert info.field_dropped == 0 and r.status == 0 and 2 < r.rounds < 500
    # a bound that the reopen hits leaves a valid status-2 field, as the build does: the first wall without its gap, so the build sees
    # the goal's run only and needs few rounds; the gap cleared, the relaxation has the whole corridor before it
    gap = [(23, 1, 0), (23, 1, 1), (23, 1, 2)]
    shut = _with(before, gap)
    eng = _engine(pkg, shut)
    short = eng.frontend_field_build(_centre(goal), max_rounds=8)
    assert short.status == 0 and short.rounds < 8 and short.reached_voxels == 24 * 3
    info = eng.clear_voxels(gap, **INCR)
    r2 = eng.frontend_field_reopen_info()
    assert info.field_dropped == 0 and (r2.status, r2.rounds, r2.reachable, r2.opened_voxels) == (2, 8, 1, 3)
    got, want = eng.frontend_field(), fr.field(before == 0, goal)
    assert (got >= want).all() and np.isinf(got).sum() > np.isinf(want).sum() and r2.reached_voxels == int(np.isfinite(got).sum())
    assert eng.clear_voxels([wall], **INCR).field_dropped == 1     # ... which the next clear drops: an upper bound, not a fixed point
    eng = _engine(pkg, before)
    eng.frontend_field_build(_centre(goal))
    assert eng.clear_voxels([wall], **INCR).field_dropped == 0
    r2 = eng.frontend_field_reopen_info()
    # nothing cleared: no reopen, the last report stays
    info = eng.clear_voxels([wall], **INCR)
    assert (info.n_cleared_voxels, info.field_dropped) == (0, 0) and eng.frontend_field_reopen_info().rounds == r2.rounds
    # argument errors
    with pytest.raises(pkg.IsdfError) as err:
        eng.frontend_field_set_reopen(2)
    assert err.value.code == capi.ISDF_ERR_INVALID_ARG
    with pytest.raises(pkg.IsdfError) as err:
        eng.frontend_field_set_repair(2)                  # still 0 or 1 only
    assert err.value.code == capi.ISDF_ERR_INVALID_ARG
    multi = pkg.Engine(pkg.synth.default_config(capi.V3_ESDF_TILE), devices=[0, 0])
    with pytest.raises(pkg.IsdfError) as err:
        multi.frontend_field_set_reopen(1)
    assert err.value.code == capi.ISDF_ERR_UNSUPPORTED
