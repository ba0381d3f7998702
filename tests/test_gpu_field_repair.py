"""The cost-to-go field REPAIRED in place by a map update (isdf_frontend_field_set_repair mode 1; csrc/frontend_field.hip, the rule in
include/isdf_accel.h) against a FRESH ctx that is given the union map and builds its field from scratch - never against the repair itself.
Fields are compared BYTE FOR BYTE, paths node for node.  Set-up of tests/test_gpu_frontend_field.py: 0.5 m voxels, a ball smaller than a
voxel (free = not occupied), kernel_size 5, 3 x 3 attitudes.  Shapes, the smallest at which each mechanism can go wrong: 9 x 7 x 5 (less
than one brick), 17 x 9 x 70 boxes (partial bricks in x and y, a second 64-lane z block; the new voxels straddle z = 63 / 64 and the brick
edge x = 7 / 8, or touch the map's edge), the 24 x 24 x 3 serpentine (bricks left and re-entered during the repair)."""
import ctypes as C

import numpy as np
import pytest

import field_reference as fr

pytestmark = pytest.mark.gpu

RES = 0.5
MAX_ANG, ANG_RES = 30.0, 30.0
INCR = {"full_fraction": 1.0}               # the incremental path whatever share of these small maps the grown box holds
FULL = {"max_new_voxels": 0}


def _prepare(pkg, eng, mode):
    eng.set_shape(pkg.synth.make_shape("Ball", params=(0.1,)))
    eng.frontend_build(pkg.capi.frontend_config(kernel_size=5, max_roll=MAX_ANG, max_pitch=MAX_ANG, ang_res=ANG_RES, safeh=0.0))
    if mode is not None:
        eng.frontend_field_set_repair(mode)
    return eng


def _engine(pkg, occ, mode=1):
    eng = pkg.Engine(pkg.synth.default_config(pkg.capi.V1_SWEPT))
    eng.set_grid(np.ascontiguousarray(occ, dtype=np.uint8), (0, 0, 0), RES, pkg.capi.GRID_OCCUPANCY)
    return _prepare(pkg, eng, mode)


def _centre(cell):
    return (np.asarray(cell, dtype=np.float64) + 0.5) * RES


def _live(eng):
    b = (C.c_longlong * 2)()
    eng.lib.isdf_debug_live_bytes(b)
    return int(b[0]), int(b[1])


def _with(occ, cells):
    out = np.array(occ, dtype=np.uint8)
    for c in cells:
        assert out[tuple(c)] == 0, c
        out[tuple(c)] = 1
    return out


def _starts(occ):
    """16 start points in cells spread over the map (free or not), plus one outside it"""
    rng = np.random.default_rng(11)
    cells = np.stack([rng.integers(0, s, 16) for s in occ.shape], axis=1)
    return np.concatenate([(cells + rng.uniform(0.1, 0.9, cells.shape)) * RES, [[-0.4, 1.0, 1.0]]])


def _hold_to_a_fresh_build(pkg, eng, occ_union, goal, update_info, fresh=None):
    """the repaired ctx against a fresh one on the union map: the field's bytes, 17 paths, the counts; returns (repair info, field)"""
    fresh = fresh if fresh is not None else _engine(pkg, occ_union, mode=None)
    finfo = fresh.frontend_field_build(_centre(goal))
    want = fresh.frontend_field()
    got = eng.frontend_field()
    rinfo = eng.frontend_field_repair_info()
    print(f"\nclosed {rinfo.closed_voxels} ({rinfo.closed_reached} reached), tau {rinfo.tau:.4f}, reset {rinfo.reset_voxels}, seeded {rinfo.seeded_bricks}, "
          f"rounds {rinfo.rounds} (build {finfo.rounds}), visits {rinfo.brick_visits} (build {finfo.brick_visits}), {rinfo.device_ms:.3f} ms (build {finfo.device_ms:.3f} ms)")
    assert update_info.field_dropped == 0
    assert fr.same_bytes(got, want)
    assert np.isinf(got[np.asarray(occ_union) != 0]).all()
    assert (rinfo.free_voxels, rinfo.reached_voxels, rinfo.reachable, rinfo.status) == (finfo.free_voxels, finfo.reached_voxels, finfo.reachable, finfo.status)
    assert rinfo.free_voxels == int((np.asarray(occ_union) == 0).sum()) and rinfo.reached_voxels == int(np.isfinite(want).sum())
    starts = _starts(occ_union)
    cap = 48
    n, xyz, rp = eng.frontend_field_paths(starts, cap)
    n_f, xyz_f, rp_f = fresh.frontend_field_paths(starts, cap)
    assert np.array_equal(n, n_f) and np.array_equal(xyz, xyz_f) and np.array_equal(rp, rp_f)
    v = eng.frontend_field(starts)
    assert fr.same_bytes(v, fresh.frontend_field(starts))
    return rinfo, got


def _boxes(pkg):
    return pkg.synth.random_box_map((17, 9, 70), res=RES, occupancy=0.15, seed=4, edge=(0.5, 1.5))


def _boxes_straddle(occ):
    """free voxels (7, y, 63), (8, y, 63), (7, y, 64), (8, y, 64) of one y: both sides of the brick edge in x and of the 64-lane split in z"""
    for y in range(occ.shape[1]):
        if not occ[7:9, y, 63:65].any():
            return [(7, y, 63), (8, y, 63), (7, y, 64), (8, y, 64)]
    raise AssertionError("no free 2 x 1 x 2 block at the brick corner")


def _boxes_goal_low(occ):
    cells = np.argwhere(occ == 0)
    return tuple(int(v) for v in cells[np.argmin(cells.sum(axis=1))])


def test_far_obstacle_resets_a_part_only(pkg, product_lib):
    occ = _boxes(pkg)
    goal = _boxes_goal_low(occ)
    new = _boxes_straddle(occ)
    eng = _engine(pkg, occ)
    binfo = eng.frontend_field_build(_centre(goal))
    with pytest.raises(pkg.IsdfError) as err:
        eng.frontend_field_repair_info()                  # no repair since the build
    assert err.value.code == pkg.capi.ISDF_ERR_STATE
    old = eng.frontend_field()
    assert all(np.isfinite(old[c]) for c in new)
    info = eng.update_voxels(new, **INCR)
    assert info.path == 1 and info.n_new_voxels == 4
    rinfo, got = _hold_to_a_fresh_build(pkg, eng, _with(occ, new), goal, info)
    assert rinfo.closed_voxels == rinfo.closed_reached == 4 and rinfo.tau == min(old[c] for c in new)
    assert rinfo.reset_voxels == int((np.isfinite(old) & (old >= rinfo.tau)).sum())
    assert 0 < rinfo.reset_voxels < binfo.reached_voxels  # the rule was exercised: neither nothing nor a disguised rebuild
    assert 0 < rinfo.seeded_bricks <= binfo.bricks and rinfo.rounds >= 1          # (the shell d >= 67 cells has voxels on both sides of z = 64 in every brick column)
    kept = old < rinfo.tau
    assert fr.same_bytes(got[kept], old[kept])
    # a new build forgets the repair's report
    eng.frontend_field_build(_centre(goal))
    with pytest.raises(pkg.IsdfError) as err:
        eng.frontend_field_repair_info()
    assert err.value.code == pkg.capi.ISDF_ERR_STATE


def test_obstacle_at_the_maps_edge_and_the_forced_full_path(pkg, product_lib):
    occ = _boxes(pkg)
    goal = _boxes_goal_low(occ)
    cells = np.argwhere(occ == 0)
    corner = tuple(int(v) for v in cells[np.argmax(cells.sum(axis=1))])          # the free voxel nearest the far corner
    assert corner[2] == 69 or corner[0] == 16 or corner[1] == 8
    edge = [corner, next(tuple(int(v) for v in c) for c in cells if c[0] == 0 and c[2] >= 64 and tuple(c) != goal)]
    for params, path in ((INCR, 1), (FULL, 2)):
        eng = _engine(pkg, occ)
        eng.frontend_field_build(_centre(goal))
        new = edge if path == 1 else edge + _boxes_straddle(occ)
        info = eng.update_voxels(new, **params)
        assert info.path == path and info.n_new_voxels == len(new)
        rinfo, _ = _hold_to_a_fresh_build(pkg, eng, _with(occ, new), goal, info)
        assert rinfo.closed_voxels == len(new)


def test_obstacle_next_to_the_goal(pkg, product_lib):
    occ = fr.open_map()
    goal = (1, 5, 3)
    eng = _engine(pkg, occ)
    binfo = eng.frontend_field_build(_centre(goal))
    info = eng.update_voxels([(2, 5, 3)], **INCR)
    assert info.path == 1
    rinfo, got = _hold_to_a_fresh_build(pkg, eng, _with(occ, [(2, 5, 3)]), goal, info)
    assert rinfo.tau == 1.0 and rinfo.reset_voxels == binfo.reached_voxels - 1 and got[goal] == 0.0
    assert fr.same_bytes(got, fr.field(_with(occ, [(2, 5, 3)]) == 0, goal))


def test_gap_closed_leaves_the_far_side_unreached(pkg, product_lib):
    occ = fr.wall_with_gap()
    goal = (0, 0, 0)
    eng = _engine(pkg, occ)
    eng.frontend_field_build(_centre(goal))
    assert np.isfinite(eng.frontend_field()[5:]).all()
    info = eng.update_voxels([(4, 3, 2)], **INCR)
    rinfo, got = _hold_to_a_fresh_build(pkg, eng, _with(occ, [(4, 3, 2)]), goal, info)
    assert np.isinf(got[4:]).all() and np.isfinite(got[:4]).all() and rinfo.reachable == 1
    assert fr.same_bytes(got, fr.field(_with(occ, [(4, 3, 2)]) == 0, goal))


def test_goal_closed(pkg, product_lib):
    occ = fr.open_map()
    goal = (1, 5, 3)
    eng = _engine(pkg, occ)
    binfo = eng.frontend_field_build(_centre(goal))
    info = eng.update_voxels([goal], **INCR)
    rinfo, got = _hold_to_a_fresh_build(pkg, eng, _with(occ, [goal]), goal, info)
    assert rinfo.tau == 0.0 and rinfo.reset_voxels == binfo.reached_voxels
    assert rinfo.reachable == 0 and rinfo.status == 1 and rinfo.reached_voxels == 0 and np.isinf(got).all()
    n, _, _ = eng.frontend_field_paths([_centre((4, 3, 2)), _centre(goal)], 8)
    assert n[0] == 0 and n[1] == 0
    # the field stays valid and all +inf: a further update repairs it again, with nothing to do
    info2 = eng.update_voxels([(6, 1, 1)], **INCR)
    assert info2.field_dropped == 0 and np.isinf(eng.frontend_field()).all()
    r2 = eng.frontend_field_repair_info()
    assert (r2.rounds, r2.reset_voxels, r2.reachable, r2.free_voxels) == (0, 0, 0, rinfo.free_voxels - 1)


def test_nothing_reached_closes(pkg, product_lib):
    occ = fr.sealed_pocket()
    goal = (0, 0, 0)
    eng = _engine(pkg, occ)
    eng.frontend_field_build(_centre(goal))
    old = eng.frontend_field()
    assert np.isinf(old[fr.POCKET_CELL])
    info = eng.update_voxels([fr.POCKET_CELL], **INCR)
    rinfo, got = _hold_to_a_fresh_build(pkg, eng, _with(occ, [fr.POCKET_CELL]), goal, info)
    assert rinfo.rounds == 0 and rinfo.reset_voxels == 0 and rinfo.seeded_bricks == 0 and rinfo.brick_visits == 0 and np.isinf(rinfo.tau)
    assert (rinfo.closed_voxels, rinfo.closed_reached) == (1, 0)
    assert fr.same_bytes(got, old)


def test_serpentine_reactivates_bricks_and_two_updates_equal_one(pkg, product_lib):
    occ = fr.serpentine((24, 24, 3))
    goal = (0, 0, 1)
    a, b = [(12, 12, 1), (3, 4, 0)], [(12, 12, 0), (20, 20, 2), (23, 1, 1)]
    two = _engine(pkg, occ)
    binfo = two.frontend_field_build(_centre(goal))
    i1 = two.update_voxels(a, **INCR)
    r1, _ = _hold_to_a_fresh_build(pkg, two, _with(occ, a), goal, i1)
    assert 0 < r1.reset_voxels < binfo.reached_voxels
    assert r1.rounds > 1 and r1.brick_visits > r1.seeded_bricks          # the corridor leaves bricks and enters them again
    i2 = two.update_voxels(b, **INCR)
    r2, d_two = _hold_to_a_fresh_build(pkg, two, _with(occ, a + b), goal, i2)
    one = _engine(pkg, occ)
    one.frontend_field_build(_centre(goal))
    i3 = one.update_voxels(a + b, **INCR)
    r3, d_one = _hold_to_a_fresh_build(pkg, one, _with(occ, a + b), goal, i3)
    assert fr.same_bytes(d_two, d_one) and fr.same_bytes(d_one, fr.field(_with(occ, a + b) == 0, goal))
    assert (r2.free_voxels, r2.reached_voxels) == (r3.free_voxels, r3.reached_voxels)


def test_pointcloud_form(pkg, product_lib):
    """the map from isdf_set_pointcloud (one point occupies a voxel), the new voxels through isdf_update_pointcloud"""
    dims = (9, 7, 5)
    bmin, bmax = np.zeros(3), np.array(dims) * RES
    occ = fr.wall_with_gap()
    old_pts = (np.argwhere(occ == 1) + 0.5) * RES
    new_cells = [(4, 3, 2), (7, 1, 1)]
    new_pts = (np.array(new_cells) + 0.5) * RES
    goal = (0, 0, 0)

    def engine(cloud, mode):
        eng = pkg.Engine(pkg.synth.default_config(pkg.capi.V1_SWEPT))
        assert eng.set_pointcloud(cloud, RES, 1, bmin, bmax) == dims
        return _prepare(pkg, eng, mode)

    eng = engine(old_pts, 1)
    assert np.array_equal(eng.get_grid(pkg.capi.GRID_OCCUPANCY)[0], occ)
    eng.frontend_field_build(_centre(goal))
    info = eng.update_pointcloud(new_pts, **INCR)
    assert info.path == 1 and info.n_new_voxels == 2
    rinfo, got = _hold_to_a_fresh_build(pkg, eng, _with(occ, new_cells), goal, info, fresh=engine(np.concatenate([old_pts, new_pts]), None))
    assert np.isinf(got[4:]).all() and rinfo.closed_voxels == 2
    # points that occupy nothing new: nothing is touched, the last repair's report stays
    info = eng.update_pointcloud(new_pts)
    assert info.n_new_voxels == 0 and info.field_dropped == 0 and fr.same_bytes(eng.frontend_field(), got)


def test_mode_0_drops_and_a_status_2_field_is_dropped(pkg, product_lib):
    capi = pkg.capi
    occ = fr.serpentine((24, 24, 3))
    goal = (0, 0, 1)
    for mode in (0, None):                                # set explicitly, and the default
        eng = _engine(pkg, occ, mode=mode)
        eng.frontend_field_build(_centre(goal))
        info = eng.update_voxels([(12, 12, 1)], **INCR)
        assert info.field_dropped == 1
        for call in (eng.frontend_field, eng.frontend_field_repair_info, lambda: eng.frontend_field_paths([_centre(goal)], 8)):
            with pytest.raises(pkg.IsdfError) as err:
                call()
            assert err.value.code == capi.ISDF_ERR_STATE
    # mode 1, but the field is only an upper bound (the round bound was hit): no fixed point to repair
    eng = _engine(pkg, occ, mode=1)
    part = eng.frontend_field_build(_centre(goal), max_rounds=1)
    assert part.status == 2
    info = eng.update_voxels([(12, 12, 1)], **INCR)
    assert info.field_dropped == 1
    with pytest.raises(pkg.IsdfError) as err:
        eng.frontend_field()
    assert err.value.code == capi.ISDF_ERR_STATE
    # mode 1 and refresh_frontend = 0: the front end goes, the field with it
    eng = _engine(pkg, occ, mode=1)
    eng.frontend_field_build(_centre(goal))
    info = eng.update_voxels([(12, 12, 1)], refresh_frontend=False, **INCR)
    assert info.field_dropped == 1 and info.frontend_refreshed == 0
    # a field built under a round bound that it did not hit is a fixed point: it is repaired, under the same bound
    eng = _engine(pkg, occ, mode=1)
    full = eng.frontend_field_build(_centre(goal), max_rounds=500)
    assert full.status == 0 and 2 < full.rounds < 500
    info = eng.update_voxels([(12, 12, 1)], **INCR)
    r = eng.frontend_field_repair_info()
    assert info.field_dropped == 0 and r.status == 0 and r.rounds < 500
    # argument errors
    with pytest.raises(pkg.IsdfError) as err:
        eng.frontend_field_set_repair(2)
    assert err.value.code == capi.ISDF_ERR_INVALID_ARG
    multi = pkg.Engine(pkg.synth.default_config(capi.V3_ESDF_TILE), devices=[0, 0])
    with pytest.raises(pkg.IsdfError) as err:
        multi.frontend_field_set_repair(1)
    assert err.value.code == capi.ISDF_ERR_UNSUPPORTED


def test_second_repair_of_a_size_takes_no_memory(pkg, product_lib):
    occ = _boxes(pkg)
    goal = _boxes_goal_low(occ)
    s = _boxes_straddle(occ)
    eng = _engine(pkg, occ)
    eng.frontend_field_build(_centre(goal))
    assert eng.update_voxels(s[:2], **INCR).field_dropped == 0
    live = _live(eng)
    info = eng.update_voxels(s[2:], **INCR)
    assert info.field_dropped == 0 and _live(eng) == live # grow-only state: the second repair of a size allocates nothing
    _hold_to_a_fresh_build(pkg, eng, _with(occ, s), goal, info)
