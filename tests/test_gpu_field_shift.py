"""The cost-to-go field CARRIED through a shift of the map window (isdf_frontend_field_set_shift mode 1; csrc/frontend_field.hip, the rule
in include/isdf_accel.h and DESIGN 4.6.4) against a FRESH ctx that is given numpy's translated counts in the shifted box and builds its
field from scratch towards the centre of cell goal - s - never against the carry itself.  Fields are compared BYTE FOR BYTE, paths node
for node.  The geometry, the robot and the helpers are those of tests/test_gpu_map_shift.py: 24 x 20 x 70 voxels at 0.5 m (partial
bricks in y and z, a second 64-lane z block), kernel_size 5, 3 x 3 attitudes."""
import ctypes as C

import numpy as np
import pytest

import field_reference as fr
import test_field_shift_host as fh
import test_gpu_map_shift as ms
import test_gpu_map_update as mu
from test_gpu_map_update import BMIN, DIMS, RES

pytestmark = pytest.mark.gpu

D = np.array(DIMS)
SHIFTS = [(1, 0, 0), (-1, 0, 0), (0, 3, 0), (0, 0, 1), (0, 0, 33), (0, 0, -37), (2, -1, 5)]


def _centre(cell, s=(0, 0, 0)):
    """the centre of `cell` of the box shifted by s"""
    return (np.asarray(cell, dtype=np.float64) + 0.5) * RES + ms._box(s)[0]


def _free_cell_near(eng, target):
    free = np.argwhere(eng.frontend_cspace_table().any(axis=3))
    return tuple(int(v) for v in free[np.argmin(np.abs(free - np.asarray(target)).sum(axis=1))])


def _goal_for(eng, s):
    """a free cell of the old map next to the middle of the voxels that stay; it stays"""
    g_new = [(max(0, -s[a]) + min(DIMS[a], DIMS[a] - s[a])) // 2 for a in range(3)]
    g_old = _free_cell_near(eng, [g_new[a] + s[a] for a in range(3)])
    assert all(0 <= g_old[a] - s[a] < DIMS[a] for a in range(3))
    return g_old


def _starts(s):
    rng = np.random.default_rng(11)
    cells = np.stack([rng.integers(0, n, 12) for n in DIMS], axis=1)
    lo = ms._box(s)[0]
    return np.concatenate([(cells + rng.uniform(0.1, 0.9, cells.shape)) * RES + lo, [lo - 0.4]])


def _live(lib):
    out = (C.c_longlong * 2)()
    lib.isdf_debug_live_bytes(out)
    return list(out)


def _hold_to_a_fresh_build(pkg, eng, fresh, goal_new, s_total):
    """the carried ctx against `fresh` (the new map, no field yet): the field's bytes, 13 paths, the values; returns (fresh's build info, field)"""
    finfo = fresh.frontend_field_build(_centre(goal_new, s_total))
    want, got = fresh.frontend_field(), eng.frontend_field()
    assert fr.same_bytes(got, want)
    starts = _starts(s_total)
    n, xyz, rp = eng.frontend_field_paths(starts, 64)
    n_f, xyz_f, rp_f = fresh.frontend_field_paths(starts, 64)
    assert np.array_equal(n, n_f) and np.array_equal(xyz, xyz_f) and np.array_equal(rp, rp_f)
    assert fr.same_bytes(eng.frontend_field(starts), fresh.frontend_field(starts))
    return finfo, got


def _check_shift_info(si, finfo, s, goal_new, d_old):
    assert tuple(si.shift) == tuple(s) and tuple(si.goal_new) == tuple(goal_new)
    assert si.left_reached == int(np.isfinite(d_old[fh.leaving(DIMS, s)]).sum())
    assert (si.free_voxels, si.reached_voxels, si.reachable, si.status) == (finfo.free_voxels, finfo.reached_voxels, finfo.reachable, finfo.status)
    assert si.closed_reached <= si.closed_voxels and si.opened_reached <= si.opened_voxels and si.reset_voxels >= si.closed_reached
    assert si.brick_visits >= si.seeded_bricks_close + si.seeded_bricks_open and si.device_ms > 0.0


# ---- 1. bytes against a fresh build ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host_table", [False, True])
@pytest.mark.parametrize("force_path", [1, 2])
@pytest.mark.parametrize("s", SHIFTS)
def test_the_carried_field_equals_a_fresh_build(pkg, product_lib, s, force_path, host_table):
    c_old = mu._counts(ms._scene())
    eng = mu._engine(pkg, ms._scene(), host_table=host_table)
    eng.frontend_field_set_shift(1)
    g_old = _goal_for(eng, s)
    g_new = tuple(g_old[a] - s[a] for a in range(3))
    binfo = eng.frontend_field_build(_centre(g_old))
    assert binfo.reachable == 1 and binfo.status == 0
    d_old = eng.frontend_field()
    with pytest.raises(pkg.IsdfError) as err:
        eng.frontend_field_shift_info()                   # no carry since the build
    assert err.value.code == pkg.capi.ISDF_ERR_STATE
    info = eng.shift_map(s, force_path=force_path)
    assert info.path == force_path and info.field_dropped == 0 and info.host_table_patched == int(force_path == 1 and host_table)
    si = eng.frontend_field_shift_info()
    print(f"\n{s} path {info.path}: left {si.left_reached}, closed {si.closed_voxels} ({si.closed_reached} reached), tau {si.tau:.3f}, reset {si.reset_voxels}, "
          f"close: {si.seeded_bricks_close} bricks {si.rounds_close} rounds; opened {si.opened_voxels} ({si.opened_reached} reached), open: {si.seeded_bricks_open} bricks "
          f"{si.rounds_open} rounds; visits {si.brick_visits} (build {binfo.brick_visits}), {si.device_ms:.3f} ms (build {binfo.device_ms:.3f} ms)")
    fresh = ms._fresh(pkg, ms._shift(c_old, s), s, host_table=host_table)
    finfo, got = _hold_to_a_fresh_build(pkg, eng, fresh, g_new, s)
    _check_shift_info(si, finfo, s, g_new, d_old)
    assert si.left_reached > 0 and si.opened_reached > 0 and finfo.reachable == 1 and got[g_new] == 0.0
    kept = host_table and force_path == 1                 # (the full path marks the A*'s host copy stale)
    mu._same(mu._products(pkg, eng, host_table=kept), mu._products(pkg, fresh, host_table=kept))                   # the shift's own products as before


# ---- 2. the wall scene: each phase matters -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("force_path", [1, 2])
def test_the_wall_scene_needs_both_phases(pkg, product_lib, force_path):
    s, g_old = fh.WALL_SHIFT, fh.WALL_GOAL_OLD
    g_new = tuple(g_old[a] - s[a] for a in range(3))
    occ = fh.wall_scene()
    assert occ.shape == DIMS
    cloud = ms._in_cells_at(BMIN, np.argwhere(occ == 1), 2, np.random.default_rng(3))
    eng = mu._engine(pkg, cloud)
    eng.frontend_field_set_shift(1)
    assert eng.frontend_field_build(_centre(g_old)).reachable == 1
    d_old = eng.frontend_field()
    assert np.isfinite(d_old[fh.WALL_X + 5:, 12:, :]).all()                       # the far side is reached - through the gap, there is no other way
    info = eng.shift_map(s, force_path=force_path)
    assert info.path == force_path and info.field_dropped == 0
    si = eng.frontend_field_shift_info()
    fresh = ms._fresh(pkg, ms._shift(mu._counts(cloud), s), s)
    finfo, got = _hold_to_a_fresh_build(pkg, eng, fresh, g_new, s)
    _check_shift_info(si, finfo, s, g_new, d_old)
    higher, lower = fh.wall_effects(d_old, got, s)
    print(f"\nwall, path {info.path}: left {si.left_reached}, tau {si.tau:.3f}, reset {si.reset_voxels}, opened {si.opened_voxels} ({si.opened_reached} reached); "
          f"{higher} higher, {lower} lower")
    assert si.reset_voxels > 0 and si.left_reached > 0 and si.opened_reached > 0
    assert higher > 0 and lower > 0


# ---- 3. a follow series, then an update and a clear on the carried field -----------------------------------------------------------------
def test_a_follow_series_then_repair_and_reopen(pkg, product_lib):
    capi = pkg.capi
    step = np.array([1, 1, 2])
    eng = mu._engine(pkg, ms._scene(), host_table=True)
    eng.frontend_field_set_shift(1); eng.frontend_field_set_repair(1); eng.frontend_field_set_reopen(1)
    goal = np.array(_free_cell_near(eng, D // 2 + np.array([8, 7, 20])))          # stays in the window for all six steps
    goal_xyz = _centre(goal)
    assert eng.frontend_field_build(goal_xyz).reachable == 1
    c, total = mu._counts(ms._scene()), np.zeros(3, dtype=int)
    for k in range(1, 7):
        d_old = eng.frontend_field()
        robot = (D // 2 + k * step + 0.5) * RES + BMIN                             # the robot, on its way to the goal
        s, info = eng.map_follow(robot, 1, full_fraction=1.0)
        assert s == tuple(step) and info.path == 1 and info.field_dropped == 0 and info.host_table_patched == 1
        c, total = ms._shift(c, s), total + step
        fresh = ms._fresh(pkg, c, tuple(total), host_table=True)
        finfo, _ = _hold_to_a_fresh_build(pkg, eng, fresh, tuple(goal - total), tuple(total))
        _check_shift_info(eng.frontend_field_shift_info(), finfo, s, tuple(goal - total), d_old)
        assert np.array_equal(_centre(goal - total, tuple(total)), goal_xyz)       # the same point of the world
    # the carried free bits and counts are the real ones: an update repairs, a clear reopens the carried field
    bmin = ms._box(tuple(total))[0]
    field = eng.frontend_field()
    empty = np.argwhere((c == 0) & np.isfinite(field) & (field > 6.0))
    cells = empty[np.random.default_rng(5).choice(len(empty), 6, replace=False)]
    added = ms._in_cells_at(bmin, cells, 2, np.random.default_rng(6))
    for name, call, info_of in (("update", lambda e: e.update_pointcloud(added, **mu.INCR), lambda e: e.frontend_field_repair_info()),
                                ("clear", lambda e: e.clear_pointcloud(added, **mu.INCR), lambda e: e.frontend_field_reopen_info())):
        info = call(eng)
        assert info.path == 1 and info.field_dropped == 0, name
        assert call(fresh).field_dropped == 1
        finfo, got = _hold_to_a_fresh_build(pkg, eng, fresh, tuple(goal - total), tuple(total))
        ri = info_of(eng)
        assert (ri.free_voxels, ri.reached_voxels) == (finfo.free_voxels, finfo.reached_voxels), name
        assert not fr.same_bytes(got, field), name
        field = got
    assert tuple(eng.frontend_field_shift_info().shift) == tuple(step)             # the repair and the reopen left the carry's report alone
    mu._same(mu._products(pkg, eng, host_table=True), mu._products(pkg, fresh, host_table=True))
    assert capi.FIELD_SHIFT_CARRY == 1


# ---- 4. drops ----------------------------------------------------------------------------------------------------------------------------
def _dropped(pkg, eng, info, goal_xyz):
    assert info.field_dropped == 1
    with pytest.raises(pkg.IsdfError) as err:
        eng.frontend_field()
    assert err.value.code == pkg.capi.ISDF_ERR_STATE
    assert eng.frontend_field_build(goal_xyz).status in (0, 1)     # the field can be built again
    assert eng.frontend_field().shape == DIMS


def test_drops(pkg, product_lib):
    s = (1, 0, 0)
    # mode 0, the default and set
    for mode in (None, 0):
        eng = mu._engine(pkg, ms._scene())
        if mode is not None:
            eng.frontend_field_set_shift(1); eng.frontend_field_set_shift(mode)
        g = _goal_for(eng, s)
        assert eng.frontend_field_build(_centre(g)).reachable == 1
        _dropped(pkg, eng, eng.shift_map(s, force_path=1), _centre(g))
        with pytest.raises(pkg.IsdfError) as err:
            eng.frontend_field_shift_info()
        assert err.value.code == pkg.capi.ISDF_ERR_STATE
    # a goal that leaves the window
    eng = mu._engine(pkg, ms._scene())
    eng.frontend_field_set_shift(1)
    g = _free_cell_near(eng, (1, 10, 35))
    assert g[0] < 3 and eng.frontend_field_build(_centre(g)).reachable == 1
    _dropped(pkg, eng, eng.shift_map((3, 0, 0), force_path=1), _centre(g))
    # a goal outside the map from the start
    assert eng.frontend_field_build(BMIN - 1.0).status == 1
    _dropped(pkg, eng, eng.shift_map((0, 1, 0)), _centre((5, 5, 5), (3, 1, 0)))
    # a shift by dim on an axis: everything leaves
    eng = mu._engine(pkg, ms._scene())
    eng.frontend_field_set_shift(1)
    g = _goal_for(eng, s)
    assert eng.frontend_field_build(_centre(g)).reachable == 1
    info = eng.shift_map((0, DIMS[1], 0))
    assert info.path == pkg.capi.MAP_SHIFT_FULL
    _dropped(pkg, eng, info, _centre(g))
    # a status-2 field
    eng = mu._engine(pkg, ms._scene())
    eng.frontend_field_set_shift(1)
    assert eng.frontend_field_build(_centre(g), max_rounds=1).status == 2
    _dropped(pkg, eng, eng.shift_map(s, force_path=1), _centre(g))
    # ... and the mode is refused on a multi-device ctx, bad modes everywhere
    multi = pkg.Engine(pkg.synth.default_config(pkg.capi.V3_ESDF_TILE), devices=[0, 0])
    with pytest.raises(pkg.IsdfError) as err:
        multi.frontend_field_set_shift(1)
    assert err.value.code == pkg.capi.ISDF_ERR_UNSUPPORTED
    for bad in (-1, 2):
        with pytest.raises(pkg.IsdfError) as err:
            eng.frontend_field_set_shift(bad)
        assert err.value.code == pkg.capi.ISDF_ERR_INVALID_ARG


def test_the_mode_outlives_a_front_end_build_and_an_all_inf_field_is_carried(pkg, product_lib):
    s = (0, 3, 0)
    c_old = mu._counts(ms._scene())
    occupied = np.argwhere(c_old >= mu.THR)
    alone = occupied[[(np.abs(occupied - v).max(axis=1) <= 2 * mu.SIDE).sum() == 1 for v in occupied]]          # no other obstacle in the robot's reach
    g_old = tuple(int(v) for v in alone[np.argmin(np.abs(alone - D // 2).sum(axis=1))])             # an occupied cell: not free; free once it is cleared
    g_new = tuple(g_old[a] - s[a] for a in range(3))
    eng = mu._engine(pkg, ms._scene())
    eng.frontend_field_set_shift(1)
    eng.frontend_build(mu._fe_cfg(pkg))                   # a new front end: the mode stays
    eng.frontend_cspace(download=False)
    binfo = eng.frontend_field_build(_centre(g_old))
    assert (binfo.reachable, binfo.status) == (0, 1) and np.isinf(eng.frontend_field()).all()
    info = eng.shift_map(s, force_path=1)
    assert info.field_dropped == 0
    si = eng.frontend_field_shift_info()
    assert (si.left_reached, si.closed_reached, si.reset_voxels, si.goal_opened, si.reached_voxels, si.reachable, si.status) == (0, 0, 0, 0, 0, 0, 1)
    assert np.isinf(si.tau) and np.isinf(eng.frontend_field()).all()
    # the goal cell opens: the carried free bits let the reopen make the field reachable
    eng.frontend_field_set_reopen(1)
    bmin = ms._box(s)[0]
    c_new = ms._shift(c_old, s)
    gone = ms._in_cells_at(bmin, [g_new], int(c_new[g_new]), np.random.default_rng(2))
    cinfo = eng.clear_pointcloud(gone, **mu.INCR)
    assert cinfo.field_dropped == 0 and eng.frontend_field_reopen_info().goal_opened == 1
    c_new[g_new] = 0
    fresh = ms._fresh(pkg, c_new, s)
    finfo, got = _hold_to_a_fresh_build(pkg, eng, fresh, g_new, s)
    assert finfo.reachable == 1 and got[g_new] == 0.0


# ---- 5. s = 0 ----------------------------------------------------------------------------------------------------------------------------
def test_a_zero_shift_touches_nothing(pkg, product_lib):
    eng = mu._engine(pkg, ms._scene())
    eng.frontend_field_set_shift(1)
    g = _goal_for(eng, (0, 0, 0))
    assert eng.frontend_field_build(_centre(g)).reachable == 1
    field = eng.frontend_field()
    info = eng.shift_map((0, 0, 0), force_path=2)
    assert info.path == pkg.capi.MAP_SHIFT_NONE and info.field_dropped == 0
    assert fr.same_bytes(eng.frontend_field(), field)
    with pytest.raises(pkg.IsdfError) as err:
        eng.frontend_field_shift_info()
    assert err.value.code == pkg.capi.ISDF_ERR_STATE


# ---- 6. nothing is allocated after the first carried shift of a size ----------------------------------------------------------------------
@pytest.mark.parametrize("force_path", [1, 2])
def test_a_second_carried_shift_allocates_nothing(pkg, product_lib, force_path):
    s = (1, 0, -2)
    eng = mu._engine(pkg, ms._scene(), esdf=False, host_table=force_path == 1)
    eng.frontend_field_set_shift(1)
    g = _goal_for(eng, (4, 0, -8))
    assert eng.frontend_field_build(_centre(g)).reachable == 1
    assert eng.shift_map(s, force_path=force_path).field_dropped == 0
    before = _live(product_lib)
    info = eng.shift_map(s, force_path=force_path)
    assert _live(product_lib) == before
    assert info.path == force_path and info.field_dropped == 0
    total = (2, 0, -4)
    fresh = ms._fresh(pkg, ms._shift(ms._shift(mu._counts(ms._scene()), s), s), total, esdf=False)
    _hold_to_a_fresh_build(pkg, eng, fresh, tuple(g[a] - total[a] for a in range(3)), total)
