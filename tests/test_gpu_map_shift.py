"""The map window shifted in place (csrc/map_shift.hip: isdf_shift_map / isdf_map_follow) against the project's own from-scratch build
in a second, fresh ctx: isdf_set_pointcloud on a cloud with numpy's translated counts placed inside the cells of the new box, then the
same derived products - never against the shift path itself.  Every comparison is == on bytes.  The geometry, the robot and the helpers
are those of tests/test_gpu_map_update.py: 24 x 20 x 70 voxels at 0.5 m, BMIN = (-1, 2, 0.5) (every shifted box is exact in fp64),
sta_threshold 2, a box robot with kernel_size 5 and 3 x 3 attitudes."""
import functools

import numpy as np
import pytest

import test_gpu_map_update as mu
from test_gpu_map_clear import CM, MARGIN, N, T, _same_report, _watch_occ
from test_gpu_map_update import BMAX, BMIN, DIMS, RES, SIDE, THR, _products, _same

pytestmark = pytest.mark.gpu

N_VOX = int(np.prod(DIMS))
D = np.array(DIMS)
SHIFTS = [(1, 0, 0), (-1, 0, 0), (0, 3, 0), (0, -3, 0), (0, 0, 1), (0, 0, -1), (0, 0, 33), (0, 0, -37), (2, -1, 5), (23, 0, 0), (24, 0, 0), (0, -25, 80)]


# ---- numpy's view of the shift: only to build the fresh ctx's cloud and to state what the tests expect
def _shift(g, s):
    """out[v] = g[v + s], zero where v + s lies outside"""
    out = np.zeros_like(g)
    dst, src = [], []
    for a in range(3):
        lo, hi = max(0, -s[a]), min(DIMS[a], DIMS[a] - s[a])
        if lo >= hi:
            return out
        dst.append(slice(lo, hi)); src.append(slice(lo + s[a], hi + s[a]))
    out[tuple(dst)] = g[tuple(src)]
    return out


def _leaving(s):
    """old voxels without a destination: v - s lies outside"""
    idx = np.stack(np.meshgrid(*[np.arange(n) for n in DIMS], indexing="ij"), axis=-1)
    return ((idx - np.array(s) < 0) | (idx - np.array(s) >= D)).any(axis=-1)


def _box(s):
    return BMIN + np.array(s) * RES, BMAX + np.array(s) * RES


def _in_cells_at(bmin, cells, per_cell, rng):
    cells = np.repeat(np.asarray(cells, dtype=np.float64).reshape(-1, 3), per_cell, axis=0)
    return ((cells + rng.uniform(0.15, 0.85, cells.shape)) * RES + bmin).astype(np.float32)


def _cloud_of(counts, bmin):
    cells = np.argwhere(counts > 0)
    return _in_cells_at(bmin, cells, counts[tuple(cells.T)].astype(np.int64), np.random.default_rng(77))


def _derive(pkg, eng, bmin, host_table=False, **derive):
    mu._derive(pkg, eng, **derive)
    if host_table:                                                  # a search that starts outside the map only fetches the table
        assert eng.frontend_astar(bmin - 1.0, bmin + 1.0)[3].table_ms > 0


def _fresh(pkg, counts, s, **derive):
    """a fresh ctx holding `counts` in the box shifted by s.  No cloud has no points: the empty map is built with one point (below the
    threshold) that a clear then takes out again - path 0, nothing but that count moves."""
    bmin, bmax = _box(s)
    eng = pkg.Engine(pkg.synth.default_config(pkg.capi.V1_SWEPT))
    lone = None
    if not counts.any():
        lone = _in_cells_at(bmin, [(1, 1, 1)], 1, np.random.default_rng(1))
    assert eng.set_pointcloud(_cloud_of(counts, bmin) if lone is None else lone, RES, THR, bmin, bmax) == DIMS
    if lone is not None:
        assert eng.clear_pointcloud(lone).path == 0
    assert np.array_equal(eng.map_counts(), counts)
    _derive(pkg, eng, bmin, **derive)
    return eng


@functools.lru_cache(maxsize=None)
def _scene():
    """the update tests' old cloud plus voxels with two or three points in every leaving slab of SHIFTS and within SIDE of every face"""
    rng = np.random.default_rng(41)
    X, Y, Z = DIMS
    faces = [(0, 5, 30), (X - 1, 12, 40), (7, 0, 20), (9, Y - 1, 50), (11, 8, 0), (15, 10, Z - 1),          # on the six faces
             (1, 9, 33), (X - 2, 3, 66), (5, 2, 5), (6, Y - 3, 64), (12, 12, 1), (13, 4, Z - 2),            # within SIDE of them
             (3, 3, 34), (20, 16, 36), (0, Y - 1, Z - 1), (X - 1, 0, 0)]
    extra = _in_cells_at(BMIN, faces, rng.integers(2, 4, len(faces)), rng)
    return np.concatenate([mu._clouds()[0], extra])


def _check_info(pkg, info, s, c_old, incr, host_table, frontend=True):
    occ_old = c_old >= THR
    gone = _leaving(s)
    bmin, _ = _box(s)
    assert info.path == (pkg.capi.MAP_SHIFT_INCREMENTAL if incr else pkg.capi.MAP_SHIFT_FULL)
    assert tuple(info.shift) == tuple(s) and np.array_equal(np.array(info.bmin_new), bmin)
    assert info.voxels_entered == N_VOX - np.prod(np.maximum(D - np.abs(s), 0))
    assert info.occupied_left == (occ_old & gone).sum() and info.counts_left == c_old[gone].sum()
    boxes = pkg.shift_bands_host(DIMS, s, SIDE)
    if frontend:
        assert info.n_boxes == (len(boxes) if incr else 0)
        assert info.cspace_voxels == (sum(int(np.prod(hi - lo + 1)) for lo, hi in boxes) if incr else N_VOX)
    assert info.host_table_patched == int(incr and host_table)


# ---- 0. the scene ---------------------------------------------------------------------------------------------------------------------
def test_the_scene_shows_what_it_is_for(pkg):
    c = mu._counts(_scene())
    occ = c >= THR
    assert 100 <= occ.sum() <= 300 and (c == 1).any() and (c >= 3).any()
    for s in SHIFTS:
        gone = _leaving(s)
        assert (occ & gone).any() and c[gone].sum() > (occ & gone).sum(), s          # occupied voxels leave, and points of free voxels with them
        if all(abs(s[a]) < DIMS[a] for a in range(3)):
            assert (occ & ~gone).any(), s                                             # ... and some stay
    for a in range(3):                                                                # within SIDE of every face, and on it
        lo, hi = [slice(None)] * 3, [slice(None)] * 3
        lo[a], hi[a] = slice(0, SIDE), slice(DIMS[a] - SIDE, DIMS[a])
        assert occ[tuple(lo)].any() and occ[tuple(hi)].any()
        lo[a], hi[a] = 0, DIMS[a] - 1
        assert occ[tuple(lo)].any() and occ[tuple(hi)].any()
    assert occ[:, :, 32:38].any()                                                     # around the z words' split (70 = 2 x 32 + 6)
    for s in SHIFTS:                                                                  # every shifted box is exact and keeps the dims
        lo, hi = pkg.shift_geometry_host(BMIN, BMAX, RES, DIMS, s)
        assert np.array_equal(lo, _box(s)[0]) and np.array_equal(hi, _box(s)[1])


# ---- 1. shifts against a fresh build ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host_table", [False, True])
@pytest.mark.parametrize("forced", ["incremental", "full"])
@pytest.mark.parametrize("s", SHIFTS)
def test_products_equal_a_fresh_build(pkg, product_lib, s, forced, host_table):
    capi = pkg.capi
    c_old = mu._counts(_scene())
    incr = forced == "incremental" and all(abs(s[a]) < DIMS[a] for a in range(3))          # everything left: the full path whatever is forced
    eng = mu._engine(pkg, _scene(), host_table=host_table)
    eng.esdf_sample(mu._sample_points(), scattered=True)                                   # the bricks exist: the shift has to mark them stale
    info = eng.shift_map(s, force_path=1 if forced == "incremental" else 2)
    print(f"\n{s} {forced}: path {info.path}, entered {info.voxels_entered}, occupied left {info.occupied_left}, counts left {info.counts_left}, boxes {info.n_boxes}, "
          f"cspace voxels {info.cspace_voxels}, translate {info.translate_ms:.3f} esdf {info.esdf_ms:.3f} frontend {info.frontend_ms:.3f} wall {info.wall_ms:.3f} ms")
    _check_info(pkg, info, s, c_old, incr, host_table)
    assert (info.field_dropped, info.watch_rechecked) == (0, 0)
    c_new = _shift(c_old, s)
    fresh = _fresh(pkg, c_new, s, host_table=host_table)
    bmin, bmax = _box(s)
    for e in (eng, fresh):
        _, origin, top = e.get_grid(capi.GRID_OCCUPANCY)
        assert np.array_equal(origin, bmin) and np.array_equal(top, bmax)
    if host_table and not incr:                                     # the full path marks the host copy stale: the next search fetches it again
        with pytest.raises(pkg.IsdfError) as err:
            eng.frontend_cspace_table(host=True)
        assert err.value.code == capi.ISDF_ERR_STATE
        assert eng.frontend_astar(bmin - 1.0, bmin + 1.0)[3].table_ms > 0
    want = _products(pkg, fresh, host_table=host_table)
    _same(_products(pkg, eng, host_table=host_table), want)
    assert np.array_equal(want["counts"], c_new) and np.array_equal(want["occ"], (c_new >= THR).astype(np.uint8))
    assert np.array_equal(want["cspace"], fresh.frontend_cspace()[0])
    if c_new.any():
        assert want["occ"].any() and want["cspace"].any()
    else:
        assert np.isinf(want["esdf"]).all() and not want["occ"].any()


# ---- 2. composition ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s1,s2", [((1, 0, 0), (2, 0, 0)), ((0, 0, -3), (0, 0, -4)), ((0, -2, 0), (0, -1, 0))])
def test_two_shifts_on_one_axis_equal_one(pkg, product_lib, s1, s2):
    both = tuple(a + b for a, b in zip(s1, s2))
    two = mu._engine(pkg, _scene(), host_table=True)
    i1, i2 = two.shift_map(s1), two.shift_map(s2)
    one = mu._engine(pkg, _scene(), host_table=True)
    i3 = one.shift_map(both)
    assert i1.path == i2.path == i3.path == 1 and i1.host_table_patched == i2.host_table_patched == i3.host_table_patched == 1          # the default full_fraction
    assert i1.counts_left + i2.counts_left == i3.counts_left and i1.occupied_left + i2.occupied_left == i3.occupied_left
    want = _products(pkg, _fresh(pkg, _shift(mu._counts(_scene()), both), both, host_table=True), host_table=True)
    _same(_products(pkg, two, host_table=True), want)
    _same(_products(pkg, one, host_table=True), want)


def test_a_shift_and_its_inverse_zero_the_two_margins(pkg, product_lib):
    s, back = (2, -1, 5), (-2, 1, -5)
    c_old = mu._counts(_scene())
    c_end = _shift(_shift(c_old, s), back)
    kept = np.zeros(DIMS, dtype=bool)
    kept[2:, :DIMS[1] - 1, 5:] = True
    assert np.array_equal(c_end, np.where(kept, c_old, 0)) and (c_end != c_old).any()
    eng = mu._engine(pkg, _scene(), host_table=True)
    i1, i2 = eng.shift_map(s, force_path=1), eng.shift_map(back, force_path=1)
    assert i1.path == i2.path == 1 and i2.counts_left == 0 and i2.occupied_left == 0          # what the way back pushes out had entered empty
    assert np.array_equal(np.array(i2.bmin_new), BMIN)
    _same(_products(pkg, eng, host_table=True), _products(pkg, _fresh(pkg, c_end, (0, 0, 0), host_table=True), host_table=True))


# ---- 3. binning after a shift -----------------------------------------------------------------------------------------------------------
def test_update_clear_and_scan_bin_with_the_new_box(pkg, product_lib):
    s = (2, -1, 5)
    bmin, bmax = _box(s)
    c_new = _shift(mu._counts(_scene()), s)
    rng = np.random.default_rng(8)
    ones, empty, taken = np.argwhere(c_new == 1), np.argwhere(c_new == 0), np.argwhere(c_new >= THR)
    # the old box without the new one: inside the map before the shift, outside now - these land in voxel (0, 0, 0)
    only_old = np.array([[-0.8, 5.0, 5.0], [3.0, 11.8, 5.0], [3.0, 5.0, 1.0]], dtype=np.float32)
    assert ((only_old >= BMIN) & (only_old <= BMAX)).all() and ((only_old < bmin) | (only_old > bmax)).any(axis=1).all()
    added = np.concatenate([_in_cells_at(bmin, ones[:6], 1, rng), _in_cells_at(bmin, empty[10:18], 2, rng), _in_cells_at(bmin, [(0, 0, 0), (23, 19, 69)], 2, rng), only_old])
    removed = np.concatenate([_in_cells_at(bmin, taken[:5], 2, rng), _in_cells_at(bmin, empty[10:12], 1, rng), only_old[:1]])
    origin = (np.array([12, 10, 30]) + 0.5) * RES + bmin
    ends = rng.uniform(bmin + 0.1, bmax - 0.1, (60, 3)).astype(np.float32)
    hit = (rng.uniform(size=60) < 0.7).astype(np.uint8)
    eng = mu._engine(pkg, _scene(), host_table=True)
    eng.esdf_sample(mu._sample_points(), scattered=True)
    assert eng.shift_map(s, force_path=1).path == 1                 # (three axes at once: the bands hold 0.63 of this small map)
    fresh = _fresh(pkg, c_new, s, host_table=True)
    steps = [("update", lambda e: e.update_pointcloud(added, **mu.INCR), lambda i: (i.path, i.n_new_voxels, list(i.dirty_lo), list(i.dirty_hi))),
             ("clear", lambda e: e.clear_pointcloud(removed, **mu.INCR), lambda i: (i.path, i.n_cleared_voxels, i.n_points_ignored, list(i.dirty_lo), list(i.dirty_hi))),
             ("scan", lambda e: e.integrate_scan(origin, ends, hit, full_fraction=1.0), lambda i: (i.n_rays_skipped, i.n_hits, i.n_free_voxels, i.clear.n_cleared_voxels, i.update.n_new_voxels))]
    for name, call, key in steps:
        got, want = key(call(eng)), key(call(fresh))
        assert got == want, (name, got, want)
        _same(_products(pkg, eng, host_table=True), _products(pkg, fresh, host_table=True))
        if name == "clear":                                         # the new box's corner voxel: its own two points and the points outside
            assert c_new[0, 0, 0] == 0 and eng.map_counts()[0, 0, 0] == 2 + len(only_old) - 1


# ---- 4. derived state ---------------------------------------------------------------------------------------------------------------------
def _watch_cloud():
    occ = _watch_occ()
    return _in_cells_at(BMIN, np.argwhere(occ == 1), 2, np.random.default_rng(5)), occ


def test_the_field_is_dropped_and_the_watch_rechecked(pkg, product_lib):
    capi = pkg.capi
    cloud, occ = _watch_cloud()
    s = (1, -1, 2)
    eng = mu._engine(pkg, cloud)
    eng.traj_check_set_watch(1)
    rep0 = eng.traj_check(T, CM, margin=MARGIN)
    assert rep0["n_below_margin"] > 0
    free = eng.frontend_cspace_table().any(axis=3)
    goal = (np.argwhere(free)[len(np.argwhere(free)) // 2] + 0.5) * RES + BMIN
    assert eng.frontend_field_build(goal).reachable == 1
    info = eng.shift_map(s, force_path=1)
    assert info.path == 1 and (info.field_dropped, info.watch_rechecked) == (1, 1)
    with pytest.raises(pkg.IsdfError) as err:
        eng.frontend_field()
    assert err.value.code == capi.ISDF_ERR_STATE
    fresh = _fresh(pkg, _shift(mu._counts(cloud), s), s)
    want = fresh.traj_check(T, CM, margin=MARGIN)
    want_rows = fresh.traj_check_points()
    rep, last = eng.traj_check_watch_info(N)                       # still armed, under the new epoch
    _same_report(rep, want, "re-checked watch after a shift")
    rows = eng.traj_check_points()
    assert rows.shape == want_rows.shape and rows.tobytes() == want_rows.tobytes() and len(rows) > 0
    assert last["path"] == 2 and last["updates_folded"] == 1
    _same(_products(pkg, eng), _products(pkg, fresh))
    assert eng.frontend_field_build(goal).status in (0, 1)         # the field can be built again
    # a second shift keeps folding into the same watch
    assert eng.shift_map((0, 1, 0)).watch_rechecked == 1 and eng.traj_check_watch_info(N)[1]["updates_folded"] == 2
    # without a watch the report from before the shift is stale for the merge
    plain = mu._engine(pkg, cloud)
    plain.traj_check(T, CM, margin=MARGIN)
    info = plain.shift_map(s)
    assert (info.field_dropped, info.watch_rechecked) == (0, 0)
    with pytest.raises(pkg.IsdfError) as err:
        plain.points_merge_check()
    assert err.value.code == capi.ISDF_ERR_STATE and "older" in str(err.value)


# ---- 5. no-ops and refusals ---------------------------------------------------------------------------------------------------------------
def test_a_zero_shift_touches_nothing(pkg, product_lib):
    capi = pkg.capi
    cloud, _ = _watch_cloud()
    eng = mu._engine(pkg, cloud, host_table=True)
    eng.traj_check(T, CM, margin=MARGIN)
    before = _products(pkg, eng, host_table=True)
    free = before["cspace"].any(axis=3)
    goal = (np.argwhere(free)[len(np.argwhere(free)) // 2] + 0.5) * RES + BMIN
    assert eng.frontend_field_build(goal).reachable == 1
    field = eng.frontend_field()
    info = eng.shift_map((0, 0, 0), force_path=2)
    assert info.path == capi.MAP_SHIFT_NONE and tuple(info.shift) == (0, 0, 0) and np.array_equal(np.array(info.bmin_new), BMIN)
    assert (info.voxels_entered, info.occupied_left, info.counts_left, info.n_boxes, info.cspace_voxels) == (0, 0, 0, 0, 0)
    assert (info.host_table_patched, info.field_dropped, info.watch_rechecked) == (0, 0, 0)
    assert np.array_equal(eng.frontend_field().view(np.uint8), field.view(np.uint8))
    _same(_products(pkg, eng, host_table=True), before)
    assert eng.points_merge_check()["n_added"] >= 0                # the epoch did not move: the report from before is still accepted


def test_refusals_change_nothing(pkg, product_lib):
    capi = pkg.capi
    cloud = _scene()
    eng = mu._engine(pkg, cloud, esdf=False, frontend=False)
    for bad in ({"full_fraction": -0.5}, {"full_fraction": float("nan")}, {"force_path": 3}, {"force_path": -1}):
        for call in (lambda: eng.shift_map((1, 0, 0), **bad), lambda: eng.map_follow(BMIN, 1, **bad)):
            with pytest.raises(pkg.IsdfError) as err:
                call()
            assert err.value.code == capi.ISDF_ERR_INVALID_ARG
    assert product_lib.isdf_shift_map(eng.h, None, None, None) == capi.ISDF_ERR_INVALID_ARG
    assert np.array_equal(eng.map_counts(), mu._counts(cloud)) and np.array_equal(eng.get_grid(capi.GRID_OCCUPANCY)[1], BMIN)
    # a box whose extent is no whole number of voxels: the dims guard refuses the shifts that would change the grid, and changes nothing
    odd = pkg.Engine(pkg.synth.default_config(capi.V1_SWEPT))
    lo, hi = np.array([0.1, 0.2, 0.3]), np.array([0.1, 0.2, 0.3]) + np.array([2.35, 2.0, 3.3])
    dims = odd.set_pointcloud(cloud, 0.1, THR, lo, hi)
    refused = 0
    for k in range(1, 40):
        s = (k, -k, 3 * k)
        try:
            pkg.shift_geometry_host(lo, hi, 0.1, dims, s)
        except pkg.IsdfError:
            refused += 1
            counts, origin = odd.map_counts(), odd.get_grid(capi.GRID_OCCUPANCY)[1]
            with pytest.raises(pkg.IsdfError) as err:
                odd.shift_map(s)
            assert err.value.code == capi.ISDF_ERR_INVALID_ARG
            assert np.array_equal(odd.map_counts(), counts) and np.array_equal(odd.get_grid(capi.GRID_OCCUPANCY)[1], origin)
    print(f"\ndims guard: {refused} of 39 shifts of the odd box refused")
    assert refused > 0
    # a map from isdf_set_grid has no counts; a ctx without a map; a multi-device ctx
    occ = (mu._counts(cloud) >= THR).astype(np.uint8)
    grid = mu._grid_engine(pkg, occ)
    kept = _products(pkg, grid, counts=False)
    bare = pkg.Engine(pkg.synth.default_config(capi.V1_SWEPT))
    multi = pkg.Engine(pkg.synth.default_config(capi.V3_ESDF_TILE), devices=[0, 0])
    multi.set_pointcloud(cloud, RES, THR, BMIN, BMAX)
    for e, code in ((grid, capi.ISDF_ERR_STATE), (bare, capi.ISDF_ERR_STATE), (multi, capi.ISDF_ERR_UNSUPPORTED)):
        for call in (lambda: e.shift_map((1, 0, 0)), lambda: e.map_follow(BMIN + 1.0, 1)):
            with pytest.raises(pkg.IsdfError) as err:
                call()
            assert err.value.code == code
    _same(_products(pkg, grid, counts=False), kept)
    assert np.array_equal(multi.get_grid(capi.GRID_OCCUPANCY)[0], occ) and np.array_equal(multi.get_grid(capi.GRID_OCCUPANCY)[1], BMIN)


def test_without_esdf_and_front_end_only_counts_and_occupancy_move(pkg, product_lib):
    capi = pkg.capi
    s = (2, -1, 5)
    c_old = mu._counts(_scene())
    bare = mu._engine(pkg, _scene(), esdf=False, frontend=False)
    info = bare.shift_map(s, force_path=1)
    _check_info(pkg, info, s, c_old, True, False, frontend=False)
    assert (info.n_boxes, info.cspace_voxels, info.field_dropped, info.watch_rechecked) == (0, 0, 0, 0)
    _same(_products(pkg, bare, esdf=False, frontend=False), _products(pkg, _fresh(pkg, _shift(c_old, s), s, esdf=False, frontend=False), esdf=False, frontend=False))
    for call in (lambda e: e.get_grid(capi.GRID_ESDF), lambda e: e.frontend_map_kernel()):
        with pytest.raises(pkg.IsdfError) as err:
            call(bare)
        assert err.value.code == capi.ISDF_ERR_STATE
    # a front end without a configuration-space pass: the bit map alone moves, and a later pass sees it
    nocs = mu._engine(pkg, _scene(), cspace=False)
    info = nocs.shift_map(s, force_path=1)
    assert info.path == 1 and (info.n_boxes, info.cspace_voxels) == (0, 0)
    _same(_products(pkg, nocs, table="compute"), _products(pkg, _fresh(pkg, _shift(c_old, s), s)))


def test_the_counters_where_the_last_wavefront_is_part_filled(pkg, product_lib):
    """5 x 7 x 67 = 2345 voxels: the counts' kernel runs nine whole workgroups and 41 lanes, the occupancy's (587 dwords) two and 75 lanes,
    and the leaving voxels of these shifts lie in the first workgroups, in the last lanes, or in all of them"""
    dims = (5, 7, 67)
    rng = np.random.default_rng(67)
    counts = (rng.integers(1, 4, dims) * (rng.uniform(size=dims) < 0.5)).astype(np.uint32)
    cells = np.argwhere(counts > 0)
    eng = pkg.Engine(pkg.synth.default_config(pkg.capi.V1_SWEPT))
    assert eng.set_pointcloud(_in_cells_at(np.zeros(3), cells, counts[tuple(cells.T)].astype(np.int64), rng), RES, THR, np.zeros(3), np.array(dims) * RES) == dims
    assert np.array_equal(eng.map_counts(), counts)
    idx = np.stack(np.meshgrid(*[np.arange(n) for n in dims], indexing="ij"), axis=-1)
    for s in ((-1, 0, 0), (0, 0, 3), (0, -2, 0), (1, 2, -30)):         # (each leaves through a face that still holds points)
        c_old = eng.map_counts()
        gone = ((idx - np.array(s) < 0) | (idx - np.array(s) >= np.array(dims))).any(axis=-1)
        info = eng.shift_map(s, force_path=2)
        assert np.array_equal(eng.map_counts(), pkg.shift_grid_host(c_old, s, lib=product_lib)), s
        assert np.array_equal(eng.get_grid(pkg.capi.GRID_OCCUPANCY)[0] != 0, eng.map_counts() >= THR), s
        assert (info.counts_left, info.occupied_left) == (int(c_old[gone].sum()), int(((c_old >= THR) & gone).sum())), s
        assert info.counts_left > 0 and info.occupied_left > 0, s


# ---- 6. isdf_map_follow ---------------------------------------------------------------------------------------------------------------------
def test_map_follow(pkg, product_lib):
    capi = pkg.capi
    c_old = mu._counts(_scene())
    mid = D // 2
    eng = mu._engine(pkg, _scene(), host_table=True)
    before = _products(pkg, eng, host_table=True)
    s, info = eng.map_follow((mid + 0.3) * RES + BMIN, 1)          # inside the middle voxel
    assert s == (0, 0, 0) and info.path == 0
    off = (mid + np.array([3, -2, 1]) + 0.5) * RES + BMIN           # 3 voxels off at the most
    s, info = eng.map_follow(off, 4)
    assert s == (0, 0, 0) and info.path == 0
    _same(_products(pkg, eng, host_table=True), before)
    s, info = eng.map_follow(off, 2, full_fraction=1.0)
    assert s == (3, -2, 1) and tuple(info.shift) == s and info.path == 1
    other = mu._engine(pkg, _scene(), host_table=True)
    assert other.shift_map(s, full_fraction=1.0).path == 1
    want = _products(pkg, other, host_table=True)
    _same(_products(pkg, eng, host_table=True), want)
    _same(want, _products(pkg, _fresh(pkg, _shift(c_old, s), s, host_table=True), host_table=True))
    s2, info = eng.map_follow(off, 1)                               # the centre is in the middle voxel now
    assert s2 == (0, 0, 0) and info.path == 0
    # a centre outside the map: the formula extends
    far = mu._engine(pkg, _scene())
    centre = BMIN + np.array([-3.2, 30.1, 7.0])
    want_s = tuple(int(v) for v in np.floor((centre - BMIN) / RES).astype(int) - mid)
    assert want_s[0] < -DIMS[0] // 2 and want_s[1] > DIMS[1]
    s3, info = far.map_follow(centre, 1)
    assert s3 == want_s and info.path == capi.MAP_SHIFT_FULL          # |s_y| >= dims_y: everything left
    _same(_products(pkg, far), _products(pkg, _fresh(pkg, _shift(c_old, s3), s3)))
    again, info = far.map_follow(centre, 1)
    assert again == (0, 0, 0) and info.path == 0
    for bad in ((float("nan"), 3.0, 3.0), (1.0, float("inf"), 3.0), (1.0, 2.0, 1e300)):
        with pytest.raises(pkg.IsdfError) as err:
            far.map_follow(bad, 1)
        assert err.value.code == capi.ISDF_ERR_INVALID_ARG
    with pytest.raises(pkg.IsdfError) as err:
        far.map_follow(centre, -1)
    assert err.value.code == capi.ISDF_ERR_INVALID_ARG
    assert np.array_equal(far.get_grid(capi.GRID_OCCUPANCY)[1], _box(s3)[0])
