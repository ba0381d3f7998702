"""The map updated in place (csrc/map_update.hip: isdf_update_pointcloud / isdf_update_voxels) against the project's own from-scratch
build in a second, fresh ctx on the concatenated cloud - never against the update path itself.  Every comparison is == on bytes.
Shapes: 24 x 20 x 70 voxels at 0.5 m (Z crosses one 64-lane block and is a multiple of neither 32 nor 64), explicit boundaries,
sta_threshold 2, a few hundred seeded points, a box robot with kernel_size 5 and 3 x 3 attitudes."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DIMS = (24, 20, 70)
RES = 0.5
BMIN = np.array([-1.0, 2.0, 0.5])
BMAX = BMIN + np.array(DIMS) * RES
THR = 2
SIDE = 2                                    # (kernel_size - 1) / 2
# The seeded clouds scatter their new voxels over the whole map: the grown dirty box holds nearly all of it, which the default
# full_fraction would send down the full path.  The incremental path is forced through params, as the full one is.
INCR = {"full_fraction": 1.0}


# ---- numpy's view of the binning (getGridIndex): only to choose the clouds and to state what the tests expect of them
def _bin(xyz):
    p = np.asarray(xyz, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    inside = ~((p < BMIN).any(axis=1) | (p > BMAX).any(axis=1))
    idx = np.minimum(np.floor((p - BMIN) / RES).astype(np.int64), np.array(DIMS) - 1)
    idx[~inside] = 0
    return idx, inside


def _counts(xyz):
    c = np.zeros(DIMS, dtype=np.uint32)
    if len(xyz):
        np.add.at(c, tuple(_bin(xyz)[0].T), 1)
    return c


def _in_cells(cells, per_cell, rng):
    """per_cell[i] points inside voxel cells[i], well away from its faces (float32 rounding cannot move them out)"""
    cells = np.repeat(np.asarray(cells, dtype=np.float64).reshape(-1, 3), per_cell, axis=0)
    return ((cells + rng.uniform(0.15, 0.85, cells.shape)) * RES + BMIN).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _clouds():
    """old: 150 voxels with 1..3 points; a: single points that complete some of old's one-point voxels, fresh voxels with two points,
    points into occupied voxels, lone points that stay below the threshold, points outside the map; b: a second such frame."""
    rng = np.random.default_rng(20)
    flat = rng.choice(np.prod(DIMS), 150 + 40, replace=False)
    cells = np.stack(np.unravel_index(flat, DIMS), axis=1)
    cells = cells[(cells != 0).any(axis=1)]                 # voxel (0, 0, 0) is kept for the points outside the map
    per = rng.integers(1, 4, 150)
    old = _in_cells(cells[:150], per, rng)
    ones, full = cells[:150][per == 1], cells[:150][per >= 2]
    spare = cells[150:]
    outside = np.array([[-3.0, 5.0, 5.0], [4.0, 40.0, 5.0]], dtype=np.float32)
    a = np.concatenate([_in_cells(ones[:8], 1, rng), _in_cells(spare[:10], 2, rng), _in_cells(full[:6], 1, rng), _in_cells(spare[10:14], 1, rng), outside])
    b = np.concatenate([_in_cells(ones[8:14], 1, rng), _in_cells(spare[10:14], 1, rng), _in_cells(spare[14:20], 2, rng), _in_cells(full[6:9], 2, rng)])
    rng.shuffle(a); rng.shuffle(b)
    return old, a, b


def _box_shape(pkg):
    return pkg.synth.make_shape("Box", params=(0.9, 0.2, 0.15))


def _fe_cfg(pkg):
    return pkg.capi.frontend_config(kernel_size=5, max_roll=30.0, max_pitch=30.0, ang_res=30.0, safeh=0.0)


def _engine(pkg, cloud, **derive):
    eng = pkg.Engine(pkg.synth.default_config(pkg.capi.V1_SWEPT))
    assert eng.set_pointcloud(cloud, RES, THR, BMIN, BMAX) == DIMS
    _derive(pkg, eng, **derive)
    return eng


def _derive(pkg, eng, shape=None, esdf=True, frontend=True, cspace=True, host_table=False, fe=None):
    """host_table: a search (its start outside the map, so nothing is searched) brings the table to the host, where the A* keeps it"""
    if esdf:
        eng.generate_esdf()
    if frontend:
        if isinstance(shape, tuple):
            eng.set_shape_program(shape[0])
        else:
            eng.set_shape(shape if shape is not None else _box_shape(pkg))
        eng.frontend_build(fe if fe is not None else _fe_cfg(pkg))
        if cspace:
            eng.frontend_cspace(download=False)
        if host_table:
            assert eng.frontend_astar(BMIN - 1.0, BMIN + 1.0)[3].table_ms > 0


@functools.lru_cache(maxsize=None)
def _sample_points():
    rng = np.random.default_rng(7)
    return rng.uniform(BMIN - 0.3, BMAX + 0.3, (200, 3))


def _products(pkg, eng, counts=True, esdf=True, frontend=True, table="kept", host_table=False):
    """table "kept": the configuration space AS IT STANDS in the ctx (isdf_frontend_cspace_get - after an update that is what the boxed
    kernel left; isdf_frontend_cspace would run the whole-map kernel again and hide it); "compute": there is none yet, run the pass.
    host_table: the A*'s host copy as it stands, whole.  Both are read before anything else can touch them."""
    capi = pkg.capi
    out = {"occ": eng.get_grid(capi.GRID_OCCUPANCY)[0]}
    if counts:
        out["counts"] = eng.map_counts()
    if esdf:
        out["esdf"] = eng.get_grid(capi.GRID_ESDF)[0]
        out["sample_value"], out["sample_grad"] = eng.esdf_sample(_sample_points(), scattered=True)       # through the (stale) bricks
    if frontend:
        out["cspace"] = eng.frontend_cspace_table() if table == "kept" else eng.frontend_cspace()[0]
        if host_table:
            out["host_table"] = eng.frontend_cspace_table(host=True)
        out["map_kernel"] = eng.frontend_map_kernel()
    eng.gather_points([(BMIN + BMAX) / 2], (3.0, 3.0, 3.0))                                                  # through the (stale) bit grid
    out["gathered"] = eng.get_points()
    return out


def _same(got, want):
    assert got.keys() == want.keys()
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), k          # bytes: NaN and -0 included


def _numpy_box(occ_old, occ_new):
    new = np.argwhere((occ_new == 1) & (occ_old == 0))
    return new.min(axis=0).tolist(), new.max(axis=0).tolist(), len(new)


# ---- 1. products equal, on both paths -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("forced", ["incremental", "full_by_max_new_voxels", "full_by_fraction"])
def test_products_equal_a_fresh_build(pkg, product_lib, forced):
    capi = pkg.capi
    old, a, _ = _clouds()
    c_old, c_new, c_all = _counts(old), _counts(a), _counts(np.concatenate([old, a]))
    crossing = (c_all >= THR) & (c_old < THR)
    assert 5 <= crossing.sum() <= 100
    assert (crossing & (c_old > 0) & (c_new < THR)).any()            # a voxel that crosses only by old and new points together
    assert 300 <= len(old) + len(a) <= 400 and 30 <= len(a) <= 50
    incr = forced == "incremental"
    eng = _engine(pkg, old, host_table=incr)
    params = {"incremental": INCR, "full_by_max_new_voxels": {"max_new_voxels": 0}, "full_by_fraction": {"full_fraction": 0.0}}[forced]
    info = eng.update_pointcloud(a, **params)
    print(f"\n{forced}: new {info.n_new_voxels}, lowered {info.esdf_voxels_lowered}, cspace voxels {info.cspace_voxels_recomputed}, "
          f"count {info.count_ms:.3f} esdf {info.esdf_ms:.3f} frontend {info.frontend_ms:.3f} ms")
    assert info.path == (capi.MAP_UPDATE_INCREMENTAL if forced == "incremental" else capi.MAP_UPDATE_FULL)
    assert info.n_points == len(a) and info.n_new_voxels == crossing.sum()
    lo, hi, _ = _numpy_box(c_old >= THR, c_all >= THR)
    assert list(info.dirty_lo) == lo and list(info.dirty_hi) == hi
    assert (info.esdf_refreshed, info.frontend_refreshed, info.cspace_refreshed, info.host_table_patched, info.field_dropped) == (1, 1, 1, int(incr), 0)
    fresh = _engine(pkg, np.concatenate([old, a]), host_table=incr)
    want = _products(pkg, fresh, host_table=incr)
    _same(_products(pkg, eng, host_table=incr), want)
    assert np.array_equal(want["cspace"], fresh.frontend_cspace()[0]) and want["cspace"].any()
    assert np.array_equal(want["counts"], c_all) and np.array_equal(want["occ"], (c_all >= THR).astype(np.uint8))
    if forced == "incremental":
        before = _engine(pkg, old).get_grid(capi.GRID_ESDF)[0]
        assert info.esdf_voxels_lowered == (want["esdf"] < before).sum() > 0
        g_lo = np.maximum(np.array(lo) - SIDE, 0); g_hi = np.minimum(np.array(hi) + SIDE, np.array(DIMS) - 1)
        assert info.cspace_voxels_recomputed == np.prod(g_hi - g_lo + 1)


# ---- 2. edges of the box --------------------------------------------------------------------------------------------------------
def test_box_clamps_on_every_side_and_crosses_the_z_split(pkg, product_lib):
    old, _, _ = _clouds()
    rng = np.random.default_rng(3)
    X, Y, Z = DIMS
    outside = np.array([[-3.0, 5.0, 5.0], [0.0, 2.5, 36.0], [5.0, 5.0, 0.49]], dtype=np.float32)              # the three land in voxel (0, 0, 0)
    new = np.concatenate([outside, _in_cells([(X - 1, Y - 1, Z - 1), (10, 10, 63), (10, 10, 64)], 2, rng)])
    assert not _bin(outside)[1].any() and _counts(old)[0, 0, 0] == 0
    eng = _engine(pkg, old, host_table=True)
    info = eng.update_pointcloud(new, **INCR)
    c_old, c_all = _counts(old), _counts(np.concatenate([old, new]))
    assert eng.map_counts()[0, 0, 0] == 3                                  # the points outside the map count for voxel (0, 0, 0)
    lo, hi, n_new = _numpy_box(c_old >= THR, c_all >= THR)
    assert (lo, hi, n_new) == ([0, 0, 0], [X - 1, Y - 1, Z - 1], 4)
    assert info.path == 1 and info.n_new_voxels == 4 and list(info.dirty_lo) == lo and list(info.dirty_hi) == hi
    assert info.cspace_voxels_recomputed == X * Y * Z                      # (the grown box is the map, clamped on all six sides)
    assert info.host_table_patched == 1
    _same(_products(pkg, eng, host_table=True), _products(pkg, _engine(pkg, np.concatenate([old, new]), host_table=True), host_table=True))
    # the column alone: a box of 1 x 1 x 2 voxels whose grown box starts at z = 61 and ends at z = 66
    eng2 = _engine(pkg, old, host_table=True)
    col = _in_cells([(10, 10, 63), (10, 10, 64)], 2, rng)
    info2 = eng2.update_pointcloud(col)
    assert list(info2.dirty_lo) == [10, 10, 63] and list(info2.dirty_hi) == [10, 10, 64] and info2.cspace_voxels_recomputed == 5 * 5 * 6
    _same(_products(pkg, eng2, host_table=True), _products(pkg, _engine(pkg, np.concatenate([old, col]), host_table=True), host_table=True))
    # the words outside the grown box were not written: those of the map before, which differ from the fresh ones nowhere else
    before = _engine(pkg, old).frontend_cspace()[0]
    differs = (before != eng2.frontend_cspace_table()).any(axis=3)
    assert differs.any() and not differs[:8].any() and not differs[13:].any() and not differs[:, :8].any() and not differs[:, 13:].any() and not differs[:, :, :61].any() and not differs[:, :, 67:].any()


# ---- 3. nothing new; the cost-to-go field ---------------------------------------------------------------------------------------
def test_nothing_new_keeps_everything_and_a_new_voxel_drops_the_field(pkg, product_lib):
    capi = pkg.capi
    old, a, _ = _clouds()
    c_old = _counts(old)
    rng = np.random.default_rng(5)
    occupied = np.argwhere(c_old >= THR)[:5]
    empty = np.argwhere(c_old == 0)[5:9]
    quiet = np.concatenate([_in_cells(occupied, 2, rng), _in_cells(empty, 1, rng)])
    eng = _engine(pkg, old)
    before = _products(pkg, eng, counts=False)
    free = before["cspace"].any(axis=3)
    goal = np.argwhere(free)[len(np.argwhere(free)) // 2]
    finfo = eng.frontend_field_build((goal + 0.5) * RES + BMIN)
    assert finfo.reachable == 1
    field = eng.frontend_field()
    info = eng.update_pointcloud(quiet)
    assert info.path == capi.MAP_UPDATE_NONE and info.n_new_voxels == 0 and info.n_points == len(quiet)
    assert list(info.dirty_lo) > list(info.dirty_hi) and info.field_dropped == 0 and info.esdf_refreshed == 0 and info.frontend_refreshed == 0
    assert np.array_equal(eng.frontend_field().view(np.uint8), field.view(np.uint8))
    _same(_products(pkg, eng, counts=False), before)
    assert np.array_equal(eng.map_counts(), _counts(np.concatenate([old, quiet])))
    # a new voxel: the field goes, and its entry points answer as they do before a build
    info = eng.update_pointcloud(_in_cells(empty[:1], 1, rng))               # the second point of that voxel
    assert info.n_new_voxels == 1 and info.field_dropped == 1
    never = _engine(pkg, old)
    for e in (eng, never):
        with pytest.raises(pkg.IsdfError) as err:
            e.frontend_field()
        assert err.value.code == capi.ISDF_ERR_STATE
        with pytest.raises(pkg.IsdfError) as err:
            e.frontend_field_paths([(goal + 0.5) * RES + BMIN], 8)
        assert err.value.code == capi.ISDF_ERR_STATE
    assert eng.frontend_field_build((goal + 0.5) * RES + BMIN).status in (0, 1)        # and it can be built again


# ---- 4. two steps equal one -----------------------------------------------------------------------------------------------------
def test_two_updates_equal_one(pkg, product_lib):
    old, a, b = _clouds()
    c_oa, c_all = _counts(np.concatenate([old, a])), _counts(np.concatenate([old, a, b]))
    assert ((c_all >= THR) & (c_oa < THR)).sum() >= 5
    assert ((c_all >= THR) & (c_oa == 1) & (_counts(a) == 1) & (_counts(old) == 0)).any()      # a voxel completed by one point of a and one of b
    two = _engine(pkg, old, host_table=True)
    i1, i2 = two.update_pointcloud(a, **INCR), two.update_pointcloud(b, **INCR)
    one = _engine(pkg, old, host_table=True)
    i3 = one.update_pointcloud(np.concatenate([a, b]), **INCR)
    assert i1.path == i2.path == i3.path == 1 and i1.n_new_voxels + i2.n_new_voxels == i3.n_new_voxels
    assert i1.host_table_patched == i2.host_table_patched == i3.host_table_patched == 1
    want = _products(pkg, _engine(pkg, np.concatenate([old, a, b]), host_table=True), host_table=True)
    _same(_products(pkg, two, host_table=True), want)
    _same(_products(pkg, one, host_table=True), want)


# ---- 5. the A* over a patched host table ----------------------------------------------------------------------------------------
def _wall_clouds():
    """A floor at z = 35 with two openings of 5 x 5 voxels; the update closes the one above the start."""
    rng = np.random.default_rng(9)
    X, Y, _ = DIMS
    plane = np.array([(x, y, 35) for x in range(X) for y in range(Y)])
    in_a = (np.abs(plane[:, 0] - 5) <= 2) & (np.abs(plane[:, 1] - 5) <= 2)
    in_b = (np.abs(plane[:, 0] - 18) <= 2) & (np.abs(plane[:, 1] - 14) <= 2)
    return _in_cells(plane[~in_a & ~in_b], 2, rng), _in_cells(plane[in_a], 2, rng)


def test_astar_over_the_patched_host_table(pkg, orc, product_lib):
    capi, synth = pkg.capi, pkg.synth
    old, plug = _wall_clouds()
    start, goal = (np.array([5, 5, 30]) + 0.5) * RES + BMIN, (np.array([5, 5, 40]) + 0.5) * RES + BMIN
    eng = _engine(pkg, old)
    xyz0, _, _, r0 = eng.frontend_astar(start, goal)                        # the host table is valid from here on
    assert r0.success == 1 and r0.table_ms > 0 and r0.n_path == 11          # straight up through the opening
    info = eng.update_pointcloud(plug)
    assert info.path == 1 and info.n_new_voxels == 25 and info.host_table_patched == 1
    # the oracle's A* on the union map still finds a way (through the other opening)
    occ_all = (_counts(np.concatenate([old, plug])) >= THR).astype(np.uint8)
    o = orc.Oracle(synth.default_config(capi.V1_SWEPT), threads=16)
    o.set_grid(occ_all, BMIN, RES, capi.GRID_OCCUPANCY)
    o.set_shape(_box_shape(pkg)); o.frontend_build(_fe_cfg(pkg))
    x_or, rp_or, st = o.frontend_astar(start, goal)
    assert x_or is not None and len(x_or) > 11
    xyz1, rp1, _, r1 = eng.frontend_astar(start, goal)
    assert r1.table_ms == 0                                                 # the patched table was used, not a new copy of the whole one
    fresh = _engine(pkg, np.concatenate([old, plug]))
    xyz2, rp2, _, r2 = fresh.frontend_astar(start, goal)
    assert r2.success == 1 and r2.table_ms > 0
    assert np.array_equal(xyz1, xyz2) and np.array_equal(rp1, rp2)
    assert (r1.success, r1.n_path, r1.expansions, r1.checks) == (r2.success, r2.n_path, r2.expansions, r2.checks)
    assert np.array_equal(xyz1, x_or) and np.array_equal(rp1, rp_or) and (r1.checks, r1.expansions) == (st["checks"], st["expansions"])
    assert not np.array_equal(xyz0, xyz1[:len(xyz0)])
    assert np.array_equal(eng.frontend_cspace_table(host=True), fresh.frontend_cspace_table(host=True))        # the patched copy, whole
    assert np.array_equal(eng.frontend_cspace_table(), fresh.frontend_cspace_table())
    # the full path invalidates the host table instead: the next search fetches it again, with the same result
    eng3 = _engine(pkg, old)
    eng3.frontend_astar(start, goal)
    info3 = eng3.update_pointcloud(plug, max_new_voxels=0)
    assert info3.path == 2 and info3.host_table_patched == 0
    with pytest.raises(pkg.IsdfError) as err:
        eng3.frontend_cspace_table(host=True)
    assert err.value.code == capi.ISDF_ERR_STATE
    xyz3, rp3, _, r3 = eng3.frontend_astar(start, goal)
    assert r3.table_ms > 0 and np.array_equal(xyz3, xyz2) and np.array_equal(rp3, rp2) and r3.checks == r2.checks


# ---- 6. the voxel form ----------------------------------------------------------------------------------------------------------
def _grid_engine(pkg, occ, **derive):
    eng = pkg.Engine(pkg.synth.default_config(pkg.capi.V1_SWEPT))
    eng.set_grid(occ, BMIN, RES, pkg.capi.GRID_OCCUPANCY, bmax=BMAX)
    _derive(pkg, eng, **derive)
    return eng


@pytest.mark.parametrize("forced", ["incremental", "full"])
def test_voxel_form(pkg, product_lib, forced):
    capi = pkg.capi
    occ = (_counts(_clouds()[0]) >= THR).astype(np.uint8)
    rng = np.random.default_rng(11)
    empty, taken = np.argwhere(occ == 0), np.argwhere(occ == 1)
    fresh_cells = empty[rng.choice(len(empty), 30, replace=False)]
    fresh_cells = np.concatenate([fresh_cells, [[0, 0, 69], [23, 19, 0]]])          # the last byte of a row that is no multiple of 4, a far corner
    ijk = np.concatenate([fresh_cells, fresh_cells[:7], taken[:5], fresh_cells[3:4]]).astype(np.int32)      # duplicates and occupied voxels
    rng.shuffle(ijk)
    edited = occ.copy()
    edited[tuple(ijk.T)] = 1
    incr = forced == "incremental"
    eng = _grid_engine(pkg, occ, host_table=incr)
    info = eng.update_voxels(ijk, **(INCR if incr else {"max_new_voxels": 3}))
    assert info.host_table_patched == int(incr)
    assert info.path == (1 if forced == "incremental" else 2) and info.n_points == len(ijk) and info.n_new_voxels == 32
    lo, hi, _ = _numpy_box(occ, edited)
    assert list(info.dirty_lo) == lo and list(info.dirty_hi) == hi
    want = _products(pkg, _grid_engine(pkg, edited, host_table=incr), counts=False, host_table=incr)
    _same(_products(pkg, eng, counts=False, host_table=incr), want)
    assert np.array_equal(want["occ"], edited)
    # an index outside the grid: refused, nothing changed
    for bad in ([[1, 1, 70]], [[24, 0, 0]], [[3, 3, 3], [0, -1, 0]]):
        with pytest.raises(pkg.IsdfError) as err:
            eng.update_voxels(bad)
        assert err.value.code == capi.ISDF_ERR_INVALID_ARG
    assert np.array_equal(eng.get_grid(capi.GRID_OCCUPANCY)[0], edited)
    # no counts on a map from isdf_set_grid
    for call in (lambda: eng.update_pointcloud(_clouds()[1]), eng.map_counts):
        with pytest.raises(pkg.IsdfError) as err:
            call()
        assert err.value.code == capi.ISDF_ERR_STATE


def test_status_codes_of_the_pointcloud_form(pkg, product_lib):
    capi = pkg.capi
    old, a, _ = _clouds()
    eng = _engine(pkg, old, esdf=False, frontend=False)
    assert eng.update_voxels(np.argwhere(_counts(old) >= THR)[:3]).n_new_voxels == 0
    assert eng.update_pointcloud(a[:1]).n_points == 1                      # (an update_voxels that occupied nothing leaves the counts in place)
    assert eng.update_voxels(np.argwhere(_counts(old) == 0)[:1]).n_new_voxels == 1
    with pytest.raises(pkg.IsdfError) as err:
        eng.update_pointcloud(a)
    assert err.value.code == capi.ISDF_ERR_STATE
    multi = pkg.Engine(pkg.synth.default_config(capi.V3_ESDF_TILE), devices=[0, 0])
    multi.set_pointcloud(old, RES, THR, BMIN, BMAX)
    for call in (lambda: multi.update_pointcloud(a), lambda: multi.update_voxels([[1, 1, 1]])):
        with pytest.raises(pkg.IsdfError) as err:
            call()
        assert err.value.code == capi.ISDF_ERR_UNSUPPORTED


# ---- 7. no ESDF, no front end, the switches off ---------------------------------------------------------------------------------
def test_without_products_and_with_the_switches_off(pkg, product_lib):
    capi = pkg.capi
    old, a, _ = _clouds()
    both = np.concatenate([old, a])
    bare = _engine(pkg, old, esdf=False, frontend=False)
    info = bare.update_pointcloud(a, **INCR)
    assert info.path == 1 and info.n_new_voxels > 0
    assert (info.esdf_refreshed, info.frontend_refreshed, info.cspace_refreshed, info.host_table_patched, info.field_dropped) == (0, 0, 0, 0, 0)
    assert info.esdf_voxels_lowered == 0 and info.cspace_voxels_recomputed == 0
    _same(_products(pkg, bare, esdf=False, frontend=False), _products(pkg, _engine(pkg, both, esdf=False, frontend=False), esdf=False, frontend=False))
    for call in (lambda e: e.get_grid(capi.GRID_ESDF), lambda e: e.frontend_map_kernel()):
        with pytest.raises(pkg.IsdfError) as err:
            call(bare)
        assert err.value.code == capi.ISDF_ERR_STATE
    # a front end without a configuration-space pass: the bit map alone is refreshed, and a later pass sees it
    nocs = _engine(pkg, old, cspace=False)
    info = nocs.update_pointcloud(a, **INCR)
    assert (info.frontend_refreshed, info.cspace_refreshed, info.cspace_voxels_recomputed) == (1, 0, 0)
    with pytest.raises(pkg.IsdfError) as err:
        nocs.frontend_cspace_table()
    assert err.value.code == capi.ISDF_ERR_STATE
    want = _products(pkg, _engine(pkg, both))
    _same(_products(pkg, nocs, table="compute"), want)
    # refresh_esdf = 0 drops the ESDF, refresh_frontend = 0 releases the front end - each as before a build; the other product is refreshed
    for off, gone, kept in (("refresh_esdf", lambda e: e.get_grid(capi.GRID_ESDF), ("map_kernel", "cspace")),
                            ("refresh_frontend", lambda e: e.frontend_map_kernel(), ("esdf", "sample_value", "sample_grad"))):
        eng = _engine(pkg, old)
        info = eng.update_pointcloud(a, **{off: False}, **INCR)
        assert info.path == 1 and (info.esdf_refreshed, info.frontend_refreshed) == ((0, 1) if off == "refresh_esdf" else (1, 0))
        with pytest.raises(pkg.IsdfError) as err:
            gone(eng)
        assert err.value.code == capi.ISDF_ERR_STATE
        got = _products(pkg, eng, esdf=off != "refresh_esdf", frontend=off != "refresh_frontend")
        for k in kept + ("occ", "counts", "gathered"):
            assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), (off, k)


def test_esdf_of_an_empty_map_takes_the_full_path(pkg, product_lib):
    old, a, _ = _clouds()
    c = _counts(old)
    lone = _in_cells(np.argwhere(c == 0)[:20], 1, np.random.default_rng(1))       # no voxel reaches the threshold
    eng = _engine(pkg, lone)
    assert not eng.get_grid(pkg.capi.GRID_OCCUPANCY)[0].any() and np.isinf(eng.get_grid(pkg.capi.GRID_ESDF)[0]).all()
    info = eng.update_pointcloud(a)
    assert info.path == 2 and info.n_new_voxels > 0
    _same(_products(pkg, eng), _products(pkg, _engine(pkg, np.concatenate([lone, a]))))


# ---- 8. mesh and program robots: the boxed pass reads the same row lists as the whole-map one -----------------------------------
@pytest.mark.parametrize("robot", ["program", "mybox", "box_169_attitudes"])
def test_cspace_of_other_robot_kinds(pkg, product_lib, robot):
    """The table and the host copy AS THE UPDATE LEFT THEM (isdf_frontend_cspace_get), against a fresh ctx's whole-map pass.  169 attitudes
    (13 x 13): two 128-attitude groups per voxel, the second partly filled."""
    old, a, _ = _clouds()
    shape = fe = None
    if robot == "program":
        csg = pkg.csg
        shape = (csg.unionOp(csg.box((0.8, 0.3, 0.2)), csg.translate(csg.sphere(0.35), (0.5, 0.0, 0.2))),)
    elif robot == "mybox":
        from benchlib.meshes import reference_mesh
        shape = pkg.synth.make_mesh_shape(*reference_mesh("mybox", bound_radius=1.0))
    else:
        fe = pkg.capi.frontend_config(kernel_size=5, max_roll=30.0, max_pitch=30.0, ang_res=5.0, safeh=0.0)
    eng = _engine(pkg, old, shape=shape, fe=fe, host_table=True)
    info = eng.update_pointcloud(a, **INCR)
    assert info.path == 1 and info.cspace_refreshed == 1 and info.host_table_patched == 1
    got, got_host = eng.frontend_cspace_table(), eng.frontend_cspace_table(host=True)
    fresh = _engine(pkg, np.concatenate([old, a]), shape=shape, fe=fe)
    want = fresh.frontend_cspace()[0]
    assert want.shape == DIMS + (8 if fe is not None else 4,)
    assert np.array_equal(got, want) and np.array_equal(got_host, want) and want.any() and not want.all()
    assert fe is None or (want[..., 4:].any() and (want[..., 5] >> 9 == 0).all() and not want[..., 6:].any())      # bits 169 .. 255 stay clear
    assert not np.array_equal(want, _engine(pkg, old, shape=shape, fe=fe).frontend_cspace()[0])                    # (the update had something to change)
    assert np.array_equal(eng.frontend_map_kernel(), fresh.frontend_map_kernel())


# ---- 9. nothing is allocated after the first call of a size -----------------------------------------------------------------------
def _live(lib):
    out = (C.c_longlong * 2)()
    lib.isdf_debug_live_bytes(out)
    return list(out)


def test_a_second_update_of_the_same_size_allocates_nothing(pkg, product_lib):
    old, a, _ = _clouds()
    eng = _engine(pkg, old, host_table=True)
    assert eng.update_pointcloud(a, **INCR).path == 1
    first = _products(pkg, eng, host_table=True)
    # the same map again in the same ctx, whose update scratch stays; then the same update
    assert eng.set_pointcloud(old, RES, THR, BMIN, BMAX) == DIMS
    _derive(pkg, eng, host_table=True)
    before = _live(product_lib)
    info = eng.update_pointcloud(a, **INCR)
    assert _live(product_lib) == before
    assert info.path == 1 and info.n_new_voxels > 0 and info.host_table_patched == 1
    _same(_products(pkg, eng, host_table=True), first)
