"""Voxels cleared from the map in place (csrc/map_clear.hip: isdf_clear_pointcloud / isdf_clear_voxels) against the project's own
from-scratch build in a second, fresh ctx on what is left - never against the clear path itself.  Every comparison is == on bytes.
The geometry, the robot and the helpers are those of tests/test_gpu_map_update.py: 24 x 20 x 70 voxels at 0.5 m, sta_threshold 2, a box
robot with kernel_size 5 and 3 x 3 attitudes."""
import functools

import numpy as np
import pytest

import test_gpu_map_update as mu
from test_gpu_map_update import BMAX, BMIN, DIMS, RES, SIDE, THR, _counts, _engine, _grid_engine, _in_cells, _live, _products, _same

pytestmark = pytest.mark.gpu

INCR = {"full_fraction": 1.0}               # the incremental path whatever share of this small map the boxes hold
N_VOX = int(np.prod(DIMS))


def _edt(occ):
    """numpy's exact transform, as isdf_generate_esdf converts it (an occupied voxel exists)"""
    idx = np.stack(np.meshgrid(*[np.arange(n) for n in DIMS], indexing="ij"), axis=-1).reshape(-1, 3).astype(np.int32)
    o = np.argwhere(occ == 1).astype(np.int32)
    d2 = np.full(len(idx), np.iinfo(np.int64).max, dtype=np.int64)
    for k in range(0, len(o), 32):
        d2 = np.minimum(d2, ((idx[:, None, :] - o[None, k:k + 32, :]).astype(np.int64) ** 2).sum(axis=2).min(axis=1))
    return (np.float64(RES) * np.sqrt(d2.astype(np.float64))).astype(np.float32).reshape(DIMS)


@functools.lru_cache(maxsize=None)
def _scene():
    """old cloud and the points to take out of it.  Voxel groups: A two points, one removed (falls below the threshold); B three points,
    two removed (falls only through both together); C three points, one removed (stays occupied); D one point (free already), two removed
    (one of them finds the count at 0); the rest untouched.  Plus a removal in a voxel without points and one outside the map."""
    rng = np.random.default_rng(31)
    flat = rng.choice(N_VOX, 160, replace=False)
    cells = np.stack(np.unravel_index(flat, DIMS), axis=1)
    cells = cells[(cells != 0).any(axis=1)][:150]
    groups = {"A": (cells[:12], 2, 1), "B": (cells[12:20], 3, 2), "C": (cells[20:30], 3, 1), "D": (cells[30:36], 1, 1)}
    keep, out = [], []
    for g, (cs, n, n_out) in groups.items():
        for c in cs:
            p = _in_cells([c], n, rng)
            out.append(p[:n_out]); keep.append(p[n_out:])
    for c in cells[36:]:
        keep.append(_in_cells([c], int(rng.integers(2, 4)), rng))
    extra = np.concatenate([_in_cells(groups["D"][0], 1, rng),                         # the second removal of D's voxels
                            _in_cells([(1, 1, 1)], 1, rng),                            # a voxel without points
                            np.array([[-3.0, 5.0, 5.0]], dtype=np.float32)])            # outside the map: voxel (0, 0, 0), count 0
    keep, out = np.concatenate(keep), np.concatenate(out)
    old = np.concatenate([keep, out])
    removed = np.concatenate([out, extra])
    rng.shuffle(old); rng.shuffle(removed)
    return old, removed, keep, len(extra), {k: v[0] for k, v in groups.items()}


def _numpy_box(cells):
    return cells.min(axis=0).tolist(), cells.max(axis=0).tolist()


# ---- 1. products equal a fresh build on the remaining cloud ---------------------------------------------------------------------
@pytest.mark.parametrize("host_table", [False, True])
@pytest.mark.parametrize("forced", ["incremental", "full_by_max_cleared_voxels", "full_by_fraction"])
def test_products_equal_a_fresh_build(pkg, product_lib, forced, host_table):
    capi = pkg.capi
    old, removed, keep, n_ignored, G = _scene()
    c_old, c_rem, c_keep = _counts(old), _counts(removed), _counts(keep)
    assert c_old[1, 1, 1] == 0 and c_old[0, 0, 0] == 0
    assert np.array_equal(np.where(c_rem > c_old, 0, c_old - c_rem), c_keep)                     # the multiset difference, count by count
    cleared = (c_old >= THR) & (c_keep < THR)
    assert 5 <= cleared.sum() <= 100
    assert (cleared & (c_old - 1 >= THR)).any()                      # falls below the threshold only through several removed points together
    assert ((c_rem > 0) & (c_keep >= THR)).any()                     # loses points, stays occupied
    assert (c_rem > c_old).sum() == n_ignored == np.maximum(c_rem.astype(np.int64) - c_old, 0).sum() > 0      # removals beyond the count
    eng = _engine(pkg, old, host_table=host_table)
    params = {"incremental": INCR, "full_by_max_cleared_voxels": {"max_cleared_voxels": 0}, "full_by_fraction": {"full_fraction": 0.0}}[forced]
    info = eng.clear_pointcloud(removed, **params)
    print(f"\n{forced}: cleared {info.n_cleared_voxels}, ignored {info.n_points_ignored}, raised {info.esdf_voxels_raised}, recomputed {info.esdf_voxels_recomputed}, "
          f"cspace voxels {info.cspace_voxels_recomputed}, count {info.count_ms:.3f} esdf {info.esdf_ms:.3f} frontend {info.frontend_ms:.3f} ms")
    incr = forced == "incremental"
    assert info.path == (capi.MAP_CLEAR_INCREMENTAL if incr else capi.MAP_CLEAR_FULL)
    assert info.n_points == len(removed) and info.n_cleared_voxels == cleared.sum() and info.n_points_ignored == n_ignored
    lo, hi = _numpy_box(np.argwhere(cleared))
    assert list(info.dirty_lo) == lo and list(info.dirty_hi) == hi
    assert (info.esdf_refreshed, info.frontend_refreshed, info.cspace_refreshed, info.host_table_patched) == (1, 1, 1, int(incr and host_table))
    assert (info.field_dropped, info.watch_rechecked) == (0, 0)
    fresh = _engine(pkg, keep, host_table=host_table)
    want = _products(pkg, fresh, host_table=host_table)
    if host_table and not incr:                                     # the full path marks the host copy stale: the next search fetches it again
        with pytest.raises(pkg.IsdfError) as err:
            eng.frontend_cspace_table(host=True)
        assert err.value.code == capi.ISDF_ERR_STATE
        assert eng.frontend_astar(BMIN - 1.0, BMIN + 1.0)[3].table_ms > 0
    _same(_products(pkg, eng, host_table=host_table), want)
    assert np.array_equal(want["cspace"], fresh.frontend_cspace()[0]) and want["cspace"].any()
    assert np.array_equal(want["counts"], c_keep) and np.array_equal(want["occ"], (c_keep >= THR).astype(np.uint8))
    if incr:
        before = _engine(pkg, old, frontend=False).get_grid(capi.GRID_ESDF)[0]
        raised = (want["esdf"].view(np.uint32) != before.view(np.uint32)).sum()
        assert (want["esdf"] >= before).all() and info.esdf_voxels_raised == raised > 0
        t_lo, t_hi = np.array(info.touched_lo), np.array(info.touched_hi)
        assert raised <= info.esdf_voxels_recomputed == np.prod(t_hi - t_lo + 1)
        g_lo = np.maximum(np.array(lo) - SIDE, 0); g_hi = np.minimum(np.array(hi) + SIDE, np.array(DIMS) - 1)
        assert info.cspace_voxels_recomputed == np.prod(g_hi - g_lo + 1)


# ---- 2. locality ------------------------------------------------------------------------------------------------------------------
def test_only_the_neighbourhood_of_a_cleared_cluster_is_recomputed(pkg, product_lib):
    capi = pkg.capi
    rng = np.random.default_rng(2)
    lattice = np.array([(x, y, z) for x in range(3, 24, 6) for y in range(2, 20, 5) for z in range(5, 70, 10)])
    cluster = np.array([(x, y, z) for x in (1, 2) for y in (1, 2) for z in (1, 2)])
    keep, out = _in_cells(lattice, 2, rng), _in_cells(cluster, 2, rng)
    occ_old, occ_new = (_counts(np.concatenate([keep, out])) >= THR).astype(np.uint8), (_counts(keep) >= THR).astype(np.uint8)
    assert occ_old.sum() == len(lattice) + 8 and occ_new.sum() == len(lattice)
    e_old, e_new = _edt(occ_old), _edt(occ_new)
    raised = e_new.view(np.uint32) != e_old.view(np.uint32)
    assert 8 <= raised.sum() < N_VOX // 4
    eng = _engine(pkg, np.concatenate([keep, out]))
    assert np.array_equal(eng.get_grid(capi.GRID_ESDF)[0].view(np.uint32), e_old.view(np.uint32))
    info = eng.clear_pointcloud(out[::2], **INCR)                  # one of each voxel's two points
    t_lo, t_hi = np.array(info.touched_lo), np.array(info.touched_hi)
    print(f"\nlocality: raised {info.esdf_voxels_raised} of {N_VOX}, recomputed {info.esdf_voxels_recomputed}, touched box {t_lo.tolist()} .. {t_hi.tolist()}")
    assert info.path == 1 and info.n_cleared_voxels == 8 and info.n_points_ignored == 0
    assert info.esdf_voxels_raised == raised.sum()
    assert raised.sum() <= info.esdf_voxels_recomputed <= np.prod(t_hi - t_lo + 1)
    r = np.argwhere(raised)
    assert (t_lo <= r.min(axis=0)).all() and (t_hi >= r.max(axis=0)).all()
    assert (t_lo > 0).any() or (t_hi < np.array(DIMS) - 1).any()  # strictly inside the map on at least one side
    got = eng.get_grid(capi.GRID_ESDF)[0]
    assert np.array_equal(got.view(np.uint32), e_new.view(np.uint32))
    _same(_products(pkg, eng), _products(pkg, _engine(pkg, np.concatenate([keep, out[1::2]]))))


# ---- 3. edges of the boxes ----------------------------------------------------------------------------------------------------------
def test_boxes_clamp_on_every_side_and_cross_the_z_split(pkg, product_lib):
    base = mu._clouds()[0]
    rng = np.random.default_rng(3)
    X, Y, Z = DIMS
    corners = _in_cells([(0, 0, 0), (X - 1, Y - 1, Z - 1)], 2, rng)
    col = _in_cells([(10, 10, 63), (10, 10, 64)], 2, rng)
    assert _counts(base)[0, 0, 0] == 0 and _counts(base)[10, 10, 63] == 0 and _counts(base)[10, 10, 64] == 0
    old = np.concatenate([base, corners, col])
    eng = _engine(pkg, old, host_table=True)
    out = np.concatenate([corners[::2], col[::2]])
    info = eng.clear_pointcloud(out, **INCR)
    assert info.path == 1 and info.n_cleared_voxels == 4 and list(info.dirty_lo) == [0, 0, 0] and list(info.dirty_hi) == [X - 1, Y - 1, Z - 1]
    assert info.cspace_voxels_recomputed == N_VOX and info.host_table_patched == 1                 # the grown box is the map, clamped on all six sides
    assert min(info.touched_lo) >= 0 and (np.array(info.touched_hi) < np.array(DIMS)).all()
    assert list(info.touched_lo) == [0, 0, 0] and list(info.touched_hi) == [X - 1, Y - 1, Z - 1]      # the two corners are touched
    keep = np.concatenate([base, corners[1::2], col[1::2]])
    _same(_products(pkg, eng, host_table=True), _products(pkg, _engine(pkg, keep, host_table=True), host_table=True))
    # the column alone: a dirty box of 1 x 1 x 2 voxels whose grown box starts at z = 61; the touched box crosses z = 64
    eng2 = _engine(pkg, old, host_table=True)
    info2 = eng2.clear_pointcloud(col[::2])
    assert info2.path == 1 and list(info2.dirty_lo) == [10, 10, 63] and list(info2.dirty_hi) == [10, 10, 64] and info2.cspace_voxels_recomputed == 5 * 5 * 6
    assert info2.touched_lo[2] < 64 <= info2.touched_hi[2] and info2.esdf_voxels_raised >= 2
    keep2 = np.concatenate([base, corners, col[1::2]])
    fresh2 = _engine(pkg, keep2, host_table=True)
    _same(_products(pkg, eng2, host_table=True), _products(pkg, fresh2, host_table=True))
    # the words outside the grown box were not written: those of the map before, which differ from the fresh ones nowhere else
    before = _engine(pkg, old, esdf=False).frontend_cspace()[0]
    differs = (before != eng2.frontend_cspace_table()).any(axis=3)
    assert differs.any() and not differs[:8].any() and not differs[13:].any() and not differs[:, :8].any() and not differs[:, 13:].any() and not differs[:, :, :61].any() and not differs[:, :, 67:].any()


# ---- 4. there and back; two steps equal one ---------------------------------------------------------------------------------------
def test_update_then_clear_returns_and_two_clears_equal_one(pkg, product_lib):
    old, a, b = mu._clouds()
    want = _products(pkg, _engine(pkg, old, host_table=True), host_table=True)
    eng = _engine(pkg, old, host_table=True)
    up = eng.update_pointcloud(a, **INCR)
    down = eng.clear_pointcloud(a, **INCR)
    assert up.n_new_voxels == down.n_cleared_voxels > 0 and down.n_points_ignored == 0 and down.path == 1
    assert list(up.dirty_lo) == list(down.dirty_lo) and list(up.dirty_hi) == list(down.dirty_hi)
    assert up.esdf_voxels_lowered == down.esdf_voxels_raised
    _same(_products(pkg, eng, host_table=True), want)                                          # the counts included
    everything = np.concatenate([old, a, b])
    two = _engine(pkg, everything, host_table=True)
    i1, i2 = two.clear_pointcloud(b, **INCR), two.clear_pointcloud(a, **INCR)
    one = _engine(pkg, everything, host_table=True)
    i3 = one.clear_pointcloud(np.concatenate([a, b]), **INCR)
    assert i1.path == i2.path == i3.path == 1 and i1.n_cleared_voxels + i2.n_cleared_voxels == i3.n_cleared_voxels > 0
    _same(_products(pkg, two, host_table=True), want)
    _same(_products(pkg, one, host_table=True), want)


# ---- 5. the voxel form --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("forced", ["incremental", "full"])
def test_voxel_form(pkg, product_lib, forced):
    capi = pkg.capi
    occ = (_counts(mu._clouds()[0]) >= THR).astype(np.uint8)
    occ[0, 0, 69] = occ[23, 19, 0] = 1                              # the last byte of a row that is no multiple of 4, a far corner
    rng = np.random.default_rng(11)
    empty, taken = np.argwhere(occ == 0), np.argwhere(occ == 1)
    go = np.concatenate([taken[rng.choice(len(taken), 30, replace=False)], [[0, 0, 69], [23, 19, 0]]])
    go = np.unique(go, axis=0)
    ijk = np.concatenate([go, go[:7], empty[:5], go[3:4]]).astype(np.int32)                     # duplicates and free voxels
    rng.shuffle(ijk)
    edited = occ.copy()
    edited[tuple(ijk.T)] = 0
    incr = forced == "incremental"
    eng = _grid_engine(pkg, occ, host_table=incr)
    info = eng.clear_voxels(ijk, **(INCR if incr else {"max_cleared_voxels": 3}))
    assert info.host_table_patched == int(incr) and info.n_points_ignored == 0
    assert info.path == (1 if incr else 2) and info.n_points == len(ijk) and info.n_cleared_voxels == len(go)
    assert list(info.dirty_lo) == go.min(axis=0).tolist() and list(info.dirty_hi) == go.max(axis=0).tolist()
    want = _products(pkg, _grid_engine(pkg, edited, host_table=incr), counts=False, host_table=incr)
    _same(_products(pkg, eng, counts=False, host_table=incr), want)
    assert np.array_equal(want["occ"], edited)
    # an index outside the grid: refused, nothing changed
    for bad in ([[1, 1, 70]], [[24, 0, 0]], [[3, 3, 3], [0, -1, 0]]):
        with pytest.raises(pkg.IsdfError) as err:
            eng.clear_voxels(bad)
        assert err.value.code == capi.ISDF_ERR_INVALID_ARG
    assert np.array_equal(eng.get_grid(capi.GRID_OCCUPANCY)[0], edited)
    # no counts on a map from isdf_set_grid
    with pytest.raises(pkg.IsdfError) as err:
        eng.clear_pointcloud(mu._clouds()[1])
    assert err.value.code == capi.ISDF_ERR_STATE


def test_voxel_form_drops_the_counts_only_when_a_voxel_was_freed(pkg, product_lib):
    capi = pkg.capi
    old = mu._clouds()[0]
    c = _counts(old)
    eng = _engine(pkg, old, esdf=False, frontend=False)
    info = eng.clear_voxels(np.argwhere(c < THR)[:6])
    assert info.n_cleared_voxels == 0 and info.path == 0
    assert np.array_equal(eng.map_counts(), c)                      # (a clear_voxels that freed nothing leaves the counts in place)
    assert eng.clear_pointcloud(old[:1]).n_points == 1
    assert eng.clear_voxels(np.argwhere(c >= THR)[:1]).n_cleared_voxels == 1
    for call in (eng.map_counts, lambda: eng.clear_pointcloud(old[:1])):
        with pytest.raises(pkg.IsdfError) as err:
            call()
        assert err.value.code == capi.ISDF_ERR_STATE


# ---- 6. / 7. the cost-to-go field and the clearance watch ---------------------------------------------------------------------------
T = np.array([1.5, 1.2, 1.8, 1.5])
N = len(T)
P0, P1 = (np.array([4, 4, 9]) + 0.5) * RES + BMIN, (np.array([19, 15, 60]) + 0.5) * RES + BMIN
MARGIN = 1.0
TIMES = ("select_ms", "field_ms", "reduce_ms")


def _traj():
    v = (P1 - P0) / T.sum()
    c = np.zeros((3, N, 6))
    t0 = np.concatenate([[0.0], np.cumsum(T)[:-1]])
    for i in range(N):
        c[:, i, 0] = P0 + v * t0[i]
        c[:, i, 1] = v
    return c.reshape(-1)


CM = _traj()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_report(got, want, what):
    assert got.keys() == want.keys()
    for k, v in want.items():
        if k not in TIMES:
            assert np.array_equal(_bits(got[k]), _bits(v)), (what, k, got[k], v)


@functools.lru_cache(maxsize=None)
def _watch_occ():
    """the seeded map plus voxels beside the straight trajectory: some of them lie below the margin"""
    occ = (_counts(mu._clouds()[0]) >= THR).astype(np.uint8)
    for f in (0.2, 0.4, 0.6, 0.8):
        cell = np.floor((P0 + (P1 - P0) * f - BMIN) / RES).astype(int)
        occ[tuple(cell + [2, 0, 0])] = occ[tuple(cell + [0, -2, 1])] = 1
    return occ


def _watched(pkg, occ, repair=0):
    eng = _grid_engine(pkg, occ)
    eng.frontend_field_set_repair(repair)
    eng.traj_check_set_watch(1)
    rep = eng.traj_check(T, CM, margin=MARGIN)
    free = eng.frontend_cspace_table().any(axis=3)
    goal = np.argwhere(free)[len(np.argwhere(free)) // 2]
    assert eng.frontend_field_build((goal + 0.5) * RES + BMIN).reachable == 1
    return eng, rep, (goal + 0.5) * RES + BMIN


def test_nothing_cleared_keeps_the_field_and_the_watch(pkg, product_lib):
    capi = pkg.capi
    occ = _watch_occ()
    eng, rep0, _ = _watched(pkg, occ)
    assert rep0["n_below_margin"] > 0
    before = _products(pkg, eng, counts=False)
    field, rows = eng.frontend_field(), eng.traj_check_points()
    rep_a, last_a = eng.traj_check_watch_info(N)
    quiet = np.concatenate([np.argwhere(occ == 0)[5:9], np.argwhere(occ == 0)[5:6]])
    info = eng.clear_voxels(quiet)
    assert info.path == capi.MAP_CLEAR_NONE and info.n_cleared_voxels == 0 and info.n_points == len(quiet)
    assert list(info.dirty_lo) > list(info.dirty_hi) and list(info.touched_lo) > list(info.touched_hi)
    assert (info.field_dropped, info.watch_rechecked, info.esdf_refreshed, info.frontend_refreshed) == (0, 0, 0, 0)
    assert np.array_equal(eng.frontend_field().view(np.uint8), field.view(np.uint8))
    rep_b, last_b = eng.traj_check_watch_info(N)
    _same_report(rep_b, rep_a, "nothing cleared")
    assert last_b == last_a and last_b["updates_folded"] == 0 and eng.traj_check_points().tobytes() == rows.tobytes()
    _same(_products(pkg, eng, counts=False), before)
    # the point form: points that take no count below the threshold
    old = mu._clouds()[0]
    cloud = _engine(pkg, old)
    three = np.argwhere(_counts(old) == 3)[:4]
    pts = _in_cells(three, 1, np.random.default_rng(1))
    kept = _products(pkg, cloud, counts=False)
    info = cloud.clear_pointcloud(pts)
    assert info.path == 0 and info.n_cleared_voxels == 0 and info.n_points_ignored == 0
    assert np.array_equal(cloud.map_counts()[tuple(three.T)], [2, 2, 2, 2])
    _same(_products(pkg, cloud, counts=False), kept)


@pytest.mark.parametrize("repair", [0, 1])
def test_a_cleared_voxel_drops_the_field_and_rechecks_the_watch(pkg, product_lib, repair):
    capi = pkg.capi
    occ = _watch_occ()
    eng, rep0, goal = _watched(pkg, occ, repair=repair)
    rows0 = eng.traj_check_points()
    gone = np.floor((rows0[[0, len(rows0) // 2], :3] - BMIN) / RES).astype(np.int32)       # two voxels of the kept rows
    assert occ[tuple(gone.T)].all() and len(np.unique(gone, axis=0)) == 2
    info = eng.clear_voxels(gone, **INCR)
    assert info.n_cleared_voxels == 2 and info.path == 1 and (info.field_dropped, info.watch_rechecked) == (1, 1)
    with pytest.raises(pkg.IsdfError) as err:
        eng.frontend_field()
    assert err.value.code == capi.ISDF_ERR_STATE
    edited = occ.copy()
    edited[tuple(gone.T)] = 0
    fresh = _grid_engine(pkg, edited)
    want = fresh.traj_check(T, CM, margin=MARGIN)
    want_rows = fresh.traj_check_points()
    rep, last = eng.traj_check_watch_info(N)
    _same_report(rep, want, f"re-checked watch (repair mode {repair})")
    rows = eng.traj_check_points()
    assert rows.shape == want_rows.shape == (len(rows0) - 2, 5) and rows.tobytes() == want_rows.tobytes()
    assert rep["n_below_margin"] == rep0["n_below_margin"] - 2 and last["path"] == 2 and last["updates_folded"] == 1
    _same(_products(pkg, eng, counts=False), _products(pkg, fresh, counts=False))
    assert eng.frontend_field_build(goal).status in (0, 1)            # and the field can be built again


# ---- 8. the last occupied voxel ---------------------------------------------------------------------------------------------------
def test_clearing_the_last_occupied_voxel_takes_the_full_path(pkg, product_lib):
    capi = pkg.capi
    rng = np.random.default_rng(1)
    c = _counts(mu._clouds()[0])
    lone = _in_cells(np.argwhere(c == 0)[:20], 1, rng)              # no voxel of these reaches the threshold
    last = _in_cells([(12, 9, 40)], 2, rng)
    eng = _engine(pkg, np.concatenate([lone, last]))
    assert eng.get_grid(capi.GRID_OCCUPANCY)[0].sum() == 1 and np.isfinite(eng.get_grid(capi.GRID_ESDF)[0]).all()
    info = eng.clear_pointcloud(last[:1], **INCR)
    assert info.path == 2 and info.n_cleared_voxels == 1 and info.esdf_refreshed == 1 and info.esdf_voxels_recomputed == N_VOX
    got = eng.get_grid(capi.GRID_ESDF)[0]
    with np.errstate(over="ignore"):
        assert (got == np.float32(np.float64(RES) * np.sqrt(np.float64(1.7976931348623157e308)))).all() and np.isinf(got).all()
    assert not eng.get_grid(capi.GRID_OCCUPANCY)[0].any()
    _same(_products(pkg, eng), _products(pkg, _engine(pkg, np.concatenate([lone, last[1:]]))))


# ---- 9. status codes ----------------------------------------------------------------------------------------------------------------
def test_status_codes(pkg, product_lib):
    capi = pkg.capi
    old, a, _ = mu._clouds()
    eng = _engine(pkg, old, esdf=False, frontend=False)
    for bad in ({"max_cleared_voxels": -1}, {"full_fraction": -0.5}, {"full_fraction": float("nan")}):
        for call in (lambda: eng.clear_pointcloud(old[:2], **bad), lambda: eng.clear_voxels([[1, 1, 1]], **bad)):
            with pytest.raises(pkg.IsdfError) as err:
                call()
            assert err.value.code == capi.ISDF_ERR_INVALID_ARG
    assert np.array_equal(eng.map_counts(), _counts(old))           # a refused call changed nothing
    assert eng.clear_pointcloud(np.zeros((0, 3), dtype=np.float32)).path == 0 and eng.clear_voxels(np.zeros((0, 3), dtype=np.int32)).path == 0
    assert product_lib.isdf_clear_pointcloud(eng.h, None, 3, None, None) == capi.ISDF_ERR_INVALID_ARG
    assert product_lib.isdf_clear_voxels(eng.h, None, -1, None, None) == capi.ISDF_ERR_INVALID_ARG
    assert product_lib.isdf_clear_pointcloud(eng.h, old[:1].ctypes.data_as(product_lib.isdf_clear_pointcloud.argtypes[1]), 1, None, None) == capi.ISDF_OK     # params and info_out may be NULL
    bare = pkg.Engine(pkg.synth.default_config(capi.V1_SWEPT))      # no grid at all
    for call in (lambda: bare.clear_pointcloud(a), lambda: bare.clear_voxels([[1, 1, 1]])):
        with pytest.raises(pkg.IsdfError) as err:
            call()
        assert err.value.code == capi.ISDF_ERR_STATE
    multi = pkg.Engine(pkg.synth.default_config(capi.V3_ESDF_TILE), devices=[0, 0])
    multi.set_pointcloud(old, RES, THR, BMIN, BMAX)
    for call in (lambda: multi.clear_pointcloud(a), lambda: multi.clear_voxels([[1, 1, 1]])):
        with pytest.raises(pkg.IsdfError) as err:
            call()
        assert err.value.code == capi.ISDF_ERR_UNSUPPORTED


# ---- nothing is allocated after the first call of a size --------------------------------------------------------------------------
def test_a_second_clear_of_the_same_size_allocates_nothing(pkg, product_lib):
    old, removed, _, _, _ = _scene()
    eng = _engine(pkg, old, host_table=True)
    assert eng.clear_pointcloud(removed, **INCR).path == 1
    first = _products(pkg, eng, host_table=True)
    # the same map again in the same ctx, whose clear scratch stays; then the same clear
    assert eng.set_pointcloud(old, RES, THR, BMIN, BMAX) == DIMS
    mu._derive(pkg, eng, host_table=True)
    before = _live(product_lib)
    info = eng.clear_pointcloud(removed, **INCR)
    assert _live(product_lib) == before
    assert info.path == 1 and info.n_cleared_voxels > 0 and info.host_table_patched == 1
    _same(_products(pkg, eng, host_table=True), first)
