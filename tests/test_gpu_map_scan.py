"""A range scan integrated into the map (csrc/map_scan.hip: isdf_integrate_scan) against the sequence it is defined as, run on a second
ctx - isdf_clear_pointcloud of miss_weight centres of every voxel of F, then isdf_update_pointcloud of the hit end points - and against a
fresh build on the new counts; F and H come from the plain host form (isdf_scan_sets_host), which tests/test_map_scan_host.py holds to the
definition.  Every comparison is == on bytes.  Geometry, robot and helpers of tests/test_gpu_map_update.py: 24 x 20 x 70 voxels at 0.5 m,
sta_threshold 2, a box robot with kernel_size 5 and 3 x 3 attitudes."""
import ctypes as C
import functools

import numpy as np
import pytest

import test_gpu_map_update as mu
from test_gpu_map_clear import CM, MARGIN, N, T, _same_report
from test_gpu_map_update import BMAX, BMIN, DIMS, RES, THR, _counts, _engine, _in_cells, _products, _same

pytestmark = pytest.mark.gpu

N_VOX = int(np.prod(DIMS))
ORIGIN_CELL = np.array([12, 10, 35])
ORIGIN = (ORIGIN_CELL + 0.5) * RES + BMIN + np.array([0.11, -0.07, 0.13])
MISS = 2


def _centres(cells):
    """voxel centres: multiples of 0.25 m here, exact in float32"""
    return ((np.asarray(cells, dtype=np.float64).reshape(-1, 3) + 0.5) * RES + BMIN).astype(np.float32)


def _sets(pkg, lib, xyz, hit):
    return pkg.engine.scan_sets_host(BMIN, BMAX, RES, DIMS, ORIGIN, xyz, hit, lib=lib)


def _pocket_base():
    """the seeded map of the update's tests without the points within three voxels of the sensor's"""
    base = mu._clouds()[0]
    cell = np.floor((base.astype(np.float64) - BMIN) / RES)
    return base[np.abs(cell - ORIGIN_CELL).max(axis=1) > 3]


@functools.lru_cache(maxsize=None)
def _scene():
    """old cloud, end points and hit flags of about 400 rays from a free pocket.  The seeded map of the update's tests, cleared around
    the sensor; then rays in random directions, 1.5 to 6.5 m long and stretched along z (some leave the map: skipped), a third of them without a hit; thirty hit
    rays doubled with a little jitter (two hits together in one voxel); and walls of two- and three-point voxels half-way along sixty
    rays, with one-point voxels beside them."""
    rng = np.random.default_rng(77)
    base = _pocket_base()
    d = rng.normal(size=(360, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[:, 2] *= 2.5                                                  # the map is longest in z
    ends = ORIGIN + d * rng.uniform(1.5, 6.5, (360, 1))
    hit = (rng.uniform(size=360) < 0.67).astype(np.uint8)
    twice = np.flatnonzero(hit)[:30]
    ends = np.concatenate([ends, ends[twice] + rng.uniform(-0.02, 0.02, (30, 3)), [[np.nan, 3.0, 3.0], [4.0, 40.0, 5.0]]])
    hit = np.concatenate([hit, np.ones(30, dtype=np.uint8), [1, 0]])
    mid = np.floor((ORIGIN + (ends[:60] - ORIGIN) * 0.5 - BMIN) / RES).astype(int)
    mid = mid[((mid >= 0) & (mid < np.array(DIMS))).all(axis=1)]
    mid = np.unique(mid, axis=0)
    per = rng.integers(1, 4, len(mid))
    walls = _in_cells(mid, per, rng)
    order = rng.permutation(len(ends))
    return np.concatenate([base, walls]), ends[order].astype(np.float32), hit[order]


@functools.lru_cache(maxsize=None)
def _expected(pkg, lib, miss=MISS):
    """(F, H multiplicities, counts', rays skipped) of the scene from the host form"""
    old, ends, hit = _scene()
    free, hits, skipped = _sets(pkg, lib, ends, hit)
    c = _counts(old).astype(np.int64)
    new = np.where(free == 1, np.maximum(c - miss, 0), c + hits)
    return free, hits, new.astype(np.uint32), skipped


def test_the_scene_shows_what_it_is_for(pkg, product_lib):
    old, ends, hit = _scene()
    assert 380 <= len(ends) <= 420
    free, hits, new, skipped = _expected(pkg, product_lib)
    c = _counts(old).astype(np.int64)
    assert c[tuple(ORIGIN_CELL)] == 0 and free[tuple(ORIGIN_CELL)] == 1
    freed = (c >= THR) & (new < THR)
    assert freed.sum() >= 5 and (freed & (c - 1 >= THR)).sum() >= 2                    # some only because miss_weight is 2
    born = (c < THR) & (new >= THR)
    assert born.sum() >= 5 and (born & (c == 0) & (hits >= 2)).sum() >= 2              # some through two hits together
    visited = np.zeros(DIMS, dtype=np.uint8)                                            # passed AND hit: in H, so not in F
    for e in ends[hit == 0][:40]:
        r = pkg.engine.scan_ray_host(BMIN, BMAX, RES, DIMS, ORIGIN, e, lib=product_lib)
        if len(r):
            visited[tuple(r.T)] = 1
    assert ((visited == 1) & (hits > 0)).any() and not ((free == 1) & (hits > 0)).any()
    assert ((free == 1) & (c > 0) & (c < MISS)).sum() >= 2                               # counted down to 0 from below miss_weight
    assert skipped >= 2 and (hit == 0).sum() >= 50


def _cloud_of(counts, seed=5):
    cells = np.argwhere(counts > 0)
    return _in_cells(cells, counts[tuple(cells.T)].astype(int), np.random.default_rng(seed))


def _fields(info):
    """every field outside the *_ms times, nested structs included"""
    out = {}
    for name, _ in info._fields_:
        v = getattr(info, name)
        if name.endswith("_ms"):
            continue
        out[name] = _fields(v) if isinstance(v, C.Structure) else (list(v) if hasattr(v, "__len__") else v)
    return out


def _two_calls(eng, free, ends, hit, inside, miss, clear_params, update_params):
    f = np.repeat(_centres(np.argwhere(free == 1)), miss, axis=0)
    ci = eng.clear_pointcloud(f, **clear_params)
    ui = eng.update_pointcloud(ends[(hit != 0) & inside], **update_params)
    return ci, ui


def _inside(ends):
    p = ends.astype(np.float64)
    return np.isfinite(p).all(axis=1) & ~((p < BMIN).any(axis=1) | (p > BMAX).any(axis=1))


PATHS = {"incremental": ({"full_fraction": 1.0}, {"full_fraction": 1.0}, {"full_fraction": 1.0}, 1),
         "full": ({"max_cleared_voxels": 0, "max_new_voxels": 0}, {"max_cleared_voxels": 0}, {"max_new_voxels": 0}, 2)}


# ---- 1. the device's sets are the host form's
def test_counts_equal_the_host_sets(pkg, product_lib):
    old, ends, hit = _scene()
    free, hits, new, skipped = _expected(pkg, product_lib)
    eng = _engine(pkg, old, esdf=False, frontend=False)
    info = eng.integrate_scan(ORIGIN, ends, hit, miss_weight=MISS)
    print(f"\n{info.n_rays} rays, {info.n_rays_skipped} skipped, {info.n_hits} hits in {info.n_hit_voxels} voxels, |F| {info.n_free_voxels}, "
          f"cleared {info.clear.n_cleared_voxels}, new {info.update.n_new_voxels}, trace {info.trace_ms:.3f} ms")
    assert np.array_equal(eng.map_counts(), new)
    assert np.array_equal(eng.get_grid(pkg.capi.GRID_OCCUPANCY)[0], (new >= THR).astype(np.uint8))
    assert (info.n_rays, info.n_rays_skipped, info.n_hits) == (len(ends), skipped, hits.sum())
    assert (info.n_free_voxels, info.n_hit_voxels) == (free.sum(), (hits > 0).sum())
    seen = np.argwhere((free == 1) | (hits > 0))
    assert list(info.ray_lo) == seen.min(axis=0).tolist() and list(info.ray_hi) == seen.max(axis=0).tolist()
    c = _counts(old).astype(np.int64)
    assert info.clear.n_points == MISS * free.sum() and info.clear.n_points_ignored == np.maximum(MISS - c, 0)[free == 1].sum() > 0
    # hit = None: every ray is a hit
    free_a, hits_a, _ = _sets(pkg, product_lib, ends, None)
    eng = _engine(pkg, old, esdf=False, frontend=False)
    info = eng.integrate_scan(ORIGIN, ends, None)
    assert np.array_equal(eng.map_counts(), np.where(free_a == 1, np.maximum(c - 1, 0), c + hits_a))
    assert info.n_hits == len(ends) - skipped == hits_a.sum()


# ---- 2. products equal the two-call sequence and a fresh build
@pytest.mark.parametrize("host_table", [False, True])
@pytest.mark.parametrize("forced", list(PATHS))
def test_products_equal_the_two_calls_and_a_fresh_build(pkg, product_lib, forced, host_table):
    old, ends, hit = _scene()
    free, hits, new, skipped = _expected(pkg, product_lib)
    scan_p, clear_p, update_p, path = PATHS[forced]
    eng = _engine(pkg, old, host_table=host_table)
    info = eng.integrate_scan(ORIGIN, ends, hit, miss_weight=MISS, **scan_p)
    two = _engine(pkg, old, host_table=host_table)
    ci, ui = _two_calls(two, free, ends, hit, _inside(ends), MISS, clear_p, update_p)
    assert info.clear.path == info.update.path == path
    assert _fields(info.clear) == _fields(ci) and _fields(info.update) == _fields(ui)
    assert info.clear.n_cleared_voxels >= 5 and info.update.n_new_voxels >= 5
    incr = forced == "incremental"
    keep_host = host_table and incr                                 # the full path marks the host copy stale
    assert info.clear.host_table_patched == info.update.host_table_patched == int(keep_host)
    got = _products(pkg, eng, host_table=keep_host)
    _same(got, _products(pkg, two, host_table=keep_host))
    fresh = _engine(pkg, _cloud_of(new), host_table=keep_host)
    _same(got, _products(pkg, fresh, host_table=keep_host))
    assert np.array_equal(got["counts"], new) and got["cspace"].any()


# ---- 3. the cost-to-go field and the clearance watch
def _watched(pkg, cloud, mode):
    eng = _engine(pkg, cloud)
    eng.frontend_field_set_repair(mode)
    eng.frontend_field_set_reopen(mode)
    eng.traj_check_set_watch(1)
    rep = eng.traj_check(T, CM, margin=MARGIN)
    free = eng.frontend_cspace_table().any(axis=3)
    goal = (np.argwhere(free)[len(np.argwhere(free)) // 2] + 0.5) * RES + BMIN
    assert eng.frontend_field_build(goal).reachable == 1
    return eng, rep


def _field_or_none(pkg, eng):
    try:
        return eng.frontend_field()
    except pkg.IsdfError as e:
        assert e.code == pkg.capi.ISDF_ERR_STATE
        return None


@pytest.mark.parametrize("mode", [0, 1])
def test_field_and_watch_equal_the_two_calls(pkg, product_lib, mode):
    old, ends, hit = _scene()
    free, hits, new, _ = _expected(pkg, product_lib)
    incr = {"full_fraction": 1.0}
    eng, rep0 = _watched(pkg, old, mode)
    two, _ = _watched(pkg, old, mode)
    info = eng.integrate_scan(ORIGIN, ends, hit, miss_weight=MISS, **incr)
    ci, ui = _two_calls(two, free, ends, hit, _inside(ends), MISS, incr, incr)
    assert _fields(info.clear) == _fields(ci) and _fields(info.update) == _fields(ui)
    assert info.clear.watch_rechecked == 1 and info.clear.field_dropped == 1 - mode
    a, b = _field_or_none(pkg, eng), _field_or_none(pkg, two)
    assert (a is None) == (b is None)
    if mode == 0:
        assert a is None
    elif a is not None:
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    rep_a, last_a = eng.traj_check_watch_info(N)
    rep_b, last_b = two.traj_check_watch_info(N)
    _same_report(rep_a, rep_b, f"watch after the scan (mode {mode})")
    assert {k: v for k, v in last_a.items() if not k.endswith("_ms")} == {k: v for k, v in last_b.items() if not k.endswith("_ms")}
    assert last_a["updates_folded"] == 2 and eng.traj_check_points().tobytes() == two.traj_check_points().tobytes()
    fresh = _engine(pkg, _cloud_of(new))
    _same_report(rep_a, fresh.traj_check(T, CM, margin=MARGIN), "watch against a fresh check")
    _same(_products(pkg, eng), _products(pkg, two))


# ---- 4. a scan that changes only counts
def test_a_scan_that_changes_only_counts_keeps_the_field_and_the_watch(pkg, product_lib):
    old = _pocket_base()
    pocket = _counts(old)[tuple(slice(v - 3, v + 4) for v in ORIGIN_CELL)]
    assert pocket.shape == (7, 7, 7) and not pocket.any()
    rng = np.random.default_rng(8)
    lone = _in_cells([ORIGIN_CELL + [2, 0, 0], ORIGIN_CELL + [0, -2, 1]], 1, rng)       # one point each: below the threshold
    cloud = np.concatenate([old, lone])
    ends = np.concatenate([_centres([ORIGIN_CELL + [3, 0, 0], ORIGIN_CELL + [0, -3, 1], ORIGIN_CELL + [0, 2, -2]]),        # through the lone voxels
                           _centres([ORIGIN_CELL + [-2, 1, 0]])])                                                           # one hit into an empty voxel
    hit = np.array([0, 0, 0, 1], dtype=np.uint8)
    eng, _ = _watched(pkg, cloud, 1)
    before = _products(pkg, eng, counts=False)
    field, rows = eng.frontend_field(), eng.traj_check_points()
    rep_a, last_a = eng.traj_check_watch_info(N)
    info = eng.integrate_scan(ORIGIN, ends, hit, miss_weight=MISS)
    assert (info.clear.path, info.update.path) == (0, 0) and info.n_free_voxels >= 9 and info.n_hits == 1
    assert (info.clear.n_cleared_voxels, info.update.n_new_voxels, info.clear.field_dropped, info.update.field_dropped, info.clear.watch_rechecked) == (0, 0, 0, 0, 0)
    assert info.clear.n_points_ignored == MISS * info.n_free_voxels - 2 and list(info.clear.dirty_lo) > list(info.clear.dirty_hi)
    c = _counts(cloud)
    want = c.copy()
    want[tuple((ORIGIN_CELL + [2, 0, 0]))] = want[tuple((ORIGIN_CELL + [0, -2, 1]))] = 0
    want[tuple((ORIGIN_CELL + [-2, 1, 0]))] = 1
    assert np.array_equal(eng.map_counts(), want) and not np.array_equal(want, c)
    assert np.array_equal(eng.frontend_field().view(np.uint8), field.view(np.uint8))
    rep_b, last_b = eng.traj_check_watch_info(N)
    _same_report(rep_b, rep_a, "only counts changed")
    assert last_b == last_a and eng.traj_check_points().tobytes() == rows.tobytes()
    _same(_products(pkg, eng, counts=False), before)


# ---- 5. no rays, no miss weight, every ray skipped
def test_empty_scans(pkg, product_lib):
    old, ends, hit = _scene()
    c = _counts(old)
    eng = _engine(pkg, old)
    before = _products(pkg, eng)
    info = eng.integrate_scan(ORIGIN, np.zeros((0, 3), dtype=np.float32))
    assert (info.n_rays, info.clear.path, info.update.path, info.clear.n_points, info.update.n_points) == (0, 0, 0, 0, 0)
    assert list(info.ray_lo) > list(info.ray_hi) and info.n_free_voxels == 0
    outside = np.array([[-3.0, 5.0, 5.0], [4.0, 40.0, 5.0], [np.nan, 3.0, 3.0], [np.inf, 3.0, 3.0]], dtype=np.float32)
    info = eng.integrate_scan(ORIGIN, outside)
    assert (info.n_rays, info.n_rays_skipped, info.n_hits, info.n_free_voxels, info.clear.path, info.update.path) == (4, 4, 0, 0, 0, 0)
    assert list(info.ray_lo) > list(info.ray_hi)
    _same(_products(pkg, eng), before)                              # voxel (0, 0, 0) included: a ray is no map point
    # miss_weight 0: only the hits count - isdf_update_pointcloud of the hit end points
    free, hits, _ = _sets(pkg, product_lib, ends, hit)
    info = eng.integrate_scan(ORIGIN, ends, hit, miss_weight=0, full_fraction=1.0)
    assert (info.clear.path, info.clear.n_points, info.clear.n_points_ignored, info.n_free_voxels) == (0, 0, 0, free.sum()) and info.update.path == 1
    two = _engine(pkg, old)
    ui = two.update_pointcloud(ends[(hit != 0) & _inside(ends)], full_fraction=1.0)
    assert _fields(info.update) == _fields(ui)
    _same(_products(pkg, eng), _products(pkg, two))
    assert np.array_equal(eng.map_counts(), c + hits)


# ---- 6. status codes
def test_status_codes(pkg, product_lib):
    capi = pkg.capi
    old, ends, hit = _scene()
    eng = _engine(pkg, old, esdf=False, frontend=False)
    for origin in (BMAX + [0.1, 0.0, 0.0], BMIN - [0.0, 1e-6, 0.0], [np.nan, 5.0, 5.0]):
        with pytest.raises(pkg.IsdfError) as err:
            eng.integrate_scan(origin, ends, hit)
        assert err.value.code == capi.ISDF_ERR_INVALID_ARG
    for bad in ({"miss_weight": -1}, {"max_cleared_voxels": -1}, {"max_new_voxels": -1}, {"full_fraction": float("nan")}):
        with pytest.raises(pkg.IsdfError) as err:
            eng.integrate_scan(ORIGIN, ends, hit, **bad)
        assert err.value.code == capi.ISDF_ERR_INVALID_ARG
    o = np.ascontiguousarray(ORIGIN)
    op = o.ctypes.data_as(C.POINTER(C.c_double))
    assert product_lib.isdf_integrate_scan(eng.h, op, None, None, 3, None, None) == capi.ISDF_ERR_INVALID_ARG
    assert product_lib.isdf_integrate_scan(eng.h, op, None, None, -1, None, None) == capi.ISDF_ERR_INVALID_ARG
    assert product_lib.isdf_integrate_scan(eng.h, None, ends.ctypes.data_as(C.POINTER(C.c_float)), None, 3, None, None) == capi.ISDF_ERR_INVALID_ARG
    assert np.array_equal(eng.map_counts(), _counts(old))           # a refused call changed nothing
    assert product_lib.isdf_integrate_scan(eng.h, op, None, None, 0, None, None) == capi.ISDF_OK             # params and info_out may be NULL
    assert eng.update_voxels(np.argwhere(_counts(old) == 0)[:1]).n_new_voxels == 1                            # the counts are gone
    with pytest.raises(pkg.IsdfError) as err:
        eng.integrate_scan(ORIGIN, ends, hit)
    assert err.value.code == capi.ISDF_ERR_STATE
    bare = pkg.Engine(pkg.synth.default_config(capi.V1_SWEPT))      # no grid at all
    with pytest.raises(pkg.IsdfError) as err:
        bare.integrate_scan(ORIGIN, ends, hit)
    assert err.value.code == capi.ISDF_ERR_STATE
    multi = pkg.Engine(pkg.synth.default_config(capi.V3_ESDF_TILE), devices=[0, 0])
    multi.set_pointcloud(old, RES, THR, BMIN, BMAX)
    with pytest.raises(pkg.IsdfError) as err:
        multi.integrate_scan(ORIGIN, ends, hit)
    assert err.value.code == capi.ISDF_ERR_UNSUPPORTED


# ---- 7. nothing is allocated after the first call of a size
def _live(lib):
    out = (C.c_longlong * 2)()
    lib.isdf_debug_live_bytes(out)
    return list(out)


def test_a_second_scan_of_the_same_size_allocates_nothing(pkg, product_lib):
    old, ends, hit = _scene()
    _, _, new, _ = _expected(pkg, product_lib)
    eng = _engine(pkg, old, host_table=True)
    eng.integrate_scan(ORIGIN, ends, hit, miss_weight=MISS, full_fraction=1.0)
    first = _products(pkg, eng, host_table=True)
    # the same map again in the same ctx, whose scan scratch stays; then the same scan
    assert eng.set_pointcloud(old, RES, THR, BMIN, BMAX) == DIMS
    mu._derive(pkg, eng, host_table=True)
    before = _live(product_lib)
    info = eng.integrate_scan(ORIGIN, ends, hit, miss_weight=MISS, full_fraction=1.0)
    assert _live(product_lib) == before
    assert info.clear.path == info.update.path == 1
    _same(_products(pkg, eng, host_table=True), first)
    assert np.array_equal(first["counts"], new)
