"""Candidate views on the device (csrc/view_cand.hip: isdf_view_candidates) against the plain host form, which
tests/test_view_cand_host.py holds to the NumPy restatement.  Every output and every integer word of the info is compared with == on
bytes.  Grids are tests/test_map_known_host.py's, the scenes tests/view_cand_cases.py's, the camera the view gain's."""
import ctypes as C

import numpy as np
import pytest

import known_reference as kr
import view_cand_cases as cs
import view_cand_reference as vc
from test_gpu_map_update import _live
from test_map_known_host import GRIDS, IDS
from test_view_gain_host import RANGES, STRIDES, cam_of

pytestmark = pytest.mark.gpu
RES = cs.RES
FILTER_BLOCK = 128                      # csrc/view_cand.hip's VC_BLOCK


def _scene_engine(pkg, dims, known=True):
    """the scene's map from a cloud (two points in every occupied voxel, sta_threshold 2) and its K from the scene's fills"""
    occ, fills, targets, offsets = cs.scene(dims)
    cells = np.concatenate([np.repeat(np.argwhere(occ), 2, axis=0), [[0, 0, 0]]])
    eng = pkg.Engine(pkg.synth.default_config(pkg.capi.V1_SWEPT))
    assert eng.set_pointcloud(((cells + 0.5) * RES).astype(np.float32), RES, 2, np.zeros(3), np.array(dims) * RES) == tuple(dims)
    assert np.array_equal(eng.get_grid(pkg.capi.GRID_OCCUPANCY)[0] != 0, occ)
    if known:
        eng.map_known_enable(True)
        for box, value in fills:
            eng.map_known_fill(box, value)
    return eng, targets, offsets


def _host(pkg, lib, eng, cam, targets, offsets, **params):
    """the host form on the ctx's own K, occupancy and box"""
    occ, bmin, bmax = eng.get_grid(pkg.capi.GRID_OCCUPANCY)
    params.pop("scratch_bytes", None)
    return pkg.engine.view_candidates_host(eng.map_known()[0], occ, bmin, bmax, RES, cam, targets, offsets, lib=lib, **params)


def _same(pkg, lib, eng, cam, targets, offsets, chunks=None, **params):
    want = _host(pkg, lib, eng, cam, targets, offsets, **params)
    got = eng.view_candidates(cam, targets, offsets, **params)
    for a, b, name in zip(got[:4], want[:4], ("cand", "poses", "target rows", "best")):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (params, name, np.argwhere(a != b)[:8])
    assert [getattr(got[4], w) for w in vc.INFO_WORDS] == [getattr(want[4], w) for w in vc.INFO_WORDS], params
    info = got[4]
    assert info.chunks == ((1 if info.n_kept else 0) if chunks is None else chunks), (info.chunks, info.n_kept)
    assert info.filter_ms >= 0.0 and info.gain_ms >= 0.0 and info.select_ms >= 0.0 and (info.n_kept > 0 or (info.gain_ms, info.select_ms) == (0.0, 0.0))
    return got


def _sweep(pkg, lib, eng, cam, targets, offsets):
    kept = 0
    for stride in STRIDES:
        for rng_m in RANGES:
            kept += int(_same(pkg, lib, eng, cam, targets, offsets, stride=stride, max_range_m=rng_m)[4].n_kept)
    return kept


@pytest.mark.parametrize("dims", GRIDS, ids=IDS)
def test_outputs_equal_the_host_form(pkg, product_lib, dims):
    eng, targets, offsets = _scene_engine(pkg, dims)
    cam = cam_of(pkg)
    cand, _, rows, best, info = _same(pkg, product_lib, eng, cam, targets, offsets, stride=1, max_range_m=2.0)
    cs.conditions(cand, rows, best, len(offsets), 3)            # the scene's conditions, on the device's own rows
    assert _sweep(pkg, product_lib, eng, cam, targets, offsets) > 0
    for r in (0, 2):
        _same(pkg, product_lib, eng, cam, targets, offsets, stride=1, max_range_m=40.0, clearance_voxels=r)
    for k_best, min_gain in ((1, 0), (len(offsets) + 1, 0), (3, 10 ** 9)):
        _same(pkg, product_lib, eng, cam, targets, offsets, stride=1, max_range_m=40.0, k_best=k_best, min_gain=min_gain)
    ext = np.array(dims) * RES                                  # a scan from inside the room: its merge makes more of the space behind the wall known
    ends = (np.random.default_rng(5).uniform(0.05, 0.95, (200, 3)) * ext).astype(np.float32)
    eng.integrate_scan((np.array([1, dims[1] // 2, dims[2] // 2]) + 0.5) * RES, ends, np.zeros(len(ends), dtype=np.uint8), miss_weight=0)
    assert eng.map_known()[1].merges == 1
    assert _sweep(pkg, product_lib, eng, cam, targets, offsets) > 0
    eng.shift_map((2, -3, 5))
    _sweep(pkg, product_lib, eng, cam, targets, offsets)
    got = eng.view_candidates(cam, targets[:0], offsets)        # no targets, no offsets: nothing launched, nothing written
    assert [a.shape for a in got[:4]] == [(0, 8), (0, 12), (0, 8), (0, 3)] and (got[4].n_candidates, got[4].best_candidate, got[4].chunks) == (0, -1, 0)
    got = eng.view_candidates(cam, targets, offsets[:0])
    assert (got[4].n_targets, got[4].n_candidates, got[4].best_target) == (len(targets), 0, -1) and not got[2].any()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_fills_on_the_largest_grid(pkg, product_lib, seed):
    """tests/view_cand_cases.py's random scene: K with structure at every alignment, the cube's columns crossing words"""
    dims = GRIDS[2]
    occ, fills, targets, offsets = cs.random_scene(dims, seed)
    cells = np.concatenate([np.repeat(np.argwhere(occ), 2, axis=0), [[0, 0, 0]]])
    eng = pkg.Engine(pkg.synth.default_config(pkg.capi.V1_SWEPT))
    assert eng.set_pointcloud(((cells + 0.5) * RES).astype(np.float32), RES, 2, np.zeros(3), np.array(dims) * RES) == tuple(dims)
    eng.map_known_enable(True)
    for box, value in fills:
        eng.map_known_fill(box, value)
    assert np.array_equal(kr.unpack(eng.map_known()[0], dims), cs.known_of(dims, fills))
    cam = cam_of(pkg)
    for r, stride, rng_m in ((1, (1, 1), 40.0), (2, (3, 2), 2.0), (8, (3, 2), 40.0)):
        got = _same(pkg, product_lib, eng, cam, targets, offsets, clearance_voxels=r, stride=stride, max_range_m=rng_m, k_best=4, min_gain=0)
        assert cs.cube_columns_crossing_words(got[0], dims, r) > 20 and got[4].n_close > 0 and (r == 8 or got[4].n_kept > 0)


def _room_inputs(dims, n_targets, n_offsets, seed=9):
    """targets in the scene's room and behind its wall, offsets up to 1.5 m: every status but `bad` is likely, none is asserted"""
    rng = np.random.default_rng(seed)
    ext = np.array(dims) * RES
    targets = rng.uniform(0.05, 0.95, (n_targets, 3)) * ext
    targets[0] = (np.array([3, 10, 35]) + 0.5) * RES            # the first stands in the room: a lone target keeps some
    return targets, rng.uniform(-1.5, 1.5, (n_offsets, 3))


@pytest.mark.parametrize("n_offsets", [1, 63, 64, 65, 130])
def test_the_straddles(pkg, product_lib, n_offsets):
    """a lane, a wavefront, the filter's workgroup of 128 and the selection's of 256, with one target and with seventy"""
    dims = GRIDS[2]
    eng, _, _ = _scene_engine(pkg, dims)
    cam = cam_of(pkg)
    for n_targets in (1, 70):
        targets, offsets = _room_inputs(dims, n_targets, n_offsets)
        info = _same(pkg, product_lib, eng, cam, targets, offsets, stride=(3, 2), max_range_m=40.0, k_best=5, min_gain=0)[4]
        assert info.n_kept > 0, (n_targets, n_offsets)
    assert n_offsets == 64 or (70 * n_offsets) % FILTER_BLOCK != 0


def test_zero_kept_and_all_kept(pkg, product_lib):
    dims = GRIDS[2]
    eng, targets, offsets = _scene_engine(pkg, dims)
    cam = cam_of(pkg)
    eng.map_known_fill(None, 0)                                 # nothing is seen: no eye passes test 3
    cand, poses, rows, best, info = _same(pkg, product_lib, eng, cam, targets, offsets, chunks=0, stride=1, max_range_m=40.0)
    assert info.n_kept == 0 and info.n_unknown > 0 and info.chunks == 0 and not cand[:, 3:7].any() and (best == -1).all() and (cand[:, 7] == -1).all()
    assert not poses.any() and (rows[:, 6:] == [-1, 0]).all() and (info.best_target, info.best_candidate, info.best_gain) == (-1, -1, 0)
    eng.map_known_fill(None, 1)                                 # everything is seen, and these eyes stand well inside the room
    room = (np.array([[3, 12, 30], [4, 13, 40], [5, 15, 20]]) + 0.5) * RES
    ring = pkg.engine.view_ring_offsets((0.5, 1.0), 8, (-0.5, 0.0, 0.5))
    cand, poses, rows, best, info = _same(pkg, product_lib, eng, cam, room, ring, stride=1, max_range_m=40.0, min_gain=0)
    assert info.n_kept == info.n_candidates == 3 * 48 and (cand[:, 0] == 0).all() and (rows[:, 0] == 48).all() and not cand[:, 3].any() and best[:, 0].tolist() == [0, 48, 96]


def test_the_chunk_size_does_not_change_a_byte(pkg, product_lib):
    dims = GRIDS[2]
    eng, targets, offsets = _scene_engine(pkg, dims)
    cam = cam_of(pkg)
    n_kept = int(_host(pkg, product_lib, eng, cam, targets, offsets, stride=1, max_range_m=40.0)[4].n_kept)
    assert n_kept > 4
    two_views = 2 * 4 * pkg.engine.known_words(dims)
    a = _same(pkg, product_lib, eng, cam, targets, offsets, chunks=n_kept, stride=1, max_range_m=40.0, scratch_bytes=0)
    b = _same(pkg, product_lib, eng, cam, targets, offsets, chunks=(n_kept + 1) // 2, stride=1, max_range_m=40.0, scratch_bytes=two_views)
    c = _same(pkg, product_lib, eng, cam, targets, offsets, chunks=1, stride=1, max_range_m=40.0)
    for x, y, z in zip(a[:4], b[:4], c[:4]):
        assert x.tobytes() == y.tobytes() == z.tobytes()
    assert a[0][:, 3].sum() > 0


@pytest.mark.parametrize("dims", GRIDS, ids=IDS)
def test_a_kept_candidates_words_are_the_view_gains(pkg, product_lib, dims):
    eng, targets, offsets = _scene_engine(pkg, dims)
    cam = cam_of(pkg)
    for stride, rng_m in (((1, 1), 40.0), ((3, 2), 2.0)):
        cand, poses, _, _, info = eng.view_candidates(cam, targets, offsets, stride=stride, max_range_m=rng_m)
        kept = np.flatnonzero(cand[:, 0] == 0)
        assert len(kept) == info.n_kept == info.n_scored > 0
        rows, _ = eng.view_gain(cam, poses[kept], stride=stride, max_range_m=rng_m)
        assert (rows[:, 0] == 0).all() and np.array_equal(rows[:, [1, 4, 5, 6]], cand[kept, 3:7])


def _raw(pkg, eng, cam, targets, offsets, outs, want_info=True, **kw):
    p = pkg.capi.IsdfViewCandidatesParams()
    eng.lib.isdf_view_candidates_params_default(C.byref(p))
    p.gain.stride_u = p.gain.stride_v = 1
    p.gain.max_range_m = 40.0
    for key, v in kw.items():
        setattr(p, key, v)
    info = pkg.capi.IsdfViewCandidatesInfo()
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)      # noqa: E731
    t, o = np.ascontiguousarray(targets, dtype=np.float64), np.ascontiguousarray(offsets, dtype=np.float64)
    rc = eng.lib.isdf_view_candidates(eng.h, C.byref(cam), ptr(t), len(t), ptr(o), len(o), C.byref(p), *[ptr(a) for a in outs], C.byref(info) if want_info else None)
    return rc, info


def _err(eng):
    return (eng.lib.isdf_last_error(eng.h) or b"").decode()


def test_each_output_is_nullable(pkg, product_lib):
    dims = GRIDS[1]
    eng, targets, offsets = _scene_engine(pkg, dims)
    cam = cam_of(pkg)
    want = _same(pkg, product_lib, eng, cam, targets, offsets, stride=1, max_range_m=40.0)
    for skip in range(5):
        outs = [np.full_like(a, -7) for a in want[:4]]
        rc, info = _raw(pkg, eng, cam, targets, offsets, [None if i == skip else a for i, a in enumerate(outs)], want_info=skip != 4)
        assert rc == 0
        for i, (a, b) in enumerate(zip(outs, want[:4])):
            assert (a == -7).all() if i == skip else a.tobytes() == b.tobytes(), (skip, i)
        if skip != 4:
            assert [getattr(info, w) for w in vc.INFO_WORDS] == [getattr(want[4], w) for w in vc.INFO_WORDS]
    rc, info = _raw(pkg, eng, cam, targets, offsets, [None] * 4)
    assert rc == 0 and info.n_kept == want[4].n_kept and info.best_candidate == want[4].best_candidate


def test_the_call_is_read_only_and_allocates_once(pkg, product_lib):
    """the scan tests' map with every product, a valid cost-to-go field, an armed watch and a kept report; K from one scan's merge"""
    import test_gpu_map_scan as ms
    import test_gpu_map_update as mu
    from test_gpu_map_clear import N, _same_report
    capi = pkg.capi
    old, ends, hit = ms._scene()
    eng, _ = ms._watched(pkg, old, 1)
    eng.map_known_enable(True)
    eng.integrate_scan(ms.ORIGIN, ends, hit, miss_weight=ms.MISS)
    lo, hi = ms.ORIGIN_CELL - 3, ms.ORIGIN_CELL + 3
    eng.map_known_fill(tuple(int(v) for v in np.concatenate([lo, hi])), 1)       # the sensor's pocket is free: eyes in it are kept
    cam = cam_of(pkg)

    def state():
        bits, info = eng.map_known()
        return bits.tobytes(), eng.get_grid(capi.GRID_OCCUPANCY)[0].tobytes(), info.merges, info.newly_known, info.n_known
    before = state()
    products = mu._products(pkg, eng)                           # counts, occupancy, ESDF, configuration space, bit map
    field, kept_report = eng.frontend_field(), eng.traj_check_points().tobytes()
    rep_a, last_a = eng.traj_check_watch_info(N)
    front0 = eng.map_frontier()[1].tobytes()
    targets = np.array([ms.ORIGIN + (1.0, 0.0, 0.0), ms.ORIGIN + (0.0, 2.5, 1.0)])
    ring = pkg.engine.view_ring_offsets((0.5,), 8, (0.0, 0.5))
    first = _same(pkg, product_lib, eng, cam, targets, ring, stride=1, max_range_m=40.0, min_gain=0)
    assert first[4].n_kept > 0
    views = eng.next_views(cam, ring, stride=1, max_range_m=40.0, clearance_voxels=0, min_gain=0)
    live = _live(product_lib)
    second = eng.view_candidates(cam, targets, ring, stride=1, max_range_m=40.0, min_gain=0)
    again = eng.next_views(cam, ring, stride=1, max_range_m=40.0, clearance_voxels=0, min_gain=0)
    assert _live(product_lib) == live
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first[:4], second[:4])) and all(a.tobytes() == b.tobytes() for a, b in zip(views[:5], again[:5]))
    assert state() == before and before[2] == 1
    mu._same(mu._products(pkg, eng), products)
    assert np.array_equal(eng.frontend_field().view(np.uint8), field.view(np.uint8))        # the kept field
    rep_b, last_b = eng.traj_check_watch_info(N)                # the armed watch: its report and the last index it folded
    _same_report(rep_b, rep_a, "after the candidate views")
    assert last_b == last_a
    assert eng.traj_check_points().tobytes() == kept_report and eng.map_frontier()[1].tobytes() == front0
    assert eng.points_merge_check()["n_added"] >= 0             # the kept report is not stale: the grid epoch did not move


def test_status_codes_and_their_order(pkg, product_lib):
    capi = pkg.capi
    dims = GRIDS[0]
    cam = cam_of(pkg)
    _, _, targets, offsets = cs.scene(dims)
    outs = [None] * 4
    eng, _, _ = _scene_engine(pkg, dims, known=False)           # an occupancy grid, the known mode off
    assert _raw(pkg, eng, cam, targets, offsets, outs)[0] == capi.ISDF_ERR_STATE and "known grid" in _err(eng)
    # every argument error comes before the state's
    assert _raw(pkg, eng, pkg.engine.depth_camera(0, 6, 6, 6, 3, 3), targets, offsets, outs, k_best=0)[0] == capi.ISDF_ERR_INVALID_ARG and "camera" in _err(eng)
    for kw in ({"clearance_voxels": 9}, {"clearance_voxels": -1}, {"k_best": 0}, {"k_best": 65}, {"min_gain": -1}):
        assert _raw(pkg, eng, cam, targets, offsets, outs, **kw)[0] == capi.ISDF_ERR_INVALID_ARG, kw
    p = pkg.capi.IsdfViewCandidatesParams()
    eng.lib.isdf_view_candidates_params_default(C.byref(p))
    t = np.ascontiguousarray(targets)
    o = np.ascontiguousarray(offsets)
    call = lambda tp, nt, op, no: eng.lib.isdf_view_candidates(eng.h, C.byref(cam), tp, nt, op, no, C.byref(p), None, None, None, None, None)      # noqa: E731
    tp, op = t.ctypes.data_as(C.c_void_p), o.ctypes.data_as(C.c_void_p)
    E = capi.ISDF_ERR_INVALID_ARG
    assert call(tp, -1, op, len(o)) == E and call(tp, len(t), op, -1) == E and call(tp, 1, op, (1 << 20) + 1) == E and call(tp, 1 << 11, op, 1 << 20) == E
    assert call(None, len(t), op, len(o)) == E and call(tp, len(t), None, len(o)) == E
    assert eng.lib.isdf_view_candidates(None, C.byref(cam), tp, len(t), op, len(o), C.byref(p), None, None, None, None, None) == E
    bare = pkg.Engine(pkg.synth.default_config(capi.V1_SWEPT))  # no map at all: the occupancy's sentence comes first
    assert _raw(pkg, bare, cam, targets, offsets, outs)[0] == capi.ISDF_ERR_STATE and "occupancy" in _err(bare)
    bare.map_known_enable(True)
    bare.set_grid(np.ones(dims, dtype=np.float32), (0, 0, 0), RES, capi.GRID_ESDF)      # a map with a known grid and no occupancy grid
    assert _raw(pkg, bare, cam, targets, offsets, outs)[0] == capi.ISDF_ERR_STATE and "occupancy" in _err(bare)
    eng.map_known_enable(True)
    assert _raw(pkg, eng, cam, targets, offsets, outs)[0] == 0
    with pytest.raises(pkg.engine.IsdfError) as e:
        eng.view_candidates(cam, targets, offsets, k_best=0)
    assert e.value.code == E


def test_next_views_closes_the_loop(pkg, product_lib):
    """K as one integrate_depth leaves it; the best eye is a seen, free place, and integrating an empty image from the best pose leaves
    that pose nothing to gain: its rays' voxels are all known then"""
    dims = GRIDS[2]
    capi = pkg.capi
    rng = np.random.default_rng(3)
    occ = np.zeros(dims, dtype=bool)
    occ[:4] = rng.uniform(size=(4,) + dims[1:]) < 0.2
    cloud = ((np.repeat(np.argwhere(occ), 2, axis=0) + 0.5) * RES).astype(np.float32)
    eng = pkg.Engine(pkg.synth.default_config(capi.V1_SWEPT))
    assert eng.set_pointcloud(cloud, RES, 2, np.zeros(3), np.array(dims) * RES) == tuple(dims)
    eng.map_known_enable(True)
    cam = cam_of(pkg, 32, 24, 20.0)
    eye = (np.array([6, 10, 35]) + 0.5) * RES
    empty = np.zeros((cam.height, cam.width), dtype=np.uint16)
    eng.integrate_depth(cam, pkg.engine.look_at(eye, eye + (1.0, 0.1, -0.2)), empty, stride=1, max_range_m=6.0, no_return_is_free=True)
    ring = pkg.engine.view_ring_offsets((1.0, 1.5, 2.0), 8, (-0.5, 0.0, 0.5))
    params = {"stride": 1, "max_range_m": 4.0, "min_gain": 5, "k_best": 2}
    clusters, cand, poses, rows, best, info = eng.next_views(cam, ring, **params)
    assert len(clusters) == len(rows) == info.n_targets > 0 and info.n_offsets == len(ring) and info.n_kept > 0 and info.best_candidate >= 0
    want = _host(pkg, product_lib, eng, cam, pkg.engine.cluster_points(clusters, np.zeros(3), RES, dims)[1], ring, **params)
    assert all(a.tobytes() == b.tobytes() for a, b in zip((cand, poses, rows, best), want[:4]))
    k = kr.unpack(eng.map_known()[0], dims).reshape(-1)
    o8 = eng.get_grid(capi.GRID_OCCUPANCY)[0].reshape(-1)
    ranked = best[best >= 0]
    assert len(ranked) > 0 and k[cand[ranked, 1]].all() and not o8[cand[ranked, 1]].any() and (cand[ranked, 3] >= 5).all() and (cand[ranked, 0] == 0).all()
    assert cand[info.best_candidate, 3] == info.best_gain == cand[:, 3].max() and rows[info.best_target, 6] == info.best_candidate
    pose = poses[info.best_candidate]
    eng.integrate_depth(cam, pose, empty, stride=1, max_range_m=4.0, no_return_is_free=True)
    assert eng.map_known()[1].newly_known >= info.best_gain
    after, _ = eng.view_gain(cam, pose, stride=1, max_range_m=4.0)
    assert after[0, 0] == 0 and after[0, 1] == 0
