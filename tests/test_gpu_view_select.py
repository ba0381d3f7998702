"""The view selection on the device (csrc/view_select.hip: isdf_view_select) against the plain host form, which
tests/test_view_select_host.py holds to the NumPy restatement.  Every output and every integer word of the info is compared with == on
bytes.  Grids are tests/test_map_known_host.py's, the scenes tests/view_select_cases.py's, the camera the view gain's; the closed loop
holds the marginals to what isdf_integrate_depth then reports as newly known, view by view."""
import ctypes as C

import numpy as np
import pytest

import known_reference as kr
import view_select_cases as cs
import view_select_reference as sr
from test_gpu_map_update import _live
from test_map_known_host import GRIDS, IDS
from test_view_gain_host import STRIDES, cam_of

pytestmark = pytest.mark.gpu
RES = cs.RES
PICK_BLOCK = 256                        # csrc/view_select.hip's VS_BLOCK


def _case_engine(pkg, dims, known=True):
    """the case's map from a cloud (two points in every occupied voxel, sta_threshold 2) and its K from the case's fills"""
    if tuple(dims) == cs.BASE_DIMS:
        occ, fills, poses = cs.base_case()
        rng_m = cs.BASE_RANGE
    else:
        occ, fills, poses = cs.generic_case(dims, pkg.engine.look_at)
        rng_m = 40.0
    cells = np.concatenate([np.repeat(np.argwhere(occ), 2, axis=0), [[0, 0, 0]]])
    eng = pkg.Engine(pkg.synth.default_config(pkg.capi.V1_SWEPT))
    assert eng.set_pointcloud(((cells + 0.5) * RES).astype(np.float32), RES, 2, np.zeros(3), np.array(dims) * RES) == tuple(dims)
    assert np.array_equal(eng.get_grid(pkg.capi.GRID_OCCUPANCY)[0] != 0, occ)
    if known:
        eng.map_known_enable(True)
        for box, value in fills:
            eng.map_known_fill(box, value)
    return eng, poses, rng_m


def _host(pkg, lib, eng, cam, poses, **params):
    """the host form on the ctx's own K, occupancy and box"""
    occ, bmin, bmax = eng.get_grid(pkg.capi.GRID_OCCUPANCY)
    params.pop("scratch_bytes", None)
    return pkg.engine.view_select_host(eng.map_known()[0], occ, bmin, bmax, RES, cam, poses, lib=lib, **params)


def _same(pkg, lib, eng, cam, poses, chunks=None, **params):
    want = _host(pkg, lib, eng, cam, poses, **params)
    got = eng.view_select(cam, poses, **params)
    for a, b, name in zip(got[:4], want[:4], ("rows", "select", "round", "claimed")):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (params, name, np.argwhere(a != b)[:8], a[:8], b[:8])
    assert [getattr(got[4], w) for w in sr.INFO_WORDS] == [getattr(want[4], w) for w in sr.INFO_WORDS], params
    info = got[4]
    assert info.chunks == ((1 if len(got[0]) else 0) if chunks is None else chunks), info.chunks
    assert info.gain_ms >= 0.0 and info.lists_ms >= 0.0 and info.select_ms >= 0.0
    return got


def _sweep(pkg, lib, eng, cam, poses, rng_m):
    n = len(poses)
    picked = 0
    for stride in STRIDES:
        rows, _ = eng.view_gain(cam, poses, stride=stride, max_range_m=rng_m)
        largest = int(rows[:, 1].max())
        for k_select, min_gain in ((n, 1), (3, 0), (1, 1), (n + 1, 0), (n, largest), (n, largest + 1)):
            got = _same(pkg, lib, eng, cam, poses, stride=stride, max_range_m=rng_m, k_select=k_select, min_gain=min_gain)
            assert got[0].tobytes() == rows.tobytes()           # the rows are the view gain's
            if (k_select, min_gain) == (n + 1, 0):              # more rounds than scored views: every scored view is picked, gain 0 or not
                assert got[4].n_selected == got[4].n_scored == int((rows[:, 0] == 0).sum()) < k_select and (got[2][rows[:, 0] == 0] >= 0).all()
            picked += got[4].n_selected
    return picked


@pytest.mark.parametrize("dims", GRIDS, ids=IDS)
def test_outputs_equal_the_host_form(pkg, product_lib, dims):
    eng, poses, rng_m = _case_engine(pkg, dims)
    cam = cam_of(pkg)
    assert _sweep(pkg, product_lib, eng, cam, poses, rng_m) > 0
    ext = np.array(dims) * RES                                  # a scan from the first pose's eye: its merge makes what that pose sees known
    ends = (np.random.default_rng(5).uniform(0.05, 0.95, (200, 3)) * ext).astype(np.float32)
    eng.integrate_scan(poses[0].reshape(3, 4)[:, 3], ends, np.zeros(len(ends), dtype=np.uint8), miss_weight=0)
    assert eng.map_known()[1].merges == 1
    _sweep(pkg, product_lib, eng, cam, poses, rng_m)
    eng.shift_map((2, -3, 5))
    _sweep(pkg, product_lib, eng, cam, poses, rng_m)
    rows, select, rnd, claimed, info = _same(pkg, product_lib, eng, cam, poses[:0], k_select=3)        # no views: nothing launched
    assert rows.shape == (0, 8) and select.tolist() == [[-1, 0, 0, 0]] * 3 and np.array_equal(claimed, eng.map_known()[0])
    assert (info.n_views, info.n_selected, info.chunks, info.gain_ms, info.lists_ms, info.select_ms) == (0, 0, 0, 0.0, 0.0, 0.0)


def test_the_chunk_size_does_not_change_a_byte(pkg, product_lib):
    dims = cs.BASE_DIMS
    eng, poses, rng_m = _case_engine(pkg, dims)
    cam = cam_of(pkg)
    n = len(poses)
    two_views = 2 * 4 * pkg.engine.known_words(dims)
    a = _same(pkg, product_lib, eng, cam, poses, chunks=n, stride=1, max_range_m=rng_m, k_select=n, scratch_bytes=0)
    b = _same(pkg, product_lib, eng, cam, poses, chunks=(n + 1) // 2, stride=1, max_range_m=rng_m, k_select=n, scratch_bytes=two_views)
    c = _same(pkg, product_lib, eng, cam, poses, chunks=1, stride=1, max_range_m=rng_m, k_select=n)
    for x, y, z in zip(a[:4], b[:4], c[:4]):
        assert x.tobytes() == y.tobytes() == z.tobytes()
    assert a[4].n_selected >= 3 and a[4].list_words == b[4].list_words == c[4].list_words > 0


@pytest.mark.parametrize("n_views", [1, 255, 256, 257, 600])
def test_the_pick_workgroups_width(pkg, product_lib, n_views):
    """the base case's poses repeated: a lane, the pick workgroup's 256 lanes and past them; the winners lie in the first eight"""
    eng, poses, rng_m = _case_engine(pkg, cs.BASE_DIMS)
    cam = cam_of(pkg)
    many = np.ascontiguousarray(np.resize(poses, (n_views, 12)))
    many[-1] = poses[7] if n_views > 8 else many[-1]            # the last lane's view is one that is picked
    got = _same(pkg, product_lib, eng, cam, many, stride=(3, 2), max_range_m=rng_m, k_select=6, min_gain=1)
    assert got[4].n_selected >= (3 if n_views >= 3 else 1) and (n_views <= PICK_BLOCK) == (n_views in (1, 255, 256))
    two = _same(pkg, product_lib, eng, cam, many, chunks=(n_views + 1) // 2, stride=(3, 2), max_range_m=rng_m, k_select=6, min_gain=1,
                scratch_bytes=2 * 4 * pkg.engine.known_words(cs.BASE_DIMS)) if n_views in (1, 257) else got
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got[:4], two[:4]))


def test_lists_of_no_entry_one_entry_and_more_than_a_workgroups(pkg, product_lib):
    dims = cs.BASE_DIMS
    eng, _, _ = _case_engine(pkg, dims)
    eng.map_known_fill((4, 10, 40, 4, 10, 40), 0)               # one unknown voxel in the seen half
    cam = cam_of(pkg, 32, 24, 20.0)
    look = pkg.engine.look_at
    poses = np.array([look((4.0, 5.0, 28.0), (0.0, 5.0, 28.0)), look((4.0, 5.25, 20.25), (0.0, 5.25, 20.25)), look((9.0, 5.0, 2.0), (9.0, 5.0, 30.0), up=(1, 0, 0))])
    words = [_host(pkg, product_lib, eng, cam, poses[j:j + 1], stride=1, max_range_m=4.0 if j < 2 else 40.0, k_select=1)[4].list_words for j in range(3)]
    assert words[:2] == [0, 1], words
    got = _same(pkg, product_lib, eng, cam, poses, stride=1, max_range_m=40.0, k_select=3, min_gain=0)
    one = [_host(pkg, product_lib, eng, cam, poses[j:j + 1], stride=1, max_range_m=40.0, k_select=1)[4].list_words for j in range(3)]
    assert one[0] == 0 and one[1] == 1 and one[2] > PICK_BLOCK and got[4].list_words == sum(one), one
    # the long view sees the lone voxel too: the other two tie at 0 and the lower index goes first; the one-entry view's voxel is overlap
    assert got[1][:, 0].tolist() == [2, 0, 1] and got[1][1:, 1].tolist() == [0, 0] and got[1][2, 3] == 1


def _raw(pkg, eng, cam, poses, outs, want_info=True, gain=None, **kw):
    p = pkg.capi.IsdfViewSelectParams()
    eng.lib.isdf_view_select_params_default(C.byref(p))
    p.gain.stride_u = p.gain.stride_v = 1
    p.gain.max_range_m = 40.0
    for key, v in (gain or {}).items():
        setattr(p.gain, key, v)
    for key, v in kw.items():
        setattr(p, key, v)
    info = pkg.capi.IsdfViewSelectInfo()
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)      # noqa: E731
    P = None if poses is None else np.ascontiguousarray(poses, dtype=np.float64)
    rc = eng.lib.isdf_view_select(eng.h, C.byref(cam), ptr(P), 0 if P is None else len(P), C.byref(p), *[ptr(a) for a in outs], C.byref(info) if want_info else None)
    return rc, info


def _err(eng):
    return (eng.lib.isdf_last_error(eng.h) or b"").decode()


def test_each_output_is_nullable(pkg, product_lib):
    dims = GRIDS[1]
    eng, poses, rng_m = _case_engine(pkg, dims)
    cam = cam_of(pkg)
    want = _same(pkg, product_lib, eng, cam, poses, stride=1, max_range_m=40.0, k_select=4)
    for skip in range(5):
        outs = [np.full_like(a, 7) for a in want[:4]]
        rc, info = _raw(pkg, eng, cam, poses, [None if i == skip else a for i, a in enumerate(outs)], want_info=skip != 4)
        assert rc == 0
        for i, (a, b) in enumerate(zip(outs, want[:4])):
            assert (a == 7).all() if i == skip else a.tobytes() == b.tobytes(), (skip, i)
        if skip != 4:
            assert [getattr(info, w) for w in sr.INFO_WORDS] == [getattr(want[4], w) for w in sr.INFO_WORDS]
    rc, info = _raw(pkg, eng, cam, poses, [None] * 4)
    assert rc == 0 and (info.n_selected, info.gain_selected) == (want[4].n_selected, want[4].gain_selected)
    assert _raw(pkg, eng, cam, poses, [None] * 4, want_info=False)[0] == 0


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
    cam = cam_of(pkg)

    def state():
        bits, info = eng.map_known()
        return bits.tobytes(), eng.get_grid(capi.GRID_OCCUPANCY)[0].tobytes(), info.merges, info.newly_known, info.n_known
    before = state()
    products = mu._products(pkg, eng)                           # counts, occupancy, ESDF, configuration space, bit map
    field, kept_report = eng.frontend_field(), eng.traj_check_points().tobytes()
    rep_a, last_a = eng.traj_check_watch_info(N)
    front0 = eng.map_frontier()[1].tobytes()
    look = pkg.engine.look_at
    poses = np.array([look(ms.ORIGIN, ms.ORIGIN + d) for d in ((1.0, 0.0, 0.0), (1.0, 0.1, 0.0), (0.0, 1.0, 0.2), (-1.0, 0.0, 0.1), (1.0, 0.0, 0.0))])
    first = _same(pkg, product_lib, eng, cam, poses, stride=1, max_range_m=40.0, k_select=5)
    assert first[4].n_selected >= 1 and first[4].gain_selected <= first[4].gain_solo_sum and first[2][4] == -1       # the repeated pose adds nothing
    live = _live(product_lib)
    second = eng.view_select(cam, poses, stride=1, max_range_m=40.0, k_select=5)
    assert _live(product_lib) == live
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first[:4], second[:4]))
    assert [getattr(first[4], w) for w in sr.INFO_WORDS] == [getattr(second[4], w) for w in sr.INFO_WORDS]
    assert state() == before and before[2] == 1
    mu._same(mu._products(pkg, eng), products)
    assert np.array_equal(eng.frontend_field().view(np.uint8), field.view(np.uint8))        # the kept field
    rep_b, last_b = eng.traj_check_watch_info(N)                # the armed watch: its report and the last index it folded
    _same_report(rep_b, rep_a, "after the view selection")
    assert last_b == last_a
    assert eng.traj_check_points().tobytes() == kept_report and eng.map_frontier()[1].tobytes() == front0
    assert eng.points_merge_check()["n_added"] >= 0             # the kept report is not stale: the grid epoch did not move
    rows, _ = eng.view_gain(cam, poses, stride=1, max_range_m=40.0)
    assert rows.tobytes() == first[0].tobytes()


def test_status_codes_and_their_order(pkg, product_lib):
    capi = pkg.capi
    dims = GRIDS[0]
    cam = cam_of(pkg)
    outs = [None] * 4
    E = capi.ISDF_ERR_INVALID_ARG
    eng, poses, _ = _case_engine(pkg, dims, known=False)        # an occupancy grid, the known mode off
    assert _raw(pkg, eng, cam, poses, outs)[0] == capi.ISDF_ERR_STATE and "known grid" in _err(eng)
    # every argument error comes before the state's: the view gain's in its order, then the selection's, then the key's room
    assert _raw(pkg, eng, pkg.engine.depth_camera(0, 6, 6, 6, 3, 3), poses, outs, gain={"stride_u": 0}, k_select=0)[0] == E and "camera" in _err(eng)
    assert _raw(pkg, eng, cam, None, outs, gain={"stride_u": 0}, k_select=0)[0] == E and "view gain parameters" in _err(eng)
    for kw in ({"k_select": 0}, {"min_gain": -1}):
        assert _raw(pkg, eng, cam, poses, outs, **kw)[0] == E and "view select parameters" in _err(eng), kw
    p = capi.IsdfViewSelectParams()
    eng.lib.isdf_view_select_params_default(C.byref(p))
    P = np.ascontiguousarray(poses)
    call = lambda pp, n: eng.lib.isdf_view_select(eng.h, C.byref(cam), pp, n, C.byref(p), None, None, None, None, None)      # noqa: E731
    assert call(P.ctypes.data_as(C.c_void_p), -1) == E and call(None, 2) == E and "view gain arguments" in _err(eng)
    assert call(P.ctypes.data_as(C.c_void_p), (1 << 24) + 1) == E and "2^24" in _err(eng)
    assert eng.lib.isdf_view_select(None, C.byref(cam), P.ctypes.data_as(C.c_void_p), len(P), C.byref(p), None, None, None, None, None) == E
    bare = pkg.Engine(pkg.synth.default_config(capi.V1_SWEPT))  # no map at all: the occupancy's sentence comes first
    assert _raw(pkg, bare, cam, poses, outs)[0] == capi.ISDF_ERR_STATE and "occupancy" in _err(bare)
    eng.map_known_enable(True)
    assert _raw(pkg, eng, cam, poses, outs)[0] == 0
    with pytest.raises(pkg.engine.IsdfError) as e:
        eng.view_select(cam, poses, k_select=0)
    assert e.value.code == E


def _open_scene(pkg, dims):
    """every occupied voxel behind the cameras: nothing occupied in any frustum that looks down +x from x >= 6"""
    rng = np.random.default_rng(3)
    occ = np.zeros(dims, dtype=bool)
    occ[:4] = rng.uniform(size=(4,) + dims[1:]) < 0.2
    cloud = ((np.repeat(np.argwhere(occ), 2, axis=0) + 0.5) * RES).astype(np.float32)
    eng = pkg.Engine(pkg.synth.default_config(pkg.capi.V1_SWEPT))
    assert eng.set_pointcloud(cloud, RES, 2, np.zeros(3), np.array(dims) * RES) == tuple(dims)
    eng.map_known_enable(True)
    return eng


def test_the_marginals_are_what_integrating_the_views_in_order_makes_known(pkg, product_lib):
    dims = GRIDS[2]
    eng = _open_scene(pkg, dims)
    cam = cam_of(pkg, 32, 24, 20.0)
    eyes = (np.array([[6, 10, 35], [6, 10, 37], [8, 6, 50], [6, 10, 35], [7, 12, 20]]) + 0.5) * RES
    poses = np.array([pkg.engine.look_at(e, e + (1.0, 0.1, -0.2)) for e in eyes])
    image = np.zeros((cam.height, cam.width), dtype=np.uint16)
    for stride, rng_m in (((1, 1), 4.0), ((3, 2), 40.0)):
        eng.map_known_fill(None, 0)
        rows, select, rnd, claimed, info = _same(pkg, product_lib, eng, cam, poses, stride=stride, max_range_m=rng_m, k_select=len(poses), min_gain=1)
        assert not rows[:, 4].any() and 3 <= info.n_selected < len(poses) and rnd[3] == -1 and info.gain_selected < info.gain_solo_sum
        for r in range(info.n_selected):
            eng.integrate_depth(cam, poses[select[r, 0]], image, stride=stride, max_range_m=rng_m, no_return_is_free=True)
            assert eng.map_known()[1].newly_known == select[r, 1], (r, select)
        assert np.array_equal(eng.map_known()[0], claimed)
        again = _same(pkg, product_lib, eng, cam, poses, stride=stride, max_range_m=rng_m, k_select=len(poses), min_gain=1)
        assert again[4].n_selected == 0 and (again[1] == [-1, 0, 0, 0]).all() and np.array_equal(again[3], claimed) and not again[0][:, 1].any()


def test_next_view_set(pkg, product_lib):
    """K as one integrate_depth leaves it: the set's poses are candidates of next_views, in the order picked, with the selection's marginals"""
    dims = GRIDS[2]
    eng = _open_scene(pkg, dims)
    cam = cam_of(pkg, 32, 24, 20.0)
    eye = (np.array([6, 10, 35]) + 0.5) * RES
    empty = np.zeros((cam.height, cam.width), dtype=np.uint16)
    eng.integrate_depth(cam, pkg.engine.look_at(eye, eye + (1.0, 0.1, -0.2)), empty, stride=1, max_range_m=6.0, no_return_is_free=True)
    ring = pkg.engine.view_ring_offsets((1.0, 1.5, 2.0), 8, (-0.5, 0.0, 0.5))
    params = {"stride": 1, "max_range_m": 4.0, "min_gain": 5, "k_best": 2}
    _, cand, poses, _, best, _ = eng.next_views(cam, ring, **params)
    listed = best[best >= 0]
    assert len(listed) >= 2
    set_poses, marginals, index, info = eng.next_view_set(cam, ring, k_select=3, **params)
    want = _host(pkg, product_lib, eng, cam, poses[listed], stride=1, max_range_m=4.0, k_select=3, min_gain=1)
    n = want[4].n_selected
    assert n == info.n_selected == len(set_poses) >= 1 and np.array_equal(marginals, want[1][:n, 1]) and np.array_equal(index, listed[want[1][:n, 0]])
    assert set_poses.tobytes() == poses[index].tobytes() and (np.diff(marginals) <= 0).all() and marginals[0] == cand[listed, 3].max()
    assert info.gain_selected == marginals.sum() <= info.gain_solo_sum == cand[index, 3].sum()
