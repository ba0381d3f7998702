"""The routed view selection on the device (csrc/view_select.hip: isdf_view_select_routed) against the plain host form
(isdf_view_select_routed_host, which tests/test_view_route_host.py holds to the NumPy restatement): every output and every integer word
of the info compared with == on bytes.  The host form gets its costs from isdf_frontend_field_host on the table isdf_frontend_cspace_get
gives; for a gated field the TEST gates the table with tests/known_erode_reference.py, as tests/test_gpu_field_known.py does.  The map,
the robot and the scene are that file's (24 x 20 x 70 voxels at 0.5 m, kernel_size 5, 3 x 3 attitudes); the eyes are
tests/view_route_cases.py's; the field is built towards the robot's cell."""
import ctypes as C

import numpy as np
import pytest

import field_reference as fr
import known_erode_reference as er
import known_reference as kr
import test_gpu_field_known as fk
import test_gpu_map_update as mu
import view_route_cases as rc
import view_route_reference as rr
from test_gpu_map_update import BMIN, DIMS, RES, _live
from test_view_gain_host import cam_of

pytestmark = pytest.mark.gpu

N_ATT = fk.N_ATT
ROBOT = fk._centre(rc.START)
GAIN = {"stride": 1, "max_range_m": rc.RANGE_M}
NAMES = ("rows", "select", "round", "claimed", "cost", "util")
PICK_BLOCK = 256                        # csrc/view_select.hip's VS_BLOCK
_SHARED = {}


def shared(pkg, lib):
    """computed once: the table, K, the host fields towards the robot's cell (ungated, and gated at the front end's radius), the poses"""
    if not _SHARED:
        eng = fk._engine(pkg)
        table = eng.frontend_cspace_table()
        k = kr.unpack(eng.map_known()[0], DIMS)
        e = er.erode(k, mu.SIDE, 0)
        plain, reach = pkg.frontend_field_host(table, rc.START, N_ATT, lib=lib)
        gated, reach_g = pkg.frontend_field_host(table * e[..., None].astype(np.uint32), rc.START, N_ATT, lib=lib)
        assert reach and reach_g
        _SHARED.update(table=table, k=k, e=e, d={False: plain, True: gated}, poses=rc.gpu_poses(BMIN, RES))
    return _SHARED


def _build(eng, gated):
    info = eng.frontend_field_build_known(ROBOT)[0] if gated else eng.frontend_field_build(ROBOT)
    assert info.reachable == 1 and info.status == 0


def _host(pkg, lib, eng, cam, poses, cost, **params):
    """the host form on the ctx's own K, occupancy and box"""
    occ, bmin, bmax = eng.get_grid(pkg.capi.GRID_OCCUPANCY)
    return pkg.engine.view_select_routed_host(eng.map_known()[0], occ, bmin, bmax, RES, cam, poses, cost, lib=lib, **params)


def _same(got, want, source=0, what=None):
    """got: Engine.view_select_routed's tuple, want: the host form's"""
    for a, b, name in zip(got[:6], want[:6], NAMES):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (what, name, np.argwhere(a != b)[:8], a[:8], b[:8])
    assert rr.info_words(got[7]) == rr.info_words(want[6]), (what, rr.info_words(got[7]), rr.info_words(want[6]))
    assert np.float64(got[7].cost_selected).tobytes() == np.float64(want[6].cost_selected).tobytes()
    assert (got[7].cost_source, want[6].cost_source) == (source, 1)
    info = got[7]
    assert info.cost_ms >= 0.0 and info.paths_ms >= 0.0 and info.select.select_ms >= 0.0


def _routed(pkg, lib, eng, cam, poses, d, what=None, **params):
    """the device form with the ctx's field against the host form with the host field's values at the eyes"""
    cost = rc.field_at(d, rc.eyes_of(poses), BMIN, RES)
    got = eng.view_select_routed(cam, poses, **GAIN, **params)
    params.pop("path_cap", None)
    _same(got, _host(pkg, lib, eng, cam, poses, cost, **GAIN, **params), 0, what)
    return got


@pytest.mark.parametrize("gated", [False, True], ids=["ungated", "gated"])
def test_a_wall_between_near_and_far(pkg, product_lib, gated):
    S = shared(pkg, product_lib)
    poses, d, table = S["poses"], S["d"][gated], S["table"]
    eyes = rc.eyes_of(poses)
    cost = rc.field_at(d, eyes, BMIN, RES)
    occ = fk.scene()
    # the scene, by the host field alone
    assert not occ[rc.EYES[rc.CLOSED]] and not table[rc.EYES[rc.CLOSED]].any() and np.isinf(cost[rc.CLOSED])      # free in the occupancy, closed in the configuration space
    assert np.isinf(cost[rc.OUTSIDE]) and np.isfinite(cost[[rc.NEAR, rc.FAR, rc.BAFFLED, rc.BAD, rc.LOW, rc.FAR2, rc.MID]]).all()
    assert np.isinf(cost[rc.UNSEEN]) == gated and not S["k"][rc.EYES[rc.UNSEEN]] and table[rc.EYES[rc.UNSEEN]].any()
    straight = np.linalg.norm(np.array([rc.EYES[rc.BAFFLED], rc.EYES[rc.LOW]]) - np.array(rc.START), axis=1)
    assert straight[0] < straight[1] and cost[rc.BAFFLED] > cost[rc.LOW] + 3.0          # near in a straight line, far by the way under the baffle
    assert cost[rc.FAR] > cost[rc.BAFFLED] > cost[rc.NEAR] > 0.0
    eng = fk._engine(pkg)
    cam = cam_of(pkg)
    _build(eng, gated)
    n = len(poses)
    got = _routed(pkg, product_lib, eng, cam, poses, d, k_select=n)
    assert got[4].tobytes() == eng.frontend_field(eyes).tobytes() == cost.tobytes()
    rows, select, rnd, _, _, util, _, info = got
    assert rows[[rc.OUTSIDE, rc.BAD], 0].tolist() == [1, 1] and (rows[[rc.NEAR, rc.FAR, rc.CLOSED, rc.UNSEEN, rc.LOW], 0] == 0).all() and rows[rc.LOW, 1] == 0
    assert info.n_unreachable == (2 if gated else 1) and info.n_over_budget == 0 and info.n_eligible == info.select.n_scored - info.n_unreachable
    assert rnd[rc.CLOSED] == rnd[rc.OUTSIDE] == rnd[rc.BAD] == rnd[rc.LOW] == -1 and (not gated or rnd[rc.UNSEEN] == -1) and info.select.n_selected >= 3
    # the near view goes before the far one, which alone has the larger gain; its copy adds nothing afterwards
    assert rows[rc.FAR, 1] > rows[rc.NEAR, 1] > 0 and 0 <= rnd[rc.NEAR] < rnd[rc.FAR] and rnd[rc.NEAR2] == -1
    assert eng.view_select(cam, poses, k_select=n, **GAIN)[0].tobytes() == rows.tobytes()
    for params in ({"k_select": 2, "cost0": 0.125}, {"k_select": n + 2, "cost0": 50.0}, {"k_select": n, "max_cost": float(cost[rc.BAFFLED])},
                   {"k_select": n, "max_cost": float(np.nextafter(cost[rc.BAFFLED], 0.0)), "min_gain": 3}, {"k_select": 3, "max_cost": 0.0}):
        got = _routed(pkg, product_lib, eng, cam, poses, d, what=params, **params)
        if "max_cost" in params and params["max_cost"] > 0.0:
            assert (got[2][rc.BAFFLED] >= 0) == (params["max_cost"] == cost[rc.BAFFLED]) and got[7].n_over_budget >= 2
    assert got[7].select.n_selected == 0 and got[7].n_eligible == 0 and np.array_equal(got[3], eng.map_known()[0])       # max_cost 0: the robot's own cell alone
    got = _routed(pkg, product_lib, eng, cam, poses[:0], d, k_select=3)          # no views: nothing launched
    assert got[1].tolist() == [[-1, 0, 0, 0]] * 3 and not got[5].any() and np.array_equal(got[3], eng.map_known()[0]) and got[7].cost_ms == 0.0


@pytest.mark.parametrize("n_views", [1, 255, 256, 257, 600])
def test_the_pick_workgroups_width(pkg, product_lib, n_views):
    """the scene's poses repeated; the first pick stands in the last lane alone, the second in lanes 255 and 256 - a tie across the
    pick workgroup's first and second trip"""
    S = shared(pkg, product_lib)
    poses, d = S["poses"], S["d"][False]
    eng = fk._engine(pkg)
    cam = cam_of(pkg)
    _build(eng, False)
    base_cost = rc.field_at(d, rc.eyes_of(poses), BMIN, RES)
    first, second = _host(pkg, product_lib, eng, cam, poses, base_cost, k_select=2, **GAIN)[1][:, 0]
    assert first >= 0 and second >= 0 and not np.array_equal(poses[first], poses[second], equal_nan=True)
    rest = np.array([p for j, p in enumerate(poses) if not any(np.array_equal(p, poses[w], equal_nan=True) for w in (first, second))])
    many = np.ascontiguousarray(np.resize(rest, (n_views, 12)))
    many[-1] = poses[first]
    tie = n_views > PICK_BLOCK + 1                              # (with 257 views lane 256 is the last one: the first pick's)
    if tie:
        many[PICK_BLOCK - 1] = many[PICK_BLOCK] = poses[second]
    got = _routed(pkg, product_lib, eng, cam, many, d, what=n_views, k_select=6)
    assert got[1][0, 0] == n_views - 1 and got[7].select.n_selected >= (2 if n_views > 1 else 1) and (n_views <= PICK_BLOCK) == (n_views in (1, 255, 256))
    if tie:
        assert got[1][1, 0] == PICK_BLOCK - 1 and got[2][PICK_BLOCK] == -1 and got[4][PICK_BLOCK - 1] == got[4][PICK_BLOCK]
    if n_views in (1, 257):                                     # two chunks of the view gain give the same bytes
        two = eng.view_select_routed(cam, many, k_select=6, scratch_bytes=((n_views + 1) // 2) * 4 * pkg.engine.known_words(DIMS), **GAIN)
        assert two[7].select.chunks == (2 if n_views > 1 else 1) and all(a.tobytes() == b.tobytes() for a, b in zip(got[:6], two[:6]))


@pytest.mark.parametrize("gated", [False, True], ids=["ungated", "gated"])
def test_paths_are_the_fields_paths_from_the_picked_eyes(pkg, product_lib, gated):
    S = shared(pkg, product_lib)
    poses, d = S["poses"], S["d"][gated]
    eng = fk._engine(pkg)
    cam = cam_of(pkg)
    _build(eng, gated)
    n = len(poses)
    for cap in (256, 6, 1):
        got = _routed(pkg, product_lib, eng, cam, poses, d, what=cap, k_select=n + 1, path_cap=cap)
        ns = got[7].select.n_selected
        pn, pxyz, prp = got[6]
        assert 3 <= ns < n and pn.shape == (n + 1,) and pxyz.shape == (n + 1, cap, 3) and prp.shape == (n + 1, cap, 2)
        picked = rc.eyes_of(poses)[got[1][:ns, 0]]
        wn, wxyz, wrp = eng.frontend_field_paths(picked, cap)
        assert pn[:ns].tobytes() == wn.tobytes() and pxyz[:ns].tobytes() == wxyz.tobytes() and prp[:ns].tobytes() == wrp.tobytes()
        assert not pn[ns:].any() and not pxyz[ns:].any() and not prp[ns:].any() and (pn[:ns] >= 2).all()
        assert (pn[:ns] > cap).any() == (cap < 256) and got[7].paths_ms > 0.0
        if cap == 256:                                          # a walk runs from the eye's cell to the robot's, down the field
            for r in range(ns):
                cells = fk._cells(pxyz[r, :pn[r]])
                assert tuple(cells[0]) == tuple(fk._cells(picked[r])) and tuple(cells[-1]) == rc.START and (np.diff(d[tuple(cells.T)]) < 0).all()
                assert d[tuple(cells[0])] == got[5][r, 0]
    without = eng.view_select_routed(cam, poses, k_select=n + 1, **GAIN)
    assert without[6] is None and without[7].paths_ms == 0.0 and all(a.tobytes() == b.tobytes() for a, b in zip(got[:6], without[:6]))


def _raw(pkg, eng, cam, poses, cost=None, outs=(None,) * 9, want_info=True, select=None, **kw):
    p = pkg.capi.IsdfViewSelectRoutedParams()
    eng.lib.isdf_view_select_routed_params_default(C.byref(p))
    p.select.gain.max_range_m = rc.RANGE_M
    for key, v in (select or {}).items():
        setattr(p.select, key, v)
    for key, v in kw.items():
        setattr(p, key, v)
    info = pkg.capi.IsdfViewSelectRoutedInfo()
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)      # noqa: E731
    P = None if poses is None else np.ascontiguousarray(poses, dtype=np.float64)
    cc = None if cost is None else np.ascontiguousarray(cost, dtype=np.float64)
    rc_ = eng.lib.isdf_view_select_routed(eng.h, C.byref(cam), ptr(P), 0 if P is None else len(P), ptr(cc), C.byref(p), *[ptr(a) for a in outs],
                                          C.byref(info) if want_info else None)
    return rc_, info, (eng.lib.isdf_last_error(eng.h) or b"").decode()


def test_a_callers_cost_array(pkg, product_lib):
    """no field on the ctx at all: the array form needs none; path outputs with it are refused"""
    S = shared(pkg, product_lib)
    poses = S["poses"]
    eng = fk._engine(pkg)
    cam = cam_of(pkg)
    n = len(poses)
    rng = np.random.default_rng(11)
    for cost in (rc.field_at(S["d"][True], rc.eyes_of(poses), BMIN, RES), rng.uniform(0.0, 30.0, n), np.zeros(n), np.full(n, np.inf)):
        for params in ({"k_select": n}, {"k_select": 3, "cost0": 0.5, "max_cost": 20.0}):
            got = eng.view_select_routed(cam, poses, cost=cost, **GAIN, **params)
            _same(got, _host(pkg, product_lib, eng, cam, poses, cost, **GAIN, **params), 1, params)
            assert got[4].tobytes() == np.asarray(cost, dtype=np.float64).tobytes() and got[6] is None
    E = pkg.capi.ISDF_ERR_INVALID_ARG
    with pytest.raises(pkg.engine.IsdfError) as err:
        eng.view_select_routed(cam, poses, cost=np.zeros(n), path_cap=8, **GAIN)
    assert err.value.code == E and "cost array" in str(err.value) + (eng.lib.isdf_last_error(eng.h) or b"").decode()
    for bad in (np.where(np.arange(n) == 4, np.nan, 1.0), np.where(np.arange(n) == n - 1, -1e-9, 1.0)):
        rc_, _, msg = _raw(pkg, eng, cam, poses, cost=bad)
        assert rc_ == E and "cost" in msg
    # the argument errors and their order: the selection's, then the routed form's, then the field's state
    for kw, word in (({"select": {"k_select": 0, "min_gain": 0}, "cost0": 0.0}, "view select parameters"), ({"select": {"min_gain": 0}, "cost0": 0.0}, "min_gain >= 1"),
                     ({"cost0": 0.0}, "routed view select parameters"), ({"cost0": np.inf}, "routed view select parameters"),
                     ({"max_cost": np.nan}, "routed view select parameters"), ({"max_cost": -1.0}, "routed view select parameters"),
                     ({"path_cap": -1}, "routed view select parameters")):
        rc_, _, msg = _raw(pkg, eng, cam, poses, **kw)          # (no field: the state's error would be ISDF_ERR_STATE)
        assert rc_ == E and word in msg, (kw, msg)
    assert eng.lib.isdf_view_select_routed(None, C.byref(cam), None, 0, None, None, *([None] * 10)) == E
    bare = mu._engine(pkg, mu._clouds()[0], esdf=False)         # no known grid: the selection's state error comes before the routed arguments
    rc_, _, msg = _raw(pkg, bare, cam, poses, cost0=0.0)
    assert rc_ == pkg.capi.ISDF_ERR_STATE and "known grid" in msg


def test_the_field_state(pkg, product_lib):
    S = shared(pkg, product_lib)
    poses = S["poses"]
    cam = cam_of(pkg)
    n = len(poses)
    St = pkg.capi.ISDF_ERR_STATE
    extra = fk._centre([[5, 3, 5], [5, 3, 5]]).astype(np.float32)        # two points: one new occupied voxel, in seen space, away from everything
    eng = fk._engine(pkg)
    rc_, _, msg = _raw(pkg, eng, cam, poses)
    assert rc_ == St and "isdf_frontend_field_build" in msg    # a front end, no field
    rc_, _, msg = _raw(pkg, eng, cam, poses[:0])
    assert rc_ == St                                            # ... also with no views
    _build(eng, False)
    first = eng.view_select_routed(cam, poses, k_select=n, path_cap=64, **GAIN)
    assert first[7].select.n_selected >= 3
    assert eng.update_pointcloud(extra, **mu.INCR).field_dropped == 1
    rc_, _, msg = _raw(pkg, eng, cam, poses)
    assert rc_ == St and "isdf_frontend_field_build" in msg    # a dropped field is no field
    none = mu._engine(pkg, mu._in_cells(np.argwhere(fk.scene()), 2, np.random.default_rng(3)), esdf=False, frontend=False)
    none.map_known_enable(True)
    rc_, _, msg = _raw(pkg, none, cam, poses)
    assert rc_ == St and "isdf_frontend_build" in msg          # no front end
    # repaired in place, the field serves the call as a fresh build does
    eng = fk._engine(pkg)
    eng.frontend_field_set_repair(1)
    _build(eng, False)
    assert eng.update_pointcloud(extra, **mu.INCR).field_dropped == 0 and eng.frontend_field_repair_info().closed_voxels > 0
    repaired = eng.view_select_routed(cam, poses, k_select=n, path_cap=64, **GAIN)
    _build(eng, False)
    fresh = eng.view_select_routed(cam, poses, k_select=n, path_cap=64, **GAIN)
    for a, b in zip(repaired[:6] + repaired[6], fresh[:6] + fresh[6]):
        assert a.tobytes() == b.tobytes()
    assert rr.info_words(repaired[7]) == rr.info_words(fresh[7]) and repaired[7].select.n_selected >= 3
    cost = rc.field_at(eng.frontend_field(), rc.eyes_of(poses), BMIN, RES)
    _same(repaired, _host(pkg, product_lib, eng, cam, poses, cost, k_select=n, **GAIN))


def test_the_call_is_read_only_and_allocates_once(pkg, product_lib):
    """a gated field that follows (mode 1) with a follow report, beside K and the epochs"""
    S = shared(pkg, product_lib)
    poses = S["poses"]
    cam = cam_of(pkg)
    n = len(poses)
    eng = fk._engine(pkg)
    eng.frontend_field_set_known_follow(1)
    _build(eng, True)
    eng.map_known_fill((0, 0, 35, 6, 6, 37), 1)                 # a followed change: a follow report is kept
    follow = eng.frontend_field_follow_info()
    assert follow.opening == 1

    def state():
        bits, info = eng.map_known()
        f = eng.frontend_field_follow_info()
        return (bits.tobytes(), eng.get_grid(pkg.capi.GRID_OCCUPANCY)[0].tobytes(), info.merges, info.newly_known, info.n_known, eng.frontend_field().tobytes(),
                eng.frontend_field_known_info(), bytes(f), eng.frontend_cspace_table().tobytes(), eng.map_frontier()[1].tobytes())
    before = state()
    d = eng.frontend_field()
    first = _routed(pkg, product_lib, eng, cam, poses, d, k_select=n, path_cap=64)
    assert first[7].select.n_selected >= 3
    live = _live(product_lib)
    second = eng.view_select_routed(cam, poses, k_select=n, path_cap=64, **GAIN)
    assert _live(product_lib) == live
    third = eng.view_select_routed(cam, poses, cost=first[4], k_select=n, **GAIN)         # the array form stages n doubles more, once
    live = _live(product_lib)
    eng.view_select_routed(cam, poses, cost=first[4], k_select=n, **GAIN)
    assert _live(product_lib) == live
    for a, b in zip(first[:6] + first[6], second[:6] + second[6]):
        assert a.tobytes() == b.tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first[:6], third[:6]))
    assert rr.info_words(first[7]) == rr.info_words(second[7]) == rr.info_words(third[7])
    assert state() == before
    plain = eng.view_select(cam, poses, k_select=n, **GAIN)     # the plain selection beside it is untouched by the routed state
    rows, _ = eng.view_gain(cam, poses, **GAIN)
    assert plain[0].tobytes() == rows.tobytes() == first[0].tobytes()


def test_the_utility_is_the_ieee_quotient(pkg, product_lib):
    """util_out from select_out and cost_out by NumPy's float64 division, for costs with full mantissas (sums of sqrt 2 and sqrt 3)"""
    S = shared(pkg, product_lib)
    poses, d = S["poses"], S["d"][False]
    eng = fk._engine(pkg)
    cam = cam_of(pkg)
    _build(eng, False)
    n = len(poses)
    seen = 0
    for cost0 in (1.0, 1.0 / 3.0, 0.7, 3.141592653589793, 1e-3, 977.0):
        rows, select, rnd, claimed, cost, util, _, info = _routed(pkg, product_lib, eng, cam, poses, d, what=cost0, k_select=n, cost0=cost0)
        ns = info.select.n_selected
        m, c = select[:ns, 1], cost[select[:ns, 0]]
        want = np.float64(m) / (np.float64(cost0) + c)
        assert util[:ns, 0].tobytes() == c.tobytes() and util[:ns, 1].tobytes() == want.tobytes() and not util[ns:].any(), (cost0, util, want)
        total = np.float64(0.0)                                 # the picked costs, added in pick order
        for v in c:
            total = total + v
        assert np.float64(info.cost_selected).tobytes() == total.tobytes()
        seen += int((np.modf(c)[0] != 0.0).sum())
    assert seen >= 6                                            # costs that are not whole numbers were divided by


def test_next_view_set_routed(pkg, product_lib):
    S = shared(pkg, product_lib)
    eng = fk._engine(pkg)
    cam = cam_of(pkg, 32, 24, 20.0)
    ring = pkg.engine.view_ring_offsets((1.0, 1.5, 2.0), 8, (-1.5, -1.0, -0.5))
    params = {"stride": 1, "max_range_m": 4.0, "min_gain": 5, "k_best": 2}
    _, cand, poses, _, best, _ = eng.next_views(cam, ring, **params)
    listed = best[best >= 0]
    assert len(listed) >= 2
    for known in (True, False):
        set_poses, marginals, costs, ways, index, info = eng.next_view_set_routed(cam, ring, ROBOT, known=known, radius=0, k_select=3, cost0=2.0, **params)
        table = S["table"] * S["k"][..., None].astype(np.uint32) if known else S["table"]          # radius 0: E = K
        d, reach = pkg.frontend_field_host(table, rc.START, N_ATT, lib=product_lib)
        assert reach and fr.same_bytes(eng.frontend_field(), d) and eng.frontend_field_known_info() == ((1, 0, 0) if known else (0, 0, 0))
        cost = rc.field_at(d, rc.eyes_of(poses[listed]), BMIN, RES)
        want = _host(pkg, product_lib, eng, cam, poses[listed], cost, stride=1, max_range_m=4.0, k_select=3, min_gain=1, cost0=2.0)
        n = want[6].select.n_selected
        assert n == info.select.n_selected == len(set_poses) == len(ways) >= 1
        assert np.array_equal(marginals, want[1][:n, 1]) and np.array_equal(index, listed[want[1][:n, 0]]) and costs.tobytes() == want[5][:n, 0].tobytes()
        assert set_poses.tobytes() == poses[index].tobytes() and np.isfinite(costs).all() and info.n_eligible >= n
        for r in range(n):                                      # robot -> eye, up the field
            cells = fk._cells(ways[r])
            assert tuple(cells[0]) == rc.START and tuple(cells[-1]) == tuple(fk._cells(set_poses[r].reshape(3, 4)[:, 3])), (r, cells[[0, -1]])
            assert (np.diff(d[tuple(cells.T)]) > 0).all() and d[tuple(cells[-1])] == costs[r]
        u = want[5][:n, 1]
        assert (u > 0).all() and u[0] == (marginals[0] / (2.0 + costs[0]))
