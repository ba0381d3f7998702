"""The kept clearance report folded across map updates (isdf_traj_check_set_watch mode 1; csrc/traj_watch.hip).

The yardstick is always the existing full check on a ctx whose map holds the union: every field of isdf_traj_check_info except the
three times, the piece minima, the kept rows and what isdf_points_merge_check makes of them must be equal to the byte."""
import ctypes as C
import gc

import numpy as np
import pytest

from common import small_world

pytestmark = pytest.mark.gpu

RES, SAFETY, MARGIN = 0.5, 0.5, 1.0
DIMS = (48, 48, 32)
CONE = ((0.8, 0.3, 1.6), 1.9)
N = 4
T = np.array([1.5, 1.2, 1.8, 1.5])
P0, P1 = np.array([6.0, 8.0, 6.0]), np.array([18.0, 14.0, 9.0])         # a straight line across the map: its box leaves voxels outside
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


def _ids(cells):
    cells = np.asarray(cells, dtype=np.int64).reshape(-1, 3)
    return (cells[:, 0] * DIMS[1] + cells[:, 1]) * DIMS[2] + cells[:, 2]


def _cells(ids):
    ids = np.asarray(ids, dtype=np.int64)
    return np.stack([ids // (DIMS[1] * DIMS[2]), (ids // DIMS[2]) % DIMS[1], ids % DIMS[2]], axis=1).astype(np.int32)


def _centres(ids):
    return (_cells(ids) + 0.5) * RES


def _occ(ids):
    occ = np.zeros(DIMS, dtype=np.uint8)
    occ.reshape(-1)[np.asarray(ids, dtype=np.int64)] = 1
    return occ


def _shape(pkg, kind):
    synth = pkg.synth
    if kind == "cone":
        return synth.make_shape("RoundedCone", params=CONE[0], bound_radius=CONE[1])
    if kind == "ball":
        return synth.make_shape("Ball", params=(0.6,), bound_radius=0.6)
    return synth.make_shape("RoundedCone", params=CONE[0])              # no bound radius: culled == 0


def _engine(pkg, ids, form="grid", shape="cone", watch=1):
    """a ctx holding the voxels `ids`: form "grid" = isdf_set_grid (updated by isdf_update_voxels), "cloud" = isdf_set_pointcloud"""
    capi = pkg.capi
    eng = pkg.Engine(pkg.synth.default_config(capi.V1_SWEPT, kernel_size=9, integral_intervs=16, safety_hor=SAFETY))
    eng.set_shape(_shape(pkg, shape))
    if form == "grid":
        eng.set_grid(_occ(ids), (0, 0, 0), RES, capi.GRID_OCCUPANCY)
    else:
        eng.set_pointcloud(_centres(ids).astype(np.float32), RES, sta_threshold=1, bmin=(0, 0, 0), bmax=np.array(DIMS) * RES)
    eng.form = form
    if watch is not None:
        eng.traj_check_set_watch(watch)
    return eng


def _update(eng, ids, **params):
    ids = np.asarray(ids, dtype=np.int64)
    params.setdefault("full_fraction", 1.0)             # the incremental path whatever share of this small map the dirty box holds
    if eng.form == "grid":
        return eng.update_voxels(_cells(ids), **params)
    return eng.update_pointcloud(_centres(ids).astype(np.float32), **params)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_report(got, want, what):
    for k, v in want.items():
        if k in TIMES:
            continue
        assert np.array_equal(_bits(got[k]), _bits(v)), (what, k, got[k], v)


def _yardstick(pkg, ids, shape="cone", mode=0, merge=False):
    """the full check on a fresh ctx (watch off) holding `ids`: report, rows, and - merge - the point set a merge from empty gives"""
    eng = _engine(pkg, ids, shape=shape, watch=None)
    rep = eng.traj_check(T, CM, margin=MARGIN, mode=mode)
    rows = eng.traj_check_points()
    out = dict(rep=rep, rows=rows)
    if merge:
        eng.set_points(np.zeros((0, 3)))
        out["merge"] = eng.points_merge_check()
        out["points"] = eng.get_points()
        out["step"] = eng.eval_single(T, CM)
    eng.close()
    return out


def _hold(pkg, eng, ids, what, shape="cone", mode=0, merge=False, want=None):
    """the watched ctx against the yardstick on the union `ids`"""
    want = want or _yardstick(pkg, ids, shape=shape, mode=mode, merge=merge)
    rep, last = eng.traj_check_watch_info(N)
    _same_report(rep, want["rep"], what)
    rows = eng.traj_check_points()
    assert rows.shape == want["rows"].shape and rows.tobytes() == want["rows"].tobytes(), what
    if merge:
        eng.set_points(np.zeros((0, 3)))
        info = eng.points_merge_check()
        for k in info:
            if k != "merge_ms":
                assert info[k] == want["merge"][k], (what, k)
        assert eng.get_points().tobytes() == want["points"].tobytes(), what
        c, gT, gC = eng.eval_single(T, CM)                          # the step after the merge reads the set and its lastTstar
        c0, gT0, gC0 = want["step"]
        assert c == c0 and np.array_equal(_bits(gT), _bits(gT0)) and np.array_equal(_bits(gC), _bits(gC0)), what
    return rep, last, want


def _locate_piece(t):
    idx = 0
    while idx < N and t > T[idx]:
        t -= T[idx]; idx += 1
    return N - 1 if idx == N else idx


_SCENE = {}


def _scene(pkg):
    """The universe: the occupied voxels of the random 48 x 48 x 32 map plus eight voxels on the trajectory itself (penetrating for
    sure), checked once.  From its rows: an initial map of a few hundred voxels, some below the margin, WITHOUT the global minimum's
    voxel; frame 1 with that voxel, rows below and above every initial row's id, voxels outside far_r and outside the box; more frames."""
    if _SCENE:
        return _SCENE
    occ_full, _, _ = small_world(pkg, seed=3, shape=DIMS, res=RES)
    c = CM.reshape(3, N, 6)
    on_path = [np.floor((c[:, i, 0] + c[:, i, 1] * f * T[i]) / RES).astype(np.int64) for i in range(N) for f in (0.3, 0.7)]
    universe = np.unique(np.concatenate([np.flatnonzero(occ_full.reshape(-1)), _ids(on_path)]))
    y = _yardstick(pkg, universe)
    rows, rep = y["rows"], y["rep"]
    row_ids = _ids(np.floor(rows[:, :3] / RES))
    assert np.all(np.diff(row_ids) > 0) and len(row_ids) >= 24 and rep["n_penetrating"] >= 2
    m = rep["min_voxel"]
    rng = np.random.default_rng(5)
    rest = rng.permutation(np.setdiff1d(universe, row_ids))
    keep = row_ids[(row_ids != m) & (row_ids != row_ids[0]) & (row_ids != row_ids[-1])]
    init_rows, f1_rows, f2_rows, f3_rows, big_rows = keep[0::2], keep[1::8], keep[3::8], keep[5::8], keep[7::8]
    pen = row_ids[(rows[:, 3] < 0) & (row_ids != m)]
    f1_rows = np.unique(np.concatenate([f1_rows, [m, row_ids[0], row_ids[-1], pen[0]]]))
    init_rows = np.setdiff1d(init_rows, f1_rows)
    _SCENE.update(universe=universe, m=m, row_ids=row_ids,
                  init=np.unique(np.concatenate([init_rows, rest[:350]])),
                  f1=np.unique(np.concatenate([f1_rows, rest[350:500]])),
                  f2=np.unique(np.concatenate([np.setdiff1d(f2_rows, f1_rows), rest[500:600]])),
                  f3=np.unique(np.concatenate([np.setdiff1d(f3_rows, f1_rows), rest[600:700]])),
                  big=np.unique(np.concatenate([np.setdiff1d(big_rows, f1_rows), rest[700:1400]])),
                  init_rows=init_rows, f1_rows=f1_rows)
    return _SCENE


def _armed(pkg, form="grid", shape="cone", mode=0, ids=None):
    s = _scene(pkg)
    eng = _engine(pkg, s["init"] if ids is None else ids, form=form, shape=shape)
    rep = eng.traj_check(T, CM, margin=MARGIN, mode=mode)
    return s, eng, rep


# ---- 1. one update -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["grid", "cloud"])
def test_one_update_equals_the_full_check(pkg, product_lib, form):
    s, eng, rep0 = _armed(pkg, form=form)
    assert 300 <= len(s["init"]) <= 900 and rep0["n_below_margin"] > 0 and rep0["min_voxel"] != s["m"]
    rep_a, last_a = eng.traj_check_watch_info(N)
    _same_report(rep_a, rep0, "armed")
    assert last_a["path"] == 0 and last_a["updates_folded"] == 0 and last_a["new_min_voxel"] == -1
    uinfo = _update(eng, s["f1"])
    assert uinfo.n_new_voxels == len(s["f1"]) and uinfo.path == 1
    union = np.union1d(s["init"], s["f1"])
    rep, last, want = _hold(pkg, eng, union, f"one update ({form})", merge=True)
    print(f"\n[traj_watch] {form}: new {last['new_voxels']} in box {last['new_in_box']} candidates {last['new_candidates']} qualified {last['new_qualified']} "
          f"below {last['new_below_margin']} penetrating {last['new_penetrating']} min {last['new_min_clearance']!r} | rows {rep0['n_below_margin']} -> "
          f"{rep['n_below_margin']} | select {last['select_ms']:.3f} field {last['field_ms']:.3f} reduce {last['reduce_ms']:.3f} merge {last['merge_ms']:.3f} ms")
    # the scenario: inside and outside far_r, outside the box, below the margin, penetrating, ids on both sides, the new global minimum
    assert last["path"] == 1 and last["updates_folded"] == 1 and last["new_voxels"] == len(s["f1"])
    assert 0 < last["new_candidates"] < last["new_in_box"] < last["new_voxels"]
    assert last["new_below_margin"] >= 4 and last["new_penetrating"] >= 2
    assert s["f1_rows"].min() < s["init_rows"].min() and s["f1_rows"].max() > s["init_rows"].max()
    assert last["min_changed"] == 1 and rep["min_voxel"] == s["m"] == last["new_min_voxel"]
    # the sums are the difference of two full checks; the rest is a host reduction of isdf_swept_sdf over exactly the new voxels
    for k, n in (("occupied_in_box", "new_in_box"), ("candidates", "new_candidates"), ("qualified", "new_qualified"),
                 ("n_below_margin", "new_below_margin"), ("n_penetrating", "new_penetrating")):
        assert last[n] == want["rep"][k] - rep0[k], (k, last[n])
    val, ts = eng.swept_sdf(T, CM, _centres(s["f1"]))
    q = val != 10.0
    assert (last["new_qualified"], last["new_below_margin"], last["new_penetrating"]) == (int(q.sum()), int((q & (val < MARGIN)).sum()), int((q & (val < 0)).sum()))
    j = int(np.lexsort((s["f1"][q], val[q]))[0])
    assert last["new_min_clearance"] == val[q][j] and last["new_min_tstar"] == ts[q][j] and last["new_min_voxel"] == s["f1"][q][j]
    assert last["new_min_piece"] == _locate_piece(ts[q][j])
    eng.close()


# ---- 2. three updates in a row -------------------------------------------------------------------------------------------------
def test_three_updates_against_one_full_check(pkg, product_lib):
    s, eng, _ = _armed(pkg, form="cloud")
    for f in ("f1", "f2", "f3"):
        # (the second update takes its full path with a complete list: the fold still reads the list)
        uinfo = _update(eng, s[f], **({"full_fraction": 0.0} if f == "f2" else {}))
        assert uinfo.n_new_voxels == len(s[f]) and uinfo.path == (2 if f == "f2" else 1)
        assert eng.traj_check_watch_info(N)[1]["path"] == 1
    union = np.unique(np.concatenate([s["init"], s["f1"], s["f2"], s["f3"]]))
    rep, last, _ = _hold(pkg, eng, union, "three updates", merge=True)
    assert last["updates_folded"] == 3 and last["path"] == 1 and last["new_voxels"] == len(s["f3"])
    eng.close()


# ---- 3. more than 256 new voxels: several workgroups, an undefined list order ------------------------------------------------------
def test_large_frame_twice_gives_the_same_bytes(pkg, product_lib):
    s = _scene(pkg)
    assert len(s["big"]) > 600
    union = np.union1d(s["init"], s["big"])
    want = _yardstick(pkg, union)
    got = []
    for run in range(2):
        _, eng, _ = _armed(pkg, form="grid")
        order = np.random.default_rng(run).permutation(len(s["big"]))       # the caller's order differs too
        assert _update(eng, s["big"][order]).n_new_voxels == len(s["big"])
        rep, last, _ = _hold(pkg, eng, union, f"large frame, run {run}", want=want)
        assert last["new_voxels"] == len(s["big"]) > 256 and last["new_below_margin"] > 0
        got.append((rep, eng.traj_check_points(), {k: v for k, v in last.items() if not k.endswith("_ms")}))
        eng.close()
    _same_report(got[0][0], got[1][0], "two runs")
    assert got[0][1].tobytes() == got[1][1].tobytes() and got[0][2] == got[1][2]


# ---- 4. both query modes, a radius-less shape, an analytic shape with a radius ------------------------------------------------------
@pytest.mark.parametrize("shape,mode", [("cone", 1), ("noradius", 0), ("ball", 0), ("ball", 1)])
def test_modes_and_shapes(pkg, product_lib, shape, mode):
    s, eng, rep0 = _armed(pkg, shape=shape, mode=mode)
    assert rep0["culled"] == (0 if shape == "noradius" else 1)
    _update(eng, s["f1"])
    rep, last, _ = _hold(pkg, eng, np.union1d(s["init"], s["f1"]), f"{shape}, mode {mode}", shape=shape, mode=mode)
    assert last["path"] == 1 and last["new_below_margin"] > 0
    if shape == "noradius":
        assert last["new_candidates"] == last["new_in_box"] == last["new_voxels"]
    eng.close()


# ---- 5. the update's full path ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["grid", "cloud"])
def test_forced_full_update_path(pkg, product_lib, form):
    s, eng, rep0 = _armed(pkg, form=form)
    uinfo = _update(eng, s["f1"], max_new_voxels=1)
    assert uinfo.path == 2 and uinfo.n_new_voxels == len(s["f1"])
    rep, last, want = _hold(pkg, eng, np.union1d(s["init"], s["f1"]), f"full path ({form})", merge=True)
    assert last["path"] == 2 and last["updates_folded"] == 1 and last["new_voxels"] == len(s["f1"])
    assert last["min_changed"] == 1 and last["new_min_voxel"] == s["m"] and last["new_below_margin"] == rep["n_below_margin"] - rep0["n_below_margin"]
    _update(eng, s["f2"])                                       # and the list path goes on from a report the full path left
    _, last, _ = _hold(pkg, eng, np.unique(np.concatenate([s["init"], s["f1"], s["f2"]])), "list after full")
    assert last["path"] == 1 and last["updates_folded"] == 2
    eng.close()


# ---- 6. an update that adds nothing ----------------------------------------------------------------------------------------------
def test_update_that_occupies_nothing(pkg, product_lib):
    s, eng, _ = _armed(pkg, form="grid")
    _update(eng, s["f1"])
    rep, last = eng.traj_check_watch_info(N)
    rows = eng.traj_check_points()
    again = np.concatenate([s["f1"][:40], s["f1"][:40], s["init"][:40]])         # occupied already, and duplicates
    assert _update(eng, again).n_new_voxels == 0
    rep2, last2 = eng.traj_check_watch_info(N)
    _same_report(rep2, rep, "nothing new")
    assert last2 == last and last2["updates_folded"] == 1 and eng.traj_check_points().tobytes() == rows.tobytes()
    eng.close()
    # the point form: points that lift no count over the threshold
    capi = pkg.capi
    cloud = pkg.Engine(pkg.synth.default_config(capi.V1_SWEPT, kernel_size=9, integral_intervs=16, safety_hor=SAFETY))
    cloud.set_shape(_shape(pkg, "cone")); cloud.form = "cloud"
    pts = _centres(s["init"]).astype(np.float32)
    cloud.set_pointcloud(np.concatenate([pts, pts, pts]), RES, sta_threshold=3, bmin=(0, 0, 0), bmax=np.array(DIMS) * RES)
    cloud.traj_check_set_watch(1)
    rep = cloud.traj_check(T, CM, margin=MARGIN)
    assert _update(cloud, s["f1"]).n_new_voxels == 0               # one point per voxel, three needed
    rep2, last2 = cloud.traj_check_watch_info(N)
    _same_report(rep2, rep, "below the threshold")
    assert last2["updates_folded"] == 0 and last2["path"] == 0
    cloud.close()


# ---- 7. mode 0 -------------------------------------------------------------------------------------------------------------------
def test_mode_0_leaves_the_report_alone(pkg, product_lib):
    capi = pkg.capi
    s = _scene(pkg)
    fresh = _engine(pkg, s["init"], watch=None)
    info = capi.IsdfTrajCheckInfo()
    assert product_lib.isdf_traj_check_watch_info(fresh.h, C.byref(info), None, None) == capi.ISDF_ERR_STATE       # a fresh ctx
    for mode in (2, -1):
        assert product_lib.isdf_traj_check_set_watch(fresh.h, mode) == capi.ISDF_ERR_INVALID_ARG
    assert product_lib.isdf_traj_check_watch_info(fresh.h, None, None, None) == capi.ISDF_ERR_INVALID_ARG
    fresh.traj_check(T, CM, margin=MARGIN)
    rows = fresh.traj_check_points()
    assert _update(fresh, s["f1"]).n_new_voxels == len(s["f1"])
    assert fresh.traj_check_points().tobytes() == rows.tobytes()            # stale, untouched: today's behaviour
    assert product_lib.isdf_traj_check_watch_info(fresh.h, C.byref(info), None, None) == capi.ISDF_ERR_STATE
    fresh.traj_check_set_watch(1)                                           # the mode alone arms nothing: a check does
    assert product_lib.isdf_traj_check_watch_info(fresh.h, C.byref(info), None, None) == capi.ISDF_ERR_STATE
    fresh.traj_check(T, CM, margin=MARGIN)
    assert product_lib.isdf_traj_check_watch_info(fresh.h, C.byref(info), None, None) == 0
    fresh.traj_check_set_watch(0)
    assert product_lib.isdf_traj_check_watch_info(fresh.h, C.byref(info), None, None) == capi.ISDF_ERR_STATE
    fresh.close()
    multi = pkg.Engine(pkg.synth.default_config(capi.V1_SWEPT, kernel_size=9, integral_intervs=16, safety_hor=SAFETY), devices=[0, 0])
    assert product_lib.isdf_traj_check_set_watch(multi.h, 1) == capi.ISDF_ERR_UNSUPPORTED
    multi.close()


# ---- 8. disarming ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["set_pointcloud", "set_shape", "release"])
def test_disarming(pkg, product_lib, how):
    capi = pkg.capi
    s, eng, _ = _armed(pkg, form="cloud")
    if how == "set_pointcloud":
        eng.set_pointcloud(_centres(s["init"]).astype(np.float32), RES, sta_threshold=1, bmin=(0, 0, 0), bmax=np.array(DIMS) * RES)
    elif how == "set_shape":
        eng.set_shape(_shape(pkg, "ball"))
    else:
        eng.traj_check_release()
    info = capi.IsdfTrajCheckInfo()
    assert product_lib.isdf_traj_check_watch_info(eng.h, C.byref(info), None, None) == capi.ISDF_ERR_STATE
    kept = None if how == "release" else eng.traj_check_points()
    assert _update(eng, s["f1"]).n_new_voxels == len(s["f1"])              # succeeds, folds nothing
    assert product_lib.isdf_traj_check_watch_info(eng.h, C.byref(info), None, None) == capi.ISDF_ERR_STATE
    if kept is not None:
        eng._traj_check_rows = len(kept)
        assert eng.traj_check_points().tobytes() == kept.tobytes()
    rep = eng.traj_check(T, CM, margin=MARGIN)                              # the mode outlives the check: armed again
    rep2, last = eng.traj_check_watch_info(N)
    _same_report(rep2, rep, how)
    assert last["updates_folded"] == 0
    eng.close()


# ---- 9. the field repair and the watch in the same update ------------------------------------------------------------------------
def test_field_repair_and_watch_in_one_update(pkg, product_lib):
    import field_reference as fr
    capi = pkg.capi
    s = _scene(pkg)
    free = np.setdiff1d(np.arange(np.prod(DIMS)), s["universe"])
    goal = _cells([free[len(free) // 2]])[0]
    fe = capi.frontend_config(kernel_size=5, max_roll=30.0, max_pitch=30.0, ang_res=30.0, safeh=0.0)

    def prepared(ids, repair):
        e = _engine(pkg, ids, shape="ball", watch=1 if repair else None)
        e.frontend_build(fe)
        if repair:
            e.frontend_field_set_repair(1)
        e.frontend_field_build((goal + 0.5) * RES)
        return e
    eng = prepared(s["init"], True)
    eng.traj_check(T, CM, margin=MARGIN)
    uinfo = _update(eng, s["f1"], full_fraction=1.0)
    assert uinfo.field_dropped == 0 and uinfo.path == 1
    union = np.union1d(s["init"], s["f1"])
    _, last, _ = _hold(pkg, eng, union, "with the field repair", shape="ball")
    assert last["updates_folded"] == 1
    fresh = prepared(union, False)
    assert fr.same_bytes(eng.frontend_field(), fresh.frontend_field())
    assert eng.frontend_field_repair_info().reached_voxels == int(np.isfinite(fresh.frontend_field()).sum())
    eng.close(); fresh.close()


# ---- 10. lifetime ------------------------------------------------------------------------------------------------------------------
def test_every_byte_comes_back(pkg, product_lib):
    def live():
        out = (C.c_longlong * 2)()
        product_lib.isdf_debug_live_bytes(out)
        return int(out[0]), int(out[1])
    s = _scene(pkg)
    gc.collect()
    before = live()
    _, eng, _ = _armed(pkg, form="cloud")
    _update(eng, s["f1"])
    held = live()
    assert held[0] > before[0] and held[1] > before[1]
    _update(eng, s["f2"])                                       # a smaller frame: the fold's scratch only grows
    _update(eng, s["f3"], max_new_voxels=1)
    eng.traj_check_watch_info(N)
    eng.close()
    assert live() == before, "bytes still held after isdf_destroy (device, pinned)"
