"""Trajectory clearance check on the device (isdf_traj_check*, isdf_traj_collide).

The report must be what a user could compute before this existed: every occupied voxel centre of the map through the field
query (Engine.swept_sdf), reduced in numpy - bit for bit, in both modes, for analytic robots with a bound radius, a mesh robot
and a shape without a radius (no cull).  The selection must be a superset of what the field query qualifies, the oracle agrees
within the field tests' tolerances, and the check leaves the V1 step and the kept swept mesh alone."""
import ctypes as C
import os

import numpy as np
import pytest

from common import make_pair, small_world

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "ref_demo_inputs.npz")
MESHES = os.path.join(ROOT, "tests", "golden", "ref_meshes.npz")
SHAPES = {"RoundedCone": ((0.8, 0.3, 1.6), 1.9), "Torus": ((1.2, 0.25), 1.45), "Box": ((1.2, 0.4, 0.3), 1.3)}     # test_gpu_swept_mesh.py
SAFETY = 0.5
BALL_R = 0.5
# a trajectory of small_world that grazes obstacles (the mesh tests' margin = 4.0 only keeps it off the walls)
WORLD_SEED, TRAJ_SEED, TRAJ_N, PIECE_T = 3, 43, 6, 1.5
ORACLE_MARGIN = 0.2371


def _world(pkg, traj_seed=TRAJ_SEED):
    synth = pkg.synth
    occ, esdf, res = small_world(pkg, seed=WORLD_SEED)
    ext = np.array(occ.shape) * res
    T, Cf = synth.random_trajectory(ext, TRAJ_N, seed=traj_seed, piece_T=PIECE_T, margin=4.0, occ=occ, res=res)
    return occ, res, T, synth.colmajor(Cf)


def _engine(pkg, shape, occ, res, origin=(0, 0, 0), safety_hor=SAFETY, variant=None):
    capi, synth = pkg.capi, pkg.synth
    cfg = synth.default_config(capi.V1_SWEPT if variant is None else variant, safety_hor=safety_hor)
    eng = pkg.Engine(cfg)
    eng.set_shape(shape)
    eng.set_grid(occ, origin, res, capi.GRID_OCCUPANCY)
    return eng


def _centres(occ, origin, res, box=None):
    """occupied voxels in ascending voxel index (x * ny + y) * nz + z and their centres (index + 0.5) * res + origin"""
    o = occ != 0
    if box is not None:
        keep = np.zeros_like(o)
        keep[box[0][0]:box[1][0] + 1, box[0][1]:box[1][1] + 1, box[0][2]:box[1][2] + 1] = True
        o = o & keep
    vox = np.flatnonzero(o.ravel())
    ijk = np.stack(np.unravel_index(vox, occ.shape), axis=1)
    return vox.astype(np.int64), (ijk + 0.5) * res + np.asarray(origin, dtype=np.float64)


def _piece_of(T, t):
    """Trajectory::locatePieceIdx: sequential subtraction, `>` rule"""
    idx = 0
    while idx < len(T) and t > T[idx]:
        t -= T[idx]; idx += 1
    return min(idx, len(T) - 1)


def _reduce(T, vox, P, val, ts, margin):
    q = val != 10.0
    rep = {"qualified": int(q.sum()), "n_below_margin": int((q & (val < margin)).sum()), "n_penetrating": int((q & (val < 0.0)).sum())}
    piece_min = np.full(len(T), 10.0)
    for j in np.flatnonzero(q):
        i = _piece_of(T, ts[j])
        piece_min[i] = min(piece_min[i], val[j])
    rep["piece_min"] = piece_min
    if q.any():
        jq = np.flatnonzero(q)
        j = jq[np.argmin(val[jq])]                 # argmin: the first of equals = the lowest voxel index
        rep.update(min_clearance=val[j], min_tstar=ts[j], min_voxel=int(vox[j]), min_point=P[j], min_piece=_piece_of(T, ts[j]))
    else:
        rep.update(min_clearance=10.0, min_tstar=-1.0, min_voxel=-1, min_point=np.zeros(3), min_piece=-1)
    v = q & (val < margin)
    rep["rows"] = np.column_stack([P[v], val[v], ts[v]]).reshape(-1, 5)
    return rep


def _brute(eng, occ, origin, res, T, cm, margin, mode, box=None):
    vox, P = _centres(occ, origin, res, box)
    val, ts = eng.swept_sdf(T, cm, P, mode=mode)
    rep = _reduce(T, vox, P, val, ts, margin)
    rep["vox"], rep["P"], rep["val"], rep["ts"] = vox, P, val, ts
    return rep


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _assert_same(rep, rows, want, what):
    print(f"[traj_check] {what}: occupied_in_box {rep['occupied_in_box']} candidates {rep['candidates']} qualified {rep['qualified']} "
          f"below {rep['n_below_margin']} penetrating {rep['n_penetrating']} min {rep['min_clearance']!r} t* {rep['min_tstar']!r} "
          f"voxel {rep['min_voxel']} piece {rep['min_piece']} | brute: qualified {want['qualified']} below {want['n_below_margin']} "
          f"penetrating {want['n_penetrating']} min {want['min_clearance']!r} voxel {want['min_voxel']} | "
          f"ms {rep['select_ms']:.3f} / {rep['field_ms']:.3f} / {rep['reduce_ms']:.3f}")
    for k in ("qualified", "n_below_margin", "n_penetrating", "min_voxel", "min_piece"):
        assert rep[k] == want[k], (what, k, rep[k], want[k])
    for k in ("min_clearance", "min_tstar", "min_point", "piece_min"):
        assert np.array_equal(_bits(rep[k]), _bits(want[k])), (what, k, rep[k], want[k])
    assert rows.shape == want["rows"].shape and np.array_equal(_bits(rows), _bits(want["rows"])), what
    assert rep["candidates"] >= rep["qualified"]


def _shape(pkg, name):
    synth = pkg.synth
    if name in SHAPES:
        return synth.make_shape(name, params=SHAPES[name][0], bound_radius=SHAPES[name][1])
    if name == "RoundedCone_noradius":
        return synth.make_shape("RoundedCone", params=SHAPES["RoundedCone"][0], bound_radius=0.0)
    g = np.load(MESHES)
    return synth.make_mesh_shape(g[name + "_V"], g[name + "_F"])


# ---- 1. equals brute force, bit for bit ---------------------------------------------------------------------------------
@pytest.mark.parametrize("mode_name", ["PLANNER", "CLOSED"])
@pytest.mark.parametrize("shape_name", ["RoundedCone", "Torus", "Box", "drone", "RoundedCone_noradius"])
def test_check_equals_brute_force_bit_for_bit(pkg, product_lib, shape_name, mode_name):
    capi = pkg.capi
    mode = getattr(capi, "SWEPT_FIELD_" + mode_name)
    occ, res, T, cm = _world(pkg)
    eng = _engine(pkg, _shape(pkg, shape_name), occ, res)
    want = _brute(eng, occ, (0, 0, 0), res, T, cm, SAFETY, mode)
    rep = eng.traj_check(T, cm, mode=mode)                    # margin None: cfg.safety_hor
    rows = eng.traj_check_points()
    assert rep["margin"] == SAFETY
    _assert_same(rep, rows, want, f"{shape_name} {mode_name}")
    # not a trivial world: something is below the margin, and the selection did select
    assert (rep["piece_min"] < SAFETY).sum() >= 1 and rep["n_below_margin"] >= 1
    if shape_name == "RoundedCone_noradius":
        assert rep["culled"] == 0 and rep["far_r"] == 0.0 and rep["candidates"] == rep["occupied_in_box"] == int((occ != 0).sum())
    else:
        assert rep["culled"] == 1 and 0 < rep["candidates"] < rep["occupied_in_box"] <= int((occ != 0).sum())
    if mode == capi.SWEPT_FIELD_PLANNER:
        assert eng.traj_collide(T, cm) == (want["n_penetrating"] > 0)


# ---- 2. against the oracle ------------------------------------------------------------------------------------------------
def _dense_path(T, cm, n=4000):
    N = len(T)
    C6 = np.asarray(cm).reshape(3, 6 * N)
    ts = np.linspace(0.0, T.sum(), n)
    starts = np.concatenate([[0.0], np.cumsum(T)[:-1]])
    piece = np.clip(np.searchsorted(starts, ts, side="right") - 1, 0, N - 1)
    tl = ts - starts[piece]
    out = np.zeros((n, 3))
    for a in range(3):
        c = C6[a].reshape(N, 6)[piece]
        out[:, a] = ((((c[:, 5] * tl + c[:, 4]) * tl + c[:, 3]) * tl + c[:, 2]) * tl + c[:, 1]) * tl + c[:, 0]
    return out


def _oracle_reduce(o, T, cm, vox, P, margin):
    val = np.zeros(len(P)); ts = np.zeros(len(P))
    for k in range(len(P)):
        val[k], ts[k], _, _ = o.swept_sdf(T, cm, P[k], tstar0=-1.0)
    return _reduce(T, vox, P, val, ts, margin), val, ts


def _near_path(occ, res, T, cm, radius):
    from scipy.spatial import cKDTree
    vox, P = _centres(occ, (0, 0, 0), res)
    d, _ = cKDTree(_dense_path(T, cm)).query(P)
    near = d <= radius
    return vox[near], P[near]


@pytest.mark.parametrize("shape_name", ["RoundedCone", "Torus", "Box"])
def test_check_against_the_oracle(pkg, orc, product_lib, shape_name):
    """The oracle's own query over every occupied voxel near the path (a superset of the candidates), reduced in numpy.
    Tolerances of test_gpu_swept_mesh.py::_check_planner_vs_oracle: value 1e-9 * max(1, |s|), t* 2e-5.  ORACLE_MARGIN was
    chosen so that no oracle value lies within that tolerance of the margin or of 0 (checked on the oracle alone)."""
    capi, synth = pkg.capi, pkg.synth
    occ, res, T, cm = _world(pkg)
    shape = _shape(pkg, shape_name)
    cfg = synth.default_config(capi.V1_SWEPT, safety_hor=SAFETY)
    eng, o = make_pair(pkg, orc, cfg, shape, occ=occ, res=res)
    rep = eng.traj_check(T, cm, margin=ORACLE_MARGIN)
    # every candidate lies within far_r of a coarse sample, which is on the path
    vox, P = _near_path(occ, res, T, cm, rep["far_r"] + res)
    assert rep["candidates"] <= len(vox) <= 6000
    want, val, ts = _oracle_reduce(o, T, cm, vox, P, ORACLE_MARGIN)
    tol = lambda s: 1e-9 * max(1.0, abs(s))     # noqa: E731
    edge = sum(1 for s in val if s != 10.0 and (abs(s - ORACLE_MARGIN) <= tol(s) or abs(s) <= tol(s)))
    print(f"[traj_check] oracle {shape_name}: {len(vox)} points, qualified {want['qualified']} (device {rep['qualified']}), "
          f"min {want['min_clearance']!r} (device {rep['min_clearance']!r}), values at an edge {edge}")
    assert edge <= 0.01 * want["qualified"]
    if edge == 0:
        for k in ("qualified", "n_below_margin", "n_penetrating"):
            assert rep[k] == want[k], (k, rep[k], want[k])
    assert want["qualified"] > 100 and want["n_below_margin"] >= 1
    assert abs(rep["min_clearance"] - want["min_clearance"]) <= tol(want["min_clearance"])
    # (several voxels may share the minimum within the tolerance - deep inside a box every point reads minus its half width - so
    # the device's voxel is held to the oracle's value and t* AT that voxel)
    k = int(np.flatnonzero(vox == rep["min_voxel"])[0])
    assert abs(val[k] - want["min_clearance"]) <= 2 * tol(want["min_clearance"]) and abs(rep["min_tstar"] - ts[k]) <= 2e-5
    assert rep["min_piece"] == _piece_of(T, ts[k])
    for i in range(len(T)):
        assert abs(rep["piece_min"][i] - want["piece_min"][i]) <= tol(want["piece_min"][i]), (i, rep["piece_min"][i], want["piece_min"][i])
    rows = eng.traj_check_points()
    if edge == 0:
        assert rows.shape == want["rows"].shape and np.array_equal(rows[:, :3], want["rows"][:, :3])
        assert np.all(np.abs(rows[:, 3] - want["rows"][:, 3]) <= 1e-9 * np.maximum(1.0, np.abs(want["rows"][:, 3])))
        assert np.all(np.abs(rows[:, 4] - want["rows"][:, 4]) <= 2e-5)


# ---- 3. the selection is a superset -------------------------------------------------------------------------------------
# isdf_shape_default states no bound radius for any kind (bound_radius = 0 throughout its table), so with the registry constants
# every kind takes the no-cull path; the radii below are the ones this tree states for analytic shapes (the field and mesh tests,
# tools/shapes_bench.py, benchlib/configs.py)
_REGISTRY = ["Torus", "Cappedtorus", "CappedCone", "WireframeBox", "BendLinear", "TwistBox", "BendBox", "Table", "Trefoil",
             "SmoothDifference", "SmoothIntersection", "CSG", "Box", "Ball", "Torus_big", "BendLinear_big", "SmoothIntersection_big"]
_STATED = {"RoundedCone": ((0.8, 0.3, 1.6), 1.9), "Torus": ((1.2, 0.25), 1.45), "Box": ((1.2, 0.4, 0.3), 1.3), "Ball": ((0.5,), 0.5),
           "CappedCone": ((0.0, 0.0, -0.9, 0.0, 0.0, 0.9, 0.6, 0.25), 1.1), "BendLinear": ((1.3, 0.2), 1.6),
           "SmoothIntersection": ((1.2, 1.2, 0.2, 0.4, 0.1), 1.7), "Box_bench": ((0.8, 0.15, 0.15), 0.83)}


@pytest.mark.parametrize("name", sorted(_STATED))
def test_selection_is_a_superset_of_what_the_field_qualifies(pkg, product_lib, name):
    capi, synth = pkg.capi, pkg.synth
    occ, res, T, cm = _world(pkg)
    params, R = _STATED[name]
    eng = _engine(pkg, synth.make_shape(name.split("_")[0], params=params, bound_radius=R), occ, res)
    band = 2 * SAFETY + 0.1
    for mode in (capi.SWEPT_FIELD_PLANNER, capi.SWEPT_FIELD_CLOSED):
        rep = eng.traj_check(T, cm, margin=band, mode=mode)
        rows = eng.traj_check_points()
        b = _brute(eng, occ, (0, 0, 0), res, T, cm, band, mode)
        assert rep["culled"] == 1 and rep["far_r"] == R + band
        # as many qualified among the candidates as in the whole map: no voxel outside the candidates reads anything but 10 / -1
        assert rep["qualified"] == b["qualified"] > 0, name
        q = b["val"] != 10.0
        assert np.all(b["ts"][~q] == -1.0)
        _assert_same(rep, rows, b, name)
        assert 0 < rep["candidates"] < rep["occupied_in_box"]


@pytest.mark.parametrize("name", _REGISTRY)
def test_registry_constants_state_no_radius_and_are_not_culled(pkg, product_lib, name):
    capi, synth = pkg.capi, pkg.synth
    occ, res, T, cm = _world(pkg)
    shape = synth.make_shape(name)
    assert shape.bound_radius == 0.0
    eng = _engine(pkg, shape, occ, res)
    rep = eng.traj_check(T, cm)
    assert rep["culled"] == 0 and rep["candidates"] == rep["occupied_in_box"] == int((occ != 0).sum())
    b = _brute(eng, occ, (0, 0, 0), res, T, cm, SAFETY, capi.SWEPT_FIELD_PLANNER)
    _assert_same(rep, eng.traj_check_points(), b, name + " (registry constants)")


# ---- 4. a ball ----------------------------------------------------------------------------------------------------------
def _ball_curve(pkg, N=3, piece_T=1.2):
    """a gentle arc (radius 6 m, 100 degrees) through the middle of a 24 x 24 x 16 m map"""
    synth = pkg.synth
    ang = np.linspace(0.0, np.deg2rad(100.0), N + 1)
    pts = np.stack([6.0 * np.cos(ang), 6.0 * np.sin(ang), 0.4 * np.sin(2 * ang)], axis=1) + np.array([10.0, 10.0, 5.0])
    head = np.zeros((3, 3)); head[:, 0] = pts[0]
    tail = np.zeros((3, 3)); tail[:, 0] = pts[-1]
    T = np.full(N, piece_T)
    return T, synth.colmajor(synth.minco_coeffs(head, tail, pts[1:-1].T, T))


def _dist_to_polyline(poly, x):
    A, B = poly[:-1], poly[1:]
    AB = B - A
    t = np.clip(np.einsum("ij,ij->i", x - A, AB) / np.maximum(np.einsum("ij,ij->i", AB, AB), 1e-300), 0.0, 1.0)
    return np.linalg.norm(x - (A + t[:, None] * AB), axis=1).min()


def test_ball_far_from_obstacles_and_with_a_voxel_on_its_path(pkg, product_lib):
    capi, synth = pkg.capi, pkg.synth
    res = 0.5
    T, cm = _ball_curve(pkg)
    occ = np.zeros((48, 48, 32), dtype=np.uint8)
    occ[1:4, 1:4, 28:31] = 1                                   # a block in a far corner
    ball = synth.make_shape("Ball", params=(BALL_R,), bound_radius=BALL_R)
    eng = _engine(pkg, ball, occ, res)
    rep = eng.traj_check(T, cm)
    assert rep["min_clearance"] == 10.0 and rep["min_tstar"] == -1.0 and rep["min_voxel"] == -1 and rep["min_piece"] == -1
    assert rep["qualified"] == rep["n_below_margin"] == rep["n_penetrating"] == 0 and np.all(rep["piece_min"] == 10.0)
    assert eng.traj_check_points().shape == (0, 5)
    assert eng.traj_collide(T, cm) is False
    dp = C.POINTER(C.c_double)
    assert eng.lib.isdf_traj_collide(eng.h, T.size, T.ctypes.data_as(dp), np.ascontiguousarray(cm).ctypes.data_as(dp)) == 0
    # one voxel on the path, in the middle of piece 1 (t = 1.8 of 3 x 1.2 s); the path sampled every 1e-4 s
    D = T.sum()
    n = int(round(D / 1e-4)) + 1
    poly = _dense_path(T, cm, n=n)
    on_path = poly[int(round(1.8 / 1e-4))]
    ijk = np.floor(on_path / res).astype(int)
    occ[ijk[0], ijk[1], ijk[2]] = 1
    eng.set_grid(occ, (0, 0, 0), res, capi.GRID_OCCUPANCY)
    rep = eng.traj_check(T, cm)
    centre = (ijk + 0.5) * res
    want = _dist_to_polyline(poly, centre) - BALL_R
    print(f"[traj_check] ball: min_clearance {rep['min_clearance']!r} distance to path - r {want!r} t* {rep['min_tstar']!r}")
    assert want < 0.0
    assert rep["n_penetrating"] >= 1 and rep["qualified"] == 1
    assert abs(rep["min_clearance"] - want) <= 1e-6
    assert rep["min_piece"] == 1 and rep["min_voxel"] == (ijk[0] * 48 + ijk[1]) * 32 + ijk[2]
    assert np.array_equal(rep["min_point"], centre)
    assert rep["piece_min"][1] == rep["min_clearance"] and rep["piece_min"][0] == 10.0 and rep["piece_min"][2] == 10.0
    assert eng.traj_collide(T, cm) is True
    assert eng.lib.isdf_traj_collide(eng.h, T.size, T.ctypes.data_as(dp), np.ascontiguousarray(cm).ctypes.data_as(dp)) == 1


# ---- 5. state isolation -------------------------------------------------------------------------------------------------
def test_check_leaves_the_v1_step_and_the_kept_mesh_alone(pkg, product_lib):
    capi, synth = pkg.capi, pkg.synth
    occ, res, T, cm = _world(pkg)
    way = np.asarray(cm).reshape(3, TRAJ_N, 6)[:, 1:, 0].T
    pts = synth.constraint_points(occ, (0, 0, 0), res, way, half=4 * res * 1.5)
    assert pts.shape[0] > 50
    shape = _shape(pkg, "RoundedCone")
    Tq, cmq = _ball_curve(pkg)
    out = {}
    dp = C.POINTER(C.c_double)
    for with_check in (False, True):
        eng = _engine(pkg, shape, occ, res)
        eng.set_points(pts)
        V, F, _ = eng.swept_mesh(Tq, cmq, 0.2)
        r1 = eng.eval_single(T, cm)
        if with_check:
            eng.traj_check(Tq * 1.7, cmq, mode=capi.SWEPT_FIELD_CLOSED)
            b = eng.traj_check(T * 0.8, cm)
            b_rows = eng.traj_check_points()
            b2 = eng.traj_check(T * 0.8, cm)
            b2_rows = eng.traj_check_points()
            # two checks in a row: identical bytes
            for k in b:
                if k.endswith("_ms"):
                    continue
                assert (np.array_equal(_bits(b[k]), _bits(b2[k])) if isinstance(b[k], np.ndarray) else b[k] == b2[k]), k
            assert b_rows.tobytes() == b2_rows.tobytes() and b["n_below_margin"] == b_rows.shape[0] > 0
            # a buffer that is too small: nothing written
            buf = np.full((b_rows.shape[0] + 2, 5), 7.0)
            assert eng.lib.isdf_traj_check_get(eng.h, buf.ctypes.data_as(dp), b_rows.shape[0] - 1) == capi.ISDF_ERR_OVERFLOW
            assert np.all(buf == 7.0)
            assert eng.lib.isdf_traj_check_get(eng.h, buf.ctypes.data_as(dp), b_rows.shape[0] + 2) == capi.ISDF_OK
            assert np.array_equal(buf[:b_rows.shape[0]], b_rows) and np.all(buf[b_rows.shape[0]:] == 7.0)
            eng.traj_check_release()
            assert eng.lib.isdf_traj_check_get(eng.h, buf.ctypes.data_as(dp), buf.shape[0]) == capi.ISDF_ERR_STATE
        r2 = eng.eval_single(T * 1.05, cm)
        ts = np.zeros(pts.shape[0])
        r3 = eng.eval_single(T, cm, tstar=ts)
        # the kept swept mesh survives
        V2 = np.zeros_like(V); F2 = np.zeros_like(F)
        assert eng.lib.isdf_swept_mesh_get(eng.h, V2.ctypes.data_as(dp), V.shape[0], F2.ctypes.data_as(C.POINTER(C.c_int32)), F.shape[0]) == capi.ISDF_OK
        assert V.shape[0] > 100 and np.array_equal(V2, V) and np.array_equal(F2, F)
        out[with_check] = (r1, r2, r3, ts)
    a, b = out[False], out[True]
    for k in range(3):
        assert a[k][0] == b[k][0] and np.array_equal(a[k][1], b[k][1]) and np.array_equal(a[k][2], b[k][2]), k
    assert np.array_equal(a[3], b[3])


def test_check_argument_errors_on_a_ctx(pkg, product_lib):
    capi, synth = pkg.capi, pkg.synth
    occ, res, T, cm = _world(pkg)
    shape = _shape(pkg, "RoundedCone")
    cfg = synth.default_config(capi.V3_ESDF_TILE, safety_hor=SAFETY)
    eng = pkg.Engine(cfg); eng.set_shape(shape)
    with pytest.raises(pkg.IsdfError) as e:                  # no occupancy grid
        eng.traj_check(T, cm)
    assert e.value.code == capi.ISDF_ERR_INVALID_ARG and "occupancy" in str(e.value)
    eng.set_grid(occ, (0, 0, 0), res, capi.GRID_OCCUPANCY)
    assert eng.traj_check(T, cm)["margin"] == SAFETY         # any variant
    assert eng.traj_check(T, cm, margin=2 * SAFETY + 0.1)["margin"] == 2 * SAFETY + 0.1
    for kw in (dict(margin=2 * SAFETY + 0.1001), dict(mode=2)):
        with pytest.raises(pkg.IsdfError) as e:
            eng.traj_check(T, cm, **kw)
        assert e.value.code == capi.ISDF_ERR_INVALID_ARG
    with pytest.raises(pkg.IsdfError) as e:
        eng.traj_check(T * 100.0, cm)
    assert e.value.code == capi.ISDF_ERR_INVALID_ARG
    with pytest.raises(pkg.IsdfError) as e:
        eng.traj_collide(T * 100.0, cm)
    assert e.value.code == capi.ISDF_ERR_INVALID_ARG
    multi = pkg.Engine(cfg, devices=[0, 0])
    multi.set_shape(shape); multi.set_grid(occ, (0, 0, 0), res, capi.GRID_OCCUPANCY)
    with pytest.raises(pkg.IsdfError) as e:
        multi.traj_check(T, cm)
    assert e.value.code == capi.ISDF_ERR_UNSUPPORTED


def test_device_form_equals_host_form(pkg, product_lib):
    import torch
    capi = pkg.capi
    occ, res, T, cm = _world(pkg)
    eng = _engine(pkg, _shape(pkg, "Box"), occ, res)
    host = eng.traj_check(T, cm, mode=capi.SWEPT_FIELD_CLOSED)
    rows = eng.traj_check_points()
    dT = torch.tensor(T, dtype=torch.float64, device="cuda")
    dC = torch.tensor(np.ascontiguousarray(cm).reshape(-1), dtype=torch.float64, device="cuda")
    dpm = torch.zeros(len(T), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    dev = eng.traj_check_device(len(T), dT.data_ptr(), dC.data_ptr(), mode=capi.SWEPT_FIELD_CLOSED, d_piece_min=dpm.data_ptr())
    assert np.array_equal(_bits(dpm.cpu().numpy()), _bits(host["piece_min"]))
    for k in host:
        if k.endswith("_ms") or k == "piece_min":
            continue
        assert (np.array_equal(_bits(host[k]), _bits(dev[k])) if isinstance(host[k], np.ndarray) else host[k] == dev[k]), k
    assert eng.traj_check_points().tobytes() == rows.tobytes()
    assert eng.traj_check_device(len(T), dT.data_ptr(), dC.data_ptr())["min_voxel"] == eng.traj_check(T, cm)["min_voxel"]


# ---- 6. the map replaced between two checks -----------------------------------------------------------------------------
def test_second_check_follows_a_replaced_map(pkg, product_lib):
    capi = pkg.capi
    occ, res, T, cm = _world(pkg)
    ext = np.array(occ.shape) * res
    eng = _engine(pkg, _shape(pkg, "RoundedCone"), occ, res)

    def cloud(o):
        return ((np.argwhere(o != 0) + 0.5) * res).astype(np.float32)

    occ_b = np.roll(occ, (5, -7, 3), axis=(0, 1, 2))
    reports = []
    for o in (occ, occ_b):
        dims = eng.set_pointcloud(cloud(o), res, sta_threshold=1, bmin=(0, 0, 0), bmax=ext)
        assert tuple(dims) == occ.shape
        got, origin, _ = eng.get_grid(capi.GRID_OCCUPANCY)
        assert np.array_equal(got != 0, o != 0)
        rep = eng.traj_check(T, cm)
        _assert_same(rep, eng.traj_check_points(), _brute(eng, got, origin, res, T, cm, SAFETY, capi.SWEPT_FIELD_PLANNER), "replaced map")
        reports.append(rep)
    assert reports[0]["min_voxel"] != reports[1]["min_voxel"] or reports[0]["qualified"] != reports[1]["qualified"]


# ---- 7. the reference's own demo map ------------------------------------------------------------------------------------
def test_demo_map_with_a_mesh_robot(pkg, product_lib):
    """demo1's point cloud (80 107 points) at its yaml resolution and threshold, robot Lthick, a seeded random trajectory across
    the map (the fixture holds none; no optimiser is run).  Brute force over the occupied voxels of the path's box grown by far_r
    plus one voxel: all candidates lie inside it, and a voxel outside it reads 10 / -1."""
    capi, synth = pkg.capi, pkg.synth
    g = np.load(GOLD)
    res = float(g["CappedCone_yaml_occupancy_resolution"]); sta = int(g["CappedCone_yaml_sta_threshold"])
    safety = float(g["CappedCone_yaml_safety_hor"])
    cfg = synth.default_config(capi.V1_SWEPT, safety_hor=safety)
    eng = pkg.Engine(cfg)
    eng.set_shape(synth.make_mesh_shape(g["Lthick_V"], g["Lthick_F"]))
    eng.set_pointcloud(g["CappedCone_xyz"], res, sta_threshold=sta)
    occ, origin, bmax = eng.get_grid(capi.GRID_OCCUPANCY)
    ext = np.array(occ.shape) * res
    N = 8
    T, Cf = synth.random_trajectory(ext, N, seed=5, piece_T=1.5, margin=3.0, occ=occ, res=res)
    Cf = np.array(Cf); Cf[0::6, :] += origin                # constant terms: into the map's frame
    cm = synth.colmajor(Cf)
    rep = eng.traj_check(T, cm)
    rows = eng.traj_check_points()
    rmax = np.linalg.norm(g["Lthick_V"], axis=1).max()
    assert rep["culled"] == 1 and abs(rep["far_r"] - (rmax + 1.05 * (2 * safety + 0.1))) <= 1e-12
    path = _dense_path(T, cm)
    top = np.array(occ.shape) - 1
    lo = np.clip(np.floor((path.min(0) - rep["far_r"] - origin) / res).astype(int) - 1, 0, top)
    hi = np.clip(np.floor((path.max(0) + rep["far_r"] - origin) / res).astype(int) + 1, 0, top)
    want = _brute(eng, occ, origin, res, T, cm, safety, capi.SWEPT_FIELD_PLANNER, box=(lo, hi))
    assert rep["candidates"] <= len(want["vox"]) and 0 < rep["candidates"] < int((occ != 0).sum())
    _assert_same(rep, rows, want, "demo1 map, Lthick")
    assert rep["qualified"] > 0
