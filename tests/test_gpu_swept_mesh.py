"""Swept-volume SDF field (isdf_swept_sdf) and its surface mesh (isdf_swept_mesh_*) on the device.

Field: PLANNER mode is getSDFofSweptVolume as the collision term binds it - pinned point by point to the oracle; CLOSED mode
equals it wherever a point's in-range runs all close before the trajectory's end and is never larger; for a ball it is the
distance to the path minus the radius.  The query leaves the V1 step's state alone.
Mesh: a ball along a gentle curve gives a closed, edge-manifold tube of the right volume on the analytic surface; the narrow band
gives the dense mesh; builds are bitwise reproducible."""
import ctypes as C
import os

import numpy as np
import pytest

from common import make_pair, small_world

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "ref_demo_inputs.npz")
BALL_R = 0.5
SHAPES = {"RoundedCone": ((0.8, 0.3, 1.6), 1.9), "Torus": ((1.2, 0.25), 1.45), "Box": ((1.2, 0.4, 0.3), 1.3)}


def _swept_world(pkg, seed=3, N=6, piece_T=1.5):
    synth = pkg.synth
    occ, esdf, res = small_world(pkg, seed=seed)
    ext = np.array(occ.shape) * res
    T, Cf = synth.random_trajectory(ext, N, seed=seed + 40, piece_T=piece_T, margin=4.0, occ=occ, res=res)
    cm = synth.colmajor(Cf)
    way = Cf.reshape(N, 6, 3)[1:, 0, :]
    pts = synth.constraint_points(occ, (0, 0, 0), res, way, half=4 * res * 1.5)
    return occ, esdf, res, T, cm, pts


def _positions(T, cm, ts):
    """positions at global times ts (column-major 6N x 3 coefficients, ascending powers)"""
    N = len(T)
    C6 = np.asarray(cm).reshape(3, 6 * N)
    starts = np.concatenate([[0.0], np.cumsum(T)[:-1]])
    piece = np.clip(np.searchsorted(starts, ts, side="right") - 1, 0, N - 1)
    tl = ts - starts[piece]
    out = np.zeros((len(ts), 3))
    for a in range(3):
        c = C6[a].reshape(N, 6)[piece]
        out[:, a] = ((((c[:, 5] * tl + c[:, 4]) * tl + c[:, 3]) * tl + c[:, 2]) * tl + c[:, 1]) * tl + c[:, 0]
    return out


def _query_points(T, cm, pts, n_rand=1200, n_far=100, seed=9):
    rng = np.random.default_rng(seed)
    path = _positions(T, cm, np.linspace(0, T.sum(), 400))
    lo, hi = path.min(0) - 2.5, path.max(0) + 2.5
    near = path[rng.integers(0, len(path), n_rand)] + rng.normal(0, 1.0, (n_rand, 3))
    box = lo + rng.uniform(0, 1, (n_rand // 2, 3)) * (hi - lo)
    far = hi + 20.0 + rng.uniform(0, 5, (n_far, 3))
    return np.vstack([pts, near, box, far])


def _check_planner_vs_oracle(eng, o, T, cm, P, check_tstar=True):
    val, ts = eng.swept_sdf(T, cm, P)
    n_int = 0
    for k in range(P.shape[0]):
        s0, t0, _, nr = o.swept_sdf(T, cm, P[k], tstar0=-1.0)
        if s0 == 10.0 and t0 == -1.0:
            assert val[k] == 10.0 and ts[k] == -1.0, (k, val[k], ts[k], nr)
            continue
        n_int += 1
        assert abs(val[k] - s0) <= 1e-9 * max(1.0, abs(s0)), (k, val[k], s0)
        if check_tstar:
            assert abs(ts[k] - t0) <= 2e-5, (k, ts[k], t0)
        else:
            assert ts[k] >= 0.0
    return val, ts, n_int


@pytest.mark.parametrize("shape_name", ["RoundedCone", "Torus", "Box"])
def test_field_planner_matches_oracle(pkg, orc, product_lib, shape_name):
    capi, synth = pkg.capi, pkg.synth
    occ, esdf, res, T, cm, pts = _swept_world(pkg)
    params, R = SHAPES[shape_name]
    shape = synth.make_shape(shape_name, params=params, bound_radius=R)
    cfg = synth.default_config(capi.V3_ESDF_TILE, safety_hor=0.5)        # any variant: the query does not depend on it
    eng, o = make_pair(pkg, orc, cfg, shape)
    P = _query_points(T, cm, pts)
    assert P.shape[0] > 2000
    val, ts, n_int = _check_planner_vs_oracle(eng, o, T, cm, P)
    assert n_int > 500 and (val == 10.0).sum() > 100


def test_field_planner_mesh_robot(pkg, orc, product_lib):
    capi, synth = pkg.capi, pkg.synth
    g = np.load(GOLD)
    occ, esdf, res, T, cm, pts = _swept_world(pkg)
    shape = synth.make_mesh_shape(g["Lthick_V"], g["Lthick_F"])
    cfg = synth.default_config(capi.V1_SWEPT, safety_hor=0.5)
    eng, o = make_pair(pkg, orc, cfg, shape)
    P = _query_points(T, cm, pts, n_rand=500, n_far=50)
    # a tie of the seed rule may pick the other minimiser: values, not t*
    _, _, n_int = _check_planner_vs_oracle(eng, o, T, cm, P, check_tstar=False)
    assert n_int > 200


@pytest.mark.parametrize("shape_name", ["RoundedCone", "Box"])
def test_field_closed_against_planner(pkg, product_lib, shape_name):
    capi, synth = pkg.capi, pkg.synth
    occ, esdf, res, T, cm, pts = _swept_world(pkg)
    params, R = SHAPES[shape_name]
    shape = synth.make_shape(shape_name, params=params, bound_radius=R)
    cfg = synth.default_config(capi.V1_SWEPT, safety_hor=0.5)
    eng = pkg.Engine(cfg); eng.set_shape(shape)
    P = _query_points(T, cm, pts)
    D = T.sum()
    end = _positions(T, cm, np.linspace(D - 0.25, D, 60))
    P = np.vstack([P, end[-1] + np.random.default_rng(2).normal(0, 0.8, (400, 3))])      # points around the final pose
    vp, tp = eng.swept_sdf(T, cm, P, mode=capi.SWEPT_FIELD_PLANNER)
    vc, tc = eng.swept_sdf(T, cm, P, mode=capi.SWEPT_FIELD_CLOSED)
    assert np.all(vc <= vp)
    # sdf >= |p - x| - R: a point farther than R + 2 safety_hor + 0.1 from every pose of the last 0.25 s is out of range at the
    # last coarse samples, so all its runs close before the end
    d_end = np.min(np.linalg.norm(P[:, None, :] - end[None, :, :], axis=2), axis=1)
    closed_before = d_end > R + 2 * 0.5 + 0.1 + 0.05
    assert closed_before.sum() > 1000 and (~closed_before).sum() > 100
    assert np.array_equal(vc[closed_before].view(np.uint64), vp[closed_before].view(np.uint64))
    assert np.array_equal(tc[closed_before].view(np.uint64), tp[closed_before].view(np.uint64))
    # near the end, PLANNER drops the open run: CLOSED finds the end cap
    assert (vc[~closed_before] < vp[~closed_before]).sum() > 50


def _ball_curve(pkg, N=3, piece_T=1.2):
    """a gentle arc (radius 6 m, 100 degrees) - it never comes within 2 r of itself"""
    synth = pkg.synth
    ang = np.linspace(0.0, np.deg2rad(100.0), N + 1)
    pts = np.stack([6.0 * np.cos(ang), 6.0 * np.sin(ang), 0.4 * np.sin(2 * ang)], axis=1) + np.array([10.0, 10.0, 5.0])
    head = np.zeros((3, 3)); head[:, 0] = pts[0]
    tail = np.zeros((3, 3)); tail[:, 0] = pts[-1]
    T = np.full(N, piece_T)
    Cf = synth.minco_coeffs(head, tail, pts[1:-1].T, T)
    return T, synth.colmajor(Cf)


def _ball_engine(pkg, safety_hor=0.5):
    capi, synth = pkg.capi, pkg.synth
    cfg = synth.default_config(capi.V1_SWEPT, safety_hor=safety_hor)
    eng = pkg.Engine(cfg)
    eng.set_shape(synth.make_shape("Ball", params=(BALL_R,), bound_radius=BALL_R))
    return eng


def _curve_tree(T, cm, dt=1e-4):
    from scipy.spatial import cKDTree
    D = T.sum()
    poly = _positions(T, cm, np.append(np.arange(0.0, D, dt), D))
    return poly, cKDTree(poly)


def _dist_to_polyline(poly, tree, X, k=4):
    """distance of X to the polyline through poly (segments around the k nearest samples)"""
    _, idx = tree.query(X, k=k)
    best = np.full(X.shape[0], np.inf)
    for j in range(k):
        for s in (-1, 0):
            a = np.clip(idx[:, j] + s, 0, len(poly) - 2)
            A, B = poly[a], poly[a + 1]
            AB = B - A
            t = np.clip(np.einsum("ij,ij->i", X - A, AB) / np.maximum(np.einsum("ij,ij->i", AB, AB), 1e-300), 0.0, 1.0)
            best = np.minimum(best, np.linalg.norm(X - (A + t[:, None] * AB), axis=1))
    return best


def test_field_closed_ball_is_distance_to_the_path(pkg, product_lib):
    capi = pkg.capi
    T, cm = _ball_curve(pkg)
    eng = _ball_engine(pkg)
    poly, tree = _curve_tree(T, cm)
    rng = np.random.default_rng(4)
    P = poly[rng.integers(0, len(poly), 3000)] + rng.normal(0, 0.7, (3000, 3))
    P = np.vstack([P, poly[0] + rng.normal(0, 0.6, (300, 3)), poly[-1] + rng.normal(0, 0.6, (300, 3))])     # both end caps
    v, ts = eng.swept_sdf(T, cm, P, mode=capi.SWEPT_FIELD_CLOSED)
    q = ts >= 0.0
    assert q.sum() > 2500
    want = _dist_to_polyline(poly, tree, P[q]) - BALL_R
    assert np.abs(v[q] - want).max() <= 1e-5, np.abs(v[q] - want).max()


def test_field_query_leaves_the_v1_step_alone(pkg, product_lib):
    capi, synth = pkg.capi, pkg.synth
    occ, esdf, res, T, cm, pts = _swept_world(pkg)
    params, R = SHAPES["RoundedCone"]
    shape = synth.make_shape("RoundedCone", params=params, bound_radius=R)
    cfg = synth.default_config(capi.V1_SWEPT, safety_hor=0.5)
    P = _query_points(T, cm, pts, n_rand=70000, n_far=10)       # more than one chunk of the query
    Tq, cmq = _ball_curve(pkg)
    out = {}
    for with_query in (False, True):
        eng = pkg.Engine(cfg); eng.set_shape(shape); eng.set_points(pts)
        r1 = eng.eval_single(T, cm)                  # the ctx's own lastTstar
        if with_query:
            eng.swept_sdf(Tq * 1.7, cmq, P, mode=capi.SWEPT_FIELD_CLOSED)
            eng.swept_sdf(T * 0.8, cm, P[:5000], mode=capi.SWEPT_FIELD_PLANNER)
        r2 = eng.eval_single(T * 1.05, cm)
        ts = np.zeros(pts.shape[0])
        r3 = eng.eval_single(T, cm, tstar=ts)
        out[with_query] = (r1, r2, r3, ts)
    a, b = out[False], out[True]
    for k in range(3):
        assert a[k][0] == b[k][0] and np.array_equal(a[k][1], b[k][1]) and np.array_equal(a[k][2], b[k][2]), k
    assert np.array_equal(a[3], b[3])


def test_field_refuses_long_trajectories(pkg, product_lib):
    capi = pkg.capi
    T, cm = _ball_curve(pkg)
    eng = _ball_engine(pkg)
    with pytest.raises(pkg.IsdfError) as e:
        eng.swept_sdf(T * 100.0, cm, np.zeros((4, 3)))
    assert e.value.code == capi.ISDF_ERR_INVALID_ARG
    with pytest.raises(pkg.IsdfError) as e:
        eng.swept_sdf(T, cm, np.zeros((4, 3)), mode=2)
    assert e.value.code == capi.ISDF_ERR_INVALID_ARG


# ---- mesh ------------------------------------------------------------------------------------------------------------
def _edge_counts(F):
    E = np.sort(np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]]), axis=1)
    _, cnt = np.unique(E, axis=0, return_counts=True)
    return cnt


def _signed_volume(V, F):
    a, b, c = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
    return np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0


@pytest.fixture(scope="module")
def ball_meshes(pkg):
    T, cm = _ball_curve(pkg)
    eng = _ball_engine(pkg)
    eps = BALL_R / 10
    dense = eng.swept_mesh(T, cm, eps, band=0)
    band = eng.swept_mesh(T, cm, eps, band=4)
    band2 = eng.swept_mesh(T, cm, eps, band=4)
    planner = eng.swept_mesh(T, cm, eps, band=4, mode=pkg.capi.SWEPT_FIELD_PLANNER)
    return T, cm, eps, eng, dense, band, band2, planner


def test_ball_tube_mesh_is_closed_manifold_on_the_surface(pkg, product_lib, ball_meshes):
    T, cm, eps, eng, dense, band, band2, planner = ball_meshes
    V, F, info = band
    assert info["n_vertices"] == V.shape[0] > 1000 and info["n_triangles"] == F.shape[0]
    assert info["unqualified_edges"] == 0
    assert F.min() >= 0 and F.max() < V.shape[0] and len(np.unique(F)) == V.shape[0]      # every vertex is used
    cnt = _edge_counts(F)
    assert np.all(cnt == 2), np.bincount(cnt)
    assert V.shape[0] - cnt.size + F.shape[0] == 2                                         # Euler characteristic of a sphere
    poly, tree = _curve_tree(T, cm)
    err = np.abs(_dist_to_polyline(poly, tree, V) - BALL_R)
    assert err.max() <= 0.1 * eps, err.max()
    L = np.linalg.norm(np.diff(poly, axis=0), axis=1).sum()
    vol = _signed_volume(V, F)
    want = np.pi * BALL_R ** 2 * L + 4.0 / 3.0 * np.pi * BALL_R ** 3
    assert vol > 0 and abs(vol - want) <= 0.02 * want, (vol, want)
    assert info["field_ms"] > 0 and info["mesh_ms"] > 0


def test_band_mesh_equals_dense_mesh_and_builds_are_reproducible(pkg, product_lib, ball_meshes):
    T, cm, eps, eng, dense, band, band2, planner = ball_meshes
    (Vd, Fd, Id), (Vb, Fb, Ib), (Vb2, Fb2, Ib2) = dense, band, band2
    assert Id["dims"] == Ib["dims"] and Id["origin"] == Ib["origin"]
    assert np.array_equal(Vd.view(np.uint64), Vb.view(np.uint64)) and np.array_equal(Fd, Fb)
    assert Ib["fine_points"] * 5 <= Id["fine_points"] and Ib["coarse_points"] > 0 and Id["coarse_points"] == 0
    assert Id["fine_points"] == Id["dims"][0] * Id["dims"][1] * Id["dims"][2]
    assert Vb.tobytes() == Vb2.tobytes() and Fb.tobytes() == Fb2.tobytes()


@pytest.mark.parametrize("shape_name", ["RoundedCone", "Box"])
def test_band_mesh_equals_dense_mesh_analytic_robots(pkg, product_lib, shape_name):
    capi, synth = pkg.capi, pkg.synth
    occ, esdf, res, T, cm, pts = _swept_world(pkg)
    params, R = SHAPES[shape_name]
    cfg = synth.default_config(capi.V1_SWEPT, safety_hor=0.5)
    eng = pkg.Engine(cfg); eng.set_shape(synth.make_shape(shape_name, params=params, bound_radius=R))
    Vd, Fd, Id = eng.swept_mesh(T, cm, 0.1, band=0)
    Vb, Fb, Ib = eng.swept_mesh(T, cm, 0.1, band=4)
    assert Fd.shape[0] > 1000
    assert np.array_equal(Vd.view(np.uint64), Vb.view(np.uint64)) and np.array_equal(Fd, Fb)
    assert Ib["fine_points"] * 5 <= Id["fine_points"]
    assert np.all(_edge_counts(Fb) == 2) and _signed_volume(Vb, Fb) > 0


def test_mesh_get_refuses_a_short_buffer(pkg, product_lib, ball_meshes):
    capi = pkg.capi
    T, cm, eps, eng, dense, band, band2, planner = ball_meshes
    V, F, info = eng.swept_mesh(T, cm, eps)
    nV, nF = V.shape[0], F.shape[0]
    L = eng.lib
    Vo = np.full((nV + 4, 3), 7.0); Fo = np.full((nF + 4, 3), -7, dtype=np.int32)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    assert L.isdf_swept_mesh_get(eng.h, Vo.ctypes.data_as(dp), nV - 1, Fo.ctypes.data_as(ip), nF) == capi.ISDF_ERR_OVERFLOW
    assert L.isdf_swept_mesh_get(eng.h, Vo.ctypes.data_as(dp), nV, Fo.ctypes.data_as(ip), nF - 1) == capi.ISDF_ERR_OVERFLOW
    assert np.all(Vo == 7.0) and np.all(Fo == -7)
    assert L.isdf_swept_mesh_get(eng.h, Vo.ctypes.data_as(dp), nV, Fo.ctypes.data_as(ip), nF) == capi.ISDF_OK
    assert np.array_equal(Vo[:nV], V) and np.array_equal(Fo[:nF], F) and np.all(Vo[nV:] == 7.0) and np.all(Fo[nF:] == -7)
    eng.swept_mesh_release()
    assert L.isdf_swept_mesh_get(eng.h, Vo.ctypes.data_as(dp), nV, Fo.ctypes.data_as(ip), nF) == capi.ISDF_ERR_STATE


def test_planner_mode_mesh_loses_the_end_cap(pkg, product_lib, ball_meshes):
    """Why CLOSED is the default: in PLANNER mode the points around the final pose read 'outside'."""
    T, cm, eps, eng, dense, band, band2, planner = ball_meshes
    (Vc, Fc, _), (Vp, Fp, _) = band, planner
    end = _positions(T, cm, np.array([T.sum()]))[0]
    near_c = (np.linalg.norm(Vc - end, axis=1) < 2 * BALL_R).sum()
    near_p = (np.linalg.norm(Vp - end, axis=1) < 2 * BALL_R).sum() if Vp.shape[0] else 0
    closed_p = Fp.shape[0] > 0 and np.all(_edge_counts(Fp) == 2)
    assert (not closed_p) or near_p < near_c, (closed_p, near_p, near_c)


def test_mesh_robot_mesh(pkg, product_lib, tmp_path):
    capi, synth = pkg.capi, pkg.synth
    g = np.load(GOLD)
    T, cm = _ball_curve(pkg)
    cfg = synth.default_config(capi.V1_SWEPT, safety_hor=0.6)
    eng = pkg.Engine(cfg); eng.set_shape(synth.make_mesh_shape(g["Lthick_V"], g["Lthick_F"]))
    V, F, info = eng.swept_mesh(T, cm, 0.1)
    assert F.shape[0] > 1000 and np.all(_edge_counts(F) == 2) and _signed_volume(V, F) > 0
    path = str(tmp_path / "swept.obj")
    eng.write_obj(path, V, F)
    V2, F2 = pkg.fixtures.read_obj(path)
    assert np.array_equal(V2, V) and np.array_equal(F2, F)
