"""The swept mesh's extractor held to tests/swept_mesh_reference.py byte for byte (test_swept_mesh_reference_host.py holds that
reference to first principles).

Extractor alone (X1-X6): Engine.lattice_mesh on fields that drive it into its corners - every (tetrahedron, pattern) pair, unknown
nodes, ties and signed zeros, thin and ragged lattices, many blocks, empty meshes.
Whole pipeline (P1-P6): isdf_swept_mesh_build for a ball on a two-piece trajectory against the same rule applied to
Engine.swept_sdf(mode=CLOSED) at the lattice's nodes: dense, every band bookkeeping path, boxes that cut the tube, empty boxes, an
unaligned lattice and unqualified edges."""
import ctypes as C

import numpy as np
import pytest

import swept_mesh_reference as R

pytestmark = pytest.mark.gpu

COUNTERS = ("band_cells", "n_vertices", "n_triangles", "unqualified_edges")
UNALIGNED = ((0.3, -1.7, 2.05), 0.1)              # origin, eps: no power of two - node = origin + i * eps rounds twice


def noise(seed, dims):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, dims)


@pytest.fixture(scope="module")
def bare(pkg, product_lib):
    """a ctx without shape, grid or trajectory"""
    return pkg.Engine(pkg.synth.default_config(pkg.capi.V1_SWEPT))


def assert_same(got, want, what=""):
    (V, F, info), (Vr, Fr, cr) = got, want
    assert {k: info[k] for k in COUNTERS} == cr, what
    assert V.shape == Vr.shape and F.shape == Fr.shape and F.dtype == np.int32, what
    assert F.tobytes() == Fr.tobytes(), (what, int((F != Fr).any(1).sum()), "triangles differ")
    assert V.tobytes() == Vr.tobytes(), (what, int((V.view(np.uint64) != Vr.view(np.uint64)).sum()), "coordinates differ of", V.size)


def lattice_case(eng, f, origin, eps, iso, what=""):
    got = eng.lattice_mesh(f, origin, eps, iso)
    info = got[2]
    assert info["dims"] == list(f.shape) and info["origin"] == list(origin) and info["eps"] == eps, what
    assert info["coarse_points"] == 0 and info["fine_points"] == 0 and info["field_ms"] == 0 and info["mesh_ms"] > 0, what
    want = R.extract(f, origin, eps, iso, detail=True)
    assert_same(got, want[:3], what)
    return got, want


# ---- extractor alone ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_x1_noise_every_tetrahedron_and_pattern(bare, seed):
    f = noise(seed, (9, 7, 5))
    _, want = lattice_case(bare, f, (0.0, 0.0, 0.0), 0.25, 0.0)
    assert want[3]["pairs"][:, 1:15].sum() == 84
    assert want[2]["n_triangles"] > 500


def _edge_cell_census(f, iso):
    """per sign-changing edge with both ends evaluated: (cells holding it whose corners are all evaluated, those with a NaN corner)
    - plain loops over nodes, directions and cells"""
    nx, ny, nz = f.shape
    K = R.known_cells(f)
    out = []
    for i in range(nx):
        for j in range(ny):
            for k in range(nz):
                for dx, dy, dz in R.DIR_OFFSETS:
                    a, b, c = i + dx, j + dy, k + dz
                    if a >= nx or b >= ny or c >= nz or np.isnan(f[i, j, k]) or np.isnan(f[a, b, c]):
                        continue
                    if (f[i, j, k] < iso) == (f[a, b, c] < iso):
                        continue
                    n_known = n_unknown = 0
                    for ci in range(max(a - 1, 0), min(i, nx - 2) + 1):
                        for cj in range(max(b - 1, 0), min(j, ny - 2) + 1):
                            for ck in range(max(c - 1, 0), min(k, nz - 2) + 1):
                                if K[ci, cj, ck]:
                                    n_known += 1
                                else:
                                    n_unknown += 1
                    out.append((n_known, n_unknown))
    return np.array(out)


@pytest.mark.parametrize("seed", [3, 4])
def test_x2_unknown_nodes(bare, seed):
    rng = np.random.default_rng(seed)
    f = noise(seed, (9, 7, 5))
    f[rng.uniform(size=f.shape) < 0.2] = np.nan
    census = _edge_cell_census(f, 0.0)
    K = R.known_cells(f)
    assert 0 < K.sum() < K.size
    assert (census[:, 0] == 0).sum() > 0                                   # sign changes in no known cell: no vertex
    assert ((census[:, 0] > 0) & (census[:, 1] > 0)).sum() > 0             # in a known cell and next to an unknown one: a vertex
    _, want = lattice_case(bare, f, UNALIGNED[0], UNALIGNED[1], 0.0)
    assert want[2]["n_vertices"] == (census[:, 0] > 0).sum() > 0


@pytest.mark.parametrize("iso", [0.0, -0.0, -0.3])
def test_x3_ties_and_signed_zeros(bare, iso):
    rng = np.random.default_rng(5)
    f = noise(5, (9, 7, 5))
    u = rng.uniform(size=f.shape)
    f[u < 0.05] = iso
    f[(u >= 0.05) & (u < 0.07)] = -0.0
    assert (f == iso).sum() >= 10 and np.signbit(f[f == 0.0]).sum() >= 3
    (V, F, info), want = lattice_case(bare, f, UNALIGNED[0], UNALIGNED[1], iso)
    assert info["n_triangles"] > 300


def test_x3_unqualified_edges(bare):
    rng = np.random.default_rng(6)
    f = noise(6, (9, 7, 5))
    f[rng.uniform(size=f.shape) < 0.03] = 10.0
    assert (f == 10.0).sum() >= 3
    (V, F, info), want = lattice_case(bare, f, UNALIGNED[0], UNALIGNED[1], 0.5)
    assert info["unqualified_edges"] > 0


@pytest.mark.parametrize("dims", [(2, 2, 2), (2, 2, 66), (66, 2, 2), (2, 258, 2), (5, 5, 14)])
def test_x4_thin_and_ragged_lattices(bare, dims):
    """a single cell; 65 and 257 cells in a row (one past a wavefront, one past a 256-thread block); a partial last wavefront"""
    for seed in (7, 8):
        f = noise(seed, dims)
        (V, F, info), _ = lattice_case(bare, f, UNALIGNED[0], UNALIGNED[1], 0.0, (dims, seed))
        assert info["band_cells"] == (dims[0] - 1) * (dims[1] - 1) * (dims[2] - 1)
        assert info["n_triangles"] > 0 or dims == (2, 2, 2)
    if dims == (2, 2, 2):
        f = np.ones(dims); f[0, 0, 0] = -1.0                    # the lone inside corner of every tetrahedron: six triangles
        (V, F, info), _ = lattice_case(bare, f, UNALIGNED[0], UNALIGNED[1], 0.0)
        assert info["n_triangles"] == 6 and info["n_vertices"] == 7


def test_x5_many_blocks(bare):
    f = noise(9, (41, 41, 41))
    (V, F, info), _ = lattice_case(bare, f, (0.0, 0.0, 0.0), 0.25, 0.0)
    assert info["n_triangles"] >= 100000 and info["band_cells"] == 40 ** 3


def test_x6_kept_mesh_behaviour(pkg, bare):
    capi, L = pkg.capi, bare.lib
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    nan = np.full((5, 4, 3), np.nan)
    for f, cells in ((np.ones((5, 4, 3)), 24), (nan, 0)):
        (V, F, info), _ = lattice_case(bare, f, UNALIGNED[0], UNALIGNED[1], 0.0)
        assert V.shape == (0, 3) and F.shape == (0, 3) and info["band_cells"] == cells
        assert L.isdf_swept_mesh_get(bare.h, None, 0, None, 0) == capi.ISDF_OK
    (V, F, info), _ = lattice_case(bare, noise(10, (5, 4, 3)), UNALIGNED[0], UNALIGNED[1], 0.0)
    assert F.shape[0] > 0
    Vo = np.zeros_like(V); Fo = np.zeros_like(F)
    assert L.isdf_swept_mesh_get(bare.h, Vo.ctypes.data_as(dp), V.shape[0], Fo.ctypes.data_as(ip), F.shape[0]) == capi.ISDF_OK
    assert Vo.tobytes() == V.tobytes() and Fo.tobytes() == F.tobytes()
    bare.swept_mesh_release()
    assert L.isdf_swept_mesh_get(bare.h, Vo.ctypes.data_as(dp), V.shape[0], Fo.ctypes.data_as(ip), F.shape[0]) == capi.ISDF_ERR_STATE
    with pytest.raises(pkg.IsdfError) as e:
        bare.lattice_mesh(np.zeros((1, 4, 4)), (0, 0, 0), 0.1)
    assert e.value.code == capi.ISDF_ERR_INVALID_ARG


# ---- whole pipeline ----------------------------------------------------------------------------------------------------
BALL_R, EPS = 0.5, 0.125
UNQ = 2 * 0.5 + 0.1                                       # the qualification radius 2 safety_hor + 0.1 of _engine()'s default
BMIN = np.array([-1.0, 2.5, 0.375])                       # multiples of EPS: every node coordinate is exact
P1_DIMS = (33, 26, 19)
# about 2 m, nearly level: the tube's underside dips 0.02 - 0.04 m below the coarse plane k = 5 of a band of 5 (z = 0.625 above
# BMIN) in a strip that holds fine nodes and no coarse one - what a band with too small a Lipschitz bound loses
WAY = np.array([[1.0, 1.5, 1.1], [2.0, 1.62, 1.11], [3.0, 1.52, 1.12]]) + BMIN


def _trajectory(pkg, shift=(0.0, 0.0, 0.0)):
    synth = pkg.synth
    way = WAY + np.asarray(shift)
    head = np.zeros((3, 3)); head[:, 0] = way[0]
    tail = np.zeros((3, 3)); tail[:, 0] = way[-1]
    T = np.array([1.0, 1.0])
    return T, synth.colmajor(synth.minco_coeffs(head, tail, way[1:-1].T, T))


def _positions(T, cm, ts):
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


def _engine(pkg, shape="Ball", safety_hor=0.5):
    capi, synth = pkg.capi, pkg.synth
    eng = pkg.Engine(synth.default_config(capi.V1_SWEPT, safety_hor=safety_hor))
    if shape == "Ball":
        eng.set_shape(synth.make_shape("Ball", params=(BALL_R,), bound_radius=BALL_R))
    else:
        eng.set_shape(synth.make_shape("Box", params=(1.2, 0.4, 0.3), bound_radius=1.3))
    return eng


def _bbox(dims, bmin=BMIN, eps=EPS):
    return tuple(bmin), tuple(np.asarray(bmin) + (np.asarray(dims) - 1) * eps)


def _field(pkg, eng, T, cm, info):
    """the CLOSED field at the nodes of the lattice a build reported"""
    dims, origin, eps = info["dims"], info["origin"], info["eps"]
    val, _ = eng.swept_sdf(T, cm, R.lattice_xyz(dims, origin, eps), mode=pkg.capi.SWEPT_FIELD_CLOSED)
    return val.reshape(dims)


@pytest.fixture(scope="module")
def p1(pkg, product_lib):
    T, cm = _trajectory(pkg)
    eng = _engine(pkg)
    got = eng.swept_mesh(T, cm, EPS, band=0, bbox=_bbox(P1_DIMS))
    info = got[2]
    assert info["dims"] == list(P1_DIMS) and info["origin"] == list(BMIN) and info["eps"] == EPS
    f = _field(pkg, eng, T, cm, info)
    return T, cm, eng, got, f


def test_p1_dense(pkg, p1):
    T, cm, eng, got, f = p1
    # the stand-in dist(path) - R reaches every (tetrahedron, pattern) pair on this lattice; so must the device's field
    path = _positions(T, cm, np.linspace(0.0, T.sum(), 801))
    X = R.lattice_xyz(P1_DIMS, BMIN, EPS)
    d = np.full(X.shape[0], np.inf)
    for s in range(0, path.shape[0], 100):
        d = np.minimum(d, np.linalg.norm(X[:, None, :] - path[None, s:s + 100, :], axis=2).min(1))
    stand_in = (d - BALL_R).reshape(P1_DIMS)
    assert R.extract(stand_in, BMIN, EPS, 0.0, detail=True)[3]["pairs"][:, 1:15].sum() == 84
    want = R.extract(f, BMIN, EPS, 0.0, detail=True)
    assert want[3]["pairs"][:, 1:15].sum() == 84
    info = got[2]
    assert info["coarse_points"] == 0 and info["fine_points"] == f.size and info["unqualified_edges"] == 0
    assert info["n_triangles"] > 2000
    assert_same(got, want[:3])
    unpaired, multi = R.directed_edge_report(got[0], got[1], P1_DIMS, BMIN, EPS)
    assert unpaired.shape[0] == 0 and multi.shape[0] == 0                 # the box holds the whole tube: closed


@pytest.mark.parametrize("B", [1, 2, 3, 5, 40])
def test_p2_bands(pkg, p1, B):
    T, cm, eng, dense, f = p1
    got = eng.swept_mesh(T, cm, EPS, band=B, bbox=_bbox(P1_DIMS))
    fb, n_coarse, n_fine = R.band_field(f, B, 0.0, 1.0, EPS, UNQ)
    info = got[2]
    assert (info["coarse_points"], info["fine_points"]) == (n_coarse, n_fine)
    want = R.extract(fb, BMIN, EPS, 0.0)
    assert_same(got, want)
    assert got[0].tobytes() == dense[0].tobytes() and got[1].tobytes() == dense[1].tobytes()
    if B == 1:
        assert n_fine == 0 and n_coarse == f.size
    elif B == 40:                                           # one coarse cell, its corners all without an interval: refined
        assert n_coarse == 8 and n_fine == f.size - 8 and np.all(f[::32, ::25, ::18] == 10.0)
    else:
        assert 0 < n_fine < f.size - n_coarse and info["band_cells"] < dense[2]["band_cells"]


def test_p2_band_with_a_small_lipschitz_bound(pkg, p1):
    T, cm, eng, dense, f = p1
    got = eng.swept_mesh(T, cm, EPS, band=5, bbox=_bbox(P1_DIMS), lipschitz=0.05)
    fb, n_coarse, n_fine = R.band_field(f, 5, 0.0, 0.05, EPS, UNQ)
    assert (got[2]["coarse_points"], got[2]["fine_points"]) == (n_coarse, n_fine)
    assert_same(got, R.extract(fb, BMIN, EPS, 0.0))
    assert got[1].tobytes() != dense[1].tobytes() and 0 < got[2]["n_triangles"] < dense[2]["n_triangles"]


@pytest.mark.parametrize("dims, bmin", [((17, 26, 19), BMIN), ((33, 26, 2), BMIN + np.array([0.0, 0.0, 1.0]))])
def test_p3_boxes_that_cut_the_tube(pkg, p1, dims, bmin):
    T, cm, eng, dense, f = p1
    lo, hi = _bbox(dims, bmin)
    if dims[2] == 2:
        hi = (hi[0], hi[1], lo[2] + 0.1)                    # bmax - bmin < eps: two nodes along z all the same
    for band in (0, 4):
        got = eng.swept_mesh(T, cm, EPS, band=band, bbox=(lo, hi))
        info = got[2]
        assert info["dims"] == list(dims) and info["origin"] == list(bmin)
        fc = _field(pkg, eng, T, cm, info)
        if band:
            fc, n_coarse, n_fine = R.band_field(fc, band, 0.0, 1.0, EPS, UNQ)
            assert (info["coarse_points"], info["fine_points"]) == (n_coarse, n_fine)
        assert_same(got, R.extract(fc, bmin, EPS, 0.0), (dims, band))
        V, F = got[0], got[1]
        assert F.shape[0] > 200
        unpaired, multi = R.directed_edge_report(V, F, dims, bmin, EPS)
        w = R.on_boundary_face(V, dims, bmin, EPS)
        assert multi.shape[0] == 0 and unpaired.shape[0] > 0
        assert np.all((w[unpaired[:, 0]] & w[unpaired[:, 1]]) != 0)


@pytest.mark.parametrize("band", [4, 0])
def test_p4_empty_box(pkg, p1, band):
    T, cm, eng, dense, f = p1
    bmin = BMIN + 10.0
    V, F, info = eng.swept_mesh(T, cm, EPS, band=band, bbox=_bbox((14, 11, 7), bmin))
    assert info["dims"] == [14, 11, 7]
    assert V.shape == (0, 3) and F.shape == (0, 3) and info["n_vertices"] == 0 and info["n_triangles"] == 0
    if band:
        assert info["fine_points"] == 0 and info["coarse_points"] == len(R.band_nodes((14, 11, 7), band)) and info["band_cells"] == 0
    else:
        assert info["fine_points"] == 14 * 11 * 7 and info["band_cells"] == 13 * 10 * 6
    assert eng.lib.isdf_swept_mesh_get(eng.h, None, 0, None, 0) == pkg.capi.ISDF_OK


def test_p5_unaligned_lattice(pkg, product_lib):
    """eps = 0.1 and the derived box: origin = floor(lo / eps) * eps, nodes at origin + i * eps rounded twice.  No node's value lies
    within 1e-6 of iso, so a last-place difference in a coordinate cannot change a sign: it changes vertex bytes only."""
    T, cm = _trajectory(pkg, shift=(0.0137, 0.0291, 0.0173))      # off the lattice: the box's faces at rest pass through no node
    eng = _engine(pkg, "Box")
    for band in (0, 4):
        got = eng.swept_mesh(T, cm, 0.1, band=band)
        info = got[2]
        f = _field(pkg, eng, T, cm, info)
        assert np.abs(f).min() > 1e-6
        if band:
            f, n_coarse, n_fine = R.band_field(f, band, 0.0, 1.0, 0.1, UNQ)
            assert (info["coarse_points"], info["fine_points"]) == (n_coarse, n_fine)
        assert info["n_triangles"] > 5000
        assert_same(got, R.extract(f, info["origin"], 0.1, 0.0), band)


def test_p6_unqualified_edges(pkg, product_lib):
    """iso above the qualification radius 2 safety_hor + 0.1 = 0.5: the level set runs between evaluated values and 10s"""
    T, cm = _trajectory(pkg)
    eng = _engine(pkg, safety_hor=0.2)
    got = eng.swept_mesh(T, cm, EPS, iso=0.9, band=0, bbox=_bbox(P1_DIMS))
    info = got[2]
    f = _field(pkg, eng, T, cm, info)
    assert (f == 10.0).any()
    want = R.extract(f, BMIN, EPS, 0.9)
    assert info["unqualified_edges"] > 0 and info["unqualified_edges"] == want[2]["unqualified_edges"]
    assert_same(got, want)
