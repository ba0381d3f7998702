"""tests/swept_mesh_reference.py (the swept mesh's extraction rule in numpy) held to first principles - no device.

The reference is what test_gpu_swept_mesh_exact.py compares the extractor's bytes with, so it is checked here against properties
that do not depend on how either is written: directed edges pair off, every triangle faces along the gradient of its tetrahedron's
linear interpolant, vertices sit where that interpolant crosses iso, a sphere comes out closed with the right volume, and the
narrow band loses nothing for a 1-Lipschitz field."""
from fractions import Fraction

import numpy as np
import pytest

import swept_mesh_reference as R


def noise(seed, dims=(9, 7, 5)):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, dims)


def segment_field(dims, eps, origin, seed, r):
    """distance to a random segment inside the lattice's box, minus r: 1-Lipschitz"""
    rng = np.random.default_rng(seed)
    X = R.lattice_xyz(dims, origin, eps)
    lo, hi = X.min(0), X.max(0)
    A = lo + (0.2 + 0.6 * rng.uniform(size=3)) * (hi - lo)
    B = lo + (0.2 + 0.6 * rng.uniform(size=3)) * (hi - lo)
    AB = B - A
    t = np.clip((X - A) @ AB / (AB @ AB), 0.0, 1.0)
    return (np.linalg.norm(X - (A + t[:, None] * AB), axis=1) - r).reshape(dims)


@pytest.fixture(scope="module", params=[0, 1, 2])
def noise_mesh(request):
    f = noise(request.param)
    origin, eps, iso = (0.0, 0.0, 0.0), 0.25, 0.0
    V, F, counts, det = R.extract(f, origin, eps, iso, detail=True)
    return f, origin, eps, iso, V, F, counts, det


def test_noise_reaches_every_tetrahedron_and_pattern(noise_mesh):
    f, origin, eps, iso, V, F, counts, det = noise_mesh
    assert det["pairs"][:, 1:15].sum() == 84                      # 6 tetrahedra x 14 mixed patterns
    assert counts["band_cells"] == 8 * 6 * 4 and counts["n_triangles"] == F.shape[0] > 500 and counts["n_vertices"] == V.shape[0]
    assert len(np.unique(F)) == V.shape[0]                        # every vertex is used


def test_noise_directed_edges_pair_off(noise_mesh):
    f, origin, eps, iso, V, F, counts, det = noise_mesh
    unpaired, multi = R.directed_edge_report(V, F, f.shape, origin, eps)
    assert multi.shape[0] == 0                                    # no directed edge twice: one mis-oriented triangle makes one
    w = R.on_boundary_face(V, f.shape, origin, eps)
    assert unpaired.shape[0] > 0                                  # noise cuts the box
    assert np.all((w[unpaired[:, 0]] & w[unpaired[:, 1]]) != 0)   # ... and only there is an edge without its reverse


def test_noise_triangles_face_the_gradient_of_their_tetrahedron(noise_mesh):
    f, origin, eps, iso, V, F, counts, det = noise_mesh
    nx, ny, nz = f.shape
    paths = np.array(R.tet_paths())
    cell, tet = det["tri_cell"], det["tri_tet"]
    ci, cj, ck = cell // ((ny - 1) * (nz - 1)), (cell // (nz - 1)) % (ny - 1), cell % (nz - 1)
    q = paths[tet]                                                # n x 4 corners
    X = R.CORNER_XYZ[q].astype(float)                             # n x 4 x 3 (cell units: the gradient's direction is what matters)
    val = f[ci[:, None] + R.CORNER_XYZ[q, 0], cj[:, None] + R.CORNER_XYZ[q, 1], ck[:, None] + R.CORNER_XYZ[q, 2]]
    g = np.linalg.solve(X[:, 1:] - X[:, :1], (val[:, 1:] - val[:, :1])[..., None])[..., 0]
    a, b, c = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
    n = np.cross(b - a, c - a)
    assert np.all(np.einsum("ij,ij->i", n, g) > 0)
    # 0, 1 or 2 triangles per tetrahedron by its count of inside corners
    n_in = (val < iso).sum(1)
    per_tet = np.zeros((int(cell.max()) + 1, 6), dtype=int)
    np.add.at(per_tet, (cell, tet), 1)
    assert np.all(per_tet[cell, tet] == np.where(n_in == 2, 2, 1)) and np.all((n_in >= 1) & (n_in <= 3))
    inside = f < iso
    all_in = np.zeros((nx - 1, ny - 1, nz - 1, 6), dtype=int)
    for p, path in enumerate(paths):
        for cnr in path:
            x, y, z = R.CORNER_XYZ[cnr]
            all_in[..., p] += inside[x:nx - 1 + x, y:ny - 1 + y, z:nz - 1 + z]
    want = np.where(all_in == 2, 2, np.where((all_in == 1) | (all_in == 3), 1, 0)).reshape(-1, 6)
    have = np.zeros_like(want)
    have[:per_tet.shape[0]] = per_tet
    assert np.array_equal(have, want)


def test_noise_vertices_sit_where_the_interpolant_crosses_iso(noise_mesh):
    """Every vertex lies on its lattice edge: the axes the edge does not move along carry the node's coordinate exactly, the others
    lie within 4 ulp of node + eps * (iso - f0) / (f1 - f0) evaluated in rational arithmetic - the point where the linear
    interpolant of f along the edge equals iso.  (Subtraction, division, product and sum round once each: under 3 ulp.)"""
    f, origin, eps, iso, V, F, counts, det = noise_mesh
    nx, ny, nz = f.shape
    node, dr = det["edge_node"], det["edge_dir"]
    assert np.all(np.diff(node * 7 + dr) > 0)                     # ascending edge ids
    ijk = np.stack([node // (ny * nz), (node // nz) % ny, node % nz], axis=1)
    off = R.DIR_OFFSETS[dr]
    P0 = np.array(origin) + ijk * eps
    f0 = f[ijk[:, 0], ijk[:, 1], ijk[:, 2]]
    f1 = f[ijk[:, 0] + off[:, 0], ijk[:, 1] + off[:, 1], ijk[:, 2] + off[:, 2]]
    assert np.all((f0 < iso) != (f1 < iso))
    worst = 0.0
    for v in range(V.shape[0]):
        t = (Fraction(iso) - Fraction(f0[v])) / (Fraction(f1[v]) - Fraction(f0[v]))
        assert 0 < t <= 1
        for a in range(3):
            if not off[v, a]:
                assert V[v, a] == P0[v, a]
                continue
            exact = Fraction(P0[v, a]) + Fraction(eps) * t
            err = abs(Fraction(V[v, a]) - exact) / Fraction(np.spacing(abs(V[v, a])))
            worst = max(worst, float(err))
    assert worst <= 4.0, worst


def _closed_stats(V, F):
    E = np.sort(np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]]), axis=1)
    _, cnt = np.unique(E, axis=0, return_counts=True)
    a, b, c = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
    vol = np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0
    return cnt, V.shape[0] - cnt.size + F.shape[0], vol


def test_sphere_is_closed_and_its_volume_converges():
    """|x| - 1 on [-2, 2]^3.  Along a lattice edge (length h <= sqrt(3) eps) the linear interpolant of |x| - 1 is off by at most
    h^2 / 8 / r_min, and a flat triangle (diameter <= sqrt(3) eps) sags by at most as much again: every surface point has
    ||x| - 1| <= delta = 3 eps^2 / 8 * (1 + 1 / (1 - sqrt(3) eps)), so the volume is within 4 pi / 3 ((1 + delta)^3 - 1)."""
    errs = []
    for n in (17, 33):
        eps = 4.0 / (n - 1)
        X = R.lattice_xyz((n, n, n), (-2.0, -2.0, -2.0), eps)
        f = (np.linalg.norm(X, axis=1) - 1.0).reshape(n, n, n)
        V, F, counts = R.extract(f, (-2.0, -2.0, -2.0), eps, 0.0)
        cnt, euler, vol = _closed_stats(V, F)
        unpaired, multi = R.directed_edge_report(V, F, f.shape, (-2.0,) * 3, eps)
        assert np.all(cnt == 2) and euler == 2 and unpaired.shape[0] == 0 and multi.shape[0] == 0
        delta = 3 * eps ** 2 / 8 * (1 + 1 / (1 - np.sqrt(3) * eps))
        assert np.abs(np.linalg.norm(V, axis=1) - 1.0).max() <= delta
        err = abs(vol - 4 * np.pi / 3)
        assert vol > 0 and err <= 4 * np.pi / 3 * ((1 + delta) ** 3 - 1), (vol, err)
        errs.append(err)
    assert errs[1] < errs[0], errs


BAND_DIMS, BAND_EPS, BAND_ORIGIN = (23, 18, 9), 0.25, (0.0, 0.0, 0.0)


@pytest.fixture(scope="module")
def band_case():
    f = segment_field(BAND_DIMS, BAND_EPS, BAND_ORIGIN, seed=6, r=0.6)
    return f, R.extract(f, BAND_ORIGIN, BAND_EPS, 0.0)


@pytest.mark.parametrize("B", [1, 2, 3, 5, 40])
def test_band_extraction_equals_dense_for_a_lipschitz_field(band_case, B):
    f, (Vd, Fd, cd) = band_case
    assert Fd.shape[0] > 300
    fb, n_coarse, n_fine = R.band_field(f, B, 0.0, 1.0, BAND_EPS)
    assert n_coarse == np.prod([-(-(n - 1) // B) + 1 for n in BAND_DIMS])
    assert n_coarse + n_fine == (~np.isnan(fb)).sum() <= f.size
    if B == 1:
        assert n_fine == 0 and n_coarse == f.size
    if B == 40:
        assert n_coarse == 8
    Vb, Fb, cb = R.extract(fb, BAND_ORIGIN, BAND_EPS, 0.0)
    assert Vb.tobytes() == Vd.tobytes() and Fb.tobytes() == Fd.tobytes()
    assert cb["band_cells"] <= cd["band_cells"] and {k: cb[k] for k in cb if k != "band_cells"} == {k: cd[k] for k in cd if k != "band_cells"}
    if B in (2, 3, 5):
        assert 0 < n_fine and cb["band_cells"] < cd["band_cells"]                # a band: some cells are culled


def test_band_with_too_small_a_lipschitz_bound_loses_triangles(band_case):
    """the precondition of the test above: the cull is what keeps the band mesh dense, not an accident of the field"""
    f, (Vd, Fd, cd) = band_case
    fb, _, _ = R.band_field(f, 5, 0.0, 0.05, BAND_EPS)
    Vb, Fb, cb = R.extract(fb, BAND_ORIGIN, BAND_EPS, 0.0)
    assert 0 < cb["n_triangles"] < cd["n_triangles"]


def test_unknown_nodes_open_the_mesh_and_count_unqualified_edges():
    rng = np.random.default_rng(11)
    f = noise(11)
    g = f.copy()
    g[rng.uniform(size=f.shape) < 0.2] = np.nan
    V, F, counts, det = R.extract(g, (0.0, 0.0, 0.0), 0.25, 0.0, detail=True)
    K = R.known_cells(g)
    assert 0 < K.sum() == counts["band_cells"] < K.size
    Vd, Fd, cdense = R.extract(f, (0.0, 0.0, 0.0), 0.25, 0.0)
    # the triangles are the dense mesh's triangles of the known cells, vertex for vertex
    _, _, _, dd = R.extract(f, (0.0, 0.0, 0.0), 0.25, 0.0, detail=True)
    keep = K.ravel()[dd["tri_cell"]]
    assert np.array_equal(V[F].view(np.uint64), Vd[Fd[keep]].view(np.uint64))
    h = f.copy()
    h[f > 0.8] = 10.0
    _, _, ch, dh = R.extract(h, (0.0, 0.0, 0.0), 0.25, 0.5, detail=True)
    ny, nz = f.shape[1:]
    node, off = dh["edge_node"], R.DIR_OFFSETS[dh["edge_dir"]]
    ends = h.ravel()[node], h.ravel()[node + (off[:, 0] * ny + off[:, 1]) * nz + off[:, 2]]
    assert ch["unqualified_edges"] == int(((ends[0] == 10.0) | (ends[1] == 10.0)).sum()) > 0
