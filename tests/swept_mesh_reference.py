"""The swept mesh's extraction rule (include/isdf_accel.h, the swept-mesh block) restated in plain numpy - test
infrastructure, written from the documented rule and held to first principles by test_swept_mesh_reference_host.py.

Lattice: node (i, j, k) has id (i * ny + j) * nz + k and lies at origin + i * eps per axis (product and sum rounded separately).
Inside is f < iso.  A NaN node is "not evaluated"; a cell is known when its eight corners are evaluated.
Cell corners are numbered by their offset bits x | y << 1 | z << 2.  The Kuhn split cuts a cell into the six tetrahedra that are
the monotone lattice paths 0 -> 7, in the order of itertools.permutations of the axes.
Vertices sit on sign-changing lattice edges (lower node, direction +x +y +z +xy +xz +yz +xyz) that lie in a known cell, numbered by
ascending edge id node * 7 + dir, at node + t * (d * eps), t = (iso - f0) / (f1 - f0).  Triangles come by cell (z fastest), then by
tetrahedron, and face towards larger f.
"""
import itertools

import numpy as np

DIR_OFFSETS = np.array([(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)])       # +x +y +z +xy +xz +yz +xyz
CORNER_XYZ = np.array([(c & 1, (c >> 1) & 1, (c >> 2) & 1) for c in range(8)])
_DIR_OF = {tuple(o): d for d, o in enumerate(DIR_OFFSETS)}


def tet_paths():
    """the six tetrahedra of a cell as corner paths 0 -> e_a -> e_a + e_b -> 7, one per permutation (a, b, c) of the axes"""
    return [(0, 1 << a, (1 << a) | (1 << b), 7) for a, b, _ in itertools.permutations(range(3))]


def _det3(u, v, w):
    return int(round(np.linalg.det(np.array([u, v, w], dtype=float))))


def _faces_larger_f(tri, inside_corners, outside_corners):
    """Does the triangle through the midpoints of its three cell edges (corner pairs) face from the inside corners to the outside
    ones?  Integer arithmetic on the unit cell: twice the midpoints, the normal by a cross product, against the direction from
    the inside corners' centroid to the outside corners' (scaled to integers).  The midpoint triangle is the level set of the
    linear field that is -1 on the inside corners and +1 on the outside ones, whose gradient has a positive product with every
    (outside - inside) difference; moving the vertices along their edges never turns the triangle over."""
    M = [CORNER_XYZ[u] + CORNER_XYZ[w] for u, w in tri]
    n = np.cross(M[1] - M[0], M[2] - M[0])
    d = len(inside_corners) * CORNER_XYZ[list(outside_corners)].sum(0) - len(outside_corners) * CORNER_XYZ[list(inside_corners)].sum(0)
    s = int(n @ d)
    assert s != 0
    return s > 0


def tet_triangles(path, inside):
    """The triangles of one tetrahedron: path = its four corners along the lattice path, inside[m] = corner path[m] is inside.
    Returns a list of 0, 1 or 2 triangles, each three cell edges (u, w) as corner pairs.

    Geometry decides which edges carry a vertex (those between an inside and an outside corner) and which way every triangle is
    wound (_faces_larger_f).  What geometry leaves open - which vertex a triangle starts with, and which diagonal splits the quad of
    a two-and-two pattern - is the extractor's stated convention, restated here and ONLY here:
      * the corners are listed so that the tetrahedron is positively oriented, det(q1 - q0, q2 - q0, q3 - q0) > 0, by exchanging
        the two middle corners of the path where it is not;
      * one corner a apart from the other three: the triangle's first edge is a-b with b the first other corner of the listing;
        the other two edges follow in the order that makes it face larger f;
      * two and two: a, b the inside corners and c, d the outside ones, each pair in listing order, c and d exchanged if the
        triangle (ac, ad, bd) would face the wrong way; the quad ac, ad, bd, bc is split along ac - bd into (ac, ad, bd) and
        (ac, bd, bc)."""
    q = list(path)
    X = CORNER_XYZ
    if _det3(X[q[1]] - X[q[0]], X[q[2]] - X[q[0]], X[q[3]] - X[q[0]]) < 0:
        q[1], q[2] = q[2], q[1]
    ins = {path[m] for m in range(4) if inside[m]}
    cin = [c for c in q if c in ins]
    cout = [c for c in q if c not in ins]
    if not cin or not cout:
        return []
    if len(cin) == 1 or len(cout) == 1:
        a = cin[0] if len(cin) == 1 else cout[0]
        b, c, d = [x for x in q if x != a]
        tri = [(a, b), (a, c), (a, d)]
        if not _faces_larger_f(tri, cin, cout):
            tri = [(a, b), (a, d), (a, c)]
        assert _faces_larger_f(tri, cin, cout)
        return [tri]
    (a, b), (c, d) = cin, cout
    if not _faces_larger_f([(a, c), (a, d), (b, d)], cin, cout):
        c, d = d, c
    t0, t1 = [(a, c), (a, d), (b, d)], [(a, c), (b, d), (b, c)]
    assert _faces_larger_f(t0, cin, cout) and _faces_larger_f(t1, cin, cout)
    return [t0, t1]


def _edge_lo_dir(u, w):
    """a cell edge as (lower corner, direction): the lower corner is the one whose offsets are all <= the other's"""
    xu, xw = CORNER_XYZ[u], CORNER_XYZ[w]
    if np.all(xu <= xw):
        lo, hi = u, w
    else:
        assert np.all(xw <= xu)
        lo, hi = w, u
    return lo, _DIR_OF[tuple(CORNER_XYZ[hi] - CORNER_XYZ[lo])]


def _tables():
    """per (tetrahedron, pattern): pattern bit m = corner path[m] inside; up to two triangles of (lower corner, direction) edges"""
    paths = tet_paths()
    valid = np.zeros((6, 16, 2), dtype=bool)
    lo = np.zeros((6, 16, 2, 3), dtype=np.int64)
    dr = np.zeros((6, 16, 2, 3), dtype=np.int64)
    for p, path in enumerate(paths):
        for pat in range(16):
            tris = tet_triangles(path, [(pat >> m) & 1 for m in range(4)])
            for r, tri in enumerate(tris):
                valid[p, pat, r] = True
                for s, (u, w) in enumerate(tri):
                    lo[p, pat, r, s], dr[p, pat, r, s] = _edge_lo_dir(u, w)
    return paths, valid, lo, dr


_PATHS, _TRI_VALID, _TRI_LO, _TRI_DIR = _tables()


def lattice_xyz(dims, origin, eps):
    """node positions in node order (n x 3): origin + i * eps, the product rounded, then the sum"""
    nx, ny, nz = (int(d) for d in dims)
    ax = [np.float64(origin[a]) + np.arange(n, dtype=np.float64) * np.float64(eps) for a, n in enumerate((nx, ny, nz))]
    X, Y, Z = np.meshgrid(*ax, indexing="ij")
    return np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1)


def known_cells(f):
    ok = ~np.isnan(f)
    k = np.ones(tuple(n - 1 for n in f.shape), dtype=bool)
    for c in range(8):
        x, y, z = CORNER_XYZ[c]
        k &= ok[x:f.shape[0] - 1 + x, y:f.shape[1] - 1 + y, z:f.shape[2] - 1 + z]
    return k


def extract(f, origin, eps, iso, detail=False):
    """(V, F, counts) of the field f (nx x ny x nz, NaN = not evaluated); counts: band_cells, n_vertices, n_triangles,
    unqualified_edges.  detail: a fourth dict - edge_node / edge_dir per vertex, tri_cell / tri_tet per triangle, pairs[tet, pattern]
    = that pattern occurred in a known cell."""
    f = np.asarray(f, dtype=np.float64)
    nx, ny, nz = f.shape
    eps = np.float64(eps); iso = np.float64(iso)
    inside = f < iso
    ok = ~np.isnan(f)
    K = known_cells(f)
    Kp = np.pad(K, 1, constant_values=False)         # Kp[c + 1] = K[c], False outside
    ii, jj, kk = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    # ---- vertices: per (node, dir), in edge-id order
    has = np.zeros((nx, ny, nz, 7), dtype=bool)
    unq = 0
    for d, (dx, dy, dz) in enumerate(DIR_OFFSETS):
        sx, sy, sz = nx - dx, ny - dy, nz - dz
        lo = (slice(0, sx), slice(0, sy), slice(0, sz))
        hi = (slice(dx, nx), slice(dy, ny), slice(dz, nz))
        q = ok[lo] & ok[hi] & (inside[lo] != inside[hi])
        # the edge lies in cell c iff c = node on the axes the edge moves along, c in {node - 1, node} on the others
        incell = np.zeros_like(q)
        for s in itertools.product(*[(0,) if o else (0, 1) for o in (dx, dy, dz)]):
            incell |= Kp[1 - s[0]:1 - s[0] + sx, 1 - s[1]:1 - s[1] + sy, 1 - s[2]:1 - s[2] + sz]
        q &= incell
        has[:sx, :sy, :sz, d] = q
        unq += int((q & ((f[lo] == 10.0) | (f[hi] == 10.0))).sum())
    flat = has.reshape(-1)
    vid = np.where(flat, np.cumsum(flat) - 1, -1).reshape(nx * ny * nz, 7)
    e = np.flatnonzero(flat)
    node, dr = e // 7, e % 7
    ni, nj, nk = node // (ny * nz), (node // nz) % ny, node % nz
    off = DIR_OFFSETS[dr]
    f0 = f[ni, nj, nk]
    f1 = f[ni + off[:, 0], nj + off[:, 1], nk + off[:, 2]]
    with np.errstate(all="ignore"):
        t = (iso - f0) / (f1 - f0)
        V = np.empty((e.size, 3))
        for a, idx in enumerate((ni, nj, nk)):
            p = np.float64(origin[a]) + idx.astype(np.float64) * eps
            V[:, a] = p + t * (off[:, a].astype(np.float64) * eps)
    # ---- triangles: per (cell, tetrahedron, triangle), cells z fastest
    ex, ey, ez = nx - 1, ny - 1, nz - 1
    ci, cj, ck = ii[:ex, :ey, :ez].ravel(), jj[:ex, :ey, :ez].ravel(), kk[:ex, :ey, :ez].ravel()
    Kf = K.ravel()
    n_cells = Kf.size
    tri = np.full((n_cells, 6, 2, 3), -1, dtype=np.int64)
    tri_ok = np.zeros((n_cells, 6, 2), dtype=bool)
    pairs = np.zeros((6, 16), dtype=bool)
    for p, path in enumerate(_PATHS):
        pat = np.zeros(n_cells, dtype=np.int64)
        for m, c in enumerate(path):
            x, y, z = CORNER_XYZ[c]
            pat |= inside[ci + x, cj + y, ck + z].astype(np.int64) << m
        pairs[p, np.unique(pat[Kf])] = True
        tri_ok[:, p, :] = _TRI_VALID[p][pat] & Kf[:, None]
        lo = _TRI_LO[p][pat]                          # n_cells x 2 x 3 lower corners
        lx, ly, lz = CORNER_XYZ[lo, 0], CORNER_XYZ[lo, 1], CORNER_XYZ[lo, 2]
        nid = ((ci[:, None, None] + lx) * ny + (cj[:, None, None] + ly)) * nz + (ck[:, None, None] + lz)
        tri[:, p] = vid[nid, _TRI_DIR[p][pat]]
    F = tri[tri_ok]
    assert F.size == 0 or F.min() >= 0, "a triangle of a known cell uses an edge without a vertex"
    counts = {"band_cells": int(Kf.sum()), "n_vertices": int(e.size), "n_triangles": int(F.shape[0]), "unqualified_edges": unq}
    F = F.astype(np.int32).reshape(-1, 3)
    if not detail:
        return V, F, counts
    cell_of, tet_of, _ = np.nonzero(tri_ok)
    return V, F, counts, {"edge_node": node, "edge_dir": dr, "tri_cell": cell_of, "tri_tet": tet_of, "pairs": pairs}


# ---- the narrow band ---------------------------------------------------------------------------------------------------
def _coarse_axis(n, B):
    """every B-th fine coordinate of an axis, the last one always included"""
    return np.unique(np.append(np.arange(0, n - 1, B), n - 1))


def band_nodes(dims, B):
    """ids of the coarse nodes, ascending"""
    nx, ny, nz = (int(d) for d in dims)
    cx, cy, cz = (_coarse_axis(n, B) for n in (nx, ny, nz))
    return np.sort(((cx[:, None, None] * ny + cy[None, :, None]) * nz + cz[None, None, :]).ravel())


def band_refine(f_coarse, dims, B, iso, L, eps, unqualified=None):
    """f_coarse: the field on the coarse lattice (one value per coarse node, axes as _coarse_axis lists them).  A coarse cell is
    refined when its corners change sign about iso or all lie within L * sqrt(3) * B * eps of it; a corner that reads 10 (no
    qualifying interval) counts as the value `unqualified` (the qualification radius 2 safety_hor + 0.1) in the second test.
    Returns (refined, fine node ids): a fine node is flagged if any coarse cell whose closed span contains it is refined; coarse
    nodes are never flagged."""
    nx, ny, nz = (int(d) for d in dims)
    axes = [_coarse_axis(n, B) for n in (nx, ny, nz)]
    f_coarse = np.asarray(f_coarse, dtype=np.float64)
    assert f_coarse.shape == tuple(a.size for a in axes)
    thr = np.float64(L) * np.sqrt(np.float64(3.0)) * np.float64(B) * np.float64(eps)
    sh = tuple(a.size - 1 for a in axes)
    corners = np.stack([f_coarse[x:sh[0] + x, y:sh[1] + y, z:sh[2] + z] for x, y, z in CORNER_XYZ])
    ins = corners < iso
    mixed = ins.any(0) & (~ins).any(0)
    dist = corners if unqualified is None else np.where(corners == 10.0, np.float64(unqualified), corners)
    near = (np.abs(dist - iso) <= thr).all(0)
    refined = mixed | near
    flag = np.zeros((nx, ny, nz), dtype=bool)
    for a, b, c in zip(*np.nonzero(refined)):
        flag[axes[0][a]:axes[0][a + 1] + 1, axes[1][b]:axes[1][b + 1] + 1, axes[2][c]:axes[2][c + 1] + 1] = True
    flag[np.ix_(*axes)] = False
    return refined, np.flatnonzero(flag.ravel())


def band_field(f, B, iso, L, eps, unqualified=None):
    """the field as a band build leaves it: f on the coarse nodes and the flagged fine nodes, NaN elsewhere; and (coarse, fine)"""
    dims = f.shape
    axes = [_coarse_axis(n, B) for n in dims]
    coarse = band_nodes(dims, B)
    _, fine = band_refine(f[np.ix_(*axes)], dims, B, iso, L, eps, unqualified)
    out = np.full(f.size, np.nan)
    out[coarse] = f.ravel()[coarse]
    out[fine] = f.ravel()[fine]
    return out.reshape(dims), coarse.size, fine.size


# ---- what the tests share ------------------------------------------------------------------------------------------------
def directed_edge_report(V, F, dims, origin, eps):
    """(unpaired, multi): unpaired = directed edges (u, w) of F whose reverse does not occur; multi = directed edges that occur more
    than once.  Used with on_boundary()."""
    E = np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]]).astype(np.int64)
    nV = max(int(V.shape[0]), 1)
    key = E[:, 0] * nV + E[:, 1]
    rev = E[:, 1] * nV + E[:, 0]
    uniq, cnt = np.unique(key, return_counts=True)
    multi = E[np.isin(key, uniq[cnt > 1])]
    unpaired = E[~np.isin(rev, uniq)]
    return unpaired, multi


def on_boundary_face(P, dims, origin, eps):
    """per point: the set of boundary faces of the lattice box it lies in, as a 6-bit word (exact: boundary vertices sit on
    boundary edges, whose fixed coordinates are the box's own doubles)"""
    w = np.zeros(P.shape[0], dtype=np.int64)
    for a in range(3):
        lo = np.float64(origin[a])
        hi = np.float64(origin[a]) + np.float64(dims[a] - 1) * np.float64(eps)
        w |= (P[:, a] == lo).astype(np.int64) << (2 * a)
        w |= (P[:, a] == hi).astype(np.int64) << (2 * a + 1)
    return w
