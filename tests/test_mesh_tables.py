"""The mesh kind's device tables as the host builds them (csrc/mesh_tables.hpp): the child-major (node, child) records, the flat
slot blob of a small mesh and the index-paired "closed" test, on the meshes of tests/test_fwn_host.py.  Exact assertions (the
outward-rounded boxes: to the one float ulp the rounding may cost).  CPU only."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_fwn_host import _meshes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
dp = C.POINTER(C.c_double)
Q_REC, Q_TRI, FLAT_SLOTS, FLAT_LEVELS = 40, 10, 64, 8        # csrc/dev_shapes.hpp MESH_Q_REC, MESH_Q_TRI, MESH_FLAT_SLOTS, MESH_FLAT_LEVELS


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("mesh_tables") / "libmesh_tables_shim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wno-unknown-pragmas",
                           "-I", os.path.join(ROOT, "implicit-sdf-planner_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "mesh_tables_shim.cpp"), "-o", out])
    L = C.CDLL(out)
    L.shim_mt_build.restype = C.c_void_p
    return L


class Tables:
    def __init__(self, shim, V, F):
        self.shim = shim
        self.V = np.ascontiguousarray(V, dtype=np.float64); self.F = np.ascontiguousarray(F, dtype=np.int32)
        self.h = C.c_void_p(shim.shim_mt_build(self.V.ctypes.data_as(dp), self.V.shape[0], self.F.ctypes.data_as(C.c_void_p), self.F.shape[0]))
        n = self.n = shim.shim_mt_num_nodes(self.h)
        self.child = np.zeros((n, 4), dtype=np.int32); self.box = np.zeros((n, 92), dtype=np.float32)
        self.boxq = np.zeros((n, 4, Q_REC), dtype=np.float32); self.triq = np.zeros((n, 4, Q_TRI), dtype=np.float64)
        shim.shim_mt_dump(self.h, *(a.ctypes.data_as(C.c_void_p) for a in (self.child, self.box, self.boxq, self.triq)))
        self.tri = self.V[self.F].reshape(-1, 9)              # nine fp64 coordinates per face

    def blob(self, max_slots=FLAT_SLOTS, max_levels=FLAT_LEVELS, root=0):
        size = self.shim.shim_mt_blob(self.h, root, max_slots, max_levels, None, 0)
        out = np.zeros(size, dtype=np.int32)
        if size:
            assert self.shim.shim_mt_blob(self.h, root, max_slots, max_levels, out.ctypes.data_as(C.c_void_p), size) == size
        return out

    def levels(self):
        """(number of non-empty (node, child) pairs, number of levels) of the hierarchy, breadth first from the root"""
        level = {0: 0}; order = [0]
        for nd in order:
            for ci in self.child[nd]:
                if ci < -1 and int(ci & 0x7fffffff) not in level:
                    level[int(ci & 0x7fffffff)] = level[nd] + 1; order.append(int(ci & 0x7fffffff))
        assert len(order) == self.n                             # every node hangs below the root
        return int((self.child != -1).sum()), max(level.values()) + 1

    def close(self):
        self.shim.shim_mt_destroy(self.h)


@pytest.fixture(scope="module")
def tables(pkg, shim):
    out = {name: Tables(shim, V, F) for name, (V, F) in _meshes(pkg).items()}
    yield out
    for t in out.values():
        t.close()


def _faces_below(t):
    """per node, the faces of each of its four children (memoised like the product's node_boxes, but as index lists)"""
    memo = {}

    def node(nd):
        if nd not in memo:
            memo[nd] = [[] if ci == -1 else ([int(ci)] if ci >= 0 else sum(node(int(ci & 0x7fffffff)), [])) for ci in t.child[nd]]
        return memo[nd]
    return [node(nd) for nd in range(t.n)]


def test_child_major_records(tables):
    f32 = np.float32
    for name, t in tables.items():
        below = _faces_below(t)
        bits = t.boxq.view(np.uint32)
        for nd in range(t.n):
            for ch in range(4):
                rq, ci = t.boxq[nd, ch], int(t.child[nd, ch])
                # floats 0-22: the child's column of the hierarchy's node record; word 23: the child word - bit for bit
                assert np.array_equal(bits[nd, ch, :23], t.box[nd, ch:92:4].view(np.uint32)), (name, nd, ch)
                assert bits[nd, ch, 23] == np.uint32(ci & 0xffffffff), (name, nd, ch)
                if ci >= 0:                                     # a triangle child carries its nine floats and nine doubles
                    assert np.array_equal(rq[24:33], t.tri[ci].astype(f32)), (name, nd, ch)
                    assert np.array_equal(t.triq[nd, ch, :9].view(np.uint64), t.tri[ci].view(np.uint64)), (name, nd, ch)
                lo, hi = rq[34:37], rq[37:40]
                if ci == -1:                                    # an empty child: an empty box
                    assert (lo > hi).all(), (name, nd, ch)
                    continue
                # floats 34-39 contain the fp64 extent of the child's triangles, and no more than the rounding to float costs:
                # lo is the largest float <= min, hi the smallest float >= max
                pts = t.tri[below[nd][ch]].reshape(-1, 3)
                mn, mx = pts.min(axis=0), pts.max(axis=0)
                assert (lo.astype(np.float64) <= mn).all() and (hi.astype(np.float64) >= mx).all(), (name, nd, ch, lo, mn, hi, mx)
                assert (np.nextafter(lo, f32(np.inf)).astype(np.float64) > mn).all(), (name, nd, ch, lo, mn)
                assert (np.nextafter(hi, f32(-np.inf)).astype(np.float64) < mx).all(), (name, nd, ch, hi, mx)


def test_flat_blob(tables):
    qualified = 0
    for name, t in tables.items():
        n_pairs, n_levels = t.levels()
        flat = t.blob()
        # more than 64 slots, or more than 8 levels: no blob
        assert (flat.size > 0) == (n_pairs <= FLAT_SLOTS and n_levels <= FLAT_LEVELS), (name, n_pairs, n_levels, flat.size)
        if not flat.size:
            continue
        qualified += 1
        nF = t.F.shape[0]
        lvl_begin, step_begin = flat[0:9], flat[9:18]
        n_tris, ns, nl, size, rec_off, trec_off = (int(v) for v in flat[18:24])
        assert (size, size % 4, rec_off % 4, trec_off % 4) == (flat.size, 0, 0, 0), name
        assert (n_tris, ns, nl) == (nF, n_pairs, n_levels), name
        nn = int(step_begin[8])
        assert nn == t.n, name
        slots = flat[24:24 + 4 * ns].reshape(ns, 4)             # (4 node + child, parent slot, triangle, level)
        tris = flat[24 + 4 * ns:24 + 4 * ns + n_tris]
        nodes = flat[24 + 4 * ns + n_tris:24 + 4 * ns + n_tris + 5 * nn].reshape(nn, 5)
        assert rec_off == -(-(24 + 4 * ns + n_tris + 5 * nn) // 4) * 4 and trec_off == rec_off + ns * Q_REC, name
        assert size == -(-(trec_off + 2 * ns * Q_TRI) // 4) * 4, name
        rec, parent, tri, level = slots.T
        # every (node, child) pair once, with its own child word
        assert np.array_equal(np.sort(rec), np.flatnonzero(t.child.reshape(-1) != -1)), name
        assert np.array_equal(tri, np.where(t.child.reshape(-1)[rec] >= 0, t.child.reshape(-1)[rec], -1)), name
        # every face index in exactly one slot; the triangle table lists exactly those slots
        assert np.array_equal(np.sort(tri[tri >= 0]), np.arange(nF)), name
        assert np.array_equal(np.sort(tris), np.flatnonzero(tri >= 0)), name
        # levels: ascending, the level-begin table consistent with them, a slot's parent slot in the previous level
        assert (np.diff(level) >= 0).all() and level[0] == 0 and level[-1] == nl - 1, name
        for l in range(9):
            assert lvl_begin[l] == (np.searchsorted(level, l) if l < nl else ns), (name, l)
        assert (parent[level == 0] == -1).all(), name
        deeper = level > 0
        assert (parent[deeper] >= 0).all() and np.array_equal(level[parent[deeper]], level[deeper] - 1), name
        # ... and that parent slot is the slot of the node the pair belongs to
        assert np.array_equal(t.child.reshape(-1)[rec[parent[deeper]]] & 0x7fffffff, rec[deeper] >> 2), name
        assert (t.child.reshape(-1)[rec[parent[deeper]]] < -1).all(), name
        # the node table: every slot exactly once as a child, in its node's row at its child's place; own slot -1 for the root only
        kids = nodes[:, 1:]
        assert np.array_equal(np.sort(kids[kids >= 0]), np.arange(ns)), name
        assert (nodes[:, 0] == -1).sum() == 1, name
        for row in nodes:
            nd = 0 if row[0] < 0 else int(t.child.reshape(-1)[rec[row[0]]] & 0x7fffffff)
            for ch in range(4):
                assert (row[1 + ch] == -1) == (t.child[nd, ch] == -1), (name, nd, ch)
                if row[1 + ch] >= 0:
                    assert rec[row[1 + ch]] == 4 * nd + ch, (name, nd, ch)
        # the combine steps: deepest level first
        node_level = np.array([0 if r[0] < 0 else level[r[0]] + 1 for r in nodes])
        assert (np.diff(node_level) <= 0).all() and node_level[0] == nl - 1 and node_level[-1] == 0, name
        for st in range(9):
            assert step_begin[st] == (np.searchsorted(-node_level, -(nl - 1 - st)) if st < nl else nn), (name, st)
        # behind each slot: the record and the fp64 triangle of its (node, child), byte for byte
        recs = flat[rec_off:rec_off + ns * Q_REC].reshape(ns, Q_REC)
        trecs = flat[trec_off:trec_off + 2 * ns * Q_TRI].reshape(ns, 2 * Q_TRI)
        assert np.array_equal(recs, t.boxq.reshape(-1, Q_REC).view(np.int32)[rec]), name
        assert np.array_equal(trecs, t.triq.reshape(-1, Q_TRI).view(np.int32).reshape(-1, 2 * Q_TRI)[rec]), name
    assert qualified >= 5            # one triangle ... box (12) and the smallest blobs


def test_flat_blob_refusals(tables):
    # the first blob mesh over 64 slots: refused for its slots (and taken once the limit is its own count)
    name, t = next((n, t) for n, t in tables.items() if n.startswith("blob") and t.levels()[0] > FLAT_SLOTS)
    n_pairs, n_levels = t.levels()
    assert n_levels <= FLAT_LEVELS, (name, n_levels)
    assert t.blob().size == 0, name
    assert t.blob(max_slots=n_pairs - 1).size == 0 and t.blob(max_slots=n_pairs).size > 0, name
    # more levels than allowed: refused whatever the slots (the largest mesh is deeper than 8 levels)
    for name, t in tables.items():
        n_pairs, n_levels = t.levels()
        assert (t.blob(max_slots=1 << 30).size > 0) == (n_levels <= FLAT_LEVELS), (name, n_levels)
        if 1 < n_levels <= FLAT_LEVELS:
            assert t.blob(max_slots=1 << 30, max_levels=n_levels - 1).size == 0, name
            assert t.blob(max_slots=1 << 30, max_levels=n_levels).size > 0, name
    assert max(t.levels()[1] for t in tables.values()) > FLAT_LEVELS


def test_closed_by_index(shim):
    def closed(F, nV):
        F = np.ascontiguousarray(F, dtype=np.int32)
        return shim.shim_mt_closed(F.ctypes.data_as(C.c_void_p), F.shape[0], nV)
    Ft = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], dtype=np.int32)
    assert closed(Ft, 4) == 1
    assert closed(Ft[:3], 4) == 0                       # one face removed
    # a closed box as a triangle soup (three vertices of its own per face): open BY INDEX, whatever its geometry
    assert closed(np.arange(36).reshape(12, 3), 36) == 0
