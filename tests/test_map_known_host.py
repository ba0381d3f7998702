"""The known grid without a device (csrc/map_known_host.hpp through isdf_known_merge_host / _shift_host / _fill_host / _frontier_host)
against the NumPy restatement of the four definitions (tests/known_reference.py), == on bytes; the struct sizes; and the header in a
stand-alone program built with the address and undefined-behaviour sanitizers.  Three grids: 7 x 3 x 5 (a dword covers seven columns,
105 voxels leave a tail that must stay 0), 6 x 5 x 64 (aligned columns) and the map tests' 24 x 20 x 70."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import known_reference as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = [(7, 3, 5), (6, 5, 64), (24, 20, 70)]
IDS = ["7x3x5", "6x5x64", "24x20x70"]


def shifts_of(dims):
    nx, ny, nz = dims
    return [(0, 0, 0), (0, 0, 1), (0, 0, -1), (0, 0, 33), (0, 1, 0), (-1, 0, 0), (2, -3, 5), (0, 0, nz), (nx, 0, 0), (0, -ny, 0)]


def masks_of(dims, seed=5):
    rng = np.random.default_rng(seed)
    return {"0.1": rng.uniform(size=dims) < 0.1, "0.9": rng.uniform(size=dims) < 0.9, "ones": np.ones(dims, dtype=bool), "zeros": np.zeros(dims, dtype=bool)}


def fill_boxes(dims):
    """one voxel; the whole grid (as a box and as None); a box whose z range begins at bit 31 of a word and ends at bit 0 of the next"""
    nx, ny, nz = dims
    out = [(nx // 2, ny // 2, nz // 2) * 2, (0, 0, 0, nx - 1, ny - 1, nz - 1), None]
    for a in range(31, nx * ny * nz - 1, 32):                   # voxel a is bit 31: a and a + 1 in one column
        z = a % nz
        if z + 1 < nz:
            col = a // nz
            out.append((col // ny, col % ny, z, col // ny, col % ny, z + 1))
            out.append((max(col // ny - 1, 0), 0, z, col // ny, ny - 1, z + 1))
            break
    return out


def bad_boxes(dims):
    nx, ny, nz = dims
    return [(-1, 0, 0, 0, 0, 0), (0, 0, 0, nx, 0, 0), (0, 0, 0, 0, ny, 0), (0, 0, 0, 0, 0, nz), (1, 0, 0, 0, 0, 0), (0, 0, 2, 0, 0, 1), (0, ny, 0, 0, ny, 0)]


def frontier_cases(dims, seed=9):
    """(name, K, occupancy) of the frontier's cases"""
    nx, ny, nz = dims
    rng = np.random.default_rng(seed)
    none = np.zeros(dims, dtype=np.uint8)
    cases = []
    k = np.zeros(dims, dtype=bool)
    k[1:nx - 1, 1:ny - 1, 1:nz - 1] = True                        # a known block inside unknown space: its shell minus occupied voxels
    occ = none.copy()
    occ[1, 1, 1:3] = 1
    occ[nx // 2, ny // 2, nz // 2] = 1
    cases.append(("block", k, occ))
    k = np.zeros(dims, dtype=bool)
    k[0:max(nx - 2, 1), 0:max(ny - 1, 1), 0:max(nz - 2, 1)] = True    # touching three faces: the face voxels are not frontier by themselves
    cases.append(("faces", k, none))
    k = np.ones(dims, dtype=bool)
    hole = (nx // 2, ny // 2, nz // 2)
    k[hole] = False                                               # one unknown voxel inside known space: its free 6-neighbours
    occ = none.copy()
    occ[hole[0], hole[1], hole[2] - 1] = 1
    cases.append(("hole", k, occ))
    cases.append(("all known", np.ones(dims, dtype=bool), none))
    cases.append(("all unknown", np.zeros(dims, dtype=bool), none))
    cases.append(("random", rng.uniform(size=dims) < 0.6, (rng.uniform(size=dims) < 0.2).astype(np.uint8) * rng.integers(1, 255, dims).astype(np.uint8)))
    cases.append(("random sparse", rng.uniform(size=dims) < 0.05, (rng.uniform(size=dims) < 0.5).astype(np.uint8)))
    return cases


def test_pack_layout(pkg):
    """the restatement's layout by hand, and the package's pack / unpack against it"""
    m = np.zeros((7, 3, 5), dtype=bool)
    m[0, 0, 0] = m[1, 0, 1] = m[6, 2, 4] = True                  # voxels 0, 16, 104
    w = kr.pack(m)
    assert w.tolist() == [1 | 1 << 16, 0, 0, 1 << 8] and np.array_equal(kr.unpack(w, m.shape), m)
    assert np.array_equal(pkg.engine.known_pack(m), w) and np.array_equal(pkg.engine.known_unpack(w, m.shape), m)
    assert pkg.engine.known_words(m.shape) == 4


@pytest.mark.parametrize("dims", GRIDS, ids=IDS)
def test_shift_equals_the_definition(pkg, product_lib, dims):
    for name, k in masks_of(dims).items():
        for s in shifts_of(dims):
            got = pkg.engine.known_shift_host(kr.pack(k), dims, s, lib=product_lib)
            assert got.dtype == np.uint32 and np.array_equal(got, kr.pack(kr.shift(k, s))), (name, s)
    assert np.array_equal(pkg.engine.known_pack(k), kr.pack(k)) and np.array_equal(pkg.engine.known_unpack(kr.pack(k), dims), k)


@pytest.mark.parametrize("dims", GRIDS, ids=IDS)
def test_fill_equals_the_definition(pkg, product_lib, dims):
    boxes = fill_boxes(dims)
    assert len(boxes) >= 4                                      # the bit 31 / bit 0 box exists on every grid
    for name, k in masks_of(dims).items():
        for box in boxes:
            for value in (1, 0):
                got, newly = pkg.engine.known_fill_host(kr.pack(k), dims, box, value, lib=product_lib)
                want = kr.fill(k, box, value)
                assert np.array_equal(got, kr.pack(want)), (name, box, value)
                assert newly == int((want & ~k).sum())
    for box in bad_boxes(dims):
        with pytest.raises(pkg.engine.IsdfError) as e:
            pkg.engine.known_fill_host(kr.pack(k), dims, box, 1, lib=product_lib)
        assert e.value.code == pkg.capi.ISDF_ERR_INVALID_ARG


@pytest.mark.parametrize("dims", GRIDS, ids=IDS)
def test_frontier_equals_the_definition(pkg, product_lib, dims):
    counts = {}
    for name, k, occ in frontier_cases(dims):
        bits, vox, info = pkg.engine.known_frontier_host(kr.pack(k), occ, lib=product_lib)
        want = kr.frontier(k, occ)
        assert np.array_equal(bits, kr.pack(want)), name
        assert vox.dtype == np.int64 and np.array_equal(vox, np.flatnonzero(want.reshape(-1))), name          # ascending
        lo, hi = kr.box_of(want)
        assert (info.n_frontier, list(info.lo), list(info.hi)) == (int(want.sum()), lo, hi), name
        counts[name] = int(want.sum())
        if counts[name] > 1:
            with pytest.raises(pkg.engine.IsdfError) as e:
                pkg.engine.known_frontier_host(kr.pack(k), occ, capacity=counts[name] - 1, lib=product_lib)
            assert e.value.code == pkg.capi.ISDF_ERR_OVERFLOW
    assert counts["all known"] == 0 and counts["all unknown"] == 0 and counts["random"] > 0
    if dims == GRIDS[2]:                                        # the cases by hand, where the grid is large enough to keep them apart
        nx, ny, nz = dims
        assert counts["block"] == (nx - 2) * (ny - 2) * (nz - 2) - (nx - 4) * (ny - 4) * (nz - 4) - 2       # the shell minus its two occupied voxels
        assert counts["hole"] == 5                              # six neighbours, one occupied
        a, b, c = nx - 2, ny - 1, nz - 2                        # the block's three faces inside the grid, none of the three on the grid's faces
        assert counts["faces"] == a * b * c - (a - 1) * (b - 1) * (c - 1)


def test_overflow_leaves_the_list_untouched(pkg, product_lib):
    dims = GRIDS[2]
    _, k, occ = frontier_cases(dims)[0]
    w = kr.pack(k)
    d = (C.c_int32 * 3)(*dims)
    vox = np.full(8, -7, dtype=np.int64)
    info = pkg.capi.IsdfMapFrontierInfo()
    rc = product_lib.isdf_known_frontier_host(w.ctypes.data_as(C.c_void_p), occ.ctypes.data_as(C.c_void_p), d, None, vox.ctypes.data_as(C.c_void_p), 8, C.byref(info))
    assert rc == pkg.capi.ISDF_ERR_OVERFLOW and (vox == -7).all() and info.n_frontier == int(kr.frontier(k, occ).sum())


def test_merge_equals_the_scan_sets(pkg, product_lib):
    import test_gpu_map_scan as ms
    _, ends, hit = ms._scene()
    free, hits, _ = ms._sets(pkg, product_lib, ends, hit)
    assert free.any() and (hits > 0).any()
    for name, k in masks_of(ms.DIMS).items():
        got, newly = pkg.engine.known_merge_host(kr.pack(k), ms.DIMS, free, hits, lib=product_lib)
        want = kr.merge(k, free, hits)
        assert np.array_equal(got, kr.pack(want)) and newly == int((want & ~k).sum()), name
    got, _ = pkg.engine.known_merge_host(kr.pack(k), ms.DIMS, None, hits, lib=product_lib)
    assert np.array_equal(got, kr.pack(k | (hits > 0)))


def test_struct_sizes(pkg, product_lib):
    sz = (C.c_int * 4)()
    product_lib.isdf_map_known_sizes(sz)
    assert list(sz) == [C.sizeof(pkg.capi.IsdfMapKnownInfo), C.sizeof(pkg.capi.IsdfMapFrontierInfo), C.sizeof(pkg.capi.IsdfTrajKnownParams),
                        C.sizeof(pkg.capi.IsdfTrajKnownInfo)] == [56, 40, 16, 160]
    p = pkg.capi.IsdfTrajKnownParams()
    product_lib.isdf_traj_known_params_default(C.byref(p))
    assert (p.margin, p.mode) == (-1.0, pkg.capi.SWEPT_FIELD_PLANNER)
    product_lib.isdf_traj_known_params_default(None)
    product_lib.isdf_map_known_sizes(None)


def test_bad_arguments(pkg, product_lib):
    w = kr.pack(np.ones((2, 2, 2), dtype=bool))
    p = w.ctypes.data_as(C.c_void_p)
    d, bad = (C.c_int32 * 3)(2, 2, 2), (C.c_int32 * 3)(2, 0, 2)
    s = (C.c_int32 * 3)(0, 0, 1)
    E = pkg.capi.ISDF_ERR_INVALID_ARG
    assert product_lib.isdf_known_shift_host(p, d, s, p) == E and product_lib.isdf_known_shift_host(p, bad, s, p) == E
    assert product_lib.isdf_known_merge_host(None, d, None, None) == E and product_lib.isdf_known_fill_host(p, bad, None, 1) == E
    assert product_lib.isdf_known_frontier_host(p, None, d, None, None, 0, None) == E


HOST_PROGRAM = r'''
#include "map_known_host.hpp"
#include <cstdio>
#include <vector>
using namespace isdf;
int main() {
    const int32_t grids[3][3] = {{7, 3, 5}, {6, 5, 64}, {24, 20, 70}};
    for (int g = 0; g < 3; g++) {
        const int32_t *dims = grids[g];
        const long long n = mk_voxels(dims), nw = mk_words(n);
        std::vector<uint32_t> k((size_t)nw), out((size_t)nw), front((size_t)nw);          // exactly nw words: a read beyond them is caught
        std::vector<uint8_t> occ((size_t)n);                                              // exactly n bytes
        uint64_t x = 88172645463325252ull + g;
        for (long long a = 0; a < n; a++) {
            x ^= x << 13; x ^= x >> 7; x ^= x << 17;
            if (x % 10 < 6) k[a >> 5] |= 1u << (a & 31);
            occ[a] = (x >> 20) % 5 == 0 ? (uint8_t)(1 + (x >> 30) % 200) : 0;
        }
        // shifts whose delta is negative, beyond the stream on either side, and beyond int32
        const int32_t shifts[][3] = {{0, 0, 0}, {0, 0, -1}, {0, 0, 33}, {-1, 0, 0}, {2, -3, 5}, {0, 0, dims[2]}, {dims[0], 0, 0}, {0, -dims[1], 0}, {-dims[0], -dims[1], -dims[2]},
                                     {dims[0] - 1, dims[1] - 1, dims[2] - 1}, {1 - dims[0], 1 - dims[1], 1 - dims[2]}, {2147483647, 2147483647, 2147483647},
                                     {-2147483647 - 1, -2147483647 - 1, -2147483647 - 1}, {0, 0, 2147483647}};
        for (const auto &s : shifts) {
            mk_shift_host(k.data(), dims, s, out.data());
            unsigned long long sum = 0;
            for (uint32_t w : out) sum = sum * 1000003ull + w;
            std::printf("%llu\n", sum);
        }
        for (long long b : {-100ll, -32ll, -31ll, -1ll, 0ll, 1ll, 32 * nw - 33, 32 * nw - 32, 32 * nw - 1, 32 * nw, 32 * nw + 5, (long long)1 << 40, -((long long)1 << 40)})
            std::printf("%u\n", mk_bits_at(k.data(), nw, b));
        int lo[3], hi[3];
        std::vector<int64_t> vox((size_t)n);
        const long long nf = mk_frontier_host(k.data(), occ.data(), dims, front.data(), vox.data(), n, lo, hi);
        unsigned long long sum = 0;
        for (long long i = 0; i < nf; i++) sum = sum * 1000003ull + (unsigned long long)vox[i];
        std::printf("%lld %llu %d %d %d %d %d %d\n", nf, sum, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]);
        const int32_t box[6] = {0, 0, 0, dims[0] - 1, dims[1] - 1, dims[2] - 1}, one[6] = {dims[0] - 1, dims[1] - 1, dims[2] - 1, dims[0] - 1, dims[1] - 1, dims[2] - 1};
        std::printf("%lld ", mk_fill_host(k.data(), dims, one, 0));
        std::printf("%lld ", mk_fill_host(k.data(), dims, one, 1));
        std::printf("%lld\n", mk_fill_host(k.data(), dims, box, 1));
        std::vector<uint32_t> hits((size_t)n, 1u);
        std::printf("%lld\n", mk_merge_host(k.data(), dims, occ.data(), hits.data()));
    }
    std::printf("ok\n");
    return 0;
}
'''


def test_host_header_under_sanitizers(pkg, product_lib):
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "host.cpp")
        open(p, "w").write(HOST_PROGRAM)
        exe = os.path.join(d, "host")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I", os.path.join(ROOT, "implicit-sdf-planner_amd", "csrc"), p, "-o", exe])
        r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:]
    lines = r.stdout.strip().splitlines()[:-1]
    per = len(lines) // 3
    for g, dims in enumerate(GRIDS):
        # the same generator in Python: the program's K and occupancy, its shifts through the library and the restatement
        n = int(np.prod(dims))
        x = (88172645463325252 + g) & (2**64 - 1)
        k, occ = np.zeros(n, dtype=bool), np.zeros(n, dtype=np.uint8)
        for a in range(n):
            x ^= (x << 13) & (2**64 - 1); x ^= x >> 7; x ^= (x << 17) & (2**64 - 1)
            k[a] = x % 10 < 6
            occ[a] = 1 + (x >> 30) % 200 if (x >> 20) % 5 == 0 else 0
        k, occ = k.reshape(dims), occ.reshape(dims)
        L = lines[g * per:(g + 1) * per]
        nx, ny, nz = dims
        big = 2147483647
        shifts = [(0, 0, 0), (0, 0, -1), (0, 0, 33), (-1, 0, 0), (2, -3, 5), (0, 0, nz), (nx, 0, 0), (0, -ny, 0), (-nx, -ny, -nz), (nx - 1, ny - 1, nz - 1),
                  (1 - nx, 1 - ny, 1 - nz), (big, big, big), (-big - 1, -big - 1, -big - 1), (0, 0, big)]
        for s, line in zip(shifts, L):
            h = 0
            for w in kr.pack(kr.shift(k, s)).tolist():
                h = (h * 1000003 + w) & (2**64 - 1)
            assert int(line) == h, (dims, s)
        want = kr.frontier(k, occ)
        vox = np.flatnonzero(want.reshape(-1))
        h = 0
        for v in vox.tolist():
            h = (h * 1000003 + v) & (2**64 - 1)
        lo, hi = kr.box_of(want)
        assert [int(v) for v in L[len(shifts) + 13].split()] == [len(vox), h] + lo + hi, dims
        last = bool(k[-1, -1, -1])
        assert [int(v) for v in L[len(shifts) + 14].split()] == [0, 1, n - int(k.sum()) - (0 if last else 1)]
        assert int(L[len(shifts) + 15]) == 0
