"""Voxels cleared from the map in place, without a device: the plain-C++ ESDF raise (isdf_clear_esdf_host, csrc/map_clear_host.hpp)
against a brute-force numpy distance transform on maps of at most 12 x 10 x 9 voxels, the touched test as a superset of the voxels
that truly rise, the sizes and status codes of the new ABI - and the host header in a stand-alone program built with the address and
undefined-behaviour sanitizers.  Every comparison of ESDF values is == on bytes."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("isdf_map_clear_params_default", "isdf_map_clear_sizes", "isdf_clear_pointcloud", "isdf_clear_voxels", "isdf_clear_esdf_host",
           "isdf_clear_touched_host")
DBL_MAX = 1.7976931348623157e308


def _edt(occ, res):
    """float32(res * sqrt(d2)) of the exact integer d2 to the nearest occupied voxel, by brute force; no occupied voxel: sqrt(DBL_MAX)"""
    idx = np.stack(np.meshgrid(*[np.arange(n) for n in occ.shape], indexing="ij"), axis=-1).reshape(-1, 3).astype(np.int64)
    o = idx[occ.reshape(-1) == 1]
    if len(o) == 0:
        with np.errstate(over="ignore"):
            return np.full(occ.shape, np.float32(np.float64(res) * np.sqrt(np.float64(DBL_MAX))), dtype=np.float32)
    d2 = ((idx[:, None, :] - o[None, :, :]) ** 2).sum(axis=2).min(axis=1)
    return (np.float64(res) * np.sqrt(d2.astype(np.float64))).astype(np.float32).reshape(occ.shape)


def _occ(dims, cells):
    occ = np.zeros(dims, dtype=np.uint8)
    for c in cells:
        occ[tuple(c)] = 1
    return occ


def _random_case(seed, dims, n_occ, n_clear):
    rng = np.random.default_rng(seed)
    flat = rng.choice(int(np.prod(dims)), n_occ, replace=False)
    cells = np.stack(np.unravel_index(flat, dims), axis=1)
    return cells, cells[:n_clear]


# (name, dims, res, occupied before, cleared)
CASES = [
    ("isolated voxel, others far", (12, 10, 9), 0.5, [(2, 2, 2), (10, 8, 7), (11, 0, 8)], [(2, 2, 2)]),
    ("neighbour remains", (12, 10, 9), 0.5, [(5, 5, 4), (5, 5, 5), (0, 9, 0)], [(5, 5, 4)]),
    ("map corner", (12, 10, 9), 0.2, [(0, 0, 0), (11, 9, 8), (6, 4, 4)], [(0, 0, 0)]),
    ("far corner", (11, 7, 9), 0.2, [(10, 6, 8), (0, 0, 0)], [(10, 6, 8)]),
    ("tie: two equidistant, one cleared", (12, 10, 9), 0.5, [(3, 5, 4), (9, 5, 4), (6, 0, 0)], [(3, 5, 4)]),
    ("tie: a ring of four, two cleared", (9, 9, 5), 0.1, [(4, 1, 2), (4, 7, 2), (1, 4, 2), (7, 4, 2)], [(4, 1, 2), (7, 4, 2)]),
    ("all cleared", (6, 5, 4), 0.5, [(1, 1, 1), (4, 3, 2), (5, 4, 3)], [(1, 1, 1), (4, 3, 2), (5, 4, 3)]),
    ("the only voxel cleared", (3, 1, 2), 0.037, [(2, 0, 1)], [(2, 0, 1)]),
    ("nothing cleared", (5, 4, 3), 0.5, [(1, 1, 1)], []),
    ("one column", (1, 1, 9), 0.5, [(0, 0, 0), (0, 0, 4), (0, 0, 8)], [(0, 0, 4)]),
] + [(f"random {s}", (12, 10, 9), 0.5) + _random_case(s, (12, 10, 9), 25, 7) for s in range(3)] \
  + [("random dense", (7, 10, 9), 0.3) + _random_case(11, (7, 10, 9), 300, 120)]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_host_raise_against_numpy(pkg, product_lib, case):
    capi = pkg.capi
    _, dims, res, before_cells, cleared = case
    assert dims[0] <= 12 and dims[1] <= 10 and dims[2] <= 9
    occ_old = _occ(dims, before_cells)
    occ_new = occ_old.copy()
    for c in cleared:
        occ_new[tuple(c)] = 0
    old, want = _edt(occ_old, res), _edt(occ_new, res)
    raised = want.view(np.uint32) != old.view(np.uint32)
    assert (want >= old).all()
    ijk = np.ascontiguousarray(np.asarray(cleared, dtype=np.int32).reshape(-1, 3))
    d = (C.c_int32 * 3)(*dims)
    # the touched test alone: a superset of the voxels that truly rise
    touched = np.zeros(dims, dtype=np.uint8)
    n_t = product_lib.isdf_clear_touched_host(old.ctypes.data_as(C.c_void_p), d, res, ijk.ctypes.data_as(C.c_void_p), len(ijk), touched.ctypes.data_as(C.c_void_p))
    assert n_t == touched.sum() and set(np.unique(touched)) <= {0, 1}
    assert not (raised & (touched == 0)).any(), "a voxel rose that the touched test left out"
    # the raise
    got = old.copy()
    info = capi.IsdfMapClearInfo()
    assert product_lib.isdf_clear_esdf_host(occ_new.ctypes.data_as(C.c_void_p), got.ctypes.data_as(C.c_void_p), d, res, ijk.ctypes.data_as(C.c_void_p), len(ijk),
                                            C.byref(info)) == capi.ISDF_OK
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert info.esdf_voxels_raised == raised.sum() and info.n_cleared_voxels == len(ijk) == info.n_points
    if len(ijk) == 0:
        assert info.path == 0 and n_t == 0 and info.esdf_voxels_recomputed == 0 and list(info.dirty_lo) > list(info.dirty_hi)
        return
    assert list(info.dirty_lo) == ijk.min(axis=0).tolist() and list(info.dirty_hi) == ijk.max(axis=0).tolist()
    if not occ_new.any():
        with np.errstate(over="ignore"):
            inf_like = np.float32(np.float64(res) * np.sqrt(np.float64(DBL_MAX)))
        assert info.path == 2 and (got == inf_like).all() and np.isinf(inf_like) and info.esdf_voxels_recomputed == np.prod(dims)
        return
    assert info.path == 1 and raised.any()
    t = np.argwhere(touched == 1)
    assert list(info.touched_lo) == t.min(axis=0).tolist() and list(info.touched_hi) == t.max(axis=0).tolist()
    assert raised.sum() <= n_t <= info.esdf_voxels_recomputed == np.prod(t.max(axis=0) - t.min(axis=0) + 1)
    # a remaining occupied voxel is never touched, a cleared one always
    assert not touched[occ_new == 1].any() and touched[tuple(ijk.T)].all()


def test_symbols_defaults_and_sizes(pkg, product_lib):
    capi = pkg.capi
    for n in SYMBOLS:
        assert n in capi.EXPORTED_SYMBOLS and hasattr(product_lib, n)
    assert hasattr(pkg.Engine, "clear_pointcloud") and hasattr(pkg.Engine, "clear_voxels")
    p = capi.IsdfMapClearParams()
    product_lib.isdf_map_clear_params_default(C.byref(p))
    assert (p.max_cleared_voxels, p.full_fraction, p.refresh_esdf, p.refresh_frontend) == (65536, 0.5, 1, 1)
    sz = (C.c_int * 2)()
    product_lib.isdf_map_clear_sizes(sz)
    assert list(sz) == [C.sizeof(capi.IsdfMapClearParams), C.sizeof(capi.IsdfMapClearInfo)] == [24, 152]
    product_lib.isdf_map_clear_params_default(None)             # null-safe
    product_lib.isdf_map_clear_sizes(None)
    # the update's structs are untouched
    product_lib.isdf_map_update_sizes(sz)
    assert list(sz) == [24, 104]
    assert product_lib.isdf_abi_version() == 1


def test_struct_layouts_match_header(pkg):
    capi = pkg.capi
    structs = {"isdf_map_clear_params": capi.IsdfMapClearParams, "isdf_map_clear_info": capi.IsdfMapClearInfo}
    lines = []
    for cname, S in structs.items():
        lines.append(f'printf("%zu\\n", sizeof({cname}));')
        lines += [f'printf("%zu\\n", offsetof({cname}, {f}));' for f, _ in S._fields_]
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"isdf_accel.h\"\nint main(void) {\n" + "\n".join(lines) + "\nreturn 0; }\n"
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "t.c")
        open(p, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), p, "-o", exe])
        out = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    want = []
    for S in structs.values():
        want.append(C.sizeof(S))
        want += [getattr(S, f).offset for f, _ in S._fields_]
    assert out == want


def test_status_codes_without_a_ctx(pkg, product_lib):
    capi = pkg.capi
    xyz = np.zeros((2, 3), dtype=np.float32); ijk = np.zeros((2, 3), dtype=np.int32)
    info = capi.IsdfMapClearInfo()
    assert product_lib.isdf_clear_pointcloud(None, xyz.ctypes.data_as(C.POINTER(C.c_float)), 2, None, C.byref(info)) == capi.ISDF_ERR_INVALID_ARG
    assert product_lib.isdf_clear_voxels(None, ijk.ctypes.data_as(C.POINTER(C.c_int32)), 2, None, C.byref(info)) == capi.ISDF_ERR_INVALID_ARG
    dims = (4, 3, 2)
    occ = np.zeros(dims, dtype=np.uint8); esdf = np.zeros(dims, dtype=np.float32)
    d = (C.c_int32 * 3)(*dims)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)

    def raise_(occ_p, esdf_p, d_p, res, ijk_a, n):
        return product_lib.isdf_clear_esdf_host(occ_p, esdf_p, d_p, res, None if ijk_a is None else vp(ijk_a), n, None)
    good = np.array([[1, 1, 1]], dtype=np.int32)
    assert raise_(vp(occ), vp(esdf), d, 0.5, good, 1) == capi.ISDF_OK                      # info_out may be NULL
    assert np.isinf(esdf).all()                                                             # (no occupied voxel is left)
    esdf[:] = 0.0
    assert raise_(None, vp(esdf), d, 0.5, good, 1) == capi.ISDF_ERR_INVALID_ARG
    assert raise_(vp(occ), None, d, 0.5, good, 1) == capi.ISDF_ERR_INVALID_ARG
    assert raise_(vp(occ), vp(esdf), None, 0.5, good, 1) == capi.ISDF_ERR_INVALID_ARG
    assert raise_(vp(occ), vp(esdf), d, 0.0, good, 1) == capi.ISDF_ERR_INVALID_ARG
    assert raise_(vp(occ), vp(esdf), d, 0.5, None, 1) == capi.ISDF_ERR_INVALID_ARG
    assert raise_(vp(occ), vp(esdf), d, 0.5, good, -1) == capi.ISDF_ERR_INVALID_ARG
    assert raise_(vp(occ), vp(esdf), (C.c_int32 * 3)(4, 0, 2), 0.5, good, 1) == capi.ISDF_ERR_INVALID_ARG
    assert raise_(vp(occ), vp(esdf), (C.c_int32 * 3)(4, 3, 4097), 0.5, good, 1) == capi.ISDF_ERR_INVALID_ARG
    for bad in ([[4, 0, 0]], [[0, 3, 0]], [[0, 0, 2]], [[1, 1, 1], [0, -1, 0]]):
        b = np.array(bad, dtype=np.int32)
        assert raise_(vp(occ), vp(esdf), d, 0.5, b, len(b)) == capi.ISDF_ERR_INVALID_ARG
        assert product_lib.isdf_clear_touched_host(vp(esdf), d, 0.5, vp(b), len(b), None) == capi.ISDF_ERR_INVALID_ARG
    assert not esdf.any()                                                                       # a refused call wrote nothing
    assert product_lib.isdf_clear_touched_host(None, d, 0.5, vp(good), 1, None) == capi.ISDF_ERR_INVALID_ARG
    assert product_lib.isdf_clear_touched_host(vp(esdf), d, 0.5, vp(good), 1, None) == 1       # touched_out may be NULL: esdf 0 = only the voxel itself


HOST_PROGRAM = r'''
#include "map_clear_host.hpp"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
using namespace isdf;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); return 1; } } while (0)

static std::vector<float> brute(const std::vector<uint8_t> &occ, const int d[3], double res) {
    std::vector<float> e((size_t)d[0] * d[1] * d[2]);
    for (int x = 0; x < d[0]; x++) for (int y = 0; y < d[1]; y++) for (int z = 0; z < d[2]; z++) {
        int best = MC_EDT_INF;
        for (int i = 0; i < d[0]; i++) for (int j = 0; j < d[1]; j++) for (int k = 0; k < d[2]; k++)
            if (occ[((size_t)i * d[1] + j) * d[2] + k] == 1) { const int v = (x - i) * (x - i) + (y - j) * (y - j) + (z - k) * (z - k); if (v < best) best = v; }
        e[((size_t)x * d[1] + y) * d[2] + z] = mc_esdf_value(res, best);
    }
    return e;
}

int main() {
    // the touched test accepts the voxel's own d2 and everything nearer - at small, large and the largest distances, several resolutions
    const double ress[4] = {0.5, 0.2, 0.1, 0.037};
    for (double res : ress) {
        std::vector<long long> d2s;
        for (long long d2 = 0; d2 < 5000; d2++) d2s.push_back(d2);
        for (long long d2 = 8388000; d2 < 8389500; d2++) d2s.push_back(d2);
        for (long long d2 = 3ll * 4095 * 4095 - 1500; d2 <= 3ll * 4095 * 4095; d2++) d2s.push_back(d2);
        for (long long d2 : d2s) {
            const float old = (float)(res * std::sqrt((double)d2));
            CHECK(mc_touched(old, res, d2));
            if (d2 > 0) CHECK(mc_touched(old, res, d2 - 1));
            CHECK(!mc_touched(old, res, d2 + 2 + d2 / 1000000));                      // ... and it lets go just beyond
        }
        CHECK(mc_touched(INFINITY, res, 3ll * 4095 * 4095) && mc_touched(mc_esdf_value(res, MC_EDT_INF), res, 1ll << 40));
        CHECK(mc_touched(0.f, res, 0) && !mc_touched(0.f, res, 1));
        CHECK(std::isinf(mc_esdf_value(res, MC_EDT_INF)) && mc_esdf_value(res, 4) == (float)(res * 2.0));
    }
    // the line minimum at both ends of a line and with no sample on it
    {
        const int line[5] = {MC_EDT_INF, 9, MC_EDT_INF, 0, MC_EDT_INF};
        CHECK(mc_line_min(line, 5, 1, 0) == 9 && mc_line_min(line, 5, 1, 1) == 4 && mc_line_min(line, 5, 1, 4) == 1 && mc_line_min(line, 5, 1, 3) == 0);
        const int none[3] = {MC_EDT_INF, MC_EDT_INF, MC_EDT_INF};
        CHECK(mc_line_min(none, 3, 1, 1) >= MC_EDT_INF);
        const int strided[6] = {4, -1, 0, -1, 1, -1};
        CHECK(mc_line_min(strided, 3, 2, 0) == 1 && mc_line_min(strided, 3, 2, 2) == 1);
    }
    // the raise on seeded maps of 12 x 10 x 9 and 1 x 7 x 3 voxels: the bytes of the brute-force transform, the touched box inside the map
    unsigned seed = 12345u;
    auto rnd = [&seed]() { seed = seed * 1664525u + 1013904223u; return seed >> 8; };
    const int shapes[3][3] = {{12, 10, 9}, {1, 7, 3}, {5, 1, 1}};
    for (int round = 0; round < 12; round++) {
        const int *d = shapes[round % 3];
        const size_t n_vox = (size_t)d[0] * d[1] * d[2];
        std::vector<uint8_t> occ(n_vox, 0);
        const int n_occ = 1 + (int)(rnd() % (round % 3 == 0 ? 30 : 4));
        for (int i = 0; i < n_occ; i++) occ[rnd() % n_vox] = 1;
        std::vector<float> esdf = brute(occ, d, 0.5);
        std::vector<int32_t> cleared;
        const bool all = round >= 9;
        for (size_t a = 0; a < n_vox; a++)
            if (occ[a] == 1 && (all || rnd() % 3 == 0)) {
                occ[a] = 0;
                cleared.push_back((int32_t)(a / ((size_t)d[1] * d[2]))); cleared.push_back((int32_t)((a / d[2]) % d[1])); cleared.push_back((int32_t)(a % d[2]));
            }
        const std::vector<float> before = esdf, want = brute(occ, d, 0.5);
        McRaise R;
        std::vector<uint8_t> touched(n_vox, 7);
        mc_touched_host(before.data(), d, 0.5, cleared.data(), (long long)cleared.size() / 3, touched.data(), R);
        mc_esdf_raise_host(occ.data(), esdf.data(), d, 0.5, cleared.data(), (long long)cleared.size() / 3, R);
        long long raised = 0;
        for (size_t a = 0; a < n_vox; a++) {
            CHECK(std::memcmp(&esdf[a], &want[a], sizeof(float)) == 0);
            const bool rose = std::memcmp(&before[a], &want[a], sizeof(float)) != 0;
            raised += rose;
            CHECK(touched[a] <= 1 && (!rose || touched[a] == 1));
        }
        CHECK(R.raised == raised);
        if (all) CHECK(R.none_left && R.recomputed == (long long)n_vox);
        else if (!cleared.empty() && !R.none_left) {
            for (int a = 0; a < 3; a++) CHECK(R.touched.lo[a] >= 0 && R.touched.hi[a] < d[a] && R.touched.lo[a] <= R.touched.hi[a]);
            CHECK(R.recomputed == mu_box_voxels(R.touched) && R.n_touched <= R.recomputed);
        } else if (cleared.empty()) CHECK(mu_box_empty(R.touched) && R.recomputed == 0 && raised == 0);
    }
    std::printf("ok\n");
    return 0;
}
'''


def test_host_header_under_sanitizers(pkg):
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "host.cpp")
        open(p, "w").write(HOST_PROGRAM)
        exe = os.path.join(d, "host")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I", os.path.join(ROOT, "implicit-sdf-planner_amd", "csrc"), p, "-o", exe])
        r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:]
