"""The in-place map update's boundary without a device: exported symbols, the params defaults, the struct layouts of the header against
the ctypes mirror, the argument errors that need no ctx - and the host arithmetic of csrc/map_update_host.hpp (box growth and clamping,
the ESDF skip rule, the scatter of a packed box into the host table) in a stand-alone program built with the address and
undefined-behaviour sanitizers."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("isdf_map_update_params_default", "isdf_map_update_sizes", "isdf_update_pointcloud", "isdf_update_voxels", "isdf_map_counts_get")


def test_symbols_defaults_and_sizes(pkg, product_lib):
    capi = pkg.capi
    for n in SYMBOLS:
        assert n in capi.EXPORTED_SYMBOLS and hasattr(product_lib, n)
    assert hasattr(pkg.Engine, "update_pointcloud") and hasattr(pkg.Engine, "update_voxels") and hasattr(pkg.Engine, "map_counts")
    p = capi.IsdfMapUpdateParams()
    product_lib.isdf_map_update_params_default(C.byref(p))
    assert (p.max_new_voxels, p.full_fraction, p.refresh_esdf, p.refresh_frontend) == (65536, 0.5, 1, 1)
    sz = (C.c_int * 2)()
    product_lib.isdf_map_update_sizes(sz)
    assert list(sz) == [C.sizeof(capi.IsdfMapUpdateParams), C.sizeof(capi.IsdfMapUpdateInfo)] == [24, 104]
    product_lib.isdf_map_update_params_default(None)            # null-safe
    product_lib.isdf_map_update_sizes(None)


def test_struct_layouts_match_header(pkg):
    capi = pkg.capi
    structs = {"isdf_map_update_params": capi.IsdfMapUpdateParams, "isdf_map_update_info": capi.IsdfMapUpdateInfo}
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
    assert [f for f, _ in capi.IsdfMapUpdateInfo._fields_] == ["n_points", "n_new_voxels", "dirty_lo", "dirty_hi", "path", "esdf_refreshed", "frontend_refreshed",
                                                               "cspace_refreshed", "host_table_patched", "field_dropped", "esdf_voxels_lowered",
                                                               "cspace_voxels_recomputed", "count_ms", "esdf_ms", "frontend_ms"]


def test_argument_errors_without_a_ctx(pkg, product_lib):
    capi = pkg.capi
    xyz = np.zeros((2, 3), dtype=np.float32); ijk = np.zeros((2, 3), dtype=np.int32); out = np.zeros(4, dtype=np.uint32)
    info = capi.IsdfMapUpdateInfo()
    assert product_lib.isdf_update_pointcloud(None, xyz.ctypes.data_as(C.POINTER(C.c_float)), 2, None, C.byref(info)) == capi.ISDF_ERR_INVALID_ARG
    assert product_lib.isdf_update_voxels(None, ijk.ctypes.data_as(C.POINTER(C.c_int32)), 2, None, C.byref(info)) == capi.ISDF_ERR_INVALID_ARG
    assert product_lib.isdf_map_counts_get(None, out.ctypes.data_as(C.c_void_p)) == capi.ISDF_ERR_INVALID_ARG


HOST_PROGRAM = r'''
#include "map_update_host.hpp"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
using namespace isdf;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); return 1; } } while (0)
int main() {
    const int dims[3] = {24, 20, 70};
    // growth and clamping: every side, no side, an empty box
    MuBox all{{0, 0, 0}, {23, 19, 69}};
    MuBox g = mu_box_grow(all, 2, dims);
    for (int a = 0; a < 3; a++) CHECK(g.lo[a] == 0 && g.hi[a] == dims[a] - 1);
    MuBox col{{10, 10, 63}, {10, 10, 64}};
    g = mu_box_grow(col, 2, dims);
    CHECK(g.lo[0] == 8 && g.hi[0] == 12 && g.lo[2] == 61 && g.hi[2] == 66 && mu_box_voxels(g) == 5 * 5 * 6);
    g = mu_box_grow(col, 15, dims);
    CHECK(g.lo[0] == 0 && g.hi[0] == 23 && g.lo[1] == 0 && g.hi[1] == 19 && g.lo[2] == 48 && g.hi[2] == 69);
    MuBox none{{0x7FFFFFFF, 0x7FFFFFFF, 0x7FFFFFFF}, {-1, -1, -1}};
    CHECK(mu_box_empty(none) && mu_box_voxels(none) == 0 && mu_box_empty(mu_box_grow(none, 2, dims)));
    const int big[3] = {4096, 4096, 4096};
    MuBox whole{{0, 0, 0}, {4095, 4095, 4095}};
    CHECK(mu_box_voxels(mu_box_grow(whole, 15, big)) == 4096ll * 4096 * 4096);
    // distance to the box
    CHECK(mu_box_dist2(10, 10, 63, col.lo, col.hi) == 0 && mu_box_dist2(10, 10, 60, col.lo, col.hi) == 9 && mu_box_dist2(7, 14, 66, col.lo, col.hi) == 9 + 16 + 4);
    CHECK(mu_box_dist2(4095, 4095, 4095, all.lo, all.hi) == 4072ll * 4072 + 4076ll * 4076 + 4026ll * 4026);
    // the skip rule never skips a voxel that a new voxel at box distance d could lower: for every d2_old, old = float(res * sqrt(d2_old)),
    // a box distance below d2_old must be scanned - at small, large and the largest distances, and at several resolutions
    const double ress[4] = {0.5, 0.2, 0.1, 0.037};
    for (double res : ress) {
        std::vector<long long> d2s;
        for (long long d2 = 0; d2 < 5000; d2++) d2s.push_back(d2);
        for (long long d2 = 8388000; d2 < 8389500; d2++) d2s.push_back(d2);            // around 2^23, where the float's error reaches one unit
        for (long long d2 = 3ll * 4095 * 4095 - 1500; d2 <= 3ll * 4095 * 4095; d2++) d2s.push_back(d2);
        for (long long d2 : d2s) {
            const float old = (float)(res * std::sqrt((double)d2));
            if (d2 > 0) CHECK(!mu_esdf_skip(old, res, d2 - 1));
            CHECK(mu_esdf_skip(old, res, d2 + 2 + d2 / 1000000));                      // ... and it does skip just beyond
        }
        CHECK(!mu_esdf_skip(INFINITY, res, 3ll * 4095 * 4095) && !mu_esdf_skip(NAN, res, 0));
        CHECK(!mu_esdf_skip((float)(res * std::sqrt(1.7976931348623157e308)), res, 1ll << 40));
        CHECK(!mu_esdf_skip(0.f, res, 0) && mu_esdf_skip(0.f, res, 1));
    }
    // the scatter: a box of a 6 x 5 x 7 table with 4 and with 12 dwords per voxel, rows placed exactly, nothing else touched
    for (size_t nw : {(size_t)4, (size_t)12}) {
        const int d[3] = {6, 5, 7};
        std::vector<uint32_t> table((size_t)6 * 5 * 7 * nw, 0xAAAAAAAAu);
        const MuBox b{{1, 0, 2}, {3, 4, 6}};
        std::vector<uint32_t> packed((size_t)mu_box_voxels(b) * nw);
        for (size_t i = 0; i < packed.size(); i++) packed[i] = (uint32_t)i;
        mu_scatter_box(table.data(), d, nw, b, packed.data());
        size_t i = 0, touched = 0;
        for (int x = 0; x < 6; x++) for (int y = 0; y < 5; y++) for (int z = 0; z < 7; z++) for (size_t w = 0; w < nw; w++) {
            const bool in = x >= 1 && x <= 3 && z >= 2;
            const uint32_t v = table[(((size_t)x * 5 + y) * 7 + z) * nw + w];
            if (in) { const size_t k = ((((size_t)(x - 1) * 5 + y) * 5) + (z - 2)) * nw + w; CHECK(v == (uint32_t)k); touched++; }
            else CHECK(v == 0xAAAAAAAAu);
            i++;
        }
        CHECK(touched == packed.size());
        mu_scatter_box(table.data(), d, nw, MuBox{{1, 1, 1}, {0, 0, 0}}, nullptr);      // an empty box reads nothing
    }
    std::printf("ok\n");
    return 0;
}
'''


def test_host_arithmetic_under_sanitizers(pkg):
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "host.cpp")
        open(p, "w").write(HOST_PROGRAM)
        exe = os.path.join(d, "host")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I", os.path.join(ROOT, "implicit-sdf-planner_amd", "csrc"), p, "-o", exe])
        r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:]
