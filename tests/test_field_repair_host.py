"""isdf_frontend_field_repair_host (csrc/frontend_field_host.hpp): the cost-to-go field repaired after voxels closed - every d below tau, the
smallest old d of a closed voxel, is kept, the rest is reset and relaxed again - against a from-scratch isdf_frontend_field_host on the
new table and against the tests' own Dijkstra (tests/field_reference.py), BYTE FOR BYTE; and, as a stand-alone program, under the
sanitizers.  No device."""
import math
import os
import subprocess

import numpy as np
import pytest

import field_reference as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "implicit-sdf-planner_amd", "csrc")
N_ATT = 121


def _far_cell(d, share=0.7):
    """a reached voxel whose d is nearest to `share` of the largest finite d: closing it must reset some of the field and keep some"""
    fin = np.isfinite(d)
    target = share * d[fin].max()
    cells = np.argwhere(fin)
    return tuple(int(v) for v in cells[np.argmin(np.abs(d[fin] - target))])


def _serpentine_cell(d):
    return (12, 12, 1)                                    # row y = 12 is the seventh of the twelve runs of the corridor


CASES = {
    # name: (occupancy, goal, the voxels to close (a function of the old field), far)
    "open_far": (fr.open_map(), (1, 5, 3), lambda d: [_far_cell(d)], True),
    "open_next_to_goal": (fr.open_map(), (1, 5, 3), lambda d: [(2, 5, 3)], False),
    "gap_closed": (fr.wall_with_gap(), (0, 0, 0), lambda d: [(4, 3, 2)], False),
    "serpentine_half_way": (fr.serpentine((24, 24, 3)), (0, 0, 1), lambda d: [_serpentine_cell(d)], True),
    "goal_closed": (fr.open_map(), (1, 5, 3), lambda d: [(1, 5, 3)], False),
    "pocket": (fr.sealed_pocket(), (0, 0, 0), lambda d: [fr.POCKET_CELL], False),
}


def _close(free, cells):
    out = free.copy()
    for c in cells:
        assert out[c]
        out[c] = False
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_repair_equals_a_build_on_the_new_table_byte_for_byte(pkg, product_lib, name):
    occ, goal, pick, far = CASES[name]
    free = occ == 0
    old, _ = pkg.frontend_field_host(fr.table_from_free(free), goal, N_ATT)
    cells = pick(old)
    free2 = _close(free, cells)
    table2 = fr.table_from_free(free2)
    got, reachable, info = pkg.frontend_field_repair_host(table2, goal, N_ATT, old)
    scratch, scratch_reachable = pkg.frontend_field_host(table2, goal, N_ATT)
    want = fr.field(free2, goal)
    print(f"\n{name}: closed {cells}, tau {info.tau:.6f}, reset {info.reset_voxels} of {int(np.isfinite(old).sum())} reached, reached now {info.reached_voxels}")
    assert fr.same_bytes(scratch, want) and fr.same_bytes(got, want), name
    assert reachable == scratch_reachable == bool(free2[goal]) and info.reachable == int(reachable) and info.status == (0 if reachable else 1)
    assert info.free_voxels == int(free2.sum()) and info.reached_voxels == int(np.isfinite(want).sum())
    reached_before = int(np.isfinite(old).sum())
    closed_reached = [c for c in cells if math.isfinite(old[c])]
    assert info.closed_reached == info.closed_voxels == len(closed_reached)
    tau = min((old[c] for c in closed_reached), default=math.inf)
    assert info.tau == tau and info.reset_voxels == int((np.isfinite(old) & (old >= tau)).sum())
    kept = old < tau
    assert fr.same_bytes(got[kept], old[kept])            # every value below tau is the old one
    if far:
        assert 0 < info.reset_voxels < reached_before     # the rule was exercised: neither nothing nor a disguised rebuild
    if name == "open_next_to_goal":
        assert tau == 1.0 and info.reset_voxels == reached_before - 1
    if name == "gap_closed":
        assert np.isinf(got[5:]).all() and np.isfinite(got[:4]).all() and np.isfinite(old[5:]).all()
    if name == "serpentine_half_way":
        assert np.isfinite(got[free2]).all() and not fr.same_bytes(got, np.where(free2, old, np.inf))      # the way round the cell is longer
    if name == "goal_closed":
        assert tau == 0.0 and info.reset_voxels == reached_before and np.isinf(got).all() and not reachable
    if name == "pocket":
        assert math.isinf(tau) and info.reset_voxels == 0 and fr.same_bytes(got, old) and np.isinf(old[fr.POCKET_CELL])


def test_two_repairs_equal_one(pkg, product_lib):
    occ, goal = fr.serpentine((24, 24, 3)), (0, 0, 1)
    free = occ == 0
    old, _ = pkg.frontend_field_host(fr.table_from_free(free), goal, N_ATT)
    a, b = [(12, 12, 1), (3, 4, 0)], [(12, 12, 0), (20, 20, 2), (23, 1, 1)]
    free_a, free_ab = _close(free, a), _close(free, a + b)
    d_a, _, _ = pkg.frontend_field_repair_host(fr.table_from_free(free_a), goal, N_ATT, old)
    d_ab, _, i_ab = pkg.frontend_field_repair_host(fr.table_from_free(free_ab), goal, N_ATT, d_a)
    d_one, _, i_one = pkg.frontend_field_repair_host(fr.table_from_free(free_ab), goal, N_ATT, old)
    want = fr.field(free_ab, goal)
    assert fr.same_bytes(d_a, fr.field(free_a, goal))
    assert fr.same_bytes(d_ab, want) and fr.same_bytes(d_one, want)
    assert i_ab.reached_voxels == i_one.reached_voxels and i_ab.free_voxels == i_one.free_voxels
    # a repair with nothing closed changes nothing
    d_same, _, i_same = pkg.frontend_field_repair_host(fr.table_from_free(free_ab), goal, N_ATT, d_ab)
    assert fr.same_bytes(d_same, want) and i_same.reset_voxels == 0 and math.isinf(i_same.tau)


def test_symbols_struct_mirror_and_argument_errors(pkg, product_lib, tmp_path):
    import ctypes as C
    capi = pkg.capi
    for n in ("isdf_frontend_field_set_repair", "isdf_frontend_field_repair_info", "isdf_frontend_field_repair_sizes", "isdf_frontend_field_repair_host"):
        assert n in capi.EXPORTED_SYMBOLS and hasattr(product_lib, n)
    assert hasattr(pkg.Engine, "frontend_field_set_repair") and hasattr(pkg.Engine, "frontend_field_repair_info")
    S = capi.IsdfFieldRepairInfo
    lines = ['printf("%zu\\n", sizeof(isdf_field_repair_info));'] + [f'printf("%zu\\n", offsetof(isdf_field_repair_info, {f}));' for f, _ in S._fields_]
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"isdf_accel.h\"\nint main(void) {\n" + "\n".join(lines) + "\nreturn 0; }\n"
    p = tmp_path / "t.c"
    p.write_text(src)
    exe = str(tmp_path / "t")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(p), "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    assert got == [C.sizeof(S)] + [getattr(S, f).offset for f, _ in S._fields_]
    sz = (C.c_int * 1)()
    product_lib.isdf_frontend_field_repair_sizes(sz)
    assert sz[0] == C.sizeof(S)
    product_lib.isdf_frontend_field_repair_sizes(None)         # null-safe
    # no ctx: argument errors, never a crash
    assert product_lib.isdf_frontend_field_set_repair(None, 1) == capi.ISDF_ERR_INVALID_ARG
    assert product_lib.isdf_frontend_field_repair_info(None, None) == capi.ISDF_ERR_INVALID_ARG
    assert product_lib.isdf_frontend_field_repair_host(None, None, 9, None, None, None) == capi.ISDF_ERR_INVALID_ARG
    with pytest.raises(ValueError):
        pkg.frontend_field_repair_host(np.zeros((4, 3, 2, 4), dtype=np.uint32), (0, 0, 0), N_ATT, np.zeros((4, 3, 3)))


HOST_PROGRAM = r'''
#include "frontend_field_host.hpp"
#include <cstdio>
#include <cstring>
#include <vector>
using namespace isdf_host;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); return 1; } } while (0)
static std::vector<uint32_t> table(const std::vector<unsigned char> &free_) {
    std::vector<uint32_t> t(free_.size() * 4, 0u);
    for (size_t v = 0; v < free_.size(); v++) if (free_[v]) t[4 * v + (v % 4)] = 1u << (v % 32);
    return t;
}
static int repair_against_scratch(std::vector<unsigned char> fr, int X, int Y, int Z, const int goal[3], const std::vector<size_t> &close, bool want_reachable) {
    const size_t n = fr.size();
    std::vector<double> d(n), scratch(n);
    CHECK(field_dijkstra(table(fr).data(), X, Y, Z, 121, goal, d.data()));
    long long reached_before = 0;
    for (size_t v = 0; v < n; v++) reached_before += d[v] < 1e300;
    for (size_t v : close) { CHECK(fr[v]); fr[v] = 0; }
    const std::vector<uint32_t> t2 = table(fr);
    FieldRepairCounts C;
    CHECK(field_repair(t2.data(), X, Y, Z, 121, goal, d.data(), &C) == want_reachable);
    CHECK(field_dijkstra(t2.data(), X, Y, Z, 121, goal, scratch.data()) == want_reachable);
    CHECK(std::memcmp(d.data(), scratch.data(), n * sizeof(double)) == 0);
    CHECK(C.closed_reached == (long long)close.size());
    if (want_reachable) CHECK(C.reset_voxels > 0 && C.reset_voxels < reached_before);
    else CHECK(C.tau == 0.0 && C.reset_voxels == reached_before && C.reached_voxels == 0);
    CHECK(field_repair(t2.data(), X, Y, Z, 121, goal, d.data(), nullptr) == want_reachable);        // again, nothing closed, no counts
    CHECK(std::memcmp(d.data(), scratch.data(), n * sizeof(double)) == 0);
    return 0;
}
int main() {
    const int X = 24, Y = 24, Z = 3;
    std::vector<unsigned char> fr((size_t)X * Y * Z, 1);
    for (int y = 1; y < Y; y += 2)
        for (int x = 0; x < X; x++)
            for (int z = 0; z < Z; z++) fr[((size_t)x * Y + y) * Z + z] = (x == ((y / 2) % 2 == 0 ? X - 1 : 0)) ? 1 : 0;
    const int goal[3] = {0, 0, 1};
    if (repair_against_scratch(fr, X, Y, Z, goal, {((size_t)12 * Y + 12) * Z + 1}, true)) return 1;
    if (repair_against_scratch(fr, X, Y, Z, goal, {((size_t)0 * Y + 0) * Z + 1}, false)) return 1;
    std::printf("ok\n");
    return 0;
}
'''


def test_host_repair_under_sanitizers(tmp_path):
    """The serpentine half-way case and the goal-closed case in a stand-alone program under AddressSanitizer and UBSan; nothing of it runs
    in the Python process."""
    p = tmp_path / "repair.cpp"
    p.write_text(HOST_PROGRAM)
    exe = str(tmp_path / "repair")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                           "-I", CSRC, str(p), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:]
