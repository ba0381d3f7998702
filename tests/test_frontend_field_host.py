"""isdf_frontend_field_host (csrc/frontend_field_host.hpp): the cost-to-go field of one goal over the front end's free graph in plain host
code, against the tests' own reference (tests/field_reference.py, written from the definition) BIT FOR BIT - every relaxation order
reaches the same bytes, so there is no tolerance - and, as a stand-alone program, under the sanitizers.  No device."""
import math
import os
import subprocess

import numpy as np
import pytest

import field_reference as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "implicit-sdf-planner_amd", "csrc")

CASES = {
    "open": (fr.open_map(), (1, 5, 3)),
    "wall_with_gap": (fr.wall_with_gap(), (0, 0, 0)),
    "sealed_pocket": (fr.sealed_pocket(), (0, 0, 0)),
    "goal_not_free": (fr.sealed_pocket(), (3, 1, 0)),
    "serpentine": (fr.serpentine((20, 20, 3)), (0, 0, 1)),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_form_equals_the_reference_bit_for_bit(pkg, product_lib, name):
    occ, goal = CASES[name]
    free = occ == 0
    want = fr.field(free, goal)
    d, reachable = pkg.frontend_field_host(fr.table_from_free(free), goal, 121)
    assert fr.same_bytes(d, want), name
    assert reachable == bool(free[goal])
    assert np.isinf(d[~free]).all()
    if name == "sealed_pocket":
        assert np.isinf(d[4:7, 2:5, 1:4]).all() and np.isfinite(d[free]).sum() == free.sum() - 27
    if name == "goal_not_free":
        assert np.isinf(d).all()
    if name in ("open", "wall_with_gap", "serpentine"):
        assert np.isfinite(d[free]).all() and d[goal] == 0.0
    if name == "serpentine":
        assert d.max() > 9 * 19.0                     # the corridor's length, not the straight line


def test_goal_outside_the_map_and_argument_errors(pkg, product_lib):
    free = np.ones((4, 3, 2), dtype=bool)
    for goal in ((4, 0, 0), (0, -1, 0), (0, 0, 2)):
        d, reachable = pkg.frontend_field_host(fr.table_from_free(free), goal, 121)
        assert not reachable and np.isinf(d).all()
    with pytest.raises(ValueError):
        pkg.frontend_field_host(np.zeros((4, 3, 2, 8), dtype=np.uint32), (0, 0, 0), 121)
    assert product_lib.isdf_frontend_field_host(None, None, 9, None, None) == pkg.capi.ISDF_ERR_INVALID_ARG
    # one attitude word more than 128 attitudes: any bit of any of the 8 dwords
    t = np.zeros((4, 3, 2, 8), dtype=np.uint32)
    t[..., 7] = 1
    t[2, 1, 1, :] = 0
    d, reachable = pkg.frontend_field_host(t, (0, 0, 0), 200)
    want = np.ones((4, 3, 2), dtype=bool); want[2, 1, 1] = False
    assert reachable and fr.same_bytes(d, fr.field(want, (0, 0, 0)))


def test_open_map_closed_form(pkg, product_lib):
    """In an open map a shortest path takes dmin space diagonals, dmid - dmin face diagonals and dmax - dmid straight steps.  The closed
    form sums in another order than the path does: at most about 30 additions (and three products) of 2^-53 relative error each, held to 1e-12."""
    occ, goal = CASES["open"]
    d, _ = pkg.frontend_field_host(fr.table_from_free(occ == 0), goal, 121)
    for x in range(9):
        for y in range(7):
            for z in range(5):
                a = sorted((abs(x - goal[0]), abs(y - goal[1]), abs(z - goal[2])))
                want = math.sqrt(3.0) * a[0] + math.sqrt(2.0) * (a[1] - a[0]) + (a[2] - a[1])
                assert abs(d[x, y, z] - want) <= 1e-12 * max(want, 1.0), (x, y, z)


def test_struct_mirrors_and_defaults(pkg, product_lib, tmp_path):
    import ctypes as C
    capi = pkg.capi
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "isdf_accel.h"
    int main(void) {
      printf("%zu %zu %zu %zu %zu %zu\n", sizeof(isdf_frontend_field_params), sizeof(isdf_frontend_field_info), offsetof(isdf_frontend_field_info, bricks),
             offsetof(isdf_frontend_field_info, brick_visits), offsetof(isdf_frontend_field_info, reached_voxels), offsetof(isdf_frontend_field_info, device_ms));
      return 0; }'''
    p = tmp_path / "t.c"
    p.write_text(src)
    exe = str(tmp_path / "t")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(p), "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    I = capi.IsdfFrontendFieldInfo
    assert got == [C.sizeof(capi.IsdfFrontendFieldParams), C.sizeof(I), I.bricks.offset, I.brick_visits.offset, I.reached_voxels.offset, I.device_ms.offset]
    prm = capi.IsdfFrontendFieldParams(); prm.max_rounds = 7
    product_lib.isdf_frontend_field_params_default(C.byref(prm))
    assert prm.max_rounds == 0
    # no ctx: argument errors, never a crash
    assert product_lib.isdf_frontend_field_build(None, None, None, None) == capi.ISDF_ERR_INVALID_ARG
    assert product_lib.isdf_frontend_field_paths(None, None, 1, 1, None, None, None) == capi.ISDF_ERR_INVALID_ARG
    assert product_lib.isdf_frontend_field_release(None) == capi.ISDF_ERR_INVALID_ARG


def test_sanitizer_program(tmp_path):
    """frontend_field_host.hpp as a stand-alone program under AddressSanitizer and UBSan on the same maps (open, goal outside, wall with a gap,
    sealed pocket from outside and inside, goal not free, serpentine); nothing of it runs in the Python process."""
    exe = str(tmp_path / "frontend_field_sanitize")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
                           "-I", CSRC, os.path.join(ROOT, "tests", "native", "frontend_field_sanitize_main.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert r.stdout.count(" ok: ") == 7 and "FAILED" not in r.stdout and "all ok" in r.stdout, r.stdout
    print("\n" + r.stdout)
