"""Host side of the trajectory clearance check (isdf_traj_check*, isdf_traj_collide): what needs no device - the parameter
defaults, the argument checks that come before the ctx is looked at, and the struct layouts against the header."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_traj_check_params_defaults(pkg, product_lib):
    capi = pkg.capi
    p = capi.IsdfTrajCheckParams()
    p.margin = 3.0; p.mode = 7; p.reserved = 9
    product_lib.isdf_traj_check_params_default(C.byref(p))
    # negative margin = cfg.safety_hor of the ctx the check runs on; the collision term's own query
    assert (p.margin, p.mode, p.reserved) == (-1.0, capi.SWEPT_FIELD_PLANNER, 0)
    product_lib.isdf_traj_check_params_default(None)        # tolerated


def test_traj_check_bad_arguments_are_refused_without_a_device(pkg, product_lib):
    capi = pkg.capi
    dp = C.POINTER(C.c_double)
    T = np.array([1.0, 1.5]); Cc = np.zeros(36)
    pT, pC = T.ctypes.data_as(dp), Cc.ctypes.data_as(dp)
    L = product_lib
    info = capi.IsdfTrajCheckInfo()
    p = capi.IsdfTrajCheckParams()
    L.isdf_traj_check_params_default(C.byref(p))
    # NULL ctx
    assert L.isdf_traj_check(None, 2, pT, pC, C.byref(p), C.byref(info), None) == capi.ISDF_ERR_INVALID_ARG
    assert b"ctx" in L.isdf_last_error(None)
    assert L.isdf_traj_check(None, 2, pT, pC, None, None, None) == capi.ISDF_ERR_INVALID_ARG
    assert L.isdf_traj_check_device(None, 2, C.c_void_p(8), C.c_void_p(8), None, None, None, None) == capi.ISDF_ERR_INVALID_ARG
    assert b"ctx" in L.isdf_last_error(None)
    assert L.isdf_traj_check_get(None, None, 0) == capi.ISDF_ERR_INVALID_ARG
    assert L.isdf_traj_check_release(None) == capi.ISDF_ERR_INVALID_ARG
    assert L.isdf_traj_collide(None, 2, pT, pC) == capi.ISDF_ERR_INVALID_ARG
    # the arguments are checked before the ctx: the message names what is wrong
    for args in ((2, None, pC), (2, pT, None), (0, pT, pC), (-3, pT, pC)):
        assert L.isdf_traj_check(None, args[0], args[1], args[2], C.byref(p), C.byref(info), None) == capi.ISDF_ERR_INVALID_ARG
        assert b"trajectory" in L.isdf_last_error(None)
        assert L.isdf_traj_collide(None, *args) == capi.ISDF_ERR_INVALID_ARG
    assert L.isdf_traj_check_device(None, 2, None, None, None, None, None, None) == capi.ISDF_ERR_INVALID_ARG
    assert b"trajectory" in L.isdf_last_error(None)
    for field, value, word in (("mode", 2, b"mode"), ("mode", -1, b"mode"), ("margin", float("nan"), b"margin"),
                               ("margin", float("inf"), b"margin")):
        q = capi.IsdfTrajCheckParams()
        L.isdf_traj_check_params_default(C.byref(q))
        setattr(q, field, value)
        assert L.isdf_traj_check(None, 2, pT, pC, C.byref(q), C.byref(info), None) == capi.ISDF_ERR_INVALID_ARG, field
        assert word in L.isdf_last_error(None), (field, L.isdf_last_error(None))
        assert L.isdf_traj_check_device(None, 2, C.c_void_p(8), C.c_void_p(8), C.byref(q), None, None, None) == capi.ISDF_ERR_INVALID_ARG
        assert word in L.isdf_last_error(None)


def test_traj_check_struct_layouts_match_header(pkg):
    info_fields = ["occupied_in_box", "candidates", "qualified", "n_below_margin", "n_penetrating", "min_clearance", "min_tstar",
                   "min_point", "min_voxel", "min_piece", "culled", "margin", "far_r", "select_ms", "field_ms", "reduce_ms"]
    offs = ", ".join(f"offsetof(isdf_traj_check_info, {f})" for f in info_fields)
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "isdf_accel.h"
    int main(void) {
      size_t o[] = {%s};
      printf("%%zu %%zu\n", sizeof(isdf_traj_check_params), sizeof(isdf_traj_check_info));
      printf("%%zu %%zu %%zu\n", offsetof(isdf_traj_check_params, margin), offsetof(isdf_traj_check_params, mode),
             offsetof(isdf_traj_check_params, reserved));
      for (size_t i = 0; i < sizeof(o) / sizeof(o[0]); i++) printf("%%zu ", o[i]);
      printf("\n%%zu %%zu %%zu %%zu %%zu\n", sizeof(isdf_config), sizeof(isdf_shape), sizeof(isdf_stats), sizeof(isdf_swept_mesh_params),
             sizeof(isdf_swept_mesh_info));
      return 0; }''' % offs
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "t.c")
        open(p, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), p, "-o", exe])
        out = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    capi = pkg.capi
    P, I = capi.IsdfTrajCheckParams, capi.IsdfTrajCheckInfo
    assert [name for name, _ in I._fields_] == info_fields
    assert out[0:2] == [C.sizeof(P), C.sizeof(I)]
    assert out[2:5] == [P.margin.offset, P.mode.offset, P.reserved.offset]
    assert out[5:5 + len(info_fields)] == [getattr(I, f).offset for f in info_fields]
    # the existing ABI is unchanged
    assert out[5 + len(info_fields):] == [C.sizeof(capi.IsdfConfig), C.sizeof(capi.IsdfShape), C.sizeof(capi.IsdfStats),
                                          C.sizeof(capi.IsdfSweptMeshParams), C.sizeof(capi.IsdfSweptMeshInfo)]


def test_traj_check_entry_points_are_exported(pkg, product_lib):
    names = ["isdf_traj_check_params_default", "isdf_traj_check", "isdf_traj_check_device", "isdf_traj_check_get",
             "isdf_traj_check_release", "isdf_traj_collide"]
    for n in names:
        assert n in pkg.capi.EXPORTED_SYMBOLS and hasattr(product_lib, n)
    assert hasattr(pkg.Engine, "traj_check") and hasattr(pkg.Engine, "traj_check_points") and hasattr(pkg.Engine, "traj_collide")
