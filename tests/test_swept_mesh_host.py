"""Host side of the swept-volume field and mesh (isdf_swept_sdf*, isdf_swept_mesh_*, isdf_write_obj): what needs no device -
the .obj writer against the reader, the parameter defaults, argument checks and the struct layouts against the header."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_write_obj_read_obj_round_trip_is_exact(pkg, product_lib, tmp_path):
    rng = np.random.default_rng(7)
    V = rng.normal(0, 3, (9, 3))
    V[0] = (1e-300, -0.0, 123456789.123456789)
    V[1] = (np.nextafter(1.0, 2.0), np.pi, -np.e)
    F = np.array([[0, 1, 2], [2, 3, 4], [4, 5, 6], [6, 7, 8], [8, 0, 3]], dtype=np.int32)
    path = str(tmp_path / "m.obj")
    pkg.write_obj(path, V, F)
    V2, F2 = pkg.fixtures.read_obj(path)
    assert V2.shape == V.shape and F2.shape == F.shape
    assert np.array_equal(V2.view(np.uint64), V.view(np.uint64))     # bit for bit (the sign of -0.0 included)
    assert np.array_equal(F2, F)
    # an empty mesh and an index out of range
    pkg.write_obj(str(tmp_path / "e.obj"), np.zeros((0, 3)), np.zeros((0, 3), np.int32))
    assert open(str(tmp_path / "e.obj")).read() == ""
    Fb = F.copy(); Fb[1, 1] = 9
    rc = product_lib.isdf_write_obj(path.encode(), V.ctypes.data_as(C.POINTER(C.c_double)), 9, Fb.ctypes.data_as(C.POINTER(C.c_int32)), 5)
    assert rc == pkg.capi.ISDF_ERR_INVALID_ARG


def test_mesh_params_defaults(pkg, product_lib):
    capi = pkg.capi
    p = capi.IsdfSweptMeshParams()
    p.eps = -5.0; p.band = 99; p.use_bbox = 7
    product_lib.isdf_swept_mesh_params_default(C.byref(p))
    assert (p.eps, p.iso, p.mode, p.band, p.lipschitz, p.use_bbox) == (0.1, 0.0, capi.SWEPT_FIELD_CLOSED, 4, 1.0, 0)
    assert list(p.bmin) == [0, 0, 0] and list(p.bmax) == [0, 0, 0]
    assert (capi.SWEPT_FIELD_PLANNER, capi.SWEPT_FIELD_CLOSED) == (0, 1)


def test_bad_arguments_are_refused_without_a_device(pkg, product_lib):
    capi = pkg.capi
    dp = C.POINTER(C.c_double)
    T = np.array([1.0, 1.5]); Cc = np.zeros(36)
    pT, pC = T.ctypes.data_as(dp), Cc.ctypes.data_as(dp)
    xyz = np.zeros(3); val = np.zeros(1)
    L = product_lib
    # NULL ctx
    assert L.isdf_swept_sdf(None, 2, pT, pC, xyz.ctypes.data_as(dp), 1, 0, val.ctypes.data_as(dp), None) == capi.ISDF_ERR_INVALID_ARG
    assert L.isdf_swept_sdf_device(None, 2, None, None, None, 1, 0, None, None, None) == capi.ISDF_ERR_INVALID_ARG
    assert L.isdf_swept_mesh_get(None, None, 0, None, 0) == capi.ISDF_ERR_INVALID_ARG
    assert L.isdf_swept_mesh_release(None) == capi.ISDF_ERR_INVALID_ARG
    p = capi.IsdfSweptMeshParams()
    L.isdf_swept_mesh_params_default(C.byref(p))
    assert L.isdf_swept_mesh_build(None, 2, pT, pC, C.byref(p), None) == capi.ISDF_ERR_INVALID_ARG
    assert b"ctx" in L.isdf_last_error(None)
    # the arguments are checked before the ctx: the message names what is wrong
    assert L.isdf_swept_mesh_build(None, 2, None, pC, C.byref(p), None) == capi.ISDF_ERR_INVALID_ARG
    assert b"trajectory" in L.isdf_last_error(None)
    assert L.isdf_swept_mesh_build(None, 0, pT, pC, C.byref(p), None) == capi.ISDF_ERR_INVALID_ARG
    assert L.isdf_swept_mesh_build(None, 2, pT, pC, None, None) == capi.ISDF_ERR_INVALID_ARG
    for field, value, word in (("eps", 0.0, b"eps"), ("eps", -0.1, b"eps"), ("eps", float("nan"), b"eps"), ("mode", 2, b"mode"),
                               ("mode", -1, b"mode"), ("band", -1, b"band"), ("iso", -0.5, b"iso"), ("lipschitz", 0.0, b"lipschitz")):
        q = capi.IsdfSweptMeshParams()
        L.isdf_swept_mesh_params_default(C.byref(q))
        setattr(q, field, value)
        assert L.isdf_swept_mesh_build(None, 2, pT, pC, C.byref(q), None) == capi.ISDF_ERR_INVALID_ARG, field
        assert word in L.isdf_last_error(None), (field, L.isdf_last_error(None))
    q = capi.IsdfSweptMeshParams()
    L.isdf_swept_mesh_params_default(C.byref(q))
    q.use_bbox = 1; q.bmin[0] = 1.0; q.bmax[0] = 0.0
    assert L.isdf_swept_mesh_build(None, 2, pT, pC, C.byref(q), None) == capi.ISDF_ERR_INVALID_ARG
    assert b"bbox" in L.isdf_last_error(None)
    # isdf_lattice_mesh_build: the same order - arguments, then the ctx
    dims = (C.c_int32 * 3)(3, 4, 5)
    org = np.zeros(3); f = np.zeros(60)
    pO, pF = org.ctypes.data_as(dp), f.ctypes.data_as(dp)
    assert L.isdf_lattice_mesh_build(None, dims, pO, 0.1, 0.0, pF, None) == capi.ISDF_ERR_INVALID_ARG
    assert b"ctx" in L.isdf_last_error(None)
    assert L.isdf_lattice_mesh_build(None, dims, pO, 0.1, -0.5, pF, None) == capi.ISDF_ERR_INVALID_ARG
    assert b"ctx" in L.isdf_last_error(None)                   # a negative iso is allowed here
    for args, word in (((None, pO, 0.1, 0.0, pF), b"null"), ((dims, None, 0.1, 0.0, pF), b"null"), ((dims, pO, 0.1, 0.0, None), b"null"),
                       ((dims, pO, 0.0, 0.0, pF), b"eps"), ((dims, pO, -0.1, 0.0, pF), b"eps"), ((dims, pO, float("inf"), 0.0, pF), b"eps"),
                       ((dims, pO, float("nan"), 0.0, pF), b"eps"), ((dims, pO, 0.1, float("nan"), pF), b"iso"),
                       ((dims, pO, 0.1, float("inf"), pF), b"iso"), (((C.c_int32 * 3)(3, 1, 5), pO, 0.1, 0.0, pF), b"dims"),
                       (((C.c_int32 * 3)(3, 4, -5), pO, 0.1, 0.0, pF), b"dims"), (((C.c_int32 * 3)(1024, 1024, 129), pO, 0.1, 0.0, pF), b"cap"),
                       (((C.c_int32 * 3)(2 ** 30, 2 ** 30, 2 ** 30), pO, 0.1, 0.0, pF), b"cap")):
        assert L.isdf_lattice_mesh_build(None, *args, None) == capi.ISDF_ERR_INVALID_ARG, word
        assert word in L.isdf_last_error(None), (word, L.isdf_last_error(None))


def test_swept_mesh_struct_layouts_match_header(pkg):
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "isdf_accel.h"
    int main(void) {
      printf("%zu %zu\n", sizeof(isdf_swept_mesh_params), sizeof(isdf_swept_mesh_info));
      printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", offsetof(isdf_swept_mesh_params, eps), offsetof(isdf_swept_mesh_params, iso),
             offsetof(isdf_swept_mesh_params, mode), offsetof(isdf_swept_mesh_params, band), offsetof(isdf_swept_mesh_params, lipschitz),
             offsetof(isdf_swept_mesh_params, use_bbox), offsetof(isdf_swept_mesh_params, bmin), offsetof(isdf_swept_mesh_params, bmax));
      printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", offsetof(isdf_swept_mesh_info, dims), offsetof(isdf_swept_mesh_info, origin),
             offsetof(isdf_swept_mesh_info, eps), offsetof(isdf_swept_mesh_info, coarse_points), offsetof(isdf_swept_mesh_info, fine_points),
             offsetof(isdf_swept_mesh_info, band_cells), offsetof(isdf_swept_mesh_info, n_vertices), offsetof(isdf_swept_mesh_info, n_triangles),
             offsetof(isdf_swept_mesh_info, unqualified_edges), offsetof(isdf_swept_mesh_info, field_ms), offsetof(isdf_swept_mesh_info, mesh_ms));
      printf("%d %d %zu %zu %zu\n", ISDF_SWEPT_FIELD_PLANNER, ISDF_SWEPT_FIELD_CLOSED, sizeof(isdf_config), sizeof(isdf_shape), sizeof(isdf_stats));
      return 0; }'''
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "t.c")
        open(p, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), p, "-o", exe])
        out = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    capi = pkg.capi
    P, I = capi.IsdfSweptMeshParams, capi.IsdfSweptMeshInfo
    assert out[0:2] == [C.sizeof(P), C.sizeof(I)]
    assert out[2:10] == [P.eps.offset, P.iso.offset, P.mode.offset, P.band.offset, P.lipschitz.offset, P.use_bbox.offset, P.bmin.offset, P.bmax.offset]
    assert out[10:21] == [I.dims.offset, I.origin.offset, I.eps.offset, I.coarse_points.offset, I.fine_points.offset, I.band_cells.offset,
                          I.n_vertices.offset, I.n_triangles.offset, I.unqualified_edges.offset, I.field_ms.offset, I.mesh_ms.offset]
    # the existing ABI is unchanged
    assert out[21:23] == [capi.SWEPT_FIELD_PLANNER, capi.SWEPT_FIELD_CLOSED]
    assert out[23:26] == [C.sizeof(capi.IsdfConfig), C.sizeof(capi.IsdfShape), C.sizeof(capi.IsdfStats)]
