"""Host-side mirror of the reference's cost-callback plumbing over the C-ABI (include/isdf_accel.h).

``Engine`` plays the role TrajOptimizer's members play around the two sweeps
(src/planner_algorithm/include/planner_algorithm/back_end_optimizer.hpp:59-62, :386-405, :667-725):
setParam -> Engine(cfg), setGridMap -> set_grid, setEnvironment/initShape -> set_shape,
parallel_points -> set_points, and eval() == addSaftyPenaOnSweptVolumeParallel / addTimeIntPenaltyParallel
with the same ACCUMULATE semantics.  All arithmetic happens in libisdf_accel.so on the GPU; this file only
marshals numpy arrays / device pointers.  No CPU fallback exists: errors raise IsdfError.
"""
import ctypes as C
import os

import numpy as np

from . import capi

_dp = C.POINTER(C.c_double)


class IsdfError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"isdf error {code}: {msg}")
        self.code = code


def _p(a):
    return a.ctypes.data_as(_dp)


def lbfgs_params(lib, **kw):
    p = capi.IsdfLbfgsParams()
    lib.isdf_lbfgs_params_default(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise TypeError(f"unknown L-BFGS parameter {k}")
        setattr(p, k, v)
    return p


def midend_params(lib, **kw):
    p = capi.IsdfMidendParams()
    lib.isdf_midend_params_default(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise TypeError(f"unknown mid-end parameter {k}")
        setattr(p, k, v)
    return p


_lbfgs_params = lbfgs_params        # (Engine.optimize_lbfgs_checked has an argument of that name)


def lbfgs_minimize(fun, x0, lib=None, progress=None, **params):
    """Driver on an arbitrary Python callback fun(x) -> (f, g) (host only; used by the CPU tests).
    progress(x, g, fx, step, k, ls) -> truthy cancels (isdf_lbfgs_minimize_progress: the reference's lbfgs_progress_t)."""
    lib = lib or capi.load_library()
    x = np.ascontiguousarray(x0, dtype=np.float64).copy()
    n = x.size

    def tramp(_inst, xp, gp, nn):
        xv = np.ctypeslib.as_array(xp, shape=(nn,))
        f, g = fun(xv.copy())
        np.ctypeslib.as_array(gp, shape=(nn,))[:] = g
        return float(f)
    cb = capi.EVALUATE_FN(tramp)
    p = lbfgs_params(lib, **params)
    r = capi.IsdfLbfgsResult()
    if progress is None:
        rc = lib.isdf_lbfgs_minimize(cb, None, _p(x), n, C.byref(p), C.byref(r))
    else:
        def ptramp(_inst, xp, gp, fx, step, k, ls):
            return 1 if progress(np.ctypeslib.as_array(xp, shape=(n,)).copy(), np.ctypeslib.as_array(gp, shape=(n,)).copy(), fx, step, k, ls) else 0
        pcb = capi.PROGRESS_FN(ptramp)
        rc = lib.isdf_lbfgs_minimize_progress(cb, pcb, None, _p(x), n, C.byref(p), C.byref(r))
    if rc != capi.ISDF_OK:
        raise IsdfError(rc, "isdf_lbfgs_minimize")
    return x, {"f": r.f, "status": r.status, "iterations": r.iterations, "evaluations": r.evaluations, "wall_ms": r.wall_ms}


def write_obj(path, V, F, lib=None):
    """Writes a triangle mesh as Wavefront .obj (isdf_write_obj: isdf_read_obj reads the same doubles back)."""
    lib = lib or capi.load_library()
    V = np.ascontiguousarray(V, dtype=np.float64).reshape(-1, 3)
    F = np.ascontiguousarray(F, dtype=np.int32).reshape(-1, 3)
    rc = lib.isdf_write_obj(os.fsencode(path), _p(V), V.shape[0], F.ctypes.data_as(C.POINTER(C.c_int32)), F.shape[0])
    if rc != capi.ISDF_OK:
        raise IsdfError(rc, f"isdf_write_obj {path}")


def traj_limits_params(lib, samples=0, tol_t=None, max_acc=None, max_thrust=None, min_thrust=None):
    """isdf_traj_limits_params from its defaults; None keeps a default (a limit left None is not judged)."""
    p = capi.IsdfTrajLimitsParams()
    lib.isdf_traj_limits_params_default(C.byref(p))
    p.samples = int(samples)
    for name, v in (("tol_t", tol_t), ("max_acc", max_acc), ("max_thrust", max_thrust), ("min_thrust", min_thrust)):
        if v is not None:
            setattr(p, name, float(v))
    return p


def traj_limits_report(info, piece=None):
    """An isdf_traj_limits_info as a dict of numpy arrays / ints, "piece_out" (N x 12: per piece [2 ch] value, [2 ch + 1] time) next to it."""
    d = {}
    for name, _ in capi.IsdfTrajLimitsInfo._fields_:
        v = getattr(info, name)
        if name != "reserved":
            d[name] = np.array(v) if hasattr(v, "__len__") else v
    d["piece_out"] = piece
    return d


def _traj_arrays(T, coeffs_colmajor):
    T = np.ascontiguousarray(T, dtype=np.float64).reshape(-1)
    Cc = np.ascontiguousarray(coeffs_colmajor, dtype=np.float64).reshape(-1)
    if Cc.size != 18 * T.size:
        raise ValueError(f"coefficients: {Cc.size} doubles for {T.size} pieces (18 per piece)")
    return T, Cc


def _traj_batch_arrays(T, coeffs_colmajor=None):
    """B trajectories of N pieces each as T (B x N), Cc (B x 18 N; None when no coefficients are given), B, N."""
    T = np.ascontiguousarray(T, dtype=np.float64)
    if T.ndim != 2:
        raise ValueError("T must be B x N")
    B, N = T.shape
    if coeffs_colmajor is None:
        return T, None, B, N
    Cc = np.ascontiguousarray(coeffs_colmajor, dtype=np.float64).reshape(B, -1)
    if Cc.shape[1] != 18 * N:
        raise ValueError(f"coefficients: {Cc.shape[1]} doubles per trajectory for {N} pieces (18 per piece)")
    return T, Cc, B, N


def traj_limits_host(cfg, T, coeffs_colmajor, lib=None, **params):
    """isdf_traj_limits_host: the dynamic-limits report in plain host code (no ctx, no device)."""
    lib = lib or capi.load_library()
    T, Cc = _traj_arrays(T, coeffs_colmajor)
    p = traj_limits_params(lib, **params)
    info = capi.IsdfTrajLimitsInfo()
    piece = np.zeros((T.size, 12))
    rc = lib.isdf_traj_limits_host(C.byref(cfg), T.size, _p(T), _p(Cc), C.byref(p), C.byref(info), _p(piece))
    if rc != capi.ISDF_OK:
        raise IsdfError(rc, (lib.isdf_last_error(None) or b"").decode())
    return traj_limits_report(info, piece)


def traj_sample_host(cfg, T, coeffs_colmajor, t, lib=None):
    """isdf_traj_sample_host: rows pos3 | vel3 | acc3 | jer3 | quat4 | omg3 | thr at the stamps t."""
    lib = lib or capi.load_library()
    T, Cc = _traj_arrays(T, coeffs_colmajor)
    t = np.ascontiguousarray(t, dtype=np.float64).reshape(-1)
    rows = np.zeros((t.size, capi.TRAJ_SAMPLE_ROW))
    rc = lib.isdf_traj_sample_host(C.byref(cfg), T.size, _p(T), _p(Cc), t.size, _p(t), _p(rows))
    if rc != capi.ISDF_OK:
        raise IsdfError(rc, (lib.isdf_last_error(None) or b"").decode())
    return rows


def traj_retime_params(lib, s_lo=None, s_hi=None, ladder=None, rounds=None, check=False, **limits):
    """isdf_traj_retime_params from its defaults; None keeps a default.  limits: the keywords of traj_limits_params."""
    p = capi.IsdfTrajRetimeParams()
    lib.isdf_traj_retime_params_default(C.byref(p))
    for name, v, conv in (("s_lo", s_lo, float), ("s_hi", s_hi, float), ("ladder", ladder, int), ("rounds", rounds, int)):
        if v is not None:
            setattr(p, name, conv(v))
    p.check = 1 if check else 0
    p.limits = traj_limits_params(lib, **limits)
    return p


def _struct_dict(st):
    d = {}
    for name, _ in st._fields_:
        v = getattr(st, name)
        if name != "reserved":
            d[name] = np.array(v) if hasattr(v, "__len__") else v
    return d


def traj_retime_report(info, T_out=None, coeffs_out=None):
    """An isdf_traj_retime_info as a dict: its scalars, "limits" (the dict traj_limits returns, at `scale`), "check" (a dict of the
    isdf_traj_check_info fields, or None when nothing was checked), and the retimed arrays "T" and "coeffs" (None: they are on the device)."""
    d = {}
    for name, _ in capi.IsdfTrajRetimeInfo._fields_:
        if name not in ("limits", "check"):
            d[name] = getattr(info, name)
    d["limits"] = traj_limits_report(info.limits)
    d["check"] = _struct_dict(info.check) if info.checked else None
    d["T"], d["coeffs"] = T_out, coeffs_out
    return d


def traj_scale_host(T, coeffs_colmajor, s, lib=None):
    """isdf_traj_scale_host: (T * s, the coefficient of t^k divided by s^k), the bytes every form of the retiming returns for the factor s."""
    lib = lib or capi.load_library()
    T, Cc = _traj_arrays(T, coeffs_colmajor)
    To, Co = np.zeros_like(T), np.zeros_like(Cc)
    rc = lib.isdf_traj_scale_host(T.size, _p(T), _p(Cc), float(s), _p(To), _p(Co))
    if rc != capi.ISDF_OK:
        raise IsdfError(rc, (lib.isdf_last_error(None) or b"").decode())
    return To, Co


def traj_retime_host(cfg, T, coeffs_colmajor, lib=None, **params):
    """isdf_traj_retime_host: the retiming in plain host code (no ctx, no device); the dict of traj_retime_report."""
    lib = lib or capi.load_library()
    T, Cc = _traj_arrays(T, coeffs_colmajor)
    params.pop("check", None)
    p = traj_retime_params(lib, **params)
    info = capi.IsdfTrajRetimeInfo()
    To, Co = np.zeros_like(T), np.zeros_like(Cc)
    rc = lib.isdf_traj_retime_host(C.byref(cfg), T.size, _p(T), _p(Cc), C.byref(p), _p(To), _p(Co), C.byref(info))
    if rc != capi.ISDF_OK:
        raise IsdfError(rc, (lib.isdf_last_error(None) or b"").decode())
    return traj_retime_report(info, To, Co)


def traj_realloc_params(lib, rounds=None, headroom=None, f_max=None, check=False, **limits):
    """isdf_traj_realloc_params from its defaults; None keeps a default.  limits: the keywords of traj_limits_params."""
    p = capi.IsdfTrajReallocParams()
    lib.isdf_traj_realloc_params_default(C.byref(p))
    for name, v, conv in (("rounds", rounds, int), ("headroom", headroom, float), ("f_max", f_max, float)):
        if v is not None:
            setattr(p, name, conv(v))
    p.check = 1 if check else 0
    p.limits = traj_limits_params(lib, **limits)
    return p


def traj_realloc_report(info, T_out=None, coeffs_out=None):
    """An isdf_traj_realloc_info as a dict: its scalars, "limits" (the dict traj_limits returns, of the result), "check" (a dict of the
    isdf_traj_check_info fields, or None when nothing was checked), and the arrays "T" and "coeffs" (None: they are on the device)."""
    d = {}
    for name, _ in capi.IsdfTrajReallocInfo._fields_:
        if name not in ("limits", "check", "reserved"):
            d[name] = getattr(info, name)
    d["limits"] = traj_limits_report(info.limits)
    d["check"] = _struct_dict(info.check) if info.checked else None
    d["T"], d["coeffs"] = T_out, coeffs_out
    return d


def _realloc_arrays(head_pva, tail_pva, Q, T):
    """One trajectory's inputs as flat arrays: head / tail position | velocity | acceleration (9), Q (N - 1) x 3 point-major, T (N)."""
    T = np.ascontiguousarray(T, dtype=np.float64).reshape(-1)
    h = np.ascontiguousarray(head_pva, dtype=np.float64).reshape(-1)
    t = np.ascontiguousarray(tail_pva, dtype=np.float64).reshape(-1)
    q = np.zeros(3) if Q is None else np.ascontiguousarray(Q, dtype=np.float64).reshape(-1)
    if h.size != 9 or t.size != 9:
        raise ValueError("head_pva and tail_pva hold 9 doubles each: position, velocity, acceleration")
    if T.size > 1 and q.size != 3 * (T.size - 1):
        raise ValueError(f"waypoints: {q.size} doubles for {T.size} pieces (3 per inner waypoint)")
    if T.size <= 1:
        q = np.zeros(3)
    return h, t, q, T


def traj_minco_host(head_pva, tail_pva, Q, T, lib=None):
    """isdf_traj_minco_host: the MINCO (s = 3) coefficients (6N x 3 column-major, flat) through the waypoints Q with durations T."""
    lib = lib or capi.load_library()
    h, t, q, T = _realloc_arrays(head_pva, tail_pva, Q, T)
    Co = np.zeros(18 * T.size)
    rc = lib.isdf_traj_minco_host(T.size, _p(h), _p(t), _p(q), _p(T), _p(Co))
    if rc != capi.ISDF_OK:
        raise IsdfError(rc, (lib.isdf_last_error(None) or b"").decode())
    return Co


def traj_realloc_host(cfg, head_pva, tail_pva, Q, T, lib=None, **params):
    """isdf_traj_realloc_host: the per-piece re-allocation in plain host code (no ctx, no device); the dict of traj_realloc_report."""
    lib = lib or capi.load_library()
    h, t, q, T = _realloc_arrays(head_pva, tail_pva, Q, T)
    params.pop("check", None)
    p = traj_realloc_params(lib, **params)
    info = capi.IsdfTrajReallocInfo()
    To, Co = np.zeros_like(T), np.zeros(18 * T.size)
    rc = lib.isdf_traj_realloc_host(C.byref(cfg), T.size, _p(h), _p(t), _p(q), _p(T), C.byref(p), _p(To), _p(Co), C.byref(info))
    if rc != capi.ISDF_OK:
        raise IsdfError(rc, (lib.isdf_last_error(None) or b"").decode())
    return traj_realloc_report(info, To, Co)


def frontend_field_host(free_mask, goal_index, n_att, lib=None):
    """isdf_frontend_field_host: the cost-to-go field in plain host code (Dijkstra, no ctx, no device).  free_mask: uint32
    [X, Y, Z, 4 * ceil(n_att / 128)] in isdf_frontend_cspace's layout; goal_index: the goal's voxel.  Returns (d [X, Y, Z], reachable)."""
    lib = lib or capi.load_library()
    m = np.ascontiguousarray(free_mask, dtype=np.uint32)
    nw = 4 * ((int(n_att) + 127) // 128)
    if m.ndim != 4 or m.shape[3] != nw:
        raise ValueError(f"free_mask must be [X, Y, Z, {nw}]")
    dims = np.array(m.shape[:3], dtype=np.int32)
    g = np.ascontiguousarray(goal_index, dtype=np.int32).reshape(3)
    d = np.zeros(m.shape[:3])
    rc = lib.isdf_frontend_field_host(m.ctypes.data_as(C.c_void_p), dims.ctypes.data_as(C.c_void_p), int(n_att), g.ctypes.data_as(C.c_void_p), _p(d))
    if rc < 0:
        raise IsdfError(rc, "isdf_frontend_field_host: bad arguments")
    return d, bool(rc)


def frontend_field_repair_host(free_mask_new, goal_index, n_att, d, lib=None):
    """isdf_frontend_field_repair_host: the field `d` of `goal_index` (float64 [X, Y, Z], of a table of which free_mask_new is a subset:
    voxels only closed) repaired in plain host code - every d below the smallest d of a closed voxel is kept, the rest is reset and
    Dijkstra runs on from the kept voxels.  Returns (d_new [X, Y, Z], reachable, IsdfFieldRepairInfo); `d` itself is not changed."""
    lib = lib or capi.load_library()
    m = np.ascontiguousarray(free_mask_new, dtype=np.uint32)
    nw = 4 * ((int(n_att) + 127) // 128)
    if m.ndim != 4 or m.shape[3] != nw:
        raise ValueError(f"free_mask_new must be [X, Y, Z, {nw}]")
    out = np.array(d, dtype=np.float64, order="C")
    if out.shape != m.shape[:3]:
        raise ValueError(f"d must be {m.shape[:3]}")
    dims = np.array(m.shape[:3], dtype=np.int32)
    g = np.ascontiguousarray(goal_index, dtype=np.int32).reshape(3)
    info = capi.IsdfFieldRepairInfo()
    rc = lib.isdf_frontend_field_repair_host(m.ctypes.data_as(C.c_void_p), dims.ctypes.data_as(C.c_void_p), int(n_att), g.ctypes.data_as(C.c_void_p), _p(out),
                                             C.byref(info))
    if rc < 0:
        raise IsdfError(rc, "isdf_frontend_field_repair_host: bad arguments")
    return out, bool(rc), info


def frontend_field_reopen_host(free_mask_new, goal_index, n_att, d, lib=None):
    """isdf_frontend_field_reopen_host: the field `d` of `goal_index` (float64 [X, Y, Z], of a table of which free_mask_new is a superset:
    voxels only opened) lowered in plain host code - every old value is kept, an opened goal cell takes 0, and Dijkstra runs on from the
    finite neighbours of the free voxels that hold +inf.  Returns (d_new [X, Y, Z], reachable, IsdfFieldReopenInfo); `d` itself is not
    changed.  No old table is given: opened_voxels counts the voxels that were +inf and are finite now."""
    lib = lib or capi.load_library()
    m = np.ascontiguousarray(free_mask_new, dtype=np.uint32)
    nw = 4 * ((int(n_att) + 127) // 128)
    if m.ndim != 4 or m.shape[3] != nw:
        raise ValueError(f"free_mask_new must be [X, Y, Z, {nw}]")
    out = np.array(d, dtype=np.float64, order="C")
    if out.shape != m.shape[:3]:
        raise ValueError(f"d must be {m.shape[:3]}")
    dims = np.array(m.shape[:3], dtype=np.int32)
    g = np.ascontiguousarray(goal_index, dtype=np.int32).reshape(3)
    info = capi.IsdfFieldReopenInfo()
    rc = lib.isdf_frontend_field_reopen_host(m.ctypes.data_as(C.c_void_p), dims.ctypes.data_as(C.c_void_p), int(n_att), g.ctypes.data_as(C.c_void_p), _p(out),
                                             C.byref(info))
    if rc < 0:
        raise IsdfError(rc, "isdf_frontend_field_reopen_host: bad arguments")
    return out, bool(rc), info


def frontend_field_shift_host(free_mask_new, shift, goal_index_old, n_att, d, lib=None):
    """isdf_frontend_field_shift_host: the field `d` of `goal_index_old` (float64 [X, Y, Z], on the table before the shift) carried through
    a shift of the map window by `shift` in plain host code - d translated (new voxel v holds old voxel v + shift), the leaving and the
    closed voxels' threshold reset and relaxed on the translated graph, then the opened voxels relaxed on free_mask_new (the table after
    the shift).  Returns (d_new [X, Y, Z], code, IsdfFieldShiftInfo): code 1 the goal cell goal_index_old - shift is free, 0 it is not,
    capi.FIELD_SHIFT_GOAL_LEFT it lies outside the grid (all +inf); `d` itself is not changed."""
    lib = lib or capi.load_library()
    m = np.ascontiguousarray(free_mask_new, dtype=np.uint32)
    nw = 4 * ((int(n_att) + 127) // 128)
    if m.ndim != 4 or m.shape[3] != nw:
        raise ValueError(f"free_mask_new must be [X, Y, Z, {nw}]")
    out = np.array(d, dtype=np.float64, order="C")
    if out.shape != m.shape[:3]:
        raise ValueError(f"d must be {m.shape[:3]}")
    dims = np.array(m.shape[:3], dtype=np.int32)
    s = np.ascontiguousarray(shift, dtype=np.int32).reshape(3)
    g = np.ascontiguousarray(goal_index_old, dtype=np.int32).reshape(3)
    info = capi.IsdfFieldShiftInfo()
    rc = lib.isdf_frontend_field_shift_host(m.ctypes.data_as(C.c_void_p), dims.ctypes.data_as(C.c_void_p), int(n_att), s.ctypes.data_as(C.c_void_p),
                                            g.ctypes.data_as(C.c_void_p), _p(out), C.byref(info))
    if rc < 0:
        raise IsdfError(rc, "isdf_frontend_field_shift_host: bad arguments")
    return out, int(rc), info


def _scan_geometry(bmin, bmax, dims, origin):
    return (np.ascontiguousarray(bmin, dtype=np.float64).reshape(3), np.ascontiguousarray(bmax, dtype=np.float64).reshape(3),
            (C.c_int32 * 3)(*[int(v) for v in dims]), np.ascontiguousarray(origin, dtype=np.float64).reshape(3))


def scan_ray_host(bmin, bmax, res, dims, origin, end, lib=None):
    """isdf_scan_ray_host: the voxels the ray origin -> end visits, int32 [n, 3] in the order of the walk (n = 0: the end point lies
    outside the map).  Raises IsdfError on a negative status (the origin outside the map)."""
    lib = lib or capi.load_library()
    b0, b1, d, o = _scan_geometry(bmin, bmax, dims, origin)
    e = np.ascontiguousarray(end, dtype=np.float32).reshape(3)
    ep = e.ctypes.data_as(C.POINTER(C.c_float))
    n = lib.isdf_scan_ray_host(_p(b0), _p(b1), float(res), d, _p(o), ep, None, 0)
    if n < 0:
        raise IsdfError(int(n), "isdf_scan_ray_host")
    out = np.zeros((int(n), 3), dtype=np.int32)
    if n > 0:
        assert lib.isdf_scan_ray_host(_p(b0), _p(b1), float(res), d, _p(o), ep, out.ctypes.data_as(C.c_void_p), int(n)) == n
    return out


def scan_sets_host(bmin, bmax, res, dims, origin, xyz, hit=None, lib=None):
    """isdf_scan_sets_host: (free uint8 [X, Y, Z] - 1 = in F -, hits uint32 [X, Y, Z] - the multiplicity in H -, rays skipped)."""
    lib = lib or capi.load_library()
    b0, b1, d, o = _scan_geometry(bmin, bmax, dims, origin)
    pts = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
    h = None if hit is None else np.ascontiguousarray(hit, dtype=np.uint8).reshape(pts.shape[0])
    shape = tuple(int(v) for v in dims)
    free, hits = np.zeros(shape, dtype=np.uint8), np.zeros(shape, dtype=np.uint32)
    skipped = C.c_longlong(0)
    n = lib.isdf_scan_sets_host(_p(b0), _p(b1), float(res), d, _p(o), pts.ctypes.data_as(C.POINTER(C.c_float)), None if h is None else h.ctypes.data_as(C.c_void_p),
                                pts.shape[0], free.ctypes.data_as(C.c_void_p), hits.ctypes.data_as(C.c_void_p), C.byref(skipped))
    if n < 0:
        raise IsdfError(int(n), "isdf_scan_sets_host")
    assert n == int(free.sum())
    return free, hits, int(skipped.value)


def known_words(dims):
    """Words of a known grid over dims voxels: ceil(nx ny nz / 32)."""
    return (int(dims[0]) * int(dims[1]) * int(dims[2]) + 31) // 32


def known_pack(mask):
    """A boolean [X, Y, Z] array as the known grid's words (voxel a = (x * ny + y) * nz + z is bit a & 31 of word a >> 5)."""
    m = np.ascontiguousarray(mask).astype(bool).reshape(-1)
    b = np.packbits(m, bitorder="little")
    out = np.zeros(4 * known_words(np.shape(mask)), dtype=np.uint8)
    out[:b.size] = b
    return out.view("<u4").astype(np.uint32)


def known_unpack(words, dims):
    """The words of a known grid as a boolean [X, Y, Z] array."""
    n = int(dims[0]) * int(dims[1]) * int(dims[2])
    w = np.ascontiguousarray(words, dtype=np.uint32).astype("<u4").view(np.uint8)
    return np.unpackbits(w, bitorder="little")[:n].astype(bool).reshape(tuple(int(v) for v in dims))


def _known_args(bits, dims):
    d = (C.c_int32 * 3)(*[int(v) for v in dims])
    w = np.ascontiguousarray(bits, dtype=np.uint32).reshape(-1)
    if w.size != known_words(dims):
        raise ValueError(f"a known grid over {tuple(dims)} has {known_words(dims)} words")
    return w, d


def known_merge_host(bits, dims, free, hits, lib=None):
    """isdf_known_merge_host: (bits | V, bits that went from 0 to 1); free / hits as scan_sets_host returns them (either may be None)."""
    lib = lib or capi.load_library()
    w, d = _known_args(bits, dims)
    out = w.copy()
    f = None if free is None else np.ascontiguousarray(free, dtype=np.uint8)
    h = None if hits is None else np.ascontiguousarray(hits, dtype=np.uint32)
    n = lib.isdf_known_merge_host(out.ctypes.data_as(C.c_void_p), d, None if f is None else f.ctypes.data_as(C.c_void_p),
                                  None if h is None else h.ctypes.data_as(C.c_void_p))
    if n < 0:
        raise IsdfError(int(n), "isdf_known_merge_host")
    return out, int(n)


def known_shift_host(bits, dims, shift, lib=None):
    """isdf_known_shift_host: the grid translated, K'[v] = K[v + shift] where v + shift lies in the grid, else 0."""
    lib = lib or capi.load_library()
    w, d = _known_args(bits, dims)
    out = np.zeros_like(w)
    rc = lib.isdf_known_shift_host(w.ctypes.data_as(C.c_void_p), d, _i3(shift), out.ctypes.data_as(C.c_void_p))
    if rc < 0:
        raise IsdfError(rc, "isdf_known_shift_host")
    return out


def known_erode_host(bits, dims, radius, border=0, lib=None):
    """isdf_known_erode_host: the eroded known grid's words - voxel v is set when every voxel of the cube of 2 radius + 1 a side round v is
    known, a voxel outside the grid counting as `border`."""
    lib = lib or capi.load_library()
    w, d = _known_args(bits, dims)
    out = np.zeros_like(w)
    rc = lib.isdf_known_erode_host(w.ctypes.data_as(C.c_void_p), d, int(radius), int(border), out.ctypes.data_as(C.c_void_p))
    if rc < 0:
        raise IsdfError(rc, "isdf_known_erode_host")
    return out


def known_fill_host(bits, dims, box, value, lib=None):
    """isdf_known_fill_host: (the grid with the inclusive box (lo_x, lo_y, lo_z, hi_x, hi_y, hi_z) - None: all of it - set or cleared,
    bits that went from 0 to 1).  Raises IsdfError for a box outside the grid or with lo > hi."""
    lib = lib or capi.load_library()
    w, d = _known_args(bits, dims)
    out = w.copy()
    n = lib.isdf_known_fill_host(out.ctypes.data_as(C.c_void_p), d, None if box is None else (C.c_int32 * 6)(*[int(v) for v in box]), int(value))
    if n < 0:
        raise IsdfError(int(n), "isdf_known_fill_host")
    return out, int(n)


def known_frontier_host(bits, occ, capacity=None, lib=None):
    """isdf_known_frontier_host on occupancy bytes [X, Y, Z]: (frontier words, voxel indices int64 ascending, IsdfMapFrontierInfo).
    capacity: of the list (default: as many as there are); too short raises IsdfError(ISDF_ERR_OVERFLOW)."""
    lib = lib or capi.load_library()
    o = np.ascontiguousarray(occ, dtype=np.uint8)
    w, d = _known_args(bits, o.shape)
    out = np.zeros_like(w)
    info = capi.IsdfMapFrontierInfo()
    vox = np.zeros(o.size if capacity is None else int(capacity), dtype=np.int64)
    rc = lib.isdf_known_frontier_host(w.ctypes.data_as(C.c_void_p), o.ctypes.data_as(C.c_void_p), d, out.ctypes.data_as(C.c_void_p),
                                      vox.ctypes.data_as(C.c_void_p), vox.size, C.byref(info))
    if rc < 0:
        raise IsdfError(rc, "isdf_known_frontier_host")
    return out, vox[:int(info.n_frontier)], info


def _cluster_params(lib, connectivity, min_size):
    p = capi.IsdfFrontierClusterParams()
    lib.isdf_frontier_cluster_params_default(C.byref(p))
    p.connectivity, p.min_size = int(connectivity), int(min_size)
    return p


def _cluster_call(call, name):
    """the sizing call (every output NULL), then the call at exactly the sizes it reported: (vox, labels, rows, info)"""
    info = capi.IsdfFrontierClusterInfo()
    rc = call(None, None, 0, None, 0, info)
    if rc < 0:
        raise IsdfError(rc, name)
    n, r = int(info.n_voxels), int(info.n_rows)
    vox, labels, rows = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int32), np.zeros((r, capi.FRONTIER_CLUSTER_ROW), dtype=np.int64)
    if n:
        rc = call(vox.ctypes.data_as(C.c_void_p), labels.ctypes.data_as(C.c_void_p), n, rows.ctypes.data_as(C.c_void_p), r, info)
        if rc < 0:
            raise IsdfError(rc, name)
    return vox, labels, rows, info


def known_clusters_host(bits, dims, connectivity=26, min_size=1, lib=None):
    """isdf_known_clusters_host: the connected components (connectivity 6, 18 or 26) of the voxel set `bits`, a bit grid over dims in the
    known grid's layout (known_pack), in plain host code.  Returns (voxels int64 ascending, labels int32 - the row of each voxel's
    cluster, -1 where min_size dropped it -, rows int64 [n_rows, 16] = (label, size, lo xyz, hi xyz, sum xyz, rep_voxel, rep_d2,
    first_pos, 0, 0), IsdfFrontierClusterInfo)."""
    lib = lib or capi.load_library()
    w, d = _known_args(bits, dims)
    p = _cluster_params(lib, connectivity, min_size)
    return _cluster_call(lambda vox, labels, nv, rows, nr, info: lib.isdf_known_clusters_host(w.ctypes.data_as(C.c_void_p), d, C.byref(p), vox, labels, nv, rows, nr,
                                                                                              C.byref(info)), "isdf_known_clusters_host")


def cluster_points(rows, bmin, resolution, dims):
    """Of cluster rows (known_clusters_host, Engine.map_frontier_clusters) in a map of dims voxels with lower corner bmin and this
    resolution, in metres as float64: (the centroids [n, 3], (sum / size + 0.5) * resolution + bmin; the centres of the rep_voxel cells
    [n, 3] - points of the set itself, which the centroid need not be).  dims: rep_voxel is a voxel index, (x * ny + y) * nz + z."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, capi.FRONTIER_CLUSTER_ROW)
    b = np.asarray(bmin, dtype=np.float64).reshape(3)
    ny, nz = int(dims[1]), int(dims[2])
    centroid = (rows[:, 8:11] / rows[:, 1:2].astype(np.float64) + 0.5) * float(resolution) + b
    v = rows[:, 11]
    cells = np.stack([v // (ny * nz), v // nz % ny, v % nz], axis=1)
    return centroid, (cells + 0.5) * float(resolution) + b


def _raycast_params(lib, test_origin_voxel, per_ray_origin):
    p = capi.IsdfMapRaycastParams()
    lib.isdf_map_raycast_params_default(C.byref(p))
    p.test_origin_voxel = int(bool(test_origin_voxel)); p.per_ray_origin = int(bool(per_ray_origin))
    return p


def _raycast_origins(origins, n, per_ray_origin):
    o = np.ascontiguousarray(origins, dtype=np.float64)
    per_ray = (o.ndim == 2) if per_ray_origin is None else bool(per_ray_origin)
    return o.reshape((n, 3) if per_ray else (3,)), per_ray


def raycast_host(occ, bmin, bmax, res, origins, ends, test_origin_voxel=False, per_ray_origin=None, lib=None):
    """isdf_raycast_host: the rays origins -> ends (ends n x 3 float32; origins 3 doubles for all rays, or n x 3 - per_ray_origin None:
    by the array's rank) cast through the occupancy bytes occ [X, Y, Z] in plain host code.  Returns (rows int32 [n, 8] =
    (status, steps, i, j, k, axis, num, den) per ray, the number of hits).  Raises IsdfError on a negative status (a shared origin outside)."""
    lib = lib or capi.load_library()
    o8 = np.ascontiguousarray(occ, dtype=np.uint8)
    pts = np.ascontiguousarray(ends, dtype=np.float32).reshape(-1, 3)
    o, per_ray = _raycast_origins(origins, pts.shape[0], per_ray_origin)
    b0, b1, d, _ = _scan_geometry(bmin, bmax, o8.shape, np.zeros(3))
    p = _raycast_params(lib, test_origin_voxel, per_ray)
    rows = np.zeros((pts.shape[0], capi.RAYCAST_ROW), dtype=np.int32)
    n = lib.isdf_raycast_host(o8.ctypes.data_as(C.c_void_p), _p(b0), _p(b1), float(res), d, _p(o), pts.ctypes.data_as(C.POINTER(C.c_float)), pts.shape[0], C.byref(p),
                              rows.ctypes.data_as(C.c_void_p))
    if n < 0:
        raise IsdfError(int(n), "isdf_raycast_host")
    return rows, int(n)


def _raycast_ticks(p, bmin, bmax, res, dims):
    """the scan's quantisation in numpy: (ticks int64 [n, 3], inside [n]); the ticks of a point outside are 0"""
    p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
    b0, b1 = np.asarray(bmin, dtype=np.float64), np.asarray(bmax, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        inside = ((p >= b0) & (p <= b1)).all(axis=1)
        u = (np.where(inside[:, None], p, b0) - b0) / np.float64(res)
    q = np.minimum(np.floor(u * 1024.0).astype(np.int64), np.asarray(dims, dtype=np.int64) * 1024 - 1)
    return q, inside


def rows_to_points(rows, origins, ends, geometry):
    """What a cast's rows say in metres.  geometry = (bmin, bmax, res, dims).  Returns (range float64 [n], point float64 [n, 3]): the point
    at which the ray entered the voxel its walk ended in - Po + (Pe - Po) * num / den between the two tick centres, taken to world
    coordinates - and its distance from the origin's tick centre (0 for a walk that ended in its first voxel); NaN for status 2 and 3."""
    bmin, bmax, res, dims = geometry
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, capi.RAYCAST_ROW)
    n = rows.shape[0]
    o = np.asarray(origins, dtype=np.float64)
    o = np.broadcast_to(o.reshape(-1, 3), (n, 3))
    qo, _ = _raycast_ticks(o, bmin, bmax, res, dims)
    qe, _ = _raycast_ticks(np.asarray(ends, dtype=np.float32).astype(np.float64), bmin, bmax, res, dims)
    Po, Pe = (2 * qo + 1).astype(np.float64), (2 * qe + 1).astype(np.float64)
    num, den = rows[:, 6].astype(np.float64)[:, None], rows[:, 7].astype(np.float64)[:, None]
    P = Po + (Pe - Po) * num / den                    # half ticks; |Pe - Po| num < 2^48: the product is exact
    b0 = np.asarray(bmin, dtype=np.float64)
    point = b0 + P / 2048.0 * np.float64(res)
    rng = np.linalg.norm((P - Po) / 2048.0 * np.float64(res), axis=1)
    bad = rows[:, 0] >= capi.RAYCAST_END_OUTSIDE
    point[bad] = np.nan; rng[bad] = np.nan
    return rng, point


def scan_from_map(engine_or_occ, origin, ends, res=None, lib=None):
    """A range sensor simulated on a map: the scan isdf_integrate_scan would have to be given for the map to read back what the sensor
    saw.  engine_or_occ: an Engine (the casts run on the device; res: the map's resolution when the Engine did not set the map itself)
    or (occ [X, Y, Z], bmin, bmax, res) (isdf_raycast_host).  The rays
    origin -> ends (n x 3 float32) are cast; a ray that reaches its end keeps it with hit 0; a ray stopped by an occupied voxel is re-aimed
    at the middle of its own chord through that voxel (the slab test in tick coordinates in fp64, then world coordinates rounded to
    float32) and cast again: it is kept, with hit 1, only when the second cast stops at its own end voxel and that voxel is the first
    cast's.  Every other ray is dropped.  Returns (ends' float32 [m, 3], hit uint8 [m], the number of rays dropped)."""
    pts = np.ascontiguousarray(ends, dtype=np.float32).reshape(-1, 3)
    o = np.ascontiguousarray(origin, dtype=np.float64).reshape(3)
    if isinstance(engine_or_occ, Engine):
        eng = engine_or_occ
        occ, bmin, bmax = eng.get_grid(capi.GRID_OCCUPANCY)
        res = eng._map_res if res is None else float(res)
        if res is None:
            raise ValueError("scan_from_map: the Engine's map was not set through set_grid / set_pointcloud; pass res")
        cast = lambda e: eng.map_raycast(o, e)[0]
    else:
        occ, bmin, bmax, res = engine_or_occ
        cast = lambda e: raycast_host(occ, bmin, bmax, res, o, e, lib=lib)[0]
    dims = np.asarray(occ).shape
    rows = cast(pts)
    clear, hit = rows[:, 0] == capi.RAYCAST_CLEAR, rows[:, 0] == capi.RAYCAST_HIT
    # the chord of the original ray through the hit voxel, in half ticks: the voxel v spans [2048 v, 2048 (v + 1)]
    qo, _ = _raycast_ticks(o[None], bmin, bmax, res, dims)
    qe, _ = _raycast_ticks(pts[hit].astype(np.float64), bmin, bmax, res, dims)
    Po, Pe = (2 * qo + 1).astype(np.float64), (2 * qe + 1).astype(np.float64)
    d = Pe - Po
    lo = 2048.0 * rows[hit, 2:5].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (lo - Po) / d, (lo + 2048.0 - Po) / d
    par = d == 0.0                                      # parallel to the slab: the walk is inside it
    t_in = np.where(par, -np.inf, np.minimum(t0, t1)).max(axis=1)
    t_out = np.where(par, np.inf, np.maximum(t0, t1)).min(axis=1)
    t_mid = 0.5 * (np.maximum(t_in, 0.0) + np.minimum(t_out, 1.0))
    mid = (np.asarray(bmin, dtype=np.float64) + (Po + t_mid[:, None] * d) / 2048.0 * np.float64(res)).astype(np.float32)
    rows2 = cast(mid)
    q2, inside2 = _raycast_ticks(mid.astype(np.float64), bmin, bmax, res, dims)
    own = (rows2[:, 2:5] == (q2 >> 10)).all(axis=1) & inside2
    keep_hit = (rows2[:, 0] == capi.RAYCAST_HIT) & own & (rows2[:, 2:5] == rows[hit, 2:5]).all(axis=1)
    out = pts.copy()
    hit_idx = np.flatnonzero(hit)
    out[hit_idx] = mid
    keep = clear.copy()
    keep[hit_idx[keep_hit]] = True
    flag = np.zeros(len(pts), dtype=np.uint8)
    flag[hit_idx[keep_hit]] = 1
    return np.ascontiguousarray(out[keep]), np.ascontiguousarray(flag[keep]), int(len(pts) - keep.sum())


def depth_camera(width, height, fx, fy, cx, cy):
    """isdf_depth_camera"""
    return capi.IsdfDepthCamera(int(width), int(height), float(fx), float(fy), float(cx), float(cy))


def camera_from_yaml(path):
    """The reference's local_sensing/params/camera.yaml: `key: value` lines with cam_width, cam_height, cam_fx, cam_fy, cam_cx, cam_cy
    (other keys and # comments are ignored).  Returns an IsdfDepthCamera."""
    vals = {}
    with open(path) as f:
        for line in f:
            line = line.split("#", 1)[0]
            if ":" in line:
                k, v = line.split(":", 1)
                vals[k.strip()] = v.strip()
    missing = [k for k in ("cam_width", "cam_height", "cam_fx", "cam_fy", "cam_cx", "cam_cy") if k not in vals]
    if missing:
        raise ValueError(f"{path}: no {', '.join(missing)}")
    return depth_camera(int(vals["cam_width"]), int(vals["cam_height"]), *(float(vals[k]) for k in ("cam_fx", "cam_fy", "cam_cx", "cam_cy")))


def _pose12(cam2world):
    """cam2world as the ABI takes it: 12 doubles, from a 3 x 4, a 4 x 4 (the last row is dropped) or 12 values"""
    m = np.asarray(cam2world, dtype=np.float64)
    if m.shape == (4, 4):
        m = m[:3]
    return np.ascontiguousarray(m.reshape(12))


def _depth_render_params(lib, splat_m=None, min_depth_m=None, max_splat_px=None, source=None):
    p = capi.IsdfDepthRenderParams()
    lib.isdf_depth_render_params_default(C.byref(p))
    if splat_m is not None:
        p.splat_m = float(splat_m)
    if min_depth_m is not None:
        p.min_depth_m = float(min_depth_m)
    if max_splat_px is not None:
        p.max_splat_px = int(max_splat_px)
    if source is not None:
        p.source = int(source)
    return p


def _depth_rays_params(lib, stride=None, min_range_m=None, max_range_m=None, no_return_is_free=None):
    p = capi.IsdfDepthRaysParams()
    lib.isdf_depth_rays_params_default(C.byref(p))
    if stride is not None:
        p.stride_u, p.stride_v = (int(stride), int(stride)) if np.isscalar(stride) else (int(stride[0]), int(stride[1]))
    if min_range_m is not None:
        p.min_range_m = float(min_range_m)
    if max_range_m is not None:
        p.max_range_m = float(max_range_m)
    if no_return_is_free is not None:
        p.no_return_is_free = int(bool(no_return_is_free))
    return p


_DEPTH_DTYPES = {np.dtype(np.int32): capi.DEPTH_I32_MM, np.dtype(np.uint16): capi.DEPTH_U16_MM, np.dtype(np.float32): capi.DEPTH_F32_M}


def _depth_image(cam, image):
    """(contiguous image of the camera's shape, its ISDF_DEPTH_* format by dtype: int32 mm, uint16 mm, float32 m)"""
    img = np.ascontiguousarray(image)
    if img.dtype not in _DEPTH_DTYPES:
        raise ValueError("a depth image is int32 (mm), uint16 (mm) or float32 (m)")
    return img.reshape(cam.height, cam.width), _DEPTH_DTYPES[img.dtype]


def _depth_rows(lib, cam, p):
    n = lib.isdf_depth_rays_rows(C.byref(cam), C.byref(p))
    if n < 0:
        raise IsdfError(int(n), "isdf_depth_rays_rows")
    return int(n)


def depth_render_host(cam, cam2world, xyz=None, occ=None, bmin=None, res=None, lib=None, **params):
    """isdf_depth_render_host: the depth image (int32 [height, width], millimetres, 999999 = empty) of the cloud xyz (n x 3 float32), or -
    xyz None - of the centres of the occupied voxels of occ [X, Y, Z] with the map's bmin and res, in plain host code.  params: splat_m,
    min_depth_m, max_splat_px.  Returns (image, IsdfDepthRenderInfo)."""
    lib = lib or capi.load_library()
    pose = _pose12(cam2world)
    image = np.zeros((cam.height, cam.width), dtype=np.int32)
    info = capi.IsdfDepthRenderInfo()
    if xyz is not None:
        pts = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        p = _depth_render_params(lib, source=capi.DEPTH_SOURCE_CLOUD, **params)
        rc = lib.isdf_depth_render_host(C.byref(cam), _p(pose), pts.ctypes.data_as(C.c_void_p), pts.shape[0], None, None, 0.0, None, C.byref(p),
                                        image.ctypes.data_as(C.c_void_p), C.byref(info))
    else:
        o8 = np.ascontiguousarray(occ, dtype=np.uint8)
        b0 = np.ascontiguousarray(bmin, dtype=np.float64).reshape(3)
        p = _depth_render_params(lib, source=capi.DEPTH_SOURCE_MAP, **params)
        rc = lib.isdf_depth_render_host(C.byref(cam), _p(pose), None, 0, o8.ctypes.data_as(C.c_void_p), _p(b0), float(res), (C.c_int32 * 3)(*o8.shape), C.byref(p),
                                        image.ctypes.data_as(C.c_void_p), C.byref(info))
    if rc != capi.ISDF_OK:
        raise IsdfError(int(rc), "isdf_depth_render_host")
    return image, info


def depth_rays_host(cam, cam2world, image, bmin, bmax, res, dims, lib=None, **params):
    """isdf_depth_rays_host: the depth image (int32 mm, uint16 mm or float32 m, by dtype) unprojected, cut to range and clipped to the map
    (bmin, bmax, res, dims) in plain host code.  params: stride (one number or (u, v)), min_range_m, max_range_m, no_return_is_free.
    Returns (ends float32 [n, 3] - NaN rows for dropped pixels -, hit uint8 [n], IsdfDepthRaysInfo)."""
    lib = lib or capi.load_library()
    pose = _pose12(cam2world)
    img, fmt = _depth_image(cam, image)
    p = _depth_rays_params(lib, **params)
    b0, b1, d, _ = _scan_geometry(bmin, bmax, dims, np.zeros(3))
    n = _depth_rows(lib, cam, p)
    ends, hit = np.zeros((n, 3), dtype=np.float32), np.zeros(n, dtype=np.uint8)
    info = capi.IsdfDepthRaysInfo()
    rc = lib.isdf_depth_rays_host(C.byref(cam), _p(pose), img.ctypes.data_as(C.c_void_p), fmt, C.byref(p), _p(b0), _p(b1), float(res), d,
                                  ends.ctypes.data_as(C.c_void_p), hit.ctypes.data_as(C.c_void_p), C.byref(info))
    if rc < 0:
        raise IsdfError(int(rc), "isdf_depth_rays_host")
    return ends, hit, info


def look_at(eye, target, up=(0, 0, 1)):
    """The cam2world (12 doubles, rows (R | t)) of a camera at `eye` whose optical axis z points at `target`, x to the right and y down;
    `up` is the world's up (an axis parallel to it takes the world's x, or y, instead)."""
    eye, target, up = (np.asarray(v, dtype=np.float64).reshape(3) for v in (eye, target, up))
    z = target - eye
    z = z / np.linalg.norm(z)
    for ref in (up, np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0])):
        x = np.cross(z, ref)
        if np.linalg.norm(x) > 1e-9:
            break
    x = x / np.linalg.norm(x)
    y = np.cross(z, x)                  # z forward, x right: y = z x x points down when `up` is up
    return np.ascontiguousarray(np.column_stack([x, y, z, eye]).reshape(12))


def _view_gain_params(lib, stride=None, max_range_m=None, scratch_bytes=None):
    p = capi.IsdfViewGainParams()
    lib.isdf_view_gain_params_default(C.byref(p))
    if stride is not None:
        p.stride_u, p.stride_v = (int(stride), int(stride)) if np.isscalar(stride) else (int(stride[0]), int(stride[1]))
    if max_range_m is not None:
        p.max_range_m = float(max_range_m)
    if scratch_bytes is not None:
        p.scratch_bytes = int(scratch_bytes)
    return p


def _view_poses(poses):
    return np.ascontiguousarray(np.asarray(poses, dtype=np.float64).reshape(-1, 12))


def view_gain_host(bits, occ, bmin, bmax, res, cam, poses, lib=None, **params):
    """isdf_view_gain_host: per candidate pose (poses n x 12 doubles, look_at's), the unknown voxels - K = bits, a known grid's words over
    occ [X, Y, Z] - the depth camera would see through the map (bmin, bmax, res), in plain host code.  params: stride (one number or
    (u, v)), max_range_m.  Returns (rows int64 [n, 8] = (status, gain, n_rays, n_skipped, n_hits, steps_total, n_rays_unknown, 0),
    IsdfViewGainInfo - best_view -1: none scored)."""
    lib = lib or capi.load_library()
    o8 = np.ascontiguousarray(occ, dtype=np.uint8)
    w, d = _known_args(bits, o8.shape)
    b0, b1, _, _ = _scan_geometry(bmin, bmax, o8.shape, np.zeros(3))
    P = _view_poses(poses)
    p = _view_gain_params(lib, **params)
    rows = np.zeros((P.shape[0], capi.VIEW_GAIN_ROW), dtype=np.int64)
    info = capi.IsdfViewGainInfo()
    info.n_views = -1                   # a refused call leaves the info alone: that tells its -1 from "no view scored"
    rc = lib.isdf_view_gain_host(w.ctypes.data_as(C.c_void_p), o8.ctypes.data_as(C.c_void_p), _p(b0), _p(b1), float(res), d, C.byref(cam), _p(P), P.shape[0], C.byref(p),
                                 rows.ctypes.data_as(C.c_void_p), C.byref(info))
    if rc < 0 and info.n_views < 0:
        raise IsdfError(int(rc), "isdf_view_gain_host")
    assert rc == info.best_view
    return rows, info


def view_ring_offsets(radii, n_azimuth, heights):
    """Eye offsets round a target for view_candidates: for every radius r, azimuth a = 2 pi j / n_azimuth (j = 0 .. n_azimuth - 1) and
    height h the offset (r cos a, r sin a, h), float64 [len(radii) * n_azimuth * len(heights), 3], radius slowest, height fastest.  The
    C ABI takes offsets as data and does no trigonometry; this is where the caller's NumPy does it."""
    r = np.asarray(radii, dtype=np.float64).reshape(-1)
    h = np.asarray(heights, dtype=np.float64).reshape(-1)
    a = 2.0 * np.pi * np.arange(int(n_azimuth), dtype=np.float64) / float(n_azimuth)
    out = np.zeros((r.size, a.size, h.size, 3), dtype=np.float64)
    out[..., 0] = (r[:, None] * np.cos(a)[None, :])[:, :, None]
    out[..., 1] = (r[:, None] * np.sin(a)[None, :])[:, :, None]
    out[..., 2] = h[None, None, :]
    return np.ascontiguousarray(out.reshape(-1, 3))


def _view_cand_params(lib, clearance_voxels=None, k_best=None, min_gain=None, **gain):
    p = capi.IsdfViewCandidatesParams()
    lib.isdf_view_candidates_params_default(C.byref(p))
    p.gain = _view_gain_params(lib, **gain)
    if clearance_voxels is not None:
        p.clearance_voxels = int(clearance_voxels)
    if k_best is not None:
        p.k_best = int(k_best)
    if min_gain is not None:
        p.min_gain = int(min_gain)
    return p


def _view_cand_arrays(targets, offsets, k_best):
    """(targets [n, 3], offsets [m, 3], and the four outputs sized for them)"""
    t = np.ascontiguousarray(np.asarray(targets, dtype=np.float64).reshape(-1, 3))
    o = np.ascontiguousarray(np.asarray(offsets, dtype=np.float64).reshape(-1, 3))
    n = t.shape[0] * o.shape[0]
    return (t, o, np.zeros((n, capi.VIEW_CANDIDATE_ROW), dtype=np.int64), np.zeros((n, 12), dtype=np.float64), np.zeros((t.shape[0], 8), dtype=np.int64),
            np.full((t.shape[0], max(int(k_best), 0)), -1, dtype=np.int64))


def view_candidates_host(bits, occ, bmin, bmax, res, cam, targets, offsets, lib=None, **params):
    """isdf_view_candidates_host: candidate c = i * len(offsets) + k has eye = targets[i] + offsets[k]; each is tested (1 bad, 2 occupied,
    3 unknown, 4 close, 5 blocked, 0 kept) against K = bits - a known grid's words over occ [X, Y, Z] - and the map (bmin, bmax, res), the
    kept ones are posed looking at their target, scored by the view gain and ranked per target, in plain host code.  params:
    clearance_voxels, k_best, min_gain, and the view gain's stride, max_range_m.  Returns (cand int64 [n, 8] = (status, eye_voxel,
    los_steps, gain, n_hits, steps_total, n_rays_unknown, rank), poses float64 [n, 12], target rows int64 [n_targets, 8] = (n_kept, n_bad,
    n_occupied, n_unknown, n_close, n_blocked, best_candidate, best_gain), best int64 [n_targets, k_best] padded with -1,
    IsdfViewCandidatesInfo)."""
    lib = lib or capi.load_library()
    o8 = np.ascontiguousarray(occ, dtype=np.uint8)
    w, d = _known_args(bits, o8.shape)
    b0, b1, _, _ = _scan_geometry(bmin, bmax, o8.shape, np.zeros(3))
    p = _view_cand_params(lib, **params)
    t, o, cand, poses, rows, best = _view_cand_arrays(targets, offsets, p.k_best)
    info = capi.IsdfViewCandidatesInfo()
    rc = lib.isdf_view_candidates_host(w.ctypes.data_as(C.c_void_p), o8.ctypes.data_as(C.c_void_p), _p(b0), _p(b1), float(res), d, C.byref(cam),
                                       t.ctypes.data_as(C.c_void_p), t.shape[0], o.ctypes.data_as(C.c_void_p), o.shape[0], C.byref(p),
                                       cand.ctypes.data_as(C.c_void_p), poses.ctypes.data_as(C.c_void_p), rows.ctypes.data_as(C.c_void_p),
                                       best.ctypes.data_as(C.c_void_p), C.byref(info))
    if rc < 0:
        raise IsdfError(int(rc), "isdf_view_candidates_host")
    return cand, poses, rows, best, info


def _view_select_params(lib, k_select=None, min_gain=None, **gain):
    p = capi.IsdfViewSelectParams()
    lib.isdf_view_select_params_default(C.byref(p))
    p.gain = _view_gain_params(lib, **gain)
    if k_select is not None:
        p.k_select = int(k_select)
    if min_gain is not None:
        p.min_gain = int(min_gain)
    return p


def _view_select_arrays(poses, k_select, dims):
    """(poses [n, 12] and the four outputs sized for them)"""
    P = _view_poses(poses)
    return (P, np.zeros((P.shape[0], capi.VIEW_GAIN_ROW), dtype=np.int64), np.zeros((max(int(k_select), 0), capi.VIEW_SELECT_ROW), dtype=np.int64),
            np.zeros(P.shape[0], dtype=np.int64), np.zeros(known_words(dims), dtype=np.uint32))


def view_select_host(bits, occ, bmin, bmax, res, cam, poses, lib=None, **params):
    """isdf_view_select_host: the greedy coverage selection of up to k_select of the poses (n x 12 doubles, look_at's) by their joint gain -
    each round the view that sees the most voxels unknown in K = bits (a known grid's words over occ [X, Y, Z]) that no view picked so far
    sees - in plain host code.  params: k_select, min_gain, and the view gain's stride, max_range_m.  Returns (rows int64 [n, 8], the view
    gain's; select int64 [k_select, 4] = (view, marginal, cumulative, overlap), (-1, 0, 0, 0) for a round that did not happen; round int64
    [n], -1: not picked; claimed uint32 words = K | the picked views' voxels; IsdfViewSelectInfo)."""
    lib = lib or capi.load_library()
    o8 = np.ascontiguousarray(occ, dtype=np.uint8)
    w, d = _known_args(bits, o8.shape)
    b0, b1, _, _ = _scan_geometry(bmin, bmax, o8.shape, np.zeros(3))
    p = _view_select_params(lib, **params)
    P, rows, select, rnd, claimed = _view_select_arrays(poses, p.k_select, o8.shape)
    info = capi.IsdfViewSelectInfo()
    rc = lib.isdf_view_select_host(w.ctypes.data_as(C.c_void_p), o8.ctypes.data_as(C.c_void_p), _p(b0), _p(b1), float(res), d, C.byref(cam),
                                   P.ctypes.data_as(C.c_void_p), P.shape[0], C.byref(p), rows.ctypes.data_as(C.c_void_p), select.ctypes.data_as(C.c_void_p),
                                   rnd.ctypes.data_as(C.c_void_p), claimed.ctypes.data_as(C.c_void_p), C.byref(info))
    if rc < 0:
        raise IsdfError(int(rc), "isdf_view_select_host")
    return rows, select, rnd, claimed, info


def _view_route_params(lib, cost0=None, max_cost=None, path_cap=None, **select):
    p = capi.IsdfViewSelectRoutedParams()
    lib.isdf_view_select_routed_params_default(C.byref(p))
    p.select = _view_select_params(lib, **select)
    if cost0 is not None:
        p.cost0 = float(cost0)
    if max_cost is not None:
        p.max_cost = float(max_cost)
    if path_cap is not None:
        p.path_cap = int(path_cap)
    return p


def _view_route_cost(cost, n):
    """the caller's cost array as n doubles, or None"""
    if cost is None:
        return None
    c = np.ascontiguousarray(cost, dtype=np.float64).reshape(-1)
    if c.size != n:
        raise ValueError(f"cost must hold one value per pose ({n}), not {c.size}")
    return c


def view_select_routed_host(bits, occ, bmin, bmax, res, cam, poses, cost, lib=None, **params):
    """isdf_view_select_routed_host: view_select_host by utility - each round the view with the largest marginal gain per travel cost, m /
    (cost0 + cost[j]), among the scored views whose cost is finite and <= max_cost - in plain host code.  cost: one non-negative double
    or +inf per pose, in cells (frontend_field_host gives a field to read it from).  params: cost0, max_cost, and view_select_host's
    (min_gain >= 1).  Returns (rows, select, round, claimed, cost float64 [n], util float64 [k_select, 2] = (cost, utility) of each
    round's view, (0, 0) for a round that did not happen, IsdfViewSelectRoutedInfo)."""
    lib = lib or capi.load_library()
    o8 = np.ascontiguousarray(occ, dtype=np.uint8)
    w, d = _known_args(bits, o8.shape)
    b0, b1, _, _ = _scan_geometry(bmin, bmax, o8.shape, np.zeros(3))
    p = _view_route_params(lib, **params)
    P, rows, select, rnd, claimed = _view_select_arrays(poses, p.select.k_select, o8.shape)
    c = _view_route_cost(cost, P.shape[0])
    cost_out, util = np.zeros(P.shape[0]), np.zeros((max(int(p.select.k_select), 0), 2))
    info = capi.IsdfViewSelectRoutedInfo()
    rc = lib.isdf_view_select_routed_host(w.ctypes.data_as(C.c_void_p), o8.ctypes.data_as(C.c_void_p), _p(b0), _p(b1), float(res), d, C.byref(cam),
                                          P.ctypes.data_as(C.c_void_p), P.shape[0], None if c is None else c.ctypes.data_as(C.c_void_p), C.byref(p),
                                          rows.ctypes.data_as(C.c_void_p), select.ctypes.data_as(C.c_void_p), rnd.ctypes.data_as(C.c_void_p),
                                          claimed.ctypes.data_as(C.c_void_p), cost_out.ctypes.data_as(C.c_void_p), util.ctypes.data_as(C.c_void_p), C.byref(info))
    if rc < 0:
        raise IsdfError(int(rc), "isdf_view_select_routed_host")
    return rows, select, rnd, claimed, cost_out, util, info


def _traj_check_info_from(d):
    info = capi.IsdfTrajCheckInfo()
    for name, _ in capi.IsdfTrajCheckInfo._fields_:
        if name == "min_point":
            for q in range(3):
                info.min_point[q] = float(d[name][q])
        elif name in d:
            setattr(info, name, d[name])
    return info


def traj_check_fold_host(a, rows_a, vox_a, b, rows_b, vox_b, lib=None):
    """isdf_traj_check_fold_host: see Engine.traj_check_fold_host.  Raises ValueError on a negative status."""
    lib = lib or capi.load_library()
    ia, ib, out = _traj_check_info_from(a), _traj_check_info_from(b), capi.IsdfTrajCheckInfo()
    pa, pb = a.get("piece_min"), b.get("piece_min")
    N = len(pa) if pa is not None else (len(pb) if pb is not None else 1)
    pa = None if pa is None else np.ascontiguousarray(pa, dtype=np.float64)
    pb = None if pb is None else np.ascontiguousarray(pb, dtype=np.float64)
    ra = np.ascontiguousarray(rows_a, dtype=np.float64).reshape(-1, 5); rb = np.ascontiguousarray(rows_b, dtype=np.float64).reshape(-1, 5)
    va = np.ascontiguousarray(vox_a, dtype=np.int64).reshape(-1); vb = np.ascontiguousarray(vox_b, dtype=np.int64).reshape(-1)
    n = ra.shape[0] + rb.shape[0]
    rows = np.zeros((n, 5)); vox = np.zeros(n, dtype=np.int64); pm = np.zeros(N)
    rc = lib.isdf_traj_check_fold_host(N, C.byref(ia), None if pa is None else _p(pa), _p(ra), va.ctypes.data_as(C.c_void_p),
                                       C.byref(ib), None if pb is None else _p(pb), _p(rb), vb.ctypes.data_as(C.c_void_p),
                                       C.byref(out), _p(pm), _p(rows), vox.ctypes.data_as(C.c_void_p), n)
    if rc != 0:
        raise ValueError(f"isdf_traj_check_fold_host: status {rc}")
    return Engine._traj_check_report(out, pm), rows, vox


def _i3(v):
    return (C.c_int32 * 3)(*[int(x) for x in v])


def shift_geometry_host(bmin, bmax, res, dims, shift, lib=None):
    """isdf_shift_geometry_host: (bmin', bmax') of the window shifted by `shift` voxels.  Raises IsdfError (ISDF_ERR_INVALID_ARG) when
    isdf_set_pointcloud's ceil((bmax' - bmin') / res) would not give dims again."""
    lib = lib or capi.load_library()
    b0, b1 = np.ascontiguousarray(bmin, dtype=np.float64).reshape(3), np.ascontiguousarray(bmax, dtype=np.float64).reshape(3)
    o0, o1 = np.zeros(3), np.zeros(3)
    rc = lib.isdf_shift_geometry_host(_p(b0), _p(b1), float(res), _i3(dims), _i3(shift), _p(o0), _p(o1))
    if rc != capi.ISDF_OK:
        raise IsdfError(rc, "isdf_shift_geometry_host")
    return o0, o1


def shift_grid_host(grid, shift, lib=None):
    """isdf_shift_grid_host: out[v] = grid[v + shift], zero where v + shift lies outside.  grid: [X, Y, Z] or [X, Y, Z, m] (one element =
    the m values of a voxel), any dtype."""
    lib = lib or capi.load_library()
    g = np.ascontiguousarray(grid)
    assert g.ndim in (3, 4)
    elem = g.itemsize * (g.shape[3] if g.ndim == 4 else 1)
    out = np.empty_like(g)
    rc = lib.isdf_shift_grid_host(g.ctypes.data_as(C.c_void_p), elem, _i3(g.shape[:3]), _i3(shift), out.ctypes.data_as(C.c_void_p))
    if rc != capi.ISDF_OK:
        raise IsdfError(rc, "isdf_shift_grid_host")
    return out


def shift_bands_host(dims, shift, side, lib=None):
    """isdf_shift_bands_host: the bands of the configuration space a shift recomputes, int32 [n, 2, 3] = (lo, hi) inclusive, n <= 6."""
    lib = lib or capi.load_library()
    boxes = np.zeros((6, 6), dtype=np.int32)
    n = C.c_int(0)
    rc = lib.isdf_shift_bands_host(_i3(dims), _i3(shift), int(side), boxes.ctypes.data_as(C.c_void_p), C.byref(n))
    if rc != capi.ISDF_OK:
        raise IsdfError(rc, "isdf_shift_bands_host")
    return boxes[:n.value].reshape(-1, 2, 3).copy()


class Engine:
    def __init__(self, cfg, lib=None, devices=None):
        """devices: None = one device (cfg.device); a list = ONE ctx over those devices (isdf_create_multi), used like any other."""
        self.lib = lib or capi.load_library()
        self.cfg = cfg
        h = C.c_void_p()
        if devices is None:
            rc = self.lib.isdf_create(C.byref(h), C.byref(cfg))
        else:
            dv = (C.c_int * len(devices))(*[int(d) for d in devices])
            rc = self.lib.isdf_create_multi(C.byref(h), C.byref(cfg), dv, len(devices))
        if rc != capi.ISDF_OK:
            msg = self.lib.isdf_last_error(None)
            raise IsdfError(rc, (msg or b"").decode())
        self.h = h
        self._keep = []
        self._map_res = None            # the resolution set_grid / set_pointcloud gave (scan_from_map: the ABI has no getter for it)

    def close(self):
        if getattr(self, "h", None):
            self.lib.isdf_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != capi.ISDF_OK:
            msg = self.lib.isdf_last_error(self.h)
            raise IsdfError(rc, (msg or b"").decode())

    # ---- once-per-plan state
    def set_grid(self, vox, origin, res, kind, bmax=None):
        dt = {np.dtype(np.uint8): capi.U8, np.dtype(np.float32): capi.F32, np.dtype(np.float64): capi.F64}
        vox = np.ascontiguousarray(vox)
        o = np.asarray(origin, dtype=np.float64)
        bm = None if bmax is None else np.asarray(bmax, dtype=np.float64)
        self._check(self.lib.isdf_set_grid(self.h, vox.ctypes.data_as(C.c_void_p), dt[vox.dtype], vox.shape[0],
                                           vox.shape[1], vox.shape[2], _p(o), None if bm is None else _p(bm),
                                           float(res), kind))
        self._map_res = float(res)

    def set_shape(self, shape):
        self._keep.append(shape)
        self._check(self.lib.isdf_set_shape(self.h, C.byref(shape)))

    def set_shape_grid(self, cells, grid_min, nres, bound_radius=0.0, bbox=None):
        """ISDF_SHAPE_GRID: cells [nx, ny, nz, 4] = (unit gradient xyz, distance) per lattice node (BasicShape::num_sdf_map)."""
        cells = np.ascontiguousarray(cells, dtype=np.float64)
        nx, ny, nz, four = cells.shape
        assert four == 4
        gm = np.ascontiguousarray(grid_min, dtype=np.float64)
        bc = bh = None
        if bbox is not None:
            bc = np.ascontiguousarray(bbox[0], dtype=np.float64); bh = np.ascontiguousarray(bbox[1], dtype=np.float64)
        self._check(self.lib.isdf_set_shape_grid(self.h, _p(cells), nx, ny, nz, _p(gm), float(nres), float(bound_radius),
                                                 None if bc is None else _p(bc), None if bh is None else _p(bh)))

    def set_shape_program(self, program, trans=None, rotate=None, bound_radius=0.0, bbox=None):
        """ISDF_SHAPE_PROGRAM: a composition from the reference's CSG op library.  program: a csg expression tree (compiled
        here) or an instruction array from csg.compile(); trans / rotate: the body offset (p - trans) * Rotate; bbox = (centre, half)."""
        from . import csg
        instr = csg.compile(program) if isinstance(program, csg.Node) else program
        tr = None if trans is None else np.ascontiguousarray(trans, dtype=np.float64).reshape(3)
        ro = None if rotate is None else np.ascontiguousarray(rotate, dtype=np.float64).reshape(9)
        bc = bh = None
        if bbox is not None:
            bc = np.ascontiguousarray(bbox[0], dtype=np.float64); bh = np.ascontiguousarray(bbox[1], dtype=np.float64)
        opt = lambda a: None if a is None else _p(a)
        self._check(self.lib.isdf_set_shape_program(self.h, instr, csg._n(instr), opt(tr), opt(ro), float(bound_radius), opt(bc), opt(bh)))

    def set_shape_sampled(self, fn, nd, nres, bound_radius=0.0):
        """fn(p[3]) -> (distance, gradient[3]): any host shape's getSDFwithGrad1; tabulated like BasicShape::initShape."""
        def tramp(_u, pp, gp):
            d, g = fn(np.array([pp[0], pp[1], pp[2]]))
            gp[0], gp[1], gp[2] = float(g[0]), float(g[1]), float(g[2])
            return float(d)
        cb = capi.SDF_WITH_GRAD_FN(tramp)
        self._check(self.lib.isdf_set_shape_sampled(self.h, cb, None, float(nd[0]), float(nd[1]), float(nd[2]), float(nres), float(bound_radius), None, None))

    def set_points(self, pts):
        pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
        self._check(self.lib.isdf_set_points(self.h, _p(pts), pts.shape[0]))

    # ---- map products built on the device
    def set_pointcloud(self, xyz, res, sta_threshold=1, bmin=None, bmax=None):
        """xyz: n x 3 float32 (pcl::PointXYZ).  Returns the grid dimensions."""
        pts = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        dims = (C.c_int * 3)()
        bm0 = None if bmin is None else np.asarray(bmin, dtype=np.float64)
        bm1 = None if bmax is None else np.asarray(bmax, dtype=np.float64)
        self._check(self.lib.isdf_set_pointcloud(self.h, pts.ctypes.data_as(C.POINTER(C.c_float)), pts.shape[0],
                                                 None if bm0 is None else _p(bm0), None if bm1 is None else _p(bm1),
                                                 float(res), int(sta_threshold), dims))
        self._map_res = float(res)
        return tuple(dims)

    def generate_esdf(self):
        self._check(self.lib.isdf_generate_esdf(self.h))

    def get_grid(self, kind):
        dims = (C.c_int * 3)()
        o = np.zeros(3); bm = np.zeros(3)
        self._check(self.lib.isdf_get_grid(self.h, kind, None, capi.F32, dims, _p(o), _p(bm)))
        shape = tuple(dims)
        if kind == capi.GRID_ESDF:
            out = np.zeros(shape, dtype=np.float32); dt = capi.F32
        else:
            out = np.zeros(shape, dtype=np.uint8); dt = capi.U8
        self._check(self.lib.isdf_get_grid(self.h, kind, out.ctypes.data_as(C.c_void_p), dt, dims, _p(o), _p(bm)))
        return out, o, bm

    # ---- the map updated in place (csrc/map_update.hip)
    def _map_update_params(self, max_new_voxels=None, full_fraction=None, refresh_esdf=True, refresh_frontend=True):
        p = capi.IsdfMapUpdateParams()
        self.lib.isdf_map_update_params_default(C.byref(p))
        if max_new_voxels is not None:
            p.max_new_voxels = int(max_new_voxels)
        if full_fraction is not None:
            p.full_fraction = float(full_fraction)
        p.refresh_esdf = int(bool(refresh_esdf)); p.refresh_frontend = int(bool(refresh_frontend))
        return p

    def update_pointcloud(self, xyz, **params):
        """isdf_update_pointcloud: NEW points (n x 3 float32) added to the map of set_pointcloud; every derived product is refreshed
        where it can change.  params: max_new_voxels, full_fraction, refresh_esdf, refresh_frontend.  Returns IsdfMapUpdateInfo."""
        pts = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        p = self._map_update_params(**params)
        info = capi.IsdfMapUpdateInfo()
        self._check(self.lib.isdf_update_pointcloud(self.h, pts.ctypes.data_as(C.POINTER(C.c_float)), pts.shape[0], C.byref(p), C.byref(info)))
        self._watch_refresh_rows()
        return info

    def update_voxels(self, ijk, **params):
        """isdf_update_voxels: the listed voxels (n x 3 indices) become occupied.  Returns IsdfMapUpdateInfo."""
        v = np.ascontiguousarray(ijk, dtype=np.int32).reshape(-1, 3)
        p = self._map_update_params(**params)
        info = capi.IsdfMapUpdateInfo()
        self._check(self.lib.isdf_update_voxels(self.h, v.ctypes.data_as(C.POINTER(C.c_int32)), v.shape[0], C.byref(p), C.byref(info)))
        self._watch_refresh_rows()
        return info

    # ---- voxels cleared from the map in place (csrc/map_clear.hip)
    def _map_clear_params(self, max_cleared_voxels=None, full_fraction=None, refresh_esdf=True, refresh_frontend=True):
        p = capi.IsdfMapClearParams()
        self.lib.isdf_map_clear_params_default(C.byref(p))
        if max_cleared_voxels is not None:
            p.max_cleared_voxels = int(max_cleared_voxels)
        if full_fraction is not None:
            p.full_fraction = float(full_fraction)
        p.refresh_esdf = int(bool(refresh_esdf)); p.refresh_frontend = int(bool(refresh_frontend))
        return p

    def clear_pointcloud(self, xyz, **params):
        """isdf_clear_pointcloud: points (n x 3 float32) taken OUT of the counts set_pointcloud keeps; a voxel that falls below the
        threshold becomes free and every derived product is refreshed where it can change.  params: max_cleared_voxels, full_fraction,
        refresh_esdf, refresh_frontend.  Returns IsdfMapClearInfo."""
        pts = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        p = self._map_clear_params(**params)
        info = capi.IsdfMapClearInfo()
        self._check(self.lib.isdf_clear_pointcloud(self.h, pts.ctypes.data_as(C.POINTER(C.c_float)), pts.shape[0], C.byref(p), C.byref(info)))
        self._watch_refresh_rows()
        return info

    def clear_voxels(self, ijk, **params):
        """isdf_clear_voxels: the listed voxels (n x 3 indices) become free.  Returns IsdfMapClearInfo."""
        v = np.ascontiguousarray(ijk, dtype=np.int32).reshape(-1, 3)
        p = self._map_clear_params(**params)
        info = capi.IsdfMapClearInfo()
        self._check(self.lib.isdf_clear_voxels(self.h, v.ctypes.data_as(C.POINTER(C.c_int32)), v.shape[0], C.byref(p), C.byref(info)))
        self._watch_refresh_rows()
        return info

    # ---- a range scan integrated into the map (csrc/map_scan.hip)
    def integrate_scan(self, origin, xyz, hit=None, miss_weight=None, max_cleared_voxels=None, max_new_voxels=None, full_fraction=None, refresh_esdf=True,
                       refresh_frontend=True):
        """isdf_integrate_scan: the rays from `origin` to the end points xyz (n x 3 float32) traced on the device; the counts go down by
        miss_weight once in every voxel a ray passes and up by one at the end voxel of every ray with hit != 0 (hit None: all).  The
        other params go to the clear stage (max_cleared_voxels), the update stage (max_new_voxels) or both.  Returns IsdfMapScanInfo."""
        pts = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        o = np.ascontiguousarray(origin, dtype=np.float64).reshape(3)
        h = None if hit is None else np.ascontiguousarray(hit, dtype=np.uint8).reshape(pts.shape[0])
        p = capi.IsdfMapScanParams()
        self.lib.isdf_map_scan_params_default(C.byref(p))
        if miss_weight is not None:
            p.miss_weight = int(miss_weight)
        p.clear = self._map_clear_params(max_cleared_voxels=max_cleared_voxels, full_fraction=full_fraction, refresh_esdf=refresh_esdf, refresh_frontend=refresh_frontend)
        p.update = self._map_update_params(max_new_voxels=max_new_voxels, full_fraction=full_fraction, refresh_esdf=refresh_esdf, refresh_frontend=refresh_frontend)
        info = capi.IsdfMapScanInfo()
        self._check(self.lib.isdf_integrate_scan(self.h, _p(o), pts.ctypes.data_as(C.POINTER(C.c_float)), None if h is None else h.ctypes.data_as(C.c_void_p),
                                                 pts.shape[0], C.byref(p), C.byref(info)))
        self._watch_refresh_rows()
        return info

    # ---- rays cast through the map (csrc/map_raycast.hip)
    def map_raycast(self, origins, ends, test_origin_voxel=False, per_ray_origin=None):
        """isdf_map_raycast: the rays origins -> ends (ends n x 3 float32; origins 3 doubles for all rays, or n x 3 - per_ray_origin None:
        by the array's rank) cast through the occupancy on the device, read-only.  Returns (rows int32 [n, 8] = (status, steps, i, j, k,
        axis, num, den) per ray, IsdfMapRaycastInfo)."""
        pts = np.ascontiguousarray(ends, dtype=np.float32).reshape(-1, 3)
        o, per_ray = _raycast_origins(origins, pts.shape[0], per_ray_origin)
        p = _raycast_params(self.lib, test_origin_voxel, per_ray)
        rows = np.zeros((pts.shape[0], capi.RAYCAST_ROW), dtype=np.int32)
        info = capi.IsdfMapRaycastInfo()
        self._check(self.lib.isdf_map_raycast(self.h, _p(o), pts.ctypes.data_as(C.POINTER(C.c_float)), pts.shape[0], C.byref(p), rows.ctypes.data_as(C.c_void_p),
                                              C.byref(info)))
        return rows, info

    def map_raycast_device(self, origins, d_ends, d_rows, test_origin_voxel=False, want_info=True, stream=None):
        """isdf_map_raycast_device: d_ends (float32 [n, 3]) and d_rows (int32 [n, 8]) are torch tensors on the ctx's device; origins is a
        host array of 3 doubles (shared) or a float64 [n, 3] tensor on the device (per ray).  The work goes on `stream` (None: torch's
        current stream).  want_info False: info_out = NULL - nothing is handed over and nothing synchronised; returns None then."""
        import torch
        n = int(d_ends.shape[0])
        per_ray = isinstance(origins, torch.Tensor)
        if per_ray:
            assert origins.dtype == torch.float64 and origins.is_contiguous() and tuple(origins.shape) == (n, 3)
            op = C.c_void_p(origins.data_ptr())
        else:
            o = np.ascontiguousarray(origins, dtype=np.float64).reshape(3)
            op = o.ctypes.data_as(C.c_void_p)
        assert d_ends.dtype == torch.float32 and d_ends.is_contiguous() and d_rows.dtype == torch.int32 and d_rows.is_contiguous()
        assert tuple(d_rows.shape) == (n, capi.RAYCAST_ROW)
        p = _raycast_params(self.lib, test_origin_voxel, per_ray)
        info = capi.IsdfMapRaycastInfo() if want_info else None
        st = torch.cuda.current_stream().cuda_stream if stream is None else stream
        self._check(self.lib.isdf_map_raycast_device(self.h, op, C.c_void_p(d_ends.data_ptr()), n, C.byref(p), C.c_void_p(d_rows.data_ptr()),
                                                     None if info is None else C.byref(info), C.c_void_p(st)))
        return info

    # ---- the depth camera (csrc/depth_cam.hip)
    def depth_render(self, cam, cam2world, xyz=None, **params):
        """isdf_depth_render: the depth image (int32 [height, width], millimetres, 999999 = empty) of the cloud xyz (n x 3 float32) or -
        xyz None - of the ctx's own occupied voxels, rendered on the device, read-only.  params: splat_m, min_depth_m, max_splat_px.
        Returns (image, IsdfDepthRenderInfo)."""
        pose = _pose12(cam2world)
        image = np.zeros((cam.height, cam.width), dtype=np.int32)
        info = capi.IsdfDepthRenderInfo()
        if xyz is None:
            p = _depth_render_params(self.lib, source=capi.DEPTH_SOURCE_MAP, **params)
            pts, n = None, 0
        else:
            p = _depth_render_params(self.lib, source=capi.DEPTH_SOURCE_CLOUD, **params)
            pts = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
            n = pts.shape[0]
        self._check(self.lib.isdf_depth_render(self.h, C.byref(cam), _p(pose), None if pts is None else pts.ctypes.data_as(C.c_void_p), n, C.byref(p),
                                               image.ctypes.data_as(C.c_void_p), C.byref(info)))
        return image, info

    def depth_render_device(self, cam, cam2world, d_xyz, d_image, want_info=True, stream=None, **params):
        """isdf_depth_render_device: d_xyz (float32 [n, 3]; None: the ctx's map) and d_image (int32 [height, width]) are torch tensors on
        the ctx's device; the work goes on `stream` (None: torch's current stream).  want_info False: info_out = NULL - nothing is
        counted, handed over or synchronised; returns None then."""
        import torch
        pose = _pose12(cam2world)
        assert d_image.dtype == torch.int32 and d_image.is_contiguous() and tuple(d_image.shape) == (cam.height, cam.width)
        if d_xyz is None:
            p = _depth_render_params(self.lib, source=capi.DEPTH_SOURCE_MAP, **params)
            xp, n = None, 0
        else:
            assert d_xyz.dtype == torch.float32 and d_xyz.is_contiguous() and d_xyz.shape[1] == 3
            p = _depth_render_params(self.lib, source=capi.DEPTH_SOURCE_CLOUD, **params)
            xp, n = C.c_void_p(d_xyz.data_ptr()), int(d_xyz.shape[0])
        info = capi.IsdfDepthRenderInfo() if want_info else None
        st = torch.cuda.current_stream().cuda_stream if stream is None else stream
        self._check(self.lib.isdf_depth_render_device(self.h, C.byref(cam), _p(pose), xp, n, C.byref(p), C.c_void_p(d_image.data_ptr()),
                                                      None if info is None else C.byref(info), C.c_void_p(st)))
        return info

    def depth_rays(self, cam, cam2world, image, **params):
        """isdf_depth_rays: the depth image (int32 mm, uint16 mm or float32 m, by dtype) unprojected on the device, cut to range and clipped
        to the ctx's map.  params: stride, min_range_m, max_range_m, no_return_is_free.  Returns (ends float32 [n, 3], hit uint8 [n],
        IsdfDepthRaysInfo) - what integrate_scan takes, the camera's position as the origin."""
        pose = _pose12(cam2world)
        img, fmt = _depth_image(cam, image)
        p = _depth_rays_params(self.lib, **params)
        n = _depth_rows(self.lib, cam, p)
        ends, hit = np.zeros((n, 3), dtype=np.float32), np.zeros(n, dtype=np.uint8)
        info = capi.IsdfDepthRaysInfo()
        self._check(self.lib.isdf_depth_rays(self.h, C.byref(cam), _p(pose), img.ctypes.data_as(C.c_void_p), fmt, C.byref(p), ends.ctypes.data_as(C.c_void_p),
                                             hit.ctypes.data_as(C.c_void_p), C.byref(info)))
        return ends, hit, info

    def integrate_depth(self, cam, cam2world, image, stride=None, min_range_m=None, max_range_m=None, no_return_is_free=None, miss_weight=None,
                        max_cleared_voxels=None, max_new_voxels=None, full_fraction=None, refresh_esdf=True, refresh_frontend=True):
        """isdf_integrate_depth: integrate_scan of the rays depth_rays_host gives for the image, with only the image uploaded.  The first
        four params are depth_rays', the others integrate_scan's.  Returns (IsdfDepthRaysInfo, IsdfMapScanInfo)."""
        pose = _pose12(cam2world)
        img, fmt = _depth_image(cam, image)
        rp = _depth_rays_params(self.lib, stride=stride, min_range_m=min_range_m, max_range_m=max_range_m, no_return_is_free=no_return_is_free)
        p = capi.IsdfMapScanParams()
        self.lib.isdf_map_scan_params_default(C.byref(p))
        if miss_weight is not None:
            p.miss_weight = int(miss_weight)
        p.clear = self._map_clear_params(max_cleared_voxels=max_cleared_voxels, full_fraction=full_fraction, refresh_esdf=refresh_esdf, refresh_frontend=refresh_frontend)
        p.update = self._map_update_params(max_new_voxels=max_new_voxels, full_fraction=full_fraction, refresh_esdf=refresh_esdf, refresh_frontend=refresh_frontend)
        dinfo, sinfo = capi.IsdfDepthRaysInfo(), capi.IsdfMapScanInfo()
        self._check(self.lib.isdf_integrate_depth(self.h, C.byref(cam), _p(pose), img.ctypes.data_as(C.c_void_p), fmt, C.byref(rp), C.byref(p), C.byref(dinfo),
                                                  C.byref(sinfo)))
        self._watch_refresh_rows()
        return dinfo, sinfo

    # ---- the map window shifted in place (csrc/map_shift.hip)
    def _map_shift_params(self, full_fraction=None, force_path=None):
        p = capi.IsdfMapShiftParams()
        self.lib.isdf_map_shift_params_default(C.byref(p))
        if full_fraction is not None:
            p.full_fraction = float(full_fraction)
        if force_path is not None:
            p.force_path = int(force_path)
        return p

    def shift_map(self, shift, **params):
        """isdf_shift_map: the window moves by `shift` voxels (new voxel v holds what old voxel v + shift held); every built product is
        the shifted map's afterwards.  params: full_fraction, force_path.  Returns IsdfMapShiftInfo."""
        p = self._map_shift_params(**params)
        info = capi.IsdfMapShiftInfo()
        self._check(self.lib.isdf_shift_map(self.h, _i3(shift), C.byref(p), C.byref(info)))
        self._watch_refresh_rows()
        return info

    def map_follow(self, centre, min_shift=1, **params):
        """isdf_map_follow: shifts the window so that `centre` (world) falls into its middle voxel, unless that takes fewer than
        min_shift voxels on every axis.  Returns (shift applied as a tuple, IsdfMapShiftInfo)."""
        ctr = np.ascontiguousarray(centre, dtype=np.float64).reshape(3)
        p = self._map_shift_params(**params)
        info = capi.IsdfMapShiftInfo()
        s = (C.c_int32 * 3)()
        self._check(self.lib.isdf_map_follow(self.h, _p(ctr), int(min_shift), C.byref(p), s, C.byref(info)))
        self._watch_refresh_rows()
        return tuple(s), info

    # ---- observed space: the known grid and the frontier (csrc/map_known.hip)
    def map_known_enable(self, on=True):
        """isdf_map_known_enable: the ctx keeps (on) or releases (off) one known bit per voxel of its map; the mode outlives maps."""
        self._check(self.lib.isdf_map_known_enable(self.h, int(bool(on))))

    def map_known_fill(self, box=None, value=1):
        """isdf_map_known_fill: the inclusive box (lo_x, lo_y, lo_z, hi_x, hi_y, hi_z) - None: the whole map - declared known (value 1)
        or unknown (0)."""
        self._check(self.lib.isdf_map_known_fill(self.h, None if box is None else (C.c_int32 * 6)(*[int(v) for v in box]), int(value)))

    def map_known_merge_ms(self, enable=True):
        """isdf_map_known_merge_ms: the device time of the last timed merge kernel (-1: none), and whether later merges are timed."""
        ms = C.c_double(-1.0)
        self._check(self.lib.isdf_map_known_merge_ms(self.h, int(bool(enable)), C.byref(ms)))
        return float(ms.value)

    def map_known(self):
        """isdf_map_known_get: (the grid's uint32 words - known_unpack gives booleans -, IsdfMapKnownInfo)."""
        out = np.zeros(known_words(self._grid_dims()), dtype=np.uint32)
        info = capi.IsdfMapKnownInfo()
        self._check(self.lib.isdf_map_known_get(self.h, out.ctypes.data_as(C.c_void_p), C.byref(info)))
        return out, info

    def known_erode(self, radius=-1, border=0, want_bits=True):
        """isdf_map_known_erode: (the eroded known grid's uint32 words - None when not wanted -, IsdfKnownErodeInfo).  Voxel v is set when
        the whole cube of 2 radius + 1 voxels a side round it is known; radius -1: the front end's (kernel_size - 1) / 2; border: what
        the grid's outside counts as (0 unseen, 1 seen).  Read-only."""
        out = np.zeros(known_words(self._grid_dims()), dtype=np.uint32) if want_bits else None
        p = capi.IsdfKnownErodeParams(int(radius), int(border))
        info = capi.IsdfKnownErodeInfo()
        self._check(self.lib.isdf_map_known_erode(self.h, C.byref(p), None if out is None else out.ctypes.data_as(C.c_void_p), C.byref(info)))
        return out, info

    def map_frontier(self, capacity=None, want_list=True):
        """isdf_map_frontier: (frontier words, voxel indices int64 ascending - None when not wanted -, IsdfMapFrontierInfo).  capacity:
        of the list (default: grown to the number of frontier voxels, which a first short call reports); an explicit one that is too
        short raises IsdfError(ISDF_ERR_OVERFLOW)."""
        out = np.zeros(known_words(self._grid_dims()), dtype=np.uint32)
        info = capi.IsdfMapFrontierInfo()
        if not want_list:
            self._check(self.lib.isdf_map_frontier(self.h, out.ctypes.data_as(C.c_void_p), None, 0, C.byref(info)))
            return out, None, info
        vox = np.zeros(int(capacity) if capacity is not None else max(getattr(self, "_frontier_cap", 0), 1024), dtype=np.int64)
        rc = self.lib.isdf_map_frontier(self.h, out.ctypes.data_as(C.c_void_p), vox.ctypes.data_as(C.c_void_p), vox.size, C.byref(info))
        if rc == capi.ISDF_ERR_OVERFLOW and capacity is None:      # the info is filled: once more with room
            vox = np.zeros(int(info.n_frontier), dtype=np.int64)
            rc = self.lib.isdf_map_frontier(self.h, out.ctypes.data_as(C.c_void_p), vox.ctypes.data_as(C.c_void_p), vox.size, C.byref(info))
        self._check(rc)
        self._frontier_cap = max(getattr(self, "_frontier_cap", 0), int(info.n_frontier))
        return out, vox[:int(info.n_frontier)], info

    def map_frontier_clusters(self, bits=None, connectivity=26, min_size=1):
        """isdf_map_frontier_clusters: the connected components (connectivity 6, 18 or 26) of the frontier - or of `bits`, any voxel set as
        a bit grid in the known grid's layout (known_pack) -, on the device, read-only.  Does the sizing call itself.  Returns (voxels
        int64 ascending - the frontier's list -, labels int32 - the row of each voxel's cluster, -1 where min_size dropped it -, rows int64
        [n_rows, 16] = (label, size, lo xyz, hi xyz, sum xyz, rep_voxel, rep_d2, first_pos, 0, 0) in ascending label order,
        IsdfFrontierClusterInfo).  From the frontier to scored goals without the list crossing the bus twice:

            vox, labels, rows, info = eng.map_frontier_clusters(min_size=20)
            _, bmin, _ = eng.get_grid(capi.GRID_OCCUPANCY)
            centroids, reps = cluster_points(rows, bmin, res, dims)
            poses = [look_at(eye, rep) for rep in reps]         # rep: the centre of a frontier voxel, known and free
            gains, best = eng.view_gain(cam, poses, max_range_m=5.0)
        """
        w = None if bits is None else _known_args(bits, self._grid_dims())[0]
        p = _cluster_params(self.lib, connectivity, min_size)
        try:
            return _cluster_call(lambda vox, labels, nv, rows, nr, info: self.lib.isdf_map_frontier_clusters(
                self.h, None if w is None else w.ctypes.data_as(C.c_void_p), C.byref(p), vox, labels, nv, rows, nr, C.byref(info)), "isdf_map_frontier_clusters")
        except IsdfError as e:
            self._check(e.code)
            raise

    def _traj_known_params(self, margin, mode):
        p = capi.IsdfTrajKnownParams()
        self.lib.isdf_traj_known_params_default(C.byref(p))
        if margin is not None:
            p.margin = float(margin)
        p.mode = int(mode)
        return p

    @staticmethod
    def _traj_known_report(info):
        return {name: (np.array(getattr(info, name)) if name == "horizon_point" else getattr(info, name)) for name, _ in capi.IsdfTrajKnownInfo._fields_}

    def traj_known_horizon(self, T, coeffs_colmajor, margin=None, mode=capi.SWEPT_FIELD_PLANNER):
        """isdf_traj_known_horizon: the earliest time at which the swept body comes within `margin` of an unknown voxel's centre - a dict of
        the isdf_traj_known_info fields (horizon_t -1: never).  margin None = cfg.safety_hor."""
        T = np.ascontiguousarray(T, dtype=np.float64)
        Cc = np.ascontiguousarray(coeffs_colmajor, dtype=np.float64).reshape(-1)
        p = self._traj_known_params(margin, mode)
        info = capi.IsdfTrajKnownInfo()
        self._check(self.lib.isdf_traj_known_horizon(self.h, T.size, _p(T), _p(Cc), C.byref(p), C.byref(info)))
        return self._traj_known_report(info)

    def traj_known_horizon_device(self, N, d_T, d_coeffs, margin=None, mode=capi.SWEPT_FIELD_PLANNER, stream=0):
        """The same with the trajectory on the device, on `stream`."""
        p = self._traj_known_params(margin, mode)
        info = capi.IsdfTrajKnownInfo()
        self._check(self.lib.isdf_traj_known_horizon_device(self.h, N, C.c_void_p(d_T), C.c_void_p(d_coeffs), C.byref(p), C.byref(info), C.c_void_p(stream)))
        return self._traj_known_report(info)

    # ---- the view gain (csrc/view_gain.hip)
    def view_gain(self, cam, poses, **params):
        """isdf_view_gain: per candidate pose (poses n x 12 doubles, look_at's), the voxels unknown today that the depth camera would see
        from there, on the device, read-only.  params: stride (one number or (u, v)), max_range_m, scratch_bytes.  Returns (rows int64
        [n, 8] = (status, gain, n_rays, n_skipped, n_hits, steps_total, n_rays_unknown, 0), IsdfViewGainInfo)."""
        P = _view_poses(poses)
        p = _view_gain_params(self.lib, **params)
        rows = np.zeros((P.shape[0], capi.VIEW_GAIN_ROW), dtype=np.int64)
        info = capi.IsdfViewGainInfo()
        self._check(self.lib.isdf_view_gain(self.h, C.byref(cam), _p(P), P.shape[0], C.byref(p), rows.ctypes.data_as(C.c_void_p), C.byref(info)))
        return rows, info

    def view_gain_device(self, cam, d_poses, d_rows, want_info=True, stream=None, **params):
        """isdf_view_gain_device: d_poses (float64 [n, 12]) and d_rows (int64 [n, 8]) are torch tensors on the ctx's device; the work goes
        on `stream` (None: torch's current stream).  want_info False: info_out = NULL - nothing is handed over and nothing synchronised;
        returns None then."""
        import torch
        n = int(d_poses.shape[0])
        assert d_poses.dtype == torch.float64 and d_poses.is_contiguous() and tuple(d_poses.shape) == (n, 12)
        assert d_rows.dtype == torch.int64 and d_rows.is_contiguous() and tuple(d_rows.shape) == (n, capi.VIEW_GAIN_ROW)
        p = _view_gain_params(self.lib, **params)
        info = capi.IsdfViewGainInfo() if want_info else None
        st = torch.cuda.current_stream().cuda_stream if stream is None else stream
        self._check(self.lib.isdf_view_gain_device(self.h, C.byref(cam), C.c_void_p(d_poses.data_ptr()), n, C.byref(p), C.c_void_p(d_rows.data_ptr()),
                                                   None if info is None else C.byref(info), C.c_void_p(st)))
        return info

    # ---- candidate views (csrc/view_cand.hip)
    def view_candidates(self, cam, targets, offsets, **params):
        """isdf_view_candidates: eyes targets[i] + offsets[k] (metres; view_ring_offsets builds rings) tested on the device for being a
        safe, seen place from which the target is visible, the survivors posed, scored by the view gain and ranked per target, read-only.
        params: clearance_voxels, k_best, min_gain, and the view gain's stride, max_range_m, scratch_bytes.  Returns what
        view_candidates_host returns: (cand, poses, target_rows, best, IsdfViewCandidatesInfo)."""
        p = _view_cand_params(self.lib, **params)
        t, o, cand, poses, rows, best = _view_cand_arrays(targets, offsets, p.k_best)
        info = capi.IsdfViewCandidatesInfo()
        self._check(self.lib.isdf_view_candidates(self.h, C.byref(cam), t.ctypes.data_as(C.c_void_p), t.shape[0], o.ctypes.data_as(C.c_void_p), o.shape[0], C.byref(p),
                                                  cand.ctypes.data_as(C.c_void_p), poses.ctypes.data_as(C.c_void_p), rows.ctypes.data_as(C.c_void_p),
                                                  best.ctypes.data_as(C.c_void_p), C.byref(info)))
        return cand, poses, rows, best, info

    def next_views(self, cam, offsets, connectivity=26, min_size=1, **params):
        """One turn of a next-best-view loop: map_frontier_clusters, the centres of the clusters' rep_voxel cells (cluster_points) as
        targets, view_candidates round them.  Returns (cluster rows, cand, poses, target_rows, best, IsdfViewCandidatesInfo); the best
        eye overall is poses[info.best_candidate] (-1: no candidate qualified), a goal for frontend_field_build."""
        _, _, rows, _ = self.map_frontier_clusters(connectivity=connectivity, min_size=min_size)
        _, bmin, _ = self.get_grid(capi.GRID_OCCUPANCY)
        _, reps = cluster_points(rows, bmin, self._map_res, self._grid_dims())          # (the resolution set_grid / set_pointcloud gave)
        return (rows,) + self.view_candidates(cam, reps, offsets, **params)

    # ---- the view selection (csrc/view_select.hip)
    def view_select(self, cam, poses, **params):
        """isdf_view_select: the greedy coverage selection of up to k_select of the poses by their joint gain, every round on the device,
        read-only.  params: k_select, min_gain, and the view gain's stride, max_range_m, scratch_bytes.  Returns what view_select_host
        returns: (rows, select, round, claimed, IsdfViewSelectInfo)."""
        p = _view_select_params(self.lib, **params)
        P, rows, select, rnd, claimed = _view_select_arrays(poses, p.k_select, self._grid_dims())
        info = capi.IsdfViewSelectInfo()
        self._check(self.lib.isdf_view_select(self.h, C.byref(cam), P.ctypes.data_as(C.c_void_p), P.shape[0], C.byref(p), rows.ctypes.data_as(C.c_void_p),
                                              select.ctypes.data_as(C.c_void_p), rnd.ctypes.data_as(C.c_void_p), claimed.ctypes.data_as(C.c_void_p), C.byref(info)))
        return rows, select, rnd, claimed, info

    def next_view_set(self, cam, offsets, k_select=4, select_min_gain=1, connectivity=26, min_size=1, **params):
        """next_views, then view_select over the poses of all targets' best lists (in the order of the lists): the next k_select places to
        look, chosen by what they add together rather than each alone.  params go to next_views (clearance_voxels, k_best, min_gain, and
        the view gain's, which the selection shares); select_min_gain is the selection's min_gain.  Returns (poses float64 [n_selected, 12]
        in the order picked, their marginal gains int64 [n_selected], their candidate indices int64 [n_selected], IsdfViewSelectInfo).
        The loop's last link is frontend_field_build_known towards a picked pose's eye (poses[i, 3::4]): the cost-to-go field through
        observed space only, off which frontend_field_paths reads the way there."""
        _, _, poses, _, best, _ = self.next_views(cam, offsets, connectivity=connectivity, min_size=min_size, **params)
        listed = best[best >= 0]
        gain = {k: v for k, v in params.items() if k in ("stride", "max_range_m", "scratch_bytes")}
        _, select, _, _, info = self.view_select(cam, poses[listed], k_select=k_select, min_gain=select_min_gain, **gain)
        picked = select[:info.n_selected]
        return np.ascontiguousarray(poses[listed[picked[:, 0]]]), picked[:, 1].copy(), listed[picked[:, 0]], info

    def view_select_routed(self, cam, poses, cost=None, **params):
        """isdf_view_select_routed: view_select by utility = marginal gain per travel cost.  cost None: the travel cost of a view is the
        ctx's valid cost-to-go field at its eye - build the field TOWARDS THE ROBOT first (frontend_field_build[_known]) -, an eye the
        field does not reach is never picked; else one non-negative double or +inf per pose.  params: cost0, max_cost, path_cap, and
        view_select's (min_gain >= 1).  Returns (rows, select, round, claimed, cost float64 [n], util float64 [k_select, 2], paths,
        IsdfViewSelectRoutedInfo); paths is None with path_cap 0, else (n int32 [k_select], xyz [k_select, path_cap, 3], roll/pitch
        [k_select, path_cap, 2]) as frontend_field_paths gives them for the picked eyes in pick order: each walks from the eye to the
        robot's cell, with the attitudes of walking that way."""
        p = _view_route_params(self.lib, **params)
        k = max(int(p.select.k_select), 0)
        P, rows, select, rnd, claimed = _view_select_arrays(poses, k, self._grid_dims())
        c = _view_route_cost(cost, P.shape[0])
        cost_out, util = np.zeros(P.shape[0]), np.zeros((k, 2))
        cap = max(int(p.path_cap), 0)
        paths = (np.zeros(k, dtype=np.int32), np.zeros((k, cap, 3)), np.zeros((k, cap, 2))) if cap else None
        info = capi.IsdfViewSelectRoutedInfo()
        ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)          # noqa: E731
        self._check(self.lib.isdf_view_select_routed(self.h, C.byref(cam), ptr(P), P.shape[0], ptr(c), C.byref(p), ptr(rows), ptr(select), ptr(rnd), ptr(claimed),
                                                     ptr(cost_out), ptr(util), *([ptr(a) for a in paths] if paths else [None] * 3), C.byref(info)))
        return rows, select, rnd, claimed, cost_out, util, paths, info

    def next_view_set_routed(self, cam, offsets, robot_xyz, known=True, radius=-1, border=0, k_select=4, select_min_gain=1, cost0=1.0, max_cost=np.inf,
                             path_cap=256, connectivity=26, min_size=1, **params):
        """next_view_set with the robot in it: next_views, then the cost-to-go field towards robot_xyz (frontend_field_build_known with
        radius and border when `known`, else frontend_field_build; it replaces the ctx's field), then view_select_routed over the poses
        of all targets' best lists.  Returns (poses float64 [n_selected, 12] in the order picked, their marginal gains int64
        [n_selected], their travel costs float64 [n_selected] in cells, paths: a list of n_selected arrays [n, 3] running robot -> eye
        (a walk of more than path_cap nodes keeps the path_cap nearest the eye and so no longer starts at the robot), their candidate
        indices int64 [n_selected], IsdfViewSelectRoutedInfo).  Every returned view is one the field reaches."""
        _, _, poses, _, best, _ = self.next_views(cam, offsets, connectivity=connectivity, min_size=min_size, **params)
        listed = best[best >= 0]
        if known:
            self.frontend_field_build_known(robot_xyz, radius, border)
        else:
            self.frontend_field_build(robot_xyz)
        gain = {k: v for k, v in params.items() if k in ("stride", "max_range_m", "scratch_bytes")}
        _, select, _, _, _, util, paths, info = self.view_select_routed(cam, poses[listed], k_select=k_select, min_gain=select_min_gain, cost0=cost0, max_cost=max_cost,
                                                                        path_cap=path_cap, **gain)
        n_sel = info.select.n_selected
        picked = select[:n_sel]
        n, xyz, _ = paths
        cap = xyz.shape[1]
        # (a walk longer than path_cap is cut at its far end, the robot's)
        ways = [np.ascontiguousarray(xyz[r, :min(int(n[r]), cap)][::-1]) for r in range(n_sel)]
        return np.ascontiguousarray(poses[listed[picked[:, 0]]]), picked[:, 1].copy(), util[:n_sel, 0].copy(), ways, listed[picked[:, 0]], info

    def map_counts(self):
        """The per-voxel point counts set_pointcloud keeps, uint32 [X, Y, Z]."""
        out = np.zeros(self._grid_dims(), dtype=np.uint32)
        self._check(self.lib.isdf_map_counts_get(self.h, out.ctypes.data_as(C.c_void_p)))
        return out

    def gather_points(self, waypoints, half, offset=None):
        W = np.ascontiguousarray(np.asarray(waypoints, dtype=np.float64).reshape(-1, 3))
        h = np.asarray(half, dtype=np.float64) * np.ones(3)
        off = None if offset is None else np.asarray(offset, dtype=np.float64)
        M = C.c_int(0)
        self._check(self.lib.isdf_gather_points(self.h, _p(W) if W.size else None, W.shape[0], _p(h),
                                                None if off is None else _p(off), C.byref(M)))
        return M.value

    def get_points(self):
        M = self.lib.isdf_get_points(self.h, None, 0)
        if M < 0:
            self._check(M)
        out = np.zeros((M, 3))
        if M:
            rc = self.lib.isdf_get_points(self.h, _p(out), M)
            if rc < 0:
                self._check(rc)
        return out

    def shape_eval(self, p_rel, want_grad=True):
        """(sdf[n], grad[n, 3]) of the installed shape at body-frame points (getonlySDF / getonlyGrad1)."""
        p_rel = np.ascontiguousarray(p_rel, dtype=np.float64).reshape(-1, 3)
        n = p_rel.shape[0]
        sdf = np.zeros(n); grad = np.zeros((n, 3)) if want_grad else None
        self._check(self.lib.isdf_shape_eval(self.h, _p(p_rel), n, _p(sdf), _p(grad) if want_grad else None))
        return sdf, grad

    def esdf_sample(self, xyz, want_grad=True, scattered=False):
        """(value[n], grad[n, 3]) of the environment ESDF at world points (GridMap3D::getSDFValue / getSDFValueWithGrad);
        scattered: through the bricked copy (points in no particular order) - the same bits."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        n = xyz.shape[0]
        val = np.zeros(n); grad = np.zeros((n, 3)) if want_grad else None
        fn = self.lib.isdf_esdf_sample_scattered if scattered else self.lib.isdf_esdf_sample
        self._check(fn(self.h, _p(xyz), n, _p(val), _p(grad) if want_grad else None))
        return val, grad

    def esdf_sample_device(self, d_xyz, n, d_value, d_grad=0, stream=0, scattered=False):
        """device pointers (ints), asynchronous on `stream`"""
        fn = self.lib.isdf_esdf_sample_scattered_device if scattered else self.lib.isdf_esdf_sample_device
        self._check(fn(self.h, C.c_void_p(d_xyz), n, C.c_void_p(d_value), C.c_void_p(d_grad), C.c_void_p(stream)))

    # ---- front end: pose feasibility by kernel convolution (SweptVolumeManager::checkKernelValue)
    def frontend_build(self, fe_cfg):
        self._fe_cfg = fe_cfg
        self._check(self.lib.isdf_frontend_build(self.h, C.byref(fe_cfg)))

    def frontend_shape_kernels(self):
        """ByteShapeKernel::map of every attitude (reference byte layout): uint8 [xk * yk, k * k * ceil(k / 8)]."""
        d = (C.c_int * 3)()
        self._check(self.lib.isdf_frontend_get_shape_kernels(self.h, None, d))
        out = np.zeros((d[0] * d[1], d[2]), dtype=np.uint8)
        self._check(self.lib.isdf_frontend_get_shape_kernels(self.h, out.ctypes.data_as(C.c_void_p), d))
        return out

    def frontend_map_kernel(self):
        """The array generateMapKernel produces (reference byte layout): uint8 [X + 2h, Y + 2h, ceil((Z + 2h) / 8)]."""
        d = (C.c_int * 3)()
        self._check(self.lib.isdf_frontend_get_map_kernel(self.h, None, d))
        out = np.zeros((d[0], d[1], d[2]), dtype=np.uint8)
        self._check(self.lib.isdf_frontend_get_map_kernel(self.h, out.ctypes.data_as(C.c_void_p), d))
        return out

    def frontend_check(self, index, father_roll, father_pitch):
        """(ok[n] uint8, child_roll[n], child_pitch[n], kernel_index[n]) of AstarGetSucc's per-neighbour test."""
        index = np.ascontiguousarray(index, dtype=np.int32).reshape(-1, 3)
        n = index.shape[0]
        fr = np.ascontiguousarray(np.broadcast_to(father_roll, (n,)), dtype=np.float64)
        fp = np.ascontiguousarray(np.broadcast_to(father_pitch, (n,)), dtype=np.float64)
        ok = np.zeros(n, dtype=np.uint8); cr = np.zeros(n); cp = np.zeros(n); ki = np.zeros(n, dtype=np.int32)
        self._check(self.lib.isdf_frontend_check(self.h, n, index.ctypes.data_as(C.c_void_p), _p(fr), _p(fp), ok.ctypes.data_as(C.c_void_p),
                                                 _p(cr), _p(cp), ki.ctypes.data_as(C.c_void_p)))
        return ok, cr, cp, ki

    def frontend_cspace(self, download=True):
        """(free_mask uint32 [X, Y, Z, 4 * ceil(attitudes / 128)] or None, kernel ms): bit (i * yk + j) of a voxel's mask = attitude fits."""
        dims = (C.c_int * 3)()
        o = np.zeros(3); bm = np.zeros(3)
        self._check(self.lib.isdf_get_grid(self.h, capi.GRID_OCCUPANCY, None, capi.U8, dims, _p(o), _p(bm)))
        kd = (C.c_int * 3)()
        self._check(self.lib.isdf_frontend_get_shape_kernels(self.h, None, kd))
        nw = 4 * ((kd[0] * kd[1] + 127) // 128)
        out = np.zeros((dims[0], dims[1], dims[2], nw), dtype=np.uint32) if download else None
        ms = C.c_double(0.0)
        self._check(self.lib.isdf_frontend_cspace(self.h, out.ctypes.data_as(C.c_void_p) if download else None, C.byref(ms)))
        return out, ms.value

    def frontend_cspace_table(self, host=False):
        """isdf_frontend_cspace_get: the table as it stands, not computed again - the device's, or (host=True) the copy the A* keeps
        on the host.  Same layout as frontend_cspace()."""
        X, Y, Z = self._grid_dims()
        kd = (C.c_int * 3)()
        self._check(self.lib.isdf_frontend_get_shape_kernels(self.h, None, kd))
        out = np.zeros((X, Y, Z, 4 * ((kd[0] * kd[1] + 127) // 128)), dtype=np.uint32)
        self._check(self.lib.isdf_frontend_cspace_get(self.h, int(bool(host)), out.ctypes.data_as(C.c_void_p)))
        return out

    def host_info(self):
        """isdf_host_info: {"handovers", "late", "late_polls"} of the host-mapped result hand-overs of this ctx."""
        a = (C.c_int64 * 8)()
        self._check(self.lib.isdf_host_info(self.h, a))
        return {"handovers": int(a[0]), "late": int(a[1]), "late_polls": int(a[2])}

    def frontend_astar(self, start, goal):
        """AstarPathSearcher::AstarPathSearch + getPath + getastarSE3Path (front_end_Astar.hpp:238-403) over the device-built
        configuration space.  Returns (xyz (n, 3), roll/pitch degrees (n, 2), rot (n, 3, 3), IsdfAstarResult); the three arrays
        are None when success == 0."""
        s = np.ascontiguousarray(start, dtype=np.float64); g = np.ascontiguousarray(goal, dtype=np.float64)
        r = capi.IsdfAstarResult()
        self._check(self.lib.isdf_frontend_astar_search(self.h, _p(s), _p(g), C.byref(r)))
        if not r.success:
            return None, None, None, r
        n = r.n_path
        xyz = np.zeros((n, 3)); rp = np.zeros((n, 2)); rot = np.zeros((n, 3, 3))
        got = self.lib.isdf_frontend_astar_path(self.h, n, _p(xyz), _p(rp), _p(rot))
        if got != n:
            raise RuntimeError(f"isdf_frontend_astar_path returned {got}, the search said {n}")
        return xyz, rp, rot, r

    # ---- the cost-to-go field of one goal over the front end's free graph (csrc/frontend_field.hip), and paths read off it
    def _grid_dims(self):
        dims = (C.c_int * 3)()
        o = np.zeros(3); bm = np.zeros(3)
        self._check(self.lib.isdf_get_grid(self.h, capi.GRID_OCCUPANCY, None, capi.U8, dims, _p(o), _p(bm)))
        return int(dims[0]), int(dims[1]), int(dims[2])

    def frontend_field_build(self, goal, max_rounds=0):
        """isdf_frontend_field_build: the field of the cell of `goal` (world coordinates); returns IsdfFrontendFieldInfo
        (reachable, status 0 fixed point / 1 no reachable goal / 2 max_rounds hit, rounds, bricks, brick_visits, free_voxels,
        reached_voxels, device_ms).  The configuration-space table stays on the device."""
        g = np.ascontiguousarray(goal, dtype=np.float64).reshape(3)
        p = capi.IsdfFrontendFieldParams()
        self.lib.isdf_frontend_field_params_default(C.byref(p))
        p.max_rounds = int(max_rounds)
        info = capi.IsdfFrontendFieldInfo()
        self._check(self.lib.isdf_frontend_field_build(self.h, _p(g), C.byref(p), C.byref(info)))
        return info

    def frontend_field_build_known(self, goal, radius=-1, border=0, max_rounds=0):
        """isdf_frontend_field_build_known: the field of the cell of `goal` through observed space only - a voxel is free when the
        configuration-space table says so AND the whole cube of 2 radius + 1 voxels round it is known (known_erode's radius and border).
        Returns (IsdfFrontendFieldInfo, IsdfKnownErodeInfo).  The robot's own cell is usually unseen: declare a box round it known first
        (map_known_fill); the paths never need a free start cell.  Whatever changes the known grid or the map drops a gated field."""
        g = np.ascontiguousarray(goal, dtype=np.float64).reshape(3)
        p = capi.IsdfFrontendFieldParams()
        self.lib.isdf_frontend_field_params_default(C.byref(p))
        p.max_rounds = int(max_rounds)
        e = capi.IsdfKnownErodeParams(int(radius), int(border))
        info, gate = capi.IsdfFrontendFieldInfo(), capi.IsdfKnownErodeInfo()
        self._check(self.lib.isdf_frontend_field_build_known(self.h, _p(g), C.byref(e), C.byref(p), C.byref(info), C.byref(gate)))
        return info, gate

    def frontend_field_known_info(self):
        """isdf_frontend_field_known_info: (gated, radius_used, border) of the live field; zeros for an ungated field or none."""
        out = (C.c_int32 * 4)()
        self._check(self.lib.isdf_frontend_field_known_info(self.h, out))
        return int(out[0]), int(out[1]), int(out[2])

    def frontend_field_set_known_follow(self, mode):
        """isdf_frontend_field_set_known_follow: what updates, clears, scans, depth images and known-grid fills do with a valid GATED field -
        0 (default) drop it, 1 follow the change in place (the mark against ballot(table) & E of the K of that moment)."""
        self._check(self.lib.isdf_frontend_field_set_known_follow(self.h, int(mode)))

    def frontend_field_follow_info(self):
        """isdf_frontend_field_follow_info: the last followed call's IsdfFieldFollowInfo (ISDF_ERR_STATE: none since the last build)."""
        info = capi.IsdfFieldFollowInfo()
        self._check(self.lib.isdf_frontend_field_follow_info(self.h, C.byref(info)))
        return info

    def frontend_field(self, xyz=None):
        """The whole field, float64 [X, Y, Z] (cells; +inf where a voxel is not free or cannot reach the goal), or, with `xyz`
        (n, 3) world points, the values at their cells (+inf outside the map)."""
        if xyz is None:
            out = np.zeros(self._grid_dims())
            self._check(self.lib.isdf_frontend_field_get(self.h, _p(out)))
            return out
        q = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        out = np.zeros(q.shape[0])
        self._check(self.lib.isdf_frontend_field_value(self.h, _p(q), q.shape[0], _p(out)))
        return out

    def frontend_field_paths(self, starts, cap):
        """Paths for B starts in one launch: (n [B] int32, xyz [B, cap, 3], roll/pitch degrees [B, cap, 2]).  n[b] is the true
        number of nodes of path b (0: none; more than cap: truncated); rows are zero past a path's end.  xyz[b, :n[b]] is what
        the mid end's fit takes as reference points."""
        s = np.ascontiguousarray(starts, dtype=np.float64).reshape(-1, 3)
        B = s.shape[0]
        n = np.zeros(B, dtype=np.int32); xyz = np.zeros((B, int(cap), 3)); rp = np.zeros((B, int(cap), 2))
        self._check(self.lib.isdf_frontend_field_paths(self.h, _p(s), B, int(cap), n.ctypes.data_as(C.c_void_p), _p(xyz), _p(rp)))
        return n, xyz, rp

    def frontend_field_paths_device(self, d_starts, B, cap, d_n, d_xyz, d_rp, stream=0):
        """device pointers (ints), asynchronous on `stream`"""
        self._check(self.lib.isdf_frontend_field_paths_device(self.h, C.c_void_p(d_starts), int(B), int(cap), C.c_void_p(d_n), C.c_void_p(d_xyz),
                                                              C.c_void_p(d_rp), C.c_void_p(stream)))

    def frontend_field_set_repair(self, mode):
        """isdf_frontend_field_set_repair: what update_pointcloud / update_voxels do with a valid field when a voxel became occupied -
        0 (default) drop it, 1 repair it in place (only the values that a closed voxel can have fed are reset and relaxed again)."""
        self._check(self.lib.isdf_frontend_field_set_repair(self.h, int(mode)))

    def frontend_field_repair_info(self):
        """isdf_frontend_field_repair_info: the last repair's IsdfFieldRepairInfo (ISDF_ERR_STATE: none since the last build)."""
        info = capi.IsdfFieldRepairInfo()
        self._check(self.lib.isdf_frontend_field_repair_info(self.h, C.byref(info)))
        return info

    def frontend_field_set_reopen(self, mode):
        """isdf_frontend_field_set_reopen: what clear_pointcloud / clear_voxels do with a valid field when a voxel became free -
        0 (default) drop it, 1 lower it in place (every old value is kept, the relaxation starts at the opened voxels' bricks)."""
        self._check(self.lib.isdf_frontend_field_set_reopen(self.h, int(mode)))

    def frontend_field_reopen_info(self):
        """isdf_frontend_field_reopen_info: the last reopen's IsdfFieldReopenInfo (ISDF_ERR_STATE: none since the last build)."""
        info = capi.IsdfFieldReopenInfo()
        self._check(self.lib.isdf_frontend_field_reopen_info(self.h, C.byref(info)))
        return info

    def frontend_field_set_shift(self, mode):
        """isdf_frontend_field_set_shift: what shift_map / map_follow do with a valid field - 0 (default) drop it, 1 carry it (the
        values translated, the leaving and the closed voxels' threshold reset and relaxed, then the entering and the opened voxels)."""
        self._check(self.lib.isdf_frontend_field_set_shift(self.h, int(mode)))

    def frontend_field_shift_info(self):
        """isdf_frontend_field_shift_info: the last carry's IsdfFieldShiftInfo (ISDF_ERR_STATE: none since the last build)."""
        info = capi.IsdfFieldShiftInfo()
        self._check(self.lib.isdf_frontend_field_shift_info(self.h, C.byref(info)))
        return info

    def frontend_field_release(self):
        self._check(self.lib.isdf_frontend_field_release(self.h))

    # ---- one-shot peer-to-peer exchange of the multi-GPU path (csrc/xchg.hip); see parallel.XgmiExchange
    def xchg_create(self, rank, world, max_doubles):
        h = (C.c_ubyte * 64)()
        self._check(self.lib.isdf_xchg_create(self.h, int(rank), int(world), int(max_doubles), h))
        return bytes(h)

    def xchg_connect(self, handles_bytes):
        buf = (C.c_ubyte * len(handles_bytes)).from_buffer_copy(handles_bytes)
        self._check(self.lib.isdf_xchg_connect(self.h, buf))

    def xchg_allreduce(self, d_ptr, count, stream=0):
        self._check(self.lib.isdf_xchg_allreduce(self.h, C.c_void_p(d_ptr), int(count), C.c_void_p(stream)))

    def xchg_fuse(self, on):
        """on: every following eval_device is a complete multi-GPU step (exchange inside the fused launch)."""
        self._check(self.lib.isdf_xchg_fuse(self.h, 1 if on else 0))

    def xchg_status(self):
        return int(self.lib.isdf_xchg_status(self.h))

    def xchg_timeout_ms(self):
        """bound of every wait of the exchange, milliseconds of the device wall clock"""
        return float(self.lib.isdf_xchg_timeout_ms(self.h))

    def xchg_set_timeout_ms(self, ms):
        self._check(self.lib.isdf_xchg_set_timeout_ms(self.h, float(ms)))

    def xchg_destroy(self):
        self._check(self.lib.isdf_xchg_destroy(self.h))

    def set_shard(self, rank, world):
        self._check(self.lib.isdf_set_shard(self.h, rank, world))

    # ---- per-step, host buffers (drop-in semantics: accumulate)
    def eval(self, T_list, coeffs_list, tstar=None, accumulate_into=None):
        """T_list[b]: N_b durations; coeffs_list[b]: 18*N_b doubles, column-major 6N x 3.
        Returns (cost[n_traj], [gradT_b], [gradC_b]); pass accumulate_into=(cost, gTs, gCs) to add into existing
        buffers exactly like the reference's += on cost / gradT / gradC."""
        n = len(T_list)
        Ts = [np.ascontiguousarray(t, dtype=np.float64) for t in T_list]
        Cs = [np.ascontiguousarray(c, dtype=np.float64).reshape(-1) for c in coeffs_list]
        Ns = (C.c_int * n)(*[t.size for t in Ts])
        for t, c in zip(Ts, Cs):
            if c.size != 18 * t.size:
                raise ValueError("coeffs must hold 18*N doubles (6N x 3 column-major)")
        if accumulate_into is None:
            cost = np.zeros(n)
            gTs = [np.zeros(t.size) for t in Ts]
            gCs = [np.zeros(18 * t.size) for t in Ts]
        else:
            cost, gTs, gCs = accumulate_into
        arr = lambda xs: (_dp * n)(*[_p(x) for x in xs])
        self._check(self.lib.isdf_eval(self.h, n, Ns, arr(Ts), arr(Cs), _p(cost), arr(gTs), arr(gCs),
                                       None if tstar is None else _p(tstar)))
        return cost, gTs, gCs

    def eval_single(self, T, coeffs_colmajor, tstar=None):
        cost, gT, gC = self.eval([T], [coeffs_colmajor], tstar=tstar)
        return float(cost[0]), gT[0], gC[0]

    # ---- per-step, device-resident (async on `stream`); arguments are raw device pointers (ints)
    def eval_device(self, n_traj, N, d_T, d_coeffs, d_out, d_tstar=0, stream=0):
        self._check(self.lib.isdf_eval_device(self.h, n_traj, N, C.c_void_p(d_T), C.c_void_p(d_coeffs),
                                              C.c_void_p(d_out), C.c_void_p(d_tstar), C.c_void_p(stream)))

    def eval_swept_at_tstar(self, N, d_T, d_coeffs, d_out, d_tstar, stream=0):
        """The swept-volume sweep's back-prop at GIVEN minimisers (device pointers; a negative t* = no interval)."""
        self._check(self.lib.isdf_eval_swept_at_tstar(self.h, N, C.c_void_p(d_T), C.c_void_p(d_coeffs), C.c_void_p(d_out),
                                                      C.c_void_p(d_tstar), C.c_void_p(stream)))

    def eval_swept_at_tstar_host(self, T, coeffs_colmajor, tstar):
        """Host arrays in, (cost, gradT, gradC) of the swept-volume sweep evaluated AT the given minimisers out."""
        T = np.ascontiguousarray(T, dtype=np.float64); N = T.size
        Cc = np.ascontiguousarray(coeffs_colmajor, dtype=np.float64).reshape(-1)
        ts = np.ascontiguousarray(tstar, dtype=np.float64)
        cost = np.zeros(1); gT = np.zeros(N); gC = np.zeros(18 * N)
        self._check(self.lib.isdf_eval_swept_at_tstar_host(self.h, N, _p(T), _p(Cc), _p(ts), _p(cost), _p(gT), _p(gC)))
        return float(cost[0]), gT, gC

    def out_stride(self, N):
        return int(self.lib.isdf_out_stride(N))

    # ---- swept-volume field and mesh (isdf_swept_sdf, isdf_swept_mesh_*)
    def swept_sdf(self, T, coeffs_colmajor, xyz, mode=capi.SWEPT_FIELD_PLANNER):
        """The swept-volume SDF of the trajectory at the points xyz (n x 3): (value, t*); no qualifying interval: (10, -1)."""
        T = np.ascontiguousarray(T, dtype=np.float64); N = T.size
        Cc = np.ascontiguousarray(coeffs_colmajor, dtype=np.float64).reshape(-1)
        xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        n = xyz.shape[0]
        val = np.zeros(n); ts = np.zeros(n)
        self._check(self.lib.isdf_swept_sdf(self.h, N, _p(T), _p(Cc), _p(xyz), n, int(mode), _p(val), _p(ts)))
        return val, ts

    def swept_sdf_device(self, N, d_T, d_coeffs, d_xyz, n, d_value, d_tstar=0, mode=capi.SWEPT_FIELD_PLANNER, stream=0):
        self._check(self.lib.isdf_swept_sdf_device(self.h, N, C.c_void_p(d_T), C.c_void_p(d_coeffs), C.c_void_p(d_xyz), n, int(mode),
                                                   C.c_void_p(d_value), C.c_void_p(d_tstar), C.c_void_p(stream)))

    def swept_mesh(self, T, coeffs_colmajor, eps, iso=0.0, mode=capi.SWEPT_FIELD_CLOSED, band=4, bbox=None, lipschitz=1.0):
        """Surface mesh of the swept volume: (V (nV x 3), F (nF x 3, int32, zero based), info dict).  bbox: ((x, y, z), (x, y, z))."""
        T = np.ascontiguousarray(T, dtype=np.float64); N = T.size
        Cc = np.ascontiguousarray(coeffs_colmajor, dtype=np.float64).reshape(-1)
        p = capi.IsdfSweptMeshParams()
        self.lib.isdf_swept_mesh_params_default(C.byref(p))
        p.eps, p.iso, p.mode, p.band, p.lipschitz = float(eps), float(iso), int(mode), int(band), float(lipschitz)
        if bbox is not None:
            p.use_bbox = 1
            for a in range(3):
                p.bmin[a], p.bmax[a] = float(bbox[0][a]), float(bbox[1][a])
        info = capi.IsdfSweptMeshInfo()
        self._check(self.lib.isdf_swept_mesh_build(self.h, N, _p(T), _p(Cc), C.byref(p), C.byref(info)))
        return self._kept_mesh(info)

    def _kept_mesh(self, info):
        nV, nF = int(info.n_vertices), int(info.n_triangles)
        V = np.zeros((nV, 3)); F = np.zeros((nF, 3), dtype=np.int32)
        self._check(self.lib.isdf_swept_mesh_get(self.h, _p(V), nV, F.ctypes.data_as(C.POINTER(C.c_int32)), nF))
        d = {name: (list(getattr(info, name)) if name in ("dims", "origin") else getattr(info, name))
             for name, _ in capi.IsdfSweptMeshInfo._fields_ if name != "reserved"}
        return V, F, d

    def lattice_mesh(self, f, origin, eps, iso=0.0):
        """Marching tetrahedra (the swept mesh's rule) on a caller's lattice field f (nx x ny x nz, NaN = node not evaluated):
        (V, F, info) as swept_mesh gives them.  Needs no shape, grid or trajectory."""
        f = np.ascontiguousarray(f, dtype=np.float64)
        if f.ndim != 3:
            raise ValueError("lattice_mesh: f must be a 3-D array")
        dims = (C.c_int32 * 3)(*f.shape)
        org = np.ascontiguousarray(origin, dtype=np.float64).reshape(3)
        info = capi.IsdfSweptMeshInfo()
        self._check(self.lib.isdf_lattice_mesh_build(self.h, dims, _p(org), float(eps), float(iso), _p(f), C.byref(info)))
        return self._kept_mesh(info)

    def swept_mesh_release(self):
        self._check(self.lib.isdf_swept_mesh_release(self.h))

    def write_obj(self, path, V, F):
        return write_obj(path, V, F, self.lib)

    # ---- trajectory clearance against the whole occupancy grid (isdf_traj_check*, isdf_traj_collide)
    def _traj_check_params(self, margin, mode):
        p = capi.IsdfTrajCheckParams()
        self.lib.isdf_traj_check_params_default(C.byref(p))
        if margin is not None:
            p.margin = float(margin)
        p.mode = int(mode)
        return p

    @staticmethod
    def _traj_check_report(info, piece_min):
        d = {name: (np.array(getattr(info, name)) if name == "min_point" else getattr(info, name))
             for name, _ in capi.IsdfTrajCheckInfo._fields_}
        d["piece_min"] = piece_min
        return d

    def traj_check(self, T, coeffs_colmajor, margin=None, mode=capi.SWEPT_FIELD_PLANNER):
        """Clearance of the trajectory's swept volume against every occupied voxel centre of the ctx's occupancy grid: a dict of the
        isdf_traj_check_info fields and "piece_min" (N,).  margin None = cfg.safety_hor.  The points below the margin: traj_check_points()."""
        T = np.ascontiguousarray(T, dtype=np.float64); N = T.size
        Cc = np.ascontiguousarray(coeffs_colmajor, dtype=np.float64).reshape(-1)
        p = self._traj_check_params(margin, mode)
        info = capi.IsdfTrajCheckInfo()
        piece_min = np.zeros(N)
        self._check(self.lib.isdf_traj_check(self.h, N, _p(T), _p(Cc), C.byref(p), C.byref(info), _p(piece_min)))
        self._traj_check_rows = int(info.n_below_margin)
        self._traj_check_N = N
        return self._traj_check_report(info, piece_min)

    def traj_check_device(self, N, d_T, d_coeffs, margin=None, mode=capi.SWEPT_FIELD_PLANNER, d_piece_min=0, stream=0):
        """The same with the trajectory (and, if given, the N per-piece minima) on the device; "piece_min" of the dict is None."""
        p = self._traj_check_params(margin, mode)
        info = capi.IsdfTrajCheckInfo()
        self._check(self.lib.isdf_traj_check_device(self.h, N, C.c_void_p(d_T), C.c_void_p(d_coeffs), C.byref(p), C.byref(info),
                                                    C.c_void_p(d_piece_min), C.c_void_p(stream)))
        self._traj_check_rows = int(info.n_below_margin)
        return self._traj_check_report(info, None)

    def traj_check_points(self):
        """The last check's points below the margin in voxel order: rows (x, y, z, value, t*)."""
        rows = np.zeros((getattr(self, "_traj_check_rows", 0), 5))
        self._check(self.lib.isdf_traj_check_get(self.h, _p(rows), rows.shape[0]))
        return rows

    def traj_check_release(self):
        self._check(self.lib.isdf_traj_check_release(self.h))

    # ---- the kept report folded across map updates (isdf_traj_check_set_watch)
    def traj_check_set_watch(self, mode):
        """isdf_traj_check_set_watch: 0 - a map update leaves the kept report alone (default); 1 - every successful check arms a watch and
        every update_pointcloud / update_voxels that occupies a voxel folds the new voxels into the kept report."""
        self._check(self.lib.isdf_traj_check_set_watch(self.h, int(mode)))
        self._watch_mode = int(mode)

    def _watch_refresh_rows(self):
        # a fold changes the number of kept rows traj_check_points() sizes its array by
        if getattr(self, "_watch_mode", 0) != 1:
            return
        info = capi.IsdfTrajCheckInfo()
        if self.lib.isdf_traj_check_watch_info(self.h, C.byref(info), None, None) == 0:
            self._traj_check_rows = int(info.n_below_margin)

    def traj_check_watch_info(self, N=None):
        """isdf_traj_check_watch_info: (report, last) - the current folded report as traj_check returns it ("piece_min": N values; N
        None = the N of the last traj_check, None when unknown) and the isdf_traj_watch_info fields of the last fold as a dict."""
        N = getattr(self, "_traj_check_N", None) if N is None else int(N)
        info = capi.IsdfTrajCheckInfo(); last = capi.IsdfTrajWatchInfo()
        piece_min = np.zeros(N) if N else None
        self._check(self.lib.isdf_traj_check_watch_info(self.h, C.byref(info), _p(piece_min) if N else None, C.byref(last)))
        self._traj_check_rows = int(info.n_below_margin)
        return (self._traj_check_report(info, piece_min),
                {name: getattr(last, name) for name, _ in capi.IsdfTrajWatchInfo._fields_ if name != "reserved"})

    def traj_check_fold_host(self, a, rows_a, vox_a, b, rows_b, vox_b):
        """isdf_traj_check_fold_host (no ctx, no device): two report dicts as traj_check returns them (IsdfTrajCheckInfo fields and
        "piece_min"), over DISJOINT voxel sets, with their rows (n x 5) and ascending voxel ids -> (report, rows, vox) of the union."""
        return traj_check_fold_host(a, rows_a, vox_a, b, rows_b, vox_b, self.lib)

    def traj_collide(self, T, coeffs_colmajor):
        """isTrajCollide: True if an occupied voxel centre lies inside the swept volume (default parameters)."""
        T = np.ascontiguousarray(T, dtype=np.float64)
        Cc = np.ascontiguousarray(coeffs_colmajor, dtype=np.float64).reshape(-1)
        rc = self.lib.isdf_traj_collide(self.h, T.size, _p(T), _p(Cc))
        if rc < 0:
            self._check(rc)
        return bool(rc)

    # ---- dynamic limits of a trajectory and its per-time state (isdf_traj_limits*, isdf_traj_sample*)
    def traj_limits(self, T, coeffs_colmajor, **params):
        """Largest speed, acceleration, body rate, tilt, thrust and smallest thrust of the trajectory: a dict of the
        isdf_traj_limits_info fields (arrays of 6, capi.LIMIT_*) and "piece_out" (N x 12).  params: samples, tol_t, max_acc, max_thrust,
        min_thrust (None: not judged); speed, body rate and tilt are judged against the configuration's vmax, omgmax, thetamax."""
        T, Cc = _traj_arrays(T, coeffs_colmajor)
        p = traj_limits_params(self.lib, **params)
        info = capi.IsdfTrajLimitsInfo()
        piece = np.zeros((T.size, 12))
        self._check(self.lib.isdf_traj_limits(self.h, T.size, _p(T), _p(Cc), C.byref(p), C.byref(info), _p(piece)))
        return traj_limits_report(info, piece)

    def traj_limits_batch(self, T, coeffs_colmajor, **params):
        """B trajectories of N pieces each (T: B x N, coefficients: B x 18 N) in one call: a list of B dicts."""
        T, Cc, B, N = _traj_batch_arrays(T, coeffs_colmajor)
        p = traj_limits_params(self.lib, **params)
        infos = (capi.IsdfTrajLimitsInfo * B)()
        piece = np.zeros((B, N, 12))
        self._check(self.lib.isdf_traj_limits_batch(self.h, B, N, _p(T), _p(Cc), C.byref(p), infos, _p(piece)))
        return [traj_limits_report(infos[b], piece[b]) for b in range(B)]

    def traj_limits_device(self, N, d_T, d_coeffs, d_piece_out=0, stream=0, **params):
        """The same with the trajectory (and, if given, the N x 12 per-piece rows) on the device; "piece_out" of the dict is None."""
        p = traj_limits_params(self.lib, **params)
        info = capi.IsdfTrajLimitsInfo()
        self._check(self.lib.isdf_traj_limits_device(self.h, N, C.c_void_p(d_T), C.c_void_p(d_coeffs), C.byref(p), C.byref(info),
                                                     C.c_void_p(d_piece_out), C.c_void_p(stream)))
        return traj_limits_report(info, None)

    def traj_sample(self, T, coeffs_colmajor, t):
        """The state at the time stamps t: rows pos3 | vel3 | acc3 | jer3 | quat4 | omg3 | thr (psi = 0)."""
        T, Cc = _traj_arrays(T, coeffs_colmajor)
        t = np.ascontiguousarray(t, dtype=np.float64).reshape(-1)
        rows = np.zeros((t.size, capi.TRAJ_SAMPLE_ROW))
        self._check(self.lib.isdf_traj_sample(self.h, T.size, _p(T), _p(Cc), t.size, _p(t), _p(rows)))
        return rows

    def traj_sample_device(self, N, d_T, d_coeffs, n, d_t, d_rows, stream=0):
        self._check(self.lib.isdf_traj_sample_device(self.h, N, C.c_void_p(d_T), C.c_void_p(d_coeffs), n, C.c_void_p(d_t), C.c_void_p(d_rows),
                                                     C.c_void_p(stream)))

    # ---- retiming a trajectory to its dynamic limits (isdf_traj_retime*)
    def _note_check(self, info):        # a result that went through the clearance check left that check's kept rows in the ctx
        if info.checked:
            self._traj_check_rows = int(info.check.n_below_margin)

    def traj_retime(self, T, coeffs_colmajor, **params):
        """The smallest uniform slow-down factor of a ladder search at which the limits report is feasible, and the trajectory scaled by
        it: the dict of traj_retime_report.  params: s_lo, s_hi, ladder, rounds, check (True: the result goes through the clearance
        check, "check" of the dict), and the limits' keywords (samples, tol_t, max_acc, max_thrust, min_thrust)."""
        T, Cc = _traj_arrays(T, coeffs_colmajor)
        p = traj_retime_params(self.lib, **params)
        info = capi.IsdfTrajRetimeInfo()
        To, Co = np.zeros_like(T), np.zeros_like(Cc)
        self._check(self.lib.isdf_traj_retime(self.h, T.size, _p(T), _p(Cc), C.byref(p), _p(To), _p(Co), C.byref(info)))
        self._note_check(info)
        return traj_retime_report(info, To, Co)

    def traj_retime_batch(self, T, coeffs_colmajor, **params):
        """B trajectories of N pieces each (T: B x N, coefficients: B x 18 N), each with its own brackets and status: a list of B dicts."""
        T, Cc, B, N = _traj_batch_arrays(T, coeffs_colmajor)
        p = traj_retime_params(self.lib, **params)
        infos = (capi.IsdfTrajRetimeInfo * B)()
        To, Co = np.zeros_like(T), np.zeros_like(Cc)
        self._check(self.lib.isdf_traj_retime_batch(self.h, B, N, _p(T), _p(Cc), C.byref(p), _p(To), _p(Co), infos))
        return [traj_retime_report(infos[b], To[b], Co[b]) for b in range(B)]

    def traj_retime_device(self, N, d_T, d_coeffs, d_T_out, d_coeffs_out, stream=0, **params):
        """The same with every array on the device (d_T_out: N, d_coeffs_out: 18 N doubles); "T" and "coeffs" of the dict are None."""
        p = traj_retime_params(self.lib, **params)
        info = capi.IsdfTrajRetimeInfo()
        self._check(self.lib.isdf_traj_retime_device(self.h, N, C.c_void_p(d_T), C.c_void_p(d_coeffs), C.byref(p), C.c_void_p(d_T_out),
                                                     C.c_void_p(d_coeffs_out), C.byref(info), C.c_void_p(stream)))
        self._note_check(info)
        return traj_retime_report(info)

    # ---- re-allocating piece durations to the dynamic limits (isdf_traj_realloc*)
    def traj_realloc(self, head_pva, tail_pva, Q, T, **params):
        """Slows down only the pieces that are over a limit, keeps the waypoints Q and solves MINCO again, until the limits report is
        clean: the dict of traj_realloc_report.  params: rounds, headroom, f_max, check (True: the result goes through the clearance
        check), and the limits' keywords (samples, tol_t, max_acc, max_thrust, min_thrust)."""
        h, t, q, T = _realloc_arrays(head_pva, tail_pva, Q, T)
        p = traj_realloc_params(self.lib, **params)
        info = capi.IsdfTrajReallocInfo()
        To, Co = np.zeros_like(T), np.zeros(18 * T.size)
        self._check(self.lib.isdf_traj_realloc(self.h, T.size, _p(h), _p(t), _p(q), _p(T), C.byref(p), _p(To), _p(Co), C.byref(info)))
        self._note_check(info)
        return traj_realloc_report(info, To, Co)

    def traj_realloc_batch(self, heads, tails, Q, T, **params):
        """B trajectories of N pieces each (heads, tails: B x 9; Q: B x (N - 1) x 3; T: B x N), each with its own status: a list of B dicts."""
        T, _, B, N = _traj_batch_arrays(T)
        h = np.ascontiguousarray(heads, dtype=np.float64).reshape(B, 9)
        t = np.ascontiguousarray(tails, dtype=np.float64).reshape(B, 9)
        q = np.ascontiguousarray(Q, dtype=np.float64).reshape(B, 3 * (N - 1)) if N > 1 else np.zeros((B, 3))
        p = traj_realloc_params(self.lib, **params)
        infos = (capi.IsdfTrajReallocInfo * B)()
        To, Co = np.zeros_like(T), np.zeros((B, 18 * N))
        self._check(self.lib.isdf_traj_realloc_batch(self.h, B, N, _p(h), _p(t), _p(q), _p(T), C.byref(p), _p(To), _p(Co), infos))
        return [traj_realloc_report(infos[b], To[b], Co[b]) for b in range(B)]

    def traj_realloc_device(self, N, d_head, d_tail, d_Q, d_T, d_T_out, d_coeffs_out, stream=0, **params):
        """The same with every array on the device (d_head, d_tail: 9; d_Q: 3 (N - 1); d_T, d_T_out: N; d_coeffs_out: 18 N doubles);
        "T" and "coeffs" of the dict are None."""
        p = traj_realloc_params(self.lib, **params)
        info = capi.IsdfTrajReallocInfo()
        self._check(self.lib.isdf_traj_realloc_device(self.h, N, C.c_void_p(d_head), C.c_void_p(d_tail), C.c_void_p(d_Q), C.c_void_p(d_T), C.byref(p),
                                                      C.c_void_p(d_T_out), C.c_void_p(d_coeffs_out), C.byref(info), C.c_void_p(stream)))
        self._note_check(info)
        return traj_realloc_report(info)

    def points_merge_check(self, below=None):
        """Merges the last check's kept points with value < below (None: all of them) into the obstacle-point set on the device: the
        isdf_points_merge_info fields as a dict.  New points are appended in voxel order; existing ones keep index and lastTstar."""
        info = capi.IsdfPointsMergeInfo()
        self._check(self.lib.isdf_points_merge_check(self.h, -1.0 if below is None else float(below), C.byref(info)))
        return {name: getattr(info, name) for name, _ in capi.IsdfPointsMergeInfo._fields_ if name != "reserved"}

    # ---- full objective callback (TrajOptimizer::costFunctionLmbm)
    def set_trajectory(self, N, head_pva, tail_pva, rho):
        """head/tail: 3x3 arrays whose COLUMNS are position, velocity, acceleration (Eigen::Matrix3d of setConditions)."""
        h = np.ascontiguousarray(np.asarray(head_pva, dtype=np.float64).T).reshape(-1)   # column-major
        t = np.ascontiguousarray(np.asarray(tail_pva, dtype=np.float64).T).reshape(-1)
        self._check(self.lib.isdf_set_trajectory(self.h, int(N), _p(h), _p(t), float(rho)))
        self._N = int(N)

    def num_variables(self):
        return int(self.lib.isdf_num_variables(self.h))

    def pack_variables(self, T, waypoints):
        """T: N durations, waypoints: (N-1) x 3 -> x = [tau | xi]."""
        T = np.ascontiguousarray(T, dtype=np.float64)
        W = np.ascontiguousarray(np.asarray(waypoints, dtype=np.float64).reshape(-1))
        x = np.zeros(self.num_variables())
        self._check(self.lib.isdf_pack_variables(self.h, _p(T), _p(W) if W.size else None, _p(x)))
        return x

    def unpack_variables(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        T = np.zeros(self._N)
        cm = np.zeros(18 * self._N)
        self._check(self.lib.isdf_unpack_variables(self.h, _p(x), _p(T), _p(cm)))
        return T, cm

    def cost_function(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        g = np.zeros_like(x)
        cost = C.c_double(0)
        self._check(self.lib.isdf_cost_function(self.h, _p(x), _p(g), x.size, C.byref(cost)))
        return cost.value, g

    def cost_function_launch(self, x, stream=0):
        """Multi-GPU form, first half: returns (device pointer, count) of this rank's partial sums (to be all-reduced)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        self._cb_x = x
        ptr = C.c_void_p()
        cnt = C.c_size_t(0)
        self._check(self.lib.isdf_cost_function_launch(self.h, _p(x), x.size, C.c_void_p(stream), C.byref(ptr), C.byref(cnt)))
        return ptr.value, cnt.value

    def cost_function_finish(self, stream=0):
        g = np.zeros_like(self._cb_x)
        cost = C.c_double(0)
        self._check(self.lib.isdf_cost_function_finish(self.h, _p(g), C.byref(cost), C.c_void_p(stream)))
        return cost.value, g

    def set_minco_mode(self, mode):
        """capi.MINCO_AUTO (default): wherever it is faster; capi.MINCO_HOST: the host's band LU; capi.MINCO_DEVICE: the device kernels."""
        self._check(self.lib.isdf_set_minco_mode(self.h, int(mode)))

    def minco_path(self):
        """Where the last callback ran MINCO: 1 = device, 0 = host."""
        return int(self.lib.isdf_minco_path(self.h))

    def cost_parts(self):
        p = np.zeros(4)
        self._check(self.lib.isdf_cost_parts(self.h, _p(p)))
        return {"energy": p[0], "swept": p[1], "integral": p[2], "time": p[3]}

    # ---- optimizer driver (lbfgs::lbfgs_optimize behind the callback)
    def set_progress(self, fn, n_traj=1):
        """fn(traj, x, g, fx, step, k, ls) -> truthy cancels that trajectory (isdf_set_progress; None removes the hook).  In the batch
        driver the hook runs on the trajectories' host threads: trajectory t's instance is the t-th int of an array (stride 4)."""
        if fn is None:
            self._progress_keep = None
            self._check(self.lib.isdf_set_progress(self.h, None, None, 0))
            return
        n = self.num_variables()
        ids = (C.c_int * max(1, int(n_traj)))(*range(max(1, int(n_traj))))

        def tramp(inst, xp, gp, fx, step, k, ls):
            t = C.cast(inst, C.POINTER(C.c_int))[0]
            return 1 if fn(t, np.ctypeslib.as_array(xp, shape=(n,)).copy(), np.ctypeslib.as_array(gp, shape=(n,)).copy(), fx, step, k, ls) else 0
        cb = capi.PROGRESS_FN(tramp)
        self._progress_keep = (cb, ids)
        self._check(self.lib.isdf_set_progress(self.h, C.cast(cb, C.c_void_p), C.cast(ids, C.c_void_p), 4))

    def optimize_lbfgs(self, x0, **params):
        """Returns (x, result dict).  params override lbfgs_parameter_t defaults (mem_size, max_iterations, ...)."""
        x = np.ascontiguousarray(x0, dtype=np.float64).copy()
        p = lbfgs_params(self.lib, **params)
        r = capi.IsdfLbfgsResult()
        self._check(self.lib.isdf_optimize_lbfgs(self.h, _p(x), x.size, C.byref(p), C.byref(r)))
        return x, {"f": r.f, "status": r.status, "iterations": r.iterations, "evaluations": r.evaluations, "wall_ms": r.wall_ms}

    def optimize_lbfgs_checked(self, x0, lbfgs_params=None, max_rounds=4, margin=None, below=None, mode=capi.SWEPT_FIELD_PLANNER):
        """optimise -> traj_check -> points_merge_check until the check is clear, a merge adds nothing or max_rounds is reached
        (isdf_optimize_lbfgs_checked).  lbfgs_params: a dict of overrides as optimize_lbfgs takes them.  Returns (x, dict) with
        "rounds", "clear", "stalled", "M_round" (one entry per round, at most 16), "last_opt" and "last_check" (dicts)."""
        x = np.ascontiguousarray(x0, dtype=np.float64).copy()
        p = _lbfgs_params(self.lib, **(lbfgs_params or {}))
        rp = capi.IsdfRefineParams()
        self.lib.isdf_refine_params_default(C.byref(rp))
        rp.max_rounds, rp.mode = int(max_rounds), int(mode)
        if margin is not None:
            rp.margin = float(margin)
        if below is not None:
            rp.below = float(below)
        r = capi.IsdfRefineResult()
        self._check(self.lib.isdf_optimize_lbfgs_checked(self.h, _p(x), x.size, C.byref(p), C.byref(rp), C.byref(r)))
        self._traj_check_rows = int(r.last_check.n_below_margin)
        o = r.last_opt
        return x, {"rounds": r.rounds, "clear": bool(r.clear), "stalled": bool(r.stalled), "M_round": list(r.M_round)[:min(r.rounds, 16)],
                   "last_opt": {"f": o.f, "status": o.status, "iterations": o.iterations, "evaluations": o.evaluations, "wall_ms": o.wall_ms},
                   "last_check": self._traj_check_report(r.last_check, None)}

    def optimize_lbfgs_batch(self, N, heads, tails, rho, x0s, **params):
        """heads / tails: n_traj x 3 x 3 (columns pos, vel, acc); x0s: n_traj x n.  Returns (xs, [result dicts], wall_ms)."""
        x = np.ascontiguousarray(x0s, dtype=np.float64).copy()
        n_traj = x.shape[0]
        h = np.ascontiguousarray(np.asarray(heads, dtype=np.float64).transpose(0, 2, 1)).reshape(-1)     # column-major 3x3 each
        t = np.ascontiguousarray(np.asarray(tails, dtype=np.float64).transpose(0, 2, 1)).reshape(-1)
        p = lbfgs_params(self.lib, **params)
        res = (capi.IsdfLbfgsResult * n_traj)()
        wall = C.c_double(0)
        self._check(self.lib.isdf_optimize_lbfgs_batch(self.h, n_traj, int(N), _p(h), _p(t), float(rho), _p(x), C.byref(p), res, C.byref(wall)))
        out = [{"f": r.f, "status": r.status, "iterations": r.iterations, "evaluations": r.evaluations, "rounds": r.reserved} for r in res]
        return x, out, wall.value

    # ---- mid end (OriTraj::getOriTraj: the MINCO fit to the front end's waypoints, whose x the back end starts from)
    def midend_params(self, **kw):
        """isdf_midend_params_default with overrides (weight_pr, rho_mid_end, rel_cost_tol, min_step, g_epsilon, integral_intervs,
        mem_size, past)."""
        return midend_params(self.lib, **kw)

    def midend_cost(self, ref_points, x, params=None):
        """ref_points: (N-1) x 3.  Returns (cost, g, {"energy", "pose", "time"}) - isdf_midend_cost on isdf_set_trajectory's ends."""
        p = params or midend_params(self.lib)
        R = np.ascontiguousarray(np.asarray(ref_points, dtype=np.float64).reshape(-1))
        x = np.ascontiguousarray(x, dtype=np.float64)
        g = np.zeros_like(x); parts = np.zeros(3); cost = C.c_double(0)
        self._check(self.lib.isdf_midend_cost(self.h, C.byref(p), _p(R), _p(x), _p(g), x.size, C.byref(cost), _p(parts)))
        return cost.value, g, {"energy": parts[0], "pose": parts[1], "time": parts[2]}

    def midend_cost_batch(self, heads, tails, ref_points, xs, params=None):
        """heads / tails: nb x 3 x 3 (columns pos, vel, acc); ref_points: nb x (N-1) x 3; xs: nb x n.  Returns (costs, gs)."""
        p = params or midend_params(self.lib)
        x = np.ascontiguousarray(xs, dtype=np.float64)
        nb = x.shape[0]
        h = np.ascontiguousarray(np.asarray(heads, dtype=np.float64).transpose(0, 2, 1)).reshape(-1)
        t = np.ascontiguousarray(np.asarray(tails, dtype=np.float64).transpose(0, 2, 1)).reshape(-1)
        R = np.ascontiguousarray(np.asarray(ref_points, dtype=np.float64).reshape(-1))
        g = np.zeros_like(x); cost = np.zeros(nb)
        self._check(self.lib.isdf_midend_cost_batch(self.h, C.byref(p), nb, _p(h), _p(t), _p(R), _p(x), _p(g), _p(cost)))
        return cost, g

    def midend_fit(self, ref_points, T_init, params=None):
        """Returns (x, T, coeffs 18N column-major, result dict); x is isdf_optimize_lbfgs's start (isdf_midend_fit)."""
        p = params or midend_params(self.lib)
        R = np.ascontiguousarray(np.asarray(ref_points, dtype=np.float64).reshape(-1))
        T0 = np.ascontiguousarray(T_init, dtype=np.float64)
        N = T0.size
        x = np.zeros(N + 3 * (N - 1)); T = np.zeros(N); cm = np.zeros(18 * N)
        r = capi.IsdfLbfgsResult()
        self._check(self.lib.isdf_midend_fit(self.h, C.byref(p), _p(R), _p(T0), _p(x), _p(T), _p(cm), C.byref(r)))
        return x, T, cm, {"f": r.f, "status": r.status, "iterations": r.iterations, "evaluations": r.evaluations, "wall_ms": r.wall_ms}

    def midend_fit_batch(self, heads, tails, ref_points, T_inits, params=None):
        """heads / tails: nb x 3 x 3; ref_points: nb x (N-1) x 3; T_inits: nb x N.  Returns (xs, [result dicts], wall_ms)."""
        p = params or midend_params(self.lib)
        T0 = np.ascontiguousarray(T_inits, dtype=np.float64)
        nb, N = T0.shape
        h = np.ascontiguousarray(np.asarray(heads, dtype=np.float64).transpose(0, 2, 1)).reshape(-1)
        t = np.ascontiguousarray(np.asarray(tails, dtype=np.float64).transpose(0, 2, 1)).reshape(-1)
        R = np.ascontiguousarray(np.asarray(ref_points, dtype=np.float64).reshape(-1))
        x = np.zeros((nb, N + 3 * (N - 1)))
        res = (capi.IsdfLbfgsResult * nb)()
        wall = C.c_double(0)
        self._check(self.lib.isdf_midend_fit_batch(self.h, C.byref(p), nb, N, _p(h), _p(t), _p(R), _p(T0), _p(x), res, C.byref(wall)))
        out = [{"f": r.f, "status": r.status, "iterations": r.iterations, "evaluations": r.evaluations, "rounds": r.reserved} for r in res]
        return x, out, wall.value

    # ---- instrumentation
    def mesh_info(self):
        """isdf_mesh_info as a dict (faces, nodes, depth, wg, closed, solid, lattice dims, measured |1 - 2w| range)"""
        a = (C.c_int * 16)()
        self._check(self.lib.isdf_mesh_info(self.h, a))
        return {"faces": a[0], "nodes": a[1], "depth": a[2], "wg": a[3], "closed": a[4], "solid": a[5], "lattice": (a[6], a[7], a[8]),
                "s_range": (a[9] * 1e-6, a[10] * 1e-6), "flat_slots": a[11],
                "defect_thickness": a[12] * 1e-9, "defect_s": a[13] * 1e-3}

    def multi_info(self):
        n = C.c_int(0); m = C.c_int(0)
        self._check(self.lib.isdf_multi_info(self.h, C.byref(n), C.byref(m)))
        return n.value, m.value

    def host_path(self):
        """How the last host-array step crossed PCIe (capi.HOST_PATH_*)."""
        return int(self.lib.isdf_host_path(self.h))

    def stats(self):
        s = capi.IsdfStats()
        self._check(self.lib.isdf_get_stats(self.h, C.byref(s)))
        return {"units": s.n_units, "culled": s.n_units_culled, "pairs": s.n_pairs,
                "grad_pairs": s.n_grad_pairs, "overflow": s.overflow}

    def profile_enable(self, every=1, secondary=False):
        """every = N > 0: instrument every N-th eval_device (dominant kernel; secondary=True: also the kernel after it);
        0/False: off."""
        every = int(every)
        self._check(self.lib.isdf_profile_enable(self.h, every | (0x10000 if (secondary and every > 0) else 0)))

    def profile_read(self):
        n = C.c_int(0)
        ms = C.c_double(0)
        self._check(self.lib.isdf_profile_read(self.h, C.byref(n), C.byref(ms)))
        return n.value, ms.value

    def profile_read_secondary(self):
        ms = C.c_double(0)
        self._check(self.lib.isdf_profile_read_secondary(self.h, C.byref(ms)))
        return ms.value
