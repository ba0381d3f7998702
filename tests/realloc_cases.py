"""Inputs of the re-allocation tests (isdf_traj_realloc*), shared by the host and the device test files: seeded waypoint problems at
rest at both ends (in the style of tests/retime_cases.py: limits chosen so that known things bind), the test shim, and helpers that
hold a result to the rules of include/isdf_accel.h through INDEPENDENT calls of the solve and of the limits report."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "implicit-sdf-planner_amd", "csrc")

OVER = dict(vmax=2.0, omgmax=2.5, thetamax=0.6)                 # the configuration's limits: channels 0, 2, 3
KW = dict(max_acc=5.0, max_thrust=9.0, min_thrust=3.0)          # channels 1, 4, 5: every channel is judged


def config(pkg, **over):
    kw = dict(OVER)
    kw.update(over)
    return pkg.synth.default_config(pkg.capi.V1_SWEPT, integral_intervs=4, **kw)


def problem(N, seed, piece_T, jitter=0.4):
    """head[9], tail[9] (position | velocity | acceleration, at rest), Q (N - 1) x 3, T[N]: waypoints along a line of 1.2 m per piece
    with N(0, jitter) noise, durations piece_T * exp(U(-0.2, 0.2))."""
    rng = np.random.default_rng(seed)
    p0 = np.array([1.0, 1.0, 1.0])
    d = rng.normal(0, 1, 3)
    d[2] *= 0.3
    d /= np.linalg.norm(d)
    p1 = p0 + 1.2 * N * d
    lam = np.linspace(0, 1, N + 1)[1:-1]
    Q = p0[None, :] + (p1 - p0)[None, :] * lam[:, None] + rng.normal(0, jitter, (N - 1, 3))
    head = np.concatenate([p0, np.zeros(6)])
    tail = np.concatenate([p1, np.zeros(6)])
    T = np.full(N, float(piece_T)) * np.exp(rng.uniform(-0.2, 0.2, N))
    return dict(N=N, head=head, tail=tail, Q=Q, T=T)


def feasible_case(N, seed=None):
    """Generous durations: nothing binds (status 1)."""
    return problem(N, N if seed is None else seed, piece_T=2.0)


def short_piece_case(N, seed=None):
    """The feasible case with ONE interior piece's duration divided by 4."""
    p = feasible_case(N, seed)
    p["T"] = p["T"].copy()
    p["short"] = N // 2
    p["T"][N // 2] /= 4.0
    return p


def aggressive_case(N, seed=None):
    """Durations far too short for the limits, more scatter: every channel binds somewhere."""
    return problem(N, 100 + (N if seed is None else seed), piece_T=0.45, jitter=0.6)


def args(p):
    return p["head"], p["tail"], p["Q"], p["T"]


def extent(p):
    pts = np.vstack([p["head"][None, :3], p["Q"].reshape(-1, 3), p["tail"][None, :3]])
    return float(np.max(pts.max(axis=0) - pts.min(axis=0)))


def build_shim(out_dir):
    out = os.path.join(str(out_dir), "libtraj_realloc_shim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", CSRC,
                           os.path.join(ROOT, "tests", "native", "traj_realloc_shim.cpp"), "-o", out])
    L = C.CDLL(out)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    L.shim_ra_piece_factor.restype = C.c_double
    L.shim_ra_piece_factor.argtypes = [dp, dp, C.c_double, C.c_double, ip]
    L.shim_ra_update.restype = C.c_double
    L.shim_ra_update.argtypes = [C.c_double, C.c_double]
    L.shim_ra_rounds.restype = None
    L.shim_ra_rounds.argtypes = [C.c_int, ip, ip]
    L.shim_ra_realloc_trace.argtypes = [C.c_void_p, C.c_int, dp, dp, dp, dp, C.c_void_p, dp, dp, C.c_void_p, ip, dp, ip]
    return L


def host_trace(pkg, shim, cfg, p, **params):
    """The host loop through the shim: (the dict of traj_realloc_report, margins per evaluated iterate, per-piece union of masks)."""
    engine = pkg.engine
    lib = pkg.capi.load_library()
    h, t, q, T = engine._realloc_arrays(*args(p))
    pr = engine.traj_realloc_params(lib, **params)
    info = pkg.capi.IsdfTrajReallocInfo()
    To, Co = np.zeros_like(T), np.zeros(18 * T.size)
    evals = C.c_int(0)
    margin = np.zeros(17)
    ever = np.zeros(T.size, dtype=np.int32)
    f = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))      # noqa: E731
    rc = shim.shim_ra_realloc_trace(C.byref(cfg), T.size, f(h), f(t), f(q), f(T), C.byref(pr), f(To), f(Co), C.byref(info), C.byref(evals), f(margin),
                                    ever.ctypes.data_as(C.POINTER(C.c_int)))
    assert rc == 0, rc
    return engine.traj_realloc_report(info, To, Co), margin[:evals.value].copy(), ever


def limits_kw(kw):
    return {k: v for k, v in kw.items() if k in ("samples", "tol_t", "max_acc", "max_thrust", "min_thrust")}


def same_limits(a, b):
    """None, or the first field in which two limits dicts differ (bytes; device_ms and piece_out aside)."""
    for k in a:
        if k in ("device_ms", "piece_out"):
            continue
        if np.asarray(a[k]).tobytes() != np.asarray(b[k]).tobytes():
            return k
    return None


def same_result(a, b):
    """None, or the first field in which two results differ (bytes; device_ms and the check aside)."""
    for k in a:
        if k in ("device_ms", "limits", "check"):
            continue
        if np.asarray(a[k]).tobytes() != np.asarray(b[k]).tobytes():
            return k
    return same_limits(a["limits"], b["limits"])


def hold_common(p, res):
    """What every form's result obeys whatever computed it: durations never shrink, the info's sums and counts are those of the arrays,
    every piece starts at its waypoint (the constant coefficients against head, Q: 1e-12 of the path's extent; they are copies)."""
    T, To = p["T"], res["T"]
    N = len(T)
    assert (To >= T).all()
    assert res["duration_in"] == float(np.add.accumulate(T)[-1]) and res["duration_out"] == float(np.add.accumulate(To)[-1])
    assert res["pieces_changed"] == int((To != T).sum()) and res["max_factor"] == float(np.max(To / T))
    c0 = res["coeffs"].reshape(3, N, 6)[:, :, 0].T                              # N x 3: the pieces' start points
    way = np.vstack([p["head"][None, :3], p["Q"].reshape(-1, 3)])
    assert np.max(np.abs(c0 - way)) <= 1e-12 * extent(p)
    if res["status"] == 1:
        assert res["rounds"] == 0 and To.tobytes() == T.tobytes() and res["binding"] == 0 and res["pieces_changed"] == 0
    feas = res["limits"]["feasible"] == res["limits"]["judged"]
    assert feas == (res["status"] in (0, 1))
    if res["status"] == 0:
        assert res["rounds"] >= 1 and res["binding"] != 0 and res["pieces_changed"] >= 1
