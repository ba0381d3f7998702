"""Host form of the mid end (csrc/midend_host.hpp: OriTraj's objective and fit over minco_host.hpp / lbfgs_host.hpp) against the
reference's own MINCO and L-BFGS (oracle/_ref) with the pose penalty restated in numpy (tests/midend_common.py).  CPU only: the
header is compiled into a test shim with g++."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import midend_common as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "implicit-sdf-planner_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_midend_fit.npz")
dp = C.POINTER(C.c_double)

# Test 3's bounds, shared with tests/test_gpu_midend.py: 10 x what the host form was measured to end from the reference's own run
# (DESIGN 4.10 has the measured values), per case N -> (cost, relative | waypoints, metres | durations, seconds)
FIT_BOUNDS = {3: (2.9e-15, 4.5e-14, 1.6e-14), 8: (1.4e-6, 9.2e-3, 2.6e-3), 40: (3.0e-4, 1.1e-1, 2.5e-2)}


def _p(a):
    return a.ctypes.data_as(dp)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("shim") / "libmidend_shim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", CSRC,
                           os.path.join(ROOT, "tests", "native", "midend_shim.cpp"), "-o", out])
    L = C.CDLL(out)
    L.shim_midend_cost.restype = C.c_double
    return L


@pytest.fixture(scope="module")
def ref_side(orc):
    if not os.path.exists(orc.REF_MINCO):
        pytest.skip("oracle/_ref/libref_minco.so not built")
    return orc


def host_cost(shim, head, tail, ref, x, prm=mc.PRM):
    N = (x.size + 3) // 4
    g = np.zeros_like(x); parts = np.zeros(3); pos = np.zeros(3 * (N - 1)); vel = np.zeros(3 * (N - 1))
    R = np.ascontiguousarray(np.asarray(ref, dtype=np.float64).reshape(-1)); pa = mc.prm_array(prm); xx = np.ascontiguousarray(x, dtype=np.float64)
    c = shim.shim_midend_cost(N, _p(mc.colmajor9(head)), _p(mc.colmajor9(tail)), _p(R), _p(pa), _p(xx), _p(g), _p(parts), _p(pos), _p(vel))
    host_cost.vel = vel.reshape(N - 1, 3)
    return c, g, parts, pos.reshape(N - 1, 3)


def host_fit(shim, head, tail, ref, T0, prm=mc.PRM):
    N = T0.size
    x = np.zeros(N + 3 * (N - 1)); res = np.zeros(4)
    R = np.ascontiguousarray(ref.reshape(-1)); pa = mc.prm_array(prm)
    shim.shim_midend_fit(N, _p(mc.colmajor9(head)), _p(mc.colmajor9(tail)), _p(R), _p(pa), _p(np.ascontiguousarray(T0)), _p(x), _p(res))
    return x, {"f": res[0], "status": int(res[1]), "iterations": int(res[2]), "evaluations": int(res[3])}


def cost_cases(shim):
    """(name, head, tail, ref, x): N = 2, 3, 5, 40 with durations of 0.05 .. 12 s, the 100:1 mix, a waypoint exactly on its sample
    (d = 0: the skipped branch) and one 1e-9 m off it."""
    out = []
    for N in (2, 3, 5, 40):
        out.append((f"N{N}",) + mc.cost_problem(N, 10 + N))
    out.append(("N5-mix100",) + mc.cost_problem(5, 77, mix=True))
    out.append(("N40-mix100",) + mc.cost_problem(40, 78, mix=True))
    for name, off in (("N3-d0", 0.0), ("N3-d1e-9", 1e-9)):
        head, tail, ref, x = mc.cost_problem(3, 91)
        pos = host_cost(shim, head, tail, ref, x)[3]
        ref = ref.copy(); ref[1] = pos[1] + off * np.array([0.6, -0.8, 0.0])
        out.append((name, head, tail, ref, x))
    return out


def assert_close(a, b, rtol, what):
    """rtol relative, with the absolute floor tests/test_oracle_ref.py gives the same MINCO against the same reference
    (1e-12 of the array's largest entry)."""
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    sc = max(float(np.abs(b).max()), 1e-300)
    err = np.abs(a - b) - 1e-12 * sc
    worst = float((err / np.maximum(np.abs(b), 1e-300)).max())
    print(f"{what}: worst relative deviation beyond the floor {max(worst, 0.0):.3e} (bound {rtol:g})")
    assert np.all(err <= rtol * np.abs(b)), (what, worst)


def test_cost_and_gradient_match_the_reference(shim, ref_side):
    """1.  Tolerance: csrc/minco_host.hpp is bitwise the oracle's restatement (tests/test_minco_host.py) and that restatement is held
    to the reference's minco.hpp at 1e-10 relative (tests/test_oracle_ref.py); the penalty adds only products."""
    for name, head, tail, ref, x in cost_cases(shim):
        c, g, parts, pos = host_cost(shim, head, tail, ref, x)
        c0, g0, parts0, cps, _ = mc.ref_cost(ref_side, head, tail, ref, x)
        assert_close([c], [c0], 1e-10, name + " cost")
        assert_close(g, g0, 1e-10, name + " g")
        assert_close(parts, parts0, 1e-10, name + " parts")
        if name == "N3-d0":
            assert cps[1] < 1e-40 and np.isfinite(g).all()          # the skipped branch: no NaN from d / |d|
            c1, g1, _, _ = host_cost(shim, head, tail, np.where(np.arange(2)[:, None] == 1, pos[1], ref), x)
            assert c1 == c and np.array_equal(g1, g)


def test_grad_T_keeps_the_reference_quirk(shim):
    """2.  One constraint (N = 2).  The objective's time gradient carries the penalty's direct term TIMES cost_p
    (mid_end.hpp:256): central differences of the cost in T see w * alpha * gradp.vel, the objective has cost_p times that.  In the
    waypoints the objective's gradient IS the derivative."""
    N, h = 2, 1e-6
    head = np.zeros((3, 3)); tail = np.zeros((3, 3)); tail[:, 0] = [6.0, 0.5, 0.2]; head[0, 1] = 0.4
    way = np.array([[3.0, 0.3, 0.1]]); ref = np.array([[3.6, -0.2, 0.4]])
    T = np.array([1.6, 2.1])
    prm = dict(mc.PRM, integral_intervs=4)          # the sample a quarter into piece 1: a sizeable velocity term
    x = np.concatenate([mc.backward_T(T), way.reshape(-1)])
    c, g, parts, pos = host_cost(shim, head, tail, ref, x, prm)
    vel = host_cost.vel[0].copy()
    F = lambda T_, w_: host_cost(shim, head, tail, ref, np.concatenate([mc.backward_T(T_), w_.reshape(-1)]), prm)[0]
    gT_obj = g[:N] / mc.backward_grad_T(x[:N], np.ones(N))          # undo the tau chain rule
    # the penalty's direct time term as it would be without the quirk (:253): q = w * alpha * gradp . vel
    w, alpha = prm["weight_pr"], 1.0 / prm["integral_intervs"]
    d = pos[0] - ref[0]; nrm = np.linalg.norm(d); cost_p = nrm ** 3
    q = w * alpha * float((3 * nrm ** 2 * (d / nrm)) @ vel)
    fd_T = np.zeros(N)
    for i in range(N):
        Tp = T.copy(); Tp[i] += h; Tm = T.copy(); Tm[i] -= h
        fd_T[i] = (F(Tp, way) - F(Tm, way)) / (2 * h)
    tol_T = 2e-5 * np.maximum(1.0, np.abs(fd_T))        # tests/test_minco_host.py's figure for central differences in T at h = 1e-6
    gap = fd_T - gT_obj
    print(f"cost_p {cost_p:.6g}, q {q:.6g}; fd_T {fd_T}; objective gradT {gT_obj}; gap {gap}")
    assert abs(gap[0]) <= tol_T[0]                      # piece 0 carries no penalty: no quirk there
    # the derivative has q where the objective has cost_p * q: they disagree by (1 - cost_p) q, far beyond the differences' error
    assert abs(gap[1] - (1.0 - cost_p) * q) <= tol_T[1]
    assert abs(gap[1]) > 100 * tol_T[1], (cost_p, q, gap)
    # waypoints: F is quadratic (energy) + w |d|^3 with d affine in the waypoint, d = d0 + t a along coordinate k.  The third
    # derivative of |d0 + t a|^3 in t is bounded by 6 |a|^3, so the central difference is off by at most h^2 / 6 * w * 6 |a|^3.
    # Rounding: an evaluation of F is good to gamma * u * |F| (u = 2^-53) with gamma the floating-point operations on its longest
    # dependency chain - 6N pivots of the band LU with a division and up to 6 multiply-subtracts each, as many again in the two
    # substitutions, about 40 in the energy and penalty sums - and the difference of two of them is divided by 2h
    gamma = 6 * N * 7 + 6 * N * 7 + 40
    for k in range(3):
        wp = way.copy(); wp[0, k] += h; wm = way.copy(); wm[0, k] -= h
        fd = (F(T, wp) - F(T, wm)) / (2 * h)
        a = (host_cost(shim, head, tail, ref, np.concatenate([x[:N], wp.reshape(-1)]), prm)[3][0] -
             host_cost(shim, head, tail, ref, np.concatenate([x[:N], wm.reshape(-1)]), prm)[3][0]) / (2 * h)
        bound = w * h * h * np.linalg.norm(a) ** 3 + gamma * 2.0 ** -53 * abs(c) / h
        print(f"waypoint axis {k}: fd {fd:.9g}, gradP {g[N + k]:.9g}, |diff| {abs(fd - g[N + k]):.3e}, bound {bound:.3e}")
        assert abs(fd - g[N + k]) <= bound


@pytest.fixture(scope="module")
def ref_fits(ref_side):
    """The reference's own lbfgs_optimize on (reference MINCO + numpy penalty), once per case."""
    out = {}
    for N in (3, 8, 40):
        head, tail, ref, T0 = mc.fit_problem(N)
        x0 = np.concatenate([mc.backward_T(T0), ref.reshape(-1)])
        fun = lambda xv: mc.ref_cost(ref_side, head, tail, ref, xv)[:2]
        out[N] = ref_side.ref_lbfgs_optimize(fun, x0, mem_size=mc.PRM["mem_size"], g_epsilon=mc.PRM["g_epsilon"], past=mc.PRM["past"],
                                             delta=mc.PRM["rel_cost_tol"], max_iterations=100000)
    return out


@pytest.mark.parametrize("N", [3, 8, 40])
def test_fit_matches_the_reference_lbfgs(shim, ref_fits, capfd, N):
    """3.  lbfgs_host.hpp is pinned iterate for iterate, minco_host.hpp equals minco.hpp to rounding only, and a stop test on a
    1e-6 relative decrease amplifies that.  Measured here (host form against the reference's run, these inputs): N = 3 cost 2.8e-16 /
    waypoints 4.4e-15 m / durations 1.6e-15 s (25 iterations); N = 8 cost 1.3e-7 / 9.2e-4 m / 2.5e-4 s (374 iterations); N = 40 cost
    2.9e-5 / 1.1e-2 m / 2.4e-3 s (4590 iterations).  FIT_BOUNDS allows 10 x that."""
    head, tail, ref, T0 = mc.fit_problem(N)
    xr, fr, sr, er = ref_fits[N]
    capfd.readouterr()
    x, r = host_fit(shim, head, tail, ref, T0)
    # the condition on the inputs: the reference ends with status >= 0, and well inside 5 000 iterations (counted by the host
    # form, whose driver walks the reference's iterates)
    assert sr >= 0 and r["status"] >= 0 and r["iterations"] < 5000, (sr, r)
    dc = abs(r["f"] - fr) / abs(fr); dw = np.abs(x[N:] - xr[N:]).max(); dT = np.abs(mc.forward_T(x[:N]) - mc.forward_T(xr[:N])).max()
    print(f"N={N}: reference f {fr:.12g} status {sr} ({er} evaluations); host {r}; cost rel {dc:.3e}, waypoints {dw:.3e} m, durations {dT:.3e} s")
    bc, bw, bT = FIT_BOUNDS[N]
    assert dc <= bc and dw <= bw and dT <= bT
    # the recorded run the GPU test compares against is this run
    gold = np.load(GOLDEN)
    assert int(gold[f"status_{N}"]) == sr
    assert abs(float(gold[f"f_{N}"]) - fr) <= bc * abs(fr) and np.abs(gold[f"x_{N}"][N:] - xr[N:]).max() <= bw


def test_sanitizer_program(tmp_path):
    """4.  The host cost and a short fit at N = 2, 5, 40 as a stand-alone program under AddressSanitizer and UBSan."""
    exe = str(tmp_path / "midend_sanitize")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
                           "-I", CSRC, os.path.join(ROOT, "tests", "native", "midend_sanitize_main.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert r.stdout.count(" ok: ") == 3, r.stdout


def test_yaml_and_defaults(pkg, product_lib, tmp_path):
    """isdf_midend_params_default / isdf_load_yaml_midend: the values every shipped yaml agrees on; a file overrides them."""
    capi = pkg.capi
    p = capi.IsdfMidendParams()
    product_lib.isdf_midend_params_default(C.byref(p))
    cfg = capi.IsdfConfig(); product_lib.isdf_config_default(C.byref(cfg))
    assert (p.weight_pr, p.rho_mid_end, p.rel_cost_tol, p.mem_size, p.past, p.min_step, p.g_epsilon) == (1000.0, 200.0, 1e-6, 16, 10, 1e-32, 0.0)
    assert p.integral_intervs == cfg.integral_intervs
    y = tmp_path / "plan.yaml"
    y.write_text("weight_pr:   500.0   # comment\nrho_mid_end: 150\nrelCostTolMidEnd: 1.0e-5\nintegralIntervs: 32\nmem_size: 8\npast: 3\nmin_step: 1.0e-20\ng_epsilon: 1.0e-5\nrho: 7\n")
    q = capi.IsdfMidendParams()
    assert product_lib.isdf_load_yaml_midend(os.fsencode(str(y)), C.byref(q)) == 0
    assert (q.weight_pr, q.rho_mid_end, q.rel_cost_tol, q.integral_intervs, q.mem_size, q.past, q.min_step, q.g_epsilon) == (500.0, 150.0, 1e-5, 32, 8, 3, 1e-20, 1e-5)
    assert product_lib.isdf_load_yaml_midend(b"/nonexistent.yaml", C.byref(q)) == capi.ISDF_ERR_INVALID_ARG
