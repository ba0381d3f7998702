"""The mid end on the device (csrc/midend.hip: one launch per callback, one workgroup per trajectory) against the reference side of
tests/test_midend_host.py (the reference's own MINCO + the numpy penalty, tests/midend_common.py), against the host form, as a
batch, as a fit, and in front of the back end."""
import ctypes as C
import os

import numpy as np
import pytest

import midend_common as mc
from test_midend_host import FIT_BOUNDS, GOLDEN

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV_TOL = 1e-10          # the project's figure for the device MINCO against the host's
REF_FLOOR = 1e-11        # inputs are kept only where the reference side itself moves by at most a tenth of that under one-ulp input changes

# N -> what it exercises: 2 one inner junction, no PCR round, one constraint | 3 first real PCR round | 5 not a power of two |
# 64 / 65 wavefront boundary of the row mapping | 320 / 321 the SPLIT boundary | 400 CB_MAX_N
SHAPES = [2, 3, 5, 64, 65, 320, 321, 400]


def _engine(pkg, N, head, tail):
    """A ctx with nothing but isdf_set_trajectory: no grid, no shape, no points."""
    eng = pkg.Engine(pkg.synth.default_config(pkg.capi.V3_ESDF_TILE))
    eng.set_trajectory(N, head, tail, 0.0)
    return eng


def _close(a, b, tol, what):
    """relative to the array's largest entry: the measure DESIGN 6 states the device MINCO's 1e-10 in"""
    a = np.atleast_1d(np.asarray(a, dtype=np.float64)); b = np.atleast_1d(np.asarray(b, dtype=np.float64))
    sc = max(float(np.abs(b).max()), 1e-300)
    dev = float(np.abs(a - b).max()) / sc
    print(f"{what}: deviation {dev:.3e} of the largest entry (bound {tol:g})")
    assert dev <= tol, (what, dev)


@pytest.fixture(scope="module")
def ref_side(orc):
    if not os.path.exists(orc.REF_MINCO):
        pytest.skip("oracle/_ref/libref_minco.so not built")
    return orc


@pytest.fixture(scope="module")
def cases(pkg, ref_side):
    """Per shape: the problem (durations log-uniform in 0.05 .. 12 s; mc.posed_cost_problem: the first seed at which the reference
    side's own one-ulp sensitivity is within REF_FLOOR), the reference side's (cost, g, parts), once for all tests."""
    out = {}
    for N in SHAPES + [401]:
        seed, sens, (head, tail, ref, x) = mc.posed_cost_problem(ref_side, N, 300 + N, REF_FLOOR)
        print(f"N={N}: seed {seed}, reference side's one-ulp sensitivity {sens:.2e}")
        out[N] = (head, tail, ref, x) + mc.ref_cost(ref_side, head, tail, ref, x)[:3]
    return out


@pytest.mark.parametrize("N", SHAPES)
def test_device_cost_vs_reference_and_host(pkg, cases, N):
    """5 + 6.  Device form (mode 2) against the reference side and against the host form (mode 1), 1e-10."""
    head, tail, ref, x, c0, g0, parts0 = cases[N]
    eng = _engine(pkg, N, head, tail)
    eng.set_minco_mode(pkg.capi.MINCO_DEVICE)
    c, g, parts = eng.midend_cost(ref, x)
    assert eng.minco_path() == 1
    eng.set_minco_mode(pkg.capi.MINCO_HOST)
    ch, gh, partsh = eng.midend_cost(ref, x)
    assert eng.minco_path() == 0
    eng.close()
    for name, (cc, gg, pp) in (("reference", (c0, g0, parts0)), ("host form", (ch, gh, [partsh[k] for k in ("energy", "pose", "time")]))):
        _close(c, cc, DEV_TOL, f"N={N} cost vs {name}")
        _close(g[:N], gg[:N], DEV_TOL, f"N={N} g(tau) vs {name}")
        _close(g[N:], gg[N:], DEV_TOL, f"N={N} g(waypoints) vs {name}")
        _close([parts[k] for k in ("energy", "pose", "time")], pp, DEV_TOL, f"N={N} parts vs {name}")


def test_waypoint_on_its_sample(pkg, ref_side):
    """5.  d = 0: the reference point of one constraint is its sample position as the reference side computes it (the device
    reproduces it to rounding, so d is zero or a few ulp) - no NaN from d / |d|, and the reference's result."""
    N = 3
    head, tail, ref, x = mc.cost_problem(N, 91)
    T = mc.forward_T(x[:N])
    cm = ref_side.ref_minco(head, tail, x[N:].reshape(N - 1, 3).T, T)[0]
    pos = mc.sample_points(cm, T, N, mc.PRM["integral_intervs"])[0]
    ref = ref.copy(); ref[1] = pos[1]
    c0, g0, parts0 = mc.ref_cost(ref_side, head, tail, ref, x)[:3]
    eng = _engine(pkg, N, head, tail)
    eng.set_minco_mode(pkg.capi.MINCO_DEVICE)
    c, g, parts = eng.midend_cost(ref, x)
    eng.close()
    assert np.isfinite(c) and np.isfinite(g).all()
    _close(c, c0, DEV_TOL, "d=0 cost"); _close(g[:N], g0[:N], DEV_TOL, "d=0 g(tau)"); _close(g[N:], g0[N:], DEV_TOL, "d=0 g(waypoints)")


def test_beyond_cb_max_n_runs_the_host_form(pkg, cases):
    """5.  N = 401: the host form runs whatever the mode, and isdf_minco_path says so."""
    N = 401
    head, tail, ref, x, c0, g0, _ = cases[N]
    eng = _engine(pkg, N, head, tail)
    eng.set_minco_mode(pkg.capi.MINCO_DEVICE)
    c, g, _ = eng.midend_cost(ref, x)
    assert eng.minco_path() == 0
    eng.close()
    _close(c, c0, DEV_TOL, "N=401 cost"); _close(g, g0, DEV_TOL, "N=401 g")


@pytest.mark.parametrize("nb", [1, 3, 130])
def test_cost_batch_rows_are_the_single_call(pkg, nb):
    """6.  isdf_midend_cost_batch: every row bitwise the single call in device mode (N = 5; 130 only crosses 128)."""
    N = 5
    probs = [mc.cost_problem(N, 500 + b, mix=(b % 7 == 3)) for b in range(nb)]
    heads = np.array([p[0] for p in probs]); tails = np.array([p[1] for p in probs])
    refs = np.array([p[2] for p in probs]); xs = np.array([p[3] for p in probs])
    eng = _engine(pkg, N, probs[0][0], probs[0][1])
    eng.set_minco_mode(pkg.capi.MINCO_DEVICE)
    costs, gs = eng.midend_cost_batch(heads, tails, refs, xs)
    assert eng.minco_path() == 1
    for b in sorted({0, nb // 2, nb - 1}):
        eng.set_trajectory(N, probs[b][0], probs[b][1], 0.0)
        c, g, _ = eng.midend_cost(probs[b][2], probs[b][3])
        assert c == costs[b] and np.array_equal(g, gs[b]), b
    eng.close()


def test_argument_checks(pkg):
    capi = pkg.capi
    head, tail, ref, x = mc.cost_problem(2, 1)
    eng = pkg.Engine(pkg.synth.default_config(capi.V3_ESDF_TILE))
    eng.set_trajectory(1, head, tail, 0.0)
    with pytest.raises(pkg.IsdfError) as e:
        eng.midend_cost(np.zeros((1, 3)), np.zeros(1))
    assert e.value.code == capi.ISDF_ERR_INVALID_ARG
    eng.close()


@pytest.mark.parametrize("N", [3, 8, 40])
def test_device_fit_vs_reference_run(pkg, N):
    """7.  isdf_midend_fit in device mode on test 3's cases against the reference's recorded run (tests/golden/ref_midend_fit.npz,
    which tests/test_midend_host.py holds to a live run), within test 3's bounds; status >= 0."""
    head, tail, ref, T0 = mc.fit_problem(N)
    gold = np.load(GOLDEN)
    xr, fr = gold[f"x_{N}"], float(gold[f"f_{N}"])
    eng = _engine(pkg, N, head, tail)
    eng.set_minco_mode(pkg.capi.MINCO_DEVICE)
    x, T, cm, r = eng.midend_fit(ref, T0)
    assert eng.minco_path() == 1
    eng.close()
    dc = abs(r["f"] - fr) / abs(fr); dw = np.abs(x[N:] - xr[N:]).max(); dT = np.abs(T - mc.forward_T(xr[:N])).max()
    print(f"N={N}: device fit {r}; against the reference's run: cost rel {dc:.3e}, waypoints {dw:.3e} m, durations {dT:.3e} s (bounds {FIT_BOUNDS[N]})")
    assert r["status"] >= 0
    bc, bw, bT = FIT_BOUNDS[N]
    assert dc <= bc and dw <= bw and dT <= bT


def test_fit_batch_bitwise_and_cancel(pkg):
    """8.  Six trajectories of N = 8 with different ends: bitwise six single device-mode fits; then one of them cancelled through
    isdf_set_progress ends with status 2 while the others finish as before."""
    N, nb = 8, 6
    heads, tails, refs, T0s = [], [], [], []
    for b in range(nb):
        head, tail, ref, T0 = mc.fit_problem(N)
        head[:, 0] += [0.0, 0.2 * b, 0.0]; tail[:, 0] += [0.3 * b, 0.0, 0.1 * b]; head[0, 1] = 0.1 * b
        heads.append(head); tails.append(tail); refs.append(ref + 0.05 * b); T0s.append(T0 + 0.1 * b)
    eng = _engine(pkg, N, heads[0], tails[0])
    eng.set_minco_mode(pkg.capi.MINCO_DEVICE)
    xs, res, wall = eng.midend_fit_batch(np.array(heads), np.array(tails), np.array(refs), np.array(T0s))
    singles = []
    for b in range(nb):
        eng.set_trajectory(N, heads[b], tails[b], 0.0)
        x, _, _, r = eng.midend_fit(refs[b], T0s[b])
        singles.append((x, r))
        assert res[b]["status"] == r["status"] >= 0 and res[b]["iterations"] == r["iterations"] and res[b]["evaluations"] == r["evaluations"]
        assert res[b]["f"] == r["f"] and np.array_equal(xs[b], x), b
    print(f"batch of {nb}: {wall:.1f} ms, {res[0]['rounds']} rounds; iterations {[r['iterations'] for r in res]}")
    victim = 2
    eng.set_progress(lambda t, x, g, fx, step, k, ls: t == victim and k >= 5, n_traj=nb)
    xs2, res2, _ = eng.midend_fit_batch(np.array(heads), np.array(tails), np.array(refs), np.array(T0s))
    eng.set_progress(None)
    eng.close()
    assert res2[victim]["status"] == 2 and res2[victim]["iterations"] == 5
    for b in range(nb):
        if b != victim:
            assert res2[b]["status"] == res[b]["status"] and np.array_equal(xs2[b], xs[b]), b


def test_pipeline_front_end_mid_end_back_end(pkg):
    """9.  build_plan of tests/demo_headless.py on the committed demo1 inputs, the mid end on its waypoints, its x into
    isdf_optimize_lbfgs on the V1 ctx.  Reported, not asserted: the back end's final cost from the mid end's start against the
    raw-waypoint start."""
    from test_gpu_demo import _demo
    g, plan, cfg, shape, eng, P = _demo(pkg, "CappedCone")
    N = P["N"]
    prm = eng.midend_params(integral_intervs=int(plan.sweep.integral_intervs))
    x_mid, T, cm, r = eng.midend_fit(P["Q"], np.full(N, plan.inittime), prm)
    assert r["status"] >= 0, r
    assert x_mid.size == eng.num_variables()
    assert (T > 0).all() and np.isfinite(cm).all()
    iters = 10
    x1, r1 = eng.optimize_lbfgs(x_mid, max_iterations=iters)
    assert np.isfinite(r1["f"])
    x2, r2 = eng.optimize_lbfgs(P["x0"], max_iterations=iters)
    eng.close()
    print(f"demo1, N={N}: mid end {r}; back end ({iters} iterations) from the mid end's x: f = {r1['f']:.9g} (status {r1['status']}); "
          f"from the raw waypoints: f = {r2['f']:.9g} (status {r2['status']})")


def test_lifetime(pkg, product_lib):
    """10.  create / use / destroy: every device and pinned byte the mid end took comes back (isdf_debug_live_bytes)."""
    import gc

    def live():
        out = (C.c_longlong * 2)()
        product_lib.isdf_debug_live_bytes(out)
        return [int(out[0]), int(out[1])]
    gc.collect()                    # (engines other tests dropped go now, not in the middle of the count)
    before = live()
    N = 8
    head, tail, ref, T0 = mc.fit_problem(N)
    eng = _engine(pkg, N, head, tail)
    eng.set_minco_mode(pkg.capi.MINCO_DEVICE)
    x = np.concatenate([mc.backward_T(T0), ref.reshape(-1)])
    eng.midend_cost(ref, x)
    eng.midend_cost_batch(np.array([head] * 3), np.array([tail] * 3), np.array([ref] * 3), np.array([x] * 3))
    eng.midend_fit_batch(np.array([head] * 2), np.array([tail] * 2), np.array([ref] * 2), np.array([T0] * 2), eng.midend_params(rel_cost_tol=1e-2))
    during = live()
    assert during[0] > before[0] and during[1] > before[1]
    eng.close()
    assert live() == before
    if before == [0, 0]:
        assert live() == [0, 0]
