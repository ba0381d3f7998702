"""The dynamic-limits report and the state sampler on the device (isdf_traj_limits*, isdf_traj_sample*): the golden cases of
tests/limits_reference.py through the host-pointer, device-pointer and batch entry points with the host form's bounds, bitwise
batch independence and repeatability, state isolation on a V1 ctx, device against host form, and the report on an optimised
40-piece trajectory against the penalty's own K + 1 samples."""
import ctypes as C

import numpy as np
import pytest

import limits_reference as lr
from common import small_world

pytestmark = pytest.mark.gpu

GOLD = lr.load_golden()
NAMES = [c["name"] for c in GOLD]
BY_NAME = {c["name"]: c for c in GOLD}


@pytest.fixture(scope="module")
def eng(pkg, product_lib):
    """One ctx for every golden case (they share one configuration)."""
    cfgs = {tuple(sorted(c["cfg"].items())) for c in GOLD}
    assert len(cfgs) == 1
    e = pkg.Engine(lr.make_config(pkg, GOLD[0]))
    yield e
    e.close()


def _same(a, b, skip=("device_ms",)):
    for k in a:
        if k in skip:
            continue
        x, y = a[k], b[k]
        if isinstance(x, np.ndarray):
            if x.tobytes() != np.asarray(y).tobytes():
                return k
        elif x != y and not (x is None and y is None):
            return k
    return None


@pytest.mark.parametrize("name", NAMES)
def test_device_report_within_bounds(pkg, eng, name):
    """host-pointer, device-pointer and batch entry points: the same bytes, held to the golden per channel."""
    import torch
    case = BY_NAME[name]
    N = len(case["T"])
    rep = eng.traj_limits(case["T"], case["coeffs"], samples=case["samples_param"])
    lines, bad = lr.check_report(case, rep, "device")
    print("\n" + "\n".join(lines))
    assert not bad, "\n".join(bad)
    assert rep["samples"] == case["samples"] and rep["tol_t"] == lr.TOL_T
    dT = torch.tensor(case["T"], dtype=torch.float64, device="cuda")
    dC = torch.tensor(case["coeffs"], dtype=torch.float64, device="cuda")
    dP = torch.zeros(N * 12, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    dev = eng.traj_limits_device(N, dT.data_ptr(), dC.data_ptr(), d_piece_out=dP.data_ptr(), samples=case["samples_param"])
    dev["piece_out"] = dP.cpu().numpy().reshape(N, 12)
    assert _same(rep, dev) is None, _same(rep, dev)
    bat = eng.traj_limits_batch(case["T"][None, :], case["coeffs"][None, :], samples=case["samples_param"])
    assert len(bat) == 1 and _same(rep, bat[0]) is None, _same(rep, bat[0])
    # against the host form: within the sum of the two forms' bounds
    host = pkg.traj_limits_host(lr.make_config(pkg, case), case["T"], case["coeffs"], samples=case["samples_param"])
    for ch in range(lr.NCH):
        b = 2 * lr.bound(float(case["e_cond"][ch]), float(case["kappa"][ch]))
        assert lr.rel_err(float(rep["value"][ch]), float(host["value"][ch])) <= b, (name, ch, rep["value"][ch], host["value"][ch])
    if name == "n2_junction":
        po = rep["piece_out"]
        for ch in (0, 1):
            assert po[0, 2 * ch] == po[1, 2 * ch] == case["value"][ch] and po[0, 2 * ch + 1] == po[1, 2 * ch + 1] == 1.0
            assert rep["piece"][ch] == 0 and rep["time"][ch] == 1.0
    if name == "n2_hover":
        assert list(rep["time"]) == [0.0] * 6 and list(rep["piece"]) == [0] * 6 and rep["value"][2] == 0.0 and rep["value"][3] == 0.0
    if name == "n1_monotone":
        assert rep["time"][5] == 0.0 and rep["time"][0] == 1.5 and rep["time"][4] == 1.5


@pytest.mark.parametrize("name", NAMES)
def test_device_sampler(pkg, eng, name):
    import torch
    case = BY_NAME[name]
    rows = eng.traj_sample(case["T"], case["coeffs"], case["stamps"])
    worst = 0.0
    for k in range(len(case["stamps"])):
        for g, err in enumerate(lr.group_errors(rows[k], case["rows"][k])):
            b = lr.bound(float(case["rows_e_cond"][k][g]), 0.0)
            worst = max(worst, err / b)
            assert err <= b, (name, k, float(case["stamps"][k]), g, err, b)
    print(f"\n{name}: {len(case['stamps'])} stamps, worst error / bound {worst:.3f}")
    n = len(case["stamps"])
    dT = torch.tensor(case["T"], dtype=torch.float64, device="cuda")
    dC = torch.tensor(case["coeffs"], dtype=torch.float64, device="cuda")
    dt = torch.tensor(case["stamps"], dtype=torch.float64, device="cuda")
    dR = torch.zeros(n * 20, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    eng.traj_sample_device(len(case["T"]), dT.data_ptr(), dC.data_ptr(), n, dt.data_ptr(), dR.data_ptr())
    assert dR.cpu().numpy().tobytes() == rows.tobytes()
    assert eng.traj_sample(case["T"], case["coeffs"], []).shape == (0, 20)


def test_batch_independence_and_repeatability(pkg, eng):
    cs = [BY_NAME[n] for n in lr.BATCH]
    T = np.stack([c["T"] for c in cs]); Cc = np.stack([c["coeffs"] for c in cs])
    alone = [eng.traj_limits(c["T"], c["coeffs"]) for c in cs]
    fwd = eng.traj_limits_batch(T, Cc)
    rev = eng.traj_limits_batch(T[::-1], Cc[::-1])
    again = eng.traj_limits_batch(T, Cc)
    for b in range(3):
        for other, what in ((fwd[b], "batch"), (rev[2 - b], "reversed"), (again[b], "second call")):
            assert _same(alone[b], other) is None, (b, what, _same(alone[b], other))
        lines, bad = lr.check_report(cs[b], fwd[b], "batch")
        assert not bad, "\n".join(bad)
    assert _same(alone[0], alone[1]) is not None            # three different trajectories


def test_limits_judged_on_the_device(pkg, product_lib):
    case = BY_NAME["n3_durations"]
    e = pkg.Engine(lr.make_config(pkg, case))
    v = e.traj_limits(case["T"], case["coeffs"])["value"]
    e.close()
    e = pkg.Engine(lr.make_config(pkg, case, vmax=v[0], omgmax=v[2], thetamax=v[3]))
    eq = e.traj_limits(case["T"], case["coeffs"], max_acc=v[1], max_thrust=v[4], min_thrust=v[5])
    e.close()
    assert eq["judged"] == 63 and eq["feasible"] == 63 and list(eq["n_pieces_over"]) == [0] * 6
    e = pkg.Engine(lr.make_config(pkg, case, vmax=np.nextafter(v[0], 0), omgmax=np.nextafter(v[2], 0), thetamax=np.nextafter(v[3], 0)))
    lt = e.traj_limits(case["T"], case["coeffs"], max_acc=np.nextafter(v[1], 0), max_thrust=np.nextafter(v[4], 0), min_thrust=np.nextafter(v[5], np.inf))
    nj = e.traj_limits(case["T"], case["coeffs"])
    e.close()
    assert lt["judged"] == 63 and lt["feasible"] == 0 and list(lt["n_pieces_over"]) == [1] * 6
    assert nj["judged"] == 0b001101 and list(nj["n_pieces_over"][[1, 4, 5]]) == [0, 0, 0]


def test_state_isolation_on_a_v1_ctx(pkg, product_lib):
    capi, synth = pkg.capi, pkg.synth
    occ, esdf, res = small_world(pkg, seed=3)
    ext = np.array(occ.shape) * res
    N = 6
    T, Cf = synth.random_trajectory(ext, N, seed=43, piece_T=1.5, margin=4.0, occ=occ, res=res)
    cm = synth.colmajor(Cf)
    way = np.asarray(cm).reshape(3, N, 6)[:, 1:, 0].T
    pts = synth.constraint_points(occ, (0, 0, 0), res, way, half=4 * res * 1.5)
    shape = synth.make_shape("RoundedCone", params=(0.8, 0.3, 1.6), bound_radius=1.9)
    case = BY_NAME["n3_durations"]
    out = {}
    for with_limits in (False, True):
        e = pkg.Engine(synth.default_config(capi.V1_SWEPT, safety_hor=0.5))
        e.set_shape(shape)
        e.set_grid(occ, (0, 0, 0), res, capi.GRID_OCCUPANCY)
        e.set_points(pts)
        ts = np.zeros(pts.shape[0])
        r1 = e.eval_single(T, cm, tstar=ts)
        ts1 = ts.copy()
        chk = e.traj_check(T * 0.8, cm)
        rows = e.traj_check_points()
        if with_limits:
            live = []
            for _ in range(3):
                e.traj_limits(case["T"], case["coeffs"])
                e.traj_sample(case["T"], case["coeffs"], case["stamps"])
                e.traj_limits_batch(np.stack([T, T * 1.1]), np.stack([cm, cm]))
                b = (C.c_longlong * 2)()
                e.lib.isdf_debug_live_bytes(b)
                live.append(tuple(b))
            assert live[1] == live[2], live          # no allocation in the steady state
            assert e.traj_check_points().tobytes() == rows.tobytes() and chk["n_below_margin"] == rows.shape[0]
        r2 = e.eval_single(T, cm, tstar=ts)
        out[with_limits] = (r1, r2, ts1, ts.copy())
        e.close()
    a, b = out[False], out[True]
    for k in range(2):
        assert a[k][0] == b[k][0] and np.array_equal(a[k][1], b[k][1]) and np.array_equal(a[k][2], b[k][2]), k
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])


def test_argument_errors_on_a_ctx(pkg, eng):
    capi = pkg.capi
    case = BY_NAME["n1_mid"]
    for bad in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(pkg.IsdfError) as ei:
            eng.traj_limits([bad], case["coeffs"])
        assert ei.value.code == capi.ISDF_ERR_INVALID_ARG
        with pytest.raises(pkg.IsdfError):
            eng.traj_sample([bad], case["coeffs"], [0.0])
    info = capi.IsdfTrajLimitsInfo()
    assert eng.lib.isdf_traj_limits(eng.h, 0, None, None, None, C.byref(info), None) == capi.ISDF_ERR_INVALID_ARG
    eng.traj_limits(case["T"], case["coeffs"])          # the ctx still works
    # one ctx over several devices: not supported
    multi = pkg.Engine(lr.make_config(pkg, case), devices=[0, 0])
    for call in (lambda: multi.traj_limits(case["T"], case["coeffs"]), lambda: multi.traj_limits_batch(case["T"][None, :], case["coeffs"][None, :]),
                 lambda: multi.traj_sample(case["T"], case["coeffs"], [0.0])):
        with pytest.raises(pkg.IsdfError) as ei:
            call()
        assert ei.value.code == capi.ISDF_ERR_UNSUPPORTED
    multi.close()


def test_report_against_the_penaltys_own_samples(pkg, product_lib):
    """A 40-piece trajectory after a few L-BFGS iterations under binding limits: per channel the report is no smaller than the
    largest of the penalty's K + 1 samples per piece (taken through traj_sample at j T_i / K)."""
    capi, synth = pkg.capi, pkg.synth
    occ, esdf, res = small_world(pkg, seed=3)
    ext = np.array(occ.shape) * res
    N, K = 40, 16
    T0, Cf = synth.random_trajectory(ext, N, seed=11, piece_T=0.35, margin=4.0, occ=occ, res=res)
    cfg = synth.default_config(capi.V3_ESDF_TILE, kernel_size=9, integral_intervs=K, safety_hor=0.5, vmax=1.5, omgmax=0.6, thetamax=0.25)
    e = pkg.Engine(cfg)
    e.set_grid(esdf, (0, 0, 0), res, capi.GRID_ESDF)
    e.set_shape(synth.make_shape("RoundedCone", params=(0.8, 0.3, 1.6), bound_radius=1.9))
    head = np.zeros((3, 3)); tail = np.zeros((3, 3))
    head[:, 0] = Cf[0]; tail[:, 0] = sum(Cf[6 * (N - 1) + p] * T0[-1] ** p for p in range(6))
    e.set_trajectory(N, head, tail, 2.5)
    x, r = e.optimize_lbfgs(e.pack_variables(T0, Cf[6::6]), max_iterations=5)
    T, cm = e.unpack_variables(x)
    rep = e.traj_limits(T, cm)
    # piece by piece with LOCAL stamps j T_i / K (a one-piece trajectory: the stamp is the local time, as the penalty forms it)
    rows = []
    for i in range(N):
        t = T[i] * np.arange(K + 1) / K
        t[K] = T[i]
        rows.append(e.traj_sample(T[i:i + 1], lr.pack(np.asarray(cm).reshape(3, N, 6)[:, i:i + 1, :].transpose(1, 0, 2)), t))
    rows = np.concatenate(rows)
    e.close()
    q = rows[:, 12:16]
    sampled = [np.linalg.norm(rows[:, 3:6], axis=1), np.linalg.norm(rows[:, 6:9], axis=1), np.linalg.norm(rows[:, 16:19], axis=1),
               np.arccos(1.0 - 2.0 * (q[:, 1] ** 2 + q[:, 2] ** 2)), rows[:, 19], rows[:, 19]]
    print(f"\nL-BFGS: {r}; limits vmax 1.5 omgmax 0.6 thetamax 0.25; feasible {rep['feasible']:06b} of judged {rep['judged']:06b}, pieces over {[int(n) for n in rep['n_pieces_over']]}")
    for ch in range(lr.NCH):
        s = sampled[ch].min() if ch == 5 else sampled[ch].max()
        v = rep["value"][ch]
        print(f"{lr.CH_NAMES[ch]:<10} report {v:.9g} at t {rep['time'][ch]:.6g} (piece {rep['piece'][ch]}); largest of the K + 1 samples {s:.9g}; beyond it by {abs(v - s):.3e}")
        # the K + 1 samples are among the report's own 4 K + 1 (4 j T / (4 K) = j T / K exactly).  The thrust is the sampler kernel's own
        # number - the same inline code as the report kernel's, 4 ulp for a contraction the compiler may place differently in the two
        # kernels.  The norms and the tilt are formed here by numpy from the rows: an ulp in the arccos argument is worth
        # 1 / (theta sin theta) <= 16 ulp of a tilt above 0.25 rad, a contracted sum of squares an ulp or two - 64 ulp.
        slack = (4 if ch >= 4 else 64) * np.spacing(abs(s)) + 1e-300
        assert (v <= s + slack) if ch == 5 else (v >= s - slack), (ch, v, s)
    # the limits bind: the penalty's own samples are over them (the optimiser traded them against clearance), so are the report and pieces
    for ch, lim in ((0, 1.5), (2, 0.6), (3, 0.25)):
        assert sampled[ch].max() > lim and rep["value"][ch] > lim and rep["n_pieces_over"][ch] > 0 and rep["limit"][ch] == lim, (ch, sampled[ch].max())
        assert not (rep["feasible"] >> ch) & 1
    assert rep["judged"] == 0b001101
    assert rep["samples"] == 4 * K
