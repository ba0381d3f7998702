"""Inputs of the retiming tests (isdf_traj_retime*), shared by the host and the device test files: trajectories of the limits golden
(tests/limits_reference.py) under limits chosen so that a known channel binds, and helpers that hold a result to the rules of
include/isdf_accel.h through INDEPENDENT calls of the limits report and the scaling."""
import math

import numpy as np

import limits_reference as lr

GOLD = {c["name"]: c for c in lr.load_golden()}
FAR = 1000.0            # a limit out of reach
HOVER = 0.61 * 9.8      # m g of the golden's configuration: the thrust every channel tends to as s grows


def _n5():
    c = GOLD["n130"]
    return dict(name="n5", T=c["T"][:5].copy(), C=c["C"][:5], coeffs=lr.pack(c["C"][:5]), cfg=c["cfg"], samples_param=5)


def case(name):
    """dict(T, coeffs, gold (the golden case or None), cfg overrides `over`, params of the retiming `kw`)."""
    g = GOLD
    if name == "speed_n1":          # only the speed is judged to bind: s* = v_peak / vmax = 2.37
        c = g["n1_mid"]
        return dict(src=c, over=dict(vmax=float(c["value"][0]) / 2.37, omgmax=FAR, thetamax=FAR), kw={})
    if name == "acc_n3":            # only the acceleration: s* = sqrt(a_peak / max_acc) = 1.9
        c = g["n3_durations"]
        return dict(src=c, over=dict(vmax=FAR, omgmax=FAR, thetamax=FAR), kw=dict(max_acc=float(c["value"][1]) / 1.9 ** 2))
    if name == "all_n2":            # every channel judged, several over their limit at s = 1
        return dict(src=g["n2_junction"], over=dict(vmax=1.0, omgmax=1.0, thetamax=0.4), kw=dict(max_acc=3.0, max_thrust=7.5, min_thrust=5.5))
    if name == "all_n1":
        return dict(src=g["n1_tilted"], over=dict(vmax=2.0, omgmax=3.0, thetamax=0.6), kw=dict(max_acc=6.0, max_thrust=8.0, min_thrust=4.5))
    if name == "all_n5":
        return dict(src=_n5(), over=dict(vmax=1.5, omgmax=2.0, thetamax=0.5), kw=dict(max_acc=4.0, max_thrust=8.0, min_thrust=4.5, samples=5))
    if name == "at_lower":          # status 1: nothing binds at s_lo
        return dict(src=g["n1_omg"], over=dict(vmax=FAR, omgmax=FAR, thetamax=FAR), kw={})
    if name == "not_reachable":     # status 2: a smallest thrust above m g is never reached
        return dict(src=g["n1_tilted"], over=dict(vmax=FAR, omgmax=FAR, thetamax=FAR), kw=dict(min_thrust=6.5))
    raise KeyError(name)


BY_N = {1: "all_n1", 2: "all_n2", 5: "all_n5"}
# three two-piece trajectories under ONE set of limits that end in status 0, 1 and 2: speeds 3.12, 2.28 and 3.75 against vmax 2.4 on [1, 1.5]
BATCH = dict(names=["batch_2", "batch_0", "batch_1"], status=[0, 1, 2], over=dict(vmax=2.4, omgmax=FAR, thetamax=FAR), kw=dict(s_lo=1.0, s_hi=1.5))


def config(pkg, cs):
    return lr.make_config(pkg, cs["src"], **cs["over"])


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


def feasible(rep):
    return rep["feasible"] == rep["judged"]


def hold_result(pkg, cs, res, report, L, R, s_lo=1.0, s_hi=8.0):
    """The rules a result obeys, through independent calls: report(T, coeffs) -> a limits dict (host or device form)."""
    src = cs["src"]
    To, Co = pkg.traj_scale_host(src["T"], src["coeffs"], res["scale"])
    assert To.tobytes() == res["T"].tobytes() and Co.tobytes() == res["coeffs"].tobytes(), "the arrays are not the input scaled by `scale`"
    at = report(res["T"], res["coeffs"])
    assert same_limits(res["limits"], at) is None, same_limits(res["limits"], at)
    assert res["duration_in"] == float(np.add.accumulate(src["T"])[-1]) and res["duration_out"] == float(np.add.accumulate(res["T"])[-1])
    if res["status"] == 0:
        assert feasible(at) and res["rounds"] == R and res["candidates"] == L * R
        assert s_lo <= res["scale_below"] < res["scale"] <= s_hi
        below = report(*pkg.traj_scale_host(src["T"], src["coeffs"], res["scale_below"]))
        assert not feasible(below)
        assert res["binding"] == below["judged"] & ~below["feasible"] and res["binding"] != 0
        # (s_hi - s_lo) / (L - 1)^R: a round's step is one rounded quotient and one rounded sum, a few ulp of s_hi in all
        width = (s_hi - s_lo) / (L - 1) ** R
        assert res["scale"] - res["scale_below"] <= width + 8 * R * np.spacing(s_hi), (res["scale"], res["scale_below"], width)
    elif res["status"] == 1:
        assert feasible(at) and res["scale"] == s_lo and math.isnan(res["scale_below"]) and res["binding"] == 0
        assert res["rounds"] == 1 and res["candidates"] == L
    else:
        assert res["status"] == 2 and not feasible(at) and res["scale"] == s_hi and res["rounds"] == 1 and res["candidates"] == L


def ladder_is_monotone(pkg, cs, res, L, R, cfg, s_lo=1.0, s_hi=8.0):
    """Whether the host form's verdicts are a clean step (False ... False True ... True) on the ladder of EVERY round, the rounds walked
    here with independent host calls and candidates restated in Python, and end at the result.  A rounding-level flip of one verdict in
    another form then moves its pick by one candidate of the last ladder and no further."""
    src = cs["src"]
    a, b = s_lo, s_hi
    for r in range(R):
        cand = [a if i == 0 else (b if i == L - 1 else a + (b - a) * i / (L - 1)) for i in range(L)]
        v = [feasible(pkg.traj_limits_host(cfg, *pkg.traj_scale_host(src["T"], src["coeffs"], s), **limits_kw(cs["kw"]))) for s in cand]
        if v != sorted(v) or v[0] or not v[-1]:
            return False
        k = v.index(True)
        a, b = cand[k - 1], cand[k]
    return res["nonmonotone"] == 0 and (a, b) == (res["scale_below"], res["scale"])
