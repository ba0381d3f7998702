"""Retiming a trajectory to its dynamic limits on the device (isdf_traj_retime, _device, _batch): the result held to the rules of
include/isdf_accel.h through independent calls of the device's own limits report and the host scaling, at N = 1, 2, 5, ladders 2, 5,
33, 64 and 1 and 3 rounds; a batch whose three trajectories end in status 0, 1 and 2; host form against device form where the host
ladder is monotone; determinism, lifetime, the clearance check of the result, and the error paths on a ctx."""
import ctypes as C
import math

import numpy as np
import pytest

import limits_reference as lr
import retime_cases as rc
from common import small_world

pytestmark = pytest.mark.gpu


def _engine(pkg, cs):
    return pkg.Engine(rc.config(pkg, cs))


def _same_result(a, b):
    """None, or the first field in which two results differ (bytes; device_ms aside)."""
    for k in a:
        if k in ("device_ms", "limits", "check"):
            continue
        if np.asarray(a[k]).tobytes() != np.asarray(b[k]).tobytes():
            return k
    return rc.same_limits(a["limits"], b["limits"])


@pytest.fixture(scope="module")
def engines(pkg, product_lib):
    es = {N: _engine(pkg, rc.case(name)) for N, name in rc.BY_N.items()}
    yield es
    for e in es.values():
        e.close()


@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("L", [2, 5, 33, 64])
@pytest.mark.parametrize("N", [1, 2, 5])
def test_composition_and_minimality_on_the_device(pkg, engines, N, L, R):
    """The arrays are traj_scale_host(input, scale) and info.limits is isdf_traj_limits_batch on them, byte for byte; F(scale) holds and
    F(scale_below) fails by independent isdf_traj_limits calls; the _device form, the batch form with B = 1 and a second call give the
    same bytes."""
    import torch
    cs = rc.case(rc.BY_N[N])
    e = engines[N]
    T, Cc = cs["src"]["T"], cs["src"]["coeffs"]
    assert len(T) == N
    res = e.traj_retime(T, Cc, ladder=L, rounds=R, **cs["kw"])
    print(f"\nN {N} L {L} R {R}: scale {res['scale']:.17g} below {res['scale_below']:.17g} status {res['status']} binding {res['binding']:06b} "
          f"device {res['device_ms']:.3f} ms")
    assert res["status"] == 0 and res["checked"] == 0
    lk = rc.limits_kw(cs["kw"])
    rc.hold_result(pkg, cs, res, lambda t, c: e.traj_limits_batch(t[None, :], c[None, :], **lk)[0], L, R)
    rc.hold_result(pkg, cs, res, lambda t, c: e.traj_limits(t, c, **lk), L, R)
    again = e.traj_retime(T, Cc, ladder=L, rounds=R, **cs["kw"])
    assert _same_result(res, again) is None, _same_result(res, again)
    bat = e.traj_retime_batch(T[None, :], Cc[None, :], ladder=L, rounds=R, **cs["kw"])
    assert len(bat) == 1 and _same_result(res, bat[0]) is None, _same_result(res, bat[0])
    dT = torch.tensor(T, dtype=torch.float64, device="cuda"); dC = torch.tensor(Cc, dtype=torch.float64, device="cuda")
    oT = torch.zeros(N, dtype=torch.float64, device="cuda"); oC = torch.zeros(18 * N, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    dev = e.traj_retime_device(N, dT.data_ptr(), dC.data_ptr(), oT.data_ptr(), oC.data_ptr(), ladder=L, rounds=R, **cs["kw"])
    dev["T"], dev["coeffs"] = oT.cpu().numpy(), oC.cpu().numpy()
    assert _same_result(res, dev) is None, _same_result(res, dev)


@pytest.mark.parametrize("N,L", [(1, 5), (1, 33), (1, 64), (2, 5), (2, 33), (5, 5), (5, 33)])
def test_host_form_against_device_form(pkg, engines, N, L):
    """On cases whose every host round is a clean step (verified here, and without a GPU in test_traj_retime_host.py) a rounding-level
    difference of the reports can flip one verdict next to the step: the same scale, or one step of the last ladder apart."""
    R = 3
    cs = rc.case(rc.BY_N[N])
    cfg = rc.config(pkg, cs)
    T, Cc = cs["src"]["T"], cs["src"]["coeffs"]
    host = pkg.traj_retime_host(cfg, T, Cc, ladder=L, rounds=R, **cs["kw"])
    assert rc.ladder_is_monotone(pkg, cs, host, L, R, cfg)
    dev = engines[N].traj_retime(T, Cc, ladder=L, rounds=R, **cs["kw"])
    step = 7.0 / (L - 1) ** R
    print(f"\nN {N} L {L}: host {host['scale']:.17g} device {dev['scale']:.17g} difference {abs(host['scale'] - dev['scale']):.3e} last step {step:.3e}")
    assert dev["status"] == host["status"] == 0 and dev["nonmonotone"] == 0
    assert host["scale"] == dev["scale"] or abs(host["scale"] - dev["scale"]) <= step + 8 * R * np.spacing(8.0)


@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("L", [2, 5, 33, 64])
def test_batch_of_three_statuses(pkg, product_lib, L, R):
    """Status 0, 1 and 2 in one launch: the brackets diverge, and row b equals the single call byte for byte wherever it stands."""
    cases = [rc.GOLD[n] for n in rc.BATCH["names"]]
    e = pkg.Engine(lr.make_config(pkg, cases[0], **rc.BATCH["over"]))
    T = np.stack([c["T"] for c in cases]); Cc = np.stack([c["coeffs"] for c in cases])
    kw = dict(ladder=L, rounds=R, **rc.BATCH["kw"])
    alone = [e.traj_retime(c["T"], c["coeffs"], **kw) for c in cases]
    fwd = e.traj_retime_batch(T, Cc, **kw)
    rev = e.traj_retime_batch(T[::-1], Cc[::-1], **kw)
    live = []
    for _ in range(2):
        again = e.traj_retime_batch(T, Cc, **kw)
        b = (C.c_longlong * 2)()
        e.lib.isdf_debug_live_bytes(b)
        live.append(tuple(b))
    assert live[0] == live[1], live                  # no allocation from the second call on
    if L > 2:
        assert [r["status"] for r in fwd] == rc.BATCH["status"]
    else:
        assert [r["status"] for r in fwd] == [0, 1, 2]
    for b in range(3):
        for other, what in ((fwd[b], "batch"), (rev[2 - b], "reversed"), (again[b], "again")):
            assert _same_result(alone[b], other) is None, (b, what, _same_result(alone[b], other))
        cs = dict(src=cases[b], over=rc.BATCH["over"], kw={})
        rc.hold_result(pkg, cs, fwd[b], lambda t, c: e.traj_limits(t, c), L, R, s_lo=1.0, s_hi=1.5)
    e.close()


def test_status_one_and_two_single(pkg, product_lib):
    for name, want, L in (("at_lower", 1, 5), ("not_reachable", 2, 9)):
        cs = rc.case(name)
        e = _engine(pkg, cs)
        res = e.traj_retime(cs["src"]["T"], cs["src"]["coeffs"], ladder=L, **cs["kw"])
        host = pkg.traj_retime_host(rc.config(pkg, cs), cs["src"]["T"], cs["src"]["coeffs"], ladder=L, **cs["kw"])
        assert res["status"] == want == host["status"] and res["scale"] == host["scale"]
        assert res["T"].tobytes() == host["T"].tobytes() and res["coeffs"].tobytes() == host["coeffs"].tobytes()
        if want == 2:
            assert res["scale_below"] == host["scale_below"] == 1.0 + 7.0 * 7 / 8 and res["binding"] == 1 << 5
        rc.hold_result(pkg, cs, res, lambda t, c: e.traj_limits(t, c, **rc.limits_kw(cs["kw"])), L, 3)
        e.close()


def test_check_of_the_result_and_state_isolation(pkg, product_lib):
    """check = 1 on a 16^3 occupancy grid with a box robot: info.check is an independent isdf_traj_check of the returned arrays (its
    three timings aside), the kept rows are that check's; a V1 ctx's points and lastTstar are what they were."""
    capi, synth = pkg.capi, pkg.synth
    res_m = 0.5
    occ = np.zeros((16, 16, 16), dtype=np.uint8)
    occ[6:10, 6:10, 0:9] = 1
    ext = np.array(occ.shape) * res_m
    N = 2
    T, Cf = synth.random_trajectory(ext, N, seed=5, piece_T=0.9, margin=1.5)
    cm = synth.colmajor(Cf)
    shape = synth.make_shape("Box", params=(0.5, 0.3, 0.15), bound_radius=0.7)
    way = np.asarray(cm).reshape(3, N, 6)[:, 1:, 0].T
    pts = synth.constraint_points(occ, (0, 0, 0), res_m, way, half=3.0)
    assert pts.shape[0] > 0
    e = pkg.Engine(synth.default_config(capi.V1_SWEPT, safety_hor=0.5, vmax=1.0, omgmax=1.0, thetamax=0.5, integral_intervs=4))
    # what the check needs is missing: said before anything is computed
    with pytest.raises(pkg.IsdfError) as ei:
        e.traj_retime(T, cm, check=True)
    assert ei.value.code != 0
    e.set_shape(shape)
    with pytest.raises(pkg.IsdfError) as ei:
        e.traj_retime(T, cm, check=True)
    assert ei.value.code == capi.ISDF_ERR_INVALID_ARG
    e.set_grid(occ, (0, 0, 0), res_m, capi.GRID_OCCUPANCY)
    e.set_points(pts)
    ts = np.zeros(pts.shape[0])
    r1 = e.eval_single(T, cm, tstar=ts)
    ts1 = ts.copy()
    res = e.traj_retime(T, cm, check=True, ladder=5, rounds=3)
    rows = e.traj_check_points()
    assert res["checked"] == 1 and res["status"] == 0 and res["scale"] > 1.0
    ind = e.traj_check(res["T"], res["coeffs"])
    for k, v in res["check"].items():
        if k.endswith("_ms"):
            continue
        assert np.asarray(v).tobytes() == np.asarray(ind[k]).tobytes(), k
    assert rows.shape[0] == res["check"]["n_below_margin"] and e.traj_check_points().tobytes() == rows.tobytes()
    plain = e.traj_retime(T, cm, ladder=5, rounds=3)
    assert plain["checked"] == 0 and plain["check"] is None and _same_result(res, plain) in (None, "checked")
    assert e.traj_check_points().tobytes() == rows.tobytes()        # without check the kept rows stay
    ts2 = ts1.copy()
    r2 = e.eval_single(T, cm, tstar=ts2)
    e.close()
    # the same two steps on a ctx that never retimed
    f = pkg.Engine(synth.default_config(capi.V1_SWEPT, safety_hor=0.5, vmax=1.0, omgmax=1.0, thetamax=0.5, integral_intervs=4))
    f.set_shape(shape); f.set_grid(occ, (0, 0, 0), res_m, capi.GRID_OCCUPANCY); f.set_points(pts)
    us = np.zeros(pts.shape[0])
    q1 = f.eval_single(T, cm, tstar=us)
    us1 = us.copy()
    q2 = f.eval_single(T, cm, tstar=us)
    f.close()
    assert np.array_equal(ts1, us1) and np.array_equal(ts2, us)
    for a, b in ((r1, q1), (r2, q2)):
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_argument_errors_on_a_ctx(pkg, engines):
    capi = pkg.capi
    e = engines[1]
    cs = rc.case(rc.BY_N[1])
    T, Cc = cs["src"]["T"], cs["src"]["coeffs"]
    for bad in (dict(s_lo=0.0), dict(s_lo=math.inf), dict(s_lo=math.nan), dict(s_hi=1.0), dict(s_hi=0.25), dict(ladder=1), dict(ladder=65),
                dict(rounds=0), dict(rounds=5)):
        for call in (lambda: e.traj_retime(T, Cc, **bad), lambda: e.traj_retime_batch(T[None, :], Cc[None, :], **bad)):
            with pytest.raises(pkg.IsdfError) as ei:
                call()
            assert ei.value.code == capi.ISDF_ERR_INVALID_ARG, bad
    with pytest.raises(pkg.IsdfError) as ei:
        e.traj_retime_batch(T[None, :], Cc[None, :], check=True)
    assert ei.value.code == capi.ISDF_ERR_INVALID_ARG
    for Tb in (0.0, -1.0, math.inf, math.nan):
        with pytest.raises(pkg.IsdfError) as ei:
            e.traj_retime([Tb], Cc)
        assert ei.value.code == capi.ISDF_ERR_INVALID_ARG
    many = capi.TRAJ_RETIME_MAX_PIECES // 64 + 1
    with pytest.raises(pkg.IsdfError) as ei:
        e.traj_retime_batch(np.ones((many, 1)), np.zeros((many, 18)), ladder=64)
    assert ei.value.code == capi.ISDF_ERR_INVALID_ARG
    e.traj_retime(T, Cc, **cs["kw"])                 # the ctx still works
    # one ctx over several devices: not supported (two shards on device 0 make such a ctx on any machine)
    multi = pkg.Engine(rc.config(pkg, cs), devices=[0, 0])
    for call in (lambda: multi.traj_retime(T, Cc), lambda: multi.traj_retime_batch(T[None, :], Cc[None, :])):
        with pytest.raises(pkg.IsdfError) as ei:
            call()
        assert ei.value.code == capi.ISDF_ERR_UNSUPPORTED
    multi.close()
