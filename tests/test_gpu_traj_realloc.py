"""Re-allocating piece durations to the dynamic limits on the device (isdf_traj_realloc, _device, _batch): the result held to the rules
of include/isdf_accel.h through independent calls of the device's own limits report and of the host solve, at N = 1, 2, 3, 5, 33 (several
PCR rounds, no power of two) and 65 (pieces beyond one wavefront's lanes in the update kernel); a batch whose three trajectories end in
status 0, 1 and 2; host form against device form where every host round is a clean step; determinism, lifetime, the clearance check of
the result, and the error paths on a ctx."""
import ctypes as C
import math

import numpy as np
import pytest

import realloc_cases as ra

pytestmark = pytest.mark.gpu

CASES = [("aggressive", 1), ("aggressive", 2), ("aggressive", 3), ("aggressive", 5), ("aggressive", 33), ("short", 65), ("aggressive", 65)]
# device against host: every candidate, none dropped (their host margins are asserted in the test; 0 of 10 were not clean, the worst
# being aggressive N = 33 with 1.9e-5 against the 1e-6 that is asked)
CLEAN = [("aggressive", 1), ("aggressive", 2), ("aggressive", 3), ("aggressive", 5), ("aggressive", 33), ("short", 5), ("short", 9), ("short", 33),
         ("short", 65), ("aggressive", 65)]
DROPPED = 0


def _case(kind, N):
    return ra.short_piece_case(N) if kind == "short" else ra.aggressive_case(N)


@pytest.fixture(scope="module")
def engine(pkg, product_lib):
    e = pkg.Engine(ra.config(pkg))
    yield e
    e.close()


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return ra.build_shim(tmp_path_factory.mktemp("shim"))


def _coeffs_rel(c, c0, N):
    """Largest relative difference per coefficient order (the derivatives differ in scale by powers of 1 / T)."""
    a = c.reshape(3, N, 6); b = c0.reshape(3, N, 6)
    return max(float(np.abs(a[:, :, r] - b[:, :, r]).max() / max(np.abs(b[:, :, r]).max(), 1e-300)) for r in range(6))


@pytest.mark.parametrize("kind,N", CASES)
def test_result_on_the_device(pkg, engine, kind, N):
    """The self-consistency of a device result.  info.limits is isdf_traj_limits of the returned arrays, byte for byte (and so the same
    verdict bits).  The coefficients are held to isdf_traj_minco_host of the returned durations at 1e-10 relative per coefficient order,
    not bytes: the solve kernel runs csrc/minco_pcr.hpp with the device's reciprocal (v_rcp_f64 + two Newton steps, <= 1 ulp) and fused
    multiply-adds where the host form divides and rounds every product, which is why that header pins its two forms at 1e-10 relative.
    The _device form, the batch form with B = 1 and a second call give the same bytes."""
    import torch
    p = _case(kind, N)
    e = engine
    res = e.traj_realloc(*ra.args(p), **ra.KW)
    print(f"\n{kind} N {N}: status {res['status']} rounds {res['rounds']} changed {res['pieces_changed']} max factor {res['max_factor']:.6g} "
          f"duration {res['duration_in']:.6g} -> {res['duration_out']:.6g} binding {res['binding']:06b} device {res['device_ms']:.3f} ms")
    assert res["status"] == (2 if (kind, N) == ("aggressive", 65) else 0) and res["checked"] == 0
    ra.hold_common(p, res)
    rel = _coeffs_rel(res["coeffs"], pkg.traj_minco_host(p["head"], p["tail"], p["Q"], res["T"]), N)
    print(f"coefficients against the host solve: {rel:.2e}")
    assert rel <= 1e-10
    lk = ra.limits_kw(ra.KW)
    at = e.traj_limits(res["T"], res["coeffs"], **lk)
    assert ra.same_limits(res["limits"], at) is None, ra.same_limits(res["limits"], at)
    at = e.traj_limits_batch(res["T"][None, :], res["coeffs"][None, :], **lk)[0]
    assert ra.same_limits(res["limits"], at) is None
    again = e.traj_realloc(*ra.args(p), **ra.KW)
    assert ra.same_result(res, again) is None, ra.same_result(res, again)
    Q2 = p["Q"][None, :, :] if N > 1 else None
    bat = e.traj_realloc_batch(p["head"][None, :], p["tail"][None, :], Q2, p["T"][None, :], **ra.KW)
    assert len(bat) == 1 and ra.same_result(res, bat[0]) is None, ra.same_result(res, bat[0])
    dev_t = lambda a: torch.tensor(np.ascontiguousarray(a).reshape(-1), dtype=torch.float64, device="cuda")     # noqa: E731
    dh, dt, dT = dev_t(p["head"]), dev_t(p["tail"]), dev_t(p["T"])
    dQ = dev_t(p["Q"]) if N > 1 else None
    oT = torch.zeros(N, dtype=torch.float64, device="cuda"); oC = torch.zeros(18 * N, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    dev = e.traj_realloc_device(N, dh.data_ptr(), dt.data_ptr(), dQ.data_ptr() if N > 1 else 0, dT.data_ptr(), oT.data_ptr(), oC.data_ptr(), **ra.KW)
    dev["T"], dev["coeffs"] = oT.cpu().numpy(), oC.cpu().numpy()
    assert ra.same_result(res, dev) is None, ra.same_result(res, dev)


def test_batch_of_three_statuses(pkg, product_lib):
    """Status 0, 1 and 2 in one set of launches (N = 5, two rounds): row b equals the single call byte for byte wherever it stands, and
    nothing is allocated from the second call on."""
    ps = [ra.short_piece_case(5), ra.feasible_case(5), ra.aggressive_case(5)]
    e = pkg.Engine(ra.config(pkg))
    kw = dict(rounds=2, **ra.KW)
    H = np.stack([p["head"] for p in ps]); Tl = np.stack([p["tail"] for p in ps]); Q = np.stack([p["Q"] for p in ps]); T = np.stack([p["T"] for p in ps])
    alone = [e.traj_realloc(*ra.args(p), **kw) for p in ps]
    fwd = e.traj_realloc_batch(H, Tl, Q, T, **kw)
    rev = e.traj_realloc_batch(H[::-1], Tl[::-1], Q[::-1], T[::-1], **kw)
    live = []
    for _ in range(2):
        again = e.traj_realloc_batch(H, Tl, Q, T, **kw)
        b = (C.c_longlong * 2)()
        e.lib.isdf_debug_live_bytes(b)
        live.append(tuple(b))
    assert live[0] == live[1], live
    assert [r["status"] for r in fwd] == [0, 1, 2] and [r["rounds"] for r in fwd] == [2, 0, 2]
    for b in range(3):
        for other, what in ((fwd[b], "batch"), (rev[2 - b], "reversed"), (again[b], "again")):
            assert ra.same_result(alone[b], other) is None, (b, what, ra.same_result(alone[b], other))
        ra.hold_common(ps[b], fwd[b])
        at = e.traj_limits(fwd[b]["T"], fwd[b]["coeffs"], **ra.limits_kw(kw))
        assert ra.same_limits(fwd[b]["limits"], at) is None
    e.close()


@pytest.mark.parametrize("kind,N", CLEAN)
def test_host_form_against_device_form(pkg, engine, shim, kind, N):
    """On cases whose every host round is a clean step (every judged per-piece ratio farther than 1e-6 relative from 1: asserted here on
    the host form's trace) a rounding-level difference of the solves and reports flips no verdict: the same status and rounds, the same
    pieces changed, T_out to 1e-9 relative.  Candidate cases dropped as not clean: DROPPED = 0 of 10."""
    assert DROPPED * 2 <= len(CLEAN) + DROPPED
    p = _case(kind, N)
    host, margin, ever = ra.host_trace(pkg, shim, ra.config(pkg), p, **ra.KW)
    assert margin.min() > 1e-6, margin
    dev = engine.traj_realloc(*ra.args(p), **ra.KW)
    rel = float(np.max(np.abs(dev["T"] - host["T"]) / host["T"]))
    print(f"\n{kind} N {N}: status {host['status']} rounds {host['rounds']} smallest margin {margin.min():.2e}  T_out host vs device {rel:.2e}")
    assert (dev["status"], dev["rounds"], dev["binding"]) == (host["status"], host["rounds"], host["binding"])
    assert rel <= 1e-9
    assert ((dev["T"] != p["T"]) == (ever != 0)).all()          # pieces never over in any round keep their bytes


def test_check_of_the_result(pkg, product_lib):
    """check = 1 on a 16^3 occupancy grid with a box robot: info.check is an independent isdf_traj_check of the returned arrays (its three
    timings aside) and the kept rows are that check's; without check the kept rows stay."""
    capi, synth = pkg.capi, pkg.synth
    res_m = 0.5
    occ = np.zeros((16, 16, 16), dtype=np.uint8)
    occ[6:10, 6:10, 0:9] = 1
    head = np.array([1.5, 1.5, 2.0, 0, 0, 0, 0, 0, 0.0]); tail = np.array([6.5, 6.5, 2.5, 0, 0, 0, 0, 0, 0.0])
    Q = np.array([[4.0, 4.0, 5.6]])
    T = np.array([0.9, 0.9])
    shape = synth.make_shape("Box", params=(0.5, 0.3, 0.15), bound_radius=0.7)
    e = pkg.Engine(synth.default_config(capi.V1_SWEPT, safety_hor=0.5, vmax=1.0, omgmax=1.0, thetamax=0.5, integral_intervs=4))
    with pytest.raises(pkg.IsdfError) as ei:            # what the check needs is missing: said before anything is computed
        e.traj_realloc(head, tail, Q, T, check=True)
    assert ei.value.code != 0
    e.set_shape(shape)
    with pytest.raises(pkg.IsdfError) as ei:
        e.traj_realloc(head, tail, Q, T, check=True)
    assert ei.value.code != 0
    e.set_grid(occ, (0, 0, 0), res_m, capi.GRID_OCCUPANCY)
    res = e.traj_realloc(head, tail, Q, T, check=True)
    rows = e.traj_check_points()
    assert res["checked"] == 1 and res["status"] == 0 and res["max_factor"] > 1.0
    ind = e.traj_check(res["T"], res["coeffs"])
    for k, v in res["check"].items():
        if k.endswith("_ms"):
            continue
        assert np.asarray(v).tobytes() == np.asarray(ind[k]).tobytes(), k
    assert rows.shape[0] == res["check"]["n_below_margin"] and e.traj_check_points().tobytes() == rows.tobytes()
    plain = e.traj_realloc(head, tail, Q, T)
    assert plain["checked"] == 0 and plain["check"] is None and ra.same_result(res, plain) in (None, "checked")
    assert e.traj_check_points().tobytes() == rows.tobytes()
    e.close()


def test_argument_errors_on_a_ctx(pkg, engine):
    capi = pkg.capi
    e = engine
    p = ra.short_piece_case(5)
    H, Tl, Q, T = p["head"][None, :], p["tail"][None, :], p["Q"][None, :, :], p["T"][None, :]
    for bad in (dict(rounds=0), dict(rounds=17), dict(headroom=-1.0), dict(headroom=math.nan), dict(f_max=1.0), dict(f_max=math.inf), dict(f_max=math.nan)):
        for call in (lambda: e.traj_realloc(*ra.args(p), **bad), lambda: e.traj_realloc_batch(H, Tl, Q, T, **bad)):
            with pytest.raises(pkg.IsdfError) as ei:
                call()
            assert ei.value.code == capi.ISDF_ERR_INVALID_ARG, bad
    with pytest.raises(pkg.IsdfError) as ei:
        e.traj_realloc_batch(H, Tl, Q, T, check=True)
    assert ei.value.code == capi.ISDF_ERR_INVALID_ARG
    for Tb in (0.0, -1.0, math.inf, math.nan):
        Tx = p["T"].copy(); Tx[1] = Tb
        with pytest.raises(pkg.IsdfError) as ei:
            e.traj_realloc(p["head"], p["tail"], p["Q"], Tx)
        assert ei.value.code == capi.ISDF_ERR_INVALID_ARG
    big = ra.problem(capi.TRAJ_REALLOC_MAX_N + 1, 3, piece_T=2.0)
    with pytest.raises(pkg.IsdfError) as ei:
        e.traj_realloc(*ra.args(big))
    assert ei.value.code == capi.ISDF_ERR_INVALID_ARG
    dp = C.POINTER(C.c_double)
    ptr = lambda a: a.ctypes.data_as(dp)      # noqa: E731
    Qf = np.ascontiguousarray(p["Q"]).reshape(-1)
    Co = np.zeros(18 * 5)
    assert e.lib.isdf_traj_realloc(e.h, 5, ptr(p["head"]), ptr(p["tail"]), ptr(Qf), ptr(p["T"]), None, ptr(p["T"]), ptr(Co), None) == capi.ISDF_ERR_INVALID_ARG
    assert e.traj_realloc(*ra.args(p), **ra.KW)["status"] == 0         # the ctx still works
    # one ctx over several devices: not supported (two shards on device 0 make such a ctx on any machine)
    multi = pkg.Engine(ra.config(pkg), devices=[0, 0])
    for call in (lambda: multi.traj_realloc(*ra.args(p)), lambda: multi.traj_realloc_batch(H, Tl, Q, T)):
        with pytest.raises(pkg.IsdfError) as ei:
            call()
        assert ei.value.code == capi.ISDF_ERR_UNSUPPORTED
    multi.close()
