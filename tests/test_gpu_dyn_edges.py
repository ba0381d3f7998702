"""The tail of the integral sweep (tile_sweep.hip: flat_core, flat_core2, the three dynamics penalties, flat_backward_from under
ISDF_LEAN_MATH) held to the high-precision golden of tests/dyn_reference.py at its edges: tilt up to pi - 0.05, near free fall,
exact hover, every region of the smoothed L1 of each penalty, drag off / tiny speed_eps / 50 m/s, T = 0.05 and 12, K across the
128-sample pass boundary.

Measure, per piece: max(max|g - g_ref| / max|g_ref| over the 19 entries, |cost - cost_ref| / |cost_ref|).
Bound, per case:    32 x max(e_orc, e_cond, 2^-50), never looser than REL_TOL.  e_orc is the oracle's own deviation from the
golden, computed here; e_cond the golden's movement under one ulp of every input (in the fixture).  The five bits stand for what
separates device from oracle by construction - one ulp per reciprocal-multiply quotient at up to two levels of nesting, FMA
contraction, the re-associated sums - and are not fitted to the device.  The device's measured deviations go to the pytest log
(DESIGN.md section 6 keeps the worst per path).

Which launch a path reaches: without the collision term (enable_pos = 0) a step is the stand-alone tail launch whatever K is;
the fused one-launch step needs enable_pos = 1, so the fused tail (K + 1 <= 128) is reached by the collision-slot tests.
"""
import numpy as np
import pytest

import dyn_reference as dr
from common import REL_TOL, assert_close, traj

pytestmark = pytest.mark.gpu

GOLD = dr.load_golden()
BY_NAME = {c["name"]: c for c in GOLD}
MARGIN = 32.0
FLOOR = 2.0 ** -50
_LINES = []
_WORST = {}


def report(capsys, *paths):
    """The device's deviations of the given paths into the log, uncaptured."""
    with capsys.disabled():
        print("\ndynamics edges: device vs the high-precision model (e_dev | bound = 32 max(e_orc, e_cond, 2^-50))")
        for l in _LINES:
            print(l)
        del _LINES[:]
        for path in paths:
            w = _WORST[path]
            print(f"worst {path:<24} e_dev {w['e'][0]:.2e} ({w['e'][1]}); largest e_dev / bound {w['r'][0]:.3f} ({w['r'][1]})")


@pytest.fixture(scope="module")
def bounds(pkg, orc):
    """name -> (bound, e_orc): the oracle against the golden, once."""
    out = {}
    for case in GOLD:
        o = orc.Oracle(dr.make_config(pkg, case), threads=1)
        cost, gT, gC, _ = o.eval(np.array([case["T"]]), case["coeffs"])
        e_orc = dr.measure(cost, dr.piece_entries(gT, gC), case["cost"], case["grad"])
        out[case["name"]] = (min(MARGIN * max(e_orc, case["e_cond"], FLOOR), REL_TOL), e_orc)
    return out


def hold(path, case, cost, g, bounds, failures, quiet=False):
    e = dr.measure(cost, g, case["cost"], case["grad"])
    bound, e_orc = bounds[case["name"]]
    if not quiet:
        _LINES.append(f"{path:<24} {case['name']:<22} e_dev {e:.2e} bound {bound:.2e} e_orc {e_orc:.2e} e_cond {case['e_cond']:.2e}")
    w = _WORST.setdefault(path, dict(e=(-1.0, ""), r=(-1.0, "")))
    w["e"] = max(w["e"], (e, case["name"]))
    w["r"] = max(w["r"], (e / bound, case["name"]))
    if not e <= bound:
        failures.append(f"{path} {case['name']}: e_dev {e:.3e} > bound {bound:.3e}")


def groups():
    """Cases that share K and every config value, in the golden's order."""
    out = {}
    for case in GOLD:
        out.setdefault(dr.group_key(case), []).append(case)
    return list(out.values())


def single(pkg, case, **cfg_kw):
    eng = pkg.Engine(dr.make_config(pkg, case, **cfg_kw))
    cost, gT, gC = eng.eval_single(np.array([case["T"]]), case["coeffs"])
    eng.close()
    return cost, dr.piece_entries(gT, gC)


@pytest.mark.parametrize("no_fuse", [False, True], ids=["default", "ISDF_NO_FUSE"])
def test_each_case_on_a_fresh_engine(pkg, product_lib, bounds, monkeypatch, capsys, no_fuse):
    """Paths 1, 2 and 6: every case alone; the below-zero cases give exactly 0.0 everywhere."""
    if no_fuse:
        monkeypatch.setenv("ISDF_NO_FUSE", "1")
    else:
        monkeypatch.delenv("ISDF_NO_FUSE", raising=False)
    failures = []
    for case in GOLD:
        cost, g = single(pkg, case)
        hold("single" + ("/no_fuse" if no_fuse else ""), case, cost, g, bounds, failures)
        if case["name"] in dr.BELOW:
            assert cost == 0.0 and not np.any(g), case["name"]
    a, b = single(pkg, BY_NAME["hover_omg"]), single(pkg, BY_NAME["hover_omg_tilt"])
    assert a[0] == b[0] and np.array_equal(a[1], b[1]), "the tilt term must read exactly zero at hover"
    report(capsys, "single" + ("/no_fuse" if no_fuse else ""))
    assert not failures, "\n".join(failures)


def test_batched_rows_and_accumulate(pkg, product_lib, bounds, capsys):
    """Path 3: every group of cases with one K and config as ONE batched eval, each row held to its own case; then the same call
    adding into non-zero buffers."""
    failures = []
    n_batched = 0
    for grp in groups():
        if len(grp) < 2:
            continue
        n_batched += 1
        eng = pkg.Engine(dr.make_config(pkg, grp[0]))
        Ts = [np.array([c["T"]]) for c in grp]; Cs = [c["coeffs"] for c in grp]
        cost, gTs, gCs = eng.eval(Ts, Cs)
        for b, case in enumerate(grp):
            hold("batch", case, cost[b], dr.piece_entries(gTs[b], gCs[b]), bounds, failures)
        acc = (np.full(len(grp), 2.5), [np.full(1, -1.0) for _ in grp], [np.full(18, 3.0) for _ in grp])
        eng.eval(Ts, Cs, accumulate_into=acc)
        eps = np.finfo(np.float64).eps
        for b in range(len(grp)):       # prior + result, rounded once (a second rounding would still pass; a lost prior would not)
            for got, prior, r in ((acc[0][b], 2.5, cost[b]), (acc[1][b], -1.0, gTs[b]), (acc[2][b], 3.0, gCs[b])):
                assert np.all(np.abs(got - (prior + r)) <= 2 * eps * (abs(prior) + np.abs(r))), (grp[b]["name"], got, r)
        eng.close()
    assert n_batched >= 3
    report(capsys, "batch")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("which", ["body_rate_alone", "all_on"])
def test_long_trajectory_places_every_piece(pkg, product_lib, bounds, capsys, which):
    """Path 4: 70 pieces drawn from one group of cases, shuffled; pieces are independent, so every piece's 19 entries are its
    case's golden at the piece's rows.  Also as three shards, summed.  Two groups: the largest (the tilt sweep and hover with the
    body-rate penalty alone) and the K = 16 cases with all three penalties on (near free fall, 50 m/s, T = 0.05 ... 12 in one
    trajectory)."""
    grp = max(groups(), key=len) if which == "body_rate_alone" else next(g for g in groups() if g[0]["name"] == "near_free_fall")
    assert len(grp) >= 5 and (which == "body_rate_alone" or len({c["T"] for c in grp}) >= 4)
    N = 70
    order = np.random.default_rng(7).permutation(np.arange(N) % len(grp))
    T = np.array([grp[k]["T"] for k in order])
    cm = np.zeros(18 * N)
    for i, k in enumerate(order):
        for d in range(3):
            cm[d * 6 * N + 6 * i: d * 6 * N + 6 * i + 6] = grp[k]["c"][d]
    want_cost = float(sum(grp[k]["cost"] for k in order))
    # the trajectory's cost is a sum of 70 piece costs of one sign: each within its bound, plus half an ulp per addition
    cost_bound = sum(bounds[grp[k]["name"]][0] * grp[k]["cost"] for k in order) + N * 2.0 ** -53 * want_cost
    eng = pkg.Engine(dr.make_config(pkg, grp[0]))
    cost, gT, gC = eng.eval_single(T, cm)
    sharded = [np.zeros(1), np.zeros(N), np.zeros(18 * N)]
    for r in range(3):
        eng.set_shard(r, 3)
        c_r, gT_r, gC_r = eng.eval_single(T, cm)
        sharded[0] += c_r; sharded[1] += gT_r; sharded[2] += gC_r
    eng.close()
    failures = []
    paths = (f"long {which}", f"long {which}/3 shards")
    for path, (c_, gT_, gC_) in zip(paths, ((cost, gT, gC), (float(sharded[0][0]), sharded[1], sharded[2]))):
        assert abs(c_ - want_cost) <= cost_bound, (path, c_, want_cost, cost_bound)
        for i, k in enumerate(order):
            hold(path, grp[k], grp[k]["cost"], dr.piece_entries(gT_, gC_, i), bounds, failures, quiet=True)
    report(capsys, *paths)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("no_fuse", [False, True], ids=["fused", "ISDF_NO_FUSE"])
def test_collision_slot_path_with_zero_sums(pkg, product_lib, bounds, monkeypatch, capsys, no_fuse):
    """Path 5: enable_pos = 1 on V3 over an obstacle-free ESDF with a Box: the tail takes the collision sums from their slots -
    all zero - and must give the same goldens within the same bounds.  K + 1 <= 128 is the fused launch's tail (one pass), from
    K = 128 on sweep and tail are two launches; with ISDF_NO_FUSE always two.

    Whether a step is the fused launch is the library's decision (sweep_can_fuse: the shape's identity flag, the workgroup budget,
    the profiler off).  It shows in how the step crossed PCIe: only a step that is ONE fused launch is handed over host-direct,
    every other one takes the copy path (include/isdf_accel.h, isdf_host_path) - asserted per case, so a change that stops these
    steps from fusing fails here instead of leaving the fused tail uncovered."""
    capi, synth = pkg.capi, pkg.synth
    if no_fuse:
        monkeypatch.setenv("ISDF_NO_FUSE", "1")
    else:
        monkeypatch.delenv("ISDF_NO_FUSE", raising=False)
    for k in ("ISDF_NO_HOST_DIRECT", "ISDF_FUSE_MAX_BLOCKS"):
        monkeypatch.delenv(k, raising=False)
    direct = (capi.HOST_PATH_DIRECT_BAR, capi.HOST_PATH_DIRECT_MAPPED)
    res = 4.0
    esdf = np.full((64, 64, 64), 100.0, dtype=np.float32)       # 256 m cube, nothing within reach: dr.CENTRE is its middle
    shape = synth.make_shape("Box")
    failures = []
    for grp in groups():
        eng = pkg.Engine(dr.make_config(pkg, grp[0], enable_pos=1, kernel_size=3, safety_hor=0.5))
        eng.set_grid(esdf, (0, 0, 0), res, capi.GRID_ESDF)
        eng.set_shape(shape)
        for case in grp:
            assert np.all(np.abs(np.polyval(case["c"][:, ::-1].T, np.linspace(0, case["T"], 65)[:, None]) - 128.0) <= 100.0)
            cost, gT, gC = eng.eval_single(np.array([case["T"]]), case["coeffs"])
            hold("slots" + ("/no_fuse" if no_fuse else ""), case, cost, dr.piece_entries(gT, gC), bounds, failures)
            fused = not no_fuse and case["K"] + 1 <= 128
            assert (eng.host_path() in direct) == fused, (case["name"], eng.host_path(), "fused launch expected" if fused else "two launches expected")
            if case["name"] in dr.BELOW:
                assert cost == 0.0 and not np.any(gT) and not np.any(gC), case["name"]
        assert eng.stats()["grad_pairs"] == 0
        eng.close()
    report(capsys, "slots" + ("/no_fuse" if no_fuse else ""))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("limit", ["vmax", "omgmax", "thetamax"])
def test_each_penalty_alone_on_a_benign_trajectory(pkg, orc, product_lib, limit):
    """Path 7: what test_dynamics_only_sweep never established - each penalty, with the other two out of reach, is active and right."""
    capi, synth = pkg.capi, pkg.synth
    res = 0.5
    occ = synth.random_box_map((48, 48, 32), res=res, occupancy=0.12, seed=3, edge=(1.0, 3.0))
    T, cm = traj(pkg, occ, res, N=6, piece_T=0.35)
    lim = dict(vmax=1.0e3, omgmax=1.0e3, thetamax=1.0e3)
    lim[limit] = dict(vmax=2.0, omgmax=1.0, thetamax=0.3)[limit]
    cfg = synth.default_config(capi.V3_ESDF_TILE, integral_intervs=16, enable_pos=0, **lim)
    eng = pkg.Engine(cfg)
    cost, gT, gC = eng.eval_single(T, cm)
    eng.close()
    c0, gT0, gC0, _ = orc.Oracle(cfg, threads=1).eval(T, cm)
    assert c0 > 0 and cost > 0, (limit, cost, c0)
    assert abs(cost - c0) <= REL_TOL * abs(c0)
    assert_close(gC, gC0, limit + " gradC")
    assert_close(gT, gT0, limit + " gradT")
