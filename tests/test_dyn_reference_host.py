"""The dynamics edge cases (tests/dyn_reference.py) on the CPU: the committed golden is what the high-precision model gives, and
the oracle - the restated adjoint in float64 - stays within 1e-5 of it at every edge, exactly zero below the penalties' zero."""
import numpy as np
import pytest

import dyn_reference as dr

GOLD = dr.load_golden()
BY_NAME = {c["name"]: c for c in GOLD}
E_ORC_MAX = 1e-5        # the north star's tolerance: past it the oracle would be no reference for the device at that edge


def oracle_piece(pkg, orc, case):
    o = orc.Oracle(dr.make_config(pkg, case), threads=1)
    cost, gT, gC, _ = o.eval(np.array([case["T"]]), case["coeffs"])
    return cost, dr.piece_entries(gT, gC)


def test_case_list_covers_the_edges():
    names = set(BY_NAME)
    for tag in ("0.31", "1.0", "pi_2", "2.5", "3.0", "pi-0.05"):
        assert {f"tilt_{tag}_theta", f"tilt_{tag}_omg"} <= names
    for pen in ("vel", "omg", "theta"):
        for tag in ("below", "under_mu", "3mu") + (("quarter",) if pen != "theta" else ()):
            assert f"l1_{pen}_{tag}" in names
    assert {"small_tilt", "hover_omg", "hover_omg_tilt", "near_free_fall", "no_drag", "speed_eps_1e-12", "speed_50", "T_0.05", "T_12"} <= names
    assert {BY_NAME[f"K{K}_{s}"]["K"] for K in (1, 2, 16, 127, 128, 150) for s in ("mid", "tilted")} == {1, 2, 16, 127, 128, 150}
    for n in dr.BELOW:
        assert BY_NAME[n]["K"] == 1 and BY_NAME[n]["cost"] == 0.0 and not np.any(BY_NAME[n]["grad"])
    for c in GOLD:      # every other case has its penalty ACTIVE
        assert c["name"] in dr.BELOW or (c["cost"] > 0 and np.max(np.abs(c["grad"])) > 0), c["name"]


def test_builder_reproduces_golden_inputs():
    pytest.importorskip("mpmath")
    built = dr.build_cases()        # also asserts that no sample stands within 1e-12 of a smoothed-L1 region boundary
    assert [c["name"] for c in built] == [c["name"] for c in GOLD]
    for b, g in zip(built, GOLD):
        assert np.array_equal(b["c"], g["c"]) and b["T"] == g["T"] and b["K"] == g["K"] and b["cfg"] == g["cfg"], b["name"]


@pytest.mark.parametrize("name", [c["name"] for c in GOLD])
def test_golden_is_the_live_model(name):
    """(a) cost and all 19 gradient entries, to 1e-30."""
    pytest.importorskip("mpmath")
    mp = dr._mp()
    case = BY_NAME[name]
    cost = dr.cost_mp(case["c"], case["T"], case["K"], case["cfg"])
    want = mp.mpf(case["cost_digits"])
    assert abs(cost - want) <= mp.mpf("1e-30") * abs(want)
    assert float(want) == case["cost"]
    gref = [mp.mpf(s) for s in case["grad_digits"]]
    assert [float(x) for x in gref] == list(case["grad"])
    got = dr.grad_mp(case["c"], case["T"], case["K"], case["cfg"])
    scale = max(abs(x) for x in gref)
    for e in range(19):
        assert abs(got[e] - gref[e]) <= mp.mpf("1e-30") * scale, (name, e)


def test_oracle_within_bound_of_the_model(pkg, orc, capsys):
    """(b) per piece, every case, no exceptions.  The table goes to the log uncaptured."""
    bad = []
    worst, lines = 0.0, ["", "dynamics edges: oracle vs the high-precision model (e_orc), conditioning (e_cond)"]
    for case in GOLD:
        cost, g = oracle_piece(pkg, orc, case)
        e = dr.measure(cost, g, case["cost"], case["grad"])
        lines.append(f"{case['name']:<22} K {case['K']:>3} T {case['T']:<5g} cost {case['cost']:.6e} max|g| {np.max(np.abs(case['grad'])):.3e} "
                     f"e_orc {e:.2e} e_cond {case['e_cond']:.2e}")
        worst = max(worst, e)
        bad += [(case["name"], e)] if not e <= E_ORC_MAX else []
    with capsys.disabled():
        print("\n".join(lines + [f"worst e_orc {worst:.2e}"]))
    assert not bad, bad


@pytest.mark.parametrize("name", dr.BELOW)
def test_oracle_exactly_zero_below_zero(pkg, orc, name):
    """(c)"""
    cost, g = oracle_piece(pkg, orc, BY_NAME[name])
    assert cost == 0.0 and not np.any(g)


def test_oracle_tilt_term_reads_zero_at_hover(pkg, orc):
    """thetamax = 0.3 at exact hover: the tilt penalty is switched on and contributes exactly nothing."""
    a = oracle_piece(pkg, orc, BY_NAME["hover_omg"]); b = oracle_piece(pkg, orc, BY_NAME["hover_omg_tilt"])
    assert a[0] == b[0] and np.array_equal(a[1], b[1])
