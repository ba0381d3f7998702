#!/usr/bin/env python
"""Generates tests/golden/dyn_edges.npz: the edge cases of tests/dyn_reference.py with their high-precision cost and gradient.

Unlike the other fixtures this one does NOT come from the oracle: cost and the 19 gradient entries of every case are the mpmath
model's (forward map only, central differences at 70 digits), stored as float64 and as 40-digit strings.  e_cond is the largest
movement of that cost / gradient (dyn_reference.measure) when every input - the 18 coefficients and T - moves by one ulp, over two
fixed sign patterns: what no float64 evaluation of these inputs can be held below.  Needs mpmath; takes a few minutes:
    python tests/golden/make_golden_dyn.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import dyn_reference as dr  # noqa: E402

DIGITS = 40


def one_ulp_patterns(case):
    """Two (c, T) with every input moved by one ulp, signs from a fixed generator."""
    rng = np.random.default_rng(20240607)
    out = []
    for _ in range(2):
        s = rng.integers(0, 2, size=19) * 2 - 1
        c = case["c"] + s[:18].reshape(3, 6) * np.spacing(np.abs(case["c"]))
        out.append((c, case["T"] + s[18] * np.spacing(case["T"])))
    return out


def reference(case):
    mp = dr._mp()
    cost = dr.cost_mp(case["c"], case["T"], case["K"], case["cfg"])
    grad = dr.grad_mp(case["c"], case["T"], case["K"], case["cfg"])
    e_cond = 0.0
    gs = max(abs(x) for x in grad)
    for c, T in one_ulp_patterns(case):
        c1 = dr.cost_mp(c, T, case["K"], case["cfg"])
        g1 = dr.grad_mp(c, T, case["K"], case["cfg"])
        eg = max(abs(a - b) for a, b in zip(g1, grad))
        e_cond = max(e_cond, float(eg / gs) if gs > 0 else float(eg), float(abs(c1 - cost) / cost) if cost > 0 else float(abs(c1 - cost)))
    return cost, grad, e_cond, mp


def main():
    cases = dr.build_cases()
    rows = dict(names=[], c=[], T=[], K=[], cfg=[], cost=[], grad=[], cost_digits=[], grad_digits=[], e_cond=[])
    for case in cases:
        cost, grad, e_cond, mp = reference(case)
        rows["names"].append(case["name"]); rows["c"].append(case["c"]); rows["T"].append(case["T"]); rows["K"].append(case["K"])
        rows["cfg"].append([case["cfg"][k] for k in dr.CFG_KEYS])
        rows["cost"].append(float(cost)); rows["grad"].append([float(x) for x in grad])
        rows["cost_digits"].append(mp.nstr(cost, DIGITS)); rows["grad_digits"].append([mp.nstr(x, DIGITS) for x in grad])
        rows["e_cond"].append(e_cond)
        print(f"{case['name']:<22} K {case['K']:>3} T {case['T']:<5g} cost {float(cost):.6e} max|g| {max(abs(float(x)) for x in grad):.3e} e_cond {e_cond:.2e}",
              flush=True)
    np.savez_compressed(dr.GOLDEN, cfg_keys=np.array(dr.CFG_KEYS), names=np.array(rows["names"]), c=np.array(rows["c"]), T=np.array(rows["T"]),
                        K=np.array(rows["K"], dtype=np.int32), cfg=np.array(rows["cfg"]), cost=np.array(rows["cost"]), grad=np.array(rows["grad"]),
                        cost_digits=np.array(rows["cost_digits"]), grad_digits=np.array(rows["grad_digits"]), e_cond=np.array(rows["e_cond"]))
    print(len(cases), "cases,", os.path.getsize(dr.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
