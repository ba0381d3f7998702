#!/usr/bin/env python
"""Generates tests/golden/traj_limits.npz: the cases of tests/limits_reference.py with the reference extremum of every channel (value,
global time, piece; as float64 and as 40-digit strings), e_cond and kappa, and the sampler's reference rows at the stamps of every
case with their e_cond.  Nothing here comes from the product or the oracle: it is the mpmath model alone.  Every case must pass
limits_reference.check_admissible for every channel - one that does not is replaced by another input, never skipped.  Needs mpmath;
takes a few minutes:
    python tests/golden/make_golden_limits.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import dyn_reference as dr  # noqa: E402
import limits_reference as lr  # noqa: E402


def main():
    mp = lr._mp()
    cases = lr.build_cases()
    R = dict(names=[], n_pieces=[], piece_offset=[], T=[], C=[], cfg=[], samples=[], samples_param=[], value=[], time=[], piece=[], s_digits=[],
             value_digits=[], e_cond=[], kappa=[], const=[], n_stamps=[], stamp_offset=[], stamps=[], rows=[], rows_e_cond=[])
    po = so = 0
    for case in cases:
        ref = lr.reference_extrema(case)
        lr.check_admissible(case, ref)
        e_cond, kappa = lr.conditioning(case, ref)
        if case["name"] == "n2_junction":       # speed and acceleration peak exactly at the junction, seen from the earlier piece
            for ch in (0, 1):
                assert ref[ch]["piece"] == 0 and ref[ch]["s"] == mp.mpf(1) and ref[ch]["t"] == mp.mpf(1), (ch, ref[ch]["piece"], float(ref[ch]["s"]))
        if case["name"] == "n1_monotone":       # extrema at t = 0 and at t = sum(T)
            assert ref[5]["t"] == 0 and ref[0]["t"] == mp.mpf(1.5) and ref[4]["t"] == mp.mpf(1.5), [float(r["t"]) for r in ref]
        if case["name"] == "n2_hover":
            assert all(ref[ch]["const"] for ch in range(lr.NCH)) and ref[2]["value"] == 0 and ref[3]["value"] == 0
        t = lr.stamps(case)
        rows, rec = lr.sampler_reference(case, t)
        n = len(case["T"])
        R["names"].append(case["name"]); R["n_pieces"].append(n); R["piece_offset"].append(po); po += n
        R["T"] += list(case["T"]); R["C"] += list(case["C"])
        R["cfg"].append([case["cfg"][k] for k in dr.CFG_KEYS]); R["samples"].append(case["samples"]); R["samples_param"].append(case["samples_param"])
        R["value"].append([float(r["value"]) for r in ref]); R["time"].append([float(r["t"]) for r in ref]); R["piece"].append([r["piece"] for r in ref])
        R["s_digits"].append([mp.nstr(r["s"], lr.DIGITS) for r in ref]); R["value_digits"].append([mp.nstr(r["value"], lr.DIGITS) for r in ref])
        R["e_cond"].append(e_cond); R["kappa"].append(kappa); R["const"].append([bool(r["const"]) for r in ref])
        R["n_stamps"].append(len(t)); R["stamp_offset"].append(so); so += len(t)
        R["stamps"] += list(t); R["rows"] += [[float(x) for x in row] for row in rows]; R["rows_e_cond"] += list(rec)
        print(f"{case['name']:<14} N {n:>3} S {case['samples']:>3} " + " ".join(
            f"{lr.CH_NAMES[ch]} {float(ref[ch]['value']):.6g}@{float(ref[ch]['t']):.4g} e {e_cond[ch]:.1e} k {kappa[ch]:.1e}" for ch in range(lr.NCH)), flush=True)
    np.savez_compressed(lr.GOLDEN, cfg_keys=np.array(dr.CFG_KEYS), names=np.array(R["names"]), n_pieces=np.array(R["n_pieces"], dtype=np.int32),
                        piece_offset=np.array(R["piece_offset"], dtype=np.int32), T=np.array(R["T"]), C=np.array(R["C"]), cfg=np.array(R["cfg"]),
                        samples=np.array(R["samples"], dtype=np.int32), samples_param=np.array(R["samples_param"], dtype=np.int32),
                        value=np.array(R["value"]), time=np.array(R["time"]), piece=np.array(R["piece"], dtype=np.int32),
                        s_digits=np.array(R["s_digits"]), value_digits=np.array(R["value_digits"]), e_cond=np.array(R["e_cond"]),
                        kappa=np.array(R["kappa"]), const=np.array(R["const"]), n_stamps=np.array(R["n_stamps"], dtype=np.int32),
                        stamp_offset=np.array(R["stamp_offset"], dtype=np.int32), stamps=np.array(R["stamps"]), rows=np.array(R["rows"]),
                        rows_e_cond=np.array(R["rows_e_cond"]))
    print(len(cases), "cases,", os.path.getsize(lr.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
