#!/usr/bin/env python
"""Developer tool: the mid end, host form against device form, medians of 5 after a warm-up:
  - time per callback (isdf_midend_cost) at N = 8, 40, 400, a loop of calls per sample; both forms go through the same ctypes call,
    whose few microseconds are in both figures
  - time per round of isdf_midend_cost_batch at 128 x 40 in device mode against the host form's 128 solves (mode 1: one after the
    other on the calling thread)
  - iterations and wall time of the demo1 fit (tests/demo_headless.py's plan) in both forms
Writes profiles/midend_bench.json.  usage: midend_bench.py [quick]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as graft
import torch  # noqa: F401  (torch first: see tests/conftest.py)
import midend_common as mc

pkg = graft.load_package(); capi = pkg.capi
quick = len(sys.argv) > 1 and sys.argv[1] == "quick"
REPS, CALLS = 5, (50 if quick else 400)


def median_us(fn, calls):
    fn()                                        # warm-up (buffers, first launch)
    samples = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        samples.append((time.perf_counter() - t0) / calls * 1e6)
    return float(np.median(samples)), [float(s) for s in samples]


out = {"reps": REPS, "calls_per_sample": CALLS, "callback_us": {}, "batch_round_us": {}, "demo1_fit": {}}
for N in (8, 40, 400):
    head, tail, ref, x = mc.cost_problem(N, 300 + N)
    eng = pkg.Engine(pkg.synth.default_config(capi.V3_ESDF_TILE)); eng.set_trajectory(N, head, tail, 0.0)
    prm = eng.midend_params()
    row = {}
    for mode, label in ((capi.MINCO_HOST, "host"), (capi.MINCO_DEVICE, "device")):
        eng.set_minco_mode(mode)
        row[label], row[label + "_samples"] = median_us(lambda: eng.midend_cost(ref, x, prm), CALLS)
    out["callback_us"][str(N)] = row
    print(f"callback N={N}: host {row['host']:.1f} us, device {row['device']:.1f} us", flush=True)
    eng.close()

N, nb = 40, 128
probs = [mc.cost_problem(N, 900 + b) for b in range(nb)]
heads = np.array([p[0] for p in probs]); tails = np.array([p[1] for p in probs]); refs = np.array([p[2] for p in probs]); xs = np.array([p[3] for p in probs])
eng = pkg.Engine(pkg.synth.default_config(capi.V3_ESDF_TILE)); eng.set_trajectory(N, heads[0], tails[0], 0.0)
prm = eng.midend_params()
for mode, label in ((capi.MINCO_HOST, "host_128_solves"), (capi.MINCO_DEVICE, "device_round")):
    eng.set_minco_mode(mode)
    out["batch_round_us"][label], out["batch_round_us"][label + "_samples"] = median_us(lambda: eng.midend_cost_batch(heads, tails, refs, xs, prm), max(10, CALLS // 10))
print(f"batch 128 x 40: host {out['batch_round_us']['host_128_solves']:.0f} us, device round {out['batch_round_us']['device_round']:.0f} us", flush=True)
eng.close()

from test_gpu_demo import _demo
g, plan, cfg, shape, eng, P = _demo(pkg, "CappedCone")
prm = eng.midend_params(integral_intervs=int(plan.sweep.integral_intervs))
for mode, label in ((capi.MINCO_HOST, "host"), (capi.MINCO_DEVICE, "device")):
    eng.set_minco_mode(mode)
    walls = []
    for _ in range(REPS + 1):
        x, T, cm, r = eng.midend_fit(P["Q"], np.full(P["N"], plan.inittime), prm)
        walls.append(r["wall_ms"])
    out["demo1_fit"][label] = {"N": int(P["N"]), "status": r["status"], "iterations": r["iterations"], "evaluations": r["evaluations"], "f": r["f"],
                               "wall_ms_median": float(np.median(walls[1:])), "wall_ms_samples": walls[1:]}
    print(f"demo1 fit ({label}): {out['demo1_fit'][label]}", flush=True)
eng.close()
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "midend_bench.json"), "w") as f:
    json.dump(out, f, indent=1)
print("wrote profiles/midend_bench.json")
