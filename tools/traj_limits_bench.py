#!/usr/bin/env python
"""Times the dynamic-limits report (isdf_traj_limits*): the device time of one report at N = 40 and N = 400, of a batch of
128 x N = 40, and one host-form thread (isdf_traj_limits_host) on the same inputs.

Device time = isdf_traj_limits_info.device_ms: events on the stream around the call's two launches (no copies).  Call time = a
host clock around the whole entry point, which ends in a stream synchronise (it includes staging the trajectory and fetching the
report).  Every shape is warmed up before its window; medians and the spread (min, max) of `--repeats` calls are kept.  The
inputs are seeded MINCO trajectories of the synthetic workload, so two runs time the same work.

    python tools/traj_limits_bench.py --out profiles/traj_limits_bench.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402


def trajectories(synth, B, N, seed):
    ext = np.array([60.0, 60.0, 20.0])
    T, Cc = [], []
    for b in range(B):
        t, cf = synth.random_trajectory(ext, N, seed=seed + b, piece_T=0.6, jitter=0.8, margin=3.0)
        T.append(t); Cc.append(synth.colmajor(cf))
    return np.stack(T), np.stack(Cc)


def stats(x):
    x = np.asarray(x, dtype=np.float64)
    return {"median": float(np.median(x)), "min": float(x.min()), "max": float(x.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--host-repeats", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch  # noqa: F401  (torch first: see tests/conftest.py)
    if torch.cuda.is_available():
        torch.zeros(1, device="cuda")
    pkg = g.load_package()
    capi, synth = pkg.capi, pkg.synth
    cfg = synth.default_config(capi.V3_ESDF_TILE, integral_intervs=16)
    eng = pkg.Engine(cfg)
    rows = []
    for label, B, N in (("one report, N = 40", 1, 40), ("one report, N = 400", 1, 400), ("batch of 128, N = 40", 128, 40)):
        T, Cc = trajectories(synth, B, N, seed=100 + N)
        for _ in range(a.warmup):
            rep = eng.traj_limits_batch(T, Cc)
        dev, call = [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            rep = eng.traj_limits_batch(T, Cc)
            call.append((time.perf_counter() - t0) * 1e3)
            dev.append(rep[0]["device_ms"])
        t0 = time.perf_counter()
        for _ in range(a.host_repeats):
            host = [pkg.traj_limits_host(cfg, T[b], Cc[b]) for b in range(B)]
        host_ms = (time.perf_counter() - t0) * 1e3 / a.host_repeats
        worst = max(abs(host[b]["value"][ch] - rep[b]["value"][ch]) / max(abs(host[b]["value"][ch]), 1e-300) for b in range(B) for ch in range(6))
        rows.append({"case": label, "B": B, "N": N, "samples": int(rep[0]["samples"]), "launches": 2, "device_ms": stats(dev), "call_ms": stats(call),
                     "host_form_one_thread_ms": host_ms, "device_vs_host_max_rel": float(worst)})
        print(f"{label:<22} samples {rep[0]['samples']:>3}  device {rows[-1]['device_ms']['median']:.4f} ms "
              f"[{rows[-1]['device_ms']['min']:.4f}, {rows[-1]['device_ms']['max']:.4f}]  call {rows[-1]['call_ms']['median']:.4f} ms  "
              f"host form, one thread {host_ms:.2f} ms  device vs host {worst:.1e}", flush=True)
    eng.close()
    res = {"tool": "tools/traj_limits_bench.py", "repeats": a.repeats, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "rows": rows}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
