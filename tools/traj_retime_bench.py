#!/usr/bin/env python
"""Times the retiming of a trajectory to its dynamic limits (isdf_traj_retime*): one trajectory of N = 40 and of N = 400 (ladder 32, 3
rounds) and a batch of 16 x N = 40 (ladder 16, 3 rounds).  Per case:

  device_ms         isdf_traj_retime_info.device_ms: events on the stream around the call's 1 + 4 rounds launches (no copies)
  call_ms           a host clock around the whole entry point (staging, the launches, the one hand-over)
  composed_ms       what a caller had before this entry point: per round the candidates scaled on the host (isdf_traj_scale_host), one
                    isdf_traj_limits_batch over them, the pick on the host
  host_form_ms      isdf_traj_retime_host on one thread

Every case is warmed up before its window; medians and the spread (min, max) of `--repeats` calls are kept.  The inputs are seeded MINCO
trajectories of the synthetic workload under limits that bind (vmax 1.5, omgmax 1.0, thetamax 0.4), so two runs time the same work.

    python tools/traj_retime_bench.py --out profiles/traj_retime_bench.json
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


def composed(pkg, eng, T, Cc, L, R, s_lo=1.0, s_hi=8.0):
    """The search out of the parts a caller had before: host scaling + isdf_traj_limits_batch per round, picked on the host."""
    B, N = T.shape
    a = np.full(B, s_lo); b = np.full(B, s_hi)
    done = np.zeros(B, dtype=bool)
    scale = np.zeros(B)
    for r in range(R):
        cand = np.empty((B, L))
        sT = np.empty((B * L, N)); sC = np.empty((B * L, 18 * N))
        for t in range(B):
            for i in range(L):
                cand[t, i] = a[t] if i == 0 else (b[t] if i == L - 1 else a[t] + (b[t] - a[t]) * i / (L - 1))
                sT[t * L + i], sC[t * L + i] = pkg.traj_scale_host(T[t], Cc[t], cand[t, i])
        reps = eng.traj_limits_batch(sT, sC)
        for t in range(B):
            if done[t]:
                continue
            ok = [reps[t * L + i]["feasible"] == reps[t * L + i]["judged"] for i in range(L)]
            bad = [i for i in range(L) if not ok[i]]
            k = bad[-1] + 1 if bad else 0
            if r == 0 and (k == L or k == 0):
                done[t] = True; scale[t] = cand[t, min(k, L - 1)]
                continue
            k = min(max(k, 1), L - 1)
            a[t], b[t] = cand[t, k - 1], cand[t, k]
            scale[t] = cand[t, k]
    return scale


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--composed-repeats", type=int, default=20)
    ap.add_argument("--host-repeats", type=int, default=1)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch  # noqa: F401  (torch first: see tests/conftest.py)
    if torch.cuda.is_available():
        torch.zeros(1, device="cuda")
    pkg = g.load_package()
    capi, synth = pkg.capi, pkg.synth
    cfg = synth.default_config(capi.V3_ESDF_TILE, integral_intervs=16, vmax=1.5, omgmax=1.0, thetamax=0.4)
    eng = pkg.Engine(cfg)
    rows = []
    for label, B, N, L, R in (("one trajectory, N = 40", 1, 40, 32, 3), ("one trajectory, N = 400", 1, 400, 32, 3), ("batch of 16, N = 40", 16, 40, 16, 3)):
        T, Cc = trajectories(synth, B, N, seed=100 + N)
        for _ in range(a.warmup):
            res = eng.traj_retime_batch(T, Cc, ladder=L, rounds=R)
        dev, call = [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            res = eng.traj_retime_batch(T, Cc, ladder=L, rounds=R)
            call.append((time.perf_counter() - t0) * 1e3)
            dev.append(res[0]["device_ms"])
        comp = []
        for it in range(2 + a.composed_repeats):
            t0 = time.perf_counter()
            sc = composed(pkg, eng, T, Cc, L, R)
            if it >= 2:
                comp.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        for _ in range(a.host_repeats):
            host = [pkg.traj_retime_host(cfg, T[b], Cc[b], ladder=L, rounds=R) for b in range(B)]
        host_ms = (time.perf_counter() - t0) * 1e3 / a.host_repeats
        step = 7.0 / (L - 1) ** R
        rows.append({"case": label, "B": B, "N": N, "ladder": L, "rounds": R, "launches": 1 + 4 * R, "device_ms": stats(dev), "call_ms": stats(call),
                     "composed_ms": stats(comp), "host_form_one_thread_ms": host_ms, "status": [int(r["status"]) for r in res],
                     "scale": [float(r["scale"]) for r in res],
                     "composed_equals_device": bool(all(sc[b] == res[b]["scale"] for b in range(B))),
                     "host_vs_device_steps": float(max(abs(host[b]["scale"] - res[b]["scale"]) for b in range(B)) / step)})
        q = rows[-1]
        print(f"{label:<24} L {L} R {R}  device {q['device_ms']['median']:.3f} ms [{q['device_ms']['min']:.3f}, {q['device_ms']['max']:.3f}]  "
              f"call {q['call_ms']['median']:.3f} ms [{q['call_ms']['min']:.3f}, {q['call_ms']['max']:.3f}]  composed {q['composed_ms']['median']:.3f} ms "
              f"[{q['composed_ms']['min']:.3f}, {q['composed_ms']['max']:.3f}]  host form {host_ms:.1f} ms  status {q['status']}  "
              f"composed == device {q['composed_equals_device']}  host vs device {q['host_vs_device_steps']:.2f} last steps", flush=True)
    eng.close()
    out = {"tool": "tools/traj_retime_bench.py", "repeats": a.repeats, "warmup": a.warmup, "composed_repeats": a.composed_repeats,
           "device": torch.cuda.get_device_name(0), "rows": rows}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
