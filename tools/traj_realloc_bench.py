#!/usr/bin/env python
"""Times the per-piece re-allocation of durations to the dynamic limits (isdf_traj_realloc*) and records what it achieves, on the inputs
of tools/traj_retime_bench.py: one trajectory of N = 40 and of N = 400 and a batch of 16 x N = 40 (defaults: 8 rounds, headroom 0.02,
f_max 2).  Per case:

  device_ms         isdf_traj_realloc_info.device_ms: events on the stream around the call's 4 (rounds + 1) launches (no copies)
  call_ms           a host clock around the whole entry point (staging, the launches, the one hand-over)
  composed_ms       what a caller had before this entry point: per round a host solve per trajectory, one isdf_traj_limits_batch over the
                    batch with its per-piece rows, the factor rule and the update on the host (numpy)
  host_form_ms      isdf_traj_realloc_host on one thread
  outcome           status, rounds, duration_in, duration_out per trajectory, next to the scale and duration_out of uniform retiming
                    (isdf_traj_retime_batch, its defaults) on the same input

Every case is warmed up before its window; medians and the spread (min, max) of `--repeats` calls are kept.

    python tools/traj_realloc_bench.py --out profiles/traj_realloc_bench.json
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


def problems(synth, B, N, seed):
    """The waypoint problems behind traj_retime_bench.py's trajectories: heads, tails (at rest), Q, T and the coefficients themselves."""
    ext = np.array([60.0, 60.0, 20.0])
    H, Tl, Q, T, Cc = [], [], [], [], []
    for b in range(B):
        t, cf = synth.random_trajectory(ext, N, seed=seed + b, piece_T=0.6, jitter=0.8, margin=3.0)
        c = np.asarray(cf).reshape(N, 6, 3)
        end = sum(c[N - 1, k] * t[N - 1] ** k for k in range(6))
        H.append(np.concatenate([c[0, 0], np.zeros(6)])); Tl.append(np.concatenate([end, np.zeros(6)]))
        Q.append(c[1:, 0].copy()); T.append(t); Cc.append(synth.colmajor(cf))
    return np.stack(H), np.stack(Tl), np.stack(Q), np.stack(T), np.stack(Cc)


def stats(x):
    x = np.asarray(x, dtype=np.float64)
    return {"median": float(np.median(x)), "min": float(x.min()), "max": float(x.max())}


def factors(piece, limit, headroom, f_max):
    """The factor rule of include/isdf_accel.h on B x N x 12 piece rows (numpy): (f B x N, any piece over B)."""
    v = piece[:, :, 0::2]
    lim = np.asarray(limit)[None, None, :]
    with np.errstate(all="ignore"):
        over = np.where(np.arange(6)[None, None, :] == 5, v < lim, v > lim) & ~np.isnan(lim)
        rho = v / lim
        rho[:, :, 1] = np.sqrt(rho[:, :, 1])
        rho[:, :, 5] = np.where(v[:, :, 5] > 0.0, lim[:, :, 5] / v[:, :, 5], f_max)
    rho = np.where(over, rho, 0.0)
    bad = (over & ~np.isfinite(rho)).any(axis=2)
    f = np.clip((1.0 + headroom) * rho.max(axis=2), 1.0, f_max)
    f = np.where(bad, f_max, f)
    f = np.where(over.any(axis=2), f, 1.0)
    return f, over.any(axis=(1, 2))


def composed(pkg, eng, cfg, H, Tl, Q, T, R=8, headroom=0.02, f_max=2.0):
    """The loop out of the parts a caller had before: host solve + isdf_traj_limits_batch per round, factor rule and update on the host."""
    B, N = T.shape
    limit = [cfg.vmax, np.nan, cfg.omgmax, cfg.thetamax, np.nan, np.nan]
    cur = T.copy()
    done = np.zeros(B, dtype=bool)
    rounds = np.zeros(B, dtype=int)
    for k in range(R + 1):
        Cc = np.stack([pkg.traj_minco_host(H[b], Tl[b], Q[b], cur[b]) for b in range(B)])
        reps = eng.traj_limits_batch(cur, Cc)
        f, over = factors(np.stack([r["piece_out"] for r in reps]), limit, headroom, f_max)
        newly = ~done & ~over
        rounds[newly] = k
        done |= ~over
        if done.all() or k == R:
            rounds[~done] = R
            break
        cur = np.where(done[:, None], cur, cur * f)
    return cur, rounds


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
    for label, B, N in (("one trajectory, N = 40", 1, 40), ("one trajectory, N = 400", 1, 400), ("batch of 16, N = 40", 16, 40)):
        H, Tl, Q, T, Cc = problems(synth, B, N, seed=100 + N)
        for _ in range(a.warmup):
            res = eng.traj_realloc_batch(H, Tl, Q, T)
        dev, call = [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            res = eng.traj_realloc_batch(H, Tl, Q, T)
            call.append((time.perf_counter() - t0) * 1e3)
            dev.append(res[0]["device_ms"])
        comp = []
        for it in range(2 + a.composed_repeats):
            t0 = time.perf_counter()
            cT, cR = composed(pkg, eng, cfg, H, Tl, Q, T)
            if it >= 2:
                comp.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        for _ in range(a.host_repeats):
            host = [pkg.traj_realloc_host(cfg, H[b], Tl[b], Q[b], T[b]) for b in range(B)]
        host_ms = (time.perf_counter() - t0) * 1e3 / a.host_repeats
        uni = eng.traj_retime_batch(T, Cc)
        rows.append({"case": label, "B": B, "N": N, "rounds_param": 8, "launches": 4 * 9, "device_ms": stats(dev), "call_ms": stats(call),
                     "composed_ms": stats(comp), "host_form_one_thread_ms": host_ms,
                     "status": [int(r["status"]) for r in res], "rounds": [int(r["rounds"]) for r in res],
                     "pieces_changed": [int(r["pieces_changed"]) for r in res], "max_factor": [float(r["max_factor"]) for r in res],
                     "duration_in": [float(r["duration_in"]) for r in res], "duration_out": [float(r["duration_out"]) for r in res],
                     "uniform_status": [int(u["status"]) for u in uni], "uniform_scale": [float(u["scale"]) for u in uni],
                     "uniform_duration_out": [float(u["duration_out"]) for u in uni],
                     "composed_rounds": [int(x) for x in cR],
                     "composed_vs_device_T_rel": float(np.max(np.abs(cT - np.stack([r["T"] for r in res])) / cT)),
                     "host_vs_device_T_rel": float(max(np.max(np.abs(host[b]["T"] - res[b]["T"]) / host[b]["T"]) for b in range(B))),
                     "host_status": [int(h["status"]) for h in host], "host_rounds": [int(h["rounds"]) for h in host]})
        q = rows[-1]
        print(f"{label:<24} device {q['device_ms']['median']:.3f} ms [{q['device_ms']['min']:.3f}, {q['device_ms']['max']:.3f}]  "
              f"call {q['call_ms']['median']:.3f} ms [{q['call_ms']['min']:.3f}, {q['call_ms']['max']:.3f}]  composed {q['composed_ms']['median']:.3f} ms "
              f"[{q['composed_ms']['min']:.3f}, {q['composed_ms']['max']:.3f}]  host form {host_ms:.1f} ms  status {q['status']} rounds {q['rounds']}  "
              f"duration {np.sum(q['duration_in']):.2f} -> {np.sum(q['duration_out']):.2f} s, uniform {np.sum(q['uniform_duration_out']):.2f} s "
              f"(status {q['uniform_status']})", flush=True)
    eng.close()
    out = {"tool": "tools/traj_realloc_bench.py", "repeats": a.repeats, "warmup": a.warmup, "composed_repeats": a.composed_repeats,
           "device": torch.cuda.get_device_name(0), "rows": rows}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
