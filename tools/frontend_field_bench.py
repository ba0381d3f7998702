#!/usr/bin/env python
"""Times the cost-to-go field of the front end (isdf_frontend_field_*) against the existing A* (isdf_frontend_astar_search) on the
map of profiles/r6_astar_bench.txt: 256 x 256 x 64 at 0.2 m, 12 % occupied, the box robot, k = 21, 11 x 11 attitudes, and that record's
start/goal pairs 1..7 (pair 0 carries the table's transfer there).

  field build   isdf_frontend_field_info.device_ms (events around the launches of one build) and a host clock around the whole call,
                `--warmup` + `--repeats` calls towards the goal of pair 1, a short window (`--short`) towards the other goals;
  field paths   a host clock around isdf_frontend_field_paths for 1 and for 128 starts (free cells drawn with a fixed seed), cap 1024;
  A*            isdf_astar_result.search_ms per pair, the configuration-space table already on the host (`--astar-repeats` calls each):
                the baseline is the existing code on the same commit and machine;
  host form     isdf_frontend_field_host once on the same table: its time, and that the device field has the same bytes at this size.

The break-even count is the smallest number of starts S for which one field build plus one paths call costs less than S searches at
the mean of the pairs' medians.

    python tools/frontend_field_bench.py --out profiles/frontend_field_bench.json
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402


def stats(x):
    x = np.asarray(x, dtype=np.float64)
    return {"median": float(np.median(x)), "min": float(x.min()), "max": float(x.max())}


def fmt(s):
    return f"{s['median']:.3f} [{s['min']:.3f}, {s['max']:.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--short", type=int, default=20)
    ap.add_argument("--astar-repeats", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch  # noqa: F401  (torch first: see tests/conftest.py)
    if torch.cuda.is_available():
        torch.zeros(1, device="cuda")
    pkg = g.load_package()
    capi, synth = pkg.capi, pkg.synth
    res, dims, k = 0.2, (256, 256, 64), 21
    occ = synth.random_box_map(dims, res=res, occupancy=0.12, seed=12345)
    eng = pkg.Engine(synth.default_config(capi.V1_SWEPT))
    eng.set_grid(occ, (0, 0, 0), res, capi.GRID_OCCUPANCY)
    eng.set_shape(synth.bench_box_shape())
    eng.frontend_build(capi.frontend_config(kernel_size=k, max_roll=45.0, max_pitch=45.0, ang_res=9.0, safeh=0.0))
    table, cspace_ms = eng.frontend_cspace()
    fits = (table != 0).any(axis=-1)
    good = np.argwhere(fits)
    rng = np.random.default_rng(0)                       # tools/astar_bench.py's pairs
    pairs = []
    while len(pairs) < 8:
        p, q = good[rng.choice(len(good), 2, replace=False)]
        if np.abs(p - q).max() >= 150:
            pairs.append(((p + 0.5) * res, (q + 0.5) * res))
    pairs = pairs[1:]
    print(f"map {dims} at {res} m, {occ.mean():.3f} occupied, free {fits.mean():.3f}; configuration-space kernel {cspace_ms:.2f} ms", flush=True)

    builds = []
    for q, (s, goal) in enumerate(pairs):
        warm, reps = (a.warmup, a.repeats) if q == 0 else (3, a.short)
        for _ in range(warm):
            info = eng.frontend_field_build(goal)
        dev, call = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            info = eng.frontend_field_build(goal)
            call.append((time.perf_counter() - t0) * 1e3)
            dev.append(info.device_ms)
        d_start = float(eng.frontend_field([s])[0])
        builds.append({"pair": q + 1, "calls": reps, "device_ms": stats(dev), "call_ms": stats(call), "rounds": int(info.rounds), "bricks": int(info.bricks),
                       "brick_visits": int(info.brick_visits), "free_voxels": int(info.free_voxels), "reached_voxels": int(info.reached_voxels),
                       "status": int(info.status), "d_start_cells": d_start})
        print(f"field build, goal of pair {q + 1}: device {fmt(builds[-1]['device_ms'])} ms, call {fmt(builds[-1]['call_ms'])} ms, {info.rounds} rounds, "
              f"{info.brick_visits} brick visits over {info.bricks} bricks, d[start] {d_start:.3f} cells", flush=True)

    # the field of the last goal is in place: the host form on the same table, and the bytes at this size
    goal_cell = np.floor(pairs[-1][1] / res).astype(int)
    t0 = time.perf_counter()
    host, _ = pkg.frontend_field_host(table, goal_cell, 121)
    host_ms = (time.perf_counter() - t0) * 1e3
    same = bool(np.array_equal(host.view(np.uint64), eng.frontend_field().view(np.uint64)))
    print(f"host form (one thread) {host_ms:.0f} ms; device field has the same bytes: {same}", flush=True)

    # paths off the field of pair 1's goal
    eng.frontend_field_build(pairs[0][1])
    srng = np.random.default_rng(1)
    starts = (good[srng.choice(len(good), 128, replace=False)] + 0.5) * res
    starts[0] = pairs[0][0]
    cap = 1024
    paths = []
    for B in (1, 128):
        for _ in range(a.warmup):
            n, xyz, rp = eng.frontend_field_paths(starts[:B], cap)
        call = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            n, xyz, rp = eng.frontend_field_paths(starts[:B], cap)
            call.append((time.perf_counter() - t0) * 1e3)
        paths.append({"starts": B, "cap": cap, "call_ms": stats(call), "nodes_mean": float(n[n > 0].mean()) if (n > 0).any() else 0.0, "nodes_max": int(n.max()),
                      "no_path": int((n == 0).sum())})
        print(f"field paths, {B:3d} starts: call {fmt(paths[-1]['call_ms'])} ms, {paths[-1]['nodes_mean']:.0f} nodes on average, {paths[-1]['no_path']} without a path", flush=True)

    astar = []
    eng.frontend_astar(*pairs[0])                        # brings the table to the host once
    for q, (s, goal) in enumerate(pairs):
        ms = []
        for _ in range(2 + a.astar_repeats):
            xyz, rp, rot, r = eng.frontend_astar(s, goal)
            ms.append(r.search_ms)
        ms = ms[2:]
        steps = np.rint(np.diff(xyz, axis=0) / res).astype(int) if r.success else np.zeros((0, 3), dtype=int)
        cost = float(sum(math.sqrt(float((st * st).sum())) for st in steps))
        astar.append({"pair": q + 1, "calls": len(ms), "search_ms": stats(ms), "success": int(r.success), "n_path": int(r.n_path), "expansions": int(r.expansions),
                      "path_cost_cells": cost, "d_start_cells": builds[q]["d_start_cells"]})
        print(f"A*, pair {q + 1}: search {fmt(astar[-1]['search_ms'])} ms, {r.n_path} nodes, {r.expansions} expansions, cost {cost:.3f} cells "
              f"(field: {builds[q]['d_start_cells']:.3f})", flush=True)

    build_ms = float(np.mean([b["call_ms"]["median"] for b in builds]))
    astar_ms = float(np.mean([x["search_ms"]["median"] for x in astar]))
    p1, p128 = paths[0]["call_ms"]["median"], paths[1]["call_ms"]["median"]
    per_start = max(p128 - p1, 0.0) / 127.0
    S = 1
    while build_ms + p1 + per_start * (S - 1) >= S * astar_ms and S < 100000:
        S += 1
    summary = {"field_build_call_ms_mean_of_medians": build_ms, "astar_search_ms_mean_of_medians": astar_ms, "break_even_starts": S,
               "field_plus_128_paths_ms": build_ms + p128, "astar_128_searches_ms": 128 * astar_ms}
    print(f"one build {build_ms:.2f} ms (mean of the goals' medians) against one search {astar_ms:.2f} ms (mean of the pairs' medians): the field "
          f"pays from {S} starts per goal; 128 starts: {build_ms + p128:.1f} ms against {128 * astar_ms:.0f} ms", flush=True)
    eng.close()
    out = {"tool": "tools/frontend_field_bench.py", "repeats": a.repeats, "warmup": a.warmup, "short": a.short, "astar_repeats": a.astar_repeats,
           "device": torch.cuda.get_device_name(0), "map": {"dims": list(dims), "res": res, "occupied": float(occ.mean()), "free": float(fits.mean()),
                                                             "kernel_size": k, "attitudes": 121, "cspace_kernel_ms": cspace_ms},
           "field_build": builds, "host_form_ms": host_ms, "device_equals_host_form": same, "field_paths": paths, "astar": astar, "summary": summary}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
