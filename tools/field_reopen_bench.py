#!/usr/bin/env python
"""Developer tool: the cost-to-go field lowered in place by the map clear (isdf_frontend_field_set_reopen mode 1) against what mode 0
makes a caller do - the clear, which drops the field, followed by isdf_frontend_field_build - in the same run, on the 256 x 256 x 64 map
at 0.2 m of tools/map_update_bench.py (box robot, k = 21, 11 x 11 attitudes) towards the goal of pair 1 of tools/frontend_field_bench.py:
the map, robot and goal of tools/field_repair_bench.py.

Frames as in tools/field_repair_bench.py - about a quarter of the voxels of a cube of 8^3 or 16^3 voxels, at disjoint places, 3 frames of
warm-up and 9 timed per series, three series per size by the distance of the frames from the goal (the cubes whose centre's d on the base
map is nearest to 10 %, 50 % and 90 % of the field's largest finite d) - played BACKWARDS as in tools/map_clear_bench.py: the ctx starts
on the base cloud plus every frame of the series, and the frames are taken out one by one.  Per series and mode: median [min, max] of the
whole call's wall time (it ends in a stream synchronisation); for mode 1 the reopen's rounds, brick visits, opened voxels and device
time; for mode 0 the rebuild's.  After every mode-1 series the field's bytes are compared with a fresh ctx's build on the base cloud,
whose rounds, brick visits and device time are recorded next to the reopen's.  Writes one JSON record.

    python tools/field_reopen_bench.py --out profiles/field_reopen_bench.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_reopen_bench.json"))
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--warmup", type=int, default=3)
args = ap.parse_args()
import torch  # noqa: E402,F401  (torch first: see tests/conftest.py)
if torch.cuda.is_available():
    torch.zeros(1, device="cuda")
pkg = graft.load_package(); capi, synth = pkg.capi, pkg.synth
res, dims = 0.2, (256, 256, 64)
bmin, bmax = np.zeros(3), np.array(dims) * res
occ = synth.random_box_map(dims, res=res, occupancy=0.12, seed=12345)
base = ((np.argwhere(occ == 1) + 0.5) * res).astype(np.float32)          # one point per occupied voxel, sta_threshold 1
fe = capi.frontend_config(kernel_size=21, max_roll=45.0, max_pitch=45.0, ang_res=9.0, safeh=0.0)
stat = lambda v: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}      # noqa: E731
n_frames = args.warmup + args.repeats


def build(cloud, mode):
    eng = pkg.Engine(synth.default_config(capi.V1_SWEPT))
    eng.set_pointcloud(cloud, res, 1, bmin, bmax)
    eng.generate_esdf()
    eng.set_shape(synth.bench_box_shape()); eng.frontend_build(fe)
    eng.frontend_cspace(download=False)
    eng.frontend_field_set_reopen(mode)
    return eng


# the goal of pair 1 (tools/astar_bench.py's pairs: drawn from the free cells with seed 0, the first pair dropped)
eng = build(base, 0)
good = np.argwhere((eng.frontend_cspace_table() != 0).any(axis=-1))
rng = np.random.default_rng(0)
pairs = []
while len(pairs) < 2:
    p, q = good[rng.choice(len(good), 2, replace=False)]
    if np.abs(p - q).max() >= 150:
        pairs.append(((p + 0.5) * res, (q + 0.5) * res))
goal = pairs[1][1]
goal_cell = np.floor(goal / res).astype(int)
binfo = eng.frontend_field_build(goal)
d0 = eng.frontend_field()
eng.close()
d_max = float(d0[np.isfinite(d0)].max())
print(f"goal {goal.tolist()}: build {binfo.rounds} rounds, {binfo.brick_visits} brick visits, {binfo.reached_voxels} reached, largest d {d_max:.1f} cells", flush=True)


def places(s, share):
    """lower corners of n_frames disjoint cubes of s^3 voxels on a lattice of stride 24, their centres' d on the base map nearest to share * d_max"""
    lat = np.array([(x, y, z) for x in range(4, dims[0] - s, 24) for y in range(4, dims[1] - s, 24) for z in range(0, dims[2] - s + 1, 24)])
    dc = d0[tuple((lat + s // 2).T)]
    gap = np.maximum(np.maximum(lat - goal_cell, goal_cell - (lat + s - 1)), 0).max(axis=1)      # voxels between the cube and the goal cell
    keep = np.isfinite(dc) & (gap > 12)                   # (a voxel within (k - 1) / 2 = 10 of the goal cell could close the goal itself)
    lat, dc = lat[keep], dc[keep]
    order = np.argsort(np.abs(dc - share * d_max), kind="stable")[:n_frames]
    return lat[order], dc[order]


def frames(s, los, rng):
    out = []
    for lo in los:
        cells = np.argwhere(rng.random((s, s, s)) < 0.25)
        cells = np.unique(np.concatenate([cells, [[0, 0, 0], [s - 1, s - 1, s - 1]]]), axis=0) + lo
        out.append(((cells + 0.5) * res).astype(np.float32))
    return out


record = {"tool": "tools/field_reopen_bench.py", "device": torch.cuda.get_device_name(0), "map": list(dims), "resolution": res, "robot": "box 3.2 x 0.6 x 0.6 m",
          "kernel_size": 21, "attitudes": 121, "goal": goal.tolist(), "largest_d_cells": d_max, "repeats": args.repeats, "warmup": args.warmup,
          "build_on_base": {"rounds": int(binfo.rounds), "brick_visits": int(binfo.brick_visits), "bricks": int(binfo.bricks), "reached_voxels": int(binfo.reached_voxels),
                            "device_ms": float(binfo.device_ms)}, "series": []}
frng = np.random.default_rng(1)
for s in (8, 16):
    for name, share in (("near", 0.1), ("middle", 0.5), ("far", 0.9)):
        los, dcs = places(s, share)
        fr = frames(s, los, frng)
        start = np.concatenate([base] + fr)
        row = {"box": s, "distance": name, "centre_d_over_largest": stat(dcs / d_max)}
        # mode 1: the clear lowers the field in place
        eng = build(start, 1)
        first = eng.frontend_field_build(goal)
        assert first.reachable == 1 and first.status == 0
        wall, rows = [], []
        for f in fr[::-1]:
            t0 = time.perf_counter(); info = eng.clear_pointcloud(f); wall.append((time.perf_counter() - t0) * 1e3)
            assert info.path == 1 and info.field_dropped == 0, (info.path, info.field_dropped)
            r = eng.frontend_field_reopen_info()
            assert r.reachable == 1 and r.status == 0
            rows.append((r.device_ms, r.rounds, r.brick_visits, r.seeded_bricks, r.opened_voxels, r.reached_voxels - r.reached_before, info.n_cleared_voxels,
                         info.count_ms + info.esdf_ms + info.frontend_ms))
        rows = np.array(rows)[args.warmup:]
        got = eng.frontend_field()
        eng.close()
        fresh = build(base, 0)
        finfo = fresh.frontend_field_build(goal)
        same = bool(np.array_equal(got.view(np.uint64), fresh.frontend_field().view(np.uint64)))
        fresh.close()
        assert same, "the reopened field differs from a fresh build on the base cloud"
        row.update({"reopen_call_ms": stat(wall[args.warmup:]), "reopen_device_ms": stat(rows[:, 0]), "rounds": stat(rows[:, 1]), "brick_visits": stat(rows[:, 2]),
                    "seeded_bricks": stat(rows[:, 3]), "opened_voxels": stat(rows[:, 4]), "newly_reached_voxels": stat(rows[:, 5]), "cleared_voxels": stat(rows[:, 6]),
                    "clear_device_ms_without_field": stat(rows[:, 7]), "equal_to_fresh_build": same,
                    "fresh_build": {"rounds": int(finfo.rounds), "brick_visits": int(finfo.brick_visits), "device_ms": float(finfo.device_ms)}})
        # mode 0: the clear drops the field, the caller builds it again (the behaviour without this mode)
        eng = build(start, 0)
        eng.frontend_field_build(goal)
        wall, clr, bld = [], [], []
        for f in fr[::-1]:
            t0 = time.perf_counter(); info = eng.clear_pointcloud(f); t1 = time.perf_counter(); b = eng.frontend_field_build(goal); t2 = time.perf_counter()
            assert info.path == 1 and info.field_dropped == 1
            wall.append((t2 - t0) * 1e3); clr.append((t1 - t0) * 1e3); bld.append((b.device_ms, b.rounds, b.brick_visits))
        eng.close()
        bld = np.array(bld)[args.warmup:]
        row.update({"drop_and_build_call_ms": stat(wall[args.warmup:]), "drop_clear_call_ms": stat(clr[args.warmup:]), "rebuild_device_ms": stat(bld[:, 0]),
                    "rebuild_rounds": stat(bld[:, 1]), "rebuild_brick_visits": stat(bld[:, 2])})
        row["reopen_over_drop_and_build"] = row["reopen_call_ms"]["median"] / row["drop_and_build_call_ms"]["median"]
        record["series"].append(row)
        print(json.dumps(row), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
json.dump(record, open(args.out, "w"), indent=1)
print("wrote", args.out)
