#!/usr/bin/env python
"""Developer tool: the cost-to-go field repaired by the map update (isdf_frontend_field_set_repair mode 1) against what mode 0 makes a
caller do - the update, which drops the field, followed by isdf_frontend_field_build - on the 256 x 256 x 64 map at 0.2 m of
tools/map_update_bench.py (box robot, k = 21, 11 x 11 attitudes) towards the goal of pair 1 of tools/frontend_field_bench.py.

Frames as in tools/map_update_bench.py: about a quarter of the voxels of a cube of 8^3 or 16^3 voxels, at disjoint places, 3 frames of
warm-up and 9 timed per series.  Three series per size by the distance of the frames from the goal: the cubes whose centre's OLD d is
nearest to 10 % (near), 50 % (middle) and 90 % (far) of the field's largest finite d.  Per series and mode: median [min, max] of the
whole call's wall time (it ends in a stream synchronisation), and for mode 1 the repair's share reset_voxels / reached_voxels, its
rounds, brick visits and device time.  After every mode-1 series the field's bytes are compared with a fresh ctx's build on the union
cloud, whose rounds, brick visits and device time are recorded next to the repair's.  Writes one JSON record.

    python tools/field_repair_bench.py --out profiles/field_repair_bench.json
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_repair_bench.json"))
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
    eng.frontend_field_set_repair(mode)
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
    """lower corners of n_frames disjoint cubes of s^3 voxels on a lattice of stride 24, their centres' old d nearest to share * d_max"""
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


record = {"tool": "tools/field_repair_bench.py", "device": torch.cuda.get_device_name(0), "map": list(dims), "resolution": res, "robot": "box 3.2 x 0.6 x 0.6 m",
          "kernel_size": 21, "attitudes": 121, "goal": goal.tolist(), "largest_d_cells": d_max, "repeats": args.repeats, "warmup": args.warmup,
          "build": {"rounds": int(binfo.rounds), "brick_visits": int(binfo.brick_visits), "bricks": int(binfo.bricks), "reached_voxels": int(binfo.reached_voxels),
                    "device_ms": float(binfo.device_ms)}, "series": []}
frng = np.random.default_rng(1)
for s in (8, 16):
    for name, share in (("near", 0.1), ("middle", 0.5), ("far", 0.9)):
        los, dcs = places(s, share)
        fr = frames(s, los, frng)
        row = {"box": s, "distance": name, "centre_d_over_largest": stat(dcs / d_max)}
        # mode 1: the update repairs
        eng = build(base, 1)
        reached = eng.frontend_field_build(goal).reached_voxels
        wall, rows = [], []
        for f in fr:
            t0 = time.perf_counter(); info = eng.update_pointcloud(f); wall.append((time.perf_counter() - t0) * 1e3)
            assert info.path == 1 and info.field_dropped == 0, (info.path, info.field_dropped)
            r = eng.frontend_field_repair_info()
            rows.append((r.device_ms, r.reset_voxels / max(reached, 1), r.rounds, r.brick_visits, r.seeded_bricks, r.closed_voxels, info.n_new_voxels,
                         info.count_ms + info.esdf_ms + info.frontend_ms))
            assert r.reachable == 1
            reached = r.reached_voxels
        rows = np.array(rows)[args.warmup:]
        got = eng.frontend_field()
        eng.close()
        fresh = build(np.concatenate([base] + fr), 0)
        finfo = fresh.frontend_field_build(goal)
        same = bool(np.array_equal(got.view(np.uint64), fresh.frontend_field().view(np.uint64)))
        fresh.close()
        assert same, "the repaired field differs from a fresh build on the union"
        row.update({"repair_call_ms": stat(wall[args.warmup:]), "repair_device_ms": stat(rows[:, 0]), "reset_over_reached": stat(rows[:, 1]), "rounds": stat(rows[:, 2]),
                    "brick_visits": stat(rows[:, 3]), "seeded_bricks": stat(rows[:, 4]), "closed_voxels": stat(rows[:, 5]), "new_voxels": stat(rows[:, 6]),
                    "update_device_ms_without_field": stat(rows[:, 7]), "equal_to_fresh_build": same,
                    "fresh_build": {"rounds": int(finfo.rounds), "brick_visits": int(finfo.brick_visits), "device_ms": float(finfo.device_ms)}})
        # mode 0: the update drops the field, the caller builds it again
        eng = build(base, 0)
        eng.frontend_field_build(goal)
        wall, upd, bld = [], [], []
        for f in fr:
            t0 = time.perf_counter(); info = eng.update_pointcloud(f); t1 = time.perf_counter(); b = eng.frontend_field_build(goal); t2 = time.perf_counter()
            assert info.path == 1 and info.field_dropped == 1
            wall.append((t2 - t0) * 1e3); upd.append((t1 - t0) * 1e3); bld.append((b.device_ms, b.rounds, b.brick_visits))
        eng.close()
        bld = np.array(bld)[args.warmup:]
        row.update({"drop_and_build_call_ms": stat(wall[args.warmup:]), "drop_update_call_ms": stat(upd[args.warmup:]), "rebuild_device_ms": stat(bld[:, 0]),
                    "rebuild_rounds": stat(bld[:, 1]), "rebuild_brick_visits": stat(bld[:, 2])})
        record["series"].append(row)
        print(json.dumps(row), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
json.dump(record, open(args.out, "w"), indent=1)
print("wrote", args.out)
