#!/usr/bin/env python
"""Developer tool: the cost-to-go field carried through a shift of the map window (isdf_frontend_field_set_shift mode 1) against what
mode 0 makes a caller do - the shift, which drops the field, followed by isdf_frontend_field_build - on the 256 x 256 x 64 map at 0.2 m
of tools/map_shift_bench.py (box robot, k = 21, 11 x 11 attitudes, the box ending a quarter voxel early) towards the goal of pair 1 of
tools/frontend_field_bench.py.

The shifts of tools/map_shift_bench.py's table, each timed and then undone untimed, 2 calls of warm-up and 7 timed per series; then a
series of isdf_map_follow steps of a robot that flies from the middle of the window towards the goal in the plane, 4 voxels a step on
x and y.  Per series and mode: median [min, max] of the whole call's wall time (mode 0: the shift plus the build), and for mode 1 the
carry's counters and device time.  After every mode-1 series the field's bytes are compared with a fresh ctx's build on the counts the
ctx holds, in its box.  Writes one JSON record.

    python tools/field_shift_bench.py --out profiles/field_shift_bench.json
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_shift_bench.json"))
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--follow_steps", type=int, default=12)
args = ap.parse_args()
import torch  # noqa: E402,F401  (torch first: see tests/conftest.py)
if torch.cuda.is_available():
    torch.zeros(1, device="cuda")
pkg = graft.load_package(); capi, synth = pkg.capi, pkg.synth
res, dims = 0.2, (256, 256, 64)
D = np.array(dims)
bmin, bmax = np.zeros(3), (D - 0.25) * res
occ = synth.random_box_map(dims, res=res, occupancy=0.12, seed=12345)
fe = capi.frontend_config(kernel_size=21, max_roll=45.0, max_pitch=45.0, ang_res=9.0, safeh=0.0)
SHIFTS = [(1, 0, 0), (4, 0, 0), (16, 0, 0), (4, 4, 0), (0, 0, 4)]
stat = lambda v: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}      # noqa: E731


def build(cloud, lo, hi, mode):
    eng = pkg.Engine(synth.default_config(capi.V1_SWEPT))
    assert eng.set_pointcloud(cloud, res, 1, lo, hi) == dims
    eng.generate_esdf()
    eng.set_shape(synth.bench_box_shape()); eng.frontend_build(fe)
    eng.frontend_cspace(download=False)
    eng.frontend_field_set_shift(mode)
    return eng


def fresh_field(eng, goal):
    """a fresh ctx on the counts `eng` holds, in its box: the field towards `goal`"""
    counts = eng.map_counts()
    _, lo, hi = eng.get_grid(capi.GRID_OCCUPANCY)
    cells = np.argwhere(counts > 0)
    cloud = ((np.repeat(cells, counts[tuple(cells.T)].astype(np.int64), axis=0) + 0.5) * res + lo).astype(np.float32)
    fresh = build(cloud, lo, hi, 0)
    assert np.array_equal(fresh.map_counts(), counts)
    info = fresh.frontend_field_build(goal)
    d = fresh.frontend_field()
    fresh.close()
    return d, info


base = ((np.argwhere(occ == 1) + 0.5) * res + bmin).astype(np.float32)          # one point per occupied voxel, sta_threshold 1
# the goal of pair 1 (tools/astar_bench.py's pairs: drawn from the free cells with seed 0, the first pair dropped)
eng = build(base, bmin, bmax, 0)
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
eng.close()
print(f"goal {goal.tolist()} (cell {goal_cell.tolist()}): build {binfo.rounds} rounds, {binfo.brick_visits} brick visits, {binfo.device_ms:.2f} ms", flush=True)
record = {"tool": "tools/field_shift_bench.py", "device": torch.cuda.get_device_name(0), "map": list(dims), "resolution": res, "bmax": "bmin + (dims - 0.25) * resolution",
          "robot": "box 3.2 x 0.6 x 0.6 m", "kernel_size": 21, "attitudes": 121, "goal": goal.tolist(), "goal_cell": goal_cell.tolist(), "repeats": args.repeats,
          "warmup": args.warmup, "build": {"rounds": int(binfo.rounds), "brick_visits": int(binfo.brick_visits), "device_ms": float(binfo.device_ms)}, "shift": [], "follow": None}


def carry_row(si):
    return (si.device_ms, si.left_reached, si.reset_voxels, si.opened_voxels, si.rounds_close, si.rounds_open, si.brick_visits, si.seeded_bricks_close, si.seeded_bricks_open)


CARRY = ("carry_device_ms", "left_reached", "reset_voxels", "opened_voxels", "rounds_close", "rounds_open", "brick_visits", "seeded_bricks_close", "seeded_bricks_open")

for s in SHIFTS:
    back = tuple(-v for v in s)
    assert all(0 <= goal_cell[a] - s[a] < dims[a] for a in range(3)), "the goal leaves the window"
    row = {"shift": list(s)}
    # mode 1: the shift carries the field
    eng = build(base, bmin, bmax, 1)
    eng.frontend_field_build(goal)
    wall, rows = [], []
    for i in range(args.warmup + args.repeats):
        if i:
            assert eng.shift_map(back).field_dropped == 0          # untimed
        t0 = time.perf_counter(); info = eng.shift_map(s); wall.append((time.perf_counter() - t0) * 1e3)
        assert info.field_dropped == 0
        rows.append(carry_row(eng.frontend_field_shift_info()) + (info.path,))
    rows = np.array(rows, dtype=np.float64)[args.warmup:]
    want, finfo = fresh_field(eng, goal)
    same = bool(np.array_equal(eng.frontend_field().view(np.uint64), want.view(np.uint64)))
    eng.close()
    assert same, "the carried field differs from a fresh build"
    row.update({"carry_call_ms": stat(wall[args.warmup:]), "paths": sorted(set(int(v) for v in rows[:, -1])), "equal_to_fresh_build": same,
                "fresh_build": {"rounds": int(finfo.rounds), "brick_visits": int(finfo.brick_visits), "device_ms": float(finfo.device_ms)}})
    row.update({k: stat(rows[:, j]) for j, k in enumerate(CARRY)})
    # mode 0: the shift drops the field, the caller builds it again
    eng = build(base, bmin, bmax, 0)
    eng.frontend_field_build(goal)
    wall, shf, bld = [], [], []
    for i in range(args.warmup + args.repeats):
        if i:
            eng.shift_map(back); eng.frontend_field_build(goal)   # untimed
        t0 = time.perf_counter(); info = eng.shift_map(s); t1 = time.perf_counter(); b = eng.frontend_field_build(goal); t2 = time.perf_counter()
        assert info.field_dropped == 1
        wall.append((t2 - t0) * 1e3); shf.append((t1 - t0) * 1e3); bld.append((b.device_ms, b.rounds, b.brick_visits))
    eng.close()
    bld = np.array(bld)[args.warmup:]
    row.update({"drop_and_build_call_ms": stat(wall[args.warmup:]), "drop_shift_call_ms": stat(shf[args.warmup:]), "rebuild_device_ms": stat(bld[:, 0]),
                "rebuild_rounds": stat(bld[:, 1]), "rebuild_brick_visits": stat(bld[:, 2])})
    record["shift"].append(row)
    print(json.dumps(row), flush=True)

# the follow series: the robot starts in the middle of the window and flies towards the goal in the plane
step = np.array([4 * np.sign(goal_cell[0] - D[0] // 2), 4 * np.sign(goal_cell[1] - D[1] // 2), 0])
n_steps = int(min(args.follow_steps, (np.abs(goal_cell[:2] - D[:2] // 2) // 4).min()))
centres = [(D // 2 + (k + 1) * step + 0.5) * res + bmin for k in range(n_steps)]
row = {"step": step.tolist(), "steps": n_steps, "min_shift": 4}
eng = build(base, bmin, bmax, 1)
eng.frontend_field_build(goal)
wall, rows = [], []
for c in centres:
    t0 = time.perf_counter(); s, info = eng.map_follow(c, 4); wall.append((time.perf_counter() - t0) * 1e3)
    assert s == tuple(step) and info.field_dropped == 0, (s, info.field_dropped)
    rows.append(carry_row(eng.frontend_field_shift_info()) + (info.path,))
rows = np.array(rows, dtype=np.float64)
want, finfo = fresh_field(eng, goal)
same = bool(np.array_equal(eng.frontend_field().view(np.uint64), want.view(np.uint64)))
eng.close()
assert same, "the carried field differs from a fresh build after the follow series"
row.update({"carry_call_ms": stat(wall[args.warmup:]), "paths": sorted(set(int(v) for v in rows[:, -1])), "equal_to_fresh_build": same,
            "fresh_build": {"rounds": int(finfo.rounds), "brick_visits": int(finfo.brick_visits), "device_ms": float(finfo.device_ms)}})
row.update({k: stat(rows[args.warmup:, j]) for j, k in enumerate(CARRY)})
eng = build(base, bmin, bmax, 0)
eng.frontend_field_build(goal)
wall = []
for c in centres:
    t0 = time.perf_counter(); s, info = eng.map_follow(c, 4); eng.frontend_field_build(goal); wall.append((time.perf_counter() - t0) * 1e3)
    assert info.field_dropped == 1
eng.close()
row["drop_and_build_call_ms"] = stat(wall[args.warmup:])
record["follow"] = row
print(json.dumps(row), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
json.dump(record, open(args.out, "w"), indent=1)
print("wrote", args.out)
