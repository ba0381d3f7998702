#!/usr/bin/env python
"""Developer tool: voxels cleared in place (isdf_clear_pointcloud) against the from-scratch sequence on the remaining cloud, on the
256 x 256 x 64 map at 0.2 m of tools/map_update_bench.py (box robot, k = 21, 11 x 11 attitudes).  The frames of that tool played
backwards: the ctx starts on the base cloud plus every frame, and the frames (about 8^3, 16^3, 32^3 voxels each, at disjoint places)
are taken out one by one, with and without a valid host table.  Median [min, max] of the call's wall time and of its device times
after warm-up frames; then the products are compared byte for byte with a fresh build on what is left - the configuration space and
the A*'s host copy as the clear left them - and the from-scratch sequence is timed on that same cloud.  No path is forced: the paths
taken are counted.  Writes one JSON record (default profiles/map_clear_bench.json)."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as graft

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "map_clear_bench.json"))
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--warmup", type=int, default=3)
args = ap.parse_args()
pkg = graft.load_package(); capi, synth = pkg.capi, pkg.synth
res, dims = 0.2, (256, 256, 64)
bmin, bmax = np.zeros(3), np.array(dims) * res
occ = synth.random_box_map(dims, res=res, occupancy=0.12, seed=12345)
base = ((np.argwhere(occ == 1) + 0.5) * res).astype(np.float32)          # one point per occupied voxel, sta_threshold 1
fe = capi.frontend_config(kernel_size=21, max_roll=45.0, max_pitch=45.0, ang_res=9.0, safeh=0.0)
stat = lambda v: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}      # noqa: E731


def build(cloud, host_table):
    eng = pkg.Engine(synth.default_config(capi.V1_SWEPT))
    t = [time.perf_counter()]
    eng.set_pointcloud(cloud, res, 1, bmin, bmax); t.append(time.perf_counter())
    eng.generate_esdf(); t.append(time.perf_counter())
    eng.set_shape(synth.bench_box_shape()); eng.frontend_build(fe); t.append(time.perf_counter())
    eng.frontend_cspace(download=False); t.append(time.perf_counter())
    if host_table:
        eng.frontend_astar((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))           # (a start outside the map: the table comes to the host, no search)
    t.append(time.perf_counter())
    return eng, np.diff(t) * 1e3


def frames(s, n, rng):
    """tools/map_update_bench.py's frames: about a quarter of the voxels of a cube of s^3 voxels, its two far corners included"""
    out = []
    for i in range(n):
        lo = np.array([8 + (i % 6) * 40, 8 + (i // 6) * 40, rng.integers(0, dims[2] - s + 1)])
        cells = np.argwhere(rng.random((s, s, s)) < 0.25)
        cells = np.unique(np.concatenate([cells, [[0, 0, 0], [s - 1, s - 1, s - 1]]]), axis=0) + lo
        out.append(((cells + 0.5) * res).astype(np.float32))
    return out


record = {"map": list(dims), "resolution": res, "robot": "box 3.2 x 0.6 x 0.6 m", "kernel_size": 21, "attitudes": 121, "base_points": int(len(base)),
          "repeats": args.repeats, "warmup": args.warmup, "clear": [], "from_scratch": []}
rng = np.random.default_rng(1)
for host_table in (False, True):
    for s in (8, 16, 32):
        fr = frames(s, args.warmup + args.repeats, rng)
        eng, _ = build(np.concatenate([base] + fr), host_table)
        wall, rows = [], []
        for f in fr[::-1]:
            t0 = time.perf_counter(); info = eng.clear_pointcloud(f); wall.append((time.perf_counter() - t0) * 1e3)
            t_vox = int(np.prod(np.array(info.touched_hi) - np.array(info.touched_lo) + 1)) if info.touched_hi[0] >= info.touched_lo[0] else 0
            rows.append((info.count_ms, info.esdf_ms, info.frontend_ms, info.n_cleared_voxels, info.esdf_voxels_raised, info.esdf_voxels_recomputed,
                         info.cspace_voxels_recomputed, info.path, t_vox, info.host_table_patched))
        rows = np.array(rows)[args.warmup:]; wall = wall[args.warmup:]
        fresh, _ = build(base, False)
        want = fresh.frontend_cspace()[0]
        pairs = [(eng.get_grid(capi.GRID_OCCUPANCY)[0], fresh.get_grid(capi.GRID_OCCUPANCY)[0]),
                 (eng.get_grid(capi.GRID_ESDF)[0].view(np.uint32), fresh.get_grid(capi.GRID_ESDF)[0].view(np.uint32)),
                 (eng.map_counts(), fresh.map_counts()),
                 (eng.frontend_cspace_table(), want)]                # the table as the clear left it
        if host_table and rows[:, 9].all():
            pairs.append((eng.frontend_cspace_table(host=True), want))      # the patched host copy, whole
        same = all(np.array_equal(a, b) for a, b in pairs)
        assert same, "the products after the clears differ from a fresh build"
        row = {"box": s, "host_table": host_table, "wall_ms": stat(wall), "count_ms": stat(rows[:, 0]), "esdf_ms": stat(rows[:, 1]), "frontend_ms": stat(rows[:, 2]),
               "cleared_voxels": stat(rows[:, 3]), "esdf_voxels_raised": stat(rows[:, 4]), "esdf_voxels_recomputed": stat(rows[:, 5]),
               "cspace_voxels_recomputed": stat(rows[:, 6]), "touched_box_voxels": stat(rows[:, 8]),
               "paths": {"incremental": int((rows[:, 7] == 1).sum()), "full": int((rows[:, 7] == 2).sum())}, "equal_to_fresh_build": same}
        record["clear"].append(row)
        print(json.dumps(row), flush=True)
        eng.close(); fresh.close()
for host_table in (False, True):            # what is left after every series: the base cloud
    parts = []
    for _ in range(2 + 5):
        e, t = build(base, host_table); parts.append(t); e.close()
    parts = np.array(parts)[2:]
    row = {"host_table": host_table, "points": int(len(base)), "total_ms": stat(parts.sum(axis=1)), "set_pointcloud_ms": stat(parts[:, 0]),
           "generate_esdf_ms": stat(parts[:, 1]), "frontend_build_ms": stat(parts[:, 2]), "frontend_cspace_ms": stat(parts[:, 3]), "host_table_ms": stat(parts[:, 4])}
    record["from_scratch"].append(row)
    print(json.dumps(row), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
json.dump(record, open(args.out, "w"), indent=1)
print("wrote", args.out)
