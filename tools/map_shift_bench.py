#!/usr/bin/env python
"""Developer tool: the map window shifted in place (isdf_shift_map) against the from-scratch sequence on the shifted cloud, on the
256 x 256 x 64 map at 0.2 m of tools/map_update_bench.py (box robot, k = 21, 11 x 11 attitudes).  For each shift, with and without a
valid host table: the shift is timed, the map is shifted back untimed, and so on - median [min, max] of the call's wall time and of its
device times after the warm-up calls; after the last timed call the products are compared byte for byte with a fresh build on the
translated cloud in the shifted box - the configuration space and the A*'s host copy as the shift left them.  No path is forced.
0.2 is no binary fraction, so a box of exactly dims x 0.2 m fails the dims guard for many shifts (the ceil lands on dims + 1): the box
here ends a quarter voxel early, bmax = bmin + (dims - 0.25) x res, which every shift keeps.  Writes one JSON record (default
profiles/map_shift_bench.json)."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as graft

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "map_shift_bench.json"))
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
args = ap.parse_args()
pkg = graft.load_package(); capi, synth = pkg.capi, pkg.synth
res, dims = 0.2, (256, 256, 64)
D = np.array(dims)
bmin, bmax = np.zeros(3), (D - 0.25) * res
occ = synth.random_box_map(dims, res=res, occupancy=0.12, seed=12345)
fe = capi.frontend_config(kernel_size=21, max_roll=45.0, max_pitch=45.0, ang_res=9.0, safeh=0.0)
SHIFTS = [(1, 0, 0), (4, 0, 0), (16, 0, 0), (4, 4, 0), (0, 0, 4)]
stat = lambda v: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}      # noqa: E731


def cloud_of(o, lo):
    return ((np.argwhere(o == 1) + 0.5) * res + lo).astype(np.float32)          # one point per occupied voxel, sta_threshold 1


def shifted(o, s):
    out = np.zeros_like(o)
    dst = tuple(slice(max(0, -s[a]), min(dims[a], dims[a] - s[a])) for a in range(3))
    src = tuple(slice(max(0, -s[a]) + s[a], min(dims[a], dims[a] - s[a]) + s[a]) for a in range(3))
    out[dst] = o[src]
    return out


def build(cloud, lo, hi, host_table):
    eng = pkg.Engine(synth.default_config(capi.V1_SWEPT))
    t = [time.perf_counter()]
    assert eng.set_pointcloud(cloud, res, 1, lo, hi) == dims; t.append(time.perf_counter())
    eng.generate_esdf(); t.append(time.perf_counter())
    eng.set_shape(synth.bench_box_shape()); eng.frontend_build(fe); t.append(time.perf_counter())
    eng.frontend_cspace(download=False); t.append(time.perf_counter())
    if host_table:
        eng.frontend_astar(lo - 1.0, lo + 1.0)           # (a start outside the map: the table comes to the host, no search)
    t.append(time.perf_counter())
    return eng, np.diff(t) * 1e3


record = {"map": list(dims), "resolution": res, "bmax": "bmin + (dims - 0.25) * resolution", "robot": "box 3.2 x 0.6 x 0.6 m", "kernel_size": 21, "attitudes": 121,
          "base_points": int((occ == 1).sum()), "repeats": args.repeats, "warmup": args.warmup, "shift": [], "from_scratch": []}
n_vox = int(np.prod(D))
for host_table in (False, True):
    for s in SHIFTS:
        back = tuple(-v for v in s)
        lo, hi = pkg.shift_geometry_host(bmin, bmax, res, dims, s)
        eng, _ = build(cloud_of(occ, bmin), bmin, bmax, host_table)
        wall, rows = [], []
        for i in range(args.warmup + args.repeats):
            if i:
                eng.shift_map(back)                      # untimed
            t0 = time.perf_counter(); info = eng.shift_map(s); wall.append((time.perf_counter() - t0) * 1e3)
            rows.append((info.translate_ms, info.esdf_ms, info.frontend_ms, info.cspace_voxels, info.path, info.n_boxes, info.host_table_patched, info.occupied_left))
        rows = np.array(rows)[args.warmup:]; wall = wall[args.warmup:]
        fresh, _ = build(cloud_of(shifted(occ, s), lo), lo, hi, False)
        want = fresh.frontend_cspace()[0]
        pairs = [(eng.get_grid(capi.GRID_OCCUPANCY)[0], fresh.get_grid(capi.GRID_OCCUPANCY)[0]),
                 (eng.get_grid(capi.GRID_ESDF)[0].view(np.uint32), fresh.get_grid(capi.GRID_ESDF)[0].view(np.uint32)),
                 (eng.map_counts(), fresh.map_counts()),
                 (eng.get_grid(capi.GRID_OCCUPANCY)[1], fresh.get_grid(capi.GRID_OCCUPANCY)[1]),
                 (eng.frontend_cspace_table(), want)]                # the table as the shift left it
        if host_table and rows[:, 6].all():
            pairs.append((eng.frontend_cspace_table(host=True), want))      # the translated and patched host copy, whole
        same = all(np.array_equal(a, b) for a, b in pairs)
        assert same, "the products after the shifts differ from a fresh build"
        row = {"shift": list(s), "host_table": host_table, "wall_ms": stat(wall), "translate_ms": stat(rows[:, 0]), "esdf_ms": stat(rows[:, 1]),
               "frontend_ms": stat(rows[:, 2]), "cspace_voxels": int(rows[0, 3]), "band_fraction": float(rows[0, 3]) / n_vox, "n_boxes": int(rows[0, 5]),
               "paths": {"incremental": int((rows[:, 4] == 1).sum()), "full": int((rows[:, 4] == 2).sum())}, "host_table_patched": bool(rows[:, 6].all()),
               "equal_to_fresh_build": same}
        record["shift"].append(row)
        print(json.dumps(row), flush=True)
        eng.close(); fresh.close()
s = (4, 0, 0)                                   # the baseline: the from-scratch sequence on the shifted cloud
lo, hi = pkg.shift_geometry_host(bmin, bmax, res, dims, s)
cloud = cloud_of(shifted(occ, s), lo)
for host_table in (False, True):
    parts = []
    for _ in range(2 + 5):
        e, t = build(cloud, lo, hi, host_table); parts.append(t); e.close()
    parts = np.array(parts)[2:]
    row = {"host_table": host_table, "points": int(len(cloud)), "total_ms": stat(parts.sum(axis=1)), "set_pointcloud_ms": stat(parts[:, 0]),
           "generate_esdf_ms": stat(parts[:, 1]), "frontend_build_ms": stat(parts[:, 2]), "frontend_cspace_ms": stat(parts[:, 3]), "host_table_ms": stat(parts[:, 4])}
    record["from_scratch"].append(row)
    print(json.dumps(row), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
json.dump(record, open(args.out, "w"), indent=1)
print("wrote", args.out)
