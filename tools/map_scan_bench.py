#!/usr/bin/env python
"""Developer tool: a range scan integrated on the device (isdf_integrate_scan) against what a caller had to do before it existed - trace
the rays on one host thread (isdf_scan_sets_host), then isdf_clear_pointcloud of the voxels passed and isdf_update_pointcloud of the hit
end points - on a 256 x 256 x 256 map at 0.2 m with its ESDF and front end built (box robot, k = 21, 11 x 11 attitudes).
The sensor stands in a free voxel near the middle and looks at a WORLD that differs from the map the ctx holds: one block of obstacles of
the map is gone from the world and another stands where the map is free, so that every scan both frees and occupies voxels.  Scans of
64 x 64, 256 x 256 and 512 x 512 rays over the whole sphere, each marched through the world to its first occupied voxel or to max range
(no hit).  After every timed call the map is put back with the two in-place calls (untimed), so every repeat starts from the same map;
both ways alternate within one size.  Median [min, max] after warm-up.  The counts after a scan are compared with numpy's on the host
sets.  Writes one JSON record (default profiles/map_scan_bench.json)."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as graft

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "map_scan_bench.json"))
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--dim", type=int, default=256)
ap.add_argument("--sides", type=int, nargs="+", default=[64, 256, 512])
ap.add_argument("--max-range", type=float, default=12.0)
args = ap.parse_args()
pkg = graft.load_package(); capi, synth = pkg.capi, pkg.synth
res, dims = 0.2, (args.dim,) * 3
bmin, bmax = np.zeros(3), np.array(dims) * res
stat = lambda v: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}      # noqa: E731
centres = lambda cells: ((np.asarray(cells).reshape(-1, 3) + 0.5) * res).astype(np.float32)             # noqa: E731

occ = synth.random_box_map(dims, res=res, occupancy=0.12, seed=12345)
mid = np.array(dims) // 2
occ[tuple(slice(m - 6, m + 7) for m in mid)] = 0                    # the sensor's pocket
origin = (mid + 0.5) * res + np.array([0.03, -0.05, 0.07])
world = occ.copy()
s = min(16, args.dim // 8)
gone = tuple(slice(m + 10, m + 10 + s) for m in mid)                # a block of the map that the world no longer has ...
occ[gone] = 1
world[gone] = 0
new = (slice(mid[0] - 10 - s, mid[0] - 10), slice(mid[1] - s // 2, mid[1] + s // 2), slice(mid[2] - s // 2, mid[2] + s // 2))
occ[new] = 0                                                        # ... and one the map does not know yet
world[new] = 1
base = centres(np.argwhere(occ == 1))                               # one point per occupied voxel, sta_threshold 1
c0 = occ.astype(np.int64)


def scan(side):
    """side x side directions over the sphere, marched through the world in steps of a quarter voxel"""
    az, el = np.meshgrid(np.linspace(-np.pi, np.pi, side, endpoint=False), np.arcsin(np.linspace(-0.98, 0.98, side)), indexing="ij")
    d = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], axis=-1).reshape(-1, 3)
    n = len(d)
    length = np.full(n, args.max_range)
    hit = np.zeros(n, dtype=np.uint8)
    alive = np.ones(n, dtype=bool)
    for t in np.arange(0.25 * res, args.max_range, 0.25 * res):
        idx = np.flatnonzero(alive)
        if not len(idx):
            break
        cell = np.floor((origin + d[idx] * t) / res).astype(np.int64)
        out = ((cell < 0) | (cell >= np.array(dims))).any(axis=1)
        length[idx[out]] = t - 0.25 * res                           # the map's edge: cut to length, no hit
        alive[idx[out]] = False
        idx, cell = idx[~out], cell[~out]
        struck = world[tuple(cell.T)] == 1
        length[idx[struck]] = t; hit[idx[struck]] = 1
        alive[idx[struck]] = False
    return (origin + d * length[:, None]).astype(np.float32), hit


def build():
    eng = pkg.Engine(synth.default_config(capi.V1_SWEPT))
    eng.set_pointcloud(base, res, 1, bmin, bmax)
    eng.generate_esdf()
    eng.set_shape(synth.bench_box_shape())
    eng.frontend_build(capi.frontend_config(kernel_size=21, max_roll=45.0, max_pitch=45.0, ang_res=9.0, safeh=0.0))
    eng.frontend_cspace(download=False)
    return eng


record = {"map": list(dims), "resolution": res, "robot": "box 3.2 x 0.6 x 0.6 m", "kernel_size": 21, "attitudes": 121, "base_points": int(len(base)),
          "max_range_m": args.max_range, "miss_weight": 1, "repeats": args.repeats, "warmup": args.warmup, "scans": []}
eng = build()
for side in args.sides:
    xyz, hit = scan(side)
    t0 = time.perf_counter()
    free, hits, skipped = pkg.engine.scan_sets_host(bmin, bmax, res, dims, origin, xyz, hit)
    c1 = np.where(free == 1, np.maximum(c0 - 1, 0), c0 + hits)
    up, down = np.repeat(np.argwhere(c1 > c0), (c1 - c0)[c1 > c0], axis=0), np.repeat(np.argwhere(c0 > c1), (c0 - c1)[c0 > c1], axis=0)

    def put_back():
        eng.clear_pointcloud(centres(up)); eng.update_pointcloud(centres(down))

    dev, old = [], []
    for k in range(args.warmup + args.repeats):
        t0 = time.perf_counter(); info = eng.integrate_scan(origin, xyz, hit); wall = (time.perf_counter() - t0) * 1e3
        if k == 0:
            assert np.array_equal(eng.map_counts(), c1.astype(np.uint32)), "the counts after the scan differ from numpy's on the host sets"
        dev.append((wall, info.trace_ms, info.clear.count_ms, info.clear.esdf_ms, info.clear.frontend_ms, info.update.count_ms, info.update.esdf_ms, info.update.frontend_ms,
                    info.clear.path, info.update.path, info.clear.n_cleared_voxels, info.update.n_new_voxels, info.n_free_voxels, info.n_hits))
        put_back()
        t0 = time.perf_counter()
        f, _, _ = pkg.engine.scan_sets_host(bmin, bmax, res, dims, origin, xyz, hit); t1 = time.perf_counter()
        ci = eng.clear_pointcloud(centres(np.argwhere(f == 1))); t2 = time.perf_counter()
        ui = eng.update_pointcloud(xyz[hit != 0]); t3 = time.perf_counter()
        old.append(((t3 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3))
        assert (ci.n_cleared_voxels, ui.n_new_voxels, ci.path, ui.path) == (info.clear.n_cleared_voxels, info.update.n_new_voxels, info.clear.path, info.update.path)
        put_back()
    assert np.array_equal(eng.map_counts(), c0.astype(np.uint32)), "the map did not come back"
    dev, old = np.array(dev)[args.warmup:], np.array(old)[args.warmup:]
    row = {"rays": int(len(xyz)), "hits": int(dev[0, 13]), "free_voxels": int(dev[0, 12]), "cleared_voxels": int(dev[0, 10]), "new_voxels": int(dev[0, 11]),
           "paths": {"clear": int(dev[0, 8]), "update": int(dev[0, 9])},
           "integrate_scan": {"wall_ms": stat(dev[:, 0]), "trace_ms": stat(dev[:, 1]), "clear_count_ms": stat(dev[:, 2]), "clear_esdf_ms": stat(dev[:, 3]),
                              "clear_frontend_ms": stat(dev[:, 4]), "update_count_ms": stat(dev[:, 5]), "update_esdf_ms": stat(dev[:, 6]), "update_frontend_ms": stat(dev[:, 7])},
           "host_trace_and_two_calls": {"wall_ms": stat(old[:, 0]), "scan_sets_host_ms": stat(old[:, 1]), "clear_pointcloud_ms": stat(old[:, 2]),
                                        "update_pointcloud_ms": stat(old[:, 3])},
           "wall_ratio_old_over_new": float(np.median(old[:, 0]) / np.median(dev[:, 0]))}
    record["scans"].append(row)
    print(json.dumps(row), flush=True)
eng.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
json.dump(record, open(args.out, "w"), indent=1)
print("wrote", args.out)
