#!/usr/bin/env python
"""Developer tool: rays cast through the map on the device (isdf_map_raycast / isdf_map_raycast_device) against what a caller had before
it existed - isdf_raycast_host on one host thread, and the numpy march in quarter-voxel steps that tools/map_scan_bench.py makes its
scans with (its function, copied) - on the 256 x 256 x 256 map at 0.2 m of DESIGN 4.16: seeded boxes, 12 % occupied, the sensor in a
free pocket near the middle.  Casts of 64 x 64, 256 x 256 and 512 x 512 rays over the whole sphere, each to max range.  The cast reads
the occupancy only: no ESDF and no front end are built.  Median [min, max] after warm-up; the numpy march is timed once per size.  After
each series the device's rows are compared with the host form's.  Writes one JSON record (default profiles/map_raycast_bench.json)."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as graft

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "map_raycast_bench.json"))
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--dim", type=int, default=256)
ap.add_argument("--sides", type=int, nargs="+", default=[64, 256, 512])
ap.add_argument("--max-range", type=float, default=12.0)
args = ap.parse_args()
import torch                                                        # before the library touches the device (tests/conftest.py says why)
torch.zeros(1, device="cuda")
pkg = graft.load_package(); capi, synth = pkg.capi, pkg.synth
res, dims = 0.2, (args.dim,) * 3
bmin, bmax = np.zeros(3), np.array(dims) * res
stat = lambda v: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}      # noqa: E731

occ = synth.random_box_map(dims, res=res, occupancy=0.12, seed=12345)
mid = np.array(dims) // 2
occ[tuple(slice(m - 6, m + 7) for m in mid)] = 0                    # the sensor's pocket
origin = (mid + 0.5) * res + np.array([0.03, -0.05, 0.07])
base = ((np.argwhere(occ == 1) + 0.5) * res).astype(np.float32)     # one point per occupied voxel, sta_threshold 1


def directions(side):
    az, el = np.meshgrid(np.linspace(-np.pi, np.pi, side, endpoint=False), np.arcsin(np.linspace(-0.98, 0.98, side)), indexing="ij")
    return np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], axis=-1).reshape(-1, 3)


def march(d, world):
    """tools/map_scan_bench.py's scan(): every direction marched through `world` in steps of a quarter voxel"""
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


eng = pkg.Engine(synth.default_config(capi.V1_SWEPT))
eng.set_pointcloud(base, res, 1, bmin, bmax)
got_occ, got_bmin, got_bmax = eng.get_grid(capi.GRID_OCCUPANCY)
assert np.array_equal(got_occ, occ)
record = {"map": list(dims), "resolution": res, "occupied_share": float(occ.mean()), "max_range_m": args.max_range, "repeats": args.repeats, "warmup": args.warmup,
          "casts": []}
for side in args.sides:
    d = directions(side)
    with np.errstate(divide="ignore", invalid="ignore"):
        t_box = np.where(d > 0, (bmax - origin) / d, np.where(d < 0, (bmin - origin) / d, np.inf)).min(axis=1)
    ends = (origin + d * np.minimum(args.max_range, 0.999 * t_box)[:, None]).astype(np.float32)          # clipped to the box by the caller
    n = len(ends)
    d_ends = torch.from_numpy(ends).cuda()
    d_rows = torch.zeros((n, 8), dtype=torch.int32, device="cuda")
    host_ptr, dev_ptr, host_form = [], [], []
    for k in range(args.warmup + args.repeats):
        t0 = time.perf_counter(); rows, info = eng.map_raycast(origin, ends); wall = (time.perf_counter() - t0) * 1e3
        host_ptr.append((wall, info.cast_ms))
        t0 = time.perf_counter(); dinfo = eng.map_raycast_device(origin, d_ends, d_rows); wall = (time.perf_counter() - t0) * 1e3
        dev_ptr.append((wall, dinfo.cast_ms))
        t0 = time.perf_counter(); want, _ = pkg.engine.raycast_host(got_occ, got_bmin, got_bmax, res, origin, ends); wall = (time.perf_counter() - t0) * 1e3
        host_form.append(wall)
    assert rows.tobytes() == want.tobytes() == d_rows.cpu().numpy().tobytes(), "the device's rows differ from the host form's"
    t0 = time.perf_counter(); m_ends, m_hit = march(d, occ); march_ms = (time.perf_counter() - t0) * 1e3
    host_ptr, dev_ptr, host_form = np.array(host_ptr)[args.warmup:], np.array(dev_ptr)[args.warmup:], np.array(host_form)[args.warmup:]
    dev_ms = np.concatenate([host_ptr[:, 1], dev_ptr[:, 1]])
    row = {"rays": n, "hits": int(info.n_hits), "clear": int(info.n_clear), "skipped": int(info.n_skipped), "steps_total": int(info.steps_total),
           "cast_ms": stat(dev_ms), "steps_per_second": float(info.steps_total / (np.median(dev_ms) * 1e-3)),
           "map_raycast_wall_ms": stat(host_ptr[:, 0]), "map_raycast_device_wall_ms": stat(dev_ptr[:, 0]),
           "raycast_host_one_thread_ms": stat(host_form), "numpy_quarter_voxel_march_ms": float(march_ms), "march_hits": int(m_hit.sum()),
           "wall_ratio_host_form_over_map_raycast": float(np.median(host_form) / np.median(host_ptr[:, 0])),
           "wall_ratio_march_over_map_raycast": float(march_ms / np.median(host_ptr[:, 0]))}
    record["casts"].append(row)
    print(json.dumps(row), flush=True)
eng.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
json.dump(record, open(args.out, "w"), indent=1)
print("wrote", args.out)
