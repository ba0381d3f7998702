#!/usr/bin/env python
"""Developer tool: the view gain (csrc/view_gain.hip) on the scene of tools/map_known_bench.py - a 256 x 256 x 256 map at 0.1 m, seeded
boxes, 12 % occupied, the 640 x 480 camera of tests/golden/camera.yaml in a free pocket at the middle, K as one integrated image
leaves it.  64 candidate views: eyes inside the pocket, each looking at a sampled frontier voxel (look_at).  isdf_view_gain at strides
1, 4 and 8 with max_range_m 5: 3 warm-up and 9 timed calls by default, median [min, max] of gain_ms and of the wall time in ms.  After
each series the rows are compared with a second call's.  Beside it (a) the way without the call, per view isdf_depth_rays on an empty
image + isdf_map_raycast + a replay of every walk on the host (isdf_scan_ray_host per ray, a NumPy union, the test against K), on 4 views
at stride 8, its rows compared with the call's; (b) --trace-json: the record tools/map_known_bench.py wrote in the same session, whose
isdf_integrate_depth trace stage (the same walk with an OR at every voxel, one image) is copied next to the stride-1 time per view.
Writes one JSON record (default profiles/view_gain_bench.json)."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "view_gain_bench.json"))
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--dim", type=int, default=256)
ap.add_argument("--views", type=int, default=64)
ap.add_argument("--max-range", type=float, default=5.0)
ap.add_argument("--trace-json", default=None)
args = ap.parse_args()
import torch                                                        # before the library touches the device (tests/conftest.py says why)
torch.zeros(1, device="cuda")
pkg = graft.load_package(); capi, synth, E = pkg.capi, pkg.synth, pkg.engine
res, dims = 0.1, (args.dim,) * 3
bmin, bmax = np.zeros(3), np.array(dims) * res
stat = lambda v: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}      # noqa: E731
total = args.warmup + args.repeats

occ = synth.random_box_map(dims, res=res, occupancy=0.12, seed=12345)
mid = np.array(dims) // 2
occ[tuple(slice(m - 6, m + 7) for m in mid)] = 0                    # the camera's pocket
cloud = np.ascontiguousarray(((np.argwhere(occ == 1) + 0.5) * res).astype(np.float32))
cam = E.camera_from_yaml(os.path.join(ROOT, "tests", "golden", "camera.yaml"))
t = (mid + 0.5) * res + np.array([0.03, -0.02, 0.01])
pose = np.concatenate([np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]]), t.reshape(3, 1)], axis=1).reshape(12)
rp = {"max_range_m": 10.0, "no_return_is_free": True, "min_range_m": 0.2}          # tools/map_known_bench.py's


def timed(fn):
    t0 = time.perf_counter(); out = fn(); return out, (time.perf_counter() - t0) * 1e3


eng = pkg.Engine(synth.default_config(capi.V1_SWEPT))
eng.set_pointcloud(cloud, res, 1, bmin, bmax)
eng.map_known_enable(True)
image, _ = eng.depth_render(cam, pose, None)
eng.integrate_depth(cam, pose, image, **rp)
_, vox, finfo = eng.map_frontier()
_, kinfo = eng.map_known()
rng = np.random.default_rng(64)
targets = np.stack(np.unravel_index(rng.choice(vox, args.views, replace=False), dims), axis=1)
eyes = t + rng.uniform(-0.5, 0.5, (args.views, 3))
poses = np.array([E.look_at(e, (v + 0.5) * res) for e, v in zip(eyes, targets)])
record = {"map": list(dims), "resolution": res, "points": int(len(cloud)), "repeats": args.repeats, "warmup": args.warmup, "views": args.views,
          "max_range_m": args.max_range, "n_known": int(kinfo.n_known), "n_frontier": int(finfo.n_frontier), "series": []}

for stride in (1, 4, 8):
    rows = []
    for _ in range(total):
        (out, info), w = timed(lambda: eng.view_gain(cam, poses, stride=stride, max_range_m=args.max_range))
        rows.append((w, info.gain_ms))
    rows = np.array(rows)[args.warmup:]
    again, _ = eng.view_gain(cam, poses, stride=stride, max_range_m=args.max_range)
    record["series"].append({"stride": stride, "rays_per_view": int(info.n_rays_per_view), "chunks": int(info.chunks), "n_scored": int(info.n_scored),
                             "best_view": int(info.best_view), "best_gain": int(info.best_gain), "gain_total": int(info.gain_total),
                             "steps_total": int(out[:, 5].sum()), "n_hits": int(out[:, 4].sum()), "gain_ms": stat(rows[:, 1]), "wall_ms": stat(rows[:, 0]),
                             "gain_ms_per_view": float(np.median(rows[:, 1])) / args.views, "two_calls_same_bytes": bool(again.tobytes() == out.tobytes())})
    print(json.dumps(record["series"][-1]), flush=True)
    if stride == 8:
        rows8 = out

# ---- (a) without the call: rays down, rows down, the walks replayed on the host; 4 views at stride 8
k_unknown = ~E.known_unpack(eng.map_known()[0], dims).reshape(-1)
empty = np.zeros((cam.height, cam.width), dtype=np.uint16)
ms, same = [], True
for j in range(4):
    def one():
        ends, _, _ = eng.depth_rays(cam, poses[j], empty, stride=8, max_range_m=args.max_range, no_return_is_free=True)
        rc, _ = eng.map_raycast(eyes[j], ends, test_origin_voxel=False)
        seen = np.zeros(k_unknown.size, dtype=bool)
        for e, steps in zip(ends[rc[:, 0] <= 1], rc[rc[:, 0] <= 1, 1]):
            w = E.scan_ray_host(bmin, bmax, res, dims, eyes[j], e)[:int(steps) + 1].astype(np.int64)
            seen[(w[:, 0] * dims[1] + w[:, 1]) * dims[2] + w[:, 2]] = True
        return int((seen & k_unknown).sum())
    g, w = timed(one)
    ms.append(w)
    same = same and g == int(rows8[j, 1])
record["without_the_call_stride_8"] = {"views": 4, "wall_ms_per_view": stat(ms), "gains_equal_the_calls": bool(same)}
print(json.dumps(record["without_the_call_stride_8"]), flush=True)

# ---- (b) the trace stage of isdf_integrate_depth, one image, from tools/map_known_bench.py's record of the same session
if args.trace_json:
    tr = json.load(open(args.trace_json))["integrate_depth_on"]
    record["integrate_depth_trace_stage"] = {"trace_ms": tr["trace_ms"], "rays": tr["rays"], "tool": "tools/map_known_bench.py, same session",
                                             "view_gain_stride_1_ms_per_view": record["series"][0]["gain_ms_per_view"]}
    print(json.dumps(record["integrate_depth_trace_stage"]), flush=True)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
json.dump(record, open(args.out, "w"), indent=1)
