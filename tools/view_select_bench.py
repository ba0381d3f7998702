#!/usr/bin/env python
"""Developer tool: the view selection (csrc/view_select.hip) on the scene of tools/view_gain_bench.py - a 256 x 256 x 256 map at 0.1 m,
seeded boxes, 12 % occupied, the 640 x 480 camera of tests/golden/camera.yaml in a free pocket at the middle, K as one integrated image
leaves it, the same 64 candidate views (eyes inside the pocket, each looking at a sampled frontier voxel), max_range_m 5.
isdf_view_select at strides 4 and 8 with k_select 1, 4 and 16: 3 warm-up and 9 timed calls by default, median [min, max] of gain_ms,
lists_ms, select_ms and of the wall time in ms, list_words, gain_selected beside gain_solo_sum, and whether a second call gave the same
bytes.  Beside it, in the same session and under the same protocol, isdf_view_gain of the same views: its gain_ms is the floor the call
cannot go under.  Writes one JSON record (default profiles/view_select_bench.json)."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "view_select_bench.json"))
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--dim", type=int, default=256)
ap.add_argument("--views", type=int, default=64)
ap.add_argument("--max-range", type=float, default=5.0)
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
rng = np.random.default_rng(64)                                     # tools/view_gain_bench.py's views
targets = np.stack(np.unravel_index(rng.choice(vox, args.views, replace=False), dims), axis=1)
eyes = t + rng.uniform(-0.5, 0.5, (args.views, 3))
poses = np.array([E.look_at(e, (v + 0.5) * res) for e, v in zip(eyes, targets)])
record = {"map": list(dims), "resolution": res, "points": int(len(cloud)), "repeats": args.repeats, "warmup": args.warmup, "views": args.views,
          "max_range_m": args.max_range, "n_known": int(kinfo.n_known), "n_frontier": int(finfo.n_frontier), "series": [], "view_gain_floor": []}

for stride in (4, 8):
    ms = []
    for _ in range(total):
        (rows, ginfo), w = timed(lambda: eng.view_gain(cam, poses, stride=stride, max_range_m=args.max_range))
        ms.append((w, ginfo.gain_ms))
    ms = np.array(ms)[args.warmup:]
    record["view_gain_floor"].append({"stride": stride, "gain_ms": stat(ms[:, 1]), "wall_ms": stat(ms[:, 0]), "gain_total": int(ginfo.gain_total),
                                      "best_gain": int(ginfo.best_gain)})
    print(json.dumps(record["view_gain_floor"][-1]), flush=True)
    for k_select in (1, 4, 16):
        ms = []
        for _ in range(total):
            out, w = timed(lambda: eng.view_select(cam, poses, stride=stride, max_range_m=args.max_range, k_select=k_select))
            ms.append((w, out[4].gain_ms, out[4].lists_ms, out[4].select_ms))
        ms = np.array(ms)[args.warmup:]
        again = eng.view_select(cam, poses, stride=stride, max_range_m=args.max_range, k_select=k_select)
        info = out[4]
        device = ms[:, 1] + ms[:, 2] + ms[:, 3]
        record["series"].append({"stride": stride, "k_select": k_select, "n_scored": int(info.n_scored), "n_selected": int(info.n_selected), "chunks": int(info.chunks),
                                 "list_words": int(info.list_words), "list_bytes": int(info.list_words) * 8, "gain_selected": int(info.gain_selected),
                                 "gain_solo_sum": int(info.gain_solo_sum), "best_single_gain": int(info.best_single_gain), "gain_ms": stat(ms[:, 1]),
                                 "lists_ms": stat(ms[:, 2]), "select_ms": stat(ms[:, 3]), "wall_ms": stat(ms[:, 0]),
                                 "share_of_device_time": {"lists": float(np.median(ms[:, 2] / device)), "rounds": float(np.median(ms[:, 3] / device))},
                                 "rows_equal_the_view_gains": bool(out[0].tobytes() == rows.tobytes()),
                                 "two_calls_same_bytes": bool(all(a.tobytes() == b.tobytes() for a, b in zip(out[:4], again[:4])))})
        print(json.dumps(record["series"][-1]), flush=True)
record["counters"] = "none collected: nothing is known about what bounds the kernels"
os.makedirs(os.path.dirname(args.out), exist_ok=True)
json.dump(record, open(args.out, "w"), indent=1)
