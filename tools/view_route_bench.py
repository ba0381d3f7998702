#!/usr/bin/env python
"""Developer tool: the routed view selection (csrc/view_select.hip) against today's composition on the same ctx, on the
scene of tools/view_select_bench.py scaled to --dim (default 128 x 128 x 128 at 0.1 m, seeded boxes, 12 % occupied, the 640 x 480
camera of tests/golden/camera.yaml in a free pocket at the middle, K as one integrated image leaves it, --views candidate views with
eyes in the pocket) with a box robot's front end (kernel_size 5, 3 x 3 attitudes) and the ungated cost-to-go field towards the camera's
cell.
  one call      isdf_view_select_routed with path_cap: the selection, the costs and the ways in one call;
  composition   isdf_view_select over all poses, isdf_frontend_field_value at the eyes, isdf_frontend_field_paths for the picked
                eyes, each with its own hand-overs - what a caller does today.  It cannot drop an unreachable view before the rounds and
                does not weigh by cost, so it may pick another set: the record says whether it did.
3 warm-up and 9 timed rounds by default, the two alternating within a round; median [min, max] of the wall time in ms and of the call's
*_ms words.  No speed-up is promised: the file records what was measured.  Writes one JSON record (default
profiles/view_route_bench.json)."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "view_route_bench.json"))
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--dim", type=int, default=128)
ap.add_argument("--views", type=int, default=64)
ap.add_argument("--max-range", type=float, default=5.0)
ap.add_argument("--path-cap", type=int, default=256)
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


def timed(fn):
    t0 = time.perf_counter(); out = fn(); return out, (time.perf_counter() - t0) * 1e3


eng = pkg.Engine(synth.default_config(capi.V1_SWEPT))
eng.set_pointcloud(cloud, res, 1, bmin, bmax)
eng.set_shape(synth.make_shape("Box", params=(0.09, 0.02, 0.015)))
eng.frontend_build(capi.frontend_config(kernel_size=5, max_roll=30.0, max_pitch=30.0, ang_res=30.0, safeh=0.0))
eng.frontend_cspace(download=False)
eng.map_known_enable(True)
image, _ = eng.depth_render(cam, pose, None)
eng.integrate_depth(cam, pose, image, max_range_m=10.0, no_return_is_free=True, min_range_m=0.2)
_, vox, finfo = eng.map_frontier()
finfo_field = eng.frontend_field_build(t)
rng = np.random.default_rng(64)
targets = np.stack(np.unravel_index(rng.choice(vox, args.views, replace=False), dims), axis=1)
eyes = t + rng.uniform(-0.5, 0.5, (args.views, 3))
poses = np.array([E.look_at(e, (v + 0.5) * res) for e, v in zip(eyes, targets)])
record = {"map": list(dims), "resolution": res, "points": int(len(cloud)), "repeats": args.repeats, "warmup": args.warmup, "views": args.views,
          "max_range_m": args.max_range, "path_cap": args.path_cap, "n_frontier": int(finfo.n_frontier),
          "field": {"reachable": int(finfo_field.reachable), "status": int(finfo_field.status), "reached_voxels": int(finfo_field.reached_voxels)}, "series": []}


def composed(stride, k_select):
    """today: the selection over all poses, the field at the eyes, the paths of the picked ones"""
    rows, select, rnd, claimed, info = eng.view_select(cam, poses, stride=stride, max_range_m=args.max_range, k_select=k_select)
    cost = eng.frontend_field(eyes)
    picked = select[:info.n_selected, 0]
    keep = picked[np.isfinite(cost[picked])]
    paths = eng.frontend_field_paths(eyes[keep], args.path_cap) if len(keep) else None
    return select, cost, keep, paths, info


for stride in (4, 8):
    for k_select in (4, 16):
        one, two = [], []
        for _ in range(total):
            out, w = timed(lambda: eng.view_select_routed(cam, poses, stride=stride, max_range_m=args.max_range, k_select=k_select, path_cap=args.path_cap))
            info = out[7]
            one.append((w, info.select.gain_ms, info.select.lists_ms, info.select.select_ms, info.cost_ms, info.paths_ms))
            comp, w = timed(lambda: composed(stride, k_select))
            two.append(w)
        one, two = np.array(one)[args.warmup:], np.array(two)[args.warmup:]
        again = eng.view_select_routed(cam, poses, stride=stride, max_range_m=args.max_range, k_select=k_select, path_cap=args.path_cap)
        ns = int(info.select.n_selected)
        record["series"].append({"stride": stride, "k_select": k_select, "n_scored": int(info.select.n_scored), "n_selected": ns, "n_eligible": int(info.n_eligible),
                                 "n_unreachable": int(info.n_unreachable), "cost_selected": float(info.cost_selected), "gain_selected": int(info.select.gain_selected),
                                 "one_call_wall_ms": stat(one[:, 0]), "composition_wall_ms": stat(two), "gain_ms": stat(one[:, 1]), "lists_ms": stat(one[:, 2]),
                                 "select_ms": stat(one[:, 3]), "cost_ms": stat(one[:, 4]), "paths_ms": stat(one[:, 5]),
                                 "composition_selected": int(comp[4].n_selected), "composition_kept_reachable": int(len(comp[2])),
                                 "composition_gain_selected": int(comp[4].gain_selected),
                                 "same_views_picked": bool(out[1][:ns, 0].tolist() == comp[2].tolist()),
                                 "costs_equal_field_value": bool(out[4].tobytes() == comp[1].tobytes()),
                                 "two_calls_same_bytes": bool(all(a.tobytes() == b.tobytes() for a, b in zip(out[:6] + out[6], again[:6] + again[6])))})
        print(json.dumps(record["series"][-1]), flush=True)
record["counters"] = "none collected: nothing is known about what bounds the kernels"
os.makedirs(os.path.dirname(args.out), exist_ok=True)
json.dump(record, open(args.out, "w"), indent=1)
