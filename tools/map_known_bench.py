#!/usr/bin/env python
"""Developer tool: the known grid (csrc/map_known.hip) on the scene of tools/depth_cam_bench.py - a 256 x 256 x 256 map at 0.1 m, seeded
boxes, 12 % occupied, the 640 x 480 camera of tests/golden/camera.yaml in a free pocket at the middle.  Records isdf_integrate_depth
with the mode off and on (wall and the scan's trace stage) and the merge kernel between its own optional events
(isdf_map_known_merge_ms, in a series of its own so that the on / off rows carry no extra event), the
translation stage of a (3, 0, -2) shift off and on, isdf_map_frontier with and without the list, and isdf_traj_known_horizon on a 40-piece
trajectory with the map known in a box round the first half, three quarters and 95 % of the path.  3 warm-up and 9 timed calls by default, median [min, max] in ms.  Writes one JSON record
(default profiles/map_known_bench.json).  --parent-json: the record that tools/depth_cam_bench.py of the PARENT commit, built and run in
the same session, wrote; its isdf_integrate_depth wall time (the same calls on the same scene with the same warm-up and repeats) is
recorded next to this tool's mode-off row with the verdict: the mode-off median inside the parent's [min, max] or not.  --head-json: the
record the same tool wrote on THIS tree (mode off is the default), the like-for-like pair of the parent's."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_known_bench.json"))
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--dim", type=int, default=256)
ap.add_argument("--max-range", type=float, default=10.0)
ap.add_argument("--parent-json", default=None)
ap.add_argument("--head-json", default=None)
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
rp = {"max_range_m": args.max_range, "no_return_is_free": True, "min_range_m": 0.2}          # tools/depth_cam_bench.py's
record = {"map": list(dims), "resolution": res, "points": int(len(cloud)), "repeats": args.repeats, "warmup": args.warmup}


def timed(fn):
    t0 = time.perf_counter(); out = fn(); return out, (time.perf_counter() - t0) * 1e3


eng = pkg.Engine(synth.default_config(capi.V1_SWEPT))
eng.set_pointcloud(cloud, res, 1, bmin, bmax)
image, _ = eng.depth_render(cam, pose, None)

# ---- isdf_integrate_depth, the mode off and on: a fresh map before every call, as tools/depth_cam_bench.py does
for mode in ("off", "on"):
    eng.map_known_enable(mode == "on")
    rows = []
    for _ in range(total):
        eng.set_pointcloud(cloud, res, 1, bmin, bmax)
        (dinfo, sinfo), w = timed(lambda: eng.integrate_depth(cam, pose, image, **rp))
        rows.append((w, sinfo.trace_ms, sinfo.clear.count_ms))
    rows = np.array(rows)[args.warmup:]
    record["integrate_depth_" + mode] = {"wall_ms": stat(rows[:, 0]), "trace_ms": stat(rows[:, 1]), "clear_count_ms": stat(rows[:, 2]),
                                         "rays": int(sinfo.n_rays), "free_voxels": int(sinfo.n_free_voxels)}
    print(json.dumps({mode: record["integrate_depth_" + mode]}), flush=True)
eng.map_known_merge_ms(True)                                        # the merge kernel between events of its own, a series of its own
ms = []
for _ in range(total):
    eng.set_pointcloud(cloud, res, 1, bmin, bmax)
    eng.integrate_depth(cam, pose, image, **rp)
    ms.append(eng.map_known_merge_ms(True))
eng.map_known_merge_ms(False)
record["merge_kernel_ms"] = stat(ms[args.warmup:])
print(json.dumps({"merge_kernel_ms": record["merge_kernel_ms"]}), flush=True)
if args.parent_json:
    par = json.load(open(args.parent_json))["integrate"]["integrate_depth_wall_ms"]
    off = record["integrate_depth_off"]["wall_ms"]
    record["parent_commit"] = {"integrate_depth_wall_ms": par, "tool": "tools/depth_cam_bench.py of the parent commit, same session",
                               "mode_off_median_inside_parent_min_max": bool(par["min"] <= off["median"] <= par["max"])}
    print(json.dumps(record["parent_commit"]), flush=True)
if args.head_json:          # the same unchanged tool on this tree's library (the mode is off by default): the like-for-like pair
    head = json.load(open(args.head_json))["integrate"]["integrate_depth_wall_ms"]
    record["this_tree_same_tool"] = {"integrate_depth_wall_ms": head}
    if args.parent_json:
        record["this_tree_same_tool"]["median_inside_parent_min_max"] = bool(par["min"] <= head["median"] <= par["max"])
    print(json.dumps(record["this_tree_same_tool"]), flush=True)
_, kinfo = eng.map_known()
record["known_after_one_image"] = {"n_known": int(kinfo.n_known), "newly_known": int(kinfo.newly_known)}

# ---- the translation stage of a (3, 0, -2) shift and its way back
for mode in ("off", "on"):
    eng.map_known_enable(mode == "on")
    if mode == "on":
        eng.integrate_depth(cam, pose, image, **rp)
    ms = []
    for k in range(total):
        ms.append(eng.shift_map((3, 0, -2) if k % 2 == 0 else (-3, 0, 2), force_path=2).translate_ms)
    record["shift_translate_ms_" + mode] = stat(ms[args.warmup:])
    if total % 2:
        eng.shift_map((-3, 0, 2), force_path=2)
print(json.dumps({k: v for k, v in record.items() if k.startswith("shift")}), flush=True)

# ---- the frontier of what one image has shown
eng.set_pointcloud(cloud, res, 1, bmin, bmax)
eng.integrate_depth(cam, pose, image, **rp)
for want_list in (False, True):
    rows = []
    for _ in range(total):
        (_, vox, finfo), w = timed(lambda: eng.map_frontier(want_list=want_list))
        rows.append((w, finfo.kernel_ms))
    rows = np.array(rows)[args.warmup:]
    record["frontier_with_list" if want_list else "frontier_bits_only"] = {"wall_ms": stat(rows[:, 0]), "kernel_ms": stat(rows[:, 1]), "n_frontier": int(finfo.n_frontier)}
print(json.dumps({k: v for k, v in record.items() if k.startswith("frontier")}), flush=True)

# ---- the known horizon of a 40-piece trajectory, the map known in a box round the first part of the path
eng.set_shape(synth.make_shape("RoundedCone", params=(0.8, 0.3, 1.6), bound_radius=1.9))
NP = 40
T, Cf = synth.random_trajectory(np.array(dims) * res, NP, seed=780, piece_T=1.0, jitter=0.5, margin=4.0, occ=occ, res=res)
cm = synth.colmajor(Cf)
ends = np.asarray(Cf).reshape(NP, 6, 3).sum(axis=1)                 # a piece's end point: its polynomial at t = T = 1, whatever the order of the rows
way = np.concatenate([[2 * ends[0] - ends[1]], ends])               # ... and the start, to within the waypoints' jitter
record["horizon"] = []
for frac in (0.5, 0.75, 0.95):
    k = int(round(frac * NP))
    lo = np.clip(np.floor((way[:k + 1].min(axis=0) - 4.0) / res).astype(int), 0, np.array(dims) - 1)      # 4 m: beyond far_r = 1.9 + 1.1
    hi = np.clip(np.floor((way[:k + 1].max(axis=0) + 4.0) / res).astype(int), 0, np.array(dims) - 1)
    eng.map_known_fill(None, 0)
    eng.map_known_fill(tuple(lo) + tuple(hi), 1)
    rows = []
    for _ in range(total):
        rep, w = timed(lambda: eng.traj_known_horizon(T, cm))
        rows.append((w, rep["select_ms"], rep["field_ms"], rep["reduce_ms"]))
    rows = np.array(rows)[args.warmup:]
    record["horizon"].append({"known_round_the_first": frac, "candidates": int(rep["candidates"]), "n_below_margin": int(rep["n_below_margin"]), "horizon_t": rep["horizon_t"],
                              "horizon_piece": int(rep["horizon_piece"]), "wall_ms": stat(rows[:, 0]), "select_ms": stat(rows[:, 1]), "field_ms": stat(rows[:, 2]),
                              "reduce_ms": stat(rows[:, 3])})
    print(json.dumps(record["horizon"][-1]), flush=True)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
json.dump(record, open(args.out, "w"), indent=1)
