#!/usr/bin/env python
"""Developer tool: the gated cost-to-go field kept across depth images (isdf_frontend_field_set_known_follow mode 1) against
what mode 0 makes a caller do - the image, which drops the field, followed by isdf_frontend_field_build_known - on the scene of
tools/known_gate_bench.py: a 256 x 256 x 256 map at 0.1 m, seeded boxes, 12 % occupied, the 640 x 480 camera of tests/golden/camera.yaml in
a free pocket at the middle, K as one integrated image leaves it and the pocket declared known, the field benches' robot and front end
(kernel_size 21).  The gate's radii are 1 and 3.

A sequence is a short motion of the camera along its viewing axis towards the goal, one depth image per pose, rendered once from the
untouched map.  Two ctxs start every sequence from the same map, K and gated field; per image
  follow   mode 1: isdf_integrate_depth, the stages' device_ms + erode_ms (isdf_frontend_field_follow_info; 0 where no stage ran);
  rebuild  mode 0: isdf_integrate_depth, then isdf_frontend_field_build_known: its erode_ms + device_ms.
Both run in one session, alternated sequence by sequence: 3 warm-up and 9 timed sequences by default, median [min, max] per image.  After
the last sequence the followed field's bytes are compared with the rebuilt one's.  The yardstick is the rebuild of the same session.
--guard: the paths this feature does not change, for comparing two builds of the library (ISDF_ACCEL_LIB) in one session: the ungated
isdf_frontend_field_build's device_ms, and the ungated repair's device_ms (isdf_frontend_field_set_repair mode 1) over updates of about a
quarter of the voxels of an 8^3 cube at disjoint places along +y, the same places in every run.
--join LABEL=FILE ...: no device work - the guard records of several such runs, each a process of its own with its own --out, put
together in the order given into one file (profiles/known_follow_guard.json) with the verdict: the medians of every run not labelled
"parent commit" lie inside each parent run's own [min, max], and every run's repairs reset the same voxels frame by frame.
Writes one JSON record (default profiles/known_follow_bench.json)."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "known_follow_bench.json"))
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--dim", type=int, default=256)
ap.add_argument("--images", type=int, default=4)
ap.add_argument("--guard", action="store_true")
ap.add_argument("--join", nargs="+", metavar="LABEL=FILE")
args = ap.parse_args()
if args.join:
    PARENT, KEYS = "parent commit", ("ungated_build_device_ms", "ungated_repair_device_ms")
    runs, first = [], None
    for order, item in enumerate(args.join, 1):
        label, path = item.split("=", 1)
        rec = json.load(open(path))
        first = first or rec
        runs.append({"library": label, "order": order, **rec["guard"]})
    parents, trees = [r for r in runs if r["library"] == PARENT], [r for r in runs if r["library"] != PARENT]
    holds = bool(parents and trees) and all(p[k]["min"] <= t[k]["median"] <= p[k]["max"] for t in trees for p in parents for k in KEYS) \
        and all(r["reset_voxels_per_frame"] == runs[0]["reset_voxels_per_frame"] for r in runs)
    what = ("the ungated isdf_frontend_field_build's device_ms and the ungated repair's device_ms (isdf_frontend_field_set_repair mode 1, nine updates of 128 voxels at the "
            "same disjoint places in every run) on the parent commit's library and on this tree's, alternated twice in one session (tools/known_follow_bench.py --guard; "
            f"{first['map'][0]}^3 at {first['resolution']} m, kernel_size 21, {first['warmup']} warm-up and {first['repeats']} timed each)")
    json.dump({"what": what, "rule": "this tree's medians lie inside each of the parent's own [min, max]; the repairs reset the same voxels frame by frame",
               "holds": holds, "runs": runs}, open(args.out, "w"), indent=1)
    sys.exit(0)
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
t0 = (mid + 0.5) * res + np.array([0.03, -0.02, 0.01])
rot = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])      # the camera looks along +x
rp = {"max_range_m": 10.0, "no_return_is_free": True, "min_range_m": 0.2}          # tools/map_known_bench.py's
step = np.array([0.12, 0.0, 0.0])                                   # per image, inside the pocket
goal = t0 + (args.images + 1) * step                                # ahead of the last pose, in the pocket
pocket = tuple(int(m) - 6 for m in mid) + tuple(int(m) + 6 for m in mid)


def pose_at(i):
    return np.concatenate([rot, (t0 + i * step).reshape(3, 1)], axis=1).reshape(12)


def start(eng):
    """the map, K and the front end as at the start of a sequence"""
    eng.set_pointcloud(cloud, res, 1, bmin, bmax)
    eng.map_known_enable(True)
    eng.integrate_depth(cam, pose_at(0), images[0], **rp)
    eng.map_known_fill(pocket, 1)                                   # no ray starts inside the robot: its pocket is declared known
    eng.set_shape(synth.bench_box_shape())
    eng.frontend_build(capi.frontend_config(kernel_size=21, max_roll=45.0, max_pitch=45.0, ang_res=9.0, safeh=0.0))
    eng.frontend_cspace(download=False)


follow, rebuild = pkg.Engine(synth.default_config(capi.V1_SWEPT)), pkg.Engine(synth.default_config(capi.V1_SWEPT))
follow.set_pointcloud(cloud, res, 1, bmin, bmax)
images = [follow.depth_render(cam, pose_at(i), None)[0] for i in range(args.images + 1)]     # of the untouched map
record = {"map": list(dims), "resolution": res, "points": int(len(cloud)), "repeats": args.repeats, "warmup": args.warmup, "images": args.images,
          "library": os.path.relpath(os.environ.get("ISDF_ACCEL_LIB", capi.LIB_PATH), ROOT), "goal": [float(v) for v in goal], "step_m": float(step[0]), "series": []}

if args.guard:
    start(follow)
    follow.frontend_field_set_repair(1)
    builds = [follow.frontend_field_build(goal).device_ms for _ in range(total)]
    rng = np.random.default_rng(77)
    repairs, shares = [], []
    for j in range(total):
        lo = mid + np.array([10, 14 + 9 * j - 9 * (total // 2), 10])
        cells = lo + rng.permutation(np.argwhere(np.ones((8, 8, 8), dtype=bool)))[:128]
        info = follow.update_pointcloud(((cells + 0.5) * res).astype(np.float32), full_fraction=1.0)
        assert info.field_dropped == 0
        r = follow.frontend_field_repair_info()
        repairs.append(r.device_ms); shares.append(int(r.reset_voxels))
    record["guard"] = {"ungated_build_device_ms": stat(builds[args.warmup:]), "ungated_repair_device_ms": stat(repairs[args.warmup:]),
                       "ungated_repair_device_ms_per_frame": [float(v) for v in repairs[args.warmup:]], "reset_voxels_per_frame": shares[args.warmup:]}
    print(json.dumps(record["guard"]), flush=True)
    json.dump(record, open(args.out, "w"), indent=1)
    sys.exit(0)

follow.frontend_field_set_known_follow(1)
for radius in (1, 3):
    f_ms, r_ms, frames = [], [], None
    t_start = time.time()
    for seq in range(total):
        rows_f, rows_r, notes = [], [], []
        # follow
        start(follow)
        info, _ = follow.frontend_field_build_known(goal, radius, 0)
        for i in range(1, args.images + 1):
            _, s = follow.integrate_depth(cam, pose_at(i), images[i], **rp)
            ran = s.clear.n_cleared_voxels > 0 or s.update.n_new_voxels > 0 or follow.map_known()[1].newly_known > 0
            assert (s.clear.field_dropped, s.update.field_dropped) == (0, 0)
            f = follow.frontend_field_follow_info() if ran else None
            rows_f.append(f.device_ms + f.erode_ms if f else 0.0)
            notes.append({"cleared": int(s.clear.n_cleared_voxels), "new": int(s.update.n_new_voxels), "opening": int(f.opening) if f else 0,
                          "closing": int(f.closing) if f else 0, "opened_voxels": int(f.opened_voxels) if f else 0, "closed_voxels": int(f.closed_voxels) if f else 0,
                          "reached_voxels": int(f.reached_voxels) if f else int(info.reached_voxels),
                          "reset_share": float(follow.frontend_field_repair_info().reset_voxels) / max(1, int(info.reached_voxels)) if f and f.closing else 0.0})
        # rebuild
        start(rebuild)
        rebuild.frontend_field_build_known(goal, radius, 0)
        for i in range(1, args.images + 1):
            _, s = rebuild.integrate_depth(cam, pose_at(i), images[i], **rp)
            assert (s.clear.field_dropped, s.update.field_dropped) == (1, 1)
            binfo, gate = rebuild.frontend_field_build_known(goal, radius, 0)
            rows_r.append(binfo.device_ms + gate.erode_ms)
        f_ms.append(rows_f); r_ms.append(rows_r); frames = notes
        if seq == 0:
            print(f"radius {radius}: one sequence of both modes took {time.time() - t_start:.1f} s", flush=True)
    same = np.array_equal(follow.frontend_field().view(np.uint64), rebuild.frontend_field().view(np.uint64))
    f_ms, r_ms = np.array(f_ms)[args.warmup:], np.array(r_ms)[args.warmup:]
    for i in range(args.images):
        frames[i].update(image=i + 1, follow_ms=stat(f_ms[:, i]), rebuild_ms=stat(r_ms[:, i]),
                         follow_loses=bool(np.median(f_ms[:, i]) > np.median(r_ms[:, i])))
    record["series"].append({"radius": radius, "border": 0, "reachable": int(info.reachable), "free_voxels": int(info.free_voxels),
                             "reached_voxels_at_start": int(info.reached_voxels), "same_bytes_after_the_last_sequence": bool(same), "frames": frames})
    print(json.dumps(record["series"][-1]), flush=True)
    assert same
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
json.dump(record, open(args.out, "w"), indent=1)
