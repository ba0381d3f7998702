#!/usr/bin/env python
"""Developer tool: candidate views (csrc/view_cand.hip) on the scene of tools/view_gain_bench.py - a 256 x 256 x 256 map at 0.1 m, seeded
boxes, 12 % occupied, the 640 x 480 camera of tests/golden/camera.yaml in a free pocket at the middle, K as one integrated image leaves
it.  Targets: the rep_voxel centres of the frontier's clusters at connectivity 26, and at 6 for more targets.  Offsets: 3 radii x 16
azimuths x 3 heights (view_ring_offsets).  isdf_view_candidates at gain strides 8 and 4 with max_range_m 5: 3 warm-up and 9 timed calls
by default, median [min, max] of filter_ms, gain_ms, select_ms and of the wall time in ms, the kept counts, and whether a second call
gave the same bytes.  Beside it the way without the call on the same inputs (connectivity 26, stride 8): K and the occupancy pulled to
the host, the eyes sampled and tested in NumPy, one isdf_map_raycast per eye for the line of sight, look_at poses uploaded to
isdf_view_gain, the rows sorted - its best lists compared with the call's.  Writes one JSON record (default
profiles/view_candidates_bench.json)."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "view_candidates_bench.json"))
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--dim", type=int, default=256)
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
_, kinfo = eng.map_known()
offsets = E.view_ring_offsets((0.5, 1.0, 1.5), 16, (-0.3, 0.0, 0.3))
record = {"map": list(dims), "resolution": res, "points": int(len(cloud)), "repeats": args.repeats, "warmup": args.warmup, "offsets": int(len(offsets)),
          "max_range_m": args.max_range, "n_known": int(kinfo.n_known), "series": []}
kept26 = None
for conn in (26, 6):
    _, _, rows, cinfo = eng.map_frontier_clusters(connectivity=conn)
    targets = E.cluster_points(rows, bmin, res, dims)[1]
    for stride in (8, 4):
        ms = []
        for _ in range(total):
            out, w = timed(lambda: eng.view_candidates(cam, targets, offsets, stride=stride, max_range_m=args.max_range))
            ms.append((w, out[4].filter_ms, out[4].gain_ms, out[4].select_ms))
        ms = np.array(ms)[args.warmup:]
        again = eng.view_candidates(cam, targets, offsets, stride=stride, max_range_m=args.max_range)
        info = out[4]
        record["series"].append({"connectivity": conn, "targets": int(len(targets)), "candidates": int(info.n_candidates), "stride": stride,
                                 "counts": {w: int(getattr(info, w)) for w in ("n_kept", "n_bad", "n_occupied", "n_unknown", "n_close", "n_blocked")},
                                 "chunks": int(info.chunks), "best_target": int(info.best_target), "best_candidate": int(info.best_candidate),
                                 "best_gain": int(info.best_gain), "filter_ms": stat(ms[:, 1]), "gain_ms": stat(ms[:, 2]), "select_ms": stat(ms[:, 3]),
                                 "wall_ms": stat(ms[:, 0]), "two_calls_same_bytes": bool(all(a.tobytes() == b.tobytes() for a, b in zip(out[:4], again[:4])))})
        print(json.dumps(record["series"][-1]), flush=True)
        if conn == 26 and stride == 8:
            kept26 = (targets, out)


# ---- the way without the call: connectivity 26, stride 8, the call's defaults (clearance 1, k_best 3, min_gain 1)
def without(targets):
    k = E.known_unpack(eng.map_known()[0], dims)
    o8 = eng.get_grid(capi.GRID_OCCUPANCY)[0]
    no = len(offsets)
    tgt = np.repeat(targets, no, axis=0)
    eye = tgt + np.tile(offsets, (len(targets), 1))
    qe, inside = E._raycast_ticks(eye, bmin, bmax, res, dims)
    vt = E._raycast_ticks(tgt, bmin, bmax, res, dims)[0] >> 10
    ve = qe >> 10
    poses, index = [], []
    for c in np.flatnonzero(inside):
        v = tuple(int(a) for a in ve[c])
        box = tuple(slice(max(a - 1, 0), min(a + 1, m - 1) + 1) for a, m in zip(v, dims))
        if o8[box].any() or not k[box].all():
            continue
        row, _ = eng.map_raycast(eye[c], tgt[c].astype(np.float32).reshape(1, 3), test_origin_voxel=False)       # one ray at a time
        if row[0, 0] == 1 and (row[0, 2:5] != vt[c]).any():
            continue
        poses.append(E.look_at(eye[c], tgt[c])); index.append(c)
    best = np.full((len(targets), 3), -1, dtype=np.int64)
    if index:
        g, _ = eng.view_gain(cam, np.array(poses), stride=8, max_range_m=args.max_range)
        index, gain = np.array(index), g[:, 1]
        for i in range(len(targets)):
            q = np.flatnonzero((index // no == i) & (gain >= 1))
            q = q[np.lexsort((index[q], -gain[q]))][:3]
            best[i, :len(q)] = index[q]
    return best, len(index)


targets, out = kept26
ms = []
for _ in range(total):                                              # the call's protocol: the same warm-up and timed calls
    (best, n_kept), w = timed(lambda: without(targets))
    ms.append(w)
ms = ms[args.warmup:]
record["without_the_call"] = {"connectivity": 26, "stride": 8, "warmup": args.warmup, "calls": args.repeats, "wall_ms": stat(ms), "wall_ms_per_kept_view": float(np.median(ms)) / max(n_kept, 1),
                              "n_kept": int(n_kept), "n_kept_equals_the_calls": bool(n_kept == out[4].n_kept), "best_lists_equal_the_calls": bool(np.array_equal(best, out[3]))}
print(json.dumps(record["without_the_call"]), flush=True)
record["counters"] = "none collected: nothing is known about what bounds the kernels"
os.makedirs(os.path.dirname(args.out), exist_ok=True)
json.dump(record, open(args.out, "w"), indent=1)
