#!/usr/bin/env python
"""Developer tool: the frontier clusters (csrc/frontier_cluster.hip) on the scene of tools/map_known_bench.py - a 256 x 256 x 256 map at
0.1 m, seeded boxes, 12 % occupied, the 640 x 480 camera of tests/golden/camera.yaml in a free pocket at the middle, ONE image integrated
with the known grid's mode on.  Records isdf_map_frontier_clusters at connectivity 6 and 26 (the exact-capacity call: wall time and the
three stage times), isdf_known_clusters_host on the same set, and isdf_map_frontier with the list.  3 warm-up and 9 timed calls by
default, median [min, max] in ms.  Writes one JSON record (default profiles/frontier_cluster_bench.json).
--root DIR --frontier-only: the package and the library of ANOTHER tree (the parent commit, built in the same session), isdf_map_frontier
alone - the calls a tree without the clusters has.  --parent-json: the record such a run wrote; its isdf_map_frontier row is recorded
next to this tree's with the verdict: this tree's median inside the parent's [min, max] or not."""
import argparse, json, os, sys, time
import numpy as np
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(HERE, "profiles", "frontier_cluster_bench.json"))
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--dim", type=int, default=256)
ap.add_argument("--max-range", type=float, default=10.0)
ap.add_argument("--root", default=HERE)
ap.add_argument("--frontier-only", action="store_true")
ap.add_argument("--parent-json", default=None)
args = ap.parse_args()
ROOT = os.path.abspath(args.root)
sys.path.insert(0, ROOT)
import __graft_entry__ as graft
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
record = {"map": list(dims), "resolution": res, "points": int(len(cloud)), "repeats": args.repeats, "warmup": args.warmup, "tree": ROOT == HERE and "this" or "other"}


def timed(fn):
    t0 = time.perf_counter(); out = fn(); return out, (time.perf_counter() - t0) * 1e3


eng = pkg.Engine(synth.default_config(capi.V1_SWEPT))
eng.map_known_enable(True)
eng.set_pointcloud(cloud, res, 1, bmin, bmax)
image, _ = eng.depth_render(cam, pose, None)
eng.integrate_depth(cam, pose, image, **rp)


def frontier_row():
    rows = []
    for _ in range(total):
        (_, vox, finfo), w = timed(lambda: eng.map_frontier())
        rows.append((w, finfo.kernel_ms))
    rows = np.array(rows)[args.warmup:]
    return {"wall_ms": stat(rows[:, 0]), "kernel_ms": stat(rows[:, 1]), "n_frontier": int(finfo.n_frontier)}


record["frontier_with_list"] = frontier_row()
print(json.dumps({"frontier_with_list": record["frontier_with_list"]}), flush=True)
if not args.frontier_only:
    import ctypes as C
    bits = eng.map_frontier()[0]
    for conn in (6, 26):
        p = capi.IsdfFrontierClusterParams(conn, 0, 1)
        info = capi.IsdfFrontierClusterInfo()
        eng._check(eng.lib.isdf_map_frontier_clusters(eng.h, None, C.byref(p), None, None, 0, None, 0, C.byref(info)))        # the sizing call
        n, r = int(info.n_voxels), int(info.n_rows)
        vox, labels, out = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int32), np.zeros((r, capi.FRONTIER_CLUSTER_ROW), dtype=np.int64)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)                # noqa: E731
        rows = []
        for _ in range(total):                                      # the exact-capacity call: everything comes back
            rc, w = timed(lambda: eng.lib.isdf_map_frontier_clusters(eng.h, None, C.byref(p), ptr(vox), ptr(labels), n, ptr(out), r, C.byref(info)))
            eng._check(rc)
            rows.append((w, info.frontier_ms, info.label_ms, info.stats_ms))
        rows = np.array(rows)[args.warmup:]
        sizing = [timed(lambda: eng.lib.isdf_map_frontier_clusters(eng.h, None, C.byref(p), None, None, 0, None, 0, C.byref(info)))[1] for _ in range(total)][args.warmup:]
        host = []
        for _ in range(max(args.repeats // 3, 1)):
            hout, w = timed(lambda: E.known_clusters_host(bits, dims, conn, 1))
            host.append(w)
        same = all(np.array_equal(a, b) for a, b in zip((vox, labels, out), hout[:3]))
        record[f"clusters_{conn}"] = {"wall_ms": stat(rows[:, 0]), "frontier_ms": stat(rows[:, 1]), "label_ms": stat(rows[:, 2]), "stats_ms": stat(rows[:, 3]),
                                      "sizing_call_wall_ms": stat(sizing), "host_form_wall_ms": stat(host), "host_form_calls": len(host), "host_form_same_bytes": bool(same),
                                      "n_voxels": n, "n_clusters": int(info.n_clusters), "largest_size": int(info.largest_size)}
        print(json.dumps({f"clusters_{conn}": record[f"clusters_{conn}"]}), flush=True)
    record["frontier_with_list_after"] = frontier_row()             # once more after the cluster calls: the same series, later in the session
if args.parent_json:
    par = json.load(open(args.parent_json))["frontier_with_list"]["wall_ms"]
    here = record["frontier_with_list"]["wall_ms"]
    record["parent_commit"] = {"frontier_with_list_wall_ms": par, "tool": "this tool with --root <parent tree> --frontier-only, same session",
                               "median_inside_parent_min_max": bool(par["min"] <= here["median"] <= par["max"])}
    print(json.dumps(record["parent_commit"]), flush=True)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
json.dump(record, open(args.out, "w"), indent=1)
