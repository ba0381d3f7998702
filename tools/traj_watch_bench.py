#!/usr/bin/env python
"""Developer tool: the kept clearance report folded by a map update (isdf_traj_check_set_watch mode 1) against what a user has without
it - the same update with the watch off, followed by isdf_traj_check on the updated map.  The 256 x 256 x 64 map at 0.2 m and the
rounded-cone robot of DESIGN 4.8's first row (tools/traj_check_bench.py), frames of DESIGN 4.14's three box sizes (about a quarter of
the voxels of a cube of 8^3, 16^3, 32^3 voxels) placed along the trajectory's corridor.  Two contexts take the same frames: A with
the watch on, B with it off.  Per frame: the fold's four device times, the update's wall time on A and on B, the wall time of the
full check on B; the two reports are compared field by field and row by row every frame.  Medians [min, max] of --repeats frames
after --warmup.  Writes one JSON record (default profiles/traj_watch_bench.json)."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as graft

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "traj_watch_bench.json"))
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--warmup", type=int, default=3)
args = ap.parse_args()
pkg = graft.load_package(); capi, synth = pkg.capi, pkg.synth
res, dims, safety, N = 0.2, (256, 256, 64), 0.5, 20
bmin, bmax = np.zeros(3), np.array(dims) * res
occ = synth.random_box_map(dims, res=res, occupancy=0.12, seed=12345)
base = ((np.argwhere(occ == 1) + 0.5) * res).astype(np.float32)          # one point per occupied voxel, sta_threshold 1
T, Cf = synth.random_trajectory(np.array(dims) * res, N, seed=780, piece_T=1.0, jitter=0.5, margin=4.0, occ=occ, res=res)
cm = synth.colmajor(Cf)
starts = np.asarray(cm).reshape(3, N, 6)[:, :, 0].T                      # where each piece begins
stat = lambda v: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}      # noqa: E731
TIMES = ("select_ms", "field_ms", "reduce_ms")


def engine(watch):
    eng = pkg.Engine(synth.default_config(capi.V1_SWEPT, safety_hor=safety))
    eng.set_pointcloud(base, res, 1, bmin, bmax)
    eng.set_shape(synth.make_shape("RoundedCone", params=(0.8, 0.3, 1.6), bound_radius=1.9))
    eng.traj_check_set_watch(1 if watch else 0)
    eng.traj_check(T, cm)
    return eng


def frames(s, n, rng):
    """n frames: about a quarter of the voxels of a cube of s^3 voxels centred on the start of pieces 1, 2, ... of the trajectory"""
    out = []
    for i in range(n):
        lo = np.clip(np.floor(starts[1 + i % (N - 1)] / res).astype(np.int64) - s // 2, 0, np.array(dims) - s)
        cells = np.argwhere(rng.random((s, s, s)) < 0.25) + lo
        out.append(((cells + 0.5) * res).astype(np.float32))
    return out


record = {"map": list(dims), "resolution": res, "robot": "rounded cone (0.8, 0.3, 1.6), bound 1.9 m", "pieces": N, "base_points": int(len(base)),
          "repeats": args.repeats, "warmup": args.warmup, "frames": []}
rng = np.random.default_rng(1)
for s in (8, 16, 32):
    a, b = engine(True), engine(False)
    rows = []
    for f in frames(s, args.warmup + args.repeats, rng):
        t0 = time.perf_counter(); ia = a.update_pointcloud(f); wall_on = (time.perf_counter() - t0) * 1e3
        rep, last = a.traj_check_watch_info(N)
        t0 = time.perf_counter(); ib = b.update_pointcloud(f); wall_off = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter(); want = b.traj_check(T, cm); wall_check = (time.perf_counter() - t0) * 1e3
        assert ia.n_new_voxels == ib.n_new_voxels and last["path"] == 1 and last["new_voxels"] == ia.n_new_voxels
        same = all(np.array_equal(np.asarray(rep[k]), np.asarray(want[k])) for k in want if k not in TIMES)
        same = same and a.traj_check_points().tobytes() == b.traj_check_points().tobytes()
        assert same, "the folded report differs from the full check"
        rows.append((wall_on, wall_off, wall_check, last["select_ms"], last["field_ms"], last["reduce_ms"], last["merge_ms"], last["new_voxels"],
                     last["new_candidates"], last["new_below_margin"], want["select_ms"], want["field_ms"], want["reduce_ms"], want["candidates"]))
    r = np.array(rows)[args.warmup:]
    row = {"box": s, "update_wall_ms_watch_on": stat(r[:, 0]), "update_wall_ms_watch_off": stat(r[:, 1]), "full_check_wall_ms": stat(r[:, 2]),
           "baseline_wall_ms": stat(r[:, 1] + r[:, 2]), "fold_wall_ms": stat(r[:, 0] - r[:, 1]),
           "fold_select_ms": stat(r[:, 3]), "fold_field_ms": stat(r[:, 4]), "fold_reduce_ms": stat(r[:, 5]), "fold_merge_ms": stat(r[:, 6]),
           "new_voxels": stat(r[:, 7]), "new_candidates": stat(r[:, 8]), "new_below_margin": stat(r[:, 9]),
           "full_check_select_ms": stat(r[:, 10]), "full_check_field_ms": stat(r[:, 11]), "full_check_reduce_ms": stat(r[:, 12]),
           "full_check_candidates": stat(r[:, 13]),
           "baseline_over_watch_on": float(np.median(r[:, 1] + r[:, 2]) / np.median(r[:, 0])),
           "full_check_over_fold": float(np.median(r[:, 2]) / max(np.median(r[:, 0] - r[:, 1]), 1e-9)), "equal_to_full_check": True}
    record["frames"].append(row)
    print(json.dumps(row), flush=True)
    a.close(); b.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
json.dump(record, open(args.out, "w"), indent=1)
print("wrote", args.out)
