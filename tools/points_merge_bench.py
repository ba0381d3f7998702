#!/usr/bin/env python
"""Developer tool: the report merge (isdf_points_merge_check) and the checked optimiser (isdf_optimize_lbfgs_checked) on one GPU.
Prints ONE JSON line: per map (the two rounded-cone rows of tools/traj_check_bench.py: 256 x 256 x 64 at 0.2 m, the 512^3 C5 map at
0.1 m; a 20-piece seeded trajectory, the obstacle points gathered in boxes of 1.4 m half size around its waypoints)
  merge     the merge of one check's rows into the gathered set: merge_ms (the library's events on the ctx's stream) and the wall
            clock of the call, against the path a user had before it - traj_check_points, get_points, de-duplication by voxel id
            in numpy, set_points - wall clock in the same process; medians of the repeats after a warm-up, the set and the report
            restored (untimed) before every repeat
  loop      isdf_optimize_lbfgs_checked from the empty set (lazy) and from the gathered set on the same plan: rounds, the size of the
            set every round optimised with, the final M, the wall clock of a V1 step (isdf_eval) at the final M, total wall clock
usage: tools/points_merge_bench.py [--out profiles/points_merge_bench.json] [--reps 5] [--max-rounds 4] [--iterations 30]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402
import torch  # noqa: E402,F401  (first: tests/conftest.py::_torch_first)

pkg = graft.load_package()
capi, synth = pkg.capi, pkg.synth
SAFETY, HALF, RHO = 0.5, 1.4, 1.0


def engine(occ, res, shape):
    eng = pkg.Engine(synth.default_config(capi.V1_SWEPT, kernel_size=9, integral_intervs=16, safety_hor=SAFETY))
    eng.set_grid(occ, (0, 0, 0), res, capi.GRID_OCCUPANCY)
    eng.generate_esdf()
    eng.set_shape(shape)
    return eng


def voxel_ids(P, dims, res):
    idx = np.minimum(np.floor(P / res).astype(np.int64), np.asarray(dims) - 1)
    ids = (idx[:, 0] * dims[1] + idx[:, 1]) * dims[2] + idx[:, 2]
    ids[~np.all((P >= 0) & (P <= np.asarray(dims) * res), axis=1)] = -1
    return ids


def by_hand(eng, dims, res):
    """the parent commit's path: rows and set to the host, de-duplicate by voxel id, the whole set back (lastTstar starts over)"""
    rows = eng.traj_check_points()
    pts = eng.get_points()
    new = ~np.isin(voxel_ids(rows[:, :3], dims, res), voxel_ids(pts, dims, res))
    eng.set_points(np.concatenate([pts, rows[new, :3]]))
    return int(new.sum())


def med(xs):
    return float(np.median(xs))


def merge_times(eng, dims, res, way, T, cm, reps):
    out = {}
    for name in ("device", "by_hand"):
        walls, dev_ms, added = [], [], 0
        for rep in range(reps + 1):                         # the first is the warm-up
            M = eng.gather_points(way, HALF)
            rep_info = eng.traj_check(T, cm)
            t0 = time.perf_counter()
            if name == "device":
                info = eng.points_merge_check()
                added = info["n_added"]
            else:
                added = by_hand(eng, dims, res)
            w = (time.perf_counter() - t0) * 1e3
            if rep:
                walls.append(w)
                if name == "device":
                    dev_ms.append(info["merge_ms"])
        out[name] = {"wall_ms": med(walls), "n_added": added}
        if name == "device":
            out[name]["merge_ms"] = med(dev_ms)
    out.update(M_gathered=M, n_rows=rep_info["n_below_margin"], same_added=out["device"]["n_added"] == out["by_hand"]["n_added"],
               speedup_wall=out["by_hand"]["wall_ms"] / max(out["device"]["wall_ms"], 1e-9))
    return out


def loop(occ, res, shape, head, tail, way, T, start, reps, max_rounds, iterations):
    eng = engine(occ, res, shape)
    N = len(T)
    if start == "lazy":
        eng.set_points(np.zeros((0, 3)))
    else:
        eng.gather_points(way, HALF)
    eng.set_trajectory(N, head, tail, RHO)
    x0 = eng.pack_variables(T, way)
    eng.cost_function(x0)                                   # warm-up (code objects, the callback's buffers)
    t0 = time.perf_counter()
    x, r = eng.optimize_lbfgs_checked(x0, lbfgs_params=dict(max_iterations=iterations, g_epsilon=0.0, past=0), max_rounds=max_rounds)
    total = (time.perf_counter() - t0) * 1e3
    T1, cm1 = eng.unpack_variables(x)
    M = eng.get_points().shape[0]
    steps = []
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        eng.eval_single(T1, cm1)
        if rep:
            steps.append((time.perf_counter() - t0) * 1e3)
    c = r["last_check"]
    out = {"start": start, "rounds": r["rounds"], "clear": r["clear"], "stalled": r["stalled"], "M_round": r["M_round"], "final_M": M,
           "v1_step_wall_ms": med(steps), "total_wall_ms": total, "n_below_margin": c["n_below_margin"], "n_penetrating": c["n_penetrating"],
           "min_clearance": c["min_clearance"], "lbfgs_status": r["last_opt"]["status"], "cost": r["last_opt"]["f"]}
    eng.close()
    return out


def run(name, occ, res, shape, reps, max_rounds, iterations):
    ext = np.array(occ.shape) * res
    N = 20
    T, Cf = synth.random_trajectory(ext, N, seed=780, piece_T=1.0, jitter=0.5, margin=4.0, occ=occ, res=res)
    cm = synth.colmajor(Cf)
    c = np.asarray(cm).reshape(3, N, 6)
    head = np.zeros((3, 3)); tail = np.zeros((3, 3))
    head[:, 0] = c[:, 0, 0]
    tail[:, 0] = sum(c[:, N - 1, p] * T[-1] ** p for p in range(6))
    way = c[:, 1:, 0].T.copy()
    eng = engine(occ, res, shape)
    ent = {"name": name, "occupied": int((occ != 0).sum()), "reps": reps, "max_rounds": max_rounds, "lbfgs_iterations": iterations,
           "merge": merge_times(eng, occ.shape, res, way, T, cm, reps)}
    eng.close()
    ent["loop"] = [loop(occ, res, shape, head, tail, way, T, s, reps, max_rounds, iterations) for s in ("lazy", "gathered")]
    print(json.dumps(ent), file=sys.stderr, flush=True)
    return ent


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-rounds", type=int, default=4)
    ap.add_argument("--iterations", type=int, default=30)
    args = ap.parse_args()
    cone = synth.make_shape("RoundedCone", params=(0.8, 0.3, 1.6), bound_radius=1.9)
    out = []
    res = 0.2
    occ = synth.random_box_map((256, 256, 64), res=res, occupancy=0.12, seed=12345)
    out.append(run("256x256x64 @ 0.2 m, rounded cone (C2)", occ, res, cone, args.reps, args.max_rounds, args.iterations))
    res = 0.1
    occ = synth.random_box_map((512,) * 3, res=res, occupancy=0.15, seed=12345, edge=(0.4, 2.0))
    out.append(run("512^3 @ 0.1 m (C5 map), rounded cone (C2)", occ, res, cone, args.reps, args.max_rounds, args.iterations))
    line = json.dumps({"tool": "points_merge_bench", "device": torch.cuda.get_device_name(0), "entries": out})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
