#!/usr/bin/env python
"""Developer tool: the trajectory clearance check (isdf_traj_check) on one GPU against what a user had before it.  Prints ONE JSON line:
per map (the 256 x 256 x 64 map of tools/astar_bench.py at 0.2 m; the 512^3 C5 map of benchlib/configs.py at 0.1 m) and robot
(the C2 rounded cone; the reference's Lthick.obj scaled to a 0.83 m bound):
  check     select_ms / field_ms / reduce_ms (the library's events on the ctx's stream, median of the repeats after a warm-up), the
            wall clock of the whole call, occupied voxels, candidates and their share
  baseline  get_grid + numpy listing of the occupied voxels + Engine.swept_sdf over all of them + numpy reduction, wall clock,
            same process (the mesh robot on the 512^3 map only with --all-baselines: minutes)
usage: tools/traj_check_bench.py [--out profiles/traj_check_bench.json] [--reps 5] [--all-baselines]"""
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
from benchlib.meshes import reference_mesh  # noqa: E402


def baseline(eng, T, cm, margin):
    t0 = time.perf_counter()
    occ, origin, _ = eng.get_grid(capi.GRID_OCCUPANCY)
    res = (eng_res[id(eng)])
    vox = np.flatnonzero(occ.ravel())
    ijk = np.stack(np.unravel_index(vox, occ.shape), axis=1)
    P = (ijk + 0.5) * res + origin
    val, ts = eng.swept_sdf(T, cm, P)
    q = val != 10.0
    out = {"points": int(len(vox)), "qualified": int(q.sum()), "n_below_margin": int((q & (val < margin)).sum()),
           "n_penetrating": int((q & (val < 0)).sum()), "min_clearance": float(val[q].min()) if q.any() else 10.0,
           "min_voxel": int(vox[np.flatnonzero(q)[np.argmin(val[q])]]) if q.any() else -1}
    out["wall_ms"] = (time.perf_counter() - t0) * 1e3
    return out


eng_res = {}


def run(name, occ, res, shape, safety, T, cm, reps, with_baseline):
    cfg = synth.default_config(capi.V1_SWEPT, safety_hor=safety)
    eng = pkg.Engine(cfg)
    eng.set_grid(occ, (0, 0, 0), res, capi.GRID_OCCUPANCY)
    eng.set_shape(shape)
    eng_res[id(eng)] = res
    eng.traj_check(T, cm)                                   # warm-up (allocations of the query's scratch, code objects)
    rows, walls = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = eng.traj_check(T, cm)
        walls.append((time.perf_counter() - t0) * 1e3)
        rows.append(r)
    med = lambda k: float(np.median([r[k] for r in rows]))        # noqa: E731
    r = rows[-1]
    ent = {"name": name, "occupied": int((occ != 0).sum()), "occupied_in_box": r["occupied_in_box"], "candidates": r["candidates"],
           "candidate_share": r["candidates"] / max(1, int((occ != 0).sum())), "qualified": r["qualified"],
           "n_below_margin": r["n_below_margin"], "n_penetrating": r["n_penetrating"], "min_clearance": r["min_clearance"],
           "min_voxel": r["min_voxel"], "select_ms": med("select_ms"), "field_ms": med("field_ms"), "reduce_ms": med("reduce_ms"),
           "check_wall_ms": float(np.median(walls)), "reps": reps}
    if with_baseline:
        baseline(eng, T, cm, safety)                        # warm-up
        b = baseline(eng, T, cm, safety)
        ent["baseline"] = b
        ent["same_report"] = all(b[k] == r[k] for k in ("qualified", "n_below_margin", "n_penetrating", "min_clearance", "min_voxel"))
        ent["speedup_wall"] = b["wall_ms"] / ent["check_wall_ms"]
    else:
        ent["baseline"] = None
    print(json.dumps(ent), file=sys.stderr, flush=True)
    return ent


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--all-baselines", action="store_true")
    args = ap.parse_args()
    cone = synth.make_shape("RoundedCone", params=(0.8, 0.3, 1.6), bound_radius=1.9)
    Vm, Fm = reference_mesh("Lthick", 0.83)
    out = []
    # the front end's bench map
    res = 0.2
    occ = synth.random_box_map((256, 256, 64), res=res, occupancy=0.12, seed=12345)
    ext = np.array(occ.shape) * res
    T, Cf = synth.random_trajectory(ext, 20, seed=780, piece_T=1.0, jitter=0.5, margin=4.0, occ=occ, res=res)
    cm = synth.colmajor(Cf)
    out.append(run("256x256x64 @ 0.2 m, rounded cone (C2)", occ, res, cone, 0.5, T, cm, args.reps, True))
    out.append(run("256x256x64 @ 0.2 m, Lthick.obj (0.83 m bound)", occ, res, synth.make_mesh_shape(Vm, Fm), 0.5, T, cm, args.reps, True))
    # the C5 map
    res = 0.1
    occ = synth.random_box_map((512,) * 3, res=res, occupancy=0.15, seed=12345, edge=(0.4, 2.0))
    ext = np.array(occ.shape) * res
    T, Cf = synth.random_trajectory(ext, 20, seed=780, piece_T=1.0, jitter=0.5, margin=4.0, occ=occ, res=res)
    cm = synth.colmajor(Cf)
    out.append(run("512^3 @ 0.1 m (C5 map), rounded cone (C2)", occ, res, cone, 0.5, T, cm, args.reps, True))
    out.append(run("512^3 @ 0.1 m (C5 map), Lthick.obj (0.83 m bound)", occ, res, synth.make_mesh_shape(Vm, Fm), (3 ** 0.5 / 2) * res, T, cm,
                   args.reps, args.all_baselines))
    line = json.dumps({"tool": "traj_check_bench", "device": torch.cuda.get_device_name(0), "entries": out})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
