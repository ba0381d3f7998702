#!/usr/bin/env python
"""Developer tool: the swept-volume field (isdf_swept_sdf_device) and mesher (isdf_swept_mesh_build) on one GPU.  Prints ONE JSON line:
  field   points/s of both modes on lattice points (0.1 m) around the path - a C2-like trajectory (40 pieces, the bench's rounded
          cone) and demo1's robot (the RoundedCone class with its 120 degree roll) on demo1's initial trajectory (map, front end
          and waypoints of tests/demo_headless.py)
  mesh    build time dense against narrow band (B = 4) with the counts, demo1's robot and trajectory at eps 0.1; one mesh robot
          (demo6's Lthick.obj from the committed fixtures).
usage: tools/swept_mesh_bench.py [--out profiles/swept_mesh_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as graft  # noqa: E402
import torch  # noqa: E402

pkg = graft.load_package()
capi, synth = pkg.capi, pkg.synth
GOLD = os.path.join(ROOT, "tests", "golden", "ref_demo_inputs.npz")


def positions(T, cm, ts):
    N = len(T)
    C6 = np.asarray(cm).reshape(3, 6 * N)
    starts = np.concatenate([[0.0], np.cumsum(T)[:-1]])
    piece = np.clip(np.searchsorted(starts, ts, side="right") - 1, 0, N - 1)
    tl = ts - starts[piece]
    out = np.zeros((len(ts), 3))
    for a in range(3):
        c = C6[a].reshape(N, 6)[piece]
        out[:, a] = ((((c[:, 5] * tl + c[:, 4]) * tl + c[:, 3]) * tl + c[:, 2]) * tl + c[:, 1]) * tl + c[:, 0]
    return out


def tube_lattice(T, cm, radius, h=0.1, cap=2_000_000):
    """lattice points (spacing h) within `radius` of the path, at most `cap` of them (lattice order)"""
    from scipy.spatial import cKDTree
    path = positions(T, cm, np.linspace(0.0, T.sum(), 20000))
    tree = cKDTree(path)
    lo, hi = path.min(0) - radius, path.max(0) + radius
    xs = [np.arange(lo[a], hi[a] + h, h) for a in range(3)]
    out, n = [], 0
    for x in xs[0]:
        g = np.stack(np.meshgrid([x], xs[1], xs[2], indexing="ij"), axis=-1).reshape(-1, 3)
        d, _ = tree.query(g, distance_upper_bound=radius)
        sel = g[np.isfinite(d)]
        out.append(sel); n += sel.shape[0]
        if n >= cap:
            break
    return np.concatenate(out)[:cap]


def field_rate(eng, T, cm, P, mode, reps=3):
    st = torch.cuda.current_stream().cuda_stream
    dT = torch.tensor(T, dtype=torch.float64, device="cuda"); dC = torch.tensor(np.asarray(cm).reshape(-1), dtype=torch.float64, device="cuda")
    dP = torch.tensor(P, dtype=torch.float64, device="cuda")
    dv = torch.empty(P.shape[0], dtype=torch.float64, device="cuda"); dt = torch.empty_like(dv)
    eng.swept_sdf_device(len(T), dT.data_ptr(), dC.data_ptr(), dP.data_ptr(), P.shape[0], dv.data_ptr(), dt.data_ptr(), mode, st)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        eng.swept_sdf_device(len(T), dT.data_ptr(), dC.data_ptr(), dP.data_ptr(), P.shape[0], dv.data_ptr(), dt.data_ptr(), mode, st)
        ts.append(time.perf_counter() - t0)      # (the call synchronises the stream)
    v = dv.cpu().numpy()
    return {"points": int(P.shape[0]), "points_per_s": float(P.shape[0] / np.median(ts)), "ms": 1e3 * float(np.median(ts)),
            "qualified": int((v < 10.0).sum())}


def mesh_case(eng, T, cm, eps, band):
    eng.swept_mesh(T, cm, eps, band=band)            # warm-up (allocations, code objects)
    t0 = time.perf_counter()
    V, F, info = eng.swept_mesh(T, cm, eps, band=band)
    wall = time.perf_counter() - t0
    return {"band": band, "eps": eps, "wall_ms": 1e3 * wall, "field_ms": info["field_ms"], "mesh_ms": info["mesh_ms"],
            "dims": info["dims"], "coarse_points": info["coarse_points"], "fine_points": info["fine_points"],
            "band_cells": info["band_cells"], "vertices": info["n_vertices"], "triangles": info["n_triangles"],
            "unqualified_edges": info["unqualified_edges"]}, (V, F)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {"tool": "swept_mesh_bench", "device": torch.cuda.get_device_name(0)}
    # ---- C2-like: 40 pieces of 1 s through a 51.2 m cube, the bench's rounded cone
    T, Cf = synth.random_trajectory(np.full(3, 51.2), 40, seed=777, piece_T=1.0, jitter=0.5, margin=4.0)
    cm = synth.colmajor(Cf)
    cfg = synth.default_config(capi.V1_SWEPT, safety_hor=0.5)
    eng = pkg.Engine(cfg); shape = synth.bench_rounded_cone_shape(); eng.set_shape(shape)
    P = tube_lattice(T, cm, shape.bound_radius + 1.2)
    res["field_c2"] = {m: field_rate(eng, T, cm, P, v) for m, v in (("planner", capi.SWEPT_FIELD_PLANNER), ("closed", capi.SWEPT_FIELD_CLOSED))}
    # ---- demo1: RoundedCone (1.5, 0.6, 4.5) with poly_params [0 0 0 120 0 0], the plan's initial trajectory
    from demo_headless import build_plan, plan_config_from_golden
    g = np.load(GOLD)
    plan = plan_config_from_golden(pkg, g, "CappedCone")
    shape1 = pkg.fixtures.shape_from_config(plan, "")
    shape1.bound_radius = 4.5 + 0.6
    cfg1 = capi.IsdfConfig.from_buffer_copy(plan.sweep)
    eng1 = pkg.Engine(cfg1); eng1.set_shape(shape1)
    Pl = build_plan(pkg, eng1, plan, g["CappedCone_xyz"], (5, 25, 17), (48, 25, 17))
    T1, cm1 = eng1.unpack_variables(Pl["x0"])
    P1 = tube_lattice(T1, cm1, shape1.bound_radius + 2 * cfg1.safety_hor + 0.1)
    res["field_demo1"] = {m: field_rate(eng1, T1, cm1, P1, v) for m, v in (("planner", capi.SWEPT_FIELD_PLANNER), ("closed", capi.SWEPT_FIELD_CLOSED))}
    res["field_demo1"]["pieces"] = int(len(T1)); res["field_demo1"]["duration_s"] = float(T1.sum())
    dense, md = mesh_case(eng1, T1, cm1, 0.1, 0)
    band, mb = mesh_case(eng1, T1, cm1, 0.1, 4)
    res["mesh_demo1"] = {"dense": dense, "band": band, "identical": bool(np.array_equal(md[0], mb[0]) and np.array_equal(md[1], mb[1]))}
    # ---- mesh robot: demo6's Lthick.obj (safety_hor 0.6 of config_L.yaml) on the first 10 pieces of the C2-like trajectory
    cfgm = synth.default_config(capi.V1_SWEPT, safety_hor=0.6)
    engm = pkg.Engine(cfgm); engm.set_shape(synth.make_mesh_shape(g["Lthick_V"], g["Lthick_F"]))
    N10 = 10
    cm10 = np.asarray(cm).reshape(3, 6 * 40)[:, :6 * N10].reshape(-1)
    res["mesh_lthick"], _ = mesh_case(engm, T[:N10], cm10, 0.1, 4)
    line = json.dumps(res, separators=(",", ":"))
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
