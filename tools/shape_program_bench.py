#!/usr/bin/env python
"""Developer tool: what the interpreter of ISDF_SHAPE_PROGRAM costs against the built-in kind it restates, in the same process.
For CSG and RoundedCone (class constants): the step time of the V3 sweep on the 40-piece trajectory of BASELINE configs[1] and of the
V1 sweep on its 7 773-point workload, each as the median of 5 steps after a warm-up, with the built-in kind and with
csg.reference_class(name) installed.  The baseline is the built-in kind of the same run; no ratio is expected or checked.
Writes profiles/shape_program_bench.json."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402
from benchlib.workloads import build_workload  # noqa: E402


def median_ms(step, warmup=2, reps=5):
    for _ in range(warmup):
        step()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        step()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), ts


def main():
    pkg = graft.load_package()
    capi, synth, csg = pkg.capi, pkg.synth, pkg.csg
    res, N = 0.2, 40
    occ, esdf, T, cm = build_workload(pkg, N, 256, res)
    way = cm.reshape(3, -1).T.reshape(N, 6, 3)[1:, 0, :]
    cfg3 = synth.default_config(capi.V3_ESDF_TILE, kernel_size=21, integral_intervs=64, safety_hor=(3 ** 0.5 / 2) * res, weight_p=4000.0,
                                smoothing_eps=0.01, enable_dyn=1, enable_pos=1)
    cfg1 = synth.default_config(capi.V1_SWEPT, safety_hor=(3 ** 0.5 / 2) * res, weight_p=4000.0)
    out = {"workload": "BASELINE configs[1]: 256^3 map at 0.2 m, one 40-piece trajectory; V3: 65 samples per piece, kernel_size 21; "
                       "V1: the points isdf_gather_points collects around its waypoints (half 1.4 m)",
           "timing": "host wall clock of Engine.eval_single (isdf_eval), median of 5 steps after 2 warm-up steps, milliseconds", "shapes": {}}
    for name in ("CSG", "RoundedCone"):
        tree = csg.reference_class(name)
        row = {}
        for kind, install in (("builtin", lambda e: e.set_shape(synth.make_shape(name))), ("program", lambda e: e.set_shape_program(tree))):
            e3 = pkg.Engine(cfg3); e3.set_grid(esdf, (0, 0, 0), res, capi.GRID_ESDF); install(e3)
            m3, all3 = median_ms(lambda: e3.eval_single(T, cm))
            c3 = e3.eval_single(T, cm)[0]
            e1 = pkg.Engine(cfg1); e1.set_grid(occ, (0, 0, 0), res, capi.GRID_OCCUPANCY); install(e1)
            M = e1.gather_points(way, 1.4)
            ts = np.zeros(M)
            m1, all1 = median_ms(lambda: e1.eval_single(T, cm, tstar=ts))
            c1 = e1.eval_single(T, cm, tstar=ts)[0]
            row[kind] = {"v3_ms": m3, "v3_all_ms": all3, "v3_cost": c3, "v3_grad_pairs": int(e3.stats()["grad_pairs"]),
                         "v1_ms": m1, "v1_all_ms": all1, "v1_cost": c1, "v1_points": int(M)}
            print(f"{name:12s} {kind:8s} V3 {m3:9.3f} ms  V1 {m1:9.3f} ms ({M} points)", flush=True)
            e3.close(); e1.close()
        row["program_over_builtin"] = {"v3": row["program"]["v3_ms"] / row["builtin"]["v3_ms"], "v1": row["program"]["v1_ms"] / row["builtin"]["v1_ms"]}
        out["shapes"][name] = row
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    path = os.environ.get("ISDF_SHAPE_PROGRAM_BENCH_OUT", os.path.join(ROOT, "profiles", "shape_program_bench.json"))
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote " + path)


if __name__ == "__main__":
    main()
