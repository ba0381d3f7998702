"""Child process of tests/test_gpu_shape_program.py: a registered class as a PROGRAM against the built-in kind through the V3 and
the V1 sweep, with the bounds given and with zeros.  Run once as it is (the fused launch) and once with ISDF_NO_FUSE=1 (read at
isdf_create).  Prints one JSON object: per class the figures the parent asserts on."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# name -> (bound_radius, (bbox centre, bbox half)): valid for the class constants (sdf(p) >= |p| - R; the shape inside the box)
BOUNDS = {
    "CSG": (3.0, ((0, 0, 0), (2.25, 2.25, 2.25))),
    "RoundedCone": (5.1, ((0, 0, 1.8), (1.5, 1.5, 3.3))),
    "Table": (4.9, ((0, 0, 1.4), (3.5, 1.75, 1.4))),
    "SmoothDifference": (2.2, ((0, 0, 0), (1.5, 1.5, 0.25))),
    "TwistBox": (1.74, ((0, 0, 0), (1.415, 1.415, 1.0))),
}


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(np.asarray(b)), 1e-300))


def main():
    import __graft_entry__ as g
    from common import small_world, traj
    pkg = g.load_package()
    capi, synth, csg = pkg.capi, pkg.synth, pkg.csg
    occ, esdf, res = small_world(pkg)
    T, cm = traj(pkg, occ, res)
    N = T.size
    way = cm.reshape(3, -1).T.reshape(N, 6, 3)[1:, 0, :]
    pts = synth.constraint_points(occ, (0, 0, 0), res, way, half=3.0)
    cfg3 = synth.default_config(capi.V3_ESDF_TILE, kernel_size=9, integral_intervs=16, safety_hor=0.5)
    cfg1 = synth.default_config(capi.V1_SWEPT, safety_hor=0.5)
    out = {}
    for name, (R, bbox) in BOUNDS.items():
        tree = csg.reference_class(name)

        def engines(cfg, v1):
            es = [pkg.Engine(cfg) for _ in range(3)]
            es[0].set_shape(synth.make_shape(name, bound_radius=R, bbox=bbox))
            es[1].set_shape_program(tree, bound_radius=R, bbox=bbox)
            es[2].set_shape_program(tree)
            for e in es:
                if v1: e.set_points(pts)
                else: e.set_grid(esdf, (0, 0, 0), res, capi.GRID_ESDF)
            return es
        r = {}
        v3 = []
        for e in engines(cfg3, False):
            c, gT, gC = e.eval_single(T, cm)
            v3.append((c, gT, gC, e.stats()["grad_pairs"], e.host_path()))
        v1 = []
        for e in engines(cfg1, True):
            ts = np.zeros(len(pts))
            c, gT, gC = e.eval_single(T, cm, tstar=ts)
            v1.append((c, gT, gC, ts))
        for tag, k in (("bounds", 1), ("zeros", 2)):
            r[f"v3_{tag}"] = dict(cost=v3[k][0], cost_ref=v3[0][0], gradT=rel(v3[k][1], v3[0][1]), gradC=rel(v3[k][2], v3[0][2]),
                                  pairs=int(v3[k][3]), pairs_ref=int(v3[0][3]), finite=bool(np.isfinite(v3[k][2]).all()))
            r[f"v1_{tag}"] = dict(cost=v1[k][0], cost_ref=v1[0][0], gradT=rel(v1[k][1], v1[0][1]), gradC=rel(v1[k][2], v1[0][2]),
                                  dt=float(np.abs(v1[k][3] - v1[0][3]).max()), finite=bool(np.isfinite(v1[k][2]).all()))
        r["v3_bounds_vs_zeros"] = dict(cost=v3[1][0], cost_ref=v3[2][0], gradT=rel(v3[1][1], v3[2][1]), gradC=rel(v3[1][2], v3[2][2]), pairs=int(v3[1][3]), pairs_ref=int(v3[2][3]))
        r["v1_bounds_vs_zeros"] = dict(cost=v1[1][0], cost_ref=v1[2][0], gradT=rel(v1[1][1], v1[2][1]), gradC=rel(v1[1][2], v1[2][2]), dt=float(np.abs(v1[1][3] - v1[2][3]).max()))
        r["host_path"] = [int(v[4]) for v in v3]
        out[name] = r
    print("RESULT " + json.dumps(out))


if __name__ == "__main__":
    main()
