#!/usr/bin/env python
"""Developer tool: how far the tile sweep's fp32 pre-filter value is from the fp64 SDF, per analytic kind - the number behind
TS_FILTER_EPS (tile_sweep.hip).  The filter's value cannot be read back, but its decision can: a one-piece hover at a voxel centre
(identity attitude, identity body offset: the body-frame point is an exact multiple of the voxel size in fp32 and fp64 alike) over a
map with ONE occupied voxel makes stats()["pairs"] 2 or 0 as the filter keeps or rejects that voxel, i.e. as
sdf32 < (float)safety_hor + TS_FILTER_EPS or not.  Bisecting safety_hor brackets sdf32 to one fp32 ulp; the oracle gives the fp64
value at the same point.  Voxels: per shape up to 10 on the body's axes and planes (a zero coordinate: the singular sets) and 6 more,
those with an SDF nearest 0.5 m.  Prints one line per shape and a table per kind."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import __graft_entry__ as graft
pkg = graft.load_package(); orc = graft.load_oracle(); capi, synth = pkg.capi, pkg.synth

EPS = np.float32(2e-3)          # TS_FILTER_EPS
S40, C40 = float(np.sin(40.0)), float(np.cos(40.0))
THIN = {"Torus": (2.5, 0.02), "Cappedtorus": (S40, C40, 3.5, 0.02), "CappedCone": (0.02, 0.01, 0, 0, -1, 0, 0, 1), "RoundedCone": (0.02, 0.01, 3.0),
        "WireframeBox": (1.8, 2.5, 3.5, 0.02), "BendLinear": (2.0, 0.02), "TwistBox": (2.0, 2.0, 0.02, np.pi / 6), "BendBox": (2.0, 2.0, 0.02, 0.5),
        "Table": (0.0, 0.0, 0.0, 3.5, 1.75, 0.02, 2.8, 1.05, 0.0, 2.82, 1.07, 2.8), "Trefoil": (3.5, 0.02, 0.02, 0.005, 0.4), "Ball": (0.02,)}
KINDS = ["Torus", "Cappedtorus", "CappedCone", "RoundedCone", "WireframeBox", "BendLinear", "TwistBox", "BendBox", "Table", "Trefoil",
         "SmoothDifference", "SmoothIntersection", "CSG", "Ball"]          # (Box: its filter is compiled out)
res, n, ks = 0.5, 24, 17
pos = (np.array([12, 12, 12]) + 0.5) * res
T = np.array([1.0]); Cf = np.zeros((6, 3)); Cf[0] = pos; cm = synth.colmajor(Cf)


def thr32(t):
    return np.float32(np.float32(np.float32(t) * np.float32(1.0)) + EPS)


def kept(shape, idx, t):
    occ = np.zeros((n, n, n), dtype=np.uint8); occ[12 + idx[0], 12 + idx[1], 12 + idx[2]] = 1
    cfg = synth.default_config(capi.V2_OCC_TILE, kernel_size=ks, integral_intervs=1, safety_hor=float(t), enable_dyn=0)
    e = pkg.Engine(cfg); e.set_grid(occ, (0, 0, 0), res, capi.GRID_OCCUPANCY); e.set_shape(shape)
    e.eval_single(T, cm); p = e.stats()["pairs"]; e.close()
    assert p in (0, 2), p
    return p == 2


worst = {}
t_all = time.time()
for name in KINDS:
    for params in [None] + ([THIN[name]] if name in THIN else []):
        shape = synth.make_shape(name, params=params)
        k = np.arange(-(ks // 2), ks // 2 + 1)
        I = np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3)
        o = orc.Oracle(synth.default_config(capi.V2_OCC_TILE)); o.set_shape(shape)
        s, _ = o.shape_eval(I * res)
        ok = np.isfinite(s) & (s > 0.05) & (s < 2.0)
        onset = ok & (I == 0).any(axis=1)
        order = np.argsort(np.abs(s - 0.5))
        pick = [i for i in order if onset[i]][:10] + [i for i in order if ok[i] and not onset[i]][:6]
        diffs = []
        for i in pick:
            lo, hi = s[i] - float(EPS) - 3e-3, s[i] - float(EPS) + 3e-3          # rejected at lo, kept at hi if |sdf32 - sdf64| < 3 mm
            if kept(shape, I[i], lo) or not kept(shape, I[i], hi):
                print(f"  {name} {I[i] * res}: fp32 and fp64 differ by more than 3 mm (or the fp32 value is a NaN): sdf64 {s[i]:.6f}", flush=True)
                diffs.append(np.inf); continue
            for _ in range(18):
                mid = 0.5 * (lo + hi)
                if kept(shape, I[i], mid): hi = mid
                else: lo = mid
            s32 = 0.5 * (float(thr32(lo)) + float(thr32(hi)))                       # thr32(lo) <= sdf32 < thr32(hi)
            diffs.append(s32 - s[i])
        d = np.abs(np.array(diffs))
        j = int(np.argmax(d))
        print(f"{name:18s} {'default' if params is None else 'thin   '} {len(pick):2d} voxels: max |sdf32 - sdf64| = {d[j]:.2e} m at {I[pick[j]] * res} (sdf64 {s[pick[j]]:.4f}), "
              f"median {np.median(d):.1e}   [{time.time() - t_all:.0f} s]", flush=True)
        worst[name] = max(worst.get(name, 0.0), float(d[j]))
print("\n| kind | largest fp32 - fp64 difference seen (m) |\n|---|---|")
for name, v in worst.items():
    print(f"| {name} | {v:.1e} |")
