#!/usr/bin/env python
"""Developer tool: the eroded known grid (csrc/known_erode.hip) and the cost-to-go field gated by it (csrc/frontend_field.hip) on the scene
of tools/map_known_bench.py - a 256 x 256 x 256 map at 0.1 m, seeded boxes, 12 % occupied, the 640 x 480 camera of
tests/golden/camera.yaml in a free pocket at the middle, K as one integrated image leaves it and the pocket declared known -, with the field benches' robot and front
end (kernel_size 21, so the default radius is 10).  For the radii 1, 3 and -1: 3 warm-up and 9 timed calls by default, median [min, max]
of erode_ms, of the gated build's device_ms and, in the same session, of the ungated build's device_ms towards the same goal (the
camera's cell).  --plain-only: the ungated build alone, for comparing two builds of the library (ISDF_ACCEL_LIB) in one session.
Writes one JSON record (default profiles/known_gate_bench.json)."""
import argparse, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "known_gate_bench.json"))
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--dim", type=int, default=256)
ap.add_argument("--plain-only", action="store_true")
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

eng = pkg.Engine(synth.default_config(capi.V1_SWEPT))
eng.set_pointcloud(cloud, res, 1, bmin, bmax)
eng.map_known_enable(True)
image, _ = eng.depth_render(cam, pose, None)
eng.integrate_depth(cam, pose, image, **rp)
eng.map_known_fill(tuple(int(m) - 6 for m in mid) + tuple(int(m) + 6 for m in mid), 1)     # no ray starts inside the robot: its pocket is declared known
eng.set_shape(synth.bench_box_shape())
eng.frontend_build(capi.frontend_config(kernel_size=21, max_roll=45.0, max_pitch=45.0, ang_res=9.0, safeh=0.0))
eng.frontend_cspace(download=False)
_, kinfo = eng.map_known()
record = {"map": list(dims), "resolution": res, "points": int(len(cloud)), "repeats": args.repeats, "warmup": args.warmup, "n_known": int(kinfo.n_known),
          "library": os.environ.get("ISDF_ACCEL_LIB", capi.LIB_PATH), "goal": [float(v) for v in t], "series": []}


def plain():
    ms = []
    for _ in range(total):
        info = eng.frontend_field_build(t)
        ms.append(info.device_ms)
    return {"device_ms": stat(ms[args.warmup:]), "reachable": int(info.reachable), "free_voxels": int(info.free_voxels), "reached_voxels": int(info.reached_voxels),
            "rounds": int(info.rounds)}


if args.plain_only:
    record["ungated_build"] = plain()
    print(json.dumps(record["ungated_build"]), flush=True)
else:
    for radius in (1, 3, -1):
        for border in (0, 1):
            er, gb = [], []
            for _ in range(total):
                _, einfo = eng.known_erode(radius, border, want_bits=False)
                er.append(einfo.erode_ms)
            for _ in range(total):
                info, gate = eng.frontend_field_build_known(t, radius, border)
                gb.append((info.device_ms, gate.erode_ms))
            gb = np.array(gb)[args.warmup:]
            record["series"].append({"radius": radius, "radius_used": int(einfo.radius_used), "border": border, "known_voxels": int(einfo.known_voxels),
                                     "eroded_voxels": int(einfo.eroded_voxels), "erode_ms": stat(er[args.warmup:]), "gated_build_device_ms": stat(gb[:, 0]),
                                     "gated_build_erode_ms": stat(gb[:, 1]), "reachable": int(info.reachable), "free_voxels": int(info.free_voxels),
                                     "reached_voxels": int(info.reached_voxels), "rounds": int(info.rounds), "ungated_build_same_session": plain()})
            print(json.dumps(record["series"][-1]), flush=True)
    record["counters"] = "none collected: nothing is known about what bounds the erosion's kernel"
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
json.dump(record, open(args.out, "w"), indent=1)
