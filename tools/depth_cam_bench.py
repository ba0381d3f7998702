#!/usr/bin/env python
"""Developer tool: the depth camera on the device (isdf_depth_render*, isdf_depth_rays, isdf_integrate_depth) at the reference's camera
(tests/golden/camera.yaml, 640 x 480) in a 256 x 256 x 256 map at 0.1 m: seeded boxes, 12 % occupied, the camera in a free pocket near
the middle, one point per occupied voxel as the cloud.  Records the render from the cloud (already on the device) and from the map with
max_splat_px 0 and 32, the unprojection, isdf_integrate_depth against the same work done as isdf_depth_rays_host + isdf_integrate_scan,
the render against engine.scan_from_map on a pixel grid, and the host form's time.  Median [min, max] after warm-up.  After each series the
device's image is compared with the host form's.  --lib: another build of the library (csrc/Makefile EXTRA=-DISDF_DC_WAVE_AREA=...), with
--render-only for the A/B of the render kernel.  Writes one JSON record (default profiles/depth_cam_bench.json)."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_cam_bench.json"))
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--dim", type=int, default=256)
ap.add_argument("--max-range", type=float, default=10.0)
ap.add_argument("--lib", default=None)
ap.add_argument("--render-only", action="store_true")
args = ap.parse_args()
import torch                                                        # before the library touches the device (tests/conftest.py says why)
torch.zeros(1, device="cuda")
pkg = graft.load_package(); capi, synth, E = pkg.capi, pkg.synth, pkg.engine
lib = capi.load_library(args.lib) if args.lib else capi.load_library()
res, dims = 0.1, (args.dim,) * 3
bmin, bmax = np.zeros(3), np.array(dims) * res
stat = lambda v: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}      # noqa: E731

occ = synth.random_box_map(dims, res=res, occupancy=0.12, seed=12345)
mid = np.array(dims) // 2
occ[tuple(slice(m - 6, m + 7) for m in mid)] = 0                    # the camera's pocket
cloud = np.ascontiguousarray(((np.argwhere(occ == 1) + 0.5) * res).astype(np.float32))       # one point per occupied voxel, sta_threshold 1
cam = E.camera_from_yaml(os.path.join(ROOT, "tests", "golden", "camera.yaml"))
t = (mid + 0.5) * res + np.array([0.03, -0.02, 0.01])
pose = np.concatenate([np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]]), t.reshape(3, 1)], axis=1).reshape(12)        # looking along +x

eng = pkg.Engine(synth.default_config(capi.V1_SWEPT), lib=lib)
eng.set_pointcloud(cloud, res, 1, bmin, bmax)
d_xyz = torch.from_numpy(cloud).cuda()
d_img = torch.zeros((cam.height, cam.width), dtype=torch.int32, device="cuda")
record = {"map": list(dims), "resolution": res, "points": int(len(cloud)), "camera": [cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy], "library": args.lib or "default",
          "repeats": args.repeats, "warmup": args.warmup, "render": []}
total = args.warmup + args.repeats


def timed(fn):
    t0 = time.perf_counter(); out = fn(); return out, (time.perf_counter() - t0) * 1e3


for max_splat in (0, 32):
    want, _ = E.depth_render_host(cam, pose, xyz=cloud, lib=lib, max_splat_px=max_splat)
    for source in ("cloud", "map"):
        ms, wall = [], []
        for _ in range(total):
            if source == "cloud":
                info, w = timed(lambda: eng.depth_render_device(cam, pose, d_xyz, d_img, max_splat_px=max_splat))
            else:
                info, w = timed(lambda: eng.depth_render_device(cam, pose, None, d_img, max_splat_px=max_splat))
            ms.append(info.render_ms); wall.append(w)
        assert np.array_equal(d_img.cpu().numpy(), want), "the device's image differs from the host form's"
        # info_out == NULL: no counters, no synchronisation; timed with torch events round a batch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            eng.depth_render_device(cam, pose, d_xyz if source == "cloud" else None, d_img, want_info=False, max_splat_px=max_splat)
        e1.record(); torch.cuda.synchronize()
        row = {"source": source, "max_splat_px": max_splat, "points": int(info.n_points), "splat_pixels": int(info.n_splat_pixels), "pixels_set": int(info.n_pixels_set),
               "render_ms": stat(ms[args.warmup:]), "wall_ms": stat(wall[args.warmup:]), "splat_pixels_per_second": float(info.n_splat_pixels / (np.median(ms[args.warmup:]) * 1e-3)),
               "no_info_ms_per_call_batch_of_20": float(e0.elapsed_time(e1) / 20)}
        record["render"].append(row)
        print(json.dumps(row), flush=True)

if not args.render_only:
    image, _ = eng.depth_render(cam, pose, None)
    rp = {"max_range_m": args.max_range, "no_return_is_free": True, "min_range_m": 0.2}
    # ---- the unprojection
    ms, wall, host = [], [], []
    for _ in range(total):
        (ends, hit, info), w = timed(lambda: eng.depth_rays(cam, pose, image, **rp))
        ms.append(info.rays_ms); wall.append(w)
    for _ in range(3):
        (h_ends, h_hit, h_info), w = timed(lambda: E.depth_rays_host(cam, pose, image, bmin, bmax, res, dims, lib=lib, **rp))
        host.append(w)
    assert ends.tobytes() == h_ends.tobytes() and hit.tobytes() == h_hit.tobytes(), "the device's rays differ from the host form's"
    record["rays"] = {"rays": int(info.n_pixels), "hits": int(info.n_hits), "no_return": int(info.n_no_return), "clipped": int(info.n_clipped), "truncated": int(info.n_truncated),
                      "rays_ms": stat(ms[args.warmup:]), "depth_rays_wall_ms": stat(wall[args.warmup:]), "depth_rays_host_one_thread_ms": stat(host)}
    print(json.dumps(record["rays"]), flush=True)
    # ---- the integration: the same map before every call (set_pointcloud outside the clock); no ESDF, no front end
    one, two = [], []
    for k in range(total):
        eng.set_pointcloud(cloud, res, 1, bmin, bmax)
        (dinfo, sinfo), w = timed(lambda: eng.integrate_depth(cam, pose, image, **rp))
        one.append((w, sinfo.trace_ms, dinfo.rays_ms))
        counts_one = eng.map_counts() if k == total - 1 else None
        eng.set_pointcloud(cloud, res, 1, bmin, bmax)

        def both():
            e, h, _ = E.depth_rays_host(cam, pose, image, bmin, bmax, res, dims, lib=lib, **rp)
            return eng.integrate_scan(t, e, h)
        winfo, w = timed(both)
        two.append((w, winfo.trace_ms))
    assert np.array_equal(counts_one, eng.map_counts()), "isdf_integrate_depth and the two-call form left different counts"
    one, two = np.array(one)[args.warmup:], np.array(two)[args.warmup:]
    record["integrate"] = {"rays": int(sinfo.n_rays), "free_voxels": int(sinfo.n_free_voxels), "hits": int(sinfo.n_hits),
                           "integrate_depth_wall_ms": stat(one[:, 0]), "its_trace_ms_with_the_unprojection": stat(one[:, 1]), "its_rays_ms": stat(one[:, 2]),
                           "rays_host_then_integrate_scan_wall_ms": stat(two[:, 0]), "wall_ratio_two_calls_over_integrate_depth": float(np.median(two[:, 0]) / np.median(one[:, 0]))}
    print(json.dumps(record["integrate"]), flush=True)
    # ---- the project's earlier simulated sensor on a pixel grid of stride 8 (80 x 60 rays).  The semantics differ: the render splats
    # the voxel CENTRES as points of splat_m, scan_from_map walks each pixel's ray to the first occupied voxel and takes its chord.
    eng.set_pointcloud(cloud, res, 1, bmin, bmax)
    u, v = np.meshgrid(np.arange(0, cam.width, 8), np.arange(0, cam.height, 8))
    d_cam = np.stack([(u.ravel() - cam.cx) / cam.fx, (v.ravel() - cam.cy) / cam.fy, np.ones(u.size)], axis=1)
    d_world = d_cam @ pose.reshape(3, 4)[:, :3].T
    d_world /= np.linalg.norm(d_world, axis=1, keepdims=True)
    ends8 = (t + d_world * args.max_range).astype(np.float32)
    sfm = [timed(lambda: E.scan_from_map(eng, t, ends8))[1] for _ in range(3)]
    record["against_scan_from_map"] = {"rays": int(len(ends8)), "scan_from_map_wall_ms": stat(sfm),
                                       "depth_render_map_source_wall_ms_all_307200_pixels": next(r["wall_ms"] for r in record["render"] if r["source"] == "map" and r["max_splat_px"] == 0),
                                       "note": "different semantics: splatted voxel centres against per-ray voxel chords; 4 800 rays against 307 200 pixels"}
    print(json.dumps(record["against_scan_from_map"]), flush=True)
    # ---- the host form of the render, one thread
    hostr = [timed(lambda: E.depth_render_host(cam, pose, xyz=cloud, lib=lib))[1] for _ in range(3)]
    record["depth_render_host_one_thread_ms"] = stat(hostr)
    print(json.dumps({"depth_render_host_one_thread_ms": record["depth_render_host_one_thread_ms"]}), flush=True)
eng.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
json.dump(record, open(args.out, "w"), indent=1)
print("wrote", args.out)
