#!/usr/bin/env python
"""Generates tests/golden/ref_demo_inputs.npz: the INPUTS of the reference's demo1 / demo6 (they cannot travel to the GPU box
with /root/reference) as the PRODUCT's own readers deliver them - the point cloud of src/plan_manager/map_pcds/CappedCone.pcd
(float32, compressed), the vertices / faces of shapes/Lthick.obj and shapes/mybox.obj after the Generalshape constructor's
transform with their configs' poly_params, and the yaml values of config_CappedCone.yaml / config_L.yaml / config_box.yaml the
tests use.  tests/test_fixtures.py checks the readers against independent parsing of the files (here) and this file against
the readers.  Also writes tests/golden/ref_demo_files.npz (below).  Run where the reference is: python tests/golden/make_golden_demo.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

PM = "/root/reference/src/plan_manager"
pkg = graft.load_package()
fx = pkg.fixtures
out = {"CappedCone_xyz": fx.read_pcd(os.path.join(PM, "map_pcds", "CappedCone.pcd"))}
for cfg_name, tag in (("config_CappedCone.yaml", "CappedCone"), ("config_L.yaml", "L"), ("config_box.yaml", "box")):
    p = fx.load_yaml_config(os.path.join(PM, "config", cfg_name))
    s = p.sweep
    for k in ("kernel_size", "integral_intervs", "safety_hor", "weight_p", "weight_v", "weight_omg", "weight_theta", "vmax", "omgmax",
              "thetamax", "smoothing_eps", "vehicle_mass", "grav_acc", "horiz_drag", "vert_drag", "paras_drag", "speed_eps"):
        out[f"{tag}_yaml_{k}"] = np.array(getattr(s, k))
    for k in ("occupancy_resolution", "sta_threshold", "rho", "inittime", "traj_parlength"):
        out[f"{tag}_yaml_{k}"] = np.array(getattr(p, k))
    out[f"{tag}_yaml_poly_params"] = np.array(list(p.poly_params))
    out[f"{tag}_yaml_offset_aabb"] = np.array(list(p.offset_aabb))
    out[f"{tag}_yaml_inputdata"] = np.array(p.inputdata.decode())
    stem = os.path.splitext(os.path.basename(p.inputdata.decode()))[0]
    shape = fx.shape_from_config(p, PM)
    if shape.kind == pkg.capi.SHAPE_MESH:
        out[f"{stem}_V"] = shape._keep[0][:shape.n_vertices].copy()
        out[f"{stem}_F"] = shape._keep[1][:shape.n_faces].copy()
np.savez_compressed(os.path.join(ROOT, "tests", "golden", "ref_demo_inputs.npz"), **out)
print({k: (v.shape, str(v.dtype)) for k, v in out.items() if v.ndim})

# tests/golden/ref_demo_files.npz: the input FILES tests/test_fixtures.py reads, so that it runs without the reference.  The
# .obj / .yaml files verbatim (uint8); each .pcd as its 11 header lines + the sha256 of the whole file, its points as the
# library reads them - CappedCone's are ref_demo_inputs.npz's CappedCone_xyz, the other three maps' lie on a 0.25 mm grid and
# are stored as lzma-compressed int32 row differences of the grid indices (column-major).  The data lines are "%.8g" of the
# float32 values (pcl's ascii writer), so header + points rebuild each file byte for byte (checked here and in the test).
import hashlib  # noqa: E402
import lzma  # noqa: E402

PCD_STEP = 0.00025
files = {}
for rel in ("shapes/Lthick.obj", "shapes/mybox.obj", "shapes/RoundedCone.obj", "config/config_CappedCone.yaml", "config/config_L.yaml"):
    files[rel] = np.frombuffer(open(os.path.join(PM, rel), "rb").read(), dtype=np.uint8)
for name in ("CappedCone", "Torus_big", "Bendlinear_big", "SmoothIntersection"):
    path = os.path.join(PM, "map_pcds", name + ".pcd")
    raw = open(path, "rb").read()
    header = b"".join(raw.splitlines(keepends=True)[:11])
    xyz = fx.read_pcd(path)
    if name == "CappedCone":
        assert np.array_equal(xyz, out["CappedCone_xyz"])
    else:
        k = np.rint(xyz.astype(np.float64) / PCD_STEP).astype(np.int32)
        assert np.array_equal((k * PCD_STEP).astype(np.float32), xyz), name
        files[f"pcd/{name}/dk"] = np.frombuffer(lzma.compress(np.ascontiguousarray(np.diff(k, axis=0, prepend=0).T, dtype=np.int32).tobytes(), preset=9), dtype=np.uint8)
    assert header + "".join(" ".join("%.8g" % v for v in r) + "\n" for r in xyz.astype(np.float64)).encode() == raw, name
    files[f"pcd/{name}/header"] = np.frombuffer(header, dtype=np.uint8)
    files[f"pcd/{name}/sha256"] = np.array(hashlib.sha256(raw).hexdigest())
np.savez_compressed(os.path.join(ROOT, "tests", "golden", "ref_demo_files.npz"), **files)
print(sorted(files))
