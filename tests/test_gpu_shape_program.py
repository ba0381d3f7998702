"""ISDF_SHAPE_PROGRAM on the device: the interpreter against the host evaluator, programs that restate registered classes against
the built-in kinds through every consumer of the shape plugin, a shape no class offers, and the context's state."""
import ctypes as C
import gc
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import shape_program_cases as cases
from common import REL_TOL, assert_close, small_world, traj

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASS_NAMES = ["CSG", "Table", "SmoothDifference", "SmoothIntersection", "SmoothIntersection_big", "RoundedCone", "CappedCone",
               "WireframeBox", "TwistBox", "BendBox", "Torus", "Torus_big", "Ball"]
NOVEL_NAMES = ["shell_dilate_blend", "scale_pyramid", "erode_negate_capped_cylinder", "smooth_union_rotate_to", "wireframe_box_op"]
SWEEP_NAMES = ["CSG", "RoundedCone", "Table", "SmoothDifference", "TwistBox"]


@pytest.fixture(scope="module")
def pts():
    return cases.points()


def _tree(pkg, name):
    return pkg.csg.reference_class(name) if name in CLASS_NAMES else cases.novel_programs(pkg.csg)[name]


@pytest.mark.parametrize("name", CLASS_NAMES + NOVEL_NAMES)
def test_plugin_alone_matches_the_host_evaluator(pkg, product_lib, pts, name):
    """Engine.shape_eval against isdf_shape_program_eval_host: SDF within 1e-12 x max(1, |sdf|) (the same arithmetic; the device's
    sqrt / sincos may differ from the host's by an ulp); gradient within 1e-5, where only a point whose stencil mixes branches may
    be left out, at most 1 % of the points (see tests/test_shape_program_host.py)."""
    capi, csg = pkg.capi, pkg.csg
    tree = _tree(pkg, name)
    eng = pkg.Engine(pkg.synth.default_config())
    eng.set_shape_program(tree)
    s, g = eng.shape_eval(pts)
    s0, g0 = csg.eval_host(tree, pts)
    rel = np.abs(s - s0) / np.maximum(1.0, np.abs(s0))
    same = cases.stencil_same_branch(capi, tree, pts)
    gerr = np.abs(g - g0).max(axis=1)
    left_out = ~same & ~(gerr <= 1e-5)
    print(f"\n{name}: max |device - host| / max(1, |sdf|) {rel.max():.3e}; stencil mixes branches at {1.0 - same.mean():.3%}, left out "
          f"{left_out.mean():.3%}; max |grad - host| {gerr[~left_out].max():.3e}")
    assert rel.max() <= 1e-12
    assert left_out.mean() <= 0.01
    assert gerr[~left_out].max() <= 1e-5
    # with a body offset: offset first, then the program
    R = pkg.synth.poly_rotation(20.0, -35.0, 60.0); t = np.array([0.3, -0.2, 0.5])
    eng.set_shape_program(tree, trans=t, rotate=R)
    s1, _ = eng.shape_eval(pts[:512], want_grad=False)
    s2, _ = csg.eval_host(tree, pts[:512], trans=t, rotate=R, want_grad=False)
    assert (np.abs(s1 - s2) / np.maximum(1.0, np.abs(s2))).max() <= 1e-12


@pytest.mark.parametrize("no_fuse", [False, True], ids=["fused", "ISDF_NO_FUSE"])
def test_through_the_sweeps_program_equals_builtin_kind(no_fuse):
    """CSG, RoundedCone, Table, SmoothDifference and TwistBox as programs against the built-in kinds, V3 and V1, with the bounds given
    and with zeros, in a fresh child process (tests/shape_program_sweep_worker.py)."""
    env = dict(os.environ)
    env.pop("ISDF_NO_FUSE", None)
    if no_fuse:
        env["ISDF_NO_FUSE"] = "1"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "shape_program_sweep_worker.py")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    res = json.loads(line[len("RESULT "):])
    assert sorted(res) == sorted(SWEEP_NAMES)
    for name, rr in res.items():
        print(f"\n{name} ({'two launches' if no_fuse else 'fused'}; host paths {rr['host_path']}):")
        for key, f in rr.items():
            if key == "host_path":
                continue
            print(f"  {key}: " + ", ".join(f"{k} {v:.6g}" if isinstance(v, float) else f"{k} {v}" for k, v in f.items()))
            assert f["cost_ref"] > 0 and abs(f["cost"] - f["cost_ref"]) <= REL_TOL * abs(f["cost_ref"]), (name, key)
            assert f["gradT"] <= REL_TOL and f["gradC"] <= REL_TOL, (name, key)
            assert f.get("finite", True)
            if "pairs" in f:
                assert f["pairs"] == f["pairs_ref"] and f["pairs"] > 0, (name, key)
            if "dt" in f:
                assert f["dt"] <= 1e-9, (name, key)


def test_the_other_consumers_csg_program_equals_builtin(pkg, product_lib):
    capi, synth, csg = pkg.capi, pkg.synth, pkg.csg
    occ, esdf, res = small_world(pkg)
    T, cm = traj(pkg, occ, res)
    cfg = synth.default_config(capi.V1_SWEPT, safety_hor=0.5)
    a = pkg.Engine(cfg); b = pkg.Engine(cfg)
    a.set_shape(synth.make_shape("CSG", bound_radius=3.0))
    b.set_shape_program(csg.reference_class("CSG"), bound_radius=3.0)
    for e in (a, b):
        e.set_grid(occ, (0, 0, 0), res, capi.GRID_OCCUPANCY)
    # front end: byte-identical attitude kernels
    fe = capi.frontend_config(kernel_size=9)
    ka = kb = None
    for e in (a, b):
        e.frontend_build(fe)
    ka, kb = a.frontend_shape_kernels(), b.frontend_shape_kernels()
    diff = np.unpackbits(ka ^ kb)
    assert ka.any() and diff.sum() == 0, f"{int(diff.sum())} differing bits of {diff.size}; first at (attitude, byte) {np.argwhere(ka != kb)[:8].tolist()}"
    # clearance check
    assert a.traj_collide(T, cm) == b.traj_collide(T, cm)
    ra, rb = a.traj_check(T, cm), b.traj_check(T, cm)
    print(f"\nclearance: builtin {ra['min_clearance']:.12g}, program {rb['min_clearance']:.12g}; penetrating {ra['n_penetrating']} / {rb['n_penetrating']}")
    assert ra["qualified"] > 0 and abs(ra["min_clearance"] - rb["min_clearance"]) <= 1e-9
    assert (ra["n_penetrating"] > 0) == (rb["n_penetrating"] > 0) and ra["culled"] == rb["culled"] == 1
    # swept-volume field on 2 000 points around the trajectory
    rng = np.random.default_rng(7)
    N = T.size
    way = cm.reshape(3, -1).T.reshape(N, 6, 3)[:, 0, :]
    Q = way[rng.integers(0, N, 2000)] + rng.uniform(-4.0, 4.0, (2000, 3))
    va, _ = a.swept_sdf(T, cm, Q); vb, _ = b.swept_sdf(T, cm, Q)
    assert (va != 10.0).sum() > 200 and np.abs(va - vb).max() <= 1e-9


def _novel_robot(csg):
    body = csg.rounded_box((1.6, 0.8, 0.5), 0.1)
    arms = [csg.translate(csg.capped_cylinder((0.0, -0.6, 0.0), (0.0, 0.6, 0.0), 0.15), (0.6, 0.0, 0.3)),
            csg.translate(csg.capped_cylinder((0.0, -0.6, 0.0), (0.0, 0.6, 0.0), 0.15), (-0.6, 0.0, 0.3))]
    return csg.bendOp(csg.unionOp(body, arms, 0.2), 0.15)


def test_a_shape_no_class_offers_needs_no_lattice(pkg, product_lib):
    """The smooth union of a rounded box and two translated capped cylinders, bent - until now to be had only as a sampled lattice.
    The program against the host evaluator sampled onto a 0.1 m lattice (set_shape_grid) in a second engine: V3 cost within 5 %,
    gradC within 10 % in norm (the bounds tests/test_gpu_gridshape.py holds the documented approximation to)."""
    capi, synth, csg = pkg.capi, pkg.synth, pkg.csg
    tree = _novel_robot(csg)
    occ, esdf, res = small_world(pkg)
    T, cm = traj(pkg, occ, res)
    cfg = synth.default_config(capi.V3_ESDF_TILE, kernel_size=9, integral_intervs=16, safety_hor=0.5)
    nd, nres = (4.4, 4.4, 4.4), 0.1
    X, Y, Z = (int(np.ceil(n / nres)) for n in nd)
    mn = np.array([-nd[0] / 2, -nd[1] / 2, -nd[2] / 2])
    I, J, K = np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing="ij")
    P = np.stack([mn[0] + I * nres, mn[1] + J * nres, mn[2] + K * nres], axis=-1).reshape(-1, 3)
    s, g = csg.eval_host(tree, P)
    cells = np.concatenate([g, s[:, None]], axis=1).reshape(X, Y, Z, 4)
    ep = pkg.Engine(cfg); eg = pkg.Engine(cfg)
    for e in (ep, eg):
        e.set_grid(esdf, (0, 0, 0), res, capi.GRID_ESDF)
    ep.set_shape_program(tree)
    eg.set_shape_grid(cells, mn, nres)
    c, _, gC = ep.eval_single(T, cm)
    cg, _, gCg = eg.eval_single(T, cm)
    print(f"\nprogram vs its 0.1 m lattice, V3 sweep: cost {c:.6g} vs {cg:.6g} (rel {abs(c - cg) / c:.2e}), gradC rel {np.linalg.norm(gC - gCg) / np.linalg.norm(gC):.2e}")
    assert c > 0 and ep.stats()["grad_pairs"] > 0
    assert abs(c - cg) <= 0.05 * c and np.linalg.norm(gC - gCg) <= 0.1 * np.linalg.norm(gC)


def _live(lib):
    out = (C.c_longlong * 2)()
    lib.isdf_debug_live_bytes(out)
    return int(out[0]), int(out[1])


def test_state(pkg, product_lib):
    capi, synth, csg, lib = pkg.capi, pkg.synth, pkg.csg, product_lib
    occ, esdf, res = small_world(pkg)
    T, cm = traj(pkg, occ, res)
    cfg = synth.default_config(capi.V3_ESDF_TILE, kernel_size=9, integral_intervs=16, safety_hor=0.5)
    cone = synth.make_shape("RoundedCone", params=(0.8, 0.3, 1.6), bound_radius=1.9)
    tree = _novel_robot(csg)
    V, F = synth.l_prism_mesh()
    gc.collect()
    before = _live(lib)

    def fresh(install):
        e = pkg.Engine(cfg); e.set_grid(esdf, (0, 0, 0), res, capi.GRID_ESDF); install(e)
        return e, e.eval_single(T, cm)
    same = lambda r, q: r[0] == q[0] and np.array_equal(r[1], q[1]) and np.array_equal(r[2], q[2])
    e, r_cone = fresh(lambda e: e.set_shape(cone))
    # a rejected program leaves the previous shape's results bitwise unchanged
    bad = csg.instructions([(capi.OP_SPHERE, [1.0, 0, 0, 0]), (capi.OP_SPHERE, [float("nan"), 0, 0, 0]), (capi.OP_UNION, [0.0])])
    with pytest.raises(pkg.IsdfError, match="non-finite"):
        e.set_shape_program(bad)
    with pytest.raises(pkg.IsdfError, match="stack underflow"):
        e.set_shape_program(csg.instructions([(capi.OP_NEGATE, [])]))
    assert same(e.eval_single(T, cm), r_cone)
    s = capi.IsdfShape(); lib.isdf_shape_default(C.byref(s), capi.SHAPE_PROGRAM)
    with pytest.raises(pkg.IsdfError, match="isdf_set_shape_program"):
        e.set_shape(s)
    assert same(e.eval_single(T, cm), r_cone)
    # a program after a built-in kind, a built-in kind after a program, a program after a mesh: each as on a fresh context
    e2, r_prog = fresh(lambda e: e.set_shape_program(tree))
    e2.close()
    e.set_shape_program(tree)
    assert same(e.eval_single(T, cm), r_prog)
    e.set_shape(cone)
    assert same(e.eval_single(T, cm), r_cone)
    e.set_shape(synth.make_mesh_shape(V, F))
    e.eval_single(T, cm)
    e.set_shape_program(tree)
    assert same(e.eval_single(T, cm), r_prog)
    assert e.mesh_info()["faces"] == 0
    # the multi-device form replicates the program to its shards
    m = pkg.Engine(cfg, devices=[0, 0]); m.set_grid(esdf, (0, 0, 0), res, capi.GRID_ESDF); m.set_shape_program(tree)
    cm_, gTm, gCm = m.eval_single(T, cm)
    assert abs(cm_ - r_prog[0]) <= REL_TOL * r_prog[0]; assert_close(gCm, r_prog[2], "two shards gradC"); assert_close(gTm, r_prog[1], "two shards gradT")
    for x in (e, m):
        x.close()
    del e, m, e2
    gc.collect()
    assert _live(lib) == before
