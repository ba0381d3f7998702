"""Buffer, event and state lifetime (csrc/dev_buf.hpp, csrc/ctx_state.hpp): every device and pinned byte and every event the library
takes while a ctx lives is given back when the ctx is destroyed, and every state a ctx creates on first use goes with it.  The
figures are isdf_debug_live_bytes and isdf_debug_live_events - integers the library keeps itself about its own buffers and events -
never the device's free memory, which other jobs on a shared card move."""
import ctypes as C
import gc

import numpy as np
import pytest

from common import small_world, traj

pytestmark = pytest.mark.gpu


def _live(lib):
    out = (C.c_longlong * 2)()
    lib.isdf_debug_live_bytes(out)
    return int(out[0]), int(out[1])


def _held(lib):
    """(device bytes, pinned bytes), events"""
    return _live(lib), int(lib.isdf_debug_live_events())


def _ends(pkg, occ, res, N, seed):
    """boundary states, inner waypoints and durations of a synthetic trajectory (what isdf_set_trajectory / pack_variables take)"""
    T, Cf = pkg.synth.random_trajectory(np.array(occ.shape) * res, N, seed=seed, piece_T=1.2, margin=4.0, occ=occ, res=res)
    c = Cf.reshape(N, 6, 3)
    head = np.zeros((3, 3)); tail = np.zeros((3, 3))
    head[:, 0] = c[0, 0]
    tail[:, 0] = sum(c[N - 1, p] * 1.2 ** p for p in range(6))
    return head, tail, c[1:, 0, :].copy(), T


def test_every_byte_comes_back(pkg, product_lib):
    capi, synth, lib = pkg.capi, pkg.synth, product_lib
    occ, esdf, res = small_world(pkg, seed=3)
    cone = synth.make_shape("RoundedCone", params=(0.8, 0.3, 1.6), bound_radius=1.9)
    V, F = synth.l_prism_mesh()
    mesh = synth.make_mesh_shape(V, F)
    T6, C6 = traj(pkg, occ, res, N=6, seed=11)
    T12, C12 = traj(pkg, occ, res, N=12, seed=12)
    pts = (np.argwhere(occ != 0) + 0.5) * res
    gc.collect()                                            # (engines other tests dropped go now, not in the middle of the count)
    before = _live(lib)
    events_before = _held(lib)[1]

    # ---- V3 ctx, analytic robot: grid + ESDF generation, fused and batch steps, callback, ESDF samples, batch optimizer, front end
    a = pkg.Engine(synth.default_config(capi.V3_ESDF_TILE, kernel_size=9, integral_intervs=16, safety_hor=0.5))
    a.set_grid(occ, (0, 0, 0), res, capi.GRID_OCCUPANCY)
    a.generate_esdf()
    a.set_shape(cone)
    assert _live(lib)[0] > before[0] and _live(lib)[0] > 0, "a living ctx holds device memory"
    a.eval_single(T6, C6)                                   # one fused launch through isdf_eval (host-direct where the host allows it)
    once = _live(lib)
    assert once[0] > before[0] and once[1] > before[1], (before, once)
    a.eval_single(T6, C6)
    assert _live(lib) == once, "grow-only buffers are reused by an identical call"
    a.eval_single(T12, C12)                                 # twice the pieces: the sweep's and the host-direct buffers grow
    assert _live(lib)[0] > once[0] and _live(lib)[1] > once[1]
    a.eval([T6] * 24, [C6] * 24)                            # a batch: sweep + tail as two launches
    for mode in (capi.MINCO_HOST, capi.MINCO_DEVICE):       # the objective callback on both MINCO paths
        a.set_minco_mode(mode)
        head, tail, way, T0 = _ends(pkg, occ, res, 6, 70)
        a.set_trajectory(6, head, tail, 5.0)
        a.cost_function(a.pack_variables(T0, way))
    a.set_minco_mode(capi.MINCO_AUTO)
    a.esdf_sample(pts[:500] + 0.1)
    a.esdf_sample(pts[:500] + 0.1, scattered=True)
    heads, tails, x0s = [], [], []
    for b in range(4):
        head, tail, way, T0 = _ends(pkg, occ, res, 4, 80 + b)
        a.set_trajectory(4, head, tail, 5.0)
        x0s.append(a.pack_variables(T0, way)); heads.append(head); tails.append(tail)
    a.optimize_lbfgs_batch(4, np.array(heads), np.array(tails), 5.0, np.array(x0s), max_iterations=3, g_epsilon=0.0, past=0)
    a.frontend_build(capi.frontend_config(kernel_size=9))
    a.frontend_cspace(download=False)
    a.frontend_astar((1.0, 1.0, -0.1), (3.0, 3.0, 3.0))     # (found or not: the search builds the host table and the orders)

    # ---- V1 ctx, mesh robot: points set and gathered, swept-volume steps, field query, mesh build, clearance check with kept rows
    v = pkg.Engine(synth.default_config(capi.V1_SWEPT, safety_hor=0.5))
    v.set_grid(occ, (0, 0, 0), res, capi.GRID_OCCUPANCY)
    v.set_shape(mesh)
    v.gather_points(np.array([[6.0, 6.0, 4.0], [12.0, 12.0, 8.0]]), (3.0, 3.0, 3.0))
    v.set_points(pts[:300])
    v.eval_single(T6, C6)
    once = _live(lib)
    v.eval_single(T6, C6)
    assert _live(lib) == once, "grow-only buffers are reused by an identical call"
    v.set_points(pts[:900])                                 # three times the points: the V1 scratch grows as one group
    v.eval_single(T6, C6)
    assert _live(lib)[0] > once[0]
    v.swept_sdf(T6, C6, pts[:200])
    v.swept_mesh(T6, C6, 0.4)
    v.traj_check(T6, C6, margin=1.0)
    v.traj_check_points()

    # ---- two shards of one step on the one device (isdf_create_multi)
    m = pkg.Engine(synth.default_config(capi.V3_ESDF_TILE, kernel_size=9, integral_intervs=16, safety_hor=0.5), devices=[0, 0])
    m.set_grid(esdf, (0, 0, 0), res, capi.GRID_ESDF)
    m.set_shape(cone)
    m.eval_single(T6, C6)

    assert _held(lib)[1] > events_before, "a living multi-device ctx holds its hand-over events"

    # ---- every state a ctx creates on first use, touched once - and once more, which must take nothing further: the in-place map
    # changes, the ray cast, the depth camera, the known grid, the trajectory tools, the watch's fold, the cost-to-go field
    w = pkg.Engine(synth.default_config(capi.V1_SWEPT, safety_hor=0.5))
    ext = np.array(occ.shape) * res
    assert tuple(w.set_pointcloud(pts, res, bmin=(0, 0, 0), bmax=ext)) == occ.shape
    w.set_shape(cone)
    w.frontend_build(capi.frontend_config(kernel_size=9))
    w.map_known_enable(True)
    w.map_known_merge_ms(True)                              # (the merge kernel's own pair of events)
    free = (np.argwhere(occ == 0) + 0.5) * res
    few, other = free[[100, 2000, 30000]], free[[500, 9000, 20000]]      # free voxels' centres: `few` for the map changes, `other` for the watch
    origin = (2.1, 2.2, 2.3)
    cam = pkg.engine.depth_camera(16, 12, 10.0, 10.0, 8.0, 6.0)
    pose = np.hstack([np.eye(3), np.array(origin)[:, None]])
    image, _ = w.depth_render(cam, pose, xyz=pts[:500])
    head, tail, way, T0 = _ends(pkg, occ, res, 6, 70)
    head, tail = np.concatenate([head[:, 0], np.zeros(6)]), np.concatenate([tail[:, 0], np.zeros(6)])
    w.traj_check_set_watch(1)

    def watch_fold():                                       # arms the watch, folds three new voxels, puts the map back (the clear re-checks)
        w.traj_check(T6, C6, margin=1.0)
        w.update_pointcloud(other)
        w.clear_pointcloud(other)

    touches = [("update_pointcloud", lambda: w.update_pointcloud(few)), ("clear_pointcloud", lambda: w.clear_pointcloud(few)),
               ("integrate_scan", lambda: w.integrate_scan(origin, few)), ("map_raycast", lambda: w.map_raycast(origin, pts[:8])),
               ("depth_render", lambda: w.depth_render(cam, pose, xyz=pts[:500])), ("depth_rays", lambda: w.depth_rays(cam, pose, image)),
               ("map_known", w.map_known), ("map_frontier", w.map_frontier),
               ("traj_limits", lambda: w.traj_limits(T6, C6)), ("traj_retime", lambda: w.traj_retime(T6, C6)),
               ("traj_realloc", lambda: w.traj_realloc(head, tail, way, T0)), ("watch fold", watch_fold),
               ("frontend_field_build", lambda: w.frontend_field_build((3.0, 3.0, 3.0))), ("shift_map", lambda: w.shift_map((1, 0, 0)))]
    events_idle = _held(lib)[1]
    for what, touch in touches:
        touch()
        once = _held(lib)
        touch()
        assert _held(lib) == once, f"{what}: a second identical call took bytes or events ((device, pinned), events)"
    assert _held(lib)[1] > events_idle, "the states keep their events while the ctx lives"

    for e in (w, m, v, a):
        e.close()
    assert _held(lib) == (before, events_before), "bytes or events still held after isdf_destroy ((device, pinned), events)"
