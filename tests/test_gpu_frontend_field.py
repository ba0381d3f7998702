"""The cost-to-go field of one goal on the device (csrc/frontend_field.hip) and the paths read off it.  Every relaxation order that reaches
a fixed point reaches the same bytes, so the device field, the host form and the tests' own Dijkstra (tests/field_reference.py) are compared
BYTE FOR BYTE.  Free masks come from isdf_frontend_cspace of a ball or a box robot with kernel_size 5 and 3 x 3 attitudes on small maps: the
smallest shapes at which each mechanism (partial bricks, a second 64-lane z block, brick re-activation, the round bound) can go wrong."""
import ctypes as C
import math

import numpy as np
import pytest

import field_reference as fr

pytestmark = pytest.mark.gpu

RES = 0.5
MAX_ANG, ANG_RES, XK = 30.0, 30.0, 3        # attitudes -30, 0, +30 degrees in roll and in pitch


def _engine(pkg, occ, robot="ball"):
    capi, synth = pkg.capi, pkg.synth
    eng = pkg.Engine(synth.default_config(capi.V1_SWEPT))
    eng.set_grid(occ, (0, 0, 0), RES, capi.GRID_OCCUPANCY)
    # the ball is smaller than a voxel: it fills its own voxel only, so free = not occupied and the maps keep their walls and gaps
    eng.set_shape(synth.make_shape("Ball", params=(0.1,)) if robot == "ball" else synth.make_shape("Box", params=(0.9, 0.2, 0.15)))
    _build_frontend(pkg, eng)
    table, _ = eng.frontend_cspace()
    free = table.any(axis=3)
    if robot == "ball":
        assert np.array_equal(free, occ == 0)
    return eng, table, free


def _build_frontend(pkg, eng):
    eng.frontend_build(pkg.capi.frontend_config(kernel_size=5, max_roll=MAX_ANG, max_pitch=MAX_ANG, ang_res=ANG_RES, safeh=0.0))


def _centre(cell):
    return (np.asarray(cell, dtype=np.float64) + 0.5) * RES


def _live(eng):
    b = (C.c_longlong * 2)()
    eng.lib.isdf_debug_live_bytes(b)
    return int(b[0]), int(b[1])


FIELD_CASES = {
    "open_9x7x5": (lambda synth: fr.open_map(), (1, 5, 3)),                                   # smaller than one brick
    "boxes_17x9x70": (lambda synth: synth.random_box_map((17, 9, 70), res=RES, occupancy=0.15, seed=4, edge=(0.5, 1.5)), None),   # partial bricks, two z blocks
    "wall_with_gap": (lambda synth: fr.wall_with_gap(), (0, 0, 0)),
    "sealed_pocket": (lambda synth: fr.sealed_pocket(), (0, 0, 0)),
    "goal_not_free": (lambda synth: fr.sealed_pocket(), (3, 1, 0)),
}


@pytest.mark.parametrize("name", sorted(FIELD_CASES))
def test_field_equals_host_form_and_reference_byte_for_byte(pkg, product_lib, name):
    make, goal = FIELD_CASES[name]
    occ = make(pkg.synth)
    eng, table, free = _engine(pkg, occ)
    if goal is None:                                      # the free voxel farthest from the origin corner: the wave crosses every brick
        cells = np.argwhere(free)
        goal = tuple(int(v) for v in cells[np.argmax(cells.sum(axis=1))])
    want = fr.field(free, goal)
    info = eng.frontend_field_build(_centre(goal))
    d = eng.frontend_field()
    host, host_reachable = pkg.frontend_field_host(table, goal, XK * XK)
    print(f"\n{name}: rounds {info.rounds}, bricks {info.bricks}, visits {info.brick_visits}, free {info.free_voxels}, reached {info.reached_voxels}, "
          f"{info.device_ms:.3f} ms")
    assert fr.same_bytes(host, want)
    assert fr.same_bytes(d, want)
    assert info.reachable == int(free[goal]) == int(host_reachable)
    assert info.status == (0 if free[goal] else 1)
    assert info.free_voxels == int(free.sum()) and info.reached_voxels == int(np.isfinite(want).sum())
    if name == "sealed_pocket":
        assert np.isinf(d[4:7, 2:5, 1:4]).all() and free[4:7, 2:5, 1:4].all()
    if name == "goal_not_free":
        assert np.isinf(d).all() and info.rounds == 0
    if name == "boxes_17x9x70":
        assert info.bricks == 3 * 2 * 2 and np.isfinite(want[:, :, 64:]).any() and np.isfinite(want[:, :, :64]).any()
    # values at world points' cells; a point outside the map is +inf
    rng = np.random.default_rng(3)
    cells = np.stack([rng.integers(0, s, 50) for s in occ.shape], axis=1)
    pts = np.concatenate([(cells + rng.uniform(0.05, 0.95, cells.shape)) * RES, [[-0.3, 1.0, 1.0]]])
    v = eng.frontend_field(pts)
    assert fr.same_bytes(v[:-1], want[cells[:, 0], cells[:, 1], cells[:, 2]]) and np.isinf(v[-1])


def test_goal_outside_the_map(pkg, product_lib):
    eng, table, free = _engine(pkg, fr.open_map())
    info = eng.frontend_field_build((-1.0, 1.0, 1.0))
    assert info.reachable == 0 and info.status == 1 and info.rounds == 0 and info.reached_voxels == 0
    assert np.isinf(eng.frontend_field()).all()
    n, _, _ = eng.frontend_field_paths([_centre((2, 2, 2))], 8)
    assert n[0] == 0


def test_brick_reactivation_and_round_bound(pkg, product_lib):
    """A corridor that runs the length of x twelve times crosses every 8 x 8 brick again and again: bricks are left and re-entered."""
    occ = fr.serpentine((24, 24, 3))
    goal = (0, 0, 1)
    eng, table, free = _engine(pkg, occ)
    want = fr.field(free, goal)
    info = eng.frontend_field_build(_centre(goal))
    print(f"\nserpentine: rounds {info.rounds}, bricks {info.bricks}, visits {info.brick_visits}, {info.device_ms:.3f} ms")
    assert fr.same_bytes(eng.frontend_field(), want)
    assert info.status == 0 and info.reachable == 1
    assert info.bricks == 9 and info.brick_visits > info.bricks and info.rounds > 1
    # one round only: the field as it stands, an upper bound of d everywhere
    part = eng.frontend_field_build(_centre(goal), max_rounds=1)
    d1 = eng.frontend_field()
    assert part.status == 2 and part.rounds == 1 and part.reachable == 1
    fin = np.isfinite(d1)
    assert fin.any() and not fin[np.isinf(want)].any() and (d1[fin] >= want[fin]).all()
    assert np.isinf(d1[np.isfinite(want)]).any()          # (one round cannot have walked the corridor)
    again = eng.frontend_field_build(_centre(goal))
    assert again.status == 0 and fr.same_bytes(eng.frontend_field(), want)


def test_repeatable_and_tracks_the_map(pkg, product_lib):
    synth, capi = pkg.synth, pkg.capi
    occ = synth.random_box_map((17, 9, 70), res=RES, occupancy=0.15, seed=4, edge=(0.5, 1.5))
    eng, table, free = _engine(pkg, occ)
    goal = tuple(int(v) for v in np.argwhere(free)[0])
    eng.frontend_field_build(_centre(goal))
    d_a = eng.frontend_field()
    eng.frontend_field_build(_centre(goal))
    live2 = _live(eng)
    d_b = eng.frontend_field()
    eng.frontend_field_build(_centre(goal))
    assert _live(eng) == live2                            # grow-only state: nothing is taken or given from the second build on
    assert fr.same_bytes(d_a, d_b) and fr.same_bytes(d_a, eng.frontend_field()) and fr.same_bytes(d_a, fr.field(free, goal))
    # a changed map: isdf_set_grid and isdf_frontend_build drop the field; the next build is the new map's
    occ2 = occ.copy()
    occ2[8, :, 10:60] = 1
    occ2[8, 4, 30] = 0
    eng.set_grid(occ2, (0, 0, 0), RES, capi.GRID_OCCUPANCY)
    with pytest.raises(pkg.IsdfError):
        eng.frontend_field_build(_centre(goal))           # ISDF_ERR_STATE before isdf_frontend_build
    _build_frontend(pkg, eng)
    with pytest.raises(pkg.IsdfError):
        eng.frontend_field()                              # no field yet
    eng.frontend_field_build(_centre(goal))
    free2 = occ2 == 0
    want2 = fr.field(free2, goal)
    assert fr.same_bytes(eng.frontend_field(), want2) and not fr.same_bytes(want2, d_a)
    eng.frontend_field_release()
    with pytest.raises(pkg.IsdfError):
        eng.frontend_field()
    with pytest.raises(pkg.IsdfError):
        eng.frontend_field_paths([_centre(goal)], 0)      # cap < 1


def _bfs_order(xk, yk, sx, sy):
    """The order in which visit_kernels_by_distance tests attitudes for a parent at (sx, sy), restated: the level attitude first, then
    breadth-first from the parent, neighbours pushed as (0, +1) (0, -1) (+1, 0) (-1, 0), the level attitude skipped when it comes up
    again, at most 801 pops."""
    zi, zj = (xk - 1) // 2, (yk - 1) // 2
    out = [zi * yk + zj]
    seen = {(sx, sy)}
    queue = [(sx, sy)]
    pops = 0
    while queue:
        pops += 1
        x, y = queue.pop(0)
        if (x, y) != (zi, zj):
            out.append(x * yk + y)
        for dx, dy in ((0, 1), (0, -1), (1, 0), (-1, 0)):
            nx, ny = x + dx, y + dy
            if 0 <= nx < xk and 0 <= ny < yk and (nx, ny) not in seen:
                seen.add((nx, ny))
                queue.append((nx, ny))
        if pops > 800:
            break
    return out


def _hold_path(n, xyz, rp, start_cell, goal, d, free, table):
    """one path against the rules, each restated here"""
    cells = np.floor(xyz[:n] / RES).astype(int)
    assert np.array_equal((cells + 0.5) * RES, xyz[:n])                                     # cube centres
    assert tuple(cells[0]) == tuple(start_cell) and tuple(cells[-1]) == tuple(goal)
    assert rp[0, 0] == 0.0 and rp[0, 1] == 0.0
    X, Y, Z = free.shape
    for s in range(n - 1):
        cur, nxt = cells[s], cells[s + 1]
        step = nxt - cur
        assert np.abs(step).max() == 1 and free[tuple(nxt)]                                 # a free 26-neighbour
        best, first = math.inf, None
        for i, j, k in fr.NEIGHBOURS:                                                       # the first minimiser in i, j, k order
            v = (cur[0] + i, cur[1] + j, cur[2] + k)
            if not (0 <= v[0] < X and 0 <= v[1] < Y and 0 <= v[2] < Z):
                continue
            cand = d[v] + fr.EDGE[i * i + j * j + k * k]
            if cand < best:
                best, first = cand, (i, j, k)
        assert tuple(step) == first
        if free[tuple(cur)]:
            assert d[tuple(nxt)] + fr.EDGE[int((step * step).sum())] == d[tuple(cur)]       # fl(d[next] + w) == d[cur], exactly
        # the first set bit of the node's word in the breadth-first order of the previous node's attitude
        fr_, fp_ = rp[s]
        fi, fj = int((fr_ + MAX_ANG) / ANG_RES), int((fp_ + MAX_ANG) / ANG_RES)
        word = table[tuple(nxt)]
        att = next(a for a in _bfs_order(XK, XK, fi, fj) if (int(word[a >> 5]) >> (a & 31)) & 1)
        ri, rj = att // XK, att % XK
        assert rp[s + 1, 0] == fr_ + (ri - fi) * ANG_RES and rp[s + 1, 1] == fp_ + (rj - fj) * ANG_RES


def test_paths(pkg, product_lib):
    import torch
    occ = np.zeros((14, 11, 7), dtype=np.uint8)
    occ[6:11, 3:8, 1:6] = 1
    occ[7:10, 4:7, 2:5] = 0                                # a sealed pocket
    occ[3, 2:6, 0:4] = 1                                 # a pillar to walk around
    occ[11:, 9, 3:] = 1
    goal = (1, 1, 3)
    eng, table, free = _engine(pkg, occ, robot="box")
    assert free[goal] and not free.all() and (table.reshape(-1, 4)[:, 0] & 0x1FF != 0x1FF)[free.reshape(-1)].any()      # some free voxel lacks an attitude
    info = eng.frontend_field_build(_centre(goal))
    d = eng.frontend_field()
    assert info.reachable == 1 and fr.same_bytes(d, fr.field(free, goal))
    # a cell that is not free next to free ones with a way to the goal; a cell of the pocket
    blocked = next(tuple(int(v) for v in c) for c in np.argwhere(~free)
                   if np.isfinite(d[max(c[0] - 1, 0):c[0] + 2, max(c[1] - 1, 0):c[1] + 2, max(c[2] - 1, 0):c[2] + 2]).any())
    pocket = (8, 5, 3)
    assert np.isinf(d[7:10, 4:7, 2:5]).all()
    far = [tuple(int(v) for v in c) for c in np.argwhere(np.isfinite(d)) if d[tuple(c)] > 10.0][::37][:4]
    assert len(far) >= 3
    cells = far + [blocked, pocket, goal]
    rng = np.random.default_rng(5)
    starts = np.array([(np.array(c) + rng.uniform(0.1, 0.9, 3)) * RES for c in cells] + [[3.0, -0.2, 1.0]])      # the last: outside the map
    cap = 40
    n, xyz, rp = eng.frontend_field_paths(starts, cap)
    B = len(starts)
    assert n[B - 1] == 0 and n[B - 2] == 1 and n[B - 3] == 0 and (n[:B - 3] > 1).all() and n.max() <= cap
    assert np.array_equal(xyz[B - 2, 0], _centre(goal)) and np.array_equal(rp[B - 2, 0], [0.0, 0.0])
    for b in range(B):
        n1, xyz1, rp1 = eng.frontend_field_paths(starts[b:b + 1], cap)                      # row b of the batch = the single call
        assert n1[0] == n[b] and np.array_equal(xyz1[0], xyz[b]) and np.array_equal(rp1[0], rp[b])
        assert not xyz[b, n[b]:].any() and not rp[b, n[b]:].any()
        if n[b] > 0:
            _hold_path(int(n[b]), xyz[b], rp[b], cells[b], goal, d, free, table)
    assert (rp[:, :, :] != 0.0).any()                     # the box does not fit level everywhere: the attitude rule is exercised
    # a cap shorter than a path: the true length is reported, cap nodes are written
    short = 4
    ns, xyzs, rps = eng.frontend_field_paths(starts, short)
    assert np.array_equal(ns, n) and n[0] > short
    for b in range(B):
        m = min(int(n[b]), short)
        assert np.array_equal(xyzs[b, :m], xyz[b, :m]) and np.array_equal(rps[b, :m], rp[b, :m])
    # the device form
    d_s = torch.tensor(starts.reshape(-1), dtype=torch.float64, device="cuda")
    d_n = torch.zeros(B, dtype=torch.int32, device="cuda")
    d_xyz = torch.zeros(B * cap * 3, dtype=torch.float64, device="cuda"); d_rp = torch.zeros(B * cap * 2, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    eng.frontend_field_paths_device(d_s.data_ptr(), B, cap, d_n.data_ptr(), d_xyz.data_ptr(), d_rp.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(d_n.cpu().numpy(), n)
    assert np.array_equal(d_xyz.cpu().numpy().reshape(B, cap, 3), xyz) and np.array_equal(d_rp.cpu().numpy().reshape(B, cap, 2), rp)


def test_against_the_astar(pkg, product_lib):
    """The existing A* walks the same graph with an inflated heuristic and an open set that keeps stale keys (front_end_Astar.hpp:319-328):
    its path is a real path, so its cost cannot be below d[start] - only that bound is asserted -, and it finds a path exactly where d is
    finite."""
    synth = pkg.synth
    occ = synth.random_box_map((32, 32, 8), res=RES, occupancy=0.12, seed=21, edge=(0.5, 2.0))
    eng, table, free = _engine(pkg, occ, robot="box")
    rng = np.random.default_rng(17)
    cells = np.argwhere(free)
    ok = 0
    for _ in range(14):
        s, g = (tuple(int(v) for v in cells[i]) for i in rng.choice(len(cells), 2, replace=False))
        info = eng.frontend_field_build(_centre(g))
        d_start = float(eng.frontend_field([_centre(s)])[0])
        xyz, rp, rot, r = eng.frontend_astar(_centre(s), _centre(g))
        assert bool(r.success) == math.isfinite(d_start), (s, g)
        if not r.success:
            continue
        ok += 1
        steps = np.rint(np.diff(xyz, axis=0) / RES).astype(int)
        cost = 0.0
        for st in steps:
            cost += math.sqrt(float((st * st).sum()))
        print(f"\n{s} -> {g}: A* {cost:.6f} over {len(xyz)} nodes, d[start] {d_start:.6f}, field {info.rounds} rounds {info.device_ms:.3f} ms")
        assert cost >= d_start * (1.0 - 1e-12)
    assert ok >= 10, ok
