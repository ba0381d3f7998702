"""The cost-to-go field gated by the eroded known grid (csrc/frontend_field.hip: isdf_frontend_field_build_known) against
the plain host Dijkstra (isdf_frontend_field_host) on a table the TEST gates - table'[v] = E[v] ? table[v] : 0 with the table as
isdf_frontend_cspace_get gives it and E from the NumPy restatement (tests/known_erode_reference.py), never from the library's erosion.
Fields are compared byte for byte.  The map, the robot and the helpers are tests/test_gpu_map_update.py's: 24 x 20 x 70 voxels at 0.5 m,
kernel_size 5 (footprint radius 2), 3 x 3 attitudes.

The scene, in voxels: a wall across x = 16 with one gap (y 6 .. 13, z 22 .. 47), a baffle across x = 8 over z 14 .. 39 that stands
between the start and the gap, and K: the half z < 35 seen, the half z >= 35 unseen.  Round the baffle the short way is over its top,
through unseen space; the way under it stays in seen space and is longer.  The goal lies beyond the wall in the seen half."""
import ctypes as C

import numpy as np
import pytest

import field_reference as fr
import known_erode_reference as er
import known_reference as kr
import test_gpu_depth_cam as dc
import test_gpu_map_update as mu
from test_gpu_map_update import BMIN, DIMS, RES

pytestmark = pytest.mark.gpu

N_ATT = 9
SEEN = (0, 0, 0, DIMS[0] - 1, DIMS[1] - 1, 34)
START, GOAL, GOAL_UNSEEN = (3, 10, 30), (21, 10, 28), (21, 10, 50)
CASES = [(r, border) for r in (0, 1, -1) for border in (0, 1)]
_SHARED = {}


def scene():
    occ = np.zeros(DIMS, dtype=bool)
    occ[16, :, :] = True
    occ[16, 6:14, 22:48] = False
    occ[8, :, 14:40] = True
    return occ


def _centre(cell, bmin=BMIN):
    return (np.asarray(cell, dtype=np.float64) + 0.5) * RES + bmin


def _cells(xyz, bmin=BMIN):
    return np.floor((np.asarray(xyz) - bmin) / RES).astype(int)


def _engine(pkg, seen=SEEN):
    eng = mu._engine(pkg, mu._in_cells(np.argwhere(scene()), 2, np.random.default_rng(3)), esdf=False)
    assert np.array_equal(eng.get_grid(pkg.capi.GRID_OCCUPANCY)[0] != 0, scene())
    eng.map_known_enable(True)
    eng.map_known_fill(seen, 1)
    return eng


def _radius(r):
    return mu.SIDE if r < 0 else r


def shared(pkg, lib):
    """the table, K and the host fields of every case, computed once: (table, K, {case: (E, d, reachable)}, ungated d)"""
    if not _SHARED:
        eng = _engine(pkg)
        table = eng.frontend_cspace_table()
        k = kr.unpack(eng.map_known()[0], DIMS)
        assert np.array_equal(k, kr.fill(np.zeros(DIMS, dtype=bool), SEEN, 1)) and table.shape[3] == 4
        fields = {}
        for r, border in CASES:
            e = er.erode(k, _radius(r), border)
            fields[(r, border)] = (e,) + pkg.frontend_field_host(table * e[..., None].astype(np.uint32), GOAL, N_ATT, lib=lib)
        _SHARED.update(table=table, k=k, fields=fields, ungated=pkg.frontend_field_host(table, GOAL, N_ATT, lib=lib)[0])
    return _SHARED["table"], _SHARED["k"], _SHARED["fields"], _SHARED["ungated"]


def _gone(pkg, eng):
    """no valid field, no gate, and nothing of the repair, the reopen or the carry ran"""
    S = pkg.capi.ISDF_ERR_STATE
    for call in (eng.frontend_field, lambda: eng.frontend_field(_centre(START)[None]), lambda: eng.frontend_field_paths(_centre(START)[None], 8),
                 eng.frontend_field_repair_info, eng.frontend_field_reopen_info, eng.frontend_field_shift_info):
        with pytest.raises(pkg.IsdfError) as err:
            call()
        assert err.value.code == S
    assert eng.frontend_field_known_info() == (0, 0, 0)


def test_the_gate_bites_by_the_reference_alone(pkg, product_lib):
    table, k, fields, ungated = shared(pkg, product_lib)
    free = table.any(axis=3)
    assert free[GOAL] and free[START] and not free[16, 0, 0] and not free[8, 0, 20]
    e, gated, reach = fields[(-1, 0)]
    assert reach and e[GOAL] and e[START] and not e[GOAL_UNSEEN] and free[GOAL_UNSEEN]
    lost = np.isfinite(ungated) & np.isinf(gated)                # free and reached, but not through seen space
    assert lost[:, :, 35:].sum() > 1000 and np.isfinite(ungated[GOAL_UNSEEN])
    assert np.isfinite(gated[START]) and gated[START] > ungated[START] + 3.0      # under the baffle, not over it
    assert not np.isfinite(gated[~e]).any() and (gated >= ungated).all()


@pytest.mark.parametrize("r,border", CASES)
def test_the_gated_field_equals_the_host_form_on_the_gated_table(pkg, product_lib, r, border):
    table, k, fields, ungated = shared(pkg, product_lib)
    e, want, reach = fields[(r, border)]
    eng = _engine(pkg)
    assert eng.frontend_field_known_info() == (0, 0, 0)
    info, gate = eng.frontend_field_build_known(_centre(GOAL), r, border)
    got = eng.frontend_field()
    assert fr.same_bytes(got, want)
    free_g = table.any(axis=3) & e
    assert (info.reachable, info.status, info.free_voxels, info.reached_voxels) == (int(reach), 0, int(free_g.sum()), int(np.isfinite(want).sum()))
    assert (gate.radius_used, gate.border, gate.known_voxels, gate.eroded_voxels) == (_radius(r), border, int(k.sum()), int(e.sum()))
    assert eng.frontend_field_known_info() == (1, _radius(r), border) and info.device_ms > 0.0 and gate.erode_ms >= 0.0
    assert np.array_equal(eng.map_known()[0], kr.pack(k))       # K is read, not written
    # the values and the paths read off the gated field
    rng = np.random.default_rng(5)
    reached = np.argwhere(np.isfinite(want) & (want > 0.0))
    assert len(reached) > 1000 and np.isfinite(want[START])
    starts = np.concatenate([[START], reached[rng.choice(len(reached), 10, replace=False)], [(3, 10, 50), GOAL]])      # ... one start in unseen space, one in the goal cell
    xyz0 = _centre(starts)
    assert fr.same_bytes(eng.frontend_field(xyz0), want[tuple(starts.T)])
    n, xyz, _ = eng.frontend_field_paths(xyz0, 256)
    assert n[-1] == 1 and n[-2] == 0 and (n[:-2] > 1).all() and (n <= 256).all()       # every cube round the unseen start is unseen: no path
    for b in range(len(starts)):
        cells = _cells(xyz[b, :n[b]])
        if n[b] == 0:
            continue
        d = want[tuple(cells.T)]
        assert tuple(cells[0]) == tuple(starts[b]) and tuple(cells[-1]) == GOAL and e[tuple(cells[1:].T)].all()
        assert (np.diff(d) < 0).all() and d[-1] == 0.0
    # a plain build afterwards is the plain build: no gate, the bytes of a fresh ctx
    plain = eng.frontend_field_build(_centre(GOAL))
    assert eng.frontend_field_known_info() == (0, 0, 0) and fr.same_bytes(eng.frontend_field(), ungated)
    if (r, border) == CASES[0]:
        fresh = _engine(pkg)
        finfo = fresh.frontend_field_build(_centre(GOAL))
        assert fr.same_bytes(fresh.frontend_field(), eng.frontend_field())
        assert (plain.free_voxels, plain.reached_voxels, plain.bricks) == (finfo.free_voxels, finfo.reached_voxels, finfo.bricks)


def test_goal_cells(pkg, product_lib):
    table, k, fields, ungated = shared(pkg, product_lib)
    eng = _engine(pkg)
    info, _ = eng.frontend_field_build_known(_centre(GOAL_UNSEEN))                # free, but unseen
    assert (info.reachable, info.status, info.reached_voxels) == (0, 1, 0) and np.isinf(eng.frontend_field()).all()
    assert eng.frontend_field_known_info() == (1, mu.SIDE, 0)
    assert eng.frontend_field_paths(_centre(START)[None], 8)[0][0] == 0
    info, _ = eng.frontend_field_build_known(_centre((21, 10, 33)))               # seen, but its cube reaches z = 35
    assert (info.reachable, info.status) == (0, 1)
    info, _ = eng.frontend_field_build_known(_centre(GOAL))
    assert (info.reachable, info.status) == (1, 0)
    info, _ = eng.frontend_field_build_known(BMIN - 1.0)                          # outside the map
    assert (info.reachable, info.status) == (0, 1)
    info, _ = eng.frontend_field_build_known(_centre(GOAL), max_rounds=1)
    assert info.status == 2 and eng.frontend_field_known_info()[0] == 1


def test_all_known_and_border_1_is_the_ungated_build(pkg, product_lib):
    ungated = shared(pkg, product_lib)[3]
    eng = _engine(pkg, seen=None)
    info, gate = eng.frontend_field_build_known(_centre(GOAL), -1, 1)
    assert gate.eroded_voxels == gate.known_voxels == int(np.prod(DIMS))
    assert fr.same_bytes(eng.frontend_field(), ungated)
    plain = eng.frontend_field_build(_centre(GOAL))
    assert (info.free_voxels, info.reached_voxels, info.bricks) == (plain.free_voxels, plain.reached_voxels, plain.bricks)


def _empty_image(pkg):
    cam = dc._cam(pkg, dc.WIDE)
    return cam, dc.ref.pose(dc.ref.rot(0.05, 0.1, -0.2), [5.2, 7.1, 14.0]), np.full((cam.height, cam.width), 999999, dtype=np.int32)


def test_whatever_changes_k_or_the_map_drops_a_gated_field_and_no_other(pkg, product_lib):
    """repair, reopen and shift modes at 1: the ungated field of the same sequence is kept or carried as ever, the gated one goes"""
    extra = _centre([[5, 3, 5], [5, 3, 5]]).astype(np.float32)    # two points: one new occupied voxel, in seen space, away from everything
    gated, plain = _engine(pkg), _engine(pkg)
    for eng in (gated, plain):
        eng.frontend_field_set_repair(1); eng.frontend_field_set_reopen(1); eng.frontend_field_set_shift(1)
    cam, p12, image = _empty_image(pkg)
    goal_xyz = _centre(GOAL)

    def build():
        info, _ = gated.frontend_field_build_known(goal_xyz)
        assert info.reachable == 1 and gated.frontend_field_known_info() == (1, mu.SIDE, 0)
        if not plain.frontend_field_known_info() == (0, 0, 0) or not _valid(plain):
            raise AssertionError("the ungated field went")
    assert plain.frontend_field_build(goal_xyz).reachable == 1
    # update
    build()
    assert gated.update_pointcloud(extra, **mu.INCR).field_dropped == 1
    _gone(pkg, gated)
    assert plain.update_pointcloud(extra, **mu.INCR).field_dropped == 0 and plain.frontend_field_repair_info().closed_voxels > 0
    # clear
    build()
    assert gated.clear_pointcloud(np.repeat(extra, 2, axis=0), **mu.INCR).field_dropped == 1
    _gone(pkg, gated)
    assert plain.clear_pointcloud(np.repeat(extra, 2, axis=0), **mu.INCR).field_dropped == 0 and plain.frontend_field_reopen_info().opened_voxels > 0
    # a depth image without a return: no ray, no occupancy changed, K as it was
    build()
    before = plain.frontend_field()
    k0 = gated.map_known()[0]
    _, sinfo = gated.integrate_depth(cam, p12, image)
    assert (sinfo.clear.n_cleared_voxels, sinfo.update.n_new_voxels, sinfo.clear.field_dropped, sinfo.update.field_dropped) == (0, 0, 1, 1)
    assert np.array_equal(gated.map_known()[0], k0)
    _gone(pkg, gated)
    _, sinfo = plain.integrate_depth(cam, p12, image)
    assert (sinfo.clear.field_dropped, sinfo.update.field_dropped) == (0, 0) and fr.same_bytes(plain.frontend_field(), before)
    # a fill of the known grid, also one that sets nothing new
    build()
    gated.map_known_fill((0, 0, 0, 1, 1, 1), 1)
    _gone(pkg, gated)
    plain.map_known_fill((0, 0, 0, 1, 1, 1), 1)
    assert fr.same_bytes(plain.frontend_field(), before)
    # a shift of the window: the ungated field is carried
    build()
    s = (1, 0, 0)
    assert gated.shift_map(s, force_path=1).field_dropped == 1
    _gone(pkg, gated)
    assert plain.shift_map(s, force_path=1).field_dropped == 0 and tuple(plain.frontend_field_shift_info().shift) == s
    # ... and a shift by nothing
    build()
    assert gated.shift_map((0, 0, 0)).field_dropped == 1
    _gone(pkg, gated)
    assert plain.shift_map((0, 0, 0)).field_dropped == 0 and _valid(plain)
    # the known grid switched off
    build()
    gated.map_known_enable(False)
    _gone(pkg, gated)
    plain.map_known_enable(False)
    assert _valid(plain)
    with pytest.raises(pkg.IsdfError) as err:
        gated.frontend_field_build_known(goal_xyz)
    assert err.value.code == pkg.capi.ISDF_ERR_STATE            # no known grid any more
    # a new front end
    gated.map_known_enable(True)
    gated.map_known_fill(None, 1)
    assert gated.frontend_field_build_known(goal_xyz)[0].reachable == 1
    gated.frontend_build(mu._fe_cfg(pkg))
    _gone(pkg, gated)


def _valid(eng):
    return eng.frontend_field().shape == DIMS


def test_status_codes_and_their_order(pkg, product_lib):
    capi = pkg.capi
    E, S, U = capi.ISDF_ERR_INVALID_ARG, capi.ISDF_ERR_STATE, capi.ISDF_ERR_UNSUPPORTED
    bare = mu._engine(pkg, mu._clouds()[0], esdf=False, frontend=False)       # no front end, no known grid
    lib = bare.lib
    goal = (C.c_double * 3)(*_centre(GOAL))

    def call(h, g=goal, r=-1, border=0, max_rounds=0, want_info=True):
        e, p, info = capi.IsdfKnownErodeParams(r, border), capi.IsdfFrontendFieldParams(max_rounds, 0), capi.IsdfFrontendFieldInfo()
        rc = lib.isdf_frontend_field_build_known(h, g, C.byref(e), C.byref(p), C.byref(info) if want_info else None, None)
        return rc, (lib.isdf_last_error(h) or b"").decode()
    assert call(None, g=None, r=99, border=7, max_rounds=-1)[0] == E
    chain = [({"g": None}, E, "null goal"), ({"max_rounds": -1}, E, "max_rounds"), ({"border": 7}, E, "border"), ({"r": 99}, E, "radius")]
    for first in range(len(chain)):                              # every argument error, in its order, before the ctx's state is looked at
        kw = {}
        for more, _, _ in chain[first:]:
            kw.update(more)
        rc, msg = call(bare.h, **kw)
        assert rc == chain[first][1] and chain[first][2] in msg, (kw, msg)
    rc, msg = call(bare.h, want_info=False)
    assert rc == E and "null goal / info" in msg
    rc, msg = call(bare.h, r=-2)
    assert rc == E and "radius" in msg
    multi = pkg.Engine(pkg.synth.default_config(capi.V3_ESDF_TILE), devices=[0, 0])
    rc, msg = call(multi.h, r=99)
    assert rc == E and "radius" in msg
    rc, msg = call(multi.h)
    assert rc == U and "multi-device" in msg
    rc, msg = call(bare.h)
    assert rc == S and "isdf_frontend_build" in msg             # the front end before the known grid
    out = (C.c_int32 * 4)(9, 9, 9, 9)
    assert lib.isdf_frontend_field_known_info(bare.h, out) == 0 and list(out) == [0, 0, 0, 0]
    assert lib.isdf_frontend_field_known_info(bare.h, None) == E and lib.isdf_frontend_field_known_info(None, out) == E
    eng = mu._engine(pkg, mu._clouds()[0], esdf=False)
    rc, msg = call(eng.h)
    assert rc == S and "known grid" in msg
    with pytest.raises(pkg.IsdfError) as err:
        eng.frontend_field()
    assert err.value.code == S                                  # a refused build leaves no field
    eng.map_known_enable(True)
    assert call(eng.h)[0] == 0 and call(eng.h, r=64, border=1)[0] == 0
