"""The eroded known grid on the device (csrc/known_erode.hip: isdf_map_known_erode) against the plain host form, which
tests/test_known_erode_host.py holds to the NumPy restatement (tests/known_erode_reference.py).  The words and the integer words of the
info are compared with ==.  Grids, radii, borders and patterns are the host test's; the scan scene is tests/test_gpu_map_scan.py's, the
depth image tests/test_gpu_depth_cam.py's corridor."""
import ctypes as C

import numpy as np
import pytest

import known_erode_reference as er
import known_reference as kr
import test_gpu_depth_cam as dc
import test_gpu_map_scan as ms
import test_gpu_map_update as mu
from test_gpu_map_known import _grid_engine
from test_known_erode_host import BORDERS, GRIDS, IDS, RADII, big_radius, patterns, reference

pytestmark = pytest.mark.gpu


def _live(lib):
    out = (C.c_longlong * 2)()
    lib.isdf_debug_live_bytes(out)
    return list(out)


def _set_known(eng, k):
    """K on the device: everything known, then the unknown voxels one by one (all unknown: one fill)"""
    if not k.any():
        eng.map_known_fill(None, 0)
        return
    eng.map_known_fill(None, 1)
    for v in np.argwhere(~k):
        eng.map_known_fill(tuple(int(c) for c in v) * 2, 0)


def _same(pkg, lib, eng, r, border, k=None, want=None):
    """the device against the host form on the device's own K; returns E as booleans"""
    bits = eng.map_known()[0]
    dims = eng._grid_dims()
    if k is not None:
        assert np.array_equal(bits, kr.pack(k))
    host = pkg.engine.known_erode_host(bits, dims, r, border, lib=lib)
    got, info = eng.known_erode(r, border)
    assert got.dtype == np.uint32 and np.array_equal(got, host), (r, border)
    e = kr.unpack(got, dims)                                    # (asserts the tail bits)
    assert (info.radius_used, info.border, info.known_voxels, info.eroded_voxels) == (r, border, int(kr.unpack(bits, dims).sum()), int(e.sum()))
    assert info.erode_ms >= 0.0
    if want is not None:
        assert np.array_equal(e, want), (r, border)
    return e


@pytest.mark.parametrize("dims", GRIDS, ids=IDS)
def test_the_device_equals_the_host_form(pkg, product_lib, dims):
    eng, _ = _grid_engine(pkg, dims)
    with pytest.raises(pkg.engine.IsdfError) as e:
        eng.known_erode(1, 0)
    assert e.value.code == pkg.capi.ISDF_ERR_STATE              # no known grid
    eng.map_known_enable(True)
    for name, k in patterns(dims):
        _set_known(eng, k)
        for border in BORDERS:
            for r in RADII + (big_radius(dims),):
                _same(pkg, product_lib, eng, r, border, k=k, want=reference(dims, name, k, r, border))


def _depth_engine(pkg):
    """the scan tests' map, K as one integrated depth image of the corridor leaves it"""
    eng = mu._engine(pkg, ms._scene()[0], esdf=False, frontend=False)
    eng.map_known_enable(True)
    cam = dc._cam(pkg, dc.WIDE)
    p12 = dc.ref.pose(dc.ref.rot(0.05, 0.1, -0.2), [5.2, 7.1, 14.0])
    image, _ = eng.depth_render(cam, p12, dc._corridor(), splat_m=0.15)
    eng.integrate_depth(cam, p12, image, max_range_m=9.0, no_return_is_free=True, min_range_m=0.3)
    return eng


def test_after_a_depth_merge_and_after_a_shift(pkg, product_lib):
    eng = _depth_engine(pkg)
    k = kr.unpack(eng.map_known()[0], ms.DIMS)
    assert eng.map_known()[1].merges == 1 and 1000 < k.sum() < k.size
    for border in BORDERS:
        for r in (0, 1, 2):
            e = _same(pkg, product_lib, eng, r, border, want=er.erode(k, r, border))
            assert r == 0 or e.sum() < k.sum()
            assert r == 2 or e.any()
    s = (2, -3, 5)
    eng.shift_map(s)
    k2 = kr.shift(k, s)
    entered = ~kr.shift(np.ones(ms.DIMS, dtype=bool), s)        # the slabs that entered: unknown
    assert entered.any() and not (k2 & entered).any()
    for border in BORDERS:
        for r in (1, 2):
            e = _same(pkg, product_lib, eng, r, border, k=k2, want=er.erode(k2, r, border))
            assert not (e & ~er.erode(~entered, r, 1)).any()                    # the entering slab is eroded inwards by r, whatever the border


def test_no_bits_two_calls_and_no_allocation(pkg, product_lib):
    eng = _depth_engine(pkg)
    lib, E = eng.lib, pkg.capi
    p = E.IsdfKnownErodeParams(2, 0)
    first, info1 = eng.known_erode(2, 0)
    live = _live(product_lib)
    info = E.IsdfKnownErodeInfo()
    assert lib.isdf_map_known_erode(eng.h, C.byref(p), None, C.byref(info)) == 0                 # bits_out = NULL: the counts alone
    assert (info.radius_used, info.border, info.known_voxels, info.eroded_voxels) == (2, 0, info1.known_voxels, info1.eroded_voxels)
    out = np.zeros_like(first)
    assert lib.isdf_map_known_erode(eng.h, C.byref(p), out.ctypes.data_as(C.c_void_p), None) == 0        # info_out = NULL
    assert np.array_equal(out, first)
    assert lib.isdf_map_known_erode(eng.h, None, None, None) == E.ISDF_ERR_STATE                # the default radius -1 needs a front end
    second, info2 = eng.known_erode(2, 0)
    assert second.tobytes() == first.tobytes() and (info2.known_voxels, info2.eroded_voxels) == (info1.known_voxels, info1.eroded_voxels)
    for r, border in ((1, 1), (0, 0), (2, 1)):                   # a smaller radius, the one-launch radius: nothing grows
        eng.known_erode(r, border)
    assert _live(product_lib) == live
    eng.map_known_enable(False)                                  # the scratch goes with the grid
    assert _live(product_lib)[0] < live[0]


def test_the_call_is_read_only(pkg, product_lib):
    """the scan tests' map with every product, a valid (ungated) cost-to-go field, an armed watch and a kept report; K from one scan's merge"""
    from test_gpu_map_clear import N, _same_report
    capi = pkg.capi
    old, ends, hit = ms._scene()
    eng, _ = ms._watched(pkg, old, 1)
    eng.map_known_enable(True)
    eng.integrate_scan(ms.ORIGIN, ends, hit, miss_weight=ms.MISS)
    assert eng.frontend_field_build(eng_goal(eng)).reachable == 1

    def state():
        bits, info = eng.map_known()
        return bits.tobytes(), eng.get_grid(capi.GRID_OCCUPANCY)[0].tobytes(), info.merges, info.newly_known, info.n_known
    before = state()
    products = mu._products(pkg, eng)
    field, kept_report = eng.frontend_field(), eng.traj_check_points().tobytes()
    rep_a, last_a = eng.traj_check_watch_info(N)
    for r in (-1, 1):                                           # -1: the front end's footprint, (5 - 1) / 2
        e = _same(pkg, product_lib, eng, mu.SIDE if r < 0 else r, 0)
        got, info = eng.known_erode(r, 0)
        assert np.array_equal(kr.unpack(got, ms.DIMS), e) and info.radius_used == (mu.SIDE if r < 0 else r)
    assert state() == before and before[2] == 1
    mu._same(mu._products(pkg, eng), products)
    assert np.array_equal(eng.frontend_field().view(np.uint8), field.view(np.uint8)) and eng.frontend_field_known_info() == (0, 0, 0)
    rep_b, last_b = eng.traj_check_watch_info(N)
    _same_report(rep_b, rep_a, "after the erosion")
    assert last_b == last_a and eng.traj_check_points().tobytes() == kept_report
    assert eng.points_merge_check()["n_added"] >= 0             # the kept report is not stale: the grid epoch did not move


def eng_goal(eng):
    free = eng.frontend_cspace_table().any(axis=3)
    return (np.argwhere(free)[len(np.argwhere(free)) // 2] + 0.5) * ms.RES + ms.BMIN


def test_status_codes_and_their_order(pkg, product_lib):
    capi = pkg.capi
    E, S, U = capi.ISDF_ERR_INVALID_ARG, capi.ISDF_ERR_STATE, capi.ISDF_ERR_UNSUPPORTED
    eng, _ = _grid_engine(pkg, GRIDS[0])                          # no known grid, no front end
    lib = eng.lib

    def call(h, r, border):
        p = capi.IsdfKnownErodeParams(r, border)
        rc = lib.isdf_map_known_erode(h, C.byref(p), None, None)
        return rc, (lib.isdf_last_error(h) or b"").decode()
    assert call(None, 99, 7)[0] == E                             # a null ctx first
    for (r, border), (code, word) in (((99, 7), (E, "border")), ((99, 1), (E, "radius")), ((-2, 0), (E, "radius")), ((-1, 0), (S, "no known grid")), ((1, 0), (S, "no known grid"))):
        rc, msg = call(eng.h, r, border)
        assert rc == code and word in msg, (r, border, msg)
    multi = pkg.Engine(pkg.synth.default_config(capi.V3_ESDF_TILE), devices=[0, 0])
    rc, msg = call(multi.h, 99, 0)
    assert rc == E and "radius" in msg                           # the arguments before the ctx's kind ...
    rc, msg = call(multi.h, -1, 0)
    assert rc == U and "multi-device" in msg                     # ... which comes before the state
    eng.map_known_enable(True)
    rc, msg = call(eng.h, -1, 0)
    assert rc == S and "isdf_frontend_build" in msg              # with a known grid: radius -1 needs the front end
    assert call(eng.h, 64, 1)[0] == 0 and call(eng.h, 0, 0)[0] == 0
