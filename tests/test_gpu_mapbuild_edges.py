"""The device map products (csrc/map_build.hip: isdf_generate_esdf, isdf_gather_points, isdf_set_pointcloud) past the first trip of
their loops, against the exact references of tests/mapbuild_reference.py and the oracle's point-cloud binning.  The cases and what
each of them reaches are in tests/mapbuild_cases.py; tests/test_mapbuild_reference_host.py holds the references themselves.  Every
expectation is equality: integers, bytes and one correctly rounded square root."""
import numpy as np
import pytest

import mapbuild_cases as mc
import mapbuild_reference as mr

pytestmark = pytest.mark.gpu


def _same_esdf(esdf, d2, occ, res, what):
    with np.errstate(over="ignore"):
        want = mr.esdf_from_d2(d2, res).astype(np.float32)                 # the reference's double, stored as float32
    bad = np.argwhere(esdf != want)
    assert bad.shape[0] == 0, (what, bad.shape[0], bad[0].tolist(), float(esdf[tuple(bad[0])]), float(want[tuple(bad[0])]))
    assert np.array_equal(esdf == 0, occ != 0), what


@pytest.mark.parametrize("gid", mc.EDT_IDS)
def test_generate_esdf_exact(pkg, product_lib, gid):
    capi, synth = pkg.capi, pkg.synth
    mc.holds(mc.edt_preconditions(synth, gid))
    eng = pkg.Engine(synth.default_config(capi.V3_ESDF_TILE))               # one context per shape: every map after the first finds an ESDF
    for name, occ in mc.edt_maps(synth, gid).items():                       # of the previous occupancy in place and must not keep any of it
        eng.set_grid(occ, mc.EDT_ORIGIN, mc.EDT_RES, capi.GRID_OCCUPANCY)
        eng.generate_esdf()
        esdf, o, _ = eng.get_grid(capi.GRID_ESDF)
        assert esdf.shape == occ.shape and np.array_equal(o, mc.EDT_ORIGIN)
        _same_esdf(esdf, mc.edt_d2(synth, gid, name), occ, mc.EDT_RES, (gid, name))


@pytest.mark.parametrize("name", mc.GATHER_IDS)
def test_gather_points_exact(pkg, product_lib, name):
    capi, synth = pkg.capi, pkg.synth
    mc.holds(mc.gather_preconditions(name))
    cs = mc.gather_case(name)
    eng = pkg.Engine(synth.default_config(capi.V1_SWEPT))
    eng.set_grid(cs["occ"], cs["bmin"], cs["res"], capi.GRID_OCCUPANCY, bmax=cs["bmax"])
    for run, way, off in cs["runs"]:                                        # on ONE context: no mark of an earlier call may survive
        want = mc.gather_want(name, run)[1]
        M = eng.gather_points(way, mc.gather_half(cs, run), off)
        pts = eng.get_points()
        assert M == want.shape[0] and pts.shape == want.shape, (name, run, M, want.shape)
        bad = np.flatnonzero((pts != want).any(axis=1))
        assert bad.size == 0, (name, run, bad.size, pts[bad[0]].tolist(), want[bad[0]].tolist())
    if name == "G2":
        assert M == 0 and eng.get_points().shape == (0, 3)


def test_pointcloud_p1_chain(pkg, orc, product_lib):
    """600 000 points -> occupancy -> ESDF and gathered points, on one context"""
    capi, synth = pkg.capi, pkg.synth
    mc.holds(mc.cloud_preconditions(orc, "P1"))
    cs = mc.cloud_case("P1")
    occ0, b0, b1 = mc.cloud_want(orc, "P1")
    eng = pkg.Engine(synth.default_config(capi.V2_OCC_TILE))
    dims = eng.set_pointcloud(cs["P"], cs["res"], cs["thr"], bmin=cs["bmin"], bmax=cs["bmax"])
    occ, o, bm = eng.get_grid(capi.GRID_OCCUPANCY)
    assert dims == cs["dims"] == occ0.shape == occ.shape
    assert np.array_equal(o, b0) and np.array_equal(bm, b1)
    bad = np.argwhere(occ != occ0)
    assert bad.shape[0] == 0, (bad.shape[0], bad[0].tolist())
    eng.generate_esdf()
    esdf, _, _ = eng.get_grid(capi.GRID_ESDF)
    _same_esdf(esdf, mr.exact_d2(occ0), occ0, cs["res"], "P1")
    want = mr.gather_reference(occ0, cs["bmin"], cs["bmax"], cs["res"], cs["way"], cs["half"])
    M = eng.gather_points(cs["way"], cs["half"])
    assert M == want.shape[0] and M > 0
    assert np.array_equal(eng.get_points(), want)


def test_pointcloud_p2_threshold_zero(pkg, orc, product_lib):
    capi, synth = pkg.capi, pkg.synth
    mc.holds(mc.cloud_preconditions(orc, "P2"))
    cs = mc.cloud_case("P2")
    occ0, b0, b1 = mc.cloud_want(orc, "P2")
    eng = pkg.Engine(synth.default_config(capi.V2_OCC_TILE))
    dims = eng.set_pointcloud(cs["P"], cs["res"], cs["thr"], bmin=cs["bmin"], bmax=cs["bmax"])
    occ, o, bm = eng.get_grid(capi.GRID_OCCUPANCY)
    assert dims == cs["dims"] == occ0.shape == occ.shape
    assert np.array_equal(o, b0) and np.array_equal(bm, b1)
    assert np.array_equal(occ, occ0) and occ.all()
