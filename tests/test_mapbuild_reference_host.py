"""The references of the map-product edge tests, without a device: tests/mapbuild_reference.py against a brute-force minimum and
against the oracle's restatements (orc.build_esdf bit for bit in float64 on every EDT case, orc.gather_points on the small world of
tests/test_gpu_mapbuild.py), and every precondition of tests/mapbuild_cases.py.  What tests/test_gpu_mapbuild_edges.py holds the
kernels to is checked here."""
import numpy as np
import pytest

import mapbuild_cases as mc
import mapbuild_reference as mr
from common import small_world, traj


def test_exact_d2_is_the_brute_force_minimum():
    rng = np.random.default_rng(7)
    shapes = [(9, 8, 7), (1, 1, 7), (9, 1, 1), (1, 8, 1), (2, 3, 7), (9, 8, 1), (5, 5, 5), (3, 8, 2)]
    grids = [(rng.uniform(size=s) < p).astype(np.uint8) for s, p in zip(shapes, (0.05, 0.3, 0.2, 0.2, 0.1, 0.02, 0.5, 0.9))]
    grids += [np.zeros((9, 8, 7), dtype=np.uint8), np.ones((9, 8, 7), dtype=np.uint8)]
    assert len(grids) == 10
    for occ in grids:
        d2 = mr.exact_d2(occ)
        assert d2.dtype == np.int64 and np.array_equal(d2, mr.brute_d2(occ)), occ.shape
    assert np.all(mr.exact_d2(grids[-2]) == mr.NONE) and not mr.exact_d2(grids[-1]).any()


@pytest.mark.parametrize("gid", mc.EDT_IDS)
def test_edt_cases_equal_the_oracle_bit_for_bit(pkg, orc, gid):
    mc.holds(mc.edt_preconditions(pkg.synth, gid))
    for name, occ in mc.edt_maps(pkg.synth, gid).items():
        with np.errstate(over="ignore"):
            got = mr.esdf_from_d2(mc.edt_d2(pkg.synth, gid, name), mc.EDT_RES)
            want = orc.build_esdf(occ, mc.EDT_RES)
        assert got.dtype == want.dtype == np.float64
        assert got.tobytes() == want.tobytes(), (gid, name, int((got != want).sum()))


@pytest.mark.parametrize("offset", [None, (0.4, -0.3, 0.2)])
def test_gather_reference_equals_the_oracle(pkg, orc, offset):
    occ, _, res = small_world(pkg, seed=12)
    T, cm = traj(pkg, occ, res, N=7, seed=3)
    way = cm.reshape(3, -1).T.reshape(7, 6, 3)[1:, 0, :]
    way = np.concatenate([way, [[-2.0, 30.0, 7.0]], way[:1]])              # ... one outside the map, and a box seen before
    half = np.array([1.5, 1.2, 1.0])
    bmax = np.array(occ.shape) * res
    got = mr.gather_reference(occ, np.zeros(3), bmax, res, way, half, offset)
    want = orc.gather_points(occ, np.zeros(3), bmax, res, way, half, offset if offset is not None else (0, 0, 0))
    assert want.shape[0] > 0 and got.tobytes() == want.tobytes()
    # an origin that is no multiple of the resolution, and an explicit bmax short of the last voxel's face
    bmin = np.array([0.5, -1.0, 2.0])
    got = mr.gather_reference(occ, bmin, bmin + bmax - 0.2, res, way + bmin, half, offset)
    want = orc.gather_points(occ, bmin, bmin + bmax - 0.2, res, way + bmin, half, offset if offset is not None else (0, 0, 0))
    assert want.shape[0] > 0 and got.tobytes() == want.tobytes()


@pytest.mark.parametrize("name", mc.GATHER_IDS)
def test_gather_cases_reach_their_loops(name):
    mc.holds(mc.gather_preconditions(name))


def test_gather_g2_equals_the_oracle(orc):
    cs = mc.gather_case("G2")
    for run, way, off in cs["runs"]:
        want = orc.gather_points(cs["occ"], cs["bmin"], cs["bmax"], cs["res"], way, mc.gather_half(cs, run), off if off is not None else (0, 0, 0))
        assert mc.gather_want("G2", run)[1].tobytes() == want.tobytes(), run


@pytest.mark.parametrize("name", ["P1", "P2"])
def test_cloud_cases_reach_their_loops(orc, name):
    mc.holds(mc.cloud_preconditions(orc, name))
