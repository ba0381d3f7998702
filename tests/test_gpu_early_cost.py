"""A fused single-GPU step whose results stay on the device publishes each piece's cost as soon as the collision sums of its samples
are taken, before the reverse mode (tile_sweep.hip, tail_piece: `early_cost`), so that the hand-over to the collector runs under
the rest of the tail.  No bit may move: held here through isdf_eval_device against the two-launch path byte for byte - at the
sample counts where the early sum's row groups are empty, exactly full and ragged, with one piece (the collector takes its own
early cost), several, and more pieces than the collector has lanes - over an empty map and without the collision term against the
oracle as well, for the rounded cone's instantiation, for cost slots handed back empty between steps, and against a host-pointer
call on the same engine, which keeps the late order.

Both paths run in a fresh child process each (tests/early_cost_worker.py; ISDF_NO_FUSE is read at isdf_create).  That a step of a
case's engine is ONE fused launch shows in how its host-pointer call crossed PCIe: only such a step is handed over host-direct
(include/isdf_accel.h, isdf_host_path), as in tests/test_gpu_fused_tail_parked.py.  A step without the collision term has no sweep
launch and never fuses: that case checks that the cost still appears, on the path both runs share."""
import os
import subprocess
import sys

import numpy as np
import pytest

import early_cost_worker as w
from common import REL_TOL, assert_close

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def runs(tmp_path_factory, product_lib):
    """(fused, two-launch): the worker's results, one child process each."""
    d = tmp_path_factory.mktemp("early_cost")
    out = []
    for tag, no_fuse in (("fused", False), ("two_launch", True)):
        env = dict(os.environ)
        for k in ("ISDF_NO_FUSE", "ISDF_NO_HOST_DIRECT", "ISDF_FUSE_MAX_BLOCKS", "ISDF_DEBUG_TIMING"):
            env.pop(k, None)
        if no_fuse:
            env["ISDF_NO_FUSE"] = "1"
        path = str(d / (tag + ".npz"))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "early_cost_worker.py"), path], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "RESULT ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
        out.append(dict(np.load(path)))
    return out


@pytest.fixture(scope="module")
def scene(pkg):
    occ, esdf = w.world(pkg)
    return occ, {"boxes": esdf, "empty": w.empty_esdf()}


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_same(a, b, what):
    diff = np.flatnonzero(a.view(np.uint64) != b.view(np.uint64)) if a.shape == b.shape else None
    assert same_bytes(a, b), (what, "outputs differ at", None if diff is None else (diff[:8].tolist(), a[diff[:8]], b[diff[:8]]))


def fused_vs_two_launch(pkg, runs, name, fuses=True):
    fused, two = runs
    N = w.cases()[name][2]
    direct = (pkg.capi.HOST_PATH_DIRECT_BAR, pkg.capi.HOST_PATH_DIRECT_MAPPED)
    if fuses:
        assert int(fused[name + "/host_path"]) in direct, (name, "one fused launch expected")
    else:
        assert int(fused[name + "/host_path"]) not in direct, (name, "a step without a sweep launch does not fuse")
    assert int(two[name + "/host_path"]) not in direct, (name, "two launches expected")
    for r in runs:
        assert int(r[name + "/overflow_device"]) == 0 and int(r[name + "/overflow_host"]) == 0, (name, "a bounded poll gave up")
    got = fused[name]
    assert got.shape == (1 + 19 * N,) and np.all(np.isfinite(got)), (name, got[:4])
    assert_same(got, two[name], name + ": fused device-resident step against two launches")
    # the host-pointer call on the same engine: the late order, the same bytes (isdf_eval ADDS a step's outputs into the caller's
    # arrays, zeros here - the same addition is made to the device-resident outputs); and the device-resident step after it
    assert_same(got + 0.0, fused[name + "/host"], name + ": device-resident step against the host-pointer call")
    assert_same(got, fused[name + "/again"], name + ": the step after the host-pointer call")
    assert_same(two[name] + 0.0, two[name + "/host"], name + ": two launches, device-resident against host-pointer")


def against_oracle(pkg, orc, scene, runs, name):
    m, K1, N, dyn, pos, shp, seed, vmax = w.cases()[name]
    occ, grids = scene
    o = orc.Oracle(w.config(pkg, K1, dyn, pos, vmax), threads=4)
    o.set_grid(grids[m], (0, 0, 0), w.RES, pkg.capi.GRID_ESDF)
    o.set_shape(w.shape(pkg, shp))
    T, cm = w.trajectory(pkg, occ, N, seed)
    c0, gT0, gC0, st0 = o.eval(T, cm)
    got = runs[0][name]
    assert abs(got[0] - c0) <= REL_TOL * max(abs(c0), 1e-9), (name, got[0], c0)
    assert_close(got[1:1 + N], gT0, name + " gradT")
    assert_close(got[1 + N:], gC0, name + " gradC")
    return c0, st0


@pytest.mark.parametrize("K1", w.K1S)
def test_sample_counts(pkg, runs, K1):
    """Fewer rows than row groups (2, 5), one row per group (6), ragged groups (7, 65), the pass limit (127, 128)."""
    name = f"boxes_K1_{K1}_N3"
    fused_vs_two_launch(pkg, runs, name)
    if K1 >= 65:
        assert int(runs[0][name + "/grad_pairs"]) > 0, (name, "the scenario must exercise the collision branch")


def test_single_piece_collector_takes_its_own_early_cost(pkg, runs):
    fused_vs_two_launch(pkg, runs, "boxes_K1_65_N1")
    assert int(runs[0]["boxes_K1_65_N1/grad_pairs"]) > 0


def test_more_pieces_than_collector_lanes(pkg, runs):
    """N = 65: the collector's lane 0 takes a second slot (k += 64)."""
    fused_vs_two_launch(pkg, runs, "boxes_K1_7_N65")


def test_empty_map(pkg, orc, scene, runs):
    """The sums arrive as zeros: the cost is the dynamics penalties' alone."""
    fused_vs_two_launch(pkg, runs, "empty_K1_65_N3")
    assert int(runs[0]["empty_K1_65_N3/grad_pairs"]) == 0
    against_oracle(pkg, orc, scene, runs, "empty_K1_65_N3")


def test_no_poll(pkg, orc, scene, runs):
    """enable_pos = 0: no collision sums to wait for; the cost still appears."""
    fused_vs_two_launch(pkg, runs, "nopos_K1_65_N3", fuses=False)
    c0, _ = against_oracle(pkg, orc, scene, runs, "nopos_K1_65_N3")
    assert c0 > 0.0, "the scenario must have a dynamics cost"


def test_no_dynamics(pkg, orc, scene, runs):
    """enable_dyn = 0: the collision sums are all the cost is made of."""
    fused_vs_two_launch(pkg, runs, "nodyn_K1_65_N3")
    c0, st0 = against_oracle(pkg, orc, scene, runs, "nodyn_K1_65_N3")
    assert int(runs[0]["nodyn_K1_65_N3/grad_pairs"]) == st0[3] and c0 > 0.0


@pytest.mark.parametrize("which", [0, 1], ids=["fused", "two_launch"])
def test_cost_slots_are_handed_back_empty(runs, which):
    """Trajectory A, then B, then A on one engine: a cost slot that kept a value, or a collector that took a stale one, would not
    give A's bytes twice."""
    r = runs[which]
    assert not same_bytes(r["aba_A1"], r["aba_B"])
    assert same_bytes(r["aba_A1"], r["aba_A2"])
    assert same_bytes(runs[0]["aba_B"], runs[1]["aba_B"])
    assert same_bytes(runs[0]["aba_A1"], runs[0]["boxes_K1_65_N3"])       # (the same trajectory on a fresh engine)


def test_rounded_cone_fused_instantiation(pkg, runs):
    fused_vs_two_launch(pkg, runs, "cone_K1_65_N3")
    assert int(runs[0]["cone_K1_65_N3/grad_pairs"]) > 0
