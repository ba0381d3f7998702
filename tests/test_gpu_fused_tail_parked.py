"""The fused step's tail parks what it forms before the collision sums arrive - basis rows, jerk, snap - in its thread's own row of
the partial-sum array (tile_sweep.hip, tail_piece).  Held here at the edges of that layout: the fused launch against the
two-launch path byte for byte, over an empty map and without the dynamics penalties against the oracle as well, no state left in
the shared array between steps, and the rounded cone's fused instantiation.

Both paths run in a fresh child process each (tests/fused_tail_parked_worker.py; ISDF_NO_FUSE is read at isdf_create).  That a
step was ONE fused launch shows in how it crossed PCIe: only such a step is handed over host-direct (include/isdf_accel.h,
isdf_host_path), as in tests/test_gpu_dyn_edges.py.

K + 1 = 1 is no case: isdf_create refuses integral_intervs < 1 (the integration step is T / K), which is asserted instead."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fused_tail_parked_worker as w
from common import REL_TOL, assert_close

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(K1, N) for K1 in w.K1S for N in w.NS]


@pytest.fixture(scope="module")
def runs(tmp_path_factory, product_lib):
    """(fused, two-launch): the worker's results, one child process each."""
    d = tmp_path_factory.mktemp("fused_tail_parked")
    out = []
    for tag, no_fuse in (("fused", False), ("two_launch", True)):
        env = dict(os.environ)
        for k in ("ISDF_NO_FUSE", "ISDF_NO_HOST_DIRECT", "ISDF_FUSE_MAX_BLOCKS"):
            env.pop(k, None)
        if no_fuse:
            env["ISDF_NO_FUSE"] = "1"
        path = str(d / (tag + ".npz"))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fused_tail_parked_worker.py"), path], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "RESULT ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
        out.append(dict(np.load(path)))
    return out


@pytest.fixture(scope="module")
def scene(pkg):
    occ, esdf = w.world(pkg)
    return occ, {"boxes": esdf, "empty": w.empty_esdf()}


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def fused_vs_two_launch(pkg, runs, name, N):
    fused, two = runs
    direct = (pkg.capi.HOST_PATH_DIRECT_BAR, pkg.capi.HOST_PATH_DIRECT_MAPPED)
    assert int(fused[name + "/host_path"]) in direct, (name, "one fused launch expected")
    assert int(two[name + "/host_path"]) not in direct, (name, "two launches expected")
    assert fused[name].shape == (1 + 19 * N,) and np.all(np.isfinite(fused[name])), name
    diff = np.flatnonzero(fused[name].view(np.uint64) != two[name].view(np.uint64))
    assert same_bytes(fused[name], two[name]), (name, "outputs differ at", diff[:8].tolist(), fused[name][diff[:8]], two[name][diff[:8]])


def against_oracle(pkg, orc, scene, runs, name):
    m, K1, N, dyn, shp, seed = w.cases()[name]
    occ, grids = scene
    o = orc.Oracle(w.config(pkg, K1, dyn), threads=4)
    o.set_grid(grids[m], (0, 0, 0), w.RES, pkg.capi.GRID_ESDF)
    o.set_shape(w.shape(pkg, shp))
    T, cm = w.trajectory(pkg, occ, N, seed)
    c0, gT0, gC0, st0 = o.eval(T, cm)
    got = runs[0][name]
    assert abs(got[0] - c0) <= REL_TOL * max(abs(c0), 1e-9), (name, got[0], c0)
    assert_close(got[1:1 + N], gT0, name + " gradT")
    assert_close(got[1 + N:], gC0, name + " gradC")
    return st0


@pytest.mark.parametrize("K1,N", SHAPES)
def test_fused_equals_two_launch_at_the_layout_edges(pkg, runs, K1, N):
    name = f"boxes_K1_{K1}_N{N}"
    fused_vs_two_launch(pkg, runs, name, N)
    if K1 >= 63:
        assert int(runs[0][name + "/grad_pairs"]) > 0, (name, "the scenario must exercise the collision branch")


@pytest.mark.parametrize("K1,N", SHAPES)
def test_collision_free(pkg, orc, scene, runs, K1, N):
    """Over an empty map the sums arrive as zeros: the `a[0] > 0` branch is never taken."""
    name = f"empty_K1_{K1}_N{N}"
    fused_vs_two_launch(pkg, runs, name, N)
    assert int(runs[0][name + "/grad_pairs"]) == 0
    against_oracle(pkg, orc, scene, runs, name)


@pytest.mark.parametrize("K1,N", SHAPES)
def test_collision_only(pkg, orc, scene, runs, K1, N):
    """enable_dyn = 0: the collision sums are all the reverse mode gets."""
    name = f"nodyn_K1_{K1}_N{N}"
    fused_vs_two_launch(pkg, runs, name, N)
    st0 = against_oracle(pkg, orc, scene, runs, name)
    assert int(runs[0][name + "/grad_pairs"]) == st0[3]


@pytest.mark.parametrize("which", [0, 1], ids=["fused", "two_launch"])
def test_no_state_left_in_the_shared_area(runs, which):
    """Trajectory A, then B, then A on one engine: a tail thread that read a value parked by an earlier step, or by another role's use
    of the same LDS, would not give A's bytes twice."""
    r = runs[which]
    assert not same_bytes(r["aba_A1"], r["aba_B"])
    assert same_bytes(r["aba_A1"], r["aba_A2"])
    assert same_bytes(runs[0]["aba_B"], runs[1]["aba_B"])


def test_rounded_cone_fused_instantiation(pkg, runs):
    fused_vs_two_launch(pkg, runs, "cone_K1_65_N3", 3)
    assert int(runs[0]["cone_K1_65_N3/grad_pairs"]) > 0


def test_a_single_sample_per_piece_is_refused(pkg, product_lib):
    with pytest.raises(Exception):
        pkg.Engine(w.config(pkg, 1))
