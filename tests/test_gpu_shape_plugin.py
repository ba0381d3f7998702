"""isdf_shape_eval (csrc/shape_eval.hip, dev_shapes.hpp) of every analytic kind, pointwise, against the high-precision restatement of
the reference's classes (tests/shape_reference.py; the oracle is held to it on the CPU by tests/test_shape_reference_host.py).

Points per kind and body offset (identity / the rotated one of the parity tests): 2000 - uniform in a cube of half side 6, and 40 base
points on the formula's singular sets and switching surfaces (axes, symmetry planes, the origin, Cappedtorus' scy x = scx y,
CappedCone's paba = 0.5 and the clip of f at 0 and 1, RoundedCone's k = 0 and k = a h, BendLinear's clips, the spheres and faces),
each with the points +-1e-9, +-5e-6 (the gradient's own dx) and +-1e-3 beside it.

SDF bound: 8 x the ORACLE's largest error against the high-precision value, taken per kind, offset and class of points (uniform /
special: the special points of a kind with an axis are worse conditioned by orders of magnitude and would blunt the bound for the
uniform ones) - the device contracts and reorders the same operations and never does more of them; floor 16 ulp of
(|p| + largest parameter).  Nothing is measured against the device.  The gradient is compared with the high-precision value of the SAME
difference quotient (lo = c - dx, hi = lo + 2 dx; Box forward, not normalised), entry by entry within the SDF bound x 1 / (2 dx) /
|quotient|.  Points whose high-precision margin to a discontinuous decision is in (0, 1e-12) are left out, at most 2 % per kind (checked
on the CPU as well).

The oracle's largest SDF error (m) against the reference on these points, as measured on the CPU (printed again by every run):

    kind                identity offset          rotated offset
                        uniform    special       uniform    special
    Torus               1.3e-15    6.9e-16       2.3e-15    1.2e-15
    Cappedtorus         1.1e-14    9.4e-14       8.4e-15    1.1e-13
    CappedCone          1.2e-16    1.1e-16       2.0e-16    1.1e-16
    RoundedCone         2.1e-15    1.1e-15       2.5e-15    1.7e-15
    WireframeBox        1.0e-15    7.0e-16       1.9e-15    1.6e-15
    BendLinear          1.3e-15    6.8e-16       2.0e-15    1.2e-15
    TwistBox            1.4e-15    9.0e-16       3.0e-15    1.4e-15
    BendBox             1.5e-15    9.3e-16       2.3e-15    1.7e-15
    Table               1.4e-15    5.9e-16       2.1e-15    8.6e-16
    Trefoil             7.7e-16    5.0e-16       9.9e-16    4.8e-07   (1e-9 beside the axis, about which the value turns)
    SmoothDifference    1.1e-15    4.7e-16       1.8e-15    1.1e-15
    SmoothIntersection  1.4e-15    1.0e-15       2.3e-15    1.2e-15
    CSG                 1.4e-15    1.0e-15       2.3e-15    1.2e-15
    Box                 9.9e-16    1.0e-15       2.0e-15    1.1e-15
    Ball                1.4e-15    1.0e-15       1.4e-15    1.0e-15
"""
import numpy as np
import pytest

import shape_reference as sr
from common import BODY_OFFSETS, grad_bound, plugin_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("offset", list(BODY_OFFSETS))
@pytest.mark.parametrize("name", sr.KINDS)
def test_plugin_pointwise(pkg, orc, product_lib, name, offset):
    capi, synth = pkg.capi, pkg.synth
    sh, pts, special, tab, kept, floor = plugin_case(pkg, name, offset)
    cfg = synth.default_config(capi.V2_OCC_TILE)
    o = orc.Oracle(cfg)
    o.set_shape(sh)
    s0, _ = o.shape_eval(pts)
    e0 = sr.abs_err(s0, tab["sdf"])
    eng = pkg.Engine(cfg)
    eng.set_shape(sh)
    s, g = eng.shape_eval(pts)
    err = sr.abs_err(s, tab["sdf"])
    gerr = sr.abs_err(g, tab["grad"]).max(axis=1)
    bound = np.zeros(len(pts))
    line = f"\n[plugin] {name}/{offset}: left out {int((~kept).sum())}"
    for cls, mask in (("uniform", ~special), ("special", special)):
        k = kept & mask
        assert np.all(np.isfinite(e0[k])), (name, offset, cls, "the oracle is not finite on a kept point")
        bound[mask] = np.maximum(8.0 * e0[k].max(), floor[mask])
        line += f" | {cls}: oracle max error {e0[k].max():.2e}, device {err[k].max():.2e}"
    gb = grad_bound(name, bound, tab, pts)
    cmp = kept & np.isfinite(gb)
    print(line + f" | gradient: device max error / bound {np.max(gerr[cmp] / gb[cmp]):.2e}")
    bad = kept & ~(err <= bound)
    assert not bad.any(), (name, offset, "sdf", pts[bad][:3], s[bad][:3], err[bad][:3], bound[bad][:3])
    bad = cmp & ~(gerr <= gb)
    assert not bad.any(), (name, offset, "gradient", pts[bad][:3], g[bad][:3], gerr[bad][:3], gb[bad][:3])
    # consistency: without the gradient the same SDF bits; an empty input gives an empty output
    s1, g1 = eng.shape_eval(pts, want_grad=False)
    assert g1 is None and np.array_equal(s1.view(np.uint64), s.view(np.uint64))
    s2, g2 = eng.shape_eval(np.zeros((0, 3)))
    assert s2.shape == (0,) and g2.shape == (0, 3)
