"""CPU: the oracle's analytic shape formulas (oracle/shapes.hpp) held to the high-precision restatement of the reference's classes
(tests/shape_reference.py, mpmath at 50 digits) on the points the device plugin test uses (tests/test_gpu_shape_plugin.py) - so that
what the device is later compared with is itself pinned, and the share of points that test leaves out is checked without a device.

Bound of the oracle's SDF: 4096 ulp of (|p| + largest parameter).  The formulas are 20-40 fp64 operations; the worst conditioned
step is a root of a radicand that sums squares of magnitude (|p| + parameter)^2 ~ 150 and can be as small as a tube radius squared,
0.3^2 (Cappedtorus: dot(p, p) + ra^2 - 2 ra k): 150 / 0.09 ~ 2^11 times a few roundings.  Measured: <= 60 ulp.  Points next to a
discontinuous decision (margin m < 1: CappedCone, Trefoil; shape_reference.py) get that bound / m: an fp64 body offset moves a point
by an ulp of |p|, and the value turns with the point's angle about the axis, which that shift changes by ulp / m."""
import numpy as np
import pytest

import shape_reference as sr
from common import BODY_OFFSETS, LEFT_OUT_MAX, grad_bound, plugin_case


@pytest.mark.parametrize("offset", list(BODY_OFFSETS))
@pytest.mark.parametrize("name", sr.KINDS)
def test_oracle_matches_high_precision_reference(pkg, orc, name, offset):
    sh, pts, special, tab, kept, floor = plugin_case(pkg, name, offset)
    assert 1.0 - kept.mean() <= LEFT_OUT_MAX, (name, offset, "too many points next to a discontinuous decision", int((~kept).sum()))
    o = orc.Oracle(pkg.synth.default_config(pkg.capi.V2_OCC_TILE))
    o.set_shape(sh)
    s, g = o.shape_eval(pts)
    assert np.all(np.isfinite(s[kept])), (name, offset, pts[kept][~np.isfinite(s[kept])][:3])
    err = sr.abs_err(s, tab["sdf"])
    with np.errstate(divide="ignore"):          # (margin exactly 0: the decision sits on its switch in fp64 too, e.g. on the axis)
        bound = 256 * floor / np.minimum(tab["margin"], 1.0)
    bad = kept & (err > bound)
    print(f"\n[oracle vs reference] {name}/{offset}: left out {int((~kept).sum())}, max sdf error random {err[kept & ~special].max():.2e} "
          f"special {err[kept & special].max():.2e}")
    assert not bad.any(), (name, offset, pts[bad][:3], err[bad][:3], bound[bad][:3])
    gb = grad_bound(name, bound, tab, pts)
    gerr = sr.abs_err(g, tab["grad"]).max(axis=1)
    bad = kept & np.isfinite(gb) & ~(gerr <= gb)
    assert not bad.any(), (name, offset, pts[bad][:3], gerr[bad][:3], gb[bad][:3])


def test_reference_values_at_known_points():
    """The restatement against values known in closed form (no code involved)."""
    import mpmath as mp
    S = sr.Shape("Torus", (2.5, 0.3))
    assert abs(S.sdf((2.5, 0.0, 0.0))[0] + mp.mpf(0.3)) < mp.mpf(10) ** -45 and abs(S.sdf((0.0, 4.0, 0.0))[0] - (mp.sqrt(mp.mpf(2.5) ** 2 + 16) - mp.mpf(0.3))) < mp.mpf(10) ** -45
    S = sr.Shape("Box", (3.0, 0.3, 0.3))
    assert S.sdf((4.0, 0.0, 0.0))[0] == 1 and S.sdf((0.0, 0.0, 0.0))[0] == mp.mpf(-0.3)
    assert S.sdf((4.0, 1.3, 0.0))[0] == mp.sqrt(1 + (mp.mpf(1.3) - mp.mpf(0.3)) ** 2)
    S = sr.Shape("Ball", (1.0,), trans=(5, 5, 5))
    assert S.sdf((3.0, 4.0, 0.0))[0] == 4                      # Ball ignores the body offset
    S = sr.Shape("RoundedCone", (1.5, 0.6, 4.5))
    assert S.sdf((0.0, 0.0, -2.0))[0] == mp.mpf(0.5) and abs(S.sdf((0.0, 0.0, 6.0))[0] - mp.mpf(1.5) + mp.mpf(0.6)) < mp.mpf(10) ** -45
    S = sr.Shape("CappedCone", (2.0, 0.8, 0, 0, -1, 0, 0, 1))
    v, m = S.sdf((0.0, 0.0, 0.0))                              # on the axis, mid-height: the decision paba < 0.5 sits exactly on its switch
    assert m == 0 and v < 0
    S = sr.Shape("Torus", (2.5, 0.3), trans=(1, 0, 0), rotate=(0, -1, 0, 1, 0, 0, 0, 0, 1))       # (p - trans) * Rotate
    assert abs(S.sdf((1.0, 2.5, 0.0))[0] + mp.mpf(0.3)) < mp.mpf(10) ** -45
