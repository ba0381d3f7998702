"""The tile sweep's three stages in front of the fp64 exact pass - whole-tile cull (bound_radius), row pruning (bbox) and the
fp32 pre-filter - may only drop voxels that provably carry no penalty.  Every analytic kind is installed five times on engines of
one process and the COUNT of active voxels (grad_pairs) must be the same in all five and the oracle's:

    (a) all stages on: bbox, bound_radius, filter        (b) (a) + ISDF_NO_F32_FILTER=1        (c) (a) + ISDF_NO_ROW_PRUNE=1
    (d) (a) without bound_radius                          (e) no bbox, no bound_radius, filter off: every stage off

Both switches are read by isdf_set_shape, so one process runs all sides.  Cost agrees within 1e-12 relative between any two runs
(the same non-negative fp64 terms in other groupings: 1e4 terms x 1.1e-16), gradients entry by entry within 1e-10 x the largest
|entry| of the array (a factor 100 for cancellation among signed terms).  A wrongly dropped voxel next to the band's edge changes
the cost by ~1e-9 relative - invisible at the parity tests' 1e-5, visible here as a count.

bbox and bound_radius are computed here, on the CPU, from the oracle's SDF on a body-frame lattice over the tile cube (spacing h):
the box of the nodes with sdf <= 0 and the largest |p| - sdf(p), each grown until the contract of include/isdf_accel.h
(sdf(p) >= dist(p, box), sdf(p) >= |p| - R) holds at EVERY node out to bd / 2 with a margin of h sqrt(3) - several kinds are no
distance functions (twist, bend, Trefoil's 0.4 scale, CappedCone's sqrt(d) / |baba|, the smooth ops), so containment alone does
not give it.  The nodes reach only to the tile cube (the sweep looks at nothing outside it), so a finite box always exists: at
worst the cube itself; no kind needs bbox zeros.

The second test puts voxel centres ON the shapes' singular sets: a one-piece hover (only the constant coefficient, at a voxel
centre: zero acceleration, identity attitude, identity body offset) in a map that is half occupied at random (a fully occupied
one is symmetric and every gradient cancels to rounding noise), with the three body axes through the hover point occupied, so that
the body-frame points of the filter and of the exact pass are exact multiples of the voxel size - on the axis of Torus, Trefoil and
CappedCone, on the symmetry planes of WireframeBox and Table, at p.x = 0 of Cappedtorus, at angle 0 of TwistBox / BendBox, at k = 0
of RoundedCone and, with h = 3.0 = 6 voxels (the reference's h = 4.5 puts k = a h outside the tile), at k = a h and in the r2 cap.
The band's edge is laid through a voxel: safety_hor = the oracle's SDF at the voxel nearest 0.5 m, and that +- 1 mm and +- 3 mm, so
voxels sit at the edge exactly and inside the filter's 2 mm slack on both sides.  Default parameters and one thin variant per kind
(tube / radius 0.02).

Two deviations from plain equality with the oracle, both decided on the CPU from the oracle and the high-precision restatement
alone (DESIGN.md section 6 has the lists and figures):
  - With the edge laid exactly through voxels (+- 0 mm), `sdf < safety_hor` hangs on the last bit of the fp64 SDF, which device and
    oracle need not share: there the device's count is bracketed by the oracle's counts 1e-12 below and above the edge - looser than
    the equality asked for by the number of voxels on the edge (24 of 582 for Cappedtorus), equality again wherever the two counts
    coincide.  The five runs must agree with each other exactly everywhere.
  - Voxels at which the class's difference quotient all but vanishes have no reference gradient (the normalised gradient is rounding
    noise blown up to a direction; the oracle's own is off the exact quotient by 2e-5 ... 2).  They stay in the map for the five runs
    - counts against the oracle's, cost, run against run - and only the comparison of run (a)'s gradients with the oracle's is made
    on a second map without them (at most 8 voxels per case, printed).
Parameter sets with a NaN in the reference formula itself are not here (CappedCone as a needle along a long axis, baba = 36).

Every case prints which stages really ran: voxels the row pruning kept off the list, voxels the filter rejected, poses culled."""
import functools

import numpy as np
import pytest

import shape_reference as sr
from common import ALL_KINDS, BODY_OFFSETS, REL_TOL, assert_close, grad_bound, sdf_floor, small_world, traj

pytestmark = pytest.mark.gpu

_NAMES = ALL_KINDS + ["Torus_big", "BendLinear_big", "SmoothIntersection_big"]
_OFFSETS = BODY_OFFSETS
_CASES = [(n, "V3") for n in _NAMES] + [(n, "V2") for n in ("Torus", "CappedCone", "Trefoil", "TwistBox")]
_LATTICE_N = 51                 # nodes per axis over the tile cube
_RUNS = {                       # tag: (bbox, bound_radius, environment)
    "a": (True, True, ()),
    "b": (True, True, ("ISDF_NO_F32_FILTER",)),
    "c": (True, True, ("ISDF_NO_ROW_PRUNE",)),
    "d": (True, False, ()),
    "e": (False, False, ("ISDF_NO_F32_FILTER",)),
}
_SWITCHES = ("ISDF_NO_F32_FILTER", "ISDF_NO_ROW_PRUNE")


def _shape(pkg, name, params, pp, **kw):
    return pkg.synth.make_shape(name, params=params, poly_params=pp, **kw)


_HINTS = {}


def _hints(pkg, orc, name, params, pp, bd_half):
    """((centre, half), radius) satisfying the contract of isdf_shape.bbox_* / bound_radius at every lattice node of the tile cube,
    with a margin of h sqrt(3) (what a 1-Lipschitz SDF can change between a point and its nearest node, both ways)."""
    key = (name, params, pp, bd_half)
    if key in _HINTS:
        return _HINTS[key]
    ax = np.linspace(-bd_half, bd_half, _LATTICE_N)
    h = ax[1] - ax[0]
    P = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), axis=-1).reshape(-1, 3)
    o = orc.Oracle(pkg.synth.default_config(pkg.capi.V2_OCC_TILE))
    o.set_shape(_shape(pkg, name, params, pp))
    sdf, _ = o.shape_eval(P)
    assert np.all(np.isfinite(sdf)), (name, params, pp, "the oracle's SDF is not finite on the lattice")
    inside = sdf <= 0.0
    if not inside.any():                           # thinner than the lattice: start from the node nearest the surface
        inside = sdf == sdf.min()
    lo, hi = P[inside].min(axis=0), P[inside].max(axis=0)

    def dist(lo, hi):
        return np.linalg.norm(np.maximum(np.maximum(lo - P, P - hi), 0.0), axis=1)
    margin = h * np.sqrt(3.0)
    grow = max(float(np.max(dist(lo, hi) - sdf)), 0.0) + margin      # inflating by e shortens every outside node's distance by >= e
    lo, hi = lo - grow, hi + grow
    d = dist(lo, hi)
    assert np.all((d == 0.0) | (sdf >= d + margin - 1e-12)), (name, "bbox contract")          # every node outside the box
    r = np.linalg.norm(P, axis=1)
    R = float(np.max(r - sdf)) + margin
    assert np.all(sdf >= r - R + margin - 1e-12), (name, "bound_radius contract")
    _HINTS[key] = ((tuple(0.5 * (lo + hi)), tuple(0.5 * (hi - lo))), R)
    return _HINTS[key]


def _five_runs(pkg, monkeypatch, cfg, set_grids, name, params, pp, bbox, radius, T, cm):
    out = {}
    for tag, (with_box, with_radius, env) in _RUNS.items():
        for k in _SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k in env:
            monkeypatch.setenv(k, "1")
        eng = pkg.Engine(cfg)
        set_grids(eng)
        eng.set_shape(_shape(pkg, name, params, pp, bbox=bbox if with_box else None, bound_radius=radius if with_radius else 0.0))
        c, gT, gC = eng.eval_single(T, cm)
        out[tag] = (float(c), np.array(gT, copy=True), np.array(gC, copy=True), eng.stats())
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    return out


def _assert_stages_change_nothing(what, name, runs, oracle, active_range=None, oracle_grads=True):
    """runs: tag -> (cost, gradT, gradC, stats); oracle: (cost, gradT, gradC, st0) of the shape without any hint.  active_range: the
    oracle's count of active voxels just below and just above a band's edge that was laid THROUGH voxels (see the second test).
    oracle_grads = False: the oracle's gradients are not compared here (the caller does it on a map the oracle can judge)."""
    c0, gT0, gC0, st0 = oracle
    # which stages really ran: voxels the row pruning kept off the list (both runs unfiltered), voxels the filter rejected, poses culled
    pruned = runs["e"][3]["pairs"] - runs["b"][3]["pairs"]
    print(f"\n[stages] {what}: oracle pairs {st0[2]} active {st0[3]} | " +
          " ".join(f"{t}: pairs {r[3]['pairs']} active {r[3]['grad_pairs']} culled {r[3]['culled']}" for t, r in runs.items()) +
          f" | row pruning dropped {pruned}, filter rejected {runs['b'][3]['pairs'] - runs['a'][3]['pairs']}, culled {runs['a'][3]['culled']}" +
          ("  (ROW PRUNING IDLE: the box covers the tile)" if pruned == 0 else ""))
    assert pruned >= 0, (what, "row pruning added voxels")
    for tag, (c, gT, gC, st) in runs.items():
        assert st["overflow"] == 0, (what, tag, st)
        assert st["units"] == st0[0], (what, tag, st, st0)
        assert st["grad_pairs"] == runs["e"][3]["grad_pairs"], (what, tag, "active voxels: a stage dropped one", st, runs["e"][3])
        if active_range is None:
            assert st["grad_pairs"] == st0[3], (what, tag, "active voxels differ from the oracle's", st, st0)
        else:       # (equality again whenever the two counts coincide)
            assert active_range[0] <= st["grad_pairs"] <= active_range[1], (what, tag, st, active_range)
    assert st0[3] > 0, (what, "scenario must have active voxels")
    pa, pb = runs["a"][3]["pairs"], runs["b"][3]["pairs"]
    assert pa <= pb <= st0[2], (what, pa, pb, st0)
    if name != "Box":            # Box's filter is compiled out (its exact pass takes the listed voxels directly)
        assert pa < pb, (what, "the fp32 filter rejected nothing: the case does not exercise it", pa, pb)
    tags = list(runs)
    for i, s in enumerate(tags):
        for t in tags[i + 1:]:
            cs, ct = runs[s][0], runs[t][0]
            assert abs(cs - ct) <= 1e-12 * max(abs(cs), abs(ct)), (what, s, t, cs, ct)
            for k, arr in ((1, "gradT"), (2, "gradC")):
                x, y = runs[s][k], runs[t][k]
                scale = max(np.abs(x).max(), np.abs(y).max())
                assert np.abs(x - y).max() <= 1e-10 * scale, (what, s, t, arr, np.abs(x - y).max(), scale)
    # run (a) against the oracle, as the parity tests do
    c, gT, gC, _ = runs["a"]
    assert abs(c - c0) <= REL_TOL * max(abs(c0), 1e-9), (what, c, c0)
    if oracle_grads:
        assert_close(gT, gT0, what + " gradT")
        assert_close(gC, gC0, what + " gradC")


@functools.lru_cache(maxsize=None)
def _scene(pkg):
    occ, esdf, res = small_world(pkg, shape=(40, 40, 40), occupancy=0.10, seed=9)
    T, cm = traj(pkg, occ, res, N=3, seed=41, margin=6.0)
    return occ, esdf, res, T, cm


@pytest.mark.parametrize("offset", list(_OFFSETS))
@pytest.mark.parametrize("name,variant", _CASES)
def test_stages_on_equal_stages_off(pkg, orc, product_lib, monkeypatch, name, variant, offset):
    """The parity tests' small scene (seed 9 / 41: every kind's filter rejects something there, so no other seed was needed);
    enable_cull = 1 so that bound_radius has a stage to switch (V3)."""
    capi, synth = pkg.capi, pkg.synth
    occ, esdf, res, T, cm = _scene(pkg)
    pp = _OFFSETS[offset]
    v3 = variant == "V3"
    cfg = synth.default_config(capi.V3_ESDF_TILE if v3 else capi.V2_OCC_TILE, kernel_size=17, integral_intervs=6, safety_hor=0.5, enable_cull=1)
    bbox, radius = _hints(pkg, orc, name, None, pp, 0.5 * 17 * res)

    def set_grids(tgt):
        if v3:
            tgt.set_grid(esdf, (0, 0, 0), res, capi.GRID_ESDF)
        else:
            tgt.set_grid(occ, (0, 0, 0), res, capi.GRID_OCCUPANCY)
    o = orc.Oracle(cfg, threads=4)
    set_grids(o)
    o.set_shape(_shape(pkg, name, None, pp))
    oracle = o.eval(T, cm)
    runs = _five_runs(pkg, monkeypatch, cfg, set_grids, name, None, pp, bbox, radius, T, cm)
    _assert_stages_change_nothing(f"{name}/{variant}/{offset}", name, runs, oracle)


# ---- voxel centres on the singular sets ------------------------------------------------------------------------------------------
_S40, _C40 = float(np.sin(40.0)), float(np.cos(40.0))
_SINGULAR = [       # (registry name, parameters or None for the reference's constants)
    ("Torus", None), ("Torus", (2.5, 0.02)),
    ("Cappedtorus", None), ("Cappedtorus", (_S40, _C40, 3.5, 0.02)),
    ("CappedCone", None), ("CappedCone", (0.02, 0.01, 0, 0, -1, 0, 0, 1)),
    # RoundedCone: the reference's h = 4.5 puts k = a h (z >= 4.5) outside the tile (|z| <= 4): k = 0 only.  h = 3.0 = 6 voxels puts the
    # voxel (0, 0, 3) ON k = a h and the whole r2 cap inside the tile, at the reference's radii and as a needle
    ("RoundedCone", None), ("RoundedCone", (1.5, 0.6, 3.0)), ("RoundedCone", (0.02, 0.01, 3.0)),
    ("WireframeBox", None), ("WireframeBox", (1.8, 2.5, 3.5, 0.02)),
    ("BendLinear", None), ("BendLinear", (2.0, 0.02)),
    ("TwistBox", None), ("TwistBox", (2.0, 2.0, 0.02, np.pi / 6)),
    ("BendBox", None), ("BendBox", (2.0, 2.0, 0.02, 0.5)),
    ("Table", None), ("Table", (0.0, 0.0, 0.0, 3.5, 1.75, 0.02, 2.8, 1.05, 0.0, 2.82, 1.07, 2.8)),
    ("Trefoil", None), ("Trefoil", (3.5, 0.02, 0.02, 0.005, 0.4)),
    ("SmoothDifference", None), ("SmoothIntersection", None), ("CSG", None), ("Box", None), ("Ball", None), ("Ball", (0.02,)),
]


def _variant(params):
    return "default" if params is None else ("h3" if params == (1.5, 0.6, 3.0) else "thin")


@pytest.mark.parametrize("name,params", _SINGULAR, ids=[f"{n}-{_variant(p)}" for n, p in _SINGULAR])
def test_voxel_centres_on_singular_sets(pkg, orc, product_lib, monkeypatch, name, params):
    capi, synth = pkg.capi, pkg.synth
    res, n, ks = 0.5, 24, 17
    occ = (np.random.default_rng(5).random((n, n, n)) < 0.5).astype(np.uint8)      # (not symmetric: the gradients do not cancel)
    occ[12, 12, :] = occ[12, :, 12] = occ[:, 12, 12] = 1       # the three body axes through the hover point, the point itself
    pos = (np.array([12, 12, 12]) + 0.5) * res                 # a voxel centre: p_rel of every voxel is a multiple of res
    T = np.array([1.0])
    Cf = np.zeros((6, 3)); Cf[0] = pos
    cm = synth.colmajor(Cf)
    pp = _OFFSETS["ident"]
    sh = _shape(pkg, name, params, pp)
    o0 = orc.Oracle(synth.default_config(capi.V2_OCC_TILE))
    o0.set_shape(sh)
    k = np.arange(-(ks // 2), ks // 2 + 1)
    I = np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3)      # the tile's voxels, relative to the hover point

    def occupied():
        J = I[occ[12 + I[:, 0], 12 + I[:, 1], 12 + I[:, 2]] != 0]
        return J, np.ascontiguousarray(J * res)
    # The reference alone, first.  (1) A voxel centre at which the class's difference quotient all but vanishes has NO reference
    # gradient: the quotient is rounding noise and its normalisation blows the noise up to a direction (DESIGN.md section 6 lists
    # the voxels); the oracle's own gradient is off the exact quotient by 2e-5 ... 2 there, so it cannot judge the device's.
    # Decided with the high-precision quotient and the plugin test's rounding floor, nothing of the device's.  These voxels STAY in
    # the map for the five runs (counts against the oracle's, cost, run against run); only the comparison of the gradients with
    # the oracle's is made on a second map without them.
    J, Q = occupied()
    s, g = o0.shape_eval(Q)
    # (2) the oracle's SDF and gradient at every occupied voxel centre of the tile must be finite (no case may rest on a NaN)
    assert np.all(np.isfinite(s)) and np.all(np.isfinite(g)), (name, params, "reference formula undefined at a voxel centre")
    near = s < 0.81                                             # every voxel that can be active at any of the edges below
    tab = sr.reference_table(name, list(sh.params), list(sh.trans), list(sh.rotate), np.ascontiguousarray(Q[near]))
    gb = grad_bound(name, sdf_floor(Q[near], list(sh.params)), tab, Q[near])
    noise = np.isfinite(gb) & (gb > 1e-6)                       # direction undetermined beyond 1e-6: a tenth of the parity tolerance
    occ_judged = occ.copy()
    for j in J[near][noise]:
        occ_judged[12 + j[0], 12 + j[1], 12 + j[2]] = 0
    print(f"\n[singular] {name}/{_variant(params)}: {int(noise.sum())} voxel(s) without a reference gradient: {Q[near][noise].tolist()}")
    assert noise.sum() <= 8, (name, params, "too many")
    s_edge = float(s[np.argmin(np.abs(s - 0.5))])              # the voxel whose SDF is nearest 0.5 m: the band's edge goes through it
    assert 0.2 < s_edge < 0.8, (name, params, s_edge)
    bbox, radius = _hints(pkg, orc, name, params, pp, 0.5 * ks * res)

    def oracle_at(safety, grid):
        cfg = synth.default_config(capi.V2_OCC_TILE, kernel_size=ks, integral_intervs=1, safety_hor=safety, enable_dyn=0)
        o = orc.Oracle(cfg, threads=2)
        o.set_grid(grid, (0, 0, 0), res, capi.GRID_OCCUPANCY)
        o.set_shape(_shape(pkg, name, params, pp))
        return cfg, o.eval(T, cm)
    for delta in (0.0, 1e-3, -1e-3, 3e-3, -3e-3):
        what = f"{name}/{_variant(params)}/edge{delta:+g}"
        cfg, oracle = oracle_at(s_edge + delta, occ)
        assert np.isfinite(oracle[0]) and oracle[3][2] == 2 * len(Q), (name, params, oracle[0], oracle[3])     # identity attitude: the whole tile, twice
        # delta = 0: voxels sit ON the edge, where `sdf < safety_hor` is decided by the last bit of the fp64 SDF - which device and
        # oracle (contraction, order) need not share.  There the device's count lies between the oracle's counts a hair below and
        # above the edge (a bound looser than equality, by the number of voxels on the edge); the five runs still have to agree with
        # each other exactly.
        span = (oracle_at(s_edge - 1e-12, occ)[1][3][3], oracle_at(s_edge + 1e-12, occ)[1][3][3]) if delta == 0.0 else None
        runs = _five_runs(pkg, monkeypatch, cfg, lambda tgt: tgt.set_grid(occ, (0, 0, 0), res, capi.GRID_OCCUPANCY), name, params, pp, bbox, radius, T, cm)
        _assert_stages_change_nothing(what, name, runs, oracle, span, oracle_grads=not noise.any())
        if noise.any():          # run (a) on the map the oracle can judge: its gradients against the oracle's
            eng = pkg.Engine(cfg)
            eng.set_grid(occ_judged, (0, 0, 0), res, capi.GRID_OCCUPANCY)
            eng.set_shape(_shape(pkg, name, params, pp, bbox=bbox, bound_radius=radius))
            c, gT, gC = eng.eval_single(T, cm)
            c0, gT0, gC0, _ = oracle_at(s_edge + delta, occ_judged)[1]
            assert abs(c - c0) <= REL_TOL * max(abs(c0), 1e-9), (what, c, c0)
            assert_close(gT, gT0, what + " gradT (judged map)")
            assert_close(gC, gC0, what + " gradC (judged map)")
