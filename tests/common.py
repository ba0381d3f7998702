"""Shared scenario builders for the parity tests (inputs only; expected values always come from the oracle)."""
import numpy as np

REL_TOL = 1e-5   # BASELINE.json north_star: cost/grad within 1e-5 relative of the CPU reference arithmetic


def small_world(pkg, seed=3, shape=(48, 48, 32), res=0.5, occupancy=0.12):
    synth = pkg.synth
    occ = synth.random_box_map(shape, res=res, occupancy=occupancy, seed=seed, edge=(1.0, 3.0))
    esdf = synth.esdf_from_occupancy(occ, res)
    return occ, esdf, res


def traj(pkg, occ, res, N=6, seed=11, piece_T=1.5, margin=4.0, jitter=0.5):
    ext = np.array(occ.shape) * res
    T, Cf = pkg.synth.random_trajectory(ext, N, seed=seed, piece_T=piece_T, margin=margin, occ=occ, res=res, jitter=jitter)
    return T, pkg.synth.colmajor(Cf)


def make_pair(pkg, orc, cfg, shape, occ=None, esdf=None, res=0.5, origin=(0, 0, 0), bmax=None, points=None, threads=4):
    """(Engine, Oracle) with identical once-per-plan state."""
    capi = pkg.capi
    eng = pkg.Engine(cfg)
    o = orc.Oracle(cfg, threads=threads)
    for tgt in (eng, o):
        if esdf is not None:
            tgt.set_grid(esdf, origin, res, capi.GRID_ESDF, bmax=bmax)
        if occ is not None:
            tgt.set_grid(occ, origin, res, capi.GRID_OCCUPANCY, bmax=bmax)
        if shape is not None:
            tgt.set_shape(shape)
        if points is not None:
            tgt.set_points(points)
    return eng, o


def assert_close(got, want, what, tol=REL_TOL):
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.all(np.isfinite(got)) or not np.all(np.isfinite(want)), f"{what}: non-finite output"
    scale = max(np.linalg.norm(want.ravel()), 1e-12)
    err = np.linalg.norm((got - want).ravel())
    assert err <= tol * max(scale, 1e-9) + 1e-12, f"{what}: |diff|={err:.3e} vs |ref|={scale:.3e} (rel {err / scale:.3e} > {tol})"


# ---- the full objective callback composed from oracle pieces (costFunctionLmbm, back_end_optimizer.hpp:358-430) ----
def tau_to_T(tau):
    tau = np.asarray(tau, dtype=np.float64)
    return np.where(tau > 0.0, (0.5 * tau + 1.0) * tau + 1.0, 1.0 / ((0.5 * tau - 1.0) * tau + 1.0))


def T_to_tau(T):
    T = np.asarray(T, dtype=np.float64)
    return np.where(T > 1.0, np.sqrt(np.abs(2.0 * T - 1.0)) - 1.0, 1.0 - np.sqrt(np.abs(2.0 / T - 1.0)))


def oracle_cost_function(orc, sweeps, head, tail, rho, x, N):
    """sweeps: list of oracle contexts whose eval() ACCUMULATES into (cost, gradT, gradC), in the reference's order.
    head/tail: 3x3 with columns pos, vel, acc.  Returns (cost, g)."""
    x = np.asarray(x, dtype=np.float64)
    tau, xi = x[:N], x[N:]
    T = tau_to_T(tau)
    way = xi.reshape(N - 1, 3).T if N > 1 else np.zeros((3, 0))
    C6 = orc.minco_coeffs(head, tail, way, T)                 # 6N x 3
    cm = np.ascontiguousarray(C6.T).reshape(-1)               # column-major
    e, gC, gT = orc.minco_energy(cm, T)
    cost = np.array([e])
    for o in sweeps:
        o.eval(T, cm, accumulate_into=(cost, gT, gC))
    gP, gTt = orc.minco_propagate(head, tail, way, T, gC, gT)
    total = float(cost[0]) + rho * float(T.sum())
    gTt = gTt + rho
    den = (0.5 * tau - 1.0) * tau + 1.0
    g_tau = np.where(tau > 0, gTt * (tau + 1.0), gTt * (1.0 - tau) / (den * den))
    return total, np.concatenate([g_tau, gP.T.reshape(-1)])


# ---- mesh robot x swept-volume sweep, free-running -----------------------------------------------------------------------------
# The argmin over t of a mesh SDF is a chain of accept/reject comparisons on values that differ by less than one float ulp of the
# winding number: the reference's own code does not reproduce its t* under a 1-ulp perturbation of w
# (tests/test_oracle_ref.py::test_mesh_swept_volume_argmin_is_sensitive_to_one_ulp_of_w).  Rounds 1-2 therefore allowed the device
# the reference's measured self-spread.  Since round 3 the device computes w BIT FOR BIT like the reference's library (glibc's
# atan2f restated, reciprocal-multiply normalisation, the tree-shaped float sum of the HDK traversal: csrc/dev_mesh.hpp), so the
# free-running tests hold the device to the plain tolerance again: t* identical, gradients at the north-star's 1e-5.
SPREAD_LINES = []       # printed by conftest.py's pytest_terminal_summary: the measured deviations end up in the pytest log itself


def _spread_log(line):
    import os
    print("\n[mesh x V1] " + line)
    SPREAD_LINES.append(line)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.environ.get("ISDF_MESH_SPREAD_LOG", os.path.join(root, "gpurun_out", "mesh_spread.txt"))
    try:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "a") as f:
            f.write(line + "\n")
    except OSError:
        pass


def assert_mesh_v1_free_running(what, tg, to, gT, gT0, gC, gC0, allow_ties=0):
    """Device (tg, gT, gC) vs oracle (to, gT0, gC0), both searching for their own minimisers: the measured deviations are logged
    (the pytest log's "mesh x V1" summary section; gpurun_out/mesh_spread.txt -> profiles/), then held to: every t* within 1e-9 s, gradients at REL_TOL."""
    dt = np.abs(np.asarray(tg) - np.asarray(to))
    moved = float((dt > 1e-9).mean())
    eC = float(np.linalg.norm(gC - gC0) / max(np.linalg.norm(gC0), 1e-300)); eT = float(np.linalg.norm(gT - gT0) / max(np.linalg.norm(gT0), 1e-300))
    _spread_log(f"{what}: {len(dt)} points | device vs oracle, free-running: gradC {eC:.3e} gradT {eT:.3e} dt_max {dt.max():.3e} "
                f"identical t*: {1 - moved:.2%} | applied: gradC, gradT <= {REL_TOL:g}, every |dt*| <= 1e-9")
    # allow_ties (full-size runs only): this many points may end on another t*.  The reference seeds an interval's descent with a
    # fine sample only if it is STRICTLY below the coarse sample the interval was entered on (quirk q1, sw_manager.hpp:405,431-435);
    # when the interval's only in-range coarse sample IS its minimum, that test compares two evaluations of the same time, which
    # device and oracle both get right to 1 ulp - and may order differently (tools/trefoil_tstar_diag.py: point 14 167 of the
    # Trefoil.obj workload, sdf* above the safety distance on both sides, contribution zero).  Gradients are held to REL_TOL regardless.
    n_moved = int((dt > 1e-9).sum())
    assert n_moved <= allow_ties, f"{what}: {moved:.2%} of the points ({n_moved}) end on another t* (max {dt.max():.3e} s)"
    assert_close(gC, gC0, what + " gradC")
    assert_close(gT, gT0, what + " gradT")


# ---- every analytic shape kind (tests/test_gpu_sweep_stages.py, test_gpu_shape_plugin.py, test_shape_reference_host.py) --------------
ALL_KINDS = ["Torus", "Cappedtorus", "CappedCone", "RoundedCone", "WireframeBox", "BendLinear", "TwistBox", "BendBox", "Table", "Trefoil",
             "SmoothDifference", "SmoothIntersection", "CSG", "Box", "Ball"]
BODY_OFFSETS = {"ident": (0, 0, 0, 0, 0, 0), "offset": (0.2, -0.1, 0.15, 30, 10, 120)}      # yaml poly_params: the two sweep instantiations
PLUGIN_POINTS, PLUGIN_BASE = 2000, 40
MARGIN_MIN = 1e-12          # points with 0 < margin < this may be left out: the decision is not determined in fp64 ...
LEFT_OUT_MAX = 0.02         # ... but at most this share of a kind's points
DX_CENTRAL, DX_BOX = 0.000005, 0.01


def sdf_floor(pts, params):
    """16 ulp of (|p| + largest parameter): the rounding floor of an SDF bound."""
    return 16 * np.spacing(np.linalg.norm(pts, axis=1) + max(abs(v) for v in params))


def plugin_case(pkg, name, offset):
    """(shape struct, points, is_special, high-precision table, kept mask, floor[n]) of one kind and body offset."""
    import shape_reference as sr
    sh = pkg.synth.make_shape(name, poly_params=BODY_OFFSETS[offset])
    params, trans, rot = list(sh.params), list(sh.trans), list(sh.rotate)
    pts, special = sr.sample_points(name, params, trans, rot, n=PLUGIN_POINTS, n_base=PLUGIN_BASE, seed=sr.KINDS.index(name))
    tab = sr.reference_table(name, params, trans, rot, pts)
    m = tab["margin"]
    kept = ~((m > 0) & (m < MARGIN_MIN))
    return sh, pts, special, tab, kept, sdf_floor(pts, params)


def grad_bound(name, sdf_bound, tab, pts):
    """Entry-wise bound of the gradient from a bound of the SDF: x 1 / (2 dx) / |quotient| (Box: forward and not normalised, x 1 / dx;
    Ball: the analytic p / |p|, 16 ulp of 1).  inf where the quotient vanishes (nothing to normalise: the axis of a symmetric shape)."""
    if name == "Ball":
        return np.where(np.linalg.norm(pts, axis=1) > 0, 16 * np.finfo(np.float64).eps, np.inf)
    if name == "Box":
        return sdf_bound / DX_BOX
    with np.errstate(divide="ignore"):
        return np.where(tab["qnorm"] > 0, sdf_bound / (2 * DX_CENTRAL) / tab["qnorm"], np.inf)
