"""High-precision model of ONE piece's dynamics cost (the integral sweep with enable_pos = 0) and the edge cases held against it.

The model is written from the mathematics, not from the oracle: it holds only the forward map (quintic -> flat outputs -> tilt
quaternion and its kinematics -> the three smoothed-L1 penalties -> trapezoid sum) and no adjoint; its gradient is a central
difference at 70 digits.  The body rate comes from the quaternion kinematics omega = 2 vec(conj(q) (x) dq/dt) of the psi = 0 tilt
quaternion, the projector as (I - z z^T) / |zu|, the tilt as acos(z . e3).

Needs mpmath for cost_mp / grad_mp / the case builder's limit placement; the GPU tests never import this module's mp half - they
read tests/golden/dyn_edges.npz (written by tests/golden/make_golden_dyn.py) through load_golden().
"""
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dyn_edges.npz")
DPS = 70            # working digits
H = "1e-25"         # central-difference step
KINK_GUARD = 1e-12  # no sample's violation may lie this close to 0 or mu (the smoothed L1 changes its formula there)
MU = 1.0e-2         # smoothing_eps of every case

# config values every case starts from (synth.default_config's vehicle, weights and smoothing)
BASE = dict(weight_v=1000.0, weight_omg=1000.0, weight_theta=1000.0, vmax=1.0e3, omgmax=1.0e3, thetamax=1.0e3,
            smoothing_eps=MU, vehicle_mass=0.61, grav_acc=9.8, horiz_drag=0.10, vert_drag=0.10, paras_drag=0.01, speed_eps=1.0e-4)
CFG_KEYS = sorted(BASE)
ALL_ON = dict(vmax=2.0, omgmax=1.0, thetamax=0.3)       # test_dynamics_only_sweep's limits: all three penalties active


def _mp():
    import mpmath
    mpmath.mp.dps = DPS
    return mpmath


def full_cfg(over):
    c = dict(BASE)
    c.update(over)
    return c


# ---- the forward model --------------------------------------------------------------------------------------------------------
def _smoothed_l1(mp, x, mu):
    """0 below zero, the quartic blend (mu - x / 2) (x / mu)^3 on [0, mu], x - mu / 2 above."""
    if x < 0:
        return mp.mpf(0)
    if x > mu:
        return x - mu / 2
    r = x / mu
    return (mu - x / 2) * r * r * r


def sample_mp(c, s, cfg):
    """Flat outputs of the quintic c (3 x 6 mp numbers, c[d][k] the coefficient of s^k on axis d) at local time s:
    dict with vel, zu, z, omega, theta."""
    mp = _mp()
    vel, acc, jer = [], [], []
    for d in range(3):
        cd = c[d]
        vel.append(cd[1] + s * (2 * cd[2] + s * (3 * cd[3] + s * (4 * cd[4] + s * 5 * cd[5]))))
        acc.append(2 * cd[2] + s * (6 * cd[3] + s * (12 * cd[4] + s * 20 * cd[5])))
        jer.append(6 * cd[3] + s * (24 * cd[4] + s * 60 * cd[5]))
    m, g, dh, cp, eps = (mp.mpf(cfg[k]) for k in ("vehicle_mass", "grav_acc", "horiz_drag", "paras_drag", "speed_eps"))
    v2 = vel[0] ** 2 + vel[1] ** 2 + vel[2] ** 2
    sp = mp.sqrt(v2 + eps)                                   # smoothed speed
    kd = dh / m
    va = vel[0] * acc[0] + vel[1] * acc[1] + vel[2] * acc[2]
    # thrust vector zu = a + (dh / m) (1 + cp sp) v + g e3 and its time derivative
    zu = [acc[d] + kd * (1 + cp * sp) * vel[d] for d in range(3)]
    zu[2] += g
    dzu = [jer[d] + kd * ((1 + cp * sp) * acc[d] + cp * va / sp * vel[d]) for d in range(3)]
    n = mp.sqrt(zu[0] ** 2 + zu[1] ** 2 + zu[2] ** 2)
    z = [zu[d] / n for d in range(3)]
    zd = z[0] * dzu[0] + z[1] * dzu[1] + z[2] * dzu[2]
    dz = [(dzu[d] - z[d] * zd) / n for d in range(3)]       # (I - z z^T) / |zu| . dzu
    # tilt quaternion of psi = 0: q = (w, x, y, 0), w = sqrt((1 + z2) / 2), (x, y) = (-z1, z0) / (2 w); body rate from its kinematics
    w = mp.sqrt((1 + z[2]) / 2)
    x, y = -z[1] / (2 * w), z[0] / (2 * w)
    dw = dz[2] / (4 * w)
    dx = -dz[1] / (2 * w) + z[1] * dw / (2 * w * w)
    dy = dz[0] / (2 * w) - z[0] * dw / (2 * w * w)
    omg = [2 * (w * dx - dw * x), 2 * (w * dy - dw * y), -2 * (x * dy - y * dx)]
    return dict(vel=vel, v2=v2, zu=zu, zu_norm=n, z=z, omg=omg, omg2=omg[0] ** 2 + omg[1] ** 2 + omg[2] ** 2, theta=mp.acos(z[2]))


def violations_mp(c, T, K, cfg):
    """[(violaVel, violaOmg, violaTheta)] of the K + 1 samples."""
    mp = _mp()
    out = []
    for j in range(K + 1):
        f = sample_mp(c, j * T / K, cfg)
        out.append((f["v2"] - mp.mpf(cfg["vmax"]) ** 2, f["omg2"] - mp.mpf(cfg["omgmax"]) ** 2, f["theta"] - mp.mpf(cfg["thetamax"])))
    return out


def cost_mp(c, T, K, cfg):
    """Trapezoid sum over j = 0..K of node . (T / K) . penalty at s = j T / K; c: 3 x 6, anything mpf() takes."""
    mp = _mp()
    c = [[mp.mpf(x) for x in row] for row in c]
    T = mp.mpf(T)
    mu = mp.mpf(cfg["smoothing_eps"])
    wts = [mp.mpf(cfg[k]) for k in ("weight_v", "weight_omg", "weight_theta")]
    step = T / K
    total = mp.mpf(0)
    for j, viola in enumerate(violations_mp(c, T, K, cfg)):
        pena = sum(w * _smoothed_l1(mp, x, mu) for w, x in zip(wts, viola))
        total += (mp.mpf(1) / 2 if j in (0, K) else 1) * step * pena
    return total


def grad_mp(c, T, K, cfg):
    """The piece's 19 entries: d cost / d c in column-major order (axis-major: 6 coefficients of x, of y, of z), then d cost / d T."""
    mp = _mp()
    h = mp.mpf(H)
    c = [[mp.mpf(x) for x in row] for row in c]
    T = mp.mpf(T)
    g = []
    for d in range(3):
        for k in range(6):
            c0 = c[d][k]
            c[d][k] = c0 + h
            fp = cost_mp(c, T, K, cfg)
            c[d][k] = c0 - h
            fm = cost_mp(c, T, K, cfg)
            c[d][k] = c0
            g.append((fp - fm) / (2 * h))
    g.append((cost_mp(c, T + h, K, cfg) - cost_mp(c, T - h, K, cfg)) / (2 * h))
    return g


def measure(cost, g, cost_ref, g_ref):
    """The one measure every comparison uses: max(max|g - g_ref| / max|g_ref|, |cost - cost_ref| / |cost_ref|).  A zero reference
    admits only zero."""
    g = np.asarray(g, dtype=np.float64); g_ref = np.asarray(g_ref, dtype=np.float64)
    gs, cs = float(np.max(np.abs(g_ref))), abs(float(cost_ref))
    eg = float(np.max(np.abs(g - g_ref)))
    ec = abs(float(cost) - float(cost_ref))
    eg = eg / gs if gs > 0 else (0.0 if eg == 0 else math.inf)
    ec = ec / cs if cs > 0 else (0.0 if ec == 0 else math.inf)
    return max(eg, ec)


def piece_entries(gT, gC, i=0):
    """The 19 entries of piece i out of an evaluation's (gradT[N], gradC[18 N] column-major)."""
    gT = np.asarray(gT); gC = np.asarray(gC)
    N = gT.size
    return np.concatenate([gC[d * 6 * N + 6 * i: d * 6 * N + 6 * i + 6] for d in range(3)] + [gT[i:i + 1]])


# ---- the case builder ---------------------------------------------------------------------------------------------------------
CENTRE = (128.0, 128.0, 128.0)  # every piece is centred here (the collision-slot test puts a 256 m obstacle-free map around it)


def quintic_to_rest(v0, a0, j0, T):
    """3 x 6 float64 coefficients of the quintic with (vel, acc, jerk)(0) = (v0, a0, j0) and vel(T) = acc(T) = 0, its path's
    bounding box centred on CENTRE."""
    c = np.zeros((3, 6))
    for d in range(3):
        c1, c2, c3 = float(v0[d]), float(a0[d]) / 2.0, float(j0[d]) / 6.0
        A = c1 + 2 * c2 * T + 3 * c3 * T * T
        B = 2 * c2 + 6 * c3 * T
        c5 = (3 * A / T - B) / (5 * T ** 3)
        c4 = (-A - 5 * c5 * T ** 4) / (4 * T ** 3)
        c[d, 1:] = (c1, c2, c3, c4, c5)
        s = np.linspace(0.0, T, 257)
        p = np.polyval(c[d, ::-1], s)
        assert p.max() - p.min() <= 200.0, (d, p.min(), p.max())      # stays inside that map
        c[d, 0] = CENTRE[d] - 0.5 * (p.min() + p.max())
    return c


def tilt_state(theta, zu_norm=6.0, phi=0.7, v0=(0.0, 0.0, 0.0), cfg=BASE):
    """The acceleration that puts the thrust direction at theta from vertical (azimuth phi) with |zu| = zu_norm at velocity v0."""
    v0 = np.asarray(v0, dtype=np.float64)
    sp = math.sqrt(float(v0 @ v0) + cfg["speed_eps"])
    zu = zu_norm * np.array([math.sin(theta) * math.cos(phi), math.sin(theta) * math.sin(phi), math.cos(theta)])
    return zu - cfg["horiz_drag"] / cfg["vehicle_mass"] * (1.0 + cfg["paras_drag"] * sp) * v0 - np.array([0.0, 0.0, cfg["grav_acc"]])


J0 = (0.8, -0.5, 0.3)
MID = dict(v0=(1.5, -1.0, 0.5), a0=(2.0, -1.5, 1.0), j0=(3.0, -2.0, 1.5))            # a well-conditioned state with drag, tilt and body rate
TILTED = dict(v0=(0.0, 0.0, 0.0), a0=tuple(tilt_state(2.5)), j0=J0)                  # thrust 2.5 rad from vertical
VEL = dict(v0=(3.0, -2.0, 1.0), a0=(0.5, 0.3, -0.4), j0=(0.2, -0.1, 0.3))
# (the jerk at the end of a piece is j0 + 12 v0 / T^2 + 6 a0 / T: this j0 cancels its horizontal part at T = 1, so the body rate at the
# resting end stays below the one at the start - the below-zero case needs that)
OMG = dict(v0=(0.4, 0.2, -0.1), a0=(2.0, -1.5, 1.0), j0=(-16.8, 6.6, 2.0))
THETA = dict(v0=(0.5, -0.4, 0.2), a0=tuple(tilt_state(0.8, 9.0, v0=(0.5, -0.4, 0.2))), j0=J0)
HOVER = dict(v0=(0.0, 0.0, 0.0), a0=(0.0, 0.0, 0.0), j0=(1.5, -1.0, 0.7))


def _specs():
    """(name, state, T, K, config overrides, placement).  placement = (penalty, violation): the limit of that penalty is set so
    that sample 0's violation is `violation` (the other two limits stay as the overrides give them)."""
    S = []
    tilts = [("0.31", 0.31), ("1.0", 1.0), ("pi_2", math.pi / 2), ("2.5", 2.5), ("3.0", 3.0), ("pi-0.05", math.pi - 0.05)]
    for tag, th in tilts:
        st = dict(v0=(0, 0, 0), a0=tuple(tilt_state(th)), j0=J0)
        # thetamax = 0.3 puts theta = 0.31 ON the upper boundary mu of the smoothing band, where no central difference may stand
        # (KINK_GUARD): that one state is built 1e-6 rad further out, just past the band.
        st_t = st if tag != "0.31" else dict(v0=(0, 0, 0), a0=tuple(tilt_state(th + 1e-6)), j0=J0)
        S.append((f"tilt_{tag}_theta", st_t, 1.0, 16, dict(thetamax=0.3), None))
        S.append((f"tilt_{tag}_omg", st, 1.0, 16, dict(omgmax=0.05), None))
    S.append(("small_tilt", dict(v0=(0, 0, 0), a0=tuple(tilt_state(0.02 + MU / 2)), j0=J0), 1.0, 16, dict(thetamax=0.02), None))
    for pen, st in (("vel", VEL), ("omg", OMG), ("theta", THETA)):
        for tag, viola in (("below", -1e-6), ("quarter", MU / 4), ("under_mu", MU - 1e-6), ("3mu", 3 * MU)):
            if pen == "theta" and tag == "quarter":
                continue                                       # small_tilt stands in the middle of the tilt penalty's band
            S.append((f"l1_{pen}_{tag}", st, 1.0, 1 if tag == "below" else 16, {}, (pen, viola)))
    S.append(("hover_omg", HOVER, 1.0, 16, dict(omgmax=0.05), None))
    S.append(("hover_omg_tilt", HOVER, 1.0, 16, dict(omgmax=0.05, thetamax=0.3), None))
    S.append(("near_free_fall", dict(v0=(0, 0, 0), a0=(0.02, 0.01, -BASE["grav_acc"] + 0.05), j0=(0.3, -0.2, 0.1)), 1.0, 16, ALL_ON, None))
    S.append(("no_drag", MID, 1.0, 16, dict(ALL_ON, horiz_drag=0.0, paras_drag=0.0), None))
    S.append(("speed_eps_1e-12", dict(v0=(0, 0, 0), a0=(2.0, -1.5, 1.0), j0=(3.0, -2.0, 1.5)), 1.0, 16, dict(ALL_ON, speed_eps=1e-12), None))
    S.append(("speed_50", dict(v0=(40.0, -25.0, 16.583123951777), a0=(2.0, -1.5, 1.0), j0=(3.0, -2.0, 1.5)), 0.4, 16, ALL_ON, None))
    for T in (0.05, 12.0):
        S.append((f"T_{T:g}", MID, T, 16, ALL_ON, None))
    for K in (1, 2, 16, 127, 128, 150):
        S.append((f"K{K}_mid", MID, 1.0, K, ALL_ON, None))
        S.append((f"K{K}_tilted", TILTED, 1.0, K, ALL_ON, None))
    return S


def build_cases():
    """[dict(name, c (3 x 6 float64), T, K, cfg)] - needs mpmath (limit placement and the kink guard)."""
    mp = _mp()
    out = []
    for name, st, T, K, over, place in _specs():
        c = quintic_to_rest(st["v0"], st["a0"], st["j0"], T)
        cfg = full_cfg(over)
        if place is not None:
            pen, viola = place
            f = sample_mp([[mp.mpf(x) for x in row] for row in c], mp.mpf(0), cfg)
            if pen == "vel":
                cfg["vmax"] = float(mp.sqrt(f["v2"] - viola))
            elif pen == "omg":
                cfg["omgmax"] = float(mp.sqrt(f["omg2"] - viola))
            else:
                cfg["thetamax"] = float(f["theta"] - viola)
        case = dict(name=name, c=c, T=float(T), K=int(K), cfg=cfg)
        check_case(case, below=place is not None and place[1] < 0)
        out.append(case)
    assert len({x["name"] for x in out}) == len(out)
    return out


def check_case(case, below=False):
    """No sample within KINK_GUARD of a smoothed-L1 region boundary; a below-zero case has no sample above zero."""
    mp = _mp()
    mu = mp.mpf(case["cfg"]["smoothing_eps"])
    for j, viola in enumerate(violations_mp([[mp.mpf(x) for x in row] for row in case["c"]], mp.mpf(case["T"]), case["K"], case["cfg"])):
        for x in viola:
            assert abs(x) > KINK_GUARD and abs(x - mu) > KINK_GUARD, (case["name"], j, float(x))
            assert not below or x < 0, (case["name"], j, float(x))


# ---- the committed golden ------------------------------------------------------------------------------------------------------
def load_golden(path=GOLDEN):
    """[dict(name, c, T, K, cfg, cost, grad[19], e_cond, coeffs (18, column-major))] from the npz alone (no mpmath)."""
    z = np.load(path)
    keys = [str(k) for k in z["cfg_keys"]]
    out = []
    for i, name in enumerate(z["names"]):
        out.append(dict(name=str(name), c=z["c"][i], coeffs=np.ascontiguousarray(z["c"][i].reshape(-1)), T=float(z["T"][i]), K=int(z["K"][i]),
                        cfg=dict(zip(keys, (float(v) for v in z["cfg"][i]))), cost=float(z["cost"][i]), grad=z["grad"][i],
                        cost_digits=str(z["cost_digits"][i]), grad_digits=[str(s) for s in z["grad_digits"][i]], e_cond=float(z["e_cond"][i])))
    return out


def make_config(pkg, case, **kw):
    """The product / oracle configuration of a case (V3, dynamics only unless overridden)."""
    over = dict(case["cfg"])
    over.update(integral_intervs=case["K"], enable_pos=0)
    over.update(kw)
    return pkg.synth.default_config(pkg.capi.V3_ESDF_TILE, **over)


def group_key(case):
    return (case["K"],) + tuple(case["cfg"][k] for k in CFG_KEYS)


BELOW = ("l1_vel_below", "l1_omg_below", "l1_theta_below")
