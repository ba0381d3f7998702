"""Yardstick of the dynamic-limits report (isdf_traj_limits*) and the state sampler (isdf_traj_sample*): the 70-digit model of
tests/dyn_reference.py (sample_mp) plus the thrust, the reference extremum of every channel of every case, the case list and the
bounds the host and the device form are held to.

The thrust is written from the formula, not from the product code: with sp = sqrt(|v|^2 + eps) the collective force is
f = m (a + g e3) + dv (1 + cp sp) v and thr = z . f, z the unit thrust direction of the model.

Reference extremum of a channel: the model on a grid 16 x finer than the report's coarse grid; every local extremum of that grid
that could still be the global one (within 5 % of the grid's range of it: refining moves a grid extremum by about kappa / (8 (16 S)^2)
of its value, far less) is refined by golden section in mp to a bracket of 1e-30 T; the global one is kept (ties: the smaller
global time, then the earlier piece - the report's own rule).  A channel that is exactly constant on the grid (hover) has its
extremum at t = 0 by that rule.

Bounds (value, relative to the reference): 32 max(e_cond, 2^-50) + kappa tol_t^2 / 2.
  e_cond   movement of the model under one-ulp changes of every input (the piece's 18 coefficients and its duration; two fixed sign
           patterns), taken at the reference time scaled with the duration: by the envelope theorem the extremum's value moves
           like the function at the fixed (scaled) time, to first order.
  kappa    |f''| T_i^2 / |f| at the extremum, from the model: a search that stops with a bracket shorter than tol_t T_i has evaluated
           a point within tol_t T_i of the maximiser, hence lost at most f'' (tol_t T_i)^2 / 2.  An extremum at an end of its piece is a
           coarse sample, evaluated exactly: kappa = 0 there.
A zero reference admits only zero.  The time is judged through the value: the model at the reported time within the same bound.

Needs mpmath for everything but load_golden().
"""
import math
import os

import numpy as np

import dyn_reference as dr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "traj_limits.npz")
NCH = 6
CH_NAMES = ["speed", "acc", "omg", "tilt", "thrust_max", "thrust_min"]
TOL_T = 2.0 ** -26
FINE = 16                   # the reference grid is this many times finer than the report's
MP_BRACKET = "1e-30"
SEPARATION = 1e-6           # no second local extremum within this (relative) of the global one
DIGITS = 40
ROW = 20
GROUPS = [(0, 3), (3, 6), (6, 9), (9, 12), (12, 16), (16, 19), (19, 20)]     # pos vel acc jer quat omg thr
INTERVS = 4                 # integral_intervs of every case: the default coarse grid is 4 x 4 = 16 intervals


def _mp():
    return dr._mp()


# ---- the model ------------------------------------------------------------------------------------------------------------------
def state_mp(c, s, cfg):
    """The sampler's row at local time s of the quintic c (3 x 6 mp): 20 mp numbers pos3 vel3 acc3 jer3 quat4 omg3 thr."""
    mp = _mp()
    f = dr.sample_mp(c, s, cfg)
    pos, acc, jer = [], [], []
    for d in range(3):
        cd = c[d]
        pos.append(cd[0] + s * (cd[1] + s * (cd[2] + s * (cd[3] + s * (cd[4] + s * cd[5])))))
        acc.append(2 * cd[2] + s * (6 * cd[3] + s * (12 * cd[4] + s * 20 * cd[5])))
        jer.append(6 * cd[3] + s * (24 * cd[4] + s * 60 * cd[5]))
    m, g, dv, cp, eps = (mp.mpf(cfg[k]) for k in ("vehicle_mass", "grav_acc", "vert_drag", "paras_drag", "speed_eps"))
    sp = mp.sqrt(f["v2"] + eps)
    force = [m * acc[d] + dv * (1 + cp * sp) * f["vel"][d] for d in range(3)]
    force[2] += m * g
    thr = sum(f["z"][d] * force[d] for d in range(3))
    w = mp.sqrt((1 + f["z"][2]) / 2)
    quat = [w, -f["z"][1] / (2 * w), f["z"][0] / (2 * w), mp.mpf(0)]
    return pos + list(f["vel"]) + acc + jer + quat + list(f["omg"]) + [thr]


def channels_mp(c, s, cfg):
    """The six channels as reported."""
    mp = _mp()
    f = dr.sample_mp(c, s, cfg)
    r = state_mp(c, s, cfg)
    return [mp.sqrt(f["v2"]), mp.sqrt(r[6] ** 2 + r[7] ** 2 + r[8] ** 2), mp.sqrt(f["omg2"]), f["theta"], r[19], r[19]]


def _sign(ch):
    return -1 if ch == 5 else 1


def mpc(c):
    mp = _mp()
    return [[mp.mpf(float(x)) for x in row] for row in c]


def golden_max_mp(fun, a, b, width):
    """Golden section for the maximum of fun on [a, b] in mp until the bracket is shorter than width: (value, x) of the best evaluation."""
    mp = _mp()
    r = (mp.sqrt(5) - 1) / 2
    x1, x2 = b - r * (b - a), a + r * (b - a)
    f1, f2 = fun(x1), fun(x2)
    best = max((f1, -x1), (f2, -x2))
    while b - a >= width:
        if f1 >= f2:
            b, x2, f2 = x2, x1, f1
            x1 = b - r * (b - a); f1 = fun(x1); best = max(best, (f1, -x1))
        else:
            a, x1, f1 = x1, x2, f2
            x2 = a + r * (b - a); f2 = fun(x2); best = max(best, (f2, -x2))
    return best[0], -best[1]


def sample_time(T, S, j):
    """The report's coarse sample time (float64 arithmetic, both ends exact)."""
    return 0.0 if j <= 0 else (T if j >= S else float(j) * T / float(S))


def locate(T, t):
    """Trajectory::locatePieceIdx in float64: (piece, local time)."""
    idx = 0
    N = len(T)
    while idx < N and t > T[idx]:
        t = t - T[idx]
        idx += 1
    if idx == N:
        idx -= 1
        t = t + T[idx]
    return idx, t


def piece_starts(T):
    out, t0 = [], 0.0
    for x in T:
        out.append(t0)
        t0 = t0 + float(x)
    return out, t0


# ---- reference extrema --------------------------------------------------------------------------------------------------------
def _piece_candidates(c, T, S, cfg):
    """Per channel the local extrema of the fine grid of one piece: [(grid value in maximised form, lo, hi, s_grid)]."""
    mp = _mp()
    n = FINE * S
    Tm = mp.mpf(T)
    xs = [Tm * k / n for k in range(n + 1)]
    xs[-1] = Tm
    vals = [channels_mp(c, x, cfg) for x in xs]
    out = []
    for ch in range(NCH):
        g = [_sign(ch) * v[ch] for v in vals]
        cand = []
        for k in range(n + 1):
            left = k == 0 or g[k] >= g[k - 1]
            right = k == n or g[k] >= g[k + 1]
            if left and right:
                cand.append((g[k], xs[max(k - 1, 0)], xs[min(k + 1, n)], xs[k]))
        out.append((cand, min(g), max(g)))
    return out


def reference_extrema(case):
    """Per channel dict(value, piece, s (mp local time), t (mp global time), const, candidates refined [(value, piece, s)])."""
    mp = _mp()
    T, C, cfg, S = case["T"], case["C"], case["cfg"], case["samples"]
    N = len(T)
    starts, _ = piece_starts(T)
    per_piece = [_piece_candidates(mpc(C[i]), float(T[i]), S, cfg) for i in range(N)]
    res = []
    for ch in range(NCH):
        gmin = min(p[ch][1] for p in per_piece)
        gmax = max(p[ch][2] for p in per_piece)
        if gmin == gmax:                                  # exactly constant: the tie rule puts it at t = 0
            res.append(dict(value=_sign(ch) * gmax, piece=0, s=mp.mpf(0), t=mp.mpf(0), const=True, refined=[]))
            continue
        keep = gmax - (gmax - gmin) / 20
        refined = []
        for i in range(N):
            ci = mpc(C[i])
            fun = lambda x, ci=ci, ch=ch: _sign(ch) * channels_mp(ci, x, cfg)[ch]      # noqa: E731
            for gv, lo, hi, sg in per_piece[i][ch][0]:
                if gv < keep:
                    continue
                v, x = golden_max_mp(fun, lo, hi, mp.mpf(MP_BRACKET) * mp.mpf(float(T[i])))
                if gv > v or (gv == v and sg < x):
                    v, x = gv, sg                          # never below a grid sample (an end sample above all)
                # an extremum at an end of the piece is the end sample itself
                for e in (mp.mpf(0), mp.mpf(float(T[i]))):
                    if abs(x - e) <= mp.mpf("1e-28") * mp.mpf(float(T[i])):
                        ve = fun(e)
                        if ve >= v:
                            v, x = ve, e
                refined.append((v, i, x, mp.mpf(starts[i]) + x))
        # the global one: larger value, then smaller global time, then the earlier piece
        best = max(refined, key=lambda r: (r[0], -r[3], -r[1]))
        res.append(dict(value=_sign(ch) * best[0], piece=best[1], s=best[2], t=best[3], const=False,
                        refined=[(_sign(ch) * r[0], r[1], r[2], r[3]) for r in refined]))
    return res


def check_admissible(case, ref):
    """The generator's assertions on a case (every channel): the report's coarse grid brackets the global extremum and refines to it;
    no second local extremum within SEPARATION (relative) of it."""
    mp = _mp()
    T, C, cfg, S = case["T"], case["C"], case["cfg"], case["samples"]
    total = piece_starts(T)[1]
    for ch in range(NCH):
        r = ref[ch]
        if r["const"]:
            continue
        scale = abs(r["value"])
        for v, i, s, t in r["refined"]:
            if abs(t - r["t"]) <= mp.mpf("1e-9") * total:
                continue                                   # the same extremum (seen from the other side of a junction)
            assert abs(v - r["value"]) > SEPARATION * scale, (case["name"], CH_NAMES[ch], "second extremum", float(v), float(r["value"]), float(t), float(r["t"]))
        i = r["piece"]
        ci, Ti = mpc(C[i]), float(T[i])
        fun = lambda x: _sign(ch) * channels_mp(ci, x, cfg)[ch]      # noqa: E731
        ts = [sample_time(Ti, S, j) for j in range(S + 1)]
        g = [fun(mp.mpf(x)) for x in ts]
        ok = False
        for j in range(S + 1):
            start = j == 0 or j == S or (g[j] >= g[j - 1] and g[j] >= g[j + 1])
            lo, hi = mp.mpf(ts[max(j - 1, 0)]), mp.mpf(ts[min(j + 1, S)])
            if not start or not (lo <= r["s"] <= hi):
                continue
            v, x = golden_max_mp(fun, lo, hi, mp.mpf(MP_BRACKET) * Ti)
            v = max(v, g[j])
            if abs(v - _sign(ch) * r["value"]) <= mp.mpf("1e-25") * max(scale, mp.mpf("1e-300")):
                ok = True
                break
        assert ok, (case["name"], CH_NAMES[ch], "the coarse grid does not bracket the global extremum", float(r["s"]), Ti, S)


def one_ulp_patterns(c, T):
    rng = np.random.default_rng(20240607)
    out = []
    for _ in range(2):
        s = rng.integers(0, 2, size=19) * 2 - 1
        out.append((c + s[:18].reshape(3, 6) * np.spacing(np.abs(c)), T + s[18] * np.spacing(T), int(s[18])))
    return out


def conditioning(case, ref):
    """(e_cond[6], kappa[6]) of a case's reference extrema."""
    mp = _mp()
    e_cond, kappa = [], []
    for ch in range(NCH):
        r = ref[ch]
        i = r["piece"]
        c, Ti, cfg = case["C"][i], float(case["T"][i]), case["cfg"]
        f0 = r["value"]
        e = mp.mpf(0)
        for c1, T1, _ in one_ulp_patterns(c, Ti):
            f1 = channels_mp(mpc(c1), r["s"] * mp.mpf(T1) / mp.mpf(Ti), cfg)[ch]
            e = max(e, abs(f1 - f0) / abs(f0) if f0 != 0 else abs(f1 - f0))
        e_cond.append(float(e))
        interior = (not r["const"]) and r["s"] > mp.mpf("1e-9") * Ti and r["s"] < Ti * (1 - mp.mpf("1e-9"))
        if interior and f0 != 0:
            h = mp.mpf("1e-12") * Ti
            ci = mpc(c)
            f2 = (channels_mp(ci, r["s"] + h, cfg)[ch] - 2 * f0 + channels_mp(ci, r["s"] - h, cfg)[ch]) / (h * h)
            kappa.append(float(abs(f2) * Ti * Ti / abs(f0)))
        else:
            kappa.append(0.0)
    return e_cond, kappa


def bound(e_cond, kappa, tol_t=TOL_T):
    return 32.0 * max(e_cond, 2.0 ** -50) + 0.5 * kappa * tol_t * tol_t


def rel_err(x, ref):
    """|x - ref| / |ref|; a zero reference admits only zero."""
    if ref == 0:
        return 0.0 if x == 0 else math.inf
    return abs(x - ref) / abs(ref)


# ---- sampler ------------------------------------------------------------------------------------------------------------------
def stamps(case):
    """0, sum(T), every junction and one ulp either side of it, two out-of-range stamps, seeded uniform ones up to at least 50."""
    T = [float(x) for x in case["T"]]
    starts, total = piece_starts(T)
    out = [0.0, total, -0.25 * T[0], total + 0.5 * T[-1]]
    for t in starts[1:]:
        out += [t, np.nextafter(t, -np.inf), np.nextafter(t, np.inf)]
    rng = np.random.default_rng(len(T) * 1000 + int(case["samples"]))
    out += list(rng.uniform(0.0, total, max(0, 50 - len(out))))
    return np.array(out, dtype=np.float64)


def sampler_reference(case, t):
    """(rows n x 20 as mp lists, e_cond n x 7): the model at the float64 (piece, local time) of every stamp; e_cond per group of a row
    = max |movement| / max |reference| of the group under one-ulp changes of the coefficients and the local time."""
    mp = _mp()
    rows, econd = [], []
    T = [float(x) for x in case["T"]]
    for tt in t:
        i, s = locate(T, float(tt))
        c = case["C"][i]
        r0 = state_mp(mpc(c), mp.mpf(s), case["cfg"])
        e = [mp.mpf(0)] * len(GROUPS)
        for c1, _, sg in one_ulp_patterns(c, T[i]):
            r1 = state_mp(mpc(c1), mp.mpf(s + sg * np.spacing(s)), case["cfg"])
            for k, (a, b) in enumerate(GROUPS):
                scale = max(abs(x) for x in r0[a:b])
                mv = max(abs(x - y) for x, y in zip(r1[a:b], r0[a:b]))
                e[k] = max(e[k], mv / scale if scale != 0 else mv)
        rows.append(r0)
        econd.append([float(x) for x in e])
    return rows, np.array(econd)


def group_errors(row, ref_row):
    """Per group max |x - ref| / max |ref| (a zero group admits only zero)."""
    out = []
    for a, b in GROUPS:
        scale = float(np.max(np.abs(ref_row[a:b])))
        err = float(np.max(np.abs(np.asarray(row[a:b]) - ref_row[a:b])))
        out.append(err / scale if scale > 0 else (0.0 if err == 0 else math.inf))
    return out


# ---- the cases ----------------------------------------------------------------------------------------------------------------
def pack(C):
    """(N, 3, 6) -> the 6N x 3 column-major image isdf_eval takes (18 N doubles)."""
    C = np.asarray(C, dtype=np.float64)
    return np.ascontiguousarray(C.transpose(1, 0, 2)).reshape(-1)


def _rest(state, T):
    return dr.quintic_to_rest(state["v0"], state["a0"], state["j0"], T)


def _junction_pair():
    """Two pieces of duration 1 that are point reflections of each other about the junction state: p0(s) = 2 p* - p1(1 - s) (up to a bump
    that is flat to fourth order at the junction).  Speed
    and acceleration are then even about the junction, where v . a < 0 and a . j < 0 put a cusp maximum of both; every coefficient is a
    small dyadic number and T = 1, so both pieces evaluate the junction state without rounding: the same bits from either side."""
    from fractions import Fraction as F
    k = [F(3, 2), F(-1), F(1, 2)]
    c1s = [F(17, 16) * x for x in k]                 # velocity at the junction
    c2s = [-2 * x for x in k]                        # half the acceleration: v . a < 0
    c3s = [F(1, 4) * x for x in k]                   # a sixth of the jerk: a . j < 0; 3 c1 + 4 c2 + 3 c3 = -65 k / 16 makes c5 dyadic
    bump = [F(1, 16), F(0), F(-1, 16)]
    p1 = np.zeros((3, 6)); p0 = np.zeros((3, 6))
    for d in range(3):
        c1, c2, c3 = c1s[d], c2s[d], c3s[d]
        A, B = c1 + 2 * c2 + 3 * c3, 2 * c2 + 6 * c3
        c5 = (3 * A - B) / 5
        c4 = (-A - 5 * c5) / 4
        q = [F(int(dr.CENTRE[d])), c1, c2, c3, c4, c5]
        # 2 q0 - q(1 - s) in powers of s
        m = [F(0)] * 6
        for k in range(6):
            for r in range(k + 1):
                m[r] -= q[k] * math.comb(k, r) * (-1) ** r
        m[0] += 2 * q[0]
        # ... plus bump[d] (1 - s)^5 on the earlier piece: velocity, acceleration and jerk at the junction stay what they are, but the
        # two pieces stop being twins away from it (their rest ends would otherwise tie in body rate)
        for r in range(6):
            m[r] += bump[d] * math.comb(5, r) * (-1) ** r
        for k in range(6):
            p1[d, k], p0[d, k] = float(q[k]), float(m[k])
            assert F(p1[d, k]) == q[k] and F(p0[d, k]) == m[k], (d, k)
            assert (q[k] * 2 ** 20).denominator == 1 and (m[k] * 2 ** 20).denominator == 1, (d, k, q[k], m[k])
    return np.stack([p0, p1])


def _specs():
    """(name, T, C (N, 3, 6), samples (0: the default 4 x INTERVS), config overrides)"""
    S = []
    S.append(("n1_mid", [1.0], [_rest(dr.MID, 1.0)], 0, {}))
    S.append(("n1_tilted", [1.0], [_rest(dr.TILTED, 1.0)], 0, {}))
    S.append(("n1_omg", [1.0], [_rest(dr.OMG, 1.0)], 0, {}))
    S.append(("n2_junction", [1.0, 1.0], _junction_pair(), 0, {}))
    S.append(("n3_durations", [0.05, 12.0, 1.0], [_rest(dr.MID, 0.05), _rest(dr.MID, 12.0), _rest(dr.VEL, 1.0)], 0, {}))
    mono = np.zeros((3, 6))
    d = np.array([0.6, 0.0, 0.8])
    mono[:, 0] = dr.CENTRE
    mono[:, 1], mono[:, 2], mono[:, 3] = 0.5 * d, 0.75 * d, 0.25 * d
    S.append(("n1_monotone", [1.5], [mono], 0, {}))
    hov = np.zeros((2, 3, 6)); hov[:, :, 0] = dr.CENTRE
    S.append(("n2_hover", [1.0, 2.0], hov, 0, {}))
    for s in (2, 5, 63, 64, 65, 257):
        S.append((f"samples_{s}", [1.0], [_rest(dr.THETA, 1.0)], s, {}))
    rng = np.random.default_rng(130)
    T, C = [], []
    for _ in range(130):
        Ti = float(rng.uniform(0.5, 1.5))
        st = dict(v0=rng.uniform(-2, 2, 3), a0=rng.uniform(-2, 2, 3), j0=rng.uniform(-3, 3, 3))
        T.append(Ti); C.append(_rest(st, Ti))
    S.append(("n130", T, C, 5, {}))
    for b, (sa, sb) in enumerate(((dr.MID, dr.OMG), (dr.VEL, dr.THETA), (dr.TILTED, dr.MID))):
        S.append((f"batch_{b}", [0.8, 1.25], [_rest(sa, 0.8), _rest(sb, 1.25)], 0, {}))
    return S


BATCH = ["batch_0", "batch_1", "batch_2"]


def build_cases():
    out = []
    for name, T, C, samples, over in _specs():
        cfg = dr.full_cfg(over)
        out.append(dict(name=name, T=np.array(T, dtype=np.float64), C=np.array(C, dtype=np.float64), cfg=cfg,
                        samples=samples if samples > 0 else 4 * INTERVS, samples_param=samples))
    assert len({c["name"] for c in out}) == len(out)
    return out


def make_config(pkg, case, **kw):
    """The product configuration of a case (any variant will do: the report does not use it)."""
    over = dict(case["cfg"])
    over.update(integral_intervs=INTERVS)
    over.update(kw)
    return pkg.synth.default_config(pkg.capi.V1_SWEPT, **over)


# ---- the committed golden ------------------------------------------------------------------------------------------------------
def load_golden(path=GOLDEN):
    """[dict(name, T, C, coeffs, cfg, samples, samples_param, value[6], time[6], piece[6], s_digits, value_digits, e_cond[6], kappa[6], const[6],
    stamps, rows, rows_e_cond)] from the npz alone (no mpmath)."""
    z = np.load(path)
    keys = [str(k) for k in z["cfg_keys"]]
    out = []
    for i, name in enumerate(z["names"]):
        n = int(z["n_pieces"][i]); o = int(z["piece_offset"][i])
        ns = int(z["n_stamps"][i]); so = int(z["stamp_offset"][i])
        C = z["C"][o:o + n]
        out.append(dict(name=str(name), T=z["T"][o:o + n].copy(), C=C, coeffs=pack(C), cfg=dict(zip(keys, (float(v) for v in z["cfg"][i]))),
                        samples=int(z["samples"][i]), samples_param=int(z["samples_param"][i]), value=z["value"][i], time=z["time"][i],
                        piece=z["piece"][i], s_digits=[str(s) for s in z["s_digits"][i]], value_digits=[str(s) for s in z["value_digits"][i]],
                        e_cond=z["e_cond"][i], kappa=z["kappa"][i], const=z["const"][i],
                        stamps=z["stamps"][so:so + ns].copy(), rows=z["rows"][so:so + ns], rows_e_cond=z["rows_e_cond"][so:so + ns]))
    return out


def check_report(case, rep, label, tol_t=TOL_T, with_time=True):
    """Holds a report (dict with value[6], time[6], piece[6]) to the golden of its case: returns the printed lines, raises on a miss."""
    lines, bad = [], []
    T = [float(x) for x in case["T"]]
    for ch in range(NCH):
        b = bound(float(case["e_cond"][ch]), float(case["kappa"][ch]), tol_t)
        ev = rel_err(float(rep["value"][ch]), float(case["value"][ch]))
        et = 0.0
        if with_time:
            # the model at the reported time, on the reported piece (a junction time belongs to two pieces; a discontinuous trajectory has two
            # values there): local time = reported time - the piece's start, exact in mp, kept inside the piece.  No tolerance in t.
            mp = _mp()
            i = int(rep["piece"][ch])
            starts, _ = piece_starts(T)
            ref = mp.mpf(case["value_digits"][ch])
            s = min(max(mp.mpf(float(rep["time"][ch])) - mp.mpf(starts[i]), mp.mpf(0)), mp.mpf(T[i]))
            at = channels_mp(mpc(case["C"][i]), s, case["cfg"])[ch]
            et = float(abs(at - ref) / abs(ref)) if ref != 0 else (0.0 if at == 0 else math.inf)
        lines.append(f"{label} {case['name']:<14} {CH_NAMES[ch]:<10} value {float(rep['value'][ch]):.17g} ref {float(case['value'][ch]):.17g} err {ev:.2e} "
                     f"time {float(rep['time'][ch]):.12g} ref {float(case['time'][ch]):.12g} model-at-time err {et:.2e} bound {b:.2e}")
        if not (ev <= b and et <= b):
            bad.append(lines[-1])
        if case["const"][ch] and float(rep["time"][ch]) != 0.0:
            bad.append(lines[-1] + "  (constant channel: the time must be 0)")
    return lines, bad
