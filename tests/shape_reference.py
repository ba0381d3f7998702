"""High-precision reference of the 15 analytic robot-shape formulas (the reference planner's Shape.hpp classes Torus, Cappedtorus,
CappedCone, RoundedCone, WireframeBox, BendLinear, TwistBox, BendBox, Table, Trefoil, SmoothDifference, SmoothIntersection, CSG, Box,
Ball), restated operation by operation in mpmath at 50 digits, and the points the plugin tests evaluate them at.

TEST INFRASTRUCTURE.  Reads no project code: a shape is a class name, its constants (the fp64 numbers the classes hold, taken as
exact), the body offset (trans, Rotate) and fp64 points.  Every function returns (sdf, margin): margin is the smallest distance of a
DISCONTINUOUS decision of the formula from its switching point (None: it has none) - CappedCone's `paba < 0.5` pick between ra and
rb and the sign of its radicand papa - paba^2 baba (relative to papa), Trefoil's atan2 on its axis (radius relative to |p|).  Every
other branch (min, max, clip, abs, selects between expressions that agree at the switch, the floor() pick of Trefoil: a rotation by a
multiple of pi at q.x = 0) is continuous and needs no margin.
"""
import math

import mpmath as mp

mp.mp.dps = 50
_0, _1, _H = mp.mpf(0), mp.mpf(1), mp.mpf("0.5")
PI64 = mp.mpf(3.14159265358979323846)          # the classes' PI: the fp64 number

KINDS = ["Torus", "Cappedtorus", "CappedCone", "RoundedCone", "WireframeBox", "BendLinear", "TwistBox", "BendBox", "Table", "Trefoil",
         "SmoothDifference", "SmoothIntersection", "CSG", "Box", "Ball"]


def _box_q(qx, qy, qz):
    mx, my, mz = max(qx, _0), max(qy, _0), max(qz, _0)
    return mp.sqrt(mx * mx + my * my + mz * mz) + min(max(qx, qy, qz), _0)


def _clip(v, lo, hi):
    return max(min(v, hi), lo)


def _torus(P, x, y, z):
    qx = mp.sqrt(x * x + z * z) - P[0]
    return mp.sqrt(qx * qx + y * y) - P[1], None


def _cappedtorus(P, x, y, z):
    scx, scy, ra, rb = P[0], P[1], P[2], P[3]
    x = abs(x)
    k = (x * scx + y * scy) if scy * x > scx * y else mp.sqrt(x * x + y * y)
    return mp.sqrt(x * x + y * y + z * z + ra * ra - 2 * ra * k) - rb, None


def _cappedcone(P, x, y, z):
    ra, rb = P[0], P[1]
    ax, ay, az, bx, by, bz = P[2:8]
    rba = rb - ra
    bax, bay, baz = bx - ax, by - ay, bz - az
    pax, pay, paz = x - ax, y - ay, z - az
    baba = bax * bax + bay * bay + baz * baz
    papa = pax * pax + pay * pay + paz * paz
    paba = (pax * bax + pay * bay + paz * baz) / baba
    rad = papa - paba * paba * baba
    margin = abs(paba - _H)
    if papa > 0:
        margin = min(margin, abs(rad) / papa)
    xr = mp.sqrt(max(rad, _0))
    cax = max(_0, xr - (ra if paba < _H else rb))
    cay = abs(paba - _H) - _H
    k = rba * rba + baba
    f = _clip((rba * (xr - ra) + paba * baba) / k, _0, _1)
    cbx = xr - ra - f * rba
    cby = paba - f
    s = -1 if (cbx < 0 and cay < 0) else 1
    d = mp.sqrt(min(cax * cax + cay * cay * baba, cbx * cbx + cby * cby * baba))
    return s * mp.sqrt(abs(d)) / abs(baba), margin


def _roundedcone(P, x, y, z):
    r1, r2, h = P[0], P[1], P[2]
    qx, qy = mp.sqrt(x * x + y * y), z
    b = (r1 - r2) / h
    a = mp.sqrt(1 - b * b)
    k = -b * qx + a * qy
    if k < 0:
        return mp.sqrt(qx * qx + qy * qy) - r1, None
    if k > a * h:
        return mp.sqrt(qx * qx + (qy - h) * (qy - h)) - r2, None
    return (a * qx + b * qy) - r1, None


def _wireframebox(P, x, y, z):
    th = P[3]
    p = [abs(c) - P[i] / 2 - th / 2 for i, c in enumerate((x, y, z))]
    q = [abs(c + th / 2) - th / 2 for c in p]
    return min(_box_q(p[0], q[1], q[2]), _box_q(q[0], p[1], q[2]), _box_q(q[0], q[1], p[2])), None


def _bendlinear(P, x, y, z):
    L, radius = P[0], P[1]
    t = _clip(((z + 1) * 2) / 4, _0, _1)         # p0 = (0, 0, -1), p1 = (0, 0, 1), v = (-1, 0, 0)
    u = 2 * t - 1
    e = 2 * t * t if t < _H else -_H * (u * (u - 2) - 1)
    ptx, pty, ptz = x - e, y, z
    pz = ptz + L
    h = max(min((pz * 2 * L) / (4 * L * L), _1), _0)
    dz = pz - h * 2 * L
    return mp.sqrt(ptx * ptx + pty * pty + dz * dz) - radius, None


def _twistbend(P, x, y, z, bend):
    ang = P[3] * (x if bend else z)
    c, s = mp.cos(ang), mp.sin(ang)
    rx, ry = c * x - s * y, s * x + c * y
    return _box_q(abs(rx) - P[0] / 2, abs(ry) - P[1] / 2, abs(z) - P[2] / 2), None


def _table(P, x, y, z):
    w = (abs(x), abs(y), z)
    f = []
    for t in range(2):
        a, b = P[6 * t:6 * t + 3], P[6 * t + 3:6 * t + 6]
        f.append(_box_q(*[abs(w[i] - (a[i] + b[i]) / 2) - (b[i] - a[i]) / 2 for i in range(3)]))
    return min(f), None


def _rot2d(qx, qy, a):
    ca, sa = mp.cos(a), mp.sin(a)
    return qx * ca + qy * sa, qy * ca - qx * sa


def _trefoil(P, x, y, z):
    r = mp.sqrt(x * x + y * y)
    n = mp.sqrt(x * x + y * y + z * z)
    margin = r / n if n > 0 else _0
    a = mp.atan2(y, x)
    qx, qy = r - P[0], -z
    qx, qy = _rot2d(qx, qy, mp.mpf("1.5") * a)
    qx, qy = _rot2d(qx, qy, -PI64 * mp.floor(mp.atan2(qy, qx) / PI64 + _H))
    qx -= 1
    dx, dy = abs(qx) - P[1], abs(qy) - P[2]
    mx, my = max(dx, _0), max(dy, _0)
    d = (min(max(dx, dy), _0) + mp.sqrt(mx * mx + my * my)) - P[3]
    return P[4] * min(d, mp.mpf(100)), margin


def _smooth(P, x, y, z, intersection):
    box = _box_q(abs(x) - P[0] / 2, abs(y) - P[1] / 2, abs(z) - P[2] / 2)
    sph = mp.sqrt(x * x + y * y + z * z) - P[3]
    kk = P[4]
    if not intersection:
        h = _clip(_H - _H * (box + sph) / kk, _0, _1)
        return (box - (box + sph) * h) + kk * h * (1 - h), None
    h = _clip(_H - _H * (sph - box) / kk, _0, _1)
    return (sph + (box - sph) * h) + kk * h * (1 - h), None


def _csg(P, x, y, z):
    # difference(intersection(sphere, box), union(cylinder about z, the same rotated X -> Y, the same rotated X -> Z)), sharp ops.
    # rotate_to(c, X, Y): angle acos(0) about Y x X = -Z; rotate_to(c, X, Z): about Z x X = +Y - quarter turns, exact here.
    f = max(mp.sqrt(x * x + y * y + z * z) - P[0], _box_q(abs(x) - P[1] / 2, abs(y) - P[1] / 2, abs(z) - P[1] / 2))

    def rot(n):
        nx, ny, nz = n
        s, c, m = _1, _0, _1
        return [[m * nx * nx + c, m * nx * ny + nz * s, m * nz * nx - ny * s],
                [m * nx * ny - nz * s, m * ny * ny + c, m * ny * nz + nx * s],
                [m * nz * nx + ny * s, m * ny * nz - nx * s, m * nz * nz + c]]
    c = [mp.sqrt(x * x + y * y) - P[2]]
    for n in ((0, 0, -1), (0, 1, 0)):
        R = rot(n)
        wx = R[0][0] * x + R[0][1] * y + R[0][2] * z
        wy = R[1][0] * x + R[1][1] * y + R[1][2] * z
        c.append(mp.sqrt(wx * wx + wy * wy) - P[2])
    return max(f, -min(c)), None


def _box(P, x, y, z):
    return _box_q(abs(x) - P[0], abs(y) - P[1], abs(z) - P[2]), None


_LOCAL = {
    "Torus": _torus, "Cappedtorus": _cappedtorus, "CappedCone": _cappedcone, "RoundedCone": _roundedcone,
    "WireframeBox": _wireframebox, "BendLinear": _bendlinear,
    "TwistBox": lambda P, x, y, z: _twistbend(P, x, y, z, False), "BendBox": lambda P, x, y, z: _twistbend(P, x, y, z, True),
    "Table": _table, "Trefoil": _trefoil,
    "SmoothDifference": lambda P, x, y, z: _smooth(P, x, y, z, False), "SmoothIntersection": lambda P, x, y, z: _smooth(P, x, y, z, True),
    "CSG": _csg, "Box": _box,
}


class Shape:
    """kind: a name of KINDS; params, trans[3], rotate[9] (row-major): fp64 numbers, exact."""

    def __init__(self, kind, params, trans=(0, 0, 0), rotate=(1, 0, 0, 0, 1, 0, 0, 0, 1)):
        self.kind = kind
        self.P = [mp.mpf(float(v)) for v in params]
        self.t = [mp.mpf(float(v)) for v in trans]
        self.R = [mp.mpf(float(v)) for v in rotate]

    def sdf(self, p):
        """(sdf, margin) at the body-frame point p (three fp64 numbers): the class formula at (p - trans) * Rotate; Ball ignores both."""
        x, y, z = (mp.mpf(float(c)) for c in p)
        if self.kind == "Ball":
            return mp.sqrt(x * x + y * y + z * z) - self.P[0], None
        dx, dy, dz = x - self.t[0], y - self.t[1], z - self.t[2]
        R = self.R
        return _LOCAL[self.kind](self.P, dx * R[0] + dy * R[3] + dz * R[6], dx * R[1] + dy * R[4] + dz * R[7], dx * R[2] + dy * R[5] + dz * R[8])

    def grad(self, p):
        """(gradient, margin, |quotient|): the classes' OWN difference quotient in high precision, at the fp64 points they evaluate
        (central: lo = c - dx, hi = lo + 2 dx in fp64, dx = 5e-6, normalised; Box: forward, dx = 0.01, not normalised; Ball: p / |p|)."""
        p = [float(c) for c in p]
        if self.kind == "Ball":
            n = mp.sqrt(sum(mp.mpf(c) ** 2 for c in p))
            return [mp.mpf(c) / n for c in p] if n > 0 else [_0, _0, _0], None, n
        margins = []
        g = []
        if self.kind == "Box":
            dx = 0.01
            s0, _ = self.sdf(p)
            for a in range(3):
                t = list(p)
                t[a] = t[a] + dx
                g.append((self.sdf(t)[0] - s0) / mp.mpf(dx))
            return g, None, _1
        dx = 0.000005
        for a in range(3):
            t = list(p)
            t[a] = t[a] - dx
            lo, m0 = self.sdf(t)
            t[a] = t[a] + 2 * dx
            hi, m1 = self.sdf(t)
            g.append((hi - lo) / mp.mpf(2 * dx))
            margins += [m for m in (m0, m1) if m is not None]
        n = mp.sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2])
        return ([c / n for c in g] if n > 0 else g), (min(margins) if margins else None), n


# ---- points ------------------------------------------------------------------------------------------------------------------------
_STEPS = (0.0, 1e-9, -1e-9, 5e-6, -5e-6, 1e-3, -1e-3)       # on the set; rounding scale; the gradient's own dx; well clear


def _special_local(kind, P, rng, n):
    """n base points (shape frame) on the singular sets and switching surfaces of the formula."""
    u = lambda lo, hi: float(rng.uniform(lo, hi))
    sets = [lambda: (0.0, u(-5, 5), u(-5, 5)), lambda: (u(-5, 5), 0.0, u(-5, 5)), lambda: (u(-5, 5), u(-5, 5), 0.0),
            lambda: (u(-5, 5), 0.0, 0.0), lambda: (0.0, u(-5, 5), 0.0), lambda: (0.0, 0.0, u(-5, 5))]
    if kind == "Torus":            # the tube's centre circle (inner root 0); the axis is among the generic sets
        sets += [lambda: (lambda th: (P[0] * math.cos(th), 0.0, P[0] * math.sin(th)))(u(0, 6.28))] * 2
    elif kind == "Cappedtorus":    # scy |x| = scx y: the switch between the two forms of k
        sets += [lambda: (lambda t: (t * abs(P[0]), t * P[1] * abs(P[0]) / P[0], u(-2, 2)))(u(0.1, 5))] * 3
    elif kind == "CappedCone":     # default axis z from -1 to 1: paba = 0.5 is z = 0 (generic); the clip of f at 0 and 1
        rba, baba = P[1] - P[0], 4.0
        k = rba * rba + baba

        def fclip(v):
            x = u(0, 5); paba = (v * k - rba * (x - P[0])) / baba; th = u(0, 6.28)
            return (x * math.cos(th), x * math.sin(th), 2 * paba - 1)
        sets += [lambda: fclip(0.0), lambda: fclip(1.0)]
    elif kind == "RoundedCone":    # k = 0 and k = a h
        b = (P[0] - P[1]) / P[2]; a = math.sqrt(1 - b * b)

        def kk(v):
            qx = u(0, 5); qy = (v + b * qx) / a; th = u(0, 6.28)
            return (qx * math.cos(th), qx * math.sin(th), qy)
        sets += [lambda: kk(0.0), lambda: kk(a * P[2]), lambda: (0.0, 0.0, u(-3, 6))]
    elif kind == "BendLinear":     # t clipped at z = -1 and 1, the switch of e at z = 0 (generic), the capsule's h clip near z = -+L
        sets += [lambda: (u(-3, 3), u(-3, 3), -1.0), lambda: (u(-3, 3), u(-3, 3), 1.0), lambda: (u(-3, 3), u(-3, 3), -P[0]), lambda: (u(-3, 3), u(-3, 3), P[0])]
    elif kind == "Trefoil":        # the axis; the cut of atan2 at y = 0, x < 0; the ring r = P[0]
        sets += [lambda: (0.0, 0.0, u(-3, 3)), lambda: (-u(0.1, 5), 0.0, u(-2, 2)), lambda: (lambda th: (P[0] * math.cos(th), P[0] * math.sin(th), u(-1, 1)))(u(0, 6.28))]
    elif kind in ("SmoothDifference", "SmoothIntersection", "CSG", "Ball"):      # the sphere
        r = P[3] if kind.startswith("Smooth") else P[0]

        def sph():
            v = rng.normal(size=3); v /= np_norm(v)
            return tuple(float(r * c) for c in v)
        sets += [sph] * 2
    elif kind in ("Box", "WireframeBox", "TwistBox", "BendBox", "Table"):        # the faces' planes
        hx = P[0] if kind == "Box" else (P[3] if kind == "Table" else P[0] / 2)
        sets += [lambda: (hx, u(-3, 3), u(-3, 3)), lambda: (-hx, u(-3, 3), u(-3, 3))]
    return [(0.0, 0.0, 0.0)] + [sets[i % len(sets)]() for i in range(n - 1)]


def np_norm(v):
    return math.sqrt(float(v[0]) ** 2 + float(v[1]) ** 2 + float(v[2]) ** 2)


def sample_points(kind, params, trans, rotate, n=2000, n_base=40, seed=0):
    """(points [n, 3] in the body frame, is_special [n]): uniform points in a cube of half side 6 and, for n_base base points on the
    formula's singular sets and switching surfaces, the point itself and the points +-1e-9, +-5e-6, +-1e-3 along a random direction -
    laid out in the SHAPE's frame and carried into the body frame by the inverse offset p = q Rotate^T + trans."""
    import numpy as np
    rng = np.random.default_rng(seed)
    P = [float(v) for v in params]
    R = np.array([float(v) for v in rotate]).reshape(3, 3)
    t = np.array([float(v) for v in trans])
    base = _special_local(kind, P, rng, n_base)
    sp = []
    for q in base:
        d = rng.normal(size=3); d /= np.linalg.norm(d)
        sp += [np.array(q) + s * d for s in _STEPS]
    sp = np.array(sp)
    if kind != "Ball":
        sp = sp @ R.T + t
    rnd = rng.uniform(-6, 6, size=(n - len(sp), 3))
    pts = np.concatenate([rnd, sp])
    return np.ascontiguousarray(pts), np.arange(n) >= len(rnd)


_TABLES = {}


def reference_table(kind, params, trans, rotate, pts):
    """The high-precision values at pts, computed once per (shape, points): dict with sdf (mpf per point), grad (3 mpf per point),
    qnorm (the difference quotient's norm before normalising, float) and margin (float; inf where the formula has no discontinuous
    decision), the smallest over the point itself and the gradient's six evaluation points."""
    import numpy as np
    key = (kind, tuple(float(v) for v in params), tuple(float(v) for v in trans), tuple(float(v) for v in rotate), pts.tobytes())
    if key in _TABLES:
        return _TABLES[key]
    S = Shape(kind, params, trans, rotate)
    sdf, grad, qn, margin = [], [], [], []
    for p in pts:
        v, m0 = S.sdf(p)
        g, m1, n = S.grad(p)
        sdf.append(v); grad.append(g); qn.append(float(n))
        ms = [m for m in (m0, m1) if m is not None]
        margin.append(float(min(ms)) if ms else float("inf"))
    _TABLES[key] = {"sdf": sdf, "grad": grad, "qnorm": np.array(qn), "margin": np.array(margin)}
    return _TABLES[key]


def abs_err(values, exact):
    """|values - exact| as fp64 numbers, the difference taken in high precision; values: fp64 array, exact: mpf per entry (nested alike)."""
    import numpy as np
    values = np.asarray(values, dtype=np.float64)
    flat = values.reshape(-1)
    ex = [e for row in exact for e in row] if values.ndim == 2 else list(exact)
    out = np.array([float(abs(mp.mpf(float(v)) - e)) if math.isfinite(v) else float("inf") for v, e in zip(flat, ex)])
    return out.reshape(values.shape)
