"""Shared by tests/test_shape_program_host.py and tests/test_gpu_shape_program.py: the point set, the programs no class exercises,
and a numpy restatement of the reference's CSG op library (src/utils/include/utils/Shape.hpp:1684-2317) that evaluates an
expression TREE the way the reference's nested closures do - a transform node maps the points and hands them to its subtree -
and reports, per point, which side every min / max / clip / ?: chose.  It shares no code with the library: it is what the
library's push-down compilation and its evaluators are compared with."""
import math

import numpy as np

PI = 3.14159265358979323846


def points():
    """5 000 seeded points in a cube of side 12 m, plus 200 on the axes and the coordinate planes"""
    rng = np.random.default_rng(20240917)
    P = rng.uniform(-6.0, 6.0, (5000, 3))
    Q = rng.uniform(-6.0, 6.0, (200, 3))
    for i in range(200):
        if i < 100:
            Q[i, i % 3] = 0.0                                  # a coordinate plane
        else:
            Q[i, (i + 1) % 3] = 0.0; Q[i, (i + 2) % 3] = 0.0   # an axis
    return np.concatenate([P, Q])


def novel_programs(csg):
    """name -> expression tree: the ops no registered class exercises"""
    X, Y = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)
    k = 0.3
    return {
        "shell_dilate_blend": csg.shellOp(csg.dilateOp(csg.blendOp(csg.twistOp(csg.rounded_box((2.0, 1.5, 3.0), 0.2), 0.4),
                                                                   [csg.translate(csg.icosahedron(1.2), (0.8, -0.5, 0.3))], 0.35), 0.1), 0.2),
        "scale_pyramid": csg.scale(csg.pyramid(1.5), (2.0, 1.5, 2.5)),
        "erode_negate_capped_cylinder": csg.erodeOp(csg.negateOp(csg.capped_cylinder((-0.5, 0.2, -1.0), (0.7, 0.4, 1.5), 0.8)), 0.15),
        "smooth_union_rotate_to": csg.unionOp(
            csg.rotate_to(csg.unionOp(csg.ellipsoid((2.0, 1.2, 0.9)), csg.translate(csg.octahedron(1.1), (2.5, 0.0, 0.0)), k), X, Y),
            [csg.rotate_to(csg.unionOp(csg.translate(csg.tetrahedron(0.9), (0.0, -2.5, 1.0)), csg.translate(csg.dodecahedron(0.8), (0.0, 2.0, -1.5)), k),
                           Y, (0.0, -1.0, 0.0)),                              # anti-parallel, a not along x: perpendicular = a x (1, 0, 0)
             csg.rotate_to(csg.unionOp(csg.capsule((-1.0, -1.0, 2.0), (1.5, 0.5, 3.0), 0.4), csg.translate(csg.rounded_cylinder(0.9, 0.2, 1.6), (-2.0, 1.0, -2.5)), k),
                           X, (-1.0, 0.0, 0.0))], k),                         # anti-parallel, a along x: perpendicular = a x (0, 1, 0)
        # (the op library's wireframe_box forms q from p itself, :1787 - not the WireframeBox class's formula, so no class exercises it)
        "wireframe_box_op": csg.wireframe_box((1.8, 2.5, 3.5), 0.1),
    }


# ---------------------------------------------------------------- numpy restatement
class _Rec:
    """collects, per point, the side every min / max / clip / ?: chose.  A min / max whose operands agree to 1e-13 (relative to
    max(1, |a|)) is no decision: either side gives the same value to rounding - 1e-13 over the stencil's 1e-5 is 1e-8 in a
    gradient component, far inside the 1e-5 the gradients are held to.  (The CSG class needs this: its second cylinder,
    rotate_to(c, X, Y), is the first one turned about its own axis, so min(c1, c2) is a tie that rounding decides at every
    point, Shape.hpp:2291-2294.)"""
    def __init__(self):
        self.rows = []

    def _side(self, a, b, c):
        return c & (np.abs(a - b) > 1e-13 * np.maximum(1.0, np.abs(a)))

    def mn(self, a, b):
        a, b = np.broadcast_arrays(np.asarray(a, dtype=float), np.asarray(b, dtype=float))
        self.rows.append(self._side(a, b, b < a))
        return np.where(b < a, b, a)          # std::min(a, b)

    def mx(self, a, b):
        a, b = np.broadcast_arrays(np.asarray(a, dtype=float), np.asarray(b, dtype=float))
        self.rows.append(self._side(a, b, a < b))
        return np.where(a < b, b, a)          # std::max(a, b)

    def clip(self, v, lo, hi):                # Shape.hpp:1703: max(min(v, hi), lo)
        return self.mx(self.mn(v, hi), lo)

    def sel(self, c, a, b):
        self.rows.append(np.asarray(c))
        return np.where(c, a, b)


def _norm(v):
    z = v[0] * v[0] + v[1] * v[1] + v[2] * v[2]
    return [c / math.sqrt(z) for c in v] if z > 0 else list(v)


def _rotation(angle, axis):                   # :2021-2034
    x, y, z = _norm(axis)
    s, c = math.sin(angle), math.cos(angle)
    m = 1 - c
    return np.array([[m * x * x + c, m * x * y + z * s, m * z * x - y * s],
                     [m * x * y - z * s, m * y * y + c, m * y * z + x * s],
                     [m * z * x + y * s, m * y * z - x * s, m * z * z + c]])


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _box_g(r, a, b, c):
    ma, mb, mc = r.mx(a, 0.0), r.mx(b, 0.0), r.mx(c, 0.0)
    return np.sqrt(ma * ma + mb * mb + mc * mc) + r.mn(r.mx(a, r.mx(b, c)), 0.0)


def _primitive(capi, op, P, x, y, z, r):
    if op == capi.OP_SPHERE:                  # :1724
        dx, dy, dz = x - P[1], y - P[2], z - P[3]
        return np.sqrt(dx * dx + dy * dy + dz * dz) - P[0]
    if op == capi.OP_CAPSULE:                 # :1734
        pa = [x - P[0], y - P[1], z - P[2]]; ba = [P[3] - P[0], P[4] - P[1], P[5] - P[2]]
        h = r.clip((pa[0] * ba[0] + pa[1] * ba[1] + pa[2] * ba[2]) / (ba[0] * ba[0] + ba[1] * ba[1] + ba[2] * ba[2]), 0.0, 1.0)
        e = [pa[i] - h * ba[i] for i in range(3)]
        return np.sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]) - P[6]
    if op == capi.OP_BOX:                     # :1748
        return _box_g(r, np.abs(x - P[3]) - P[0] / 2.0, np.abs(y - P[4]) - P[1] / 2.0, np.abs(z - P[5]) - P[2] / 2.0)
    if op == capi.OP_ROUNDED_BOX:             # :1761
        q = [np.abs(c) - s / 2 + P[3] for c, s in zip((x, y, z), P[:3])]
        m = [r.mx(c, 0.0) for c in q]
        return np.sqrt(m[0] * m[0] + m[1] * m[1] + m[2] * m[2]) + r.mn(r.mn(r.mn(q[0], q[1]), q[2]), 0.0) - P[3]
    if op == capi.OP_WIREFRAME_BOX:           # :1774
        th = P[3]
        px, py, pz = (np.abs(c) - s / 2 - th / 2 for c, s in zip((x, y, z), P[:3]))
        qx, qy, qz = (np.abs(c + th / 2) - th / 2 for c in (x, y, z))
        return r.mn(r.mn(_box_g(r, px, qy, qz), _box_g(r, qx, py, qz)), _box_g(r, qx, qy, pz))
    if op == capi.OP_TORUS:                   # :1799
        a = np.sqrt(x * x + y * y) - P[0]
        return np.sqrt(a * a + z * z) - P[1]
    if op == capi.OP_CYLINDER:                # :1812
        return np.sqrt(x * x + y * y) - P[0]
    if op == capi.OP_CAPPED_CYLINDER:         # :1823
        ba = [P[3] - P[0], P[4] - P[1], P[5] - P[2]]; pa = [x - P[0], y - P[1], z - P[2]]
        baba = ba[0] * ba[0] + ba[1] * ba[1] + ba[2] * ba[2]
        paba = pa[0] * ba[0] + pa[1] * ba[1] + pa[2] * ba[2]
        e = [pa[i] * baba - ba[i] * paba for i in range(3)]
        xx = np.sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]) - P[6] * baba
        yy = np.abs(paba - baba * 0.5) - baba * 0.5
        x2, y2 = xx * xx, yy * yy * baba
        inside = r.mx(xx, yy) < 0
        d = r.sel(inside, -r.mn(x2, y2), r.sel(xx > 0, x2, 0.0) + r.sel(yy > 0, y2, 0.0))
        return np.copysign(np.sqrt(np.abs(d)) / baba, d)
    if op == capi.OP_ROUNDED_CYLINDER:        # :1851
        dx = np.sqrt(x * x + y * y) - P[0] + P[1]; dy = np.abs(z) - (P[2] / 2) + P[1]
        mx_, my_ = r.mx(dx, 0.0), r.mx(dy, 0.0)
        return r.mn(r.mx(dx, dy), 0.0) + np.sqrt(mx_ * mx_ + my_ * my_) - P[1]
    if op == capi.OP_CAPPED_CONE:             # :1864 (parameters: ra, rb, a, b)
        ra, rb = P[0], P[1]
        ba = [P[5] - P[2], P[6] - P[3], P[7] - P[4]]; pa = [x - P[2], y - P[3], z - P[4]]
        rba = rb - ra
        baba = ba[0] * ba[0] + ba[1] * ba[1] + ba[2] * ba[2]
        papa = pa[0] * pa[0] + pa[1] * pa[1] + pa[2] * pa[2]
        paba = (pa[0] * ba[0] + pa[1] * ba[1] + pa[2] * ba[2]) / baba
        xx = np.sqrt(papa - paba * paba * baba)
        cax = r.mx(0.0, xx - r.sel(paba < 0.5, ra, rb))
        cay = np.abs(paba - 0.5) - 0.5
        k = rba * rba + baba
        f = r.clip((rba * (xx - ra) + paba * baba) / k, 0.0, 1.0)
        cbx = xx - ra - f * rba
        cby = paba - f
        s = r.sel((cbx < 0) & (cay < 0), -1.0, 1.0)
        d = np.sqrt(r.mn(cax * cax + cay * cay * baba, cbx * cbx + cby * cby * baba))
        return s * np.sqrt(np.abs(d)) / abs(baba)
    if op == capi.OP_ROUNDED_CONE:            # :1886
        r1, r2, h = P[:3]
        qx = np.sqrt(x * x + y * y); qy = z
        b = (r1 - r2) / h
        a = math.sqrt(1.0 - b * b)
        k = -b * qx + a * qy
        c1 = np.sqrt(qx * qx + qy * qy) - r1
        c2 = np.sqrt(qx * qx + (qy - h) * (qy - h)) - r2
        c3 = (a * qx + b * qy) - r1
        return r.sel(k < 0, c1, r.sel(k > a * h, c2, c3))
    if op == capi.OP_ELLIPSOID:               # :1902
        pn = np.sqrt(x * x + y * y + z * z); sn = math.sqrt(P[0] * P[0] + P[1] * P[1] + P[2] * P[2])
        k0 = pn / sn
        k1 = pn / (sn * sn)
        return k0 * (k0 - 1.0) / k1
    if op == capi.OP_PYRAMID:                 # :1913
        h = P[0]
        a0, a1 = np.abs(x) - 0.5, np.abs(y) - 0.5
        w = a1 > a0
        px = r.sel(w, a1, a0); pz = np.where(w, a0, a1); py = z
        m2 = h * h + 0.25
        qx, qy, qz = pz, h * py - 0.5 * px, h * px + 0.5 * py
        s = r.mx(-qx, 0.0)
        t = r.clip((qy - 0.5 * pz) / (m2 + 0.25), 0.0, 1.0)
        aT = m2 * ((qx + s) * (qx + s)) + qy * qy
        bT = m2 * ((qx + 0.5 * t) * (qx + 0.5 * t)) + (qy - m2 * t) * (qy - m2 * t)
        d2 = r.sel(r.mn(qy, -qx * m2 - qy * 0.5) > 0, 0.0, r.mn(aT, bT))
        return np.sqrt((d2 + qz * qz) / m2) * np.copysign(1.0, r.mx(qz, -py))
    if op == capi.OP_TETRAHEDRON:             # :1941
        return (r.mx(np.abs(x + y) - z, np.abs(x - y) + z) - P[0]) / math.sqrt(3)
    if op == capi.OP_OCTAHEDRON:              # :1953
        return (np.abs(x) + np.abs(y) + np.abs(z) - P[0]) * math.tan(PI / 6.0)
    if op in (capi.OP_DODECAHEDRON, capi.OP_ICOSAHEDRON):      # :1962, :1978
        ico = op == capi.OP_ICOSAHEDRON
        rr = P[0] * 0.8506507174597755 if ico else P[0]
        X, Y, Z = _norm([(3 + math.sqrt(5)) / 2, 1, 0] if ico else [1 + math.sqrt(5) / 2.0, 1, 0])
        nx, ny, nz = np.abs(x) / rr, np.abs(y) / rr, np.abs(z) / rr
        a = nx * X + ny * Y + nz * Z
        b = nx * Z + ny * X + nz * Y
        c = nx * Y + ny * Z + nz * X
        m = r.mx(r.mx(a, b), c) - X
        if not ico:
            return m * rr
        w = math.sqrt(3.0) / 3.0
        return r.mx(m, (nx * w + ny * w + nz * w) - X) * rr
    raise ValueError(op)


def np_eval(capi, node, pts, rec=None):
    """(sdf[n], sides[n_decisions, n]) of an expression tree at pts[n, 3]"""
    r = rec if rec is not None else _Rec()
    pts = np.asarray(pts, dtype=float)

    def ev(nd, x, y, z):
        op, P = nd.op, nd.params
        if not nd.children:
            return _primitive(capi, op, P, x, y, z, r) + 0.0 * x
        if op == capi.OP_TRANSLATE:           # :1996
            return ev(nd.children[0], x - P[0], y - P[1], z - P[2])
        if op == capi.OP_SCALE:               # :2006
            return ev(nd.children[0], x / P[0], y / P[1], z / P[2]) * min(P)
        if op in (capi.OP_ROTATE, capi.OP_ROTATE_TO):      # :2021, :2043
            if op == capi.OP_ROTATE:
                M = _rotation(P[0], P[1:4])
            else:
                a, b = _norm(P[0:3]), _norm(P[3:6])
                dot = b[0] * a[0] + b[1] * a[1] + b[2] * a[2]
                if abs(dot - 1) < 1.1920928955078125e-07:
                    return ev(nd.children[0], x, y, z)
                if abs(dot + 1) < 1.1920928955078125e-07:
                    M = _rotation(PI, _cross(a, [0, 1, 0]) if (a[1] == 0 and a[2] == 0) else _cross(a, [1, 0, 0]))
                else:
                    M = _rotation(math.acos(dot), _cross(b, a))
            return ev(nd.children[0], M[0, 0] * x + M[0, 1] * y + M[0, 2] * z, M[1, 0] * x + M[1, 1] * y + M[1, 2] * z, M[2, 0] * x + M[2, 1] * y + M[2, 2] * z)
        if op in (capi.OP_TWIST, capi.OP_BEND):            # :2198, :2215
            ang = P[0] * z if op == capi.OP_TWIST else P[0] * x
            c, s = np.cos(ang), np.sin(ang)
            return ev(nd.children[0], c * x - s * y, s * x + c * y, z)
        if op == capi.OP_NEGATE: return -ev(nd.children[0], x, y, z)
        if op == capi.OP_DILATE: return ev(nd.children[0], x, y, z) - P[0]
        if op == capi.OP_ERODE: return ev(nd.children[0], x, y, z) + P[0]
        if op == capi.OP_SHELL: return np.abs(ev(nd.children[0], x, y, z)) - P[0] / 2
        d1 = ev(nd.children[0], x, y, z); d2 = ev(nd.children[1], x, y, z); k = P[0]
        if op == capi.OP_BLEND:               # :2232
            return k * d2 + (1.0 - k) * d1
        if op == capi.OP_UNION:               # :2087
            if k == 0.0: return r.mn(d1, d2)
            h = r.clip(0.5 + 0.5 * (d2 - d1) / k, 0.0, 1.0)
            return (d2 + (d1 - d2) * h) - k * h * (1.0 - h)
        if op == capi.OP_DIFFERENCE:          # :2134
            if k == 0.0: return r.mx(d1, -d2)
            h = r.clip(0.5 - 0.5 * (d2 + d1) / k, 0.0, 1.0)
            return (d1 + (-d2 - d1) * h) + k * h * (1.0 - h)
        if op == capi.OP_INTERSECTION:        # :2178
            if k == 0.0: return r.mx(d1, d2)
            h = r.clip(0.5 - 0.5 * (d2 - d1) / k, 0.0, 1.0)
            return (d2 + (d1 - d2) * h) + k * h * (1.0 - h)
        raise ValueError(op)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = ev(node, pts[:, 0], pts[:, 1], pts[:, 2])
    sides = np.array([np.broadcast_to(row, s.shape) for row in r.rows], dtype=bool).reshape(len(r.rows), len(s))
    return s, sides


def stencil_same_branch(capi, node, pts):
    """mask[n]: all seven evaluations of the central-difference stencil (Shape.hpp:32-57; dx = 5e-6) take the same side of every
    min / max / clip / ?: as the point itself"""
    pts = np.asarray(pts, dtype=float)
    _, base = np_eval(capi, node, pts)
    ok = np.ones(len(pts), dtype=bool)
    dx = 0.000005
    for a in range(3):
        lo = pts.copy(); lo[:, a] -= dx
        hi = lo.copy(); hi[:, a] += 2 * dx
        for q in (lo, hi):
            _, s = np_eval(capi, node, q)
            ok &= (s == base).all(axis=0)
    return ok
