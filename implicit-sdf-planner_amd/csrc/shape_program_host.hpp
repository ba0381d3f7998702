// ISDF_SHAPE_PROGRAM on the host, plain C++ (no HIP): the validator and the lowering isdf_set_shape_program runs before it touches
// the ctx, and the evaluator behind isdf_shape_program_eval_host - the device interpreter's arithmetic (dev_shape_program.hpp)
// operation for operation, each opcode restating the lines of the reference's CSG class it is named after
// (src/utils/include/utils/Shape.hpp:1684-2317; include/isdf_accel.h lists them).
// LOWERING: what the reference computes once, when a closure is made, is computed once here and travels in the instruction:
//   ROTATE (angle, axis)  -> ROTATE with p[0..8] = the row-major rotation matrix (:2023-2034)
//   ROTATE_TO (a, b)      -> nothing, ROTATE about perpendicular(a) by pi, or ROTATE about b x a by acos(a.b) (:2043-2059)
//   TETRAHEDRON           p[1] = sqrt(3) (:1948)          OCTAHEDRON    p[1] = tan(pi / 6) (:1957)
//   DODECAHEDRON          p[1..3] = the normalised x (:1964-1965)
//   ICOSAHEDRON           p[0] = r * 0.8506507174597755, p[1..3] = the normalised x, p[4] = sqrt(3) / 3 (:1980-1983)
// The lowered list never holds ROTATE_TO and is never longer than the program.
#pragma once
#include "../../include/isdf_accel.h"
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <string>
#include <vector>

namespace isdf_host {

constexpr double PROG_PI = 3.14159265358979323846;      // the reference's PI (Shape.hpp:29)

// parameters an opcode reads (-1: unknown opcode); what it does to the stack: pops, pushes
inline int prog_op_params(int op) {
    switch (op) {
    case ISDF_OP_SPHERE: return 4;
    case ISDF_OP_CAPSULE: return 7;
    case ISDF_OP_BOX: return 6;
    case ISDF_OP_ROUNDED_BOX: return 4;
    case ISDF_OP_WIREFRAME_BOX: return 4;
    case ISDF_OP_TORUS: return 2;
    case ISDF_OP_CYLINDER: return 1;
    case ISDF_OP_CAPPED_CYLINDER: return 7;
    case ISDF_OP_ROUNDED_CYLINDER: return 3;
    case ISDF_OP_CAPPED_CONE: return 8;
    case ISDF_OP_ROUNDED_CONE: return 3;
    case ISDF_OP_ELLIPSOID: return 3;
    case ISDF_OP_PYRAMID: case ISDF_OP_TETRAHEDRON: case ISDF_OP_OCTAHEDRON: case ISDF_OP_DODECAHEDRON: case ISDF_OP_ICOSAHEDRON: return 1;
    case ISDF_OP_TRANSLATE: case ISDF_OP_SCALE: return 3;
    case ISDF_OP_ROTATE: return 4;
    case ISDF_OP_ROTATE_TO: return 6;
    case ISDF_OP_TWIST: case ISDF_OP_BEND: return 1;
    case ISDF_OP_MUL: case ISDF_OP_DILATE: case ISDF_OP_ERODE: case ISDF_OP_SHELL: return 1;
    case ISDF_OP_NEGATE: return 0;
    case ISDF_OP_UNION: case ISDF_OP_DIFFERENCE: case ISDF_OP_INTERSECTION: case ISDF_OP_BLEND: return 1;
    default: return -1;
    }
}
inline bool prog_is_primitive(int op) { return op >= ISDF_OP_SPHERE && op <= ISDF_OP_ICOSAHEDRON; }
inline bool prog_is_domain(int op) { return op >= ISDF_OP_TRANSLATE && op <= ISDF_OP_BEND; }
inline bool prog_is_unary(int op) { return op >= ISDF_OP_MUL && op <= ISDF_OP_SHELL; }
inline bool prog_is_binary(int op) { return op >= ISDF_OP_UNION && op <= ISDF_OP_BLEND; }

// Eigen's normalize(): unchanged unless the squared norm is > 0
inline void prog_normalize(double v[3]) {
    const double z = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
    if (z > 0) { const double s = std::sqrt(z); for (int i = 0; i < 3; i++) v[i] /= s; }
}
// rotate(): the matrix of :2023-2034, row-major
inline void prog_rotation(double angle, const double axis[3], double R[9]) {
    double n[3] = {axis[0], axis[1], axis[2]};
    prog_normalize(n);
    const double x = n[0], y = n[1], z = n[2], s = std::sin(angle), c = std::cos(angle), m = 1 - c;
    R[0] = m * x * x + c;     R[1] = m * x * y + z * s; R[2] = m * z * x - y * s;
    R[3] = m * x * y - z * s; R[4] = m * y * y + c;     R[5] = m * y * z + x * s;
    R[6] = m * z * x + y * s; R[7] = m * y * z - x * s; R[8] = m * z * z + c;
}

// Validates the whole program and lowers it (see the head of this file).  ISDF_OK, or ISDF_ERR_INVALID_ARG with the reason in err.
inline int prog_lower(const isdf_shape_instr *in, int n, std::vector<isdf_shape_instr> &out, std::string &err) {
    out.clear();
    if (!in || n < 1) { err = "shape program: fewer than 1 instruction"; return ISDF_ERR_INVALID_ARG; }
    if (n > ISDF_PROGRAM_MAX_INSTR) { err = "shape program: more than 64 instructions"; return ISDF_ERR_INVALID_ARG; }
    int depth = 0;
    for (int i = 0; i < n; i++) {
        const isdf_shape_instr &I = in[i];
        const std::string at = "shape program, instruction " + std::to_string(i) + ": ";
        const int np = prog_op_params(I.op);
        if (np < 0) { err = at + "unknown opcode " + std::to_string(I.op); return ISDF_ERR_INVALID_ARG; }
        for (int k = 0; k < np; k++)
            if (!std::isfinite(I.p[k])) { err = at + "non-finite parameter"; return ISDF_ERR_INVALID_ARG; }
        isdf_shape_instr L{};
        L.op = I.op;
        for (int k = 0; k < np; k++) L.p[k] = I.p[k];
        bool keep = true;
        const double *p = I.p;
        switch (I.op) {
        case ISDF_OP_CAPSULE: case ISDF_OP_CAPPED_CYLINDER: case ISDF_OP_CAPPED_CONE: {
            const double *a = I.op == ISDF_OP_CAPPED_CONE ? p + 2 : p, *b = a + 3;
            const double ba[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
            if (ba[0] * ba[0] + ba[1] * ba[1] + ba[2] * ba[2] == 0.0) { err = at + "a == b (ba.ba == 0)"; return ISDF_ERR_INVALID_ARG; }
            break;
        }
        case ISDF_OP_ROUNDED_CONE:
            if (p[2] == 0.0) { err = at + "h == 0"; return ISDF_ERR_INVALID_ARG; }
            break;
        case ISDF_OP_SCALE:
            if (p[0] == 0.0 || p[1] == 0.0 || p[2] == 0.0) { err = at + "zero scale factor"; return ISDF_ERR_INVALID_ARG; }
            break;
        case ISDF_OP_UNION: case ISDF_OP_DIFFERENCE: case ISDF_OP_INTERSECTION:
            if (p[0] < 0.0) { err = at + "k < 0"; return ISDF_ERR_INVALID_ARG; }
            break;
        case ISDF_OP_TETRAHEDRON: L.p[1] = std::sqrt(3.0); break;
        case ISDF_OP_OCTAHEDRON: L.p[1] = std::tan(PROG_PI / 6.0); break;
        case ISDF_OP_DODECAHEDRON: {
            double x[3] = {1 + std::sqrt(5.0) / 2.0, 1, 0};
            prog_normalize(x);
            L.p[1] = x[0]; L.p[2] = x[1]; L.p[3] = x[2];
            break;
        }
        case ISDF_OP_ICOSAHEDRON: {
            double x[3] = {(3 + std::sqrt(5.0)) / 2, 1, 0};
            prog_normalize(x);
            L.p[0] = p[0] * 0.8506507174597755;
            L.p[1] = x[0]; L.p[2] = x[1]; L.p[3] = x[2]; L.p[4] = std::sqrt(3.0) / 3.0;
            break;
        }
        case ISDF_OP_ROTATE: prog_rotation(p[0], p + 1, L.p); break;
        case ISDF_OP_ROTATE_TO: {
            double a[3] = {p[0], p[1], p[2]}, b[3] = {p[3], p[4], p[5]};
            prog_normalize(a); prog_normalize(b);
            const double dot = b[0] * a[0] + b[1] * a[1] + b[2] * a[2];
            L.op = ISDF_OP_ROTATE;
            if (std::fabs(dot - 1) < FLT_EPSILON) keep = false;
            else if (std::fabs(dot + 1) < FLT_EPSILON) {
                // _perpendicular (:1707-1721): a x (0, 1, 0) when a lies along x, else a x (1, 0, 0); a zero a throws there and
                // cannot get here (its dot is 0)
                const bool along_x = a[1] == 0 && a[2] == 0;
                const double e[3] = {along_x ? 0.0 : 1.0, along_x ? 1.0 : 0.0, 0.0};
                const double v[3] = {a[1] * e[2] - a[2] * e[1], a[2] * e[0] - a[0] * e[2], a[0] * e[1] - a[1] * e[0]};
                prog_rotation(PROG_PI, v, L.p);
            } else {
                const double v[3] = {b[1] * a[2] - b[2] * a[1], b[2] * a[0] - b[0] * a[2], b[0] * a[1] - b[1] * a[0]};
                prog_rotation(std::acos(dot), v, L.p);
            }
            break;
        }
        default: break;
        }
        if (prog_is_primitive(I.op)) depth++;
        else if (prog_is_unary(I.op)) { if (depth < 1) { err = at + "stack underflow"; return ISDF_ERR_INVALID_ARG; } }
        else if (prog_is_binary(I.op)) { if (depth < 2) { err = at + "stack underflow"; return ISDF_ERR_INVALID_ARG; } depth--; }
        if (depth > ISDF_PROGRAM_MAX_DEPTH) { err = at + "stack depth above 8"; return ISDF_ERR_INVALID_ARG; }
        if (keep) out.push_back(L);
    }
    if (depth != 1) { err = "shape program: " + std::to_string(depth) + " values left on the stack (a program ends with exactly one)"; out.clear(); return ISDF_ERR_INVALID_ARG; }
    return ISDF_OK;
}

inline double prog_clip(double v, double lo, double hi) { return std::max(std::min(v, hi), lo); }
inline double prog_box_q(double qx, double qy, double qz) {
    const double mx = std::max(qx, 0.0), my = std::max(qy, 0.0), mz = std::max(qz, 0.0);
    return std::sqrt(mx * mx + my * my + mz * mz) + std::min(std::max(qx, std::max(qy, qz)), 0.0);
}

// one primitive of a LOWERED program at q
inline double prog_primitive(const isdf_shape_instr &I, const double q[3]) {
    const double *P = I.p;
    const double x = q[0], y = q[1], z = q[2];
    switch (I.op) {
    case ISDF_OP_SPHERE: {
        const double dx = x - P[1], dy = y - P[2], dz = z - P[3];
        return std::sqrt(dx * dx + dy * dy + dz * dz) - P[0];
    }
    case ISDF_OP_CAPSULE: {
        const double pa[3] = {x - P[0], y - P[1], z - P[2]}, ba[3] = {P[3] - P[0], P[4] - P[1], P[5] - P[2]};
        const double h = prog_clip((pa[0] * ba[0] + pa[1] * ba[1] + pa[2] * ba[2]) / (ba[0] * ba[0] + ba[1] * ba[1] + ba[2] * ba[2]), 0.0, 1.0);
        const double ex = pa[0] - h * ba[0], ey = pa[1] - h * ba[1], ez = pa[2] - h * ba[2];
        return std::sqrt(ex * ex + ey * ey + ez * ez) - P[6];
    }
    case ISDF_OP_BOX:
        return prog_box_q(std::fabs(x - P[3]) - P[0] / 2.0, std::fabs(y - P[4]) - P[1] / 2.0, std::fabs(z - P[5]) - P[2] / 2.0);
    case ISDF_OP_ROUNDED_BOX: {
        const double r = P[3];
        const double qx = std::fabs(x) - P[0] / 2 + r, qy = std::fabs(y) - P[1] / 2 + r, qz = std::fabs(z) - P[2] / 2 + r;
        const double mx = std::max(qx, 0.0), my = std::max(qy, 0.0), mz = std::max(qz, 0.0);
        const double len = std::sqrt(mx * mx + my * my + mz * mz);
        const double mn = std::min(std::min(std::min(qx, qy), qz), 0.0);
        return len + mn - r;
    }
    case ISDF_OP_WIREFRAME_BOX: {
        const double th = P[3];
        const double px = std::fabs(x) - P[0] / 2 - th / 2, py = std::fabs(y) - P[1] / 2 - th / 2, pz = std::fabs(z) - P[2] / 2 - th / 2;
        const double qx = std::fabs(x + th / 2) - th / 2, qy = std::fabs(y + th / 2) - th / 2, qz = std::fabs(z + th / 2) - th / 2;      // from p itself (:1787)
        return std::min(std::min(prog_box_q(px, qy, qz), prog_box_q(qx, py, qz)), prog_box_q(qx, qy, pz));
    }
    case ISDF_OP_TORUS: {
        const double a = std::sqrt(x * x + y * y) - P[0];
        return std::sqrt(a * a + z * z) - P[1];
    }
    case ISDF_OP_CYLINDER: return std::sqrt(x * x + y * y) - P[0];
    case ISDF_OP_CAPPED_CYLINDER: {
        const double ba[3] = {P[3] - P[0], P[4] - P[1], P[5] - P[2]}, pa[3] = {x - P[0], y - P[1], z - P[2]};
        const double baba = ba[0] * ba[0] + ba[1] * ba[1] + ba[2] * ba[2];
        const double paba = pa[0] * ba[0] + pa[1] * ba[1] + pa[2] * ba[2];
        const double ex = pa[0] * baba - ba[0] * paba, ey = pa[1] * baba - ba[1] * paba, ez = pa[2] * baba - ba[2] * paba;
        const double xx = std::sqrt(ex * ex + ey * ey + ez * ez) - P[6] * baba;
        const double yy = std::fabs(paba - (baba * 0.5)) - (baba * 0.5);
        const double x2 = xx * xx, y2 = yy * yy * baba;
        double d;
        if (std::max(xx, yy) < 0) d = -std::min(x2, y2);
        else d = (xx > 0 ? x2 : 0) + (yy > 0 ? y2 : 0);
        return std::copysign(std::sqrt(std::fabs(d)) / baba, d);
    }
    case ISDF_OP_ROUNDED_CYLINDER: {
        const double dx = std::sqrt(x * x + y * y) - P[0] + P[1], dy = std::fabs(z) - (P[2] / 2) + P[1];
        const double mx = std::max(dx, 0.0), my = std::max(dy, 0.0);
        return std::min(std::max(dx, dy), 0.0) + std::sqrt(mx * mx + my * my) - P[1];
    }
    case ISDF_OP_CAPPED_CONE: {
        const double ra = P[0], rb = P[1];
        const double ba[3] = {P[5] - P[2], P[6] - P[3], P[7] - P[4]}, pa[3] = {x - P[2], y - P[3], z - P[4]};
        const double rba = rb - ra;
        const double baba = ba[0] * ba[0] + ba[1] * ba[1] + ba[2] * ba[2];
        const double papa = pa[0] * pa[0] + pa[1] * pa[1] + pa[2] * pa[2];
        const double paba = (pa[0] * ba[0] + pa[1] * ba[1] + pa[2] * ba[2]) / baba;
        const double xx = std::sqrt(papa - paba * paba * baba);
        const double cax = std::max(0.0, xx - (paba < 0.5 ? ra : rb));
        const double cay = std::fabs(paba - 0.5) - 0.5;
        const double k = rba * rba + baba;
        const double f = prog_clip((rba * (xx - ra) + paba * baba) / k, 0.0, 1.0);
        const double cbx = xx - ra - f * rba;
        const double cby = paba - f;
        const double s = (cbx < 0 && cay < 0) ? -1 : 1;
        const double d = std::sqrt(std::min(cax * cax + cay * cay * baba, cbx * cbx + cby * cby * baba));
        return s * std::sqrt(std::fabs(d)) / std::fabs(baba);
    }
    case ISDF_OP_ROUNDED_CONE: {
        const double r1 = P[0], r2 = P[1], h = P[2];
        const double qx = std::sqrt(x * x + y * y), qy = z;
        const double b = (r1 - r2) / h;
        const double a = std::sqrt(1.0 - b * b);
        const double k = -b * qx + a * qy;
        const double c1 = std::sqrt(qx * qx + qy * qy) - r1;
        const double c2 = std::sqrt((qx - 0) * (qx - 0) + (qy - h) * (qy - h)) - r2;
        const double c3 = (a * qx + b * qy) - r1;
        return (k < 0) ? c1 : ((k > a * h) ? c2 : c3);
    }
    case ISDF_OP_ELLIPSOID: {
        const double pn = std::sqrt(x * x + y * y + z * z), sn = std::sqrt(P[0] * P[0] + P[1] * P[1] + P[2] * P[2]);
        const double k0 = pn / sn;
        const double k1 = pn / (sn * sn);
        return k0 * (k0 - 1.0) / k1;
    }
    case ISDF_OP_PYRAMID: {
        const double h = P[0];
        double ax = std::fabs(x) - 0.5, ay = std::fabs(y) - 0.5;
        if (ay > ax) std::swap(ax, ay);
        const double px = ax, py = z, pz = ay;
        const double m2 = h * h + 0.25;
        const double qx = pz, qy = h * py - 0.5 * px, qz = h * px + 0.5 * py;
        const double s = std::max(-qx, 0.0);
        const double t = prog_clip((qy - 0.5 * pz) / (m2 + 0.25), 0.0, 1.0);
        const double aT = m2 * ((qx + s) * (qx + s)) + qy * qy;
        const double bT = m2 * ((qx + 0.5 * t) * (qx + 0.5 * t)) + (qy - m2 * t) * (qy - m2 * t);
        const double d2 = (std::min(qy, -qx * m2 - qy * 0.5) > 0) ? 0 : std::min(aT, bT);
        return std::sqrt((d2 + qz * qz) / m2) * std::copysign(1.0, std::max(qz, -py));
    }
    case ISDF_OP_TETRAHEDRON: return (std::max(std::fabs(x + y) - z, std::fabs(x - y) + z) - P[0]) / P[1];
    case ISDF_OP_OCTAHEDRON: return (std::fabs(x) + std::fabs(y) + std::fabs(z) - P[0]) * P[1];
    case ISDF_OP_DODECAHEDRON: case ISDF_OP_ICOSAHEDRON: {
        const double r = P[0], X = P[1], Y = P[2], Z = P[3];
        const double nx = std::fabs(x) / r, ny = std::fabs(y) / r, nz = std::fabs(z) / r;
        const double a = nx * X + ny * Y + nz * Z;
        const double b = nx * Z + ny * X + nz * Y;
        const double c = nx * Y + ny * Z + nz * X;
        if (I.op == ISDF_OP_DODECAHEDRON) return (std::max(std::max(a, b), c) - X) * r;
        const double d = (nx * P[4] + ny * P[4] + nz * P[4]) - X;
        return std::max(std::max(std::max(a, b), c) - X, d) * r;
    }
    default: return std::nan("");
    }
}

// a LOWERED program at the point p (already behind the body offset).  Guarded against programs the validator would have
// rejected (NaN), so that it is safe on arbitrary instruction arrays.
inline double prog_eval(const isdf_shape_instr *I, int n, const double p[3]) {
    double st[ISDF_PROGRAM_MAX_DEPTH];
    int sp = 0;
    double q[3] = {p[0], p[1], p[2]};
    for (int pc = 0; pc < n; pc++) {
        const isdf_shape_instr &in = I[pc];
        const double *P = in.p;
        const int op = in.op;
        if (prog_is_primitive(op)) {
            if (sp >= ISDF_PROGRAM_MAX_DEPTH) return std::nan("");
            st[sp++] = prog_primitive(in, q);
            q[0] = p[0]; q[1] = p[1]; q[2] = p[2];
        } else if (prog_is_domain(op)) {
            switch (op) {
            case ISDF_OP_TRANSLATE: q[0] -= P[0]; q[1] -= P[1]; q[2] -= P[2]; break;
            case ISDF_OP_SCALE: q[0] /= P[0]; q[1] /= P[1]; q[2] /= P[2]; break;
            case ISDF_OP_ROTATE: {
                const double x = q[0], y = q[1], z = q[2];
                q[0] = P[0] * x + P[1] * y + P[2] * z; q[1] = P[3] * x + P[4] * y + P[5] * z; q[2] = P[6] * x + P[7] * y + P[8] * z;
                break;
            }
            case ISDF_OP_TWIST: case ISDF_OP_BEND: {
                const double x = q[0], y = q[1], ang = op == ISDF_OP_TWIST ? P[0] * q[2] : P[0] * q[0];
                const double c = std::cos(ang), s = std::sin(ang);
                q[0] = c * x - s * y; q[1] = s * x + c * y;
                break;
            }
            default: return std::nan("");      // (ROTATE_TO does not survive the lowering)
            }
        } else if (prog_is_unary(op)) {
            if (sp < 1) return std::nan("");
            double &v = st[sp - 1];
            switch (op) {
            case ISDF_OP_MUL: v = v * P[0]; break;
            case ISDF_OP_NEGATE: v = -v; break;
            case ISDF_OP_DILATE: v = v - P[0]; break;
            case ISDF_OP_ERODE: v = v + P[0]; break;
            default: v = std::fabs(v) - P[0] / 2; break;      // SHELL
            }
        } else if (prog_is_binary(op)) {
            if (sp < 2) return std::nan("");
            const double d2 = st[--sp], d1 = st[sp - 1], k = P[0];
            double r;
            if (op == ISDF_OP_BLEND) r = k * d2 + (1.0 - k) * d1;
            else if (op == ISDF_OP_UNION) {
                if (k == 0.0) r = std::min(d1, d2);
                else { const double h = prog_clip(0.5 + 0.5 * (d2 - d1) / k, 0.0, 1.0); const double m = d2 + (d1 - d2) * h; r = m - k * h * (1.0 - h); }
            } else if (op == ISDF_OP_DIFFERENCE) {
                if (k == 0.0) r = std::max(d1, -d2);
                else { const double h = prog_clip(0.5 - 0.5 * (d2 + d1) / k, 0.0, 1.0); const double m = d1 + (-d2 - d1) * h; r = m + k * h * (1.0 - h); }
            } else {
                if (k == 0.0) r = std::max(d1, d2);
                else { const double h = prog_clip(0.5 - 0.5 * (d2 - d1) / k, 0.0, 1.0); const double m = d2 + (d1 - d2) * h; r = m + k * h * (1.0 - h); }
            }
            st[sp - 1] = r;
        } else return std::nan("");
    }
    return sp == 1 ? st[0] : std::nan("");
}

// the body offset (p - trans) * Rotate in front of the program (nullptr: none), getonlySDF / getonlyGrad1 of DEFINE_USEFUL_FUNCTION
struct ProgBody { bool ident = true; double trans[3] = {0, 0, 0}, rot[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}; };
inline ProgBody prog_body(const double *trans, const double *rotate) {
    ProgBody B;
    if (trans) for (int i = 0; i < 3; i++) B.trans[i] = trans[i];
    if (rotate) for (int i = 0; i < 9; i++) B.rot[i] = rotate[i];
    B.ident = B.trans[0] == 0.0 && B.trans[1] == 0.0 && B.trans[2] == 0.0;
    for (int i = 0; i < 9; i++) B.ident = B.ident && B.rot[i] == ((i % 4 == 0) ? 1.0 : 0.0);
    return B;
}
inline double prog_sdf(const isdf_shape_instr *I, int n, const ProgBody &B, const double pr[3]) {
    if (B.ident) return prog_eval(I, n, pr);
    const double dx = pr[0] - B.trans[0], dy = pr[1] - B.trans[1], dz = pr[2] - B.trans[2];
    const double *R = B.rot;
    const double q[3] = {dx * R[0] + dy * R[3] + dz * R[6], dx * R[1] + dy * R[4] + dz * R[7], dx * R[2] + dy * R[5] + dz * R[8]};
    return prog_eval(I, n, q);
}
inline void prog_grad(const isdf_shape_instr *I, int n, const ProgBody &B, const double pr[3], double g[3]) {
    const double dx = 0.000005;
    for (int a = 0; a < 3; a++) {
        double t[3] = {pr[0], pr[1], pr[2]};
        t[a] -= dx;
        const double sdfold = prog_sdf(I, n, B, t);
        t[a] += 2 * dx;
        g[a] = prog_sdf(I, n, B, t) - sdfold;
    }
    for (int a = 0; a < 3; a++) g[a] = g[a] / (2 * dx);
    const double z = g[0] * g[0] + g[1] * g[1] + g[2] * g[2];
    if (z > 0) { const double s = std::sqrt(z); for (int a = 0; a < 3; a++) g[a] /= s; }
}

}  // namespace isdf_host
