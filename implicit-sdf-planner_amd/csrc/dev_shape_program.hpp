// ISDF_SHAPE_PROGRAM on the device: the interpreter of a LOWERED instruction list (csrc/shape_program_host.hpp lowers and validates;
// include/isdf_accel.h lists the opcodes and the lines of the reference's CSG class each restates, Shape.hpp:1684-2317).
// Included by dev_shapes.hpp, which reaches it only from the KIND == ISDF_SHAPE_PROGRAM instantiations.
// Instruction words and parameters are the same for every lane: they are read through the CONSTANT address space from a
// wave-uniform address, i.e. with scalar loads, and the opcode switch never diverges.  The value stack is eight named slots moved
// by unrolled selects on the (scalar) stack pointer, not an indexed private array, so that it can live in registers.
// No contraction of the reference's products and sums (the formulas shared with the built-in kinds - box_q, sdf_cappedcone,
// sdf_roundedcone - are compiled as they are for those kinds).
#pragma once

namespace isdf {

template <typename T> using prog_cptr = const T __attribute__((address_space(4))) *;
__device__ __forceinline__ prog_cptr<isdf_shape_instr> prog_const_uni(const isdf_shape_instr *p) {
    const unsigned long long a = (unsigned long long)p;
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)a), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(a >> 32));
    return (prog_cptr<isdf_shape_instr>)(((unsigned long long)hi << 32) | lo);
}

__device__ __forceinline__ double prog_capsule(const double *P, d3 p) {
#pragma clang fp contract(off)
    const d3 pa = mk3(p.x - P[0], p.y - P[1], p.z - P[2]), ba = mk3(P[3] - P[0], P[4] - P[1], P[5] - P[2]);
    const double h = clipT((pa.x * ba.x + pa.y * ba.y + pa.z * ba.z) / (ba.x * ba.x + ba.y * ba.y + ba.z * ba.z), 0.0, 1.0);
    const double ex = pa.x - h * ba.x, ey = pa.y - h * ba.y, ez = pa.z - h * ba.z;
    return m_sqrt(ex * ex + ey * ey + ez * ez) - P[6];
}
__device__ __forceinline__ double prog_rounded_box(const double *P, d3 p) {
#pragma clang fp contract(off)
    const double r = P[3];
    const double qx = m_abs(p.x) - P[0] / 2 + r, qy = m_abs(p.y) - P[1] / 2 + r, qz = m_abs(p.z) - P[2] / 2 + r;
    const double mx = m_max(qx, 0.0), my = m_max(qy, 0.0), mz = m_max(qz, 0.0);
    const double len = m_sqrt(mx * mx + my * my + mz * mz);
    const double mn = m_min(m_min(m_min(qx, qy), qz), 0.0);
    return len + mn - r;
}
__device__ __forceinline__ double prog_wireframe_box(const double *P, d3 p) {
#pragma clang fp contract(off)
    const double th = P[3];
    const double px = m_abs(p.x) - P[0] / 2 - th / 2, py = m_abs(p.y) - P[1] / 2 - th / 2, pz = m_abs(p.z) - P[2] / 2 - th / 2;
    const double qx = m_abs(p.x + th / 2) - th / 2, qy = m_abs(p.y + th / 2) - th / 2, qz = m_abs(p.z + th / 2) - th / 2;      // from p itself (:1787), unlike the class (sdf_wireframebox)
    return m_min(m_min(box_q(px, qy, qz), box_q(qx, py, qz)), box_q(qx, qy, pz));
}
__device__ __forceinline__ double prog_capped_cylinder(const double *P, d3 p) {
#pragma clang fp contract(off)
    const d3 ba = mk3(P[3] - P[0], P[4] - P[1], P[5] - P[2]), pa = mk3(p.x - P[0], p.y - P[1], p.z - P[2]);
    const double baba = ba.x * ba.x + ba.y * ba.y + ba.z * ba.z;
    const double paba = pa.x * ba.x + pa.y * ba.y + pa.z * ba.z;
    const double ex = pa.x * baba - ba.x * paba, ey = pa.y * baba - ba.y * paba, ez = pa.z * baba - ba.z * paba;
    const double x = m_sqrt(ex * ex + ey * ey + ez * ez) - P[6] * baba;
    const double y = m_abs(paba - (baba * 0.5)) - (baba * 0.5);
    const double x2 = x * x, y2 = y * y * baba;
    const double d = (m_max(x, y) < 0) ? -m_min(x2, y2) : ((x > 0 ? x2 : 0.0) + (y > 0 ? y2 : 0.0));
    return copysign(m_sqrt(m_abs(d)) / baba, d);
}
__device__ __forceinline__ double prog_rounded_cylinder(const double *P, d3 p) {
#pragma clang fp contract(off)
    const double dx = m_sqrt(p.x * p.x + p.y * p.y) - P[0] + P[1], dy = m_abs(p.z) - (P[2] / 2) + P[1];
    const double mx = m_max(dx, 0.0), my = m_max(dy, 0.0);
    return m_min(m_max(dx, dy), 0.0) + m_sqrt(mx * mx + my * my) - P[1];
}
__device__ __forceinline__ double prog_ellipsoid(const double *P, d3 p) {
#pragma clang fp contract(off)
    const double pn = m_sqrt(p.x * p.x + p.y * p.y + p.z * p.z), sn = m_sqrt(P[0] * P[0] + P[1] * P[1] + P[2] * P[2]);
    const double k0 = pn / sn;
    const double k1 = pn / (sn * sn);
    return k0 * (k0 - 1.0) / k1;
}
__device__ __forceinline__ double prog_pyramid(const double *P, d3 p) {
#pragma clang fp contract(off)
    const double h = P[0];
    const double a0 = m_abs(p.x) - 0.5, a1 = m_abs(p.y) - 0.5;
    const bool w = a1 > a0;
    const double px = w ? a1 : a0, py = p.z, pz = w ? a0 : a1;
    const double m2 = h * h + 0.25;
    const double qx = pz, qy = h * py - 0.5 * px, qz = h * px + 0.5 * py;
    const double s = m_max(-qx, 0.0);
    const double t = clipT((qy - 0.5 * pz) / (m2 + 0.25), 0.0, 1.0);
    const double aT = m2 * ((qx + s) * (qx + s)) + qy * qy;
    const double bT = m2 * ((qx + 0.5 * t) * (qx + 0.5 * t)) + (qy - m2 * t) * (qy - m2 * t);
    const double d2 = (m_min(qy, -qx * m2 - qy * 0.5) > 0) ? 0.0 : m_min(aT, bT);
    return m_sqrt((d2 + qz * qz) / m2) * copysign(1.0, m_max(qz, -py));
}
__device__ __forceinline__ double prog_hedron(const double *P, d3 p, bool icosa) {      // dodecahedron / icosahedron
#pragma clang fp contract(off)
    const double r = P[0], X = P[1], Y = P[2], Z = P[3];
    const double nx = m_abs(p.x) / r, ny = m_abs(p.y) / r, nz = m_abs(p.z) / r;
    const double a = nx * X + ny * Y + nz * Z;
    const double b = nx * Z + ny * X + nz * Y;
    const double c = nx * Y + ny * Z + nz * X;
    const double m = m_max(m_max(a, b), c) - X;
    if (!icosa) return m * r;
    const double d = (nx * P[4] + ny * P[4] + nz * P[4]) - X;
    return m_max(m, d) * r;
}

__device__ __forceinline__ double prog_primitive(int op, const double *P, d3 q) {
#pragma clang fp contract(off)
    switch (op) {
    case ISDF_OP_SPHERE: { const d3 d = mk3(q.x - P[1], q.y - P[2], q.z - P[3]); return m_sqrt(d.x * d.x + d.y * d.y + d.z * d.z) - P[0]; }
    case ISDF_OP_CAPSULE: return prog_capsule(P, q);
    case ISDF_OP_BOX: return box_q(m_abs(q.x - P[3]) - P[0] / 2.0, m_abs(q.y - P[4]) - P[1] / 2.0, m_abs(q.z - P[5]) - P[2] / 2.0);
    case ISDF_OP_ROUNDED_BOX: return prog_rounded_box(P, q);
    case ISDF_OP_WIREFRAME_BOX: return prog_wireframe_box(P, q);
    case ISDF_OP_TORUS: { const double a = m_sqrt(q.x * q.x + q.y * q.y) - P[0]; return m_sqrt(a * a + q.z * q.z) - P[1]; }
    case ISDF_OP_CYLINDER: return m_sqrt(q.x * q.x + q.y * q.y) - P[0];
    case ISDF_OP_CAPPED_CYLINDER: return prog_capped_cylinder(P, q);
    case ISDF_OP_ROUNDED_CYLINDER: return prog_rounded_cylinder(P, q);
    case ISDF_OP_CAPPED_CONE: return sdf_cappedcone(P, q);
    case ISDF_OP_ROUNDED_CONE: return sdf_roundedcone(P, q);
    case ISDF_OP_ELLIPSOID: return prog_ellipsoid(P, q);
    case ISDF_OP_PYRAMID: return prog_pyramid(P, q);
    case ISDF_OP_TETRAHEDRON: return (m_max(m_abs(q.x + q.y) - q.z, m_abs(q.x - q.y) + q.z) - P[0]) / P[1];
    case ISDF_OP_OCTAHEDRON: return (m_abs(q.x) + m_abs(q.y) + m_abs(q.z) - P[0]) * P[1];
    case ISDF_OP_DODECAHEDRON: return prog_hedron(P, q, false);
    default: return prog_hedron(P, q, true);      // ISDF_OP_ICOSAHEDRON (the host validated the opcodes)
    }
}

// the program at a point already behind the body offset
__device__ __forceinline__ double prog_sdf(const DevShape &S, d3 p) {
#pragma clang fp contract(off)
    const prog_cptr<isdf_shape_instr> I = prog_const_uni(S.prog);
    const int n = __builtin_amdgcn_readfirstlane(S.prog_n);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0, s5 = 0.0, s6 = 0.0, s7 = 0.0;     // the value stack; sp: values on it (wave-uniform)
    int sp = 0;
    d3 q = p;
    // TOP(k): the value k below the top (slot sp - 1 - k); SET(slot, v): v into that slot
#define ISDF_PROG_TOP(k) (sp == 1 + (k) ? s0 : sp == 2 + (k) ? s1 : sp == 3 + (k) ? s2 : sp == 4 + (k) ? s3 : sp == 5 + (k) ? s4 : sp == 6 + (k) ? s5 : sp == 7 + (k) ? s6 : s7)
#define ISDF_PROG_SET(slot, v) do { const int sl_ = (slot); const double v_ = (v); \
        s0 = sl_ == 0 ? v_ : s0; s1 = sl_ == 1 ? v_ : s1; s2 = sl_ == 2 ? v_ : s2; s3 = sl_ == 3 ? v_ : s3; \
        s4 = sl_ == 4 ? v_ : s4; s5 = sl_ == 5 ? v_ : s5; s6 = sl_ == 6 ? v_ : s6; s7 = sl_ == 7 ? v_ : s7; } while (0)
    for (int pc = 0; pc < n; pc++) {
        const int op = I[pc].op;
        double P[9];
#pragma unroll
        for (int k = 0; k < 9; k++) P[k] = I[pc].p[k];
        if (op < ISDF_OP_TRANSLATE) {                    // a primitive: push, q back to the body-frame point
            ISDF_PROG_SET(sp, prog_primitive(op, P, q));
            sp++;
            q = p;
        } else if (op < ISDF_OP_MUL) {                   // the working point
            if (op == ISDF_OP_TRANSLATE) q = mk3(q.x - P[0], q.y - P[1], q.z - P[2]);
            else if (op == ISDF_OP_SCALE) q = mk3(q.x / P[0], q.y / P[1], q.z / P[2]);
            else if (op == ISDF_OP_ROTATE) q = mk3(P[0] * q.x + P[1] * q.y + P[2] * q.z, P[3] * q.x + P[4] * q.y + P[5] * q.z, P[6] * q.x + P[7] * q.y + P[8] * q.z);
            else {                                       // TWIST about z (:2198), BEND along x (:2215)
                double s, c;
                m_sincos(op == ISDF_OP_TWIST ? P[0] * q.z : P[0] * q.x, s, c);
                q = mk3(c * q.x - s * q.y, s * q.x + c * q.y, q.z);
            }
        } else if (op < ISDF_OP_UNION) {                 // the top of the stack
            const double v = ISDF_PROG_TOP(0);
            double r;
            if (op == ISDF_OP_MUL) r = v * P[0];
            else if (op == ISDF_OP_NEGATE) r = -v;
            else if (op == ISDF_OP_DILATE) r = v - P[0];
            else if (op == ISDF_OP_ERODE) r = v + P[0];
            else r = m_abs(v) - P[0] / 2;                // SHELL
            ISDF_PROG_SET(sp - 1, r);
        } else {                                         // two values -> one
            const double d2 = ISDF_PROG_TOP(0), d1 = ISDF_PROG_TOP(1), k = P[0];
            double r;
            if (op == ISDF_OP_BLEND) r = k * d2 + (1.0 - k) * d1;
            else if (k == 0.0) r = op == ISDF_OP_UNION ? m_min(d1, d2) : m_max(d1, op == ISDF_OP_DIFFERENCE ? -d2 : d2);
            else if (op == ISDF_OP_UNION) { const double h = clipT(0.5 + 0.5 * (d2 - d1) / k, 0.0, 1.0); const double m = d2 + (d1 - d2) * h; r = m - k * h * (1.0 - h); }
            else if (op == ISDF_OP_DIFFERENCE) { const double h = clipT(0.5 - 0.5 * (d2 + d1) / k, 0.0, 1.0); const double m = d1 + (-d2 - d1) * h; r = m + k * h * (1.0 - h); }
            else { const double h = clipT(0.5 - 0.5 * (d2 - d1) / k, 0.0, 1.0); const double m = d2 + (d1 - d2) * h; r = m + k * h * (1.0 - h); }
            sp--;
            ISDF_PROG_SET(sp - 1, r);
        }
    }
#undef ISDF_PROG_TOP
#undef ISDF_PROG_SET
    return s0;
}

} // namespace isdf
