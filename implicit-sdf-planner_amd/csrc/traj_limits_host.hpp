// The dynamic-limits report and the state sampler on the host, plain C++ (no HIP): the rules of csrc/traj_limits.hip - sampling,
// bracketing, refinement, tie rules - restated without a device, behind isdf_traj_limits_host / isdf_traj_sample_host.
//   tl_locate       Trajectory::locatePieceIdx (src/utils/include/utils/trajectory.hpp:545-563)
//   tl_piece_eval   Piece::getPos_Vel_Acc_Jerk (:105-149): running powers of t, ascending-power walk
//   tl_flat         FlatnessMap::optimizated_forward (src/utils/include/utils/flatness.hpp:88-148) and the thrust of forward
//                   (:203-206) with psi = dpsi = 0
//   tilt            acos(1 - 2 (q1^2 + q2^2)) (back_end_optimizer.hpp:505-508)
// What the reference has of this - Trajectory::getMaxVelRate / getMaxAccRate / checkMaxVelRate / checkMaxAccRate
// (trajectory.hpp:253-390, :631-680) - finds the roots of a polynomial and so covers speed and acceleration only; the body rate,
// the tilt and the thrust are no polynomials, hence sampling and golden section for all six channels.
// The report is a lower bound of the true extremum that is never below a coarse sample; a peak narrower than two coarse
// intervals can be missed.
#pragma once
#include "../../include/isdf_accel.h"
#include <cmath>
#include <cstring>
#include <limits>

namespace isdf_host {

constexpr int TL_CH = ISDF_LIMITS_CHANNELS;
constexpr int TL_MAX_ITERS = 64;
constexpr double TL_GOLD = 0.6180339887498949;      // (sqrt(5) - 1) / 2
constexpr double TL_TOL_DEFAULT = 1.0 / 67108864.0;  // 2^-26

struct TLFlat { double mass, grav, dv, cp, veps, dh_over_m; };
inline TLFlat tl_flat_params(const isdf_config &cfg) {
    TLFlat P;
    P.mass = cfg.vehicle_mass; P.grav = cfg.grav_acc; P.dv = cfg.vert_drag; P.cp = cfg.paras_drag; P.veps = cfg.speed_eps;
    P.dh_over_m = cfg.horiz_drag / cfg.vehicle_mass;
    return P;
}
// the parameters in force
inline int tl_samples(const isdf_traj_limits_params *p, const isdf_config &cfg) {
    return (p && p->samples > 0) ? p->samples : 4 * (cfg.integral_intervs > 0 ? cfg.integral_intervs : 1);
}
inline double tl_tol(const isdf_traj_limits_params *p) { return (p && p->tol_t > 0.0) ? p->tol_t : TL_TOL_DEFAULT; }
// limit[ch] (NaN: not judged)
inline void tl_limits(const isdf_traj_limits_params *p, const isdf_config &cfg, double limit[TL_CH]) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    limit[ISDF_LIMIT_SPEED] = cfg.vmax; limit[ISDF_LIMIT_OMG] = cfg.omgmax; limit[ISDF_LIMIT_TILT] = cfg.thetamax;
    limit[ISDF_LIMIT_ACC] = p ? p->max_acc : nan;
    limit[ISDF_LIMIT_THRUST_MAX] = p ? p->max_thrust : nan;
    limit[ISDF_LIMIT_THRUST_MIN] = p ? p->min_thrust : nan;
}
// strictly beyond the limit (a NaN limit: never); constexpr: the retiming's pick kernel judges with the same text
constexpr bool tl_over(int ch, double value, double limit) { return ch == ISDF_LIMIT_THRUST_MIN ? value < limit : value > limit; }

inline int tl_check_traj(int N, const double *T, const double *coeffs) {
    if (N < 1 || !T || !coeffs) return ISDF_ERR_INVALID_ARG;
    for (int i = 0; i < N; i++) if (!(T[i] > 0.0) || !std::isfinite(T[i])) return ISDF_ERR_INVALID_ARG;
    return ISDF_OK;
}

inline int tl_locate(const double *T, int N, double &t) {
    int idx = 0;
    double dur = 0.0;
    for (; idx < N && t > (dur = T[idx]); idx++) t -= dur;
    if (idx == N) { idx--; t += T[idx]; }
    return idx;
}
// C: 6N x 3 column-major
inline void tl_piece_eval(const double *C, int N, int piece, double t, double pos[3], double vel[3], double acc[3], double jer[3]) {
    const int ld = 6 * N;
    const double *c = C + 6 * piece;
    for (int a = 0; a < 3; a++) pos[a] = vel[a] = acc[a] = jer[a] = 0.0;
    double pos_tn = 1.0, vel_tn = 1.0, acc_tn = 1.0, jer_tn = 1.0;
    int vel_n = 1, acc_m = 1, acc_n = 2, jl = 1, jm = 2, jn = 3;
    for (int power = 0; power <= 5; power++) {
        for (int a = 0; a < 3; a++) pos[a] += pos_tn * c[a * ld + power];
        pos_tn *= t;
        if (power >= 1) { for (int a = 0; a < 3; a++) vel[a] += (vel_n * vel_tn) * c[a * ld + power]; vel_tn *= t; vel_n++; }
        if (power >= 2) { for (int a = 0; a < 3; a++) acc[a] += (acc_m * acc_n * acc_tn) * c[a * ld + power]; acc_tn *= t; acc_m++; acc_n++; }
        if (power >= 3) { for (int a = 0; a < 3; a++) jer[a] += (jl * jm * jn * jer_tn) * c[a * ld + power]; jer_tn *= t; jl++; jm++; jn++; }
    }
}
inline void tl_flat(const TLFlat &P, const double v[3], const double a[3], const double j[3], double quat[4], double omg[3], double &thr) {
    const double cp_term = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + P.veps);
    const double w_term = 1.0 + P.cp * cp_term;
    const double w0 = w_term * v[0], w1 = w_term * v[1], w2 = w_term * v[2];
    const double zu0 = a[0] + P.dh_over_m * w0, zu1 = a[1] + P.dh_over_m * w1, zu2 = a[2] + P.dh_over_m * w2 + P.grav;
    const double s0 = zu0 * zu0, s1 = zu1 * zu1, s2 = zu2 * zu2;
    const double zu_sqr_norm = s0 + s1 + s2, zu_norm = std::sqrt(zu_sqr_norm);
    const double z0 = zu0 / zu_norm, z1 = zu1 / zu_norm, z2 = zu2 / zu_norm;
    const double tilt_den = std::sqrt(2.0 * (1.0 + z2));
    quat[0] = 0.5 * tilt_den; quat[1] = -z1 / tilt_den; quat[2] = z0 / tilt_den; quat[3] = 0.0;
    const double ng_den = zu_sqr_norm * zu_norm;
    const double ng00 = (s1 + s2) / ng_den, ng01 = -(zu0 * zu1) / ng_den, ng02 = -(zu0 * zu2) / ng_den;
    const double ng11 = (s0 + s2) / ng_den, ng12 = -(zu1 * zu2) / ng_den, ng22 = (s0 + s1) / ng_den;
    const double v_dot_a = v[0] * a[0] + v[1] * a[1] + v[2] * a[2];
    const double dw_term = P.cp * v_dot_a / cp_term;
    const double dzt0 = j[0] + P.dh_over_m * (w_term * a[0] + dw_term * v[0]);
    const double dzt1 = j[1] + P.dh_over_m * (w_term * a[1] + dw_term * v[1]);
    const double dzt2 = j[2] + P.dh_over_m * (w_term * a[2] + dw_term * v[2]);
    const double dz0 = ng00 * dzt0 + ng01 * dzt1 + ng02 * dzt2;
    const double dz1 = ng01 * dzt0 + ng11 * dzt1 + ng12 * dzt2;
    const double dz2 = ng02 * dzt0 + ng12 * dzt1 + ng22 * dzt2;
    const double omg_den = z2 + 1.0, omg_term = dz2 / omg_den;
    omg[0] = -dz1 + z1 * omg_term; omg[1] = dz0 - z0 * omg_term; omg[2] = (z1 * dz0 - z0 * dz1) / omg_den;
    const double f0 = P.mass * a[0] + P.dv * w0, f1 = P.mass * a[1] + P.dv * w1, f2 = P.mass * (a[2] + P.grav) + P.dv * w2;
    thr = z0 * f0 + z1 * f1 + z2 * f2;
}
// one row of the sampler at global time t
inline void tl_sample_row(const TLFlat &P, int N, const double *T, const double *C, double t, double row[ISDF_TRAJ_SAMPLE_ROW]) {
    const int piece = tl_locate(T, N, t);
    tl_piece_eval(C, N, piece, t, row, row + 3, row + 6, row + 9);
    tl_flat(P, row + 3, row + 6, row + 9, row + 12, row + 16, row[19]);
}

// the six channels in the form that is maximised: squared norms, tilt, thrust, -thrust
inline void tl_channels(const TLFlat &P, int N, const double *C, int piece, double s, double f[TL_CH]) {
    double pos[3], v[3], a[3], j[3], q[4], w[3], thr;
    tl_piece_eval(C, N, piece, s, pos, v, a, j);
    tl_flat(P, v, a, j, q, w, thr);
    f[0] = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
    f[1] = a[0] * a[0] + a[1] * a[1] + a[2] * a[2];
    f[2] = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    f[3] = std::acos(1.0 - 2.0 * (q[1] * q[1] + q[2] * q[2]));
    f[4] = thr; f[5] = -thr;
}
inline double tl_channel(const TLFlat &P, int N, const double *C, int piece, double s, int ch) {
    double f[TL_CH];
    tl_channels(P, N, C, piece, s, f);
    return f[ch];
}
// what is reported of a maximised value
inline double tl_report(int ch, double f) { return ch <= ISDF_LIMIT_OMG ? std::sqrt(f) : (ch == ISDF_LIMIT_THRUST_MIN ? -f : f); }
// local time of coarse sample j of S: both ends exact
inline double tl_sample_time(double T, int S, int j) { return j <= 0 ? 0.0 : (j >= S ? T : (double)j * T / (double)S); }

struct TLBest { double v, t; };
// larger value, then smaller time
inline void tl_take(TLBest &b, double v, double t) { if (v > b.v || (v == b.v && t < b.t)) { b.v = v; b.t = t; } }

// golden section for the maximum of channel ch on [a, b]: every evaluation is offered to `best`
inline void tl_refine(const TLFlat &P, int N, const double *C, int piece, int ch, double a, double b, double stop, TLBest &best) {
    double x1 = b - TL_GOLD * (b - a), x2 = a + TL_GOLD * (b - a);
    double f1 = tl_channel(P, N, C, piece, x1, ch), f2 = tl_channel(P, N, C, piece, x2, ch);
    tl_take(best, f1, x1); tl_take(best, f2, x2);
    for (int it = 0; it < TL_MAX_ITERS && !(b - a < stop); it++) {
        if (f1 >= f2) { b = x2; x2 = x1; f2 = f1; x1 = b - TL_GOLD * (b - a); f1 = tl_channel(P, N, C, piece, x1, ch); tl_take(best, f1, x1); }
        else          { a = x1; x1 = x2; f1 = f2; x2 = a + TL_GOLD * (b - a); f2 = tl_channel(P, N, C, piece, x2, ch); tl_take(best, f2, x2); }
    }
}

// one piece: best[ch] = the maximised value and its LOCAL time
inline void tl_piece(const TLFlat &P, int N, const double *T, const double *C, int piece, int S, double tol_t, TLBest best[TL_CH]) {
    const double Ti = T[piece], stop = tol_t * Ti;
    for (int ch = 0; ch < TL_CH; ch++) { best[ch].v = -std::numeric_limits<double>::infinity(); best[ch].t = 0.0; }
    double fm[TL_CH], f0[TL_CH], fp[TL_CH];          // the window: samples j - 1, j, j + 1
    tl_channels(P, N, C, piece, 0.0, f0);
    for (int ch = 0; ch < TL_CH; ch++) fm[ch] = f0[ch];
    for (int j = 0; j <= S; j++) {
        const double sj = tl_sample_time(Ti, S, j);
        if (j < S) tl_channels(P, N, C, piece, tl_sample_time(Ti, S, j + 1), fp);
        const double lo = tl_sample_time(Ti, S, j - 1), hi = tl_sample_time(Ti, S, j + 1);
        for (int ch = 0; ch < TL_CH; ch++) {
            tl_take(best[ch], f0[ch], sj);
            const bool start = j == 0 || j == S || (f0[ch] >= fm[ch] && f0[ch] >= fp[ch]);
            if (start) tl_refine(P, N, C, piece, ch, lo, hi, stop, best[ch]);
        }
        for (int ch = 0; ch < TL_CH; ch++) { fm[ch] = f0[ch]; f0[ch] = fp[ch]; }
    }
}

// the whole report.  piece_out: N x 12 or null
inline int tl_report_traj(const isdf_config &cfg, int N, const double *T, const double *C, const isdf_traj_limits_params *p,
                          isdf_traj_limits_info *info, double *piece_out) {
    { const int rc = tl_check_traj(N, T, C); if (rc) return rc; }
    const TLFlat P = tl_flat_params(cfg);
    const int S = tl_samples(p, cfg);
    const double tol_t = tl_tol(p);
    double limit[TL_CH], bv[TL_CH], bt[TL_CH];
    int bp[TL_CH], over[TL_CH];
    tl_limits(p, cfg, limit);
    for (int ch = 0; ch < TL_CH; ch++) { bv[ch] = 0.0; bt[ch] = 0.0; bp[ch] = -1; over[ch] = 0; }
    double t0 = 0.0;                                 // start of the piece: the durations before it, summed in order
    for (int i = 0; i < N; i++) {
        TLBest best[TL_CH];
        tl_piece(P, N, T, C, i, S, tol_t, best);
        for (int ch = 0; ch < TL_CH; ch++) {
            const double v = tl_report(ch, best[ch].v), t = t0 + best[ch].t;
            if (piece_out) { piece_out[12 * (size_t)i + 2 * ch] = v; piece_out[12 * (size_t)i + 2 * ch + 1] = t; }
            // larger maximised value, then smaller time, then the earlier piece
            const double key = ch == ISDF_LIMIT_THRUST_MIN ? -v : v, cur = ch == ISDF_LIMIT_THRUST_MIN ? -bv[ch] : bv[ch];
            if (bp[ch] < 0 || key > cur || (key == cur && t < bt[ch])) { bv[ch] = v; bt[ch] = t; bp[ch] = i; }
            if (tl_over(ch, v, limit[ch])) over[ch]++;
        }
        t0 += T[i];
    }
    if (info) {
        std::memset(info, 0, sizeof(*info));
        for (int ch = 0; ch < TL_CH; ch++) {
            info->value[ch] = bv[ch]; info->time[ch] = bt[ch]; info->piece[ch] = bp[ch]; info->limit[ch] = limit[ch];
            info->n_pieces_over[ch] = over[ch];
            if (!std::isnan(limit[ch])) {
                info->judged |= 1 << ch;
                if (!tl_over(ch, bv[ch], limit[ch])) info->feasible |= 1 << ch;
            }
        }
        info->samples = S; info->tol_t = tol_t;
    }
    return ISDF_OK;
}

inline int tl_sample_traj(const isdf_config &cfg, int N, const double *T, const double *C, long long n, const double *t, double *rows) {
    { const int rc = tl_check_traj(N, T, C); if (rc) return rc; }
    if (n < 0 || (n > 0 && (!t || !rows))) return ISDF_ERR_INVALID_ARG;
    const TLFlat P = tl_flat_params(cfg);
    for (long long k = 0; k < n; k++) tl_sample_row(P, N, T, C, t[k], rows + ISDF_TRAJ_SAMPLE_ROW * k);
    return ISDF_OK;
}

}  // namespace isdf_host
