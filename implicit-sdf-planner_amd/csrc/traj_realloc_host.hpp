// Re-allocation of piece durations to the dynamic limits: the rules of include/isdf_accel.h (piece factor, update, rounds and
// status) in plain C++ (no HIP).  The rule functions are __host__ __device__ where a HIP compiler reads this file, so
// csrc/traj_realloc.hip's kernels run the very same text; ra_realloc_traj composes them over traj_limits_host.hpp and the host loops
// of minco_pcr.hpp (one loop per parallel round, as tests/native/minco_pcr_shim.cpp walks them) behind isdf_traj_realloc_host.
// The reference has no counterpart: soft penalties at K + 1 samples per piece (back_end_optimizer.hpp:453-536) and a Trajectory
// class that only reports (trajectory.hpp:253-390, :631-680).
#pragma once
#include "traj_limits_host.hpp"
#include "minco_pcr.hpp"
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define ISDF_RA_HD __host__ __device__
#else
#define ISDF_RA_HD
#endif

namespace isdf_host {

constexpr int RA_ROUNDS_MIN = 1, RA_ROUNDS_MAX = ISDF_TRAJ_REALLOC_MAX_ROUNDS;

// every operation of the rule is rounded on its own: no contraction on either side
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

ISDF_RA_HD inline bool ra_finite(double x) { return x - x == 0.0; }      // neither NaN nor infinite

// the ratio of a channel that is over its limit
ISDF_RA_HD inline double ra_rho(int ch, double value, double limit, double f_max) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (ch == ISDF_LIMIT_ACC) return ::sqrt(value / limit);
    if (ch == ISDF_LIMIT_THRUST_MIN) return value > 0.0 ? limit / value : f_max;
    return value / limit;
}
// row: the piece's 12 doubles of the report's piece_out ([2 ch] = value); limit[ch] NaN: not judged.  *over: the channels that are
// judged and strictly beyond their limit.  Returns f_i: exactly 1 when *over == 0, else within [1, f_max]
ISDF_RA_HD inline double ra_piece_factor(const double *row, const double *limit, double headroom, double f_max, int *over) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    int mask = 0;
    bool bad = false;
    double m = 0.0;
    for (int ch = 0; ch < TL_CH; ch++) {
        const double lim = limit[ch], v = row[2 * ch];
        if (lim != lim || !tl_over(ch, v, lim)) continue;
        mask |= 1 << ch;
        const double r = ra_rho(ch, v, lim, f_max);
        if (!ra_finite(r)) bad = true;
        else if (r > m) m = r;
    }
    *over = mask;
    if (!mask) return 1.0;
    if (bad) return f_max;
    double f = (1.0 + headroom) * m;
    if (!(f < f_max)) f = f_max;
    if (!(f > 1.0)) f = 1.0;
    return f;
}
// T_(k+1),i: one product
ISDF_RA_HD inline double ra_update(double T, double f) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return T * f;
}

struct RAState { int done, status, rounds, binding; };
ISDF_RA_HD inline void ra_begin(RAState &s) { s.done = 0; s.status = ISDF_REALLOC_NOT_REACHED; s.rounds = 0; s.binding = 0; }
// iterate k of 0..R was evaluated; over: the union of its pieces' masks.  True: the durations are to be updated for iterate k + 1
ISDF_RA_HD inline bool ra_advance(RAState &s, int over, int k, int R) {
    if (s.done) return false;
    if (!over) { s.done = 1; s.status = k == 0 ? ISDF_REALLOC_ALREADY : ISDF_REALLOC_OK; s.rounds = k; return false; }
    s.binding |= over;
    if (k >= R) { s.done = 1; s.status = ISDF_REALLOC_NOT_REACHED; s.rounds = R; return false; }
    return true;
}

// coordinate d of waypoint k (0: the head's position, N: the tail's)
ISDF_RA_HD inline double ra_waypoint(int N, const double *head, const double *tail, const double *Q, int k, int d) {
    if (k <= 0) return head[d];
    if (k >= N) return tail[d];
    return Q[3 * (size_t)(k - 1) + d];
}

inline int ra_check_params(const isdf_traj_realloc_params *p) {
    if (!p) return ISDF_OK;
    if (p->rounds < RA_ROUNDS_MIN || p->rounds > RA_ROUNDS_MAX) return ISDF_ERR_INVALID_ARG;
    if (!(p->headroom >= 0.0) || !std::isfinite(p->headroom) || !(p->f_max > 1.0) || !std::isfinite(p->f_max)) return ISDF_ERR_INVALID_ARG;
    return ISDF_OK;
}
inline void ra_params_default(isdf_traj_realloc_params *p) {
    std::memset(p, 0, sizeof(*p));
    p->rounds = 8; p->check = 0; p->headroom = 0.02; p->f_max = 2.0;
    p->limits.samples = 0; p->limits.tol_t = TL_TOL_DEFAULT;
    p->limits.max_acc = p->limits.max_thrust = p->limits.min_thrust = std::numeric_limits<double>::quiet_NaN();
}
inline bool ra_overlap(const void *a, size_t na, const void *b, size_t nb) {
    if (!a || !b || !na || !nb) return false;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}
// an output (n_out doubles) against the four input arrays of B trajectories of N pieces
inline bool ra_overlaps_inputs(const double *out, size_t n_out, long long B, int N, const double *head, const double *tail, const double *Q, const double *T) {
    const size_t d = sizeof(double), b = (size_t)B;
    return ra_overlap(out, n_out * d, head, 9 * b * d) || ra_overlap(out, n_out * d, tail, 9 * b * d) ||
           ra_overlap(out, n_out * d, Q, 3 * b * (size_t)(N - 1) * d) || ra_overlap(out, n_out * d, T, b * (size_t)N * d);
}
// what every form asks of its arrays (durations aside)
inline int ra_check_args(long long B, int N, const double *head, const double *tail, const double *Q, const double *T, const double *T_out, const double *C_out) {
    if (B < 1 || N < 1 || !head || !tail || !T || (N > 1 && !Q) || !T_out || !C_out) return ISDF_ERR_INVALID_ARG;
    return ISDF_OK;
}
inline int ra_check_durations(long long n, const double *T) {
    for (long long i = 0; i < n; i++) if (!(T[i] > 0.0) || !std::isfinite(T[i])) return ISDF_ERR_INVALID_ARG;
    return ISDF_OK;
}
// the durations summed in order
inline double ra_duration(int N, const double *T) {
    double d = 0.0;
    for (int i = 0; i < N; i++) d += T[i];
    return d;
}

// C(T): junction rows, PCR rounds one loop each, u = D^-1 r, hermite per piece.  C: 6N x 3 column-major.  No argument checks
inline void ra_minco_solve(int N, const double *head, const double *tail, const double *Q, const double *T, double *C) {
    using namespace mpcr;
    const int n = N - 1;
    std::vector<double> h((size_t)N), u((size_t)6 * (N + 1), 0.0);      // u: [(N + 1)][axis][2] = (v, a)
    for (int i = 0; i < N; i++) h[(size_t)i] = 1.0 / T[i];
    for (int d = 0; d < 3; d++) {
        u[(size_t)2 * d] = head[3 + d]; u[(size_t)2 * d + 1] = head[6 + d];
        u[(size_t)6 * N + 2 * d] = tail[3 + d]; u[(size_t)6 * N + 2 * d + 1] = tail[6 + d];
    }
    if (n >= 1) {
        std::vector<Row> rows((size_t)n);
        std::vector<Norm> norm((size_t)n);
        for (int j = 1; j <= n; j++) {
            Row &w = rows[(size_t)j - 1];
            const double hl = h[(size_t)j - 1], hr = h[(size_t)j];
            junction_blocks(hl, hr, w.L, w.D, w.U);
            double dpl[3], dpr[3];
            for (int d = 0; d < 3; d++) {
                const double pj = ra_waypoint(N, head, tail, Q, j, d);
                dpl[d] = pj - ra_waypoint(N, head, tail, Q, j - 1, d);
                dpr[d] = ra_waypoint(N, head, tail, Q, j + 1, d) - pj;
            }
            junction_rhs(hl, hr, dpl, dpr, w.r);
            if (j == 1) {
                double va[3][2];
                for (int d = 0; d < 3; d++) { va[d][0] = u[(size_t)2 * d]; va[d][1] = u[(size_t)2 * d + 1]; }
                rhs_minus(w.L, va, w.r);
                w.L = {0, 0, 0, 0};
            }
            if (j == n) {
                double va[3][2];
                for (int d = 0; d < 3; d++) { va[d][0] = u[(size_t)6 * N + 2 * d]; va[d][1] = u[(size_t)6 * N + 2 * d + 1]; }
                rhs_minus(w.U, va, w.r);
                w.U = {0, 0, 0, 0};
            }
        }
        for (int s = 1; s < n; s *= 2) {
            for (int j = 0; j < n; j++) norm[(size_t)j] = pcr_normalise(rows[(size_t)j]);
            for (int j = 0; j < n; j++) pcr_combine(rows[(size_t)j], j - s >= 0 ? &norm[(size_t)(j - s)] : nullptr, j + s < n ? &norm[(size_t)(j + s)] : nullptr);
        }
        for (int j = 1; j <= n; j++) {
            double x[3][2];
            pcr_finish(rows[(size_t)j - 1], x);
            for (int d = 0; d < 3; d++) { u[(size_t)6 * j + 2 * d] = x[d][0]; u[(size_t)6 * j + 2 * d + 1] = x[d][1]; }
        }
    }
    for (int k = 0; k < N; k++) for (int d = 0; d < 3; d++) {
        double c[6];
        hermite(T[k], h[(size_t)k], ra_waypoint(N, head, tail, Q, k, d), u[(size_t)6 * k + 2 * d], u[(size_t)6 * k + 2 * d + 1],
                ra_waypoint(N, head, tail, Q, k + 1, d), u[(size_t)6 * (k + 1) + 2 * d], u[(size_t)6 * (k + 1) + 2 * d + 1], c);
        for (int q = 0; q < 6; q++) C[(size_t)d * 6 * N + 6 * (size_t)k + q] = c[q];
    }
}
inline int ra_minco_traj(int N, const double *head, const double *tail, const double *Q, const double *T, double *C_out) {
    if (N < 1 || !head || !tail || !T || (N > 1 && !Q) || !C_out) return ISDF_ERR_INVALID_ARG;
    { const int rc = ra_check_durations(N, T); if (rc) return rc; }
    ra_minco_solve(N, head, tail, Q, T, C_out);
    return ISDF_OK;
}

// what the tests look at of the host loop, iterate by iterate
struct RATrace {
    int evals = 0;                                  // iterates evaluated
    double margin[RA_ROUNDS_MAX + 1];               // per iterate: the smallest |value - limit| / |limit| over pieces and judged channels
    std::vector<int> ever_over;                     // per piece: the union of its masks over the iterates
};

// the whole loop on the host
inline int ra_realloc_traj(const isdf_config &cfg, int N, const double *head, const double *tail, const double *Q, const double *T,
                           const isdf_traj_realloc_params *params, double *T_out, double *C_out, isdf_traj_realloc_info *info, RATrace *trace = nullptr) {
    { const int rc = ra_check_args(1, N, head, tail, Q, T, T_out, C_out); if (rc) return rc; }
    { const int rc = ra_check_durations(N, T); if (rc) return rc; }
    { const int rc = ra_check_params(params); if (rc) return rc; }
    if (ra_overlaps_inputs(T_out, (size_t)N, 1, N, head, tail, Q, T) || ra_overlaps_inputs(C_out, (size_t)18 * N, 1, N, head, tail, Q, T) ||
        ra_overlap(T_out, (size_t)N * sizeof(double), C_out, (size_t)18 * N * sizeof(double)))
        return ISDF_ERR_INVALID_ARG;
    isdf_traj_realloc_params P;
    if (params) P = *params; else ra_params_default(&P);
    const int R = P.rounds;
    double limit[TL_CH];
    tl_limits(&P.limits, cfg, limit);
    std::vector<double> piece((size_t)12 * N), f((size_t)N);
    isdf_traj_limits_info rep;
    RAState st;
    ra_begin(st);
    if (trace) { trace->evals = 0; trace->ever_over.assign((size_t)N, 0); }
    for (int i = 0; i < N; i++) T_out[i] = T[i];
    for (int k = 0; k <= R; k++) {
        ra_minco_solve(N, head, tail, Q, T_out, C_out);
        tl_report_traj(cfg, N, T_out, C_out, &P.limits, &rep, piece.data());
        int over = 0;
        double margin = std::numeric_limits<double>::infinity();
        for (int i = 0; i < N; i++) {
            int m = 0;
            f[(size_t)i] = ra_piece_factor(&piece[(size_t)12 * i], limit, P.headroom, P.f_max, &m);
            over |= m;
            if (trace) {
                trace->ever_over[(size_t)i] |= m;
                for (int ch = 0; ch < TL_CH; ch++)
                    if (!std::isnan(limit[ch])) margin = std::fmin(margin, std::fabs(piece[(size_t)12 * i + 2 * ch] - limit[ch]) / std::fabs(limit[ch]));
            }
        }
        if (trace) { trace->margin[k] = margin; trace->evals = k + 1; }
        if (!ra_advance(st, over, k, R)) break;
        for (int i = 0; i < N; i++) T_out[i] = ra_update(T_out[i], f[(size_t)i]);
    }
    if (info) {
        std::memset(info, 0, sizeof(*info));
        info->status = st.status; info->rounds = st.rounds; info->binding = st.binding;
        double mf = 0.0;
        for (int i = 0; i < N; i++) {
            if (T_out[i] != T[i]) info->pieces_changed++;
            mf = std::fmax(mf, T_out[i] / T[i]);
        }
        info->max_factor = mf;
        info->duration_in = ra_duration(N, T); info->duration_out = ra_duration(N, T_out);
        info->limits = rep;
    }
    return ISDF_OK;
}

}  // namespace isdf_host
