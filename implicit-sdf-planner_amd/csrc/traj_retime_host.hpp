// Uniform retiming of a trajectory to its dynamic limits: the rules of include/isdf_accel.h (scaling, ladder, pick, rounds) in
// plain C++ (no HIP).  The rule functions are __host__ __device__ where a HIP compiler reads this file, so csrc/traj_retime.hip's
// kernels run the very same text; tr_retime_traj composes them over traj_limits_host.hpp behind isdf_traj_retime_host.
// The reference has no counterpart (trajectory.hpp:253-390, :631-680 only report).
#pragma once
#include "traj_limits_host.hpp"
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define ISDF_TR_HD __host__ __device__
#else
#define ISDF_TR_HD
#endif

namespace isdf_host {

constexpr int TR_LADDER_MIN = 2, TR_LADDER_MAX = 64, TR_ROUNDS_MIN = 1, TR_ROUNDS_MAX = 4;

// every operation below is rounded on its own: no contraction on either side
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

// candidate i of L on [a, b]: both ends exact, in between the product, then the quotient, then the sum
ISDF_TR_HD inline double tr_candidate(double a, double b, int L, int i) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (i <= 0) return a;
    if (i >= L - 1) return b;
    const double num = (b - a) * (double)i;
    const double step = num / (double)(L - 1);
    return a + step;
}
// element r of the 19 N doubles [T | 6N x 3 column-major coefficients] of a trajectory, scaled by s
ISDF_TR_HD inline double tr_scale_elem(int N, long long r, double x, double s) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (r < N) return s * x;
    const int k = (int)(((r - N) % (6LL * N)) % 6);
    double p = 1.0;
    for (int q = 0; q < k; q++) p = p * s;
    return x / p;
}
// feas: bit i = F(s_i), i < L.  Returns i* in 0..L (L: the top candidate fails); *nonmonotone: a feasible one below an infeasible one
ISDF_TR_HD inline int tr_pick(unsigned long long feas, int L, int *nonmonotone) {
    const unsigned long long all = L >= 64 ? ~0ull : ((1ull << L) - 1ull);
    const unsigned long long bad = ~feas & all;
    int hi = -1;                                    // the highest infeasible candidate
    for (int i = 0; i < L; i++) if ((bad >> i) & 1ull) hi = i;
    if (nonmonotone) *nonmonotone = (hi > 0 && (feas & ((1ull << hi) - 1ull)) != 0ull) ? 1 : 0;
    return hi + 1;
}

struct TRState {
    double a, b;        // the bracket of the round to come (of the deciding round once done)
    int status, done;
    int res, below;     // candidate indices of the result and of scale_below (-1: none) in the bracket [a, b]
    int nonmono, rounds;
};
ISDF_TR_HD inline void tr_begin(TRState &s, double s_lo, double s_hi) {
    s.a = s_lo; s.b = s_hi; s.status = ISDF_RETIME_OK; s.done = 0; s.res = 0; s.below = -1; s.nonmono = 0; s.rounds = 0;
}
// one round's verdicts -> the state; R rounds in all.  After the last round the bracket is the one res / below index.
ISDF_TR_HD inline void tr_advance(TRState &s, unsigned long long feas, int L, int round, int R) {
    if (s.done) return;
    int nm = 0;
    int istar = tr_pick(feas, L, &nm);
    s.nonmono |= nm;
    s.rounds = round + 1;
    if (round == 0 && istar == L) {                 // F(s_hi) fails
        s.status = ISDF_RETIME_NOT_REACHABLE; s.done = 1; s.res = L - 1; s.below = -1;
        const unsigned long long all = L >= 64 ? ~0ull : ((1ull << L) - 1ull);
        const unsigned long long bad = ~feas & all;
        for (int i = 0; i < L - 1; i++) if ((bad >> i) & 1ull) s.below = i;
        return;
    }
    if (round == 0 && istar == 0) { s.status = ISDF_RETIME_AT_LOWER; s.done = 1; s.res = 0; s.below = -1; return; }
    // a later round's ends were evaluated before, with the same bytes: a fails and b holds, so 1 <= i* <= L - 1
    if (istar < 1) istar = 1;
    if (istar > L - 1) istar = L - 1;
    s.res = istar; s.below = istar - 1;
    if (round + 1 < R) {
        const double na = tr_candidate(s.a, s.b, L, istar - 1), nb = tr_candidate(s.a, s.b, L, istar);
        s.a = na; s.b = nb;
    } else {
        s.done = 1;
    }
}

inline int tr_check_params(const isdf_traj_retime_params *p) {
    if (!p) return ISDF_OK;
    if (!(p->s_lo > 0.0) || !std::isfinite(p->s_lo) || !std::isfinite(p->s_hi) || !(p->s_hi > p->s_lo)) return ISDF_ERR_INVALID_ARG;
    if (p->ladder < TR_LADDER_MIN || p->ladder > TR_LADDER_MAX || p->rounds < TR_ROUNDS_MIN || p->rounds > TR_ROUNDS_MAX) return ISDF_ERR_INVALID_ARG;
    return ISDF_OK;
}
inline void tr_params_default(isdf_traj_retime_params *p) {
    std::memset(p, 0, sizeof(*p));
    p->s_lo = 1.0; p->s_hi = 8.0; p->ladder = 32; p->rounds = 3; p->check = 0;
    p->limits.samples = 0; p->limits.tol_t = TL_TOL_DEFAULT;
    p->limits.max_acc = p->limits.max_thrust = p->limits.min_thrust = std::numeric_limits<double>::quiet_NaN();
}

inline int tr_scale_traj(int N, const double *T, const double *C, double s, double *T_out, double *C_out) {
    { const int rc = tl_check_traj(N, T, C); if (rc) return rc; }
    if (!(s > 0.0) || !std::isfinite(s) || !T_out || !C_out) return ISDF_ERR_INVALID_ARG;
    for (int r = 0; r < N; r++) T_out[r] = tr_scale_elem(N, r, T[r], s);
    for (long long e = 0; e < 18LL * N; e++) C_out[e] = tr_scale_elem(N, N + e, C[e], s);
    return ISDF_OK;
}
// the durations summed in order
inline double tr_duration(int N, const double *T) {
    double d = 0.0;
    for (int i = 0; i < N; i++) d += T[i];
    return d;
}

// the whole search on the host
inline int tr_retime_traj(const isdf_config &cfg, int N, const double *T, const double *C, const isdf_traj_retime_params *params,
                          double *T_out, double *C_out, isdf_traj_retime_info *info) {
    { const int rc = tl_check_traj(N, T, C); if (rc) return rc; }
    { const int rc = tr_check_params(params); if (rc) return rc; }
    if (!T_out || !C_out) return ISDF_ERR_INVALID_ARG;
    isdf_traj_retime_params P;
    if (params) P = *params; else tr_params_default(&P);
    const int L = P.ladder, R = P.rounds;
    std::vector<double> sT((size_t)N), sC((size_t)18 * N);
    std::vector<isdf_traj_limits_info> rep((size_t)L);
    TRState st;
    tr_begin(st, P.s_lo, P.s_hi);
    int evaluated = 0;
    for (int round = 0; round < R && !st.done; round++) {
        unsigned long long feas = 0ull;
        for (int i = 0; i < L; i++) {
            const double s = tr_candidate(st.a, st.b, L, i);
            tr_scale_traj(N, T, C, s, sT.data(), sC.data());
            tl_report_traj(cfg, N, sT.data(), sC.data(), &P.limits, &rep[(size_t)i], nullptr);
            if (rep[(size_t)i].feasible == rep[(size_t)i].judged) feas |= 1ull << i;
        }
        evaluated += L;
        tr_advance(st, feas, L, round, R);
    }
    const double scale = tr_candidate(st.a, st.b, L, st.res);
    tr_scale_traj(N, T, C, scale, T_out, C_out);
    if (info) {
        std::memset(info, 0, sizeof(*info));
        info->scale = scale;
        info->scale_below = st.below >= 0 ? tr_candidate(st.a, st.b, L, st.below) : std::numeric_limits<double>::quiet_NaN();
        info->status = st.status; info->rounds = st.rounds; info->candidates = evaluated; info->nonmonotone = st.nonmono;
        if (st.below >= 0) info->binding = rep[(size_t)st.below].judged & ~rep[(size_t)st.below].feasible;
        info->duration_in = tr_duration(N, T); info->duration_out = tr_duration(N, T_out);
        info->limits = rep[(size_t)st.res];
    }
    return ISDF_OK;
}

}  // namespace isdf_host
