// The view selection (view_select.hip), free of HIP so that a plain C++ program can run it under a sanitizer: the greedy
// coverage selection of k views by their joint gain.  Nothing of the ray, the walk or the stop rule is stated here: a view's set is built
// through view_gain_host.hpp's vg_ray, with a hook that fills a bit vector per view.
//
// The definition, integers only.  For a view j whose view-gain row has status 0, S_j is the view gain's set and U_j = {v in S_j : K[v] = 0}
// (|U_j| is the row's gain); a view of status 1 has no set and is never picked.  C_0 is empty.  Round r = 0 .. k_select - 1: m_j =
// |U_j \ C_r| for every scored view not yet picked; j* = the lowest index among the largest m_j.  If no such view is left or m_j* <
// min_gain the selection ends with n_selected = r; otherwise round r picks j* and C_{r+1} = C_r | U_j*.
//   select row r   {view, marginal, cumulative = |C_{r+1}|, overlap = gain_view - marginal}; rounds that did not happen: {-1, 0, 0, 0}
//   round[j]       the round in which view j was picked, or -1
//   claimed        K | C_final, K's layout
#pragma once
#include "view_gain_host.hpp"
#include <vector>

namespace isdf {

constexpr int VS_ROW = 4;                       // int64 per round
constexpr long long VS_MAX_VIEWS = 1ll << 24;

// The selection's integer key of a view that may be picked: larger is better - the larger marginal, then the lower index.  j < 2^24 and a
// marginal is at most the voxel count, below 2^36, so the key is below 2^61 and 0 is "none".
MU_HD unsigned long long vs_key(long long m, long long j) { return ((unsigned long long)(m + 1) << 24) | (unsigned long long)(VS_MAX_VIEWS - 1 - j); }
MU_HD long long vs_key_view(unsigned long long key) { return VS_MAX_VIEWS - 1 - (long long)(key & (unsigned long long)(VS_MAX_VIEWS - 1)); }
MU_HD long long vs_key_marginal(unsigned long long key) { return (long long)(key >> 24) - 1; }

MU_HD int vs_popcount(uint32_t v) {
    v = v - ((v >> 1) & 0x55555555u);
    v = (v & 0x33333333u) + ((v >> 2) & 0x33333333u);
    return (int)((((v + (v >> 4)) & 0x0F0F0F0Fu) * 0x01010101u) >> 24);
}

// what the info says beside the rows
struct VsCounts { long long n_scored = 0, n_selected = 0, gain_selected = 0, gain_solo_sum = 0, best_single_gain = 0, list_words = 0; };

// the counts the rows alone give (the device form takes the rest from its record)
inline void vs_counts_of_rows(const int64_t *rows, long long n_views, VsCounts &N) {
    const VgBest B = vg_best(rows, n_views);
    N.n_scored = B.n_scored; N.best_single_gain = B.best_gain;
}

// the sets: rows and round are written, U[j] is empty for a view that is not scored; N.list_words and the counts of the rows
inline void vs_sets_host(const uint32_t *bits, const uint8_t *occ, const MapGeom &M, const DcRays &base, const double *poses, long long n_views, int64_t *rows, int64_t *round,
                         std::vector<std::vector<uint32_t>> &U, VsCounts &N) {
    const long long n_words = mk_words((long long)M.dims[0] * M.dims[1] * M.dims[2]);
    const std::vector<uint16_t> zero((size_t)base.width * base.height, 0);
    N = VsCounts();
    U.assign((size_t)n_views, std::vector<uint32_t>());
    for (long long j = 0; j < n_views; j++) {
        int64_t *const row = rows + VG_ROW * j;
        for (int w = 0; w < VG_ROW; w++) row[w] = 0;
        round[j] = -1;
        VgView V;
        vg_view_setup(base, M, poses + 12 * j, V);
        if (!V.ok) { row[0] = VG_POSE_OUTSIDE; continue; }
        std::vector<uint32_t> &u = U[(size_t)j];
        u.assign((size_t)n_words, 0u);
        VgCounts C;
        auto visit = [&](size_t a) {
            const uint32_t b = 1u << (unsigned)(a & 31);
            if (bits[a >> 5] & b) return false;
            if (!(u[a >> 5] & b)) { u[a >> 5] |= b; C.gain++; }
            return true;
        };
        for (int iv = 0; iv < V.Q.nv; iv++)
            for (int iu = 0; iu < V.Q.nu; iu++)
                if (!vg_ray(V, M, zero.data(), occ, iu, iv, C.n_hits, C.steps_total, C.n_rays_unknown, visit)) C.n_skipped++;
        row[0] = VG_SCORED; row[1] = C.gain; row[2] = (int64_t)V.Q.nu * V.Q.nv; row[3] = C.n_skipped; row[4] = C.n_hits; row[5] = C.steps_total;
        row[6] = C.n_rays_unknown;
        for (long long w = 0; w < n_words; w++) N.list_words += u[(size_t)w] != 0u;
    }
    vs_counts_of_rows(rows, n_views, N);
}

inline void vs_rounds_begin(long long n_words, int k_select, int64_t *select, uint32_t *claimed) {
    for (long long w = 0; w < n_words; w++) claimed[w] = 0u;
    for (int r = 0; r < k_select; r++) {
        int64_t *const s = select + (long long)VS_ROW * r;
        s[0] = -1; s[1] = s[2] = s[3] = 0;
    }
}

// round r has picked view j with marginal m: its voxels are claimed, the counts and the outputs move on
inline void vs_round_take(int r, long long j, long long m, long long n_words, const std::vector<uint32_t> &u, const int64_t *rows, int64_t *select, int64_t *round,
                          uint32_t *claimed, VsCounts &N) {
    for (long long w = 0; w < n_words; w++) claimed[w] |= u[(size_t)w];
    N.gain_selected += m;
    N.gain_solo_sum += rows[VG_ROW * j + 1];
    N.n_selected = r + 1;
    round[j] = r;
    int64_t *const s = select + (long long)VS_ROW * r;
    s[0] = j; s[1] = m; s[2] = N.gain_selected; s[3] = rows[VG_ROW * j + 1] - m;
}

inline long long vs_marginal_host(const std::vector<uint32_t> &u, const uint32_t *claimed, long long n_words) {
    long long m = 0;
    for (long long w = 0; w < n_words; w++) m += vs_popcount(u[(size_t)w] & ~claimed[w]);
    return m;
}

// ---- host form: rows n_views x 8, select k_select x 4, round n_views, claimed n_words; all are written
inline void vs_select_host(const uint32_t *bits, const uint8_t *occ, const MapGeom &M, const DcRays &base, const double *poses, long long n_views, int k_select,
                           long long min_gain, int64_t *rows, int64_t *select, int64_t *round, uint32_t *claimed, VsCounts &N) {
    const long long n_words = mk_words((long long)M.dims[0] * M.dims[1] * M.dims[2]);
    std::vector<std::vector<uint32_t>> U;
    vs_sets_host(bits, occ, M, base, poses, n_views, rows, round, U, N);
    // the rounds
    vs_rounds_begin(n_words, k_select, select, claimed);
    for (int r = 0; r < k_select; r++) {
        unsigned long long top = 0;
        for (long long j = 0; j < n_views; j++) {
            if (rows[VG_ROW * j] != VG_SCORED || round[j] >= 0) continue;
            const unsigned long long key = vs_key(vs_marginal_host(U[(size_t)j], claimed, n_words), j);
            if (key > top) top = key;
        }
        if (top == 0 || vs_key_marginal(top) < min_gain) break;
        const long long j = vs_key_view(top);
        vs_round_take(r, j, vs_key_marginal(top), n_words, U[(size_t)j], rows, select, round, claimed, N);
    }
    for (long long w = 0; w < n_words; w++) claimed[w] |= bits[w];
}

// ---- the routed selection: greedy coverage by utility = marginal gain per travel cost.  cost: n_views doubles, each
// non-negative or +inf (the caller has checked that).  A view is eligible when it is scored, not picked so far, its cost finite and
// <= max_cost; round r: among the eligible views with m_j >= min_gain (min_gain >= 1), u_j = (double)m_j / (cost0 + c_j) - one addition,
// one division, fp64 - and j* the lowest index among the largest u_j.  util k_select x 2: {c_j*, u_j*}, {0, 0} for a round that did not
// happen.
struct VsRouteCounts { long long n_eligible = 0, n_unreachable = 0, n_over_budget = 0; double cost_selected = 0.0; };

MU_HD bool vs_cost_finite(double c) { return c - c == 0.0; }           // (not a NaN, not an infinity)
MU_HD bool vs_cost_eligible(double c, double max_cost) { return vs_cost_finite(c) && c <= max_cost; }
MU_HD double vs_utility(long long m, double cost0, double c) { return (double)m / (cost0 + c); }

inline void vs_route_counts(const int64_t *rows, const double *cost, long long n_views, double max_cost, VsRouteCounts &R) {
    R = VsRouteCounts();
    for (long long j = 0; j < n_views; j++) {
        if (rows[VG_ROW * j] != VG_SCORED) continue;
        if (!vs_cost_finite(cost[j])) R.n_unreachable++;
        else if (!(cost[j] <= max_cost)) R.n_over_budget++;
        else R.n_eligible++;
    }
}

inline void vs_select_routed_host(const uint32_t *bits, const uint8_t *occ, const MapGeom &M, const DcRays &base, const double *poses, long long n_views, int k_select,
                                  long long min_gain, const double *cost, double cost0, double max_cost, int64_t *rows, int64_t *select, int64_t *round,
                                  uint32_t *claimed, double *util, VsCounts &N, VsRouteCounts &R) {
    const long long n_words = mk_words((long long)M.dims[0] * M.dims[1] * M.dims[2]);
    std::vector<std::vector<uint32_t>> U;
    vs_sets_host(bits, occ, M, base, poses, n_views, rows, round, U, N);
    vs_route_counts(rows, cost, n_views, max_cost, R);
    vs_rounds_begin(n_words, k_select, select, claimed);
    for (int r = 0; r < k_select; r++) util[2 * r] = util[2 * r + 1] = 0.0;
    for (int r = 0; r < k_select; r++) {
        long long best = -1, best_m = 0;
        double best_u = 0.0;
        for (long long j = 0; j < n_views; j++) {
            if (rows[VG_ROW * j] != VG_SCORED || round[j] >= 0 || !vs_cost_eligible(cost[j], max_cost)) continue;
            const long long m = vs_marginal_host(U[(size_t)j], claimed, n_words);
            if (m < min_gain) continue;
            const double u = vs_utility(m, cost0, cost[j]);
            if (best < 0 || u > best_u) { best = j; best_m = m; best_u = u; }
        }
        if (best < 0) break;
        vs_round_take(r, best, best_m, n_words, U[(size_t)best], rows, select, round, claimed, N);
        util[2 * r] = cost[best]; util[2 * r + 1] = best_u;
        R.cost_selected += cost[best];
    }
    for (long long w = 0; w < n_words; w++) claimed[w] |= bits[w];
}

}  // namespace isdf
