// Stand-alone program for the sanitizers (tests/test_traj_limits_host.py builds it with -fsanitize=address,undefined and runs it):
// the dynamic-limits report and the state sampler of csrc/traj_limits_host.hpp on the shapes of the test case list - N = 1, 2, 3
// (durations 0.05, 12, 1), 130, exact hover, samples 1, 2, 5, 63, 64, 65, 257 -, the MID / TILTED / OMG, junction-tie and monotone inputs of
// the golden (traj_limits_cases.inc) with what they must report, the limit rules and the rejected arguments.
// Every array is allocated at its exact size, so a read or write past an end is seen.  Host code only.
#include "traj_limits_host.hpp"
#include <cstdio>
#include <cstdint>
#include <string>
#include <vector>
#include "traj_limits_cases.inc"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static double rndu(double a, double b) { return a + (b - a) * ((double)(rnd() >> 11) / 9007199254740992.0); }

static isdf_config config() {
    isdf_config c;
    std::memset(&c, 0, sizeof(c));
    c.integral_intervs = 4;
    c.vmax = 2.0; c.omgmax = 1.0; c.thetamax = 0.3;
    c.vehicle_mass = 0.61; c.grav_acc = 9.8; c.horiz_drag = 0.10; c.vert_drag = 0.10; c.paras_drag = 0.01; c.speed_eps = 1.0e-4;
    return c;
}
// N pieces with moderate random coefficients (column-major 6N x 3); hover: position only
static void traj(int N, const double *T, bool hover, std::vector<double> &C) {
    C.assign(18 * (size_t)N, 0.0);
    for (int a = 0; a < 3; a++)
        for (int i = 0; i < N; i++) {
            double *c = &C[(size_t)a * 6 * N + 6 * i];
            c[0] = 128.0;
            if (hover) continue;
            double scale = 1.0;
            for (int k = 1; k < 6; k++) { scale /= T[i] > 1.0 ? T[i] : 1.0; c[k] = rndu(-2.0, 2.0) * scale; }
        }
}
// the report twice (same bytes), never below a coarse sample, the trajectory's row the best of its pieces'
static int report(const isdf_config &cfg, int N, const double *T, const std::vector<double> &C, int samples, int &runs) {
    isdf_traj_limits_params p;
    std::memset(&p, 0, sizeof(p));
    p.samples = samples; p.tol_t = 0.0;
    p.max_acc = 5.0; p.max_thrust = 8.0; p.min_thrust = 3.0;
    isdf_traj_limits_info a, b;
    std::vector<double> pa(12 * (size_t)N), pb(12 * (size_t)N);
    if (isdf_host::tl_report_traj(cfg, N, T, C.data(), &p, &a, pa.data()) != ISDF_OK) return 1;
    if (isdf_host::tl_report_traj(cfg, N, T, C.data(), &p, &b, pb.data()) != ISDF_OK) return 1;
    if (std::memcmp(&a, &b, sizeof(a)) != 0 || std::memcmp(pa.data(), pb.data(), pa.size() * sizeof(double)) != 0) return 2;
    if (isdf_host::tl_report_traj(cfg, N, T, C.data(), &p, &b, nullptr) != ISDF_OK || std::memcmp(&a, &b, sizeof(a)) != 0) return 3;
    const isdf_host::TLFlat P = isdf_host::tl_flat_params(cfg);
    const int S = isdf_host::tl_samples(&p, cfg);
    if (a.samples != S || a.judged != 63) return 4;
    for (int i = 0; i < N; i++)
        for (int j = 0; j <= S; j++) {
            double f[6];
            isdf_host::tl_channels(P, N, C.data(), i, isdf_host::tl_sample_time(T[i], S, j), f);
            for (int ch = 0; ch < 6; ch++) {
                const double v = isdf_host::tl_report(ch, f[ch]), got = pa[12 * (size_t)i + 2 * ch];
                if (ch == 5 ? got > v : got < v) return 5;
            }
        }
    for (int ch = 0; ch < 6; ch++) {
        if (a.piece[ch] < 0 || a.piece[ch] >= N || pa[12 * (size_t)a.piece[ch] + 2 * ch] != a.value[ch]) return 6;
        int over = 0;
        for (int i = 0; i < N; i++) over += isdf_host::tl_over(ch, pa[12 * (size_t)i + 2 * ch], a.limit[ch]) ? 1 : 0;
        if (over != a.n_pieces_over[ch] || ((a.feasible >> ch) & 1) != (over == 0 ? 1 : 0)) return 7;
    }
    runs++;
    return 0;
}

int main() {
    const isdf_config cfg = config();
    int bad = 0, runs = 0;
    std::vector<double> C;
    {   // the case list's shapes
        const double T1[1] = {1.0}, T2[2] = {1.0, 1.0}, T3[3] = {0.05, 12.0, 1.0};
        for (int samples : {0, 1, 2, 5, 63, 64, 65, 257}) { traj(1, T1, false, C); bad += report(cfg, 1, T1, C, samples, runs) != 0; }
        traj(2, T2, false, C); bad += report(cfg, 2, T2, C, 0, runs) != 0;
        traj(3, T3, false, C); bad += report(cfg, 3, T3, C, 0, runs) != 0;
        traj(3, T3, false, C); bad += report(cfg, 3, T3, C, 1, runs) != 0;
        traj(2, T2, true, C); bad += report(cfg, 2, T2, C, 0, runs) != 0;
        isdf_traj_limits_info h;
        if (isdf_host::tl_report_traj(cfg, 2, T2, C.data(), nullptr, &h, nullptr) != ISDF_OK) bad++;
        for (int ch = 0; ch < 6; ch++) if (h.time[ch] != 0.0 || h.piece[ch] != 0) bad++;
        if (h.value[0] != 0.0 || h.value[2] != 0.0 || h.value[3] != 0.0 || h.judged != 13) bad++;
        std::vector<double> T130(130);
        for (auto &t : T130) t = rndu(0.5, 1.5);
        traj(130, T130.data(), false, C); bad += report(cfg, 130, T130.data(), C, 5, runs) != 0;
        std::printf("reports ok: %d reports, %d failures\n", runs, bad);
    }
    {   // the golden's own inputs: MID, TILTED (tilt 2.5 rad), OMG, the junction tie, the monotone piece
        isdf_config g = cfg;
        g.vmax = g.omgmax = g.thetamax = 1.0e3;
        for (const GoldenCase &gc : GOLDEN_CASES) {
            C.assign(gc.C, gc.C + 18 * (size_t)gc.N);
            bad += report(g, gc.N, gc.T, C, 0, runs) != 0;
            isdf_traj_limits_info a;
            std::vector<double> po(12 * (size_t)gc.N);
            if (isdf_host::tl_report_traj(g, gc.N, gc.T, C.data(), nullptr, &a, po.data()) != ISDF_OK) { bad++; continue; }
            for (int ch = 0; ch < 6; ch++)          // (the tight bounds are the Python tests'; here: the right extremum was found)
                if (!(std::fabs(a.value[ch] - gc.value[ch]) <= 1e-12 * std::fabs(gc.value[ch]))) bad++;
            const std::string name = gc.name;
            if (name == "n2_junction")
                for (int ch = 0; ch < 2; ch++) {    // both pieces report the junction, the same bits; the tie goes to the earlier piece
                    if (po[2 * ch] != po[12 + 2 * ch] || po[2 * ch + 1] != 1.0 || po[12 + 2 * ch + 1] != 1.0) bad++;
                    if (a.piece[ch] != 0 || a.time[ch] != 1.0 || a.value[ch] != gc.value[ch]) bad++;
                }
            if (name == "n1_monotone" && (a.time[5] != 0.0 || a.time[0] != 1.5 || a.time[1] != 1.5 || a.time[4] != 1.5)) bad++;
            if (name == "n1_tilted" && !(std::fabs(a.value[3] - 2.5) < 1e-3)) bad++;
        }
        std::printf("golden inputs ok: %d failures\n", bad);
    }
    {   // a limit equal to the reported value is feasible, one nextafter beyond it is over
        const double T3[3] = {0.7, 1.3, 1.0};
        traj(3, T3, false, C);
        isdf_traj_limits_info a, b;
        if (isdf_host::tl_report_traj(cfg, 3, T3, C.data(), nullptr, &a, nullptr) != ISDF_OK) bad++;
        isdf_config c2 = cfg;
        c2.vmax = a.value[0]; c2.omgmax = a.value[2]; c2.thetamax = a.value[3];
        isdf_traj_limits_params p;
        std::memset(&p, 0, sizeof(p));
        p.max_acc = a.value[1]; p.max_thrust = a.value[4]; p.min_thrust = a.value[5];
        if (isdf_host::tl_report_traj(c2, 3, T3, C.data(), &p, &b, nullptr) != ISDF_OK || b.feasible != 63 || b.judged != 63) bad++;
        c2.vmax = std::nextafter(a.value[0], 0.0); c2.omgmax = std::nextafter(a.value[2], 0.0); c2.thetamax = std::nextafter(a.value[3], 0.0);
        p.max_acc = std::nextafter(a.value[1], 0.0); p.max_thrust = std::nextafter(a.value[4], 0.0); p.min_thrust = std::nextafter(a.value[5], 1e300);
        if (isdf_host::tl_report_traj(c2, 3, T3, C.data(), &p, &b, nullptr) != ISDF_OK || b.feasible != 0 || b.judged != 63) bad++;
        for (int ch = 0; ch < 6; ch++) if (b.n_pieces_over[ch] < 1) bad++;
        std::printf("limits ok: %d failures\n", bad);
    }
    {   // the sampler: ends, junctions, out of range; rejected arguments
        const double T3[3] = {0.05, 12.0, 1.0};
        traj(3, T3, false, C);
        const std::vector<double> t = {0.0, 13.05, 0.05, std::nextafter(0.05, 0.0), std::nextafter(0.05, 1.0), 12.05, -0.3, 14.0, 1e9, -1e9};
        std::vector<double> rows(ISDF_TRAJ_SAMPLE_ROW * t.size());
        if (isdf_host::tl_sample_traj(cfg, 3, T3, C.data(), (long long)t.size(), t.data(), rows.data()) != ISDF_OK) bad++;
        for (size_t k = 0; k < 8 * (size_t)ISDF_TRAJ_SAMPLE_ROW; k++) if (!std::isfinite(rows[k])) bad++;
        double tt = 0.05;
        if (isdf_host::tl_locate(T3, 3, tt) != 0 || tt != 0.05) bad++;          // a junction time belongs to the earlier piece
        tt = 14.0;
        if (isdf_host::tl_locate(T3, 3, tt) != 2) bad++;
        tt = -0.3;
        if (isdf_host::tl_locate(T3, 3, tt) != 0 || tt != -0.3) bad++;
        if (isdf_host::tl_sample_traj(cfg, 3, T3, C.data(), 0, nullptr, nullptr) != ISDF_OK) bad++;
        const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
        isdf_traj_limits_info a;
        for (double x : {0.0, -1.0, inf, nan}) {
            const double Tb[2] = {1.0, x};
            if (isdf_host::tl_report_traj(cfg, 2, Tb, C.data(), nullptr, &a, nullptr) != ISDF_ERR_INVALID_ARG) bad++;
            if (isdf_host::tl_sample_traj(cfg, 2, Tb, C.data(), 1, t.data(), rows.data()) != ISDF_ERR_INVALID_ARG) bad++;
        }
        if (isdf_host::tl_report_traj(cfg, 0, T3, C.data(), nullptr, &a, nullptr) != ISDF_ERR_INVALID_ARG) bad++;
        if (isdf_host::tl_report_traj(cfg, 3, nullptr, C.data(), nullptr, &a, nullptr) != ISDF_ERR_INVALID_ARG) bad++;
        if (isdf_host::tl_sample_traj(cfg, 3, T3, C.data(), 2, nullptr, rows.data()) != ISDF_ERR_INVALID_ARG) bad++;
        if (isdf_host::tl_sample_traj(cfg, 3, T3, C.data(), -1, t.data(), rows.data()) != ISDF_ERR_INVALID_ARG) bad++;
        std::printf("sampler ok: %d failures\n", bad);
    }
    return bad ? 1 : 0;
}
