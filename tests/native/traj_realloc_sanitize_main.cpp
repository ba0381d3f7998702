// traj_realloc_host.hpp (over traj_limits_host.hpp and minco_pcr.hpp) as a stand-alone program for AddressSanitizer / UBSan: the solve
// at N = 1, 2, 3 and 33, the factor rule's edges and the whole loop with status 0, 1 and 2, on seeded waypoint problems at rest at
// both ends.  Built and run by tests/test_traj_realloc_host.py; nothing of it runs in the Python process.
#include "traj_realloc_host.hpp"
#include <cstdio>
#include <vector>

namespace {
isdf_config config(double vmax, double omgmax, double thetamax) {
    isdf_config c;
    std::memset(&c, 0, sizeof(c));
    c.vehicle_mass = 0.61; c.grav_acc = 9.8; c.horiz_drag = 0.1; c.vert_drag = 0.1; c.paras_drag = 0.01; c.speed_eps = 0.0001;
    c.integral_intervs = 4; c.vmax = vmax; c.omgmax = omgmax; c.thetamax = thetamax;
    return c;
}
int failures = 0;
void expect(bool ok, const char *what) { if (!ok) { std::printf("FAILED: %s\n", what); failures++; } }

struct Problem { int N; double head[9], tail[9]; std::vector<double> Q, T; };
// waypoints 1.2 m apart along x with a seeded zig-zag, durations piece_T with a seeded spread
Problem problem(int N, unsigned seed, double piece_T) {
    Problem p;
    p.N = N;
    std::memset(p.head, 0, sizeof(p.head)); std::memset(p.tail, 0, sizeof(p.tail));
    p.head[0] = p.head[1] = p.head[2] = 1.0;
    p.tail[0] = 1.0 + 1.2 * N; p.tail[1] = 1.0; p.tail[2] = 1.0;
    unsigned s = seed;
    auto rnd = [&s]() { s = s * 1664525u + 1013904223u; return (double)(s >> 8) / (double)(1u << 24) - 0.5; };
    p.Q.resize((size_t)3 * (N > 1 ? N - 1 : 1), 0.0);
    for (int j = 1; j < N; j++) { p.Q[3 * (size_t)(j - 1)] = 1.0 + 1.2 * j + 0.4 * rnd(); p.Q[3 * (size_t)(j - 1) + 1] = 1.0 + 0.8 * rnd(); p.Q[3 * (size_t)(j - 1) + 2] = 1.0 + 0.3 * rnd(); }
    p.T.resize((size_t)N);
    for (int i = 0; i < N; i++) p.T[(size_t)i] = piece_T * (1.0 + 0.3 * rnd());
    return p;
}

void loop(const char *name, const isdf_config &cfg, const Problem &p, const isdf_traj_realloc_params &P, int want_status) {
    const int N = p.N;
    std::vector<double> To((size_t)N), Co((size_t)18 * N), Cs((size_t)18 * N);
    isdf_traj_realloc_info info;
    isdf_host::RATrace tr;
    expect(isdf_host::ra_realloc_traj(cfg, N, p.head, p.tail, p.Q.data(), p.T.data(), &P, To.data(), Co.data(), &info, &tr) == ISDF_OK, "loop returns");
    expect(info.status == want_status, "status");
    expect(isdf_host::ra_minco_traj(N, p.head, p.tail, p.Q.data(), To.data(), Cs.data()) == ISDF_OK, "solve returns");
    expect(std::memcmp(Cs.data(), Co.data(), Co.size() * sizeof(double)) == 0, "the coefficients are the solve of the returned durations");
    isdf_traj_limits_info rep;
    isdf_host::tl_report_traj(cfg, N, To.data(), Co.data(), &P.limits, &rep, nullptr);
    expect(std::memcmp(&rep, &info.limits, sizeof(rep)) == 0, "info.limits is the report of the result");
    for (int i = 0; i < N; i++) expect(To[(size_t)i] >= p.T[(size_t)i], "durations never shrink");
    std::printf("%s ok: N %d status %d rounds %d changed %d max factor %.6g duration %.6g -> %.6g\n", name, N, info.status, info.rounds, info.pieces_changed,
                info.max_factor, info.duration_in, info.duration_out);
}
}  // namespace

int main() {
    // the solve alone: N = 1 has no junction system, N = 2 one row and no round, N = 33 six rounds
    for (int N : {1, 2, 3, 33}) {
        const Problem p = problem(N, 11u + (unsigned)N, 0.8);
        std::vector<double> C((size_t)18 * N);
        expect(isdf_host::ra_minco_traj(N, p.head, p.tail, N > 1 ? p.Q.data() : nullptr, p.T.data(), C.data()) == ISDF_OK, "solve returns");
        for (int d = 0; d < 3; d++) expect(C[(size_t)d * 6 * N] == p.head[d], "the first piece starts at the head");
    }
    std::printf("solve ok: N = 1, 2, 3, 33\n");
    // the factor rule's edges
    const double nan = std::numeric_limits<double>::quiet_NaN();
    double lim[6] = {2.0, 5.0, 2.5, 0.6, 9.0, 3.0}, row[12] = {1.0, 0, 2.0, 0, 1.0, 0, 0.3, 0, 7.0, 0, 5.0, 0};
    int over = -1;
    expect(isdf_host::ra_piece_factor(row, lim, 0.02, 2.0, &over) == 1.0 && over == 0, "nothing over");
    row[0] = 1e300; row[10] = -1.0;
    expect(isdf_host::ra_piece_factor(row, lim, 0.02, 2.0, &over) == 2.0 && over == 0b100001, "the clamp");
    double none[6] = {nan, nan, nan, nan, nan, nan};
    expect(isdf_host::ra_piece_factor(row, none, 0.02, 2.0, &over) == 1.0 && over == 0, "nothing judged");
    std::printf("factor ok: the edges\n");

    isdf_traj_realloc_params P;
    isdf_host::ra_params_default(&P);
    P.limits.max_acc = 5.0; P.limits.max_thrust = 9.0; P.limits.min_thrust = 3.0;
    const isdf_config cfg = config(2.0, 2.5, 0.6);
    loop("slow n5", cfg, problem(5, 3u, 2.5), P, ISDF_REALLOC_ALREADY);
    loop("fast n5", cfg, problem(5, 3u, 0.5), P, ISDF_REALLOC_OK);
    loop("fast n33", cfg, problem(33, 5u, 0.6), P, ISDF_REALLOC_OK);
    P.rounds = 1; P.f_max = 1.01;
    loop("fast n5 one round", cfg, problem(5, 3u, 0.5), P, ISDF_REALLOC_NOT_REACHED);
    // argument errors
    const Problem p = problem(3, 1u, 1.0);
    std::vector<double> To(3), Co(54);
    P.rounds = 17;
    expect(isdf_host::ra_realloc_traj(cfg, 3, p.head, p.tail, p.Q.data(), p.T.data(), &P, To.data(), Co.data(), nullptr) == ISDF_ERR_INVALID_ARG, "rounds 17");
    P.rounds = 8;
    expect(isdf_host::ra_realloc_traj(cfg, 3, p.head, p.tail, p.Q.data(), p.T.data(), &P, const_cast<double *>(p.T.data()), Co.data(), nullptr) == ISDF_ERR_INVALID_ARG,
           "an output that is an input");
    if (failures) return 1;
    return 0;
}
