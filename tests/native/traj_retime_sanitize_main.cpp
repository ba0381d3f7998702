// traj_retime_host.hpp (over traj_limits_host.hpp) as a stand-alone program for AddressSanitizer / UBSan: the scaling, the pick
// rule at both ends of its range and the whole search with status 0, 1 and 2, on the golden inputs of traj_limits_cases.inc.
// Built and run by tests/test_traj_retime_host.py; nothing of it runs in the Python process.
#include "traj_retime_host.hpp"
#include <cstdio>
#include <vector>

namespace {
#include "traj_limits_cases.inc"

isdf_config config(double vmax, double omgmax, double thetamax) {
    isdf_config c;
    std::memset(&c, 0, sizeof(c));
    c.vehicle_mass = 0.61; c.grav_acc = 9.8; c.horiz_drag = 0.1; c.vert_drag = 0.1; c.paras_drag = 0.01; c.speed_eps = 0.0001;
    c.integral_intervs = 4; c.vmax = vmax; c.omgmax = omgmax; c.thetamax = thetamax;
    return c;
}
int failures = 0;
void expect(bool ok, const char *what) { if (!ok) { std::printf("FAILED: %s\n", what); failures++; } }

void search(const char *name, const isdf_config &cfg, int N, const double *T, const double *C, const isdf_traj_retime_params &P, int want_status) {
    std::vector<double> To((size_t)N), Co((size_t)18 * N), Ts((size_t)N), Cs((size_t)18 * N);
    isdf_traj_retime_info info;
    expect(isdf_host::tr_retime_traj(cfg, N, T, C, &P, To.data(), Co.data(), &info) == ISDF_OK, "search returns");
    expect(info.status == want_status, "status");
    expect(isdf_host::tr_scale_traj(N, T, C, info.scale, Ts.data(), Cs.data()) == ISDF_OK, "scale returns");
    expect(std::memcmp(Ts.data(), To.data(), To.size() * sizeof(double)) == 0 && std::memcmp(Cs.data(), Co.data(), Co.size() * sizeof(double)) == 0,
           "the result is the input scaled by info.scale");
    isdf_traj_limits_info rep;
    isdf_host::tl_report_traj(cfg, N, To.data(), Co.data(), &P.limits, &rep, nullptr);
    rep.device_ms = info.limits.device_ms;
    expect(std::memcmp(&rep, &info.limits, sizeof(rep)) == 0, "info.limits is the report of the result");
    std::printf("%s ok: status %d scale %.17g below %.17g rounds %d candidates %d\n", name, info.status, info.scale, info.scale_below, info.rounds,
                info.candidates);
}
}  // namespace

int main() {
    // the pick rule at both ends of the ladder range
    int nm = 0;
    expect(isdf_host::tr_pick(3ull, 2, &nm) == 0 && nm == 0, "L = 2, all feasible");
    expect(isdf_host::tr_pick(0ull, 2, &nm) == 2 && nm == 0, "L = 2, none feasible");
    expect(isdf_host::tr_pick(~0ull, 64, &nm) == 0 && nm == 0, "L = 64, all feasible");
    expect(isdf_host::tr_pick(0ull, 64, &nm) == 64 && nm == 0, "L = 64, none feasible");
    expect(isdf_host::tr_pick(~0ull ^ (1ull << 63), 64, &nm) == 64 && nm == 1, "L = 64, the top one infeasible");
    expect(isdf_host::tr_pick(~0ull ^ (1ull << 31), 64, &nm) == 32 && nm == 1, "L = 64, one infeasible in the middle");
    std::printf("pick ok: both ends of the range\n");

    isdf_traj_retime_params P;
    isdf_host::tr_params_default(&P);
    P.ladder = 5; P.rounds = 3;
    // status 0: only the speed binds
    search("n1_mid speed", config(1.0, 1000.0, 1000.0), 1, n1_mid_T, n1_mid_C, P, ISDF_RETIME_OK);
    // status 0 at the largest ladder, two pieces, every channel judged
    P.ladder = 64; P.rounds = 4; P.limits.max_acc = 3.0; P.limits.max_thrust = 7.5; P.limits.min_thrust = 5.5;
    search("n2_junction all", config(1.0, 1.0, 0.4), 2, n2_junction_T, n2_junction_C, P, ISDF_RETIME_OK);
    // status 1: nothing binds; the smallest ladder
    isdf_host::tr_params_default(&P);
    P.ladder = 2; P.rounds = 1;
    search("n1_omg at lower", config(1000.0, 1000.0, 1000.0), 1, n1_omg_T, n1_omg_C, P, ISDF_RETIME_AT_LOWER);
    // status 2: a smallest thrust above m g is never reached
    isdf_host::tr_params_default(&P);
    P.ladder = 5; P.limits.min_thrust = 6.5;
    search("n1_tilted not reachable", config(1000.0, 1000.0, 1000.0), 1, n1_tilted_T, n1_tilted_C, P, ISDF_RETIME_NOT_REACHABLE);
    // argument errors
    double x[18] = {0}, t1[1] = {1.0}, o[18];
    expect(isdf_host::tr_scale_traj(1, t1, x, 0.0, o, o) == ISDF_ERR_INVALID_ARG, "factor 0");
    P.ladder = 65;
    expect(isdf_host::tr_retime_traj(config(1, 1, 1), 1, t1, x, &P, o, o, nullptr) == ISDF_ERR_INVALID_ARG, "ladder 65");
    if (failures) return 1;
    return 0;
}
