// Test shim: exposes the PRODUCT's host mid end (implicit-sdf-planner_amd/csrc/midend_host.hpp) to the CPU-only tests without
// needing a HIP device.  Built by tests/test_midend_host.py with g++.
#include "midend_host.hpp"
extern "C" {
// prm: weight_pr, rho_mid_end, rel_cost_tol, min_step, g_epsilon, integral_intervs, mem_size, past
static isdf_host::MidendParams params_of(const double *prm) {
    isdf_host::MidendParams p;
    p.weight_pr = prm[0]; p.rho = prm[1]; p.rel_cost_tol = prm[2]; p.min_step = prm[3]; p.g_epsilon = prm[4];
    p.integral_intervs = (int)prm[5]; p.mem_size = (int)prm[6]; p.past = (int)prm[7];
    return p;
}
// g: n, parts: 3, pos_out / vel_out (nullable together): the samples' positions and velocities [N - 1][3]
double shim_midend_cost(int N, const double *head9, const double *tail9, const double *ref, const double *prm, const double *x,
                        double *g, double *parts, double *pos_out, double *vel_out) {
    isdf_host::Midend m;
    m.setup(head9, tail9, N, ref, params_of(prm));
    const double c = m.cost(x, g);
    for (int k = 0; k < 3; k++) parts[k] = m.parts[k];
    if (pos_out && vel_out) for (int i = 0; i < N - 1; i++) m.sample_state(i, pos_out + 3 * i, vel_out + 3 * i);
    return c;
}
// x_out: n; res: f, status, iterations, evaluations
void shim_midend_fit(int N, const double *head9, const double *tail9, const double *ref, const double *prm, const double *T_init,
                     double *x_out, double *res) {
    isdf_host::Midend m;
    m.setup(head9, tail9, N, ref, params_of(prm));
    m.seed(T_init, x_out);
    const isdf_host::LbfgsResult r = m.fit(x_out, isdf_host::Midend::evaluate, &m, nullptr, nullptr);
    res[0] = r.f; res[1] = r.status; res[2] = r.iterations; res[3] = r.evaluations;
}
}
