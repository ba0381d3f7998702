// Host form of the MID END: OriTraj::getOriTraj (src/planner_algorithm/src/mid_end.cpp:3-94) - the MINCO fit to the front end's
// waypoints whose result (opt_x) the back end starts from (plan_manager.cpp:270,289) - with its objective
// (src/planner_algorithm/include/planner_algorithm/mid_end.hpp:184-304) restated over csrc/minco_host.hpp and csrc/lbfgs_host.hpp.
// Plain C++, no HIP: the device form (csrc/midend.hip) evaluates the same objective in one launch per callback.
//
//   variables   x = [tau(N) | inner waypoints 3(N-1), point-major]  (mid_end.cpp:21-23: the layout of isdf_pack_variables)
//   cost        MINCO jerk energy + weight_pr * sum(pose penalty) + rho_mid_end * sum(T)                    (mid_end.hpp:262-304)
//
// The reference stores accelerations, att_constraints and weightAR (mid_end.hpp:41-43,60) and never reads them: costFunction calls
// addPosePenalty only.  There is no attitude term here either.
#pragma once
#include "lbfgs_host.hpp"
#include "minco_host.hpp"
#include <cmath>
#include <cstring>
#include <vector>

namespace isdf_host {

struct MidendParams {               // config_*.yaml: the values all shipped files agree on
    double weight_pr = 1000.0;      // weight_pr
    double rho = 200.0;             // rho_mid_end
    double rel_cost_tol = 1.0e-6;   // relCostTolMidEnd -> lbfgs delta (mid_end.cpp:54)
    double min_step = 1.0e-32, g_epsilon = 0.0;
    int integral_intervs = 64;      // integralIntervs (mid_end.hpp:323)
    int mem_size = 16, past = 10;
};

// OriTraj::grad_cost_dir (mid_end.hpp:184-199): cost_p = |d|^3, gradp = 3 |d|^2 d / |d| with d = pos - ref; false when cost_p is
// not > 0 (d = 0: Eigen's normalized() leaves a zero vector alone, and the caller skips the contribution)
inline bool midend_pose_penalty(const double pos[3], const double ref[3], double gradp[3], double &cost_p) {
    const double d[3] = {pos[0] - ref[0], pos[1] - ref[1], pos[2] - ref[2]};
    const double nrm = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    cost_p = std::pow(nrm, 3);
    gradp[0] = gradp[1] = gradp[2] = 0.0;
    if (!(cost_p > 0.0)) return false;
    const double s = 3 * std::pow(nrm, 2);
    for (int k = 0; k < 3; k++) gradp[k] = s * (d[k] / nrm);
    return true;
}

// The driver's parameters as getOriTraj sets them (mid_end.cpp:48-54): lbfgs_parameter_t's defaults, then mem_size, past, min_step,
// g_epsilon from the config, max_iterations = 100000, delta = relCostTolMidEnd.
inline LbfgsParams midend_lbfgs_params(const MidendParams &p) {
    LbfgsParams q;
    q.mem_size = p.mem_size; q.past = p.past; q.min_step = p.min_step; q.g_epsilon = p.g_epsilon;
    q.max_iterations = 100000;
    q.delta = p.rel_cost_tol;
    return q;
}

class Midend {
public:
    MidendParams param;
    MincoS3 minco;
    std::vector<double> ref;        // [N - 1][3]: ref_points (mid_end.cpp:36)
    double parts[3] = {0, 0, 0};    // energy | weight_pr * sum(pose penalty) | rho * sum(T) of the last cost()

    // minco.setConditions (mid_end.cpp:20) + ref_points; head / tail: 3x3 column-major (position, velocity, acceleration)
    void setup(const double *head9, const double *tail9, int N, const double *ref_points, const MidendParams &p) {
        param = p;
        if (N != minco.N || std::memcmp(head_, head9, sizeof(head_)) != 0 || std::memcmp(tail_, tail9, sizeof(tail_)) != 0) {
            minco.set_conditions(head9, tail9, N);
            std::memcpy(head_, head9, sizeof(head_)); std::memcpy(tail_, tail9, sizeof(tail_));
            T.assign(N, 0.0); gdC.assign((size_t)18 * N, 0.0); gdT.assign(N, 0.0); gradP.assign((size_t)3 * (N - 1), 0.0); gradT.assign(N, 0.0);
        }
        ref.assign(ref_points, ref_points + (size_t)3 * (N - 1));
    }

    // sample position and velocity of constraint i (piece i + 1 at s1 = T(i + 1) / integral_intervs, mid_end.hpp:231-245) of the last cost()
    void sample_state(int i, double pos[3], double vel[3]) const { sample(i, pos, vel); }

    // OriTraj::costFunction (mid_end.hpp:262-304)
    double cost(const double *x, double *g) {
        const int N = minco.N;
        for (int i = 0; i < N; i++) T[i] = tau_to_T(x[i]);                       // forwardT (:275)
        minco.set_parameters(x + N, T.data());                                   // (:279)
        double cost = minco.energy(gdC.data(), gdT.data());                      // (:281-283)
        parts[0] = cost;
        // addPosePenalty (:201-260)
        const double alpha = 1.0 / param.integral_intervs;                       // (:225)
        double pen = 0.0;
        for (int i = 0; i < N - 1; i++) {                                        // constraint i samples piece i + 1: piece 0 gets none (:228-232)
            const int seg = i + 1;
            double pos[3], vel[3], gradp[3], cost_p;
            const double s1 = sample(i, pos, vel);
            if (midend_pose_penalty(pos, ref.data() + 3 * i, gradp, cost_p)) {   // (:249)
                const double beta0[6] = {1.0, s1, s1 * s1, (s1 * s1) * s1, (s1 * s1) * (s1 * s1), ((s1 * s1) * (s1 * s1)) * s1};
                const double gradViolaPt = alpha * (gradp[0] * vel[0] + gradp[1] * vel[1] + gradp[2] * vel[2]);      // (:253)
                for (int d = 0; d < 3; d++)
                    for (int q = 0; q < 6; q++) gdC[(size_t)d * 6 * N + 6 * seg + q] += param.weight_pr * (beta0[q] * gradp[d]);   // (:252,255)
                gdT[seg] += param.weight_pr * (cost_p * gradViolaPt);            // (:256) times cost_p, as the reference has it
                cost += param.weight_pr * cost_p;                                // (:257)
                pen += param.weight_pr * cost_p;
            }
        }
        parts[1] = pen;
        minco.propagate_grad(gdC.data(), gdT.data(), gradP.data(), gradT.data());                                    // (:295)
        double tsum = 0.0;
        for (int i = 0; i < N; i++) tsum += T[i];
        cost += param.rho * tsum;                                                // (:298)
        parts[2] = param.rho * tsum;
        for (int i = 0; i < N; i++) g[i] = grad_T_to_tau(x[i], gradT[i] + param.rho);                                // (:300-301)
        for (int i = 0; i < 3 * (N - 1); i++) g[N + i] = gradP[i];               // (:302)
        return cost;
    }
    static double evaluate(void *instance, const double *x, double *g, const int) { return ((Midend *)instance)->cost(x, g); }

    // tau = backwardT(T_init), xi = ref_points (mid_end.cpp:27-41)
    void seed(const double *T_init, double *x) const {
        const int N = minco.N;
        for (int i = 0; i < N; i++) x[i] = T_to_tau(T_init[i]);
        for (int i = 0; i < 3 * (N - 1); i++) x[N + i] = ref[i];
    }

    // getOriTraj's lbfgs_optimize call (mid_end.cpp:48-62) on `evaluate` (this class's, or the device form's); x holds the seed on
    // entry and the last iterate on return, whatever the status (the reference extracts the trajectory either way, :65-92).
    // The reference's own hook (earlyExit, mid_end.hpp:613-631) cancels past 8000 iterations; here the caller's hook decides.
    LbfgsResult fit(double *x, lbfgs_eval_fn eval, void *instance, lbfgs_progress_fn progress, void *progress_instance) const {
        Lbfgs opt;
        opt.param = midend_lbfgs_params(param);
        opt.evaluate = eval; opt.instance = instance;
        opt.progress = progress; opt.progress_instance = progress_instance;
        return opt.minimize(x, minco.N + 3 * (minco.N - 1));
    }

private:
    double head_[9] = {0}, tail_[9] = {0};
    std::vector<double> T, gdC, gdT, gradP, gradT;

    // pos = c^T beta0, vel = c^T beta1 of piece i + 1 at s1 (mid_end.hpp:234-245); returns s1
    double sample(int i, double pos[3], double vel[3]) const {
        const int N = minco.N, seg = i + 1;
        const double alpha = 1.0 / param.integral_intervs;
        const double s1 = alpha * T[seg], s2 = s1 * s1, s3 = s2 * s1, s4 = s2 * s2, s5 = s4 * s1;
        const double beta0[6] = {1.0, s1, s2, s3, s4, s5}, beta1[6] = {0.0, 1.0, 2.0 * s1, 3.0 * s2, 4.0 * s3, 5.0 * s4};
        for (int d = 0; d < 3; d++) {
            const double *c = minco.c.data() + (size_t)d * 6 * N + 6 * seg;
            double p = 0.0, v = 0.0;
            for (int q = 0; q < 6; q++) { p += c[q] * beta0[q]; v += c[q] * beta1[q]; }
            pos[d] = p; vel[d] = v;
        }
        return s1;
    }
};

} // namespace isdf_host
