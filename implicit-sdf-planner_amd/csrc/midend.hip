// The MID END on the device: OriTraj::costFunction (src/planner_algorithm/include/planner_algorithm/mid_end.hpp:262-304) as ONE
// launch per callback, one workgroup per trajectory, and the fit around it (OriTraj::getOriTraj, src/planner_algorithm/src/mid_end.cpp:3-94).
// The back end's callback is cb_pre_kernel -> sweeps -> cb_post_kernel; the mid end has no sweep in the middle - its pose penalty
// (addPosePenalty, mid_end.hpp:201-260) is one sample per inner waypoint - so the two bodies of csrc/minco_dev_body.hpp and the
// penalty between them fit in one kernel:
//
//   stage      the launch's inputs [x | ends | ref_points] from host-mapped memory into device memory (one round of PCIe reads)
//   pre body   tau -> T, the PCR solve, coefficients, energy and its partials
//   penalty    one thread per constraint: the packed [cost | gradT | gradC] block cb_post_body reads as its `sweep` input
//   post body  the adjoint solve, rho * sum(T), the chain rule; (cost, g, parts) and the completion flag into host-mapped memory
//
// The host form (csrc/midend_host.hpp) is the reference's arithmetic on the band LU; the two agree to rounding.
#include "isdf_ctx.hpp"
#include "minco_dev_body.hpp"
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

namespace isdf {

// mode 0 (auto): a single trajectory of up to this many pieces keeps the host form (provisional: the back end's threshold, where
// the host's band LU beats a launch plus hand-over - DESIGN 4.10)
constexpr int MID_AUTO_HOST_MAX_N = CB_AUTO_HOST_MAX_N;

struct MidDev {
    CbDev P;                    // the bodies' block: n_out = 1, sweep = pen, rho = rho_mid_end
    const double *in;           // [nb][L] host-mapped: x (N + 3 (N - 1)) | ends (18) | ref_points (3 (N - 1))
    double *xs, *ends, *ref;    // their device copies: [nb][nvar], [nb][18], [nb][3 (N - 1)]
    double *pen;                // [nb][1 + 19 N] the penalty's packed block
    int L;
    double weight_pr, alpha;    // weightPR, 1 / integralRes (mid_end.hpp:225)
};

// addPosePenalty (mid_end.hpp:201-260): constraint i (thread i) samples piece i + 1 at s1 = alpha * T(i + 1); piece 0 gets nothing.
// The block is zeroed, then every thread fills the rows of its own piece: a fixed order, no atomics.  No contraction: the
// penalty's products and sums round as the reference's do.
__device__ __forceinline__ void midend_penalty(const MidDev &M, const int b, double *s_part) {
#pragma clang fp contract(off)
    const int N = M.P.N, n = N - 1;
    const size_t ostride = (size_t)1 + 19 * (size_t)N;
    double *S = M.pen + (size_t)b * ostride;
    for (size_t i = threadIdx.x; i < ostride; i += blockDim.x) S[i] = 0.0;
    __threadfence();
    __syncthreads();
    double cp = 0.0;
    const int i = (int)threadIdx.x;
    if (i < n) {
        const int seg = i + 1;                                                     // (:231)
        const double T = M.P.T[(size_t)b * N + seg];
        const double *C = M.P.coeffs + (size_t)b * 18 * N + 6 * seg;
        const double *ref = M.ref + (size_t)b * 3 * n + 3 * i;
        const double s1 = M.alpha * T, s2 = s1 * s1, s3 = s2 * s1, s4 = s2 * s2, s5 = s4 * s1;      // (:234-238)
        double d[3], vel[3];
        for (int a = 0; a < 3; a++) {                                              // pos = c^T beta0, vel = c^T beta1 (:244-245), Horner form
            const double *c = C + (size_t)a * 6 * N;
            const double pos = c[0] + s1 * (c[1] + s1 * (c[2] + s1 * (c[3] + s1 * (c[4] + s1 * c[5]))));
            vel[a] = c[1] + s1 * (2.0 * c[2] + s1 * (3.0 * c[3] + s1 * (4.0 * c[4] + s1 * (5.0 * c[5]))));
            d[a] = pos - ref[a];
        }
        // grad_cost_dir (:184-199): cost_p = |d|^3, gradp = 3 |d|^2 d / |d|; skipped when cost_p is not > 0
        const double nrm = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        const double cost_p = nrm * nrm * nrm;
        if (cost_p > 0.0) {
            const double s = 3.0 * (nrm * nrm);
            const double gp[3] = {s * (d[0] / nrm), s * (d[1] / nrm), s * (d[2] / nrm)};
            const double beta0[6] = {1.0, s1, s2, s3, s4, s5};
            const double gradViolaPt = M.alpha * (gp[0] * vel[0] + gp[1] * vel[1] + gp[2] * vel[2]);             // (:253)
            for (int a = 0; a < 3; a++)
                for (int q = 0; q < 6; q++) S[1 + N + (size_t)a * 6 * N + 6 * seg + q] = M.weight_pr * (beta0[q] * gp[a]);   // (:252,255)
            S[1 + seg] = M.weight_pr * (cost_p * gradViolaPt);                     // (:256): times cost_p, as the reference has it
            cp = M.weight_pr * cost_p;                                             // (:257)
        }
    }
    const double total = cbd::block_sum(cp, s_part);
    if (threadIdx.x == 0) S[0] = total;
}

template <bool SPLIT> __global__ __launch_bounds__(SPLIT ? 1024 : 448) void midend_cb_kernel(const MidDev M) {
    extern __shared__ double s_mem[];
    __shared__ double s_part[16];
    const int b = (int)blockIdx.x, N = M.P.N, n = N - 1, nvar = N + 3 * n;
    const int NT = SPLIT ? (int)blockDim.x / 3 : (int)blockDim.x;
    {
        const double *in = M.in + (size_t)b * M.L;
        double *xs = M.xs + (size_t)b * nvar, *es = M.ends + (size_t)b * 18, *rs = M.ref + (size_t)b * 3 * n;
        for (int i = threadIdx.x; i < M.L; i += blockDim.x) {
            const double v = in[i];
            if (i < nvar) xs[i] = v;
            else if (i < nvar + 18) es[i - nvar] = v;
            else rs[i - nvar - 18] = v;
        }
    }
    __threadfence();
    __syncthreads();
    cbd::cb_pre_body<SPLIT>(M.P, b, NT, s_mem, s_part);
    __threadfence();                    // T, coefficients, junction states, energy block: written by other threads of this workgroup
    __syncthreads();
    midend_penalty(M, b, s_part);
    __threadfence();
    __syncthreads();
    cbd::cb_post_body<SPLIT>(M.P, b, (int)gridDim.x, NT, s_mem, s_part);
}

}  // namespace isdf

namespace {

using isdf::CB_MAX_N;
using isdf::CB_SPLIT_MAX_N;

// where the launch's arrays lie: device scratch (c->d_mid) and the pinned hand-over (c->h_mid), in doubles
struct MidLayout {
    size_t nvar, L, rs, ostride;
    size_t d_x, d_ends, d_ref, d_T, d_C, d_u, d_e, d_pen, d_total;
    size_t h_in, h_res, h_flags, h_total;
    MidLayout(int N, int nb) {
        const size_t n = (size_t)N - 1, B = (size_t)nb;
        nvar = (size_t)N + 3 * n; L = nvar + 18 + 3 * n; rs = 1 + nvar + 4; ostride = (size_t)1 + 19 * (size_t)N;
        d_x = 0; d_ends = d_x + B * nvar; d_ref = d_ends + B * 18; d_T = d_ref + B * 3 * n; d_C = d_T + B * N; d_u = d_C + B * 18 * N;
        d_e = d_u + B * 6 * ((size_t)N + 1); d_pen = d_e + B * ostride; d_total = d_pen + B * ostride;
        h_in = 0; h_res = h_in + B * L; h_flags = h_res + B * rs; h_total = h_flags + B;
    }
};

isdf_host::MidendParams host_params(const isdf_midend_params &p) {
    isdf_host::MidendParams q;
    q.weight_pr = p.weight_pr; q.rho = p.rho_mid_end; q.rel_cost_tol = p.rel_cost_tol; q.min_step = p.min_step; q.g_epsilon = p.g_epsilon;
    q.integral_intervs = p.integral_intervs; q.mem_size = p.mem_size; q.past = p.past;
    return q;
}

int mid_reserve(isdf_ctx *c, const MidLayout &Y) {
    int rc = c->d_mid.reserve(c, Y.d_total);
    if (rc) return rc;
    return c->h_mid.reserve(c, Y.h_total);
}
// trajectory b's inputs into the pinned record the launch stages from
void mid_put(isdf_ctx *c, const MidLayout &Y, int N, int b, const double *x, const double *head9, const double *tail9, const double *ref) {
    double *rec = c->h_mid + Y.h_in + (size_t)b * Y.L;
    std::memcpy(rec, x, Y.nvar * sizeof(double));
    std::memcpy(rec + Y.nvar, head9, 9 * sizeof(double));
    std::memcpy(rec + Y.nvar + 9, tail9, 9 * sizeof(double));
    std::memcpy(rec + Y.nvar + 18, ref, (size_t)3 * (N - 1) * sizeof(double));
}
// one launch for the nb records placed with mid_put; on return trajectory b's [cost | g | energy, -, pose, rho sum(T)] is at
// c->h_mid + Y.h_res + b * Y.rs.  The host's side is the hand-over of every host-mapped step: host_rows_mark / host_flag_wait /
// host_rows_wait (isdf_ctx.hpp, host_step.hip).
int mid_run(isdf_ctx *c, const isdf_midend_params &prm, const MidLayout &Y, int N, int nb) {
    const bool split = N <= CB_SPLIT_MAX_N;
    const int threads = ((N + 63) / 64) * 64 * (split ? 3 : 1);
    const size_t lds = isdf::cbd::cb_lds_doubles(N, split) * sizeof(double);
    isdf::MidDev M{};
    double *d = c->d_mid;
    M.P.N = N; M.P.nb = nb; M.P.n_out = 1; M.P.res_stride = (int)Y.rs;
    M.P.x = d + Y.d_x; M.P.ends = d + Y.d_ends; M.P.T = d + Y.d_T; M.P.coeffs = d + Y.d_C; M.P.u = d + Y.d_u; M.P.epart = d + Y.d_e;
    M.P.sweep = d + Y.d_pen; M.P.rho = prm.rho_mid_end;
    M.P.res = c->h_mid.dev() + Y.h_res; M.P.flag = (unsigned long long *)(c->h_mid.dev() + Y.h_flags);
    M.P.seq = ++c->mid_seq; M.P.stats = nullptr;
    M.in = c->h_mid.dev() + Y.h_in; M.xs = d + Y.d_x; M.ends = d + Y.d_ends; M.ref = d + Y.d_ref; M.pen = d + Y.d_pen;
    M.L = (int)Y.L; M.weight_pr = prm.weight_pr; M.alpha = 1.0 / prm.integral_intervs;
    host_rows_mark(c->h_mid + Y.h_res, (size_t)nb * Y.rs);
    std::memset((void *)(c->h_mid + Y.h_flags), 0, (size_t)nb * sizeof(double));
    __sync_synchronize();
    if (split) hipLaunchKernelGGL(isdf::midend_cb_kernel<true>, dim3(nb), dim3(threads), lds, c->stream, M);
    else hipLaunchKernelGGL(isdf::midend_cb_kernel<false>, dim3(nb), dim3(threads), lds, c->stream, M);
    HIPCHK(c, hipGetLastError());
    volatile unsigned long long *flags = (volatile unsigned long long *)(c->h_mid + Y.h_flags);
    const auto t0 = std::chrono::steady_clock::now();
    for (int b = 0; b < nb; b++) {
        unsigned long long f;
        if (!host_flag_wait(flags + b, M.P.seq, 0ull, t0, 5.0, c->stream, &f))
            return isdf_fail(c, ISDF_ERR_HIP, "mid-end callback did not complete (its completion word never arrived)");
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    if (!host_rows_wait(c, c->h_mid + Y.h_res, (size_t)nb * Y.rs)) {
        (void)hipStreamSynchronize(c->stream);
        return isdf_fail(c, ISDF_ERR_HIP, "mid-end callback: its completion word arrived but not all of its results");
    }
    return ISDF_OK;
}

// which form a call takes (isdf_set_minco_mode): 1 = host, 2 = device, 0 = host for a single trajectory of up to
// MID_AUTO_HOST_MAX_N pieces, device otherwise and for every batch; beyond CB_MAX_N pieces always the host
bool mid_on_device(const isdf_ctx *c, int N, bool batch) {
    if (N > CB_MAX_N || c->minco_mode == 1) return false;
    if (c->minco_mode == 2 || batch) return true;
    return N > isdf::MID_AUTO_HOST_MAX_N;
}

int mid_check(isdf_ctx *c, const isdf_midend_params *prm, int N) {
    if (!prm) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "mid end: null parameters");
    if (N < 2) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "mid end: at least one inner waypoint (N >= 2, plan_manager.cpp:209-213)");
    if (prm->integral_intervs < 1) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "mid end: integral_intervs must be >= 1");
    if (!c->peers.empty()) return isdf_fail(c, ISDF_ERR_UNSUPPORTED, "mid end: not on a multi-device ctx");
    return ISDF_OK;
}

// the objective of the single fit in its device form (lbfgs_eval_fn)
struct MidDevEval { isdf_ctx *c; const isdf_midend_params *prm; const double *ref; int N; int rc; };
double mid_dev_evaluate(void *instance, const double *x, double *g, const int n) {
    MidDevEval &E = *(MidDevEval *)instance;
    isdf_ctx *c = E.c;
    const MidLayout Y(E.N, 1);
    mid_put(c, Y, E.N, 0, x, c->cb_ends, c->cb_ends + 9, E.ref);
    const int rc = mid_run(c, *E.prm, Y, E.N, 1);
    if (rc) { E.rc = rc; return INFINITY; }
    const double *res = c->h_mid + Y.h_res;
    std::memcpy(g, res + 1, (size_t)n * sizeof(double));
    return res[0];
}

}  // namespace

extern "C" void isdf_midend_params_default(isdf_midend_params *p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    const isdf_host::MidendParams d;
    isdf_config cfg;
    isdf_config_default(&cfg);
    p->weight_pr = d.weight_pr; p->rho_mid_end = d.rho; p->rel_cost_tol = d.rel_cost_tol; p->min_step = d.min_step; p->g_epsilon = d.g_epsilon;
    p->integral_intervs = cfg.integral_intervs; p->mem_size = d.mem_size; p->past = d.past;
}

// OriTraj::costFunction (mid_end.hpp:262-304)
extern "C" int isdf_midend_cost(isdf_ctx *c, const isdf_midend_params *prm, const double *ref_points, const double *x, double *g, int n,
                                double *cost_out, double parts_out[3]) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    if (!ref_points || !x || !g || !cost_out) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "null argument");
    if (!c->have_traj) return isdf_fail(c, ISDF_ERR_STATE, "isdf_set_trajectory not called");
    const int N = c->minco.N;
    int rc = mid_check(c, prm, N);
    if (rc) return rc;
    if (n != N + 3 * (N - 1)) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "n must be N + 3(N-1)");
    if (!mid_on_device(c, N, false)) {
        c->mid_host.setup(c->cb_ends, c->cb_ends + 9, N, ref_points, host_params(*prm));
        *cost_out = c->mid_host.cost(x, g);
        if (parts_out) for (int k = 0; k < 3; k++) parts_out[k] = c->mid_host.parts[k];
        c->last_minco_path = 0;
        return ISDF_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    const MidLayout Y(N, 1);
    rc = mid_reserve(c, Y);
    if (rc) return rc;
    mid_put(c, Y, N, 0, x, c->cb_ends, c->cb_ends + 9, ref_points);
    rc = mid_run(c, *prm, Y, N, 1);
    if (rc) return rc;
    const double *res = c->h_mid + Y.h_res;
    *cost_out = res[0];
    std::memcpy(g, res + 1, (size_t)n * sizeof(double));
    if (parts_out) { parts_out[0] = res[1 + n]; parts_out[1] = res[1 + n + 2]; parts_out[2] = res[1 + n + 3]; }
    c->last_minco_path = 1;
    return ISDF_OK;
}

// the same for nb trajectories of the ctx's N pieces with their own boundary states: one launch, one workgroup per trajectory
extern "C" int isdf_midend_cost_batch(isdf_ctx *c, const isdf_midend_params *prm, int nb, const double *heads_pva, const double *tails_pva,
                                      const double *ref_points, const double *x, double *g, double *cost_out) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    if (nb < 1 || !heads_pva || !tails_pva || !ref_points || !x || !g || !cost_out) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "bad batch arguments");
    if (!c->have_traj) return isdf_fail(c, ISDF_ERR_STATE, "isdf_set_trajectory not called (it sets the batch's N)");
    const int N = c->minco.N;
    int rc = mid_check(c, prm, N);
    if (rc) return rc;
    const size_t n = (size_t)N + 3 * ((size_t)N - 1), nr = (size_t)3 * (N - 1);
    if (!mid_on_device(c, N, true)) {
        isdf_host::Midend m;
        for (int b = 0; b < nb; b++) {
            m.setup(heads_pva + 9 * (size_t)b, tails_pva + 9 * (size_t)b, N, ref_points + nr * b, host_params(*prm));
            cost_out[b] = m.cost(x + n * b, g + n * b);
        }
        c->last_minco_path = 0;
        return ISDF_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    const MidLayout Y(N, nb);
    rc = mid_reserve(c, Y);
    if (rc) return rc;
    for (int b = 0; b < nb; b++) mid_put(c, Y, N, b, x + n * b, heads_pva + 9 * (size_t)b, tails_pva + 9 * (size_t)b, ref_points + nr * b);
    rc = mid_run(c, *prm, Y, N, nb);
    if (rc) return rc;
    for (int b = 0; b < nb; b++) {
        const double *res = c->h_mid + Y.h_res + (size_t)b * Y.rs;
        cost_out[b] = res[0];
        std::memcpy(g + n * b, res + 1, n * sizeof(double));
    }
    c->last_minco_path = 1;
    return ISDF_OK;
}

// OriTraj::getOriTraj (mid_end.cpp:3-94)
extern "C" int isdf_midend_fit(isdf_ctx *c, const isdf_midend_params *prm, const double *ref_points, const double *T_init, double *x_out,
                               double *T_out, double *coeffs_out, isdf_lbfgs_result *out) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    if (!ref_points || !T_init || !x_out || !out) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "null argument");
    if (!c->have_traj) return isdf_fail(c, ISDF_ERR_STATE, "isdf_set_trajectory not called");
    const int N = c->minco.N;
    int rc = mid_check(c, prm, N);
    if (rc) return rc;
    for (int i = 0; i < N; i++) if (!(T_init[i] > 0.0)) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "durations must be positive");
    isdf_host::Midend &m = c->mid_host;
    m.setup(c->cb_ends, c->cb_ends + 9, N, ref_points, host_params(*prm));
    m.seed(T_init, x_out);                                  // (mid_end.cpp:27-41)
    const bool dev = mid_on_device(c, N, false);
    MidDevEval E{c, prm, ref_points, N, ISDF_OK};
    if (dev) {
        HIPCHK(c, hipSetDevice(c->device));
        rc = mid_reserve(c, MidLayout(N, 1));
        if (rc) return rc;
    }
    c->last_minco_path = dev ? 1 : 0;
    const auto t0 = std::chrono::steady_clock::now();
    const isdf_host::LbfgsResult r = dev ? m.fit(x_out, mid_dev_evaluate, &E, c->progress, c->progress_instance)
                                         : m.fit(x_out, isdf_host::Midend::evaluate, &m, c->progress, c->progress_instance);
    const auto t1 = std::chrono::steady_clock::now();
    out->f = r.f; out->status = r.status; out->iterations = r.iterations; out->evaluations = r.evaluations; out->reserved = 0;
    out->wall_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    if (E.rc) return E.rc;
    // the trajectory of the returned iterate, whatever the status (mid_end.cpp:65-92)
    if (T_out || coeffs_out) {
        std::vector<double> T((size_t)N);
        for (int i = 0; i < N; i++) T[i] = isdf_host::tau_to_T(x_out[i]);
        if (T_out) std::memcpy(T_out, T.data(), (size_t)N * sizeof(double));
        if (coeffs_out) { m.minco.set_parameters(x_out + N, T.data()); std::memcpy(coeffs_out, m.minco.c.data(), (size_t)18 * N * sizeof(double)); }
    }
    return ISDF_OK;
}

// ---- a batch of fits: the worker / coordinator shape of csrc/batch_opt.hip without its slots - a mid-end round is one small launch,
// so nothing overlaps it: every trajectory runs the driver on its own host thread, a round starts when EVERY live trajectory waits
// (every round is full) and is one launch with one workgroup per live trajectory.
namespace {

struct MidBatch {
    isdf_ctx *ctx = nullptr;
    const isdf_midend_params *prm = nullptr;
    int nb = 0, N = 0; size_t n = 0, rs = 0;
    bool dev = false;
    const double *heads = nullptr, *tails = nullptr, *ref = nullptr, *T_init = nullptr;
    double *x_out = nullptr;
    std::vector<isdf_host::LbfgsResult> results;
    std::mutex m;
    std::condition_variable cv_coord;
    std::unique_ptr<std::condition_variable[]> cv_worker;
    std::vector<char> waiting, ready;
    int n_waiting = 0, live = 0, next = 0, error = ISDF_OK;
    std::vector<double> stage_x, stage_res;
    long long rounds = 0;
    isdf_progress_fn progress = nullptr; void *progress_instance = nullptr; size_t progress_stride = 0;
};
struct MidWorker { MidBatch *b; int t; };

double mid_batch_evaluate(void *instance, const double *x, double *g, const int n) {
    MidWorker &w = *(MidWorker *)instance;
    MidBatch &b = *w.b;
    std::memcpy(b.stage_x.data() + (size_t)w.t * b.n, x, (size_t)n * sizeof(double));
    {
        std::unique_lock<std::mutex> lk(b.m);
        b.waiting[w.t] = 1;
        b.n_waiting++;
        b.cv_coord.notify_one();
        b.cv_worker[w.t].wait(lk, [&] { return b.ready[w.t] != 0; });
        b.ready[w.t] = 0;
        if (b.error != ISDF_OK) return INFINITY;
    }
    const double *res = b.stage_res.data() + (size_t)w.t * b.rs;
    std::memcpy(g, res + 1, (size_t)n * sizeof(double));
    return res[0];
}

void mid_batch_thread(MidBatch *bp) {
    MidBatch &b = *bp;
    for (;;) {
        int t;
        {
            std::unique_lock<std::mutex> lk(b.m);
            if (b.next >= b.nb) { b.live--; b.cv_coord.notify_one(); return; }
            t = b.next++;
        }
        const size_t nr = (size_t)3 * (b.N - 1);
        isdf_host::Midend m;
        m.setup(b.heads + 9 * (size_t)t, b.tails + 9 * (size_t)t, b.N, b.ref + nr * t, host_params(*b.prm));
        double *x = b.x_out + b.n * t;
        m.seed(b.T_init + (size_t)b.N * t, x);
        MidWorker w{&b, t};
        void *pi = b.progress ? (void *)((char *)b.progress_instance + (size_t)t * b.progress_stride) : nullptr;
        b.results[t] = b.dev ? m.fit(x, mid_batch_evaluate, &w, b.progress, pi) : m.fit(x, isdf_host::Midend::evaluate, &m, b.progress, pi);
    }
}

}  // namespace

extern "C" int isdf_midend_fit_batch(isdf_ctx *c, const isdf_midend_params *prm, int nb, int N, const double *heads_pva, const double *tails_pva,
                                     const double *ref_points, const double *T_init, double *x_out, isdf_lbfgs_result *results, double *wall_ms_out) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    if (nb < 1 || !heads_pva || !tails_pva || !ref_points || !T_init || !x_out || !results) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "bad batch arguments");
    int rc = mid_check(c, prm, N);
    if (rc) return rc;
    for (size_t i = 0; i < (size_t)nb * N; i++) if (!(T_init[i] > 0.0)) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "durations must be positive");
    MidBatch b;
    b.ctx = c; b.prm = prm; b.nb = nb; b.N = N; b.n = (size_t)N + 3 * ((size_t)N - 1);
    b.dev = mid_on_device(c, N, true);
    b.heads = heads_pva; b.tails = tails_pva; b.ref = ref_points; b.T_init = T_init; b.x_out = x_out;
    b.results.resize(nb);
    b.progress = c->progress; b.progress_instance = c->progress_instance; b.progress_stride = c->progress_stride;
    const MidLayout Yall(N, nb);
    b.rs = Yall.rs;
    if (b.dev) {
        HIPCHK(c, hipSetDevice(c->device));
        rc = mid_reserve(c, Yall);
        if (rc) return rc;
        b.cv_worker.reset(new std::condition_variable[nb]);
        b.waiting.assign(nb, 0); b.ready.assign(nb, 0);
        b.stage_x.assign((size_t)nb * b.n, 0.0); b.stage_res.assign((size_t)nb * b.rs, 0.0);
    }
    c->last_minco_path = b.dev ? 1 : 0;
    // live host threads: one per trajectory, like isdf_optimize_lbfgs_batch, unless ISDF_BATCH_THREADS caps them (a finished
    // trajectory's thread takes the next one)
    int n_threads = nb;
    if (const char *e = getenv("ISDF_BATCH_THREADS")) { const int v = atoi(e); if (v >= 1 && v < n_threads) n_threads = v; }
    b.live = n_threads;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<std::thread> threads;
    threads.reserve(n_threads);
    for (int k = 0; k < n_threads; k++) threads.emplace_back(mid_batch_thread, &b);
    if (b.dev) {
        const size_t nr = (size_t)3 * (N - 1);
        std::vector<int> active;
        for (;;) {
            {
                std::unique_lock<std::mutex> lk(b.m);
                b.cv_coord.wait(lk, [&] { return b.live == 0 || b.n_waiting == b.live; });
                if (b.live == 0) break;
                active.clear();
                for (int t = 0; t < nb; t++) if (b.waiting[t]) { active.push_back(t); b.waiting[t] = 0; }
                b.n_waiting = 0;
            }
            const int na = (int)active.size();
            const MidLayout Y(N, na);             // (within the reserved Yall: na <= nb)
            if (rc == ISDF_OK) {
                for (int k = 0; k < na; k++) {
                    const int t = active[k];
                    mid_put(c, Y, N, k, b.stage_x.data() + b.n * t, heads_pva + 9 * (size_t)t, tails_pva + 9 * (size_t)t, ref_points + nr * t);
                }
                rc = mid_run(c, *prm, Y, N, na);
                b.rounds++;
            }
            if (rc == ISDF_OK)
                for (int k = 0; k < na; k++)
                    std::memcpy(b.stage_res.data() + (size_t)active[k] * b.rs, c->h_mid + Y.h_res + (size_t)k * Y.rs, b.rs * sizeof(double));
            std::unique_lock<std::mutex> lk(b.m);
            if (rc != ISDF_OK) b.error = rc;
            for (int t : active) { b.ready[t] = 1; b.cv_worker[t].notify_one(); }
        }
    }
    for (auto &th : threads) th.join();
    const double wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    for (int t = 0; t < nb; t++) {
        const isdf_host::LbfgsResult &r = b.results[t];
        results[t].f = r.f; results[t].status = r.status; results[t].iterations = r.iterations; results[t].evaluations = r.evaluations;
        results[t].wall_ms = wall; results[t].reserved = (int32_t)b.rounds;
    }
    if (wall_ms_out) *wall_ms_out = wall;
    if (b.error != ISDF_OK) return isdf_fail(c, b.error, "a device round of the batched mid end failed");
    return ISDF_OK;
}
