// The full objective callback of the C ABI (host-MINCO and device-MINCO forms, whole and split) and the L-BFGS drivers behind it.
#include "isdf_ctx.hpp"
#include "minco_dev.hpp"
#include "lbfgs_host.hpp"
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

using namespace isdf;

// --------------------------------------------------------------------------------------------------------------
// full objective callback: TrajOptimizer::costFunctionLmbm (back_end_optimizer.hpp:358-430)
// --------------------------------------------------------------------------------------------------------------
extern "C" int isdf_set_trajectory(isdf_ctx *c, int N, const double head_pva[9], const double tail_pva[9], double rho) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    if (N < 1 || !head_pva || !tail_pva) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "bad trajectory setup");
    c->minco.set_conditions(head_pva, tail_pva, N);
    c->rho = rho;
    c->have_traj = true;
    std::memcpy(c->cb_ends, head_pva, 9 * sizeof(double)); std::memcpy(c->cb_ends + 9, tail_pva, 9 * sizeof(double));
    c->cb_ends_dirty = true;
    c->cb_T.assign(N, 0.0); c->cb_gdC.assign((size_t)18 * N, 0.0); c->cb_gdT.assign(N, 0.0);
    c->cb_gradP.assign((size_t)3 * (N > 1 ? N - 1 : 1), 0.0); c->cb_gradT.assign(N, 0.0);
    return ISDF_OK;
}

extern "C" int isdf_num_variables(const isdf_ctx *c) { return (c && c->have_traj) ? c->minco.N + 3 * (c->minco.N - 1) : 0; }

// x = [tau(N) | waypoints 3(N-1)]: backwardT / backwardP of optimize_traj_lmbm (back_end_optimizer.cpp:22-28)
extern "C" int isdf_pack_variables(isdf_ctx *c, const double *T, const double *waypoints, double *x) {
    if (!c || !T || !x) return ISDF_ERR_INVALID_ARG;
    if (!c->have_traj) return isdf_fail(c, ISDF_ERR_STATE, "isdf_set_trajectory not called");
    const int N = c->minco.N;
    if (N > 1 && !waypoints) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "null waypoints");
    for (int i = 0; i < N; i++) {
        if (!(T[i] > 0.0)) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "durations must be positive");
        x[i] = isdf_host::T_to_tau(T[i]);
    }
    for (int i = 0; i < 3 * (N - 1); i++) x[N + i] = waypoints[i];
    return ISDF_OK;
}

// forwardT / forwardP + minco.setParameters: the trajectory x stands for (T: N, coeffs: 6N x 3 column-major)
extern "C" int isdf_unpack_variables(isdf_ctx *c, const double *x, double *T, double *coeffs) {
    if (!c || !x) return ISDF_ERR_INVALID_ARG;
    if (!c->have_traj) return isdf_fail(c, ISDF_ERR_STATE, "isdf_set_trajectory not called");
    const int N = c->minco.N;
    for (int i = 0; i < N; i++) c->cb_T[i] = isdf_host::tau_to_T(x[i]);
    c->minco.set_parameters(x + N, c->cb_T.data());
    if (T) std::memcpy(T, c->cb_T.data(), (size_t)N * sizeof(double));
    if (coeffs) std::memcpy(coeffs, c->minco.c.data(), (size_t)18 * N * sizeof(double));
    return ISDF_OK;
}

// First half of the callback: tau -> T, MINCO, energy, and the sweeps queued on `st`.  Leaves this rank's partial sums
// ([cost | gradT | gradC] per sweep, cb_n_out blocks) in c->d_cb + 19N on the device.
// ---- the callback with its MINCO half on the device (csrc/minco_dev.hip): x goes down (through the PCIe BAR when the host can
// write device memory, else the first kernel fetches it from host-mapped memory), cb_pre_kernel writes (T, coefficients) where
// the sweeps read them, the sweeps accumulate as ever, cb_post_kernel leaves (cost, g, the four cost parts) and a completion
// word in host-mapped memory.  No copy commands, no stream synchronisation.
static size_t cb_res_stride(int N) { return (size_t)1 + (size_t)(N + 3 * (N - 1)) + 4; }
static int cb_dev_fill(isdf_ctx *c, int N, CbDev *P, hipStream_t st) {
    const size_t nvar = (size_t)N + 3 * (size_t)(N - 1), ostride = isdf_out_stride(N), in_len = (size_t)19 * N;
    // device: [x | ends | u | energy block]
    const size_t off_ends = nvar, off_u = off_ends + 18, off_e = off_u + (size_t)6 * (N + 1);
    const size_t need = off_e + ostride;
    if (c->d_cbdev.capacity() < need) { c->cb_ends_dirty = true; }
    int rc = c->d_cbdev.reserve(c, need);
    if (rc) return rc;
    rc = c->d_cb.reserve(c, in_len + 2 * ostride);
    if (rc) return rc;
    const size_t rs = cb_res_stride(N), pin_need = nvar + rs + 2;
    rc = c->h_cbres.reserve(c, pin_need);
    if (rc) return rc;
    if (c->cb_ends_dirty) {
        HIPCHK(c, hipMemcpyAsync(c->d_cbdev + off_ends, c->cb_ends, 18 * sizeof(double), hipMemcpyHostToDevice, st));
        HIPCHK(c, hipStreamSynchronize(st));            // (cb_ends may change before an asynchronous copy has read it)
        c->cb_ends_dirty = false;
    }
    P->N = N; P->nb = 1; P->n_out = c->cb_n_out; P->res_stride = (int)rs;
    P->x = c->d_cbdev; P->ends = c->d_cbdev + off_ends; P->u = c->d_cbdev + off_u; P->epart = c->d_cbdev + off_e;
    P->T = c->d_cb; P->coeffs = c->d_cb + N; P->sweep = c->d_cb + in_len;
    P->rho = c->rho;
    P->res = c->h_cbres.dev() + nvar; P->flag = (unsigned long long *)(c->h_cbres.dev() + nvar + rs);
    P->seq = c->cb_seq; P->stats = c->d_stats;
    return ISDF_OK;
}
// Where a callback's MINCO half runs.  Forced either way by isdf_set_minco_mode; left to itself (mode 0) the device takes it unless
// the step is the small single-trajectory kind whose sweep is one fused host-direct launch (C2: N <= 64, one GPU, tile sweep) -
// there the host's band LU (10 us at N = 40, growing with N) still beats two more kernels either side of a 16 us launch
// (measured: 35 us against 38; profiles/r5_callback_bench.txt), everywhere else the device form is the faster one
// (N = 400: 135 us against 216; swept-volume ctx; the batched optimiser's rounds).
static bool cb_device_minco(const isdf_ctx *c) {
    if (!c->have_traj || c->minco.N > CB_MAX_N || c->prof_on || c->minco_mode == 1) return false;
    if (c->minco_mode == 2) return true;
    const bool small_fused = c->cfg.variant != ISDF_V1_SWEPT && direct_enabled(c) && c->peers.empty() && c->minco.N <= CB_AUTO_HOST_MAX_N;
    return !small_fused;
}

// the callback's sweeps queued on `st`: a swept-volume ctx runs that sweep and the integral sweep without its collision term (their
// sums next to each other in d_o, cb_n_out = 2), every other ctx the sweep its variant names
static int cb_queue_sweeps(isdf_ctx *c, int N, const double *d_T, const double *d_C, double *d_o, hipStream_t st) {
    if (c->cfg.variant != ISDF_V1_SWEPT) return sweep_dispatch(c, 1, N, d_T, d_C, d_o, nullptr, st, 0);
    const int rc = sweep_dispatch(c, 1, N, d_T, d_C, d_o, nullptr, st, 1);
    return rc ? rc : sweep_dispatch(c, 1, N, d_T, d_C, d_o + isdf_out_stride(N), nullptr, st, 2);
}

static int cost_function_launch_dev(isdf_ctx *c, const double *x, int n, hipStream_t st, bool whole) {
    const int N = c->minco.N;
    const bool swept = c->cfg.variant == ISDF_V1_SWEPT;
    c->cb_n_out = swept ? 2 : 1;
    c->cb_direct = false; c->cb_dev = true; c->cb_post_queued = false;
    c->cb_seq = ++c->dir_seq;          // (one counter with the host-direct steps: they share the staging buffer's ready flags)
    CbDev P{};
    int rc = cb_dev_fill(c, N, &P, st);
    if (rc) return rc;
    const size_t nvar = (size_t)n;
    if (bar_usable(c, c->d_cbdev, nvar)) std::memcpy(c->d_cbdev, x, nvar * sizeof(double));      // CPU stores into device memory
    else { std::memcpy(c->h_cbres, x, nvar * sizeof(double)); P.x = c->h_cbres.dev(); }
    host_rows_mark(c->h_cbres + nvar, cb_res_stride(N));
    __sync_synchronize();
    double *d_T = c->d_cb, *d_C = c->d_cb + N, *d_o = c->d_cb + (size_t)19 * N;
    launch_cb_pre(P, st);
    rc = cb_queue_sweeps(c, N, d_T, d_C, d_o, st);
    if (rc) return rc;
    if (whole) { launch_cb_post(P, st); c->cb_post_queued = true; }      // the split form queues it in _finish, behind the caller's all-reduce
    HIPCHK(c, hipGetLastError());
    c->last_host_path = ISDF_HOST_PATH_DEVICE_CALLBACK;
    c->last_minco_path = 1;
    c->cb_pending = true;
    return ISDF_OK;
}
static int cost_function_finish_dev(isdf_ctx *c, double *g, double *cost_out, hipStream_t st) {
    c->cb_pending = false;
    const int N = c->minco.N;
    const size_t nvar = (size_t)N + 3 * (size_t)(N - 1), rs = cb_res_stride(N);
    if (!c->cb_post_queued) {
        CbDev P{};
        ISDF_TRY(cb_dev_fill(c, N, &P, st));
        if (!bar_usable(c, c->d_cbdev, nvar)) P.x = c->h_cbres.dev();
        launch_cb_post(P, st);
        HIPCHK(c, hipGetLastError());
    }
    volatile unsigned long long *flag = (volatile unsigned long long *)(c->h_cbres + nvar + rs);
    const auto t0 = std::chrono::steady_clock::now();
    unsigned long long f;
    if (!host_flag_wait(flag, c->cb_seq, HOST_FLAG_OVERFLOW, t0, 5.0, st, &f))
        return isdf_fail(c, ISDF_ERR_HIP, "device callback did not complete (its completion word never arrived)");
    std::atomic_thread_fence(std::memory_order_acquire);
    if (f & HOST_FLAG_OVERFLOW) {
        (void)clear_overflow(c);
        return isdf_fail(c, ISDF_ERR_OVERFLOW, "a bounded device work list overflowed; result invalid");
    }
    const double *res = c->h_cbres + nvar;
    if (!host_rows_wait(c, res, rs)) {
        (void)hipStreamSynchronize(st);
        return isdf_fail(c, ISDF_ERR_HIP, "device callback: its completion word arrived but not all of its results");
    }
    *cost_out = res[0];
    std::memcpy(g, res + 1, nvar * sizeof(double));
    for (int q = 0; q < 4; q++) c->last_parts[q] = res[1 + nvar + q];
    return ISDF_OK;
}

static int cost_function_launch(isdf_ctx *c, const double *x, int n, hipStream_t st, bool allow_direct = false) {
    if (!x) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "null argument");
    if (!c->have_traj) return isdf_fail(c, ISDF_ERR_STATE, "isdf_set_trajectory not called");
    const int N = c->minco.N;
    if (n != N + 3 * (N - 1)) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "n must be N + 3(N-1)");
    HIPCHK(c, hipSetDevice(c->device));
    if (cb_device_minco(c)) return cost_function_launch_dev(c, x, n, st, allow_direct);
    c->cb_dev = false; c->last_minco_path = 0;
    // tau -> T, xi -> waypoints, MINCO coefficients, energy and its partials (:363-381)
    c->cb_x.assign(x, x + n);
    for (int i = 0; i < N; i++) c->cb_T[i] = isdf_host::tau_to_T(x[i]);
    c->minco.set_parameters(x + N, c->cb_T.data());
    c->cb_energy = c->minco.energy(c->cb_gdC.data(), c->cb_gdT.data());
    // the two sweeps on the device (:386-405)
    const size_t in_len = (size_t)19 * N, ostride = isdf_out_stride(N);
    const bool swept = c->cfg.variant == ISDF_V1_SWEPT;
    c->cb_n_out = swept ? 2 : 1;
    c->cb_direct = false;
    if (allow_direct && !swept && direct_enabled(c)) {
        // one launch that reads (T, coefficients) from host-mapped memory and writes the sums back into it: no copy commands,
        // no stream synchronisation (csrc/tile_sweep.hip, host-direct step)
        const double *Tp = c->cb_T.data(), *Cp = c->minco.c.data();
        const int rcd = direct_launch(c, 1, N, &Tp, &Cp, 0, st, 0);
        if (rcd < 0) return rcd;
        if (rcd == ISDF_OK) { c->cb_direct = true; c->cb_pending = true; return ISDF_OK; }
    }
    c->last_host_path = ISDF_HOST_PATH_COPY;
    const size_t need = in_len + c->cb_n_out * ostride;
    { const int rc0 = c->h_pin.reserve(c, need); if (rc0) return rc0; }
    int rc = c->d_cb.reserve(c, need);
    if (rc) return rc;
    std::memcpy(c->h_pin, c->cb_T.data(), (size_t)N * sizeof(double));
    std::memcpy(c->h_pin + N, c->minco.c.data(), (size_t)18 * N * sizeof(double));
    HIPCHK(c, hipMemcpyAsync(c->d_cb, c->h_pin, in_len * sizeof(double), hipMemcpyHostToDevice, st));
    double *d_T = c->d_cb, *d_C = c->d_cb + N, *d_o = c->d_cb + in_len;
    rc = cb_queue_sweeps(c, N, d_T, d_C, d_o, st);
    if (rc) return rc;
    c->cb_pending = true;
    return ISDF_OK;
}

// Second half: download the (all-reduced) sums, add them in the reference's order, propagateGrad, time term, chain rule.
static int cost_function_finish(isdf_ctx *c, double *g, double *cost_out, hipStream_t st) {
    if (!g || !cost_out) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "null argument");
    if (!c->cb_pending) return isdf_fail(c, ISDF_ERR_STATE, "no callback evaluation in flight");
    if (c->cb_dev) { HIPCHK(c, hipSetDevice(c->device)); return cost_function_finish_dev(c, g, cost_out, st); }
    c->cb_pending = false;
    const int N = c->minco.N;
    const size_t in_len = (size_t)19 * N, ostride = isdf_out_stride(N);
    const int n_out = c->cb_n_out;
    const bool swept = n_out == 2;
    const double *res = nullptr;
    if (c->cb_direct) {
        bool ovf = false;
        const int rcd = direct_wait(c, st, &ovf);
        if (rcd) return rcd;
        if (ovf) {
            (void)clear_overflow(c);
            return isdf_fail(c, ISDF_ERR_OVERFLOW, "a bounded device work list overflowed; result invalid");
        }
        res = c->h_dir + c->dir_in;
    } else {
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, hipMemcpyAsync(c->h_pin + in_len, c->d_cb + in_len, n_out * ostride * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        res = c->h_pin + in_len;
    }
    double cost = c->cb_energy;
    double part[2] = {0.0, 0.0};
    for (int k = 0; k < n_out; k++) {       // swept-volume sweep first, then the integral sweep (:386-405)
        const double *o = res + k * ostride;
        cost += o[0];
        part[k] = o[0];
        for (int i = 0; i < N; i++) c->cb_gdT[i] += o[1 + i];
        for (int i = 0; i < 18 * N; i++) c->cb_gdC[i] += o[1 + N + i];
    }
    // dCost/d(c, T) -> dCost/d(waypoints, T) (:416), time regulariser (:417-420), chain rule to (tau, xi) (:426-427)
    c->minco.propagate_grad(c->cb_gdC.data(), c->cb_gdT.data(), c->cb_gradP.data(), c->cb_gradT.data());
    double tsum = 0.0;
    for (int i = 0; i < N; i++) tsum += c->cb_T[i];
    cost += c->rho * tsum;
    for (int i = 0; i < N; i++) g[i] = isdf_host::grad_T_to_tau(c->cb_x[i], c->cb_gradT[i] + c->rho);
    for (int i = 0; i < 3 * (N - 1); i++) g[N + i] = c->cb_gradP[i];
    c->last_parts[0] = c->cb_energy;
    c->last_parts[1] = swept ? part[0] : 0.0;            // swept-volume sweep
    c->last_parts[2] = swept ? part[1] : part[0];        // integral sweep
    c->last_parts[3] = c->rho * tsum;
    *cost_out = cost;
    return ISDF_OK;
}

extern "C" int isdf_cost_function(isdf_ctx *c, const double *x, double *g, int n, double *cost_out) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    if (!x || !g || !cost_out) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "null argument");
    // a sharded ctx returns only this rank's partial sums from the sweeps: the un-split callback (and the drivers built on it)
    // would optimise on them without any error - the split form (_launch / all-reduce / _finish) is the one to use
    if (c->world > 1 && c->peers.empty() && !isdf_xchg_fuse_on(c))
        return isdf_fail(c, ISDF_ERR_STATE, "sharded ctx: use isdf_cost_function_launch / _finish around the all-reduce (or switch the in-kernel exchange on)");
    ISDF_TRY(cost_function_launch(c, x, n, c->stream, true));
    return cost_function_finish(c, g, cost_out, c->stream);
}

// Multi-GPU form (one process per GPU, isdf_set_shard): _launch queues this rank's share of the sweeps on `stream` and
// hands back the device buffer of partial sums; the caller sums it over the ranks IN PLACE on the same stream (one
// all-reduce, RCCL); _finish then yields the same (cost, g) on every rank.
extern "C" int isdf_cost_function_launch(isdf_ctx *c, const double *x, int n, void *stream, double **d_partial_out, size_t *count_out) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    if (!d_partial_out || !count_out) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "null argument");
    ISDF_TRY(cost_function_launch(c, x, n, (hipStream_t)stream));
    *d_partial_out = c->d_cb + (size_t)19 * c->minco.N;       // (both MINCO paths keep the sweeps' sums here)
    *count_out = (size_t)c->cb_n_out * isdf_out_stride(c->minco.N);
    return ISDF_OK;
}
extern "C" int isdf_cost_function_finish(isdf_ctx *c, double *g, double *cost_out, void *stream) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    return cost_function_finish(c, g, cost_out, (hipStream_t)stream);
}

// Same callback with the signature LMBM / the optimizer drivers bind (lmbm_evaluate_t, lmbm.h:206-209):
// instance = isdf_ctx*.  Errors surface as +infinity (the reference has no error channel here).
extern "C" double isdf_cost_function_lmbm(void *instance, const double *x, double *g, const int n) {
    double cost = 0.0;
    const int rc = isdf_cost_function((isdf_ctx *)instance, x, g, n, &cost);
    return rc == ISDF_OK ? cost : INFINITY;
}

// where MINCO runs: 0 = wherever it is faster (cb_device_minco), 1 = on the host (band LU, the reference's elimination order bit
// for bit), 2 = on the device whenever the trajectory fits (N <= 400).  Results agree to rounding (1e-10 relative on the coefficients).
extern "C" int isdf_set_minco_mode(isdf_ctx *c, int mode) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    if (mode < 0 || mode > 2) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "minco mode must be 0 (auto), 1 (host) or 2 (device)");
    if (c->cb_pending) return isdf_fail(c, ISDF_ERR_STATE, "a callback evaluation is in flight");
    c->minco_mode = mode;
    return ISDF_OK;
}
extern "C" int isdf_minco_path(const isdf_ctx *c) { return c ? c->last_minco_path : ISDF_ERR_INVALID_ARG; }

// energy | swept-volume sweep | integral sweep | rho * sum(T) of the last isdf_cost_function call
extern "C" int isdf_cost_parts(const isdf_ctx *c, double parts[4]) {
    if (!c || !parts) return ISDF_ERR_INVALID_ARG;
    for (int k = 0; k < 4; k++) parts[k] = c->last_parts[k];
    return ISDF_OK;
}

// --------------------------------------------------------------------------------------------------------------
// optimizer driver: L-BFGS behind the callback (lbfgs::lbfgs_optimize, src/utils/include/utils/lbfgs.hpp:480-835)
// --------------------------------------------------------------------------------------------------------------
// isdf_lbfgs_params (the ABI's) <-> isdf_host::LbfgsParams (the driver's): the same fields under the same names, either way
template <class From, class To> static void lbfgs_params_copy(const From &a, To &b) {
    b.mem_size = a.mem_size; b.past = a.past; b.max_iterations = a.max_iterations; b.max_linesearch = a.max_linesearch;
    b.weak_wolfe = a.weak_wolfe; b.reference_patches = a.reference_patches;
    b.g_epsilon = a.g_epsilon; b.delta = a.delta; b.min_step = a.min_step; b.max_step = a.max_step;
    b.f_dec_coeff = a.f_dec_coeff; b.s_curv_coeff = a.s_curv_coeff; b.cautious_factor = a.cautious_factor;
    b.machine_prec = a.machine_prec; b.dir_norm_cap = a.dir_norm_cap;
}

extern "C" void isdf_lbfgs_params_default(isdf_lbfgs_params *p) {
    if (!p) return;
    lbfgs_params_copy(isdf_host::LbfgsParams(), *p);
}

static int lbfgs_run(isdf_evaluate_fn evaluate, void *instance, isdf_progress_fn progress, void *progress_instance, double *x_inout, int n,
                     const isdf_lbfgs_params *p, isdf_lbfgs_result *out) {
    if (!evaluate || !x_inout || !p || !out) return ISDF_ERR_INVALID_ARG;
    isdf_host::Lbfgs opt;
    lbfgs_params_copy(*p, opt.param);
    opt.evaluate = evaluate;
    opt.instance = instance;
    opt.progress = progress;                  // (isdf_progress_fn == lbfgs_host's lbfgs_progress_fn: lbfgs_progress_t with plain pointers)
    opt.progress_instance = progress_instance;
    const auto t0 = std::chrono::steady_clock::now();
    const isdf_host::LbfgsResult r = opt.minimize(x_inout, n);
    const auto t1 = std::chrono::steady_clock::now();
    out->f = r.f; out->status = r.status; out->iterations = r.iterations; out->evaluations = r.evaluations;
    out->wall_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    return ISDF_OK;
}

extern "C" int isdf_lbfgs_minimize(isdf_evaluate_fn evaluate, void *instance, double *x_inout, int n,
                                   const isdf_lbfgs_params *p, isdf_lbfgs_result *out) {
    return lbfgs_run(evaluate, instance, nullptr, nullptr, x_inout, n, p, out);
}
// ... with the reference's progress / cancel callback (lbfgs_optimize's proc_progress, lbfgs.hpp:256-262,480-492): called once per
// iteration with the SAME instance as evaluate; non-zero return -> status LBFGS_CANCELED (2), x_inout = the iterate it was shown
extern "C" int isdf_lbfgs_minimize_progress(isdf_evaluate_fn evaluate, isdf_progress_fn progress, void *instance, double *x_inout, int n,
                                            const isdf_lbfgs_params *p, isdf_lbfgs_result *out) {
    return lbfgs_run(evaluate, instance, progress, nullptr, x_inout, n, p, out);
}

extern "C" int isdf_set_progress(isdf_ctx *c, isdf_progress_fn progress, void *instance, size_t batch_instance_stride) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    c->progress = progress; c->progress_instance = instance; c->progress_stride = batch_instance_stride;
    return ISDF_OK;
}

extern "C" int isdf_optimize_lbfgs(isdf_ctx *c, double *x_inout, int n, const isdf_lbfgs_params *p, isdf_lbfgs_result *out) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    if (!x_inout || !p || !out) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "null argument");
    if (!c->have_traj) return isdf_fail(c, ISDF_ERR_STATE, "isdf_set_trajectory not called");
    if (n != isdf_num_variables(c)) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "n must be N + 3(N-1)");
    return lbfgs_run(isdf_cost_function_lmbm, c, c->progress, c->progress_instance, x_inout, n, p, out);
}

// --------------------------------------------------------------------------------------------------------------
// lazy constraint generation: optimise, check the result against the whole map, merge what the check found into the point set
// (where plan_manager.cpp:306-309 only warns), again
// --------------------------------------------------------------------------------------------------------------
extern "C" void isdf_refine_params_default(isdf_refine_params *p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->max_rounds = 4;
    p->mode = ISDF_SWEPT_FIELD_PLANNER;
    p->margin = -1.0;                       // negative: cfg.safety_hor of the ctx
    p->below = -1.0;                        // negative: every kept row
}

extern "C" int isdf_optimize_lbfgs_checked(isdf_ctx *c, double *x_inout, int n, const isdf_lbfgs_params *lp,
                                           const isdf_refine_params *rp, isdf_refine_result *out) {
    isdf_refine_params dflt;
    isdf_refine_params_default(&dflt);
    const isdf_refine_params &R = rp ? *rp : dflt;
    // the arguments are checked before the ctx (reported through isdf_last_error(NULL) when there is none)
    if (R.max_rounds < 1) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "checked optimisation: max_rounds must be >= 1");
    if (R.mode != ISDF_SWEPT_FIELD_PLANNER && R.mode != ISDF_SWEPT_FIELD_CLOSED) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "checked optimisation: unknown mode");
    if (!std::isfinite(R.margin)) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "checked optimisation: margin must be finite");
    if (!std::isfinite(R.below)) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "checked optimisation: below must be finite");
    if (!c) return isdf_fail(nullptr, ISDF_ERR_INVALID_ARG, "checked optimisation: null ctx");
    if (!x_inout || !lp || !out) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "null argument");
    if (c->cfg.variant != ISDF_V1_SWEPT) return isdf_fail(c, ISDF_ERR_UNSUPPORTED, "checked optimisation: the obstacle-point set belongs to the swept-volume variant (V1)");
    if (!c->have_traj) return isdf_fail(c, ISDF_ERR_STATE, "isdf_set_trajectory not called");
    if (!c->have_geom || !c->d_occ)
        return isdf_fail(c, ISDF_ERR_STATE, "trajectory check: no occupancy grid (isdf_set_grid with ISDF_GRID_OCCUPANCY, or isdf_set_pointcloud)");
    std::memset(out, 0, sizeof(*out));
    const int N = c->minco.N;
    std::vector<double> T((size_t)N), coeffs((size_t)18 * N);
    isdf_traj_check_params cp;
    isdf_traj_check_params_default(&cp);
    cp.margin = R.margin; cp.mode = R.mode;
    for (int round = 0; round < R.max_rounds; round++) {
        if (round < 16) out->M_round[round] = c->M;
        out->rounds = round + 1;
        int rc = isdf_optimize_lbfgs(c, x_inout, n, lp, &out->last_opt);
        if (rc) return rc;
        rc = isdf_unpack_variables(c, x_inout, T.data(), coeffs.data());
        if (rc) return rc;
        rc = isdf_traj_check(c, N, T.data(), coeffs.data(), &cp, &out->last_check, nullptr);
        if (rc) return rc;
        if (out->last_check.n_below_margin == 0) { out->clear = 1; break; }
        isdf_points_merge_info mi;
        rc = isdf_points_merge_check(c, R.below, &mi);
        if (rc) return rc;
        if (mi.n_added == 0) { out->stalled = 1; break; }
    }
    return ISDF_OK;
}
