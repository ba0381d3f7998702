// Host-array entry points of the C ABI (isdf_eval, isdf_eval_swept_at_tstar_host) and the ways a step's inputs and results cross
// PCIe without copy commands: the host-direct step, the swept-volume step's publish kernel, the multi-device sum's host output.
#include "isdf_ctx.hpp"
#include <atomic>
#include <chrono>
#include <cstring>
#include <vector>

using namespace isdf;

// ---- host-direct steps -----------------------------------------------------------------------------------------------
bool direct_enabled(const isdf_ctx *c) {
    return !c->env_no_direct && !c->prof_on && c->world == 1 && c->cfg.variant != ISDF_V1_SWEPT && c->cfg.enable_pos;
}
// pinned, device-mapped [inputs 19 n nb | outputs (1 + 19 n) nb | nb flags]
// Results that a kernel stores into host-mapped memory, and the completion word it stores after them, are separate PCIe writes issued
// by different wavefronts; "release, then the word" orders them for the DEVICE's view of memory, not for the order in which posted
// writes become visible to the CPU.  Observed on MI355X: the first host-direct step of a fresh ctx, about one process in twenty when two
// processes share the GPU - word and cost there, all gradient rows still the zeros of the fresh allocation, a wrong gradient returned
// without any flag (tests/native/xchg_fail_worker.py caught it as a "wrong" reference).  So the word only says the kernel is done:
// the result area is filled with a pattern no result can have (all ones: not the canonical NaN, not a count) before the launch, and
// after the word the host waits until none of it is left - normally a scan of a few hundred doubles that finds nothing.
void host_rows_mark(double *p, size_t n) { std::memset((void *)p, 0xFF, n * sizeof(double)); }
bool host_rows_wait(isdf_ctx *c, const double *p, size_t n, bool another_area_of_the_same_step) {
    const volatile unsigned long long *w = (const volatile unsigned long long *)p;
    if (!another_area_of_the_same_step) c->host_steps++;
    bool late = false;
    const auto t0 = std::chrono::steady_clock::now();
    for (size_t i = 0; i < n; i++) {
        for (unsigned spin = 0; w[i] == ~0ull; spin++) {
            late = true;
            c->host_late_spins++;
            if ((spin & 0x3FFFu) == 0x3FFFu && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 5.0) return false;
        }
    }
    if (late) { if (!another_area_of_the_same_step || c->host_late_mark != c->host_steps) { c->host_late++; c->host_late_mark = c->host_steps; } std::atomic_thread_fence(std::memory_order_acquire); }
    return true;
}

static int direct_reserve(isdf_ctx *c, int nb, int n) {
    const size_t in = (size_t)19 * n * nb, out = isdf_out_stride(n) * nb, need = in + out + (size_t)nb;
    ISDF_TRY(c->h_dir.reserve(c, need));      // pinned host memory is device-visible (unified addressing)
    c->dir_in = in; c->dir_out = out; c->dir_flags = (size_t)nb;
    return ISDF_OK;
}
// Can the host write device memory directly (large PCIe BAR)?  Verified once per ctx THE WAY THE STEPS USE IT: a kernel reads
// the buffer (its lines may now sit in an L2) and raises a host-mapped flag; the host, which waited for nothing but that flag,
// overwrites the buffer through the BAR and launches the kernel again without any host-side synchronisation in between; the
// second launch must see the second pattern (and the first launch the first).  Writes only - host READS over the BAR cost
// ~1 us per access.
__global__ void bar_probe_kernel(const double *buf, int m, double *copy, volatile unsigned long long *host_flag, unsigned long long seq) {
    for (int i = threadIdx.x; i < m; i += blockDim.x) copy[i] = buf[i];
    __syncthreads();
    if (threadIdx.x == 0) { __threadfence_system(); *host_flag = seq; }
}
bool bar_usable(isdf_ctx *c, double *d_buf, size_t n) {
    if (c->bar_state != 0) return c->bar_state > 0;
    c->bar_state = -1;
    if (c->env_no_bar) return false;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, c->device) != hipSuccess || !prop.isLargeBar) return false;
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, d_buf) != hipSuccess) { (void)hipGetLastError(); return false; }
    const int m = (int)(n < 64 ? n : 64);
    DevBuf<double> d_copy;
    PinBuf<unsigned long long> flag;
    bool ok = d_copy.alloc(2 * 64) == hipSuccess && flag.reserve(nullptr, 8) == ISDF_OK;
    unsigned long long *const h_flag = flag, *const h_flag_dev = flag.dev();
    std::vector<double> pat(2 * (size_t)m), back(2 * (size_t)m, 0.0);
    for (int i = 0; i < m; i++) { pat[i] = 1.0 + (double)i * 0.5; pat[m + i] = -3.0 - (double)i * 0.25; }
    for (int round = 0; ok && round < 2; round++) {
        *(volatile unsigned long long *)h_flag = 0ull;
        std::memcpy(d_buf, pat.data() + (size_t)round * m, (size_t)m * sizeof(double));          // CPU stores into device memory
        __sync_synchronize();
        hipLaunchKernelGGL(bar_probe_kernel, dim3(1), dim3(64), 0, c->stream, d_buf, m, d_copy + (size_t)round * 64, h_flag_dev, (unsigned long long)(round + 1));
        ok = hipGetLastError() == hipSuccess;
        const auto t0 = std::chrono::steady_clock::now();
        while (ok && *(volatile unsigned long long *)h_flag != (unsigned long long)(round + 1))       // the steps' own hand-over: no stream sync
            if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 2.0) ok = false;
    }
    if (ok) ok = hipMemcpy(back.data(), d_copy, (size_t)m * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess &&
                 hipMemcpy(back.data() + m, d_copy + 64, (size_t)m * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess &&
                 std::memcmp(pat.data(), back.data(), 2 * (size_t)m * sizeof(double)) == 0;
    (void)hipStreamSynchronize(c->stream);
    (void)hipGetLastError();
    if (ok) c->bar_state = 1;
    return ok;
}
// Places the inputs of nb trajectories of n pieces for a host-direct step and launches it.  ISDF_DIRECT_NA: not applicable
// (the step is not one fused launch), nothing launched.  T / coeffs: per-trajectory host arrays (trajectory `first` onwards).
int direct_launch(isdf_ctx *c, int nb, int n, const double *const *T, const double *const *coeffs, int first, hipStream_t st, int mode) {
    int rc = direct_reserve(c, nb, n);
    if (rc) return rc;
    const size_t in_all = (size_t)19 * n * nb;
    rc = c->d_in.reserve(c, in_all);
    if (rc) return rc;
    HostDirect hd;
    hd.via_bar = bar_usable(c, c->d_in, in_all);
    // inputs: through the BAR straight into device memory (posted writes, done before the doorbell is rung), or into the
    // pinned buffer the first workgroups of the launch read
    double *dst = hd.via_bar ? c->d_in : c->h_dir;
    for (int b = 0; b < nb; b++) {
        std::memcpy(dst + (size_t)b * n, T[first + b], (size_t)n * sizeof(double));
        std::memcpy(dst + (size_t)n * nb + (size_t)b * 18 * n, coeffs[first + b], (size_t)18 * n * sizeof(double));
    }
    host_rows_mark(c->h_dir + c->dir_in, c->dir_out);            // (the step STORES its sums there; it never reads them)
    __sync_synchronize();
    hd.T = c->h_dir.dev(); hd.coeffs = c->h_dir.dev() + (size_t)n * nb;
    hd.out = c->h_dir.dev() + c->dir_in;
    hd.flags = (unsigned long long *)(c->h_dir.dev() + c->dir_in + c->dir_out);
    hd.seq = ++c->dir_seq;
    rc = eval_device_impl(c, nb, n, c->d_in, c->d_in + (size_t)n * nb, hd.out, nullptr, st, mode, false, &hd);
    if (rc == ISDF_OK) { c->dir_pending = true; c->dir_nb = nb; c->dir_n = n; c->last_host_path = hd.via_bar ? ISDF_HOST_PATH_DIRECT_BAR : ISDF_HOST_PATH_DIRECT_MAPPED; }
    return rc;
}
// the host's side of the hand-over: spin on the trajectories' flags (the launch stores them last); bounded - a launch that
// never finishes is reported, not waited for forever
int direct_wait(isdf_ctx *c, hipStream_t st, bool *overflow) {
    c->dir_pending = false;
    volatile unsigned long long *flags = (volatile unsigned long long *)(c->h_dir + c->dir_in + c->dir_out);
    const unsigned long long seq = c->dir_seq;
    const auto t0 = std::chrono::steady_clock::now();
    *overflow = false;
    for (int b = 0; b < c->dir_nb; b++) {
        unsigned long long f;
        if (!host_flag_wait(flags + b, seq, HOST_FLAG_OVERFLOW, t0, 5.0, st, &f))
            return isdf_fail(c, ISDF_ERR_HIP, "host-direct step did not complete (flag never arrived)");
        if (f & HOST_FLAG_OVERFLOW) *overflow = true;
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    if (!host_rows_wait(c, c->h_dir + c->dir_in, (size_t)c->dir_nb * isdf_out_stride(c->dir_n))) {
        (void)hipStreamSynchronize(st);
        return isdf_fail(c, ISDF_ERR_HIP, "host-direct step: its completion word arrived but not all of its results");
    }
    return ISDF_OK;
}

// ---- host-direct form of the steps that are SEVERAL launches (the swept-volume sweep: prepare, scan, descent, back-prop, reduce):
// the inputs go down through the PCIe BAR, the launches run as ever, and one small kernel behind them copies [cost | gradT |
// gradC], the statistics words and lastTstar into host-mapped memory and raises a flag there - no copy commands (each a DMA
// packet with its own completion), no stream synchronisation (a scheduler wake-up).
__global__ __launch_bounds__(1024) void publish_kernel(const double *out, size_t count, const unsigned long long *stats, const double *tstar, int M,
                                                       double *h_out, unsigned long long *h_stats, double *h_tstar, unsigned long long *h_flag, unsigned long long seq) {
    for (size_t i = threadIdx.x; i < count; i += blockDim.x) h_out[i] = out[i];
    if (threadIdx.x < 8) h_stats[threadIdx.x] = stats[threadIdx.x];
    if (tstar) for (int i = threadIdx.x; i < M; i += blockDim.x) h_tstar[i] = tstar[i];
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(h_flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
static bool v1_direct_enabled(const isdf_ctx *c) {
    return !c->env_no_direct && !c->prof_on && c->world == 1 && c->peers.empty() && !c->rccl_comm && c->cfg.variant == ISDF_V1_SWEPT;
}
// returns ISDF_DIRECT_NA when the host cannot write device memory (no large BAR): the copy path then
static int v1_direct_eval(isdf_ctx *c, int n, const double *T, const double *coeffs, double *tstar_inout, const double **h_out, const unsigned long long **h_stat) {
    const size_t in_all = (size_t)19 * n, ostride = isdf_out_stride(n);
    const bool ts = tstar_inout && c->M > 0;
    // d_in: [T | coeffs | lastTstar] - CPU-written, GPU-read only.  (lastTstar does NOT go straight into d_tstar: the GPU itself wrote
    // that array in the step before, and CPU stores through the BAR into memory the device has written are outside what bar_usable
    // probes; the prepare kernel copies the staged values over, SweptParams::tstar_stage)
    int rc = c->d_in.reserve(c, in_all + (size_t)(ts ? c->M : 0));
    if (rc) return rc;
    rc = c->d_out.reserve(c, ostride);
    if (rc) return rc;
    if (!bar_usable(c, c->d_in, in_all + (size_t)(ts ? c->M : 0))) return ISDF_DIRECT_NA;
    // pinned, device-mapped: [out | 8 statistics words | flag | lastTstar]
    const size_t need = ostride + 8 + 2 + (size_t)(ts ? c->M : 0);
    rc = c->h_v1_pin.reserve(c, need);
    if (rc) return rc;
    std::memcpy(c->d_in, T, (size_t)n * sizeof(double));                       // CPU stores into device memory
    std::memcpy(c->d_in + n, coeffs, (size_t)18 * n * sizeof(double));
    if (ts) { std::memcpy(c->d_in + in_all, tstar_inout, (size_t)c->M * sizeof(double)); c->v1_tstar_stage = c->d_in + in_all; }
    __sync_synchronize();
    rc = eval_device_impl(c, 1, n, c->d_in, c->d_in + n, c->d_out, ts ? c->d_tstar : nullptr, c->stream, 0);
    c->v1_tstar_stage = nullptr;
    if (rc) return rc;
    const unsigned long long seq = ++c->dir_seq;
    host_rows_mark(c->h_v1_pin, ostride);
    if (ts) host_rows_mark(c->h_v1_pin + ostride + 10, (size_t)c->M);
    __sync_synchronize();
    double *ho = c->h_v1_pin.dev();
    unsigned long long *hs = (unsigned long long *)(c->h_v1_pin.dev() + ostride);
    hipLaunchKernelGGL(publish_kernel, dim3(1), dim3(1024), 0, c->stream, c->d_out, ostride, c->d_stats, ts ? c->d_tstar : nullptr, c->M,
                       ho, hs, c->h_v1_pin.dev() + ostride + 10, hs + 8, seq);
    HIPCHK(c, hipGetLastError());
    volatile unsigned long long *flag = (volatile unsigned long long *)(c->h_v1_pin + ostride) + 8;
    const auto t0 = std::chrono::steady_clock::now();
    unsigned long long f;
    if (!host_flag_wait(flag, seq, 0ull, t0, 10.0, c->stream, &f))
        return isdf_fail(c, ISDF_ERR_HIP, "host-direct swept-volume step did not complete (its flag never arrived)");
    std::atomic_thread_fence(std::memory_order_acquire);
    if (!host_rows_wait(c, c->h_v1_pin, ostride) || (ts && !host_rows_wait(c, c->h_v1_pin + ostride + 10, (size_t)c->M, true))) {
        (void)hipStreamSynchronize(c->stream);
        return isdf_fail(c, ISDF_ERR_HIP, "host-direct swept-volume step: its flag arrived but not all of its results");
    }
    if (ts) std::memcpy(tstar_inout, c->h_v1_pin + ostride + 10, (size_t)c->M * sizeof(double));
    *h_out = c->h_v1_pin;
    *h_stat = (const unsigned long long *)(c->h_v1_pin + ostride);
    c->last_host_path = ISDF_HOST_PATH_DIRECT_BAR;
    return ISDF_OK;
}

extern "C" int isdf_host_path(const isdf_ctx *c) { return c ? c->last_host_path : ISDF_ERR_INVALID_ARG; }
extern "C" int isdf_host_info(const isdf_ctx *c, int64_t info_out[8]) {
    if (!c || !info_out) return ISDF_ERR_INVALID_ARG;
    for (int k = 0; k < 8; k++) info_out[k] = 0;
    info_out[0] = (int64_t)c->host_steps; info_out[1] = (int64_t)c->host_late; info_out[2] = (int64_t)c->host_late_spins;
    return ISDF_OK;
}

// one trajectory's [cost | gradT | gradC] added into the caller's arrays (accumulate semantics of the host-array entry points)
static void add_rows(const double *o, int n, double *cost, double *gT, double *gC) {
    *cost += o[0];
    for (int i = 0; i < n; i++) gT[i] += o[1 + i];
    for (int i = 0; i < 18 * n; i++) gC[i] += o[1 + n + i];
}

extern "C" int isdf_eval(isdf_ctx *c, int n_traj, const int *N, const double *const *T, const double *const *coeffs,
                         double *cost_inout, double *const *gradT_inout, double *const *gradC_inout, double *tstar_inout) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    if (n_traj < 1 || !N || !T || !coeffs || !cost_inout || !gradT_inout || !gradC_inout) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "null argument");
    HIPCHK(c, hipSetDevice(c->device));
    // trajectories with equal N go out as one batched launch; ragged input is evaluated group by group.
    // Per group: inputs gathered into one pinned buffer, ONE upload, the launches, ONE download (outputs + the overflow
    // word), ONE synchronisation.  The pair statistics are computed on demand (isdf_get_stats) unless the input is ragged.
    int start = 0, groups = 0;
    isdf_stats total{};
    bool overflow = false;
    for (int s0 = 0; s0 < n_traj;) { int e = s0 + 1; while (e < n_traj && N[e] == N[s0]) e++; groups++; s0 = e; }
    while (start < n_traj) {
        int end = start + 1;
        while (end < n_traj && N[end] == N[start]) end++;
        const int nb = end - start, n = N[start];
        if (n < 1) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "N must be >= 1");
        const size_t in_per = (size_t)19 * n, ostride = isdf_out_stride(n);
        const size_t in_all = in_per * nb, out_all = ostride * nb;
        for (int b = 0; b < nb; b++)
            if (!T[start + b] || !coeffs[start + b] || !gradT_inout[start + b] || !gradC_inout[start + b])
                return isdf_fail(c, ISDF_ERR_INVALID_ARG, "null trajectory buffer");
        if (direct_enabled(c)) {
            // ONE launch, no copy commands, no stream synchronisation: the inputs go straight into device memory through the
            // PCIe BAR (or are fetched from host-mapped memory by the launch itself), the launch copies [cost | gradT | gradC]
            // and a completion flag per trajectory into host-mapped memory (csrc/tile_sweep.hip)
            int rcd = direct_launch(c, nb, n, T, coeffs, start, c->stream, 0);
            if (rcd < 0) return rcd;
            if (rcd == ISDF_OK) {
                bool ovf = false;
                rcd = direct_wait(c, c->stream, &ovf);
                if (rcd) return rcd;
                if (ovf) {
                    overflow = true;
                    const int rr = clear_overflow(c);
                    if (rr) return rr;
                }
                const double *hout = c->h_dir + c->dir_in;
                for (int b = 0; b < nb; b++) add_rows(hout + ostride * b, n, &cost_inout[start + b], gradT_inout[start + b], gradC_inout[start + b]);
                if (groups > 1) {
                    rcd = fetch_stats(c);
                    if (rcd) return rcd;
                    stats_add(total, c->last_stats);
                }
                start = end;
                continue;
            }
            // ISDF_DIRECT_NA: this step is not one fused launch - the copy path below
        }
        if (nb == 1 && v1_direct_enabled(c)) {
            const double *ho = nullptr; const unsigned long long *hs = nullptr;
            const int rcv = v1_direct_eval(c, n, T[start], coeffs[start], tstar_inout, &ho, &hs);
            if (rcv < 0) return rcv;
            if (rcv == ISDF_OK) {
                if (hs[4]) {
                    overflow = true;
                    const int rr = clear_overflow(c);
                    if (rr) return rr;
                }
                stats_add(total, hs);
                add_rows(ho, n, &cost_inout[start], gradT_inout[start], gradC_inout[start]);
                start = end;
                continue;
            }
        }
        c->last_host_path = ISDF_HOST_PATH_COPY;
        int rc = c->d_in.reserve(c, in_all);
        if (rc) return rc;
        rc = c->d_out.reserve(c, out_all);
        if (rc) return rc;
        rc = c->h_eval_pin.reserve(c, in_all + out_all + 16);      // pinned staging: [inputs | outputs | 8 statistics words]
        if (rc) return rc;
        double *hin = c->h_eval_pin, *hout = c->h_eval_pin + in_all;
        unsigned long long *hstat = (unsigned long long *)(c->h_eval_pin + in_all + out_all);
        double *dT = c->d_in, *dC = c->d_in + (size_t)n * nb;
        for (int b = 0; b < nb; b++) {
            std::memcpy(hin + (size_t)b * n, T[start + b], (size_t)n * sizeof(double));
            std::memcpy(hin + (size_t)n * nb + (size_t)b * 18 * n, coeffs[start + b], (size_t)18 * n * sizeof(double));
        }
        HIPCHK(c, hipMemcpyAsync(c->d_in, hin, in_all * sizeof(double), hipMemcpyHostToDevice, c->stream));
        double *dts = nullptr;
        if (c->cfg.variant == ISDF_V1_SWEPT && tstar_inout && c->M > 0) {
            dts = c->d_tstar;
            HIPCHK(c, hipMemcpyAsync(dts, tstar_inout, (size_t)c->M * sizeof(double), hipMemcpyHostToDevice, c->stream));
        }
        // a multi-device step ends in a sum kernel on the lead: it writes straight into the pinned buffer and raises a word there
        const bool host_out = (!c->peers.empty() || c->rccl_comm) && !dts && !c->env_multi_no_hostout && !c->prof_on;
        if (host_out) {
            if (!c->d_msum_blocks) HIPCHK(c, c->d_msum_blocks.alloc(1, 0x00));
            c->mh_words = (unsigned long long *)(c->h_eval_pin.dev() + in_all + out_all);
            c->mh_seq++;
            host_rows_mark(hout, out_all);                       // (see host_rows_wait: the word does not order the results for the CPU)
            host_rows_mark((double *)hstat, 8);
            __sync_synchronize();
        }
        rc = sweep_dispatch(c, nb, n, dT, dC, host_out ? c->h_eval_pin.dev() + in_all : c->d_out, dts, c->stream);
        if (rc) { c->mh_words = nullptr; return rc; }
        if (host_out) {
            volatile unsigned long long *word = hstat + 8;
            const auto t0 = std::chrono::steady_clock::now();
            unsigned long long w;
            if (!host_flag_wait(word, c->mh_seq, 0ull, t0, 5.0, c->stream, &w))
                return isdf_fail(c, ISDF_ERR_HIP, "multi-device step did not complete (its completion word never arrived)");
            std::atomic_thread_fence(std::memory_order_acquire);
            if (!host_rows_wait(c, hout, out_all) || !host_rows_wait(c, (const double *)hstat, 8, true)) {
                (void)hipStreamSynchronize(c->stream);
                return isdf_fail(c, ISDF_ERR_HIP, "multi-device step: its completion word arrived but not all of its results");
            }
        } else {
        HIPCHK(c, hipMemcpyAsync(hout, c->d_out, out_all * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(hstat, c->d_stats, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        if (dts) HIPCHK(c, hipMemcpyAsync(tstar_inout, dts, (size_t)c->M * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        }
        if (hstat[4]) {   // sticky until read; slots a late producer may still fill are emptied again
            overflow = true;
            const int rr = clear_overflow(c);
            if (rr) return rr;
        }
        if (c->cfg.variant == ISDF_V1_SWEPT) {       // the V1 kernels count straight into the statistics words
            stats_add(total, hstat);
        } else if (groups > 1) {
            rc = fetch_stats(c);                 // ragged input: the per-group counts have to be added up now
            if (rc == ISDF_OK) rc = add_peer_stats(c);
            if (rc) return rc;
            stats_add(total, c->last_stats);
        }
        for (int b = 0; b < nb; b++) add_rows(hout + ostride * b, n, &cost_inout[start + b], gradT_inout[start + b], gradC_inout[start + b]);
        start = end;
    }
    if (groups > 1 || c->cfg.variant == ISDF_V1_SWEPT) {
        total.overflow = overflow ? 1 : 0;
        c->last_stats = total;
        c->stats_cached = true;
    } else {
        c->stats_cached = false;                 // isdf_get_stats counts the pairs of the last launch when asked
    }
    if (overflow) return isdf_fail(c, ISDF_ERR_OVERFLOW, "a bounded device work list overflowed; result invalid");
    return ISDF_OK;
}

// Host-array form of the above (accumulate semantics like isdf_eval): tstar = M doubles.
extern "C" int isdf_eval_swept_at_tstar_host(isdf_ctx *c, int N, const double *T, const double *coeffs, const double *tstar,
                                             double *cost_inout, double *gradT_inout, double *gradC_inout) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    if (N < 1 || !T || !coeffs || !tstar || !cost_inout || !gradT_inout || !gradC_inout) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "null argument");
    if (!c->peers.empty() || c->is_peer || c->rccl_comm) return isdf_fail(c, ISDF_ERR_UNSUPPORTED, "isdf_eval_swept_at_tstar on a multi-device ctx");
    if (c->M <= 0) return ISDF_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t in_all = (size_t)19 * N, ostride = isdf_out_stride(N);
    int rc = c->d_in.reserve(c, in_all + (size_t)c->M);
    if (rc) return rc;
    rc = c->d_out.reserve(c, ostride);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->d_in, T, (size_t)N * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_in + N, coeffs, (size_t)18 * N * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_in + in_all, tstar, (size_t)c->M * sizeof(double), hipMemcpyHostToDevice, c->stream));
    rc = eval_device_impl(c, 1, N, c->d_in, c->d_in + N, c->d_out, c->d_in + in_all, c->stream, 1, true);
    if (rc) return rc;
    std::vector<double> h(ostride);
    HIPCHK(c, hipMemcpyAsync(h.data(), c->d_out, ostride * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    add_rows(h.data(), N, cost_inout, gradT_inout, gradC_inout);
    return ISDF_OK;
}
