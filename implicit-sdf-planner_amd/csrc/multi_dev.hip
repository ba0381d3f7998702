// One host process driving several devices (isdf_create_multi): the shards' launches, the sum of their parts, RCCL by dlopen.
#include "isdf_ctx.hpp"
#include <dlfcn.h>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace isdf;

// ---------------------------------------------------------------------------------------------------------------------------
// ONE host process, SEVERAL devices (isdf_create_multi; SURVEY 8(b) "Threading": launch -> all-reduce -> D2H from the calling
// thread, no extra host threads).  The lead ctx is shard 0 on devices[0]; every further device has a plain ctx of its own
// (shard r of n) that the lead owns.  A step: the inputs go to every device (peer copies ordered behind the caller's stream by
// an event), every shard is queued on its own device's stream FROM THE CALLING THREAD, every shard leaves [packed outputs | its 8
// statistics words as doubles] in its part buffer, and the parts are summed on the lead in rank order -
//   ISDF_MULTI_PEER_SUM  one kernel on the lead that reads the peers' parts straight over xGMI (peer access),
//   ISDF_MULTI_STAGED    peer copies into a staging buffer on the lead + the same kernel locally (no peer access needed),
//   ISDF_MULTI_RCCL      ncclAllReduce(sum, ncclDouble) over the part buffers in one group call (librccl.so by dlopen, so the
//                        library neither links nor needs RCCL unless asked: ISDF_MULTI_COLLECTIVE=rccl),
// after which the caller's stream holds the full [cost | gradT | gradC] - exactly what the single-device step leaves.
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int MULTI_TAIL = 8;
struct MultiParts { const double *p[XCHG_MAX_WORLD]; const unsigned long long *st[XCHG_MAX_WORLD]; int n; };   // st[0] != null: the shards' statistics words are read in place
// the 8 statistics words of a shard behind its packed outputs, as doubles: they ride through whichever sum is in force
__global__ void multi_tail_kernel(const unsigned long long *stats, double *tail) {
    if (threadIdx.x < MULTI_TAIL) tail[threadIdx.x] = (double)stats[threadIdx.x];
}
// out[i] = part_0[i] + part_1[i] + ... (rank order: bitwise reproducible); the summed tail back into the lead's statistics words
// (`all_stats`: V1 counts straight into the statistics words, so their device sums are the step's statistics; V2 / V3 words are
// filled on demand by isdf_get_stats and only the overflow word [4] travels)
// host_words != null: `out` is host-mapped; the step's 8 statistics words follow it into host_words[0..7] and, once every block of
// this launch has written, host_words[8] = seq tells the spinning host that the step is complete
__global__ __launch_bounds__(256) void multi_sum_kernel(double *out, MultiParts parts, size_t count, unsigned long long *stats, int all_stats,
                                                        unsigned long long *host_words, unsigned *blocks_done, unsigned long long seq) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count + MULTI_TAIL) {
        double s;
        if (i >= count && parts.st[0]) {                                    // (peer access: no tail launches, the words are read where they are)
            s = (double)parts.st[0][i - count];
            for (int r = 1; r < parts.n; r++) s += (double)parts.st[r][i - count];
        } else {
            s = parts.p[0][i];
            for (int r = 1; r < parts.n; r++) s += parts.p[r][i];
        }
        if (i < count) out[i] = s;
        else {
            const int k = (int)(i - count);
            if (k == 4) { if (s != 0.0) stats[4] = 1ull; }                 // overflow: sticky until read
            else if (all_stats) stats[k] = (unsigned long long)s;
            if (host_words) host_words[k] = k == 4 ? ((s != 0.0 || stats[4] != 0ull) ? 1ull : 0ull) : (unsigned long long)s;
        }
    }
    if (host_words) {
        __threadfence_system();
        __syncthreads();
        if (threadIdx.x == 0 && atomicAdd(blocks_done, 1u) == gridDim.x - 1u) {
            *blocks_done = 0u;
            __threadfence_system();
            *(volatile unsigned long long *)(host_words + 8) = seq;
        }
    }
}

namespace {
struct RcclApi {
    void *lib = nullptr;
    int (*CommInitAll)(void **, int, const int *) = nullptr;
    int (*CommDestroy)(void *) = nullptr;
    int (*AllReduce)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
};
RcclApi g_rccl;
bool rccl_load() {
    if (g_rccl.lib) return g_rccl.AllReduce != nullptr;
    for (const char *name : {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"}) { g_rccl.lib = dlopen(name, RTLD_NOW | RTLD_LOCAL); if (g_rccl.lib) break; }
    if (!g_rccl.lib) return false;
    g_rccl.CommInitAll = (int (*)(void **, int, const int *))dlsym(g_rccl.lib, "ncclCommInitAll");
    g_rccl.CommDestroy = (int (*)(void *))dlsym(g_rccl.lib, "ncclCommDestroy");
    g_rccl.AllReduce = (int (*)(const void *, void *, size_t, int, int, void *, hipStream_t))dlsym(g_rccl.lib, "ncclAllReduce");
    g_rccl.GroupStart = (int (*)())dlsym(g_rccl.lib, "ncclGroupStart");
    g_rccl.GroupEnd = (int (*)())dlsym(g_rccl.lib, "ncclGroupEnd");
    g_rccl.GetErrorString = (const char *(*)(int))dlsym(g_rccl.lib, "ncclGetErrorString");
    if (!g_rccl.CommInitAll || !g_rccl.CommDestroy || !g_rccl.AllReduce || !g_rccl.GroupStart || !g_rccl.GroupEnd) { g_rccl.AllReduce = nullptr; return false; }
    return true;
}
}  // namespace

void multi_release(isdf_ctx *c) {
    if (c->rccl_comm && g_rccl.CommDestroy) { (void)g_rccl.CommDestroy(c->rccl_comm); c->rccl_comm = nullptr; }
    c->mev_in.release(); c->mev_done.release();
}

extern "C" int isdf_create_multi(isdf_ctx **out, const isdf_config *cfg, const int *devices, int n_devices) {
    if (!out || !cfg || !devices) return isdf_fail(nullptr, ISDF_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (n_devices < 1 || n_devices > XCHG_MAX_WORLD) return isdf_fail(nullptr, ISDF_ERR_INVALID_ARG, "1 .. 16 devices");
    std::vector<isdf_ctx *> all;
    auto bail = [&](int code, const std::string &msg) { for (isdf_ctx *q : all) { q->is_peer = false; q->peers.clear(); (void)isdf_destroy(q); } return isdf_fail(nullptr, code, msg.c_str()); };
    for (int r = 0; r < n_devices; r++) {
        isdf_config cr = *cfg;
        cr.device = devices[r];
        isdf_ctx *q = nullptr;
        const int rc = isdf_create(&q, &cr);
        if (rc != ISDF_OK) return bail(rc, std::string("device ") + std::to_string(devices[r]) + ": " + isdf_last_error(nullptr));
        all.push_back(q);
        q->rank = r; q->world = n_devices;
        if (hipSetDevice(q->device) != hipSuccess || q->mev_done.ready(q, hipEventDisableTiming) != ISDF_OK ||
            q->mev_in.ready(q, hipEventDisableTiming) != ISDF_OK)
            return bail(ISDF_ERR_HIP, "event creation failed");
    }
    isdf_ctx *lead = all[0];
    // how the parts are summed: the lead reads the peers' buffers directly when every peer is reachable
    int mode = ISDF_MULTI_PEER_SUM;
    (void)hipSetDevice(lead->device);
    for (int r = 1; r < n_devices && mode == ISDF_MULTI_PEER_SUM; r++) {
        if (devices[r] == lead->device) continue;                         // the same device listed again (tests): plain pointers
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, lead->device, devices[r]) != hipSuccess || !can) { mode = ISDF_MULTI_STAGED; break; }
        const hipError_t e = hipDeviceEnablePeerAccess(devices[r], 0);
        if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) mode = ISDF_MULTI_STAGED;
        (void)hipGetLastError();
    }
    if (const char *e = getenv("ISDF_MULTI_COLLECTIVE")) {
        if (!std::strcmp(e, "staged")) mode = ISDF_MULTI_STAGED;
        else if (!std::strcmp(e, "peer")) { if (mode != ISDF_MULTI_PEER_SUM) return bail(ISDF_ERR_UNSUPPORTED, "ISDF_MULTI_COLLECTIVE=peer: no peer access between the listed devices"); }
        else if (!std::strcmp(e, "rccl")) {
            for (int a = 0; a < n_devices; a++) for (int b = a + 1; b < n_devices; b++)
                if (devices[a] == devices[b]) return bail(ISDF_ERR_UNSUPPORTED, "ISDF_MULTI_COLLECTIVE=rccl needs DISTINCT devices (one communicator rank per GPU)");
            if (!rccl_load()) return bail(ISDF_ERR_UNSUPPORTED, "ISDF_MULTI_COLLECTIVE=rccl: librccl.so could not be loaded");
            std::vector<void *> comms(n_devices, nullptr);
            const int rr = g_rccl.CommInitAll(comms.data(), n_devices, devices);
            if (rr != 0) return bail(ISDF_ERR_UNSUPPORTED, std::string("ncclCommInitAll: ") + (g_rccl.GetErrorString ? g_rccl.GetErrorString(rr) : "failed") + " (one communicator per DISTINCT device)");
            for (int r = 0; r < n_devices; r++) all[r]->rccl_comm = comms[r];
            mode = ISDF_MULTI_RCCL;
        } else return bail(ISDF_ERR_INVALID_ARG, "ISDF_MULTI_COLLECTIVE must be peer, staged or rccl");
    }
    // PULL: with peer access in BOTH directions the peers' kernels read T | coeffs (and, for the swept-volume sweep, read and write
    // their points' lastTstar) straight in the lead's memory over xGMI - 152 N bytes per step - instead of two to four peer copies
    // per device and step queued from the calling thread; the lead's sum reads the peers' statistics words in place
    bool pull = mode == ISDF_MULTI_PEER_SUM && !env_is("ISDF_MULTI_NO_PULL", '1');
    for (int r = 1; r < n_devices && pull; r++) {
        if (devices[r] == lead->device) continue;
        int can = 0;
        if (hipSetDevice(devices[r]) != hipSuccess || hipDeviceCanAccessPeer(&can, devices[r], lead->device) != hipSuccess || !can) { pull = false; break; }
        const hipError_t e = hipDeviceEnablePeerAccess(lead->device, 0);
        if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) pull = false;
        (void)hipGetLastError();
    }
    lead->multi_pull = pull;
    for (int r = 1; r < n_devices; r++) { all[r]->is_peer = true; lead->peers.push_back(all[r]); }
    lead->multi_collective = mode;
    (void)hipSetDevice(lead->device);
    *out = lead;
    return ISDF_OK;
}
extern "C" int isdf_multi_info(const isdf_ctx *c, int *n_devices_out, int *collective_out) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    if (n_devices_out) *n_devices_out = 1 + (int)c->peers.size();
    if (collective_out) *collective_out = c->peers.empty() ? ISDF_MULTI_NONE : c->multi_collective;
    return ISDF_OK;
}

// One step on every device.  d_T / d_coeffs / d_out / d_tstar live on the LEAD's device and are ordered on `st` (a stream of the
// lead's device) like in the single-device call.
int multi_eval_device(isdf_ctx *c, int n_traj, int N, const double *d_T, const double *d_coeffs, double *d_out,
                      double *d_tstar, hipStream_t st, int mode, bool fixed_tstar) {
    const int n = 1 + (int)c->peers.size();
    const size_t count = (size_t)n_traj * isdf_out_stride(N), in_T = (size_t)n_traj * N, in_C = (size_t)n_traj * 18 * N;
    const bool swept = c->cfg.variant == ISDF_V1_SWEPT && mode != 2;
    if (fixed_tstar) return isdf_fail(c, ISDF_ERR_UNSUPPORTED, "isdf_eval_swept_at_tstar on a multi-device ctx");
    HIPCHK(c, hipSetDevice(c->device));
    // the previous step's sum read the peers' part buffers and this ctx's own: a step issued on ANOTHER caller stream must not
    // overwrite them before that sum has run (the peers' streams follow through mev_in below)
    if (c->msum_recorded) HIPCHK(c, hipStreamWaitEvent(st, c->mev_done[0], 0));
    HIPCHK(c, hipEventRecord(c->mev_in[0], st));                              // the caller's inputs are ready from here on
    double *lead_ts = swept ? (d_tstar ? d_tstar : c->d_tstar) : nullptr;
    const bool pull = c->multi_pull && c->multi_collective == ISDF_MULTI_PEER_SUM;
    MultiParts parts{};
    parts.n = n;
    unsigned long long *const mh_words = c->mh_words;          // (isdf_eval arms this per step)
    c->mh_words = nullptr;
    for (int r = 1; r < n; r++) {
        isdf_ctx *p = c->peers[r - 1];
        HIPCHK(c, hipSetDevice(p->device));
        int rc = pull ? ISDF_OK : p->d_in.reserve(p, in_T + in_C);
        if (rc == ISDF_OK) rc = p->d_mpart.reserve(p, count + MULTI_TAIL);
        if (rc) { c->err = p->err; return rc; }
        HIPCHK(c, hipStreamWaitEvent(p->stream, c->mev_in[0], 0));
        long long pb = 0, pe = 0;
        if (pull) {
            // the shard reads the lead's inputs in place (peer access); lastTstar likewise - every point belongs to ONE shard
            rc = eval_device_impl(p, n_traj, N, d_T, d_coeffs, p->d_mpart, lead_ts, p->stream, mode, false);
            if (rc) { c->err = "device " + std::to_string(p->device) + ": " + p->err; return rc; }
            parts.st[r] = p->d_stats;
        } else {
            HIPCHK(c, hipMemcpyPeerAsync(p->d_in, p->device, d_T, c->device, in_T * sizeof(double), p->stream));
            HIPCHK(c, hipMemcpyPeerAsync(p->d_in + in_T, p->device, d_coeffs, c->device, in_C * sizeof(double), p->stream));
            if (swept && p->M > 0) {                                           // lastTstar of this shard's points travels with it
                shard_range(p->M, p->rank, p->world, pb, pe);
                if (pe > pb && lead_ts) HIPCHK(c, hipMemcpyPeerAsync(p->d_tstar + pb, p->device, lead_ts + pb, c->device, (size_t)(pe - pb) * sizeof(double), p->stream));
            }
            rc = eval_device_impl(p, n_traj, N, p->d_in, p->d_in + in_T, p->d_mpart, nullptr, p->stream, mode, false);
            if (rc) { c->err = "device " + std::to_string(p->device) + ": " + p->err; return rc; }
            hipLaunchKernelGGL(multi_tail_kernel, dim3(1), dim3(64), 0, p->stream, p->d_stats, p->d_mpart + count);
            if (swept && pe > pb && lead_ts) HIPCHK(c, hipMemcpyPeerAsync(lead_ts + pb, c->device, p->d_tstar + pb, p->device, (size_t)(pe - pb) * sizeof(double), p->stream));
        }
        HIPCHK(c, hipEventRecord(p->mev_done[0], p->stream));
        parts.p[r] = p->d_mpart;
    }
    HIPCHK(c, hipSetDevice(c->device));
    int rc = c->d_mpart.reserve(c, count + MULTI_TAIL);
    if (rc) return rc;
    rc = eval_device_impl(c, n_traj, N, d_T, d_coeffs, c->d_mpart, d_tstar, st, mode, false);
    if (rc) return rc;
    if (pull) parts.st[0] = c->d_stats;
    else hipLaunchKernelGGL(multi_tail_kernel, dim3(1), dim3(64), 0, st, c->d_stats, c->d_mpart + count);
    parts.p[0] = c->d_mpart;
    const dim3 grid((unsigned)((count + MULTI_TAIL + 255) / 256)), block(256);
    if (c->multi_collective == ISDF_MULTI_RCCL) {
        // ONE all-reduce of the packed vector per step: every device's part in place, issued from this thread as one group
        for (int r = 1; r < n; r++) HIPCHK(c, hipStreamWaitEvent(st, c->peers[r - 1]->mev_done[0], 0));      // (the merged lastTstar)
        if (g_rccl.GroupStart() != 0) return isdf_fail(c, ISDF_ERR_HIP, "ncclGroupStart failed");
        for (int r = 0; r < n; r++) {
            isdf_ctx *q = r == 0 ? c : c->peers[r - 1];
            hipStream_t qs = r == 0 ? st : q->stream;
            if (r > 0) HIPCHK(c, hipSetDevice(q->device));
            const int rr = g_rccl.AllReduce(q->d_mpart, q->d_mpart, count + MULTI_TAIL, 8 /* ncclDouble */, 0 /* ncclSum */, q->rccl_comm, qs);
            if (rr != 0) { (void)g_rccl.GroupEnd(); return isdf_fail(c, ISDF_ERR_HIP, "ncclAllReduce failed"); }
        }
        if (g_rccl.GroupEnd() != 0) return isdf_fail(c, ISDF_ERR_HIP, "ncclGroupEnd failed");
        HIPCHK(c, hipSetDevice(c->device));
        MultiParts one{}; one.n = 1; one.p[0] = c->d_mpart;
        hipLaunchKernelGGL(multi_sum_kernel, grid, block, 0, st, d_out, one, count, c->d_stats, swept ? 1 : 0, mh_words, c->d_msum_blocks, c->mh_seq);
    } else {
        for (int r = 1; r < n; r++) HIPCHK(c, hipStreamWaitEvent(st, c->peers[r - 1]->mev_done[0], 0));
        if (c->multi_collective == ISDF_MULTI_STAGED) {
            rc = c->d_mstage.reserve(c, (size_t)(n - 1) * (count + MULTI_TAIL));
            if (rc) return rc;
            for (int r = 1; r < n; r++) {
                double *dst = c->d_mstage + (size_t)(r - 1) * (count + MULTI_TAIL);
                HIPCHK(c, hipMemcpyPeerAsync(dst, c->device, c->peers[r - 1]->d_mpart, c->peers[r - 1]->device, (count + MULTI_TAIL) * sizeof(double), st));
                parts.p[r] = dst;
            }
        }
        hipLaunchKernelGGL(multi_sum_kernel, grid, block, 0, st, d_out, parts, count, c->d_stats, swept ? 1 : 0, mh_words, c->d_msum_blocks, c->mh_seq);
    }
    HIPCHK(c, hipGetLastError());
    // the next step's peer copies overwrite the peers' inputs: they are ordered behind THIS step's kernels by the peers' own
    // streams; the part buffers behind the lead's "sum done" event (its own mev_done: the lead records no other use of it)
    HIPCHK(c, hipEventRecord(c->mev_done[0], st));
    c->msum_recorded = true;
    return ISDF_OK;
}

// the peers' pair statistics of the last launch added to the lead's last_stats (V2 / V3; the V1 words of a multi-device step are
// already the devices' sums)
int add_peer_stats(isdf_ctx *c) {
    if (c->cfg.variant == ISDF_V1_SWEPT || c->peers.empty()) return ISDF_OK;
    for (isdf_ctx *p : c->peers) {
        HIPCHK(c, hipSetDevice(p->device));
        HIPCHK(c, hipDeviceSynchronize());
        const int rc = fetch_stats(p);
        if (rc) { c->err = p->err; return rc; }
        stats_add(c->last_stats, p->last_stats);
        c->last_stats.overflow |= p->last_stats.overflow;
    }
    HIPCHK(c, hipSetDevice(c->device));
    return ISDF_OK;
}
