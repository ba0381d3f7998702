// The host path the trajectory tools share (host-only): traj_limits.hip, traj_retime.hip and traj_realloc.hip check, stage, finish and
// report a call through these, so a tool's file holds its rules, its kernels and the order of its own launches.  Nothing here launches a
// kernel, and nothing here is for one tool alone.
#pragma once
#include "isdf_ctx.hpp"
#include <cmath>
#include <initializer_list>
#include <vector>

namespace traj_call {

inline int fail(isdf_ctx *c, int code, const char *msg) { return isdf_fail(c, code, msg); }

// the caller's parameters, or the defaults
template <typename P, typename F> P resolve(const P *p, F fill_default) {
    P v;
    if (p) v = *p; else fill_default(&v);
    return v;
}

// the ctx gate: always the LAST of a call's checks (a null ctx with a bad argument reports the argument)
inline int check_ctx(isdf_ctx *c, const char *what_null, const char *what_multi) {
    if (!c) return fail(nullptr, ISDF_ERR_INVALID_ARG, what_null);
    if (!c->peers.empty() || c->is_peer || c->rccl_comm) return fail(c, ISDF_ERR_UNSUPPORTED, what_multi);
    return ISDF_OK;
}

// n durations on the host: each positive and finite, or `what`
inline int check_durations(isdf_ctx *c, long long n, const double *T, const char *what) {
    for (long long q = 0; q < n; q++)
        if (!(T[q] > 0.0) || !std::isfinite(T[q])) return fail(c, ISDF_ERR_INVALID_ARG, what);
    return ISDF_OK;
}

// What every tool's state holds: the staging of its host forms, the result words on the host and the two events round its launches.
// A tool's own state derives from this and adds its scratch.
struct State {
    DevBuf<double> d_in, d_out;         // host forms: the call's inputs / its results (T | coeffs)
    std::vector<double> h_res;
    DevEvents<2> ev;
    int ready(isdf_ctx *c) { return ev.ready(c); }
    double *host_words(size_t n) { if (h_res.size() < n) h_res.resize(n); return h_res.data(); }
};

// the ctx's device made current, the tool's state (`slot`: the ctx's pointer to it) created on first use, its events ready
template <typename S> int state_of(isdf_ctx *c, Lazy<S> &slot, S **out) {
    HIPCHK(c, hipSetDevice(c->device));
    ISDF_TRY(slot.make(c, out));
    return (*out)->ready(c);
}

// n trajectories' pieces in all (nT = B N): T | coeffs into buf, which afterwards holds the durations at buf and the coefficients at buf + nT
inline int upload(isdf_ctx *c, DevBuf<double> &buf, size_t nT, const double *T, const double *coeffs, hipStream_t st) {
    ISDF_TRY(buf.reserve(c, 19 * nT));
    HIPCHK(c, hipMemcpyAsync(buf, T, nT * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(buf + nT, coeffs, 18 * nT * sizeof(double), hipMemcpyHostToDevice, st));
    return ISDF_OK;
}

// where a run leaves the B results: on the device always, on the host as well where h_T is given
struct Out { double *d_T, *d_C, *h_T, *h_C; };
struct Down { double *host; const double *dev; size_t n; };     // one copy of a run's tail (host null: none)

// The tail of a run whose launches are queued on st after ev[0]: the launches' error, ev[1], the copies in the order given, the call's ONE
// synchronisation, the device time between the events.  The caller judges its flag word and unpacks its struct.
inline int finish(isdf_ctx *c, State *k, hipStream_t st, std::initializer_list<Down> down, float *ms) {
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(k->ev[1], st));
    for (const Down &d : down)
        if (d.host) HIPCHK(c, hipMemcpyAsync(d.host, d.dev, d.n * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipEventElapsedTime(ms, k->ev[0], k->ev[1]));
    return ISDF_OK;
}

// the clearance check of a result that is on the device, into the tool's info (`check` of its parameters)
template <typename Info> int post_check(isdf_ctx *c, int N, const double *d_T, const double *d_C, Info *info, hipStream_t st) {
    isdf_traj_check_info chk;
    ISDF_TRY(isdf_traj_check_device(c, N, d_T, d_C, nullptr, &chk, nullptr, st));
    if (info) { info->check = chk; info->checked = 1; }
    return ISDF_OK;
}

}  // namespace traj_call
