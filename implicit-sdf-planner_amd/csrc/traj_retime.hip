// Uniform retiming of a trajectory to its dynamic limits on the device (isdf_traj_retime*): the smallest factor s of a ladder search
// at which the limits report of the scaled trajectory (isdf_traj_limits*, csrc/traj_limits.hip) is feasible.  The rules - scaling,
// ladder, pick, rounds - are stated in include/isdf_accel.h and written once, in csrc/traj_retime_host.hpp, as __host__ __device__
// functions: the kernels below and isdf_traj_retime_host run the same text.  The reference has no counterpart
// (trajectory.hpp:253-390, :631-680 only report).
//
//   begin    one wavefront per trajectory: the search state [s_lo, s_hi], the durations checked and summed in order.
//   scale    one thread per duration or coefficient of every (trajectory, candidate): the round's bracket from device memory, the
//            candidate's factor, one fp64 product or quotient.  B L trajectories laid out as the limits report's batch form takes them.
//   limits   the report's own two launches over those B L trajectories (isdf_traj_limits_launch), untouched.
//   pick     one wavefront per trajectory, candidates on the lanes (ladder <= 64): a lane judges its candidate's report against
//            the limits, a ballot gives the feasibility mask, tr_advance turns it into the next bracket and the status - every lane
//            computes the same state, lane 0 stores it.  After the last round the lanes copy the chosen candidate's arrays and report.
// 1 + 4 rounds launches for any B, nothing between them on the host, no atomics; the scratch lives in the ctx and grows only.
#include "traj_call.hpp"
#include "swept_field.hpp"
#include "traj_retime_host.hpp"
#include <cmath>
#include <cstring>
#include <vector>

namespace {
constexpr int CH = ISDF_LIMITS_CHANNELS;
constexpr int TW = ISDF_TL_INFO_WORDS;
constexpr int RES_WORDS = 8 + TW;       // scale, scale_below, status, rounds, nonmonotone, binding, duration_in, duration_out | the report's words
constexpr int ST_WORDS = 2;             // next to a trajectory's TRState: duration_in, 1 if a duration is not positive and finite
}  // namespace

struct TrajRetimeState : traj_call::State {     // d_in: T | coeffs of every trajectory of the call; d_out: the results, same layout
    DevBuf<double> d_scaled;            // [B L] T | [B L] coeffs
    DevBuf<double> d_piece;             // [B L N][12]
    DevBuf<double> d_info;              // [B L][TW]
    DevBuf<isdf_host::TRState> d_state; // [B]
    DevBuf<double> d_aux;               // [B][ST_WORDS]
    DevBuf<double> d_res;               // [B][RES_WORDS]
};

namespace {
using isdf_host::TRState;

struct TRLimits { double limit[CH]; };

__global__ __launch_bounds__(64) void tr_begin_kernel(int N, const double *__restrict__ T, double s_lo, double s_hi, TRState *__restrict__ state,
                                                       double *__restrict__ aux) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const double *Tb = T + (size_t)b * N;
    int bad = 0;
    for (int i = lane; i < N; i += 64) { const double t = Tb[i]; bad |= (!(t > 0.0) || !isfinite(t)) ? 1 : 0; }
    bad = __any(bad);
    if (lane != 0) return;
    double d = 0.0;                                 // summed in order, as the host form does
    for (int i = 0; i < N; i++) d += Tb[i];
    TRState s;
    isdf_host::tr_begin(s, s_lo, s_hi);
    state[b] = s;
    aux[(size_t)b * ST_WORDS] = d; aux[(size_t)b * ST_WORDS + 1] = bad ? 1.0 : 0.0;
}

__global__ __launch_bounds__(256) void tr_scale_kernel(int B, int N, int L, const double *__restrict__ T, const double *__restrict__ C,
                                                        const TRState *__restrict__ state, double *__restrict__ sT, double *__restrict__ sC) {
    const long long per = 19LL * N, total = (long long)B * L * per;
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= total) return;
    const long long g = tid / per, r = tid - g * per;       // g: (trajectory, candidate)
    const int b = (int)(g / L), i = (int)(g - (long long)b * L);
    const double s = isdf_host::tr_candidate(state[b].a, state[b].b, L, i);
    if (r < N) sT[g * N + r] = isdf_host::tr_scale_elem(N, r, T[(size_t)b * N + r], s);
    else       sC[g * 18 * N + (r - N)] = isdf_host::tr_scale_elem(N, r, C[(size_t)b * 18 * N + (r - N)], s);
}

// out_T / out_C: the B results, laid out like the inputs
__global__ __launch_bounds__(64) void tr_pick_kernel(int N, int L, int round, int R, TRLimits lim, const double *__restrict__ info,
                                                      const double *__restrict__ sT, const double *__restrict__ sC, TRState *__restrict__ state,
                                                      const double *__restrict__ aux, double *__restrict__ out_T, double *__restrict__ out_C,
                                                      double *__restrict__ res) {
    const int b = blockIdx.x, lane = threadIdx.x;
    // this lane's candidate: the channels that are judged and over their limit
    int over = 0;
    if (lane < L) {
        const double *w = info + ((size_t)b * L + lane) * TW;
#pragma unroll
        for (int ch = 0; ch < CH; ch++)
            if (!isnan(lim.limit[ch]) && isdf_host::tl_over(ch, w[4 * ch], lim.limit[ch])) over |= 1 << ch;
    }
    const unsigned long long feas = __ballot(lane < L && over == 0);
    TRState s = state[b];                           // every lane the same state: no exchange
    isdf_host::tr_advance(s, feas, L, round, R);
    if (round + 1 < R) { if (lane == 0) state[b] = s; return; }
    // the last round: a trajectory that was done early kept [s_lo, s_hi], whose candidates this round evaluated again
    const int below_over = __shfl(over, s.below >= 0 ? s.below : 0, 64);
    const size_t g = (size_t)b * L + s.res;
    const double *rT = sT + g * N, *rC = sC + g * 18 * N;
    for (int e = lane; e < N; e += 64) out_T[(size_t)b * N + e] = rT[e];
    for (int e = lane; e < 18 * N; e += 64) out_C[(size_t)b * 18 * N + e] = rC[e];
    double *o = res + (size_t)b * RES_WORDS;
    if (lane < TW) o[8 + lane] = info[g * TW + lane];
    if (lane == 0) {
        state[b] = s;
        double d = 0.0;
        for (int i = 0; i < N; i++) d += rT[i];
        o[0] = isdf_host::tr_candidate(s.a, s.b, L, s.res);
        o[1] = s.below >= 0 ? isdf_host::tr_candidate(s.a, s.b, L, s.below) : NAN;
        o[2] = (double)s.status; o[3] = (double)s.rounds; o[4] = (double)s.nonmono;
        o[5] = s.below >= 0 ? (double)below_over : 0.0;
        o[6] = aux[(size_t)b * ST_WORDS]; o[7] = d;
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------
using namespace traj_call;
constexpr const char *BAD_DURATION = "trajectory retime: a duration is not positive and finite";

// what can be said without a ctx
int check_args(isdf_ctx *c, long long B, int N, const void *T, const void *coeffs, const isdf_traj_retime_params *p, const void *T_out,
               const void *coeffs_out, bool batch) {
    if (B < 1 || N < 1 || !T || !coeffs) return fail(c, ISDF_ERR_INVALID_ARG, "trajectory retime: null trajectory");
    if (!T_out || !coeffs_out) return fail(c, ISDF_ERR_INVALID_ARG, "trajectory retime: null output");
    if (isdf_host::tr_check_params(p))
        return fail(c, ISDF_ERR_INVALID_ARG, "trajectory retime: s_lo must be positive and finite, s_hi finite and above it, ladder 2..64, rounds 1..4");
    if (batch && p && p->check) return fail(c, ISDF_ERR_INVALID_ARG, "trajectory retime: no clearance check in the batch form");
    const long long L = p ? p->ladder : 32;
    if (B > ISDF_TRAJ_RETIME_MAX_PIECES || B * L * N > ISDF_TRAJ_RETIME_MAX_PIECES)
        return fail(c, ISDF_ERR_INVALID_ARG, "trajectory retime: B x ladder x N above ISDF_TRAJ_RETIME_MAX_PIECES");
    return ISDF_OK;
}
int ctx_gate(isdf_ctx *c, const isdf_traj_retime_params &P) {
    ISDF_TRY(check_ctx(c, "trajectory retime: null ctx", "trajectory retime on a multi-device ctx"));
    if (P.check) ISDF_TRY(isdf_traj_check_ready(c));
    return ISDF_OK;
}

// the search over device arrays: everything queued on st, then ONE synchronisation
int retime_run(isdf_ctx *c, TrajRetimeState *k, int B, int N, const double *d_T, const double *d_C, const isdf_traj_retime_params &P, const Out &out,
               isdf_traj_retime_info *infos, hipStream_t st) {
    const int L = P.ladder, R = P.rounds;
    const size_t cand = (size_t)B * L, nT = cand * N, n_res = (size_t)B * RES_WORDS, n_aux = (size_t)B * ST_WORDS;
    ISDF_TRY(k->d_scaled.reserve(c, 19 * nT));
    ISDF_TRY(k->d_piece.reserve(c, 12 * nT));
    ISDF_TRY(k->d_info.reserve(c, cand * TW));
    ISDF_TRY(k->d_state.reserve(c, (size_t)B));
    ISDF_TRY(k->d_aux.reserve(c, n_aux));
    ISDF_TRY(k->d_res.reserve(c, n_res));
    double *sT = k->d_scaled, *sC = k->d_scaled + nT;
    TRLimits lim;
    isdf_host::tl_limits(&P.limits, c->cfg, lim.limit);
    const long long threads = (long long)cand * 19 * N;
    HIPCHK(c, hipEventRecord(k->ev[0], st));
    hipLaunchKernelGGL(tr_begin_kernel, dim3((unsigned)B), dim3(64), 0, st, N, d_T, P.s_lo, P.s_hi, k->d_state.get(), k->d_aux.get());
    for (int round = 0; round < R; round++) {
        hipLaunchKernelGGL(tr_scale_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, B, N, L, d_T, d_C,
                           (const TRState *)k->d_state.get(), sT, sC);
        ISDF_TRY(isdf_traj_limits_launch(c, (int)cand, N, sT, sC, &P.limits, k->d_piece, k->d_info, st));
        hipLaunchKernelGGL(tr_pick_kernel, dim3((unsigned)B), dim3(64), 0, st, N, L, round, R, lim, (const double *)k->d_info.get(),
                           (const double *)sT, (const double *)sC, k->d_state.get(), (const double *)k->d_aux.get(), out.d_T, out.d_C, k->d_res.get());
    }
    double *h_res = k->host_words(n_res + n_aux), *h_aux = h_res + n_res;
    float ms = 0.f;
    ISDF_TRY(finish(c, k, st, {{h_res, k->d_res, n_res}, {h_aux, k->d_aux, n_aux}, {out.h_T, out.d_T, (size_t)B * N}, {out.h_C, out.d_C, (size_t)B * 18 * N}}, &ms));
    for (int b = 0; b < B; b++)
        if (h_aux[(size_t)b * ST_WORDS + 1] != 0.0) return fail(c, ISDF_ERR_INVALID_ARG, BAD_DURATION);
    if (infos) for (int b = 0; b < B; b++) {
        isdf_traj_retime_info *info = infos + b;
        const double *w = h_res + (size_t)b * RES_WORDS;
        std::memset(info, 0, sizeof(*info));
        info->scale = w[0]; info->scale_below = w[1]; info->status = (int32_t)w[2]; info->rounds = (int32_t)w[3];
        info->candidates = L * info->rounds; info->nonmonotone = (int32_t)w[4]; info->binding = (int32_t)w[5];
        info->duration_in = w[6]; info->duration_out = w[7];
        isdf_traj_limits_unpack(c->cfg, &P.limits, w + 8, &info->limits);
        info->device_ms = ms;
    }
    return ISDF_OK;
}

// the host-array forms: inputs up, the search, results down
int retime_host_arrays(isdf_ctx *c, int B, int N, const double *T, const double *coeffs, const isdf_traj_retime_params &P, double *T_out,
                       double *coeffs_out, isdf_traj_retime_info *infos) {
    TrajRetimeState *k;
    ISDF_TRY(state_of(c, c->trt, &k));
    hipStream_t st = c->stream;
    const size_t nT = (size_t)B * N;
    ISDF_TRY(k->d_out.reserve(c, 19 * nT));
    ISDF_TRY(upload(c, k->d_in, nT, T, coeffs, st));
    ISDF_TRY(retime_run(c, k, B, N, k->d_in, k->d_in + nT, P, Out{k->d_out, k->d_out + nT, T_out, coeffs_out}, infos, st));
    return P.check ? post_check(c, N, k->d_out, k->d_out + nT, infos, st) : ISDF_OK;
}

}  // namespace

extern "C" void isdf_traj_retime_params_default(isdf_traj_retime_params *p) {
    if (p) isdf_host::tr_params_default(p);
}

extern "C" void isdf_traj_retime_sizes(int out[2]) {
    if (!out) return;
    out[0] = (int)sizeof(isdf_traj_retime_params); out[1] = (int)sizeof(isdf_traj_retime_info);
}

extern "C" int isdf_traj_retime_batch(isdf_ctx *c, int B, int N, const double *T, const double *coeffs, const isdf_traj_retime_params *p,
                                      double *T_out, double *coeffs_out, isdf_traj_retime_info *infos_out) {
    ISDF_TRY(check_args(c, B, N, T, coeffs, p, T_out, coeffs_out, true));
    ISDF_TRY(check_durations(c, (long long)B * N, T, BAD_DURATION));
    const isdf_traj_retime_params P = resolve(p, isdf_host::tr_params_default);
    ISDF_TRY(ctx_gate(c, P));
    return retime_host_arrays(c, B, N, T, coeffs, P, T_out, coeffs_out, infos_out);
}

extern "C" int isdf_traj_retime(isdf_ctx *c, int N, const double *T, const double *coeffs, const isdf_traj_retime_params *p,
                                double *T_out, double *coeffs_out, isdf_traj_retime_info *info_out) {
    ISDF_TRY(check_args(c, 1, N, T, coeffs, p, T_out, coeffs_out, false));
    ISDF_TRY(check_durations(c, N, T, BAD_DURATION));
    const isdf_traj_retime_params P = resolve(p, isdf_host::tr_params_default);
    ISDF_TRY(ctx_gate(c, P));
    if (P.check) {                                  // the slowest candidate must still be a trajectory the check takes
        std::vector<double> slow((size_t)N);
        for (int i = 0; i < N; i++) slow[(size_t)i] = isdf_host::tr_scale_elem(N, i, T[i], P.s_hi);
        ISDF_TRY(swept_check_traj(c, N, slow.data()));
    }
    return retime_host_arrays(c, 1, N, T, coeffs, P, T_out, coeffs_out, info_out);
}

extern "C" int isdf_traj_retime_device(isdf_ctx *c, int N, const double *d_T, const double *d_coeffs, const isdf_traj_retime_params *p,
                                       double *d_T_out, double *d_coeffs_out, isdf_traj_retime_info *info_out, void *stream) {
    ISDF_TRY(check_args(c, 1, N, d_T, d_coeffs, p, d_T_out, d_coeffs_out, false));
    const isdf_traj_retime_params P = resolve(p, isdf_host::tr_params_default);
    ISDF_TRY(ctx_gate(c, P));
    TrajRetimeState *k;
    ISDF_TRY(state_of(c, c->trt, &k));
    hipStream_t st = (hipStream_t)stream;
    ISDF_TRY(retime_run(c, k, 1, N, d_T, d_coeffs, P, Out{d_T_out, d_coeffs_out, nullptr, nullptr}, info_out, st));
    return P.check ? post_check(c, N, d_T_out, d_coeffs_out, info_out, st) : ISDF_OK;
}

extern "C" int isdf_traj_retime_host(const isdf_config *cfg, int N, const double *T, const double *coeffs, const isdf_traj_retime_params *p,
                                     double *T_out, double *coeffs_out, isdf_traj_retime_info *info_out) {
    if (!cfg) return fail(nullptr, ISDF_ERR_INVALID_ARG, "trajectory retime: null configuration");
    const int rc = isdf_host::tr_retime_traj(*cfg, N, T, coeffs, p, T_out, coeffs_out, info_out);
    return rc ? fail(nullptr, rc, "trajectory retime: null argument, a duration that is not positive and finite, or parameters out of range") : ISDF_OK;
}

extern "C" int isdf_traj_scale_host(int N, const double *T, const double *coeffs, double s, double *T_out, double *coeffs_out) {
    const int rc = isdf_host::tr_scale_traj(N, T, coeffs, s, T_out, coeffs_out);
    return rc ? fail(nullptr, rc, "trajectory scale: null argument, a duration or a factor that is not positive and finite") : ISDF_OK;
}
