// Re-allocation of piece durations to the dynamic limits on the device (isdf_traj_realloc*): only the pieces that are over a limit are
// slowed down, the path points stay, MINCO is solved again for the new durations, until the limits report (isdf_traj_limits*,
// csrc/traj_limits.hip) is clean.  The rules - piece factor, update, rounds and status - are stated in include/isdf_accel.h and
// written once, in csrc/traj_realloc_host.hpp, as __host__ __device__ functions: the kernels below and isdf_traj_realloc_host run the
// same text.  The reference has no counterpart (back_end_optimizer.hpp:453-536 penalises, trajectory.hpp:253-390, :631-680 reports).
//
//   solve    one workgroup per trajectory, threads on the junction rows x axes exactly as the callback's cb_pre_body lays them out
//            (csrc/minco_dev_body.hpp: three wavefront groups, one per axis, up to CB_SPLIT_MAX_N pieces; all axes in one thread above)
//            and its pcr_rounds over rows in LDS (1 / T: N, rows: 18 N doubles - the callback kernel's budget without its staged
//            inputs).  Reads the iterate's durations from device memory, writes T | coeffs as the limits report's batch form takes them.
//            N = 1 has no junction system, N = 2 one row and no round.
//   limits   the report's own two launches over the B trajectories (isdf_traj_limits_launch), untouched; the piece rows stay here.
//   update   one wavefront per trajectory, pieces strided over the lanes: a lane judges its pieces with tl_over, forms f_i and stores
//            T_(k+1),i; the union of the pieces' masks is a lane exchange.  A trajectory that is done stores its durations unchanged,
//            so later rounds reproduce its bytes - work that buys the absence of a host decision.  After iterate R the lanes copy the
//            result's arrays and report words.
// 4 (R + 1) launches for any B, nothing between them on the host, no atomics; the scratch lives in the ctx and grows only.
#include "traj_call.hpp"
#include "swept_field.hpp"
#include "minco_dev_body.hpp"
#include "traj_realloc_host.hpp"
#include <cmath>
#include <cstring>
#include <vector>

namespace {
constexpr int CH = ISDF_LIMITS_CHANNELS;
constexpr int TW = ISDF_TL_INFO_WORDS;
constexpr int RES_WORDS = 8 + TW;       // status, rounds, pieces_changed, binding, duration_in, duration_out, max_factor, bad duration | the report's words
struct RADevState { isdf_host::RAState s; int bad, reserved; };     // bad: a duration of the input is not positive and finite
}  // namespace

struct TrajReallocState : traj_call::State {    // d_in: heads | tails | Q | T of every trajectory of the call; d_out: the results, T | coeffs
    DevBuf<double> d_trj;               // the iterate: [B] T | [B] coeffs
    DevBuf<double> d_tnext;             // [B N]
    DevBuf<double> d_piece;             // [B N][12]
    DevBuf<double> d_info;              // [B][TW]
    DevBuf<RADevState> d_state;         // [B]
    DevBuf<double> d_res;               // [B][RES_WORDS]
};

namespace {
using isdf_host::RAState;
using mpcr::M2;

struct RASolve {
    int N;
    const double *head, *tail, *Q;      // [B][9], [B][9], [B][N - 1][3]
    const double *T_src;                // [B][N] the iterate's durations
    double *T_dst, *C;                  // [B][N], [B][6N x 3 column-major]
};
struct RALimits { double limit[CH]; };
struct RAUpdate {
    int N, k, R;
    double headroom, f_max;
    const double *T_in;                 // [B][N] the call's durations
    const double *T_cur, *C_cur;        // the iterate
    const double *piece, *info;         // its report
    double *T_next;                     // [B][N]
    RADevState *state;                  // [B]
    double *out_T, *out_C, *res;        // the B results, laid out like the iterate; [B][RES_WORDS]
};

bool ra_split(int N) { return N <= CB_SPLIT_MAX_N; }
int ra_threads(int N) { return ((N + 63) / 64) * 64 * (ra_split(N) ? 3 : 1); }

template <bool SPLIT> __global__ __launch_bounds__(SPLIT ? 1024 : 448) void ra_solve_kernel(const RASolve A) {
    extern __shared__ double s_mem[];
    const int b = blockIdx.x, N = A.N, n = N - 1;
    const int NT = SPLIT ? (int)blockDim.x / 3 : (int)blockDim.x;
    const int ax = (int)threadIdx.x / NT;
    const int k = ax < (SPLIT ? 3 : 1) ? (int)threadIdx.x % NT : N;
    constexpr int ND = SPLIT ? 1 : 3;           // axes of this thread: d0 .. d0 + ND - 1
    const int d0 = SPLIT ? ax : 0;
    const bool lead = ax == 0;                  // the thread of a row that writes what the axes share
    const double *head = A.head + (size_t)b * 9, *tail = A.tail + (size_t)b * 9;
    const double *Q = A.Q + (size_t)b * 3 * (size_t)n;       // (N = 1: never read)
    double *s_h = s_mem;                        // [N]
    double *s_row = s_mem + N;                  // [N][SH_ROW] rows 1..N-1; later the junction states [(N + 1)][6]

    double T = 1.0, h = 1.0;
    if (k < N) {
        T = A.T_src[(size_t)b * N + k];
        h = mpcr::rcp(T);
        if (lead) { s_h[k] = h; A.T_dst[(size_t)b * N + k] = T; }
    }
    __syncthreads();
    // ---- junction k (between pieces k - 1 and k), 1 <= k <= N - 1
    const bool row = k >= 1 && k <= n;
    M2 L{0, 0, 0, 0}, D{1, 0, 0, 1}, U{0, 0, 0, 0};
    double r[ND][2] = {}, pk[ND] = {}, pn[ND] = {};      // waypoints k and k + 1 (this thread's piece)
    if (k < N) _Pragma("unroll") for (int l = 0, d = d0; l < ND; l++, d++) {
        pk[l] = isdf_host::ra_waypoint(N, head, tail, Q, k, d); pn[l] = isdf_host::ra_waypoint(N, head, tail, Q, k + 1, d);
    }
    if (row) {
        const double hl = s_h[k - 1], hr = h;
        mpcr::junction_blocks(hl, hr, L, D, U);
        _Pragma("unroll") for (int l = 0, d = d0; l < ND; l++, d++) {
            const double pl = isdf_host::ra_waypoint(N, head, tail, Q, k - 1, d);
            mpcr::junction_rhs1(hl, hr, pk[l] - pl, pn[l] - pk[l], r[l]);
            if (k == 1) { const double va[2] = {head[3 + d], head[6 + d]}; double y[2]; cbd::mv(L, va, y); r[l][0] -= y[0]; r[l][1] -= y[1]; }
            if (k == n) { const double va[2] = {tail[3 + d], tail[6 + d]}; double y[2]; cbd::mv(U, va, y); r[l][0] -= y[0]; r[l][1] -= y[1]; }
        }
        if (k == 1) L = {0, 0, 0, 0};
        if (k == n) U = {0, 0, 0, 0};
    }
    cbd::pcr_rounds<ND>(row, lead, k, n, d0, L, D, U, r, s_row);
    // ---- the rows stand alone: u = D^-1 r; the junction states of every waypoint into LDS
    double *s_u = s_row;                        // [(N + 1)][6]: (v, a) per axis
    double uk[ND][2] = {};
    if (row) {
        const M2 i = mpcr::inv(D);
        _Pragma("unroll") for (int l = 0; l < ND; l++) cbd::mv(i, r[l], uk[l]);
    } else if (k == 0) {
        _Pragma("unroll") for (int l = 0, d = d0; l < ND; l++, d++) { uk[l][0] = head[3 + d]; uk[l][1] = head[6 + d]; }
    }
    if (k < N) _Pragma("unroll") for (int l = 0, d = d0; l < ND; l++, d++) { s_u[6 * k + 2 * d] = uk[l][0]; s_u[6 * k + 2 * d + 1] = uk[l][1]; }
    if (k == 0) _Pragma("unroll") for (int l = 0, d = d0; l < ND; l++, d++) { s_u[6 * N + 2 * d] = tail[3 + d]; s_u[6 * N + 2 * d + 1] = tail[6 + d]; }
    __syncthreads();
    // ---- piece k: its coefficients
    if (k < N) {
        double *C = A.C + (size_t)b * 18 * N + 6 * (size_t)k;
        _Pragma("unroll") for (int l = 0, d = d0; l < ND; l++, d++) {
            double c[6];
            mpcr::hermite(T, h, pk[l], uk[l][0], uk[l][1], pn[l], s_u[6 * (k + 1) + 2 * d], s_u[6 * (k + 1) + 2 * d + 1], c);
            for (int q = 0; q < 6; q++) C[(size_t)d * 6 * N + q] = c[q];
        }
    }
}

__global__ __launch_bounds__(64) void ra_update_kernel(const RAUpdate A, const RALimits lim) {
    const int b = blockIdx.x, lane = threadIdx.x, N = A.N;
    const double *Tc = A.T_cur + (size_t)b * N, *rows = A.piece + 12 * (size_t)b * N;
    RADevState ds;                                  // every lane the same state: no exchange
    if (A.k == 0) { isdf_host::ra_begin(ds.s); ds.bad = 0; ds.reserved = 0; }
    else ds = A.state[b];
    const bool was_done = ds.s.done != 0;
    int over = 0, bad = 0;
    for (int i = lane; i < N; i += 64) {
        const double t = Tc[i];
        int m = 0;
        const double f = isdf_host::ra_piece_factor(rows + 12 * (size_t)i, lim.limit, A.headroom, A.f_max, &m);
        over |= m;
        bad |= (!(t > 0.0) || !isdf_host::ra_finite(t)) ? 1 : 0;
        if (A.k < A.R) A.T_next[(size_t)b * N + i] = was_done ? t : isdf_host::ra_update(t, f);     // (nothing over: f is exactly 1)
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) { over |= __shfl_xor(over, off, 64); bad |= __shfl_xor(bad, off, 64); }
    if (A.k == 0) ds.bad = bad;
    (void)isdf_host::ra_advance(ds.s, over, A.k, A.R);
    if (A.k < A.R) { if (lane == 0) A.state[b] = ds; return; }
    // the last iterate: a trajectory that was done early kept its durations, so this iterate is its result again
    const double *Ti = A.T_in + (size_t)b * N, *Cc = A.C_cur + (size_t)b * 18 * N;
    int changed = 0;
    double mf = 0.0;
    for (int i = lane; i < N; i += 64) {
        const double t = Tc[i], t0 = Ti[i];
        A.out_T[(size_t)b * N + i] = t;
        changed += t != t0 ? 1 : 0;
        mf = fmax(mf, t / t0);
    }
    for (int e = lane; e < 18 * N; e += 64) A.out_C[(size_t)b * 18 * N + e] = Cc[e];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) { changed += __shfl_xor(changed, off, 64); mf = fmax(mf, __shfl_xor(mf, off, 64)); }
    double *o = A.res + (size_t)b * RES_WORDS;
    if (lane < TW) o[8 + lane] = A.info[(size_t)b * TW + lane];
    if (lane == 0) {
        A.state[b] = ds;
        double din = 0.0, dout = 0.0;               // summed in order, as the host form does
        for (int i = 0; i < N; i++) { din += Ti[i]; dout += Tc[i]; }
        o[0] = (double)ds.s.status; o[1] = (double)ds.s.rounds; o[2] = (double)changed; o[3] = (double)ds.s.binding;
        o[4] = din; o[5] = dout; o[6] = mf; o[7] = (double)ds.bad;
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------
using namespace traj_call;
constexpr const char *BAD_DURATION = "trajectory realloc: a duration is not positive and finite";

// what can be said without a ctx
int check_args(isdf_ctx *c, long long B, int N, const double *head, const double *tail, const double *Q, const double *T,
               const isdf_traj_realloc_params *p, const double *T_out, const double *C_out, bool batch) {
    if (isdf_host::ra_check_args(B, N, head, tail, Q, T, T_out, C_out)) return fail(c, ISDF_ERR_INVALID_ARG, "trajectory realloc: null argument, B < 1 or N < 1");
    if (isdf_host::ra_check_params(p))
        return fail(c, ISDF_ERR_INVALID_ARG, "trajectory realloc: rounds 1..16, headroom finite and >= 0, f_max finite and above 1");
    if (batch && p && p->check) return fail(c, ISDF_ERR_INVALID_ARG, "trajectory realloc: no clearance check in the batch form");
    if (N > ISDF_TRAJ_REALLOC_MAX_N) return fail(c, ISDF_ERR_INVALID_ARG, "trajectory realloc: N above ISDF_TRAJ_REALLOC_MAX_N on the device (the host form takes any N)");
    const size_t nT = (size_t)B * N;
    if (isdf_host::ra_overlaps_inputs(T_out, nT, B, N, head, tail, Q, T) || isdf_host::ra_overlaps_inputs(C_out, 18 * nT, B, N, head, tail, Q, T) ||
        isdf_host::ra_overlap(T_out, nT * sizeof(double), C_out, 18 * nT * sizeof(double)))
        return fail(c, ISDF_ERR_INVALID_ARG, "trajectory realloc: an output overlaps an input or the other output");
    return ISDF_OK;
}
int ctx_gate(isdf_ctx *c, const isdf_traj_realloc_params &P) {
    ISDF_TRY(check_ctx(c, "trajectory realloc: null ctx", "trajectory realloc on a multi-device ctx"));
    if (P.check) ISDF_TRY(isdf_traj_check_ready(c));
    return ISDF_OK;
}

// the loop over device arrays: everything queued on st, then ONE synchronisation
int realloc_run(isdf_ctx *c, TrajReallocState *s, int B, int N, const double *d_head, const double *d_tail, const double *d_Q, const double *d_T,
                const isdf_traj_realloc_params &P, const Out &out, isdf_traj_realloc_info *infos, hipStream_t st) {
    const int R = P.rounds;
    const size_t nT = (size_t)B * N, n_res = (size_t)B * RES_WORDS;
    ISDF_TRY(s->d_trj.reserve(c, 19 * nT));
    ISDF_TRY(s->d_tnext.reserve(c, nT));
    ISDF_TRY(s->d_piece.reserve(c, 12 * nT));
    ISDF_TRY(s->d_info.reserve(c, (size_t)B * TW));
    ISDF_TRY(s->d_state.reserve(c, (size_t)B));
    ISDF_TRY(s->d_res.reserve(c, n_res));
    double *cT = s->d_trj, *cC = s->d_trj + nT;
    RALimits lim;
    isdf_host::tl_limits(&P.limits, c->cfg, lim.limit);
    RASolve S{N, d_head, d_tail, d_Q, d_T, cT, cC};
    RAUpdate U{};
    U.N = N; U.R = R; U.headroom = P.headroom; U.f_max = P.f_max; U.T_in = d_T; U.T_cur = cT; U.C_cur = cC;
    U.piece = s->d_piece; U.info = s->d_info; U.T_next = s->d_tnext; U.state = s->d_state; U.out_T = out.d_T; U.out_C = out.d_C; U.res = s->d_res;
    const bool split = ra_split(N);
    const size_t lds = cbd::cb_lds_doubles(N, false) * sizeof(double);
    HIPCHK(c, hipEventRecord(s->ev[0], st));
    for (int k = 0; k <= R; k++) {
        if (split) hipLaunchKernelGGL(ra_solve_kernel<true>, dim3((unsigned)B), dim3(ra_threads(N)), lds, st, S);
        else hipLaunchKernelGGL(ra_solve_kernel<false>, dim3((unsigned)B), dim3(ra_threads(N)), lds, st, S);
        ISDF_TRY(isdf_traj_limits_launch(c, B, N, cT, cC, &P.limits, s->d_piece, s->d_info, st));
        U.k = k;
        hipLaunchKernelGGL(ra_update_kernel, dim3((unsigned)B), dim3(64), 0, st, U, lim);
        S.T_src = s->d_tnext;
    }
    double *h_res = s->host_words(n_res);
    float ms = 0.f;
    ISDF_TRY(finish(c, s, st, {{h_res, s->d_res, n_res}, {out.h_T, out.d_T, nT}, {out.h_C, out.d_C, 18 * nT}}, &ms));
    for (int b = 0; b < B; b++)
        if (h_res[(size_t)b * RES_WORDS + 7] != 0.0) return fail(c, ISDF_ERR_INVALID_ARG, BAD_DURATION);
    if (infos) for (int b = 0; b < B; b++) {
        isdf_traj_realloc_info *info = infos + b;
        const double *w = h_res + (size_t)b * RES_WORDS;
        std::memset(info, 0, sizeof(*info));
        info->status = (int32_t)w[0]; info->rounds = (int32_t)w[1]; info->pieces_changed = (int32_t)w[2]; info->binding = (int32_t)w[3];
        info->duration_in = w[4]; info->duration_out = w[5]; info->max_factor = w[6];
        isdf_traj_limits_unpack(c->cfg, &P.limits, w + 8, &info->limits);
        info->device_ms = ms;
    }
    return ISDF_OK;
}

// the host-array forms: inputs up, the loop, results down
int realloc_host_arrays(isdf_ctx *c, int B, int N, const double *heads, const double *tails, const double *Q, const double *T,
                        const isdf_traj_realloc_params &P, double *T_out, double *C_out, isdf_traj_realloc_info *infos) {
    TrajReallocState *s;
    ISDF_TRY(state_of(c, c->tra, &s));
    hipStream_t st = c->stream;
    const size_t b = (size_t)B, nT = b * N, nQ = 3 * b * (size_t)(N - 1);
    ISDF_TRY(s->d_in.reserve(c, 18 * b + nQ + nT));
    ISDF_TRY(s->d_out.reserve(c, 19 * nT));
    double *dh = s->d_in, *dt = dh + 9 * b, *dq = dt + 9 * b, *dT = dq + nQ;
    HIPCHK(c, hipMemcpyAsync(dh, heads, 9 * b * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(dt, tails, 9 * b * sizeof(double), hipMemcpyHostToDevice, st));
    if (nQ) HIPCHK(c, hipMemcpyAsync(dq, Q, nQ * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(dT, T, nT * sizeof(double), hipMemcpyHostToDevice, st));
    ISDF_TRY(realloc_run(c, s, B, N, dh, dt, dq, dT, P, Out{s->d_out, s->d_out + nT, T_out, C_out}, infos, st));
    return P.check ? post_check(c, N, s->d_out, s->d_out + nT, infos, st) : ISDF_OK;
}

}  // namespace

extern "C" void isdf_traj_realloc_params_default(isdf_traj_realloc_params *p) {
    if (p) isdf_host::ra_params_default(p);
}

extern "C" void isdf_traj_realloc_sizes(int out[2]) {
    if (!out) return;
    out[0] = (int)sizeof(isdf_traj_realloc_params); out[1] = (int)sizeof(isdf_traj_realloc_info);
}

extern "C" int isdf_traj_realloc_batch(isdf_ctx *c, int B, int N, const double *heads, const double *tails, const double *Q, const double *T,
                                       const isdf_traj_realloc_params *p, double *T_out, double *coeffs_out, isdf_traj_realloc_info *infos_out) {
    ISDF_TRY(check_args(c, B, N, heads, tails, Q, T, p, T_out, coeffs_out, true));
    ISDF_TRY(check_durations(c, (long long)B * N, T, BAD_DURATION));
    const isdf_traj_realloc_params P = resolve(p, isdf_host::ra_params_default);
    ISDF_TRY(ctx_gate(c, P));
    return realloc_host_arrays(c, B, N, heads, tails, Q, T, P, T_out, coeffs_out, infos_out);
}

extern "C" int isdf_traj_realloc(isdf_ctx *c, int N, const double *head_pva, const double *tail_pva, const double *Q, const double *T,
                                 const isdf_traj_realloc_params *p, double *T_out, double *coeffs_out, isdf_traj_realloc_info *info_out) {
    ISDF_TRY(check_args(c, 1, N, head_pva, tail_pva, Q, T, p, T_out, coeffs_out, false));
    ISDF_TRY(check_durations(c, N, T, BAD_DURATION));
    const isdf_traj_realloc_params P = resolve(p, isdf_host::ra_params_default);
    ISDF_TRY(ctx_gate(c, P));
    if (P.check) ISDF_TRY(swept_check_traj(c, N, T));       // the input must be a trajectory the check takes; the result's total is the check's to judge
    return realloc_host_arrays(c, 1, N, head_pva, tail_pva, Q, T, P, T_out, coeffs_out, info_out);
}

extern "C" int isdf_traj_realloc_device(isdf_ctx *c, int N, const double *d_head_pva, const double *d_tail_pva, const double *d_Q, const double *d_T,
                                        const isdf_traj_realloc_params *p, double *d_T_out, double *d_coeffs_out, isdf_traj_realloc_info *info_out,
                                        void *stream) {
    ISDF_TRY(check_args(c, 1, N, d_head_pva, d_tail_pva, d_Q, d_T, p, d_T_out, d_coeffs_out, false));
    const isdf_traj_realloc_params P = resolve(p, isdf_host::ra_params_default);
    ISDF_TRY(ctx_gate(c, P));
    TrajReallocState *s;
    ISDF_TRY(state_of(c, c->tra, &s));
    hipStream_t st = (hipStream_t)stream;
    ISDF_TRY(realloc_run(c, s, 1, N, d_head_pva, d_tail_pva, d_Q, d_T, P, Out{d_T_out, d_coeffs_out, nullptr, nullptr}, info_out, st));
    return P.check ? post_check(c, N, d_T_out, d_coeffs_out, info_out, st) : ISDF_OK;
}

extern "C" int isdf_traj_realloc_host(const isdf_config *cfg, int N, const double *head_pva, const double *tail_pva, const double *Q, const double *T,
                                      const isdf_traj_realloc_params *p, double *T_out, double *coeffs_out, isdf_traj_realloc_info *info_out) {
    if (!cfg) return fail(nullptr, ISDF_ERR_INVALID_ARG, "trajectory realloc: null configuration");
    const int rc = isdf_host::ra_realloc_traj(*cfg, N, head_pva, tail_pva, Q, T, p, T_out, coeffs_out, info_out);
    return rc ? fail(nullptr, rc, "trajectory realloc: null argument, a duration that is not positive and finite, parameters out of range or overlapping arrays") : ISDF_OK;
}

extern "C" int isdf_traj_minco_host(int N, const double *head_pva, const double *tail_pva, const double *Q, const double *T, double *coeffs_out) {
    const int rc = isdf_host::ra_minco_traj(N, head_pva, tail_pva, Q, T, coeffs_out);
    return rc ? fail(nullptr, rc, "trajectory minco: null argument, or a duration that is not positive and finite") : ISDF_OK;
}
