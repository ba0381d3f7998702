// Dynamic limits of a finished trajectory on the device (isdf_traj_limits*, isdf_traj_sample*): the largest speed, acceleration,
// body rate, tilt and thrust (and the smallest thrust) along the trajectory, and the per-time state behind them.  What the
// reference has of this: Trajectory::getMaxVelRate / getMaxAccRate / checkMaxVelRate / checkMaxAccRate
// (src/utils/include/utils/trajectory.hpp:253-390, :631-680: roots of the speed and acceleration polynomials only) and
// SweptVolumeManager::getStateOnTrajStamp (sw_manager.hpp:307-341) over FlatnessMap::optimizated_forward / forward
// (flatness.hpp:88-148, :203-206).  The rules - coarse samples, brackets, golden section, tie rules - are stated in
// include/isdf_accel.h; csrc/traj_limits_host.hpp restates them in plain host code.
//
//   pieces   one wavefront per (trajectory, piece), TL_WAVES of them per workgroup.  A pass puts 64 consecutive coarse samples
//            on the 64 lanes; lanes 1..62 OWN theirs and see the two neighbours' values through a lane exchange, so no lane holds
//            more than its own three-sample window and passes advance by 62 samples (lanes 0 and 63 only lend their values).
//            An owner refines every channel whose sample starts a bracket and keeps the best (value, time) per channel; the
//            channel of a refinement is a run-time value, so lanes refining different channels run the same code.  Each
//            channel ends in a wave argmax: larger value, then smaller time.  Lane 0 writes the piece's 12 doubles.
//   report   one wavefront per trajectory: the pieces' rows -> per channel (value, time, piece, pieces over the limit); larger
//            value, then smaller time, then the earlier piece.  A total order, maxima and integer sums only: the report does
//            not depend on the launch geometry or on the trajectory's place in a batch.
// Two launches per call whatever B is; the scratch lives in the ctx (TrajLimitsState) and grows only.
#include "traj_call.hpp"
#include "traj_limits_host.hpp"
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

struct TrajLimitsState : traj_call::State {     // d_in: T | coeffs of every trajectory of the call; d_out: unused
    DevBuf<double> d_piece;         // [B N][12]
    DevBuf<double> d_info;          // [B][INFO_WORDS]
    DevBuf<double> d_samp;          // sampler, host form: stamps | rows
    std::vector<double> h_T;
};

namespace {

constexpr int CH = ISDF_LIMITS_CHANNELS;
constexpr int TL_WAVES = 4;              // pieces per workgroup
constexpr int OWNED = 62;                // samples a pass advances by
constexpr int INFO_WORDS = 4 * CH;       // per channel: value, time, piece, pieces over the limit
constexpr double GOLD = isdf_host::TL_GOLD;

struct TLArgs {
    FlatP flat;
    int B, N, S;
    double tol_t;
    const double *T, *C;
    double *piece;
};
struct TLLimits { double limit[CH]; };

// larger value, then smaller time
__device__ __forceinline__ void take(double &bv, double &bt, double v, double t) {
    if (v > bv || (v == bv && t < bt)) { bv = v; bt = t; }
}
__device__ __forceinline__ double sample_time(double T, int S, int j) { return j <= 0 ? 0.0 : (j >= S ? T : (double)j * T / (double)S); }

// the six channels in the form that is maximised: squared norms, tilt, thrust, -thrust
__device__ __forceinline__ void channels(const FlatP &P, const TrajView &tr, int piece, double s, double (&f)[CH]) {
    d3 pos, v, a, j;
    traj_eval(tr, piece, s, pos, v, a, j);
    FlatS fs; FlatS2 ft;
    flat_core(P, v, a, fs);
    flat_core2(P, v, a, j, fs, ft);
    const d4 q = flat_quat(fs);
    const d3 w = flat_omg(fs, ft);
    const double thr = flat_thrust(P, v, a, fs);
    f[0] = dot3(v, v); f[1] = dot3(a, a); f[2] = dot3(w, w);
    f[3] = acos(1.0 - 2.0 * (q.x * q.x + q.y * q.y));
    f[4] = thr; f[5] = -thr;
}
// one of them, picked at run time (a chain of selects: no indexed array, nothing in scratch)
__device__ __forceinline__ double channel(const FlatP &P, const TrajView &tr, int piece, double s, int ch) {
    double f[CH];
    channels(P, tr, piece, s, f);
    double r = f[0];
#pragma unroll
    for (int c = 1; c < CH; c++) r = ch == c ? f[c] : r;
    return r;
}

// golden section for the maximum of channel ch on [a, b]; every evaluation is offered to (bv, bt)
__device__ __forceinline__ void refine(const FlatP &P, const TrajView &tr, int piece, int ch, double a, double b, double stop, double &bv, double &bt) {
    double x1 = b - GOLD * (b - a), x2 = a + GOLD * (b - a);
    double f1 = channel(P, tr, piece, x1, ch), f2 = channel(P, tr, piece, x2, ch);
    take(bv, bt, f1, x1); take(bv, bt, f2, x2);
    for (int it = 0; it < isdf_host::TL_MAX_ITERS && !(b - a < stop); it++) {
        // (one evaluation per iteration, at the new inner point)
        const bool left = f1 >= f2;
        if (left) { b = x2; x2 = x1; f2 = f1; x1 = b - GOLD * (b - a); }
        else      { a = x1; x1 = x2; f1 = f2; x2 = a + GOLD * (b - a); }
        const double x = left ? x1 : x2;
        const double f = channel(P, tr, piece, x, ch);
        if (left) f1 = f; else f2 = f;
        take(bv, bt, f, x);
    }
}

__global__ __launch_bounds__(64 * TL_WAVES) void tl_piece_kernel(TLArgs A) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long g = (long long)blockIdx.x * TL_WAVES + wave;
    if (g >= (long long)A.B * A.N) return;          // the whole wavefront
    const int b = (int)(g / A.N), i = (int)(g - (long long)b * A.N);
    TrajView tr;
    tr.T = A.T + (size_t)b * A.N; tr.C = A.C + (size_t)b * 18 * A.N; tr.N = A.N;
    const double Ti = tr.T[i], stop = A.tol_t * Ti;
    double t0 = 0.0;                                // start of the piece: the durations before it, summed in order
    for (int k = 0; k < i; k++) t0 += tr.T[k];
    const int S = A.S;
    double bv[CH], bt[CH];
#pragma unroll
    for (int c = 0; c < CH; c++) { bv[c] = -INFINITY; bt[c] = 0.0; }
    for (int base = 0; base <= S; base += OWNED) {
        const int j = base - 1 + lane;              // lane 0: the sample before the pass's first, lane 63: the one after its last
        const bool owner = lane >= 1 && lane <= OWNED && j <= S;
        const double sj = sample_time(Ti, S, j);    // (clamps j to 0..S)
        double f[CH];
        channels(A.flat, tr, i, sj, f);
        unsigned mask = 0;
#pragma unroll
        for (int c = 0; c < CH; c++) {
            const double fm = __shfl_up(f[c], 1, 64), fp = __shfl_down(f[c], 1, 64);
            if (owner) {
                take(bv[c], bt[c], f[c], sj);
                if (j == 0 || j == S || (f[c] >= fm && f[c] >= fp)) mask |= 1u << c;
            }
        }
        const double lo = sample_time(Ti, S, j - 1), hi = sample_time(Ti, S, j + 1);
        while (mask) {
            const int ch = __ffs(mask) - 1;
            mask &= mask - 1;
            double rv = -INFINITY, rt = 0.0;
            refine(A.flat, tr, i, ch, lo, hi, stop, rv, rt);
#pragma unroll
            for (int c = 0; c < CH; c++) if (c == ch) take(bv[c], bt[c], rv, rt);
        }
    }
    // wave argmax per channel: larger value, then smaller time
#pragma unroll
    for (int c = 0; c < CH; c++) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double ov = __shfl_xor(bv[c], off, 64), ot = __shfl_xor(bt[c], off, 64);
            take(bv[c], bt[c], ov, ot);
        }
    }
    if (lane == 0) {
        double *o = A.piece + 12 * (size_t)g;
#pragma unroll
        for (int c = 0; c < CH; c++) {
            o[2 * c] = c <= ISDF_LIMIT_OMG ? sqrt(bv[c]) : (c == ISDF_LIMIT_THRUST_MIN ? -bv[c] : bv[c]);
            o[2 * c + 1] = t0 + bt[c];
        }
    }
}

// larger key, then smaller time, then the earlier piece
__device__ __forceinline__ bool better(double k, double t, int p, double bk, double bt, int bp) {
    return k > bk || (k == bk && (t < bt || (t == bt && p < bp)));
}
__global__ __launch_bounds__(64) void tl_traj_kernel(int N, const double *__restrict__ piece, TLLimits L, double *__restrict__ info) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const double *rows = piece + 12 * (size_t)b * N;
#pragma unroll
    for (int c = 0; c < CH; c++) {
        const bool is_min = c == ISDF_LIMIT_THRUST_MIN;
        const double lim = L.limit[c];
        double bk = -INFINITY, bt = 0.0;
        int bp = INT_MAX, over = 0;
        for (int i = lane; i < N; i += 64) {
            const double v = rows[12 * (size_t)i + 2 * c], t = rows[12 * (size_t)i + 2 * c + 1];
            const double k = is_min ? -v : v;
            if (better(k, t, i, bk, bt, bp)) { bk = k; bt = t; bp = i; }
            over += (is_min ? v < lim : v > lim) ? 1 : 0;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double ok = __shfl_xor(bk, off, 64), ot = __shfl_xor(bt, off, 64);
            const int op = __shfl_xor(bp, off, 64);
            if (better(ok, ot, op, bk, bt, bp)) { bk = ok; bt = ot; bp = op; }
            over += __shfl_xor(over, off, 64);
        }
        if (lane == 0) {
            double *o = info + (size_t)b * INFO_WORDS + 4 * c;
            o[0] = is_min ? -bk : bk; o[1] = bt; o[2] = bp == INT_MAX ? -1.0 : (double)bp; o[3] = (double)over;
        }
    }
}

// one lane per stamp
__global__ __launch_bounds__(256) void tl_sample_kernel(FlatP P, TrajView tr, long long n, const double *__restrict__ t, double *__restrict__ rows) {
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    double s = t[k < n ? k : n - 1];                // (every lane walks the pieces: traj_locate is a wave-uniform loop)
    const int piece = traj_locate(tr, s);
    d3 pos, v, a, j;
    traj_eval(tr, piece, s, pos, v, a, j);
    FlatS fs; FlatS2 ft;
    flat_core(P, v, a, fs);
    flat_core2(P, v, a, j, fs, ft);
    const d4 q = flat_quat(fs);
    const d3 w = flat_omg(fs, ft);
    const double thr = flat_thrust(P, v, a, fs);
    if (k >= n) return;
    double *o = rows + ISDF_TRAJ_SAMPLE_ROW * (size_t)k;
    o[0] = pos.x; o[1] = pos.y; o[2] = pos.z; o[3] = v.x; o[4] = v.y; o[5] = v.z; o[6] = a.x; o[7] = a.y; o[8] = a.z;
    o[9] = j.x; o[10] = j.y; o[11] = j.z; o[12] = q.w; o[13] = q.x; o[14] = q.y; o[15] = q.z; o[16] = w.x; o[17] = w.y; o[18] = w.z;
    o[19] = thr;
}

// ---- host ---------------------------------------------------------------------------------------------------------------
using namespace traj_call;

int limits_ctx(isdf_ctx *c) { return check_ctx(c, "trajectory limits: null ctx", "trajectory limits on a multi-device ctx"); }
int sample_ctx(isdf_ctx *c) { return check_ctx(c, "trajectory sample: null ctx", "trajectory sample on a multi-device ctx"); }

// the two launches of B trajectories on device arrays, nothing else: no event, no copy, no synchronisation
int limits_launch(isdf_ctx *c, int B, int N, const double *d_T, const double *d_C, const isdf_traj_limits_params *p, double *d_piece, double *d_info,
                  hipStream_t st) {
    const size_t pieces = (size_t)B * N;
    TLArgs A{};
    isdf_fill_flat(c->cfg, A.flat);
    A.B = B; A.N = N; A.S = isdf_host::tl_samples(p, c->cfg); A.tol_t = isdf_host::tl_tol(p);
    A.T = d_T; A.C = d_C; A.piece = d_piece;
    TLLimits L;
    isdf_host::tl_limits(p, c->cfg, L.limit);
    hipLaunchKernelGGL(tl_piece_kernel, dim3((unsigned)((pieces + TL_WAVES - 1) / TL_WAVES)), dim3(64 * TL_WAVES), 0, st, A);
    hipLaunchKernelGGL(tl_traj_kernel, dim3((unsigned)B), dim3(64), 0, st, N, (const double *)d_piece, L, d_info);
    HIPCHK(c, hipGetLastError());
    return ISDF_OK;
}
// a trajectory's INFO_WORDS -> its info (device_ms left 0)
void limits_unpack(const isdf_config &cfg, const isdf_traj_limits_params *p, const double *w, isdf_traj_limits_info *info) {
    double limit[CH];
    isdf_host::tl_limits(p, cfg, limit);
    std::memset(info, 0, sizeof(*info));
    for (int ch = 0; ch < CH; ch++) {
        info->value[ch] = w[4 * ch]; info->time[ch] = w[4 * ch + 1]; info->piece[ch] = (int32_t)w[4 * ch + 2];
        info->n_pieces_over[ch] = (int32_t)w[4 * ch + 3]; info->limit[ch] = limit[ch];
        if (!std::isnan(limit[ch])) {
            info->judged |= 1 << ch;
            if (!isdf_host::tl_over(ch, info->value[ch], limit[ch])) info->feasible |= 1 << ch;
        }
    }
    info->samples = isdf_host::tl_samples(p, cfg); info->tol_t = isdf_host::tl_tol(p);
}

// the report of B trajectories on device arrays.  d_piece: B N x 12 on the device, or null (the state's own)
int limits_run(isdf_ctx *c, TrajLimitsState *k, int B, int N, const double *d_T, const double *d_C, const isdf_traj_limits_params *p,
               isdf_traj_limits_info *infos, double *d_piece, hipStream_t st) {
    const size_t words = (size_t)B * INFO_WORDS;
    if (!d_piece) { ISDF_TRY(k->d_piece.reserve(c, (size_t)B * N * 12)); d_piece = k->d_piece; }
    ISDF_TRY(k->d_info.reserve(c, words));
    HIPCHK(c, hipEventRecord(k->ev[0], st));
    ISDF_TRY(limits_launch(c, B, N, d_T, d_C, p, d_piece, k->d_info, st));
    double *h_info = k->host_words(words);
    float ms = 0.f;
    ISDF_TRY(finish(c, k, st, {{h_info, k->d_info, words}}, &ms));
    if (infos) for (int b = 0; b < B; b++) {
        limits_unpack(c->cfg, p, h_info + (size_t)b * INFO_WORDS, infos + b);
        infos[b].device_ms = ms;
    }
    return ISDF_OK;
}

int check_trajs(isdf_ctx *c, int B, int N, const double *T, const void *coeffs) {
    if (B < 1 || N < 1 || !T || !coeffs) return fail(c, ISDF_ERR_INVALID_ARG, "trajectory limits: null trajectory");
    return check_durations(c, (long long)B * N, T, "trajectory limits: a duration is not positive and finite");
}
// the durations of a device trajectory onto the host, checked
int check_device_traj(isdf_ctx *c, TrajLimitsState *k, int N, const double *d_T, hipStream_t st) {
    if (k->h_T.size() < (size_t)N) k->h_T.resize((size_t)N);
    HIPCHK(c, hipMemcpyAsync(k->h_T.data(), d_T, N * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    return check_trajs(c, 1, N, k->h_T.data(), d_T);
}

}  // namespace

int isdf_traj_limits_launch(isdf_ctx *c, int B, int N, const double *d_T, const double *d_C, const isdf_traj_limits_params *p, double *d_piece,
                            double *d_info, hipStream_t st) {
    return limits_launch(c, B, N, d_T, d_C, p, d_piece, d_info, st);
}
void isdf_traj_limits_unpack(const isdf_config &cfg, const isdf_traj_limits_params *p, const double *words, isdf_traj_limits_info *info) {
    limits_unpack(cfg, p, words, info);
}

extern "C" void isdf_traj_limits_params_default(isdf_traj_limits_params *p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->samples = 0;                         // 4 * cfg.integral_intervs
    p->tol_t = isdf_host::TL_TOL_DEFAULT;
    p->max_acc = p->max_thrust = p->min_thrust = std::nan("");
}

extern "C" void isdf_traj_limits_sizes(int out[2]) {
    if (!out) return;
    out[0] = (int)sizeof(isdf_traj_limits_params); out[1] = (int)sizeof(isdf_traj_limits_info);
}

extern "C" int isdf_traj_limits_batch(isdf_ctx *c, int B, int N, const double *T, const double *coeffs, const isdf_traj_limits_params *p,
                                      isdf_traj_limits_info *infos_out, double *piece_out) {
    ISDF_TRY(check_trajs(c, B, N, T, coeffs));
    ISDF_TRY(limits_ctx(c));
    TrajLimitsState *k;
    ISDF_TRY(state_of(c, c->tlm, &k));
    const size_t nT = (size_t)B * N;
    ISDF_TRY(upload(c, k->d_in, nT, T, coeffs, c->stream));
    ISDF_TRY(limits_run(c, k, B, N, k->d_in, k->d_in + nT, p, infos_out, nullptr, c->stream));
    if (piece_out) HIPCHK(c, hipMemcpy(piece_out, k->d_piece, 12 * nT * sizeof(double), hipMemcpyDeviceToHost));
    return ISDF_OK;
}

extern "C" int isdf_traj_limits(isdf_ctx *c, int N, const double *T, const double *coeffs, const isdf_traj_limits_params *p,
                                isdf_traj_limits_info *info_out, double *piece_out) {
    return isdf_traj_limits_batch(c, 1, N, T, coeffs, p, info_out, piece_out);
}

extern "C" int isdf_traj_limits_device(isdf_ctx *c, int N, const double *d_T, const double *d_coeffs, const isdf_traj_limits_params *p,
                                       isdf_traj_limits_info *info_out, double *d_piece_out, void *stream) {
    if (N < 1 || !d_T || !d_coeffs) return fail(c, ISDF_ERR_INVALID_ARG, "trajectory limits: null trajectory");
    ISDF_TRY(limits_ctx(c));
    TrajLimitsState *k;
    ISDF_TRY(state_of(c, c->tlm, &k));
    hipStream_t st = (hipStream_t)stream;
    ISDF_TRY(check_device_traj(c, k, N, d_T, st));
    return limits_run(c, k, 1, N, d_T, d_coeffs, p, info_out, d_piece_out, st);
}

extern "C" int isdf_traj_limits_host(const isdf_config *cfg, int N, const double *T, const double *coeffs, const isdf_traj_limits_params *p,
                                     isdf_traj_limits_info *info_out, double *piece_out) {
    if (!cfg) return fail(nullptr, ISDF_ERR_INVALID_ARG, "trajectory limits: null configuration");
    const int rc = isdf_host::tl_report_traj(*cfg, N, T, coeffs, p, info_out, piece_out);
    return rc ? fail(nullptr, rc, "trajectory limits: null trajectory, or a duration that is not positive and finite") : ISDF_OK;
}

extern "C" int isdf_traj_sample_device(isdf_ctx *c, int N, const double *d_T, const double *d_coeffs, long long n, const double *d_t,
                                       double *d_rows_out, void *stream) {
    if (N < 1 || !d_T || !d_coeffs || n < 0 || (n > 0 && (!d_t || !d_rows_out))) return fail(c, ISDF_ERR_INVALID_ARG, "trajectory sample: null argument");
    ISDF_TRY(sample_ctx(c));
    TrajLimitsState *k;
    ISDF_TRY(state_of(c, c->tlm, &k));
    hipStream_t st = (hipStream_t)stream;
    ISDF_TRY(check_device_traj(c, k, N, d_T, st));
    if (n == 0) return ISDF_OK;
    FlatP P;
    isdf_fill_flat(c->cfg, P);
    TrajView tr;
    tr.T = d_T; tr.C = d_coeffs; tr.N = N;
    hipLaunchKernelGGL(tl_sample_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, P, tr, n, d_t, d_rows_out);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(st));
    return ISDF_OK;
}

extern "C" int isdf_traj_sample(isdf_ctx *c, int N, const double *T, const double *coeffs, long long n, const double *t, double *rows_out) {
    if (n < 0 || (n > 0 && (!t || !rows_out))) return fail(c, ISDF_ERR_INVALID_ARG, "trajectory sample: null argument");
    ISDF_TRY(check_trajs(c, 1, N, T, coeffs));
    ISDF_TRY(sample_ctx(c));
    if (n == 0) return ISDF_OK;
    TrajLimitsState *k;
    ISDF_TRY(state_of(c, c->tlm, &k));
    hipStream_t st = c->stream;
    const size_t nT = (size_t)N, nn = (size_t)n;
    ISDF_TRY(k->d_samp.reserve(c, (1 + ISDF_TRAJ_SAMPLE_ROW) * nn));
    ISDF_TRY(upload(c, k->d_in, nT, T, coeffs, st));
    HIPCHK(c, hipMemcpyAsync(k->d_samp, t, nn * sizeof(double), hipMemcpyHostToDevice, st));
    FlatP P;
    isdf_fill_flat(c->cfg, P);
    TrajView tr;
    tr.T = k->d_in; tr.C = k->d_in + nT; tr.N = N;
    hipLaunchKernelGGL(tl_sample_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, P, tr, n, (const double *)k->d_samp.get(), k->d_samp + nn);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(rows_out, k->d_samp + nn, ISDF_TRAJ_SAMPLE_ROW * nn * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    return ISDF_OK;
}

extern "C" int isdf_traj_sample_host(const isdf_config *cfg, int N, const double *T, const double *coeffs, long long n, const double *t,
                                     double *rows_out) {
    if (!cfg) return fail(nullptr, ISDF_ERR_INVALID_ARG, "trajectory sample: null configuration");
    const int rc = isdf_host::tl_sample_traj(*cfg, N, T, coeffs, n, t, rows_out);
    return rc ? fail(nullptr, rc, "trajectory sample: null argument, or a duration that is not positive and finite") : ISDF_OK;
}
