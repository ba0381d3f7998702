// Candidate views: isdf_view_candidates, the link between the frontier's clusters and the view gain - for each target a ring
// of eye positions tested on the device, the survivors posed, scored by the view gain's own launches and the best few per target ranked.
//   vc_filter_kernel   one candidate per lane: view_cand_host.hpp's vc_candidate (tests 1 - 5 and the pose), the candidate's row opened,
//                      its pose (zeros unless kept), the flag "kept"; the six status counters through block_sum, one 64-bit atomicAdd per
//                      workgroup per word into the call's record.
//   vc_tally_kernel    one workgroup per target: its six status counts, best_candidate -1 and best_gain 0 into the target's row, its
//                      best list padded with -1 - what a call without a kept candidate returns.
//   (dev_scan.hpp)     exclusive scan of the flags: the place of every kept candidate in the dense table.
//   vc_compact_kernel  the kept poses into the dense table, the candidate index of each.
//   -- the first hand-over: the record.  n_kept sizes the gain's grid and its seen chunks; with zero kept nothing more is launched.
//   (view_gain.hip)    gain_run on the dense table: vg_setup_kernel, then per chunk the clear and vg_gain_kernel, as isdf_view_gain.
//   vc_score_kernel    one kept candidate per lane: the gain row's words 1, 4, 5, 6 into the candidate's row.
//   vc_select_kernel   one workgroup per target, at most k_best rounds: the largest key (gain, then the lower k) below the last round's,
//                      by dev_reduce.hpp's block_max through the wavefronts and LDS - no atomic, so no order to depend on.
//   -- the second hand-over: the rows, poses, target rows and best lists through their pinned copies.
// Nothing here writes to the ctx's map, its known grid, its products or its flags; no kernel waits on another workgroup.
#include "view_gain_run.hpp"
#include "view_cand_host.hpp"
#include "dev_reduce.hpp"
#include "dev_scan.hpp"
#include <algorithm>
#include <cstring>

namespace isdf {

constexpr int VC_BLOCK = 128;               // the filter's workgroup: two wavefronts, the cast's reason (walks of different lengths)
constexpr int VC_WAVES = VC_BLOCK / 64;
constexpr int VC_LANE_BLOCK = 256;          // compaction and scoring: one lane per entry
constexpr int VC_SEL_BLOCK = 256;           // tally and selection: one workgroup per target
constexpr int VC_SEL_WAVES = VC_SEL_BLOCK / 64;

// the call's record, zeroed before the filter and read back after the compaction
struct VcRecord {
    unsigned long long n[VC_STATUSES];      // candidates per status; n[0]: kept
    unsigned long long pad[2];
};
static_assert(sizeof(VcRecord) == 64, "the candidates' record is one 64-byte line");

__global__ __launch_bounds__(VC_BLOCK) void vc_filter_kernel(const double *__restrict__ targets, const double *__restrict__ offsets, long long n_offsets, long long n_cand,
                                                             MapGeom M, const uint8_t *__restrict__ occ, const unsigned *__restrict__ known, long long n_words,
                                                             int clearance, long long *__restrict__ cand, double *__restrict__ poses, int *__restrict__ flag,
                                                             VcRecord *rec) {
    const long long c = (long long)blockIdx.x * VC_BLOCK + threadIdx.x;
    long long cnt[VC_STATUSES] = {0, 0, 0, 0, 0, 0};
    if (c < n_cand) {
        const long long i = c / n_offsets, k = c - i * n_offsets;
        const double t[3] = {targets[3 * i], targets[3 * i + 1], targets[3 * i + 2]}, o[3] = {offsets[3 * k], offsets[3 * k + 1], offsets[3 * k + 2]};
        VcCand C;
        vc_candidate(known, n_words, occ, M, t, o, clearance, C);
        long long row[VC_ROW];
        vc_row_open(C, row);
        for (int w = 0; w < VC_ROW; w++) cand[VC_ROW * c + w] = row[w];
        for (int w = 0; w < 12; w++) poses[12 * c + w] = C.pose[w];
        flag[c] = C.status == VC_KEPT;
        for (int s = 0; s < VC_STATUSES; s++) cnt[s] = C.status == s;
    }
    const unsigned long long s = block_sum<VC_STATUSES, VC_WAVES>(cnt);
    if (s) atomicAdd(&rec->n[threadIdx.x], s);          // (s is 0 beyond the counters)
}

__global__ __launch_bounds__(VC_SEL_BLOCK) void vc_tally_kernel(long long n_offsets, int k_best, const long long *__restrict__ cand, long long *__restrict__ target_rows,
                                                                long long *__restrict__ best) {
    const long long i = blockIdx.x;
    long long cnt[VC_STATUSES] = {0, 0, 0, 0, 0, 0};
    for (long long k = threadIdx.x; k < n_offsets; k += VC_SEL_BLOCK) {
        const long long status = cand[VC_ROW * (i * n_offsets + k)];
        for (int s = 0; s < VC_STATUSES; s++) cnt[s] += status == s;
    }
    const unsigned long long s = block_sum<VC_STATUSES, VC_SEL_WAVES>(cnt);
    long long *const t = target_rows + VC_TARGET_ROW * i;
    if (threadIdx.x < VC_STATUSES) t[threadIdx.x] = (long long)s;
    if (threadIdx.x == 6) t[6] = -1;
    if (threadIdx.x == 7) t[7] = 0;
    if ((int)threadIdx.x < k_best) best[(long long)k_best * i + threadIdx.x] = -1;          // (k_best <= 64)
}

__global__ __launch_bounds__(VC_LANE_BLOCK) void vc_compact_kernel(long long n_cand, const int *__restrict__ flag, const int *__restrict__ pos, const double *__restrict__ poses,
                                                                   double *__restrict__ dense, int *__restrict__ index) {
    const long long c = (long long)blockIdx.x * VC_LANE_BLOCK + threadIdx.x;
    if (c >= n_cand || !flag[c]) return;
    const long long j = pos[c];
    for (int w = 0; w < 12; w++) dense[12 * j + w] = poses[12 * c + w];
    index[j] = (int)c;
}

__global__ __launch_bounds__(VC_LANE_BLOCK) void vc_score_kernel(long long n_kept, const int *__restrict__ index, const long long *__restrict__ gain_rows,
                                                                 long long *__restrict__ cand) {
    const long long j = (long long)blockIdx.x * VC_LANE_BLOCK + threadIdx.x;
    if (j >= n_kept) return;
    const long long *const g = gain_rows + VG_ROW * j;
    long long *const row = cand + (long long)VC_ROW * index[j];
    row[3] = g[1]; row[4] = g[4]; row[5] = g[5]; row[6] = g[6];
}

// cand: word 7 of a ranked candidate is written while other lanes read words 0 and 3 of it - other words
__global__ __launch_bounds__(VC_SEL_BLOCK) void vc_select_kernel(long long n_offsets, int k_best, long long min_gain, long long *cand, long long *__restrict__ target_rows,
                                                                 long long *__restrict__ best) {
    const long long i = blockIdx.x;
    unsigned long long prev = ~0ull;
    for (int r = 0; r < k_best; r++) {
        unsigned long long top = 0;
        for (long long k = threadIdx.x; k < n_offsets; k += VC_SEL_BLOCK) {
            const long long *const row = cand + VC_ROW * (i * n_offsets + k);
            if (row[0] != VC_KEPT || row[3] < min_gain) continue;
            const unsigned long long key = vc_key(row[3], k);
            if (key < prev && key > top) top = key;
        }
        top = block_max<VC_SEL_WAVES>(top);
        if (top == 0) break;                // (uniform: every thread holds the workgroup's maximum)
        if (threadIdx.x == 0) {
            const long long c = i * n_offsets + vc_key_k(top);
            best[(long long)k_best * i + r] = c;
            cand[VC_ROW * c + 7] = r;
            if (r == 0) { target_rows[VC_TARGET_ROW * i + 6] = c; target_rows[VC_TARGET_ROW * i + 7] = vc_key_gain(top); }
        }
        prev = top;
    }
}

}  // namespace isdf

// the inputs' staging, the candidates' rows and poses, the flags and their scan, the dense table and its gain rows, the targets' rows and
// best lists, the call's record and the pinned copies the outputs are handed over through
struct ViewCandState {
    isdf::DevBuf<double> d_targets, d_offsets, d_poses, d_dense;
    isdf::DevBuf<long long> d_cand, d_target_rows, d_best, d_gain_rows;
    isdf::DevBuf<int> d_flag, d_pos, d_index;
    isdf::DevBuf<unsigned char> d_scan_tmp;
    isdf::RecPair<isdf::VcRecord> rec;
    isdf::PinBuf<int64_t> h_cand, h_target_rows, h_best;
    isdf::PinBuf<double> h_poses;
    isdf::DevEvents<2> ev_filter, ev_gain, ev_select;
    int ready(isdf_ctx *c) { ISDF_TRY(ev_filter.ready(c)); ISDF_TRY(ev_gain.ready(c)); ISDF_TRY(ev_select.ready(c)); return rec.ready(c); }
};

using namespace isdf;

extern "C" void isdf_view_candidates_params_default(isdf_view_candidates_params *p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    isdf_view_gain_params_default(&p->gain);
    p->clearance_voxels = 1;
    p->k_best = 3;
    p->min_gain = 1;
}

extern "C" void isdf_view_candidates_sizes(int sizes_out[2]) {
    if (!sizes_out) return;
    sizes_out[0] = (int)sizeof(isdf_view_candidates_params); sizes_out[1] = (int)sizeof(isdf_view_candidates_info);
}

namespace {

// what the device and the host forms check and set up alike (c may be null: the host form)
int cand_setup(isdf_ctx *c, const isdf_depth_camera *cam, const double *targets, long long n_targets, const double *offsets, long long n_offsets,
               const isdf_view_candidates_params &P, const MapGeom &M, isdf_view_gain_params &Pg, DcRays &base) {
    ISDF_TRY(gain_setup(c, cam, nullptr, 0, &P.gain, nullptr, M, Pg, base));
    if (P.clearance_voxels < 0 || P.clearance_voxels > VC_MAX_CLEARANCE || P.k_best < 1 || P.k_best > VC_MAX_BEST || P.min_gain < 0)
        return isdf_fail(c, ISDF_ERR_INVALID_ARG, "bad view candidates parameters (clearance_voxels in [0, 8], k_best in [1, 64], min_gain >= 0)");
    if (n_targets < 0 || n_offsets < 0) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "view candidates: a negative count");
    if (n_offsets > VC_MAX_OFFSETS) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "view candidates: more than 2^20 offsets");
    if (n_offsets > 0 && n_targets > VC_MAX_CAND / n_offsets) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "view candidates: more than 2^31 - 1 candidates");
    if ((n_targets > 0 && !targets) || (n_offsets > 0 && !offsets)) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "view candidates: a null array with a positive count");
    return ISDF_OK;
}

void cand_info(long long n_targets, long long n_offsets, const VcCounts &N, int chunks, double filter_ms, double gain_ms, double select_ms, isdf_view_candidates_info *out) {
    isdf_view_candidates_info info{};
    info.n_targets = n_targets; info.n_offsets = n_offsets; info.n_candidates = n_targets * n_offsets;
    info.n_kept = N.n[VC_KEPT]; info.n_bad = N.n[VC_BAD]; info.n_occupied = N.n[VC_OCCUPIED]; info.n_unknown = N.n[VC_UNKNOWN]; info.n_close = N.n[VC_CLOSE];
    info.n_blocked = N.n[VC_BLOCKED];
    info.n_scored = N.n[VC_KEPT];           // a kept eye is finite and inside the map: the gain scores every kept candidate
    info.best_target = N.best_target; info.best_candidate = N.best_candidate; info.best_gain = N.best_gain;
    info.chunks = chunks; info.filter_ms = filter_ms; info.gain_ms = gain_ms; info.select_ms = select_ms;
    *out = info;
}

}  // namespace

extern "C" int isdf_view_candidates(isdf_ctx *c, const isdf_depth_camera *cam, const double *targets, long long n_targets, const double *offsets, long long n_offsets,
                                    const isdf_view_candidates_params *params, int64_t *cand_out, double *poses_out, int64_t *target_out, int64_t *best_out,
                                    isdf_view_candidates_info *info_out) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    const isdf_view_candidates_params P = map_query::resolve(params, isdf_view_candidates_params_default);
    const MapGeom M = map_geom(c->grid);            // (without a map: zeros, and the state check below refuses)
    isdf_view_gain_params Pg;
    DcRays base;
    ISDF_TRY(cand_setup(c, cam, targets, n_targets, offsets, n_offsets, P, M, Pg, base));
    ISDF_TRY(map_query::single_device(c, "candidate views are not offered on a multi-device ctx"));
    ISDF_TRY(map_query::has_occupancy(c, "candidate views"));
    ISDF_TRY(map_query::has_known(c, "candidate views need a known grid (isdf_map_known_enable)"));
    const long long n_cand = n_targets * n_offsets;
    VcCounts N;
    if (n_cand == 0) {
        if (info_out) cand_info(n_targets, n_offsets, N, 0, 0.0, 0.0, 0.0, info_out);
        return ISDF_OK;
    }
    ViewCandState *S;
    ViewGainState *G;
    ISDF_TRY(map_query::state_of(c, c->vcd, &S));
    ISDF_TRY(map_query::state_of(c, c->vgn, &G));
    const hipStream_t st = c->stream;
    const size_t nc = (size_t)n_cand, nt = (size_t)n_targets, nb = nt * (size_t)P.k_best;
    ISDF_TRY(S->d_targets.reserve(c, 3 * nt)); ISDF_TRY(S->d_offsets.reserve(c, 3 * (size_t)n_offsets));
    ISDF_TRY(S->d_cand.reserve(c, nc * VC_ROW)); ISDF_TRY(S->d_poses.reserve(c, nc * 12)); ISDF_TRY(S->d_dense.reserve(c, nc * 12));
    ISDF_TRY(S->d_flag.reserve(c, nc)); ISDF_TRY(S->d_pos.reserve(c, nc)); ISDF_TRY(S->d_index.reserve(c, nc));
    ISDF_TRY(S->d_target_rows.reserve(c, nt * VC_TARGET_ROW)); ISDF_TRY(S->d_best.reserve(c, nb));
    size_t bytes;
    ISDF_TRY(exclusive_sum_reserve(c, S->d_scan_tmp, S->d_flag.get(), S->d_pos.get(), n_cand, st, &bytes));
    ISDF_TRY(S->h_target_rows.reserve(c, nt * VC_TARGET_ROW));
    if (cand_out) ISDF_TRY(S->h_cand.reserve(c, nc * VC_ROW));
    if (poses_out) ISDF_TRY(S->h_poses.reserve(c, nc * 12));
    if (best_out) ISDF_TRY(S->h_best.reserve(c, nb));
    HIPCHK(c, hipMemcpyAsync(S->d_targets, targets, 3 * nt * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(S->d_offsets, offsets, 3 * (size_t)n_offsets * sizeof(double), hipMemcpyHostToDevice, st));
    // the filter stage and the first hand-over: the record
    const long long n_words = (long long)c->known.n_words;
    ISDF_TRY(map_query::count_begin(c, true, S->ev_filter, S->rec, st));
    hipLaunchKernelGGL(vc_filter_kernel, dim3(blocks(n_cand, VC_BLOCK)), dim3(VC_BLOCK), 0, st, (const double *)S->d_targets.get(), (const double *)S->d_offsets.get(),
                       n_offsets, n_cand, M, (const uint8_t *)c->d_occ.get(), (const unsigned *)c->known.d_bits.get(), n_words, (int)P.clearance_voxels, S->d_cand.get(),
                       S->d_poses.get(), S->d_flag.get(), S->rec.dev());
    hipLaunchKernelGGL(vc_tally_kernel, dim3((unsigned)n_targets), dim3(VC_SEL_BLOCK), 0, st, n_offsets, (int)P.k_best, (const long long *)S->d_cand.get(),
                       S->d_target_rows.get(), S->d_best.get());
    HIPCHK(c, hipGetLastError());
    ISDF_TRY(exclusive_sum_run(c, S->d_scan_tmp, bytes, S->d_flag.get(), S->d_pos.get(), n_cand, st));
    hipLaunchKernelGGL(vc_compact_kernel, dim3(blocks(n_cand, VC_LANE_BLOCK)), dim3(VC_LANE_BLOCK), 0, st, n_cand, (const int *)S->d_flag.get(),
                       (const int *)S->d_pos.get(), (const double *)S->d_poses.get(), S->d_dense.get(), S->d_index.get());
    HIPCHK(c, hipGetLastError());
    ISDF_TRY(map_query::count_end(c, true, S->ev_filter, S->rec, st));
    HIPCHK(c, hipStreamSynchronize(st));
    const VcRecord R = S->rec.host();
    for (int s = 0; s < VC_STATUSES; s++) N.n[s] = (long long)R.n[s];
    const long long n_kept = N.n[VC_KEPT];
    // the gain over the kept candidates alone, then the selection
    int chunks = 0;
    if (n_kept > 0) {
        ISDF_TRY(S->d_gain_rows.reserve(c, (size_t)n_kept * VG_ROW));
        ISDF_TRY(map_query::count_begin(c, true, S->ev_gain, st));
        ISDF_TRY(gain_run(c, G, base, M, Pg, S->d_dense.get(), n_kept, S->d_gain_rows.get(), false, &chunks, st));
        ISDF_TRY(map_query::count_end(c, true, S->ev_gain, st));
        ISDF_TRY(map_query::count_begin(c, true, S->ev_select, st));
        hipLaunchKernelGGL(vc_score_kernel, dim3(blocks(n_kept, VC_LANE_BLOCK)), dim3(VC_LANE_BLOCK), 0, st, n_kept, (const int *)S->d_index.get(),
                           (const long long *)S->d_gain_rows.get(), S->d_cand.get());
        hipLaunchKernelGGL(vc_select_kernel, dim3((unsigned)n_targets), dim3(VC_SEL_BLOCK), 0, st, n_offsets, (int)P.k_best, (long long)P.min_gain, S->d_cand.get(),
                           S->d_target_rows.get(), S->d_best.get());
        HIPCHK(c, hipGetLastError());
        ISDF_TRY(map_query::count_end(c, true, S->ev_select, st));
    }
    // the second hand-over: the results, through the pinned copies
    HIPCHK(c, hipMemcpyAsync(S->h_target_rows.get(), S->d_target_rows, nt * VC_TARGET_ROW * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    if (cand_out) HIPCHK(c, hipMemcpyAsync(S->h_cand.get(), S->d_cand, nc * VC_ROW * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    if (poses_out) HIPCHK(c, hipMemcpyAsync(S->h_poses.get(), S->d_poses, nc * 12 * sizeof(double), hipMemcpyDeviceToHost, st));
    if (best_out) HIPCHK(c, hipMemcpyAsync(S->h_best.get(), S->d_best, nb * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (cand_out) std::memcpy(cand_out, S->h_cand.get(), nc * VC_ROW * sizeof(int64_t));
    if (poses_out) std::memcpy(poses_out, S->h_poses.get(), nc * 12 * sizeof(double));
    if (target_out) std::memcpy(target_out, S->h_target_rows.get(), nt * VC_TARGET_ROW * sizeof(int64_t));
    if (best_out) std::memcpy(best_out, S->h_best.get(), nb * sizeof(int64_t));
    if (info_out) {
        vc_best_of(S->h_target_rows.get(), n_targets, N);
        cand_info(n_targets, n_offsets, N, chunks, S->ev_filter.ms(0, 1), n_kept > 0 ? S->ev_gain.ms(0, 1) : 0.0, n_kept > 0 ? S->ev_select.ms(0, 1) : 0.0, info_out);
    }
    return ISDF_OK;
}

extern "C" int isdf_view_candidates_host(const uint32_t *bits, const uint8_t *occ, const double bmin[3], const double bmax[3], double resolution, const int32_t dims[3],
                                         const isdf_depth_camera *cam, const double *targets, long long n_targets, const double *offsets, long long n_offsets,
                                         const isdf_view_candidates_params *params, int64_t *cand_out, double *poses_out, int64_t *target_out, int64_t *best_out,
                                         isdf_view_candidates_info *info_out) {
    if (ms_geometry_bad(bmin, bmax, resolution, dims) || !bits || !occ) return isdf_fail(nullptr, ISDF_ERR_INVALID_ARG, "view candidates (host form): bad arguments");
    const MapGeom M = map_geom(bmin, bmax, resolution, dims);
    const isdf_view_candidates_params P = map_query::resolve(params, isdf_view_candidates_params_default);
    isdf_view_gain_params Pg;
    DcRays base;
    ISDF_TRY(cand_setup(nullptr, cam, targets, n_targets, offsets, n_offsets, P, M, Pg, base));
    const long long n_cand = n_targets * n_offsets;
    VcCounts N;
    if (n_cand > 0) {
        const size_t nc = (size_t)n_cand, nt = (size_t)n_targets, nb = nt * (size_t)P.k_best;
        std::vector<int64_t> cand(cand_out ? 0 : nc * VC_ROW), rows(target_out ? 0 : nt * VC_TARGET_ROW), best(best_out ? 0 : nb);
        std::vector<double> poses(poses_out ? 0 : nc * 12);
        vc_candidates_host(bits, occ, M, base, targets, n_targets, offsets, n_offsets, P.clearance_voxels, P.k_best, P.min_gain, cand_out ? cand_out : cand.data(),
                           poses_out ? poses_out : poses.data(), target_out ? target_out : rows.data(), best_out ? best_out : best.data(), N);
    }
    if (info_out) cand_info(n_targets, n_offsets, N, 0, 0.0, 0.0, 0.0, info_out);
    return ISDF_OK;
}
