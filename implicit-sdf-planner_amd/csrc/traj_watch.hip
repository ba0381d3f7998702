// The kept clearance report folded across map updates (isdf_traj_check_set_watch).  Occupancy only grows, the field
// query answers every point on its own, and every quantity of the report is a sum, a minimum or a voxel-ordered list: the check on
// the updated map is the kept report merged with a report over only the voxels the update made occupied (MapUpdateState::d_list).
//
//   select   one lane per entry of the update's list: its voxel index as the sort key; in the arming check's voxel box -> counted for
//            occupied_in_box; in the box and some coarse sample within far_r (sample_within over ALL samples staged in LDS - the full
//            check's brick ranges are only a contiguous superset of them; a radius-less shape: every entry of the box) -> counted as
//            a candidate.  Counts only: no atomic decides a position.
//   order    hipCUB's radix sort of the keys: the list's order, which the update's atomics leave undefined, never shows.
//   field    EVERY new voxel, in voxel order, through the field query in the kept mode - sized by n_new, which the host has, so no
//            hand-over stands between select and field.  A voxel that is not a candidate lies farther than far_r from every coarse
//            sample and reads 10 / -1 (the selection's own premise, traj_check.hip): it qualifies for nothing, and the sums, minima
//            and rows are those of the candidates alone.
//   reduce   the full check's own kernels (tc_reduce_launch / tc_rows_launch): the update's own report, the new_* fields.
//   merge    rows on the device: both voxel-id lists are ascending and disjoint (a new voxel was not occupied before), so a row's
//            place is its own index plus tw_rank of its id in the other list - one lane per row, one binary search.  The info words
//            and the piece minima on the host from the hand-over record (tw_fold_info, the function isdf_traj_check_fold_host calls).
// One pinned record and one synchronisation per fold, the field query's overflow word inside the record.
#include "swept_field.hpp"
#include "dev_scan.hpp"
#include "map_update_host.hpp"
#include <algorithm>
#include <cmath>
#include <cstring>

namespace {

// the hand-over record, in 64-bit words: [0] new voxels in the box [1] candidates [2..4] qualified, below the margin, penetrating
// [5..11] the report's TC_REPORT_WORDS doubles [12] the field query's overflow word [13..13 + N) the piece minima of the new voxels
constexpr int REC_SEL = 0, REC_COUNTS = 2, REC_REPORT = 5, REC_OVERFLOW = 12, REC_PIECE = 13;

__global__ __launch_bounds__(256) void tw_select_kernel(SelBox B, const MuVoxel *__restrict__ list, unsigned n, const double *__restrict__ pose,
                                                        const int *__restrict__ n_coarse, long long *__restrict__ key, unsigned long long *stats) {
    __shared__ double s_pos[3 * SWEPT_MAX_COARSE];
    const int nc = min(*n_coarse, SWEPT_MAX_COARSE);
    if (B.cull) stage_samples(pose, nc, s_pos);
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    bool in = false, sel = false;
    if (i < n) {
        const MuVoxel v = list[i];
        const int x = v.x, y = v.y, z = v.z;
        key[i] = ((long long)x * B.Y + y) * B.Z + z;
        in = x >= B.lo[0] && x <= B.hi[0] && y >= B.lo[1] && y <= B.hi[1] && z >= B.lo[2] && z <= B.hi[2];
        sel = in;
        if (in && B.cull) {
            const double px = voxel_centre(x, B.res, B.bmin[0]), py = voxel_centre(y, B.res, B.bmin[1]), pz = voxel_centre(z, B.res, B.bmin[2]);
            sel = false;
            for (int k = 0; k < nc && !sel; k++) sel = sample_within(px, py, pz, s_pos, k, B.far2);
        }
    }
    const unsigned long long m_in = __ballot(in), m_sel = __ballot(sel);
    if ((threadIdx.x & 63) == 0) {
        if (m_in) atomicAdd(&stats[0], (unsigned long long)__popcll(m_in));
        if (m_sel) atomicAdd(&stats[1], (unsigned long long)__popcll(m_sel));
    }
}

// the sorted voxel indices -> their centres, as tc_emit_kernel forms them
__global__ __launch_bounds__(256) void tw_xyz_kernel(SelBox B, const long long *__restrict__ vox, unsigned n, double *__restrict__ xyz) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long id = vox[i];
    const int z = (int)(id % B.Z), y = (int)((id / B.Z) % B.Y), x = (int)(id / ((long long)B.Z * B.Y));
    xyz[3 * (size_t)i] = voxel_centre(x, B.res, B.bmin[0]); xyz[3 * (size_t)i + 1] = voxel_centre(y, B.res, B.bmin[1]);
    xyz[3 * (size_t)i + 2] = voxel_centre(z, B.res, B.bmin[2]);
}

// rows a (the kept report's, na of them) and rows b (the update's: counts[1] of them, at most nb_cap) into their places
__global__ __launch_bounds__(256) void tw_merge_rows_kernel(const double *__restrict__ rows_a, const long long *__restrict__ vox_a, long long na,
                                                            const double *__restrict__ rows_b, const long long *__restrict__ vox_b,
                                                            const unsigned long long *__restrict__ counts, long long nb_cap,
                                                            double *__restrict__ rows_out, long long *__restrict__ vox_out) {
    const long long nb = min((long long)counts[1], nb_cap);
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const double *src;
    long long id, pos;
    if (t < na) { id = vox_a[t]; pos = t + isdf::tw_rank(vox_b, nb, id); src = rows_a + 5 * (size_t)t; }
    else if (t - na < nb) { const long long j = t - na; id = vox_b[j]; pos = j + isdf::tw_rank(vox_a, na, id); src = rows_b + 5 * (size_t)j; }
    else return;
    double *o = rows_out + 5 * (size_t)pos;
    for (int q = 0; q < 5; q++) o[q] = src[q];
    vox_out[pos] = id;
}

void last_none(isdf_traj_watch_info &L) {
    L.new_min_clearance = 1e1; L.new_min_tstar = -1.0; L.new_min_voxel = -1; L.new_min_piece = -1;
}

// path 1: the new voxels are the n entries of d_list
int fold_list(isdf_ctx *c, TrajCheckState *k, const MuVoxel *d_list, unsigned n) {
    TrajWatchState &w = k->w;
    const hipStream_t st = c->stream;
    const int N = w.N;
    const double *d_T = w.d_traj, *d_C = w.d_traj + N;
    int rc;
    SweptMeshState *s;
    if ((rc = swept_field_scratch(c, &s))) return rc;
    if ((rc = w.ev.ready(c))) return rc;
    const long long na = k->n_rows;
    if ((rc = w.rec.ready(c, (size_t)REC_PIECE + N))) return rc;
    if ((rc = w.d_key.reserve(c, n)) || (rc = w.d_vox.reserve(c, n)) || (rc = w.d_xyz.reserve(c, 3 * (size_t)n))) return rc;
    if ((rc = w.d_val.reserve(c, n)) || (rc = w.d_ts.reserve(c, n))) return rc;
    if ((rc = w.d_new_rows.reserve(c, 5 * (size_t)n)) || (rc = w.d_new_row_vox.reserve(c, n))) return rc;
    if ((rc = w.d_rows_out.reserve(c, 5 * (size_t)(na + n))) || (rc = w.d_row_vox_out.reserve(c, (size_t)(na + n)))) return rc;
    SelBox B = w.box;
    if (w.box_empty) for (int a = 0; a < 3; a++) { B.lo[a] = 1; B.hi[a] = 0; }       // nothing lies in an empty box
    int end_bit = 1;
    while (end_bit < 62 && (1ll << end_bit) < (long long)B.X * B.Y * B.Z) end_bit++;
    size_t sort_bytes = 0;
    HIPCHK(c, hipcub::DeviceRadixSort::SortKeys(nullptr, sort_bytes, (const long long *)w.d_key.get(), w.d_vox.get(), (int)n, 0, end_bit, st));
    if ((rc = w.d_sort_tmp.reserve(c, std::max<size_t>(sort_bytes, 1)))) return rc;

    // ---- select, order
    HIPCHK(c, hipEventRecord(w.ev[0], st));
    HIPCHK(c, w.rec.zero(st));
    if ((rc = swept_field_coarse_table(c, N, d_T, d_C, w.mode, st))) return rc;        // the arming check's doubles again
    hipLaunchKernelGGL(tw_select_kernel, dim3(blocks(n)), dim3(256), 0, st, B, d_list, n, (const double *)s->field.coarse_pose, (const int *)s->field.n_coarse,
                       w.d_key.get(), w.rec.dev() + REC_SEL);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipcub::DeviceRadixSort::SortKeys(w.d_sort_tmp.get(), sort_bytes, (const long long *)w.d_key.get(), w.d_vox.get(), (int)n, 0, end_bit, st));
    hipLaunchKernelGGL(tw_xyz_kernel, dim3(blocks(n)), dim3(256), 0, st, B, (const long long *)w.d_vox.get(), n, w.d_xyz.get());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(w.ev[1], st));

    // ---- field
    if ((rc = swept_field_launch(c, N, d_T, d_C, w.d_xyz, n, w.mode, w.d_val, w.d_ts, st))) return rc;
    HIPCHK(c, hipMemcpyAsync(w.rec.dev() + REC_OVERFLOW, s->d_stats.get() + 4, sizeof(unsigned long long), hipMemcpyDeviceToDevice, st));
    HIPCHK(c, hipEventRecord(w.ev[2], st));

    // ---- reduce: the update's own report
    if ((rc = tc_reduce_launch(c, w.red, n, w.d_val, w.d_ts, w.d_vox, w.d_xyz, d_T, N, w.margin, w.rec.dev() + REC_COUNTS, (double *)(w.rec.dev() + REC_REPORT),
                               (double *)(w.rec.dev() + REC_PIECE), st))) return rc;
    if ((rc = tc_rows_launch(c, w.red, n, w.d_val, w.d_ts, w.d_vox, w.d_xyz, w.d_new_rows, w.d_new_row_vox, st))) return rc;
    HIPCHK(c, hipEventRecord(w.ev[3], st));

    // ---- merge the rows; the one hand-over
    hipLaunchKernelGGL(tw_merge_rows_kernel, dim3(blocks(na + n)), dim3(256), 0, st, (const double *)k->d_rows.get(), (const long long *)k->d_row_vox.get(), na,
                       (const double *)w.d_new_rows.get(), (const long long *)w.d_new_row_vox.get(), (const unsigned long long *)(w.rec.dev() + REC_COUNTS),
                       (long long)n, w.d_rows_out.get(), w.d_row_vox_out.get());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(w.ev[4], st));
    HIPCHK(c, w.rec.fetch(st));
    HIPCHK(c, hipStreamSynchronize(st));
    const unsigned long long *R = &w.rec.host();
    if (R[REC_OVERFLOW]) return isdf_fail(c, ISDF_ERR_OVERFLOW, "clearance watch: a new voxel has more than 32 in-range intervals (the kept report is dropped)");
    if (R[REC_COUNTS + 1] > (unsigned long long)n) return isdf_fail(c, ISDF_ERR_HIP, "clearance watch: inconsistent hand-over record");

    // ---- the update's report as an isdf_traj_check_info, folded into the kept one
    isdf_traj_check_info b = w.info;            // culled, margin, far_r as armed
    double rep[TC_REPORT_WORDS];
    std::memcpy(rep, R + REC_REPORT, sizeof(rep));
    b.occupied_in_box = (long long)R[REC_SEL]; b.candidates = (long long)R[REC_SEL + 1];
    b.qualified = (long long)R[REC_COUNTS]; b.n_below_margin = (long long)R[REC_COUNTS + 1]; b.n_penetrating = (long long)R[REC_COUNTS + 2];
    b.min_clearance = rep[0]; b.min_tstar = rep[1];
    for (int a = 0; a < 3; a++) b.min_point[a] = rep[2 + a];
    long long word;
    std::memcpy(&word, &rep[5], sizeof(word)); b.min_voxel = word;
    std::memcpy(&word, &rep[6], sizeof(word)); b.min_piece = (int32_t)word;
    int min_changed = 0;
    isdf::tw_fold_info(N, &w.info, w.piece_min.data(), &b, (const double *)(R + REC_PIECE), &w.info, w.piece_min.data(), &min_changed);
    k->d_rows.swap(w.d_rows_out); k->d_row_vox.swap(w.d_row_vox_out);
    k->n_rows = na + b.n_below_margin;
    isdf_traj_watch_info &L = w.last;
    const long long folded = L.updates_folded;
    L = isdf_traj_watch_info{};
    L.updates_folded = folded + 1;
    L.path = 1;
    L.new_voxels = n; L.new_in_box = b.occupied_in_box; L.new_candidates = b.candidates; L.new_qualified = b.qualified;
    L.new_below_margin = b.n_below_margin; L.new_penetrating = b.n_penetrating;
    L.new_min_clearance = b.min_clearance; L.new_min_tstar = b.min_tstar; L.new_min_voxel = b.min_voxel; L.new_min_piece = b.min_piece;
    L.min_changed = min_changed;
    L.select_ms = w.ev.ms(0, 1); L.field_ms = w.ev.ms(1, 2); L.reduce_ms = w.ev.ms(2, 3);
    L.merge_ms = w.ev.ms(3, 4);
    return ISDF_OK;
}

// path 2: the update's list was cut, so the kept trajectory is checked against the whole map again
int fold_full(isdf_ctx *c, TrajCheckState *k, unsigned n_new) {
    const isdf_traj_check_info old = k->w.info;
    const long long folded = k->w.last.updates_folded;
    isdf_traj_check_info now;
    ISDF_TRY(traj_check_rerun_kept(c, &now));
    isdf_traj_watch_info &L = k->w.last;            // (the re-check armed the watch again and cleared this)
    L.updates_folded = folded + 1;
    L.path = 2;
    L.new_voxels = n_new;
    L.new_in_box = now.occupied_in_box - old.occupied_in_box; L.new_candidates = now.candidates - old.candidates;
    L.new_qualified = now.qualified - old.qualified; L.new_below_margin = now.n_below_margin - old.n_below_margin;
    L.new_penetrating = now.n_penetrating - old.n_penetrating;
    L.min_changed = now.min_voxel != old.min_voxel ? 1 : 0;
    last_none(L);
    if (L.min_changed) { L.new_min_clearance = now.min_clearance; L.new_min_tstar = now.min_tstar; L.new_min_voxel = now.min_voxel; L.new_min_piece = now.min_piece; }
    L.select_ms = now.select_ms; L.field_ms = now.field_ms; L.reduce_ms = now.reduce_ms; L.merge_ms = 0.0;
    return ISDF_OK;
}

}  // namespace

void traj_watch_disarm(isdf_ctx *c) { if (c->tck) c->tck->w.armed = false; }

bool traj_watch_armed(isdf_ctx *c) {
    if (c->traj_watch_mode != 1 || !c->tck || !c->tck->w.armed) return false;
    if (!c->tck->have || c->tck->grid_epoch != c->grid_epoch || !c->have_geom) { c->tck->w.armed = false; return false; }     // a new grid: the voxel ids are stale
    return true;
}

int traj_watch_fold(isdf_ctx *c, const void *d_list, unsigned n_new, unsigned cap) {
    TrajCheckState *k = c->tck.get();
    if (n_new == 0) return ISDF_OK;
    const int rc = n_new <= cap ? fold_list(c, k, (const MuVoxel *)d_list, n_new) : fold_full(c, k, n_new);
    if (rc != ISDF_OK) {                // never half-merged: the report goes, the message stays
        const std::string err = c->err;
        (void)hipStreamSynchronize(c->stream);          // (launches of the failed fold may still read the buffers)
        traj_check_drop_report(c);
        c->err = err;
    }
    return rc;
}

extern "C" int isdf_traj_check_set_watch(isdf_ctx *c, int mode) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    if (mode != 0 && mode != 1) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "clearance watch: mode must be 0 or 1");
    if (!c->peers.empty() || c->is_peer) return isdf_fail(c, ISDF_ERR_UNSUPPORTED, "the clearance watch is not offered on a multi-device ctx");
    c->traj_watch_mode = mode;
    if (mode == 0) traj_watch_disarm(c);
    return ISDF_OK;
}

extern "C" int isdf_traj_check_watch_info(isdf_ctx *c, isdf_traj_check_info *report_out, double *piece_min_out, isdf_traj_watch_info *last_out) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    if (!report_out) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "null output");
    if (!traj_watch_armed(c)) return isdf_fail(c, ISDF_ERR_STATE, "no clearance watch armed (isdf_traj_check_set_watch(ctx, 1), then isdf_traj_check)");
    const TrajWatchState &w = c->tck->w;
    *report_out = w.info;
    if (piece_min_out) std::memcpy(piece_min_out, w.piece_min.data(), (size_t)w.N * sizeof(double));
    if (last_out) *last_out = w.last;
    return ISDF_OK;
}

extern "C" void isdf_traj_check_watch_sizes(int sizes_out[1]) {
    if (sizes_out) sizes_out[0] = (int)sizeof(isdf_traj_watch_info);
}

extern "C" int isdf_traj_check_fold_host(int N, const isdf_traj_check_info *a, const double *piece_min_a, const double *rows_a, const int64_t *vox_a,
                                         const isdf_traj_check_info *b, const double *piece_min_b, const double *rows_b, const int64_t *vox_b,
                                         isdf_traj_check_info *out, double *piece_min_out, double *rows_out, int64_t *vox_out, long long capacity) {
    if (N < 1 || !a || !b || !out) return isdf_fail(nullptr, ISDF_ERR_INVALID_ARG, "clearance fold: null report");
    const long long na = a->n_below_margin, nb = b->n_below_margin;
    if (na < 0 || nb < 0 || (na > 0 && (!rows_a || !vox_a)) || (nb > 0 && (!rows_b || !vox_b)))
        return isdf_fail(nullptr, ISDF_ERR_INVALID_ARG, "clearance fold: rows missing");
    if (capacity < na + nb) return isdf_fail(nullptr, ISDF_ERR_OVERFLOW, "clearance fold: output capacity smaller than the rows of both reports");
    if (na + nb > 0 && (!rows_out || !vox_out)) return isdf_fail(nullptr, ISDF_ERR_INVALID_ARG, "clearance fold: null output");
    static_assert(sizeof(long long) == sizeof(int64_t), "voxel ids are 64-bit");
    if (!isdf::tw_fold_rows(rows_a, (const long long *)vox_a, na, rows_b, (const long long *)vox_b, nb, rows_out, (long long *)vox_out))
        return isdf_fail(nullptr, ISDF_ERR_INVALID_ARG, "clearance fold: voxel ids must ascend and the two lists must be disjoint");
    isdf::tw_fold_info(N, a, piece_min_a, b, piece_min_b, out, piece_min_out, nullptr);
    return ISDF_OK;
}
