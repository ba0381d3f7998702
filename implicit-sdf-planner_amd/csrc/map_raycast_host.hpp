// A ray cast through the map's occupancy (map_raycast.hip), free of HIP so that a plain C++ program can run it under a
// sanitizer: the read-only counterpart of the scan's trace.  The ray, its quantisation and its walk are map_scan_host.hpp's and are
// not stated again here; mr_cast_ray, marked MU_HD, is the per-ray function both the kernel and the host form call, so the two write
// the same rows byte for byte.
//
// A row is eight int32: {status, steps, i, j, k, axis, num, den}.  status 0: the walk reached the end point's voxel, 1: it stopped at
// the first tested voxel whose occupancy byte is not 0, 2: the end point is outside the map or not finite, 3: the origin is.  steps is
// the 0-based index in the walk of the voxel (i, j, k) where the walk ended; axis is the axis of the last step taken, num / den the
// fraction of the segment between the two tick centres at which that step crossed into the voxel (the axis's m before the step, its
// D).  A walk that ended at voxel 0: axis -1, num 0, den 1.  Status 2 and 3: {status, -1, -1, -1, -1, -1, 0, 1}.
#pragma once
#include "map_scan_host.hpp"

namespace isdf {

constexpr int MR_ROW = 8;               // int32 per ray
constexpr int MR_CLEAR = 0, MR_HIT = 1, MR_END_OUTSIDE = 2, MR_ORIGIN_OUTSIDE = 3;

MU_HD void mr_row_none(int status, int row[MR_ROW]) {
    row[0] = status;
    row[1] = row[2] = row[3] = row[4] = row[5] = -1;
    row[6] = 0; row[7] = 1;
}

// The walk from tick qo to tick qe over the occupancy bytes (z fastest, M.dims as the grid's).  Voxel 0 of the walk is tested only when
// test_origin is set.  No bounds test: the walk stays in the box of its two end voxels, both of which lie in the grid.
MU_HD void mr_cast_walk(const uint8_t *occ, const MapGeom &M, const int qo[3], const int qe[3], bool test_origin, int row[MR_ROW]) {
    MsRay r;
    ms_ray_begin(qo, qe, r);
    int status = MR_CLEAR, steps = 0, axis = -1;
    bool test = test_origin;
    for (;;) {
        if (test && occ[map_voxel(M, r.v)] != 0) { status = MR_HIT; break; }
        if (ms_ray_done(r)) break;
        axis = ms_ray_step_axis(r);
        steps++;
        test = true;
    }
    row[0] = status; row[1] = steps;
    row[2] = r.v[0]; row[3] = r.v[1]; row[4] = r.v[2];
    row[5] = axis;
    // the last step's axis has not moved since: its m is the crossing's plus the step's 2048 (selects, not an indexed read)
    const unsigned m = axis == 0 ? r.m[0] : (axis == 1 ? r.m[1] : r.m[2]);
    const unsigned D = axis == 0 ? r.D[0] : (axis == 1 ? r.D[1] : r.D[2]);
    row[6] = axis < 0 ? 0 : (int)(m - 2048u);
    row[7] = axis < 0 ? 1 : (int)D;
}

// one ray: origin_ok / qo from ms_quantize of the origin (the caller's, so that a shared origin is quantised once)
MU_HD void mr_cast_ray(const uint8_t *occ, const MapGeom &M, bool origin_ok, const int qo[3], const float end[3], bool test_origin, int row[MR_ROW]) {
    int qe[3];
    if (!origin_ok) { mr_row_none(MR_ORIGIN_OUTSIDE, row); return; }
    if (!ms_quantize(M, (double)end[0], (double)end[1], (double)end[2], qe)) { mr_row_none(MR_END_OUTSIDE, row); return; }
    mr_cast_walk(occ, M, qo, qe, test_origin, row);
}

struct MrCounts { long long n_skipped = 0, n_origin_outside = 0, n_hits = 0, n_clear = 0, steps_total = 0; };

MU_HD void mr_count_row(const int row[MR_ROW], long long &n_skipped, long long &n_origin_outside, long long &n_hits, long long &n_clear, long long &steps_total) {
    n_skipped += row[0] == MR_END_OUTSIDE;
    n_origin_outside += row[0] == MR_ORIGIN_OUTSIDE;
    n_hits += row[0] == MR_HIT;
    n_clear += row[0] == MR_CLEAR;
    if (row[0] == MR_CLEAR || row[0] == MR_HIT) steps_total += row[1];
}

// ---- host form: rows_out = n x 8.  origins: 3 doubles for every ray, or n x 3 (per_ray).  false: a shared origin lies outside the
// map (nothing written).
inline bool mr_cast_host(const uint8_t *occ, const MapGeom &M, const double *origins, bool per_ray, const float *ends, long long n, bool test_origin, int32_t *rows_out,
                         MrCounts &K) {
    K = MrCounts();
    int qo[3] = {0, 0, 0};
    bool ok = true;
    if (!per_ray && !ms_quantize(M, origins[0], origins[1], origins[2], qo)) return false;
    for (long long i = 0; i < n; i++) {
        if (per_ray) ok = ms_quantize(M, origins[3 * i], origins[3 * i + 1], origins[3 * i + 2], qo);
        int row[MR_ROW];
        mr_cast_ray(occ, M, ok, qo, ends + 3 * i, test_origin, row);
        mr_count_row(row, K.n_skipped, K.n_origin_outside, K.n_hits, K.n_clear, K.steps_total);
        for (int w = 0; w < MR_ROW; w++) rows_out[MR_ROW * i + w] = row[w];
    }
    return true;
}

}  // namespace isdf
