// Candidate views (view_cand.hip), free of HIP so that a plain C++ program can run it under a sanitizer: eye positions round
// each target, tested for being a safe, seen place from which the target is visible, posed, scored by the view gain and ranked.
// Nothing of the quantisation, the walk, the stop rule or the gain is stated here: ms_quantize is the scan's, the line of sight
// map_raycast_host.hpp's mr_cast_walk, K's bits are read through map_known_host.hpp's mk_bits_at / mk_run, the gain is
// view_gain_host.hpp's.  vc_candidate, marked MU_HD, is the per-candidate function both the filter kernel and the host form call.
//
// Candidate c = i * n_offsets + k has eye = target_i + offset_k (one fp64 addition per component).  Its status is the first test that
// fails:
//   1 bad       a component of the target or of the eye is not finite; ms_quantize refuses the target or the eye; with d = target - eye,
//               n2 = d_x^2 + d_y^2 + d_z^2 (left to right) is 0 or not finite
//   2 occupied  the occupancy byte of the eye's voxel is not 0
//   3 unknown   K is 0 at the eye's voxel
//   4 close     some voxel of the cube of Chebyshev radius clearance_voxels round the eye's voxel, clipped to the grid, is occupied or unknown
//   5 blocked   mr_cast_walk from the eye's ticks to the target's ticks with test_origin = false ends with MR_HIT at a voxel that is not the
//               target's own
//   0 kept      and posed: n = sqrt(n2), z = d / n, x0 = (z_y, -z_x, 0), h = sqrt(x0_x^2 + x0_y^2); if h <= 1e-9: x0 = (0, z_z, -z_y),
//               h = sqrt(x0_y^2 + x0_z^2); x = x0 / h; y = z cross x; the pose's rows are (x_a, y_a, z_a, eye_a).  fp64, nothing contracted.
// A candidate's row is eight int64: {status, eye_voxel, los_steps, gain, n_hits, steps_total, n_rays_unknown, rank}.
#pragma once
#include "view_gain_host.hpp"
#include <algorithm>
#include <vector>

namespace isdf {

constexpr int VC_ROW = 8;               // int64 per candidate
constexpr int VC_TARGET_ROW = 8;        // int64 per target: n_kept, n_bad, n_occupied, n_unknown, n_close, n_blocked, best_candidate, best_gain
constexpr int VC_KEPT = 0, VC_BAD = 1, VC_OCCUPIED = 2, VC_UNKNOWN = 3, VC_CLOSE = 4, VC_BLOCKED = 5;
constexpr int VC_STATUSES = 6;
constexpr int VC_MAX_CLEARANCE = 8, VC_MAX_BEST = 64;
constexpr long long VC_MAX_OFFSETS = 1ll << 20, VC_MAX_CAND = 0x7FFFFFFFll;

// The selection's integer key of a qualified candidate: larger is better - the larger gain, then the lower k.  k < 2^20 and a gain is
// at most the voxel count, below 2^36, so the key is below 2^57 and 0 is "none".
static_assert(VC_MAX_OFFSETS == 1ll << 20, "the key keeps k in 20 bits");
MU_HD unsigned long long vc_key(long long gain, long long k) { return ((unsigned long long)(gain + 1) << 20) | (unsigned long long)(VC_MAX_OFFSETS - 1 - k); }
MU_HD long long vc_key_k(unsigned long long key) { return VC_MAX_OFFSETS - 1 - (long long)(key & (unsigned long long)(VC_MAX_OFFSETS - 1)); }
MU_HD long long vc_key_gain(unsigned long long key) { return (long long)(key >> 20) - 1; }

MU_HD bool vc_finite(double v) { return v - v == 0.0; }

struct VcCand {
    int status;
    long long eye_voxel;        // -1: status 1
    int los_steps;              // -1: test 5 was not reached
    double pose[12];            // zeros unless kept
};

// every voxel of the cube of Chebyshev radius r round voxel v, clipped to the grid, is free and known: a column's z run is one run of
// occupancy bytes and one run of at most 17 bits of K's stream
MU_HD bool vc_cube_clear(const uint32_t *bits, long long n_words, const uint8_t *occ, const MapGeom &M, const int v[3], int r) {
    int lo[3], hi[3];
    for (int a = 0; a < 3; a++) {
        lo[a] = v[a] - r < 0 ? 0 : v[a] - r;
        hi[a] = v[a] + r > M.dims[a] - 1 ? M.dims[a] - 1 : v[a] + r;
    }
    const int len = hi[2] - lo[2] + 1;
    const uint32_t run = mk_run(0, len - 1);
    for (int x = lo[0]; x <= hi[0]; x++)
        for (int y = lo[1]; y <= hi[1]; y++) {
            const int p[3] = {x, y, lo[2]};
            const size_t a0 = map_voxel(M, p);
            if ((mk_bits_at(bits, n_words, (long long)a0) & run) != run) return false;
            for (int z = 0; z < len; z++)
                if (occ[a0 + (size_t)z] != 0) return false;
        }
    return true;
}

// tests 1 - 5 and the pose of one candidate
MU_HD void vc_candidate(const uint32_t *bits, long long n_words, const uint8_t *occ, const MapGeom &M, const double target[3], const double offset[3], int clearance,
                        VcCand &C) {
    C.status = VC_BAD; C.eye_voxel = -1; C.los_steps = -1;
    for (int i = 0; i < 12; i++) C.pose[i] = 0.0;
    const double ex = target[0] + offset[0], ey = target[1] + offset[1], ez = target[2] + offset[2];
    if (!(vc_finite(target[0]) && vc_finite(target[1]) && vc_finite(target[2]) && vc_finite(ex) && vc_finite(ey) && vc_finite(ez))) return;
    int qt[3], qe[3];
    if (!ms_quantize(M, target[0], target[1], target[2], qt) || !ms_quantize(M, ex, ey, ez, qe)) return;
    const double dx = target[0] - ex, dy = target[1] - ey, dz = target[2] - ez;
    const double n2 = dx * dx + dy * dy + dz * dz;
    if (n2 == 0.0 || !vc_finite(n2)) return;
    const int ve[3] = {qe[0] >> MS_TICKS_LOG2, qe[1] >> MS_TICKS_LOG2, qe[2] >> MS_TICKS_LOG2};
    const size_t a = map_voxel(M, ve);
    C.eye_voxel = (long long)a;
    if (occ[a] != 0) { C.status = VC_OCCUPIED; return; }
    if (!(mk_bits_at(bits, n_words, (long long)a) & 1u)) { C.status = VC_UNKNOWN; return; }
    if (clearance > 0 && !vc_cube_clear(bits, n_words, occ, M, ve, clearance)) { C.status = VC_CLOSE; return; }
    int row[MR_ROW];
    mr_cast_walk(occ, M, qe, qt, false, row);
    C.los_steps = row[1];
    if (row[0] == MR_HIT && !(row[2] == qt[0] >> MS_TICKS_LOG2 && row[3] == qt[1] >> MS_TICKS_LOG2 && row[4] == qt[2] >> MS_TICKS_LOG2)) { C.status = VC_BLOCKED; return; }
    C.status = VC_KEPT;
    const double n = sqrt(n2);
    const double zx = dx / n, zy = dy / n, zz = dz / n;
    double x0x = zy, x0y = -zx, x0z = 0.0;
    double h = sqrt(x0x * x0x + x0y * x0y);
    if (h <= 1e-9) {
        x0x = 0.0; x0y = zz; x0z = -zy;
        h = sqrt(x0y * x0y + x0z * x0z);
    }
    const double xx = x0x / h, xy = x0y / h, xz = x0z / h;
    const double yx = zy * xz - zz * xy, yy = zz * xx - zx * xz, yz = zx * xy - zy * xx;
    C.pose[0] = xx; C.pose[1] = yx; C.pose[2] = zx; C.pose[3] = ex;
    C.pose[4] = xy; C.pose[5] = yy; C.pose[6] = zy; C.pose[7] = ey;
    C.pose[8] = xz; C.pose[9] = yz; C.pose[10] = zz; C.pose[11] = ez;
}

// the first six words of a candidate's row; the gain's words and the rank are filled once it is scored and ranked
MU_HD void vc_row_open(const VcCand &C, long long row[VC_ROW]) {
    row[0] = C.status; row[1] = C.eye_voxel; row[2] = C.los_steps;
    row[3] = row[4] = row[5] = row[6] = 0;
    row[7] = -1;
}

struct VcCounts { long long n[VC_STATUSES] = {0, 0, 0, 0, 0, 0}; long long best_target = -1, best_candidate = -1, best_gain = 0; };

// what the info says of the target rows: the largest best_gain, ties to the lowest candidate index (the targets ascend with it)
inline void vc_best_of(const int64_t *target_rows, long long n_targets, VcCounts &N) {
    N.best_target = N.best_candidate = -1; N.best_gain = 0;
    for (long long i = 0; i < n_targets; i++) {
        const int64_t *const t = target_rows + VC_TARGET_ROW * i;
        if (t[6] < 0) continue;
        if (N.best_candidate < 0 || t[7] > N.best_gain) { N.best_target = i; N.best_candidate = t[6]; N.best_gain = t[7]; }
    }
}

// ---- host form: cand n_cand x 8, poses n_cand x 12, target_rows n_targets x 8, best n_targets x k_best; all are written
inline void vc_candidates_host(const uint32_t *bits, const uint8_t *occ, const MapGeom &M, const DcRays &base, const double *targets, long long n_targets,
                               const double *offsets, long long n_offsets, int clearance, int k_best, long long min_gain, int64_t *cand, double *poses,
                               int64_t *target_rows, int64_t *best, VcCounts &N) {
    const long long n_words = mk_words((long long)M.dims[0] * M.dims[1] * M.dims[2]);
    N = VcCounts();
    std::vector<double> dense;
    std::vector<long long> index;
    for (long long i = 0; i < n_targets; i++) {
        int64_t *const t = target_rows + VC_TARGET_ROW * i;
        for (int w = 0; w < VC_TARGET_ROW; w++) t[w] = 0;
        t[6] = -1;
        for (long long k = 0; k < n_offsets; k++) {
            const long long c = i * n_offsets + k;
            VcCand C;
            vc_candidate(bits, n_words, occ, M, targets + 3 * i, offsets + 3 * k, clearance, C);
            long long row[VC_ROW];
            vc_row_open(C, row);
            for (int w = 0; w < VC_ROW; w++) cand[VC_ROW * c + w] = row[w];
            for (int w = 0; w < 12; w++) poses[12 * c + w] = C.pose[w];
            t[C.status]++;
            N.n[C.status]++;
            if (C.status == VC_KEPT) {
                dense.insert(dense.end(), C.pose, C.pose + 12);
                index.push_back(c);
            }
        }
        for (int r = 0; r < k_best; r++) best[(long long)k_best * i + r] = -1;
    }
    std::vector<int64_t> rows(index.size() * VG_ROW);
    vg_gain_host(bits, occ, M, base, dense.data(), (long long)index.size(), rows.data());
    for (size_t j = 0; j < index.size(); j++) {
        int64_t *const row = cand + VC_ROW * index[j];
        const int64_t *const g = rows.data() + VG_ROW * j;
        row[3] = g[1]; row[4] = g[4]; row[5] = g[5]; row[6] = g[6];
    }
    std::vector<unsigned long long> keys;
    for (long long i = 0; i < n_targets; i++) {
        keys.clear();
        for (long long k = 0; k < n_offsets; k++) {
            const int64_t *const row = cand + VC_ROW * (i * n_offsets + k);
            if (row[0] == VC_KEPT && row[3] >= min_gain) keys.push_back(vc_key(row[3], k));
        }
        std::sort(keys.begin(), keys.end(), [](unsigned long long a, unsigned long long b) { return a > b; });
        for (size_t r = 0; r < keys.size() && r < (size_t)k_best; r++) {
            const long long c = i * n_offsets + vc_key_k(keys[r]);
            best[(long long)k_best * i + (long long)r] = c;
            cand[VC_ROW * c + 7] = (int64_t)r;
        }
        if (!keys.empty()) {
            target_rows[VC_TARGET_ROW * i + 6] = i * n_offsets + vc_key_k(keys[0]);
            target_rows[VC_TARGET_ROW * i + 7] = vc_key_gain(keys[0]);
        }
    }
    vc_best_of(target_rows, n_targets, N);
}

}  // namespace isdf
