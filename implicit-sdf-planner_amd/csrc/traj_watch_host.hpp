// Host arithmetic of the kept clearance report's fold (traj_watch.hip), free of HIP so that a plain C++ program can
// run it under a sanitizer: two reports over DISJOINT voxel sets merged into the report of their union.  Integer sums add, the
// minimum is the lexicographic (value, voxel index), piece minima are element-wise minima, rows interleave by ascending voxel id.
// The functions marked TW_HD are the ones the device kernels call: one statement of the arithmetic for both sides.
#pragma once
#include "../../include/isdf_accel.h"
#include <cstddef>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define TW_HD __host__ __device__ inline
#else
#define TW_HD inline
#endif

namespace isdf {

// entries of the ascending list vox[0, n) that are smaller than id: a row's place in the merged list is its own index plus this
// count over the OTHER list
TW_HD long long tw_rank(const long long *vox, long long n, long long id) {
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = lo + (hi - lo) / 2;
        if (vox[mid] < id) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// does the minimum (vb, ib) replace (va, ia)?  A voxel index of -1 says "nothing qualified"; ties go to the lower voxel index
TW_HD bool tw_min_takes(double va, long long ia, double vb, long long ib) {
    if (ib < 0) return false;
    if (ia < 0) return true;
    return vb < va || (vb == va && ib < ia);
}

// the info words and the N piece minima; culled, margin, far_r and the three times are a's.  out / pm_out may be a / pm_a.
// min_changed_out (nullable): 1 when the minimum is b's.
inline void tw_fold_info(int N, const isdf_traj_check_info *a, const double *pm_a, const isdf_traj_check_info *b, const double *pm_b,
                         isdf_traj_check_info *out, double *pm_out, int *min_changed_out) {
    isdf_traj_check_info r = *a;
    r.occupied_in_box = a->occupied_in_box + b->occupied_in_box;
    r.candidates = a->candidates + b->candidates;
    r.qualified = a->qualified + b->qualified;
    r.n_below_margin = a->n_below_margin + b->n_below_margin;
    r.n_penetrating = a->n_penetrating + b->n_penetrating;
    const bool take = tw_min_takes(a->min_clearance, (long long)a->min_voxel, b->min_clearance, (long long)b->min_voxel);
    if (take) {
        r.min_clearance = b->min_clearance; r.min_tstar = b->min_tstar;
        for (int q = 0; q < 3; q++) r.min_point[q] = b->min_point[q];
        r.min_voxel = b->min_voxel; r.min_piece = b->min_piece;
    }
    if (min_changed_out) *min_changed_out = take ? 1 : 0;
    if (pm_out)
        for (int i = 0; i < N; i++) {
            const double x = pm_a ? pm_a[i] : 1e1, y = pm_b ? pm_b[i] : 1e1;
            pm_out[i] = y < x ? y : x;
        }
    *out = r;
}

// rows (5 doubles each) and voxel ids of both sides into their places; false when the lists are not ascending or share an id
// (nothing is then promised about the output)
inline bool tw_fold_rows(const double *rows_a, const long long *vox_a, long long na, const double *rows_b, const long long *vox_b, long long nb,
                         double *rows_out, long long *vox_out) {
    for (long long i = 1; i < na; i++) if (!(vox_a[i - 1] < vox_a[i])) return false;
    for (long long j = 1; j < nb; j++) if (!(vox_b[j - 1] < vox_b[j])) return false;
    for (long long i = 0; i < na; i++) {
        const long long r = tw_rank(vox_b, nb, vox_a[i]);
        if (r < nb && vox_b[r] == vox_a[i]) return false;
        std::memcpy(rows_out + 5 * (size_t)(i + r), rows_a + 5 * (size_t)i, 5 * sizeof(double));
        vox_out[i + r] = vox_a[i];
    }
    for (long long j = 0; j < nb; j++) {
        const long long r = tw_rank(vox_a, na, vox_b[j]);
        std::memcpy(rows_out + 5 * (size_t)(j + r), rows_b + 5 * (size_t)j, 5 * sizeof(double));
        vox_out[j + r] = vox_b[j];
    }
    return true;
}

}  // namespace isdf
