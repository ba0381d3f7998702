// Host arithmetic of the in-place map update (map_update.hip), free of HIP so that a plain C++ program can run it under a sanitizer:
// the dirty box grown and clamped, the skip rule of the ESDF refresh, the scatter of a packed box into the host table.
// The two functions marked MU_HD are the ones the device kernels call: one statement of the arithmetic for both sides.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define MU_HD __host__ __device__ inline
#else
#define MU_HD inline
#endif

namespace isdf {

struct MuBox { int lo[3], hi[3]; };       // inclusive voxel indices; lo > hi on some axis: empty
struct MuVoxel { unsigned short x, y, z, pad; };        // an entry of the update's new-voxel list (a grid dimension is at most 4096)

inline bool mu_box_empty(const MuBox &b) { return b.lo[0] > b.hi[0] || b.lo[1] > b.hi[1] || b.lo[2] > b.hi[2]; }

inline long long mu_box_voxels(const MuBox &b) {
    if (mu_box_empty(b)) return 0;
    return (long long)(b.hi[0] - b.lo[0] + 1) * (b.hi[1] - b.lo[1] + 1) * (b.hi[2] - b.lo[2] + 1);
}

// the box grown by `side` voxels on every side and clamped to the grid: every voxel whose configuration-space word reads a voxel of b
inline MuBox mu_box_grow(const MuBox &b, int side, const int dims[3]) {
    MuBox g = b;
    if (mu_box_empty(b)) return g;
    for (int a = 0; a < 3; a++) {
        g.lo[a] = b.lo[a] - side < 0 ? 0 : b.lo[a] - side;
        g.hi[a] = b.hi[a] + side > dims[a] - 1 ? dims[a] - 1 : b.hi[a] + side;
    }
    return g;
}

// the smallest box that holds both (an empty one adds nothing)
inline MuBox mu_box_union(const MuBox &a, const MuBox &b) {
    if (mu_box_empty(a)) return b;
    if (mu_box_empty(b)) return a;
    MuBox u;
    for (int k = 0; k < 3; k++) { u.lo[k] = a.lo[k] < b.lo[k] ? a.lo[k] : b.lo[k]; u.hi[k] = a.hi[k] > b.hi[k] ? a.hi[k] : b.hi[k]; }
    return u;
}

// squared distance, in voxels, from voxel (x, y, z) to the nearest voxel of the box (0 inside)
MU_HD long long mu_box_dist2(int x, int y, int z, const int lo[3], const int hi[3]) {
    const int p[3] = {x, y, z};
    long long d2 = 0;
    for (int a = 0; a < 3; a++) {
        const long long d = p[a] < lo[a] ? (long long)lo[a] - p[a] : (p[a] > hi[a] ? (long long)p[a] - hi[a] : 0);
        d2 += d * d;
    }
    return d2;
}

// The ESDF refresh may leave a voxel alone when no voxel of the dirty box can be nearer than its old nearest obstacle.  The old value
// is float(res * sqrt(d2)) of an integer d2; the float rounding moves (old / res)^2 by less than d2 * 2^-23, the divisions and the
// square by far less, so d2 <= (old / res)^2 * (1 + 2^-22) + 1 - the bound errs towards scanning.  An infinite or NaN old value never skips.
MU_HD bool mu_esdf_skip(float old_value, double res, long long box_d2) {
    const double q = (double)old_value / res;
    const double bound = q * q * (1.0 + 1.0 / 4194304.0) + 1.0;
    return (double)box_d2 >= bound;
}

// `packed` holds the words of the box's voxels (x, then y, then z fastest; nw dwords per voxel); they go to their places in the
// whole-map table (dims[0] x dims[1] x dims[2] voxels, z fastest)
inline void mu_scatter_box(uint32_t *table, const int dims[3], size_t nw, const MuBox &b, const uint32_t *packed) {
    if (mu_box_empty(b)) return;
    const size_t ez = (size_t)(b.hi[2] - b.lo[2] + 1), row = ez * nw;
    for (int x = b.lo[0]; x <= b.hi[0]; x++)
        for (int y = b.lo[1]; y <= b.hi[1]; y++) {
            std::memcpy(table + (((size_t)x * dims[1] + y) * dims[2] + b.lo[2]) * nw, packed, row * sizeof(uint32_t));
            packed += row;
        }
}

}  // namespace isdf
