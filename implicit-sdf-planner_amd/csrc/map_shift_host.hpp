// Host arithmetic of the map window's shift (map_shift.hip), free of HIP so that a plain C++ program can run it under a
// sanitizer: the shifted box and its dims guard, a z-fastest grid translated with zero fill, the bands of the configuration space
// that a translation cannot supply.  The window moves by s voxels: new voxel v holds what old voxel v + s held.
#pragma once
#include "map_update_host.hpp"
#include <cmath>

namespace isdf {

inline bool msh_dims_bad(const int32_t dims[3]) {
    if (!dims) return true;
    for (int a = 0; a < 3; a++) if (dims[a] < 1 || dims[a] > 4096) return true;
    return false;
}

// bmin' = bmin + s res, bmax' = bmax + s res: one fp64 product and one sum each.  The product goes through a volatile, so that no
// compiler, whatever its contraction default, fuses the two: the result is the one numpy and isdf_set_pointcloud's callers compute.
// false: ceil((bmax' - bmin') / res) - isdf_set_pointcloud's expression (createGridMap) - is not dims on some axis.
inline bool msh_shift_geometry(const double bmin[3], const double bmax[3], double res, const int32_t dims[3], const int32_t s[3], double bmin_out[3], double bmax_out[3]) {
    bool ok = true;
    for (int a = 0; a < 3; a++) {
        const volatile double step = (double)s[a] * res;
        const double lo = bmin[a] + step, hi = bmax[a] + step;
        bmin_out[a] = lo; bmax_out[a] = hi;
        if (!(std::ceil((hi - lo) / res) == (double)dims[a])) ok = false;          // (a NaN fails the comparison)
    }
    return ok;
}

// out[v] = in[v + s] where v + s lies in the grid, zero elsewhere; elements of eb bytes, z fastest.  Row-wise memmove; in == out is
// allowed (the A*'s host table is shifted in place): the rows are visited in the order in which no row is written before it is read.
inline void msh_shift_grid(const void *in_v, size_t eb, const int32_t dims[3], const int32_t s[3], void *out_v) {
    const unsigned char *in = (const unsigned char *)in_v;
    unsigned char *out = (unsigned char *)out_v;
    const long long X = dims[0], Y = dims[1], Z = dims[2];
    const long long s0 = s[0], s1 = s[1], s2 = s[2];
    const long long z_lo = s2 < 0 ? (-s2 < Z ? -s2 : Z) : 0, z_hi = s2 > 0 ? (Z - s2 > 0 ? Z - s2 : 0) : Z;        // destination z with a source: [z_lo, z_hi)
    const size_t row = (size_t)Z * eb;
    const bool up = s0 > 0 || (s0 == 0 && s1 >= 0);            // the source row lies at or after the destination row: ascend
    const long long n_rows = X * Y;
    for (long long k = 0; k < n_rows; k++) {
        const long long r = up ? k : n_rows - 1 - k;
        const long long x = r / Y, y = r - x * Y;
        const long long sx = x + s0, sy = y + s1;
        unsigned char *d = out + (size_t)r * row;
        if (sx < 0 || sx >= X || sy < 0 || sy >= Y || z_lo >= z_hi) { std::memset(d, 0, row); continue; }
        const unsigned char *src = in + (size_t)(sx * Y + sy) * row;
        std::memmove(d + (size_t)z_lo * eb, src + (size_t)(z_lo + s2) * eb, (size_t)(z_hi - z_lo) * eb);
        if (z_lo > 0) std::memset(d, 0, (size_t)z_lo * eb);
        if (z_hi < Z) std::memset(d + (size_t)z_hi * eb, 0, (size_t)(Z - z_hi) * eb);
    }
}

// voxels of the new window whose source lies outside the old one
inline long long msh_voxels_entered(const int32_t dims[3], const int32_t s[3]) {
    long long kept = 1;
    for (int a = 0; a < 3; a++) {
        const long long m = s[a] < 0 ? -(long long)s[a] : (long long)s[a];
        kept *= m >= dims[a] ? 0 : dims[a] - m;
    }
    return (long long)dims[0] * dims[1] * dims[2] - kept;
}

// A voxel's configuration-space word reads the window [v - side, v + side].  After a shift the translated word is the new map's
// unless the window meets an entering voxel or reaches across a face of the map on one side of the shift only.  Per shifted axis
// that is two slabs over the whole extent of the other axes: the entering slab grown by side, and the side-thick band at the face
// the window moved away from.  Clamped to the grid, empty ones left out; the boxes may overlap.  Returns their number (<= 6).
inline int msh_shift_bands(const int32_t dims[3], const int32_t s[3], int side, MuBox boxes[6]) {
    int n = 0;
    for (int a = 0; a < 3; a++) {
        if (s[a] == 0) continue;
        const long long D = dims[a], m = s[a] < 0 ? -(long long)s[a] : (long long)s[a];
        long long lo[2], hi[2];
        if (s[a] > 0) { lo[0] = D - m - side; hi[0] = D - 1; lo[1] = 0; hi[1] = (long long)side - 1; }
        else { lo[0] = 0; hi[0] = m - 1 + side; lo[1] = D - side; hi[1] = D - 1; }
        for (int b = 0; b < 2; b++) {
            const long long l = lo[b] < 0 ? 0 : lo[b], h = hi[b] > D - 1 ? D - 1 : hi[b];
            if (l > h) continue;
            MuBox &B = boxes[n++];
            for (int q = 0; q < 3; q++) { B.lo[q] = 0; B.hi[q] = dims[q] - 1; }
            B.lo[a] = (int)l; B.hi[a] = (int)h;
        }
    }
    return n;
}

}  // namespace isdf
