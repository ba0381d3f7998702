// Host arithmetic of voxels cleared from the map in place (map_clear.hip), free of HIP so that a plain C++ program can
// run it under a sanitizer: the touched test of the ESDF raise, the touched box, and the raise itself in plain C++
// (isdf_clear_esdf_host calls mc_esdf_raise_host).  mc_touched is the function the device kernel calls: one statement for both sides.
//
// Why the touched test is enough.  The ESDF holds float(res * sqrt(d2)) of the exact integer d2 to the nearest occupied voxel.  When
// voxels are cleared a value can only rise, and the value of voxel p rises exactly when NO voxel at squared distance d2(p) is left
// occupied - so some cleared voxel v had |p - v|^2 == d2(p).  No d2 grid is kept; mu_esdf_skip recovers from the old float a bound
// B(p) with d2(p) < B(p) (q = old / res; q^2 >= d2 (1 - 2^-24)^2, so q^2 (1 + 2^-22) >= d2 and the bound adds 1).  p is TOUCHED when
// some cleared v has |p - v|^2 < B(p): a superset of the voxels that rise.  An untouched voxel keeps its value; a touched voxel, or any
// voxel of the touched voxels' bounding box, is recomputed exactly, and a recomputed voxel that did not rise gets its old bytes again.
#pragma once
#include "map_update_host.hpp"
#include <cmath>
#include <vector>

namespace isdf {

constexpr int MC_EDT_INF = 0x3fffffff;          // "no occupied voxel on this line / plane": map_build.hip's EDT_INF

// can the voxel whose old ESDF value is old_value have had its nearest occupied voxel at squared distance d2 (in voxels)?
MU_HD bool mc_touched(float old_value, double res, long long d2) { return !mu_esdf_skip(old_value, res, d2); }

// generate_esdf's conversion (edt_line_kernel<0>): res * sqrt(d2) in double, rounded once to float; no occupied voxel: sqrt(DBL_MAX)
MU_HD float mc_esdf_value(double res, int d2) {
    const double v = d2 >= MC_EDT_INF ? 1.7976931348623157e308 : (double)d2;
    return (float)(res * sqrt(v));
}

// out(q) = min_p (q - p)^2 + in(p) over a line of n samples `stride` apart: edt_line_kernel's bounded outward scan
MU_HD int mc_line_min(const int *in, int n, long long stride, int q) {
    int best = in[(long long)q * stride];
    for (int r = 1; r < n; r++) {
        const int rr = r * r;
        if (rr >= best) break;
        if (q - r >= 0) { const int v = rr + in[(long long)(q - r) * stride]; if (v < best) best = v; }          // INF + rr stays < 2^31
        if (q + r < n) { const int v = rr + in[(long long)(q + r) * stride]; if (v < best) best = v; }
    }
    return best;
}

struct McRaise {
    MuBox dirty, touched;               // the box of the cleared voxels / of the touched voxels (empty: lo > hi)
    long long n_touched = 0, recomputed = 0, raised = 0;
    bool none_left = false;             // no occupied voxel is left: every value is float(res * sqrt(DBL_MAX))
};

// touched_out (nullable): one byte per voxel.  esdf: the exact transform of the map BEFORE the clear.
inline void mc_touched_host(const float *esdf, const int dims[3], double res, const int32_t *cleared, long long n, uint8_t *touched_out, McRaise &R) {
    const int X = dims[0], Y = dims[1], Z = dims[2];
    for (int a = 0; a < 3; a++) { R.dirty.lo[a] = R.touched.lo[a] = 0x7FFFFFFF; R.dirty.hi[a] = R.touched.hi[a] = -1; }
    R.n_touched = 0;
    for (long long i = 0; i < n; i++)
        for (int a = 0; a < 3; a++) {
            if (cleared[3 * i + a] < R.dirty.lo[a]) R.dirty.lo[a] = cleared[3 * i + a];
            if (cleared[3 * i + a] > R.dirty.hi[a]) R.dirty.hi[a] = cleared[3 * i + a];
        }
    for (int x = 0; x < X; x++)
        for (int y = 0; y < Y; y++)
            for (int z = 0; z < Z; z++) {
                const size_t a = ((size_t)x * Y + y) * Z + z;
                bool t = false;
                if (n > 0 && mc_touched(esdf[a], res, mu_box_dist2(x, y, z, R.dirty.lo, R.dirty.hi)))
                    for (long long i = 0; i < n && !t; i++) {
                        const long long dx = x - cleared[3 * i], dy = y - cleared[3 * i + 1], dz = z - cleared[3 * i + 2];
                        t = mc_touched(esdf[a], res, dx * dx + dy * dy + dz * dz);
                    }
                if (touched_out) touched_out[a] = t ? 1 : 0;
                if (!t) continue;
                R.n_touched++;
                const int p[3] = {x, y, z};
                for (int k = 0; k < 3; k++) { if (p[k] < R.touched.lo[k]) R.touched.lo[k] = p[k]; if (p[k] > R.touched.hi[k]) R.touched.hi[k] = p[k]; }
            }
}

// The raise: esdf (the transform before the clear) becomes the transform of occ_new.  The transform is separable: the touched box
// Tx x Ty x Tz needs the z pass over X x Y x Tz, the y pass over X x Ty x Tz and the x pass over the box - the slabs the device uses.
inline void mc_esdf_raise_host(const uint8_t *occ_new, float *esdf, const int dims[3], double res, const int32_t *cleared, long long n, McRaise &R) {
    const int X = dims[0], Y = dims[1], Z = dims[2];
    const size_t n_vox = (size_t)X * Y * Z;
    mc_touched_host(esdf, dims, res, cleared, n, nullptr, R);
    R.recomputed = R.raised = 0;
    R.none_left = true;
    for (size_t a = 0; a < n_vox && R.none_left; a++) R.none_left = occ_new[a] != 1;
    if (R.none_left) {
        const float inf_like = mc_esdf_value(res, MC_EDT_INF);
        for (size_t a = 0; a < n_vox; a++) { if (std::memcmp(&esdf[a], &inf_like, sizeof(float)) != 0) R.raised++; esdf[a] = inf_like; }
        R.recomputed = (long long)n_vox;
        return;
    }
    if (mu_box_empty(R.touched)) return;
    const MuBox &T = R.touched;
    const int Tx = T.hi[0] - T.lo[0] + 1, Ty = T.hi[1] - T.lo[1] + 1, Tz = T.hi[2] - T.lo[2] + 1;
    std::vector<int> A((size_t)X * Y * Tz), B((size_t)X * Ty * Tz);
    for (int x = 0; x < X; x++)
        for (int y = 0; y < Y; y++) {           // z: the nearest occupied voxel below and above, two sweeps of the column
            const uint8_t *col = occ_new + ((size_t)x * Y + y) * Z;
            int *out = A.data() + ((size_t)x * Y + y) * Tz;
            int last = -1;
            for (int z = 0; z <= T.hi[2]; z++) {
                if (col[z] == 1) last = z;
                if (z >= T.lo[2]) out[z - T.lo[2]] = last < 0 ? MC_EDT_INF : (z - last) * (z - last);
            }
            int next = -1;
            for (int z = Z - 1; z >= T.lo[2]; z--) {
                if (col[z] == 1) next = z;
                if (z <= T.hi[2] && next >= 0 && (next - z) * (next - z) < out[z - T.lo[2]]) out[z - T.lo[2]] = (next - z) * (next - z);
            }
        }
    for (int x = 0; x < X; x++)
        for (int ty = 0; ty < Ty; ty++)
            for (int tz = 0; tz < Tz; tz++)
                B[((size_t)x * Ty + ty) * Tz + tz] = mc_line_min(A.data() + (size_t)x * Y * Tz + tz, Y, Tz, T.lo[1] + ty);
    for (int tx = 0; tx < Tx; tx++)
        for (int ty = 0; ty < Ty; ty++)
            for (int tz = 0; tz < Tz; tz++) {
                const int d2 = mc_line_min(B.data() + (size_t)ty * Tz + tz, X, (long long)Ty * Tz, T.lo[0] + tx);
                const float nv = mc_esdf_value(res, d2);
                float &e = esdf[((size_t)(T.lo[0] + tx) * Y + T.lo[1] + ty) * Z + T.lo[2] + tz];
                if (std::memcmp(&e, &nv, sizeof(float)) != 0) R.raised++;
                e = nv;
            }
    R.recomputed = mu_box_voxels(T);
}

}  // namespace isdf
