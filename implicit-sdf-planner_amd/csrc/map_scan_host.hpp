// The ray of a range scan, in integers (map_scan.hip), free of HIP so that a plain C++ program can run it under a
// sanitizer.  The functions marked MU_HD are the ones the trace kernel calls: one statement of the quantisation and of the traversal
// for both sides, as grid_index.hpp is one statement of the binning - the host form and the kernel visit the same voxels bit for bit.
//
// A point is quantised once, in fp64, to 1/1024 of a voxel: u = (p - bmin) / res - grid_index's expression, one subtraction and one
// division -, q = floor(u * 1024) clamped to dim * 1024 - 1 (the product by a power of two is exact, so q >> 10 == floor(u) clamped:
// grid_index's voxel).  Everything after that is integer.  The ray runs between tick CENTRES, P = 2 q + 1 in half ticks, so that no
// half appears: a voxel boundary lies at 2048 v, D = |Pe - Po| is the ray's extent on an axis and m the half ticks from Po to the
// next boundary.  The next step goes to the axis with the smallest m / D, compared as m_a * D_b < m_b * D_a: m, D < 2^24 for
// dims <= 4096, so one 32 x 32 -> 64 bit multiply a side.  A tie goes to the lowest axis.  n_a = |ve_a - vo_a| steps are taken on
// axis a and no more, so the walk has exactly 1 + n_x + n_y + n_z voxels, never leaves the box of vo and ve and ends at ve whatever
// the ties did.
#pragma once
#include "map_update_host.hpp"
#include <cmath>
#include <vector>

namespace isdf {

constexpr int MS_TICKS_LOG2 = 10;           // ticks per voxel: 1024

// The map's metric geometry: the one way it travels through the map's queries and the scan, to kernels (by value) and host forms alike.
struct MapGeom { double bmin[3], bmax[3], res; int dims[3]; };

// of the host forms' arguments (ms_geometry_bad is their validator); the ctx's: map_query.hpp's map_geom(DevGrid)
inline MapGeom map_geom(const double bmin[3], const double bmax[3], double res, const int dims[3]) {
    MapGeom M;
    for (int a = 0; a < 3; a++) { M.bmin[a] = bmin[a]; M.bmax[a] = bmax[a]; M.dims[a] = dims[a]; }
    M.res = res;
    return M;
}

// the linear index of voxel v (z fastest)
MU_HD size_t map_voxel(const MapGeom &M, const int v[3]) { return ((size_t)v[0] * M.dims[1] + v[1]) * M.dims[2] + v[2]; }

// false: outside the map by grid_index's test (a coordinate < bmin or > bmax), or not finite; q is untouched then
MU_HD bool ms_quantize(const MapGeom &M, double x, double y, double z, int q[3]) {
    const double p[3] = {x, y, z};
    for (int a = 0; a < 3; a++)
        if (!(p[a] >= M.bmin[a] && p[a] <= M.bmax[a])) return false;            // (a NaN fails both comparisons)
    for (int a = 0; a < 3; a++) {
        const double u = (p[a] - M.bmin[a]) / M.res;
        const double t = floor(u * 1024.0);
        const long long top = ((long long)M.dims[a] << MS_TICKS_LOG2) - 1;
        q[a] = t >= (double)top ? (int)top : (int)(long long)t;            // 0 <= t: p >= bmin
    }
    return true;
}

// the walk from tick qo to tick qe
struct MsRay {
    int v[3];                   // the voxel the walk stands in
    int s[3];                   // direction of the steps on each axis
    int n[3];                   // steps left on each axis
    unsigned m[3], D[3];        // half ticks from the origin's centre to the next boundary; the ray's extent
};

MU_HD void ms_ray_begin(const int qo[3], const int qe[3], MsRay &r) {
    for (int a = 0; a < 3; a++) {
        const int Po = 2 * qo[a] + 1, Pe = 2 * qe[a] + 1;
        const int vo = qo[a] >> MS_TICKS_LOG2, ve = qe[a] >> MS_TICKS_LOG2;
        r.v[a] = vo;
        r.s[a] = Pe > Po ? 1 : -1;
        r.D[a] = (unsigned)(Pe > Po ? Pe - Po : Po - Pe);
        r.n[a] = ve > vo ? ve - vo : vo - ve;
        r.m[a] = (unsigned)(Pe > Po ? 2048 * (vo + 1) - Po : Po - 2048 * vo);
    }
}

MU_HD bool ms_ray_done(const MsRay &r) { return (r.n[0] | r.n[1] | r.n[2]) == 0; }

// one step: r.v becomes the voxel entered.  Only call while !ms_ray_done(r).  Returns the axis a of the step; the boundary crossed
// lies at the fraction (r.m[a] - 2048) / r.D[a] of the segment between the two tick centres (r.m[a] as it is after the call).
MU_HD int ms_ray_step_axis(MsRay &r) {
    int best = r.n[0] > 0 ? 0 : (r.n[1] > 0 ? 1 : 2);
    for (int b = best + 1; b < 3; b++)
        if (r.n[b] > 0 && (unsigned long long)r.m[b] * r.D[best] < (unsigned long long)r.m[best] * r.D[b]) best = b;
    r.v[best] += r.s[best];
    r.n[best] -= 1;
    r.m[best] += 2048u;
    return best;
}

MU_HD void ms_ray_step(MsRay &r) { (void)ms_ray_step_axis(r); }

// ---- host forms
inline bool ms_geometry_bad(const double bmin[3], const double bmax[3], double res, const int32_t dims[3]) {
    if (!bmin || !bmax || !dims || !(res > 0.0) || !(res <= 1.7976931348623157e308)) return true;
    for (int a = 0; a < 3; a++)
        if (dims[a] < 1 || dims[a] > 4096 || !(bmin[a] <= bmax[a]) || !(bmax[a] - bmin[a] <= 1.7976931348623157e308)) return true;
    return false;
}

// the visited voxels of one ray into ijk_out (capacity x 3, nullable when capacity is 0); returns their number, 0: the end point lies
// outside the map, -1: the origin does
inline long long ms_ray_host(const MapGeom &M, const double origin[3], const float end[3], int32_t *ijk_out, long long capacity) {
    int qo[3], qe[3];
    if (!ms_quantize(M, origin[0], origin[1], origin[2], qo)) return -1;
    if (!ms_quantize(M, (double)end[0], (double)end[1], (double)end[2], qe)) return 0;
    MsRay r;
    ms_ray_begin(qo, qe, r);
    long long k = 0;
    for (;;) {
        if (k < capacity) for (int a = 0; a < 3; a++) ijk_out[3 * k + a] = r.v[a];
        k++;
        if (ms_ray_done(r)) break;
        ms_ray_step(r);
    }
    return k;
}

struct MsSets {
    long long n_free = 0, n_skipped = 0, n_hits = 0, n_hit_voxels = 0;
    MuBox ray;                  // the box of every visited voxel (empty: no ray traced)
};

// The sets of one scan: visited[v] = 1 for every voxel some ray visits, a hit ray's end voxel excepted; hits[v] = the multiplicity of
// v in H.  F = visited and not in H.  false: the origin lies outside the map.
inline bool ms_sets_host(const MapGeom &M, const double origin[3], const float *xyz, const uint8_t *hit, long long n_rays, std::vector<uint8_t> &free_set,
                         std::vector<uint32_t> &hits, MsSets &S) {
    const size_t n_vox = (size_t)M.dims[0] * M.dims[1] * M.dims[2];
    free_set.assign(n_vox, 0);
    hits.assign(n_vox, 0);
    S = MsSets();
    for (int a = 0; a < 3; a++) { S.ray.lo[a] = 0x7FFFFFFF; S.ray.hi[a] = -1; }
    int qo[3], qe[3];
    if (!ms_quantize(M, origin[0], origin[1], origin[2], qo)) return false;
    for (long long i = 0; i < n_rays; i++) {
        if (!ms_quantize(M, (double)xyz[3 * i], (double)xyz[3 * i + 1], (double)xyz[3 * i + 2], qe)) { S.n_skipped++; continue; }
        const bool is_hit = !hit || hit[i] != 0;
        MsRay r;
        ms_ray_begin(qo, qe, r);
        for (int a = 0; a < 3; a++) {           // the walk stays in the box of its two ends
            const int ve = qe[a] >> MS_TICKS_LOG2;
            const int lo = r.v[a] < ve ? r.v[a] : ve, hi = r.v[a] < ve ? ve : r.v[a];
            if (lo < S.ray.lo[a]) S.ray.lo[a] = lo;
            if (hi > S.ray.hi[a]) S.ray.hi[a] = hi;
        }
        for (;;) {
            const size_t a = map_voxel(M, r.v);
            const bool last = ms_ray_done(r);
            if (last && is_hit) { hits[a]++; S.n_hits++; }
            else free_set[a] = 1;
            if (last) break;
            ms_ray_step(r);
        }
    }
    for (size_t a = 0; a < n_vox; a++) {
        if (hits[a]) { free_set[a] = 0; S.n_hit_voxels++; }
        S.n_free += free_set[a];
    }
    return true;
}

}  // namespace isdf
