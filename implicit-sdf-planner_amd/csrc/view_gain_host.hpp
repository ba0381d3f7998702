// The view gain (view_gain.hip), free of HIP so that a plain C++ program can run it under a sanitizer: how many voxels
// that are unknown today a depth camera would observe from a candidate pose.  Nothing of the ray, the walk or the stop rule is
// stated here: a ray is depth_cam_host.hpp's dc_ray on an image with no return at any pixel, its walk map_raycast_host.hpp's
// mr_cast_walk over map_scan_host.hpp's ms_ray_*, the known bit map_known_host.hpp's layout.  vg_ray, marked MU_HD, is the per-ray
// function both the kernel and the host form call; they differ only in the hook it calls per visited voxel.
//
// The definition, integers only from the ray's end point on.  For view j with pose cam2world_j (12 doubles, rows (R | t)):
//   rays   ray k = iv * nu + iu, nu = ceil(width / stride_u), nv = ceil(height / stride_v), is pixel (iu * stride_u, iv * stride_v).  Its
//          end point is dc_ray's for a pixel without a return with no_return_is_free = 1: p = ((u - cx) / fx, (v - cy) / fy, 1) taken to
//          the world (R p + t, each row summed left to right), the ray t -> that point given the length max_range_m, clipped to the
//          map's box shrunk by half a voxel, rounded to float32 once; fp64, nothing contracted into an FMA.  The origin is t.  A ray
//          whose end point is not finite or fails ms_quantize is skipped.
//   walk   mr_cast_walk from the origin's tick to the end's tick with test_origin = false: it ends at the first voxel after voxel 0 whose
//          occupancy byte is not 0, or at the end voxel.  V(ray) = the voxels of the walk from voxel 0 up to and including that one.
//          The occupancy byte decides whatever the known bit says: unknown voxels are transparent (the optimistic gain).
//   gain   S_j = the union of V(ray) over the rays that were not skipped; gain_j = |{v in S_j : K[v] = 0}| - a set per view, not a sum
//          per ray.
// A row is eight int64: {status, gain, n_rays, n_skipped, n_hits, steps_total, n_rays_unknown, 0}.  status 1: the pose has an entry that
// is not finite or its origin fails ms_quantize; every other word is 0 then.  n_rays = nu nv; n_hits: walks ended by an occupied voxel;
// steps_total: the sum of the walks' step counts as mr_count_row sums them; n_rays_unknown: rays whose V holds an unknown voxel.
#pragma once
#include "depth_cam_host.hpp"
#include "map_raycast_host.hpp"
#include "map_known_host.hpp"
#include <vector>

namespace isdf {

constexpr int VG_ROW = 8;               // int64 per view
constexpr int VG_SCORED = 0, VG_POSE_OUTSIDE = 1;

// one view: its rays and its origin's tick
struct VgView {
    DcRays Q;
    int qo[3];
    int ok;                     // 0: status 1
};

// what every view of a call shares: dc_rays_setup of the camera with a pose that the views replace
inline void vg_rays_base(int width, int height, double fx, double fy, double cx, double cy, int su, int sv, double max_range, const MapGeom &M, DcRays &Q) {
    const double eye[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    dc_rays_setup(width, height, fx, fy, cx, cy, eye, DC_FORMAT_U16_MM, su, sv, 0.0, max_range, 1, M, Q);
}

MU_HD void vg_view_setup(const DcRays &base, const MapGeom &M, const double pose[12], VgView &V) {
    V.Q = base;
    bool finite = true;
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) V.Q.R[3 * i + j] = pose[4 * i + j];
        V.Q.t[i] = pose[4 * i + 3];
    }
    for (int i = 0; i < 12; i++) finite = finite && (pose[i] - pose[i] == 0.0);
    V.qo[0] = V.qo[1] = V.qo[2] = 0;
    V.ok = finite && ms_quantize(M, pose[3], pose[7], pose[11], V.qo) ? 1 : 0;
}

struct VgCounts { long long gain = 0, n_skipped = 0, n_hits = 0, steps_total = 0, n_rays_unknown = 0; };

// One ray of a scored view.  zero_image: width x height uint16 zeros, the image with no return at any pixel.  visit(a) is called once
// for every voxel of V(ray), a = (x * ny + y) * nz + z, in the order of the walk, and returns whether K[a] = 0.  false: the ray is skipped.
template <typename Visit>
MU_HD bool vg_ray(const VgView &V, const MapGeom &M, const void *zero_image, const uint8_t *occ, int iu, int iv, long long &n_hits, long long &steps_total,
                  long long &n_rays_unknown, Visit &&visit) {
    float e[3];
    uint8_t hit;
    (void)dc_ray(V.Q, zero_image, iu, iv, e, hit);
    int qe[3], row[MR_ROW];
    if (!ms_quantize(M, (double)e[0], (double)e[1], (double)e[2], qe)) return false;
    mr_cast_walk(occ, M, V.qo, qe, false, row);
    n_hits += row[0] == MR_HIT;
    steps_total += row[1];
    // the same walk again, as far as the cast went
    MsRay r;
    ms_ray_begin(V.qo, qe, r);
    bool unknown = false;
    for (int s = 0;; s++) {
        if (visit(map_voxel(M, r.v))) unknown = true;
        if (s == row[1]) break;
        ms_ray_step(r);
    }
    n_rays_unknown += unknown;
    return true;
}

// ---- host form: rows_out = n_views x 8; seen: a plain bit vector per view, K's layout
inline void vg_gain_host(const uint32_t *bits, const uint8_t *occ, const MapGeom &M, const DcRays &base, const double *poses, long long n_views, int64_t *rows_out) {
    const long long n_words = mk_words((long long)M.dims[0] * M.dims[1] * M.dims[2]);
    const std::vector<uint16_t> zero((size_t)base.width * base.height, 0);
    std::vector<uint32_t> seen;
    for (long long j = 0; j < n_views; j++) {
        int64_t *const row = rows_out + VG_ROW * j;
        for (int w = 0; w < VG_ROW; w++) row[w] = 0;
        VgView V;
        vg_view_setup(base, M, poses + 12 * j, V);
        if (!V.ok) { row[0] = VG_POSE_OUTSIDE; continue; }
        seen.assign((size_t)n_words, 0u);
        VgCounts C;
        auto visit = [&](size_t a) {
            const uint32_t b = 1u << (unsigned)(a & 31);
            if (bits[a >> 5] & b) return false;
            if (!(seen[a >> 5] & b)) { seen[a >> 5] |= b; C.gain++; }
            return true;
        };
        for (int iv = 0; iv < V.Q.nv; iv++)
            for (int iu = 0; iu < V.Q.nu; iu++)
                if (!vg_ray(V, M, zero.data(), occ, iu, iv, C.n_hits, C.steps_total, C.n_rays_unknown, visit)) C.n_skipped++;
        row[0] = VG_SCORED; row[1] = C.gain; row[2] = (int64_t)V.Q.nu * V.Q.nv; row[3] = C.n_skipped; row[4] = C.n_hits; row[5] = C.steps_total;
        row[6] = C.n_rays_unknown;
    }
}

// what the info says of the rows: best_view = the lowest index among the largest gains of the scored rows, -1: none
struct VgBest { long long n_scored = 0, best_view = -1, best_gain = 0, gain_total = 0; };
inline VgBest vg_best(const int64_t *rows, long long n_views) {
    VgBest B;
    for (long long j = 0; j < n_views; j++) {
        const int64_t *const row = rows + VG_ROW * j;
        if (row[0] != VG_SCORED) continue;
        B.n_scored++;
        B.gain_total += row[1];
        if (B.best_view < 0 || row[1] > B.best_gain) { B.best_view = j; B.best_gain = row[1]; }
    }
    return B;
}

}  // namespace isdf
