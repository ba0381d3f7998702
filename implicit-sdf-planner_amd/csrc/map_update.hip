// The map updated in place from new sensor points: isdf_update_pointcloud / isdf_update_voxels.
//   mu_mark_kernel          one lane per new point (or listed voxel): the kept count goes up by one, and the ONE lane whose add carries
//                           a count across the threshold (old + 1 == thr: whatever the order of the adds, exactly one add sees it)
//                           sets the voxel occupied, appends it to the new-voxel list and widens the dirty box.  The voxel form
//                           exchanges the occupancy byte 0 -> 1 instead (a 32-bit atomic OR on the dword that holds it).
//   mu_esdf_kernel          one lane per voxel of the map: new = min(old, float(res * sqrt(d2 to the nearest NEW voxel))).  The
//                           conversion is monotone, so the min on floats is the float of the min integer and no d2 grid is kept.  A
//                           voxel whose distance to the dirty box cannot beat its old value is left alone (mu_esdf_skip); a workgroup
//                           whose 256 voxels all skip leaves at once; the others scan the list, staged through LDS in chunks.
// The front end is refreshed by the boxed kernels every in-place change shares (map_change.hip), through map_frontend_launch.
// Every consumer of the new-voxel list takes a minimum over it: its order, which the atomics leave undefined, never shows.
// Integer work throughout except the one res * sqrt(d2) of the ESDF, a single multiplication (nothing to contract).
#include "isdf_ctx.hpp"
#include "frontend_dev.hpp"
#include "grid_index.hpp"
#include "map_update_host.hpp"
#include "map_change.hpp"
#include "swept_field.hpp"
#include <algorithm>
#include <cmath>
#include <cstring>

namespace isdf {

void launch_threshold_counts(const unsigned *counts, size_t n, unsigned thr, uint8_t *occ, hipStream_t stream);     // map_build.hip

template <bool VOXELS>
__global__ __launch_bounds__(256) void mu_mark_kernel(const void *__restrict__ in, long long n, DevGrid G, unsigned *__restrict__ counts, unsigned thr,
                                                      uint8_t *__restrict__ occ, const float *__restrict__ esdf, MuVoxel *__restrict__ list, unsigned cap,
                                                      MapListRecord *__restrict__ rec) {
    if (esdf && blockIdx.x == 0 && threadIdx.x == 0) rec->esdf0 = __float_as_uint(esdf[0]);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        int ix, iy, iz;
        bool crossed;
        if (VOXELS) {
            const int *ijk = (const int *)in;
            ix = ijk[3 * i]; iy = ijk[3 * i + 1]; iz = ijk[3 * i + 2];      // (checked against the grid on the host)
            const size_t a = ((size_t)ix * G.Y + iy) * G.Z + iz;
            const unsigned sh = 8u * (unsigned)(a & 3);
            const unsigned old = atomicOr((unsigned *)(occ + (a & ~(size_t)3)), 1u << sh);       // occ is allocated as whole dwords
            crossed = ((old >> sh) & 0xFFu) == 0u;            // (an occupancy byte holds 0 or 1: isdf_set_grid and the threshold kernel write nothing else)
        } else {
            const float *xyz = (const float *)in;
            (void)grid_index(G, (double)xyz[3 * i], (double)xyz[3 * i + 1], (double)xyz[3 * i + 2], ix, iy, iz);
            const size_t a = ((size_t)ix * G.Y + iy) * G.Z + iz;
            const unsigned old = atomicAdd(&counts[a], 1u);
            crossed = thr >= 1u && old + 1u == thr;          // thr == 0: every voxel is occupied already
            if (crossed) occ[a] = 1;
        }
        if (crossed) map_list_append(rec, list, cap, ix, iy, iz);
    }
}

constexpr int MU_CHUNK = 1024;          // new voxels staged per round: 8 KiB of LDS

__global__ __launch_bounds__(256) void mu_esdf_kernel(DevGrid G, float *__restrict__ esdf, const MuVoxel *__restrict__ list, int n_list, MuBox box,
                                                      MapListRecord *__restrict__ rec) {
    __shared__ MuVoxel s_list[MU_CHUNK];
    const size_t total = (size_t)G.X * G.Y * G.Z;
    const size_t a = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool in = a < total;
    int x = 0, y = 0, z = 0;
    float old = 0.f;
    bool scan = false;
    if (in) {
        z = (int)(a % G.Z); y = (int)((a / G.Z) % G.Y); x = (int)(a / ((size_t)G.Y * G.Z));
        old = esdf[a];
        scan = !mu_esdf_skip(old, G.res, mu_box_dist2(x, y, z, box.lo, box.hi));
    }
    if (!__syncthreads_or(scan ? 1 : 0)) return;          // the same answer in every thread: the barriers below are uniform
    long long best = 0x7FFFFFFFFFFFll;
    for (int c0 = 0; c0 < n_list; c0 += MU_CHUNK) {
        const int m = min(MU_CHUNK, n_list - c0);
        __syncthreads();
        for (int t = threadIdx.x; t < m; t += 256) s_list[t] = list[c0 + t];
        __syncthreads();
        if (scan)
            for (int t = 0; t < m; t++) {
                const MuVoxel v = s_list[t];              // the same entry in every lane: an LDS broadcast
                const long long dx = x - (int)v.x, dy = y - (int)v.y, dz = z - (int)v.z;
                best = min(best, dx * dx + dy * dy + dz * dz);
            }
    }
    if (scan) {
        const float nv = (float)(G.res * sqrt((double)best));       // generate_esdf's conversion (edt_line_kernel<0>)
        if (nv < old) { esdf[a] = nv; atomicAdd(&rec->tally, 1ull); }
    }
}

}  // namespace isdf

using namespace isdf;

extern "C" void isdf_map_update_params_default(isdf_map_update_params *p) {
    if (!p) return;
    p->max_new_voxels = 65536;
    p->full_fraction = 0.5;
    p->refresh_esdf = 1;
    p->refresh_frontend = 1;
}

extern "C" void isdf_map_update_sizes(int sizes_out[2]) {
    if (!sizes_out) return;
    sizes_out[0] = (int)sizeof(isdf_map_update_params); sizes_out[1] = (int)sizeof(isdf_map_update_info);
}

extern "C" int isdf_map_counts_get(isdf_ctx *c, uint32_t *out) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    if (!out) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "null output");
    if (!c->have_geom || !c->d_counts) return isdf_fail(c, ISDF_ERR_STATE, "no kept point counts (isdf_set_pointcloud keeps them; isdf_set_grid and isdf_update_voxels drop them)");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy(out, c->d_counts, (size_t)c->grid.X * c->grid.Y * c->grid.Z * sizeof(unsigned), hipMemcpyDeviceToHost));
    return ISDF_OK;
}

// everything after the hand-over of a frame that occupied at least one voxel
int isdf::mu_refresh_products(isdf_ctx *c, MapUpdateState &S, const isdf_map_update_params &P, const MapListRecord &R, unsigned cap, bool voxels, isdf_map_update_info &info) {
    const hipStream_t st = c->stream;
    const DevGrid &G = c->grid;
    const size_t n_vox = (size_t)G.X * G.Y * G.Z;
    int rc;
    // The cost-to-go field: dropped (mode 0 of isdf_frontend_field_set_repair), or repaired once the configuration space is the new
    // map's (mode 1).  It is invalid from here until the repair has gone through: every error path leaves it dropped.
    const bool repair = P.refresh_frontend != 0 && isdf_field_change_wanted(c, FfChange::Closing);
    const MapRefresh M = map_refresh_begin(c, R, cap, voxels, P.refresh_esdf, P.refresh_frontend, P.full_fraction, &info.field_dropped);
    if (!repair) (void)isdf_field_gate_drop(c);          // (a gated field that does not follow: its gate and its follow report go with it)
    for (int a = 0; a < 3; a++) { info.dirty_lo[a] = M.box.lo[a]; info.dirty_hi[a] = M.box.hi[a]; }
    float esdf0;
    std::memcpy(&esdf0, &R.esdf0, sizeof(float));
    const bool full = M.over || (M.do_esdf && std::isinf(esdf0));
    info.path = full ? 2 : 1;

    // ---- ESDF
    if (full && !voxels) {
        launch_threshold_counts(c->d_counts, n_vox, (unsigned)c->counts_thr, c->d_occ, st);
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipEventRecord(S.ev[2], st));
    if (M.do_esdf) {
        if (full) { if ((rc = isdf_generate_esdf(c))) return rc; }
        else {
            hipLaunchKernelGGL(mu_esdf_kernel, dim3((unsigned)((n_vox + 255) / 256)), dim3(256), 0, st, G, c->d_esdf.get(), S.d_list.get(), (int)R.n, M.box, &S.rec.dev()->list);
            HIPCHK(c, hipGetLastError());
        }
        c->bricks_stale = true;
        info.esdf_refreshed = 1;
    }
    HIPCHK(c, hipEventRecord(S.ev[3], st));

    // ---- front end, the field's repair around the synchronisation
    MapFrontend F;
    if ((rc = map_frontend_stage(c, S, FfChange::Closing, repair, P.refresh_frontend != 0, full, M, F, &info.field_dropped))) return rc;
    map_frontend_report(F, info);
    info.esdf_voxels_lowered = (long long)S.rec.host().list.tally;
    info.esdf_ms = S.ev.ms(2, 3);
    // the kept clearance report (mode 1 of isdf_traj_check_set_watch): the new voxels folded in, after every product above.  A failing
    // step drops the report and fails the update as a whole, as a failing repair does.
    if (traj_watch_armed(c) && (rc = traj_watch_fold(c, S.d_list.get(), R.n, cap))) return rc;
    return ISDF_OK;
}

namespace {

// the update proper; `in` is the host array of the points (voxels == false) or of the checked voxel indices
int map_update(isdf_ctx *c, const void *in, long long n_in, bool voxels, const isdf_map_update_params *params, isdf_map_update_info *info_out) {
    isdf_map_update_params P;
    isdf_map_update_params_default(&P);
    if (params) P = *params;
    if (P.max_new_voxels < 0 || !(P.full_fraction >= 0.0)) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "bad map update parameters");
    isdf_map_update_info info{};
    for (int a = 0; a < 3; a++) { info.dirty_lo[a] = 0; info.dirty_hi[a] = -1; }
    info.n_points = n_in;
    info.field_dropped = c->gate_dropped ? 1 : 0;      // (a gated field went in map_change_ready, whatever this frame changes)
    MapUpdateState *Sp;
    int rc = map_begin(c, &Sp);
    if (rc) return rc;
    MapUpdateState &S = *Sp;
    const hipStream_t st = c->stream;
    const DevGrid &G = c->grid;

    // ---- count, find the new voxels: one hand-over
    const unsigned cap = map_list_cap(P.max_new_voxels, (unsigned long long)n_in, (unsigned long long)G.X * G.Y * G.Z);
    if ((rc = map_stage(c, S, in, (size_t)n_in * 3 * (voxels ? sizeof(int) : sizeof(float)), nullptr, 0, std::max<size_t>(cap, 1), S.ev[0]))) return rc;
    if (n_in > 0) {
        const unsigned blocks = (unsigned)std::min<long long>((n_in + 255) / 256, 2048);
        MapListRecord *const d_rec = &S.rec.dev()->list;
        if (voxels) hipLaunchKernelGGL(mu_mark_kernel<true>, dim3(blocks), dim3(256), 0, st, (const void *)S.d_in.get(), n_in, G, (unsigned *)nullptr, 0u, c->d_occ.get(),
                                       (const float *)c->d_esdf.get(), S.d_list.get(), cap, d_rec);
        else hipLaunchKernelGGL(mu_mark_kernel<false>, dim3(blocks), dim3(256), 0, st, (const void *)S.d_in.get(), n_in, G, c->d_counts.get(), (unsigned)c->counts_thr,
                                c->d_occ.get(), (const float *)c->d_esdf.get(), S.d_list.get(), cap, d_rec);
        HIPCHK(c, hipGetLastError());
    }
    if ((rc = map_hand_over(c, S, S.ev[1], "map update", voxels))) return rc;          // the kernel may have run: the occupancy may have advanced
    const MapListRecord R = S.rec.host().list;
    info.count_ms = S.ev.ms(0, 1);
    info.n_new_voxels = R.n;
    if (R.n > 0) {                      // (nothing but the counts changed: every product stays in place, the field included)
        // from here on the occupancy has advanced: a failure must not leave products behind that describe the old map
        rc = mu_refresh_products(c, S, P, R, cap, voxels, info);
        if (rc != ISDF_OK) { mu_drop_derived(c, voxels); return rc; }
    }
    if (info_out) *info_out = info;
    return ISDF_OK;
}

}  // namespace

extern "C" int isdf_update_pointcloud(isdf_ctx *c, const float *xyz, long long n_points, const isdf_map_update_params *params, isdf_map_update_info *info_out) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    const int rc = map_change_ready(c, "the map update", xyz, n_points, true);
    return rc ? rc : map_update(c, xyz, n_points, false, params, info_out);
}

extern "C" int isdf_update_voxels(isdf_ctx *c, const int32_t *ijk, long long n_voxels, const isdf_map_update_params *params, isdf_map_update_info *info_out) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    int rc = map_change_ready(c, "the map update", ijk, n_voxels, false);
    if (!rc) rc = map_voxels_in_grid(c, ijk, n_voxels);
    return rc ? rc : map_update(c, ijk, n_voxels, true, params, info_out);
}
