// Voxels cleared from the map in place: isdf_clear_pointcloud / isdf_clear_voxels, the inverse of map_update.hip.
//   mc_mark_kernel     one lane per point (or listed voxel).  The point form takes one off the kept count with a compare-and-swap
//                      loop that never stores below 0 (a lane that reads 0 gives up and is counted as ignored).  EXACTLY ONE LANE SEES
//                      THE CROSSING: the successful swaps on one count are totally ordered and each takes it from v to v - 1, v >= 1;
//                      nothing adds during the kernel, so the count's values strictly fall, the value thr is left at most once - by the
//                      one swap whose expected value was thr - and it is left exactly when the count starts >= thr and ends < thr.
//                      That lane frees the voxel, appends it to the cleared list and widens the dirty box.  The voxel form clears the
//                      occupancy byte with a 32-bit atomic AND on the dword that holds it; the lane that read a set byte freed it.
//   mc_touched_kernel  the ESDF raise, part one.  One lane per voxel of the map: is some cleared voxel near enough to have been this
//                      voxel's nearest obstacle (mc_touched on the old float, map_clear_host.hpp)?  Box pre-test, workgroup early-out,
//                      then the list through LDS - the update's mu_esdf_kernel with the comparison turned round.  Leaves the touched
//                      voxels' box and count, and whether any voxel of the map is still occupied.
//   mc_edt_z / _y / _x the raise, part two: the exact transform again over the touched box Tx x Ty x Tz.  It is separable: z pass over
//                      X x Y x Tz (one lane per column, two sweeps over the occupancy bytes), y pass over X x Ty x Tz, x pass over the
//                      box with edt_line_kernel<0>'s conversion - the integer d2 is unique, so float(res * sqrt(d2)) is the byte
//                      isdf_generate_esdf writes.  Scratch: the two slabs, not the map.
//   front end          the shared boxed kernels through map_frontend_launch (map_change.hip): they recompute from the occupancy.
// A value can only rise, an untouched value stays, and every consumer of the cleared list asks "is there an entry that ...": its
// order, which the atomics leave undefined, never shows.
#include "isdf_ctx.hpp"
#include "frontend_dev.hpp"
#include "grid_index.hpp"
#include "map_clear_host.hpp"
#include "map_change.hpp"
#include "swept_field.hpp"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace isdf {

template <bool VOXELS>
__global__ __launch_bounds__(256) void mc_mark_kernel(const void *__restrict__ in, long long n, DevGrid G, unsigned *__restrict__ counts, unsigned thr,
                                                      uint8_t *__restrict__ occ, MuVoxel *__restrict__ list, unsigned cap, MapListRecord *__restrict__ rec) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        int ix, iy, iz;
        bool crossed = false;
        if (VOXELS) {
            const int *ijk = (const int *)in;
            ix = ijk[3 * i]; iy = ijk[3 * i + 1]; iz = ijk[3 * i + 2];      // (checked against the grid on the host)
            const size_t a = ((size_t)ix * G.Y + iy) * G.Z + iz;
            const unsigned sh = 8u * (unsigned)(a & 3);
            const unsigned old = atomicAnd((unsigned *)(occ + (a & ~(size_t)3)), ~(0xFFu << sh));        // occ is allocated as whole dwords
            crossed = ((old >> sh) & 0xFFu) != 0u;
        } else {
            const float *xyz = (const float *)in;
            (void)grid_index(G, (double)xyz[3 * i], (double)xyz[3 * i + 1], (double)xyz[3 * i + 2], ix, iy, iz);
            const size_t a = ((size_t)ix * G.Y + iy) * G.Z + iz;
            unsigned seen = counts[a];
            for (;;) {
                if (seen == 0u) { atomicAdd(&rec->tally, 1ull); break; }
                const unsigned was = atomicCAS(&counts[a], seen, seen - 1u);
                if (was == seen) { crossed = thr >= 1u && seen == thr; break; }          // thr == 0: every voxel stays occupied
                seen = was;
            }
            if (crossed) occ[a] = 0;
        }
        if (crossed) map_list_append(rec, list, cap, ix, iy, iz);
    }
}

constexpr int MC_CHUNK = 1024;          // cleared voxels staged per round: 8 KiB of LDS

__global__ __launch_bounds__(256) void mc_touched_kernel(DevGrid G, const float *__restrict__ esdf, const uint8_t *__restrict__ occ,
                                                         const MuVoxel *__restrict__ list, int n_list, MuBox box, McEsdfRecord *__restrict__ rec) {
    __shared__ MuVoxel s_list[MC_CHUNK];
    __shared__ int s_lo[3], s_hi[3];
    __shared__ unsigned s_cnt;
    const size_t total = (size_t)G.X * G.Y * G.Z;
    const size_t a = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool in = a < total;
    if (threadIdx.x < 3) { s_lo[threadIdx.x] = 0x7FFFFFFF; s_hi[threadIdx.x] = -1; }
    if (threadIdx.x == 0) s_cnt = 0u;
    int x = 0, y = 0, z = 0;
    float old = 0.f;
    bool scan = false;
    if (in) {
        z = (int)(a % G.Z); y = (int)((a / G.Z) % G.Y); x = (int)(a / ((size_t)G.Y * G.Z));
        old = esdf[a];
        scan = mc_touched(old, G.res, mu_box_dist2(x, y, z, box.lo, box.hi));
    }
    if (__syncthreads_or(in && occ[a] == 1 ? 1 : 0) && threadIdx.x == 0) atomicOr(&rec->any_occ, 1u);
    if (!__syncthreads_or(scan ? 1 : 0)) return;          // the same answer in every thread: the barriers below are uniform
    bool hit = false;
    for (int c0 = 0; c0 < n_list; c0 += MC_CHUNK) {
        const int m = min(MC_CHUNK, n_list - c0);
        __syncthreads();
        for (int t = threadIdx.x; t < m; t += 256) s_list[t] = list[c0 + t];
        __syncthreads();
        if (scan && !hit)
            for (int t = 0; t < m && !hit; t++) {
                const MuVoxel v = s_list[t];
                const long long dx = x - (int)v.x, dy = y - (int)v.y, dz = z - (int)v.z;
                hit = mc_touched(old, G.res, dx * dx + dy * dy + dz * dz);
            }
    }
    if (hit) {
        atomicMin(&s_lo[0], x); atomicMin(&s_lo[1], y); atomicMin(&s_lo[2], z);
        atomicMax(&s_hi[0], x); atomicMax(&s_hi[1], y); atomicMax(&s_hi[2], z);
        atomicAdd(&s_cnt, 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_cnt) {
        atomicMin(&rec->lo[0], s_lo[0]); atomicMin(&rec->lo[1], s_lo[1]); atomicMin(&rec->lo[2], s_lo[2]);
        atomicMax(&rec->hi[0], s_hi[0]); atomicMax(&rec->hi[1], s_hi[1]); atomicMax(&rec->hi[2], s_hi[2]);
        atomicAdd(&rec->touched, (unsigned long long)s_cnt);
    }
}

// z pass: one lane per column (x, y) of the map; out: [X * Y][Tz], the squared distance to the nearest occupied voxel of the column
__global__ __launch_bounds__(256) void mc_edt_z_kernel(DevGrid G, const uint8_t *__restrict__ occ, int z0, int z1, int *__restrict__ out_a) {
    const long long col = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= (long long)G.X * G.Y) return;
    const int Tz = z1 - z0 + 1;
    const uint8_t *c = occ + (size_t)col * G.Z;
    int *out = out_a + (size_t)col * Tz;
    int last = -1;
    for (int z = 0; z <= z1; z++) {
        if (c[z] == 1) last = z;
        if (z >= z0) out[z - z0] = last < 0 ? MC_EDT_INF : (z - last) * (z - last);
    }
    int next = -1;
    for (int z = G.Z - 1; z >= z0; z--) {
        if (c[z] == 1) next = z;
        if (z <= z1 && next >= 0) out[z - z0] = min(out[z - z0], (next - z) * (next - z));
    }
}

// y pass: in [X][Y][Tz] -> out [X][Ty][Tz], lanes along z
__global__ __launch_bounds__(256) void mc_edt_y_kernel(DevGrid G, const int *__restrict__ in_a, int *__restrict__ out_b, MuBox T) {
    const int Ty = T.hi[1] - T.lo[1] + 1, Tz = T.hi[2] - T.lo[2] + 1;
    const long long n = (long long)G.X * Ty * Tz;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long long)gridDim.x * blockDim.x) {
        const int tz = (int)(t % Tz);
        const long long xy = t / Tz;
        const int ty = (int)(xy % Ty), x = (int)(xy / Ty);
        out_b[t] = mc_line_min(in_a + (size_t)x * G.Y * Tz + tz, G.Y, Tz, T.lo[1] + ty);
    }
}

// x pass over the box and the conversion: in [X][Ty][Tz] -> the ESDF's voxels of the box
__global__ __launch_bounds__(256) void mc_edt_x_kernel(DevGrid G, const int *__restrict__ in_b, float *__restrict__ esdf, MuBox T, McEsdfRecord *__restrict__ rec) {
    const int Tx = T.hi[0] - T.lo[0] + 1, Ty = T.hi[1] - T.lo[1] + 1, Tz = T.hi[2] - T.lo[2] + 1;
    const long long n = (long long)Tx * Ty * Tz;
    unsigned long long mine = 0;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long long)gridDim.x * blockDim.x) {
        const int tz = (int)(t % Tz);
        const long long xy = t / Tz;
        const int ty = (int)(xy % Ty), tx = (int)(xy / Ty);
        const int d2 = mc_line_min(in_b + (size_t)ty * Tz + tz, G.X, (long long)Ty * Tz, T.lo[0] + tx);
        const float nv = mc_esdf_value(G.res, d2);
        const size_t a = ((size_t)(T.lo[0] + tx) * G.Y + T.lo[1] + ty) * G.Z + T.lo[2] + tz;
        if (__float_as_uint(esdf[a]) != __float_as_uint(nv)) { esdf[a] = nv; mine++; }
    }
    if (mine) atomicAdd(&rec->raised, mine);
}

}  // namespace isdf

using namespace isdf;

extern "C" void isdf_map_clear_params_default(isdf_map_clear_params *p) {
    if (!p) return;
    p->max_cleared_voxels = 65536;
    p->full_fraction = 0.5;
    p->refresh_esdf = 1;
    p->refresh_frontend = 1;
}

extern "C" void isdf_map_clear_sizes(int sizes_out[2]) {
    if (!sizes_out) return;
    sizes_out[0] = (int)sizeof(isdf_map_clear_params); sizes_out[1] = (int)sizeof(isdf_map_clear_info);
}

namespace {

void empty_boxes(isdf_map_clear_info &info) {
    for (int a = 0; a < 3; a++) { info.dirty_lo[a] = info.touched_lo[a] = 0; info.dirty_hi[a] = info.touched_hi[a] = -1; }
}

}  // namespace

// everything after the hand-over of a call that freed at least one voxel
int isdf::mc_refresh_products(isdf_ctx *c, MapUpdateState &S, const isdf_map_clear_params &P, const MapListRecord &R, unsigned cap, bool voxels, isdf_map_clear_info &info,
                              const MuBox *field_more) {
    const hipStream_t st = c->stream;
    const DevGrid &G = c->grid;
    const int dims[3] = {G.X, G.Y, G.Z};
    const size_t n_vox = (size_t)G.X * G.Y * G.Z;
    int rc;
    // The cost-to-go field: dropped (mode 0 of isdf_frontend_field_set_reopen; the repair's rule is not proved for opened bits), or
    // lowered in place once the configuration space is the new map's (mode 1).  It is invalid from here until the reopen has gone
    // through: every error path leaves it dropped.
    const bool reopen = P.refresh_frontend != 0 && isdf_field_change_wanted(c, FfChange::Opening);
    const MapRefresh M = map_refresh_begin(c, R, cap, voxels, P.refresh_esdf, P.refresh_frontend, P.full_fraction, &info.field_dropped);
    if (!reopen) (void)isdf_field_gate_drop(c);          // (a gated field that does not follow: its gate and its follow report go with it)
    for (int a = 0; a < 3; a++) { info.dirty_lo[a] = M.box.lo[a]; info.dirty_hi[a] = M.box.hi[a]; }
    bool full = M.over;

    // ---- ESDF
    McEsdfRecord *const d_er = &S.rec.dev()->esdf;
    const McEsdfRecord *const h_er = &S.rec.host().esdf;
    HIPCHK(c, hipEventRecord(S.ev[2], st));
    if (M.do_esdf) {
        MuBox T{{0, 0, 0}, {-1, -1, -1}};
        if (!full) {
            // part one: the touched voxels.  Their box sizes the slabs and decides the path: the second hand-over of the call.
            hipLaunchKernelGGL(mc_touched_kernel, dim3((unsigned)((n_vox + 255) / 256)), dim3(256), 0, st, G, (const float *)c->d_esdf.get(), (const uint8_t *)c->d_occ.get(),
                               (const MuVoxel *)S.d_list.get(), (int)R.n, M.box, d_er);
            HIPCHK(c, hipGetLastError());
            if ((rc = map_hand_over(c, S, nullptr, "map clear", voxels))) return rc;
            for (int a = 0; a < 3; a++) { T.lo[a] = h_er->lo[a]; T.hi[a] = h_er->hi[a]; }
            if (!mu_box_empty(T))
                for (int a = 0; a < 3; a++)
                    if (T.lo[a] < 0 || T.hi[a] >= dims[a]) return isdf_fail(c, ISDF_ERR_HIP, "map clear: inconsistent hand-over record");
            full = !h_er->any_occ || (double)mu_box_voxels(T) > P.full_fraction * (double)n_vox;
        }
        if (full) { if ((rc = isdf_generate_esdf(c))) return rc; info.esdf_voxels_recomputed = (long long)n_vox; }
        else if (!mu_box_empty(T)) {
            const int Tx = T.hi[0] - T.lo[0] + 1, Ty = T.hi[1] - T.lo[1] + 1, Tz = T.hi[2] - T.lo[2] + 1;
            const size_t na = (size_t)G.X * G.Y * Tz, nb = (size_t)G.X * Ty * Tz, nc = (size_t)Tx * Ty * Tz;
            if ((rc = S.d_edt_a.reserve(c, na)) || (rc = S.d_edt_b.reserve(c, nb))) return rc;
            hipLaunchKernelGGL(mc_edt_z_kernel, dim3((unsigned)(((size_t)G.X * G.Y + 255) / 256)), dim3(256), 0, st, G, (const uint8_t *)c->d_occ.get(), T.lo[2], T.hi[2], S.d_edt_a.get());
            hipLaunchKernelGGL(mc_edt_y_kernel, dim3((unsigned)std::min<size_t>((nb + 255) / 256, 8192)), dim3(256), 0, st, G, (const int *)S.d_edt_a.get(), S.d_edt_b.get(), T);
            hipLaunchKernelGGL(mc_edt_x_kernel, dim3((unsigned)std::min<size_t>((nc + 255) / 256, 8192)), dim3(256), 0, st, G, (const int *)S.d_edt_b.get(), c->d_esdf.get(), T, d_er);
            HIPCHK(c, hipGetLastError());
            for (int a = 0; a < 3; a++) { info.touched_lo[a] = T.lo[a]; info.touched_hi[a] = T.hi[a]; }
            info.esdf_voxels_recomputed = mu_box_voxels(T);
        }
        c->bricks_stale = true;
        info.esdf_refreshed = 1;
    }
    info.path = full ? 2 : 1;
    HIPCHK(c, hipEventRecord(S.ev[3], st));

    // ---- front end, the field's reopen around the synchronisation
    MapFrontend F;
    if ((rc = map_frontend_stage(c, S, FfChange::Opening, reopen, P.refresh_frontend != 0, full, M, F, &info.field_dropped, field_more))) return rc;
    map_frontend_report(F, info);
    if (M.do_esdf && !full) info.esdf_voxels_raised = (long long)h_er->raised;
    info.esdf_ms = S.ev.ms(2, 3);
    return map_watch_recheck(c, traj_watch_armed(c), &info.watch_rechecked);
}

namespace {

// the clear proper; `in` is the host array of the points (voxels == false) or of the checked voxel indices
int map_clear(isdf_ctx *c, const void *in, long long n_in, bool voxels, const isdf_map_clear_params *params, isdf_map_clear_info *info_out) {
    isdf_map_clear_params P;
    isdf_map_clear_params_default(&P);
    if (params) P = *params;
    if (P.max_cleared_voxels < 0 || !(P.full_fraction >= 0.0)) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "bad map clear parameters");
    isdf_map_clear_info info{};
    empty_boxes(info);
    info.n_points = n_in;
    info.field_dropped = c->gate_dropped ? 1 : 0;      // (a gated field went in map_change_ready, whatever this frame changes)
    MapUpdateState *Sp;
    int rc = map_begin(c, &Sp);
    if (rc) return rc;
    MapUpdateState &S = *Sp;
    const hipStream_t st = c->stream;
    const DevGrid &G = c->grid;

    // ---- count down, find the cleared voxels: one hand-over
    const unsigned cap = map_list_cap(P.max_cleared_voxels, (unsigned long long)n_in, (unsigned long long)G.X * G.Y * G.Z);
    if ((rc = map_stage(c, S, in, (size_t)n_in * 3 * (voxels ? sizeof(int) : sizeof(float)), nullptr, 0, std::max<size_t>(cap, 1), S.ev[0]))) return rc;
    if (n_in > 0) {
        const unsigned blocks = (unsigned)std::min<long long>((n_in + 255) / 256, 2048);
        MapListRecord *const d_rec = &S.rec.dev()->list;
        if (voxels) hipLaunchKernelGGL(mc_mark_kernel<true>, dim3(blocks), dim3(256), 0, st, (const void *)S.d_in.get(), n_in, G, (unsigned *)nullptr, 0u, c->d_occ.get(),
                                       S.d_list.get(), cap, d_rec);
        else hipLaunchKernelGGL(mc_mark_kernel<false>, dim3(blocks), dim3(256), 0, st, (const void *)S.d_in.get(), n_in, G, c->d_counts.get(), (unsigned)c->counts_thr,
                                c->d_occ.get(), S.d_list.get(), cap, d_rec);
        HIPCHK(c, hipGetLastError());
    }
    if ((rc = map_hand_over(c, S, S.ev[1], "map clear", voxels))) return rc;           // the kernel may have run: the occupancy may have moved
    const MapListRecord R = S.rec.host().list;
    info.count_ms = S.ev.ms(0, 1);
    info.n_cleared_voxels = R.n;
    info.n_points_ignored = (long long)R.tally;
    if (R.n > 0) {                      // (nothing but the counts changed: every product stays in place, the field and the watch included)
        // from here on the occupancy has moved: a failure must not leave products behind that describe the old map
        rc = mc_refresh_products(c, S, P, R, cap, voxels, info);
        if (rc != ISDF_OK) { mu_drop_derived(c, voxels); return rc; }
    }
    if (info_out) *info_out = info;
    return ISDF_OK;
}

bool host_args_bad(const int32_t dims[3], double res, const int32_t *ijk, long long n) {
    if (!dims || !(res > 0.0) || n < 0 || (n > 0 && !ijk)) return true;
    for (int a = 0; a < 3; a++) if (dims[a] < 1 || dims[a] > 4096) return true;
    for (long long i = 0; i < 3 * n; i++) if (ijk[i] < 0 || ijk[i] >= dims[i % 3]) return true;
    return false;
}

}  // namespace

extern "C" int isdf_clear_pointcloud(isdf_ctx *c, const float *xyz, long long n_points, const isdf_map_clear_params *params, isdf_map_clear_info *info_out) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    const int rc = map_change_ready(c, "clearing the map", xyz, n_points, true);
    return rc ? rc : map_clear(c, xyz, n_points, false, params, info_out);
}

extern "C" int isdf_clear_voxels(isdf_ctx *c, const int32_t *ijk, long long n_voxels, const isdf_map_clear_params *params, isdf_map_clear_info *info_out) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    int rc = map_change_ready(c, "clearing the map", ijk, n_voxels, false);
    if (!rc) rc = map_voxels_in_grid(c, ijk, n_voxels);
    return rc ? rc : map_clear(c, ijk, n_voxels, true, params, info_out);
}

extern "C" long long isdf_clear_touched_host(const float *esdf_old, const int32_t dims[3], double resolution, const int32_t *cleared_ijk, long long n_cleared,
                                             uint8_t *touched_out) {
    if (!esdf_old || host_args_bad(dims, resolution, cleared_ijk, n_cleared)) return isdf_fail(nullptr, ISDF_ERR_INVALID_ARG, "clear (host form): bad arguments");
    McRaise R;
    mc_touched_host(esdf_old, dims, resolution, cleared_ijk, n_cleared, touched_out, R);
    return R.n_touched;
}

extern "C" int isdf_clear_esdf_host(const uint8_t *occ_new, float *esdf_inout, const int32_t dims[3], double resolution, const int32_t *cleared_ijk,
                                    long long n_cleared, isdf_map_clear_info *info_out) {
    if (!occ_new || !esdf_inout || host_args_bad(dims, resolution, cleared_ijk, n_cleared)) return isdf_fail(nullptr, ISDF_ERR_INVALID_ARG, "clear (host form): bad arguments");
    McRaise R;
    mc_esdf_raise_host(occ_new, esdf_inout, dims, resolution, cleared_ijk, n_cleared, R);
    if (info_out) {
        isdf_map_clear_info info{};
        empty_boxes(info);
        info.n_points = info.n_cleared_voxels = n_cleared;
        info.path = n_cleared == 0 ? 0 : (R.none_left ? 2 : 1);
        if (n_cleared > 0) for (int a = 0; a < 3; a++) { info.dirty_lo[a] = R.dirty.lo[a]; info.dirty_hi[a] = R.dirty.hi[a]; }
        if (!R.none_left && !mu_box_empty(R.touched)) for (int a = 0; a < 3; a++) { info.touched_lo[a] = R.touched.lo[a]; info.touched_hi[a] = R.touched.hi[a]; }
        info.esdf_refreshed = n_cleared > 0 ? 1 : 0;
        info.esdf_voxels_recomputed = R.recomputed; info.esdf_voxels_raised = R.raised;
        *info_out = info;
    }
    return ISDF_OK;
}
