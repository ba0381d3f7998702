// A range scan integrated into the map: isdf_integrate_scan, the producer of map_clear.hip's and map_update.hip's inputs.
//   ms_trace_kernel  one ray per lane, grid-stride: the integer walk of map_scan_host.hpp from the sensor's tick to the end point's.
//                    Every visited voxel sets its bit in the free-bit grid, the end voxel of a hit ray its bit in the hit-bit grid
//                    instead.  The rays of one scan share their first voxels: a lane reads the word and leaves the atomic OR out when
//                    the bit is set already (bits only go from 0 to 1 during the kernel, so a stale read costs an OR, never a bit).
//                    The visited box - every walk stays in the box of its two ends - the skipped rays and the hit rays are reduced per
//                    workgroup in LDS and then into the call's record.
//   ms_apply_kernel  over the visited box, which it reads from that record: one lane per dword of a column's bits.  F = free bit set and
//                    hit bit clear: the count goes down by miss_weight and not below 0, and the voxel whose count leaves
//                    [thr, inf) is freed, listed and boxed (map_list_append) exactly as mc_mark_kernel's crossing lane does it -
//                    `ignored` counts what miss_weight single removals would have found at 0.  One lane owns a voxel: no atomics on the
//                    counts.  Also |F| and the distinct voxels of H.
//   ms_hits_kernel   one lane per ray again, after the clear's products are in place: the end voxel of a hit ray counts up by one,
//                    mu_mark_kernel's crossing test, into the list record again.
// Then map_clear.hip's and map_update.hip's own refresh stages, in that order: the call IS isdf_clear_pointcloud of miss_weight
// centres of every voxel of F followed by isdf_update_pointcloud of the hit end points, and reports what those two calls report.
#include "map_query.hpp"
#include "map_change.hpp"
#include "swept_field.hpp"
#include <algorithm>
#include <cstring>
#include <vector>

namespace isdf {

__device__ __forceinline__ bool ms_end_tick(const MapGeom &M, const float *__restrict__ xyz, long long i, int q[3]) {
    return ms_quantize(M, (double)xyz[3 * i], (double)xyz[3 * i + 1], (double)xyz[3 * i + 2], q);
}

__device__ __forceinline__ void ms_set_bit(unsigned *bits, size_t a) {
    unsigned *const w = bits + (a >> 5);
    const unsigned b = 1u << (unsigned)(a & 31);
    if (!(*w & b)) atomicOr(w, b);
}

__global__ __launch_bounds__(256) void ms_trace_kernel(const float *__restrict__ xyz, const uint8_t *__restrict__ hit, long long n, MapGeom M, MsOrigin O,
                                                       unsigned *free_bits, unsigned *hit_bits, MsRecord *__restrict__ rec) {
    __shared__ int s_lo[3], s_hi[3];
    __shared__ unsigned s_skipped, s_hits;
    if (threadIdx.x < 3) { s_lo[threadIdx.x] = 0x7FFFFFFF; s_hi[threadIdx.x] = -1; }
    if (threadIdx.x == 0) { s_skipped = 0u; s_hits = 0u; }
    __syncthreads();
    int lo[3] = {0x7FFFFFFF, 0x7FFFFFFF, 0x7FFFFFFF}, hi[3] = {-1, -1, -1};
    unsigned skipped = 0, hits = 0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        int qe[3];
        if (!ms_end_tick(M, xyz, i, qe)) { skipped++; continue; }
        const bool is_hit = !hit || hit[i] != 0;
        MsRay r;
        ms_ray_begin(O.q, qe, r);
        for (int a = 0; a < 3; a++) {
            const int ve = qe[a] >> MS_TICKS_LOG2;
            lo[a] = min(lo[a], min(r.v[a], ve));
            hi[a] = max(hi[a], max(r.v[a], ve));
        }
        for (;;) {
            const size_t a = map_voxel(M, r.v);           // inside the grid: the walk stays between two voxels of it
            const bool last = ms_ray_done(r);
            if (last && is_hit) { ms_set_bit(hit_bits, a); hits++; }
            else ms_set_bit(free_bits, a);
            if (last) break;
            ms_ray_step(r);
        }
    }
    if (hi[0] >= 0) {
        atomicMin(&s_lo[0], lo[0]); atomicMin(&s_lo[1], lo[1]); atomicMin(&s_lo[2], lo[2]);
        atomicMax(&s_hi[0], hi[0]); atomicMax(&s_hi[1], hi[1]); atomicMax(&s_hi[2], hi[2]);
    }
    if (skipped) atomicAdd(&s_skipped, skipped);
    if (hits) atomicAdd(&s_hits, hits);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_hi[0] >= 0) {
            atomicMin(&rec->lo[0], s_lo[0]); atomicMin(&rec->lo[1], s_lo[1]); atomicMin(&rec->lo[2], s_lo[2]);
            atomicMax(&rec->hi[0], s_hi[0]); atomicMax(&rec->hi[1], s_hi[1]); atomicMax(&rec->hi[2], s_hi[2]);
        }
        if (s_skipped) atomicAdd(&rec->n_skipped, (unsigned long long)s_skipped);
        if (s_hits) atomicAdd(&rec->n_hits, (unsigned long long)s_hits);
    }
}

__global__ __launch_bounds__(256) void ms_apply_kernel(DevGrid G, const unsigned *__restrict__ free_bits, const unsigned *__restrict__ hit_bits,
                                                       unsigned *__restrict__ counts, unsigned thr, unsigned miss, uint8_t *__restrict__ occ,
                                                       MuVoxel *__restrict__ list, unsigned cap, MsRecord *__restrict__ srec, MapListRecord *__restrict__ rec) {
    const int lo0 = srec->lo[0], lo1 = srec->lo[1], lo2 = srec->lo[2], hi0 = srec->hi[0], hi1 = srec->hi[1], hi2 = srec->hi[2];
    if (hi0 < lo0 || hi1 < lo1 || hi2 < lo2) return;            // no ray was traced
    const int e1 = hi1 - lo1 + 1;
    const int wz = ((hi2 - lo2 + 32) >> 5) + 1;                 // dwords that the z range of one column can touch, at any alignment
    const long long n = (long long)(hi0 - lo0 + 1) * e1 * wz;
    unsigned long long n_free = 0, n_hitv = 0, ignored = 0;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long long)gridDim.x * blockDim.x) {
        const int k = (int)(t % wz);
        const long long xy = t / wz;
        const int y = lo1 + (int)(xy % e1), x = lo0 + (int)(xy / e1);
        const size_t base = ((size_t)x * G.Y + y) * G.Z;
        const size_t a0 = base + lo2, a1 = base + hi2;
        const size_t w = (a0 >> 5) + k;
        if (w > (a1 >> 5)) continue;
        const size_t first = max(a0, w << 5), last = min(a1, (w << 5) + 31);             // this column's own bits of the dword
        const unsigned mask = (0xFFFFFFFFu << (unsigned)(first & 31)) & (0xFFFFFFFFu >> (31u - (unsigned)(last & 31)));
        const unsigned hb = hit_bits[w] & mask;
        unsigned fb = free_bits[w] & mask & ~hb;
        n_hitv += __popc(hb);
        n_free += __popc(fb);
        if (miss == 0u) continue;
        while (fb) {
            const int b = __ffs(fb) - 1;
            fb &= fb - 1;
            const size_t a = (w << 5) + b;
            const unsigned was = counts[a];
            const unsigned now = was > miss ? was - miss : 0u;
            ignored += miss - (was - now);
            if (now != was) counts[a] = now;
            if (thr >= 1u && was >= thr && now < thr) {         // thr == 0: every voxel stays occupied
                occ[a] = 0;
                map_list_append(rec, list, cap, x, y, (int)(a - base));
            }
        }
    }
    if (n_free) atomicAdd(&srec->n_free, n_free);
    if (n_hitv) atomicAdd(&srec->n_hit_voxels, n_hitv);
    if (ignored) atomicAdd(&rec->tally, ignored);
}

__global__ __launch_bounds__(256) void ms_hits_kernel(const float *__restrict__ xyz, const uint8_t *__restrict__ hit, long long n, MapGeom M,
                                                      unsigned *__restrict__ counts, unsigned thr, uint8_t *__restrict__ occ, const float *__restrict__ esdf,
                                                      MuVoxel *__restrict__ list, unsigned cap, MapListRecord *__restrict__ rec) {
    if (esdf && blockIdx.x == 0 && threadIdx.x == 0) rec->esdf0 = __float_as_uint(esdf[0]);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        int qe[3];
        if ((hit && hit[i] == 0) || !ms_end_tick(M, xyz, i, qe)) continue;
        const int v[3] = {qe[0] >> MS_TICKS_LOG2, qe[1] >> MS_TICKS_LOG2, qe[2] >> MS_TICKS_LOG2};
        const size_t a = map_voxel(M, v);
        const unsigned old = atomicAdd(&counts[a], 1u);
        if (thr >= 1u && old + 1u == thr) {                     // mu_mark_kernel's crossing: exactly one add sees it
            occ[a] = 1;
            map_list_append(rec, list, cap, v[0], v[1], v[2]);
        }
    }
}

}  // namespace isdf

using namespace isdf;

extern "C" void isdf_map_scan_params_default(isdf_map_scan_params *p) {
    if (!p) return;
    p->miss_weight = 1;
    p->reserved = 0;
    isdf_map_clear_params_default(&p->clear);
    isdf_map_update_params_default(&p->update);
}

extern "C" void isdf_map_scan_sizes(int sizes_out[2]) {
    if (!sizes_out) return;
    sizes_out[0] = (int)sizeof(isdf_map_scan_params); sizes_out[1] = (int)sizeof(isdf_map_scan_info);
}

namespace {

void empty_info(isdf_map_scan_info &info) {
    for (int a = 0; a < 3; a++) {
        info.ray_lo[a] = info.clear.dirty_lo[a] = info.clear.touched_lo[a] = info.update.dirty_lo[a] = 0;
        info.ray_hi[a] = info.clear.dirty_hi[a] = info.clear.touched_hi[a] = info.update.dirty_hi[a] = -1;
    }
}

}  // namespace

// The stages behind the staging.  `in` names where the rays come from: the caller's arrays, uploaded by map_stage, or - in.produce - a
// step that writes them on the ctx's stream straight into the staged buffers (depth_cam.hip: the unprojection of a depth image).
int isdf::scan_integrate(isdf_ctx *c, const MsOrigin &O, const MsInput &in, long long n_rays, const isdf_map_scan_params &P, isdf_map_scan_info *info_out) {
    const float *const xyz = in.xyz;
    const uint8_t *const hit = in.hit;
    const bool has_hit = hit || in.produce;
    isdf_map_scan_info info{};
    empty_info(info);
    info.n_rays = n_rays;
    info.clear.field_dropped = info.update.field_dropped = c->gate_dropped ? 1 : 0;       // (a gated field went in map_change_ready, whatever the rays change)
    // ... unless it follows the change: one opening stage once K has grown and the clear's table refresh is done, over the
    // clear's grown box and the rays' box grown by the gate's radius - where E can have grown -, then the update's closing stage
    const bool follow = isdf_field_follow_wanted(c);
    MapUpdateState *Sp;
    int rc = map_begin(c, &Sp);
    if (rc) return rc;
    MapUpdateState &S = *Sp;
    const hipStream_t st = c->stream;
    const DevGrid &G = c->grid;
    const MapGeom M = map_geom(G);
    const unsigned long long n_vox = (unsigned long long)G.X * G.Y * G.Z;
    const size_t n_words = (size_t)((n_vox + 31) / 32);
    const unsigned thr = (unsigned)c->counts_thr, miss = (unsigned)P.miss_weight;

    // ---- scratch: nothing below allocates after the first call of a size.  The lists' capacities as the two calls would choose them,
    // with the number of voxels the rays can visit in place of the number of points (which is known only after the trace).
    const unsigned long long reach = (unsigned long long)n_rays >= n_vox ? n_vox : std::min<unsigned long long>(n_vox, (unsigned long long)n_rays * (unsigned)(G.X + G.Y + G.Z));
    const unsigned cap_clear = map_list_cap(P.clear.max_cleared_voxels, reach, n_vox);
    const unsigned cap_update_most = map_list_cap(P.update.max_new_voxels, (unsigned long long)n_rays, n_vox);
    const size_t xyz_bytes = (size_t)n_rays * 3 * sizeof(float);
    if ((rc = S.d_free_bits.reserve(c, n_words)) || (rc = S.d_hit_bits.reserve(c, n_words))) return rc;
    if (n_rays > 0) {
        HIPCHK(c, hipMemsetAsync(S.d_free_bits, 0, n_words * sizeof(unsigned), st));
        HIPCHK(c, hipMemsetAsync(S.d_hit_bits, 0, n_words * sizeof(unsigned), st));
    }
    if ((rc = map_stage(c, S, xyz, xyz_bytes, hit, has_hit ? (size_t)n_rays : 0, std::max<size_t>({cap_clear, cap_update_most, 1u}), S.ev_scan[0]))) return rc;
    const float *const d_xyz = (const float *)S.d_in.get();
    const uint8_t *const d_hit = has_hit ? (const uint8_t *)S.d_in.get() + xyz_bytes : nullptr;
    if (in.produce && (rc = in.produce(c, (float *)S.d_in.get(), (uint8_t *)S.d_in.get() + xyz_bytes, in.arg))) return rc;          // nothing of the map has moved yet
    MapRecords *const d_rec = S.rec.dev(), *const h_rec = &S.rec.host();
    const unsigned ray_blocks = (unsigned)std::min<long long>((n_rays + 255) / 256, 2048);

    // ---- the rays, then the frees: one hand-over
    if (n_rays > 0) {
        hipLaunchKernelGGL(ms_trace_kernel, dim3(ray_blocks), dim3(256), 0, st, d_xyz, d_hit, n_rays, M, O, S.d_free_bits.get(), S.d_hit_bits.get(), &d_rec->scan);
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipEventRecord(S.ev_scan[1], st));
    const bool known = c->known.have && n_rays > 0;         // the visited voxels join the known grid (map_known.hip); off: nothing differs
    // from the merge's launch on K may have moved: a failure before the hand-over (which drops every product itself) takes a field
    // that follows along - it is never left valid over a K it does not describe
    rc = [&]() -> int {
        if (known) ISDF_TRY(map_known_merge_launch(c, S.d_free_bits.get(), S.d_hit_bits.get(), &d_rec->scan));
        HIPCHK(c, hipEventRecord(S.ev[0], st));
        if (n_rays > 0) {
            hipLaunchKernelGGL(ms_apply_kernel, dim3(1024), dim3(256), 0, st, G, (const unsigned *)S.d_free_bits.get(), (const unsigned *)S.d_hit_bits.get(), c->d_counts.get(),
                               thr, miss, c->d_occ.get(), S.d_list.get(), cap_clear, &d_rec->scan, &d_rec->list);
            HIPCHK(c, hipGetLastError());
        }
        return ISDF_OK;
    }();
    if (rc != ISDF_OK) {
        if (follow) (void)isdf_field_gate_drop(c);
        return rc;
    }
    if ((rc = map_hand_over(c, S, S.ev[1], "scan", false))) return rc;
    const MapListRecord R = h_rec->list;
    const MsRecord RS = h_rec->scan;
    if (known) map_known_merged(c, RS);
    info.trace_ms = S.ev_scan.ms(0, 1);
    info.n_rays_skipped = (long long)RS.n_skipped;
    info.n_hits = (long long)RS.n_hits;
    info.n_free_voxels = (long long)RS.n_free;
    info.n_hit_voxels = (long long)RS.n_hit_voxels;
    if (RS.hi[0] >= RS.lo[0]) for (int a = 0; a < 3; a++) { info.ray_lo[a] = RS.lo[a]; info.ray_hi[a] = RS.hi[a]; }
    const unsigned long long n_clear_points = (unsigned long long)miss * RS.n_free;          // what isdf_clear_pointcloud would have been given
    info.clear.n_points = (long long)n_clear_points;
    info.clear.count_ms = S.ev.ms(0, 1);
    info.clear.n_cleared_voxels = R.n;
    info.clear.n_points_ignored = (long long)R.tally;
    const bool k_grew = follow && known && RS.newly_known > 0;
    MuBox kbox{{0, 0, 0}, {-1, -1, -1}};
    if (k_grew) {
        const int dims[3] = {G.X, G.Y, G.Z};
        MuBox rays;
        for (int a = 0; a < 3; a++) { rays.lo[a] = RS.lo[a]; rays.hi[a] = RS.hi[a]; }
        kbox = mu_box_grow(rays, c->fe.field_gate_radius, dims);
    }
    bool k_open = false;                // the opening stage on its own: K grew, no voxel was cleared
    if (R.n > 0) {
        // from here on the occupancy has moved: a failure must not leave products behind that describe the old map
        rc = mc_refresh_products(c, S, P.clear, R, map_list_cap(P.clear.max_cleared_voxels, n_clear_points, n_vox), false, info.clear, k_grew ? &kbox : nullptr);
        if (rc != ISDF_OK) { mu_drop_derived(c, false); return rc; }
    } else if (k_grew) {
        // K has moved: the field is invalid until the stage has gone through.  Its mark is queued here and the hits' hand-over below is its
        // synchronisation: no hand-over is added.  The mark reads the table, which the hits stage does not touch.
        c->fe.field_valid = false; c->fe.field_reachable = false;
        if (P.clear.refresh_frontend == 0) (void)isdf_field_gate_drop(c);
        else {
            k_open = true;
            rc = isdf_field_change_begin(c, FfChange::Opening, kbox.lo, kbox.hi, S.ev[6]);
            if (rc != ISDF_OK) { mu_drop_derived(c, false); return rc; }
        }
    }

    // ---- the hits, on the map the clear left: the list record empty again, second hand-over
    info.update.n_points = info.n_hits;
    const unsigned cap_update = map_list_cap(P.update.max_new_voxels, RS.n_hits, n_vox);
    h_rec->list = map_records_empty().list;
    {
        hipError_t e = hipMemcpyAsync(&d_rec->list, &h_rec->list, sizeof(MapListRecord), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipEventRecord(S.ev[0], st);
        if (e == hipSuccess && RS.n_hits > 0) {
            hipLaunchKernelGGL(ms_hits_kernel, dim3(ray_blocks), dim3(256), 0, st, d_xyz, d_hit, n_rays, M, c->d_counts.get(), thr, c->d_occ.get(),
                               (const float *)c->d_esdf.get(), S.d_list.get(), cap_update, &d_rec->list);
            e = hipGetLastError();
        }
        if (e != hipSuccess) {
            c->err = std::string("scan hits: ") + hipGetErrorString(e);
            mu_drop_derived(c, false);
            return ISDF_ERR_HIP;
        }
    }
    if ((rc = map_hand_over(c, S, S.ev[1], "scan", false))) return rc;
    const MapListRecord RU = h_rec->list;
    if (k_open) {
        int kept = 0;
        rc = isdf_field_change_end(c, FfChange::Opening, kbox.lo, kbox.hi, S.ev[6], S.ev[7], &kept);
        if (rc != ISDF_OK) { mu_drop_derived(c, false); return rc; }
        if (!kept) (void)isdf_field_gate_drop(c);
    }
    if (follow && !c->fe.field_valid) {                     // the opening stage lost the field: every stage after it says so
        c->gate_dropped = true;
        info.clear.field_dropped = info.update.field_dropped = 1;
    }
    info.update.count_ms = S.ev.ms(0, 1);
    info.update.n_new_voxels = RU.n;
    if (RU.n > 0) {
        rc = mu_refresh_products(c, S, P.update, RU, cap_update, false, info.update);
        if (rc != ISDF_OK) { mu_drop_derived(c, false); return rc; }
    }
    if (info_out) *info_out = info;
    return ISDF_OK;
}

// what every entry to the scan checks before anything moves: the ctx (`in`: the caller's rays or image), the parameters, the origin
int isdf::scan_check(isdf_ctx *c, const char *op, const double origin[3], const void *in, long long n, const isdf_map_scan_params *params, isdf_map_scan_params &P, MsOrigin &O) {
    ISDF_TRY(map_change_ready(c, op, in, n, true));
    isdf_map_scan_params_default(&P);
    if (params) P = *params;
    if (P.miss_weight < 0 || P.clear.max_cleared_voxels < 0 || !(P.clear.full_fraction >= 0.0) || P.update.max_new_voxels < 0 || !(P.update.full_fraction >= 0.0))
        return isdf_fail(c, ISDF_ERR_INVALID_ARG, "bad scan parameters");
    if (!ms_quantize(map_geom(c->grid), origin[0], origin[1], origin[2], O.q)) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "the scan's origin lies outside the map");
    return ISDF_OK;
}

extern "C" int isdf_integrate_scan(isdf_ctx *c, const double origin[3], const float *xyz, const uint8_t *hit, long long n_rays, const isdf_map_scan_params *params,
                                   isdf_map_scan_info *info_out) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    if (!origin) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "integrating a scan: null origin");
    isdf_map_scan_params P;
    MsOrigin O;
    if (int rc = scan_check(c, "integrating a scan", origin, xyz, n_rays, params, P, O)) return rc;
    return scan_integrate(c, O, MsInput{xyz, hit, nullptr, nullptr}, n_rays, P, info_out);
}

extern "C" long long isdf_scan_sets_host(const double bmin[3], const double bmax[3], double resolution, const int32_t dims[3], const double origin[3], const float *xyz,
                                         const uint8_t *hit, long long n_rays, uint8_t *free_out, uint32_t *hits_out, long long *n_skipped_out) {
    if (ms_geometry_bad(bmin, bmax, resolution, dims) || !origin || n_rays < 0 || (n_rays > 0 && !xyz)) return isdf_fail(nullptr, ISDF_ERR_INVALID_ARG, "scan (host form): bad arguments");
    std::vector<uint8_t> free_set;
    std::vector<uint32_t> hits;
    MsSets S;
    if (!ms_sets_host(map_geom(bmin, bmax, resolution, dims), origin, xyz, hit, n_rays, free_set, hits, S)) return isdf_fail(nullptr, ISDF_ERR_INVALID_ARG, "scan (host form): the origin lies outside the map");
    if (free_out) std::memcpy(free_out, free_set.data(), free_set.size());
    if (hits_out) std::memcpy(hits_out, hits.data(), hits.size() * sizeof(uint32_t));
    if (n_skipped_out) *n_skipped_out = S.n_skipped;
    return S.n_free;
}

extern "C" long long isdf_scan_ray_host(const double bmin[3], const double bmax[3], double resolution, const int32_t dims[3], const double origin[3], const float end[3],
                                        int32_t *ijk_out, long long capacity) {
    if (ms_geometry_bad(bmin, bmax, resolution, dims) || !origin || !end || capacity < 0 || (capacity > 0 && !ijk_out)) return isdf_fail(nullptr, ISDF_ERR_INVALID_ARG, "scan (host form): bad arguments");
    const long long n = ms_ray_host(map_geom(bmin, bmax, resolution, dims), origin, end, ijk_out, capacity);
    return n < 0 ? isdf_fail(nullptr, ISDF_ERR_INVALID_ARG, "scan (host form): the origin lies outside the map") : n;
}
