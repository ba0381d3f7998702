// The map updated in place from new sensor points: isdf_update_pointcloud / isdf_update_voxels.
//   mu_mark_kernel          one lane per new point (or listed voxel): the kept count goes up by one, and the ONE lane whose add carries
//                           a count across the threshold (old + 1 == thr: whatever the order of the adds, exactly one add sees it)
//                           sets the voxel occupied, appends it to the new-voxel list and widens the dirty box.  The voxel form
//                           exchanges the occupancy byte 0 -> 1 instead (a 32-bit atomic OR on the dword that holds it).
//   mu_esdf_kernel          one lane per voxel of the map: new = min(old, float(res * sqrt(d2 to the nearest NEW voxel))).  The
//                           conversion is monotone, so the min on floats is the float of the min integer and no d2 grid is kept.  A
//                           voxel whose distance to the dirty box cannot beat its old value is left alone (mu_esdf_skip); a workgroup
//                           whose 256 voxels all skip leaves at once; the others scan the list, staged through LDS in chunks.
//   mu_map_bits_box_kernel  the dwords of the front end's inflated bit map that cover the dirty box (fe_map_bits_word);
//   mu_cspace_box_kernel    the configuration-space words of the dirty box grown by (k - 1) / 2 (fe_cspace_voxel, the whole-map
//                           kernel's body: one wavefront = 64 consecutive z of one column of the box);
//   mu_pack_box_kernel      that box of the table packed for ONE copy to the host, which scatters it into the A*'s copy.
// Every consumer of the new-voxel list takes a minimum over it: its order, which the atomics leave undefined, never shows.
// Integer work throughout except the one res * sqrt(d2) of the ESDF, a single multiplication (nothing to contract).
#include "isdf_ctx.hpp"
#include "frontend_dev.hpp"
#include "grid_index.hpp"
#include "map_update_host.hpp"
#include "map_update_state.hpp"
#include "swept_field.hpp"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>

namespace isdf {

void launch_threshold_counts(const unsigned *counts, size_t n, unsigned thr, uint8_t *occ, hipStream_t stream);     // map_build.hip

template <bool VOXELS>
__global__ __launch_bounds__(256) void mu_mark_kernel(const void *__restrict__ in, long long n, DevGrid G, unsigned *__restrict__ counts, unsigned thr,
                                                      uint8_t *__restrict__ occ, const float *__restrict__ esdf, MuVoxel *__restrict__ list, unsigned cap,
                                                      MuRecord *__restrict__ rec) {
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
        if (crossed) {
            const unsigned pos = atomicAdd(&rec->n_new, 1u);
            if (pos < cap) list[pos] = MuVoxel{(unsigned short)ix, (unsigned short)iy, (unsigned short)iz, 0};
            atomicMin(&rec->lo[0], ix); atomicMin(&rec->lo[1], iy); atomicMin(&rec->lo[2], iz);
            atomicMax(&rec->hi[0], ix); atomicMax(&rec->hi[1], iy); atomicMax(&rec->hi[2], iz);
        }
    }
}

constexpr int MU_CHUNK = 1024;          // new voxels staged per round: 8 KiB of LDS

__global__ __launch_bounds__(256) void mu_esdf_kernel(DevGrid G, float *__restrict__ esdf, const MuVoxel *__restrict__ list, int n_list, MuBox box,
                                                      MuRecord *__restrict__ rec) {
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
        if (nv < old) { esdf[a] = nv; atomicAdd(&rec->lowered, 1ull); }
    }
}

// box of dwords of the inflated map: rows fx in [lo0, lo0 + e0), fy in [lo1, lo1 + e1), dwords w in [lo2, lo2 + e2)
__global__ __launch_bounds__(256) void mu_map_bits_box_kernel(FeParams F, const uint8_t *__restrict__ occ, unsigned *__restrict__ bits, int lo0, int lo1, int lo2,
                                                              int e0, int e1, int e2) {
    const long long n = (long long)e0 * e1 * e2;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long long)gridDim.x * blockDim.x) {
        const int w = lo2 + (int)(t % e2);
        const long long xy = t / e2;
        const int fy = lo1 + (int)(xy % e1), fx = lo0 + (int)(xy / e1);
        bits[((size_t)fx * F.iY + fy) * F.iZW + w] = fe_map_bits_word(F, occ, fx, fy, w);
    }
}

__global__ __launch_bounds__(256) void mu_cspace_box_kernel(FeParams F, const uint8_t *__restrict__ occ, const unsigned *__restrict__ bits,
                                                            const FeRow *__restrict__ rows, const int *__restrict__ row_ptr, uint4 *__restrict__ out, MuBox box) {
    const int e1 = box.hi[1] - box.lo[1] + 1, ez = box.hi[2] - box.lo[2] + 1;
    const int zblocks = (ez + 63) >> 6;
    const long long wv = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const long long n_wv = (long long)(box.hi[0] - box.lo[0] + 1) * e1 * zblocks;
    if (wv >= n_wv) return;
    const int lane = threadIdx.x & 63;
    const int zb = (int)(wv % zblocks);
    const long long xy = wv / zblocks;
    const int y = box.lo[1] + (int)(xy % e1), x = box.lo[0] + (int)(xy / e1);
    const int z = box.lo[2] + (zb << 6) + lane;
    fe_cspace_voxel(F, occ, bits, rows, row_ptr, out, x, y, z, z <= box.hi[2]);
}

// the box's words, x then y then z fastest, nq uint4 per voxel
__global__ __launch_bounds__(256) void mu_pack_box_kernel(const uint4 *__restrict__ table, uint4 *__restrict__ packed, int Y, int Z, int nq, MuBox box) {
    const int e1 = box.hi[1] - box.lo[1] + 1, ez = box.hi[2] - box.lo[2] + 1;
    const long long row = (long long)ez * nq;
    const long long n = (long long)(box.hi[0] - box.lo[0] + 1) * e1 * row;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long long)gridDim.x * blockDim.x) {
        const long long r = t % row, xy = t / row;
        const int y = box.lo[1] + (int)(xy % e1), x = box.lo[0] + (int)(xy / e1);
        packed[t] = table[(((size_t)x * Y + y) * Z + box.lo[2]) * nq + r];
    }
}

}  // namespace isdf

using namespace isdf;

void isdf_map_update_release_all(isdf_ctx *c) { delete c->mup; c->mup = nullptr; }

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

// ---- shared with map_clear.hip (map_update_state.hpp)
float isdf::mu_event_ms(hipEvent_t a, hipEvent_t b) {
    float ms = 0.f;
    return hipEventElapsedTime(&ms, a, b) == hipSuccess ? ms : 0.f;
}

void isdf::mu_drop_derived(isdf_ctx *c, bool voxels) {
    const std::string err = c->err;
    c->d_esdf.release(); c->grid.esdf = nullptr;
    c->bricks_stale = true; c->bits_dirty = true;
    isdf_frontend_release(c);           // the bit map, the table, its host copy and the field
    if (voxels) c->d_counts.release();
    c->err = err;
}

int isdf::mu_state(isdf_ctx *c, MapUpdateState **out) {
    if (!c->mup) { c->mup = new (std::nothrow) MapUpdateState(); if (!c->mup) return isdf_fail(c, ISDF_ERR_HIP, "out of host memory"); }
    for (hipEvent_t &e : c->mup->ev) if (!e) HIPCHK(c, hipEventCreate(&e));
    *out = c->mup;
    return ISDF_OK;
}

int isdf::mu_frontend_box_launch(isdf_ctx *c, MapUpdateState &S, const MuBox &box, const MuBox &grown, bool *patch, size_t *pack_words, long long *cspace_voxels,
                                 size_t pack_offset) {
    const hipStream_t st = c->stream;
    const DevGrid &G = c->grid;
    isdf_ctx::FrontEnd &fe = c->fe;
    const size_t nw = 4 * (size_t)((fe.xk * fe.yk + 127) / 128);
    int rc;
    const FeParams F = fe_params(c);
    // inflated rows x + side, y + side; bit z + side lies in dword (z + side) >> 5 (< iZW - 1: the spare dword stays zero)
    const int w0 = (box.lo[2] + F.side) >> 5, w1 = (box.hi[2] + F.side) >> 5;
    const int e0 = box.hi[0] - box.lo[0] + 1, e1 = box.hi[1] - box.lo[1] + 1, e2 = w1 - w0 + 1;
    const long long nb = (long long)e0 * e1 * e2;
    hipLaunchKernelGGL(mu_map_bits_box_kernel, dim3((unsigned)std::min<long long>((nb + 255) / 256, 2048)), dim3(256), 0, st, F, c->d_occ.get(), fe.d_bits.get(),
                       box.lo[0] + F.side, box.lo[1] + F.side, w0, e0, e1, e2);
    HIPCHK(c, hipGetLastError());
    if (!fe.d_cspace) return ISDF_OK;
    const long long n_wv = (long long)(grown.hi[0] - grown.lo[0] + 1) * (grown.hi[1] - grown.lo[1] + 1) * ((grown.hi[2] - grown.lo[2] + 64) >> 6);
    hipLaunchKernelGGL(mu_cspace_box_kernel, dim3((unsigned)((n_wv + 3) / 4)), dim3(256), 0, st, F, c->d_occ.get(), fe.d_bits.get(),
                       (const FeRow *)fe.d_row_list.get(), fe.d_row_ptr.get(), (uint4 *)fe.d_cspace.get(), grown);
    HIPCHK(c, hipGetLastError());
    *cspace_voxels = mu_box_voxels(grown);
    if (!fe.h_cspace_valid) return ISDF_OK;
    *pack_words = (size_t)mu_box_voxels(grown) * nw;
    if ((rc = S.d_pack.reserve(c, (pack_offset + *pack_words) / 4))) return rc;
    if ((rc = S.h_pack.reserve(c, pack_offset + *pack_words))) return rc;
    const long long np = (long long)(*pack_words / 4);
    hipLaunchKernelGGL(mu_pack_box_kernel, dim3((unsigned)std::min<long long>((np + 255) / 256, 2048)), dim3(256), 0, st, (const uint4 *)fe.d_cspace.get(),
                       S.d_pack.get() + pack_offset / 4, G.Y, G.Z, (int)(nw / 4), grown);
    HIPCHK(c, hipGetLastError());
    *patch = true;
    return ISDF_OK;
}

// everything after the hand-over of a frame that occupied at least one voxel
int isdf::mu_refresh_products(isdf_ctx *c, MapUpdateState &S, const isdf_map_update_params &P, const MuRecord &R, unsigned cap, bool voxels, isdf_map_update_info &info) {
    const hipStream_t st = c->stream;
    const DevGrid &G = c->grid;
    const int dims[3] = {G.X, G.Y, G.Z};
    const size_t n_vox = (size_t)G.X * G.Y * G.Z;
    int rc;
    MuBox box;
    for (int a = 0; a < 3; a++) { box.lo[a] = info.dirty_lo[a] = R.lo[a]; box.hi[a] = info.dirty_hi[a] = R.hi[a]; }
    if (voxels) c->d_counts.release();              // the counts no longer describe the occupancy
    c->bits_dirty = true;

    // ---- which path
    isdf_ctx::FrontEnd &fe = c->fe;
    const bool do_esdf = (bool)c->d_esdf && P.refresh_esdf != 0;
    const bool do_fe = fe.built && P.refresh_frontend != 0;
    const MuBox grown = mu_box_grow(box, do_fe ? (fe.cfg.kernel_size - 1) / 2 : 0, dims);
    float esdf0;
    std::memcpy(&esdf0, &R.esdf0, sizeof(float));
    const bool full = (unsigned long long)R.n_new > (unsigned long long)cap || (double)mu_box_voxels(grown) > P.full_fraction * (double)n_vox ||
                      (do_esdf && std::isinf(esdf0));
    info.path = full ? 2 : 1;
    // The cost-to-go field: dropped (mode 0 of isdf_frontend_field_set_repair), or repaired once the configuration space is the new
    // map's (mode 1).  It is invalid from here until the repair has gone through: every error path leaves it dropped.
    const bool repair = do_fe && isdf_field_repair_wanted(c);
    if (fe.field_valid) { fe.field_valid = false; fe.field_reachable = false; info.field_dropped = 1; }

    // ---- ESDF
    if (c->d_esdf && !P.refresh_esdf) {
        c->d_esdf.release();
        c->grid.esdf = nullptr;
        c->bricks_stale = true;
    }
    if (full && !voxels) {
        launch_threshold_counts(c->d_counts, n_vox, (unsigned)c->counts_thr, c->d_occ, st);
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipEventRecord(S.ev[2], st));
    if (do_esdf) {
        if (full) { if ((rc = isdf_generate_esdf(c))) return rc; }
        else {
            hipLaunchKernelGGL(mu_esdf_kernel, dim3((unsigned)((n_vox + 255) / 256)), dim3(256), 0, st, G, c->d_esdf.get(), S.d_list.get(), (int)R.n_new, box, S.d_rec.get());
            HIPCHK(c, hipGetLastError());
        }
        c->bricks_stale = true;
        info.esdf_refreshed = 1;
    }
    HIPCHK(c, hipEventRecord(S.ev[3], st));

    // ---- front end
    bool patch = false;
    size_t pack_words = 0;
    const size_t nw = 4 * (size_t)((fe.xk * fe.yk + 127) / 128);
    if (fe.built && !P.refresh_frontend) isdf_frontend_release(c);
    HIPCHK(c, hipEventRecord(S.ev[4], st));
    if (do_fe) {
        info.frontend_refreshed = 1;
        info.cspace_refreshed = fe.d_cspace ? 1 : 0;
        if (full) {
            if ((rc = isdf_frontend_refresh_map(c, nullptr))) return rc;
            if (fe.d_cspace) info.cspace_voxels_recomputed = (long long)n_vox;
        } else {
            long long cs_voxels = 0;
            if ((rc = mu_frontend_box_launch(c, S, box, grown, &patch, &pack_words, &cs_voxels))) return rc;
            info.cspace_voxels_recomputed = cs_voxels;
        }
    }
    HIPCHK(c, hipEventRecord(S.ev[5], st));
    if (patch) HIPCHK(c, hipMemcpyAsync(S.h_pack.get(), S.d_pack, pack_words * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(S.h_rec.get(), S.d_rec, sizeof(MuRecord), hipMemcpyDeviceToHost, st));
    if (repair && (rc = isdf_field_repair_begin(c, full ? nullptr : grown.lo, full ? nullptr : grown.hi, S.ev[6]))) return rc;
    HIPCHK(c, hipStreamSynchronize(st));
    if (repair) {                       // the rounds read one word each; the host table is patched after them
        int repaired = 0;
        if ((rc = isdf_field_repair_end(c, S.ev[6], S.ev[7], &repaired))) return rc;
        if (repaired) info.field_dropped = 0;
    }
    if (patch) {
        mu_scatter_box(fe.h_cspace, dims, nw, grown, S.h_pack.get());
        info.host_table_patched = 1;
    }
    info.esdf_voxels_lowered = (long long)S.h_rec.get()->lowered;
    info.esdf_ms = mu_event_ms(S.ev[2], S.ev[3]);
    info.frontend_ms = mu_event_ms(S.ev[4], S.ev[5]);
    // the kept clearance report (mode 1 of isdf_traj_check_set_watch): the new voxels folded in, after every product above.  A failing
    // step drops the report and fails the update as a whole, as a failing repair does.
    if (traj_watch_armed(c) && (rc = traj_watch_fold(c, S.d_list.get(), R.n_new, cap))) return rc;
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
    HIPCHK(c, hipSetDevice(c->device));
    MapUpdateState *Sp;
    { const int rc0 = mu_state(c, &Sp); if (rc0) return rc0; }
    MapUpdateState &S = *Sp;
    const hipStream_t st = c->stream;
    const DevGrid &G = c->grid;
    const size_t n_vox = (size_t)G.X * G.Y * G.Z;
    int rc;

    // ---- count, find the new voxels: one hand-over record, one synchronisation
    const size_t in_bytes = (size_t)n_in * 3 * (voxels ? sizeof(int) : sizeof(float));
    const unsigned cap = (unsigned)std::min<unsigned long long>({(unsigned long long)P.max_new_voxels, (unsigned long long)n_in, (unsigned long long)n_vox, 0x7FFFFFFFull});
    if ((rc = S.d_in.reserve(c, in_bytes))) return rc;
    if ((rc = S.d_list.reserve(c, std::max<size_t>(cap, 1)))) return rc;
    if ((rc = S.d_rec.reserve(c, 1))) return rc;
    if ((rc = S.h_rec.reserve(c, 1))) return rc;
    MuRecord zero{};
    for (int a = 0; a < 3; a++) { zero.lo[a] = 0x7FFFFFFF; zero.hi[a] = -1; }
    *S.h_rec.get() = zero;
    HIPCHK(c, hipMemcpyAsync(S.d_rec, S.h_rec.get(), sizeof(MuRecord), hipMemcpyHostToDevice, st));
    if (n_in > 0) HIPCHK(c, hipMemcpyAsync(S.d_in, in, in_bytes, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipEventRecord(S.ev[0], st));
    if (n_in > 0) {
        const unsigned blocks = (unsigned)std::min<long long>((n_in + 255) / 256, 2048);
        if (voxels) hipLaunchKernelGGL(mu_mark_kernel<true>, dim3(blocks), dim3(256), 0, st, (const void *)S.d_in.get(), n_in, G, (unsigned *)nullptr, 0u, c->d_occ.get(),
                                       (const float *)c->d_esdf.get(), S.d_list.get(), cap, S.d_rec.get());
        else hipLaunchKernelGGL(mu_mark_kernel<false>, dim3(blocks), dim3(256), 0, st, (const void *)S.d_in.get(), n_in, G, c->d_counts.get(), (unsigned)c->counts_thr,
                                c->d_occ.get(), (const float *)c->d_esdf.get(), S.d_list.get(), cap, S.d_rec.get());
        HIPCHK(c, hipGetLastError());
    }
    {
        hipError_t e = hipEventRecord(S.ev[1], st);
        if (e == hipSuccess) e = hipMemcpyAsync(S.h_rec.get(), S.d_rec, sizeof(MuRecord), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) {          // the kernel may have run: the occupancy may have advanced
            c->err = std::string("map update hand-over: ") + hipGetErrorString(e);
            mu_drop_derived(c, voxels);
            return ISDF_ERR_HIP;
        }
    }
    const MuRecord R = *S.h_rec.get();
    info.count_ms = mu_event_ms(S.ev[0], S.ev[1]);
    info.n_new_voxels = R.n_new;
    if (R.n_new == 0) {                 // nothing but the counts changed: every product stays in place, the field included
        if (info_out) *info_out = info;
        return ISDF_OK;
    }
    // from here on the occupancy has advanced: a failure must not leave products behind that describe the old map
    rc = mu_refresh_products(c, S, P, R, cap, voxels, info);
    if (rc != ISDF_OK) { mu_drop_derived(c, voxels); return rc; }
    if (info_out) *info_out = info;
    return ISDF_OK;
}

int update_ready(isdf_ctx *c, const void *in, long long n) {
    if (n < 0 || (n > 0 && !in)) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "bad update arguments");
    if (!c->peers.empty() || c->is_peer) return isdf_fail(c, ISDF_ERR_UNSUPPORTED, "the in-place map update is not offered on a multi-device ctx");
    if (!c->have_geom || !c->d_occ) return isdf_fail(c, ISDF_ERR_STATE, "the map update needs an occupancy grid");
    return ISDF_OK;
}

}  // namespace

extern "C" int isdf_update_pointcloud(isdf_ctx *c, const float *xyz, long long n_points, const isdf_map_update_params *params, isdf_map_update_info *info_out) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    const int rc = update_ready(c, xyz, n_points);
    if (rc) return rc;
    if (!c->d_counts) return isdf_fail(c, ISDF_ERR_STATE, "no kept point counts: the map did not come from isdf_set_pointcloud, or isdf_update_voxels changed it since");
    return map_update(c, xyz, n_points, false, params, info_out);
}

extern "C" int isdf_update_voxels(isdf_ctx *c, const int32_t *ijk, long long n_voxels, const isdf_map_update_params *params, isdf_map_update_info *info_out) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    const int rc = update_ready(c, ijk, n_voxels);
    if (rc) return rc;
    for (long long i = 0; i < n_voxels; i++)
        if (ijk[3 * i] < 0 || ijk[3 * i] >= c->grid.X || ijk[3 * i + 1] < 0 || ijk[3 * i + 1] >= c->grid.Y || ijk[3 * i + 2] < 0 || ijk[3 * i + 2] >= c->grid.Z)
            return isdf_fail(c, ISDF_ERR_INVALID_ARG, "a voxel index lies outside the grid");
    return map_update(c, ijk, n_voxels, true, params, info_out);
}
