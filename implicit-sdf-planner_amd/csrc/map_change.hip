// The steps every in-place change of the map goes through (map_change.hpp), each written once for map_update.hip,
// map_clear.hip, map_scan.hip and map_shift.hip, and the boxed front-end kernels they all end in:
//   mu_map_bits_box_kernel  the dwords of the front end's inflated bit map that cover the dirty box (fe_map_bits_word);
//   mu_cspace_box_kernel    the configuration-space words of the dirty box grown by (k - 1) / 2 (fe_cspace_voxel, the whole-map
//                           kernel's body: one wavefront = 64 consecutive z of one column of the box);
//   mu_pack_box_kernel      that box of the table packed for ONE copy to the host, which scatters it into the A*'s copy.
#include "isdf_ctx.hpp"
#include "frontend_dev.hpp"
#include "map_change.hpp"
#include "swept_field.hpp"
#include <algorithm>
#include <string>

namespace isdf {

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

int isdf::map_change_ready(isdf_ctx *c, const char *op, const void *in, long long n, bool needs_counts, bool may_follow) {
    const std::string o = op;
    if (n < 0 || (n > 0 && !in)) return isdf_fail(c, ISDF_ERR_INVALID_ARG, (o + ": bad arguments").c_str());
    if (!c->peers.empty() || c->is_peer) return isdf_fail(c, ISDF_ERR_UNSUPPORTED, (o + " is not offered on a multi-device ctx").c_str());
    if (!c->have_geom || !c->d_occ) return isdf_fail(c, ISDF_ERR_STATE, (o + " needs an occupancy grid").c_str());
    if (needs_counts && !c->d_counts)
        return isdf_fail(c, ISDF_ERR_STATE, (o + ": no kept point counts (the map did not come from isdf_set_pointcloud, or isdf_update_voxels / isdf_clear_voxels changed it since)").c_str());
    // a field gated by the eroded known grid describes the K and the map of its build: it goes here, also where the call then finds
    // nothing to change, and whatever the repair, reopen and shift modes say - unless it follows the change (DESIGN 4.27:
    // may_follow and isdf_frontend_field_set_known_follow(1)); the driver then runs the stages or drops it
    c->gate_dropped = (may_follow ? isdf_field_known_changed(c) : isdf_field_gate_drop(c)) != 0;
    isdf_field_follow_call(c);
    return ISDF_OK;
}

int isdf::map_voxels_in_grid(isdf_ctx *c, const int32_t *ijk, long long n) {
    const int dims[3] = {c->grid.X, c->grid.Y, c->grid.Z};
    for (long long i = 0; i < 3 * n; i++)
        if (ijk[i] < 0 || ijk[i] >= dims[i % 3]) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "a voxel index lies outside the grid");
    return ISDF_OK;
}

int isdf::map_begin(isdf_ctx *c, MapUpdateState **out) {
    HIPCHK(c, hipSetDevice(c->device));
    ISDF_TRY(c->mup.make(c, out));
    ISDF_TRY((*out)->ev.ready(c));
    return (*out)->ev_scan.ready(c);
}

unsigned isdf::map_list_cap(long long max_voxels, unsigned long long n_in, unsigned long long n_vox) {
    return (unsigned)std::min<unsigned long long>({(unsigned long long)max_voxels, n_in, n_vox, 0x7FFFFFFFull});
}

int isdf::map_stage(isdf_ctx *c, MapUpdateState &S, const void *in, size_t in_bytes, const void *in2, size_t in2_bytes, size_t list_len, hipEvent_t ev_begin) {
    const hipStream_t st = c->stream;
    int rc;
    if ((rc = S.d_in.reserve(c, in_bytes + in2_bytes))) return rc;
    if (list_len && (rc = S.d_list.reserve(c, list_len))) return rc;
    if ((rc = S.rec.ready(c))) return rc;
    HIPCHK(c, S.rec.put(map_records_empty(), st));
    if (in_bytes && in) HIPCHK(c, hipMemcpyAsync(S.d_in, in, in_bytes, hipMemcpyHostToDevice, st));
    if (in2_bytes && in2) HIPCHK(c, hipMemcpyAsync((uint8_t *)S.d_in.get() + in_bytes, in2, in2_bytes, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipEventRecord(ev_begin, st));
    return ISDF_OK;
}

int isdf::map_hand_over(isdf_ctx *c, MapUpdateState &S, hipEvent_t ev_end, const char *op, bool voxels) {
    hipError_t e = ev_end ? hipEventRecord(ev_end, c->stream) : hipSuccess;
    if (e == hipSuccess) e = S.rec.fetch(c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) return ISDF_OK;
    c->err = std::string(op) + " hand-over: " + hipGetErrorString(e);
    mu_drop_derived(c, voxels);
    return ISDF_ERR_HIP;
}

void isdf::mu_drop_derived(isdf_ctx *c, bool voxels) {
    const std::string err = c->err;
    c->d_esdf.release(); c->grid.esdf = nullptr;
    c->bricks_stale = true; c->bits_dirty = true;
    isdf_frontend_release(c);           // the bit map, the table, its host copy and the field
    if (voxels) c->d_counts.release();
    c->err = err;
}

int isdf::map_changed(isdf_ctx *c, bool voxels) {
    if (voxels) c->d_counts.release();
    c->bits_dirty = true;
    isdf_ctx::FrontEnd &fe = c->fe;
    if (!fe.field_valid) return c->gate_dropped ? 1 : 0;          // (a gated field went in map_change_ready)
    fe.field_valid = false; fe.field_reachable = false;
    return 1;
}

MapRefresh isdf::map_refresh_begin(isdf_ctx *c, const MapListRecord &R, unsigned cap, bool voxels, int refresh_esdf, int refresh_frontend, double full_fraction,
                                   int *field_dropped) {
    const DevGrid &G = c->grid;
    const int dims[3] = {G.X, G.Y, G.Z};
    *field_dropped = map_changed(c, voxels);
    MapRefresh M;
    for (int a = 0; a < 3; a++) { M.box.lo[a] = R.lo[a]; M.box.hi[a] = R.hi[a]; }
    M.do_esdf = (bool)c->d_esdf && refresh_esdf != 0;
    M.do_fe = c->fe.built && refresh_frontend != 0;
    M.grown = mu_box_grow(M.box, M.do_fe ? (c->fe.cfg.kernel_size - 1) / 2 : 0, dims);
    M.over = R.n > cap || (double)mu_box_voxels(M.grown) > full_fraction * ((double)G.X * G.Y * G.Z);
    if (c->d_esdf && !refresh_esdf) {
        c->d_esdf.release();
        c->grid.esdf = nullptr;
        c->bricks_stale = true;
    }
    return M;
}

namespace {

// one (box, grown) pair of the front-end stage; *words: what it packed at dword pack_offset of S.d_pack (0: nothing to patch).  A
// caller with several boxes (map_shift.hip) reserves S.d_pack and S.h_pack for all of them first, so that nothing grows here.
int frontend_box_launch(isdf_ctx *c, MapUpdateState &S, const MuBox &box, const MuBox &grown, size_t pack_offset, size_t *words, long long *cspace_voxels) {
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
    *words = (size_t)mu_box_voxels(grown) * nw;
    if ((rc = S.d_pack.reserve(c, (pack_offset + *words) / 4))) return rc;
    if ((rc = S.h_pack.reserve(c, pack_offset + *words))) return rc;
    const long long np = (long long)(*words / 4);
    hipLaunchKernelGGL(mu_pack_box_kernel, dim3((unsigned)std::min<long long>((np + 255) / 256, 2048)), dim3(256), 0, st, (const uint4 *)fe.d_cspace.get(),
                       S.d_pack.get() + pack_offset / 4, G.Y, G.Z, (int)(nw / 4), grown);
    HIPCHK(c, hipGetLastError());
    return ISDF_OK;
}

}  // namespace

int isdf::map_frontend_launch(isdf_ctx *c, MapUpdateState &S, bool on, bool full, const MuBox *boxes, const MuBox *grown, int n_boxes, MapFrontend &F, bool stamp) {
    const hipStream_t st = c->stream;
    isdf_ctx::FrontEnd &fe = c->fe;
    int rc;
    F = MapFrontend{};
    if (fe.built && !on) isdf_frontend_release(c);
    if (stamp) HIPCHK(c, hipEventRecord(S.ev[4], st));
    if (fe.built && on) {
        F.refreshed = 1;
        F.cspace_refreshed = fe.d_cspace ? 1 : 0;
        if (full) {
            if ((rc = isdf_frontend_refresh_map(c, nullptr))) return rc;
            if (fe.d_cspace) F.cspace_voxels = (long long)c->grid.X * c->grid.Y * c->grid.Z;
        } else {
            F.n_boxes = n_boxes;
            for (int b = 0; b < n_boxes; b++) {
                size_t words = 0;
                long long vox = 0;
                F.grown[b] = grown[b];
                F.pack_at[b] = F.pack_total;
                if ((rc = frontend_box_launch(c, S, boxes[b], grown[b], F.pack_total, &words, &vox))) return rc;
                F.pack_total += words;
                F.cspace_voxels += vox;
            }
            F.patch = F.pack_total > 0;
        }
    }
    HIPCHK(c, hipEventRecord(S.ev[5], st));
    if (F.patch) HIPCHK(c, hipMemcpyAsync(S.h_pack.get(), S.d_pack, F.pack_total * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    return ISDF_OK;
}

void isdf::map_frontend_finish(isdf_ctx *c, MapUpdateState &S, MapFrontend &F) {
    isdf_ctx::FrontEnd &fe = c->fe;
    const int dims[3] = {c->grid.X, c->grid.Y, c->grid.Z};
    if (F.patch) {
        const size_t nw = 4 * (size_t)((fe.xk * fe.yk + 127) / 128);
        for (int b = 0; b < F.n_boxes; b++) mu_scatter_box(fe.h_cspace, dims, nw, F.grown[b], S.h_pack.get() + F.pack_at[b]);
        F.host_table_patched = 1;
    }
    F.ms = S.ev.ms(4, 5);
}

int isdf::map_frontend_stage(isdf_ctx *c, MapUpdateState &S, FfChange dir, bool follow, bool on, bool full, const MapRefresh &M, MapFrontend &F, int *field_dropped,
                             const MuBox *field_more) {
    const MuBox fbox = field_more ? mu_box_union(M.grown, *field_more) : M.grown;     // the field's box: where the table or (field_more) the gate can have moved
    const int *const lo = full ? nullptr : fbox.lo, *const hi = full ? nullptr : fbox.hi;
    int rc;
    if ((rc = map_frontend_launch(c, S, on, full, &M.box, &M.grown, 1, F))) return rc;
    HIPCHK(c, S.rec.fetch(c->stream));
    if (follow && (rc = isdf_field_change_begin(c, dir, lo, hi, S.ev[6]))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (follow) {
        int kept = 0;
        if ((rc = isdf_field_change_end(c, dir, lo, hi, S.ev[6], S.ev[7], &kept))) return rc;
        if (kept) *field_dropped = 0;
        else (void)isdf_field_gate_drop(c);               // (a gated field that met a bit against the direction: its gate goes with it)
    }
    map_frontend_finish(c, S, F);
    return ISDF_OK;
}

int isdf::map_watch_recheck(isdf_ctx *c, bool armed, int32_t *rechecked) {
    if (!armed) return ISDF_OK;
    const long long folded = c->tck->w.last.updates_folded;
    isdf_traj_check_info now;
    const int rc = traj_check_rerun_kept(c, &now);
    if (rc) {
        const std::string err = c->err;
        (void)hipStreamSynchronize(c->stream);
        traj_check_drop_report(c);
        c->err = err;
        return rc;
    }
    isdf_traj_watch_info &L = c->tck->w.last;           // (the re-check armed the watch again and cleared this)
    L.updates_folded = folded + 1;
    L.path = 2;
    L.select_ms = now.select_ms; L.field_ms = now.field_ms; L.reduce_ms = now.reduce_ms;
    *rechecked = 1;
    return ISDF_OK;
}
