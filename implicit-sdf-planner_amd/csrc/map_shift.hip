// The map window shifted in place: isdf_shift_map / isdf_map_follow.  New voxel v holds what old voxel v + s held.
//   msh_translate_kernel      one lane per DESTINATION element, z fastest: a wavefront writes 64 consecutive elements and reads the 64
//                             consecutive elements s away (a run ends where a z-row does).  An element without a source is zero.
//                             T = unsigned: the kept counts, one element a voxel; T = uint4: the configuration-space table, nq
//                             elements a voxel, 16-byte loads and stores (the layout fe_cspace_voxel writes: voxel-major, nq uint4).
//                             The counts' instance also looks at its own index as a SOURCE: a voxel without a destination left the
//                             window, and its count goes into the record.
//   msh_translate_occ_kernel  the occupancy bytes, one lane per destination DWORD (the grid is allocated as whole dwords; a z-row is
//                             not: the four bytes are placed one by one, a row's end carried).  Counts the occupied voxels that left
//                             and notes whether any voxel is still occupied.
// Both reduce in the wavefront, then through LDS (dev_reduce.hpp's block_sum), and issue one set of global atomics per workgroup into one 64-byte record.  The
// destination is a second buffer that then changes places with the ctx's own: no overlap of source and destination, no copy back.
// Everything else is existing code: isdf_generate_esdf on the shifted occupancy, the whole inflated bit map, the boxed
// configuration-space kernel over the bands (map_shift_host.hpp), the pack / scatter path into the A*'s host copy - the shared steps
// of map_change.hpp.  A valid cost-to-go field is dropped or, with isdf_frontend_field_set_shift(1), carried after the front-end
// refresh (frontend_field.hip: isdf_field_shift_wanted / _begin / _end).
#include "isdf_ctx.hpp"
#include "frontend_dev.hpp"
#include "map_shift_host.hpp"
#include "map_change.hpp"
#include "swept_field.hpp"
#include "dev_reduce.hpp"
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>

namespace isdf {

struct MshGeom { int X, Y, Z, s0, s1, s2; };            // |s_a| <= dim_a (clamped on the host: beyond it everything has left anyway)

template <typename T> __device__ __forceinline__ T msh_zero();
template <> __device__ __forceinline__ unsigned msh_zero<unsigned>() { return 0u; }
template <> __device__ __forceinline__ uint4 msh_zero<uint4>() { return make_uint4(0u, 0u, 0u, 0u); }

__device__ __forceinline__ bool msh_inside(const MshGeom &g, int x, int y, int z) {
    return x >= 0 && x < g.X && y >= 0 && y < g.Y && z >= 0 && z < g.Z;
}

// called by every thread of a 256-thread workgroup: the two sums and the flag over the workgroup, then one atomic each where not zero
__device__ __forceinline__ void msh_block_reduce(unsigned long long counts_left, unsigned long long occupied_left, bool any_occ, MshRecord *__restrict__ rec) {
    __shared__ unsigned s_f[4];
    const bool wave_any = __ballot(any_occ) != 0ull;
    if ((threadIdx.x & 63) == 0) s_f[threadIdx.x >> 6] = wave_any ? 1u : 0u;
    const unsigned long long cnt[2] = {counts_left, occupied_left};
    const unsigned long long s = block_sum<2, 4>(cnt);      // thread 0: counts, thread 1: occupied (its barrier lies behind the flags' stores)
    if (threadIdx.x == 0 && s) atomicAdd(&rec->counts_left, s);
    if (threadIdx.x == 1 && s) atomicAdd(&rec->occupied_left, s);
    if (threadIdx.x == 0 && (s_f[0] | s_f[1] | s_f[2] | s_f[3])) atomicOr(&rec->any_occ, 1u);
}

template <typename T, bool COUNTS>
__global__ __launch_bounds__(256) void msh_translate_kernel(const T *__restrict__ src, T *__restrict__ dst, MshGeom g, int epv, MshRecord *__restrict__ rec) {
    const size_t rowlen = (size_t)g.Z * epv, n = (size_t)g.X * g.Y * rowlen;
    unsigned long long left = 0;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
        const size_t row = e / rowlen;
        const int r = (int)(e - row * rowlen);
        const int z = r / epv, q = r - z * epv;
        const int x = (int)(row / g.Y), y = (int)(row - (size_t)x * g.Y);
        const int sx = x + g.s0, sy = y + g.s1, sz = z + g.s2;
        T v = msh_zero<T>();
        if (msh_inside(g, sx, sy, sz)) v = src[(((size_t)sx * g.Y + sy) * g.Z + sz) * epv + q];
        dst[e] = v;
        if constexpr (COUNTS) {
            if (!msh_inside(g, x - g.s0, y - g.s1, z - g.s2)) left += src[e];
        }
    }
    if constexpr (COUNTS) msh_block_reduce(left, 0ull, false, rec);
}

__global__ __launch_bounds__(256) void msh_translate_occ_kernel(const uint8_t *__restrict__ src, unsigned *__restrict__ dst, MshGeom g, MshRecord *__restrict__ rec) {
    const size_t n = (size_t)g.X * g.Y * g.Z, nd = (n + 3) >> 2;
    unsigned long long left = 0;
    bool any = false;
    for (size_t d = (size_t)blockIdx.x * 256 + threadIdx.x; d < nd; d += (size_t)gridDim.x * 256) {
        const size_t a = d << 2;
        const size_t row = a / g.Z;
        int z = (int)(a - row * g.Z);
        int x = (int)(row / g.Y), y = (int)(row - (size_t)x * g.Y);
        const unsigned own = ((const unsigned *)src)[d];          // these four voxels as sources (bytes past the grid's end are not looked at)
        unsigned w = 0;
        for (int b = 0; b < 4 && a + b < n; b++) {
            const int sx = x + g.s0, sy = y + g.s1, sz = z + g.s2;
            if (msh_inside(g, sx, sy, sz)) w |= (unsigned)src[((size_t)sx * g.Y + sy) * g.Z + sz] << (8 * b);
            if (!msh_inside(g, x - g.s0, y - g.s1, z - g.s2) && ((own >> (8 * b)) & 0xFFu) == 1u) left++;
            if (++z == g.Z) { z = 0; if (++y == g.Y) { y = 0; ++x; } }
        }
        dst[d] = w;
        any = any || w != 0u;
    }
    msh_block_reduce(0ull, left, any, rec);
}

}  // namespace isdf

using namespace isdf;

extern "C" void isdf_map_shift_params_default(isdf_map_shift_params *p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->full_fraction = 0.5;
    p->force_path = 0;
}

extern "C" void isdf_map_shift_sizes(int sizes_out[2]) {
    if (!sizes_out) return;
    sizes_out[0] = (int)sizeof(isdf_map_shift_params); sizes_out[1] = (int)sizeof(isdf_map_shift_info);
}

namespace {

typedef std::chrono::steady_clock clk;

int shift_params(isdf_ctx *c, const isdf_map_shift_params *params, isdf_map_shift_params &P) {
    isdf_map_shift_params_default(&P);
    if (params) P = *params;
    if (!(P.full_fraction >= 0.0) || P.force_path < 0 || P.force_path > 2) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "bad map shift parameters");
    return ISDF_OK;
}

unsigned grid_blocks(size_t n) { return (unsigned)std::min<size_t>((n + 255) / 256, 2048); }

// everything after the translated counts and occupancy took the place of the old ones
// carry: the cost-to-go field follows the shift (isdf_field_shift_wanted, asked before the field was dropped)
int shift_refresh(isdf_ctx *c, MapUpdateState &S, bool full, const MuBox *boxes, int n_boxes, bool watch, bool carry, isdf_map_shift_info &info) {
    const hipStream_t st = c->stream;
    const DevGrid &G = c->grid;
    isdf_ctx::FrontEnd &fe = c->fe;
    int rc;

    // ---- ESDF: the whole-map transform on the shifted occupancy
    HIPCHK(c, hipEventRecord(S.ev[2], st));
    if (c->d_esdf && (rc = isdf_generate_esdf(c))) return rc;
    HIPCHK(c, hipEventRecord(S.ev[3], st));

    // ---- front end: the inflated map whole; of the (translated) table the bands, or all of it
    MapFrontend F;
    HIPCHK(c, hipEventRecord(S.ev[4], st));
    if (fe.built && !full && (rc = isdf_frontend_map_bits(c))) return rc;
    if ((rc = map_frontend_launch(c, S, true, full, boxes, boxes, fe.d_cspace ? n_boxes : 0, F, false))) return rc;
    if (carry && (rc = isdf_field_shift_begin(c, info.shift, S.ev[6]))) return rc;
    HIPCHK(c, hipStreamSynchronize(st));
    if (carry) {                        // outside the bands the translated word is the new one: the opening mark looks at their hull
        const bool whole = full || n_boxes == 0;
        MuBox hull{};
        for (int b = 0; b < n_boxes && !whole; b++)
            for (int a = 0; a < 3; a++) {
                hull.lo[a] = b ? std::min(hull.lo[a], boxes[b].lo[a]) : boxes[b].lo[a];
                hull.hi[a] = b ? std::max(hull.hi[a], boxes[b].hi[a]) : boxes[b].hi[a];
            }
        if ((rc = isdf_field_shift_end(c, info.shift, whole ? nullptr : hull.lo, whole ? nullptr : hull.hi, S.ev.get() + 6))) return rc;
        info.field_dropped = 0;
    }
    if (F.patch) {                      // the A*'s copy: translated in place by the host form's own function, then the bands
        const int32_t d32[3] = {G.X, G.Y, G.Z};
        msh_shift_grid(fe.h_cspace, 4 * (size_t)((fe.xk * fe.yk + 127) / 128) * sizeof(uint32_t), d32, info.shift, fe.h_cspace);
    }
    map_frontend_finish(c, S, F);
    info.n_boxes = F.n_boxes; info.cspace_voxels = F.cspace_voxels; info.host_table_patched = F.host_table_patched; info.frontend_ms = F.ms;
    info.translate_ms = S.ev.ms(0, 1);
    info.esdf_ms = S.ev.ms(2, 3);
    // the kept clearance report: the trajectory is in world coordinates, so it is checked against the whole new map again, as the
    // clear does, and stays armed under the new epoch
    return map_watch_recheck(c, watch, &info.watch_rechecked);
}

int shift_map(isdf_ctx *c, const int32_t s[3], const isdf_map_shift_params &P, isdf_map_shift_info *info_out) {
    const clk::time_point t0 = clk::now();
    isdf_map_shift_info info{};
    DevGrid &G = c->grid;
    const int32_t dims[3] = {G.X, G.Y, G.Z};
    for (int a = 0; a < 3; a++) { info.shift[a] = s[a]; info.bmin_new[a] = G.bmin[a]; }
    info.field_dropped = c->gate_dropped ? 1 : 0;       // (a gated field went in map_change_ready, also where nothing moves)
    if (s[0] == 0 && s[1] == 0 && s[2] == 0) {          // nothing is touched, the epoch included
        if (info_out) *info_out = info;
        return ISDF_OK;
    }
    double nb0[3], nb1[3];
    if (!msh_shift_geometry(G.bmin, G.bmax, G.res, dims, s, nb0, nb1))
        return isdf_fail(c, ISDF_ERR_INVALID_ARG, "map shift: the shifted box does not give the map's grid dimensions again (isdf_shift_geometry_host)");
    MapUpdateState *Sp;
    int rc = map_begin(c, &Sp);
    if (rc) return rc;
    MapUpdateState &S = *Sp;
    const hipStream_t st = c->stream;
    isdf_ctx::FrontEnd &fe = c->fe;
    const size_t n_vox = (size_t)G.X * G.Y * G.Z, n_occ = (n_vox + 3) & ~(size_t)3;
    const size_t nw = 4 * (size_t)((fe.xk * fe.yk + 127) / 128);

    // ---- what the host knows before anything runs: the bands, and the path but for an empty map
    MshGeom g{G.X, G.Y, G.Z, 0, 0, 0};
    bool all_left = false;
    {
        int *gs[3] = {&g.s0, &g.s1, &g.s2};
        for (int a = 0; a < 3; a++) {
            *gs[a] = std::max(-dims[a], std::min(dims[a], s[a]));
            if (*gs[a] == dims[a] || *gs[a] == -dims[a]) all_left = true;
        }
    }
    MuBox boxes[6];
    const int n_boxes = msh_shift_bands(dims, s, fe.built ? (fe.cfg.kernel_size - 1) / 2 : 0, boxes);
    long long band_voxels = 0;
    for (int b = 0; b < n_boxes; b++) band_voxels += mu_box_voxels(boxes[b]);
    const bool full_known = all_left || P.force_path == 2 || (P.force_path != 1 && (double)band_voxels > P.full_fraction * (double)n_vox);
    const bool table = !full_known && (bool)fe.d_cspace;            // translate the table along with the counts

    // ---- scratch: nothing below allocates after the first call of a size
    if ((rc = S.d_shift_counts.reserve(c, n_vox)) || (rc = S.d_shift_occ.reserve(c, n_occ))) return rc;
    if (table && (rc = S.d_shift_cspace.reserve(c, n_vox * nw))) return rc;
    if (table && fe.h_cspace_valid && ((rc = S.d_pack.reserve(c, (size_t)band_voxels * nw / 4)) || (rc = S.h_pack.reserve(c, (size_t)band_voxels * nw)))) return rc;
    if ((rc = map_stage(c, S, nullptr, 0, nullptr, 0, 0, S.ev[0]))) return rc;
    MshRecord *const d_rec = &S.rec.dev()->shift;

    // ---- translate into the second buffers
    hipLaunchKernelGGL((msh_translate_kernel<unsigned, true>), dim3(grid_blocks(n_vox)), dim3(256), 0, st, (const unsigned *)c->d_counts.get(), S.d_shift_counts.get(), g, 1, d_rec);
    hipLaunchKernelGGL(msh_translate_occ_kernel, dim3(grid_blocks(n_occ / 4)), dim3(256), 0, st, (const uint8_t *)c->d_occ.get(), (unsigned *)S.d_shift_occ.get(), g, d_rec);
    if (table)
        hipLaunchKernelGGL((msh_translate_kernel<uint4, false>), dim3(grid_blocks(n_vox * (nw / 4))), dim3(256), 0, st, (const uint4 *)fe.d_cspace.get(),
                           (uint4 *)S.d_shift_cspace.get(), g, (int)(nw / 4), (MshRecord *)nullptr);
    HIPCHK(c, hipGetLastError());
    if (c->known.have && (rc = map_known_shift_launch(c, s))) return rc;           // the known grid moves with the window (map_known.hip)
    HIPCHK(c, hipEventRecord(S.ev[1], st));

    // ---- the new map takes the old one's place.  From here on a failure must not leave products behind that describe the old map.
    const bool watch = traj_watch_armed(c);             // (asked before the epoch moves: a stale watch disarms itself)
    if (c->known.have) map_known_shift_swap(c);
    c->d_counts.swap(S.d_shift_counts);
    c->d_occ.swap(S.d_shift_occ);
    if (table) fe.d_cspace.swap(S.d_shift_cspace);
    G.occ = c->d_occ;
    for (int a = 0; a < 3; a++) { G.bmin[a] = info.bmin_new[a] = nb0[a]; G.bmax[a] = nb1[a]; }
    c->grid_epoch++;                    // voxel indices changed their meaning
    c->bricks_stale = true;
    const bool carry = isdf_field_shift_wanted(c, s);   // (asked before the field is dropped: it stays invalid until the carry has gone through)
    info.field_dropped = map_changed(c, false);
    if ((rc = map_hand_over(c, S, nullptr, "map shift", false))) return rc;
    const MshRecord R = S.rec.host().shift;
    info.voxels_entered = msh_voxels_entered(dims, s);
    info.occupied_left = (long long)R.occupied_left;
    info.counts_left = (long long)R.counts_left;
    const bool full = full_known || (P.force_path != 1 && !R.any_occ);
    info.path = full ? ISDF_MAP_SHIFT_FULL : ISDF_MAP_SHIFT_INCREMENTAL;
    rc = shift_refresh(c, S, full, boxes, n_boxes, watch, carry, info);
    if (rc != ISDF_OK) { mu_drop_derived(c, false); return rc; }
    info.wall_ms = std::chrono::duration<double, std::milli>(clk::now() - t0).count();
    if (info_out) *info_out = info;
    return ISDF_OK;
}

}  // namespace

extern "C" int isdf_shift_map(isdf_ctx *c, const int32_t shift_ijk[3], const isdf_map_shift_params *params, isdf_map_shift_info *info_out) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    if (!shift_ijk) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "null shift");
    int rc = map_change_ready(c, "shifting the map", nullptr, 0, true, false);
    if (rc) return rc;
    isdf_map_shift_params P;
    if ((rc = shift_params(c, params, P))) return rc;
    return shift_map(c, shift_ijk, P, info_out);
}

extern "C" int isdf_map_follow(isdf_ctx *c, const double centre_xyz[3], int min_shift, const isdf_map_shift_params *params, int32_t shift_out[3],
                               isdf_map_shift_info *info_out) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    if (shift_out) shift_out[0] = shift_out[1] = shift_out[2] = 0;
    if (!centre_xyz || min_shift < 0) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "map follow: null centre or negative min_shift");
    int rc = map_change_ready(c, "shifting the map", nullptr, 0, true, false);
    if (rc) return rc;
    isdf_map_shift_params P;
    if ((rc = shift_params(c, params, P))) return rc;
    const DevGrid &G = c->grid;
    const int dims[3] = {G.X, G.Y, G.Z};
    int32_t s[3];
    long long most = 0;
    for (int a = 0; a < 3; a++) {
        if (!std::isfinite(centre_xyz[a])) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "map follow: the centre is not finite");
        const double v = std::floor((centre_xyz[a] - G.bmin[a]) / G.res);          // grid_index's binning, not clamped: the formula extends beyond the map
        if (!(std::fabs(v) < 2147000000.0)) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "map follow: the centre's voxel index does not fit 32 bits");
        s[a] = (int32_t)((long long)v - dims[a] / 2);
        most = std::max<long long>(most, s[a] < 0 ? -(long long)s[a] : (long long)s[a]);
    }
    if (most < (long long)min_shift) { s[0] = s[1] = s[2] = 0; }
    rc = shift_map(c, s, P, info_out);
    if (rc == ISDF_OK && shift_out) for (int a = 0; a < 3; a++) shift_out[a] = s[a];
    return rc;
}

extern "C" int isdf_shift_geometry_host(const double bmin[3], const double bmax[3], double resolution, const int32_t dims[3], const int32_t shift[3],
                                        double bmin_out[3], double bmax_out[3]) {
    if (!bmin || !bmax || !shift || !bmin_out || !bmax_out || !(resolution > 0.0) || msh_dims_bad(dims)) return isdf_fail(nullptr, ISDF_ERR_INVALID_ARG, "shift (host form): bad arguments");
    if (!msh_shift_geometry(bmin, bmax, resolution, dims, shift, bmin_out, bmax_out))
        return isdf_fail(nullptr, ISDF_ERR_INVALID_ARG, "shift (host form): the shifted box does not give the grid dimensions again");
    return ISDF_OK;
}

extern "C" int isdf_shift_grid_host(const void *in, int elem_bytes, const int32_t dims[3], const int32_t shift[3], void *out) {
    if (!in || !out || !shift || elem_bytes < 1 || msh_dims_bad(dims)) return isdf_fail(nullptr, ISDF_ERR_INVALID_ARG, "shift (host form): bad arguments");
    msh_shift_grid(in, (size_t)elem_bytes, dims, shift, out);
    return ISDF_OK;
}

extern "C" int isdf_shift_bands_host(const int32_t dims[3], const int32_t shift[3], int side, int32_t boxes_out[6][6], int *n_boxes_out) {
    if (!shift || !boxes_out || !n_boxes_out || side < 0 || msh_dims_bad(dims)) return isdf_fail(nullptr, ISDF_ERR_INVALID_ARG, "shift (host form): bad arguments");
    MuBox boxes[6];
    const int n = msh_shift_bands(dims, shift, side, boxes);
    for (int b = 0; b < n; b++)
        for (int a = 0; a < 3; a++) { boxes_out[b][a] = boxes[b].lo[a]; boxes_out[b][3 + a] = boxes[b].hi[a]; }
    *n_boxes_out = n;
    return ISDF_OK;
}
