// The view gain: isdf_view_gain, the unknown voxels a depth camera would see from each of many candidate poses.
//   vg_setup_kernel  one view per lane: view_gain_host.hpp's vg_view_setup - the call's rays with the view's pose, the origin's tick, and
//                    whether the view is scored - into the per-view table; the row's status and n_rays.
//   vg_gain_kernel   grid = (blocks of rays, views of the chunk), one ray per lane, grid-stride over the view's rays: vg_ray, the ray of
//                    the depth camera, the cast's walk over the occupancy bytes, then the same walk again as far as the cast went with
//                    one look at K per voxel.  The lane keeps K's word while the walk stays inside one dword (z is the fast axis).  Only
//                    an unknown voxel touches the view's `seen` grid (K's layout, so the two share the word index): a read, then an
//                    atomicOr where the bit reads clear, and the lane whose atomicOr returned the bit clear counts the voxel - each
//                    unknown voxel of the view's set exactly once.  The five counters are summed in the wavefront, then through LDS,
//                    then one 64-bit atomicAdd per workgroup per word into the view's row.
// Every walk has at most 1 + nx + ny + nz voxels and stays in the box of its two end voxels: no bounds test, no read outside the grids.
// The lanes of a wavefront finish at different lengths, as the cast's do; a workgroup is two wavefronts for the cast's reason.
// Nothing here writes to the ctx's map, its known grid, its products or its flags.
#include "view_gain_run.hpp"
#include "dev_reduce.hpp"
#include <algorithm>
#include <cstring>

namespace isdf {

constexpr int VG_BLOCK = 128;
constexpr int VG_WAVES = VG_BLOCK / 64;
constexpr int VG_COUNTERS = 5;
constexpr int VG_SETUP_BLOCK = 64;
constexpr long long VG_MAX_CHUNK = 65535;       // gridDim.y

__global__ __launch_bounds__(VG_SETUP_BLOCK) void vg_setup_kernel(const double *__restrict__ poses, long long n_views, DcRays base, MapGeom M, VgView *__restrict__ views,
                                                                  long long *__restrict__ rows) {
    const long long j = (long long)blockIdx.x * VG_SETUP_BLOCK + threadIdx.x;
    if (j >= n_views) return;
    double pose[12];
    for (int i = 0; i < 12; i++) pose[i] = poses[12 * j + i];
    VgView V;
    vg_view_setup(base, M, pose, V);
    views[j] = V;
    long long *const row = rows + VG_ROW * j;
    row[0] = V.ok ? VG_SCORED : VG_POSE_OUTSIDE;
    row[2] = V.ok ? (long long)V.Q.nu * V.Q.nv : 0;
    row[1] = row[3] = row[4] = row[5] = row[6] = row[7] = 0;
}

// rows: the call's, view0 the chunk's first view; seen: the chunk's grids, n_words each, cleared
__global__ __launch_bounds__(VG_BLOCK) void vg_gain_kernel(const VgView *__restrict__ views, long long view0, MapGeom M, const uint8_t *__restrict__ occ,
                                                           const unsigned *__restrict__ known, unsigned *seen, long long n_words, const uint16_t *__restrict__ zero_image,
                                                           long long *rows) {
    const long long j = view0 + blockIdx.y;
    const VgView &V = views[j];
    if (!V.ok) return;          // (uniform)
    unsigned *const my_seen = seen + (size_t)blockIdx.y * (size_t)n_words;
    const long long n = (long long)V.Q.nu * V.Q.nv;
    long long gain = 0, n_skipped = 0, n_hits = 0, steps_total = 0, n_rays_unknown = 0;
    for (long long k = (long long)blockIdx.x * VG_BLOCK + threadIdx.x; k < n; k += (long long)gridDim.x * VG_BLOCK) {
        const int iv = (int)(k / V.Q.nu), iu = (int)(k - (long long)iv * V.Q.nu);
        size_t held = ~(size_t)0;               // the word of K the lane holds
        unsigned kw = 0u;
        auto visit = [&](size_t a) {
            const size_t w = a >> 5;
            const unsigned b = 1u << (unsigned)(a & 31);
            if (w != held) { held = w; kw = known[w]; }
            if (kw & b) return false;
            if (!(my_seen[w] & b) && !(atomicOr(my_seen + w, b) & b)) gain++;
            return true;
        };
        if (!vg_ray(V, M, zero_image, occ, iu, iv, n_hits, steps_total, n_rays_unknown, visit)) n_skipped++;
    }
    const long long cnt[VG_COUNTERS] = {gain, n_skipped, n_hits, steps_total, n_rays_unknown};
    const unsigned long long s = block_sum<VG_COUNTERS, VG_WAVES>(cnt);
    const int word = threadIdx.x == 0 ? 1 : threadIdx.x + 2;          // gain: word 1; the other four: words 3 .. 6
    if (s) atomicAdd((unsigned long long *)(rows + VG_ROW * j + word), s);          // (s is 0 beyond the counters)
}

}  // namespace isdf

// (ViewGainState: view_gain_run.hpp, with the declarations of gain_setup and gain_run - the candidate views score through them)

using namespace isdf;

extern "C" void isdf_view_gain_params_default(isdf_view_gain_params *p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->stride_u = p->stride_v = 4;
    p->max_range_m = 5.0;
    p->scratch_bytes = (int64_t)64 << 20;
}

extern "C" void isdf_view_gain_sizes(int sizes_out[2]) {
    if (!sizes_out) return;
    sizes_out[0] = (int)sizeof(isdf_view_gain_params); sizes_out[1] = (int)sizeof(isdf_view_gain_info);
}

namespace isdf {

// what the device and the host forms check and set up alike (c may be null: the host form)
int gain_setup(isdf_ctx *c, const isdf_depth_camera *cam, const void *poses, long long n_views, const isdf_view_gain_params *params, const void *rows, const MapGeom &M,
               isdf_view_gain_params &P, DcRays &base) {
    P = map_query::resolve(params, isdf_view_gain_params_default);
    const double k[4] = {cam ? cam->fx : 0.0, cam ? cam->fy : 0.0, cam ? cam->cx : 0.0, cam ? cam->cy : 0.0};
    if (!cam || cam->width < 1 || cam->width > DC_MAX_DIM || cam->height < 1 || cam->height > DC_MAX_DIM || !dc_finite(k, 4) || !(cam->fx > 0.0) || !(cam->fy > 0.0))
        return isdf_fail(c, ISDF_ERR_INVALID_ARG, "view gain: bad camera intrinsics");
    if (P.stride_u < 1 || P.stride_v < 1 || !(P.max_range_m > 0.0) || !(P.max_range_m <= 1.7976931348623157e308) || P.scratch_bytes < 0)
        return isdf_fail(c, ISDF_ERR_INVALID_ARG, "bad view gain parameters (strides >= 1, a finite max_range_m > 0, scratch_bytes >= 0)");
    if (n_views < 0 || (n_views > 0 && (!poses || !rows))) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "bad view gain arguments");
    vg_rays_base(cam->width, cam->height, cam->fx, cam->fy, cam->cx, cam->cy, P.stride_u, P.stride_v, P.max_range_m, M, base);
    return ISDF_OK;
}

}  // namespace isdf

namespace {

int gain_check(isdf_ctx *c, const isdf_depth_camera *cam, const void *poses, long long n_views, const isdf_view_gain_params *params, const void *rows, MapGeom &M,
               isdf_view_gain_params &P, DcRays &base) {
    M = map_geom(c->grid);          // (without a map: zeros, and the state check below refuses)
    ISDF_TRY(gain_setup(c, cam, poses, n_views, params, rows, M, P, base));
    ISDF_TRY(map_query::single_device(c, "the view gain is not offered on a multi-device ctx"));
    ISDF_TRY(map_query::has_occupancy(c, "the view gain"));
    return map_query::has_known(c, "the view gain needs a known grid (isdf_map_known_enable)");
}

}  // namespace

namespace isdf {

// the launches on st: the table, then per chunk the clear of its seen grids and the gain kernel (and after_chunk, where one is given); with
// want_info the rows' pinned copy too
int gain_run(isdf_ctx *c, ViewGainState *S, const DcRays &base, const MapGeom &M, const isdf_view_gain_params &P, const double *d_poses, long long n_views,
             long long *d_rows, bool want_info, int *chunks_out, hipStream_t st, const GainChunkHook *after_chunk) {
    const long long n_words = (long long)c->known.n_words;
    const long long fit = P.scratch_bytes / (4 * n_words);
    const long long per_chunk = std::max<long long>(1, std::min<long long>(std::min<long long>(fit, n_views), VG_MAX_CHUNK));
    *chunks_out = 0;
    if (n_views > 0) {
        ISDF_TRY(S->d_views.reserve(c, (size_t)n_views));
        ISDF_TRY(S->d_seen.reserve(c, (size_t)per_chunk * (size_t)n_words));
        ISDF_TRY(S->d_zero.reserve(c, (size_t)base.width * base.height));
    }
    if (want_info) ISDF_TRY(S->h_rows.reserve(c, (size_t)std::max<long long>(n_views, 1) * VG_ROW));
    ISDF_TRY(map_query::count_begin(c, want_info, S->ev, st));
    if (n_views > 0) {
        HIPCHK(c, hipMemsetAsync(S->d_zero, 0, (size_t)base.width * base.height * sizeof(uint16_t), st));
        hipLaunchKernelGGL(vg_setup_kernel, dim3((unsigned)((n_views + VG_SETUP_BLOCK - 1) / VG_SETUP_BLOCK)), dim3(VG_SETUP_BLOCK), 0, st, d_poses, n_views, base, M,
                           S->d_views.get(), d_rows);
        HIPCHK(c, hipGetLastError());
        const long long n_rays = (long long)base.nu * base.nv;
        const unsigned bx = (unsigned)std::min<long long>((n_rays + VG_BLOCK - 1) / VG_BLOCK, 1024);
        for (long long v0 = 0; v0 < n_views; v0 += per_chunk) {
            const long long nv = std::min<long long>(per_chunk, n_views - v0);
            HIPCHK(c, hipMemsetAsync(S->d_seen, 0, (size_t)nv * (size_t)n_words * sizeof(unsigned), st));
            hipLaunchKernelGGL(vg_gain_kernel, dim3(bx, (unsigned)nv), dim3(VG_BLOCK), 0, st, (const VgView *)S->d_views.get(), v0, M, (const uint8_t *)c->d_occ.get(),
                               (const unsigned *)c->known.d_bits.get(), S->d_seen.get(), n_words, (const uint16_t *)S->d_zero.get(), d_rows);
            HIPCHK(c, hipGetLastError());
            ++*chunks_out;
            if (after_chunk) ISDF_TRY((*after_chunk)(v0, nv, S->d_seen.get(), n_words));
        }
    }
    ISDF_TRY(map_query::count_end(c, want_info, S->ev, st));
    if (want_info && n_views > 0) HIPCHK(c, hipMemcpyAsync(S->h_rows.get(), d_rows, (size_t)n_views * VG_ROW * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    return ISDF_OK;
}

}  // namespace isdf

namespace {

void gain_info(const int64_t *rows, long long n_views, const DcRays &base, int chunks, double ms, isdf_view_gain_info *out) {
    const VgBest B = vg_best(rows, n_views);
    isdf_view_gain_info info{};
    info.n_views = n_views; info.n_scored = B.n_scored; info.n_rays_per_view = (int64_t)base.nu * base.nv;
    info.best_view = B.best_view; info.best_gain = B.best_gain; info.gain_total = B.gain_total;
    info.chunks = chunks; info.gain_ms = ms;
    *out = info;
}

}  // namespace

extern "C" int isdf_view_gain_device(isdf_ctx *c, const isdf_depth_camera *cam, const double *d_poses, long long n_views, const isdf_view_gain_params *params,
                                     int64_t *d_rows_out, isdf_view_gain_info *info_out, void *stream) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    MapGeom M;
    isdf_view_gain_params P;
    DcRays base;
    ISDF_TRY(gain_check(c, cam, d_poses, n_views, params, d_rows_out, M, P, base));
    if (((uintptr_t)d_rows_out & 7u) != 0) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "the rows of the view gain must be 8-byte aligned");
    ViewGainState *S;
    ISDF_TRY(map_query::state_of(c, c->vgn, &S));
    const hipStream_t st = (hipStream_t)stream;
    int chunks = 0;
    ISDF_TRY(gain_run(c, S, base, M, P, d_poses, n_views, (long long *)d_rows_out, info_out != nullptr, &chunks, st));
    return map_query::info_after(c, info_out, st, [&](isdf_view_gain_info *out) { gain_info(S->h_rows.get(), n_views, base, chunks, S->ev.ms(0, 1), out); });
}

extern "C" int isdf_view_gain(isdf_ctx *c, const isdf_depth_camera *cam, const double *poses, long long n_views, const isdf_view_gain_params *params, int64_t *rows_out,
                              isdf_view_gain_info *info_out) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    MapGeom M;
    isdf_view_gain_params P;
    DcRays base;
    ISDF_TRY(gain_check(c, cam, poses, n_views, params, rows_out, M, P, base));
    ViewGainState *S;
    ISDF_TRY(map_query::state_of(c, c->vgn, &S));
    const hipStream_t st = c->stream;
    ISDF_TRY(S->d_poses.reserve(c, (size_t)n_views * 12));
    ISDF_TRY(S->d_rows.reserve(c, (size_t)n_views * VG_ROW));
    if (n_views > 0) HIPCHK(c, hipMemcpyAsync(S->d_poses, poses, (size_t)n_views * 12 * sizeof(double), hipMemcpyHostToDevice, st));
    int chunks = 0;
    ISDF_TRY(gain_run(c, S, base, M, P, S->d_poses.get(), n_views, S->d_rows.get(), true, &chunks, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (n_views > 0) std::memcpy(rows_out, S->h_rows.get(), (size_t)n_views * VG_ROW * sizeof(int64_t));
    if (info_out) gain_info(S->h_rows.get(), n_views, base, chunks, S->ev.ms(0, 1), info_out);
    return ISDF_OK;
}

extern "C" long long isdf_view_gain_host(const uint32_t *bits, const uint8_t *occ, const double bmin[3], const double bmax[3], double resolution, const int32_t dims[3],
                                         const isdf_depth_camera *cam, const double *poses, long long n_views, const isdf_view_gain_params *params, int64_t *rows_out,
                                         isdf_view_gain_info *info_out) {
    if (ms_geometry_bad(bmin, bmax, resolution, dims) || !bits || !occ) return isdf_fail(nullptr, ISDF_ERR_INVALID_ARG, "view gain (host form): bad arguments");
    const MapGeom M = map_geom(bmin, bmax, resolution, dims);
    isdf_view_gain_params P;
    DcRays base;
    ISDF_TRY(gain_setup(nullptr, cam, poses, n_views, params, rows_out, M, P, base));
    vg_gain_host(bits, occ, M, base, poses, n_views, rows_out);
    isdf_view_gain_info info{};
    gain_info(rows_out, n_views, base, 0, 0.0, &info);
    if (info_out) *info_out = info;
    return info.best_view;
}
