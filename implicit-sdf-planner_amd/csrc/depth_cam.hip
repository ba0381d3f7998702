// The depth camera: a depth image rendered from a cloud or from the map, and a depth image turned back into the rays
// isdf_integrate_scan takes - the sensor's side of the map chain.  The arithmetic is depth_cam_host.hpp's, one statement for both sides.
//   dc_render_cloud_kernel  one point per lane, grid-stride: dc_project, then the window.  A window of at most DC_WAVE_AREA pixels is
//                           written by its own lane; the larger ones are then taken one after the other by the whole wavefront, the
//                           owner's window broadcast by cross-lane reads and its pixels dealt out lane by lane along the rows, so that a
//                           near point (r = 22: 2 025 pixels) costs its wavefront 32 rounds and not 2 025.  A pixel is read first and the
//                           atomic minimum left out when the value there is nearer already: depths only fall during the kernel, so a
//                           stale read costs an atomic, never a pixel.
//   dc_render_map_kernel    the same splat over the centres of the occupied voxels: one dword of occupancy bytes per lane, one pass.
//   dc_rays_kernel          one ray per lane: dc_ray, 12 + 1 bytes out.
// The image is cleared by a 32-bit fill on the same stream.  The counters are summed in the wavefront, through LDS, then one set of
// atomics per workgroup into the call's 64-byte record; with info_out == NULL the kernels count nothing and nothing is handed over.
// Built with -ffp-contract=off: the projection and the unprojection are held to their host forms byte for byte.
#include "map_query.hpp"
#include "depth_cam_host.hpp"
#include "map_change.hpp"
#include "dev_reduce.hpp"
#include <algorithm>
#include <cstring>

namespace isdf {

struct DcRecord { unsigned long long v[8]; };           // render: n_points, n_behind, n_outside, n_near, n_splat_pixels, n_pixels_set; rays: DcRaysCounts' five after n_pixels
static_assert(sizeof(DcRecord) == 64, "the hand-over record is one 64-byte line");

constexpr int DC_BLOCK = 256;
constexpr int DC_WAVES = DC_BLOCK / 64;
#ifndef ISDF_DC_WAVE_AREA
#define ISDF_DC_WAVE_AREA 64                // developer switch (Makefile EXTRA, tools/depth_cam_bench.py --lib): 0x7FFFFFFF = every window by its own lane
#endif
constexpr int DC_WAVE_AREA = ISDF_DC_WAVE_AREA;         // windows above this many pixels go to the whole wavefront
constexpr int DC_COUNTERS = 6;

struct DcMap { double bmin[3]; double res; int Y, Z; long long n_vox; };

template <bool COUNT> __device__ __forceinline__ void dc_pixel(int32_t *__restrict__ image, size_t i, int dist, unsigned long long &set) {
    if (image[i] <= dist) return;
    if (COUNT) set += atomicMin(&image[i], dist) == DC_EMPTY;       // exactly one minimum finds the pixel untouched
    else atomicMin(&image[i], dist);
}

// One point per lane (drawn: this lane holds a window), called by every lane of the wavefront together.
template <bool COUNT> __device__ __forceinline__ void dc_splat(bool drawn, const DcWindow &W, int32_t *__restrict__ image, int width, unsigned long long cnt[DC_COUNTERS]) {
    const int lane = threadIdx.x & 63;
    const int ww = W.x1 - W.x0 + 1;
    const int area = drawn ? ww * (W.y1 - W.y0 + 1) : 0;
    if (COUNT) cnt[4] += (unsigned long long)area;
    const bool big = area > DC_WAVE_AREA;
    if (drawn && !big)
        for (int y = W.y0; y <= W.y1; y++)
            for (int x = W.x0; x <= W.x1; x++) dc_pixel<COUNT>(image, (size_t)y * width + x, W.dist, cnt[5]);
    unsigned long long todo = __ballot(big);
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int x0 = __shfl(W.x0, src, 64), y0 = __shfl(W.y0, src, 64), w = __shfl(ww, src, 64), n = __shfl(area, src, 64), dist = __shfl(W.dist, src, 64);
        const int dy = 64 / w, dx = 64 - dy * w;            // 64 pixels further on: dy rows down, dx columns right
        int y = lane / w, x = lane - y * w;
        for (int k = lane; k < n; k += 64) {
            dc_pixel<COUNT>(image, (size_t)(y0 + y) * width + (x0 + x), dist, cnt[5]);
            y += dy; x += dx;
            if (x >= w) { x -= w; y++; }
        }
    }
}

__device__ __forceinline__ void dc_count_drop(int why, unsigned long long cnt[DC_COUNTERS]) {
    cnt[1] += why == DC_BEHIND; cnt[2] += why == DC_OUTSIDE; cnt[3] += why == DC_NEAR;
}

template <bool COUNT> __global__ __launch_bounds__(DC_BLOCK) void dc_render_cloud_kernel(const float *__restrict__ xyz, long long n, DcCam K, int32_t *__restrict__ image,
                                                                                          DcRecord *__restrict__ rec) {
    unsigned long long cnt[DC_COUNTERS] = {0, 0, 0, 0, 0, 0};
    const int lane = threadIdx.x & 63;
    // the wavefront's first point: every lane of it takes the same number of turns
    for (long long base = (long long)blockIdx.x * DC_BLOCK + (threadIdx.x - lane); base < n; base += (long long)gridDim.x * DC_BLOCK) {
        const long long i = base + lane;
        DcWindow W{0, 0, 0, 0, 0};
        bool drawn = false;
        if (i < n) {
            const int why = dc_project(K, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], W);
            drawn = why == DC_DRAWN;
            if (COUNT) { cnt[0]++; dc_count_drop(why, cnt); }
        }
        dc_splat<COUNT>(drawn, W, image, K.width, cnt);
    }
    if (COUNT) {                // (uniform) every thread of the workgroup is here
        const unsigned long long s = block_sum<DC_COUNTERS, DC_WAVES>(cnt);
        if (s) atomicAdd(&rec->v[threadIdx.x], s);          // (s is 0 beyond the counters)
    }
}

// occ as dwords (the ctx allocates it in whole dwords): lane t holds voxels 4 t .. 4 t + 3
template <bool COUNT> __global__ __launch_bounds__(DC_BLOCK) void dc_render_map_kernel(const unsigned *__restrict__ occ4, DcMap M, DcCam K, int32_t *__restrict__ image,
                                                                                        DcRecord *__restrict__ rec) {
    unsigned long long cnt[DC_COUNTERS] = {0, 0, 0, 0, 0, 0};
    const int lane = threadIdx.x & 63;
    const long long n_words = (M.n_vox + 3) >> 2;
    for (long long base = (long long)blockIdx.x * DC_BLOCK + (threadIdx.x - lane); base < n_words; base += (long long)gridDim.x * DC_BLOCK) {
        const long long t = base + lane;
        const unsigned word = t < n_words ? occ4[t] : 0u;
        if (!__ballot(word != 0u)) continue;                // (uniform) 256 free voxels
        for (int b = 0; b < 4; b++) {
            const long long a = 4 * t + b;
            const bool occupied = ((word >> (8 * b)) & 0xFFu) != 0u && a < M.n_vox;
            if (!__ballot(occupied)) continue;
            DcWindow W{0, 0, 0, 0, 0};
            bool drawn = false;
            if (occupied) {
                const long long xy = a / M.Z;
                float c[3];
                dc_voxel_centre(M.bmin, M.res, (int)(xy / M.Y), (int)(xy % M.Y), (int)(a - xy * M.Z), c);
                const int why = dc_project(K, c[0], c[1], c[2], W);
                drawn = why == DC_DRAWN;
                if (COUNT) { cnt[0]++; dc_count_drop(why, cnt); }
            }
            dc_splat<COUNT>(drawn, W, image, K.width, cnt);
        }
    }
    if (COUNT) {                // (uniform) every thread of the workgroup is here
        const unsigned long long s = block_sum<DC_COUNTERS, DC_WAVES>(cnt);
        if (s) atomicAdd(&rec->v[threadIdx.x], s);          // (s is 0 beyond the counters)
    }
}

__global__ __launch_bounds__(DC_BLOCK) void dc_rays_kernel(DcRays Q, const void *__restrict__ image, float *__restrict__ ends, uint8_t *__restrict__ hit, DcRecord *__restrict__ rec) {
    unsigned long long cnt[DC_COUNTERS] = {0, 0, 0, 0, 0, 0};
    const long long n = (long long)Q.nu * Q.nv;
    for (long long k = (long long)blockIdx.x * DC_BLOCK + threadIdx.x; k < n; k += (long long)gridDim.x * DC_BLOCK) {
        const int iv = (int)(k / Q.nu), iu = (int)(k - (long long)iv * Q.nu);
        float e[3];
        uint8_t h;
        const int flags = dc_ray(Q, image, iu, iv, e, h);
        ends[3 * k] = e[0]; ends[3 * k + 1] = e[1]; ends[3 * k + 2] = e[2];
        hit[k] = h;
        cnt[1] += (flags & DC_RAY_NO_RETURN) != 0; cnt[2] += (flags & DC_RAY_BELOW_MIN) != 0; cnt[3] += (flags & DC_RAY_TRUNCATED) != 0;
        cnt[4] += (flags & DC_RAY_CLIPPED) != 0; cnt[5] += (flags & DC_RAY_HIT) != 0;
    }
    if (!rec) return;           // (uniform) the caller wants no counters
    const unsigned long long s = block_sum<DC_COUNTERS, DC_WAVES>(cnt);
    if (s) atomicAdd(&rec->v[threadIdx.x], s);
}

}  // namespace isdf

// staging of the host-pointer forms, the record and its pinned copy
struct DepthCamState {
    isdf::DevBuf<void> d_in;                    // a cloud, or a depth image
    isdf::DevBuf<int32_t> d_image;              // the rendered image
    isdf::DevBuf<void> d_rays;                  // end points | hit bytes
    isdf::RecPair<isdf::DcRecord> rec;
    isdf::DevEvents<2> ev;
    int ready(isdf_ctx *c) { ISDF_TRY(ev.ready(c)); return rec.ready(c); }
};

using namespace isdf;

extern "C" void isdf_depth_render_params_default(isdf_depth_render_params *p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->splat_m = 0.0573;
    p->source = ISDF_DEPTH_SOURCE_CLOUD;
}

extern "C" void isdf_depth_rays_params_default(isdf_depth_rays_params *p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->stride_u = p->stride_v = 1;
    p->max_range_m = HUGE_VAL;
}

extern "C" void isdf_depth_render_sizes(int sizes_out[3]) {
    if (!sizes_out) return;
    sizes_out[0] = (int)sizeof(isdf_depth_camera); sizes_out[1] = (int)sizeof(isdf_depth_render_params); sizes_out[2] = (int)sizeof(isdf_depth_render_info);
}

extern "C" void isdf_depth_rays_sizes(int sizes_out[2]) {
    if (!sizes_out) return;
    sizes_out[0] = (int)sizeof(isdf_depth_rays_params); sizes_out[1] = (int)sizeof(isdf_depth_rays_info);
}

namespace {

// ---- what the device and the host forms check and set up alike (c may be null: the host forms)
int render_setup(isdf_ctx *c, const isdf_depth_camera *cam, const double *cam2world, const isdf_depth_render_params *params, isdf_depth_render_params &P, DcCam &K) {
    P = map_query::resolve(params, isdf_depth_render_params_default);
    if (!cam || dc_camera_bad(cam->width, cam->height, cam->fx, cam->fy, cam->cx, cam->cy, cam2world)) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "depth camera: bad intrinsics or pose");
    if (!(P.splat_m >= 0.0) || !(P.splat_m <= 1e300) || !(P.min_depth_m >= 0.0) || !(P.min_depth_m <= 1e30) || P.max_splat_px < 0 ||
        (P.source != ISDF_DEPTH_SOURCE_CLOUD && P.source != ISDF_DEPTH_SOURCE_MAP))
        return isdf_fail(c, ISDF_ERR_INVALID_ARG, "bad depth render parameters");
    K.width = cam->width; K.height = cam->height;
    K.fx = (float)cam->fx; K.fy = (float)cam->fy; K.cx = cam->cx; K.cy = cam->cy;
    dc_world2cam(cam2world, K.w2c);
    K.splat = P.splat_m; K.min_depth = (float)P.min_depth_m; K.max_splat = P.max_splat_px;
    return ISDF_OK;
}

int rays_setup(isdf_ctx *c, const isdf_depth_camera *cam, const double *cam2world, int format, const isdf_depth_rays_params *params, const MapGeom &M, DcRays &Q) {
    const isdf_depth_rays_params P = map_query::resolve(params, isdf_depth_rays_params_default);
    if (!cam || dc_camera_bad(cam->width, cam->height, cam->fx, cam->fy, cam->cx, cam->cy, cam2world)) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "depth camera: bad intrinsics or pose");
    if (format != ISDF_DEPTH_I32_MM && format != ISDF_DEPTH_U16_MM && format != ISDF_DEPTH_F32_M) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "unknown depth image format");
    if (P.stride_u < 1 || P.stride_v < 1 || !(P.min_range_m >= 0.0) || !(P.max_range_m > 0.0) || (P.no_return_is_free && !(P.max_range_m <= 1.7976931348623157e308)))
        return isdf_fail(c, ISDF_ERR_INVALID_ARG, "bad depth ray parameters (no_return_is_free needs a finite max_range_m)");
    int q[3];
    if (!ms_quantize(M, cam2world[3], cam2world[7], cam2world[11], q)) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "the camera lies outside the map");
    dc_rays_setup(cam->width, cam->height, cam->fx, cam->fy, cam->cx, cam->cy, cam2world, format, P.stride_u, P.stride_v, P.min_range_m, P.max_range_m,
                  P.no_return_is_free != 0, M, Q);
    return ISDF_OK;
}

size_t pixel_bytes(int format) { return format == ISDF_DEPTH_U16_MM ? 2 : 4; }

// ---- the render: the clear, the launch and, with counters, the record on its way to the host
int render_check(isdf_ctx *c, const isdf_depth_camera *cam, const double *cam2world, const void *xyz, long long n, const isdf_depth_render_params *params, const void *image,
                 isdf_depth_render_params &P, DcCam &K) {
    ISDF_TRY(render_setup(c, cam, cam2world, params, P, K));
    if (!image || (P.source == ISDF_DEPTH_SOURCE_CLOUD && (n < 0 || (n > 0 && !xyz)))) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "bad depth render arguments");
    ISDF_TRY(map_query::single_device(c, "the depth render is not offered on a multi-device ctx"));
    return P.source == ISDF_DEPTH_SOURCE_MAP ? map_query::has_occupancy(c, "rendering the map") : ISDF_OK;
}

int render_run(isdf_ctx *c, DepthCamState *S, const DcCam &K, const isdf_depth_render_params &P, const float *d_xyz, long long n, int32_t *d_image, bool count, hipStream_t st) {
    ISDF_TRY(map_query::count_begin(c, count, S->ev, S->rec, st));
    HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)d_image, DC_EMPTY, (size_t)K.width * K.height, st));
    DcRecord *const rec = count ? S->rec.dev() : nullptr;
    if (P.source == ISDF_DEPTH_SOURCE_MAP) {
        const DevGrid &G = c->grid;
        DcMap M;
        for (int a = 0; a < 3; a++) M.bmin[a] = G.bmin[a];
        M.res = G.res; M.Y = G.Y; M.Z = G.Z; M.n_vox = (long long)G.X * G.Y * G.Z;
        const unsigned blocks = (unsigned)std::min<long long>((((M.n_vox + 3) >> 2) + DC_BLOCK - 1) / DC_BLOCK, 4096);
        const unsigned *const occ4 = (const unsigned *)c->d_occ.get();
        if (count) hipLaunchKernelGGL(dc_render_map_kernel<true>, dim3(blocks), dim3(DC_BLOCK), 0, st, occ4, M, K, d_image, rec);
        else hipLaunchKernelGGL(dc_render_map_kernel<false>, dim3(blocks), dim3(DC_BLOCK), 0, st, occ4, M, K, d_image, rec);
        HIPCHK(c, hipGetLastError());
    } else if (n > 0) {
        const unsigned blocks = (unsigned)std::min<long long>((n + DC_BLOCK - 1) / DC_BLOCK, 4096);
        if (count) hipLaunchKernelGGL(dc_render_cloud_kernel<true>, dim3(blocks), dim3(DC_BLOCK), 0, st, d_xyz, n, K, d_image, rec);
        else hipLaunchKernelGGL(dc_render_cloud_kernel<false>, dim3(blocks), dim3(DC_BLOCK), 0, st, d_xyz, n, K, d_image, rec);
        HIPCHK(c, hipGetLastError());
    }
    return map_query::count_end(c, count, S->ev, S->rec, st);
}

void render_info(const DepthCamState *S, isdf_depth_render_info *out) {
    const DcRecord R = S->rec.host();
    isdf_depth_render_info info{};
    info.n_points = (int64_t)R.v[0]; info.n_behind = (int64_t)R.v[1]; info.n_outside = (int64_t)R.v[2]; info.n_near = (int64_t)R.v[3];
    info.n_splat_pixels = (int64_t)R.v[4]; info.n_pixels_set = (int64_t)R.v[5];
    info.render_ms = S->ev.ms(0, 1);
    *out = info;
}

// ---- the rays
int rays_check(isdf_ctx *c, const isdf_depth_camera *cam, const double *cam2world, const void *image, int format, const isdf_depth_rays_params *params, const void *ends,
               const void *hit, DcRays &Q) {
    if (!image || !ends || !hit) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "bad depth ray arguments");
    if (!c->have_geom) return isdf_fail(c, ISDF_ERR_STATE, "depth rays need a map: its box clips them");
    return rays_setup(c, cam, cam2world, format, params, map_geom(c->grid), Q);
}

int rays_run(isdf_ctx *c, DepthCamState *S, const DcRays &Q, const void *d_image, float *d_ends, uint8_t *d_hit, bool count, hipStream_t st) {
    ISDF_TRY(map_query::count_begin(c, count, S->ev, S->rec, st));
    const long long n = (long long)Q.nu * Q.nv;
    const unsigned blocks = (unsigned)std::min<long long>((n + DC_BLOCK - 1) / DC_BLOCK, 8192);
    hipLaunchKernelGGL(dc_rays_kernel, dim3(blocks), dim3(DC_BLOCK), 0, st, Q, d_image, d_ends, d_hit, count ? S->rec.dev() : nullptr);
    HIPCHK(c, hipGetLastError());
    return map_query::count_end(c, count, S->ev, S->rec, st);
}

void rays_info(const DepthCamState *S, const DcRays &Q, isdf_depth_rays_info *out) {
    const DcRecord R = S->rec.host();
    isdf_depth_rays_info info{};
    info.n_pixels = (int64_t)Q.nu * Q.nv;
    info.n_no_return = (int64_t)R.v[1]; info.n_below_min = (int64_t)R.v[2]; info.n_truncated = (int64_t)R.v[3]; info.n_clipped = (int64_t)R.v[4]; info.n_hits = (int64_t)R.v[5];
    info.rays_ms = S->ev.ms(0, 1);
    *out = info;
}

struct DepthProduce { DepthCamState *S; const DcRays *Q; };

// the scan's rays written by the unprojection into the scan's own staged input (scan_integrate's in.produce)
int produce_rays(isdf_ctx *c, float *d_xyz, uint8_t *d_hit, void *arg) {
    const DepthProduce *const D = (const DepthProduce *)arg;
    return rays_run(c, D->S, *D->Q, D->S->d_in.get(), d_xyz, d_hit, true, c->stream);
}

}  // namespace

extern "C" int isdf_depth_render_device(isdf_ctx *c, const isdf_depth_camera *cam, const double cam2world[12], const float *d_xyz, long long n,
                                        const isdf_depth_render_params *params, int32_t *d_image_out, isdf_depth_render_info *info_out, void *stream) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    isdf_depth_render_params P;
    DcCam K;
    ISDF_TRY(render_check(c, cam, cam2world, d_xyz, n, params, d_image_out, P, K));
    DepthCamState *S;
    ISDF_TRY(map_query::state_of(c, c->dcm, &S));
    const hipStream_t st = (hipStream_t)stream;
    ISDF_TRY(render_run(c, S, K, P, d_xyz, n, d_image_out, info_out != nullptr, st));
    return map_query::info_after(c, info_out, st, [&](isdf_depth_render_info *out) { render_info(S, out); });
}

extern "C" int isdf_depth_render(isdf_ctx *c, const isdf_depth_camera *cam, const double cam2world[12], const float *xyz, long long n, const isdf_depth_render_params *params,
                                 int32_t *image_out, isdf_depth_render_info *info_out) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    isdf_depth_render_params P;
    DcCam K;
    ISDF_TRY(render_check(c, cam, cam2world, xyz, n, params, image_out, P, K));
    DepthCamState *S;
    ISDF_TRY(map_query::state_of(c, c->dcm, &S));
    const hipStream_t st = c->stream;
    const bool cloud = P.source == ISDF_DEPTH_SOURCE_CLOUD;
    const size_t pixels = (size_t)K.width * K.height;
    ISDF_TRY(S->d_image.reserve(c, pixels));
    if (cloud) {
        ISDF_TRY(S->d_in.reserve(c, (size_t)n * 3 * sizeof(float)));
        if (n > 0) HIPCHK(c, hipMemcpyAsync(S->d_in, xyz, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice, st));
    }
    ISDF_TRY(render_run(c, S, K, P, (const float *)S->d_in.get(), cloud ? n : 0, S->d_image.get(), true, st));
    HIPCHK(c, hipMemcpyAsync(image_out, S->d_image, pixels * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (info_out) render_info(S, info_out);
    return ISDF_OK;
}

extern "C" int isdf_depth_render_host(const isdf_depth_camera *cam, const double cam2world[12], const float *xyz, long long n, const uint8_t *occ, const double bmin[3],
                                      double resolution, const int32_t dims[3], const isdf_depth_render_params *params, int32_t *image_out, isdf_depth_render_info *info_out) {
    isdf_depth_render_params P;
    DcCam K;
    ISDF_TRY(render_setup(nullptr, cam, cam2world, params, P, K));
    if (!image_out) return isdf_fail(nullptr, ISDF_ERR_INVALID_ARG, "depth render (host form): bad arguments");
    DcRenderCounts C;
    if (P.source == ISDF_DEPTH_SOURCE_MAP) {
        if (!occ || !bmin || !dims || !(resolution > 0.0) || !(resolution <= 1.7976931348623157e308)) return isdf_fail(nullptr, ISDF_ERR_INVALID_ARG, "depth render (host form): bad map");
        for (int a = 0; a < 3; a++)
            if (dims[a] < 1 || dims[a] > 4096 || !(bmin[a] - bmin[a] == 0.0)) return isdf_fail(nullptr, ISDF_ERR_INVALID_ARG, "depth render (host form): bad map");
        dc_render_map_host(K, occ, bmin, resolution, dims, image_out, C);
    } else {
        if (n < 0 || (n > 0 && !xyz)) return isdf_fail(nullptr, ISDF_ERR_INVALID_ARG, "depth render (host form): bad arguments");
        dc_render_cloud_host(K, xyz, n, image_out, C);
    }
    if (info_out) {
        isdf_depth_render_info info{};
        info.n_points = C.n_points; info.n_behind = C.n_behind; info.n_outside = C.n_outside; info.n_near = C.n_near;
        info.n_splat_pixels = C.n_splat_pixels; info.n_pixels_set = C.n_pixels_set;
        *info_out = info;
    }
    return ISDF_OK;
}

extern "C" long long isdf_depth_rays_rows(const isdf_depth_camera *cam, const isdf_depth_rays_params *params) {
    const int su = params ? params->stride_u : 1, sv = params ? params->stride_v : 1;
    if (!cam || cam->width < 1 || cam->width > DC_MAX_DIM || cam->height < 1 || cam->height > DC_MAX_DIM || su < 1 || sv < 1) return ISDF_ERR_INVALID_ARG;
    return (long long)((cam->width + su - 1) / su) * ((cam->height + sv - 1) / sv);
}

extern "C" int isdf_depth_rays_device(isdf_ctx *c, const isdf_depth_camera *cam, const double cam2world[12], const void *d_image, int format,
                                      const isdf_depth_rays_params *params, float *d_ends_out, uint8_t *d_hit_out, isdf_depth_rays_info *info_out, void *stream) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    DcRays Q;
    ISDF_TRY(rays_check(c, cam, cam2world, d_image, format, params, d_ends_out, d_hit_out, Q));
    ISDF_TRY(map_query::single_device(c, "depth rays on the device are not offered on a multi-device ctx"));
    DepthCamState *S;
    ISDF_TRY(map_query::state_of(c, c->dcm, &S));
    const hipStream_t st = (hipStream_t)stream;
    ISDF_TRY(rays_run(c, S, Q, d_image, d_ends_out, d_hit_out, info_out != nullptr, st));
    return map_query::info_after(c, info_out, st, [&](isdf_depth_rays_info *out) { rays_info(S, Q, out); });
}

extern "C" int isdf_depth_rays(isdf_ctx *c, const isdf_depth_camera *cam, const double cam2world[12], const void *image, int format, const isdf_depth_rays_params *params,
                               float *ends_out, uint8_t *hit_out, isdf_depth_rays_info *info_out) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    DcRays Q;
    ISDF_TRY(rays_check(c, cam, cam2world, image, format, params, ends_out, hit_out, Q));
    ISDF_TRY(map_query::single_device(c, "depth rays on the device are not offered on a multi-device ctx"));
    DepthCamState *S;
    ISDF_TRY(map_query::state_of(c, c->dcm, &S));
    const hipStream_t st = c->stream;
    const size_t n = (size_t)Q.nu * Q.nv, image_bytes = (size_t)Q.width * Q.height * pixel_bytes(format);
    ISDF_TRY(S->d_in.reserve(c, image_bytes));
    ISDF_TRY(S->d_rays.reserve(c, n * 13));
    float *const d_ends = (float *)S->d_rays.get();
    uint8_t *const d_hit = (uint8_t *)S->d_rays.get() + n * 12;
    HIPCHK(c, hipMemcpyAsync(S->d_in, image, image_bytes, hipMemcpyHostToDevice, st));
    ISDF_TRY(rays_run(c, S, Q, S->d_in.get(), d_ends, d_hit, true, st));
    HIPCHK(c, hipMemcpyAsync(ends_out, d_ends, n * 12, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(hit_out, d_hit, n, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (info_out) rays_info(S, Q, info_out);
    return ISDF_OK;
}

extern "C" long long isdf_depth_rays_host(const isdf_depth_camera *cam, const double cam2world[12], const void *image, int format, const isdf_depth_rays_params *params,
                                          const double bmin[3], const double bmax[3], double resolution, const int32_t dims[3], float *ends_out, uint8_t *hit_out,
                                          isdf_depth_rays_info *info_out) {
    if (ms_geometry_bad(bmin, bmax, resolution, dims) || !image || !ends_out || !hit_out) return isdf_fail(nullptr, ISDF_ERR_INVALID_ARG, "depth rays (host form): bad arguments");
    DcRays Q;
    ISDF_TRY(rays_setup(nullptr, cam, cam2world, format, params, map_geom(bmin, bmax, resolution, dims), Q));
    DcRaysCounts C;
    dc_rays_host(Q, image, ends_out, hit_out, C);
    if (info_out) {
        isdf_depth_rays_info info{};
        info.n_pixels = C.n_pixels; info.n_no_return = C.n_no_return; info.n_below_min = C.n_below_min; info.n_truncated = C.n_truncated; info.n_clipped = C.n_clipped;
        info.n_hits = C.n_hits;
        *info_out = info;
    }
    return C.n_hits;
}

extern "C" int isdf_integrate_depth(isdf_ctx *c, const isdf_depth_camera *cam, const double cam2world[12], const void *image, int format,
                                    const isdf_depth_rays_params *rays_params, const isdf_map_scan_params *scan_params, isdf_depth_rays_info *depth_info_out,
                                    isdf_map_scan_info *scan_info_out) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    if (!image || !cam || !cam2world) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "integrating a depth image: bad arguments");
    const double origin[3] = {cam2world[3], cam2world[7], cam2world[11]};
    isdf_map_scan_params P;
    MsOrigin O;
    ISDF_TRY(scan_check(c, "integrating a depth image", origin, image, 1, scan_params, P, O));
    DcRays Q;
    ISDF_TRY(rays_setup(c, cam, cam2world, format, rays_params, map_geom(c->grid), Q));
    DepthCamState *S;
    ISDF_TRY(map_query::state_of(c, c->dcm, &S));
    const size_t image_bytes = (size_t)Q.width * Q.height * pixel_bytes(format);
    ISDF_TRY(S->d_in.reserve(c, image_bytes));
    HIPCHK(c, hipMemcpyAsync(S->d_in, image, image_bytes, hipMemcpyHostToDevice, c->stream));
    DepthProduce D{S, &Q};
    // the scan's first hand-over synchronises the stream: the rays' record is on the host when it returns
    ISDF_TRY(scan_integrate(c, O, MsInput{nullptr, nullptr, produce_rays, &D}, (long long)Q.nu * Q.nv, P, scan_info_out));
    if (depth_info_out) rays_info(S, Q, depth_info_out);
    return ISDF_OK;
}
