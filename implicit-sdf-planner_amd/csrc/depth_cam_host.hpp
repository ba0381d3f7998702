// The depth camera's arithmetic (depth_cam.hip), free of HIP so that a plain C++ program can run it under a sanitizer.
// The functions marked MU_HD are the ones the kernels call: one statement of the projection and of the unprojection for both sides,
// as map_scan_host.hpp is one statement of the ray.  Nothing here may be contracted into an FMA: the library builds this header with
// -ffp-contract=off, and only + - * / and sqrt appear, so the host forms and the kernels agree byte for byte.
//
// Render (the reference's `render`, local_sensing/src/depth_render.cu:2-43): the point goes through world2cam in float32 in the source's
// order, x * r0 + y * r1 + z * r2 + t per row; the projection is (double)(x / z * fx_f) + c + 0.5 truncated towards zero, so a value
// in (-1, 0) lands in column (row) 0, as the reference's double-to-int conversion does; the splat is the (2 r + 1)^2 window round the
// pixel, clipped to the image, each pixel taking the minimum of the millimetre depths offered to it.
// Rays (render_pcl_world, pcl_render_node.cpp:224-269): a pixel's depth back to a world point in fp64, cut to range and clipped to the
// map's box shrunk by half a voxel, rounded to float32 once at the end.
#pragma once
#include "map_scan_host.hpp"
#include <cmath>
#include <cstdint>
#include <cstring>

namespace isdf {

constexpr int DC_EMPTY = 999999;            // depth_initial's value: nothing reached the pixel
constexpr int DC_NO_RETURN_MM = 500000;     // pcl_render_node.cpp:293: a rendered depth of 500 m or more is no return
constexpr int DC_MAX_DIM = 4096;
constexpr int DC_FORMAT_I32_MM = 0, DC_FORMAT_U16_MM = 1, DC_FORMAT_F32_M = 2;

// ---- the camera as the render reads it
struct DcCam {
    int width, height;
    float fx, fy;               // the reference's Parameter holds floats
    double cx, cy;
    float w2c[12];              // rows (r0 r1 r2 t) of world2cam, rounded to float32 once on the host
    double splat;               // splat_m
    float min_depth;
    int max_splat;              // 0: unlimited
};

inline bool dc_finite(const double *v, int n) {
    for (int i = 0; i < n; i++) if (!(v[i] - v[i] == 0.0)) return false;
    return true;
}

inline bool dc_camera_bad(int width, int height, double fx, double fy, double cx, double cy, const double *cam2world) {
    const double k[4] = {fx, fy, cx, cy};
    return !cam2world || width < 1 || width > DC_MAX_DIM || height < 1 || height > DC_MAX_DIM || !dc_finite(k, 4) || !(fx > 0.0) || !(fy > 0.0) || !dc_finite(cam2world, 12);
}

// world2cam = (R^T, -R^T t) of the rigid cam2world (rows (R | t), row-major), formed in fp64, rounded to float32
inline void dc_world2cam(const double c2w[12], float w2c[12]) {
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) w2c[4 * i + j] = (float)c2w[4 * j + i];
        w2c[4 * i + 3] = (float)-(c2w[i] * c2w[3] + c2w[4 + i] * c2w[7] + c2w[8 + i] * c2w[11]);
    }
}

struct DcWindow { int x0, x1, y0, y1, dist; };         // the clipped window (inclusive) and the depth in millimetres
constexpr int DC_DRAWN = 0, DC_BEHIND = 1, DC_NEAR = 2, DC_OUTSIDE = 3;

// one point: DC_DRAWN and its window, or why it is dropped.  z <= 0 and a NaN z are behind; the centre pixel must lie in the image
// (depth_render.cu:23); a depth that does not fit an int32 is INT32_MAX (it changes no pixel); r >= 4096 covers every image.
MU_HD int dc_project(const DcCam &K, float x, float y, float z, DcWindow &W) {
    const float tx = x * K.w2c[0] + y * K.w2c[1] + z * K.w2c[2] + K.w2c[3];
    const float ty = x * K.w2c[4] + y * K.w2c[5] + z * K.w2c[6] + K.w2c[7];
    const float tz = x * K.w2c[8] + y * K.w2c[9] + z * K.w2c[10] + K.w2c[11];
    if (!(tz > 0.0f)) return DC_BEHIND;
    if (tz < K.min_depth) return DC_NEAR;
    const double pxd = (double)(tx / tz * K.fx) + K.cx + 0.5;
    const double pyd = (double)(ty / tz * K.fy) + K.cy + 0.5;
    if (!(pxd > -1.0 && pxd < (double)K.width && pyd > -1.0 && pyd < (double)K.height)) return DC_OUTSIDE;
    const int px = (int)pxd, py = (int)pyd;             // truncation: (-1, 0) -> 0
    const float mm = tz * 1000.0f + 0.5f;
    W.dist = mm < 2147483648.0f ? (int)mm : 0x7FFFFFFF;
    const double rd = K.splat * (double)K.fx / (double)tz + (double)0.5f;      // depth_render.cu:32: double * float / float + float
    int r = rd < 4096.0 ? (int)rd : 4096;
    if (K.max_splat > 0 && r > K.max_splat) r = K.max_splat;
    W.x0 = px - r < 0 ? 0 : px - r;
    W.x1 = px + r > K.width - 1 ? K.width - 1 : px + r;
    W.y0 = py - r < 0 ? 0 : py - r;
    W.y1 = py + r > K.height - 1 ? K.height - 1 : py + r;
    return DC_DRAWN;
}

// the centre of voxel (x, y, z): bmin + (v + 0.5) * res in fp64, rounded to float32
MU_HD void dc_voxel_centre(const double bmin[3], double res, int x, int y, int z, float c[3]) {
    c[0] = (float)(bmin[0] + ((double)x + 0.5) * res);
    c[1] = (float)(bmin[1] + ((double)y + 0.5) * res);
    c[2] = (float)(bmin[2] + ((double)z + 0.5) * res);
}

struct DcRenderCounts { long long n_points = 0, n_behind = 0, n_outside = 0, n_near = 0, n_splat_pixels = 0, n_pixels_set = 0; };

inline void dc_render_point_host(const DcCam &K, float x, float y, float z, int32_t *image, DcRenderCounts &C) {
    DcWindow W;
    C.n_points++;
    switch (dc_project(K, x, y, z, W)) {
    case DC_BEHIND: C.n_behind++; return;
    case DC_NEAR: C.n_near++; return;
    case DC_OUTSIDE: C.n_outside++; return;
    default: break;
    }
    C.n_splat_pixels += (long long)(W.x1 - W.x0 + 1) * (W.y1 - W.y0 + 1);
    for (int yy = W.y0; yy <= W.y1; yy++)
        for (int xx = W.x0; xx <= W.x1; xx++) {
            int32_t &p = image[(size_t)yy * K.width + xx];
            if (W.dist < p) p = W.dist;
        }
}

inline void dc_image_begin_host(const DcCam &K, int32_t *image) {
    for (size_t i = 0, n = (size_t)K.width * K.height; i < n; i++) image[i] = DC_EMPTY;
}
inline void dc_image_end_host(const DcCam &K, const int32_t *image, DcRenderCounts &C) {
    for (size_t i = 0, n = (size_t)K.width * K.height; i < n; i++) C.n_pixels_set += image[i] != DC_EMPTY;
}

// the image of a cloud (n x 3 floats)
inline void dc_render_cloud_host(const DcCam &K, const float *xyz, long long n, int32_t *image, DcRenderCounts &C) {
    C = DcRenderCounts();
    dc_image_begin_host(K, image);
    for (long long i = 0; i < n; i++) dc_render_point_host(K, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], image, C);
    dc_image_end_host(K, image, C);
}

// the image of the centres of the occupied voxels (occ: X * Y * Z bytes, z fastest)
inline void dc_render_map_host(const DcCam &K, const uint8_t *occ, const double bmin[3], double res, const int32_t dims[3], int32_t *image, DcRenderCounts &C) {
    C = DcRenderCounts();
    dc_image_begin_host(K, image);
    size_t a = 0;
    for (int x = 0; x < dims[0]; x++)
        for (int y = 0; y < dims[1]; y++)
            for (int z = 0; z < dims[2]; z++, a++) {
                if (!occ[a]) continue;
                float c[3];
                dc_voxel_centre(bmin, res, x, y, z, c);
                dc_render_point_host(K, c[0], c[1], c[2], image, C);
            }
    dc_image_end_host(K, image, C);
}

// ---- the unprojection
struct DcRays {
    int width, height, su, sv, nu, nv;          // nu = ceil(width / su) columns and nv rows of rays
    int format, free_no_return;
    double fx, fy, cx, cy;
    double R[9], t[3];                          // cam2world in fp64, as given
    double min_range, max_range;
    double lo[3], hi[3];                        // the map's box shrunk by half a voxel
};
constexpr int DC_RAY_NO_RETURN = 1, DC_RAY_BELOW_MIN = 2, DC_RAY_TRUNCATED = 4, DC_RAY_CLIPPED = 8, DC_RAY_HIT = 16;

inline void dc_rays_setup(int width, int height, double fx, double fy, double cx, double cy, const double c2w[12], int format, int su, int sv, double min_range,
                          double max_range, int free_no_return, const MapGeom &M, DcRays &Q) {
    Q.width = width; Q.height = height; Q.su = su; Q.sv = sv;
    Q.nu = (width + su - 1) / su; Q.nv = (height + sv - 1) / sv;
    Q.format = format; Q.free_no_return = free_no_return;
    Q.fx = fx; Q.fy = fy; Q.cx = cx; Q.cy = cy;
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) Q.R[3 * i + j] = c2w[4 * i + j];
        Q.t[i] = c2w[4 * i + 3];
        Q.lo[i] = M.bmin[i] + 0.5 * M.res;
        Q.hi[i] = M.bmax[i] - 0.5 * M.res;
    }
    Q.min_range = min_range; Q.max_range = max_range;
}

MU_HD float dc_nan() {
    const unsigned bits = 0x7FC00000u;          // the one NaN a dropped row holds
    float f;
#if defined(__HIP_DEVICE_COMPILE__)
    f = __uint_as_float(bits);
#else
    std::memcpy(&f, &bits, sizeof(f));
#endif
    return f;
}

// the depth of pixel (u, v) in metres; false: no return
MU_HD bool dc_depth(const DcRays &Q, const void *image, int u, int v, double &d) {
    const size_t i = (size_t)v * Q.width + u;
    if (Q.format == DC_FORMAT_I32_MM) {
        const int32_t mm = ((const int32_t *)image)[i];
        if (mm >= DC_NO_RETURN_MM || mm <= 0) return false;
        d = (double)mm / 1000.0;
        return true;
    }
    if (Q.format == DC_FORMAT_U16_MM) {
        const uint16_t mm = ((const uint16_t *)image)[i];
        if (mm == 0) return false;
        d = (double)mm / 1000.0;
        return true;
    }
    const float f = ((const float *)image)[i];
    if (!(f > 0.0f) || !(f - f == 0.0f)) return false;           // 0, negative, NaN, infinite
    d = (double)f;
    return true;
}

// w = R p + t, each row summed left to right
MU_HD void dc_world(const DcRays &Q, const double p[3], double w[3]) {
    for (int a = 0; a < 3; a++) w[a] = Q.R[3 * a] * p[0] + Q.R[3 * a + 1] * p[1] + Q.R[3 * a + 2] * p[2] + Q.t[a];
}

// ray k = iv * nu + iu, pixel (iu * su, iv * sv): its end point and hit byte; returns the DC_RAY_* flags that apply
MU_HD int dc_ray(const DcRays &Q, const void *image, int iu, int iv, float e_out[3], uint8_t &hit_out) {
    const int u = iu * Q.su, v = iv * Q.sv;
    int flags = 0;
    double d = 1.0, scale_to = -1.0;            // scale_to >= 0: the ray is given this length
    bool hit = true;
    if (!dc_depth(Q, image, u, v, d)) {
        flags |= DC_RAY_NO_RETURN;
        if (!Q.free_no_return) { e_out[0] = e_out[1] = e_out[2] = dc_nan(); hit_out = 0; return flags; }
        d = 1.0; scale_to = Q.max_range; hit = false;
    }
    const double p[3] = {((double)u - Q.cx) * d / Q.fx, ((double)v - Q.cy) * d / Q.fy, d};
    double e[3];
    dc_world(Q, p, e);
    const double o[3] = {Q.t[0], Q.t[1], Q.t[2]};
    double dv[3] = {e[0] - o[0], e[1] - o[1], e[2] - o[2]};
    const double range = sqrt(dv[0] * dv[0] + dv[1] * dv[1] + dv[2] * dv[2]);
    if (scale_to < 0.0) {
        if (range < Q.min_range) { flags |= DC_RAY_BELOW_MIN; e_out[0] = e_out[1] = e_out[2] = dc_nan(); hit_out = 0; return flags; }
        if (range > Q.max_range) { flags |= DC_RAY_TRUNCATED; scale_to = Q.max_range; hit = false; }
    }
    if (scale_to >= 0.0) {
        const double k = scale_to / range;
        for (int a = 0; a < 3; a++) { e[a] = o[a] + dv[a] * k; dv[a] = e[a] - o[a]; }
    }
    // the clip: the smallest (bound - o) / (e - o) over the axes on which e lies outside the shrunk box, held to [0, 1]
    double s = 2.0;
    for (int a = 0; a < 3; a++) {
        double bound;
        if (e[a] < Q.lo[a]) bound = Q.lo[a];
        else if (e[a] > Q.hi[a]) bound = Q.hi[a];
        else continue;
        const double sa = dv[a] != 0.0 ? (bound - o[a]) / dv[a] : 0.0;
        if (sa < s) s = sa;
    }
    if (s < 2.0) {
        s = s < 0.0 ? 0.0 : (s > 1.0 ? 1.0 : s);
        for (int a = 0; a < 3; a++) e[a] = o[a] + dv[a] * s;
        flags |= DC_RAY_CLIPPED; hit = false;
    }
    for (int a = 0; a < 3; a++) e_out[a] = (float)e[a];
    if (!(e_out[0] - e_out[0] == 0.0f) || !(e_out[1] - e_out[1] == 0.0f) || !(e_out[2] - e_out[2] == 0.0f)) {       // a row is whole or dropped
        e_out[0] = e_out[1] = e_out[2] = dc_nan(); hit = false;
    }
    hit_out = hit ? 1 : 0;
    if (hit) flags |= DC_RAY_HIT;
    return flags;
}

struct DcRaysCounts { long long n_pixels = 0, n_no_return = 0, n_below_min = 0, n_truncated = 0, n_clipped = 0, n_hits = 0; };

inline void dc_count_ray(int flags, DcRaysCounts &C) {
    C.n_no_return += (flags & DC_RAY_NO_RETURN) != 0; C.n_below_min += (flags & DC_RAY_BELOW_MIN) != 0; C.n_truncated += (flags & DC_RAY_TRUNCATED) != 0;
    C.n_clipped += (flags & DC_RAY_CLIPPED) != 0; C.n_hits += (flags & DC_RAY_HIT) != 0;
}

// every ray of the image, v the outer index; ends: n x 3 floats, hit: n bytes
inline void dc_rays_host(const DcRays &Q, const void *image, float *ends, uint8_t *hit, DcRaysCounts &C) {
    C = DcRaysCounts();
    C.n_pixels = (long long)Q.nu * Q.nv;
    for (int iv = 0; iv < Q.nv; iv++)
        for (int iu = 0; iu < Q.nu; iu++) {
            const size_t k = (size_t)iv * Q.nu + iu;
            dc_count_ray(dc_ray(Q, image, iu, iv, ends + 3 * k, hit[k]), C);
        }
}

}  // namespace isdf
