// Rays cast through the map's occupancy: isdf_map_raycast, the read-only counterpart of map_scan.hip's trace.
//   mr_cast_kernel   one ray per lane, grid-stride: map_raycast_host.hpp's mr_cast_ray - the integer walk of map_scan_host.hpp from the
//                    origin's tick to the end point's, one occupancy byte read per voxel entered, until the first occupied one.  The
//                    walk stays in the box of its two end voxels: no bounds test, no read outside the grid.  Each ray's row of eight
//                    int32 goes out as two 16-byte stores.  The five counters are summed in the wavefront, then through LDS, then one
//                    set of atomics per workgroup into the call's 64-byte record: one hand-over.
// The lanes of a wavefront finish at different lengths, as the trace's do; a workgroup is two wavefronts so that a short cast still
// spreads over the compute units and a long ray holds up one other wavefront's slot at most.
// Nothing here writes to the ctx's map, its products or its flags.
#include "map_query.hpp"
#include "map_raycast_host.hpp"
#include "dev_reduce.hpp"
#include <algorithm>
#include <cstring>

namespace isdf {

// the cast's hand-over record
struct MrRecord {
    unsigned long long n_skipped, n_origin_outside, n_hits, n_clear, steps_total;
    unsigned long long pad[3];
};
static_assert(sizeof(MrRecord) == 64, "the hand-over record is one 64-byte line");

constexpr int MR_BLOCK = 128;
constexpr int MR_WAVES = MR_BLOCK / 64;
constexpr int MR_COUNTERS = 5;

struct MrOrigin { int q[3]; };

__global__ __launch_bounds__(MR_BLOCK) void mr_cast_kernel(const double *__restrict__ origins, const float *__restrict__ ends, long long n, MapGeom M, MrOrigin O,
                                                           const uint8_t *__restrict__ occ, int test_origin, int32_t *__restrict__ rows, MrRecord *__restrict__ rec) {
    long long cnt[MR_COUNTERS] = {0, 0, 0, 0, 0};
    for (long long i = (long long)blockIdx.x * MR_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * MR_BLOCK) {
        int qo[3] = {O.q[0], O.q[1], O.q[2]};
        bool ok = true;
        if (origins) ok = ms_quantize(M, origins[3 * i], origins[3 * i + 1], origins[3 * i + 2], qo);
        const float end[3] = {ends[3 * i], ends[3 * i + 1], ends[3 * i + 2]};
        int row[MR_ROW];
        mr_cast_ray(occ, M, ok, qo, end, test_origin != 0, row);
        mr_count_row(row, cnt[0], cnt[1], cnt[2], cnt[3], cnt[4]);
        int4 *const out = reinterpret_cast<int4 *>(rows + MR_ROW * i);          // 32-byte rows from a 16-byte aligned base
        out[0] = make_int4(row[0], row[1], row[2], row[3]);
        out[1] = make_int4(row[4], row[5], row[6], row[7]);
    }
    if (!rec) return;           // (uniform) the caller wants no counters
    const unsigned long long s = block_sum<MR_COUNTERS, MR_WAVES>(cnt);
    if (s) atomicAdd(&rec->n_skipped + threadIdx.x, s);            // the five counters lie next to each other; s is 0 beyond them
}

}  // namespace isdf

// the host-pointer form's staging, the record and its pinned copy
struct MapRaycastState {
    isdf::DevBuf<void> d_in;                    // origins (3 or n x 3 doubles, 16-byte multiple) | ends
    isdf::DevBuf<int32_t> d_rows;
    isdf::RecPair<isdf::MrRecord> rec;
    isdf::DevEvents<2> ev;
    int ready(isdf_ctx *c) { ISDF_TRY(ev.ready(c)); return rec.ready(c); }
};

using namespace isdf;

extern "C" void isdf_map_raycast_params_default(isdf_map_raycast_params *p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
}

extern "C" void isdf_map_raycast_sizes(int sizes_out[2]) {
    if (!sizes_out) return;
    sizes_out[0] = (int)sizeof(isdf_map_raycast_params); sizes_out[1] = (int)sizeof(isdf_map_raycast_info);
}

namespace {

// what both forms check of the ctx and of the shared origin; O is filled when the origin is shared
int raycast_check(isdf_ctx *c, const double *origins, const void *ends, long long n, const void *rows, const isdf_map_raycast_params *params,
                  isdf_map_raycast_params &P, MrOrigin &O) {
    P = map_query::resolve(params, isdf_map_raycast_params_default);
    if (n < 0 || (!origins && (n > 0 || !P.per_ray_origin)) || (n > 0 && (!ends || !rows))) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "bad ray cast arguments");
    ISDF_TRY(map_query::single_device(c, "casting rays through the map is not offered on a multi-device ctx"));
    ISDF_TRY(map_query::has_occupancy(c, "casting rays"));
    O = MrOrigin{{0, 0, 0}};
    if (!P.per_ray_origin && !ms_quantize(map_geom(c->grid), origins[0], origins[1], origins[2], O.q))
        return isdf_fail(c, ISDF_ERR_INVALID_ARG, "the rays' shared origin lies outside the map");
    return ISDF_OK;
}

// the launch and, with info_out, the one hand-over; d_origins: null for a shared origin (O holds it)
int raycast_run(isdf_ctx *c, MapRaycastState *S, const double *d_origins, const float *d_ends, long long n, const isdf_map_raycast_params &P, const MrOrigin &O,
                int32_t *d_rows, bool count, hipStream_t st) {
    ISDF_TRY(map_query::count_begin(c, count, S->ev, S->rec, st));
    if (n > 0) {
        const unsigned blocks = (unsigned)std::min<long long>((n + MR_BLOCK - 1) / MR_BLOCK, 8192);
        hipLaunchKernelGGL(mr_cast_kernel, dim3(blocks), dim3(MR_BLOCK), 0, st, d_origins, d_ends, n, map_geom(c->grid), O, (const uint8_t *)c->d_occ.get(),
                           (int)P.test_origin_voxel, d_rows, count ? S->rec.dev() : nullptr);
        HIPCHK(c, hipGetLastError());
    }
    return map_query::count_end(c, count, S->ev, S->rec, st);
}

void raycast_info(const MapRaycastState *S, long long n, isdf_map_raycast_info *info_out) {
    const MrRecord R = S->rec.host();
    isdf_map_raycast_info info{};
    info.n_rays = n;
    info.n_skipped = (int64_t)R.n_skipped;
    info.n_origin_outside = (int64_t)R.n_origin_outside;
    info.n_hits = (int64_t)R.n_hits;
    info.n_clear = (int64_t)R.n_clear;
    info.steps_total = (int64_t)R.steps_total;
    info.cast_ms = S->ev.ms(0, 1);
    *info_out = info;
}

}  // namespace

extern "C" int isdf_map_raycast_device(isdf_ctx *c, const double *d_origins, const float *d_ends, long long n, const isdf_map_raycast_params *params,
                                       int32_t *d_rows_out, isdf_map_raycast_info *info_out, void *stream) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    isdf_map_raycast_params P;
    MrOrigin O;
    ISDF_TRY(raycast_check(c, d_origins, d_ends, n, d_rows_out, params, P, O));
    if (((uintptr_t)d_rows_out & 15u) != 0) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "the rows of a ray cast must be 16-byte aligned");
    MapRaycastState *S;
    ISDF_TRY(map_query::state_of(c, c->mrc, &S));
    const hipStream_t st = (hipStream_t)stream;
    ISDF_TRY(raycast_run(c, S, P.per_ray_origin ? d_origins : nullptr, d_ends, n, P, O, d_rows_out, info_out != nullptr, st));
    return map_query::info_after(c, info_out, st, [&](isdf_map_raycast_info *out) { raycast_info(S, n, out); });
}

extern "C" int isdf_map_raycast(isdf_ctx *c, const double *origins, const float *ends, long long n, const isdf_map_raycast_params *params, int32_t *rows_out,
                                isdf_map_raycast_info *info_out) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    isdf_map_raycast_params P;
    MrOrigin O;
    ISDF_TRY(raycast_check(c, origins, ends, n, rows_out, params, P, O));
    MapRaycastState *S;
    ISDF_TRY(map_query::state_of(c, c->mrc, &S));
    const hipStream_t st = c->stream;
    const size_t origin_bytes = P.per_ray_origin ? (((size_t)n * 3 * sizeof(double) + 15) & ~(size_t)15) : 0;
    const size_t end_bytes = (size_t)n * 3 * sizeof(float);
    ISDF_TRY(S->d_in.reserve(c, origin_bytes + end_bytes));
    ISDF_TRY(S->d_rows.reserve(c, (size_t)n * MR_ROW));
    const double *const d_origins = P.per_ray_origin ? (const double *)S->d_in.get() : nullptr;
    const float *const d_ends = (const float *)((const uint8_t *)S->d_in.get() + origin_bytes);
    if (n > 0) {
        if (P.per_ray_origin) HIPCHK(c, hipMemcpyAsync(S->d_in, origins, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync((uint8_t *)S->d_in.get() + origin_bytes, ends, end_bytes, hipMemcpyHostToDevice, st));
    }
    ISDF_TRY(raycast_run(c, S, d_origins, d_ends, n, P, O, S->d_rows.get(), true, st));
    if (n > 0) HIPCHK(c, hipMemcpyAsync(rows_out, S->d_rows, (size_t)n * MR_ROW * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (info_out) raycast_info(S, n, info_out);
    return ISDF_OK;
}

extern "C" long long isdf_raycast_host(const uint8_t *occ, const double bmin[3], const double bmax[3], double resolution, const int32_t dims[3], const double *origins,
                                       const float *ends, long long n, const isdf_map_raycast_params *params, int32_t *rows_out) {
    const isdf_map_raycast_params P = map_query::resolve(params, isdf_map_raycast_params_default);
    if (ms_geometry_bad(bmin, bmax, resolution, dims) || !occ || (!origins && (n > 0 || !P.per_ray_origin)) || n < 0 || (n > 0 && (!ends || !rows_out)))
        return isdf_fail(nullptr, ISDF_ERR_INVALID_ARG, "ray cast (host form): bad arguments");
    MrCounts K;
    if (!mr_cast_host(occ, map_geom(bmin, bmax, resolution, dims), origins, P.per_ray_origin != 0, ends, n, P.test_origin_voxel != 0, rows_out, K))
        return isdf_fail(nullptr, ISDF_ERR_INVALID_ARG, "ray cast (host form): the shared origin lies outside the map");
    return K.n_hits;
}
