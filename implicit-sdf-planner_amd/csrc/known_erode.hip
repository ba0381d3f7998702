// The eroded known grid: isdf_map_known_erode - for every voxel, whether the whole cube of voxels a robot centred there
// can touch has been observed - and the hand-over of it to the gated cost-to-go field (frontend_field.hip: isdf_frontend_field_build_known).
// The definition and the per-dword arithmetic are known_erode_host.hpp's; the host form calls the same MU_HD function.
//   ke_pass_kernel<COUNT>  one lane per dword of the bit stream, grid-stride: one one-axis pass, 2 r + 1 funnel-shifted reads of the
//                          source stream under their inside masks (ke_pass_word).  COUNT (the last pass): the set bits of K and of the
//                          result through block_sum, one pair of atomics per workgroup into the call's record.
// Three launches, z then y then x, through two scratch bit grids: K -> a -> b -> a.  With r = 0 one launch copies K and counts.  The passes
// are not fused through LDS: a grid is nx ny nz / 8 bytes (2 MB at 256^3), the three of them stay in L2 between the launches, and a fused
// tile would need a halo of r dwords' worth of columns on every side for r up to 64.  The call is read-only: K, the occupancy, a kept
// field, an armed watch and the epochs are untouched; the scratch grows only.
#include "map_query.hpp"
#include "known_erode_host.hpp"
#include "dev_reduce.hpp"
#include <algorithm>
#include <cstring>
#include <vector>

namespace isdf {

struct KeGeom { int X, Y, Z; long long n_vox, n_words; };
struct KeRecord { unsigned long long known, eroded; };

template <bool COUNT>
__global__ __launch_bounds__(256) void ke_pass_kernel(KeGeom g, const unsigned *__restrict__ in, unsigned *__restrict__ out, int axis, int r, int border,
                                                      const unsigned *__restrict__ known, KeRecord *rec) {
    unsigned long long cnt[2] = {0ull, 0ull};
    for (long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x; w < g.n_words; w += (long long)gridDim.x * blockDim.x) {
        const unsigned e = ke_pass_word(in, g.n_words, w, g.X, g.Y, g.Z, g.n_vox, axis, r, border);
        out[w] = e;
        if (COUNT) { cnt[0] += __popc(known[w]); cnt[1] += __popc(e); }
    }
    if (COUNT) {
        const unsigned long long s = block_sum<2, 4>(cnt);      // thread 0: known, thread 1: eroded
        if (threadIdx.x == 0 && s) atomicAdd(&rec->known, s);
        if (threadIdx.x == 1 && s) atomicAdd(&rec->eroded, s);
    }
}

}  // namespace isdf

// the two scratch grids, the call's record and its pinned copy, the events round the passes
struct KnownErodeState {
    isdf::DevBuf<unsigned> d_a, d_b;
    isdf::RecPair<isdf::KeRecord> rec;
    isdf::DevEvents<2> ev;
    int ready(isdf_ctx *c) { ISDF_TRY(ev.ready(c)); return rec.ready(c); }
};

using namespace isdf;

extern "C" void isdf_known_erode_params_default(isdf_known_erode_params *p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->radius = -1;
}

extern "C" void isdf_known_erode_sizes(int sizes_out[2]) {
    if (!sizes_out) return;
    sizes_out[0] = (int)sizeof(isdf_known_erode_params); sizes_out[1] = (int)sizeof(isdf_known_erode_info);
}

int isdf::known_erode_check(isdf_ctx *c, const isdf_known_erode_params &P) {
    if (P.border != 0 && P.border != 1) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "known erode: border is 0 (outside unseen) or 1 (outside seen)");
    if (P.radius < -1 || P.radius > KE_MAX_RADIUS) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "known erode: radius is -1 (the front end's footprint) or 0 .. 64");
    return ISDF_OK;
}

int isdf::known_erode_radius(isdf_ctx *c, const isdf_known_erode_params &P, int *radius) {
    if (P.radius == -1 && !c->fe.built) return isdf_fail(c, ISDF_ERR_STATE, "known erode: radius -1 needs isdf_frontend_build (the footprint is its kernel_size)");
    *radius = P.radius == -1 ? (c->fe.cfg.kernel_size - 1) / 2 : P.radius;
    return ISDF_OK;
}

int isdf::known_erode_launch(isdf_ctx *c, int r, int border, const unsigned **d_E) {
    KnownErodeState *S;
    ISDF_TRY(map_query::state_of(c, c->ker, &S));
    const DevGrid &G = c->grid;
    const long long n_vox = (long long)G.X * G.Y * G.Z;
    const KeGeom g{G.X, G.Y, G.Z, n_vox, mk_words(n_vox)};
    const size_t nw = (size_t)g.n_words;
    ISDF_TRY(S->d_a.reserve(c, nw));
    if (r > 0) ISDF_TRY(S->d_b.reserve(c, nw));
    const hipStream_t st = c->stream;
    const unsigned *const K = (const unsigned *)c->known.d_bits.get();
    const dim3 grid((unsigned)std::max<long long>(1, std::min<long long>((g.n_words + 255) / 256, 2048))), block(256);
    ISDF_TRY(map_query::count_begin(c, true, S->ev, S->rec, st));
    if (r > 0) {
        hipLaunchKernelGGL(ke_pass_kernel<false>, grid, block, 0, st, g, K, S->d_a.get(), 2, r, border, K, S->rec.dev());
        hipLaunchKernelGGL(ke_pass_kernel<false>, grid, block, 0, st, g, (const unsigned *)S->d_a.get(), S->d_b.get(), 1, r, border, K, S->rec.dev());
    }
    hipLaunchKernelGGL(ke_pass_kernel<true>, grid, block, 0, st, g, r > 0 ? (const unsigned *)S->d_b.get() : K, S->d_a.get(), 0, r, border, K, S->rec.dev());
    HIPCHK(c, hipGetLastError());
    ISDF_TRY(map_query::count_end(c, true, S->ev, S->rec, st));
    *d_E = S->d_a.get();
    return ISDF_OK;
}

void isdf::known_erode_report(isdf_ctx *c, int r, int border, isdf_known_erode_info *out) {
    KnownErodeState *S = c->ker.get();
    isdf_known_erode_info info{};
    info.radius_used = r; info.border = border;
    info.known_voxels = (int64_t)S->rec.host().known; info.eroded_voxels = (int64_t)S->rec.host().eroded;
    info.erode_ms = S->ev.ms(0, 1);
    *out = info;
}

extern "C" int isdf_map_known_erode(isdf_ctx *c, const isdf_known_erode_params *params, uint32_t *bits_out, isdf_known_erode_info *info_out) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    const isdf_known_erode_params P = map_query::resolve(params, isdf_known_erode_params_default);
    ISDF_TRY(known_erode_check(c, P));
    ISDF_TRY(map_query::single_device(c, "the eroded known grid is not offered on a multi-device ctx"));
    ISDF_TRY(map_query::has_known(c, "known erode: no known grid (isdf_map_known_enable, then a map from isdf_set_pointcloud)"));
    int r;
    ISDF_TRY(known_erode_radius(c, P, &r));
    const unsigned *d_E;
    ISDF_TRY(known_erode_launch(c, r, P.border, &d_E));
    if (bits_out) HIPCHK(c, hipMemcpyAsync(bits_out, d_E, c->known.n_words * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (!info_out) {
        if (bits_out) HIPCHK(c, hipStreamSynchronize(c->stream));
        return ISDF_OK;
    }
    return map_query::info_after(c, info_out, c->stream, [&](isdf_known_erode_info *out) { known_erode_report(c, r, P.border, out); });
}

// ---- the host form: no ctx, no device
extern "C" int isdf_known_erode_host(const uint32_t *bits, const int32_t dims[3], int radius, int border, uint32_t *bits_out) {
    if (!bits || !bits_out || bits == bits_out) return isdf_fail(nullptr, ISDF_ERR_INVALID_ARG, "known erode (host form): null or aliased bit grids");
    if (mk_dims_bad(dims)) return isdf_fail(nullptr, ISDF_ERR_INVALID_ARG, "known erode (host form): bad dims (each 1 .. 4096)");
    if (border != 0 && border != 1) return isdf_fail(nullptr, ISDF_ERR_INVALID_ARG, "known erode (host form): border is 0 (outside unseen) or 1 (outside seen)");
    if (radius < 0 || radius > KE_MAX_RADIUS) return isdf_fail(nullptr, ISDF_ERR_INVALID_ARG, "known erode (host form): radius is 0 .. 64");
    try {
        std::vector<uint32_t> scratch((size_t)mk_words(mk_voxels(dims)));
        ke_erode_host(bits, dims, radius, border, bits_out, scratch.data());
    } catch (const std::bad_alloc &) {
        return isdf_fail(nullptr, ISDF_ERR_HIP, "known erode (host form): out of host memory");
    }
    return ISDF_OK;
}
