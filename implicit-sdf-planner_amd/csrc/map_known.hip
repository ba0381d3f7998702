// Observed space in the map: the known grid - one bit per voxel, set once a ray of isdf_integrate_scan /
// isdf_integrate_depth has visited the voxel or the caller declared it known -, and the frontier computed from it on demand.  The grid
// is one stream of bits (map_known_host.hpp); every kernel here is one lane per dword of it, and every word is formed by that header's
// MU_HD functions, which the host forms call too.
//   mk_merge_kernel     after a scan's trace: known |= free | hit over the dwords of the visited box, which it reads from the scan's
//                       record on the device as ms_apply_kernel does.  The box is taken as one run of the stream per x (first to last
//                       visited voxel of the slab); a dword two runs share belongs to the lower x, and since the scan's bit grids are
//                       zero outside the visited voxels the owner ORs the whole dword: a plain read-modify-write, no atomic.  The new
//                       bits are counted by __popc into the scan's own record, which the scan's first hand-over brings back.
//   mk_shift_kernel     with the window shift's translation stage: dst word = mk_bits_at(src, 32 w + delta) under the validity mask of
//                       the column segments the dword covers - two loads and a funnel shift, not 32 loads.
//   mk_fill_kernel      a box set or cleared: the same masks over the dwords between the box's first and last voxel.
//   mk_stats_kernel     isdf_map_known_get: the known voxels counted and boxed.
//   mk_frontier_kernel  K = 1, occupancy byte 0, some 6-neighbour inside the grid with K = 0: six neighbour streams at +-1, +-nz,
//                       +-ny nz, each under its edge mask; the 32 occupancy bytes arrive as two 16-byte loads.  Writes the frontier
//                       word and its count; the list is the repo's exclusive scan over the counts and mk_emit_kernel - no atomics, so
//                       the voxels come out ascending on every run.
//   mk_count_kernel     stands in for the frontier kernel where the set is a caller's (isdf_map_frontier_clusters with bits_in, DESIGN
//                       4.22): the counts and the record of words that are in d_front already.
// The reductions go through the wavefront, then LDS (dev_reduce.hpp), then one set of global atomics per workgroup into one 64-byte record.
#include "map_query.hpp"
#include "map_known_host.hpp"
#include "map_change.hpp"
#include "frontend_dev.hpp"
#include "dev_reduce.hpp"
#include "dev_scan.hpp"
#include <algorithm>
#include <climits>
#include <cstring>
#include <vector>

namespace isdf {

struct MkGeom { int X, Y, Z; long long n_vox, n_words; };

// called by every thread of a 256-thread workgroup: two sums and a box over the workgroup, then one atomic each where there is something
__device__ __forceinline__ void mk_block_reduce(unsigned long long n, unsigned long long newly, const int lo[3], const int hi[3], unsigned long long *g_n,
                                                unsigned long long *g_newly, int *g_lo, int *g_hi) {
    const BoxAcc box = BoxAcc::open();
    if (g_lo && hi[0] >= 0) box.add(lo, hi);
    const unsigned long long cnt[2] = {n, newly};
    const unsigned long long s = block_sum<2, 4>(cnt);      // thread 0: n, thread 1: newly (its barrier lies behind every add)
    if (threadIdx.x == 0 && g_n && s) atomicAdd(g_n, s);
    if (threadIdx.x == 1 && g_newly && s) atomicAdd(g_newly, s);
    if (threadIdx.x == 0 && g_lo) box.flush(g_lo, g_hi);
}

__global__ __launch_bounds__(256) void mk_merge_kernel(MkGeom g, const unsigned *__restrict__ free_bits, const unsigned *__restrict__ hit_bits,
                                                       unsigned *__restrict__ known, MsRecord *srec) {
    const int lo0 = srec->lo[0], lo1 = srec->lo[1], lo2 = srec->lo[2], hi0 = srec->hi[0], hi1 = srec->hi[1], hi2 = srec->hi[2];
    unsigned long long newly = 0;
    if (hi0 >= lo0 && hi1 >= lo1 && hi2 >= lo2) {               // (else no ray was traced; every thread still reaches the reduction)
        const long long slab = (long long)g.Y * g.Z;
        const long long r0 = (long long)lo1 * g.Z + lo2, r1 = (long long)hi1 * g.Z + hi2;      // the slab's run: first and last visited voxel
        const int wr = (int)((r1 - r0 + 31) >> 5) + 1;          // dwords that a run can touch, at any alignment
        const long long n = (long long)(hi0 - lo0 + 1) * wr;
        for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long long)gridDim.x * blockDim.x) {
            const int k = (int)(t % wr), x = lo0 + (int)(t / wr);
            const long long a0 = x * slab + r0, a1 = x * slab + r1;
            const long long w = (a0 >> 5) + k;
            if (w > (a1 >> 5)) continue;
            if (x > lo0 && w <= ((a1 - slab) >> 5)) continue;   // shared with the run of x - 1, which owns it
            const unsigned v = free_bits[w] | hit_bits[w];
            if (!v) continue;
            const unsigned old = known[w], fresh = v & ~old;
            if (fresh) { known[w] = old | v; newly += __popc(fresh); }
        }
    }
    mk_block_reduce(0ull, newly, nullptr, nullptr, nullptr, &srec->newly_known, nullptr, nullptr);
}

__global__ __launch_bounds__(256) void mk_shift_kernel(MkGeom g, const unsigned *__restrict__ src, unsigned *__restrict__ dst, MkShift P) {
    for (long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x; w < g.n_words; w += (long long)gridDim.x * blockDim.x)
        dst[w] = mk_shift_word(src, g.n_words, w, g.Y, g.Z, g.n_vox, P);
}

__global__ __launch_bounds__(256) void mk_fill_kernel(MkGeom g, unsigned *__restrict__ known, MuBox box, long long w0, long long w1, int value, MkRecord *rec) {
    unsigned long long newly = 0, gone = 0;
    for (long long w = w0 + (long long)blockIdx.x * blockDim.x + threadIdx.x; w <= w1; w += (long long)gridDim.x * blockDim.x) {
        const unsigned m = mk_box_mask(w, g.Y, g.Z, g.n_vox, box.lo, box.hi);
        if (!m) continue;
        const unsigned old = known[w], now = value ? old | m : old & ~m;
        if (now != old) known[w] = now;
        newly += __popc(now & ~old);
        gone += __popc(old & ~now);
    }
    mk_block_reduce(gone, newly, nullptr, nullptr, &rec->gone, &rec->newly, nullptr, nullptr);
}

__global__ __launch_bounds__(256) void mk_stats_kernel(MkGeom g, const unsigned *__restrict__ known, MkRecord *rec) {
    int lo[3] = {0x7FFFFFFF, 0x7FFFFFFF, 0x7FFFFFFF}, hi[3] = {-1, -1, -1};
    unsigned long long n = 0;
    for (long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x; w < g.n_words; w += (long long)gridDim.x * blockDim.x) {
        const unsigned v = known[w];
        n += __popc(v);
        mk_word_box(w, v, g.Y, g.Z, g.n_vox, lo, hi);
    }
    mk_block_reduce(n, 0ull, lo, hi, &rec->n, nullptr, rec->lo, rec->hi);
}

// occ: 16-byte aligned and allocated in whole dwords (the ctx's d_occ: a device allocation of (n_vox + 3) & ~3 bytes), so dword w's 32
// bytes are two aligned 16-byte loads wherever all 32 voxels exist, and whole dwords up to the one holding the last voxel elsewhere
__global__ __launch_bounds__(256) void mk_frontier_kernel(MkGeom g, const unsigned *__restrict__ known, const uint8_t *__restrict__ occ, unsigned *__restrict__ front,
                                                          int *__restrict__ cnt, MkRecord *rec) {
    int lo[3] = {0x7FFFFFFF, 0x7FFFFFFF, 0x7FFFFFFF}, hi[3] = {-1, -1, -1};
    unsigned long long n = 0;
    for (long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x; w < g.n_words; w += (long long)gridDim.x * blockDim.x) {
        unsigned f = 0u;
        if (known[w]) {
            unsigned free_mask = 0u;
            if (32 * w + 32 <= g.n_vox) {
                const uint4 a = ((const uint4 *)occ)[2 * w], b = ((const uint4 *)occ)[2 * w + 1];
                free_mask = mk_free4(a.x) | (mk_free4(a.y) << 4) | (mk_free4(a.z) << 8) | (mk_free4(a.w) << 12) | (mk_free4(b.x) << 16) | (mk_free4(b.y) << 20) |
                            (mk_free4(b.z) << 24) | (mk_free4(b.w) << 28);
            } else {
                for (int d = 0; d < 8 && 32 * w + 4 * d < g.n_vox; d++) free_mask |= mk_free4(((const unsigned *)occ)[8 * w + d]) << (4 * d);
            }
            f = mk_frontier_word(known, g.n_words, w, g.X, g.Y, g.Z, g.n_vox, free_mask);
        }
        front[w] = f;
        cnt[w] = __popc(f);
        n += __popc(f);
        mk_word_box(w, f, g.Y, g.Z, g.n_vox, lo, hi);
    }
    mk_block_reduce(n, 0ull, lo, hi, &rec->n, nullptr, rec->lo, rec->hi);
}

// a caller's set in place of the frontier (isdf_map_frontier_clusters with bits_in): the words are in `front` already; their counts and the record
__global__ __launch_bounds__(256) void mk_count_kernel(MkGeom g, const unsigned *__restrict__ front, int *__restrict__ cnt, MkRecord *rec) {
    int lo[3] = {0x7FFFFFFF, 0x7FFFFFFF, 0x7FFFFFFF}, hi[3] = {-1, -1, -1};
    unsigned long long n = 0;
    for (long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x; w < g.n_words; w += (long long)gridDim.x * blockDim.x) {
        const unsigned f = front[w];
        cnt[w] = __popc(f);
        n += __popc(f);
        mk_word_box(w, f, g.Y, g.Z, g.n_vox, lo, hi);
    }
    mk_block_reduce(n, 0ull, lo, hi, &rec->n, nullptr, rec->lo, rec->hi);
}

__global__ __launch_bounds__(256) void mk_emit_kernel(long long n_words, const unsigned *__restrict__ front, const int *__restrict__ base, long long *__restrict__ vox) {
    for (long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x; w < n_words; w += (long long)gridDim.x * blockDim.x) {
        long long at = base[w];
        for (unsigned f = front[w]; f; f &= f - 1) vox[at++] = 32 * w + (__ffs((int)f) - 1);
    }
}

}  // namespace isdf

using namespace isdf;

namespace {

// workgroups of the grid-stride kernels over n dwords: at most 2048, at least one
unsigned word_blocks(long long n) { return (unsigned)std::max<long long>(1, std::min<long long>((n + 255) / 256, 2048)); }

MkGeom geom(const isdf_ctx *c) {
    const DevGrid &G = c->grid;
    const long long n = (long long)G.X * G.Y * G.Z;
    return MkGeom{G.X, G.Y, G.Z, n, mk_words(n)};
}

MkRecord record_empty() {
    MkRecord r{};
    for (int a = 0; a < 3; a++) { r.lo[a] = 0x7FFFFFFF; r.hi[a] = -1; }
    return r;
}

int has_known(isdf_ctx *c, const char *op) {
    return map_query::has_known(c, (std::string(op) + ": no known grid (isdf_map_known_enable, then a map from isdf_set_pointcloud)").c_str());
}

// what every entry point here asks first; the record and its pinned copy exist afterwards, the device record is empty
int known_begin(isdf_ctx *c, const char *op) {
    ISDF_TRY(has_known(c, op));
    isdf_ctx::Known &K = c->known;
    HIPCHK(c, hipSetDevice(c->device));
    ISDF_TRY(K.rec.ready(c));
    ISDF_TRY(K.ev.ready(c));
    HIPCHK(c, K.rec.put(record_empty(), c->stream));
    return ISDF_OK;
}

int known_fetch(isdf_ctx *c) {
    HIPCHK(c, c->known.rec.fetch(c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ISDF_OK;
}

void box_out(const MkRecord &R, int32_t lo[3], int32_t hi[3]) {
    for (int a = 0; a < 3; a++) { lo[a] = R.n ? R.lo[a] : 0; hi[a] = R.n ? R.hi[a] : -1; }
}

}  // namespace

int map_known_reset(isdf_ctx *c) {
    isdf_ctx::Known &K = c->known;
    K.have = false;                     // (a failure below must not leave a grid of the old size behind a map of the new one)
    if (!K.on || !c->have_geom) return ISDF_OK;
    const MkGeom g = geom(c);
    ISDF_TRY(K.d_bits.reserve(c, (size_t)g.n_words));
    HIPCHK(c, hipMemsetAsync(K.d_bits, 0, (size_t)g.n_words * sizeof(unsigned), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    K.n_words = (size_t)g.n_words; K.have = true; K.newly = 0; K.merges = 0;
    return ISDF_OK;
}

int isdf::map_known_merge_launch(isdf_ctx *c, const unsigned *d_free_bits, const unsigned *d_hit_bits, MsRecord *d_scan) {
    const MkGeom g = geom(c);
    isdf_ctx::Known &K = c->known;
    if (K.time_merge) {
        ISDF_TRY(K.ev_merge.ready(c));
        HIPCHK(c, hipEventRecord(K.ev_merge[0], c->stream));
    }
    hipLaunchKernelGGL(mk_merge_kernel, dim3(1024), dim3(256), 0, c->stream, g, d_free_bits, d_hit_bits, K.d_bits.get(), d_scan);
    HIPCHK(c, hipGetLastError());
    if (K.time_merge) HIPCHK(c, hipEventRecord(K.ev_merge[1], c->stream));
    return ISDF_OK;
}

void isdf::map_known_merged(isdf_ctx *c, const MsRecord &scan) {
    c->known.newly = (long long)scan.newly_known;
    c->known.merges++;
    if (c->known.time_merge && c->known.ev_merge[1]) c->known.merge_ms = c->known.ev_merge.ms(0, 1);      // (the hand-over has synchronised)
}

int isdf::map_known_shift_launch(isdf_ctx *c, const int32_t s[3]) {
    isdf_ctx::Known &K = c->known;
    const MkGeom g = geom(c);
    const int32_t dims[3] = {g.X, g.Y, g.Z};
    ISDF_TRY(K.d_shift.reserve(c, K.n_words));
    hipLaunchKernelGGL(mk_shift_kernel, dim3(word_blocks(g.n_words)), dim3(256), 0, c->stream, g, (const unsigned *)K.d_bits.get(), K.d_shift.get(), mk_shift_plan(dims, s));
    HIPCHK(c, hipGetLastError());
    return ISDF_OK;
}

void isdf::map_known_shift_swap(isdf_ctx *c) { c->known.d_bits.swap(c->known.d_shift); }

extern "C" void isdf_map_known_sizes(int sizes_out[4]) {
    if (!sizes_out) return;
    sizes_out[0] = (int)sizeof(isdf_map_known_info); sizes_out[1] = (int)sizeof(isdf_map_frontier_info);
    sizes_out[2] = (int)sizeof(isdf_traj_known_params); sizes_out[3] = (int)sizeof(isdf_traj_known_info);
}

extern "C" int isdf_map_known_enable(isdf_ctx *c, int on) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    ISDF_TRY(map_query::single_device(c, "the known grid is not offered on a multi-device ctx"));
    isdf_ctx::Known &K = c->known;
    HIPCHK(c, hipSetDevice(c->device));
    (void)isdf_field_gate_drop(c);              // a field gated by K's erosion goes with either answer, whatever its follow mode
    if (!on) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        K.on = K.have = false; K.n_words = 0; K.newly = K.merges = 0;
        K.d_bits.release(); K.d_shift.release(); K.d_front.release(); K.d_cnt.release(); K.d_base.release(); K.d_list.release(); K.d_scan_tmp.release();
        c->ker.reset();                         // the erosion's scratch grids
        return ISDF_OK;
    }
    if (K.on) return ISDF_OK;           // (a grid that exists stays as it is)
    K.on = true;
    return c->d_counts ? map_known_reset(c) : ISDF_OK;
}

extern "C" int isdf_map_known_merge_ms(isdf_ctx *c, int enable, double *ms_out) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    if (ms_out) *ms_out = c->known.merge_ms;
    c->known.time_merge = enable != 0;
    if (!enable) c->known.merge_ms = -1.0;
    return ISDF_OK;
}

extern "C" int isdf_map_known_fill(isdf_ctx *c, const int32_t *box, int value) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    ISDF_TRY(has_known(c, "filling the known grid"));
    const MkGeom g = geom(c);
    const int32_t dims[3] = {g.X, g.Y, g.Z};
    const int32_t whole[6] = {0, 0, 0, g.X - 1, g.Y - 1, g.Z - 1};
    if (!box) box = whole;
    if (mk_box_bad(dims, box)) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "filling the known grid: the box lies outside the grid or has lo > hi");
    ISDF_TRY(known_begin(c, "filling the known grid"));
    // K changes: a field gated by its erosion is dropped, or - isdf_frontend_field_set_known_follow(1), DESIGN 4.27 - kept
    // for the stage below: a set box can only grow E (opening), a cleared one only shrink it (closing), inside the box grown by the radius
    const bool follow = isdf_field_follow_wanted(c);
    (void)isdf_field_known_changed(c);
    isdf_field_follow_call(c);
    isdf_ctx::Known &K = c->known;
    MuBox B;
    for (int a = 0; a < 3; a++) { B.lo[a] = box[a]; B.hi[a] = box[3 + a]; }
    const long long w0 = (((long long)B.lo[0] * g.Y + B.lo[1]) * g.Z + B.lo[2]) >> 5, w1 = (((long long)B.hi[0] * g.Y + B.hi[1]) * g.Z + B.hi[2]) >> 5;
    hipLaunchKernelGGL(mk_fill_kernel, dim3(word_blocks(w1 - w0 + 1)), dim3(256), 0, c->stream, g, K.d_bits.get(), B, w0, w1, value ? 1 : 0, K.rec.dev());
    int rc = hipGetLastError() == hipSuccess ? known_fetch(c) : isdf_fail(c, ISDF_ERR_HIP, "filling the known grid: the launch failed");
    if (rc != ISDF_OK) {                        // the kernel may have run: K may have moved
        if (follow) { const std::string err = c->err; (void)isdf_field_gate_drop(c); c->err = err; }
        return rc;
    }
    K.newly = (long long)K.rec.host().newly;
    if (follow && (value ? K.rec.host().newly : K.rec.host().gone) > 0) {
        const MuBox grown = mu_box_grow(B, c->fe.field_gate_radius, dims);
        int kept = 0;
        ISDF_TRY(isdf_field_follow_stage(c, value ? FfChange::Opening : FfChange::Closing, grown.lo, grown.hi, K.ev[0], K.ev[1], &kept));
    }
    return ISDF_OK;
}

extern "C" int isdf_map_known_get(isdf_ctx *c, uint32_t *bits_out, isdf_map_known_info *info_out) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    ISDF_TRY(known_begin(c, "reading the known grid"));
    isdf_ctx::Known &K = c->known;
    const MkGeom g = geom(c);
    if (info_out) {
        hipLaunchKernelGGL(mk_stats_kernel, dim3(word_blocks(g.n_words)), dim3(256), 0, c->stream, g, (const unsigned *)K.d_bits.get(), K.rec.dev());
        HIPCHK(c, hipGetLastError());
    }
    if (bits_out) HIPCHK(c, hipMemcpyAsync(bits_out, K.d_bits, (size_t)g.n_words * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    ISDF_TRY(known_fetch(c));
    if (info_out) {
        const MkRecord R = K.rec.host();
        isdf_map_known_info info{};
        info.n_known = (int64_t)R.n; info.n_unknown = (int64_t)(g.n_vox - (long long)R.n);
        box_out(R, info.lo, info.hi);
        info.newly_known = K.newly; info.merges = K.merges;
        *info_out = info;
    }
    return ISDF_OK;
}

// The frontier stage, shared by isdf_map_frontier and isdf_map_frontier_clusters (frontier_cluster.hip): the set's words into d_front with
// their per-dword counts - the frontier kernel, or with set_bits (host words in K's layout, tail bits clean) the upload and the count
// kernel -, the record's hand-over, and with want_list the exclusive scan of the counts into d_base and the emit pass into d_list (not
// synchronised; nothing is launched for an empty set).  *counted: *rec_out is the record (the caller's info can be filled) even where the
// call then fails.  list_ev (nullable): two events recorded round the scan and the emit pass.
int isdf::map_frontier_stage(isdf_ctx *c, const char *op, const uint32_t *set_bits, uint32_t *bits_out, bool want_list, long long capacity, const hipEvent_t *list_ev,
                             MkRecord *rec_out, bool *counted) {
    *counted = false;
    const std::string what(op);
    if (c->known.have && !set_bits && !c->d_occ) return isdf_fail(c, ISDF_ERR_STATE, (what + ": no occupancy grid").c_str());
    ISDF_TRY(known_begin(c, op));
    isdf_ctx::Known &K = c->known;
    const MkGeom g = geom(c);
    const hipStream_t st = c->stream;
    if (g.n_words > (long long)INT_MAX) return isdf_fail(c, ISDF_ERR_OVERFLOW, (what + ": more than 2^31 words").c_str());
    ISDF_TRY(K.d_front.reserve(c, (size_t)g.n_words)); ISDF_TRY(K.d_cnt.reserve(c, (size_t)g.n_words)); ISDF_TRY(K.d_base.reserve(c, (size_t)g.n_words));
    if (set_bits) HIPCHK(c, hipMemcpyAsync(K.d_front, set_bits, (size_t)g.n_words * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipEventRecord(K.ev[0], st));
    if (set_bits)
        hipLaunchKernelGGL(mk_count_kernel, dim3(word_blocks(g.n_words)), dim3(256), 0, st, g, (const unsigned *)K.d_front.get(), K.d_cnt.get(), K.rec.dev());
    else
        hipLaunchKernelGGL(mk_frontier_kernel, dim3(word_blocks(g.n_words)), dim3(256), 0, st, g, (const unsigned *)K.d_bits.get(), (const uint8_t *)c->d_occ.get(), K.d_front.get(),
                           K.d_cnt.get(), K.rec.dev());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(K.ev[1], st));
    if (bits_out) HIPCHK(c, hipMemcpyAsync(bits_out, K.d_front, (size_t)g.n_words * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    ISDF_TRY(known_fetch(c));
    const MkRecord R = K.rec.host();
    *rec_out = R;
    *counted = true;
    if (!want_list || R.n == 0) return ISDF_OK;
    if ((unsigned long long)capacity < R.n) return isdf_fail(c, ISDF_ERR_OVERFLOW, (what + ": output capacity smaller than the number of frontier voxels").c_str());
    if (R.n > (unsigned long long)INT_MAX) return isdf_fail(c, ISDF_ERR_OVERFLOW, (what + ": more than 2^31 frontier voxels").c_str());
    size_t bytes;
    ISDF_TRY(exclusive_sum_reserve(c, K.d_scan_tmp, K.d_cnt.get(), K.d_base.get(), g.n_words, st, &bytes)); ISDF_TRY(K.d_list.reserve(c, (size_t)R.n));
    if (list_ev) HIPCHK(c, hipEventRecord(list_ev[0], st));
    ISDF_TRY(exclusive_sum_run(c, K.d_scan_tmp, bytes, K.d_cnt.get(), K.d_base.get(), g.n_words, st));
    hipLaunchKernelGGL(mk_emit_kernel, dim3(word_blocks(g.n_words)), dim3(256), 0, st, g.n_words, (const unsigned *)K.d_front.get(), (const int *)K.d_base.get(), K.d_list.get());
    HIPCHK(c, hipGetLastError());
    if (list_ev) HIPCHK(c, hipEventRecord(list_ev[1], st));
    return ISDF_OK;
}

extern "C" int isdf_map_frontier(isdf_ctx *c, uint32_t *bits_out, int64_t *vox_out, long long capacity, isdf_map_frontier_info *info_out) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    if (capacity < 0) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "frontier: negative capacity");
    MkRecord R;
    bool counted = false;
    const int rc = map_frontier_stage(c, "frontier", nullptr, bits_out, vox_out != nullptr, capacity, nullptr, &R, &counted);
    if (counted && info_out) {
        isdf_map_frontier_info info{};
        info.n_frontier = (int64_t)R.n;
        box_out(R, info.lo, info.hi);
        info.kernel_ms = c->known.ev.ms(0, 1);
        *info_out = info;
    }
    if (rc) return rc;
    if (!vox_out || R.n == 0) return ISDF_OK;
    HIPCHK(c, hipMemcpyAsync(vox_out, c->known.d_list, (size_t)R.n * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ISDF_OK;
}

// ---- host forms: no ctx, no device
extern "C" long long isdf_known_merge_host(uint32_t *bits_inout, const int32_t dims[3], const uint8_t *free_bytes, const uint32_t *hits_u32) {
    if (!bits_inout || mk_dims_bad(dims)) return isdf_fail(nullptr, ISDF_ERR_INVALID_ARG, "known grid (host form): bad arguments");
    return mk_merge_host(bits_inout, dims, free_bytes, hits_u32);
}

extern "C" int isdf_known_shift_host(const uint32_t *bits_in, const int32_t dims[3], const int32_t shift[3], uint32_t *bits_out) {
    if (!bits_in || !bits_out || bits_in == bits_out || !shift || mk_dims_bad(dims)) return isdf_fail(nullptr, ISDF_ERR_INVALID_ARG, "known grid (host form): bad arguments");
    mk_shift_host(bits_in, dims, shift, bits_out);
    return ISDF_OK;
}

extern "C" long long isdf_known_fill_host(uint32_t *bits_inout, const int32_t dims[3], const int32_t *box, int value) {
    if (!bits_inout || mk_dims_bad(dims)) return isdf_fail(nullptr, ISDF_ERR_INVALID_ARG, "known grid (host form): bad arguments");
    const int32_t whole[6] = {0, 0, 0, dims[0] - 1, dims[1] - 1, dims[2] - 1};
    if (!box) box = whole;
    if (mk_box_bad(dims, box)) return isdf_fail(nullptr, ISDF_ERR_INVALID_ARG, "known grid (host form): the box lies outside the grid or has lo > hi");
    return mk_fill_host(bits_inout, dims, box, value);
}

extern "C" int isdf_known_frontier_host(const uint32_t *bits, const uint8_t *occ, const int32_t dims[3], uint32_t *bits_out, int64_t *vox_out, long long capacity,
                                        isdf_map_frontier_info *info_out) {
    if (!bits || !occ || capacity < 0 || mk_dims_bad(dims)) return isdf_fail(nullptr, ISDF_ERR_INVALID_ARG, "known grid (host form): bad arguments");
    int lo[3], hi[3];
    const long long n = mk_frontier_host(bits, occ, dims, bits_out, vox_out, capacity, lo, hi);
    if (info_out) {
        isdf_map_frontier_info info{};
        info.n_frontier = n;
        for (int a = 0; a < 3; a++) { info.lo[a] = lo[a]; info.hi[a] = hi[a]; }
        *info_out = info;
    }
    if (vox_out && capacity < n) return isdf_fail(nullptr, ISDF_ERR_OVERFLOW, "known grid (host form): output capacity smaller than the number of frontier voxels");
    return ISDF_OK;
}
