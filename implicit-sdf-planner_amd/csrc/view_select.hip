// The view selection: isdf_view_select, the greedy coverage selection of k views of a pose list by their joint gain - the
// view that sees the most voxels which are unknown today and which no view picked so far sees, k times, on the device.
//   vs_begin_kernel     one lane per view / round: the per-view counts and marginals 0, round -1, the select rows padded.
//   (view_gain.hip)     gain_run on the poses: vg_setup_kernel, then per chunk the clear and vg_gain_kernel, as isdf_view_gain - so the rows
//                       are the view gain's.  After each chunk's gain kernel its seen grids are live, and a scored view's seen grid IS U_j:
//   vs_count_kernel     grid = (blocks of words, views of the chunk): the non-zero words of each seen grid, block_sum, one 64-bit atomicAdd
//                       per workgroup into the view's count.
//   vs_scan_kernel      one workgroup: the exclusive scan of the chunk's counts from the running base in the call's record - every view's
//                       segment start and its fill cursor; the chunk's total and the new base into the record.
//   -- one hand-over per chunk: the record.  The total sizes the list (grow-only, content kept).
//   vs_fill_kernel      the same grid: the non-zero words as {word index, bits}, 8 bytes each, appended to the view's segment through its
//                       cursor, one atomicAdd per wavefront (ballot, the lanes' ranks from the mask).  The order inside a segment depends
//                       on the atomics; nothing consumes it.
//   then k rounds, a fixed sequence of launches without a hand-over; once the record's `done` is set the later kernels return at once:
//   vs_marginal_kernel  grid = (blocks, views): popcount(bits & ~claimed[w]) over the view's segment, block_sum, one 64-bit atomicAdd per
//                       workgroup into m[j]; a picked or unscored view, and a workgroup past the segment's end, is skipped (uniform).
//   vs_pick_kernel      one workgroup: the largest vs_key(m[j], j) by dev_reduce.hpp's block_max (one barrier) - no atomic, so no order to
//                       depend on; thread 0 writes the round's select row, round[j*], the running sums, or `done`; every m is cleared.
//   vs_claim_kernel     the winner's segment, read from the record: claimed[w] |= bits.  A word occurs once per view: no atomic.
//   vs_final_kernel     claimed |= K, where claimed_out is asked for.
//   -- the last hand-over: the record and the outputs asked for, through their pinned copies.
// The routed selection: isdf_view_select_routed, the same sets and lists, the rounds by utility = marginal gain per travel cost.
//   vs_cost_kernel         one lane per view, after the gain: c_j = the ctx's cost-to-go field at the cell of the view's eye (field_cell.hpp's
//                          ff_cell, the field's own rule), or the caller's staged array; the scored views that are eligible, unreachable and
//                          over the budget, block_sum, one atomicAdd per counter and workgroup.
//   vs_marginal_kernel<true>  as above, and a view whose cost is not finite or above the budget is skipped (uniform).
//   vs_pick_util_kernel    one workgroup instead of vs_pick_kernel: every lane keeps the best of its views - the largest u = m / (cost0 + c),
//                          among equals the lowest j -, then block_max over the bit pattern of u plus one (u >= 0: the pattern orders as the
//                          value does, 0 stays "none") and block_max over VS_MAX_VIEWS - j among the lanes that hold the top.  No atomic.
//   vs_claim_kernel        unchanged.
//   vs_gather_eyes_kernel  with path_cap >= 1: the picked views' eyes as starts, a start outside the map for a round that did not happen;
//   (frontend_field.hip)   then isdf_frontend_field_paths_device on the same stream - no hand-over between the rounds and the paths.
// Nothing here writes to the ctx's map, its known grid, its field, its products or its flags; no kernel waits on another workgroup.
#include "view_gain_run.hpp"
#include "view_select_host.hpp"
#include "frontend_dev.hpp"
#include "field_cell.hpp"
#include "dev_reduce.hpp"
#include "dev_scan.hpp"
#include <algorithm>
#include <cstring>
#include <limits>
#include <vector>

namespace isdf {

constexpr int VS_BLOCK = 256;
constexpr int VS_WAVES = VS_BLOCK / 64;
constexpr unsigned VS_MAX_Y = 65535;            // gridDim.y
constexpr unsigned VS_MAX_X = 256;              // workgroups over a grid's words or a segment's entries
constexpr int VS_PER_LANE = 4;                  // words / entries a lane is sized for

struct VsEntry { unsigned w, bits; };           // a non-zero word of a view's set: its index in K's layout, its bits
static_assert(sizeof(VsEntry) == 8, "a list entry is 8 bytes");

// the call's record, zeroed before the first launch, read back after every chunk's scan and at the end
struct VsCtl {
    unsigned long long base;                // list entries so far: the next chunk's first segment starts here
    unsigned long long chunk_total;         // the last chunk's entries
    long long done;                         // the stop rule has ended the selection
    long long winner;                       // the last round's view
    long long n_selected, cumulative, solo_sum;
    double cost_selected;                   // the routed selection: the picked views' costs, added in pick order (zeroed as +0.0)
};

// the routed selection's counts over the scored views, zeroed before the cost kernel
struct VsCostRec { unsigned long long n_eligible, n_unreachable, n_over_budget, pad; };
static_assert(sizeof(VsCtl) == 64, "the selection's record is one 64-byte line");

__global__ __launch_bounds__(VS_BLOCK) void vs_begin_kernel(long long n_views, long long rounds, unsigned long long *__restrict__ count, unsigned long long *__restrict__ m,
                                                            long long *__restrict__ round, long long *__restrict__ select) {
    const long long i = (long long)blockIdx.x * VS_BLOCK + threadIdx.x;
    if (i < n_views) { count[i] = 0; m[i] = 0; round[i] = -1; }
    if (i < rounds) { select[VS_ROW * i] = -1; select[VS_ROW * i + 1] = select[VS_ROW * i + 2] = select[VS_ROW * i + 3] = 0; }
}

// seen: the chunk's grids, n_words each; view0 the chunk's first view
__global__ __launch_bounds__(VS_BLOCK) void vs_count_kernel(const unsigned *__restrict__ seen, long long n_words, long long view0, unsigned long long *count) {
    const unsigned *const g = seen + (size_t)blockIdx.y * (size_t)n_words;
    long long cnt[1] = {0};
    for (long long w = (long long)blockIdx.x * VS_BLOCK + threadIdx.x; w < n_words; w += (long long)gridDim.x * VS_BLOCK) cnt[0] += g[w] != 0u;
    const unsigned long long s = block_sum<1, VS_WAVES>(cnt);
    if (s) atomicAdd(count + view0 + blockIdx.y, s);            // (s is 0 beyond thread 0)
}

__global__ __launch_bounds__(VS_BLOCK) void vs_scan_kernel(long long view0, long long nv, const unsigned long long *__restrict__ count,
                                                           unsigned long long *__restrict__ start, unsigned long long *__restrict__ cursor, VsCtl *ctl) {
    __shared__ unsigned long long s_part[VS_BLOCK];
    const long long per = (nv + VS_BLOCK - 1) / VS_BLOCK;
    const long long lo = (long long)threadIdx.x * per < nv ? (long long)threadIdx.x * per : nv, hi = lo + per < nv ? lo + per : nv;
    unsigned long long sum = 0;
    for (long long i = lo; i < hi; i++) sum += count[view0 + i];
    s_part[threadIdx.x] = sum;
    const unsigned long long base = ctl->base;
    __syncthreads();
    for (int off = 1; off < VS_BLOCK; off <<= 1) {
        const unsigned long long v = (int)threadIdx.x >= off ? s_part[threadIdx.x - off] : 0ull;
        __syncthreads();
        s_part[threadIdx.x] += v;
        __syncthreads();
    }
    unsigned long long run = base + s_part[threadIdx.x] - sum;
    for (long long i = lo; i < hi; i++) {
        start[view0 + i] = run; cursor[view0 + i] = run;
        run += count[view0 + i];
    }
    if (threadIdx.x == VS_BLOCK - 1) { ctl->chunk_total = s_part[VS_BLOCK - 1]; ctl->base = base + s_part[VS_BLOCK - 1]; }     // (every thread read the base before the barriers)
}

// list: at least the record's base entries; a view's cursor ends at its segment's end, since the grids are what the count saw
__global__ __launch_bounds__(VS_BLOCK) void vs_fill_kernel(const unsigned *__restrict__ seen, long long n_words, long long view0, unsigned long long *cursor,
                                                           VsEntry *__restrict__ list) {
    const unsigned *const g = seen + (size_t)blockIdx.y * (size_t)n_words;
    const long long j = view0 + blockIdx.y;
    const int lane = threadIdx.x & 63;
    for (long long w0 = (long long)blockIdx.x * VS_BLOCK; w0 < n_words; w0 += (long long)gridDim.x * VS_BLOCK) {
        const long long w = w0 + threadIdx.x;
        const unsigned b = w < n_words ? g[w] : 0u;
        const unsigned long long mask = __ballot(b != 0u);
        if (mask == 0ull) continue;             // (uniform in the wavefront)
        const int leader = __ffsll((unsigned long long)mask) - 1;
        unsigned long long pos = 0;
        if (lane == leader) pos = atomicAdd(cursor + j, (unsigned long long)__popcll(mask));
        pos = __shfl(pos, leader, 64);
        if (b) list[pos + (unsigned long long)__popcll(mask & ((1ull << lane) - 1ull))] = VsEntry{(unsigned)w, b};
    }
}

// ROUTED: cost is the per-view travel cost and a view that is not eligible by it is skipped; else cost is null and never read
template <bool ROUTED>
__global__ __launch_bounds__(VS_BLOCK) void vs_marginal_kernel(long long n_views, const long long *__restrict__ rows, const long long *__restrict__ round,
                                                               const unsigned long long *__restrict__ start, const unsigned long long *__restrict__ count,
                                                               const VsEntry *__restrict__ list, const unsigned *__restrict__ claimed, unsigned long long *m,
                                                               const VsCtl *__restrict__ ctl, const double *__restrict__ cost, double max_cost) {
    if (ctl->done) return;          // (uniform)
    for (long long j = blockIdx.y; j < n_views; j += gridDim.y) {
        if (rows[VG_ROW * j] != VG_SCORED || round[j] >= 0) continue;           // (uniform)
        if (ROUTED && !vs_cost_eligible(cost[j], max_cost)) continue;           // (uniform)
        const unsigned long long n = count[j];
        if ((unsigned long long)blockIdx.x * VS_BLOCK >= n) continue;           // (uniform)
        const VsEntry *const seg = list + start[j];
        long long cnt[1] = {0};
        for (unsigned long long i = (unsigned long long)blockIdx.x * VS_BLOCK + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * VS_BLOCK) {
            const VsEntry e = seg[i];
            cnt[0] += __popc(e.bits & ~claimed[e.w]);
        }
        const unsigned long long s = block_sum<1, VS_WAVES>(cnt);
        if (s) atomicAdd(m + j, s);
        __syncthreads();            // (block_sum's LDS words are written again for the next view)
    }
}

__global__ __launch_bounds__(VS_BLOCK) void vs_pick_kernel(long long n_views, int r, long long min_gain, const long long *__restrict__ rows, long long *round,
                                                           unsigned long long *m, long long *__restrict__ select, VsCtl *ctl) {
    if (ctl->done) return;          // (uniform: thread 0 writes it after the barrier)
    unsigned long long top = 0;
    for (long long j = threadIdx.x; j < n_views; j += VS_BLOCK) {
        const unsigned long long mj = m[j];
        m[j] = 0;                   // for the next round
        if (rows[VG_ROW * j] != VG_SCORED || round[j] >= 0) continue;
        const unsigned long long key = vs_key((long long)mj, j);
        top = key > top ? key : top;
    }
    top = block_max<VS_WAVES, false>(top);          // (called once: no second barrier)
    if (threadIdx.x != 0) return;
    if (top == 0 || vs_key_marginal(top) < min_gain) { ctl->done = 1; return; }
    const long long j = vs_key_view(top), marginal = vs_key_marginal(top), gain = rows[VG_ROW * j + 1];
    const long long cumulative = ctl->cumulative + marginal;
    long long *const s = select + (long long)VS_ROW * r;
    s[0] = j; s[1] = marginal; s[2] = cumulative; s[3] = gain - marginal;
    round[j] = r;
    ctl->winner = j; ctl->n_selected = r + 1; ctl->cumulative = cumulative; ctl->solo_sum += gain;
}

// One lane per view.  staged null: c_j from the field d (the map's X Y Z doubles) at the eye's cell, +inf outside the map - what
// ff_value_kernel answers for the eye; else the caller's array.  rows are the gain's: the counts are over the scored views.
__global__ __launch_bounds__(VS_BLOCK) void vs_cost_kernel(long long n_views, FfMap M, const double *__restrict__ d, const double *__restrict__ poses,
                                                           const double *__restrict__ staged, const long long *__restrict__ rows, double max_cost,
                                                           double *__restrict__ cost, VsCostRec *rec) {
    const long long j = (long long)blockIdx.x * VS_BLOCK + threadIdx.x;
    long long cnt[3] = {0, 0, 0};
    if (j < n_views) {
        double cj;
        if (staged) cj = staged[j];
        else {
            const double p[3] = {poses[12 * j + 3], poses[12 * j + 7], poses[12 * j + 11]};
            int cell[3];
            cj = ff_cell(M, p, cell) ? d[((size_t)cell[0] * M.Y + cell[1]) * M.Z + cell[2]] : __longlong_as_double(0x7FF0000000000000ll);
        }
        cost[j] = cj;
        if (rows[VG_ROW * j] == VG_SCORED) cnt[!vs_cost_finite(cj) ? 1 : !(cj <= max_cost) ? 2 : 0] = 1;
    }
    const unsigned long long s = block_sum<3, VS_WAVES>(cnt);
    if (threadIdx.x < 3 && s) atomicAdd(&rec->n_eligible + threadIdx.x, s);         // (the record's first three words, in the order of cnt)
}

__global__ __launch_bounds__(VS_BLOCK) void vs_pick_util_kernel(long long n_views, int r, long long min_gain, double cost0, double max_cost,
                                                                const long long *__restrict__ rows, const double *__restrict__ cost, long long *round,
                                                                unsigned long long *m, long long *__restrict__ select, double *__restrict__ util, VsCtl *ctl) {
    if (ctl->done) return;          // (uniform: thread 0 writes it after a barrier)
    __shared__ unsigned long long s_marginal;
    unsigned long long key = 0, best_m = 0;
    long long best_j = 0;
    for (long long j = threadIdx.x; j < n_views; j += VS_BLOCK) {
        const unsigned long long mj = m[j];
        m[j] = 0;                   // for the next round
        if (rows[VG_ROW * j] != VG_SCORED || round[j] >= 0 || !vs_cost_eligible(cost[j], max_cost) || (long long)mj < min_gain) continue;
        const unsigned long long k = (unsigned long long)__double_as_longlong(vs_utility((long long)mj, cost0, cost[j])) + 1ull;
        if (k > key) { key = k; best_m = mj; best_j = j; }          // (j rises in a lane: among equals the lowest stays)
    }
    const unsigned long long top = block_max<VS_WAVES, true>(key);
    if (top == 0) {                 // (uniform: every thread holds the top)
        if (threadIdx.x == 0) ctl->done = 1;
        return;
    }
    const long long j = VS_MAX_VIEWS - (long long)block_max<VS_WAVES, false>(key == top ? (unsigned long long)(VS_MAX_VIEWS - best_j) : 0ull);
    if (key == top && best_j == j) s_marginal = best_m;             // (one lane: a view belongs to one lane)
    __syncthreads();
    if (threadIdx.x != 0) return;
    const long long marginal = (long long)s_marginal, gain = rows[VG_ROW * j + 1];
    const long long cumulative = ctl->cumulative + marginal;
    const double c = cost[j];
    long long *const s = select + (long long)VS_ROW * r;
    s[0] = j; s[1] = marginal; s[2] = cumulative; s[3] = gain - marginal;
    util[2 * r] = c; util[2 * r + 1] = __longlong_as_double((long long)(top - 1ull));
    round[j] = r;
    ctl->winner = j; ctl->n_selected = r + 1; ctl->cumulative = cumulative; ctl->solo_sum += gain; ctl->cost_selected += c;
}

// starts: rounds x 3, the eye of round r's view, or a point outside every map for a round that did not happen (its path has n = 0)
__global__ __launch_bounds__(VS_BLOCK) void vs_gather_eyes_kernel(long long rounds, const long long *__restrict__ select, const double *__restrict__ poses,
                                                                  double *__restrict__ starts) {
    const long long r = (long long)blockIdx.x * VS_BLOCK + threadIdx.x;
    if (r >= rounds) return;
    const long long j = select[VS_ROW * r];
    for (int a = 0; a < 3; a++) starts[3 * r + a] = j >= 0 ? poses[12 * j + 3 + 4 * a] : __longlong_as_double((long long)0xFFF0000000000000ull);
}

__global__ __launch_bounds__(VS_BLOCK) void vs_claim_kernel(const unsigned long long *__restrict__ start, const unsigned long long *__restrict__ count,
                                                            const VsEntry *__restrict__ list, unsigned *claimed, const VsCtl *__restrict__ ctl) {
    if (ctl->done) return;          // (uniform)
    const long long j = ctl->winner;
    const unsigned long long n = count[j];
    const VsEntry *const seg = list + start[j];
    for (unsigned long long i = (unsigned long long)blockIdx.x * VS_BLOCK + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * VS_BLOCK) {
        const VsEntry e = seg[i];
        claimed[e.w] |= e.bits;
    }
}

__global__ __launch_bounds__(VS_BLOCK) void vs_final_kernel(const unsigned *__restrict__ known, unsigned *__restrict__ claimed, long long n_words) {
    const long long w = (long long)blockIdx.x * VS_BLOCK + threadIdx.x;
    if (w < n_words) claimed[w] |= known[w];
}

}  // namespace isdf

// the poses' staging, the rows, the per-view counts, segment starts, cursors, marginals and rounds, the select rows, the list, the claimed
// grid, the call's record and the pinned copies the outputs are handed over through
struct ViewSelectState {
    isdf::DevBuf<double> d_poses;
    isdf::DevBuf<long long> d_rows, d_round, d_select;
    isdf::DevBuf<unsigned long long> d_count, d_start, d_cursor, d_m;
    isdf::DevBuf<isdf::VsEntry> d_list;
    isdf::DevBuf<unsigned> d_claimed;
    isdf::RecPair<isdf::VsCtl> ctl;
    isdf::PinBuf<int64_t> h_rows, h_select, h_round;
    isdf::PinBuf<uint32_t> h_claimed;
    isdf::DevEvents<2> ev_gain, ev_lists, ev_fill, ev_select;
    // the routed selection's: the staged and the per-view costs, the rounds' {cost, utility}, the picked eyes and their paths
    isdf::DevBuf<double> d_cost_in, d_cost, d_util, d_starts, d_path_xyz, d_path_rp;
    isdf::DevBuf<int32_t> d_path_n;
    isdf::RecPair<isdf::VsCostRec> cost_rec;
    isdf::PinBuf<double> h_cost, h_util, h_path_xyz, h_path_rp;
    isdf::PinBuf<int32_t> h_path_n;
    isdf::DevEvents<2> ev_cost, ev_paths;
    int ready(isdf_ctx *c) {
        ISDF_TRY(ev_gain.ready(c)); ISDF_TRY(ev_lists.ready(c)); ISDF_TRY(ev_fill.ready(c)); ISDF_TRY(ev_select.ready(c));
        ISDF_TRY(ev_cost.ready(c)); ISDF_TRY(ev_paths.ready(c)); ISDF_TRY(cost_rec.ready(c));
        return ctl.ready(c);
    }
};

using namespace isdf;

extern "C" void isdf_view_select_params_default(isdf_view_select_params *p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    isdf_view_gain_params_default(&p->gain);
    p->k_select = 4;
    p->min_gain = 1;
}

extern "C" void isdf_view_select_sizes(int sizes_out[2]) {
    if (!sizes_out) return;
    sizes_out[0] = (int)sizeof(isdf_view_select_params); sizes_out[1] = (int)sizeof(isdf_view_select_info);
}

extern "C" void isdf_view_select_routed_params_default(isdf_view_select_routed_params *p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    isdf_view_select_params_default(&p->select);
    p->cost0 = 1.0;
    p->max_cost = std::numeric_limits<double>::infinity();
}

extern "C" void isdf_view_select_routed_sizes(int sizes_out[2]) {
    if (!sizes_out) return;
    sizes_out[0] = (int)sizeof(isdf_view_select_routed_params); sizes_out[1] = (int)sizeof(isdf_view_select_routed_info);
}

namespace {

// what the device and the host forms check and set up alike (c may be null: the host form)
int select_setup(isdf_ctx *c, const isdf_depth_camera *cam, const double *poses, long long n_views, const isdf_view_select_params &P, const MapGeom &M,
                 isdf_view_gain_params &Pg, DcRays &base) {
    ISDF_TRY(gain_setup(c, cam, poses, n_views, &P.gain, poses, M, Pg, base));          // (rows_out is nullable here: the poses stand in for it)
    if (P.k_select < 1 || P.min_gain < 0) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "bad view select parameters (k_select >= 1, min_gain >= 0)");
    if (n_views > VS_MAX_VIEWS) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "view select: more than 2^24 views");
    return ISDF_OK;
}

void select_info(long long n_views, const VsCounts &N, int chunks, double gain_ms, double lists_ms, double select_ms, isdf_view_select_info *out) {
    isdf_view_select_info info{};
    info.n_views = n_views; info.n_scored = N.n_scored; info.n_selected = N.n_selected;
    info.gain_selected = N.gain_selected; info.gain_solo_sum = N.gain_solo_sum; info.best_single_gain = N.best_single_gain;
    info.list_words = N.list_words;
    info.chunks = chunks; info.gain_ms = gain_ms; info.lists_ms = lists_ms; info.select_ms = select_ms;
    *out = info;
}

void select_pad(int64_t *select, long long from, long long k_select) {
    for (long long r = from; r < k_select; r++) {
        select[VS_ROW * r] = -1;
        select[VS_ROW * r + 1] = select[VS_ROW * r + 2] = select[VS_ROW * r + 3] = 0;
    }
}

// the routed call's additions to the selection's arguments (null: isdf_view_select)
struct VsRoute {
    const double *cost;             // the caller's array, or null: the ctx's field
    double cost0, max_cost;
    int path_cap;                   // 0: no paths
    double *cost_out, *util_out;
    int32_t *path_n_out;
    double *path_xyz_out, *path_rp_out;
    isdf_view_select_routed_info *info_out;
};

// the routed form's own argument rules, after the selection's (c may be null: the host form, which has no paths)
int route_check(isdf_ctx *c, const isdf_view_select_routed_params &P, const double *cost, long long n_views) {
    if (P.select.min_gain < 1) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "routed view select: min_gain >= 1 (with a utility a view that adds nothing is never picked)");
    if (!(P.cost0 > 0.0) || !vs_cost_finite(P.cost0) || !(P.max_cost >= 0.0) || P.path_cap < 0)
        return isdf_fail(c, ISDF_ERR_INVALID_ARG, "bad routed view select parameters (cost0 finite and > 0, max_cost >= 0, path_cap >= 0)");
    if (cost && P.path_cap >= 1) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "routed view select: paths are read off the ctx's field, not with a cost array");
    if (cost)
        for (long long j = 0; j < n_views; j++)
            if (!(cost[j] >= 0.0)) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "routed view select: a cost is negative or not a number");
    return ISDF_OK;
}

void route_info(const VsRouteCounts &R, int source, double cost_ms, double paths_ms, isdf_view_select_routed_info *out) {
    out->n_eligible = R.n_eligible; out->n_unreachable = R.n_unreachable; out->n_over_budget = R.n_over_budget;
    out->cost_selected = R.cost_selected; out->cost_source = source; out->reserved = 0; out->cost_ms = cost_ms; out->paths_ms = paths_ms;
}

// what a round that did not happen leaves in the routed outputs, from round `from` on
void route_pad(const VsRoute &R, long long from, long long k_select) {
    const size_t cap = (size_t)R.path_cap, n = (size_t)(k_select - from);
    if (R.util_out) std::memset(R.util_out + 2 * from, 0, n * 2 * sizeof(double));
    if (cap == 0) return;
    if (R.path_n_out) std::memset(R.path_n_out + from, 0, n * sizeof(int32_t));
    if (R.path_xyz_out) std::memset(R.path_xyz_out + (size_t)from * cap * 3, 0, n * cap * 3 * sizeof(double));
    if (R.path_rp_out) std::memset(R.path_rp_out + (size_t)from * cap * 2, 0, n * cap * 2 * sizeof(double));
}

// workgroups over n words or entries, each lane sized for a few
unsigned wide_blocks(long long n) { return (unsigned)std::min<long long>(std::max<long long>((n + VS_BLOCK * VS_PER_LANE - 1) / (VS_BLOCK * VS_PER_LANE), 1), VS_MAX_X); }

// the list holds `used` entries and is to hold `need`: grow-only, the content kept
int list_reserve(isdf_ctx *c, ViewSelectState *S, size_t need, size_t used, hipStream_t st) {
    const size_t cap = S->d_list.capacity();
    if (need <= cap) return ISDF_OK;
    DevBuf<VsEntry> bigger;
    const hipError_t e = bigger.alloc(std::max(need, cap + cap / 2));
    if (e != hipSuccess) return isdf_hip_fail(c, "the view selection's list", e);
    if (used > 0) HIPCHK(c, hipMemcpyAsync(bigger.get(), S->d_list.get(), used * sizeof(VsEntry), hipMemcpyDeviceToDevice, st));
    HIPCHK(c, hipStreamSynchronize(st));
    S->d_list.swap(bigger);
    return ISDF_OK;         // (the smaller one goes here)
}

// The body of both entries.  route null: isdf_view_select, which launches what it always launched; else PR are the routed call's
// parameters (P = PR->select) and the cost kernel, the routed marginal and pick kernels and the paths join in.
int select_run(isdf_ctx *c, const isdf_depth_camera *cam, const double *poses, long long n_views, const isdf_view_select_params &P, const VsRoute *route,
               const isdf_view_select_routed_params *PR, int64_t *rows_out, int64_t *select_out, int64_t *round_out, uint32_t *claimed_out, isdf_view_select_info *info_out) {
    const MapGeom M = map_geom(c->grid);            // (without a map: zeros, and the state check below refuses)
    isdf_view_gain_params Pg;
    DcRays base;
    ISDF_TRY(select_setup(c, cam, poses, n_views, P, M, Pg, base));
    ISDF_TRY(map_query::single_device(c, "the view selection is not offered on a multi-device ctx"));
    ISDF_TRY(map_query::has_occupancy(c, "the view selection"));
    ISDF_TRY(map_query::has_known(c, "the view selection needs a known grid (isdf_map_known_enable)"));
    if (route) {
        ISDF_TRY(route_check(c, *PR, route->cost, n_views));
        if (!route->cost) ISDF_TRY(isdf_field_read_ready(c));
    }
    const bool paths = route && route->path_cap >= 1;
    ViewSelectState *S;
    ViewGainState *G;
    ISDF_TRY(map_query::state_of(c, c->vsl, &S));
    ISDF_TRY(map_query::state_of(c, c->vgn, &G));
    const hipStream_t st = c->stream;
    const long long n_words = (long long)c->known.n_words;
    const size_t nw = (size_t)n_words, nv = (size_t)n_views;
    const unsigned *const d_known = (const unsigned *)c->known.d_bits.get();
    VsCounts N;
    if (claimed_out) ISDF_TRY(S->h_claimed.reserve(c, nw));
    if (n_views == 0) {             // nothing is launched: claimed_out is K
        if (claimed_out) {
            HIPCHK(c, hipMemcpyAsync(S->h_claimed.get(), d_known, nw * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipStreamSynchronize(st));
            std::memcpy(claimed_out, S->h_claimed.get(), nw * sizeof(uint32_t));
        }
        if (select_out) select_pad(select_out, 0, P.k_select);
        if (info_out) select_info(0, N, 0, 0.0, 0.0, 0.0, info_out);
        if (route) {
            route_pad(*route, 0, P.k_select);
            if (route->info_out) route_info(VsRouteCounts(), route->cost ? 1 : 0, 0.0, 0.0, route->info_out);
        }
        return ISDF_OK;
    }
    const long long rounds = std::min<long long>(P.k_select, n_views);          // a view is picked once: no later round can pick
    const bool want_rows = rows_out != nullptr || info_out != nullptr;
    ISDF_TRY(S->d_poses.reserve(c, nv * 12)); ISDF_TRY(S->d_rows.reserve(c, nv * VG_ROW)); ISDF_TRY(S->d_round.reserve(c, nv));
    ISDF_TRY(S->d_select.reserve(c, (size_t)rounds * VS_ROW));
    ISDF_TRY(S->d_count.reserve(c, nv)); ISDF_TRY(S->d_start.reserve(c, nv)); ISDF_TRY(S->d_cursor.reserve(c, nv)); ISDF_TRY(S->d_m.reserve(c, nv));
    ISDF_TRY(S->d_claimed.reserve(c, nw));
    if (want_rows) ISDF_TRY(S->h_rows.reserve(c, nv * VG_ROW));
    if (select_out) ISDF_TRY(S->h_select.reserve(c, (size_t)rounds * VS_ROW));
    if (round_out) ISDF_TRY(S->h_round.reserve(c, nv));
    const size_t nr = (size_t)rounds, cap = route ? (size_t)route->path_cap : 0;
    if (route) {
        if (route->cost) ISDF_TRY(S->d_cost_in.reserve(c, nv));
        ISDF_TRY(S->d_cost.reserve(c, nv)); ISDF_TRY(S->d_util.reserve(c, nr * 2));
        if (route->cost_out) ISDF_TRY(S->h_cost.reserve(c, nv));
        if (route->util_out) ISDF_TRY(S->h_util.reserve(c, nr * 2));
    }
    if (paths) {
        if (nr * cap > (size_t)0x7FFFFFFF) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "routed view select: rounds x path_cap above 2^31 - 1");
        ISDF_TRY(S->d_starts.reserve(c, nr * 3)); ISDF_TRY(S->d_path_n.reserve(c, nr));
        ISDF_TRY(S->d_path_xyz.reserve(c, nr * cap * 3)); ISDF_TRY(S->d_path_rp.reserve(c, nr * cap * 2));
        if (route->path_n_out) ISDF_TRY(S->h_path_n.reserve(c, nr));
        if (route->path_xyz_out) ISDF_TRY(S->h_path_xyz.reserve(c, nr * cap * 3));
        if (route->path_rp_out) ISDF_TRY(S->h_path_rp.reserve(c, nr * cap * 2));
    }
    HIPCHK(c, hipMemcpyAsync(S->d_poses, poses, nv * 12 * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(c, S->ctl.zero(st));
    if (route) {
        if (route->cost) HIPCHK(c, hipMemcpyAsync(S->d_cost_in, route->cost, nv * sizeof(double), hipMemcpyHostToDevice, st));
        HIPCHK(c, S->cost_rec.zero(st));
        HIPCHK(c, hipMemsetAsync(S->d_util, 0, nr * 2 * sizeof(double), st));            // (a round that did not happen: {0, 0})
    }
    HIPCHK(c, hipMemsetAsync(S->d_claimed, 0, nw * sizeof(unsigned), st));
    // (n_views >= 1 here and a known grid has n_words >= 1: blocks() is at least one workgroup at both of its uses below)
    hipLaunchKernelGGL(vs_begin_kernel, dim3(blocks(std::max(n_views, rounds), VS_BLOCK)), dim3(VS_BLOCK), 0, st, n_views, rounds, S->d_count.get(), S->d_m.get(),
                       S->d_round.get(), S->d_select.get());
    HIPCHK(c, hipGetLastError());
    // the gain, and after every chunk its views' lists
    double lists_ms = 0.0;
    bool fill_pending = false;
    unsigned long long longest_chunk = 0;
    const unsigned word_bx = wide_blocks(n_words);
    const GainChunkHook lists = [&](long long view0, long long n, const unsigned *d_seen, long long words) -> int {
        HIPCHK(c, hipEventRecord(S->ev_lists[0], st));
        hipLaunchKernelGGL(vs_count_kernel, dim3(word_bx, (unsigned)n), dim3(VS_BLOCK), 0, st, d_seen, words, view0, S->d_count.get());
        hipLaunchKernelGGL(vs_scan_kernel, dim3(1), dim3(VS_BLOCK), 0, st, view0, n, (const unsigned long long *)S->d_count.get(), S->d_start.get(), S->d_cursor.get(),
                           S->ctl.dev());
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipEventRecord(S->ev_lists[1], st));
        HIPCHK(c, S->ctl.fetch(st));
        HIPCHK(c, hipStreamSynchronize(st));            // the chunk's hand-over (the last chunk's fill is over too)
        lists_ms += S->ev_lists.ms(0, 1) + (fill_pending ? S->ev_fill.ms(0, 1) : 0.0);
        fill_pending = false;
        const VsCtl R = S->ctl.host();
        longest_chunk = std::max(longest_chunk, R.chunk_total);
        if (R.chunk_total == 0) return ISDF_OK;
        ISDF_TRY(list_reserve(c, S, (size_t)R.base, (size_t)(R.base - R.chunk_total), st));
        HIPCHK(c, hipEventRecord(S->ev_fill[0], st));
        hipLaunchKernelGGL(vs_fill_kernel, dim3(word_bx, (unsigned)n), dim3(VS_BLOCK), 0, st, d_seen, words, view0, S->d_cursor.get(), S->d_list.get());
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipEventRecord(S->ev_fill[1], st));
        fill_pending = true;
        return ISDF_OK;
    };
    int chunks = 0;
    ISDF_TRY(map_query::count_begin(c, true, S->ev_gain, st));
    ISDF_TRY(gain_run(c, G, base, M, Pg, S->d_poses.get(), n_views, S->d_rows.get(), false, &chunks, st, &lists));
    ISDF_TRY(map_query::count_end(c, true, S->ev_gain, st));
    if (route) {                    // the costs, once the rows are the gain's
        ISDF_TRY(map_query::count_begin(c, true, S->ev_cost, st));
        hipLaunchKernelGGL(vs_cost_kernel, dim3(blocks(n_views, VS_BLOCK)), dim3(VS_BLOCK), 0, st, n_views, ff_map(c), (const double *)c->fe.d_field.get(),
                           (const double *)S->d_poses.get(), route->cost ? (const double *)S->d_cost_in.get() : (const double *)nullptr, (const long long *)S->d_rows.get(),
                           route->max_cost, S->d_cost.get(), S->cost_rec.dev());
        HIPCHK(c, hipGetLastError());
        ISDF_TRY(map_query::count_end(c, true, S->ev_cost, st));
    }
    // the rounds: a fixed sequence, no hand-over between them
    ISDF_TRY(list_reserve(c, S, 1, 0, st));             // (no entry at all: the kernels still take a pointer)
    const unsigned seg_bx = wide_blocks((long long)std::min<unsigned long long>(longest_chunk, (unsigned long long)n_words));          // a segment has at most n_words entries
    const unsigned view_by = (unsigned)std::min<long long>(n_views, VS_MAX_Y);
    ISDF_TRY(map_query::count_begin(c, true, S->ev_select, st));
    for (long long r = 0; r < rounds; r++) {
        if (route) {
            hipLaunchKernelGGL(vs_marginal_kernel<true>, dim3(seg_bx, view_by), dim3(VS_BLOCK), 0, st, n_views, (const long long *)S->d_rows.get(),
                               (const long long *)S->d_round.get(), (const unsigned long long *)S->d_start.get(), (const unsigned long long *)S->d_count.get(),
                               (const VsEntry *)S->d_list.get(), (const unsigned *)S->d_claimed.get(), S->d_m.get(), (const VsCtl *)S->ctl.dev(),
                               (const double *)S->d_cost.get(), route->max_cost);
            hipLaunchKernelGGL(vs_pick_util_kernel, dim3(1), dim3(VS_BLOCK), 0, st, n_views, (int)r, (long long)P.min_gain, route->cost0, route->max_cost,
                               (const long long *)S->d_rows.get(), (const double *)S->d_cost.get(), S->d_round.get(), S->d_m.get(), S->d_select.get(), S->d_util.get(),
                               S->ctl.dev());
        } else {
            hipLaunchKernelGGL(vs_marginal_kernel<false>, dim3(seg_bx, view_by), dim3(VS_BLOCK), 0, st, n_views, (const long long *)S->d_rows.get(),
                               (const long long *)S->d_round.get(), (const unsigned long long *)S->d_start.get(), (const unsigned long long *)S->d_count.get(),
                               (const VsEntry *)S->d_list.get(), (const unsigned *)S->d_claimed.get(), S->d_m.get(), (const VsCtl *)S->ctl.dev(),
                               (const double *)nullptr, 0.0);
            hipLaunchKernelGGL(vs_pick_kernel, dim3(1), dim3(VS_BLOCK), 0, st, n_views, (int)r, (long long)P.min_gain, (const long long *)S->d_rows.get(), S->d_round.get(),
                               S->d_m.get(), S->d_select.get(), S->ctl.dev());
        }
        hipLaunchKernelGGL(vs_claim_kernel, dim3(seg_bx), dim3(VS_BLOCK), 0, st, (const unsigned long long *)S->d_start.get(), (const unsigned long long *)S->d_count.get(),
                           (const VsEntry *)S->d_list.get(), S->d_claimed.get(), (const VsCtl *)S->ctl.dev());
        HIPCHK(c, hipGetLastError());
    }
    if (claimed_out) {
        hipLaunchKernelGGL(vs_final_kernel, dim3(blocks(n_words, VS_BLOCK)), dim3(VS_BLOCK), 0, st, d_known, S->d_claimed.get(), n_words);
        HIPCHK(c, hipGetLastError());
    }
    ISDF_TRY(map_query::count_end(c, true, S->ev_select, st));
    if (paths) {                    // the ways to the picked eyes, behind the rounds on the same stream; rows come back whole: zero past a path's end
        ISDF_TRY(map_query::count_begin(c, true, S->ev_paths, st));
        HIPCHK(c, hipMemsetAsync(S->d_path_xyz, 0, nr * cap * 3 * sizeof(double), st));
        HIPCHK(c, hipMemsetAsync(S->d_path_rp, 0, nr * cap * 2 * sizeof(double), st));
        hipLaunchKernelGGL(vs_gather_eyes_kernel, dim3(blocks(rounds, VS_BLOCK)), dim3(VS_BLOCK), 0, st, rounds, (const long long *)S->d_select.get(),
                           (const double *)S->d_poses.get(), S->d_starts.get());
        HIPCHK(c, hipGetLastError());
        ISDF_TRY(isdf_frontend_field_paths_device(c, S->d_starts.get(), (int)rounds, route->path_cap, S->d_path_n.get(), S->d_path_xyz.get(), S->d_path_rp.get(), (void *)st));
        ISDF_TRY(map_query::count_end(c, true, S->ev_paths, st));
    }
    // the last hand-over: the record and the outputs asked for, through the pinned copies
    HIPCHK(c, S->ctl.fetch(st));
    if (route) {
        HIPCHK(c, S->cost_rec.fetch(st));
        if (route->cost_out) HIPCHK(c, hipMemcpyAsync(S->h_cost.get(), S->d_cost, nv * sizeof(double), hipMemcpyDeviceToHost, st));
        if (route->util_out) HIPCHK(c, hipMemcpyAsync(S->h_util.get(), S->d_util, nr * 2 * sizeof(double), hipMemcpyDeviceToHost, st));
        if (paths && route->path_n_out) HIPCHK(c, hipMemcpyAsync(S->h_path_n.get(), S->d_path_n, nr * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        if (paths && route->path_xyz_out) HIPCHK(c, hipMemcpyAsync(S->h_path_xyz.get(), S->d_path_xyz, nr * cap * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
        if (paths && route->path_rp_out) HIPCHK(c, hipMemcpyAsync(S->h_path_rp.get(), S->d_path_rp, nr * cap * 2 * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    if (want_rows) HIPCHK(c, hipMemcpyAsync(S->h_rows.get(), S->d_rows, nv * VG_ROW * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    if (select_out) HIPCHK(c, hipMemcpyAsync(S->h_select.get(), S->d_select, (size_t)rounds * VS_ROW * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    if (round_out) HIPCHK(c, hipMemcpyAsync(S->h_round.get(), S->d_round, nv * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    if (claimed_out) HIPCHK(c, hipMemcpyAsync(S->h_claimed.get(), S->d_claimed, nw * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (fill_pending) lists_ms += S->ev_fill.ms(0, 1);
    if (rows_out) std::memcpy(rows_out, S->h_rows.get(), nv * VG_ROW * sizeof(int64_t));
    if (select_out) {
        std::memcpy(select_out, S->h_select.get(), (size_t)rounds * VS_ROW * sizeof(int64_t));
        select_pad(select_out, rounds, P.k_select);
    }
    if (round_out) std::memcpy(round_out, S->h_round.get(), nv * sizeof(int64_t));
    if (claimed_out) std::memcpy(claimed_out, S->h_claimed.get(), nw * sizeof(uint32_t));
    if (info_out) {
        const VsCtl R = S->ctl.host();
        vs_counts_of_rows(S->h_rows.get(), n_views, N);
        N.n_selected = R.n_selected; N.gain_selected = R.cumulative; N.gain_solo_sum = R.solo_sum; N.list_words = (long long)R.base;
        select_info(n_views, N, chunks, std::max(S->ev_gain.ms(0, 1) - lists_ms, 0.0), lists_ms, S->ev_select.ms(0, 1), info_out);
    }
    if (route) {
        if (route->cost_out) std::memcpy(route->cost_out, S->h_cost.get(), nv * sizeof(double));
        if (route->util_out) std::memcpy(route->util_out, S->h_util.get(), nr * 2 * sizeof(double));
        if (paths && route->path_n_out) std::memcpy(route->path_n_out, S->h_path_n.get(), nr * sizeof(int32_t));
        if (paths && route->path_xyz_out) std::memcpy(route->path_xyz_out, S->h_path_xyz.get(), nr * cap * 3 * sizeof(double));
        if (paths && route->path_rp_out) std::memcpy(route->path_rp_out, S->h_path_rp.get(), nr * cap * 2 * sizeof(double));
        route_pad(*route, rounds, P.k_select);
        if (route->info_out) {
            const VsCostRec &K = S->cost_rec.host();
            VsRouteCounts R;
            R.n_eligible = (long long)K.n_eligible; R.n_unreachable = (long long)K.n_unreachable; R.n_over_budget = (long long)K.n_over_budget;
            R.cost_selected = S->ctl.host().cost_selected;
            route_info(R, route->cost ? 1 : 0, S->ev_cost.ms(0, 1), paths ? S->ev_paths.ms(0, 1) : 0.0, route->info_out);
        }
    }
    return ISDF_OK;
}

}  // namespace

extern "C" int isdf_view_select(isdf_ctx *c, const isdf_depth_camera *cam, const double *poses, long long n_views, const isdf_view_select_params *params, int64_t *rows_out,
                                int64_t *select_out, int64_t *round_out, uint32_t *claimed_out, isdf_view_select_info *info_out) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    const isdf_view_select_params P = map_query::resolve(params, isdf_view_select_params_default);
    return select_run(c, cam, poses, n_views, P, nullptr, nullptr, rows_out, select_out, round_out, claimed_out, info_out);
}

extern "C" int isdf_view_select_routed(isdf_ctx *c, const isdf_depth_camera *cam, const double *poses, long long n_views, const double *cost,
                                       const isdf_view_select_routed_params *params, int64_t *rows_out, int64_t *select_out, int64_t *round_out, uint32_t *claimed_out,
                                       double *cost_out, double *util_out, int32_t *path_n_out, double *path_xyz_out, double *path_rp_out,
                                       isdf_view_select_routed_info *info_out) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    const isdf_view_select_routed_params P = map_query::resolve(params, isdf_view_select_routed_params_default);
    const VsRoute route{cost, P.cost0, P.max_cost, P.path_cap, cost_out, util_out, path_n_out, path_xyz_out, path_rp_out, info_out};
    // (the info's rows: the selection's words are filled through the same pointer the plain entry takes)
    return select_run(c, cam, poses, n_views, P.select, &route, &P, rows_out, select_out, round_out, claimed_out, info_out ? &info_out->select : nullptr);
}

extern "C" int isdf_view_select_host(const uint32_t *bits, const uint8_t *occ, const double bmin[3], const double bmax[3], double resolution, const int32_t dims[3],
                                     const isdf_depth_camera *cam, const double *poses, long long n_views, const isdf_view_select_params *params, int64_t *rows_out,
                                     int64_t *select_out, int64_t *round_out, uint32_t *claimed_out, isdf_view_select_info *info_out) {
    if (ms_geometry_bad(bmin, bmax, resolution, dims) || !bits || !occ) return isdf_fail(nullptr, ISDF_ERR_INVALID_ARG, "view select (host form): bad arguments");
    const MapGeom M = map_geom(bmin, bmax, resolution, dims);
    const isdf_view_select_params P = map_query::resolve(params, isdf_view_select_params_default);
    isdf_view_gain_params Pg;
    DcRays base;
    ISDF_TRY(select_setup(nullptr, cam, poses, n_views, P, M, Pg, base));
    const size_t nw = (size_t)mk_words(mk_voxels(dims)), nv = (size_t)n_views;
    std::vector<int64_t> rows(rows_out ? 0 : nv * VG_ROW), select(select_out ? 0 : (size_t)P.k_select * VS_ROW), round(round_out ? 0 : nv);
    std::vector<uint32_t> claimed(claimed_out ? 0 : nw);
    VsCounts N;
    vs_select_host(bits, occ, M, base, poses, n_views, P.k_select, P.min_gain, rows_out ? rows_out : rows.data(), select_out ? select_out : select.data(),
                   round_out ? round_out : round.data(), claimed_out ? claimed_out : claimed.data(), N);
    if (info_out) select_info(n_views, N, 0, 0.0, 0.0, 0.0, info_out);
    return ISDF_OK;
}

extern "C" int isdf_view_select_routed_host(const uint32_t *bits, const uint8_t *occ, const double bmin[3], const double bmax[3], double resolution, const int32_t dims[3],
                                            const isdf_depth_camera *cam, const double *poses, long long n_views, const double *cost,
                                            const isdf_view_select_routed_params *params, int64_t *rows_out, int64_t *select_out, int64_t *round_out, uint32_t *claimed_out,
                                            double *cost_out, double *util_out, isdf_view_select_routed_info *info_out) {
    if (ms_geometry_bad(bmin, bmax, resolution, dims) || !bits || !occ) return isdf_fail(nullptr, ISDF_ERR_INVALID_ARG, "routed view select (host form): bad arguments");
    const MapGeom M = map_geom(bmin, bmax, resolution, dims);
    const isdf_view_select_routed_params P = map_query::resolve(params, isdf_view_select_routed_params_default);
    isdf_view_gain_params Pg;
    DcRays base;
    ISDF_TRY(select_setup(nullptr, cam, poses, n_views, P.select, M, Pg, base));
    ISDF_TRY(route_check(nullptr, P, cost, n_views));
    if (P.path_cap != 0) return isdf_fail(nullptr, ISDF_ERR_INVALID_ARG, "routed view select (host form): no paths (path_cap = 0)");
    if (n_views > 0 && !cost) return isdf_fail(nullptr, ISDF_ERR_INVALID_ARG, "routed view select (host form): a cost array is required");
    const size_t nw = (size_t)mk_words(mk_voxels(dims)), nv = (size_t)n_views, k = (size_t)P.select.k_select;
    std::vector<int64_t> rows(rows_out ? 0 : nv * VG_ROW), select(select_out ? 0 : k * VS_ROW), round(round_out ? 0 : nv);
    std::vector<uint32_t> claimed(claimed_out ? 0 : nw);
    std::vector<double> util(util_out ? 0 : k * 2);
    VsCounts N;
    VsRouteCounts R;
    vs_select_routed_host(bits, occ, M, base, poses, n_views, P.select.k_select, P.select.min_gain, cost, P.cost0, P.max_cost, rows_out ? rows_out : rows.data(),
                          select_out ? select_out : select.data(), round_out ? round_out : round.data(), claimed_out ? claimed_out : claimed.data(),
                          util_out ? util_out : util.data(), N, R);
    if (cost_out && nv) std::memcpy(cost_out, cost, nv * sizeof(double));
    if (info_out) {
        select_info(n_views, N, 0, 0.0, 0.0, 0.0, &info_out->select);
        route_info(R, 1, 0.0, 0.0, info_out);
    }
    return ISDF_OK;
}
