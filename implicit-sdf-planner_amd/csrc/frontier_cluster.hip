// Frontier clusters: isdf_map_frontier_clusters, the connected components of the frontier - or of a caller's voxel set -
// with their sizes, boxes, centroid sums and representative voxels.  Stage 1 is map_known.hip's frontier stage (the set's words S, the
// per-dword bases of the exclusive scan, the ascending list); position i of the list is voxel vox[i], and frontier_cluster_host.hpp's
// fc_pos finds the position of any voxel of S from the bases: no hash table.  One lane per listed voxel everywhere below.
//   fc_init_kernel     parent[i] = i.
//   fc_union_kernel    lock-free union-find over positions.  For each lower neighbour of the connectivity that lies in the grid and in
//                      S: find both roots with path halving, atomicMin(&parent[larger root], smaller root), and where the value that
//                      comes back shows the larger one was a root no longer, go on from that value.  parent[x] <= x always and every
//                      write is an atomicMin, so every loop ends because a position strictly decreases; no lane waits for another lane
//                      or workgroup.  A finished component's root is its lowest position whatever the order of the atomics.  parent[] is
//                      read with relaxed agent-scope atomic loads: a plain load may be served from a stale line of this CU's L1 - a stale
//                      parent is still an ancestor, so the result would hold, but the retries would not be bounded by the chip's traffic.
//   fc_flatten_kernel  root[i] = find(i), and the flag "i is a root".
//   (dev_scan.hpp)     exclusive scan of the flags: the cluster number of every root, ascending with the label.
//   fc_number_kernel   each root opens its cluster's record: empty sums and box, its position as first_pos.
//   fc_stats_kernel    size, box and the three sums per cluster, integer atomics only.  The list is z-fastest, so neighbouring lanes
//                      mostly share a cluster: runs of equal cluster numbers are combined inside the wavefront (a segmented shuffle
//                      reduction) and the run's first lane issues the atomics.
//   fc_rep_kernel      after the sums are final: the key (d2 << 36) | voxel against the centroid cell, combined the same way, one 64-bit
//                      atomicMin per run.
//   fc_keep_kernel     keep[c] = size >= min_size (0 beyond the last cluster: the scan below runs over n entries, the host does not
//                      know the number of clusters yet); the largest cluster and the dropped voxels into the record.
//   (dev_scan.hpp)     exclusive scan of keep: the row number of every kept cluster.
//   fc_rows_kernel     the rows of the kept clusters as far as the caller's capacity goes; the counts into the record.
//   fc_labels_kernel   labels[i] = the row of i's cluster or -1.
// Nothing here writes to the ctx's map, its known grid, its products or its flags.
#include "map_query.hpp"
#include "frontier_cluster_host.hpp"
#include "dev_reduce.hpp"
#include "dev_scan.hpp"
#include <algorithm>
#include <climits>
#include <cstring>

namespace isdf {

constexpr int FC_BLOCK = 256;

// one cluster's record while it is being summed: one 64-byte line
struct FcAcc {
    unsigned long long size, sum[3];
    unsigned long long key;
    int lo[3], hi[3];
};
static_assert(sizeof(FcAcc) == 64, "a cluster's record is one 64-byte line");

// the call's record, zeroed before the kernels and read back after them
struct FcRecord {
    unsigned long long n_clusters, n_rows, n_voxels_dropped;
    unsigned long long largest;             // (size << 32) | (0xFFFFFFFF - cluster number): the maximum is the largest cluster, ties to the lowest number
    long long largest_label;
    unsigned long long pad[3];
};
static_assert(sizeof(FcRecord) == 64, "the clusters' record is one 64-byte line");

__device__ __forceinline__ int fc_load(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of i's tree, halving the path on the way: parent[i] <= i, so i strictly decreases until it is a root
__device__ __forceinline__ int fc_find(int *parent, int i) {
    int p = fc_load(parent + i);
    while (p != i) {
        const int g = fc_load(parent + p);
        if (g == p) return p;
        atomicMin(parent + i, g);           // (g < p <= what parent[i] holds or held: never raises it)
        i = g;
        p = fc_load(parent + i);
    }
    return i;
}

// unites the trees of positions a and b: the larger of the two values strictly decreases with every turn
__device__ __forceinline__ void fc_unite(int *parent, int a, int b) {
    a = fc_find(parent, a);
    b = fc_find(parent, b);
    while (a != b) {
        if (a < b) { const int t = a; a = b; b = t; }       // a: the larger root
        const int old = atomicMin(parent + a, b);
        if (old == a) return;               // a was a root and hangs below b now
        // a was a root no longer: its parent was old < a and is min(old, b) now; whichever of old and b lost that place is united here
        a = fc_find(parent, old);
        b = fc_find(parent, b);
    }
}

__global__ __launch_bounds__(FC_BLOCK) void fc_init_kernel(int n, int *__restrict__ parent) {
    const int i = blockIdx.x * FC_BLOCK + threadIdx.x;
    if (i < n) parent[i] = i;
}

__global__ __launch_bounds__(FC_BLOCK) void fc_union_kernel(FcGeom g, int max_nonzero, int n, const unsigned *__restrict__ set_bits, const int *__restrict__ base,
                                                            const long long *__restrict__ vox, int *parent) {
    const int i = blockIdx.x * FC_BLOCK + threadIdx.x;
    if (i >= n) return;
    int x, y, z;
    fc_xyz(vox[i], g.Y, g.Z, x, y, z);
    for (int k = 0; k < FC_LOWER; k++) {
        long long nv;
        if (!fc_lower_neighbour(max_nonzero, k, x, y, z, g, &nv) || !fc_in_set(set_bits, nv)) continue;
        fc_unite(parent, i, (int)fc_pos(set_bits, base, nv));
    }
}

__global__ __launch_bounds__(FC_BLOCK) void fc_flatten_kernel(int n, int *parent, int *__restrict__ root, int *__restrict__ flag) {
    const int i = blockIdx.x * FC_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int r = fc_find(parent, i);
    root[i] = r;
    flag[i] = r == i;
}

__global__ __launch_bounds__(FC_BLOCK) void fc_number_kernel(int n, const int *__restrict__ flag, const int *__restrict__ cnum, FcAcc *__restrict__ acc, int *__restrict__ first) {
    const int i = blockIdx.x * FC_BLOCK + threadIdx.x;
    if (i >= n || !flag[i]) return;
    FcAcc a;
    a.size = 0; a.sum[0] = a.sum[1] = a.sum[2] = 0;
    a.key = FC_KEY_NONE;
    a.lo[0] = a.lo[1] = a.lo[2] = 0x7FFFFFFF; a.hi[0] = a.hi[1] = a.hi[2] = -1;
    acc[cnum[i]] = a;
    first[cnum[i]] = i;
}

// Runs of equal cluster numbers among the 64 lanes (c < 0: a lane without a voxel, a run of its own).  *head: the lane is its run's
// first; returns the lane after its run's last.
__device__ __forceinline__ int fc_run_end(int c, int lane, bool *head) {
    const int before = __shfl_up(c, 1, 64);
    *head = lane == 0 || before != c || c < 0;
    const unsigned long long heads = __ballot(*head);
    const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
    return above ? lane + __ffsll((long long)above) : 64;
}

__global__ __launch_bounds__(FC_BLOCK) void fc_stats_kernel(FcGeom g, int n, const long long *__restrict__ vox, const int *__restrict__ root, const int *__restrict__ cnum,
                                                            FcAcc *acc) {
    const int i = blockIdx.x * FC_BLOCK + threadIdx.x, lane = threadIdx.x & 63;
    int c = -1, p[3] = {0, 0, 0};
    if (i < n) {
        c = cnum[root[i]];
        fc_xyz(vox[i], g.Y, g.Z, p[0], p[1], p[2]);
    }
    bool head;
    const int end = fc_run_end(c, lane, &head);
    int size = i < n ? 1 : 0, sum[3] = {p[0], p[1], p[2]}, lo[3] = {p[0], p[1], p[2]}, hi[3] = {p[0], p[1], p[2]};       // (64 lanes x 4095 fits an int)
    for (int off = 1; off < 64; off <<= 1) {
        const bool take = lane + off < end;     // the lane off above belongs to this run: it holds the run's values from there on
        const int s = __shfl_down(size, off, 64);
        if (take) size += s;
        for (int a = 0; a < 3; a++) {
            const int u = __shfl_down(sum[a], off, 64), l = __shfl_down(lo[a], off, 64), h = __shfl_down(hi[a], off, 64);
            if (take) { sum[a] += u; lo[a] = min(lo[a], l); hi[a] = max(hi[a], h); }
        }
    }
    if (c < 0 || !head) return;
    FcAcc *const A = acc + c;
    atomicAdd(&A->size, (unsigned long long)size);
    for (int a = 0; a < 3; a++) {
        atomicAdd(&A->sum[a], (unsigned long long)sum[a]);
        atomicMin(&A->lo[a], lo[a]);
        atomicMax(&A->hi[a], hi[a]);
    }
}

__global__ __launch_bounds__(FC_BLOCK) void fc_rep_kernel(FcGeom g, int n, const long long *__restrict__ vox, const int *__restrict__ root, const int *__restrict__ cnum,
                                                          FcAcc *acc) {
    const int i = blockIdx.x * FC_BLOCK + threadIdx.x, lane = threadIdx.x & 63;
    int c = -1;
    unsigned long long key = FC_KEY_NONE;
    if (i < n) {
        c = cnum[root[i]];
        const FcAcc *const A = acc + c;
        const unsigned long long size = A->size;
        int x, y, z;
        fc_xyz(vox[i], g.Y, g.Z, x, y, z);
        key = fc_key(fc_d2(x, y, z, (int)(A->sum[0] / size), (int)(A->sum[1] / size), (int)(A->sum[2] / size)), vox[i]);
    }
    bool head;
    const int end = fc_run_end(c, lane, &head);
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long k = __shfl_down(key, off, 64);
        if (lane + off < end && k < key) key = k;
    }
    if (c >= 0 && head) atomicMin(&acc[c].key, key);
}

// the number of clusters: the scan's last entry plus the last flag
__device__ __forceinline__ int fc_clusters(int n, const int *flag, const int *cnum) { return cnum[n - 1] + flag[n - 1]; }

__global__ __launch_bounds__(FC_BLOCK) void fc_keep_kernel(int n, const int *__restrict__ flag, const int *__restrict__ cnum, const FcAcc *__restrict__ acc,
                                                           unsigned long long min_size, int *__restrict__ keep, FcRecord *rec) {
    const int c = blockIdx.x * FC_BLOCK + threadIdx.x;
    unsigned long long largest = 0, dropped = 0;
    if (c < n) {
        const unsigned long long size = c < fc_clusters(n, flag, cnum) ? acc[c].size : 0;      // (a cluster has at least one voxel)
        keep[c] = size != 0 && size >= min_size;
        if (size) largest = (size << 32) | (0xFFFFFFFFull - (unsigned)c);       // (size < 2^31)
        if (size < min_size) dropped = size;
    }
    largest = wave_max(largest); dropped = wave_sum(dropped);       // every lane of the wavefront is here: one pair of atomics per wavefront
    if ((threadIdx.x & 63) == 0) {
        if (largest) atomicMax(&rec->largest, largest);
        if (dropped) atomicAdd(&rec->n_voxels_dropped, dropped);
    }
}

__global__ __launch_bounds__(FC_BLOCK) void fc_rows_kernel(int n, const int *__restrict__ flag, const int *__restrict__ cnum, const FcAcc *__restrict__ acc,
                                                           const int *__restrict__ first, const long long *__restrict__ vox, const int *__restrict__ keep,
                                                           const int *__restrict__ row_of, long long *__restrict__ rows, long long row_capacity, FcRecord *rec) {
    const int c = blockIdx.x * FC_BLOCK + threadIdx.x;
    if (c >= n) return;
    const int nc = fc_clusters(n, flag, cnum);
    if (c == 0) {
        rec->n_clusters = (unsigned long long)nc;
        rec->n_rows = (unsigned long long)(row_of[nc - 1] + keep[nc - 1]);
        rec->largest_label = vox[first[0xFFFFFFFFu - (unsigned)(rec->largest & 0xFFFFFFFFull)]];       // (fc_keep_kernel has finished: nc >= 1, so it is set)
    }
    if (c >= nc || !keep[c] || !rows || row_of[c] >= row_capacity) return;
    const FcAcc A = acc[c];
    long long *const r = rows + (long long)FC_ROW * row_of[c];
    r[0] = vox[first[c]]; r[1] = (long long)A.size;
    for (int a = 0; a < 3; a++) { r[2 + a] = A.lo[a]; r[5 + a] = A.hi[a]; r[8 + a] = (long long)A.sum[a]; }
    r[11] = fc_key_voxel(A.key); r[12] = fc_key_d2(A.key); r[13] = first[c];
    r[14] = r[15] = 0;
}

__global__ __launch_bounds__(FC_BLOCK) void fc_labels_kernel(int n, const int *__restrict__ root, const int *__restrict__ cnum, const int *__restrict__ keep,
                                                             const int *__restrict__ row_of, int *__restrict__ labels) {
    const int i = blockIdx.x * FC_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int c = cnum[root[i]];
    labels[i] = keep[c] ? row_of[c] : -1;
}

}  // namespace isdf

// the union-find and its numbering, the clusters' records, the rows as far as the caller's capacity goes, the call's record and the
// pinned copies the outputs are handed over through (an overflow must leave the caller's arrays untouched)
struct FrontierClusterState {
    isdf::DevBuf<int> d_parent, d_root, d_flag, d_cnum, d_first, d_keep, d_row_of, d_labels;
    isdf::DevBuf<isdf::FcAcc> d_acc;
    isdf::DevBuf<long long> d_rows;
    isdf::DevBuf<unsigned char> d_scan_tmp;
    isdf::RecPair<isdf::FcRecord> rec;
    isdf::PinBuf<int64_t> h_vox, h_rows;
    isdf::PinBuf<int32_t> h_labels;
    isdf::DevEvents<4> ev;
    int ready(isdf_ctx *c) { ISDF_TRY(ev.ready(c)); return rec.ready(c); }
};

using namespace isdf;

extern "C" void isdf_frontier_cluster_params_default(isdf_frontier_cluster_params *p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->connectivity = 26;
    p->min_size = 1;
}

extern "C" void isdf_frontier_cluster_sizes(int sizes_out[2]) {
    if (!sizes_out) return;
    sizes_out[0] = (int)sizeof(isdf_frontier_cluster_params); sizes_out[1] = (int)sizeof(isdf_frontier_cluster_info);
}

namespace {

// what the device and the host forms check alike (c may be null: the host form)
int cluster_setup(isdf_ctx *c, const isdf_frontier_cluster_params *params, long long vox_capacity, long long row_capacity, isdf_frontier_cluster_params &P) {
    P = map_query::resolve(params, isdf_frontier_cluster_params_default);
    if (!fc_max_nonzero(P.connectivity)) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "frontier clusters: connectivity must be 6, 18 or 26");
    if (P.min_size < 1) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "frontier clusters: min_size must be at least 1");
    if (vox_capacity < 0 || row_capacity < 0) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "frontier clusters: negative capacity");
    return ISDF_OK;
}

}  // namespace

extern "C" int isdf_map_frontier_clusters(isdf_ctx *c, const uint32_t *bits_in, const isdf_frontier_cluster_params *params, int64_t *vox_out, int32_t *labels_out,
                                          long long vox_capacity, int64_t *rows_out, long long row_capacity, isdf_frontier_cluster_info *info_out) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    isdf_frontier_cluster_params P;
    ISDF_TRY(cluster_setup(c, params, vox_capacity, row_capacity, P));
    ISDF_TRY(map_query::single_device(c, "frontier clusters are not offered on a multi-device ctx"));
    const DevGrid &G = c->grid;
    const int32_t dims[3] = {G.X, G.Y, G.Z};
    const FcGeom g = fc_geom(dims);
    if (bits_in && c->known.have && fc_tail_dirty(bits_in, g)) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "frontier clusters: a bit of bits_in beyond the last voxel is set");
    FrontierClusterState *S;
    ISDF_TRY(map_query::state_of(c, c->fcl, &S));
    const hipStream_t st = c->stream;
    // stage 1 and the first hand-over: |S|
    MkRecord R;
    bool counted = false;
    ISDF_TRY(map_frontier_stage(c, "frontier clusters", bits_in, nullptr, true, LLONG_MAX, S->ev.get(), &R, &counted));
    const long long n = (long long)R.n;
    isdf_frontier_cluster_info info{};
    info.n_voxels = n; info.largest_label = -1;
    const bool vox_short = (vox_out || labels_out) && vox_capacity < n;
    if (n == 0) {
        if (info_out) *info_out = info;
        return ISDF_OK;
    }
    const isdf_ctx::Known &K = c->known;
    const size_t un = (size_t)n;
    const long long rows_room = rows_out ? std::min(row_capacity, n) : 0;          // rows the device writes and hands over
    ISDF_TRY(S->d_parent.reserve(c, un)); ISDF_TRY(S->d_root.reserve(c, un)); ISDF_TRY(S->d_flag.reserve(c, un)); ISDF_TRY(S->d_cnum.reserve(c, un));
    ISDF_TRY(S->d_first.reserve(c, un)); ISDF_TRY(S->d_keep.reserve(c, un)); ISDF_TRY(S->d_row_of.reserve(c, un)); ISDF_TRY(S->d_labels.reserve(c, un));
    ISDF_TRY(S->d_acc.reserve(c, un));
    ISDF_TRY(S->d_rows.reserve(c, (size_t)rows_room * FC_ROW));
    size_t bytes;           // of both scans below: n ints into n ints
    ISDF_TRY(exclusive_sum_reserve(c, S->d_scan_tmp, S->d_flag.get(), S->d_cnum.get(), n, st, &bytes));
    if (vox_out && !vox_short) ISDF_TRY(S->h_vox.reserve(c, un));
    if (labels_out && !vox_short) ISDF_TRY(S->h_labels.reserve(c, un));
    if (rows_room) ISDF_TRY(S->h_rows.reserve(c, (size_t)rows_room * FC_ROW));
    const unsigned nb = blocks(n, FC_BLOCK);
    const int ni = (int)n;
    // stage 2: the components (ev[1], recorded after the emit pass, is its start)
    hipLaunchKernelGGL(fc_init_kernel, dim3(nb), dim3(FC_BLOCK), 0, st, ni, S->d_parent.get());
    hipLaunchKernelGGL(fc_union_kernel, dim3(nb), dim3(FC_BLOCK), 0, st, g, fc_max_nonzero(P.connectivity), ni, (const unsigned *)K.d_front.get(), (const int *)K.d_base.get(),
                       (const long long *)K.d_list.get(), S->d_parent.get());
    hipLaunchKernelGGL(fc_flatten_kernel, dim3(nb), dim3(FC_BLOCK), 0, st, ni, S->d_parent.get(), S->d_root.get(), S->d_flag.get());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(S->ev[2], st));
    // stage 3: numbering, statistics, representatives, rows
    HIPCHK(c, S->rec.zero(st));
    ISDF_TRY(exclusive_sum_run(c, S->d_scan_tmp, bytes, S->d_flag.get(), S->d_cnum.get(), n, st));
    hipLaunchKernelGGL(fc_number_kernel, dim3(nb), dim3(FC_BLOCK), 0, st, ni, (const int *)S->d_flag.get(), (const int *)S->d_cnum.get(), S->d_acc.get(), S->d_first.get());
    hipLaunchKernelGGL(fc_stats_kernel, dim3(nb), dim3(FC_BLOCK), 0, st, g, ni, (const long long *)K.d_list.get(), (const int *)S->d_root.get(), (const int *)S->d_cnum.get(),
                       S->d_acc.get());
    hipLaunchKernelGGL(fc_rep_kernel, dim3(nb), dim3(FC_BLOCK), 0, st, g, ni, (const long long *)K.d_list.get(), (const int *)S->d_root.get(), (const int *)S->d_cnum.get(),
                       S->d_acc.get());
    hipLaunchKernelGGL(fc_keep_kernel, dim3(nb), dim3(FC_BLOCK), 0, st, ni, (const int *)S->d_flag.get(), (const int *)S->d_cnum.get(), (const FcAcc *)S->d_acc.get(),
                       (unsigned long long)P.min_size, S->d_keep.get(), S->rec.dev());
    HIPCHK(c, hipGetLastError());
    ISDF_TRY(exclusive_sum_run(c, S->d_scan_tmp, bytes, S->d_keep.get(), S->d_row_of.get(), n, st));
    hipLaunchKernelGGL(fc_rows_kernel, dim3(nb), dim3(FC_BLOCK), 0, st, ni, (const int *)S->d_flag.get(), (const int *)S->d_cnum.get(), (const FcAcc *)S->d_acc.get(),
                       (const int *)S->d_first.get(), (const long long *)K.d_list.get(), (const int *)S->d_keep.get(), (const int *)S->d_row_of.get(),
                       rows_room ? S->d_rows.get() : nullptr, rows_room, S->rec.dev());
    hipLaunchKernelGGL(fc_labels_kernel, dim3(nb), dim3(FC_BLOCK), 0, st, ni, (const int *)S->d_root.get(), (const int *)S->d_cnum.get(), (const int *)S->d_keep.get(),
                       (const int *)S->d_row_of.get(), S->d_labels.get());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(S->ev[3], st));
    // the second hand-over: the record and, through the pinned copies, what the caller's capacities can hold
    HIPCHK(c, S->rec.fetch(st));
    if (vox_out && !vox_short) HIPCHK(c, hipMemcpyAsync(S->h_vox.get(), K.d_list, un * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    if (labels_out && !vox_short) HIPCHK(c, hipMemcpyAsync(S->h_labels.get(), S->d_labels, un * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (rows_room) HIPCHK(c, hipMemcpyAsync(S->h_rows.get(), S->d_rows, (size_t)rows_room * FC_ROW * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    const FcRecord F = S->rec.host();
    info.n_clusters = (int64_t)F.n_clusters; info.n_rows = (int64_t)F.n_rows; info.n_voxels_dropped = (int64_t)F.n_voxels_dropped;
    info.largest_size = (int64_t)(F.largest >> 32); info.largest_label = F.largest_label;
    info.frontier_ms = K.ev.ms(0, 1) + S->ev.ms(0, 1); info.label_ms = S->ev.ms(1, 2); info.stats_ms = S->ev.ms(2, 3);
    if (info_out) *info_out = info;
    if (vox_short || (rows_out && row_capacity < info.n_rows)) return isdf_fail(c, ISDF_ERR_OVERFLOW, "frontier clusters: an output's capacity is smaller than what it must hold");
    if (vox_out) std::memcpy(vox_out, S->h_vox.get(), un * sizeof(int64_t));
    if (labels_out) std::memcpy(labels_out, S->h_labels.get(), un * sizeof(int32_t));
    if (rows_out && info.n_rows) std::memcpy(rows_out, S->h_rows.get(), (size_t)info.n_rows * FC_ROW * sizeof(int64_t));
    return ISDF_OK;
}

extern "C" int isdf_known_clusters_host(const uint32_t *set_bits, const int32_t dims[3], const isdf_frontier_cluster_params *params, int64_t *vox_out, int32_t *labels_out,
                                        long long vox_capacity, int64_t *rows_out, long long row_capacity, isdf_frontier_cluster_info *info_out) {
    if (!set_bits || mk_dims_bad(dims)) return isdf_fail(nullptr, ISDF_ERR_INVALID_ARG, "frontier clusters (host form): bad arguments");
    isdf_frontier_cluster_params P;
    ISDF_TRY(cluster_setup(nullptr, params, vox_capacity, row_capacity, P));
    const FcGeom g = fc_geom(dims);
    if (fc_tail_dirty(set_bits, g)) return isdf_fail(nullptr, ISDF_ERR_INVALID_ARG, "frontier clusters (host form): a bit of the set beyond the last voxel is set");
    FcCounts N;
    const int over = fc_clusters_host(set_bits, g, fc_max_nonzero(P.connectivity), P.min_size, vox_out, labels_out, vox_capacity, rows_out, row_capacity, N);
    if (info_out) {
        isdf_frontier_cluster_info info{};
        info.n_voxels = N.n_voxels; info.n_clusters = N.n_clusters; info.n_rows = N.n_rows; info.n_voxels_dropped = N.n_voxels_dropped;
        info.largest_size = N.largest_size; info.largest_label = N.largest_label;
        *info_out = info;
    }
    if (N.n_voxels > (long long)INT_MAX) return isdf_fail(nullptr, ISDF_ERR_OVERFLOW, "frontier clusters (host form): more than 2^31 voxels");
    return over ? isdf_fail(nullptr, ISDF_ERR_OVERFLOW, "frontier clusters (host form): an output's capacity is smaller than what it must hold") : ISDF_OK;
}
