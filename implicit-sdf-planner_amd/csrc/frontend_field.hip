// Front end: the cost-to-go field of one goal over the configuration space, and paths read off it - on the device.
// Graph = that of AstarPathSearcher::AstarGetSucc (front_end_Astar.hpp:197-236): voxel v is FREE when any attitude bit of its word of
// the configuration-space table (fe.d_cspace, left by fe_cspace_kernel) is set - occupied voxels hold 0 -, a step goes to any of the
// 26 neighbours that is free and inside the map, its cost is edge[i*i + j*j + k*k] = sqrt(i*i + j*j + k*k) in cells (:230).
// "Any bit set" equals the reference's checkKernelValue (sw_manager.hpp:911-942) when the parent's attitude lies on the attitude grid
// and the grid has at most 801 attitudes: visit_kernels_by_distance (:850-909) pops at most maxdeepth + 1 = 801 attitudes, and only
// then does its breadth-first order reach every attitude.
//   d[goal] = 0;  d[v] = min over free neighbours u of fl(d[u] + w(u, v)) for free v, the least fixed point from +inf (fp64, one plain
//   addition per candidate); +inf where v is not free or cannot reach the goal.
// Addition is monotone and every intermediate value is the length of a real path summed from the goal outward, so every relaxation
// order that reaches a fixed point reaches the same BYTES - those of frontend_field_host.hpp's Dijkstra.
//   ff_init_kernel     one wavefront per 64 consecutive z: the free bits of the column (one ballot -> one 64-bit word), d = +inf, d[goal] = 0,
//                      the goal's brick as the first active list, the count of free voxels;
//   ff_init_known_kernel  the same for isdf_frontend_field_build_known: the ballot ANDed with the eroded known grid's bits of
//                      the column, so that the free words carry "free and seen" and nothing after it knows of the gate;
//   ff_relax_kernel    one workgroup per ACTIVE brick of 8 x 8 x 64 voxels (z fastest, 64 consecutive z per wavefront as in
//                      fe_cspace_kernel): the brick and its one-voxel halo of d in LDS (10 x 10 x 66 doubles, 52.8 KB: three workgroups per
//                      CU; a wavefront's 64 lanes read 64 consecutive doubles, which ds_read_b64 serves without bank conflicts), the
//                      brick's free bits in a register; Jacobi relaxation inside LDS until nothing in the brick changes; the lowered
//                      voxels are stored and every neighbouring brick whose halo was lowered is flagged;
//   ff_compact_kernel  one workgroup: flags -> the next round's list in brick order (a scan, no atomics) and its length, also written to the
//                      host's pinned word.
// A round is ff_relax_kernel over the list + ff_compact_kernel; the host reads one word, the next list's length, and stops at 0.  No
// workgroup waits for another inside a kernel.  A brick is stored by its own workgroup only (a brick is in a list once); a neighbour
// that reads a halo voxel while it is being lowered sees the old or the new value (8-byte relaxed atomic accesses), both lengths of real
// paths, and is flagged by the writer, so it runs again next round with the new value in sight: the fixed point does not depend on which
// it saw.  Only counts of events (free voxels, bricks seen) go through integer atomics; nothing is decided by their order.
//   ff_paths_kernel    one lane per start: the steepest walk down the field with the A*'s attitude bookkeeping (below).
// The field CHANGED IN PLACE after the map changed in ONE direction (FfChange): voxels only closed (a map update; DESIGN 4.6.2,
// isdf_frontend_field_set_repair) or only opened (a map clear; DESIGN 4.6.3, isdf_frontend_field_set_reopen).  Both directions are
// mark, seed, relax: isdf_field_change_begin / _end, one FfRecord.
//   ff_mark_kernel<dir>     one wavefront per 64 consecutive z of a column of the changed box: the new free ballot against the kept
//                           word, the new word written, the changed bits counted, a bit that moved against the direction raises
//                           the record's premise word (the host drops the field).  Closing: a closed lane folds its finite old d
//                           into tau (an integer atomicMin on the bit pattern: non-negative doubles order like their bits) and
//                           takes +inf.  Opening: the opened bits are kept in a word per wavefront, the brick is flagged, the lane
//                           on the goal voxel, when it opened, stores d = 0;
//   ff_repair_reset_kernel  closing only, one workgroup per brick: +inf wherever tau <= d < +inf (tau read from device memory), the
//                           brick flagged when it reset a voxel;
//   ff_mark_known_kernel<dir>  the mark for a gated field that follows the change (isdf_frontend_field_set_known_follow):
//                           the new ballot ANDed with the freshly eroded known grid's bits of the column, as ff_init_known_kernel reads them;
// then ff_compact_kernel and the rounds of the build from the flagged bricks, the count of reached voxels, and
//   ff_reopen_count_kernel  opening only, over the same box: the opened voxels that hold a finite d.
// Closing keeps every d < tau: the chain of minimising neighbours from such a voxel to the goal passes only voxels with d < tau, none
// of them closed, and the new graph is a subgraph of the old.  From the kept values every intermediate value is again a real path's
// length, so the fixed point has the bytes of a build on the new map.
// Opening resets nothing: the old graph is a subgraph of the new, so every old value is a path's length that still exists - an upper
// bound of the new least fixed point d* -, relaxation keeps it one, and a fixed point >= d* with d[goal] = 0 is d* (in Dijkstra order
// of d*, v's predecessor u holds d*[u], so d[v] <= fl(d*[u] + w) = d*[v]).  A brick without an opened voxel or a lowered halo voxel
// satisfies its equations as before.
// The field CARRIED through a shift of the map window, which moves bits both ways (isdf_frontend_field_set_shift):
// ff_shift_kernel translates d and the free words into second buffers (fm1 = old & new: a subgraph of both maps), ff_left_kernel
// takes the leaving voxels' tau; then the closing direction's reset and rounds on fm1, then the opening direction as it is.
// Compiled with -ffp-contract=off like frontend.hip (cell indices and cube centres round like the A*'s).
#include "isdf_ctx.hpp"
#include "frontend_dev.hpp"
#include "field_cell.hpp"
#include "frontend_field_host.hpp"
#include "map_known_host.hpp"
#include "map_query.hpp"
#include "dev_reduce.hpp"
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

namespace isdf {

constexpr int FF_BX = 8, FF_BY = 8, FF_BZ = 64;
constexpr int FF_TX = FF_BX + 2, FF_TY = FF_BY + 2, FF_TZ = FF_BZ + 2;
constexpr int FF_PER_LANE = FF_BX * FF_BY / 4;             // columns of the brick per wavefront (4 wavefronts)
constexpr int FF_CNT_ACTIVE = 0, FF_CNT_FREE = 1, FF_CNT_REACHED = 2, FF_CNT_BRICKS = 3, FF_CNT_LEFT = 4, FF_CNT_WORDS = 5;

struct FfDims {
    int X, Y, Z, nbx, nby, nbz, zblocks, nw;
    double w1, w2, w3;                                     // sqrt(1), sqrt(2), sqrt(3) as the host's std::sqrt gives them
    long long goal;                                        // voxel index of the goal cell, -1: outside the map
};

__device__ __forceinline__ double ff_load(const double *p) {
    return __longlong_as_double((long long)__hip_atomic_load((const unsigned long long *)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ void ff_store(double *p, double v) {
    __hip_atomic_store((unsigned long long *)p, (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the free bits of a wavefront whose lanes hold consecutive z of one column: lane's voxel v is free when any attitude bit of its word
// is set; a lane past the end of the column (valid = false) gives 0
__device__ __forceinline__ unsigned long long ff_free_ballot(const FfDims &D, const unsigned *__restrict__ cspace, size_t v, bool valid) {
    bool fr = false;
    if (valid) {
        const unsigned *m = cspace + v * D.nw;
        unsigned any = 0;
        for (int w = 0; w < D.nw; w++) any |= m[w];
        fr = any != 0u;
    }
    return __ballot(fr);
}

__global__ __launch_bounds__(256) void ff_init_kernel(FfDims D, const unsigned *__restrict__ cspace, unsigned long long *__restrict__ fm,
                                                       double *__restrict__ d, int *__restrict__ list, unsigned long long *__restrict__ cnt) {
    const long long wv = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const long long n_wv = (long long)D.X * D.Y * D.zblocks;
    if (wv >= n_wv) return;
    const int lane = threadIdx.x & 63;
    const int zb = (int)(wv % D.zblocks);
    const long long xy = wv / D.zblocks;
    const int z = (zb << 6) + lane;
    const long long v = xy * D.Z + z;
    const unsigned long long bits = ff_free_ballot(D, cspace, (size_t)v, z < D.Z);
    if (z < D.Z) {
        const bool is_goal = ((bits >> lane) & 1ull) && v == D.goal;
        d[v] = is_goal ? 0.0 : __longlong_as_double(0x7FF0000000000000ll);
        if (is_goal) {
            const int x = (int)(xy / D.Y), y = (int)(xy % D.Y);
            list[0] = ((x / FF_BX) * D.nby + y / FF_BY) * D.nbz + zb;
            cnt[FF_CNT_ACTIVE] = 1ull;
        }
    }
    if (lane == 0) {
        fm[wv] = bits;
        if (bits) atomicAdd(cnt + FF_CNT_FREE, (unsigned long long)__popcll(bits));
    }
}

// ff_init_kernel for the field gated by the eroded known grid (isdf_frontend_field_build_known), a second kernel so that the
// plain build's keeps its code to the instruction: the column's free ballot is ANDed with the 64 bits of `gate` that start at the
// wavefront's first voxel - the grid is one stream of bits in voxel order (map_known_host.hpp), so they are two funnel-shifted dwords,
// the same in every lane; bits past the column's end belong to the next column and meet a ballot that is 0 there.  The field's own fm
// words then carry free & E, and nothing downstream knows of the gate.
__global__ __launch_bounds__(256) void ff_init_known_kernel(FfDims D, const unsigned *__restrict__ cspace, unsigned long long *__restrict__ fm,
                                                             double *__restrict__ d, int *__restrict__ list, unsigned long long *__restrict__ cnt,
                                                             const unsigned *__restrict__ gate, long long gate_words) {
    const long long wv = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const long long n_wv = (long long)D.X * D.Y * D.zblocks;
    if (wv >= n_wv) return;
    const int lane = threadIdx.x & 63;
    const int zb = (int)(wv % D.zblocks);
    const long long xy = wv / D.zblocks;
    const int z = (zb << 6) + lane;
    const long long a0 = xy * D.Z + (zb << 6), v = a0 + lane;
    const unsigned long long seen = (unsigned long long)mk_bits_at(gate, gate_words, a0) | ((unsigned long long)mk_bits_at(gate, gate_words, a0 + 32) << 32);
    const unsigned long long bits = ff_free_ballot(D, cspace, (size_t)v, z < D.Z) & seen;
    if (z < D.Z) {
        const bool is_goal = ((bits >> lane) & 1ull) && v == D.goal;
        d[v] = is_goal ? 0.0 : __longlong_as_double(0x7FF0000000000000ll);
        if (is_goal) {
            const int x = (int)(xy / D.Y), y = (int)(xy % D.Y);
            list[0] = ((x / FF_BX) * D.nby + y / FF_BY) * D.nbz + zb;
            cnt[FF_CNT_ACTIVE] = 1ull;
        }
    }
    if (lane == 0) {
        fm[wv] = bits;
        if (bits) atomicAdd(cnt + FF_CNT_FREE, (unsigned long long)__popcll(bits));
    }
}

__device__ __forceinline__ int ff_tile(int tx, int ty, int tz) { return (tx * FF_TY + ty) * FF_TZ + tz; }

__global__ __launch_bounds__(256) void ff_relax_kernel(FfDims D, const int *__restrict__ list, double *d, const unsigned long long *__restrict__ fm,
                                                        unsigned *flags, unsigned *seen, unsigned long long *cnt) {
    __shared__ double tile[FF_TX * FF_TY * FF_TZ];
    __shared__ unsigned s_mark;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int b = list[blockIdx.x];
    const int bz = b % D.nbz, by = (b / D.nbz) % D.nby, bx = b / (D.nbz * D.nby);
    const int x0 = bx * FF_BX, y0 = by * FF_BY, z0 = bz * FF_BZ;
    const double inf = __longlong_as_double(0x7FF0000000000000ll);
    if (tid == 0) {
        s_mark = 0u;
        if (!seen[b]) { seen[b] = 1u; atomicAdd(cnt + FF_CNT_BRICKS, 1ull); }           // (a brick is in a list once: its own workgroup only)
    }
    for (int c = wave; c < FF_TX * FF_TY; c += 4) {
        const int tx = c / FF_TY, ty = c - tx * FF_TY;
        const int gx = x0 + tx - 1, gy = y0 + ty - 1;
        const bool in_xy = gx >= 0 && gx < D.X && gy >= 0 && gy < D.Y;
        for (int tz = lane; tz < FF_TZ; tz += 64) {
            const int gz = z0 + tz - 1;
            double v = inf;
            if (in_xy && gz >= 0 && gz < D.Z) v = ff_load(d + ((size_t)gx * D.Y + gy) * D.Z + gz);
            tile[ff_tile(tx, ty, tz)] = v;
        }
    }
    // this lane's voxels: column c = wave + 4 i of the brick (cx = i / 2, cy = 4 (i & 1) + wave), z = z0 + lane
    unsigned fbits = 0u;
#pragma unroll
    for (int i = 0; i < FF_PER_LANE; i++) {
        const int gx = x0 + (i >> 1), gy = y0 + 4 * (i & 1) + wave;
        if (gx < D.X && gy < D.Y && ((fm[((size_t)gx * D.Y + gy) * D.zblocks + bz] >> lane) & 1ull)) fbits |= 1u << i;
    }
    __syncthreads();
    double own[FF_PER_LANE];
#pragma unroll
    for (int i = 0; i < FF_PER_LANE; i++) own[i] = tile[ff_tile((i >> 1) + 1, 4 * (i & 1) + wave + 1, lane + 1)];
    unsigned low = 0u;
    for (;;) {
        double nv[FF_PER_LANE];
        unsigned ch = 0u;
#pragma unroll
        for (int i = 0; i < FF_PER_LANE; i++) {
            nv[i] = own[i];
            if ((fbits >> i) & 1u) {
                const double *p = tile + ff_tile(i >> 1, 4 * (i & 1) + wave, lane);      // the (-1, -1, -1) neighbour
                double m = own[i];
#pragma unroll
                for (int a = 0; a < 3; a++)
#pragma unroll
                    for (int e = 0; e < 3; e++)
#pragma unroll
                        for (int g = 0; g < 3; g++) {
                            const int q = (a != 1) + (e != 1) + (g != 1);
                            if (q == 0) continue;
                            const double cand = p[(a * FF_TY + e) * FF_TZ + g] + (q == 1 ? D.w1 : q == 2 ? D.w2 : D.w3);
                            m = cand < m ? cand : m;
                        }
                nv[i] = m;
                if (m < own[i]) ch |= 1u << i;
            }
        }
        __syncthreads();                                   // every read of this sweep is done
#pragma unroll
        for (int i = 0; i < FF_PER_LANE; i++)
            if ((ch >> i) & 1u) { own[i] = nv[i]; tile[ff_tile((i >> 1) + 1, 4 * (i & 1) + wave + 1, lane + 1)] = nv[i]; }
        low |= ch;
        if (!__syncthreads_or((int)ch)) break;
    }
    // store what fell; flag the neighbouring bricks that have a lowered voxel in their halo
    unsigned mk = 0u;
#pragma unroll
    for (int i = 0; i < FF_PER_LANE; i++) {
        if (!((low >> i) & 1u)) continue;
        const int cx = i >> 1, cy = 4 * (i & 1) + wave;
        ff_store(d + ((size_t)(x0 + cx) * D.Y + (y0 + cy)) * D.Z + (z0 + lane), own[i]);
        const int xs = cx == 0 ? -1 : cx == FF_BX - 1 ? 1 : 0, ys = cy == 0 ? -1 : cy == FF_BY - 1 ? 1 : 0, zs = lane == 0 ? -1 : lane == FF_BZ - 1 ? 1 : 0;
        for (int a = 0; a < 2; a++)
            for (int e = 0; e < 2; e++)
                for (int g = 0; g < 2; g++) {
                    const int ax = a ? xs : 0, ay = e ? ys : 0, az = g ? zs : 0;
                    if (ax | ay | az) mk |= 1u << ((ax + 1) * 9 + (ay + 1) * 3 + (az + 1));
                }
    }
    if (mk) atomicOr(&s_mark, mk);
    __syncthreads();
    if (tid < 27 && ((s_mark >> tid) & 1u)) {
        const int nx = bx + tid / 9 - 1, ny = by + (tid / 3) % 3 - 1, nz = bz + tid % 3 - 1;
        if (nx >= 0 && nx < D.nbx && ny >= 0 && ny < D.nby && nz >= 0 && nz < D.nbz) flags[(nx * D.nby + ny) * D.nbz + nz] = 1u;
    }
}

__global__ __launch_bounds__(1024) void ff_compact_kernel(unsigned *flags, int *__restrict__ list, unsigned long long *cnt, unsigned long long *host_cnt, int n_bricks) {
    __shared__ int s_sum[1024];
    const int tid = threadIdx.x;
    const int chunk = (n_bricks + 1023) / 1024;
    const int b0 = min(tid * chunk, n_bricks), b1 = min(b0 + chunk, n_bricks);
    int k = 0;
    for (int b = b0; b < b1; b++) k += flags[b] != 0u;
    s_sum[tid] = k;
    __syncthreads();
    for (int s = 1; s < 1024; s <<= 1) {
        const int add = tid >= s ? s_sum[tid - s] : 0;
        __syncthreads();
        s_sum[tid] += add;
        __syncthreads();
    }
    int off = s_sum[tid] - k;
    for (int b = b0; b < b1; b++)
        if (flags[b]) { list[off++] = b; flags[b] = 0u; }
    if (tid == 1023) { cnt[FF_CNT_ACTIVE] = (unsigned long long)s_sum[1023]; host_cnt[FF_CNT_ACTIVE] = (unsigned long long)s_sum[1023]; }     // (host_cnt: pinned, device-mapped)
}

__global__ __launch_bounds__(256) void ff_count_kernel(const double *__restrict__ d, long long n, unsigned long long *cnt) {
    unsigned long long k = 0;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long long)gridDim.x * blockDim.x) k += d[t] < __longlong_as_double(0x7FF0000000000000ll);
    k = wave_sum(k);
    if ((threadIdx.x & 63) == 0 && k) atomicAdd(cnt + FF_CNT_REACHED, k);
}

constexpr unsigned long long FF_INF_BITS = 0x7FF0000000000000ull;

// The changed box as its kernels take it, whole 64-voxel blocks in z: columns x in [x0, x0 + ex), y in [y0, y0 + ey), blocks zb in
// [zb0, zb0 + ezb); one wavefront per block of a column.  ff_box_column: this wavefront's index among the box's and its block (false: past
// the end).
struct FfBox { int x0, y0, zb0, ex, ey, ezb; };
struct FfColumn { long long wv; int x, y, zb; };
__device__ __forceinline__ bool ff_box_column(const FfBox &B, FfColumn &C) {
    C.wv = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (C.wv >= (long long)B.ex * B.ey * B.ezb) return false;
    C.zb = B.zb0 + (int)(C.wv % B.ezb);
    const long long xy = C.wv / B.ezb;
    C.y = B.y0 + (int)(xy % B.ey); C.x = B.x0 + (int)(xy / B.ey);
    return true;
}

// The mark of either direction.  flags, open: opening only (open[wv]: the opened bits of this wavefront's word, for
// ff_reopen_count_kernel; written by every wavefront of the box: nothing stale is read).
template <FfChange DIR>
__global__ __launch_bounds__(256) void ff_mark_kernel(FfDims D, FfBox B, const unsigned *__restrict__ cspace, unsigned long long *__restrict__ fm, double *__restrict__ d,
                                                       unsigned *__restrict__ flags, unsigned long long *__restrict__ open, FfRecord *__restrict__ rec) {
    constexpr bool closing = DIR == FfChange::Closing;
    FfColumn C;
    if (!ff_box_column(B, C)) return;
    const int lane = threadIdx.x & 63;
    const int z = (C.zb << 6) + lane;
    const size_t col = (size_t)C.x * D.Y + C.y;
    const size_t v = col * D.Z + z;
    const unsigned long long now = ff_free_ballot(D, cspace, v, z < D.Z);
    const unsigned long long old = fm[col * D.zblocks + C.zb];
    const unsigned long long changed = closing ? old & ~now : now & ~old, against = closing ? now & ~old : old & ~now;
    const bool mine = (changed >> lane) & 1ull;            // (a set bit of the kept or of the new word: z < D.Z)
    unsigned long long hit = 0ull;
    if (closing) {
        bool reached = false;
        if (mine) {
            const unsigned long long bits = (unsigned long long)__double_as_longlong(d[v]);
            reached = bits < FF_INF_BITS;                  // d is never negative and never NaN
            if (reached) { atomicMin(&rec->tau_bits, bits); d[v] = __longlong_as_double((long long)FF_INF_BITS); }
        }
        hit = __ballot(reached);
    } else {
        if (mine && (long long)v == D.goal) {
            d[v] = 0.0;                                    // the goal cell had not been free: the field was all +inf
            rec->goal_opened = 1ull;
        }
    }
    if (lane != 0) return;
    if (!closing) open[C.wv] = changed;
    if (now == old) return;
    fm[col * D.zblocks + C.zb] = now;
    if (changed) {
        atomicAdd(&rec->changed, (unsigned long long)__popcll(changed));
        if (!closing) flags[((C.x / FF_BX) * D.nby + C.y / FF_BY) * D.nbz + C.zb] = 1u;
    }
    if (hit) atomicAdd(&rec->changed_reached, (unsigned long long)__popcll(hit));
    if (against) rec->premise_violated = 1ull;            // outside the premise: the host drops the field
}

// ff_mark_kernel for a gated field that follows the change (isdf_frontend_field_set_known_follow), a second kernel for
// ff_init_known_kernel's reason: the new word is the column's free ballot ANDed with the 64 bits of the freshly eroded grid that start
// at the wavefront's first voxel, read as that kernel reads them.  The kept word carries free & E_old, so the comparison is between the
// gated sets, and a bit of either the table or E that moved against the direction raises the premise word.
template <FfChange DIR>
__global__ __launch_bounds__(256) void ff_mark_known_kernel(FfDims D, FfBox B, const unsigned *__restrict__ cspace, unsigned long long *__restrict__ fm, double *__restrict__ d,
                                                             unsigned *__restrict__ flags, unsigned long long *__restrict__ open, FfRecord *__restrict__ rec,
                                                             const unsigned *__restrict__ gate, long long gate_words) {
    constexpr bool closing = DIR == FfChange::Closing;
    FfColumn C;
    if (!ff_box_column(B, C)) return;
    const int lane = threadIdx.x & 63;
    const int z = (C.zb << 6) + lane;
    const size_t col = (size_t)C.x * D.Y + C.y;
    const long long a0 = (long long)col * D.Z + (C.zb << 6);
    const size_t v = (size_t)a0 + lane;
    const unsigned long long seen = (unsigned long long)mk_bits_at(gate, gate_words, a0) | ((unsigned long long)mk_bits_at(gate, gate_words, a0 + 32) << 32);
    const unsigned long long now = ff_free_ballot(D, cspace, v, z < D.Z) & seen;
    const unsigned long long old = fm[col * D.zblocks + C.zb];
    const unsigned long long changed = closing ? old & ~now : now & ~old, against = closing ? now & ~old : old & ~now;
    const bool mine = (changed >> lane) & 1ull;            // (a set bit of the kept or of the new word: z < D.Z)
    unsigned long long hit = 0ull;
    if (closing) {
        bool reached = false;
        if (mine) {
            const unsigned long long bits = (unsigned long long)__double_as_longlong(d[v]);
            reached = bits < FF_INF_BITS;
            if (reached) { atomicMin(&rec->tau_bits, bits); d[v] = __longlong_as_double((long long)FF_INF_BITS); }
        }
        hit = __ballot(reached);
    } else {
        if (mine && (long long)v == D.goal) {
            d[v] = 0.0;                                    // the goal cell had been closed by the table or by the gate: the field was all +inf
            rec->goal_opened = 1ull;
        }
    }
    if (lane != 0) return;
    if (!closing) open[C.wv] = changed;
    if (now == old) return;
    fm[col * D.zblocks + C.zb] = now;
    if (changed) {
        atomicAdd(&rec->changed, (unsigned long long)__popcll(changed));
        if (!closing) flags[((C.x / FF_BX) * D.nby + C.y / FF_BY) * D.nbz + C.zb] = 1u;
    }
    if (hit) atomicAdd(&rec->changed_reached, (unsigned long long)__popcll(hit));
    if (against) rec->premise_violated = 1ull;            // outside the premise: the host drops the field
}

// one workgroup per brick, the lanes on the voxels as in ff_relax_kernel
__global__ __launch_bounds__(256) void ff_repair_reset_kernel(FfDims D, double *__restrict__ d, unsigned *__restrict__ flags, FfRecord *__restrict__ rec) {
    __shared__ unsigned s_n;
    const unsigned long long tau = rec->tau_bits;
    if (tau >= FF_INF_BITS) return;                        // nothing reached has closed (the same word in every thread)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int b = blockIdx.x;
    const int bz = b % D.nbz, by = (b / D.nbz) % D.nby, bx = b / (D.nbz * D.nby);
    const int x0 = bx * FF_BX, y0 = by * FF_BY, gz = bz * FF_BZ + lane;
    if (tid == 0) s_n = 0u;
    __syncthreads();
    unsigned k = 0u;
    if (gz < D.Z)
        for (int i = 0; i < FF_PER_LANE; i++) {
            const int gx = x0 + (i >> 1), gy = y0 + 4 * (i & 1) + wave;
            if (gx >= D.X || gy >= D.Y) continue;
            double *p = d + ((size_t)gx * D.Y + gy) * D.Z + gz;
            const unsigned long long bits = (unsigned long long)__double_as_longlong(*p);
            if (bits >= tau && bits < FF_INF_BITS) { *p = __longlong_as_double((long long)FF_INF_BITS); k++; }
        }
    k = wave_sum(k);
    if (lane == 0 && k) atomicAdd(&s_n, k);
    __syncthreads();
    if (tid == 0 && s_n) {
        flags[b] = 1u;
        atomicAdd(&rec->reset, (unsigned long long)s_n);
        atomicAdd(&rec->seeded, 1ull);
    }
}

// after the rounds of the opening direction, over the box of its mark
__global__ __launch_bounds__(256) void ff_reopen_count_kernel(FfDims D, FfBox B, const double *__restrict__ d, const unsigned long long *__restrict__ open,
                                                               FfRecord *__restrict__ rec) {
    FfColumn C;
    if (!ff_box_column(B, C)) return;
    const unsigned long long opened = open[C.wv];
    if (!opened) return;                                   // (the same word in every lane of the wavefront)
    const int lane = threadIdx.x & 63;
    bool reached = false;
    if ((opened >> lane) & 1ull)                           // (an opened bit: z < D.Z)
        reached = (unsigned long long)__double_as_longlong(d[((size_t)C.x * D.Y + C.y) * D.Z + (C.zb << 6) + lane]) < FF_INF_BITS;
    const unsigned long long hit = __ballot(reached);
    if (lane == 0 && hit) atomicAdd(&rec->opened_reached, (unsigned long long)__popcll(hit));
}

// The field through a shift of the map window, the translation of its first phase.  New voxel v holds old voxel v + s.
struct FfShift { int s0, s1, s2; };

// ff_init_kernel's layout, one wavefront per 64 consecutive z of a DESTINATION column: each lane reads d_old[v + s] (64 consecutive
// doubles s away) and its old free bit from the source column's word (a z-shift that is no multiple of 64 straddles two), the new free
// ballot comes from the refreshed table.  fm1 = old & new and d1 go to the second buffers: the source words and values belong to other
// columns.  A lane whose bit fell folds its finite old d into tau; the counts are reduced in the wavefront, one atomic each.
__global__ __launch_bounds__(256) void ff_shift_kernel(FfDims D, FfShift S, const unsigned *__restrict__ cspace, const unsigned long long *__restrict__ fm_old,
                                                        const double *__restrict__ d_old, unsigned long long *__restrict__ fm1, double *__restrict__ d1,
                                                        FfRecord *__restrict__ rec, unsigned long long *__restrict__ cnt) {
    const long long wv = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (wv >= (long long)D.X * D.Y * D.zblocks) return;
    const int lane = threadIdx.x & 63;
    const int zb = (int)(wv % D.zblocks);
    const long long xy = wv / D.zblocks;
    const int z = (zb << 6) + lane;
    const size_t v = (size_t)xy * D.Z + z;
    const unsigned long long now = ff_free_ballot(D, cspace, v, z < D.Z);
    const int sx = (int)(xy / D.Y) + S.s0, sy = (int)(xy % D.Y) + S.s1, sz = z + S.s2;
    unsigned long long bits = FF_INF_BITS;
    bool was_free = false;
    if (z < D.Z && sx >= 0 && sx < D.X && sy >= 0 && sy < D.Y && sz >= 0 && sz < D.Z) {
        const size_t scol = (size_t)sx * D.Y + sy;
        bits = (unsigned long long)__double_as_longlong(d_old[scol * D.Z + sz]);
        was_free = (fm_old[scol * D.zblocks + (sz >> 6)] >> (sz & 63)) & 1ull;
    }
    const unsigned long long old = __ballot(was_free);
    const unsigned long long kept = old & now, closed = old & ~now;
    const bool reached = ((closed >> lane) & 1ull) && bits < FF_INF_BITS;
    const unsigned long long hit = __ballot(reached);
    const unsigned long long tau = wave_min(reached ? bits : FF_INF_BITS);
    // (a finite d_old lies on a voxel that was free: "kept" is "the source exists and the new word is non-zero" wherever it matters)
    if (z < D.Z) d1[v] = __longlong_as_double((long long)(((kept >> lane) & 1ull) ? bits : FF_INF_BITS));
    if (lane != 0) return;
    fm1[wv] = kept;
    if (kept) atomicAdd(cnt + FF_CNT_FREE, (unsigned long long)__popcll(kept));
    if (closed) atomicAdd(&rec->changed, (unsigned long long)__popcll(closed));
    if (hit) {
        atomicAdd(&rec->changed_reached, (unsigned long long)__popcll(hit));
        atomicMin(&rec->tau_bits, tau);
    }
}

// The leaving voxels - old voxels without a destination - close too: their finite d into tau, their number into the counters.  Over
// the whole old grid, the index test first: only the leaving slabs' values are read.
__global__ __launch_bounds__(256) void ff_left_kernel(FfDims D, FfShift S, const double *__restrict__ d_old, FfRecord *__restrict__ rec, unsigned long long *__restrict__ cnt) {
    const long long n = (long long)D.X * D.Y * D.Z;
    unsigned long long m = FF_INF_BITS, k = 0;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long long)gridDim.x * blockDim.x) {
        const long long xy = t / D.Z;
        const int tx = (int)(xy / D.Y) - S.s0, ty = (int)(xy % D.Y) - S.s1, tz = (int)(t - xy * D.Z) - S.s2;
        if (tx >= 0 && tx < D.X && ty >= 0 && ty < D.Y && tz >= 0 && tz < D.Z) continue;
        const unsigned long long bits = (unsigned long long)__double_as_longlong(d_old[t]);
        if (bits < FF_INF_BITS) { k++; m = bits < m ? bits : m; }
    }
    m = wave_min(m); k = wave_sum(k);
    if ((threadIdx.x & 63) == 0 && k) {
        atomicAdd(cnt + FF_CNT_LEFT, k);
        atomicMin(&rec->tau_bits, m);
    }
}

__global__ __launch_bounds__(256) void ff_value_kernel(FfMap M, const double *__restrict__ d, const double *__restrict__ xyz, int n, double *__restrict__ out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const double p[3] = {xyz[3 * (size_t)t], xyz[3 * (size_t)t + 1], xyz[3 * (size_t)t + 2]};
    int c[3];
    out[t] = ff_cell(M, p, c) ? d[((size_t)c[0] * M.Y + c[1]) * M.Z + c[2]] : __longlong_as_double(0x7FF0000000000000ll);
}

// One lane per start.  From the start's cell, step to the neighbour u that minimises fl(d[u] + w) - the first one in the A*'s i, j, k loop
// order (:207-211) among equals - until the goal cell; d is +inf on voxels that are not free, so only free voxels are stepped on, while
// the start cell itself need not be free (the A* never tests it, :260-278).  Attitudes as checkKernelValue would give them walking that
// way: the start at roll = pitch = 0, then the first set bit of the node's word in the breadth-first order of the previous node's
// attitude, roll = fr + (ri - fi) * ang_res (sw_manager.hpp:914-932); a node whose word has no bit in that order keeps its parent's
// attitude (cannot happen under the condition in this file's header).  A path longer than cap is walked to its end and truncated.
struct FfWalk {
    FfMap M;
    int gx, gy, gz, reachable;
    int xk, yk, nw, seq_stride;
    double max_roll, max_pitch, ang_res, w1, w2, w3;
};

__global__ __launch_bounds__(64) void ff_paths_kernel(FfWalk W, const double *__restrict__ d, const unsigned *__restrict__ cspace,
                                                       const unsigned short *__restrict__ seq, const int *__restrict__ seq_len,
                                                       const double *__restrict__ starts, int B, int cap, int *__restrict__ n_out,
                                                       double *__restrict__ xyz, double *__restrict__ rp) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= B) return;
    const FfMap &M = W.M;
    const double p[3] = {starts[3 * (size_t)t], starts[3 * (size_t)t + 1], starts[3 * (size_t)t + 2]};
    int c[3];
    if (!W.reachable || !ff_cell(M, p, c)) { n_out[t] = 0; return; }
    const double inf = __longlong_as_double(0x7FF0000000000000ll);
    double roll = 0.0, pitch = 0.0;
    const long long max_steps = (long long)M.X * M.Y * M.Z;
    long long n = 0;
    double *oxyz = xyz + (size_t)t * cap * 3, *orp = rp + (size_t)t * cap * 2;
    for (;;) {
        const bool at_goal = c[0] == W.gx && c[1] == W.gy && c[2] == W.gz;
        double best = inf;
        int bi = 0, bj = 0, bk = 0;
        if (!at_goal) {
            for (int i = -1; i < 2; i++)
                for (int j = -1; j < 2; j++)
                    for (int k = -1; k < 2; k++) {
                        if (!(i | j | k)) continue;
                        const int vx = c[0] + i, vy = c[1] + j, vz = c[2] + k;
                        if (vx < 0 || vx >= M.X || vy < 0 || vy >= M.Y || vz < 0 || vz >= M.Z) continue;
                        const int q = i * i + j * j + k * k;
                        const double cand = d[((size_t)vx * M.Y + vy) * M.Z + vz] + (q == 1 ? W.w1 : q == 2 ? W.w2 : W.w3);
                        if (cand < best) { best = cand; bi = i; bj = j; bk = k; }
                    }
            if (!(best < inf)) { n = 0; break; }                                // every neighbour is +inf: no path (only at a start: nothing is written)
        }
        if (n < cap) {
            oxyz[3 * n] = (c[0] + 0.5) * M.res + M.bmin[0];                   // getGridCubeCenter, Gridmap3D.cpp:182-194
            oxyz[3 * n + 1] = (c[1] + 0.5) * M.res + M.bmin[1];
            oxyz[3 * n + 2] = (c[2] + 0.5) * M.res + M.bmin[2];
            orp[2 * n] = roll; orp[2 * n + 1] = pitch;
        }
        n++;
        if (at_goal) break;
        if (n > max_steps) { n = 0; break; }                                    // (d falls strictly along a walk: cannot happen)
        c[0] += bi; c[1] += bj; c[2] += bk;
        const int fi = (int)((roll + W.max_roll) / W.ang_res), fj = (int)((pitch + W.max_pitch) / W.ang_res);
        if (fi >= 0 && fi < W.xk && fj >= 0 && fj < W.yk) {
            const int from = fi * W.yk + fj;
            const unsigned short *order = seq + (size_t)from * W.seq_stride;
            const int len = seq_len[from];
            const unsigned *m = cspace + (((size_t)c[0] * M.Y + c[1]) * M.Z + c[2]) * W.nw;
            for (int s = 0; s < len; s++) {
                const int a = order[s];
                if ((m[a >> 5] >> (a & 31)) & 1u) {
                    const int ri = a / W.yk, rj = a - ri * W.yk;
                    roll = roll + (ri - fi) * W.ang_res;
                    pitch = pitch + (rj - fj) * W.ang_res;
                    break;
                }
            }
        }
    }
    n_out[t] = (int)n;
}

}  // namespace isdf

using namespace isdf;

namespace {

int ff_ready(isdf_ctx *c) {
    if (!c->peers.empty() || c->is_peer || c->rccl_comm) return isdf_fail(c, ISDF_ERR_UNSUPPORTED, "cost-to-go field on a multi-device ctx");
    if (!c->fe.built) return isdf_fail(c, ISDF_ERR_STATE, "isdf_frontend_build has not been called");
    return ISDF_OK;
}

int ff_field_ready(isdf_ctx *c) {                          // ... and a field to read
    const int rdy = ff_ready(c);
    if (rdy != ISDF_OK) return rdy;
    if (!c->fe.field_valid) return isdf_fail(c, ISDF_ERR_STATE, "isdf_frontend_field_build has not been called");
    return ISDF_OK;
}

FfWalk ff_walk(const isdf_ctx *c) {
    const isdf_ctx::FrontEnd &fe = c->fe;
    FfWalk W{};
    W.M = ff_map(c);
    W.gx = fe.field_goal[0]; W.gy = fe.field_goal[1]; W.gz = fe.field_goal[2]; W.reachable = fe.field_reachable ? 1 : 0;
    W.xk = fe.xk; W.yk = fe.yk; W.nw = 4 * ((fe.xk * fe.yk + 127) / 128); W.seq_stride = fe.seq_stride;
    W.max_roll = fe.cfg.kernel_max_roll; W.max_pitch = fe.cfg.kernel_max_pitch; W.ang_res = fe.cfg.kernel_ang_res;
    W.w1 = std::sqrt(1.0); W.w2 = std::sqrt(2.0); W.w3 = std::sqrt(3.0);
    return W;
}

FfDims ff_dims(const isdf_ctx *c) {
    const DevGrid &G = c->grid;
    FfDims D{};
    D.X = G.X; D.Y = G.Y; D.Z = G.Z;
    D.nbx = (G.X + FF_BX - 1) / FF_BX; D.nby = (G.Y + FF_BY - 1) / FF_BY; D.nbz = (G.Z + FF_BZ - 1) / FF_BZ;
    D.zblocks = D.nbz; D.nw = 4 * ((c->fe.xk * c->fe.yk + 127) / 128);
    D.w1 = std::sqrt(1.0); D.w2 = std::sqrt(2.0); D.w3 = std::sqrt(3.0);
    D.goal = -1ll;
    return D;
}

long long ff_goal_index(const isdf_ctx *c) {               // FfDims::goal of the field's goal cell (fe.field_goal)
    const int *g = c->fe.field_goal;
    return g[0] >= 0 ? ((long long)g[0] * c->grid.Y + g[1]) * c->grid.Z + g[2] : -1ll;
}

// The rounds, shared by the build and the repair: ff_relax_kernel over the list + ff_compact_kernel, one pinned word read per round,
// until the list is empty or `bound` rounds have run (status 2).  n_active: the length of the list as it stands.
struct FfRounds { long long rounds = 0, visits = 0; int status = 0; };
hipError_t ff_run_rounds(isdf_ctx::FrontEnd &fe, const FfDims &D, long long n_active, long long bound, hipStream_t st, FfRounds &R) {
    const int n_bricks = D.nbx * D.nby * D.nbz;
    unsigned *flags = fe.d_field_flags.get(), *seen = flags + n_bricks;
    unsigned long long *cnt = fe.d_field_cnt.get();
    volatile unsigned long long *h = fe.h_field_cnt.get();
    hipError_t e = hipSuccess;
    while (n_active > 0) {
        if (R.rounds >= bound) { R.status = 2; break; }
        hipLaunchKernelGGL(ff_relax_kernel, dim3((unsigned)n_active), dim3(256), 0, st, D, fe.d_field_list.get(), fe.d_field.get(), fe.d_field_free.get(), flags, seen, cnt);
        hipLaunchKernelGGL(ff_compact_kernel, dim3(1), dim3(1024), 0, st, flags, fe.d_field_list.get(), cnt, fe.h_field_cnt.dev(), n_bricks);
        if ((e = hipGetLastError()) != hipSuccess) break;
        if ((e = hipStreamSynchronize(st)) != hipSuccess) break;            // the one word the host reads per round: the next list's length
        R.visits += n_active; R.rounds++;
        n_active = (long long)h[FF_CNT_ACTIVE];
    }
    return e;
}

int ff_paths_launch(isdf_ctx *c, const double *d_starts, int B, int cap, int *d_n, double *d_xyz, double *d_rp, hipStream_t st) {
    hipLaunchKernelGGL(ff_paths_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, ff_walk(c), c->fe.d_field.get(), c->fe.d_cspace.get(),
                       c->fe.d_seq.get(), c->fe.d_seq_len.get(), d_starts, B, cap, d_n, d_xyz, d_rp);
    HIPCHK(c, hipGetLastError());
    return ISDF_OK;
}

}  // namespace

int isdf_field_read_ready(isdf_ctx *c) { return ff_field_ready(c); }

extern "C" void isdf_frontend_field_params_default(isdf_frontend_field_params *out) {
    if (!out) return;
    *out = isdf_frontend_field_params{};
}

extern "C" int isdf_frontend_field_release(isdf_ctx *c) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    isdf_ctx::FrontEnd &fe = c->fe;
    (void)hipSetDevice(c->device);
    fe.d_field.release(); fe.d_field_free.release(); fe.d_field_list.release(); fe.d_field_flags.release(); fe.d_field_cnt.release();
    fe.h_field_cnt.release(); fe.field_rep.release(); fe.d_field_open.release();
    fe.d_field_shift.release(); fe.d_field_free_shift.release();
    fe.field_valid = false; fe.field_reachable = false; fe.field_repaired = false; fe.field_reopened = false; fe.field_shifted = false; fe.field_gated = false; fe.field_followed = false;
    return ISDF_OK;
}

namespace {

// what both builds refuse, in this order, before anything is launched; erode: the gated build's parameters (null: the plain build)
int ff_build_check(isdf_ctx *c, const double goal_xyz[3], const isdf_known_erode_params *erode, const isdf_frontend_field_params *params,
                   const isdf_frontend_field_info *info_out) {
    if (!goal_xyz || !info_out) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "null goal / info");
    if (params && params->max_rounds < 0) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "negative max_rounds");
    if (erode) ISDF_TRY(known_erode_check(c, *erode));
    const int rdy = ff_ready(c);
    if (rdy != ISDF_OK) return rdy;
    if (erode) ISDF_TRY(map_query::has_known(c, "the gated field needs a known grid (isdf_map_known_enable, then a map from isdf_set_pointcloud)"));
    if ((size_t)c->grid.X * c->grid.Y * c->grid.Z > (size_t)0x7FFFFFF0) return isdf_fail(c, ISDF_ERR_UNSUPPORTED, "the field indexes voxels with 31 bits");
    return ISDF_OK;
}

// The build of either kind, behind ff_build_check.  erode: the gated build - the erosion's passes are queued first, on the same
// stream, and ff_init_known_kernel reads their result; the build's first hand-over brings the erosion's record back with it.
int ff_build(isdf_ctx *c, const double goal_xyz[3], const isdf_known_erode_params *erode, const isdf_frontend_field_params *params, isdf_frontend_field_info *info_out,
             isdf_known_erode_info *gate_out) {
    isdf_ctx::FrontEnd &fe = c->fe;
    const DevGrid &G = c->grid;
    const size_t n_vox = (size_t)G.X * G.Y * G.Z;
    *info_out = isdf_frontend_field_info{};
    HIPCHK(c, hipSetDevice(c->device));
    fe.field_valid = false; fe.field_repaired = false; fe.field_reopened = false; fe.field_shifted = false; fe.field_gated = false; fe.field_followed = false;
    int gate_r = 0;
    const unsigned *d_gate = nullptr;
    if (erode) ISDF_TRY(known_erode_radius(c, *erode, &gate_r));
    if (!fe.d_cspace) {                                    // the table stays on the device: nothing of it comes to the host
        const int rc = isdf_frontend_cspace(c, nullptr, nullptr);
        if (rc != ISDF_OK) return rc;
    }
    FfDims D = ff_dims(c);
    const int n_bricks = D.nbx * D.nby * D.nbz;
    int gi[3] = {-1, -1, -1};
    const FfMap M = ff_map(c);
    const bool goal_in = ff_cell(M, goal_xyz, gi);                                          // outside the map: reachable = 0, as the A* (:244-249)
    fe.field_goal[0] = gi[0]; fe.field_goal[1] = gi[1]; fe.field_goal[2] = gi[2];
    D.goal = ff_goal_index(c);
    const size_t n_cols = (size_t)G.X * G.Y * D.zblocks;
    if (fe.d_field.reserve(c, n_vox) || fe.d_field_free.reserve(c, n_cols) || fe.d_field_list.reserve(c, (size_t)n_bricks) ||
        fe.d_field_flags.reserve(c, 2 * (size_t)n_bricks) || fe.d_field_cnt.reserve(c, FF_CNT_WORDS) || fe.h_field_cnt.reserve(c, FF_CNT_WORDS))
        return ISDF_ERR_HIP;
    unsigned *flags = fe.d_field_flags.get();
    unsigned long long *cnt = fe.d_field_cnt.get();
    volatile unsigned long long *h = fe.h_field_cnt.get();
    hipStream_t st = c->stream;
    DevEvents<2> ev;
    ISDF_TRY(ev.ready(c));
    auto fetch = [&]() {                                   // the counters -> host, one synchronisation
        hipError_t r = hipMemcpyAsync((void *)fe.h_field_cnt.get(), cnt, FF_CNT_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, st);
        return r == hipSuccess ? hipStreamSynchronize(st) : r;
    };
    if (erode) ISDF_TRY(known_erode_launch(c, gate_r, erode->border, &d_gate));       // (outside the build's own bracket: erode_ms is its time)
    HIPCHK(c, hipEventRecord(ev[0], st));
    HIPCHK(c, hipMemsetAsync(cnt, 0, FF_CNT_WORDS * sizeof(unsigned long long), st));
    HIPCHK(c, hipMemsetAsync(flags, 0, 2 * (size_t)n_bricks * sizeof(unsigned), st));
    if (erode)
        hipLaunchKernelGGL(ff_init_known_kernel, dim3((unsigned)((n_cols + 3) / 4)), dim3(256), 0, st, D, fe.d_cspace.get(), fe.d_field_free.get(), fe.d_field.get(),
                           fe.d_field_list.get(), cnt, d_gate, (long long)c->known.n_words);
    else
        hipLaunchKernelGGL(ff_init_kernel, dim3((unsigned)((n_cols + 3) / 4)), dim3(256), 0, st, D, fe.d_cspace.get(), fe.d_field_free.get(), fe.d_field.get(),
                           fe.d_field_list.get(), cnt);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, fetch());
    if (erode && gate_out) known_erode_report(c, gate_r, erode->border, gate_out);
    const long long n_free = (long long)h[FF_CNT_FREE];
    // Jacobi relaxation fixes at least the voxels with one more edge on their shortest path per round: free voxels bound the rounds
    long long bound = n_free;
    if (params && params->max_rounds > 0 && params->max_rounds < bound) bound = params->max_rounds;
    FfRounds R;
    HIPCHK(c, ff_run_rounds(fe, D, (long long)h[FF_CNT_ACTIVE], bound, st, R));
    hipLaunchKernelGGL(ff_count_kernel, dim3(1024), dim3(256), 0, st, fe.d_field.get(), (long long)n_vox, cnt);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(ev[1], st));
    HIPCHK(c, fetch());
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, ev[0], ev[1]));
    fe.field_reachable = goal_in && h[FF_CNT_REACHED] > 0;
    fe.field_valid = true;
    fe.field_status = fe.field_reachable ? R.status : 1;
    fe.field_max_rounds = params ? params->max_rounds : 0;
    fe.field_free_voxels = n_free;
    fe.field_reached_voxels = (long long)h[FF_CNT_REACHED];
    fe.field_repaired = false; fe.field_reopened = false; fe.field_shifted = false;
    info_out->reachable = fe.field_reachable ? 1 : 0;
    info_out->status = fe.field_status;
    info_out->rounds = (int32_t)R.rounds;
    info_out->bricks = (int32_t)h[FF_CNT_BRICKS];
    info_out->brick_visits = R.visits;
    info_out->free_voxels = n_free;
    info_out->reached_voxels = (long long)h[FF_CNT_REACHED];
    info_out->device_ms = ms;
    if (erode) { fe.field_gated = true; fe.field_gate_radius = gate_r; fe.field_gate_border = erode->border; }
    return ISDF_OK;
}

}  // namespace

extern "C" int isdf_frontend_field_build(isdf_ctx *c, const double goal_xyz[3], const isdf_frontend_field_params *params, isdf_frontend_field_info *info_out) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    ISDF_TRY(ff_build_check(c, goal_xyz, nullptr, params, info_out));
    return ff_build(c, goal_xyz, nullptr, params, info_out, nullptr);
}

extern "C" int isdf_frontend_field_build_known(isdf_ctx *c, const double goal_xyz[3], const isdf_known_erode_params *erode, const isdf_frontend_field_params *params,
                                               isdf_frontend_field_info *info_out, isdf_known_erode_info *gate_out) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    const isdf_known_erode_params P = map_query::resolve(erode, isdf_known_erode_params_default);
    ISDF_TRY(ff_build_check(c, goal_xyz, &P, params, info_out));
    return ff_build(c, goal_xyz, &P, params, info_out, gate_out);
}

extern "C" int isdf_frontend_field_known_info(isdf_ctx *c, int32_t out[4]) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    if (!out) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "null output");
    const isdf_ctx::FrontEnd &fe = c->fe;
    const bool gated = fe.field_valid && fe.field_gated;
    out[0] = gated ? 1 : 0; out[1] = gated ? fe.field_gate_radius : 0; out[2] = gated ? fe.field_gate_border : 0; out[3] = 0;
    return ISDF_OK;
}

// Whatever can change K or the map calls this first: a gated field describes the K of its build and is dropped, whatever the repair,
// reopen and shift modes say (an ungated field is not touched).  1: a field was dropped.
// With follow mode 1 (isdf_frontend_field_set_known_follow) a gated field that can follow is kept: the calling driver
// runs the stages or drops it (isdf_field_gate_drop).
int isdf_field_known_changed(isdf_ctx *c) {
    if (isdf_field_follow_wanted(c)) return 0;
    return isdf_field_gate_drop(c);
}

int isdf_field_gate_drop(isdf_ctx *c) {
    isdf_ctx::FrontEnd &fe = c->fe;
    if (!fe.field_gated) return 0;
    const bool was_valid = fe.field_valid;
    if (fe.field_followed) fe.field_repaired = fe.field_reopened = false;          // (the stages' reports go with the field they describe)
    fe.field_valid = false; fe.field_reachable = false; fe.field_gated = false; fe.field_followed = false;
    return was_valid ? 1 : 0;
}

bool isdf_field_follow_wanted(const isdf_ctx *c) {
    const isdf_ctx::FrontEnd &fe = c->fe;
    return c->field_known_follow_mode == 1 && fe.built && fe.field_valid && fe.field_gated && fe.field_status != 2 && (bool)fe.d_cspace && (bool)fe.d_field;
}

void isdf_field_follow_call(isdf_ctx *c) { c->fe.follow_fresh = true; }

// ---- the field following an in-place change of the map (called by map_change.hip; the rules and their premises: this file's header)
// A gated field is governed by the follow mode alone, in both directions; an ungated one by the direction's own mode.
bool isdf_field_change_wanted(const isdf_ctx *c, FfChange dir) {
    const isdf_ctx::FrontEnd &fe = c->fe;
    if (fe.field_gated) return isdf_field_follow_wanted(c);
    const int mode = dir == FfChange::Closing ? c->field_repair_mode : c->field_reopen_mode;
    return mode == 1 && fe.built && fe.field_valid && fe.field_status != 2 && (bool)fe.d_cspace && (bool)fe.d_field;
}

namespace {

// the box lo .. hi (null: the whole grid) as the box kernels take it, or the error
int ff_box(isdf_ctx *c, FfChange dir, const int lo[3], const int hi[3], FfBox &B) {
    const DevGrid &G = c->grid;
    B.x0 = lo ? lo[0] : 0; B.y0 = lo ? lo[1] : 0; B.zb0 = lo ? lo[2] >> 6 : 0;
    B.ex = (hi ? hi[0] : G.X - 1) - B.x0 + 1; B.ey = (hi ? hi[1] : G.Y - 1) - B.y0 + 1; B.ezb = ((hi ? hi[2] : G.Z - 1) >> 6) - B.zb0 + 1;
    if (B.x0 < 0 || B.y0 < 0 || B.zb0 < 0 || B.ex < 1 || B.ey < 1 || B.ezb < 1 || B.x0 + B.ex > G.X || B.y0 + B.ey > G.Y || B.zb0 + B.ezb > (G.Z + FF_BZ - 1) / FF_BZ)
        return isdf_fail(c, ISDF_ERR_INVALID_ARG, dir == FfChange::Closing ? "the field repair's box lies outside the grid" : "the field reopen's box lies outside the grid");
    return ISDF_OK;
}

unsigned ff_box_blocks(const FfBox &B) { return (unsigned)(((long long)B.ex * B.ey * B.ezb + 3) / 4); }      // four wavefronts per workgroup

}  // namespace

// Enqueues, after the configuration-space refresh on the ctx's stream: the direction's mark over the box, closing: the reset,
// ff_compact_kernel and the record's copy to the host.  The caller synchronises the stream, then calls ..._end with the same box.
int isdf_field_change_begin(isdf_ctx *c, FfChange dir, const int lo[3], const int hi[3], hipEvent_t ev_start) {
    isdf_ctx::FrontEnd &fe = c->fe;
    const bool closing = dir == FfChange::Closing;
    FfDims D = ff_dims(c);
    const int n_bricks = D.nbx * D.nby * D.nbz;
    ISDF_TRY(fe.field_rep.ready(c));
    // the opened words are sized for the whole grid at once: no box of a later clear grows them
    if (!closing && fe.d_field_open.reserve(c, (size_t)D.X * D.Y * D.zblocks)) return ISDF_ERR_HIP;
    FfBox B;
    const int rc = ff_box(c, dir, lo, hi, B);
    if (rc != ISDF_OK) return rc;
    if (!closing) D.goal = ff_goal_index(c);
    FfRecord *rec = fe.field_rep.dev();
    unsigned long long *cnt = fe.d_field_cnt.get();
    unsigned *flags = fe.d_field_flags.get();
    const hipStream_t st = c->stream;
    // a gated field: K eroded again at the field's own radius and border, queued with no synchronisation of its own and outside the
    // stage's bracket (erode_ms is its time); its record comes back with the stage's hand-over
    const bool gated = fe.field_gated;
    const unsigned *d_gate = nullptr;
    if (gated) {
        ISDF_TRY(map_query::has_known(c, "the gated field's follow needs the known grid"));
        ISDF_TRY(known_erode_launch(c, fe.field_gate_radius, fe.field_gate_border, &d_gate));
    }
    const long long gate_words = (long long)c->known.n_words;
    HIPCHK(c, hipEventRecord(ev_start, st));
    HIPCHK(c, fe.field_rep.put(ff_record_empty(), st));
    HIPCHK(c, hipMemsetAsync(cnt, 0, FF_CNT_WORDS * sizeof(unsigned long long), st));
    HIPCHK(c, hipMemsetAsync(flags, 0, 2 * (size_t)n_bricks * sizeof(unsigned), st));
    if (closing) {
        if (gated)
            hipLaunchKernelGGL(ff_mark_known_kernel<FfChange::Closing>, dim3(ff_box_blocks(B)), dim3(256), 0, st, D, B, fe.d_cspace.get(), fe.d_field_free.get(),
                               fe.d_field.get(), (unsigned *)nullptr, (unsigned long long *)nullptr, rec, d_gate, gate_words);
        else
            hipLaunchKernelGGL(ff_mark_kernel<FfChange::Closing>, dim3(ff_box_blocks(B)), dim3(256), 0, st, D, B, fe.d_cspace.get(), fe.d_field_free.get(), fe.d_field.get(),
                               (unsigned *)nullptr, (unsigned long long *)nullptr, rec);
        hipLaunchKernelGGL(ff_repair_reset_kernel, dim3((unsigned)n_bricks), dim3(256), 0, st, D, fe.d_field.get(), flags, rec);
    } else if (gated)
        hipLaunchKernelGGL(ff_mark_known_kernel<FfChange::Opening>, dim3(ff_box_blocks(B)), dim3(256), 0, st, D, B, fe.d_cspace.get(), fe.d_field_free.get(), fe.d_field.get(),
                           flags, fe.d_field_open.get(), rec, d_gate, gate_words);
    else
        hipLaunchKernelGGL(ff_mark_kernel<FfChange::Opening>, dim3(ff_box_blocks(B)), dim3(256), 0, st, D, B, fe.d_cspace.get(), fe.d_field_free.get(), fe.d_field.get(),
                           flags, fe.d_field_open.get(), rec);
    hipLaunchKernelGGL(ff_compact_kernel, dim3(1), dim3(1024), 0, st, flags, fe.d_field_list.get(), cnt, fe.h_field_cnt.dev(), n_bricks);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, fe.field_rep.fetch(st));
    return ISDF_OK;
}

// After the stream has been synchronised: the rounds from the seeded bricks, the counts.  *kept = 1: the field is valid again (status
// 2 when the round bound was hit, as after a build); 0: a bit had moved against the direction, the field stays dropped.
int isdf_field_change_end(isdf_ctx *c, FfChange dir, const int lo[3], const int hi[3], hipEvent_t ev_start, hipEvent_t ev_end, int *kept) {
    isdf_ctx::FrontEnd &fe = c->fe;
    const bool closing = dir == FfChange::Closing;
    *kept = 0;
    const FfRecord &rec = fe.field_rep.host();
    if (rec.premise_violated) return ISDF_OK;
    const FfDims D = ff_dims(c);
    FfBox B;
    const int rc = ff_box(c, dir, lo, hi, B);
    if (rc != ISDF_OK) return rc;
    const hipStream_t st = c->stream;
    volatile unsigned long long *h = fe.h_field_cnt.get();
    const long long n_seeded = (long long)h[FF_CNT_ACTIVE], reached_before = fe.field_reached_voxels;
    const long long n_free = fe.field_free_voxels + (closing ? -(long long)rec.changed : (long long)rec.changed);
    long long bound = n_free;
    if (fe.field_max_rounds > 0 && fe.field_max_rounds < bound) bound = fe.field_max_rounds;
    FfRounds R;
    // opening: a field without a reachable goal whose goal cell did not open is all +inf and stays so: nothing to relax
    if (closing || reached_before > 0 || rec.goal_opened) HIPCHK(c, ff_run_rounds(fe, D, n_seeded, bound, st, R));
    hipLaunchKernelGGL(ff_count_kernel, dim3(1024), dim3(256), 0, st, fe.d_field.get(), (long long)D.X * D.Y * D.Z, fe.d_field_cnt.get());
    if (!closing) hipLaunchKernelGGL(ff_reopen_count_kernel, dim3(ff_box_blocks(B)), dim3(256), 0, st, D, B, fe.d_field.get(), fe.d_field_open.get(), fe.field_rep.dev());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(ev_end, st));
    HIPCHK(c, hipMemcpyAsync((void *)fe.h_field_cnt.get(), fe.d_field_cnt.get(), FF_CNT_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    if (!closing) HIPCHK(c, fe.field_rep.fetch(st));
    HIPCHK(c, hipStreamSynchronize(st));
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, ev_start, ev_end));
    fe.field_reachable = fe.field_goal[0] >= 0 && h[FF_CNT_REACHED] > 0;
    fe.field_status = fe.field_reachable ? R.status : 1;
    fe.field_free_voxels = n_free;
    fe.field_reached_voxels = (long long)h[FF_CNT_REACHED];
    fe.field_valid = true;
    if (closing) {
        fe.field_repaired = true;
        isdf_field_repair_info &I = fe.field_repair;
        I = isdf_field_repair_info{};
        I.closed_voxels = (int64_t)rec.changed;
        I.closed_reached = (int64_t)rec.changed_reached;
        std::memcpy(&I.tau, &rec.tau_bits, sizeof(double));
        I.reset_voxels = (int64_t)(rec.reset + rec.changed_reached);
        I.seeded_bricks = (int32_t)rec.seeded;
        I.rounds = (int32_t)R.rounds; I.brick_visits = R.visits;
        I.free_voxels = n_free; I.reached_voxels = fe.field_reached_voxels;
        I.reachable = fe.field_reachable ? 1 : 0; I.status = fe.field_status;
        I.device_ms = ms;
    } else {
        fe.field_reopened = true;
        isdf_field_reopen_info &I = fe.field_reopen;
        I = isdf_field_reopen_info{};
        I.opened_voxels = (int64_t)rec.changed;
        I.opened_reached = (int64_t)rec.opened_reached;
        I.reached_before = reached_before;
        I.seeded_bricks = (int32_t)n_seeded;
        I.goal_opened = rec.goal_opened ? 1 : 0;
        I.rounds = (int32_t)R.rounds; I.brick_visits = R.visits;
        I.free_voxels = n_free; I.reached_voxels = fe.field_reached_voxels;
        I.reachable = fe.field_reachable ? 1 : 0; I.status = fe.field_status;
        I.device_ms = ms;
    }
    if (fe.field_gated) {                                  // the followed call's report: this stage added to it
        isdf_known_erode_info E;
        known_erode_report(c, fe.field_gate_radius, fe.field_gate_border, &E);              // (the stage's hand-over brought the record back)
        isdf_field_follow_info &I = fe.field_follow;
        if (fe.follow_fresh || !fe.field_followed) I = isdf_field_follow_info{};
        fe.follow_fresh = false; fe.field_followed = true;
        if (closing) { I.closing++; I.closed_voxels += (int64_t)rec.changed; }
        else { I.opening++; I.opened_voxels += (int64_t)rec.changed; }
        I.radius_used = E.radius_used; I.border = E.border;
        I.known_voxels = E.known_voxels; I.eroded_voxels = E.eroded_voxels;
        I.free_voxels = n_free; I.reached_voxels = fe.field_reached_voxels;
        I.reachable = fe.field_reachable ? 1 : 0; I.status = fe.field_status;
        I.erode_ms += E.erode_ms; I.device_ms += ms;
    }
    *kept = 1;
    return ISDF_OK;
}

// One stage on its own, for a change of K without a table refresh (isdf_map_known_fill): the field is invalid from here until the
// stage has gone through; a failure or a bit against the direction leaves it dropped.
int isdf_field_follow_stage(isdf_ctx *c, FfChange dir, const int lo[3], const int hi[3], hipEvent_t ev_start, hipEvent_t ev_end, int *kept) {
    isdf_ctx::FrontEnd &fe = c->fe;
    *kept = 0;
    fe.field_valid = false; fe.field_reachable = false;
    int rc = isdf_field_change_begin(c, dir, lo, hi, ev_start);
    if (rc == ISDF_OK && hipStreamSynchronize(c->stream) != hipSuccess) rc = isdf_fail(c, ISDF_ERR_HIP, "the gated field's follow: the mark failed");
    if (rc == ISDF_OK) rc = isdf_field_change_end(c, dir, lo, hi, ev_start, ev_end, kept);
    if (rc != ISDF_OK || !*kept) {
        const std::string err = c->err;
        (void)hipStreamSynchronize(c->stream);
        fe.field_valid = false;
        (void)isdf_field_gate_drop(c);
        c->err = err;
        *kept = 0;
    }
    return rc;
}

// ---- the field carried through a shift of the map window (called by map_shift.hip; the rule and its proof: DESIGN 4.6.4)
bool isdf_field_shift_wanted(const isdf_ctx *c, const int32_t s[3]) {
    const isdf_ctx::FrontEnd &fe = c->fe;
    if (c->field_shift_mode != 1 || !fe.built || !fe.field_valid || fe.field_gated || fe.field_status == 2 || !fe.d_cspace || !fe.d_field) return false;
    const int dims[3] = {c->grid.X, c->grid.Y, c->grid.Z};
    for (int a = 0; a < 3; a++) {
        if (s[a] <= -dims[a] || s[a] >= dims[a]) return false;                              // everything left
        const long long g = (long long)fe.field_goal[a] - s[a];                              // goal' = goal - s
        if (fe.field_goal[a] < 0 || g < 0 || g >= dims[a]) return false;
    }
    return true;
}

// Enqueues, after the shift's configuration-space refresh on the ctx's stream: the translation into the second buffers, which then
// change places with the field's own, the leaving voxels' tau, the closing direction's reset on the translated graph, ff_compact_kernel
// and the record's and the counters' copies to the host.  The goal cell becomes goal'.  The caller synchronises the stream, then calls
// ..._end.
int isdf_field_shift_begin(isdf_ctx *c, const int32_t s[3], hipEvent_t ev_start) {
    isdf_ctx::FrontEnd &fe = c->fe;
    for (int a = 0; a < 3; a++) fe.field_goal[a] -= s[a];
    FfDims D = ff_dims(c);
    D.goal = ff_goal_index(c);
    const int n_bricks = D.nbx * D.nby * D.nbz;
    const size_t n_vox = (size_t)D.X * D.Y * D.Z, n_cols = (size_t)D.X * D.Y * D.zblocks;
    if (fe.d_field_shift.reserve(c, n_vox) || fe.d_field_free_shift.reserve(c, n_cols) || fe.field_rep.ready(c) ||
        fe.d_field_cnt.reserve(c, FF_CNT_WORDS) || fe.h_field_cnt.reserve(c, FF_CNT_WORDS))
        return ISDF_ERR_HIP;
    FfRecord *rec = fe.field_rep.dev();
    unsigned long long *cnt = fe.d_field_cnt.get();
    unsigned *flags = fe.d_field_flags.get();
    const FfShift S{s[0], s[1], s[2]};
    const hipStream_t st = c->stream;
    HIPCHK(c, hipEventRecord(ev_start, st));
    HIPCHK(c, fe.field_rep.put(ff_record_empty(), st));
    HIPCHK(c, hipMemsetAsync(cnt, 0, FF_CNT_WORDS * sizeof(unsigned long long), st));
    HIPCHK(c, hipMemsetAsync(flags, 0, 2 * (size_t)n_bricks * sizeof(unsigned), st));
    hipLaunchKernelGGL(ff_shift_kernel, dim3((unsigned)((n_cols + 3) / 4)), dim3(256), 0, st, D, S, fe.d_cspace.get(), fe.d_field_free.get(), fe.d_field.get(),
                       fe.d_field_free_shift.get(), fe.d_field_shift.get(), rec, cnt);
    hipLaunchKernelGGL(ff_left_kernel, dim3(1024), dim3(256), 0, st, D, S, fe.d_field.get(), rec, cnt);
    fe.d_field.swap(fe.d_field_shift);
    fe.d_field_free.swap(fe.d_field_free_shift);
    hipLaunchKernelGGL(ff_repair_reset_kernel, dim3((unsigned)n_bricks), dim3(256), 0, st, D, fe.d_field.get(), flags, rec);
    hipLaunchKernelGGL(ff_compact_kernel, dim3(1), dim3(1024), 0, st, flags, fe.d_field_list.get(), cnt, fe.h_field_cnt.dev(), n_bricks);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, fe.field_rep.fetch(st));
    HIPCHK(c, hipMemcpyAsync((void *)fe.h_field_cnt.get(), cnt, FF_CNT_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    return ISDF_OK;
}

// After the stream has been synchronised: phase 1's rounds on the translated graph and its count, then phase 2 - the opening direction
// of isdf_field_change_begin / _end over the box lo .. hi (null: the whole grid), which leaves the field valid (status 2 when either
// phase hit the round bound).  ev: [0] recorded by ..._begin, [1] the end of phase 1, [2], [3] around phase 2.  The last reopen's report
// is not this call's to change: it is put back.
int isdf_field_shift_end(isdf_ctx *c, const int32_t s[3], const int lo[3], const int hi[3], const hipEvent_t ev[4]) {
    isdf_ctx::FrontEnd &fe = c->fe;
    FfDims D = ff_dims(c);
    D.goal = ff_goal_index(c);
    const FfRecord rec = fe.field_rep.host();            // (a copy: phase 2 uses the record again)
    const hipStream_t st = c->stream;
    volatile unsigned long long *h = fe.h_field_cnt.get();
    const long long n_seeded = (long long)h[FF_CNT_ACTIVE], n_free1 = (long long)h[FF_CNT_FREE], n_left = (long long)h[FF_CNT_LEFT];
    long long bound = n_free1;
    if (fe.field_max_rounds > 0 && fe.field_max_rounds < bound) bound = fe.field_max_rounds;
    FfRounds R1;
    HIPCHK(c, ff_run_rounds(fe, D, n_seeded, bound, st, R1));
    hipLaunchKernelGGL(ff_count_kernel, dim3(1024), dim3(256), 0, st, fe.d_field.get(), (long long)D.X * D.Y * D.Z, fe.d_field_cnt.get());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(ev[1], st));
    HIPCHK(c, hipMemcpyAsync((void *)fe.h_field_cnt.get(), fe.d_field_cnt.get(), FF_CNT_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    fe.field_free_voxels = n_free1;                        // what the opening direction starts from: the translated graph's counts
    fe.field_reached_voxels = (long long)h[FF_CNT_REACHED];

    const bool had_reopen = fe.field_reopened;
    const isdf_field_reopen_info last_reopen = fe.field_reopen;
    int kept = 0;
    int rc = isdf_field_change_begin(c, FfChange::Opening, lo, hi, ev[2]);
    if (rc == ISDF_OK && hipStreamSynchronize(st) != hipSuccess) rc = isdf_fail(c, ISDF_ERR_HIP, "field carry: the opening mark failed");
    if (rc == ISDF_OK) rc = isdf_field_change_end(c, FfChange::Opening, lo, hi, ev[2], ev[3], &kept);
    const isdf_field_reopen_info O = fe.field_reopen;
    fe.field_reopened = had_reopen; fe.field_reopen = last_reopen;
    if (rc != ISDF_OK) return rc;
    // fm1 is a subset of the new free set by construction: a bit against the opening direction is a defect, not a reason to drop
    if (!kept) return isdf_fail(c, ISDF_ERR_STATE, "field carry: a free bit of the translated graph is not free in the new map");
    if (R1.status == 2 && fe.field_reachable) fe.field_status = 2;
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, ev[0], ev[1]));
    fe.field_shifted = true;
    isdf_field_shift_info &I = fe.field_shift;
    I = isdf_field_shift_info{};
    for (int a = 0; a < 3; a++) { I.shift[a] = s[a]; I.goal_new[a] = fe.field_goal[a]; }
    I.left_reached = n_left;
    I.closed_voxels = (int64_t)rec.changed;
    I.closed_reached = (int64_t)rec.changed_reached;
    std::memcpy(&I.tau, &rec.tau_bits, sizeof(double));
    I.reset_voxels = (int64_t)(rec.reset + rec.changed_reached);
    I.seeded_bricks_close = (int32_t)rec.seeded; I.rounds_close = (int32_t)R1.rounds;
    I.opened_voxels = O.opened_voxels; I.opened_reached = O.opened_reached; I.goal_opened = O.goal_opened;
    I.seeded_bricks_open = O.seeded_bricks; I.rounds_open = O.rounds;
    I.brick_visits = R1.visits + O.brick_visits;
    I.free_voxels = O.free_voxels; I.reached_voxels = O.reached_voxels;
    I.reachable = fe.field_reachable ? 1 : 0; I.status = fe.field_status;
    I.device_ms = (double)ms + O.device_ms;
    return ISDF_OK;
}

namespace {

int ff_set_mode(isdf_ctx *c, int mode, int isdf_ctx::*slot, const char *bad_mode) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    if (mode != 0 && mode != 1) return isdf_fail(c, ISDF_ERR_INVALID_ARG, bad_mode);
    if (!c->peers.empty() || c->is_peer || c->rccl_comm) return isdf_fail(c, ISDF_ERR_UNSUPPORTED, "cost-to-go field on a multi-device ctx");
    c->*slot = mode;
    return ISDF_OK;
}

template <class Info> int ff_last_info(isdf_ctx *c, Info *out, bool have, const Info &last, const char *none) {
    if (!out) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "null output");
    if (!have) return isdf_fail(c, ISDF_ERR_STATE, none);
    *out = last;
    return ISDF_OK;
}

}  // namespace

extern "C" int isdf_frontend_field_set_reopen(isdf_ctx *c, int mode) {
    return ff_set_mode(c, mode, &isdf_ctx::field_reopen_mode, "the field's reopen mode is 0 (drop) or 1 (lower in place)");
}

extern "C" int isdf_frontend_field_reopen_info(isdf_ctx *c, isdf_field_reopen_info *out) {
    return c ? ff_last_info(c, out, c->fe.field_reopened, c->fe.field_reopen, "no reopen since the last isdf_frontend_field_build") : ISDF_ERR_INVALID_ARG;
}

extern "C" void isdf_frontend_field_reopen_sizes(int sizes_out[1]) {
    if (sizes_out) sizes_out[0] = (int)sizeof(isdf_field_reopen_info);
}

extern "C" int isdf_frontend_field_set_shift(isdf_ctx *c, int mode) {
    return ff_set_mode(c, mode, &isdf_ctx::field_shift_mode, "the field's shift mode is 0 (drop) or 1 (carry)");
}

extern "C" int isdf_frontend_field_shift_info(isdf_ctx *c, isdf_field_shift_info *out) {
    return c ? ff_last_info(c, out, c->fe.field_shifted, c->fe.field_shift, "no carried shift since the last isdf_frontend_field_build") : ISDF_ERR_INVALID_ARG;
}

extern "C" void isdf_frontend_field_shift_sizes(int sizes_out[1]) {
    if (sizes_out) sizes_out[0] = (int)sizeof(isdf_field_shift_info);
}

extern "C" int isdf_frontend_field_set_known_follow(isdf_ctx *c, int mode) {
    return ff_set_mode(c, mode, &isdf_ctx::field_known_follow_mode, "the gated field's follow mode is 0 (drop) or 1 (follow in place)");
}

extern "C" int isdf_frontend_field_follow_info(isdf_ctx *c, isdf_field_follow_info *out) {
    return c ? ff_last_info(c, out, c->fe.field_valid && c->fe.field_gated && c->fe.field_followed, c->fe.field_follow, "no followed change since the last isdf_frontend_field_build_known")
             : ISDF_ERR_INVALID_ARG;
}

extern "C" void isdf_frontend_field_follow_sizes(int sizes_out[1]) {
    if (sizes_out) sizes_out[0] = (int)sizeof(isdf_field_follow_info);
}

extern "C" int isdf_frontend_field_set_repair(isdf_ctx *c, int mode) {
    return ff_set_mode(c, mode, &isdf_ctx::field_repair_mode, "the field's repair mode is 0 (drop) or 1 (repair)");
}

extern "C" int isdf_frontend_field_repair_info(isdf_ctx *c, isdf_field_repair_info *out) {
    return c ? ff_last_info(c, out, c->fe.field_repaired, c->fe.field_repair, "no repair since the last isdf_frontend_field_build") : ISDF_ERR_INVALID_ARG;
}

extern "C" void isdf_frontend_field_repair_sizes(int sizes_out[1]) {
    if (sizes_out) sizes_out[0] = (int)sizeof(isdf_field_repair_info);
}

extern "C" int isdf_frontend_field_get(isdf_ctx *c, double *d_out) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    if (!d_out) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "null output");
    const int rdy = ff_field_ready(c);
    if (rdy != ISDF_OK) return rdy;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n_vox = (size_t)c->grid.X * c->grid.Y * c->grid.Z;
    HIPCHK(c, hipMemcpyAsync(d_out, c->fe.d_field.get(), n_vox * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ISDF_OK;
}

extern "C" int isdf_frontend_field_value(isdf_ctx *c, const double *xyz, int n, double *out) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    if (n < 0 || (n > 0 && (!xyz || !out))) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "bad field query");
    const int rdy = ff_field_ready(c);
    if (rdy != ISDF_OK) return rdy;
    if (n == 0) return ISDF_OK;
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf<double> buf;                                    // [xyz 3n | values n]
    HIPCHK(c, buf.alloc((size_t)4 * n));
    HIPCHK(c, hipMemcpyAsync(buf.get(), xyz, (size_t)3 * n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(ff_value_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, ff_map(c), c->fe.d_field.get(), buf.get(), n, buf.get() + (size_t)3 * n);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(out, buf.get() + (size_t)3 * n, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream);
    const hipError_t es = hipStreamSynchronize(c->stream);                                  // (before the scoped buffer goes)
    HIPCHK(c, e);
    HIPCHK(c, es);
    return ISDF_OK;
}

extern "C" int isdf_frontend_field_paths_device(isdf_ctx *c, const double *d_starts_xyz, int B, int cap, int32_t *d_n_out, double *d_xyz_out,
                                                double *d_roll_pitch_out, void *stream) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    if (B < 0 || cap < 1 || (B > 0 && (!d_starts_xyz || !d_n_out || !d_xyz_out || !d_roll_pitch_out))) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "bad field path query");
    const int rdy = ff_field_ready(c);
    if (rdy != ISDF_OK) return rdy;
    if (B == 0) return ISDF_OK;
    HIPCHK(c, hipSetDevice(c->device));
    return ff_paths_launch(c, d_starts_xyz, B, cap, d_n_out, d_xyz_out, d_roll_pitch_out, (hipStream_t)stream);
}

extern "C" int isdf_frontend_field_paths(isdf_ctx *c, const double *starts_xyz, int B, int cap, int32_t *n_out, double *xyz_out, double *roll_pitch_out) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    if (B < 0 || cap < 1 || (B > 0 && (!starts_xyz || !n_out || !xyz_out || !roll_pitch_out))) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "bad field path query");
    const int rdy = ff_field_ready(c);
    if (rdy != ISDF_OK) return rdy;
    if (B == 0) return ISDF_OK;
    HIPCHK(c, hipSetDevice(c->device));
    // one scoped allocation: [starts 3B | xyz 3 B cap | roll, pitch 2 B cap | n B ints]
    const size_t n_d = (size_t)3 * B + (size_t)5 * B * cap;
    DevBuf<double> buf;
    HIPCHK(c, buf.alloc(n_d + ((size_t)B + 1) / 2));
    double *d_s = buf.get(), *d_xyz = d_s + (size_t)3 * B, *d_rp = d_xyz + (size_t)3 * B * cap;
    int *d_n = (int *)(d_rp + (size_t)2 * B * cap);
    hipError_t e = hipMemcpyAsync(d_s, starts_xyz, (size_t)3 * B * sizeof(double), hipMemcpyHostToDevice, c->stream);
    // rows come back whole: what lies past a path's end is zero
    if (e == hipSuccess) e = hipMemsetAsync(d_xyz, 0, (size_t)5 * B * cap * sizeof(double), c->stream);
    int rc = ISDF_OK;
    if (e == hipSuccess) rc = ff_paths_launch(c, d_s, B, cap, d_n, d_xyz, d_rp, c->stream);
    if (e == hipSuccess && rc == ISDF_OK) e = hipMemcpyAsync(n_out, d_n, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && rc == ISDF_OK) e = hipMemcpyAsync(xyz_out, d_xyz, (size_t)3 * B * cap * sizeof(double), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && rc == ISDF_OK) e = hipMemcpyAsync(roll_pitch_out, d_rp, (size_t)2 * B * cap * sizeof(double), hipMemcpyDeviceToHost, c->stream);
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (rc != ISDF_OK) return rc;
    HIPCHK(c, e);
    HIPCHK(c, es);
    return ISDF_OK;
}

namespace {

// What the host forms share: the argument checks, the goal as ints, the call; run(g, info) fills the direction's own counts of the
// info and returns whether the goal cell is free.  1 / 0 = that answer, ISDF_ERR_HIP when the host ran out of memory.
template <class Info, class F> int ff_host_form(const uint32_t *mask, const int32_t dims[3], int n_att, const int32_t goal_index[3], double *d, Info *info_out, F run) {
    if (!mask || !dims || !goal_index || !d || n_att < 1 || dims[0] < 1 || dims[1] < 1 || dims[2] < 1) return ISDF_ERR_INVALID_ARG;
    const int g[3] = {goal_index[0], goal_index[1], goal_index[2]};
    try {
        Info I{};
        const bool goal_free = run(g, I);
        I.reachable = goal_free ? 1 : 0;
        I.status = goal_free ? 0 : 1;
        if (info_out) *info_out = I;
        return goal_free ? 1 : 0;
    } catch (const std::bad_alloc &) {
        return ISDF_ERR_HIP;
    }
}

}  // namespace

extern "C" int isdf_frontend_field_host(const uint32_t *free_mask, const int32_t dims[3], int n_att, const int32_t goal_index[3], double *d_out) {
    return ff_host_form(free_mask, dims, n_att, goal_index, d_out, (isdf_frontend_field_info *)nullptr, [&](const int g[3], isdf_frontend_field_info &) {
        return isdf_host::field_dijkstra(free_mask, dims[0], dims[1], dims[2], n_att, g, d_out);
    });
}

extern "C" int isdf_frontend_field_repair_host(const uint32_t *free_mask_new, const int32_t dims[3], int n_att, const int32_t goal_index[3], double *d_inout,
                                               isdf_field_repair_info *info_out) {
    return ff_host_form(free_mask_new, dims, n_att, goal_index, d_inout, info_out, [&](const int g[3], isdf_field_repair_info &I) {
        isdf_host::FieldRepairCounts C;
        const bool goal_free = isdf_host::field_repair(free_mask_new, dims[0], dims[1], dims[2], n_att, g, d_inout, &C);
        I.closed_voxels = I.closed_reached = C.closed_reached;      // (a closed voxel that had not been reached cannot be told from one that was never free)
        I.tau = C.tau;
        I.reset_voxels = C.reset_voxels;
        I.free_voxels = C.free_voxels;
        I.reached_voxels = C.reached_voxels;
        return goal_free;
    });
}

extern "C" int isdf_frontend_field_reopen_host(const uint32_t *free_mask_new, const int32_t dims[3], int n_att, const int32_t goal_index[3], double *d_inout,
                                               isdf_field_reopen_info *info_out) {
    return ff_host_form(free_mask_new, dims, n_att, goal_index, d_inout, info_out, [&](const int g[3], isdf_field_reopen_info &I) {
        isdf_host::FieldReopenCounts C;
        const bool goal_free = isdf_host::field_reopen(free_mask_new, dims[0], dims[1], dims[2], n_att, g, d_inout, &C);
        I.opened_voxels = I.opened_reached = C.newly_reached;       // (an opened voxel that stays +inf cannot be told from a free one that was never reached)
        I.reached_before = C.reached_before;
        I.reached_voxels = C.reached_voxels;
        I.free_voxels = C.free_voxels;
        I.goal_opened = C.goal_opened ? 1 : 0;
        return goal_free;
    });
}

extern "C" int isdf_frontend_field_shift_host(const uint32_t *free_mask_new, const int32_t dims[3], int n_att, const int32_t shift[3], const int32_t goal_index_old[3],
                                              double *d_inout, isdf_field_shift_info *info_out) {
    if (!shift) return ISDF_ERR_INVALID_ARG;
    bool goal_left = false;
    isdf_field_shift_info I{};
    const int rc = ff_host_form(free_mask_new, dims, n_att, goal_index_old, d_inout, &I, [&](const int g[3], isdf_field_shift_info &J) {
        const int s[3] = {shift[0], shift[1], shift[2]};
        isdf_host::FieldShiftCounts C;
        const bool goal_free = isdf_host::field_shift(free_mask_new, dims[0], dims[1], dims[2], n_att, s, g, d_inout, &C);
        goal_left = C.goal_left;
        for (int a = 0; a < 3; a++) { J.shift[a] = s[a]; J.goal_new[a] = g[a] - s[a]; }
        J.left_reached = C.left_reached;
        J.closed_voxels = J.closed_reached = C.close.closed_reached;      // (no old table: as isdf_frontend_field_repair_host)
        J.tau = C.close.tau;
        J.reset_voxels = C.close.reset_voxels;
        J.opened_voxels = J.opened_reached = C.open.newly_reached;        // (as isdf_frontend_field_reopen_host)
        J.goal_opened = C.open.goal_opened ? 1 : 0;
        J.free_voxels = C.open.free_voxels;
        J.reached_voxels = C.open.reached_voxels;
        return goal_free;
    });
    if (rc < 0) return rc;
    if (goal_left) I.status = ISDF_FIELD_SHIFT_GOAL_LEFT;
    if (info_out) *info_out = I;
    return goal_left ? ISDF_FIELD_SHIFT_GOAL_LEFT : rc;
}
