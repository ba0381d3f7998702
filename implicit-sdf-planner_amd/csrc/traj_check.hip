// Trajectory clearance check on the device (isdf_traj_check*, isdf_traj_collide): what the reference's
// SweptVolumeManager::isTrajCollide (sw_manager.hpp:764, a stub that returns false) is called for at the end of generateTraj
// (plan_manager.cpp) - how close the swept volume of a trajectory comes to any occupied voxel centre of the WHOLE map.
//
//   select   the occupied voxels that can matter.  The field query skips a coarse sample whose position is farther from the point
//            than far_r = R + (2 safety_hor + 0.1) (mesh robots: band x 1.05) - swept_sweep.hip, scan_body - so a point that far
//            from EVERY coarse sample has no in-range run and reads 10 / -1.  Dropping it changes no result: the selection only
//            has to be a superset of the points inside some sample's sphere.  The samples are the table the query's own prepare
//            kernel builds (same doubles, the CLOSED sample included).  Box of the samples grown by far_r -> 8 x 8 x 8 bricks
//            against the samples (radius grown by the brick's half-diagonal; each live brick keeps the range of sample indices
//            that reach it) -> the occupied voxels of live bricks singly, one wavefront per z-row, d_occ read 64 consecutive bytes
//            at a time.  Ballot masks per row, row counts, one exclusive scan, emit: candidates come out by ascending voxel index.
//            A shape with no bound radius: every occupied voxel of the grid (culled = 0).
//   field    the candidates through swept_field_run (swept_mesh.hip), PLANNER or CLOSED.
//   reduce   (value, t*) of the candidates -> minimum with its point (ties: lowest voxel index - the candidates are in voxel
//            order, so the lowest list position), counts below the margin / below 0, per piece of the trajectory the smallest value
//            among the points whose t* lies in it, and the points below the margin compacted in voxel order.  Minima and integer
//            sums only: the report does not depend on the launch geometry, and two runs give the same bytes.
#include "swept_field.hpp"
#include "dev_reduce.hpp"
#include "dev_scan.hpp"
#include "traj_call.hpp"
#include <climits>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace {

constexpr int BRICK = 8;                 // voxels per brick edge
constexpr int SEL_WAVES = 4;             // z-rows per workgroup of the row kernels

int fail(isdf_ctx *c, int code, const char *msg) { return isdf_fail(c, code, msg); }

// (SelBox, voxel_centre, stage_samples and the single-voxel test sample_within: swept_field.hpp - the fold's list kernel shares them)

// per brick of the box: the first and last coarse sample within far_r + half-diagonal of its centre (first > last: none)
__global__ __launch_bounds__(256) void tc_brick_kernel(SelBox B, const double *__restrict__ pose, const int *__restrict__ n_coarse,
                                                       int2 *__restrict__ range) {
    __shared__ double s_pos[3 * SWEPT_MAX_COARSE];
    const int n = min(*n_coarse, SWEPT_MAX_COARSE);
    stage_samples(pose, n, s_pos);
    const long long n_bricks = (long long)B.nb[0] * B.nb[1] * B.nb[2];
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < n_bricks; t += (long long)gridDim.x * blockDim.x) {
        const int bz = (int)(t % B.nb[2]), by = (int)((t / B.nb[2]) % B.nb[1]), bx = (int)(t / ((long long)B.nb[2] * B.nb[1]));
        // centre of the brick's 8 x 8 x 8 voxel centres: index + 3.5 -> (index + 4) * res + origin
        const double cx = (double)((B.b0[0] + bx) * BRICK + BRICK / 2) * B.res + B.bmin[0];
        const double cy = (double)((B.b0[1] + by) * BRICK + BRICK / 2) * B.res + B.bmin[1];
        const double cz = (double)((B.b0[2] + bz) * BRICK + BRICK / 2) * B.res + B.bmin[2];
        int first = n, last = -1;
        for (int k = 0; k < n; k++) {
            const double dx = cx - s_pos[k], dy = cy - s_pos[SWEPT_MAX_COARSE + k], dz = cz - s_pos[2 * SWEPT_MAX_COARSE + k];
            if (!(dx * dx + dy * dy + dz * dz > B.bfar2)) { first = min(first, k); last = k; }
        }
        range[t] = make_int2(first, last);
    }
}

// one wavefront per z-row (x, y) of the box: mask[row][chunk] = the candidates among 64 consecutive voxels, count[row] = their
// number; stats[0] += occupied voxels of the box, stats[1] += candidates.  KNOWN: `occ` is the known grid's words (map_known.hip) and
// the per-lane test is "known bit clear" in place of "occupancy byte set" - the known horizon's selection; everything else is shared,
// and the <false> instance is the check's kernel instruction for instruction.
template <bool KNOWN>
__global__ __launch_bounds__(64 * SEL_WAVES) void tc_row_kernel(SelBox B, const uint8_t *__restrict__ occ, const int2 *__restrict__ range,
                                                                const double *__restrict__ pose, const int *__restrict__ n_coarse,
                                                                unsigned long long *__restrict__ mask, int *__restrict__ count,
                                                                unsigned long long *stats) {
    __shared__ double s_pos[3 * SWEPT_MAX_COARSE];
    const int n = min(*n_coarse, SWEPT_MAX_COARSE);
    if (B.cull) stage_samples(pose, n, s_pos);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ny = B.hi[1] - B.lo[1] + 1;
    const long long n_rows = (long long)(B.hi[0] - B.lo[0] + 1) * ny;
    const long long row = (long long)blockIdx.x * SEL_WAVES + wave;
    if (row >= n_rows) return;
    const int x = B.lo[0] + (int)(row / ny), y = B.lo[1] + (int)(row % ny);
    const uint8_t *o = occ + ((size_t)x * B.Y + y) * B.Z;
    const double px = voxel_centre(x, B.res, B.bmin[0]), py = voxel_centre(y, B.res, B.bmin[1]);
    const long long brick_row = ((long long)(x / BRICK - B.b0[0]) * B.nb[1] + (y / BRICK - B.b0[1])) * B.nb[2];
    unsigned long long n_occ = 0;
    int n_sel = 0;
    for (int ch = 0; ch < B.n_chunks; ch++) {
        const int z = B.lo[2] + ch * 64 + lane;
        bool occupied;
        if constexpr (KNOWN) {
            const size_t a = ((size_t)x * B.Y + y) * B.Z + (size_t)(z <= B.hi[2] ? z : B.hi[2]);
            occupied = z <= B.hi[2] && !((((const unsigned *)occ)[a >> 5] >> (unsigned)(a & 31)) & 1u);
        } else occupied = z <= B.hi[2] && o[z] != 0;
        bool sel = occupied;
        if (occupied && B.cull) {
            const int2 r = range[brick_row + (z / BRICK - B.b0[2])];
            const double pz = voxel_centre(z, B.res, B.bmin[2]);
            sel = false;
            for (int k = r.x; k <= r.y && !sel; k++) sel = sample_within(px, py, pz, s_pos, k, B.far2);
        }
        const unsigned long long m = __ballot(sel);
        if (lane == 0) mask[row * B.n_chunks + ch] = m;
        n_sel += __popcll(m);
        n_occ += occupied ? 1ull : 0ull;
    }
    n_occ = wave_sum(n_occ);
    if (lane == 0) {
        count[row] = n_sel;
        if (n_occ) atomicAdd(&stats[0], n_occ);
        if (n_sel) atomicAdd(&stats[1], (unsigned long long)n_sel);
    }
}

// candidates of a row from its masks, at base[row]: voxel index (x * Y + y) * Z + z and centre
__global__ __launch_bounds__(64 * SEL_WAVES) void tc_emit_kernel(SelBox B, const unsigned long long *__restrict__ mask,
                                                                 const int *__restrict__ base, long long *__restrict__ vox,
                                                                 double *__restrict__ xyz) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ny = B.hi[1] - B.lo[1] + 1;
    const long long n_rows = (long long)(B.hi[0] - B.lo[0] + 1) * ny;
    const long long row = (long long)blockIdx.x * SEL_WAVES + wave;
    if (row >= n_rows) return;
    const int x = B.lo[0] + (int)(row / ny), y = B.lo[1] + (int)(row % ny);
    const double px = voxel_centre(x, B.res, B.bmin[0]), py = voxel_centre(y, B.res, B.bmin[1]);
    long long out = base[row];
    for (int ch = 0; ch < B.n_chunks; ch++) {
        const unsigned long long m = mask[row * B.n_chunks + ch];
        if ((m >> lane) & 1ull) {
            const int z = B.lo[2] + ch * 64 + lane;
            const long long pos = out + __popcll(m & ((1ull << lane) - 1ull));
            vox[pos] = ((long long)x * B.Y + y) * B.Z + z;
            xyz[3 * pos] = px; xyz[3 * pos + 1] = py; xyz[3 * pos + 2] = voxel_centre(z, B.res, B.bmin[2]);
        }
        out += __popcll(m);
    }
}

// ---- reduction ------------------------------------------------------------------------------------------------------
// doubles as unsigned keys of the same order (an integer atomicMin then is the minimum of the doubles)
__device__ __forceinline__ unsigned long long ordered_key(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double ordered_value(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}
// the piece a global time lies in: Trajectory::locatePieceIdx's sequential subtraction with its `>` rule (traj_locate_l)
__device__ __forceinline__ int locate_piece(const double *T, int N, double t) {
    int idx = 0;
    while (idx < N && t > T[idx]) { t -= T[idx]; idx++; }
    return idx == N ? N - 1 : idx;
}
struct MinRec { double v; long long j; };          // value and list position; j = LLONG_MAX: nothing yet
__device__ __forceinline__ MinRec min_rec(MinRec a, MinRec b) { return (b.v < a.v || (b.v == a.v && b.j < a.j)) ? b : a; }
__device__ __forceinline__ MinRec wave_min_rec(MinRec r) {
    for (int off = 32; off >= 1; off >>= 1) {
        MinRec o;
        o.v = __shfl_xor(r.v, off, 64); o.j = __shfl_xor(r.j, off, 64);
        r = min_rec(r, o);
    }
    return r;
}
__device__ __forceinline__ MinRec block_min_rec(MinRec r, MinRec *s_w) {       // 256 threads; the result in thread 0
    r = wave_min_rec(r);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = r;
    __syncthreads();
    if (threadIdx.x == 0) for (int w = 1; w < 4; w++) r = min_rec(r, s_w[w]);
    return r;
}

// per candidate: qualified (value != 10), below the margin (flag), below 0, the piece of its t* (piece_key: ordered-key minimum);
// per workgroup the smallest (value, position); counts[0..2] += qualified, below margin, penetrating
__global__ __launch_bounds__(256) void tc_reduce_kernel(long long n, const double *__restrict__ val, const double *__restrict__ ts,
                                                        const double *__restrict__ T, int N, double margin, int *__restrict__ flag,
                                                        unsigned long long *piece_key, MinRec *__restrict__ partial,
                                                        unsigned long long *counts) {
    __shared__ MinRec s_w[4];
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    MinRec r{1.0e300, LLONG_MAX};
    unsigned long long q = 0, below = 0, pen = 0;
    if (j < n) {
        const double v = val[j];
        const bool qualified = v != 1e1;
        if (qualified) {
            r.v = v; r.j = j;
            q = 1; below = v < margin ? 1 : 0; pen = v < 0.0 ? 1 : 0;
            atomicMin(&piece_key[locate_piece(T, N, ts[j])], ordered_key(v));
        }
        flag[j] = (int)below;
    }
    q = wave_sum(q); below = wave_sum(below); pen = wave_sum(pen);
    if ((threadIdx.x & 63) == 0) {
        if (q) atomicAdd(&counts[0], q);
        if (below) atomicAdd(&counts[1], below);
        if (pen) atomicAdd(&counts[2], pen);
    }
    r = block_min_rec(r, s_w);
    if (threadIdx.x == 0) partial[blockIdx.x] = r;
}

// what the device hands back: TC_REPORT_WORDS doubles (swept_field.hpp)
constexpr int REPORT_WORDS = TC_REPORT_WORDS;
__global__ __launch_bounds__(256) void tc_final_kernel(const MinRec *__restrict__ partial, int n_partial, const double *__restrict__ val,
                                                       const double *__restrict__ ts, const long long *__restrict__ vox,
                                                       const double *__restrict__ xyz, const double *__restrict__ T, int N,
                                                       const unsigned long long *__restrict__ piece_key, double *__restrict__ piece_min,
                                                       double *__restrict__ report) {
    __shared__ MinRec s_w[4];
    MinRec r{1.0e300, LLONG_MAX};
    for (int k = threadIdx.x; k < n_partial; k += blockDim.x) r = min_rec(r, partial[k]);
    r = block_min_rec(r, s_w);
    if (threadIdx.x == 0) {
        long long voxel = -1, piece = -1;
        if (r.j == LLONG_MAX) {
            report[0] = 1e1; report[1] = -1.0; report[2] = report[3] = report[4] = 0.0;
        } else {
            report[0] = r.v; report[1] = ts[r.j];
            report[2] = xyz[3 * r.j]; report[3] = xyz[3 * r.j + 1]; report[4] = xyz[3 * r.j + 2];
            voxel = vox[r.j]; piece = locate_piece(T, N, ts[r.j]);
        }
        report[5] = __longlong_as_double(voxel); report[6] = __longlong_as_double(piece);
    }
    for (int i = threadIdx.x; i < N; i += blockDim.x) piece_min[i] = ordered_value(piece_key[i]);
}
__global__ void tc_key_fill_kernel(unsigned long long *piece_key, int N) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) piece_key[i] = ordered_key(1e1);
}
// the points below the margin, in list (= voxel) order: (x, y, z, value, t*)
__global__ void tc_rows_kernel(long long n, const int *__restrict__ flag, const int *__restrict__ base, const double *__restrict__ xyz,
                               const double *__restrict__ val, const double *__restrict__ ts, double *__restrict__ rows) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n || !flag[j]) return;
    double *o = rows + 5 * (size_t)base[j];
    o[0] = xyz[3 * j]; o[1] = xyz[3 * j + 1]; o[2] = xyz[3 * j + 2]; o[3] = val[j]; o[4] = ts[j];
}
// ... and their voxel indices next to them (isdf_points_merge_check keys the obstacle-point set by them)
__global__ void tc_row_vox_kernel(long long n, const int *__restrict__ flag, const int *__restrict__ base, const long long *__restrict__ vox,
                                  long long *__restrict__ row_vox) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n || !flag[j]) return;
    row_vox[base[j]] = vox[j];
}

// ---- the known horizon's reduction (isdf_traj_known_horizon): integer-keyed minima only, so two runs give the same bytes.
// rec: [0..2] += qualified, below the margin, penetrating; [3] min ordered_key(t*) among the candidates below the margin, [4] the lowest
// list position (= lowest voxel index: the list ascends) among those that reach it; [5], [6] the same for the value among the qualified
constexpr int TH_WORDS = 8;
__global__ __launch_bounds__(256) void th_key_kernel(long long n, const double *__restrict__ val, const double *__restrict__ ts, double margin,
                                                     unsigned long long *rec) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long q = 0, below = 0, pen = 0;
    if (j < n) {
        const double v = val[j];
        if (v != 1e1) {
            q = 1; below = v < margin ? 1 : 0; pen = v < 0.0 ? 1 : 0;
            atomicMin(&rec[5], ordered_key(v));
            if (below) atomicMin(&rec[3], ordered_key(ts[j]));
        }
    }
    q = wave_sum(q); below = wave_sum(below); pen = wave_sum(pen);
    if ((threadIdx.x & 63) == 0) {
        if (q) atomicAdd(&rec[0], q);
        if (below) atomicAdd(&rec[1], below);
        if (pen) atomicAdd(&rec[2], pen);
    }
}
__global__ __launch_bounds__(256) void th_pos_kernel(long long n, const double *__restrict__ val, const double *__restrict__ ts, double margin,
                                                     unsigned long long *rec) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const double v = val[j];
    if (v == 1e1) return;
    if (ordered_key(v) == rec[5]) atomicMin(&rec[6], (unsigned long long)j);
    if (v < margin && ordered_key(ts[j]) == rec[3]) atomicMin(&rec[4], (unsigned long long)j);
}

// ---- host ---------------------------------------------------------------------------------------------------------------
void free_rows(TrajCheckState *s) {
    s->d_rows.release();
    s->d_row_vox.release();
    s->n_rows = 0; s->have = false;
    s->w.armed = false;                 // the report the watch folds into is gone
}

// what can be checked without a ctx (reported through isdf_last_error(NULL) when there is none)
int check_args(isdf_ctx *c, int N, const void *T, const void *coeffs, const isdf_traj_check_params *p) {
    if (N < 1 || !T || !coeffs) return fail(c, ISDF_ERR_INVALID_ARG, "trajectory check: null trajectory");
    if (p) {
        if (p->mode != ISDF_SWEPT_FIELD_PLANNER && p->mode != ISDF_SWEPT_FIELD_CLOSED) return fail(c, ISDF_ERR_INVALID_ARG, "trajectory check: unknown mode");
        if (!std::isfinite(p->margin)) return fail(c, ISDF_ERR_INVALID_ARG, "trajectory check: margin must be finite");
    }
    return ISDF_OK;
}
// ... and what needs one; margin_out = the margin in force
int check_state(isdf_ctx *c, const isdf_traj_check_params *p, double *margin_out) {
    ISDF_TRY(swept_check_ctx(c));
    if (!c->have_geom || !c->d_occ)
        return fail(c, ISDF_ERR_INVALID_ARG, "trajectory check: no occupancy grid (isdf_set_grid with ISDF_GRID_OCCUPANCY, or isdf_set_pointcloud)");
    const double band = 2 * c->cfg.safety_hor + 0.1;
    const double margin = (p && p->margin >= 0.0) ? p->margin : c->cfg.safety_hor;
    if (margin > band)
        return fail(c, ISDF_ERR_INVALID_ARG, "trajectory check: margin above 2 safety_hor + 0.1 - points beyond that band read 10, the query cannot answer it");
    *margin_out = margin;
    return ISDF_OK;
}

// The select step of the check and of the known horizon: the voxels of `src` that pass the row kernel's test (known == false: occupancy
// byte set; true: src is the known grid, bit clear) within far_r of a coarse sample, in ascending voxel index, with their centres.
struct Selection {
    SelBox B{}; bool empty = true, cull = false; double far_r = 0.0;
    unsigned long long cnt[2] = {0, 0};         // voxels of the box that pass the test; candidates
    DevBuf<long long> vox; DevBuf<double> xyz;
};
int select_run(isdf_ctx *c, SweptMeshState *s, int N, const double *d_T, const double *d_C, int mode, const uint8_t *src, bool known, const char *op,
               Selection &L, hipStream_t st) {
    // ---- select: the coarse positions, their box, bricks, rows, scan, emit
    ISDF_TRY(swept_field_coarse_table(c, N, d_T, d_C, mode, st));
    std::vector<double> pos(3 * (size_t)SWEPT_MAX_COARSE);
    int n_coarse = 0;
    HIPCHK(c, hipMemcpyAsync(pos.data(), s->field.coarse_pose, pos.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(&n_coarse, s->field.n_coarse, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    const bool mesh = c->shape.kind == ISDF_SHAPE_MESH;
    const double R = mesh ? std::max(c->mesh_rmax, c->shape.bound_radius) : c->shape.bound_radius;
    const bool cull = L.cull = R > 0.0 && std::isfinite(R);
    const double band = 2 * c->cfg.safety_hor + 0.1;
    const double far_r = L.far_r = cull ? R + band * (mesh ? 1.05 : 1.0) : 0.0;       // the scan's own expression (swept_sweep.hip, scan_body)
    const DevGrid &G = c->grid;
    SelBox &B = L.B;
    B = SelBox{};
    B.X = G.X; B.Y = G.Y; B.Z = G.Z; B.res = G.res;
    const int dim[3] = {G.X, G.Y, G.Z};
    bool &empty = L.empty;
    empty = n_coarse < 1;
    for (int a = 0; a < 3 && !empty; a++) {
        B.bmin[a] = G.bmin[a];
        if (!cull) { B.lo[a] = 0; B.hi[a] = dim[a] - 1; continue; }
        double mn = 1e300, mx = -1e300;
        for (int i = 0; i < n_coarse; i++) { const double v = pos[(size_t)a * SWEPT_MAX_COARSE + i]; mn = std::min(mn, v); mx = std::max(mx, v); }
        if (!std::isfinite(mn) || !std::isfinite(mx)) return fail(c, ISDF_ERR_INVALID_ARG, (std::string(op) + ": non-finite trajectory position").c_str());
        // voxels whose centre (i + 0.5) res + origin can lie within far_r of a sample on this axis, one more on either side for the rounding
        const double l = std::floor((mn - far_r - G.bmin[a]) / G.res - 0.5) - 1.0, h = std::floor((mx + far_r - G.bmin[a]) / G.res - 0.5) + 2.0;
        if (h < 0.0 || l > (double)(dim[a] - 1)) { empty = true; break; }
        B.lo[a] = (int)std::max(l, 0.0); B.hi[a] = (int)std::min(h, (double)(dim[a] - 1));
    }
    B.cull = cull ? 1 : 0;
    const double slack = 1.0 + 1e-9;        // the scan compares its own rounding of the same distance: never tighter than it
    const double bdiag = std::sqrt(3.0) * (BRICK / 2) * G.res;        // brick centre to its farthest voxel centre is sqrt(3) 3.5 res
    B.far2 = far_r * far_r * slack; B.bfar2 = (far_r + bdiag) * (far_r + bdiag) * slack;
    unsigned long long *const cnt = L.cnt;
    cnt[0] = cnt[1] = 0;
    DevBuf<long long> &vox = L.vox;
    DevBuf<double> &xyz = L.xyz;
    if (!empty) {
        for (int a = 0; a < 3; a++) { B.b0[a] = B.lo[a] / BRICK; B.nb[a] = B.hi[a] / BRICK - B.b0[a] + 1; }
        B.n_chunks = (B.hi[2] - B.lo[2] + 64) / 64;
        const long long n_rows = (long long)(B.hi[0] - B.lo[0] + 1) * (B.hi[1] - B.lo[1] + 1);
        const long long n_bricks = (long long)B.nb[0] * B.nb[1] * B.nb[2];
        DevBuf<int2> range;
        DevBuf<unsigned long long> mask, d_cnt;
        DevBuf<int> count, base;
        HIPCHK(c, range.alloc((size_t)n_bricks));
        HIPCHK(c, mask.alloc((size_t)n_rows * B.n_chunks));
        HIPCHK(c, count.alloc((size_t)n_rows)); HIPCHK(c, base.alloc((size_t)n_rows));
        HIPCHK(c, d_cnt.alloc(2));
        HIPCHK(c, hipMemsetAsync(d_cnt.get(), 0, 2 * sizeof(unsigned long long), st));
        if (cull) hipLaunchKernelGGL(tc_brick_kernel, dim3(std::min<unsigned>(blocks(n_bricks), 4096u)), dim3(256), 0, st, B,
                                     (const double *)s->field.coarse_pose, (const int *)s->field.n_coarse, range.get());
        if (known) hipLaunchKernelGGL(tc_row_kernel<true>, dim3(blocks(n_rows, SEL_WAVES)), dim3(64 * SEL_WAVES), 0, st, B, src,
                                      (const int2 *)range.get(), (const double *)s->field.coarse_pose, (const int *)s->field.n_coarse, mask.get(), count.get(), d_cnt.get());
        else hipLaunchKernelGGL(tc_row_kernel<false>, dim3(blocks(n_rows, SEL_WAVES)), dim3(64 * SEL_WAVES), 0, st, B, src,
                                (const int2 *)range.get(), (const double *)s->field.coarse_pose, (const int *)s->field.n_coarse, mask.get(), count.get(), d_cnt.get());
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(cnt, d_cnt.get(), 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        if (cnt[1] > (unsigned long long)INT32_MAX) return fail(c, ISDF_ERR_OVERFLOW, (std::string(op) + ": more than 2^31 candidate voxels").c_str());
        if (cnt[1]) {
            DevBuf<unsigned char> tmp;          // (freed behind the scan)
            ISDF_TRY(exclusive_sum(c, tmp, count.get(), base.get(), n_rows, st)); tmp.release();
            HIPCHK(c, vox.alloc((size_t)cnt[1]));
            HIPCHK(c, xyz.alloc((size_t)cnt[1] * 3));
            hipLaunchKernelGGL(tc_emit_kernel, dim3(blocks(n_rows, SEL_WAVES)), dim3(64 * SEL_WAVES), 0, st, B,
                               (const unsigned long long *)mask.get(), (const int *)base.get(), vox.get(), xyz.get());
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipStreamSynchronize(st));          // (mask / count / base go out of scope here)
        }
    }
    return ISDF_OK;
}

// the check on device arrays; hT = the durations on the host.  d_piece_min: N doubles on the device (required).
int check_run(isdf_ctx *c, int N, const double *d_T, const double *d_C, const int mode, const double margin,
              isdf_traj_check_info *info, double *d_piece_min, hipStream_t st) {
    TrajCheckState *k;
    ISDF_TRY(c->tck.make(c, &k));
    free_rows(k);
    SweptMeshState *s;
    ISDF_TRY(swept_field_scratch(c, &s));
    DevEvents<4> ev;
    ISDF_TRY(ev.ready(c));
    HIPCHK(c, hipEventRecord(ev[0], st));

    Selection L;
    ISDF_TRY(select_run(c, s, N, d_T, d_C, mode, (const uint8_t *)c->d_occ, false, "trajectory check", L, st));
    const bool cull = L.cull, empty = L.empty;
    const double far_r = L.far_r;
    const SelBox &B = L.B;
    const unsigned long long *const cnt = L.cnt;
    DevBuf<long long> &vox = L.vox;
    DevBuf<double> &xyz = L.xyz;
    const long long n = (long long)cnt[1];
    HIPCHK(c, hipEventRecord(ev[1], st));

    // ---- field
    DevBuf<double> val, ts;
    HIPCHK(c, val.alloc((size_t)n)); HIPCHK(c, ts.alloc((size_t)n));
    ISDF_TRY(swept_field_run(c, N, d_T, d_C, xyz.get(), n, mode, val.get(), ts.get(), st));
    HIPCHK(c, hipEventRecord(ev[2], st));

    // ---- reduce
    TcReduceScratch red;
    DevBuf<unsigned long long> d_counts;
    DevBuf<double> report;
    HIPCHK(c, d_counts.alloc(3)); HIPCHK(c, report.alloc(REPORT_WORDS));
    ISDF_TRY(tc_reduce_launch(c, red, n, val.get(), ts.get(), vox.get(), xyz.get(), d_T, N, margin, d_counts.get(), report.get(), d_piece_min, st));
    unsigned long long counts[3];
    double rep[REPORT_WORDS];
    HIPCHK(c, hipMemcpyAsync(counts, d_counts.get(), sizeof(counts), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(rep, report.get(), sizeof(rep), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (counts[1]) {
        HIPCHK(c, k->d_rows.alloc((size_t)counts[1] * 5));
        HIPCHK(c, k->d_row_vox.alloc((size_t)counts[1]));
        ISDF_TRY(tc_rows_launch(c, red, n, val.get(), ts.get(), vox.get(), xyz.get(), k->d_rows.get(), k->d_row_vox.get(), st));
    }
    HIPCHK(c, hipEventRecord(ev[3], st));
    HIPCHK(c, hipStreamSynchronize(st));
    k->n_rows = (long long)counts[1]; k->have = true; k->grid_epoch = c->grid_epoch;
    isdf_traj_check_info own_info;
    const bool watch = c->traj_watch_mode == 1;
    if (!info && watch) info = &own_info;
    if (info) {
        std::memset(info, 0, sizeof(*info));
        info->occupied_in_box = (long long)cnt[0];
        info->candidates = n;
        info->qualified = (long long)counts[0];
        info->n_below_margin = (long long)counts[1];
        info->n_penetrating = (long long)counts[2];
        info->min_clearance = rep[0]; info->min_tstar = rep[1];
        for (int a = 0; a < 3; a++) info->min_point[a] = rep[2 + a];
        long long w;
        std::memcpy(&w, &rep[5], sizeof(w)); info->min_voxel = w;
        std::memcpy(&w, &rep[6], sizeof(w)); info->min_piece = (int32_t)w;
        info->culled = cull ? 1 : 0;
        info->margin = margin; info->far_r = far_r;
        float ms[3] = {0.f, 0.f, 0.f};
        for (int q = 0; q < 3; q++) HIPCHK(c, hipEventElapsedTime(&ms[q], ev[q], ev[q + 1]));
        info->select_ms = ms[0]; info->field_ms = ms[1]; info->reduce_ms = ms[2];
    }
    if (watch) {
        // arm: the trajectory, the parameters in force, the report and its piece minima, the selection box (mode 1 of
        // isdf_traj_check_set_watch; the rows and their voxel ids are the kept ones)
        TrajWatchState &w = k->w;
        ISDF_TRY(w.d_traj.reserve(c, (size_t)20 * N));
        if (d_T != w.d_traj.get()) {            // (a whole-map re-check runs on the kept copy itself)
            HIPCHK(c, hipMemcpyAsync(w.d_traj, d_T, (size_t)N * sizeof(double), hipMemcpyDeviceToDevice, st));
            HIPCHK(c, hipMemcpyAsync(w.d_traj + N, d_C, (size_t)18 * N * sizeof(double), hipMemcpyDeviceToDevice, st));
        }
        w.piece_min.assign((size_t)N, 1e1);
        HIPCHK(c, hipMemcpyAsync(w.piece_min.data(), d_piece_min, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        w.N = N; w.mode = mode; w.margin = margin;
        w.info = *info;
        w.box = B; w.box_empty = empty;
        w.last = isdf_traj_watch_info{};
        w.last.new_min_clearance = 1e1; w.last.new_min_tstar = -1.0; w.last.new_min_voxel = -1; w.last.new_min_piece = -1;
        w.armed = true;
    }
    return ISDF_OK;
}

}  // namespace

int tc_reduce_launch(isdf_ctx *c, TcReduceScratch &S, long long n, const double *d_val, const double *d_ts, const long long *d_vox, const double *d_xyz,
                     const double *d_T, int N, double margin, unsigned long long *d_counts, double *d_report, double *d_piece_min, hipStream_t st) {
    const int n_part = (int)std::max<long long>(1, blocks(n));
    ISDF_TRY(S.flag.reserve(c, (size_t)std::max<long long>(n, 1)));
    ISDF_TRY(S.fbase.reserve(c, (size_t)std::max<long long>(n, 1)));
    ISDF_TRY(S.key.reserve(c, (size_t)N));
    ISDF_TRY(S.partial.reserve(c, (size_t)n_part * sizeof(MinRec)));
    HIPCHK(c, hipMemsetAsync(d_counts, 0, 3 * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(tc_key_fill_kernel, dim3(blocks(N)), dim3(256), 0, st, S.key.get(), N);
    if (n > 0) hipLaunchKernelGGL(tc_reduce_kernel, dim3(n_part), dim3(256), 0, st, n, d_val, d_ts, d_T, N, margin, S.flag.get(), S.key.get(),
                                  (MinRec *)S.partial.get(), d_counts);
    hipLaunchKernelGGL(tc_final_kernel, dim3(1), dim3(256), 0, st, (const MinRec *)S.partial.get(), n > 0 ? n_part : 0, d_val, d_ts, d_vox, d_xyz, d_T, N,
                       (const unsigned long long *)S.key.get(), d_piece_min, d_report);
    HIPCHK(c, hipGetLastError());
    return ISDF_OK;
}

int tc_rows_launch(isdf_ctx *c, TcReduceScratch &S, long long n, const double *d_val, const double *d_ts, const long long *d_vox, const double *d_xyz,
                   double *d_rows, long long *d_row_vox, hipStream_t st) {
    if (n <= 0) return ISDF_OK;
    ISDF_TRY(exclusive_sum(c, S.scan_tmp, S.flag.get(), S.fbase.get(), n, st));
    hipLaunchKernelGGL(tc_rows_kernel, dim3(blocks(n)), dim3(256), 0, st, n, (const int *)S.flag.get(), (const int *)S.fbase.get(), d_xyz, d_val, d_ts, d_rows);
    hipLaunchKernelGGL(tc_row_vox_kernel, dim3(blocks(n)), dim3(256), 0, st, n, (const int *)S.flag.get(), (const int *)S.fbase.get(), d_vox, d_row_vox);
    HIPCHK(c, hipGetLastError());
    return ISDF_OK;
}

int traj_check_rerun_kept(isdf_ctx *c, isdf_traj_check_info *info) {
    TrajWatchState &w = c->tck->w;
    return check_run(c, w.N, w.d_traj, w.d_traj + w.N, w.mode, w.margin, info, w.d_traj + 19 * (size_t)w.N, c->stream);
}

void traj_check_drop_report(isdf_ctx *c) { if (c->tck) free_rows(c->tck.get()); }

int isdf_traj_check_ready(isdf_ctx *c) {
    double margin = 0.0;
    return check_state(c, nullptr, &margin);
}

extern "C" void isdf_traj_check_params_default(isdf_traj_check_params *p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->margin = -1.0;                       // negative: cfg.safety_hor of the ctx
    p->mode = ISDF_SWEPT_FIELD_PLANNER;
}

extern "C" int isdf_traj_check_device(isdf_ctx *c, int N, const double *d_T, const double *d_coeffs, const isdf_traj_check_params *p,
                                      isdf_traj_check_info *info_out, double *d_piece_min_out, void *stream) {
    ISDF_TRY(check_args(c, N, d_T, d_coeffs, p));
    if (!c) return fail(nullptr, ISDF_ERR_INVALID_ARG, "trajectory check: null ctx");
    double margin = 0.0;
    ISDF_TRY(check_state(c, p, &margin));
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;
    std::vector<double> hT(N);          // the 300 s rule needs the durations on the host
    HIPCHK(c, hipMemcpyAsync(hT.data(), d_T, N * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    ISDF_TRY(swept_check_traj(c, N, hT.data()));
    DevBuf<double> own;
    if (!d_piece_min_out) { HIPCHK(c, own.alloc((size_t)N)); d_piece_min_out = own.get(); }
    return check_run(c, N, d_T, d_coeffs, p ? p->mode : ISDF_SWEPT_FIELD_PLANNER, margin, info_out, d_piece_min_out, st);
}

extern "C" int isdf_traj_check(isdf_ctx *c, int N, const double *T, const double *coeffs, const isdf_traj_check_params *p,
                               isdf_traj_check_info *info_out, double *piece_min_out) {
    ISDF_TRY(check_args(c, N, T, coeffs, p));
    if (!c) return fail(nullptr, ISDF_ERR_INVALID_ARG, "trajectory check: null ctx");
    double margin = 0.0;
    ISDF_TRY(check_state(c, p, &margin));
    ISDF_TRY(swept_check_traj(c, N, T));
    for (int q = 0; q < 18 * N; q++) if (!std::isfinite(coeffs[q])) return fail(c, ISDF_ERR_INVALID_ARG, "trajectory check: non-finite coefficient");
    HIPCHK(c, hipSetDevice(c->device));
    TrajCheckState *k;
    ISDF_TRY(c->tck.make(c, &k));
    hipStream_t st = c->stream;
    ISDF_TRY(k->d_traj.reserve(c, (size_t)20 * N));     // T | coeffs | per-piece minima
    ISDF_TRY(traj_call::upload(c, k->d_traj, (size_t)N, T, coeffs, st));        // (its own 19 N fit: the layout stays)
    double *d_pm = k->d_traj + 19 * (size_t)N;
    ISDF_TRY(check_run(c, N, k->d_traj, k->d_traj + N, p ? p->mode : ISDF_SWEPT_FIELD_PLANNER, margin, info_out, d_pm, st));
    if (piece_min_out) HIPCHK(c, hipMemcpy(piece_min_out, d_pm, N * sizeof(double), hipMemcpyDeviceToHost));
    return ISDF_OK;
}

extern "C" int isdf_traj_check_get(isdf_ctx *c, double *rows_out, long long capacity) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    if (!c->tck || !c->tck->have) return fail(c, ISDF_ERR_STATE, "trajectory check: nothing kept (isdf_traj_check)");
    TrajCheckState *k = c->tck.get();
    if (capacity < k->n_rows) return fail(c, ISDF_ERR_OVERFLOW, "trajectory check: output capacity smaller than the number of points below the margin");
    if (k->n_rows > 0 && !rows_out) return fail(c, ISDF_ERR_INVALID_ARG, "trajectory check: null output");
    HIPCHK(c, hipSetDevice(c->device));
    if (k->n_rows) HIPCHK(c, hipMemcpy(rows_out, k->d_rows, (size_t)k->n_rows * 5 * sizeof(double), hipMemcpyDeviceToHost));
    return ISDF_OK;
}

extern "C" int isdf_traj_check_release(isdf_ctx *c) {
    if (!c) return ISDF_ERR_INVALID_ARG;
    if (c->tck) free_rows(c->tck.get());
    return ISDF_OK;
}

extern "C" int isdf_traj_collide(isdf_ctx *c, int N, const double *T, const double *coeffs) {
    isdf_traj_check_info info;
    ISDF_TRY(isdf_traj_check(c, N, T, coeffs, nullptr, &info, nullptr));
    return info.n_penetrating > 0 ? 1 : 0;
}

// ---- the known horizon of a trajectory: the check's three steps on the UNKNOWN voxels (known bit clear, occupied or not)
// with the earliest t* below the margin as the reduction.  Own scoped scratch; the kept report, the watch and the V1 state stay.
namespace {

int horizon_run(isdf_ctx *c, int N, const double *hT, const double *d_T, const double *d_C, int mode, double margin, isdf_traj_known_info *info, hipStream_t st) {
    SweptMeshState *s;
    ISDF_TRY(swept_field_scratch(c, &s));
    DevEvents<4> ev;
    ISDF_TRY(ev.ready(c));
    HIPCHK(c, hipEventRecord(ev[0], st));
    Selection L;
    ISDF_TRY(select_run(c, s, N, d_T, d_C, mode, (const uint8_t *)c->known.d_bits.get(), true, "known horizon", L, st));
    const long long n = (long long)L.cnt[1];
    HIPCHK(c, hipEventRecord(ev[1], st));
    DevBuf<double> val, ts;
    HIPCHK(c, val.alloc((size_t)n)); HIPCHK(c, ts.alloc((size_t)n));
    ISDF_TRY(swept_field_run(c, N, d_T, d_C, L.xyz.get(), n, mode, val.get(), ts.get(), st));
    HIPCHK(c, hipEventRecord(ev[2], st));
    DevBuf<unsigned long long> d_rec;
    unsigned long long rec[TH_WORDS] = {0, 0, 0, ~0ull, ~0ull, ~0ull, ~0ull, 0};
    HIPCHK(c, d_rec.alloc(TH_WORDS));
    HIPCHK(c, hipMemcpyAsync(d_rec.get(), rec, sizeof(rec), hipMemcpyHostToDevice, st));
    if (n > 0) {
        hipLaunchKernelGGL(th_key_kernel, dim3(blocks(n)), dim3(256), 0, st, n, (const double *)val.get(), (const double *)ts.get(), margin, d_rec.get());
        hipLaunchKernelGGL(th_pos_kernel, dim3(blocks(n)), dim3(256), 0, st, n, (const double *)val.get(), (const double *)ts.get(), margin, d_rec.get());
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipMemcpyAsync(rec, d_rec.get(), sizeof(rec), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipEventRecord(ev[3], st));
    HIPCHK(c, hipStreamSynchronize(st));
    isdf_traj_known_info out{};
    out.unknown_in_box = (int64_t)L.cnt[0]; out.candidates = n;
    out.qualified = (int64_t)rec[0]; out.n_below_margin = (int64_t)rec[1]; out.n_penetrating = (int64_t)rec[2];
    out.horizon_t = -1.0; out.horizon_voxel = -1; out.horizon_value = 1e1; out.horizon_piece = -1;
    out.min_clearance = 1e1; out.min_voxel = -1;
    if (rec[1] > 0) {
        const size_t j = (size_t)rec[4];
        long long v = -1;
        HIPCHK(c, hipMemcpyAsync(&out.horizon_t, ts.get() + j, sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemcpyAsync(&out.horizon_value, val.get() + j, sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemcpyAsync(out.horizon_point, L.xyz.get() + 3 * j, 3 * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemcpyAsync(&v, L.vox.get() + j, sizeof(long long), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        out.horizon_voxel = v;
        double t = out.horizon_t;               // locate_piece's rule
        int idx = 0;
        while (idx < N && t > hT[idx]) { t -= hT[idx]; idx++; }
        out.horizon_piece = idx == N ? N - 1 : idx;
    }
    if (rec[0] > 0) {
        const size_t j = (size_t)rec[6];
        long long v = -1;
        HIPCHK(c, hipMemcpyAsync(&out.min_clearance, val.get() + j, sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemcpyAsync(&v, L.vox.get() + j, sizeof(long long), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        out.min_voxel = v;
    }
    for (int i = 0; i < N; i++) out.duration += hT[i];
    out.culled = L.cull ? 1 : 0; out.margin = margin; out.far_r = L.far_r;
    float ms[3] = {0.f, 0.f, 0.f};
    for (int q = 0; q < 3; q++) HIPCHK(c, hipEventElapsedTime(&ms[q], ev[q], ev[q + 1]));
    out.select_ms = ms[0]; out.field_ms = ms[1]; out.reduce_ms = ms[2];
    if (info) *info = out;
    return ISDF_OK;
}

int horizon_ready(isdf_ctx *c, int N, const void *T, const void *coeffs, const isdf_traj_known_params *p, double *margin) {
    isdf_traj_check_params q;
    isdf_traj_check_params_default(&q);
    if (p) { q.margin = p->margin; q.mode = p->mode; }
    ISDF_TRY(check_args(c, N, T, coeffs, &q));
    if (!c) return fail(nullptr, ISDF_ERR_INVALID_ARG, "known horizon: null ctx");
    ISDF_TRY(check_state(c, &q, margin));
    if (!c->known.have) return fail(c, ISDF_ERR_STATE, "known horizon: no known grid (isdf_map_known_enable, then a map from isdf_set_pointcloud)");
    return ISDF_OK;
}

}  // namespace

extern "C" void isdf_traj_known_params_default(isdf_traj_known_params *p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->margin = -1.0;                       // negative: cfg.safety_hor of the ctx
    p->mode = ISDF_SWEPT_FIELD_PLANNER;
}

extern "C" int isdf_traj_known_horizon_device(isdf_ctx *c, int N, const double *d_T, const double *d_coeffs, const isdf_traj_known_params *p,
                                              isdf_traj_known_info *info_out, void *stream) {
    double margin = 0.0;
    ISDF_TRY(horizon_ready(c, N, d_T, d_coeffs, p, &margin));
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;
    std::vector<double> hT(N);
    HIPCHK(c, hipMemcpyAsync(hT.data(), d_T, N * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    ISDF_TRY(swept_check_traj(c, N, hT.data()));
    HIPCHK(c, hipStreamSynchronize(c->stream));         // the known grid is written on the ctx's stream
    return horizon_run(c, N, hT.data(), d_T, d_coeffs, p ? p->mode : ISDF_SWEPT_FIELD_PLANNER, margin, info_out, st);
}

extern "C" int isdf_traj_known_horizon(isdf_ctx *c, int N, const double *T, const double *coeffs, const isdf_traj_known_params *p, isdf_traj_known_info *info_out) {
    double margin = 0.0;
    ISDF_TRY(horizon_ready(c, N, T, coeffs, p, &margin));
    ISDF_TRY(swept_check_traj(c, N, T));
    for (int q = 0; q < 18 * N; q++) if (!std::isfinite(coeffs[q])) return fail(c, ISDF_ERR_INVALID_ARG, "known horizon: non-finite coefficient");
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf<double> traj;                    // own upload: the check's kept trajectory is not touched
    HIPCHK(c, traj.alloc((size_t)19 * N));
    hipStream_t st = c->stream;
    HIPCHK(c, hipMemcpyAsync(traj.get(), T, N * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(traj.get() + N, coeffs, (size_t)18 * N * sizeof(double), hipMemcpyHostToDevice, st));
    return horizon_run(c, N, T, traj.get(), traj.get() + N, p ? p->mode : ISDF_SWEPT_FIELD_PLANNER, margin, info_out, st);
}
