// What the users of the swept-volume field query share (swept_mesh.hip: the query and the mesher; traj_check.hip: the clearance
// check; traj_watch.hip: the check's kept report folded across map updates): the query's scratch, its host-side checks and
// launches, and the check's selection test, reduction and kept state.  (The count / scan / emit passes' host helpers: dev_scan.hpp.)
#pragma once
#include "isdf_ctx.hpp"
#include "traj_watch_host.hpp"
#include <vector>

constexpr int FIELD_CHUNK = 65536;                        // points per field launch: 65 536 x 1.5 KB of interval slots = 96 MiB
constexpr double MAX_DURATION = 300.0;                    // the reference's stale-duration rule (sw_manager.hpp:287-296)

// scratch of the field query and the last mesh (never shared with the optimizer step's state)
struct SweptMeshState {
    // field: FIELD_CHUNK points of scratch, the statistics words and the overflow word as the host reads it
    SweptScratch field;
    DevBuf<unsigned long long> d_stats;
    PinBuf<unsigned long long> h_overflow;
    // mesh build inputs (T | coeffs) and the last mesh
    DevBuf<double> d_traj;
    DevBuf<double> d_V; DevBuf<int32_t> d_F;
    long long nV = 0, nF = 0;
    bool have_mesh = false;
};

// ---- the clearance check's selection, shared by the whole-map row kernel (traj_check.hip) and the new-voxel list kernel (traj_watch.hip)
struct SelBox {
    int X, Y, Z;                 // grid
    double res, bmin[3];
    int lo[3], hi[3];            // voxel box, inclusive
    int b0[3], nb[3];            // first brick of the box per axis, bricks per axis
    int n_chunks;                // 64-voxel chunks of a z-row of the box
    int cull;                    // 0: every occupied voxel of the box is a candidate
    double far2;                 // (far_r)^2, slightly enlarged: the single-voxel test
    double bfar2;                // (far_r + brick half-diagonal)^2: the brick test
};

// a voxel's centre as numpy forms it, (index + 0.5) * res + origin with both operations rounded (no contraction into an fma)
__device__ __forceinline__ double voxel_centre(int i, double res, double origin) {
#pragma clang fp contract(off)
    const double m = ((double)i + 0.5) * res;
    return m + origin;
}

// the coarse positions into LDS as [x | y | z] (pose table: component-major, SWEPT_MAX_COARSE rows)
__device__ __forceinline__ void stage_samples(const double *pose, int n, double *s_pos) {
    for (int k = threadIdx.x; k < 3 * n; k += blockDim.x) {
        const int a = k / n, i = k - a * n;
        s_pos[a * SWEPT_MAX_COARSE + i] = pose[(size_t)a * SWEPT_MAX_COARSE + i];
    }
    __syncthreads();
}

// the single-voxel test: coarse sample k of the staged positions lies within far_r of the voxel centre (px, py, pz).  One function
// for both kernels, so that both round the distance the same way.
__device__ __forceinline__ bool sample_within(double px, double py, double pz, const double *s_pos, int k, double far2) {
    const double dx = px - s_pos[k], dy = py - s_pos[SWEPT_MAX_COARSE + k], dz = pz - s_pos[2 * SWEPT_MAX_COARSE + k];
    return !(dx * dx + dy * dy + dz * dz > far2);
}

// scratch of the check's reduction over a candidate list (grows only where a state keeps it; a local one is a scoped temporary)
constexpr int TC_REPORT_WORDS = 7;      // [0] min value [1] its t* [2..4] its point [5] voxel (as int64 bits) [6] piece (as int64 bits)
struct TcReduceScratch {
    DevBuf<int> flag, fbase;
    DevBuf<unsigned long long> key;
    DevBuf<void> partial;
    DevBuf<unsigned char> scan_tmp;
};

// a watch on the kept report (isdf_traj_check_set_watch, mode 1): what the arming check leaves for the folds, the folded report,
// the last fold's record and the fold's own scratch (grow only: nothing is allocated after the first fold of a size)
struct TrajWatchState {
    bool armed = false;
    int N = 0, mode = 0;
    double margin = 0.0;
    DevBuf<double> d_traj;              // T | coeffs | N piece minima of a whole-map re-check
    isdf_traj_check_info info{};
    std::vector<double> piece_min;
    SelBox box{}; bool box_empty = true;        // the arming check's selection box (a function of trajectory, far_r and grid geometry)
    isdf_traj_watch_info last{};
    DevBuf<long long> d_key, d_vox, d_new_row_vox, d_row_vox_out;
    DevBuf<double> d_xyz, d_val, d_ts, d_new_rows, d_rows_out;
    DevBuf<void> d_sort_tmp;
    TcReduceScratch red;
    RecPair<unsigned long long> rec;        // the hand-over record's words (traj_watch.hip)
    DevEvents<5> ev;
};

// the last clearance check's violating points (kept like the swept mesh is) and the host form's trajectory upload (traj_check.hip);
// points_merge.hip reads the rows
struct TrajCheckState {
    DevBuf<double> d_traj;
    DevBuf<double> d_rows;          // n_rows x (x, y, z, value, t*)
    DevBuf<long long> d_row_vox;    // n_rows voxel indices (x * ny + y) * nz + z, ascending
    long long n_rows = 0;
    unsigned long long grid_epoch = 0;      // the ctx's grid_epoch the check ran on
    bool have = false;
    TrajWatchState w;
};

// traj_check.hip, for the fold.  The reduction's launches on `st`, nothing copied or synchronised: d_counts[0..2] (zeroed here) +=
// qualified, below the margin, penetrating; d_report: TC_REPORT_WORDS doubles; d_piece_min: N doubles; S.flag marks the rows
int tc_reduce_launch(isdf_ctx *c, TcReduceScratch &S, long long n, const double *d_val, const double *d_ts, const long long *d_vox, const double *d_xyz,
                     const double *d_T, int N, double margin, unsigned long long *d_counts, double *d_report, double *d_piece_min, hipStream_t st);
// ... and the flagged candidates compacted in list order into d_rows (x, y, z, value, t*) / d_row_vox
int tc_rows_launch(isdf_ctx *c, TcReduceScratch &S, long long n, const double *d_val, const double *d_ts, const long long *d_vox, const double *d_xyz,
                   double *d_rows, long long *d_row_vox, hipStream_t st);
// the whole check again on the watch's kept trajectory, margin and mode (re-arms the watch)
int traj_check_rerun_kept(isdf_ctx *c, isdf_traj_check_info *info);
void traj_check_drop_report(isdf_ctx *c);           // the kept rows freed, the watch disarmed
// traj_watch.hip
// (traj_watch_disarm: isdf_ctx.hpp)
bool traj_watch_armed(isdf_ctx *c);                 // mode 1, a watch armed on the grid the ctx holds now
// the map update's call once its products are in place: d_list = the update's new-voxel list (MuVoxel), complete when n_new <= cap
int traj_watch_fold(isdf_ctx *c, const void *d_list, unsigned n_new, unsigned cap);

// swept_mesh.hip
int swept_field_scratch(isdf_ctx *c, SweptMeshState **out);          // allocates the query's scratch on first use
int swept_check_traj(isdf_ctx *c, int N, const double *T);           // durations finite and > 0, total below 300 s
int swept_check_ctx(isdf_ctx *c);                                    // single-device ctx with a shape
int swept_field_coarse_table(isdf_ctx *c, int N, const double *d_T, const double *d_coeffs, int mode, hipStream_t st);
int swept_field_run(isdf_ctx *c, int N, const double *d_T, const double *d_coeffs, const double *d_xyz, long long n, int mode,
                    double *d_value, double *d_tstar, hipStream_t st);
// the same launches without the read-back: the caller fetches the overflow word (SweptMeshState::d_stats[4]) with its own hand-over
int swept_field_launch(isdf_ctx *c, int N, const double *d_T, const double *d_coeffs, const double *d_xyz, long long n, int mode,
                       double *d_value, double *d_tstar, hipStream_t st);
