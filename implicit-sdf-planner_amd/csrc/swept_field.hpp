// What the users of the swept-volume field query share (swept_mesh.hip: the query and the mesher; traj_check.hip: the clearance
// check): the query's scratch, its host-side checks and launches, and the small host helpers of the count / scan / emit passes.
#pragma once
#include "isdf_ctx.hpp"
#include <hipcub/hipcub.hpp>

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

// the last clearance check's violating points (kept like the swept mesh is) and the host form's trajectory upload (traj_check.hip);
// points_merge.hip reads the rows
struct TrajCheckState {
    DevBuf<double> d_traj;
    DevBuf<double> d_rows;          // n_rows x (x, y, z, value, t*)
    DevBuf<long long> d_row_vox;    // n_rows voxel indices (x * ny + y) * nz + z, ascending
    long long n_rows = 0;
    unsigned long long grid_epoch = 0;      // the ctx's grid_epoch the check ran on
    bool have = false;
};

// swept_mesh.hip
int swept_field_scratch(isdf_ctx *c, SweptMeshState **out);          // allocates the query's scratch on first use
int swept_check_traj(isdf_ctx *c, int N, const double *T);           // durations finite and > 0, total below 300 s
int swept_check_ctx(isdf_ctx *c);                                    // single-device ctx with a shape
int swept_field_coarse_table(isdf_ctx *c, int N, const double *d_T, const double *d_coeffs, int mode, hipStream_t st);
int swept_field_run(isdf_ctx *c, int N, const double *d_T, const double *d_coeffs, const double *d_xyz, long long n, int mode,
                    double *d_value, double *d_tstar, hipStream_t st);

inline unsigned blocks(long long n, int b = 256) { return (unsigned)((n + b - 1) / b); }

template <typename In, typename Out> int exclusive_sum(isdf_ctx *c, In in, Out out, long long n, hipStream_t st) {
    size_t bytes = 0;
    HIPCHK(c, hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, in, out, (int)n, st));
    DevBuf<unsigned char> tmp;
    HIPCHK(c, tmp.alloc(bytes));
    HIPCHK(c, hipcub::DeviceScan::ExclusiveSum(tmp.get(), bytes, in, out, (int)n, st));
    return ISDF_OK;
}
