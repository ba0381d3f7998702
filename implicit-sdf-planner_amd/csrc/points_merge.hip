// The clearance report's voxels merged into the ctx's obstacle-point set on the device (isdf_points_merge_check): what the
// reference would have to do where plan_manager.cpp:306-309 only prints a warning - its point set (plan_manager.cpp:232-254) is
// keyed by voxel id (aabb_points, PCSmap_manager.h:182-216: unordered_map id -> centre), so a report row is new exactly when no
// point of the set lies in its voxel.
//
//   mark     one thread per point of the set: its voxel (getGridIndex, grid_index.hpp) -> a bit of a bitmap of nx ny nz bits
//            (cleared on the stream first); a point outside the grid occupies no voxel and is counted.
//   flag     one thread per kept row of the report: value < below and the bit of its voxel (the check kept the voxel index:
//            TrajCheckState::d_row_vox) -> one ballot mask and one count per 64 rows.
//   scan     exclusive sum of the counts (dev_scan.hpp).
//   append   (x, y, z) of the flagged rows, byte for byte, and lastTstar = 0 behind the old arrays, which move device to device
//            into the new allocations: old points keep index, bytes and lastTstar; new ones follow in ascending voxel index.
// The bitmap's content does not depend on the order of the ORs, the counters are integer sums and the rows are in voxel order: no
// atomic decides a position, and two merges from the same state give the same bytes.  Only four counters come back to the host.
#include "swept_field.hpp"
#include "dev_reduce.hpp"
#include "dev_scan.hpp"
#include "grid_index.hpp"
#include <climits>
#include <cmath>
#include <cstring>

namespace {

enum { CNT_ROWS = 0, CNT_ADDED = 1, CNT_DUP = 2, CNT_OUTSIDE = 3, CNT_WORDS = 4 };

__global__ __launch_bounds__(256) void pm_mark_kernel(DevGrid G, const double *__restrict__ pts, int M, unsigned *__restrict__ bits,
                                                      unsigned *__restrict__ counters) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned outside = 0;
    if (i < M) {
        int ix, iy, iz;
        if (grid_index(G, pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2], ix, iy, iz)) {
            const long long v = ((long long)ix * G.Y + iy) * G.Z + iz;
            atomicOr(&bits[v >> 5], 1u << (v & 31));
        } else outside = 1;
    }
    outside = wave_sum(outside);
    if ((threadIdx.x & 63) == 0 && outside) atomicAdd(&counters[CNT_OUTSIDE], outside);
}

// take_all: every kept row (a negative `below`)
__global__ __launch_bounds__(256) void pm_flag_kernel(long long n_rows, long long n_vox, const double *__restrict__ rows,
                                                      const long long *__restrict__ row_vox, const unsigned *__restrict__ bits, double below,
                                                      int take_all, unsigned long long *__restrict__ mask, int *__restrict__ count,
                                                      unsigned *__restrict__ counters) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    bool included = false, taken = false;
    if (j < n_rows) {
        included = take_all || rows[5 * j + 3] < below;
        const long long v = row_vox[j];
        taken = v >= 0 && v < n_vox && ((bits[v >> 5] >> (v & 31)) & 1u);
    }
    const unsigned long long m_inc = __ballot(included), m_add = __ballot(included && !taken);
    if ((threadIdx.x & 63) == 0 && (j >> 6) < (n_rows + 63) / 64) {
        mask[j >> 6] = m_add;
        count[j >> 6] = __popcll(m_add);
        const unsigned inc = (unsigned)__popcll(m_inc), add = (unsigned)__popcll(m_add);
        if (inc) atomicAdd(&counters[CNT_ROWS], inc);
        if (add) atomicAdd(&counters[CNT_ADDED], add);
        if (inc - add) atomicAdd(&counters[CNT_DUP], inc - add);
    }
}

__global__ __launch_bounds__(256) void pm_append_kernel(long long n_rows, const double *__restrict__ rows, const unsigned long long *__restrict__ mask,
                                                        const int *__restrict__ base, int M_before, double *__restrict__ pts,
                                                        double *__restrict__ tstar) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_rows) return;
    const unsigned long long m = mask[j >> 6];
    const int lane = (int)(j & 63);
    if (!((m >> lane) & 1ull)) return;
    const size_t pos = (size_t)M_before + (size_t)base[j >> 6] + (size_t)__popcll(m & ((1ull << lane) - 1ull));
    pts[3 * pos] = rows[5 * j]; pts[3 * pos + 1] = rows[5 * j + 1]; pts[3 * pos + 2] = rows[5 * j + 2];
    tstar[pos] = 0.0;                       // lastTstar of a fresh point (plan_manager.cpp:254)
}

}  // namespace

extern "C" int isdf_points_merge_check(isdf_ctx *c, double below, isdf_points_merge_info *info_out) {
    // the argument is checked before the ctx (reported through isdf_last_error(NULL) when there is none)
    if (!std::isfinite(below)) return isdf_fail(c, ISDF_ERR_INVALID_ARG, "points merge: below must be finite");
    if (!c) return isdf_fail(nullptr, ISDF_ERR_INVALID_ARG, "points merge: null ctx");
    if (!c->peers.empty() || c->is_peer || c->rccl_comm) return isdf_fail(c, ISDF_ERR_UNSUPPORTED, "points merge on a multi-device ctx");
    TrajCheckState *k = c->tck.get();
    if (!k || !k->have) return isdf_fail(c, ISDF_ERR_STATE, "points merge: no kept clearance report (isdf_traj_check)");
    if (k->grid_epoch != c->grid_epoch || !c->have_geom)
        return isdf_fail(c, ISDF_ERR_STATE, "points merge: the kept clearance report is older than the occupancy grid (check again)");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const DevGrid &G = c->grid;
    const long long n_vox = (long long)G.X * G.Y * G.Z, n_rows = k->n_rows;
    const size_t n_words = (size_t)((n_vox + 31) / 32), n_waves = (size_t)((n_rows + 63) / 64);
    const int M_before = c->M;
    unsigned cnt[CNT_WORDS] = {0, 0, 0, 0};
    float ms = 0.f;
    if (n_rows > 0 || M_before > 0) {
        DevBuf<unsigned long long> mask;
        DevBuf<int> count, base;
        DevEvents<2> ev;
        ISDF_TRY(ev.ready(c));
        ISDF_TRY(c->d_merge_bits.reserve(c, n_words));
        DevBuf<unsigned> counters;
        HIPCHK(c, counters.alloc(CNT_WORDS));
        HIPCHK(c, mask.alloc(n_waves)); HIPCHK(c, count.alloc(n_waves)); HIPCHK(c, base.alloc(n_waves));
        HIPCHK(c, hipEventRecord(ev[0], st));
        HIPCHK(c, hipMemsetAsync(c->d_merge_bits, 0, n_words * sizeof(unsigned), st));
        HIPCHK(c, hipMemsetAsync(counters.get(), 0, CNT_WORDS * sizeof(unsigned), st));
        if (M_before > 0)
            hipLaunchKernelGGL(pm_mark_kernel, dim3(blocks(M_before)), dim3(256), 0, st, G, (const double *)c->d_points.get(), M_before,
                               c->d_merge_bits.get(), counters.get());
        if (n_rows > 0)
            hipLaunchKernelGGL(pm_flag_kernel, dim3(blocks(n_rows)), dim3(256), 0, st, n_rows, n_vox, (const double *)k->d_rows.get(),
                               (const long long *)k->d_row_vox.get(), (const unsigned *)c->d_merge_bits.get(), below, below < 0.0 ? 1 : 0,
                               mask.get(), count.get(), counters.get());
        HIPCHK(c, hipGetLastError());
        DevBuf<unsigned char> tmp;          // (freed behind the scan)
        if (n_rows > 0) { ISDF_TRY(exclusive_sum(c, tmp, count.get(), base.get(), (long long)n_waves, st)); tmp.release(); }
        HIPCHK(c, hipMemcpyAsync(cnt, counters.get(), sizeof(cnt), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        if ((long long)M_before + (long long)cnt[CNT_ADDED] > (long long)INT32_MAX)
            return isdf_fail(c, ISDF_ERR_OVERFLOW, "points merge: more than 2^31 obstacle points");
        if (cnt[CNT_ADDED] > 0) {
            const int M_after = M_before + (int)cnt[CNT_ADDED];
            DevBuf<double> pts, tstar;
            HIPCHK(c, pts.alloc((size_t)3 * M_after)); HIPCHK(c, tstar.alloc((size_t)M_after));
            if (M_before > 0) {
                HIPCHK(c, hipMemcpyAsync(pts.get(), c->d_points.get(), (size_t)3 * M_before * sizeof(double), hipMemcpyDeviceToDevice, st));
                HIPCHK(c, hipMemcpyAsync(tstar.get(), c->d_tstar.get(), (size_t)M_before * sizeof(double), hipMemcpyDeviceToDevice, st));
            }
            hipLaunchKernelGGL(pm_append_kernel, dim3(blocks(n_rows)), dim3(256), 0, st, n_rows, (const double *)k->d_rows.get(),
                               (const unsigned long long *)mask.get(), (const int *)base.get(), M_before, pts.get(), tstar.get());
            HIPCHK(c, hipGetLastError());
            // the V1 words as isdf_set_points leaves them; every per-M buffer grows at the next step, which sizes them by ctx->M
            if (c->v1.words) HIPCHK(c, hipMemsetAsync(c->v1.words, 0, 8 * sizeof(unsigned), st));
            HIPCHK(c, hipEventRecord(ev[1], st));
            HIPCHK(c, hipStreamSynchronize(st));
            c->d_points = std::move(pts);
            c->d_tstar = std::move(tstar);
            c->M = M_after;
            c->points_epoch++;
        } else {
            HIPCHK(c, hipEventRecord(ev[1], st));
            HIPCHK(c, hipStreamSynchronize(st));
        }
        HIPCHK(c, hipEventElapsedTime(&ms, ev[0], ev[1]));
    }
    if (info_out) {
        std::memset(info_out, 0, sizeof(*info_out));
        info_out->M_before = M_before; info_out->M_after = c->M;
        info_out->n_rows = (int32_t)cnt[CNT_ROWS]; info_out->n_added = (int32_t)cnt[CNT_ADDED];
        info_out->n_duplicate = (int32_t)cnt[CNT_DUP]; info_out->n_outside = (int32_t)cnt[CNT_OUTSIDE];
        info_out->merge_ms = ms;
    }
    return ISDF_OK;
}
