// The counters' hand-over inside a kernel (device-only): a few per-lane counters summed over the wavefront, the wavefronts summed
// through LDS.  The map's queries (map_raycast.hip, depth_cam.hip, view_gain.hip) end their kernels with it and then add the totals to
// their own record with one atomic per word per workgroup.
#pragma once
#include <hip/hip_runtime.h>

namespace isdf {

// Called by EVERY thread of a workgroup of WAVES wavefronts, or by none (it holds the workgroup's one barrier): afterwards thread
// k < COUNTERS holds the workgroup's total of cnt[k]; the other threads hold 0.
template <int COUNTERS, int WAVES, typename T> __device__ __forceinline__ unsigned long long block_sum(const T (&cnt)[COUNTERS]) {
    __shared__ unsigned long long s_sum[WAVES][COUNTERS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int k = 0; k < COUNTERS; k++) {
        unsigned long long s = (unsigned long long)cnt[k];
        for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
        if (lane == 0) s_sum[wave][k] = s;          // lane 0 holds the wavefront's sum
    }
    __syncthreads();
    unsigned long long s = 0;
    if (threadIdx.x < COUNTERS)
        for (int w = 0; w < WAVES; w++) s += s_sum[w][threadIdx.x];
    return s;
}

}  // namespace isdf
