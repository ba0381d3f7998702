// The integer reductions inside a kernel (device-only): over the wavefront by one 64-lane __shfl_down ladder, over the
// workgroup through the wavefronts and a few LDS words.  Integers only: the double-precision reductions stay with their kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

namespace isdf {

// wave_sum / wave_min / wave_max: called by EVERY lane of a wavefront.  Afterwards LANE 0, AND ONLY LANE 0, holds the wavefront's
// result; what the other lanes hold is a partial result of no use.  (dev_math.hpp's wave_sum(double) is another function: every lane.)
template <typename T, typename Op> __device__ __forceinline__ T wave_reduce(T v, Op op) {
    static_assert(std::is_integral<T>::value, "the integer ladder: doubles go through dev_math.hpp");
    for (int off = 32; off > 0; off >>= 1) v = op(v, __shfl_down(v, off, 64));
    return v;
}
template <typename T> __device__ __forceinline__ T wave_sum(T v) { return wave_reduce(v, [](T a, T b) { return a + b; }); }
template <typename T> __device__ __forceinline__ T wave_min(T v) { return wave_reduce(v, [](T a, T b) { return b < a ? b : a; }); }
template <typename T> __device__ __forceinline__ T wave_max(T v) { return wave_reduce(v, [](T a, T b) { return b > a ? b : a; }); }

// Called by EVERY thread of a workgroup of WAVES wavefronts, or by none (it holds the workgroup's one barrier): afterwards thread
// k < COUNTERS holds the workgroup's total of cnt[k]; the other threads hold 0.
template <int COUNTERS, int WAVES, typename T> __device__ __forceinline__ unsigned long long block_sum(const T (&cnt)[COUNTERS]) {
    __shared__ unsigned long long s_sum[WAVES][COUNTERS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int k = 0; k < COUNTERS; k++) {
        unsigned long long s = (unsigned long long)cnt[k];
        for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);       // (wave_sum, in place: the queries' kernels compile to what they were)
        if (lane == 0) s_sum[wave][k] = s;
    }
    __syncthreads();
    unsigned long long s = 0;
    if (threadIdx.x < COUNTERS)
        for (int w = 0; w < WAVES; w++) s += s_sum[w][threadIdx.x];
    return s;
}

// Called by EVERY thread of a workgroup of WAVES wavefronts, or by none: afterwards every thread holds the workgroup's largest v.  The
// barrier behind the read lets a loop call it again.  AGAIN = false leaves that barrier out, for a caller that calls it once.
template <int WAVES, bool AGAIN = true> __device__ __forceinline__ unsigned long long block_max(unsigned long long v) {
    __shared__ unsigned long long s_max[WAVES];
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = v;
    __syncthreads();
    v = s_max[0];
    for (int w = 1; w < WAVES; w++) v = s_max[w] > v ? s_max[w] : v;
    if (AGAIN) __syncthreads();         // (s_max is written again by the next call)
    return v;
}

// A box over the workgroup, in six LDS words.  open: every thread of the workgroup (it holds a barrier); add: any thread with a box that
// holds something; flush: thread 0, behind a barrier that follows every add - six global atomics where any thread added, none else.
struct BoxAcc {
    int *lo, *hi;
    __device__ __forceinline__ static BoxAcc open() {
        __shared__ int s_lo[3], s_hi[3];
        if (threadIdx.x < 3) { s_lo[threadIdx.x] = 0x7FFFFFFF; s_hi[threadIdx.x] = -1; }
        __syncthreads();
        return BoxAcc{s_lo, s_hi};
    }
    __device__ __forceinline__ void add(const int l[3], const int h[3]) const {
        atomicMin(&lo[0], l[0]); atomicMin(&lo[1], l[1]); atomicMin(&lo[2], l[2]);
        atomicMax(&hi[0], h[0]); atomicMax(&hi[1], h[1]); atomicMax(&hi[2], h[2]);
    }
    __device__ __forceinline__ void flush(int *g_lo, int *g_hi) const {
        if (hi[0] < 0) return;
        atomicMin(&g_lo[0], lo[0]); atomicMin(&g_lo[1], lo[1]); atomicMin(&g_lo[2], lo[2]);
        atomicMax(&g_hi[0], hi[0]); atomicMax(&g_hi[1], hi[1]); atomicMax(&g_hi[2], hi[2]);
    }
};

}  // namespace isdf
