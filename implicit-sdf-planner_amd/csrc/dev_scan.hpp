// The device-wide exclusive scan (host-only; the one place that names hipcub's) and the workgroup count of a one-lane-per-entry launch.
#pragma once
#include "isdf_ctx.hpp"
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <climits>

inline unsigned blocks(long long n, int b = 256) { return (unsigned)((n + b - 1) / b); }

// The scan's two halves, for a caller that records an event between them or scans twice: what can allocate (the size query, scratch
// grown to it), then the launch alone.  *bytes goes from the one to the other; it depends on n and the two types, not on the pointers.
template <typename In, typename Out> int exclusive_sum_reserve(isdf_ctx *c, DevBuf<unsigned char> &scratch, In in, Out out, long long n, hipStream_t st, size_t *bytes) {
    if (n > (long long)INT_MAX) return isdf_fail(c, ISDF_ERR_OVERFLOW, "exclusive scan: more than 2^31 - 1 entries");
    *bytes = 0;
    HIPCHK(c, hipcub::DeviceScan::ExclusiveSum(nullptr, *bytes, in, out, (int)n, st));
    return scratch.reserve(c, std::max<size_t>(*bytes, 1));
}
template <typename In, typename Out> int exclusive_sum_run(isdf_ctx *c, const DevBuf<unsigned char> &scratch, size_t bytes, In in, Out out, long long n, hipStream_t st) {
    HIPCHK(c, hipcub::DeviceScan::ExclusiveSum(scratch.get(), bytes, in, out, (int)n, st));
    return ISDF_OK;
}

// out[i] = in[0] + ... + in[i - 1] on `st`.  scratch: a state's grow-only buffer, or a local one, allocated here and freed by the caller.
template <typename In, typename Out> int exclusive_sum(isdf_ctx *c, DevBuf<unsigned char> &scratch, In in, Out out, long long n, hipStream_t st) {
    size_t bytes;
    ISDF_TRY(exclusive_sum_reserve(c, scratch, in, out, n, st, &bytes));
    return exclusive_sum_run(c, scratch, bytes, in, out, n, st);
}
