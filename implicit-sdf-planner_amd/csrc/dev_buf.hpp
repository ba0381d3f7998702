// Owning buffers of the host code (host-only): device memory (DevBuf) and pinned, device-mapped host memory (PinBuf).
// Both free themselves, neither copies.  As a ctx member a buffer grows only (reserve); as a local it is a scoped temporary
// that is gone on every return.  Every allocation and every free of the two types goes through mem_take / mem_give, which
// keep the process-wide count of live bytes behind isdf_debug_live_bytes.  Events (DevEvents) are owned and counted the same way
// (event_take / event_give, isdf_debug_live_events); RecPair is a counted call's record: one Rec on the device and its pinned copy.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstddef>
#include <cstring>
#include <type_traits>
#include <utility>

struct isdf_ctx;
int isdf_hip_fail(isdf_ctx *c, const char *what, hipError_t e);     // isdf_host.hip: "<what>: <HIP's message>" into the ctx, returns ISDF_ERR_HIP

namespace isdf {
inline std::atomic<long long> g_live_bytes[2];      // [0] device, [1] pinned

inline hipError_t mem_take(void **p, size_t bytes, bool pinned) {
    *p = nullptr;
    const hipError_t e = pinned ? hipHostMalloc(p, bytes, hipHostMallocDefault) : hipMalloc(p, bytes);
    if (e != hipSuccess) { *p = nullptr; return e; }
    g_live_bytes[pinned ? 1 : 0].fetch_add((long long)bytes, std::memory_order_relaxed);
    return hipSuccess;
}
inline void mem_give(void *p, size_t bytes, bool pinned) {
    if (!p) return;
    (void)(pinned ? hipHostFree(p) : hipFree(p));
    g_live_bytes[pinned ? 1 : 0].fetch_sub((long long)bytes, std::memory_order_relaxed);
}

constexpr int NO_FILL = -1;

// Device memory: pointer + capacity in elements (DevBuf<void>: in bytes).
template <typename T> class DevBuf {
    using Elem = std::conditional_t<std::is_void<T>::value, unsigned char, T>;
    T *p_ = nullptr;
    size_t cap_ = 0;
    __attribute__((noinline)) int grow(isdf_ctx *c, size_t n, int fill) {
        const hipError_t e = alloc(n, fill);
        return e == hipSuccess ? 0 : isdf_hip_fail(c, "device buffer", e);
    }
public:
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept { swap(o); }
    DevBuf &operator=(DevBuf &&o) noexcept { if (this != &o) { release(); swap(o); } return *this; }
    ~DevBuf() { release(); }
    T *get() const { return p_; }
    operator T *() const { return p_; }
    size_t capacity() const { return cap_; }
    void release() { mem_give(p_, cap_ * sizeof(Elem), false); p_ = nullptr; cap_ = 0; }
    void swap(DevBuf &o) { std::swap(p_, o.p_); std::swap(cap_, o.cap_); }
    // drops what it holds, then exactly n elements (one where n is 0), every byte `fill` when one is given; on failure empty
    hipError_t alloc(size_t n, int fill = NO_FILL) {
        release();
        if (n == 0) n = 1;
        hipError_t e = mem_take((void **)&p_, n * sizeof(Elem), false);
        if (e != hipSuccess) return e;
        cap_ = n;
        if (fill != NO_FILL && (e = hipMemset(p_, fill, n * sizeof(Elem))) != hipSuccess) release();
        return e;
    }
    // grow-only, contents not preserved; the per-step path is the compare
    int reserve(isdf_ctx *c, size_t n, int fill = NO_FILL) { return n <= cap_ ? 0 : grow(c, n, fill); }
    // a fresh buffer of exactly n elements whatever it held (once-per-plan state)
    int renew(isdf_ctx *c, size_t n, int fill = NO_FILL) { return grow(c, n, fill); }
};

// Pinned host memory with the address the devices see it at; zero-filled when allocated.
template <typename T> class PinBuf {
    T *p_ = nullptr, *dev_ = nullptr;
    size_t cap_ = 0;
    __attribute__((noinline)) int grow(isdf_ctx *c, size_t n) {
        release();
        hipError_t e = mem_take((void **)&p_, n * sizeof(T), true);
        if (e != hipSuccess) return isdf_hip_fail(c, "pinned buffer", e);
        cap_ = n;
        if ((e = hipHostGetDevicePointer((void **)&dev_, p_, 0)) != hipSuccess) { release(); return isdf_hip_fail(c, "pinned buffer's device address", e); }
        std::memset((void *)p_, 0, n * sizeof(T));
        return 0;
    }
public:
    PinBuf() = default;
    PinBuf(const PinBuf &) = delete;
    PinBuf &operator=(const PinBuf &) = delete;
    PinBuf(PinBuf &&o) noexcept { std::swap(p_, o.p_); std::swap(dev_, o.dev_); std::swap(cap_, o.cap_); }
    PinBuf &operator=(PinBuf &&o) noexcept { if (this != &o) { release(); std::swap(p_, o.p_); std::swap(dev_, o.dev_); std::swap(cap_, o.cap_); } return *this; }
    ~PinBuf() { release(); }
    T *get() const { return p_; }
    operator T *() const { return p_; }
    T *dev() const { return dev_; }
    size_t capacity() const { return cap_; }
    void release() { mem_give(p_, cap_ * sizeof(T), true); p_ = dev_ = nullptr; cap_ = 0; }
    int reserve(isdf_ctx *c, size_t n) { return n <= cap_ ? 0 : grow(c, n); }
};

inline std::atomic<long long> g_live_events;

inline hipError_t event_take(hipEvent_t *e, unsigned flags) {
    *e = nullptr;
    const hipError_t r = hipEventCreateWithFlags(e, flags);
    if (r != hipSuccess) { *e = nullptr; return r; }
    g_live_events.fetch_add(1, std::memory_order_relaxed);
    return hipSuccess;
}
inline void event_give(hipEvent_t e) {
    if (!e) return;
    (void)hipEventDestroy(e);
    g_live_events.fetch_sub(1, std::memory_order_relaxed);
}

// N events: a ctx member keeps them from its first ready() on, a local is gone on every return.
template <int N> class DevEvents {
    hipEvent_t e_[N] = {};
public:
    DevEvents() = default;
    DevEvents(const DevEvents &) = delete;
    DevEvents &operator=(const DevEvents &) = delete;
    DevEvents(DevEvents &&o) noexcept { for (int k = 0; k < N; k++) std::swap(e_[k], o.e_[k]); }
    ~DevEvents() { release(); }
    hipEvent_t operator[](int k) const { return e_[k]; }
    const hipEvent_t *get() const { return e_; }
    void release() { for (hipEvent_t &e : e_) { event_give(e); e = nullptr; } }
    // creates the missing ones
    int ready(isdf_ctx *c, unsigned flags = hipEventDefault) {
        for (hipEvent_t &e : e_)
            if (!e) { const hipError_t r = event_take(&e, flags); if (r != hipSuccess) return isdf_hip_fail(c, "hipEventCreate", r); }
        return 0;
    }
    // device time from event a to event b; 0.0 where HIP refuses (an event never recorded)
    double ms(int a, int b) const {
        float v = 0.f;
        return hipEventElapsedTime(&v, e_[a], e_[b]) == hipSuccess ? (double)v : 0.0;
    }
};

// A counted call's record (n Recs where its length depends on the call).  The call empties it on its stream (zero: every byte 0; put:
// this value, through the pinned copy), its kernels count into dev(), fetch queues the copy back, and after the call's synchronisation
// host() is the record as the kernels left it.
template <typename Rec> class RecPair {
    DevBuf<Rec> d_;
    PinBuf<Rec> h_;
    size_t n_ = 1;
public:
    int ready(isdf_ctx *c, size_t n = 1) { n_ = n; const int rc = d_.reserve(c, n); return rc ? rc : h_.reserve(c, n); }
    void release() { d_.release(); h_.release(); }
    Rec *dev() const { return d_; }
    Rec &host() const { return *h_.get(); }
    hipError_t zero(hipStream_t st) { return hipMemsetAsync(d_, 0, n_ * sizeof(Rec), st); }
    hipError_t put(const Rec &v, hipStream_t st) { host() = v; return hipMemcpyAsync(d_, h_.get(), sizeof(Rec), hipMemcpyHostToDevice, st); }
    hipError_t fetch(hipStream_t st) { return hipMemcpyAsync(h_.get(), d_, n_ * sizeof(Rec), hipMemcpyDeviceToHost, st); }
};
}  // namespace isdf
