// The slot of a state the ctx creates on first use (host-only, and no HIP: tests/native/ctx_state_sanitize_main.cpp builds it with a
// plain compiler).  isdf_ctx.hpp declares Lazy<S> members with S incomplete; make() runs in the translation unit that defines S and
// captures the deleter there, so reset() and the destructor need no more than the pointer.  The ctx's destructor names no state: the
// slots drop what they hold, in reverse order of declaration.
#pragma once
#include <new>

struct isdf_ctx;
int isdf_fail(isdf_ctx *c, int code, const char *msg);      // records the message, returns code

namespace isdf {
constexpr int LAZY_NO_MEMORY = -3;      // ISDF_ERR_HIP (include/isdf_accel.h), as isdf_create reports it

template <typename S> class Lazy {
    S *p_ = nullptr;
    void (*drop_)(S *) = nullptr;
public:
    Lazy() = default;
    Lazy(const Lazy &) = delete;
    Lazy &operator=(const Lazy &) = delete;
    ~Lazy() { reset(); }
    S *get() const { return p_; }
    S *operator->() const { return p_; }
    explicit operator bool() const { return p_ != nullptr; }
    void reset() { if (p_) drop_(p_); p_ = nullptr; }
    // the state, created on first use
    int make(isdf_ctx *c, S **out) {
        if (!p_) {
            if (!(p_ = new (std::nothrow) S())) return isdf_fail(c, LAZY_NO_MEMORY, "out of host memory");
            drop_ = [](S *s) { delete s; };
        }
        *out = p_;
        return 0;
    }
};
}  // namespace isdf
