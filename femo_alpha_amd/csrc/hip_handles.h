// Move-only owners of the HIP runtime resources a context holds (host code only).  Each releases what it holds when it is
// destroyed, reset, re-allocated or moved over; the implicit conversions let launches and pointer arithmetic use them as before.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

namespace femo {

// n elements of T from hipMalloc (Pinned: from hipHostMalloc)
template <class T, bool Pinned>
class Buf {
public:
    Buf() = default;
    Buf(Buf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
    Buf& operator=(Buf&& o) noexcept {
        if (this != &o) { reset(); p_ = std::exchange(o.p_, nullptr); n_ = std::exchange(o.n_, 0); }
        return *this;
    }
    ~Buf() { reset(); }
    // frees what the buffer held, then allocates exactly n elements
    hipError_t alloc(size_t n) {
        reset();
        void* p = nullptr;
        const hipError_t e = Pinned ? hipHostMalloc(&p, n * sizeof(T)) : hipMalloc(&p, n * sizeof(T));
        if (e == hipSuccess) { p_ = static_cast<T*>(p); n_ = n; }
        return e;
    }
    // keeps the buffer when it already holds at least n elements
    hipError_t grow(size_t n) { return n <= n_ ? hipSuccess : alloc(n); }
    void reset() {
        if (p_) { if (Pinned) (void)hipHostFree(p_); else (void)hipFree(p_); }
        p_ = nullptr; n_ = 0;
    }
    T* get() const { return p_; }
    size_t size() const { return n_; }
    operator T*() const { return p_; }

private:
    T* p_ = nullptr;
    size_t n_ = 0;
};
template <class T> using DevBuf = Buf<T, false>;
template <class T> using PinnedBuf = Buf<T, true>;

// a stream, event or graph; created at its call site through out(), which releases the old handle first
template <class H, hipError_t (*Release)(H)>
class Handle {
public:
    Handle() = default;
    Handle(Handle&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
    Handle& operator=(Handle&& o) noexcept {
        if (this != &o) { reset(); h_ = std::exchange(o.h_, nullptr); }
        return *this;
    }
    ~Handle() { reset(); }
    H* out() { reset(); return &h_; }
    void reset() {
        if (h_) (void)Release(h_);
        h_ = nullptr;
    }
    H get() const { return h_; }
    operator H() const { return h_; }

private:
    H h_ = nullptr;
};
using Stream = Handle<hipStream_t, hipStreamDestroy>;
using Event = Handle<hipEvent_t, hipEventDestroy>;
using GraphExec = Handle<hipGraphExec_t, hipGraphExecDestroy>;
using Graph = Handle<hipGraph_t, hipGraphDestroy>;

}  // namespace femo
