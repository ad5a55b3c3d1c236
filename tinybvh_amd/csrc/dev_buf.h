// dev_buf.h — DevBuf<T>: the one owner of device memory behind the C ABI (capi_*.hip).  A move-only handle on ONE hipMalloc allocation of
// count() elements of T (DevBuf<void>: of bytes), released by reset() or the destructor.  It reports hipError_t and never sets the library's
// error text: every call site decides the code and the message.  No allocator policy, no pooling, no copy helpers.
// ScratchCarver: how the device builders (kernels_*build.hip) divide one such allocation into their arrays.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <cstdint>

namespace tbvh_capi {

// what tbvh_debug_device_allocations reports: allocations DevBufs of this process hold right now, and their bytes
inline std::atomic<uint64_t> g_devBufLive{0}, g_devBufBytes{0};

template <class T> constexpr size_t kDevBufElem = sizeof(T);
template <> inline constexpr size_t kDevBufElem<void> = 1;

template <class T>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { reset(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; }
        return *this;
    }
    ~DevBuf() { reset(); }

    // frees what it holds first; a failure leaves the buffer empty (count() == 0)
    hipError_t alloc(size_t count) {
        reset();
        void* p = nullptr;
        const hipError_t e = hipMalloc(&p, count * kDevBufElem<T>);
        if (e != hipSuccess) return e;
        p_ = static_cast<T*>(p); n_ = count;
        g_devBufLive++; g_devBufBytes += count * kDevBufElem<T>;
        return hipSuccess;
    }
    // grow-only, and the contents are NOT carried over: callers overwrite after growing
    hipError_t reserve(size_t count) { return count <= n_ ? hipSuccess : alloc(count); }
    void reset() { if (T* p = release()) hipFree(p); }
    // gives the allocation up without freeing it: the caller owns it (or leaks it on purpose) from here on
    T* release() {
        T* p = p_;
        if (p) { g_devBufLive--; g_devBufBytes -= n_ * kDevBufElem<T>; }
        p_ = nullptr; n_ = 0;
        return p;
    }
    T* get() const { return p_; }
    operator T*() const { return p_; }   // launch arguments and copies take the buffer as the pointer it is
    explicit operator bool() const { return p_ != nullptr; }
    size_t count() const { return n_; }   // capacity in elements (DevBuf<void>: bytes)

private:
    T* p_ = nullptr;
    size_t n_ = 0;
};

// One scratch allocation divided into parts, in the order they are taken, every part 256-byte aligned.  A null base only measures: the parts
// come back null and total() is the size to allocate.
class ScratchCarver {
public:
    explicit ScratchCarver(void* base) : base_(static_cast<char*>(base)) {}
    void* take_bytes(size_t bytes) {
        void* p = base_ ? base_ + off_ : nullptr;
        off_ += (bytes + 255) & ~(size_t)255;
        return p;
    }
    template <class T> T* take(size_t count) { return static_cast<T*>(take_bytes(count * sizeof(T))); }
    size_t total() const { return off_; }

private:
    char* base_;
    size_t off_ = 0;
};

}  // namespace tbvh_capi
