// A device buffer that frees itself: what a kernel set owns instead of a raw pointer, a capacity variable and a line in its destructor.  Grows only, move-only; kernel
// argument structs keep the raw pointer `p`.  Plain C++ but for hipMalloc / hipFree / hipMemsetAsync and HIP_CHECK, which the including file provides (common.h; the
// host test of tests/test_dev_buf.py provides counting stand-ins).
#pragma once
#include <cstddef>

namespace optamd {

template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;      // elements
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; } return *this; }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    bool reserve(size_t n) { if (n <= cap) return false; release(); HIP_CHECK(hipMalloc((void**)&p, n * sizeof(T))); cap = n; return true; }      // true: reallocated (the old contents are gone)
    bool reserveZeroed(size_t n, hipStream_t s) { if (!reserve(n)) return false; HIP_CHECK(hipMemsetAsync(p, 0, n * sizeof(T), s)); return true; }      // ... and the new allocation cleared, in stream order
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    operator T*() const { return p; }
};

}  // namespace optamd
