// rtw_devmem.h -- the one owner of HIP memory in the host code (rtw_shim.hip, rtw_filter.hip): device memory (DevMem) or pinned host memory
// (PinnedMem).  Move-only; the destructor frees, so a buffer is dropped by letting it go and a group of them by assigning an empty group.
// The device that was current when the memory was reserved must be current when it is freed.
#pragma once
#include <hip/hip_runtime.h>
#include <utility>

namespace rtw {

template <bool PINNED>
struct Mem {
    void *ptr = nullptr;
    size_t cap = 0;                  // bytes

    Mem() = default;
    Mem(Mem &&o) noexcept { *this = std::move(o); }
    Mem &operator=(Mem &&o) noexcept { std::swap(ptr, o.ptr); std::swap(cap, o.cap); return *this; }   // (what this held goes with `o`)
    ~Mem() { reset(); }

    void reset() { if (ptr) (void)(PINNED ? hipHostFree(ptr) : hipFree(ptr)); ptr = nullptr; cap = 0; }
    // At least `bytes`, contents NOT kept when it has to grow; on failure the buffer is empty.  (reserve(0) of an empty buffer leaves it empty.)
    hipError_t reserve(size_t bytes) {
        if (cap >= bytes) return hipSuccess;
        reset();
        const hipError_t e = PINNED ? hipHostMalloc(&ptr, bytes, hipHostMallocDefault) : hipMalloc(&ptr, bytes);
        if (e == hipSuccess) cap = bytes; else ptr = nullptr;
        return e;
    }
    template <class T> T *as() const { return static_cast<T *>(ptr); }
};
using DevMem = Mem<false>;
using PinnedMem = Mem<true>;

// Is `p` memory the kernels of GPU `device` can address (device or managed memory of that GPU)?  Anything else is staged.
inline bool on_device(const void *p, int device) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return (a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged) && a.device == device;
}

} // namespace rtw
