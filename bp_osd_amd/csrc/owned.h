// owned.h -- the owning types of the host side of libbposd_mi355x.so.  Every device block, page-locked block, stream and
// event that a handle or an engine holds is a member of one of these types, so `delete` gives all of it back and a
// resource added to a struct cannot be forgotten in a free list.  They enforce ownership and nothing else: no allocator,
// no pool.  The owner drains its streams before it is deleted (bposd_destroy, bposd_mc_destroy); the destructors ignore
// HIP errors, because a handle may be destroyed while the runtime is shutting down.  The only place in the library that
// calls hipFree, hipHostFree, hipStreamDestroy and hipEventDestroy.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <utility>

// Every entry point works on the handle's device and puts the caller's current device back on exit (a process that
// also drives torch, or handles on other GPUs, must not find its thread's device changed by a decode call).
struct DeviceGuard {
    int prev = -1, dev = -1;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int d) : dev(d) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) err = hipSetDevice(dev);
    }
    ~DeviceGuard() {
        if (prev >= 0 && prev != dev) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// A device block, sized in bytes.
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), bytes(std::exchange(o.bytes, 0)) {}
    DevBuf& operator=(DevBuf&& o) noexcept {
        std::swap(p, o.p);
        std::swap(bytes, o.bytes);
        return *this;
    }
    ~DevBuf() { (void)release(); }
    hipError_t release() {
        const hipError_t e = p ? hipFree(p) : hipSuccess;
        p = nullptr;
        bytes = 0;
        return e;
    }
    // a fresh block of exactly `want` bytes; what the buffer held is freed first
    hipError_t alloc(size_t want) {
        hipError_t e = release();
        if (e == hipSuccess) e = hipMalloc(&p, want);
        if (e == hipSuccess) bytes = want;
        else p = nullptr;
        return e;
    }
    // at least `want` bytes (and at least 256): nothing happens when the block is large enough, contents are not kept when it grows
    hipError_t ensure(size_t want) { return (p && want <= bytes) ? hipSuccess : alloc(std::max<size_t>(want, 256)); }
};

// A device block that is read as a T*: kernel parameter structs and pointer arithmetic take it as they take a raw pointer.
template <class T>
struct DevArray : DevBuf {
    operator T*() const { return static_cast<T*>(p); }
};

inline hipError_t free_pinned(void* p) { return p ? hipHostFree(p) : hipSuccess; }

// A page-locked host block, sized in bytes, with the hipHostMalloc flags it was made with.
struct PinnedBuf {
    void* p = nullptr;
    size_t bytes = 0;
    unsigned flags = hipHostMallocDefault;
    PinnedBuf() = default;
    PinnedBuf(PinnedBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), bytes(std::exchange(o.bytes, 0)), flags(o.flags) {}
    PinnedBuf& operator=(PinnedBuf&& o) noexcept {
        std::swap(p, o.p);
        std::swap(bytes, o.bytes);
        std::swap(flags, o.flags);
        return *this;
    }
    ~PinnedBuf() { release(); }
    void release() {
        (void)free_pinned(p);
        p = nullptr;
        bytes = 0;
    }
    hipError_t alloc(size_t want, unsigned f) {
        release();
        const hipError_t e = hipHostMalloc(&p, want, f);
        if (e == hipSuccess) { bytes = want; flags = f; }
        else p = nullptr;
        return e;
    }
    template <class T>
    T* as() const { return static_cast<T*>(p); }
};

// A stream or an event: converts to the raw handle, which the creating call writes into `raw`.
template <class H, hipError_t (*Destroy)(H)>
struct OwnedHandle {
    H raw = nullptr;
    OwnedHandle() = default;
    OwnedHandle(OwnedHandle&& o) noexcept : raw(std::exchange(o.raw, nullptr)) {}
    OwnedHandle& operator=(OwnedHandle&& o) noexcept {
        std::swap(raw, o.raw);
        return *this;
    }
    ~OwnedHandle() {
        if (raw) (void)Destroy(raw);
    }
    operator H() const { return raw; }
};
using Stream = OwnedHandle<hipStream_t, hipStreamDestroy>;
using Event = OwnedHandle<hipEvent_t, hipEventDestroy>;
