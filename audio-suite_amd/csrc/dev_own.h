// dev_own.h — owners of device memory, pinned host memory and events.  The
// only file in csrc/ that allocates or frees them: everything else holds a
// DevBuf, a PinnedBuf or an Event, and the owner's destructor releases it.
// None can be copied; a DevBuf can be moved (plan tables, the Bluestein cache).
// Process-wide counts of what is live are kept for msg_debug_live
// (tests/test_gpu_lifecycle.py).
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <cstdint>

namespace devown {

struct Live {
    std::atomic<int64_t> dev_n{0}, dev_bytes{0}, pinned_n{0}, events{0};
};
inline Live g_live;
constexpr auto RLX = std::memory_order_relaxed;

}  // namespace devown

// Device memory of `cap` elements.  ensure() grows with 25 % headroom (the old
// block is freed first; hipFree waits for the work that uses it), alloc() is
// exact, upload() is alloc() plus a blocking copy (tables written once).
template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;   // elements
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~DevBuf() { release(); }
    hipError_t alloc(size_t n) {
        release();
        const hipError_t e = hipMalloc(&p, n * sizeof(T));
        if (e != hipSuccess) { p = nullptr; return e; }
        cap = n;
        if (p) {
            devown::g_live.dev_n.fetch_add(1, devown::RLX);
            devown::g_live.dev_bytes.fetch_add((int64_t)(n * sizeof(T)), devown::RLX);
        }
        return e;
    }
    hipError_t ensure(size_t n) {
        if (n <= cap && p) return hipSuccess;
        const size_t want = std::max<size_t>(n, 1);
        return alloc(want + want / 4);
    }
    hipError_t upload(const T* src, size_t n) {
        const hipError_t e = alloc(n);
        return e != hipSuccess ? e : hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice);
    }
    void release() {
        if (p) {
            hipFree(p);
            devown::g_live.dev_n.fetch_sub(1, devown::RLX);
            devown::g_live.dev_bytes.fetch_sub((int64_t)(cap * sizeof(T)), devown::RLX);
        }
        p = nullptr;
        cap = 0;
    }
};

// Pinned host memory of `cap` bytes.
struct PinnedBuf {
    char* p = nullptr;
    size_t cap = 0;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    ~PinnedBuf() { release(); }
    hipError_t alloc(size_t bytes) {
        release();
        const hipError_t e = hipHostMalloc((void**)&p, bytes, hipHostMallocDefault);
        if (e != hipSuccess) { p = nullptr; return e; }
        cap = bytes;
        devown::g_live.pinned_n.fetch_add(1, devown::RLX);
        return e;
    }
    void release() {
        if (p) {
            hipHostFree(p);
            devown::g_live.pinned_n.fetch_sub(1, devown::RLX);
        }
        p = nullptr;
        cap = 0;
    }
};

// An event, null until create().  Converts to hipEvent_t for the HIP calls.
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    ~Event() { release(); }
    operator hipEvent_t() const { return e; }
    hipError_t create(unsigned flags = hipEventDefault) {
        release();
        const hipError_t err = hipEventCreateWithFlags(&e, flags);
        if (err != hipSuccess) { e = nullptr; return err; }
        devown::g_live.events.fetch_add(1, devown::RLX);
        return err;
    }
    void release() {
        if (e) {
            hipEventDestroy(e);
            devown::g_live.events.fetch_sub(1, devown::RLX);
        }
        e = nullptr;
    }
};
