// device_mem.h — host-only owners of HIP memory and events.
//
// Every device buffer, pinned host buffer and event of the library lives in one of these types: freed by the destructor,
// move-only, so at any time exactly one object owns a resource.  No HIP call appears where the owner is used: kernel
// launches and copies take the buffer itself (it converts to its pointer).  A destructor runs HIP calls: the owning
// index's device must be current and idle then (codd_knn_destroy sees to both).
//
// Three process-wide counters (live buffers, their bytes, live events) back codd_knn_debug_live_allocations.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include <utility>

namespace codd {

inline std::atomic<int64_t> g_live_buffers{0}, g_live_bytes{0}, g_live_events{0};

// `cap` elements of T in device memory (PINNED: page-locked host memory).  Never shrinks on its own.
template <typename T, bool PINNED = false>
class DevBuf {
    T* p_ = nullptr;
    int64_t cap_ = 0;

public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            (void)reset();
            p_ = std::exchange(o.p_, nullptr);
            cap_ = std::exchange(o.cap_, 0);
        }
        return *this;
    }
    ~DevBuf() { (void)reset(); }

    T* get() const { return p_; }
    operator T*() const { return p_; }
    T* operator->() const { return p_; }
    int64_t cap() const { return cap_; }
    int64_t bytes() const { return cap_ * (int64_t)sizeof(T); }

    // Frees, then allocates exactly n elements (n = 0: frees only).  No synchronisation: for callers that have drained the
    // device, or the streams that may still read the old allocation, themselves.  Empty after a failure.
    hipError_t reset(int64_t n = 0) {
        if (p_) {
            (void)(PINNED ? hipHostFree(p_) : hipFree(p_));
            g_live_buffers.fetch_sub(1, std::memory_order_relaxed);
            g_live_bytes.fetch_sub(bytes(), std::memory_order_relaxed);
            p_ = nullptr;
            cap_ = 0;
        }
        if (n <= 0) return hipSuccess;
        const size_t want = (size_t)n * sizeof(T);
        const hipError_t e = PINNED ? hipHostMalloc((void**)&p_, want, hipHostMallocDefault) : hipMalloc((void**)&p_, want);
        if (e != hipSuccess) {
            p_ = nullptr;
            return e;
        }
        cap_ = n;
        g_live_buffers.fetch_add(1, std::memory_order_relaxed);
        g_live_bytes.fetch_add(bytes(), std::memory_order_relaxed);
        return hipSuccess;
    }

    // At least `need` elements: nothing to do when they are there; otherwise exactly `need`, after a device synchronisation
    // when an allocation is replaced (work enqueued earlier may still read it).  Contents are not kept.
    hipError_t ensure(int64_t need) {
        if (need <= cap_) return hipSuccess;
        if (p_) {
            const hipError_t e = hipDeviceSynchronize();
            if (e != hipSuccess) return e;
        }
        return reset(need);
    }
};
template <typename T>
using PinnedBuf = DevBuf<T, true>;

// An event, created on first need.
class Event {
    hipEvent_t e_ = nullptr;

public:
    Event() = default;
    Event(Event&& o) noexcept : e_(std::exchange(o.e_, nullptr)) {}
    Event& operator=(Event&& o) noexcept {
        if (this != &o) {
            destroy();
            e_ = std::exchange(o.e_, nullptr);
        }
        return *this;
    }
    ~Event() { destroy(); }

    operator hipEvent_t() const { return e_; }

    // the event exists afterwards; `flags` count only for the call that creates it
    hipError_t ensure(unsigned flags = hipEventDisableTiming) {
        if (e_) return hipSuccess;
        const hipError_t e = hipEventCreateWithFlags(&e_, flags);
        if (e != hipSuccess) e_ = nullptr;
        else g_live_events.fetch_add(1, std::memory_order_relaxed);
        return e;
    }

private:
    void destroy() {
        if (!e_) return;
        (void)hipEventDestroy(e_);
        g_live_events.fetch_sub(1, std::memory_order_relaxed);
        e_ = nullptr;
    }
};

}  // namespace codd
