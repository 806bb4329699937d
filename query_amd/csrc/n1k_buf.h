// n1k_buf.h — the owners of the host engine's device memory and pinned host memory.  Host only (no kernel sees it).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstdint>

namespace n1k_eng {

// bytes of device memory the DevBufs of this process hold at this moment (n1k_device_bytes_live): added on a successful
// allocation, subtracted on the free — exact, where free device memory moves under everybody else's work
inline std::atomic<uint64_t> g_device_bytes_live{0};

// A buffer of device memory (kPinned: of pinned host memory) that frees itself: the destructor and move assignment free what
// the buffer holds, a copy does not exist.  ensure() grows by free + allocate (the contents are lost; count <= n keeps them),
// release() frees early.  Members and locals only: an owner of static or thread storage duration would free after the runtime
// has shut down.
template <typename T, bool kPinned = false>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr, o.n = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            release();
            p = o.p, n = o.n;
            o.p = nullptr, o.n = 0;
        }
        return *this;
    }
    ~DevBuf() { release(); }
    hipError_t ensure(size_t count) {
        if (count <= n) return hipSuccess;
        release();
        const size_t want = kPinned ? count : std::max(count, (size_t)16);
        hipError_t e = kPinned ? hipHostMalloc((void**)&p, want * sizeof(T), hipHostMallocDefault) : hipMalloc((void**)&p, want * sizeof(T));
        if (e != hipSuccess) {
            p = nullptr;
            return e;
        }
        n = want;
        if (!kPinned) g_device_bytes_live.fetch_add(n * sizeof(T), std::memory_order_relaxed);
        return e;
    }
    void release() {
        if (p) {
            (void)(kPinned ? hipHostFree(p) : hipFree(p));
            if (!kPinned) g_device_bytes_live.fetch_sub(n * sizeof(T), std::memory_order_relaxed);
        }
        p = nullptr;
        n = 0;
    }
};
template <typename T>
using PinBuf = DevBuf<T, true>;

}  // namespace n1k_eng
