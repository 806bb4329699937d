// devbuf_check.cpp — DevBuf / PinBuf (query_amd/csrc/n1k_buf.h) against stubbed allocation functions, on the CPU.
//
// A stand-alone host program: the four HIP allocation calls are defined HERE (malloc / free plus a ledger of what is
// outstanding), nothing of the HIP runtime is linked and no GPU is touched.  Built with -fsanitize=address,undefined it
// turns a double free, a use after free or a leak of the owners into a report; the ledger and the library's own byte count
// are asserted on top.  tests/test_devbuf_cpu.py builds and runs it.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>
#include <vector>

#include "../../query_amd/csrc/n1k_buf.h"

namespace {
std::map<void*, size_t> g_device, g_pinned;  // outstanding allocations of the stubs
size_t g_fail_at = 0;                        // fail the allocation of this many bytes (0: none)
int g_failures = 0;

hipError_t stub_alloc(std::map<void*, size_t>& ledger, void** p, size_t bytes) {
    if (bytes == g_fail_at) return hipErrorOutOfMemory;
    *p = malloc(bytes);
    ledger[*p] = bytes;
    return hipSuccess;
}
hipError_t stub_free(std::map<void*, size_t>& ledger, void* p) {
    if (!ledger.erase(p)) {
        fprintf(stderr, "free of %p, which the stub never handed out (or a second free)\n", p);
        abort();
    }
    free(p);
    return hipSuccess;
}
size_t outstanding(const std::map<void*, size_t>& ledger) {
    size_t s = 0;
    for (auto& kv : ledger) s += kv.second;
    return s;
}
}  // namespace

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) { return stub_alloc(g_device, p, bytes); }
hipError_t hipFree(void* p) { return stub_free(g_device, p); }
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned int) { return stub_alloc(g_pinned, p, bytes); }
hipError_t hipHostFree(void* p) { return stub_free(g_pinned, p); }
}

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            g_failures++;                                                   \
        }                                                                   \
    } while (0)

using n1k_eng::DevBuf;
using n1k_eng::PinBuf;
static uint64_t live() { return n1k_eng::g_device_bytes_live.load(); }
// the library's count is the device ledger's, at every step
#define LEDGER() CHECK(live() == outstanding(g_device))

template <class Buf, bool kCounted>
static void cases(std::map<void*, size_t>& ledger) {
    const size_t elem = sizeof(*Buf().p);
    {  // ensure: allocation, no-op below the size, growth by free + allocate
        Buf a;
        CHECK(a.ensure(100) == hipSuccess && a.p && a.n == 100);
        a.p[99] = 7;
        void* first = a.p;
        CHECK(a.ensure(50) == hipSuccess && a.p == first && a.n == 100 && a.p[99] == 7);
        CHECK(a.ensure(1000) == hipSuccess && a.n == 1000 && outstanding(ledger) == 1000 * elem);
        a.p[999] = 1;
        LEDGER();
        // release then reuse
        a.release();
        CHECK(!a.p && a.n == 0 && outstanding(ledger) == 0);
        a.release();  // (of an empty buffer: nothing)
        CHECK(a.ensure(20) == hipSuccess && a.n == 20);
        a.p[19] = 3;
        // a failed allocation leaves an empty buffer that can be used again
        g_fail_at = 4096 * elem;
        CHECK(a.ensure(4096) == hipErrorOutOfMemory && !a.p && a.n == 0 && outstanding(ledger) == 0);
        g_fail_at = 0;
        CHECK(a.ensure(4096) == hipSuccess && a.n == 4096);
        LEDGER();
    }
    CHECK(outstanding(ledger) == 0);  // the destructor freed
    {  // move construct: the source is left empty, one free in all
        Buf a;
        CHECK(a.ensure(64) == hipSuccess);
        void* p = a.p;
        Buf b(std::move(a));
        CHECK(b.p == p && b.n == 64 && !a.p && a.n == 0 && outstanding(ledger) == 64 * elem);
        // move assign onto a full buffer: what the target held is freed
        Buf c;
        CHECK(c.ensure(32) == hipSuccess);
        c = std::move(b);
        CHECK(c.p == p && c.n == 64 && !b.p && outstanding(ledger) == 64 * elem);
        // move assign of an empty buffer empties the target
        Buf e;
        c = std::move(e);
        CHECK(!c.p && c.n == 0 && outstanding(ledger) == 0);
        // self-move keeps the buffer
        CHECK(c.ensure(48) == hipSuccess);
        p = c.p;
        Buf& alias = c;
        c = std::move(alias);
        CHECK(c.p == p && c.n == 48 && outstanding(ledger) == 48 * elem);
        c.p[47] = 5;
        LEDGER();
    }
    CHECK(outstanding(ledger) == 0);
    {  // a vector of them resized: grown (its elements move, noexcept), shrunk (the tail is freed), cleared
        std::vector<Buf> v(3);
        for (size_t i = 0; i < v.size(); i++) CHECK(v[i].ensure(16 * (i + 1)) == hipSuccess);
        void* p0 = v[0].p;
        v.resize(200);
        CHECK(v[0].p == p0 && v[2].n == 48 && !v[199].p && outstanding(ledger) == (16 + 32 + 48) * elem);
        CHECK(v[150].ensure(16) == hipSuccess);
        v.resize(2);
        CHECK(outstanding(ledger) == (16 + 32) * elem);
        v.shrink_to_fit();
        CHECK(v[1].n == 32 && outstanding(ledger) == (16 + 32) * elem);
        LEDGER();
    }
    CHECK(outstanding(ledger) == 0);
    CHECK(live() == 0);  // the counter is back at zero (and a pinned buffer never moved it)
    (void)kCounted;
}

int main() {
    static_assert(std::is_nothrow_move_constructible<DevBuf<uint64_t>>::value && std::is_nothrow_move_assignable<DevBuf<uint64_t>>::value, "");
    static_assert(!std::is_copy_constructible<DevBuf<char>>::value && !std::is_copy_assignable<PinBuf<char>>::value, "");
    cases<DevBuf<uint64_t>, true>(g_device);
    CHECK(g_pinned.empty());
    cases<PinBuf<char>, false>(g_pinned);
    CHECK(g_device.empty());
    {  // the device minimum of 16 elements, the pinned buffer's exact size, and the count while buffers live
        DevBuf<uint32_t> d;
        PinBuf<char> h;
        CHECK(d.ensure(3) == hipSuccess && d.n == 16 && h.ensure(3) == hipSuccess && h.n == 3);
        CHECK(live() == 64 && outstanding(g_device) == 64 && outstanding(g_pinned) == 3);
    }
    CHECK(live() == 0 && g_device.empty() && g_pinned.empty());
    if (g_failures) return 1;
    puts("devbuf_check: ok");
    return 0;
}
