// n1k_wire.h — the arithmetic of the exchange's regions (n1k_exchange.cpp): what a packed row region looks like, and where the
// regions of one collective lie in the buffers they are sent from and received into.  Host only and without HIP: pointers and
// sizes in, pointers and sizes out — tests/host/wire_check.cpp checks it on the CPU.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "n1k_types.h"

namespace n1k_eng {

// a row region holds kRowSubs sub-regions of whole 16-row groups: capacities are rounded up to that
constexpr uint64_t kRowQuantum = 16ull * n1k::kRowSubs;
inline uint64_t quantum(uint64_t rows) { return (rows + kRowQuantum - 1) / kRowQuantum * kRowQuantum; }

// header of a row region: sub-region x's row count at word x * kCursorStride (128 bytes apart), the verdict in word 1
constexpr size_t kRowHeaderBytes = (size_t)n1k::kRowSubs * n1k::kCursorStride * 8;

// One packed row region for `cap` rows (kRowSubs sub-regions of cap / kRowSubs rows) of the plan's input columns: the header,
// then per column its arrays, each starting on a 16-byte boundary — DICT32: codes at a[i]; TAGGED64: payload at a[i], tags at
// b[i].  `bytes` is the whole region, a multiple of 128.
struct RowLayout {
    size_t bytes = 0;
    std::vector<size_t> a, b;
};

// (a, b: where to put the offsets of the nc columns, or null for the length alone)
inline size_t row_region_walk(const uint32_t* kinds, size_t nc, uint64_t cap, size_t* a, size_t* b) {
    size_t at = kRowHeaderBytes;
    auto pad = [](size_t x) { return (x + 15) / 16 * 16; };
    for (size_t i = 0; i < nc; i++) {
        if (a) a[i] = at;
        if (kinds[i] == n1k::COLK_DICT32) at = pad(at + cap * 4);
        else {
            at = pad(at + cap * 8);  // payload
            if (b) b[i] = at;
            at = pad(at + cap);  // tags
        }
    }
    return (at + 127) / 128 * 128;
}
inline size_t row_region_bytes(const uint32_t* kinds, size_t nc, uint64_t cap) { return row_region_walk(kinds, nc, cap, nullptr, nullptr); }
inline RowLayout row_region_layout(const uint32_t* kinds, size_t nc, uint64_t cap) {
    RowLayout L{0, std::vector<size_t>(nc), std::vector<size_t>(nc)};
    L.bytes = row_region_walk(kinds, nc, cap, L.a.data(), L.b.data());
    return L;
}

// The regions of one collective.  All-to-all: the region at send + p * send_stride goes to rank p, rank s's region lands at
// recv + s * recv_stride; `region` bytes arrive from every peer, and rank p is sent send_bytes[p] of them (null: `region`; every
// rank sizes the regions for destination p alike, so send_bytes[own rank] == region).  All-gather: `region` bytes from `send`,
// rank s's at recv + s * region.  A stride of 0 is ONE region for every peer / one sink for whatever arrives.
// send_extent / recv_extent: the sizes of the buffers behind the two pointers.
struct Wire {
    const char* send = nullptr;
    size_t send_extent = 0, send_stride = 0;
    char* recv = nullptr;
    size_t recv_extent = 0, recv_stride = 0;
    size_t region = 0;
    const size_t* send_bytes = nullptr;
};

// What one exchange step moves: nsend regions send_stride apart leave, nrecv regions of `region` bytes arrive.
struct StepShape {
    size_t send_stride = 0, region = 0;
    uint32_t nsend = 1, nrecv = 1;
    bool gathered = false;               // an all-gather (what arrives must lie contiguously), else an all-to-all
    const size_t* send_bytes = nullptr;  // all-to-all of unequal regions: see Wire
};

// the communicator's usual buffers (so many bytes each) hold this step's regions
inline bool usual_buffers_hold(const StepShape& s, size_t send_have, size_t recv_have) {
    return send_have >= s.send_stride * s.nsend && recv_have >= s.region * s.nrecv;
}
// else a rank that ships nothing but its status takes part with ONE scratch region that goes to every peer and one that
// every peer's region lands in (gathered: nrecv of them, side by side) — of these sizes
inline size_t scratch_send_bytes(const StepShape& s) { return s.send_stride; }
inline size_t scratch_recv_bytes(const StepShape& s) { return s.gathered ? s.region * s.nrecv : s.region; }

// the step's regions in a pair of buffers: the usual form, or (scratch) the one-region form
inline Wire wire_of(const StepShape& s, const char* send, size_t send_have, char* recv, size_t recv_have, bool scratch) {
    return Wire{send, send_have, scratch ? 0 : s.send_stride, recv, recv_have, scratch && !s.gathered ? 0 : s.region, s.region, s.send_bytes};
}

// what a rank that ships nothing but its status takes part with: the usual buffers when they hold the step, else the scratch pair
inline Wire voided_wire(const StepShape& s, const char* send, size_t send_have, char* recv, size_t recv_have, const char* scratch_send,
                        size_t scratch_send_have, char* scratch_recv, size_t scratch_recv_have) {
    return usual_buffers_hold(s, send_have, recv_have) ? wire_of(s, send, send_have, recv, recv_have, false)
                                                       : wire_of(s, scratch_send, scratch_send_have, scratch_recv, scratch_recv_have, true);
}

}  // namespace n1k_eng
