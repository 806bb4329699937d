// wire_check.cpp — the arithmetic of the exchange's regions (query_amd/csrc/n1k_wire.h) on the CPU.
//
// A stand-alone host program: no HIP, no GPU.  It sizes the steps of the row exchange the way n1k_exchange.cpp does (capacities
// rounded to the quantum, one layout for the largest capacity and one for this rank's own, a wire length per destination) over
// world sizes x column kinds x capacity vectors x states of the communicator's buffers, and holds every region a collective
// would touch against the extent of the buffer it lies in.  Built with -fsanitize=address,undefined by tests/test_wire_cpu.py.
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "../../query_amd/csrc/n1k_wire.h"

using namespace n1k_eng;

static int g_failures = 0;
static std::string g_case;
#define CHECK(cond)                                                                                  \
    do {                                                                                             \
        if (!(cond)) {                                                                               \
            fprintf(stderr, "%s:%d: CHECK(%s) failed [%s]\n", __FILE__, __LINE__, #cond, g_case.c_str()); \
            g_failures++;                                                                            \
        }                                                                                            \
    } while (0)

// what a DevBuf<char> holds after ensure(count) on an empty buffer
static size_t ensured(size_t count) { return count ? std::max<size_t>(count, 16) : 0; }

// one step of the row exchange as rank `rank` sizes it (the front of n1k_exchange.cpp exchange_rows_impl)
struct RowsSizes {
    std::vector<uint64_t> cap;
    uint64_t cap_max = 0;
    std::vector<size_t> wire;
    RowLayout widest, mine;
    StepShape shape;
    RowsSizes(const std::vector<uint32_t>& kinds, const std::vector<uint64_t>& rows, int rank) {
        const uint32_t P = (uint32_t)rows.size();
        for (uint64_t r : rows) {
            cap.push_back(quantum(r));
            cap_max = std::max(cap_max, cap.back());
        }
        widest = row_region_layout(kinds.data(), kinds.size(), cap_max);
        mine = row_region_layout(kinds.data(), kinds.size(), cap[rank]);
        for (uint32_t d = 0; d < P; d++) wire.push_back(row_region_bytes(kinds.data(), kinds.size(), cap[d]));
        shape.send_stride = widest.bytes;
        shape.region = mine.bytes;
        shape.nsend = shape.nrecv = P;
        shape.send_bytes = wire.data();
    }
};

// the arrays of a layout follow the header, start on 16-byte boundaries, do not overlap and end inside the region
static void check_layout(const RowLayout& L, const std::vector<uint32_t>& kinds, uint64_t cap) {
    CHECK(L.bytes % 128 == 0 && L.a.size() == kinds.size() && L.b.size() == kinds.size());
    size_t end = kRowHeaderBytes;
    for (size_t i = 0; i < kinds.size(); i++) {
        CHECK(L.a[i] % 16 == 0 && L.a[i] >= end);
        if (kinds[i] == n1k::COLK_DICT32) end = L.a[i] + cap * 4;
        else {
            CHECK(L.b[i] % 16 == 0 && L.b[i] >= L.a[i] + cap * 8);
            end = L.b[i] + cap;
        }
    }
    CHECK(end <= L.bytes && L.bytes - end < 128 + 16);
}

// every region the collective sends or lets land, the last included, lies inside its extent; regions a stride apart do not overlap
static void check_wire(const Wire& w, const StepShape& s, int world) {
    CHECK(w.region == s.region && w.region % 8 == 0);
    if (s.gathered) {
        CHECK(w.region <= w.send_extent && w.region * (size_t)world <= w.recv_extent);
        return;
    }
    for (int p = 0; p < world; p++) {
        const size_t len = w.send_bytes ? w.send_bytes[p] : w.region;
        CHECK((size_t)p * w.send_stride + len <= w.send_extent);
        CHECK(w.send_stride == 0 || len <= w.send_stride);
        CHECK((size_t)p * w.recv_stride + w.region <= w.recv_extent);
    }
    CHECK(w.recv_stride == 0 || w.region <= w.recv_stride);
}

// the communicator's usual buffers as a step of shape `sized_by` left them (null: never allocated), a step of shape `s` on
// top: the good form when the buffers hold it, and what a rank that voids the step takes part with
static void check_buffers(const StepShape& s, const StepShape* sized_by, bool must_hold, int world) {
    const size_t send_have = sized_by ? ensured(sized_by->send_stride * sized_by->nsend) : 0;
    const size_t recv_have = sized_by ? ensured(sized_by->region * sized_by->nrecv) : 0;
    // "hold": the local part's ensure() of this step's regions would find them there
    const bool hold = send_have >= s.send_stride * s.nsend && recv_have >= s.region * s.nrecv;
    CHECK(usual_buffers_hold(s, send_have, recv_have) == hold);
    if (must_hold) CHECK(hold);
    static char usual_send, usual_recv, scratch_send, scratch_recv;  // (addresses only: nothing is read or written through them)
    if (hold) {  // a step whose local part succeeded goes from the usual buffers
        const Wire good = wire_of(s, &usual_send, send_have, &usual_recv, recv_have, false);
        CHECK(good.send == &usual_send && good.recv == &usual_recv && good.send_stride == s.send_stride && good.recv_stride == s.region);
        check_wire(good, s, world);
    }
    // a voided step, as n1k_exchange.cpp void_wire composes it: the scratch pair is allocated only when the usual buffers do not
    // hold the step, and the scratch form is chosen exactly then: one region for every peer, one sink (gathered: a contiguous one)
    const size_t scratch_send_have = hold ? 0 : ensured(scratch_send_bytes(s)), scratch_recv_have = hold ? 0 : ensured(scratch_recv_bytes(s));
    const Wire w = voided_wire(s, &usual_send, send_have, &usual_recv, recv_have, &scratch_send, scratch_send_have, &scratch_recv, scratch_recv_have);
    if (hold) CHECK(w.send == &usual_send && w.recv == &usual_recv && w.send_stride == s.send_stride && w.recv_stride == s.region);
    else CHECK(w.send == &scratch_send && w.recv == &scratch_recv && w.send_stride == 0 && w.recv_stride == (s.gathered ? s.region : 0));
    check_wire(w, s, world);
}

int main() {
    const uint32_t D = n1k::COLK_DICT32, T = n1k::COLK_TAGGED64;
    const std::vector<std::pair<const char*, std::vector<uint32_t>>> kind_sets = {
        {"dict32", {D, D, D}}, {"tagged64", {T, T, T}}, {"mixed", {D, T, T, D}}};
    CHECK(kRowQuantum == 128 && quantum(1) == 128 && quantum(128) == 128 && quantum(129) == 256);
    for (int world : {1, 2, 3, 8}) {
        const std::vector<std::pair<const char*, std::vector<uint64_t>>> cap_sets = {
            {"one-quantum", std::vector<uint64_t>(world, 1)},
            {"large", std::vector<uint64_t>(world, 1000001)},
            {"hot-owner", [&] { std::vector<uint64_t> v(world, 5000); v[world / 2] = 20000; return v; }()}};
        for (auto& ks : kind_sets)
            for (auto& cs : cap_sets)
                for (int rank = 0; rank < world; rank++) {
                    g_case = std::string(ks.first) + " " + cs.first + " world " + std::to_string(world) + " rank " + std::to_string(rank);
                    const RowsSizes z(ks.second, cs.second, rank);
                    auto scaled = [&](uint64_t num, uint64_t den) {
                        std::vector<uint64_t> v;
                        for (uint64_t r : cs.second) v.push_back(std::max<uint64_t>(1, r * num / den));
                        return RowsSizes(ks.second, v, rank);
                    };
                    const RowsSizes smaller = scaled(1, 2), larger = scaled(2, 1);
                    // lengths and offsets; the receiver's layout for its own capacity is the sender's for that destination
                    check_layout(z.widest, ks.second, z.cap_max);
                    check_layout(z.mine, ks.second, z.cap[rank]);
                    for (int d = 0; d < world; d++) {
                        CHECK(z.cap[d] % kRowQuantum == 0 && z.cap[d] >= cs.second[d] && z.cap[d] - cs.second[d] < kRowQuantum);
                        CHECK(z.wire[d] % 128 == 0 && z.wire[d] <= z.widest.bytes);
                        const RowLayout sender_side = row_region_layout(ks.second.data(), ks.second.size(), z.cap[d]);
                        const RowsSizes owner(ks.second, cs.second, d);  // (rank d, sizing the same step)
                        CHECK(sender_side.bytes == z.wire[d] && owner.shape.region == z.wire[d] && owner.mine.bytes == z.wire[d]);
                        CHECK(sender_side.a == owner.mine.a && sender_side.b == owner.mine.b);
                        if (z.cap[d] == z.cap_max) CHECK(sender_side.a == z.widest.a && sender_side.b == z.widest.b);
                    }
                    CHECK(z.shape.region == z.wire[rank] && z.shape.send_stride % 128 == 0);
                    // the communicator's buffers: absent, sized by a smaller step, exact, sized by a larger step
                    check_buffers(z.shape, nullptr, false, world);
                    check_buffers(z.shape, &smaller.shape, false, world);
                    check_buffers(z.shape, &z.shape, true, world);
                    check_buffers(z.shape, &larger.shape, true, world);
                    // (one quantum halved is one quantum still: that "smaller" step left buffers that hold this one)
                    if (std::string(cs.first) != "one-quantum")
                        CHECK(!usual_buffers_hold(z.shape, smaller.shape.send_stride * world, smaller.shape.region * world));
                }
        // the regions of partial groups (8 * (2 + capacity * (1 + words)) bytes), hash-partitioned and gathered
        for (uint64_t groups : {1ull, 1024ull, 70001ull})
            for (int gathered = 0; gathered < 2; gathered++) {
                g_case = "partials " + std::to_string(groups) + " groups world " + std::to_string(world) + (gathered ? " gathered" : "");
                auto shape_of = [&](uint64_t g) {
                    StepShape s;
                    s.send_stride = s.region = 8 * (2 + g * (1 + 5));
                    s.nrecv = (uint32_t)world;
                    s.nsend = gathered ? 1u : (uint32_t)world;
                    s.gathered = gathered != 0;
                    return s;
                };
                const StepShape s = shape_of(groups), smaller = shape_of(groups / 2), larger = shape_of(groups * 4);
                check_buffers(s, nullptr, false, world);
                check_buffers(s, &smaller, false, world);
                check_buffers(s, &s, true, world);
                check_buffers(s, &larger, true, world);
            }
    }
    if (g_failures) return 1;
    puts("wire_check: ok");
    return 0;
}
