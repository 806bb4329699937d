// n1k_in.h — IN over a constant list (expression/coll_in.go:61-91): the string half, which belongs to the match table.
//
// `x IN [c, c, ...]` is TRUE when x.Equals(c) holds for some element.  Equals is FALSE across type classes, so a list
// falls apart by class: its numbers go to the row term (TERM_IN, n1k_device.h: a sorted array and a binary search), its
// booleans and its `null` are flags of the term, and its STRINGS are one more predicate over dictionary entries — "is this
// entry one of the list's strings" — evaluated once per distinct entry into the list's bit of the match table, like a LIKE
// pattern or an ANY / EVERY predicate.  Strings compare bytewise (value/string.go:82-96), so there is no UTF-8 rule.
//
// All lists of a plan share ONE open-addressed table of their distinct string constants: a constant carries the mask of
// the lists that hold it, an entry is hashed once and probed once, whatever the number of lists.  in_hash and in_lookup
// are what both the host and in_match_kernel run.
#pragma once
#include "n1k_like.h"

namespace n1k {

// Distinct STRING constants of one list.  A choice, not a measurement: with 8 lists the table is 64 Ki slots of 4 B.
constexpr uint32_t kInMaxStrings = 4096;
constexpr uint32_t kInDevMaxLen = kLikeDevMaxLen;  // bytes of a dictionary string the device kernel takes: LIKE's, the same 8 KiB slab a wave
// New dictionary entries from which the device route is taken: LIKE's figure (n1k_like.h).  Measured through the handle
// ("IN: measured", tools/exp_in.py route; strings of 29 B, a 1000-string list): the host route costs 0.040 ms
// for 256 new strings and 0.075 ms for 1023, the device route a fixed 0.14 ms up to 4 Ki (0.70 ms for 64 Ki) — the two cross
// near 2.5 Ki.  Kept at 1024: at worst 0.065 ms more, once, for a dictionary that grows by 1 Ki to 2.5 Ki strings.
constexpr uint32_t kInDeviceThreshold = kLikeDeviceThreshold;

// the string constants of a plan's lists (host or device memory)
struct InTable {
    const uint32_t* slots;   // slot_mask + 1 (a power of two, at least twice nconst): constant index + 1, 0 = free
    const uint32_t* c_off;   // nconst + 1: constant k = c_bytes[c_off[k], c_off[k + 1])
    const uint8_t* c_mask;   // nconst: the bits of the lists that hold constant k
    const uint8_t* c_bytes;
    uint32_t slot_mask, nconst;
};

N1K_HD uint32_t in_hash(const uint8_t* s, uint32_t n) {  // FNV-1a and a final avalanche (the low bits index the table)
    uint32_t h = 0x811C9DC5u;
    for (uint32_t i = 0; i < n; i++) h = (h ^ s[i]) * 0x01000193u;
    h ^= h >> 15;
    h *= 0x2C1B3C6Du;
    h ^= h >> 12;
    return h;
}

// the mask of the lists that hold the string s[0, len), 0 when none does
N1K_HD uint8_t in_lookup(const InTable& T, const uint8_t* s, uint32_t len) {
    if (T.nconst == 0) return 0;
    uint32_t i = in_hash(s, len) & T.slot_mask;
    for (uint32_t step = 0; step <= T.slot_mask; step++, i = (i + 1) & T.slot_mask) {  // (at most half full: a free slot ends it)
        const uint32_t k = T.slots[i];
        if (k == 0) return 0;
        const uint32_t o = T.c_off[k - 1];
        if (T.c_off[k] - o != len) continue;
        uint32_t b = 0;
        while (b < len && T.c_bytes[o + b] == s[b]) b++;
        if (b == len) return T.c_mask[k - 1];
    }
    return 0;
}

struct InKernelArgs {
    EntryBlockArgs blk;  // out_bits: the mask of the lists that hold the entry; left: longer than kInDevMaxLen
    InTable tab;         // device memory
};

}  // namespace n1k

#if !defined(__HIPCC_RTC__)
#include <hip/hip_runtime.h>
#include <string>
#include <vector>

namespace n1k {

struct Expr;
struct PlanError;

// one list of a plan, by class
struct InList {
    std::string text;                  // the bracketed list as the plan wrote it (two terms with the same text share everything)
    std::vector<std::string> strings;  // distinct
    std::vector<double> numbers;       // distinct, ascending; each within +-2^53
    bool has_true = false, has_false = false, has_null = false, empty = false;
    uint32_t num_begin = 0, num_end = 0;  // its range of the plan's number array
    uint8_t mask = 0;                     // its bit of a match-table entry (0: no string)
};

// the table on the host; view() is valid while the object is neither changed nor moved
struct InTableHost {
    std::vector<uint32_t> slots, c_off;
    std::vector<uint8_t> c_mask, c_bytes;
    InTable view() const {
        return InTable{slots.data(), c_off.data(), c_mask.data(), c_bytes.data(), slots.empty() ? 0u : (uint32_t)slots.size() - 1u, (uint32_t)c_mask.size()};
    }
};

// An EK::In expression -> list.  false + err (unsupported, the construct named) for what lies outside the subset.
bool in_compile(const Expr* e, InList& out, PlanError& err);
// the strings of every list with a mask into one table
void in_build_table(const std::vector<InList>& lists, InTableHost& out);
// bits[i] |= the mask of the lists that hold entry i
void in_match_block_host(const InTable& T, uint64_t n, const uint64_t* offsets, const uint8_t* bytes, uint8_t* bits);
// The table as one device allocation: bytes to upload, and the view once they lie at `base`.
void in_table_blob(const InTableHost& T, std::vector<uint8_t>& blob);
InTable in_table_at(const InTableHost& T, const uint8_t* base);
hipError_t launch_in_match(const InKernelArgs& A, hipStream_t st);

}  // namespace n1k
#endif
