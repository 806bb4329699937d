// n1k_rowdistinct.h — SELECT DISTINCT over the rows a Filter-only plan selects (execution/distinct.go:60-71, value/set.go:100-103):
// the launch interface between n1k_rowdistinct.cpp and n1k_rowdistinct.hip.
//
// The ascending selection of the Filter goes in; the representatives — per distinct row key the survivor with the smallest
// ordinal — come out, ascending, still in device memory.  A row key is the plan's 1 to kRdMaxTerms result terms, each
// normalised to (class, 64-bit word) such that two values are equal exactly when class and word are (n1k.h, at
// n1k_filter_device_batch):
//
//     MISSING 0, NULL 1, FALSE 2, TRUE 3                  word 0
//     INT 4                                               the int64; an integral FLOAT in int64 range is its INT (so -0.0 is INT 0)
//     FLOAT 5                                             the bits of every other double; all NaNs are 0x7FF8000000000000
//     STRING 6, ARRAY 7, OBJECT 8                         the dictionary code
//
// Three steps on the stream.  INSERT: a workgroup takes tiles of kRdTile survivors in ascending order and sends their rows to
// the global table.  Optionally (lds_slots > 0; off by default, DESIGN.md §4 has the measurement) a set in LDS ahead of it
// keeps, per key the workgroup has met, the smallest ordinal, and only that row goes on (a key the set has no room for sends
// all its rows on): the minimum over the workgroup's rows, not just any occurrence.  The global table is
// open-addressed, holds ordinals (kRdEmpty = free) and compares keys by reading the columns at the stored ordinal; equal keys
// settle on the smaller ordinal.  With no deletion a key never occupies two slots, and every probe loop is bounded by the
// slot count: a table with no room raises ERR_TABLE_FULL.  MARK: a survivor is a representative iff the slot its key was
// found in holds its own ordinal.  COMPACT: tile counts, their scan, the stable scatter.
#pragma once
#include <stdint.h>
#include "n1k_types.h"

namespace n1k {

constexpr uint32_t kRdMaxTerms = 4;
constexpr uint32_t kRdBlock = 256;
constexpr uint32_t kRdPer = 4;                     // survivors per thread and tile
constexpr uint32_t kRdTile = kRdBlock * kRdPer;    // survivors of a tile
constexpr uint32_t kRdEmpty = 0xFFFFFFFFu;         // a free slot; in slot_of: the row is no candidate
constexpr uint32_t kRdLdsMaxSlots = 4096;          // of the LDS set (8-byte words): 32 KiB
constexpr uint32_t kRdLdsProbes = 16;              // slots a row examines in the LDS set before it is passed on
constexpr uint64_t kRdMaxSlots = 0xFFFFFFFFull;    // slot indices are 32-bit words (slot_of), kRdEmpty is none of them

}  // namespace n1k

#if !defined(__HIPCC_RTC__)
#include <hip/hip_runtime.h>

namespace n1k {

struct RowDistinctArgs {
    const uint32_t* sel;     // the ascending selection; null: the identity (a plan without Filter: survivor i is row i)
    uint64_t n;              // survivors (< 2^32)
    uint32_t nterms;
    uint32_t lds_slots;      // slots of the LDS set (<= kRdLdsMaxSlots), 0: no pre-filter
    DevCol cols[kRdMaxTerms];
    uint32_t* table;         // `slots` ordinals, kRdEmpty when free
    uint64_t slots;          // any value in [1, kRdMaxSlots]
    uint32_t* slot_of;       // n words: INSERT leaves the slot of the survivor's key (kRdEmpty: the workgroup met a smaller
                             // ordinal of the key), MARK turns it into 1 (representative) / 0
    uint32_t* tile_count;    // ceil(n / kRdTile) + 1 words: the tiles' representatives, then their exclusive scan
    uint32_t* out;           // room for n ordinals
    unsigned long long* count;    // out: representatives
    unsigned long long* reached;  // added to: rows that went to the global table
    uint32_t* err_flags;
};

// All three steps, one after the other on `st`; grid: workgroups of the grid-stride loops over the tiles.
hipError_t launch_row_distinct(const RowDistinctArgs& A, uint32_t grid, hipStream_t st);

}  // namespace n1k
#endif
