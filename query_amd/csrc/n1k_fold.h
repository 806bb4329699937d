// n1k_fold.h — CumulateIntermediate over workgroup slabs (execution/group_intermediate.go:91-101), written once.
//
// A DIRECT-mode scan leaves every workgroup's LDS table in a slab; a slot's words in one slab are the LDS accumulator words
// of n1k_types.h (COUNT [cnt], SUM [isum][fsum][flags], AVG ... [n], MIN / MAX [flags][ival][fval][sval]).  Folding a slot
// over the slabs keeps, per aggregate, a running accumulator that IS the aggregate's words of a table row
// (COUNT [cnt], SUM [isum_lo][isum_hi][fsum][flags], AVG ... [n], MIN / MAX as in the slab):
//
//     fold_identity   the accumulator before any slab
//     fold_slab       one slab's words into the accumulator (SUM / AVG: the int sum is split into lo / hi here, so that
//                     768 partial sums of up to 2^63 each cannot overflow)
//     fold_word_op    how word i of two accumulators combines (partial folds of disjoint slab sets: lanes, waves, atomics)
//     fold_join       ... all words
//     fold_word_live  whether word i carries anything, given the accumulator's flags word: a word that is not live holds
//                     its identity, so a sink may skip it (the table's atomics) or store it as it is (a row in registers)
//     fold_row        accumulator -> the aggregate's row words
//
// Slabs a slot was never touched in carry the identities lds_table_init wrote (0, +0.0, INT64_MAX / INT64_MIN, ~0 / 0), which
// never win and add nothing: no slab needs to be skipped.  Any fixed fold order is allowed; float sums then differ within
// n * 2^-53 * sum|x|.  Host and device code, no HIP-only construct: merge_slabs_kernel and fold_rows_kernel
// (n1k_kernels.hip) and tests/host/fold_check.cpp compile it.
//
// Not written here: merge_slot (n1k_tables.h), the scan kernels' own flush of ONE LDS slot into its table row by atomics, for
// executions without slabs.  It is part of every scan kernel, those built at run time through hiprtc included, and a
// change to it changes them; it folds nothing over slabs (one slot, one row, each word one atomic), and stays as it is.
#pragma once
#include <stdint.h>
#include "n1k_types.h"

namespace n1k {

#if defined(__HIP__)
#define N1K_HD __host__ __device__ inline
#else
#define N1K_HD inline
#endif

enum : uint32_t { FOLD_ADD_U64 = 0, FOLD_ADD_F64, FOLD_OR, FOLD_MIN_I64, FOLD_MAX_I64, FOLD_MIN_U64, FOLD_MAX_U64 };
constexpr uint32_t kFoldMaxWords = 5;  // accumulator words of one aggregate at most (AVG)

N1K_HD constexpr uint64_t fold_word(uint32_t op, uint64_t a, uint64_t b) {
    switch (op) {
        case FOLD_ADD_U64: return a + b;
        case FOLD_ADD_F64: return __builtin_bit_cast(uint64_t, __builtin_bit_cast(double, a) + __builtin_bit_cast(double, b));
        case FOLD_OR: return a | b;
        case FOLD_MIN_I64: return (int64_t)a < (int64_t)b ? a : b;
        case FOLD_MAX_I64: return (int64_t)a > (int64_t)b ? a : b;
        case FOLD_MIN_U64: return a < b ? a : b;
        default: return a > b ? a : b;
    }
}

// words of the aggregate in a slab slot / in the accumulator (= in a table row)
N1K_HD constexpr uint32_t fold_slab_words(uint32_t kind) {
    return (kind == AGG_COUNT || kind == AGG_COUNTN) ? 1u : (kind == AGG_SUM ? kLdsWordsSum : (kind == AGG_AVG ? kLdsWordsAvg : kWordsMinMax));
}
N1K_HD constexpr uint32_t fold_acc_words(uint32_t kind) {
    return (kind == AGG_COUNT || kind == AGG_COUNTN) ? 1u : (kind == AGG_SUM ? kGlobWordsSum : (kind == AGG_AVG ? kGlobWordsAvg : kWordsMinMax));
}

N1K_HD constexpr uint32_t fold_word_op(uint32_t kind, uint32_t i) {
    switch (kind) {
        case AGG_COUNT:
        case AGG_COUNTN: return FOLD_ADD_U64;
        case AGG_SUM:
        case AGG_AVG: return i == 2 ? FOLD_ADD_F64 : (i == 3 ? FOLD_OR : FOLD_ADD_U64);
        case AGG_MIN: return i == 0 ? FOLD_OR : (i == 1 ? FOLD_MIN_I64 : FOLD_MIN_U64);
        default: return i == 0 ? FOLD_OR : (i == 1 ? FOLD_MAX_I64 : FOLD_MAX_U64);
    }
}

N1K_HD constexpr uint64_t fold_identity(uint32_t kind, uint32_t i) {
    if (kind == AGG_MIN) return i == 0 ? 0ull : (i == 1 ? (uint64_t)INT64_MAX : ~0ull);
    if (kind == AGG_MAX) return i == 1 ? (uint64_t)INT64_MIN : 0ull;
    return 0ull;  // counts, sums (+0.0), flags
}

// word i of the aggregate in a slab the slot was never touched in (what lds_table_init writes): folding it changes nothing
N1K_HD constexpr uint64_t fold_slab_identity(uint32_t kind, uint32_t i) { return (kind == AGG_MIN || kind == AGG_MAX) ? fold_identity(kind, i) : 0ull; }

// the accumulator word that holds the aggregate's flags (SF_* / MM_*); COUNT / COUNTN have none: the count itself
N1K_HD constexpr uint32_t fold_flags_word(uint32_t kind) { return (kind == AGG_SUM || kind == AGG_AVG) ? 3u : 0u; }

N1K_HD constexpr bool fold_word_live(uint32_t kind, uint32_t i, uint64_t flags) {
    switch (kind) {
        case AGG_COUNT:
        case AGG_COUNTN: return flags != 0;
        case AGG_SUM:
        case AGG_AVG: return i < 2 ? (flags & (SF_NONNEG_INT | SF_NEG_INT)) != 0 : (i == 2 ? (flags & SF_FLOAT) != 0 : flags != 0);
        default: return i == 0 ? flags != 0 : (i == 1 ? (flags & MM_INT) != 0 : (i == 2 ? (flags & MM_FLOAT) != 0 : (flags & MM_STRING) != 0));
    }
}

// l: the aggregate's fold_slab_words(kind) words of one slot of one slab
N1K_HD void fold_slab(uint32_t kind, uint64_t* acc, const uint64_t* l) {
    if (kind == AGG_SUM || kind == AGG_AVG) {
        const int64_t x = (int64_t)l[0];  // 0 when no int was added
        acc[0] += (uint64_t)(uint32_t)x;
        acc[1] += (uint64_t)(x >> 32);
        acc[2] = fold_word(FOLD_ADD_F64, acc[2], l[1]);  // +0.0 when no float was added
        acc[3] |= l[2];
        if (kind == AGG_AVG) acc[4] += l[3];
        return;
    }
    // COUNT / COUNTN / MIN / MAX: the slab's words are accumulator words
    const uint32_t n = fold_acc_words(kind);
    for (uint32_t i = 0; i < kFoldMaxWords; i++)
        if (i < n) acc[i] = fold_word(fold_word_op(kind, i), acc[i], l[i]);
}

N1K_HD void fold_init(uint32_t kind, uint64_t* acc) {
    for (uint32_t i = 0; i < kFoldMaxWords; i++) acc[i] = fold_identity(kind, i);
}

N1K_HD void fold_join(uint32_t kind, uint64_t* acc, const uint64_t* other) {
    const uint32_t n = fold_acc_words(kind);
    for (uint32_t i = 0; i < kFoldMaxWords; i++)
        if (i < n) acc[i] = fold_word(fold_word_op(kind, i), acc[i], other[i]);
}

// row: the aggregate's words of a table row (glob_off applied by the caller).  Words that are not live hold their identity,
// which is what glob_row_init writes: the row is the accumulator.
N1K_HD void fold_row(uint32_t kind, const uint64_t* acc, uint64_t* row) {
    const uint32_t n = fold_acc_words(kind);
    for (uint32_t i = 0; i < kFoldMaxWords; i++)
        if (i < n) row[i] = acc[i];
}

}  // namespace n1k
