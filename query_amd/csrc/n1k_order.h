// n1k_order.h — ORDER BY over the rows a Filter-only plan selects (execution/order.go:121-169): the order key both sides
// compile, and the launch interface between n1k_order.cpp and n1k_order.hip.
//
// order_key maps one value of a sort term to (64-bit key, 16-bit residual) such that comparing (key, residual) as unsigned
// integers IS value.Collate with an INT and a FLOAT compared exactly — injective up to Collate's ties, where order_image
// (the grouped tail's top-k filter) drops three mantissa bits.  The sortable form of the finite doubles and the infinities
// leaves the words below the image of -inf and above the image of +inf free; the other type classes live there:
//
//     MISSING 0, NULL 1, FALSE 2, TRUE 3, NaN 4          (NaN before every number: value/float.go:123-172)
//     number   sortable(float64 of the value), either zero as +0.0: 0x000FFFFFFFFFFFFF (-inf) .. 0xFFF0000000000000 (+inf)
//     STRING   0xFFF0000000000001 + bytewise rank of its dictionary code
//     ARRAY / OBJECT  no key (unsupported: the caller raises ERR_UNSUPPORTED_VALUE)
//
// The residual of an INT a is a - (the exact value of (double)a), biased by kOrdResBias: non-zero only beyond +-2^53, at most
// 512 in magnitude; the bias itself for everything else.  DESC complements key and residual.
#pragma once
#include <stdint.h>
#include "n1k_types.h"

namespace n1k {

#if defined(__HIP__)
#define N1K_HD __host__ __device__ inline
#else
#define N1K_HD inline
#endif

constexpr uint32_t kOrdMaxTerms = 4;     // == kOrderMaxTerms (n1k_plan.h)
constexpr uint32_t kOrdKeyDigits = 8;    // 8-bit digits of the key, digit 0 the least significant
constexpr uint32_t kOrdDigits = 10;      // ... followed by the two of the residual
constexpr uint32_t kOrdHists = kOrdMaxTerms + 1;  // the terms' histograms + those of the selection position (the select route)
constexpr uint32_t kOrdTile = 4096;      // elements of a sort tile: 4 waves x 16 rounds x 64 lanes
constexpr uint32_t kOrdBlock = 256;
constexpr uint32_t kOrdRounds = kOrdTile / kOrdBlock;

constexpr uint64_t kOrdKeyMissing = 0, kOrdKeyNull = 1, kOrdKeyFalse = 2, kOrdKeyTrue = 3, kOrdKeyNaN = 4;
constexpr uint64_t kOrdKeyPosInf = 0xFFF0000000000000ull;  // sortable(+inf)
constexpr uint64_t kOrdKeyString = kOrdKeyPosInf + 1;
constexpr uint32_t kOrdResBias = 1024;

struct OrderKey {
    uint64_t key;
    uint32_t res;      // 16 bits
    uint32_t unsupported;
};

N1K_HD uint64_t ord_sortable(double d) {  // d is no NaN
    const uint64_t b = __builtin_bit_cast(uint64_t, d);
    return (b & 0x8000000000000000ull) ? ~b : (b | 0x8000000000000000ull);
}

// rank: the bytewise rank of the string's dictionary code (read by the caller for a STRING only)
N1K_HD OrderKey order_key(uint32_t tag, uint64_t p, uint32_t rank, bool desc) {
    OrderKey k{0, kOrdResBias, 0};
    switch (tag) {
        case T_MISSING: k.key = kOrdKeyMissing; break;
        case T_NULL: k.key = kOrdKeyNull; break;
        case T_FALSE: k.key = kOrdKeyFalse; break;
        case T_TRUE: k.key = kOrdKeyTrue; break;
        case T_INT: {
            const int64_t a = (int64_t)p;
            const double d = (double)a;  // round to nearest even; INT 0 gives +0.0
            k.key = ord_sortable(d);
            // (double)INT64_MAX is 2^63, which no int64 holds: the difference is taken in unsigned arithmetic
            const uint64_t back = d >= 9223372036854775808.0 ? (1ull << 63) : (uint64_t)(int64_t)d;
            k.res = (uint32_t)((int64_t)((uint64_t)a - back) + (int64_t)kOrdResBias);
            break;
        }
        case T_FLOAT: {
            const double d = __builtin_bit_cast(double, p);
            k.key = d != d ? kOrdKeyNaN : ord_sortable(d == 0.0 ? 0.0 : d);
            break;
        }
        case T_STRING: k.key = kOrdKeyString + rank; break;
        default:
            k.key = ~0ull;
            k.unsupported = 1;
            break;
    }
    if (desc) {
        k.key = ~k.key;
        k.res = ~k.res & 0xFFFFu;
    }
    return k;
}

}  // namespace n1k

// ---------------------------------------------------------------------------------------------------------------------------
// launch interface (n1k_order.hip)
#if !defined(__HIPCC_RTC__)
#include <hip/hip_runtime.h>

namespace n1k {

// Keys of the survivors.  Survivor i is position pos = cand ? cand[i] : i of the ascending selection `rows`, row rows[pos] of
// the batch.  Term t reads cols[t] at that row; its key goes to key[t][i] and its residual to res[t][i] when bit t of `store`
// is set (every term is evaluated either way: an ARRAY / OBJECT raises the flag whatever is stored).  pos_term: key[nterms][i]
// = pos, one more — least significant — term.  hist (or null): the 256-bin histograms of all kOrdDigits digits of every term,
// [term][digit][bin], added to.
struct OrderKeyArgs {
    const uint32_t* rows;
    const uint32_t* cand;
    uint64_t n;
    uint32_t nterms, store, pos_term, pad;
    DevCol cols[kOrdMaxTerms];
    uint32_t desc[kOrdMaxTerms];
    uint64_t* key[kOrdHists];
    uint16_t* res[kOrdMaxTerms];
    const uint32_t* str_rank;
    uint32_t* hist;
    uint32_t* err_flags;
};
hipError_t launch_order_keys(const OrderKeyArgs& A, uint32_t grid, hipStream_t st);

// out[i] = key[perm[i]] (res: the 16-bit residual widened instead); perm null: the identity
hipError_t launch_order_gather(const uint64_t* key, const uint16_t* res, const uint32_t* perm, uint64_t n, uint64_t* out, hipStream_t st);

// One stable pass of the LSD radix sort over pairs (64-bit key, 32-bit position) on the 8-bit digit at `shift`: per-tile
// histograms, their scan (digit-major, so one exclusive scan gives every tile's output offset per digit; ghist: the digit's
// 256 totals over all n keys), the scatter.  vin null: position i is i.  kout null: the keys are not needed any more.
// tile_hist: 256 * ceil(n / kOrdTile) words.
hipError_t launch_order_pass(const uint64_t* kin, const uint32_t* vin, uint64_t* kout, uint32_t* vout, uint64_t n, uint32_t shift,
                             const uint32_t* ghist, uint32_t* tile_hist, uint32_t grid, hipStream_t st);

// out[i - first] = rows[pos(perm[i])] for first <= i < last; pos(j) = cand ? cand[j] : j; perm null: the identity
hipError_t launch_order_finish(const uint32_t* rows, const uint32_t* cand, const uint32_t* perm, uint64_t first, uint64_t last,
                               uint32_t* out, hipStream_t st);

}  // namespace n1k
#endif
