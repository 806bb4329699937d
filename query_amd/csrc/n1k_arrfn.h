// n1k_arrfn.h — the scalar functions over arrays whose result is a number, a boolean, NULL or MISSING
// (expression/func_array.go): array_length (:888-897), array_count (:376-393), array_sum (:1911-1928), array_avg
// (:141-164), array_contains (:307-323), array_position (:1094-1110), over a leaf path of the row.
//
// An ARRAY value on this path is a dictionary code whose entry is the array's canonical JSON text, so the function's
// result is a function of the code: it is computed once per distinct array into the term's VALUE TABLE — one tag byte
// and one 8-byte payload per dictionary code — and a row reads its entry (arrfn_lookup_kernel).  This is the match
// table's value-shaped sibling (n1k_coll.h: ANY / EVERY keeps one bit per entry), with its cursor functions.
//
// arrfn_eval<HOST> is the one algorithm.  Elements are typed as func_array.go types them: value.NewValue(x) over
// arg.Actual().([]interface{}) — the array went through encoding/json into interface{}, so EVERY number is a float64
// first (value/parsed.go:120-122, 362) and NewValue folds an integral one to int64 (value/value.go:367-381).  An integer
// that float64 does not hold exactly (2^53 + 1) is therefore the int64 of its ROUNDED float64; coll_number (n1k_coll.h)
// would keep it exact.  What only the host does (HOST = true) and the device flags for it (`left`), per function:
//   array_length, array_count                   nothing: they neither read a number nor decode a string
//   array_sum, array_avg, and array_contains / array_position with a NUMBER constant: a number beyond coll_number's exact
//     conversions (over 18 digits; over 15 digits or |e10| > 22 with a fraction), and an integer in the text that is
//     not exactly a float64 (the host types both through strtod, as the reference's decoder does)
//   array_contains / array_position with a STRING constant: a STRING element with a backslash escape that the walk
//     reaches (the host decodes it)
// array_sum adds with num_add (n1k_device.h: value/integer.go:266-352, INT-exact until overflow), the code arith_apply's
// AR_ADD runs, from INT 0 and left to right.
#pragma once
#include "n1k_coll.h"

namespace n1k {

enum : uint8_t { AF_LENGTH = 0, AF_COUNT, AF_SUM, AF_AVG, AF_CONTAINS, AF_POSITION, AF_COUNT_FNS };

constexpr uint32_t kArrFnMaxTerms = 4;     // distinct array-function terms of one plan
constexpr uint32_t kArrFnConstBytes = 104; // bytes of a STRING constant (the program is 128 bytes: four fit 512 B of LDS)
// New dictionary entries from which the device route is taken.  Measured ("Array functions: measured",
// tools/exp_arrfn.py route; arrays of 23 B, two terms): the host route costs 0.035 ms for 1 Ki new arrays, 0.123 for 4 Ki, 1.94
// for 64 Ki; the device route 0.22 ms up to 4 Ki and 0.49 for 64 Ki — a fixed 0.2 ms, which the host route reaches at about
// 7 Ki arrays.  LIKE's and ANY / EVERY's 1024 is more than 2 x off that, so the feature has its own constant.
constexpr uint32_t kArrFnDeviceThreshold = 8192;

struct ArrFnProg {
    uint8_t fn;     // AF_*
    uint8_t ctag;   // AF_CONTAINS / AF_POSITION: T_INT / T_FLOAT / T_STRING / T_TRUE / T_FALSE, or T_NULL / T_MISSING
    uint16_t clen;  // STRING constant: its bytes
    uint32_t pad;
    uint64_t c;     // NUMBER constant: int64 or float64 bits
    uint8_t cstr[kArrFnConstBytes];
    uint8_t pad2[8];
};
static_assert(sizeof(ArrFnProg) == 128, "ArrFnProg layout");

struct ArrFnKernelArgs {
    const uint8_t* bytes;     // the block's bytes (+ 4 spare: whole words are staged)
    const uint64_t* offsets;  // n + 1
    uint32_t n, nprog;
    const ArrFnProg* progs;   // nprog programs (device memory)
    uint8_t* out_tags;        // term q: out_tags[q * stride + i], out_payload[q * stride + i]
    uint64_t* out_payload;
    uint64_t stride;
    uint8_t* out_left;        // [n]: 1 = some term of this entry is left to the host evaluator (its slots hold NULL)
};

// One lookup per row: the operand column's (tag, payload) -> the term's value.
struct ArrFnLookupArgs {
    DevCol col;               // the operand: an input column
    const uint8_t* tab_tags;  // the term's value table, tab_n entries
    const uint64_t* tab_payload;
    uint32_t tab_n, pad;
    uint64_t nrows;
    // which of the nrows rows the batch really holds (CondArgs, n1k_cond.h)
    const unsigned long long* nrows_dev;
    const unsigned long long* seg_counts;
    uint64_t seg_rows;
    uint32_t nseg, pad2;
    uint8_t* out_tags;
    uint64_t* out_payload;
};

#if defined(N1K_ARRFN_EVAL)
// (the evaluator itself: only the unit that holds both of its flavours, n1k_arrfn.hip, compiles it — it needs n1k_device.h)

// does an integer typed exactly (coll_number's integral branch) survive the float64 the reference's decoder makes of it?
N1K_HD bool arrfn_int_is_f64(int64_t v) {
    const double d = (double)v;
    return d >= -9223372036854775808.0 && d < 9223372036854775808.0 && (int64_t)d == v;
}

#if !defined(__HIP_DEVICE_COMPILE__)
int arrfn_number_host(const uint8_t* s, uint32_t b, uint32_t e, uint32_t& tag, uint64_t& payload);  // strtod, then NewValue(float64)
#endif

// The NUMBER element s[b, e) as NewValue(float64) types it.  false: left to the host.
template <bool HOST>
N1K_HD bool arrfn_number(const uint8_t* s, uint32_t b, uint32_t e, uint32_t& tag, uint64_t& payload) {
    int r = coll_number(s, b, e, tag, payload);
    if (r == 1 && tag == T_INT && !arrfn_int_is_f64((int64_t)payload)) r = 2;
#if !defined(__HIP_DEVICE_COMPILE__)
    if (HOST && r != 1) r = arrfn_number_host(s, b, e, tag, payload);
#endif
    return r == 1;
}

// constant.Equals(element).Truth() for the element s[b, e) of tag `vt` (value/integer.go:68-87, float.go:74-93,
// string.go:82-96, boolean.go:74-88): FALSE across types, INT with INT exactly, else through float64 (NaN equals nothing)
template <bool HOST>
N1K_HD bool arrfn_equals(const ArrFnProg& g, const uint8_t* s, uint32_t n, uint32_t vt, uint32_t b, uint32_t e, bool& left) {
    const uint32_t ct = g.ctag;
    if (ct == T_TRUE || ct == T_FALSE) return vt == ct;
    if (ct == T_STRING) {
        if (vt != T_STRING) return false;
        bool esc;
        const uint32_t q = coll_skip_string(s, n, b, esc);
        CollStr v;
        if (q <= b + 1 || !coll_string<HOST>(s, b + 1, q - 1, esc, v)) {
            left = true;
            return false;
        }
        const bool eq = v.n == g.clen && coll_bytes_collate(v.p, v.n, g.cstr, g.clen) == 0;
        coll_string_done(v);
        return eq;
    }
    if (vt != T_INT) return false;  // (coll_tag_at: T_INT stands for any NUMBER)
    uint32_t nt = T_INT;
    uint64_t np = 0;
    if (!arrfn_number<HOST>(s, b, e, nt, np)) {
        left = true;
        return false;
    }
    if (nt == T_INT && ct == T_INT) return np == g.c;
    return num_actual(nt, np) == num_actual(ct, g.c);
}

// The function over the array whose canonical text is s[0, n) (coll_array_text holds) -> (tag, payload).  left: this side
// could not decide; the result is then not meaningful.
template <bool HOST>
N1K_HD void arrfn_eval(const ArrFnProg& g, const uint8_t* s, uint32_t n, uint32_t& tag, uint64_t& payload, bool& left) {
    tag = T_NULL;
    payload = 0;
    const bool binary = g.fn == AF_CONTAINS || g.fn == AF_POSITION;
    if (binary && g.ctag <= T_NULL) {  // (the first argument is present: MISSING for a MISSING constant, NULL for a NULL one)
        tag = g.ctag;
        return;
    }
    uint32_t p = 1, length = 0, count = 0, numbers = 0;
    Num sum = num_int(0);
    bool found = false;
    while (p < n && s[p] != ']') {
        const uint32_t q = coll_skip_value(s, n, p);
        if (q <= p) break;  // (malformed text: no progress)
        const uint32_t vt = coll_tag_at(s, p, q);
        if (g.fn == AF_COUNT) count += vt > T_NULL ? 1u : 0u;
        else if (g.fn == AF_SUM || g.fn == AF_AVG) {
            if (vt == T_INT) {
                uint32_t nt = T_INT;
                uint64_t np = 0;
                if (!arrfn_number<HOST>(s, p, q, nt, np)) {
                    left = true;
                    return;
                }
                sum = num_add(sum, Num{nt, np});
                numbers++;
            }
        } else if (binary) {
            if (arrfn_equals<HOST>(g, s, n, vt, p, q, left)) {
                found = true;
                break;
            }
            if (left) return;
        }
        length++;
        p = q;
        if (p < n && s[p] == ',') p++;
    }
    switch (g.fn) {
        case AF_LENGTH: tag = T_INT; payload = length; break;
        case AF_COUNT: tag = T_INT; payload = count; break;
        case AF_SUM: tag = sum.tag; payload = sum.p; break;
        case AF_AVG:
            if (numbers) {  // value.NewValue(sum.Actual().(float64) / float64(count))
                const Num r = num_new_value(num_actual(sum.tag, sum.p) / (double)numbers);
                tag = r.tag;
                payload = r.p;
            }
            break;
        case AF_CONTAINS: tag = found ? T_TRUE : T_FALSE; break;
        default: tag = T_INT; payload = found ? (uint64_t)length : (uint64_t)(int64_t)-1; break;
    }
}
#endif

}  // namespace n1k

#if !defined(__HIPCC_RTC__)
#include <string>
#include <vector>

namespace n1k {

struct Expr;
struct PlanError;

struct ArrFnTerm {
    std::string text;  // the whole term as the stringer wrote it
    ArrFnProg prog;
};

// Is this function name one of the six?  (n1k_plan.cpp has checked the shape of the arguments.)
bool arrfn_name(const std::string& f);
// An EK::Func over one of the six names -> program.  false + err (unsupported, the construct named).
bool arrfn_compile(const Expr* e, ArrFnProg& out, PlanError& err);
// tags[q * stride + i], payload[q * stride + i] = term q over entry i; an entry that is no array text gets NULL
void arrfn_eval_block_host(const ArrFnProg* progs, uint32_t nprog, uint64_t n, const uint64_t* offsets, const uint8_t* bytes, uint8_t* tags,
                           uint64_t* payload, uint64_t stride);
hipError_t launch_arrfn_table(const ArrFnKernelArgs& A, hipStream_t st);
hipError_t launch_arrfn_lookup(const ArrFnLookupArgs& A, hipStream_t st);

}  // namespace n1k
#endif
