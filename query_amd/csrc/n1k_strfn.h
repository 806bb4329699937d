// n1k_strfn.h — string functions in a condition (expression/func_str.go): the fourth kind of the match table.
//
// A term such as `(lower(trim(x)) = "cat_1")`, `contains(x, "amazon")` or `(position1(x, "a") < 3)` is a pure function of
// ONE dictionary string with the 4-valued profile of LIKE: MISSING for MISSING, NULL for a non-STRING, a plain boolean for a
// STRING.  So it is one more predicate over dictionary entries: compiled once per plan into a StrFnProg, evaluated once per
// distinct entry into the predicate's bit, and the row test is LIKE's as it stands.
//
// The program: up to kStrFnMaxSteps steps (innermost first) — lower, upper (func_str.go:204, :1155), trim / ltrim / rtrim
// with a cutset (func_str.go:255-275, :672-676, :1085-1089; default " \t\n\f\r", :301) — and one terminal: a comparison with
// STRING constants, contains (func_str.go:81), positionN + a comparison with NUMBER constants (func_str.go:1168-1177), or
// LIKE (the like_compile program, n1k_like.h).
//
// strfn_eval is what both the host and strfn_match_kernel run.  It never copies the string: it keeps a view {begin, end,
// case mode}.  A trim step moves the ends, reading bytes through the case mode in force at that step; a case step sets the
// mode (for ASCII the last one wins); the terminal reads bytes through the mode.
//
// Case mapping without Unicode tables.  Go maps rune by rune through unicode.ToLower / ToUpper (simple case mapping).  Under
// a case step every constant of the predicate is pure ASCII (strfn_compile refuses anything else).  Only four non-ASCII runes
// have a simple case mapping INTO ASCII: U+0130 -> i and U+212A -> k under lower, U+017F -> S and U+0131 -> I under upper.
// Every other non-ASCII rune maps to a non-ASCII rune, an invalid byte becomes U+FFFD: neither can equal, contain or sort
// below an ASCII byte, neither is in an ASCII cutset, and each is still exactly one character for `_` and `%`.  So bytes
// >= 0x80 are left untouched and the answer is still Go's — except for an entry that holds one of the four runes under the
// matching case step (strfn_needs_host), which the host evaluates over the mapped runes (strfn_eval_host).  An entry that is
// not valid UTF-8 under LIKE goes to the host too, as LIKE's own matcher has it.
// (The four-rune fact is read off the Unicode simple case mappings; it is not checked against a Go toolchain.)
#pragma once
#include "n1k_like.h"

namespace n1k {

constexpr uint32_t kStrFnMaxSteps = 4;      // functions nested around the path
constexpr uint32_t kStrFnPoolBytes = 256;   // constants of one predicate: cutsets, compare constants, needle, LIKE pattern text
constexpr uint32_t kStrFnDevMaxLen = 128;   // bytes of a dictionary string the device kernel takes: LIKE's, the same 8 KiB slab a wave
// New dictionary entries from which the device route is taken: LIKE's figure (n1k_like.h).  Measured through the handle
// ("String functions: measured", tools/exp_strfn.py route; strings of 29 B, one predicate with two steps and a
// LIKE): the host route costs 0.047 ms for 256 new strings and 0.111 ms for 1023, the device route 0.135 ms for 1 Ki, 0.141
// for 4 Ki, 0.185 for 16 Ki — the two cross near 1.25 Ki.  Kept at 1024: at worst 0.024 ms more, once.
constexpr uint32_t kStrFnDeviceThreshold = kLikeDeviceThreshold;

enum : uint8_t { SF_LOWER = 0, SF_UPPER, SF_TRIM, SF_LTRIM, SF_RTRIM };
enum : uint8_t { SFT_CMP = 0, SFT_CONTAINS, SFT_POS, SFT_LIKE };                      // the terminal
enum : uint8_t { SFC_EQ = 0, SFC_LT, SFC_LE, SFC_GT, SFC_GE, SFC_BETWEEN };           // its comparison (SFT_CMP, SFT_POS)
enum : uint8_t { SFM_NONE = 0, SFM_LOWER, SFM_UPPER };                                // case mode of the view

struct StrFnStep {
    uint8_t fn, pad;
    uint16_t cut_off, cut_len;  // SF_*TRIM: the cutset in the pool
};

// One predicate, the same struct on host and device (zero-filled where unused: equal programs are equal bytes).
struct StrFnProg {
    uint8_t nsteps, term, cmp, anchor_end;
    uint8_t has_lower, has_upper, start_pos, like_len;  // like_len: bytes of like_prog
    StrFnStep steps[kStrFnMaxSteps];                    // innermost first
    uint16_t c_off[2], c_len[2];                        // SFT_CMP: the constant(s); SFT_CONTAINS / SFT_POS: [0] the needle
    double num[2];                                      // SFT_POS: the NUMBER constant(s)
    uint8_t pool[kStrFnPoolBytes];
    uint8_t like_prog[kLikeDevProgBytes];
};
static_assert(sizeof(StrFnProg) == 552 && sizeof(StrFnProg) % 8 == 0, "StrFnProg layout");

N1K_HD uint8_t strfn_map(uint8_t c, uint8_t mode) {
    if (mode == SFM_LOWER) return (uint8_t)(c >= 'A' && c <= 'Z' ? c + 32 : c);
    if (mode == SFM_UPPER) return (uint8_t)(c >= 'a' && c <= 'z' ? c - 32 : c);
    return c;
}

N1K_HD bool strfn_in_set(uint8_t c, const uint8_t* set, uint32_t n) {
    for (uint32_t k = 0; k < n; k++)
        if (set[k] == c) return true;
    return false;
}

// Does the entry hold what only the host evaluates: one of the four runes under the matching case step (C4 B0, E2 84 AA
// under lower; C5 BF, C4 B1 under upper — none of these lead bytes can be a continuation byte, so a scan over bytes finds
// exactly what a decoder finds), or, under LIKE, bytes that are not valid UTF-8?
N1K_HD bool strfn_needs_host(const StrFnProg& g, const uint8_t* s, uint32_t n) {
    if (g.has_lower || g.has_upper)
        for (uint32_t i = 0; i + 1 < n; i++) {
            const uint8_t c = s[i], d = s[i + 1];
            if (g.has_lower && ((c == 0xC4 && d == 0xB0) || (c == 0xE2 && d == 0x84 && i + 2 < n && s[i + 2] == 0xAA))) return true;
            if (g.has_upper && ((c == 0xC4 && d == 0xB1) || (c == 0xC5 && d == 0xBF))) return true;
        }
    return g.term == SFT_LIKE && !like_utf8_valid(s, n);
}

// the view as like_match reads it (valid UTF-8; literals of a pattern under a case step are ASCII)
struct StrFnText {
    const uint8_t* s;
    uint32_t n;
    uint8_t mode;
    N1K_HD uint32_t next(uint32_t p) const { return p + like_utf8_len(s[p]); }
    N1K_HD bool newline(uint32_t p) const { return s[p] == '\n'; }
    N1K_HD uint32_t lit(uint32_t p, const uint8_t* b, uint32_t len) const {
        if (len > n - p) return 0xFFFFFFFFu;
        for (uint32_t k = 0; k < len; k++)
            if (strfn_map(s[p + k], mode) != b[k]) return 0xFFFFFFFFu;
        return p + len;
    }
};

// bytewise order of the view against a constant: < 0, 0, > 0 (strings compare bytewise, value/string.go:116-130)
N1K_HD int strfn_collate(const uint8_t* s, uint32_t n, uint8_t mode, const uint8_t* c, uint32_t clen) {
    const uint32_t m = n < clen ? n : clen;
    for (uint32_t i = 0; i < m; i++) {
        const uint8_t x = strfn_map(s[i], mode);
        if (x != c[i]) return x < c[i] ? -1 : 1;
    }
    return n < clen ? -1 : (n > clen ? 1 : 0);
}

// strings.Index over the view: the first byte offset of the needle, -1 if there is none (0 for the empty needle)
N1K_HD int32_t strfn_index(const uint8_t* s, uint32_t n, uint8_t mode, const uint8_t* c, uint32_t clen) {
    if (clen > n) return -1;
    for (uint32_t i = 0; i + clen <= n; i++) {
        uint32_t k = 0;
        while (k < clen && strfn_map(s[i + k], mode) == c[k]) k++;
        if (k == clen) return (int32_t)i;
    }
    return -1;
}

N1K_HD bool strfn_cmp_holds(uint8_t cmp, int lo, int hi) {  // lo: value against constant 0; hi: against constant 1 (BETWEEN)
    switch (cmp) {
        case SFC_EQ: return lo == 0;
        case SFC_LT: return lo < 0;
        case SFC_LE: return lo <= 0;
        case SFC_GT: return lo > 0;
        case SFC_GE: return lo >= 0;
        default: return lo >= 0 && hi <= 0;
    }
}

// the terminal over the view s[0, n) read through `mode`
N1K_HD bool strfn_terminal(const StrFnProg& g, const uint8_t* s, uint32_t n, uint8_t mode) {
    const uint8_t* c0 = g.pool + g.c_off[0];
    switch (g.term) {
        case SFT_CMP: {
            const int lo = strfn_collate(s, n, mode, c0, g.c_len[0]);
            const int hi = g.cmp == SFC_BETWEEN ? strfn_collate(s, n, mode, g.pool + g.c_off[1], g.c_len[1]) : 0;
            return strfn_cmp_holds(g.cmp, lo, hi);
        }
        case SFT_CONTAINS: return strfn_index(s, n, mode, c0, g.c_len[0]) >= 0;
        case SFT_POS: {
            const double v = (double)(strfn_index(s, n, mode, c0, g.c_len[0]) + (int32_t)g.start_pos);
            const int lo = v < g.num[0] ? -1 : (v > g.num[0] ? 1 : 0);
            const int hi = v < g.num[1] ? -1 : (v > g.num[1] ? 1 : 0);
            return strfn_cmp_holds(g.cmp, lo, hi);
        }
        default: return like_match(g.like_prog, g.like_len, g.anchor_end != 0, StrFnText{s, n, mode});
    }
}

// The predicate over the dictionary string s[0, n) — for an entry strfn_needs_host does not claim.
N1K_HD bool strfn_eval(const StrFnProg& g, const uint8_t* s, uint32_t n) {
    uint32_t b = 0, e = n;
    uint8_t mode = SFM_NONE;
    for (uint32_t k = 0; k < g.nsteps; k++) {
        const StrFnStep& st = g.steps[k];
        if (st.fn == SF_LOWER) mode = SFM_LOWER;
        else if (st.fn == SF_UPPER) mode = SFM_UPPER;
        else {
            const uint8_t* set = g.pool + st.cut_off;
            if (st.fn != SF_RTRIM)
                while (b < e && strfn_in_set(strfn_map(s[b], mode), set, st.cut_len)) b++;
            if (st.fn != SF_LTRIM)
                while (e > b && strfn_in_set(strfn_map(s[e - 1], mode), set, st.cut_len)) e--;
        }
    }
    return strfn_terminal(g, s + b, e - b, mode);
}

struct StrFnKernelArgs {
    EntryBlockArgs blk;      // out_bits: bit first_bit + q = predicate q holds; left: longer than kStrFnDevMaxLen, or strfn_needs_host
    uint32_t nprog, first_bit;
    const StrFnProg* progs;  // device memory
};

}  // namespace n1k

#if !defined(__HIPCC_RTC__)
#include <hip/hip_runtime.h>
#include <string>
#include <vector>

namespace n1k {

struct Expr;
struct PlanError;

struct StrFnPred {
    StrFnProg prog;
};

// Is this function name one of the string functions a term may hold (a step or a terminal)?
bool strfn_name(const std::string& fname);
// Does the condition node e hold a string function where a term may: contains / positionN itself, or a comparison,
// BETWEEN or LIKE with a string function on either side?
bool strfn_term(const Expr* e);
// One term -> program and the leaf path it reads.  false + err (unsupported, the construct named) for what lies outside
// the subset.
bool strfn_compile(const Expr* e, StrFnProg& out, const Expr*& path, PlanError& err);
// one string against one predicate, any bytes (the host matcher: what strfn_needs_host claims goes over the mapped runes)
bool strfn_eval_host(const StrFnProg& g, const uint8_t* s, size_t n);
// bits[i] |= OR over predicates q of (holds << (first_bit + q))
void strfn_eval_block_host(const std::vector<StrFnPred>& preds, uint32_t first_bit, uint64_t n, const uint64_t* offsets, const uint8_t* bytes, uint8_t* bits);
hipError_t launch_strfn_match(const StrFnKernelArgs& A, hipStream_t st);

}  // namespace n1k
#endif
