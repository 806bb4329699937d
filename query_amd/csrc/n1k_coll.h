// n1k_coll.h — ANY / EVERY / ANY AND EVERY `v` IN <array> SATISFIES <P> END (expression/coll_any.go, coll_every.go,
// coll_any_every.go): the predicate program and the evaluator both the host and the device run.
//
// The reference evaluates the binding expression per row, then <P> once per element with `v` bound to it, and folds:
// ANY is TRUE at the first element whose P(v).Truth() holds, EVERY is FALSE at the first whose does not, an empty array
// makes ANY FALSE and EVERY TRUE, ANY AND EVERY is EVERY but `n > 0` at the end (coll_any_every.go:84).  When the
// binding expression is a column and <P> names nothing but `v` and constants, the answer is a function of the ARRAY
// alone — of its canonical JSON text, which is what the dictionary holds for an N1K_T_ARRAY value.  So it is computed
// once per distinct array into one bit of the match table LIKE already keeps (n1k_like.h), and a row tests that bit.
//
// A predicate compiles once into at most kCollMaxNodes nodes in post order (children before parents): AND / OR / NOT
// over leaves `<e> cmp constant`, `<e> between c and c`, `<e> like "pattern"`, `<e> is [not] null|missing|valued`, with
// <e> the variable followed by at most two field names.  The 4-valued result of node i lives in bits [2i, 2i + 1] of ONE
// 32-bit word, so the fold needs neither a stack nor an array.  Field names, STRING constants and LIKE programs lie in
// the program's byte pool.
//
// coll_eval<HOST> is the one algorithm.  It walks the top-level elements of the text with a cursor; a value is skipped
// by counting brackets outside strings (canonical text is well formed, so a counter does what a stack of bracket kinds
// does for the document extractor — no depth limit); a field is found by walking the members of an object (canonical
// text has each name once).  What only the host does (HOST = true) and the device flags for it (`left`):
//   a compared / matched string or a member name with a backslash escape (the host decodes it),
//   a compared number beyond the exact conversions (over 18 digits; over 15 digits or |e10| > 22 with a fraction — the
//   limits of n1k_jsondev.hip's scan_number; the host calls strtod),
//   a string under LIKE that is not valid UTF-8.
#pragma once
#include "n1k_like.h"

namespace n1k {

enum : uint8_t { COLL_ANY = 0, COLL_EVERY = 1, COLL_ANY_EVERY = 2 };
enum : uint8_t {
    CN_AND = 0, CN_OR, CN_NOT,                 // a, b: child nodes (NOT: a)
    CN_EQ, CN_LT, CN_LE, CN_BETWEEN, CN_LIKE,  // leaves over <e> and the node's constant(s)
    CN_IS_NULL, CN_IS_NOT_NULL, CN_IS_MISSING, CN_IS_NOT_MISSING, CN_IS_VALUED, CN_IS_NOT_VALUED
};

constexpr uint32_t kCollMaxNodes = 16;    // 2 bits each in one 32-bit word
constexpr uint32_t kCollPoolBytes = 256;  // field names + STRING constants + LIKE programs of one predicate
constexpr uint32_t kCollMaxFields = 2;
// Bytes of canonical text the device kernel takes.  A wave stages the text of its 64 entries in LDS: 64 x 192 B = 12 KiB
// a wave, 48 KiB for the four waves of a workgroup, 7 KiB for the programs — 55 KiB, under the 64 KiB a workgroup may
// declare, and two workgroups fit the CU's 160 KiB with 50 KiB to spare.  256 B would need 71 KiB.
constexpr uint32_t kCollDevMaxLen = 192;
// New dictionary entries from which the device route is taken: LIKE's figure (n1k_like.h) until this one is measured.
constexpr uint32_t kCollDeviceThreshold = kLikeDeviceThreshold;

struct CollNode {
    uint8_t op;
    uint8_t a, b;         // AND / OR / NOT: child nodes
    uint8_t flip;         // CN_LT / CN_LE: 1 = the constant is the FIRST operand ("(10 < `v`)")
    uint8_t nf;           // field names behind the variable
    uint8_t ctag, ctag2;  // tag of the constant (BETWEEN: low, high): T_FALSE / T_TRUE / T_INT / T_FLOAT / T_STRING
    uint8_t anchor_end;   // CN_LIKE
    uint16_t f_off[kCollMaxFields], f_len[kCollMaxFields];  // field names in the pool
    uint16_t c_off, c_len, c2_off, c2_len;                  // STRING constant / LIKE program in the pool (BETWEEN: low, high)
    uint64_t c, c2;       // NUMBER constant: int64 or float64 bits
};

struct CollProg {
    uint32_t nn;    // nodes; the last one is the root
    uint32_t mode;  // COLL_*
    uint32_t has_like, pad;
    CollNode node[kCollMaxNodes];
    uint8_t pool[kCollPoolBytes];
};

struct CollKernelArgs {
    EntryBlockArgs blk;          // out_bits: 0 for an entry that is no array text, and for one left to the host evaluator
    uint32_t nprog, first_bit;   // program q writes bit first_bit - q
    const CollProg* progs;       // nprog programs (device memory)
};

// Is this dictionary entry array text?  The dictionary does not record tags: canonical text of an array begins with '['
// and has its ']', so at least 2 bytes.  (A STRING that begins with '[' passes too; no row with tag STRING reads its bits.)
N1K_HD bool coll_array_text(const uint8_t* s, uint64_t len) { return len >= 2 && s[0] == '['; }

// ---- the cursor

// behind the string whose opening quote is at p (p itself when the text ends first); esc: a backslash was met
N1K_HD uint32_t coll_skip_string(const uint8_t* s, uint32_t n, uint32_t p, bool& esc) {
    esc = false;
    uint32_t q = p + 1;
    while (q < n) {
        const uint8_t c = s[q];
        if (c == '"') return q + 1;
        if (c == '\\') {
            esc = true;
            q++;
        }
        q++;
    }
    return n;
}

// behind the value that begins at p: brackets counted outside strings
N1K_HD uint32_t coll_skip_value(const uint8_t* s, uint32_t n, uint32_t p) {
    uint32_t depth = 0;
    while (p < n) {
        const uint8_t c = s[p];
        if (c == '"') {
            bool e;
            p = coll_skip_string(s, n, p, e);
            if (!depth) return p;
            continue;
        }
        if (c == '[' || c == '{') depth++;
        else if (c == ']' || c == '}') {
            if (!depth) return p;  // (the enclosing bracket: an empty value, malformed text)
            if (!--depth) return p + 1;
        } else if (c == ',' && !depth) return p;
        p++;
    }
    return n;
}

N1K_HD uint32_t coll_tag_at(const uint8_t* s, uint32_t b, uint32_t e) {
    if (b >= e) return T_MISSING;
    switch (s[b]) {
        case '"': return T_STRING;
        case '[': return T_ARRAY;
        case '{': return T_OBJECT;
        case 't': return T_TRUE;
        case 'f': return T_FALSE;
        case 'n': return T_NULL;
        default: return T_INT;  // a NUMBER: typed when it is compared
    }
}

// type order of value/value.go:69-79 (n1k_device.h cls_of)
N1K_HD uint32_t coll_cls(uint32_t tag) { return (uint32_t)((0x654332210ull >> (tag * 4u)) & 0xFu); }

// Number text -> (tag, payload) as value.NewValue types it; 1 = typed here, 2 = beyond the exact conversions
// (n1k_jsondev.hip scan_number, same limits), 0 = no number.
N1K_HD int coll_number(const uint8_t* s, uint32_t p, uint32_t e, uint32_t& tag, uint64_t& payload) {
    bool neg = false;
    if (p < e && s[p] == '-') {
        neg = true;
        p++;
    }
    if (p >= e || s[p] < '0' || s[p] > '9') return 0;
    unsigned long long m = 0;
    int nd = 0, frac = 0, ex = 0;
    bool over = false, integral = true;
    for (; p < e && s[p] >= '0' && s[p] <= '9'; p++)
        if (m || s[p] != '0') {
            if (nd < 18) { m = m * 10ull + (unsigned)(s[p] - '0'); nd++; }
            else over = true;
        }
    if (p < e && s[p] == '.') {
        integral = false;
        for (p++; p < e && s[p] >= '0' && s[p] <= '9'; p++) {
            if (m || s[p] != '0') {
                if (nd < 18) { m = m * 10ull + (unsigned)(s[p] - '0'); nd++; frac++; }
                else over = true;
            } else
                frac++;
        }
    }
    if (p < e && (s[p] == 'e' || s[p] == 'E')) {
        integral = false;
        p++;
        bool eneg = false;
        if (p < e && (s[p] == '+' || s[p] == '-')) eneg = s[p++] == '-';
        for (; p < e && s[p] >= '0' && s[p] <= '9'; p++)
            if (ex < 100000) ex = ex * 10 + (s[p] - '0');
        if (eneg) ex = -ex;
    }
    if (over) return 2;
    if (integral) {
        tag = T_INT;
        payload = (uint64_t)(neg ? -(long long)m : (long long)m);
        return 1;
    }
    const int e10 = ex - frac;
    if (nd > 15 || e10 > 22 || e10 < -22) return 2;
    // Clinger's exact case: m < 2^53 and |e10| <= 22 -> one correctly rounded multiplication or division
    double pw = 1.0;
    for (int k = e10 < 0 ? -e10 : e10; k > 0; k--) pw *= 10.0;  // (exact: 10^22 < 2^74 has 22 factors of 5, 5^22 < 2^53)
    double d = (double)m;
    d = e10 >= 0 ? d * pw : d / pw;
    if (neg) d = -d;
    if (d >= -9223372036854775808.0 && d < 9223372036854775808.0 && d == (double)(long long)d) {
        tag = T_INT;
        payload = (uint64_t)(long long)d;
    } else {
        tag = T_FLOAT;
        union { double f; uint64_t u; } cv;
        cv.f = d;
        payload = cv.u;
    }
    return 1;
}

N1K_HD double coll_f64(uint32_t tag, uint64_t p) {
    if (tag == T_INT) return (double)(int64_t)p;
    union { double f; uint64_t u; } cv;
    cv.u = p;
    return cv.f;
}

// collation of two numbers (value/integer.go:100-118, float.go:106-172: NaN first)
N1K_HD int coll_num_collate(uint32_t ta, uint64_t pa, uint32_t tb, uint64_t pb) {
    if (ta == T_INT && tb == T_INT) {
        const int64_t x = (int64_t)pa, y = (int64_t)pb;
        return x < y ? -1 : (x > y ? 1 : 0);
    }
    const double t = coll_f64(ta, pa), o = coll_f64(tb, pb);
    if (t != t) return (o != o) ? 0 : -1;
    if (o != o) return 1;
    return t < o ? -1 : (t > o ? 1 : 0);
}

// bytewise, like Go strings (value/string.go:116-130)
N1K_HD int coll_bytes_collate(const uint8_t* a, uint32_t na, const uint8_t* b, uint32_t nb) {
    const uint32_t m = na < nb ? na : nb;
    for (uint32_t k = 0; k < m; k++)
        if (a[k] != b[k]) return a[k] < b[k] ? -1 : 1;
    return na < nb ? -1 : (na > nb ? 1 : 0);
}

#if !defined(__HIP_DEVICE_COMPILE__) && !defined(__HIPCC_RTC__)
// host only (n1k_coll.cpp): the bytes a JSON string's raw text [b, e) (between its quotes) stands for
void coll_unescape(const uint8_t* s, uint32_t b, uint32_t e, uint8_t*& out, uint32_t& n);
void coll_unescape_free(uint8_t* p);
int coll_number_host(const uint8_t* s, uint32_t b, uint32_t e, uint32_t& tag, uint64_t& payload);
bool coll_like_host(const CollNode& nd, const uint8_t* pool, const uint8_t* s, uint32_t n);
#endif

// the decoded bytes of a string value as the evaluator holds them
struct CollStr {
    const uint8_t* p;
    uint32_t n;
    uint8_t* owned;  // host: a decoded copy to free
};

// String raw text [b, e) -> bytes.  false: escaped, and this side does not decode (left to the host).
template <bool HOST>
N1K_HD bool coll_string(const uint8_t* s, uint32_t b, uint32_t e, bool esc, CollStr& out) {
    out.p = s + b;
    out.n = e - b;
    out.owned = nullptr;
    if (!esc) return true;
#if !defined(__HIP_DEVICE_COMPILE__) && !defined(__HIPCC_RTC__)
    if (HOST) {
        coll_unescape(s, b, e, out.owned, out.n);
        out.p = out.owned;
        return true;
    }
#endif
    return false;
}
N1K_HD void coll_string_done(CollStr& v) {
#if !defined(__HIP_DEVICE_COMPILE__) && !defined(__HIPCC_RTC__)
    if (v.owned) coll_unescape_free(v.owned);
#endif
    v.owned = nullptr;
}

// The value <e> names inside the element s[b, e): its span, or b == e for MISSING (a field of a non-object, or a name the
// object lacks: Field.Evaluate, expression/nav_field.go).
template <bool HOST>
N1K_HD void coll_resolve(const CollNode& nd, const uint8_t* pool, const uint8_t* s, uint32_t n, uint32_t& b, uint32_t& e, bool& left) {
    for (uint32_t f = 0; f < nd.nf; f++) {
        if (b >= e || s[b] != '{') {
            b = e;
            return;
        }
        uint32_t p = b + 1;
        bool found = false;
        while (p < e && s[p] == '"') {
            bool esc;
            const uint32_t q = coll_skip_string(s, n, p, esc);  // behind the name
            if (q + 1 > e || q <= p + 1) break;
            const uint32_t vb = q + 1;  // behind the ':'
            const uint32_t ve = coll_skip_value(s, e, vb);
            CollStr name;
            if (!coll_string<HOST>(s, p + 1, q - 1, esc, name)) {
                left = true;  // an escaped name may or may not be the wanted one
            } else {
                found = name.n == nd.f_len[f] && coll_bytes_collate(name.p, name.n, pool + nd.f_off[f], nd.f_len[f]) == 0;
                coll_string_done(name);
            }
            if (found) {
                b = vb;
                e = ve;
                break;
            }
            p = ve;
            if (p < e && s[p] == ',') p++;
            else break;
        }
        if (!found) {
            b = e;
            return;
        }
    }
}

// value s[b, e) of tag `vt` against one constant: X.Collate(Y) with X the value.  ok = false: left to the host.
template <bool HOST>
N1K_HD int coll_collate_const(const uint8_t* s, uint32_t n, uint32_t vt, uint32_t b, uint32_t e, uint32_t ctag, uint64_t c,
                              const uint8_t* cs, uint32_t clen, bool& left) {
    const uint32_t ca = coll_cls(vt), cb = coll_cls(ctag);
    if (ca != cb) return ca < cb ? -1 : 1;
    if (ca == 2) return vt < ctag ? -1 : (vt > ctag ? 1 : 0);
    if (ca == 3) {
        uint32_t nt = T_INT;
        uint64_t np = 0;
        int r = coll_number(s, b, e, nt, np);
#if !defined(__HIP_DEVICE_COMPILE__) && !defined(__HIPCC_RTC__)
        if (HOST && r == 2) r = coll_number_host(s, b, e, nt, np);
#endif
        if (r != 1) {
            left = true;
            return 0;
        }
        return coll_num_collate(nt, np, ctag, c);
    }
    // STRING (arrays and objects never meet a constant of their class)
    bool esc;
    const uint32_t q = coll_skip_string(s, n, b, esc);
    CollStr v;
    if (q <= b + 1 || !coll_string<HOST>(s, b + 1, q - 1, esc, v)) {
        left = true;
        return 0;
    }
    const int r = coll_bytes_collate(v.p, v.n, cs, clen);
    coll_string_done(v);
    return r;
}

// one leaf on one element -> L_*
template <bool HOST>
N1K_HD uint32_t coll_leaf(const CollNode& nd, const uint8_t* pool, const uint8_t* s, uint32_t n, uint32_t eb, uint32_t ee, bool& left) {
    uint32_t b = eb, e = ee;
    coll_resolve<HOST>(nd, pool, s, n, b, e, left);
    const uint32_t vt = coll_tag_at(s, b, e);
    switch (nd.op) {
        case CN_IS_NULL: return vt == T_NULL ? L_TRUE : (vt == T_MISSING ? L_MISSING : L_FALSE);
        case CN_IS_NOT_NULL: return vt == T_NULL ? L_FALSE : (vt == T_MISSING ? L_MISSING : L_TRUE);
        case CN_IS_MISSING: return vt == T_MISSING ? L_TRUE : L_FALSE;
        case CN_IS_NOT_MISSING: return vt == T_MISSING ? L_FALSE : L_TRUE;
        case CN_IS_VALUED: return vt <= T_NULL ? L_FALSE : L_TRUE;
        case CN_IS_NOT_VALUED: return vt <= T_NULL ? L_TRUE : L_FALSE;
        default: break;
    }
    if (vt == T_MISSING) return L_MISSING;
    if (nd.op == CN_LIKE) {  // Like.Apply, comp_like.go:68-88
        if (vt != T_STRING) return L_NULL;
        bool esc;
        const uint32_t q = coll_skip_string(s, n, b, esc);
        if (q <= b + 1) return L_NULL;
        bool hit = false;
        if (!esc && like_utf8_valid(s + b + 1, q - b - 2)) {
            hit = like_match(pool + nd.c_off, nd.c_len, nd.anchor_end != 0, LikeBytes{s + b + 1, q - b - 2});
        } else {
#if !defined(__HIP_DEVICE_COMPILE__) && !defined(__HIPCC_RTC__)
            if (HOST) {
                CollStr v;
                coll_string<HOST>(s, b + 1, q - 1, esc, v);
                hit = coll_like_host(nd, pool, v.p, v.n);
                coll_string_done(v);
            } else
#endif
                left = true;
        }
        return hit ? L_TRUE : L_FALSE;
    }
    if (vt == T_NULL) return L_NULL;
    const int c = coll_collate_const<HOST>(s, n, vt, b, e, nd.ctag, nd.c, pool + nd.c_off, nd.c_len, left);
    switch (nd.op) {
        case CN_EQ: {  // X.Equals(Y): FALSE across types, numbers by value (value/integer.go:68-87, string.go:82-96)
            if (coll_cls(vt) != coll_cls(nd.ctag)) return L_FALSE;
            return c == 0 ? L_TRUE : L_FALSE;
        }
        case CN_LT: return (nd.flip ? c > 0 : c < 0) ? L_TRUE : L_FALSE;   // comp_lt.go:57-65
        case CN_LE: return (nd.flip ? c >= 0 : c <= 0) ? L_TRUE : L_FALSE;  // comp_le.go:57-65
        default: {  // CN_BETWEEN, comp_between.go:58-78
            const int hi = coll_collate_const<HOST>(s, n, vt, b, e, nd.ctag2, nd.c2, pool + nd.c2_off, nd.c2_len, left);
            return (c >= 0 && hi <= 0) ? L_TRUE : L_FALSE;
        }
    }
}

// And.Apply / Or.Apply / Not.Apply over two values (expression/logic_and.go:64-89, logic_or.go:98-123, logic_not.go:57-69)
N1K_HD uint32_t coll_and(uint32_t x, uint32_t y) {
    if (x == L_FALSE || y == L_FALSE) return L_FALSE;
    if (x == L_MISSING || y == L_MISSING) return L_MISSING;
    if (x == L_NULL || y == L_NULL) return L_NULL;
    return L_TRUE;
}
N1K_HD uint32_t coll_or(uint32_t x, uint32_t y) {
    if (x == L_TRUE || y == L_TRUE) return L_TRUE;
    if (x == L_NULL || y == L_NULL) return L_NULL;
    if (x == L_MISSING || y == L_MISSING) return L_MISSING;
    return L_FALSE;
}

// The predicate over the array whose canonical text is s[0, n).  Text that is no array gives false (no row reads it).
template <bool HOST>
N1K_HD bool coll_eval(const CollProg& g, const uint8_t* s, uint32_t n, bool& left) {
    if (n < 2 || s[0] != '[') return false;
    uint32_t p = 1, count = 0;
    while (p < n && s[p] != ']') {
        const uint32_t q = coll_skip_value(s, n, p);
        if (q <= p) break;  // (malformed text: no progress)
        uint32_t vals = 0;
        for (uint32_t i = 0; i < g.nn; i++) {
            const CollNode& nd = g.node[i];
            uint32_t r;
            if (nd.op == CN_AND) r = coll_and((vals >> (2u * nd.a)) & 3u, (vals >> (2u * nd.b)) & 3u);
            else if (nd.op == CN_OR) r = coll_or((vals >> (2u * nd.a)) & 3u, (vals >> (2u * nd.b)) & 3u);
            else if (nd.op == CN_NOT) {
                const uint32_t v = (vals >> (2u * nd.a)) & 3u;
                r = v >= L_NULL ? v : (v ^ 1u);
            } else
                r = coll_leaf<HOST>(nd, g.pool, s, n, p, q, left);
            vals |= r << (2u * i);
        }
        const bool truth = g.nn && ((vals >> (2u * (g.nn - 1u))) & 3u) == L_TRUE;
        count++;
        if (g.mode == COLL_ANY) {
            if (truth) return true;
        } else if (!truth)
            return false;
        p = q;
        if (p < n && s[p] == ',') p++;
    }
    return g.mode == COLL_ANY ? false : (g.mode == COLL_EVERY ? true : count > 0);
}

}  // namespace n1k

#if !defined(__HIPCC_RTC__)
#include <string>
#include <vector>

namespace n1k {

struct Expr;
struct PlanError;

struct CollPred {
    std::string text;  // the whole term as the plan wrote it
    CollProg prog;
};

// An EK::Coll expression -> program.  false + err (unsupported, the construct named) for what lies outside the subset.
bool coll_compile(const Expr* e, CollProg& out, PlanError& err);
// bits[i] |= (predicate q holds for entry i) << (first_bit - q); entries that are no array text get nothing
void coll_eval_block_host(const std::vector<CollPred>& preds, uint32_t first_bit, uint64_t n, const uint64_t* offsets, const uint8_t* bytes, uint8_t* bits);
hipError_t launch_coll_match(const CollKernelArgs& A, hipStream_t st);

}  // namespace n1k
#endif
