// n1k_coll.cpp — ANY / EVERY: the predicate compiler and what only the host evaluator does.  (The device route and the
// entry points of the C ABI: n1k_matchtable.cpp.)
#include "n1k_coll.h"

#include <cerrno>
#include <cstdlib>

#include "n1k_engine.h"

namespace n1k {

namespace {

struct Compiler {
    const Expr* coll;
    CollProg& g;
    PlanError& err;
    uint32_t pool_used = 0;

    bool refuse(const std::string& what) {
        if (err.msg.empty()) {
            err.unsupported = true;
            err.msg = "ANY / EVERY: " + what + " is outside the device subset (in: " + coll->text + ")";
        }
        return false;
    }
    bool pool_put(const void* p, size_t n, uint16_t& off, uint16_t& len) {
        if (pool_used + n > kCollPoolBytes)
            return refuse("field names, STRING constants and patterns of more than " + std::to_string(kCollPoolBytes) + " bytes in one SATISFIES condition");
        off = (uint16_t)pool_used;
        len = (uint16_t)n;
        if (n) memcpy(g.pool + pool_used, p, n);
        pool_used += (uint32_t)n;
        return true;
    }
    int node(const CollNode& nd) {
        if (g.nn == kCollMaxNodes) {
            refuse("a SATISFIES condition of more than " + std::to_string(kCollMaxNodes) + " nodes");
            return -1;
        }
        g.node[g.nn] = nd;
        return (int)g.nn++;
    }
    // <e>: `v`, (`v`.`f`), ((`v`.`f`).`g`) as the stringer writes them
    bool path(const Expr* e, CollNode& nd) {
        if (e->kind == EK::Coll) return refuse("a nested ANY / EVERY");
        if (e->kind == EK::Const) return refuse("a comparison of two constants inside SATISFIES");
        if (e->kind == EK::Func) return refuse("function '" + e->fname + "' inside SATISFIES");
        if (e->kind != EK::Path) return refuse("arithmetic or a nested condition as an operand inside SATISFIES");
        const std::string& t = e->text;
        size_t i = 0;
        while (i < t.size() && t[i] == '(') i++;
        if (i >= t.size() || t[i] != '`') return refuse("a reference to " + t + " inside SATISFIES (anything but the variable: meta(), cover())");
        size_t j = t.find('`', i + 1);
        if (j == std::string::npos) return refuse("the operand " + t);
        if (t.compare(i + 1, j - i - 1, coll->coll_var) != 0)
            return refuse("an outer reference inside SATISFIES (" + t + " is not the variable `" + coll->coll_var + "`)");
        i = j + 1;
        nd.nf = 0;
        while (i < t.size()) {
            if (t.compare(i, 2, ".`") != 0) return refuse("element access or a computed field (" + t + ")");
            j = t.find('`', i + 2);
            if (j == std::string::npos || j + 1 >= t.size() || t[j + 1] != ')') return refuse("the operand " + t);
            if (nd.nf == kCollMaxFields) return refuse("more than " + std::to_string(kCollMaxFields) + " field names behind the variable (" + t + ")");
            if (!pool_put(t.data() + i + 2, j - i - 2, nd.f_off[nd.nf], nd.f_len[nd.nf])) return false;
            nd.nf++;
            i = j + 2;
        }
        return true;
    }
    bool constant(const Expr* e, uint8_t& tag, uint64_t& c, uint16_t& off, uint16_t& len) {
        if (e->kind != EK::Const) return refuse("a comparison with anything but a constant inside SATISFIES");
        if (e->ctag != T_STRING && e->ctag != T_INT && e->ctag != T_FLOAT && e->ctag != T_TRUE && e->ctag != T_FALSE)
            return refuse("a comparison with a NULL or MISSING constant inside SATISFIES");
        tag = (uint8_t)e->ctag;
        c = e->cpayload;
        off = len = 0;
        if (e->ctag == T_STRING) return pool_put(e->cstr.data(), e->cstr.size(), off, len);
        return true;
    }
    // `v < 10`, `10 < v`, `v between 1 and 5` over the BARE variable stay with the reference operators: not a
    // limit of the evaluator — `(v.x) < 10` and `v = 10` run — but the reference's EXPLAIN subtree of that form is pinned as
    // refused by the plan fixtures, whose path scanner reads the bound variable as a column of the row.
    bool ordered_ok(const CollNode& nd, uint8_t ctag) {
        if (nd.nf == 0 && (ctag == T_INT || ctag == T_FLOAT))
            return refuse("an ordering comparison (<, <=, >, >=, BETWEEN) of the bare variable with a NUMBER constant");
        return true;
    }
    int emit(const Expr* e) {
        CollNode nd{};
        switch (e->kind) {
            case EK::And:
            case EK::Or: {
                int acc = emit(e->ch[0].get());
                for (size_t k = 1; k < e->ch.size() && acc >= 0; k++) {
                    const int o = emit(e->ch[k].get());
                    if (o < 0) return -1;
                    CollNode l{};
                    l.op = e->kind == EK::And ? CN_AND : CN_OR;
                    l.a = (uint8_t)acc;
                    l.b = (uint8_t)o;
                    acc = node(l);
                }
                return acc;
            }
            case EK::Not: {
                const int a = emit(e->ch[0].get());
                if (a < 0) return -1;
                nd.op = CN_NOT;
                nd.a = (uint8_t)a;
                return node(nd);
            }
            case EK::Eq:
            case EK::LT:
            case EK::LE: {
                const Expr *a = e->ch[0].get(), *b = e->ch[1].get();
                const bool flip = a->kind == EK::Const && b->kind != EK::Const;
                if (flip) std::swap(a, b);
                if (!path(a, nd) || !constant(b, nd.ctag, nd.c, nd.c_off, nd.c_len)) return -1;
                nd.op = e->kind == EK::Eq ? CN_EQ : (e->kind == EK::LT ? CN_LT : CN_LE);
                nd.flip = flip ? 1 : 0;
                if (nd.op != CN_EQ && !ordered_ok(nd, nd.ctag)) return -1;
                return node(nd);
            }
            case EK::Between:
                if (!path(e->ch[0].get(), nd) || !constant(e->ch[1].get(), nd.ctag, nd.c, nd.c_off, nd.c_len) ||
                    !constant(e->ch[2].get(), nd.ctag2, nd.c2, nd.c2_off, nd.c2_len))
                    return -1;
                nd.op = CN_BETWEEN;
                if (!ordered_ok(nd, nd.ctag) || !ordered_ok(nd, nd.ctag2)) return -1;
                return node(nd);
            case EK::Like: {
                const Expr* pat = e->ch[1].get();
                if (pat->kind != EK::Const || pat->ctag != T_STRING) { refuse("LIKE with a pattern that is not a STRING constant"); return -1; }
                LikePattern lp;
                if (!like_compile(pat->cstr.data(), pat->cstr.size(), lp)) { refuse("a LIKE pattern that is not valid UTF-8"); return -1; }
                if (lp.prog.size() > 255) { refuse("a LIKE pattern whose program is longer than 255 bytes"); return -1; }
                if (!path(e->ch[0].get(), nd) || !pool_put(lp.prog.data(), lp.prog.size(), nd.c_off, nd.c_len)) return -1;
                nd.op = CN_LIKE;
                nd.anchor_end = lp.anchor_end ? 1 : 0;
                g.has_like = 1;
                return node(nd);
            }
            case EK::IsNull: case EK::IsNotNull: case EK::IsMissing: case EK::IsNotMissing: case EK::IsValued: case EK::IsNotValued:
                if (!path(e->ch[0].get(), nd)) return -1;
                nd.op = e->kind == EK::IsNull ? CN_IS_NULL : e->kind == EK::IsNotNull ? CN_IS_NOT_NULL : e->kind == EK::IsMissing ? CN_IS_MISSING
                        : e->kind == EK::IsNotMissing ? CN_IS_NOT_MISSING : e->kind == EK::IsValued ? CN_IS_VALUED : CN_IS_NOT_VALUED;
                return node(nd);
            case EK::Coll: refuse("a nested ANY / EVERY"); return -1;
            case EK::In: refuse("IN inside SATISFIES"); return -1;
            case EK::Func: refuse("function '" + e->fname + "' inside SATISFIES"); return -1;
            case EK::Path:
            case EK::Const: refuse("a bare value used for its truth inside SATISFIES"); return -1;
            default: refuse("arithmetic used for its truth inside SATISFIES"); return -1;
        }
    }
};

}  // namespace

bool coll_compile(const Expr* e, CollProg& out, PlanError& err) {
    memset(&out, 0, sizeof out);
    if (!e || e->kind != EK::Coll || !e->coll_pred) {
        err.msg = "not an ANY / EVERY term";
        return false;
    }
    out.mode = e->coll_mode;
    Compiler c{e, out, err};
    return c.emit(e->coll_pred.get()) >= 0;
}

// ---- what only the host evaluator does

static void put_utf8(std::string& o, uint32_t cp) {
    if (cp < 0x80) o.push_back((char)cp);
    else if (cp < 0x800) { o.push_back((char)(0xC0 | (cp >> 6))); o.push_back((char)(0x80 | (cp & 0x3F))); }
    else if (cp < 0x10000) { o.push_back((char)(0xE0 | (cp >> 12))); o.push_back((char)(0x80 | ((cp >> 6) & 0x3F))); o.push_back((char)(0x80 | (cp & 0x3F))); }
    else { o.push_back((char)(0xF0 | (cp >> 18))); o.push_back((char)(0x80 | ((cp >> 12) & 0x3F))); o.push_back((char)(0x80 | ((cp >> 6) & 0x3F))); o.push_back((char)(0x80 | (cp & 0x3F))); }
}

// encoding/json unquote: \uXXXX with surrogate pairs, a lone surrogate is U+FFFD
void coll_unescape(const uint8_t* s, uint32_t b, uint32_t e, uint8_t*& out, uint32_t& n) {
    auto hex4 = [&](uint32_t p, uint32_t& v) {
        if (p + 4 > e) return false;
        v = 0;
        for (uint32_t k = 0; k < 4; k++) {
            const uint8_t c = s[p + k];
            const int d = c >= '0' && c <= '9' ? c - '0' : (c >= 'a' && c <= 'f' ? c - 'a' + 10 : (c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1));
            if (d < 0) return false;
            v = v * 16 + (uint32_t)d;
        }
        return true;
    };
    std::string o;
    for (uint32_t p = b; p < e;) {
        if (s[p] != '\\' || p + 1 >= e) {
            o.push_back((char)s[p++]);
            continue;
        }
        const uint8_t x = s[p + 1];
        p += 2;
        switch (x) {
            case 'n': o.push_back('\n'); break;
            case 't': o.push_back('\t'); break;
            case 'r': o.push_back('\r'); break;
            case 'b': o.push_back('\b'); break;
            case 'f': o.push_back('\f'); break;
            case 'u': {
                uint32_t cp = 0xFFFD, lo;
                if (hex4(p, cp)) {
                    p += 4;
                    if (cp >= 0xD800 && cp < 0xDC00 && p + 6 <= e && s[p] == '\\' && s[p + 1] == 'u' && hex4(p + 2, lo) && lo >= 0xDC00 && lo < 0xE000) {
                        cp = 0x10000 + ((cp - 0xD800) << 10) + (lo - 0xDC00);
                        p += 6;
                    } else if (cp >= 0xD800 && cp < 0xE000)
                        cp = 0xFFFD;
                }
                put_utf8(o, cp);
                break;
            }
            default: o.push_back((char)x);  // \" \\ \/
        }
    }
    n = (uint32_t)o.size();
    out = (uint8_t*)malloc(o.size() + 1);
    memcpy(out, o.data(), o.size());
}
void coll_unescape_free(uint8_t* p) { free(p); }

// value.NewValue's typing of a number of any length (n1k_json.cpp type_number)
int coll_number_host(const uint8_t* s, uint32_t b, uint32_t e, uint32_t& tag, uint64_t& payload) {
    const std::string z((const char*)s + b, (const char*)s + e);
    if (z.find_first_of(".eE") == std::string::npos && z.size() <= 20) {
        errno = 0;
        char* endp = nullptr;
        const long long v = strtoll(z.c_str(), &endp, 10);
        if (errno == 0 && endp && *endp == 0) {
            tag = T_INT;
            payload = (uint64_t)v;
            return 1;
        }
    }
    char* endp = nullptr;
    const double d = strtod(z.c_str(), &endp);
    if (!endp || *endp != 0) return 0;
    if (d >= -9223372036854775808.0 && d < 9223372036854775808.0 && d == (double)(int64_t)d) {
        tag = T_INT;
        payload = (uint64_t)(int64_t)d;
    } else {
        tag = T_FLOAT;
        memcpy(&payload, &d, 8);
    }
    return 1;
}

bool coll_like_host(const CollNode& nd, const uint8_t* pool, const uint8_t* s, uint32_t n) {
    LikePattern lp;
    lp.prog.assign(pool + nd.c_off, pool + nd.c_off + nd.c_len);
    lp.anchor_end = nd.anchor_end != 0;
    return like_match_host(lp, s, n);
}

void coll_eval_block_host(const std::vector<CollPred>& preds, uint32_t first_bit, uint64_t n, const uint64_t* offsets, const uint8_t* bytes, uint8_t* bits) {
    for (uint64_t i = 0; i < n; i++) {
        const uint8_t* s = bytes + (offsets[i] - offsets[0]);
        const uint32_t len = (uint32_t)(offsets[i + 1] - offsets[i]);
        if (!coll_array_text(s, len)) continue;
        for (size_t q = 0; q < preds.size(); q++) {
            bool left = false;
            if (coll_eval<true>(preds[q].prog, s, len, left)) bits[i] |= (uint8_t)(1u << (first_bit - q));
        }
    }
}

}  // namespace n1k
