// n1k_strfn.cpp — string functions in a condition: the term compiler and the host matcher.  (The device route and the entry
// points of the C ABI: n1k_matchtable.cpp.)
#include "n1k_strfn.h"

#include <cstring>

#include "n1k_plan.h"

namespace n1k {

namespace {

bool is_step(const std::string& f) { return f == "lower" || f == "upper" || f == "trim" || f == "ltrim" || f == "rtrim"; }
bool is_position(const std::string& f) {
    return f == "position" || f == "pos" || f == "position0" || f == "pos0" || f == "position1" || f == "pos1";
}
bool is_strfn(const Expr* e) { return e->kind == EK::Func && strfn_name(e->fname); }
bool ascii(const std::string& s) {
    for (unsigned char c : s)
        if (c >= 0x80) return false;
    return true;
}

struct Compiler {
    const Expr* term;
    StrFnProg& g;
    PlanError& err;
    uint32_t pool_used = 0;
    bool refuse(const std::string& what) {
        if (err.msg.empty()) {
            err.unsupported = true;
            err.msg = "string functions: " + what + " is outside the device subset";
        }
        return false;
    }
    bool pool_put(const std::string& s, uint16_t& off, uint16_t& len) {
        if (pool_used + s.size() > kStrFnPoolBytes)
            return refuse("more than " + std::to_string(kStrFnPoolBytes) + " bytes of constants (cutsets, compare constants, needle, pattern) in one predicate");
        off = (uint16_t)pool_used;
        len = (uint16_t)s.size();
        if (!s.empty()) memcpy(g.pool + pool_used, s.data(), s.size());
        pool_used += (uint32_t)s.size();
        return true;
    }
    // the STRING constant second argument of `f`
    const std::string* string_arg(const Expr* e, const std::string& f) {
        if (e->kind != EK::Const || e->ctag != T_STRING) {
            refuse("a second argument of " + f + " that is not a STRING constant");
            return nullptr;
        }
        return &e->cstr;
    }
    bool case_ascii(const std::string& s, const char* what) {
        if ((g.has_lower || g.has_upper) && !ascii(s)) return refuse(std::string("a non-ASCII ") + what + " under lower / upper (case mapping of non-ASCII text is not on the device)");
        return true;
    }
    // lower(trim(path, "x")) ...: the steps innermost first, and the leaf path
    bool chain(const Expr* e, const Expr*& path) {
        std::vector<const Expr*> fns;  // outermost first
        while (e->kind == EK::Func && is_step(e->fname)) {
            fns.push_back(e);
            e = e->ch[0].get();
        }
        if (e->kind == EK::Func) return refuse("function '" + e->fname + "' inside a chain of lower / upper / trim / ltrim / rtrim");
        if (e->kind != EK::Path) return refuse("a string function over anything but a leaf path (a constant, arithmetic, a nested condition)");
        if (fns.size() > kStrFnMaxSteps) return refuse("a chain of more than " + std::to_string(kStrFnMaxSteps) + " nested string functions");
        path = e;
        for (size_t k = fns.size(); k-- > 0;) {
            const Expr* f = fns[k];
            StrFnStep& st = g.steps[g.nsteps++];
            const std::string& n = f->fname;
            st.fn = n == "lower" ? SF_LOWER : n == "upper" ? SF_UPPER : n == "trim" ? SF_TRIM : n == "ltrim" ? SF_LTRIM : SF_RTRIM;
            if (st.fn == SF_LOWER) g.has_lower = 1;
            else if (st.fn == SF_UPPER) g.has_upper = 1;
            else {
                std::string cut = " \t\n\f\r";  // _WHITESPACE, func_str.go:301
                if (f->ch.size() > 1) {
                    const std::string* c = string_arg(f->ch[1].get(), n);
                    if (!c) return false;
                    cut = *c;
                }
                // (strings.Trim* with an ASCII cutset works on bytes: exact on any text.  A cutset of other runes decodes the
                //  string, where an invalid byte and a literal U+FFFD become one: not taken, with or without a case step.)
                if (!ascii(cut)) return refuse("a non-ASCII cutset of " + n);
                if (!pool_put(cut, st.cut_off, st.cut_len)) return false;
            }
        }
        return true;
    }
    bool string_const(const Expr* e, int slot) {
        if (e->kind != EK::Const) return refuse("a string function compared with anything but a constant");
        if (e->ctag != T_STRING) return refuse("a string function's value compared with a constant that is not a STRING (a NUMBER, a boolean, NULL or MISSING)");
        return case_ascii(e->cstr, "compare constant") && pool_put(e->cstr, g.c_off[slot], g.c_len[slot]);
    }
    bool number_const(const Expr* e, int slot) {
        if (e->kind != EK::Const) return refuse("a position compared with anything but a constant");
        if (e->ctag != T_INT && e->ctag != T_FLOAT) return refuse("a position compared with a constant that is not a NUMBER (a STRING, a boolean, NULL or MISSING)");
        if (e->ctag == T_INT) g.num[slot] = (double)(int64_t)e->cpayload;
        else memcpy(&g.num[slot], &e->cpayload, 8);
        return true;
    }
    // the value side of a comparison: a chain (SFT_CMP) or positionN over the bare path (SFT_POS)
    bool value(const Expr* v, const Expr*& path) {
        if (v->kind == EK::Func && is_position(v->fname)) {
            g.term = SFT_POS;
            g.start_pos = v->fname.back() == '1' ? 1 : 0;
            const Expr* x = v->ch[0].get();
            if (x->kind == EK::Func && is_step(x->fname)) {
                const Expr* y = x;
                bool has_case = false;
                while (y->kind == EK::Func && is_step(y->fname)) {
                    has_case = has_case || y->fname == "lower" || y->fname == "upper";
                    y = y->ch[0].get();
                }
                return refuse(has_case ? v->fname + " over lower / upper (mapped runes change their byte length: the index would not be exact)"
                                       : v->fname + " over anything but the bare path");
            }
            if (x->kind != EK::Path) return refuse(v->fname + " over anything but a leaf path");
            path = x;
            const std::string* needle = string_arg(v->ch[1].get(), v->fname);
            return needle && pool_put(*needle, g.c_off[0], g.c_len[0]);
        }
        if (v->kind == EK::Func && v->fname == "contains") return refuse("the value of contains compared with a constant");
        g.term = SFT_CMP;
        return chain(v, path);
    }
    bool constant(const Expr* c, int slot) { return g.term == SFT_POS ? number_const(c, slot) : string_const(c, slot); }

    bool compile(const Expr*& path) {
        const Expr* e = term;
        switch (e->kind) {
            case EK::Func: {
                if (e->fname != "contains") return refuse("function '" + e->fname + "' used for its truth");
                g.term = SFT_CONTAINS;
                if (!chain(e->ch[0].get(), path)) return false;
                const std::string* needle = string_arg(e->ch[1].get(), "contains");
                return needle && case_ascii(*needle, "needle") && pool_put(*needle, g.c_off[0], g.c_len[0]);
            }
            case EK::Eq:
            case EK::LT:
            case EK::LE: {
                const Expr *a = e->ch[0].get(), *b = e->ch[1].get();
                const bool flip = !is_strfn(a);  // ("c" < f(x)) == (f(x) > "c"), as TERM_NUM_* mirrors
                if (flip) std::swap(a, b);
                g.cmp = e->kind == EK::Eq ? SFC_EQ : (e->kind == EK::LT ? (flip ? SFC_GT : SFC_LT) : (flip ? SFC_GE : SFC_LE));
                return value(a, path) && constant(b, 0);
            }
            case EK::Between:
                g.cmp = SFC_BETWEEN;
                if (!is_strfn(e->ch[0].get())) return refuse("BETWEEN whose bounds are string functions");
                return value(e->ch[0].get(), path) && constant(e->ch[1].get(), 0) && constant(e->ch[2].get(), 1);
            case EK::Like: {
                g.term = SFT_LIKE;
                const Expr* pat = e->ch[1].get();
                if (!is_strfn(e->ch[0].get())) return refuse("LIKE whose pattern is a string function");
                if (e->ch[0]->kind == EK::Func && !is_step(e->ch[0]->fname)) return refuse("function '" + e->ch[0]->fname + "' under LIKE");
                if (!chain(e->ch[0].get(), path)) return false;
                if (pat->kind != EK::Const || pat->ctag != T_STRING) return refuse("LIKE with a pattern that is not a STRING constant");
                if (!case_ascii(pat->cstr, "LIKE pattern")) return false;
                LikePattern lp;
                if (!like_compile(pat->cstr.data(), pat->cstr.size(), lp)) return refuse("a LIKE pattern that is not valid UTF-8");
                if (lp.prog.size() > kLikeDevProgBytes)
                    return refuse("a LIKE pattern whose program is longer than " + std::to_string(kLikeDevProgBytes) + " bytes");
                if (pool_used + pat->cstr.size() > kStrFnPoolBytes)  // (the pattern's text counts; the pool holds its program's place only by size)
                    return refuse("more than " + std::to_string(kStrFnPoolBytes) + " bytes of constants (cutsets, compare constants, needle, pattern) in one predicate");
                g.like_len = (uint8_t)lp.prog.size();
                g.anchor_end = lp.anchor_end ? 1 : 0;
                if (!lp.prog.empty()) memcpy(g.like_prog, lp.prog.data(), lp.prog.size());
                return true;
            }
            default: return refuse("this use of a string function");
        }
    }
};

}  // namespace

bool strfn_name(const std::string& f) { return is_step(f) || is_position(f) || f == "contains"; }

bool strfn_term(const Expr* e) {
    switch (e->kind) {
        case EK::Func: return strfn_name(e->fname);
        case EK::Eq:
        case EK::LT:
        case EK::LE:
        case EK::Like: return is_strfn(e->ch[0].get()) || is_strfn(e->ch[1].get());
        case EK::Between: return is_strfn(e->ch[0].get()) || is_strfn(e->ch[1].get()) || is_strfn(e->ch[2].get());
        default: return false;
    }
}

bool strfn_compile(const Expr* e, StrFnProg& out, const Expr*& path, PlanError& err) {
    memset(&out, 0, sizeof out);
    path = nullptr;
    Compiler c{e, out, err};
    if (!c.compile(path)) {
        if (err.msg.empty()) {
            err.unsupported = true;
            err.msg = "string functions: the term is outside the device subset";
        }
        return false;
    }
    return true;
}

namespace {

void put_utf8(std::string& o, uint32_t cp) {
    if (cp < 0x80) o += (char)cp;
    else if (cp < 0x800) {
        o += (char)(0xC0 | (cp >> 6));
        o += (char)(0x80 | (cp & 0x3F));
    } else if (cp < 0x10000) {
        o += (char)(0xE0 | (cp >> 12));
        o += (char)(0x80 | ((cp >> 6) & 0x3F));
        o += (char)(0x80 | (cp & 0x3F));
    } else {
        o += (char)(0xF0 | (cp >> 18));
        o += (char)(0x80 | ((cp >> 12) & 0x3F));
        o += (char)(0x80 | ((cp >> 6) & 0x3F));
        o += (char)(0x80 | (cp & 0x3F));
    }
}

// The steps over the decoded runes, as Go applies them: the mapped string is materialised (the four runes become ASCII,
// every other non-ASCII rune stays — see n1k_strfn.h), then the terminal over its runes (LIKE) or its bytes.
bool eval_runes(const StrFnProg& g, const uint8_t* s, uint32_t n) {
    std::vector<uint32_t> r;
    like_decode_runes(s, n, r);
    size_t b = 0, e = r.size();
    for (uint32_t k = 0; k < g.nsteps; k++) {
        const StrFnStep& st = g.steps[k];
        if (st.fn == SF_LOWER) {
            for (size_t i = b; i < e; i++) r[i] = r[i] >= 'A' && r[i] <= 'Z' ? r[i] + 32 : (r[i] == 0x130 ? 'i' : (r[i] == 0x212A ? 'k' : r[i]));
        } else if (st.fn == SF_UPPER) {
            for (size_t i = b; i < e; i++) r[i] = r[i] >= 'a' && r[i] <= 'z' ? r[i] - 32 : (r[i] == 0x17F ? 'S' : (r[i] == 0x131 ? 'I' : r[i]));
        } else {
            const uint8_t* set = g.pool + st.cut_off;
            auto in = [&](uint32_t c) { return c < 0x80 && strfn_in_set((uint8_t)c, set, st.cut_len); };
            if (st.fn != SF_RTRIM)
                while (b < e && in(r[b])) b++;
            if (st.fn != SF_LTRIM)
                while (e > b && in(r[e - 1])) e--;
        }
    }
    if (g.term == SFT_LIKE) return like_match_runes(g.like_prog, g.like_len, g.anchor_end != 0, r.data() + b, (uint32_t)(e - b));
    std::string bytes;
    for (size_t i = b; i < e; i++) put_utf8(bytes, r[i]);
    return strfn_terminal(g, (const uint8_t*)bytes.data(), (uint32_t)bytes.size(), SFM_NONE);
}

}  // namespace

bool strfn_eval_host(const StrFnProg& g, const uint8_t* s, size_t n) {
    return strfn_needs_host(g, s, (uint32_t)n) ? eval_runes(g, s, (uint32_t)n) : strfn_eval(g, s, (uint32_t)n);
}

void strfn_eval_block_host(const std::vector<StrFnPred>& preds, uint32_t first_bit, uint64_t n, const uint64_t* offsets, const uint8_t* bytes, uint8_t* bits) {
    for (uint64_t i = 0; i < n; i++) {
        const uint8_t* s = bytes + (offsets[i] - offsets[0]);
        const size_t len = (size_t)(offsets[i + 1] - offsets[i]);
        uint8_t b = 0;
        for (size_t q = 0; q < preds.size(); q++) b |= (uint8_t)(strfn_eval_host(preds[q].prog, s, len) ? 1u << (first_bit + q) : 0u);
        bits[i] |= b;
    }
}

}  // namespace n1k
