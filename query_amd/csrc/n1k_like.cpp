// n1k_like.cpp — LIKE: pattern compiler and the host matcher.  (The device route and the entry points of the C ABI:
// n1k_matchtable.cpp.)
#include "n1k_like.h"

#include "n1k_engine.h"

namespace n1k {

bool like_compile(const char* pattern, size_t len, LikePattern& out) {
    const uint8_t* s = (const uint8_t*)pattern;
    if (len > 0x7FFFFFFFu || !like_utf8_valid(s, (uint32_t)len)) return false;
    out.text.assign(pattern, len);
    out.prog.clear();
    out.anchor_end = true;
    std::string lit;
    bool last_many = false;
    auto flush = [&]() {
        for (size_t i = 0, m; i < lit.size(); i += m) {
            m = std::min<size_t>(255, lit.size() - i);
            // (a chunk ends on a character boundary: the matcher over code points decodes every chunk on its own)
            while (i + m < lit.size() && ((uint8_t)lit[i + m] & 0xC0) == 0x80) m--;
            out.prog.push_back(LIKE_OP_LIT);
            out.prog.push_back((uint8_t)m);
            out.prog.insert(out.prog.end(), lit.begin() + i, lit.begin() + i + m);
        }
        lit.clear();
    };
    for (size_t i = 0; i < len; i++) {
        const char c = pattern[i];
        out.anchor_end = true;
        if (c == '\\' && i + 1 < len && (pattern[i + 1] == '%' || pattern[i + 1] == '_')) {
            lit.push_back(pattern[++i]);
            last_many = false;
            out.anchor_end = false;  // (holds only if this was the last token: reset by whatever follows)
        } else if (c == '%') {
            flush();
            if (!last_many) out.prog.push_back(LIKE_OP_MANY);  // (a MANY right behind a MANY adds nothing)
            last_many = true;
        } else if (c == '_') {
            flush();
            out.prog.push_back(LIKE_OP_ONE);
            last_many = false;
        } else {
            lit.push_back(c);
            last_many = false;
        }
    }
    flush();
    return true;
}

namespace {

// Go's view of a string that is not valid UTF-8: code points, every byte that begins no valid encoding one U+FFFD
struct LikeRunes {
    const uint32_t* s;
    uint32_t n;
    uint32_t next(uint32_t p) const { return p + 1; }
    bool newline(uint32_t p) const { return s[p] == '\n'; }
    uint32_t lit(uint32_t p, const uint8_t* b, uint32_t len) const {
        for (uint32_t k = 0; k < len;) {  // (the literal is valid UTF-8 and holds whole characters)
            const uint32_t l = like_utf8_len(b[k]);
            uint32_t cp = l == 1 ? b[k] : (l == 2 ? b[k] & 0x1Fu : (l == 3 ? b[k] & 0x0Fu : b[k] & 0x07u));
            for (uint32_t j = 1; j < l; j++) cp = (cp << 6) | (b[k + j] & 0x3Fu);
            if (p >= n || s[p] != cp) return 0xFFFFFFFFu;
            p++;
            k += l;
        }
        return p;
    }
};

}  // namespace

void like_decode_runes(const uint8_t* s, uint32_t n, std::vector<uint32_t>& out) {
    out.clear();
    for (uint32_t i = 0; i < n;) {
        const uint32_t l = like_utf8_valid_at(s, n, i);
        if (!l) {
            out.push_back(0xFFFDu);
            i++;
            continue;
        }
        uint32_t cp = l == 1 ? s[i] : (l == 2 ? s[i] & 0x1Fu : (l == 3 ? s[i] & 0x0Fu : s[i] & 0x07u));
        for (uint32_t j = 1; j < l; j++) cp = (cp << 6) | (s[i + j] & 0x3Fu);
        out.push_back(cp);
        i += l;
    }
}

bool like_match_runes(const uint8_t* prog, uint32_t plen, bool anchor_end, const uint32_t* r, uint32_t n) {
    return like_match(prog, plen, anchor_end, LikeRunes{r, n});
}

bool like_match_host(const LikePattern& p, const uint8_t* s, size_t n) {
    if (like_utf8_valid(s, (uint32_t)n))
        return like_match(p.prog.data(), (uint32_t)p.prog.size(), p.anchor_end, LikeBytes{s, (uint32_t)n});
    std::vector<uint32_t> r;
    like_decode_runes(s, (uint32_t)n, r);
    return like_match(p.prog.data(), (uint32_t)p.prog.size(), p.anchor_end, LikeRunes{r.data(), (uint32_t)r.size()});
}

void like_match_block_host(const std::vector<LikePattern>& pats, uint64_t n, const uint64_t* offsets, const uint8_t* bytes, uint8_t* bits) {
    std::vector<uint32_t> r;
    for (uint64_t i = 0; i < n; i++) {
        const uint8_t* s = bytes + (offsets[i] - offsets[0]);
        const uint32_t len = (uint32_t)(offsets[i + 1] - offsets[i]);
        uint8_t b = 0;
        if (like_utf8_valid(s, len)) {
            for (size_t p = 0; p < pats.size(); p++)
                b |= (uint8_t)(like_match(pats[p].prog.data(), (uint32_t)pats[p].prog.size(), pats[p].anchor_end, LikeBytes{s, len}) ? 1u << p : 0u);
        } else {
            like_decode_runes(s, len, r);
            for (size_t p = 0; p < pats.size(); p++)
                b |= (uint8_t)(like_match(pats[p].prog.data(), (uint32_t)pats[p].prog.size(), pats[p].anchor_end, LikeRunes{r.data(), (uint32_t)r.size()}) ? 1u << p : 0u);
        }
        bits[i] |= b;
    }
}

bool like_dev_patterns(const std::vector<LikePattern>& pats, LikeDevPatterns& out) {
    memset(&out, 0, sizeof out);
    if (pats.size() > kMatchBits) return false;
    out.npat = (uint32_t)pats.size();
    for (size_t p = 0; p < pats.size(); p++) {
        if (pats[p].prog.size() > kLikeDevProgBytes) return false;
        out.plen[p] = (uint8_t)pats[p].prog.size();
        out.anchor_end[p] = pats[p].anchor_end ? 1 : 0;
        if (!pats[p].prog.empty()) memcpy(out.prog[p], pats[p].prog.data(), pats[p].prog.size());
    }
    return true;
}

}  // namespace n1k
