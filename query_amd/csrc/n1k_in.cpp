// n1k_in.cpp — IN over a constant list on the host: the list of a parsed term by class, the shared table of string
// constants, the host matcher (the algorithm itself is in n1k_in.h).
#include "n1k_in.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <unordered_map>
#include <unordered_set>

#include "n1k_plan.h"

namespace n1k {

bool in_compile(const Expr* e, InList& out, PlanError& err) {
    out = InList{};
    if (!e || e->kind != EK::In || e->ch.empty()) {
        err.msg = "not an IN term";
        return false;
    }
    auto refuse = [&](const std::string& what) {
        err.unsupported = true;
        err.msg = "IN: " + what + " is outside the device subset (in: " + (e->text.size() > 160 ? e->text.substr(0, 160) + " ..." : e->text) + ")";
        return false;
    };
    out.text = e->text;
    out.empty = e->ch.size() == 1;
    std::unordered_set<std::string> seen;
    for (size_t k = 1; k < e->ch.size(); k++) {
        const Expr* c = e->ch[k].get();
        if (c->kind != EK::Const) return refuse("a list element that is not a constant");
        switch (c->ctag) {
            case T_STRING:
                if (seen.insert(c->cstr).second) out.strings.push_back(c->cstr);
                break;
            case T_INT:
            case T_FLOAT: {
                // beyond +-2^53 ordering by float64 and exact INT equality part ways (2^53 and 2^53 + 1 are one double)
                const double d = c->ctag == T_INT ? (double)(int64_t)c->cpayload : [&] { double x; memcpy(&x, &c->cpayload, 8); return x; }();
                const bool exact = c->ctag != T_INT || ((int64_t)c->cpayload >= -(1ll << 53) && (int64_t)c->cpayload <= (1ll << 53));
                if (!exact || !(std::fabs(d) <= 9007199254740992.0)) return refuse("a number constant beyond +-2^53");
                out.numbers.push_back(d);
                break;
            }
            case T_TRUE: out.has_true = true; break;
            case T_FALSE: out.has_false = true; break;
            case T_NULL: out.has_null = true; break;
            default: return refuse("a list element `missing`");
        }
    }
    if (out.strings.size() > kInMaxStrings) return refuse("more than " + std::to_string(kInMaxStrings) + " distinct strings in one list");
    std::sort(out.numbers.begin(), out.numbers.end());
    out.numbers.erase(std::unique(out.numbers.begin(), out.numbers.end()), out.numbers.end());  // (3 and 3.0 are one constant under Equals)
    return true;
}

void in_build_table(const std::vector<InList>& lists, InTableHost& out) {
    out = InTableHost{};
    std::unordered_map<std::string, uint32_t> index;
    std::vector<const std::string*> consts;
    for (const InList& l : lists) {
        if (!l.mask) continue;
        for (const std::string& s : l.strings) {
            auto it = index.find(s);
            if (it == index.end()) {
                it = index.emplace(s, (uint32_t)consts.size()).first;
                consts.push_back(&it->first);
                out.c_mask.push_back(0);
            }
            out.c_mask[it->second] |= l.mask;
        }
    }
    out.c_off.push_back(0);
    for (const std::string* s : consts) {
        out.c_bytes.insert(out.c_bytes.end(), s->begin(), s->end());
        out.c_off.push_back((uint32_t)out.c_bytes.size());
    }
    size_t nslots = 16;
    while (nslots < 2 * consts.size()) nslots <<= 1;
    out.slots.assign(nslots, 0);
    for (size_t k = 0; k < consts.size(); k++) {
        uint32_t i = in_hash((const uint8_t*)consts[k]->data(), (uint32_t)consts[k]->size()) & (uint32_t)(nslots - 1);
        while (out.slots[i]) i = (i + 1) & (uint32_t)(nslots - 1);
        out.slots[i] = (uint32_t)k + 1;
    }
}

void in_match_block_host(const InTable& T, uint64_t n, const uint64_t* offsets, const uint8_t* bytes, uint8_t* bits) {
    for (uint64_t i = 0; i < n; i++)
        bits[i] |= in_lookup(T, bytes + (offsets[i] - offsets[0]), (uint32_t)(offsets[i + 1] - offsets[i]));
}

// slots | c_off | c_mask | c_bytes (the two word arrays first: aligned)
void in_table_blob(const InTableHost& T, std::vector<uint8_t>& blob) {
    blob.resize(T.slots.size() * 4 + T.c_off.size() * 4 + T.c_mask.size() + T.c_bytes.size() + 16);
    uint8_t* p = blob.data();
    memcpy(p, T.slots.data(), T.slots.size() * 4);
    p += T.slots.size() * 4;
    memcpy(p, T.c_off.data(), T.c_off.size() * 4);
    p += T.c_off.size() * 4;
    if (!T.c_mask.empty()) memcpy(p, T.c_mask.data(), T.c_mask.size());
    p += T.c_mask.size();
    if (!T.c_bytes.empty()) memcpy(p, T.c_bytes.data(), T.c_bytes.size());
}

InTable in_table_at(const InTableHost& T, const uint8_t* base) {
    InTable v = T.view();
    v.slots = (const uint32_t*)base;
    v.c_off = (const uint32_t*)(base + T.slots.size() * 4);
    v.c_mask = base + T.slots.size() * 4 + T.c_off.size() * 4;
    v.c_bytes = v.c_mask + T.c_mask.size();
    return v;
}

}  // namespace n1k
