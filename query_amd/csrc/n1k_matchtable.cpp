// n1k_matchtable.cpp — the match table on the host side ("The match table"): the plan's predicates and their
// bits of the four kinds (MatchTable's adders, finalize_bits), ONE driver that takes a block of dictionary entries through every kind's
// route (match_block), the handle's table around it (ensure_match_table) and the diagnostic entry points of the C ABI.
#include "n1k_engine.h"

using namespace n1k;
using namespace n1k_eng;

// ---- the plan side: which predicate owns which bit

namespace n1k_eng {

// The eight bits of an entry are shared by the four kinds: one more predicate that needs a bit, or refused.
static bool take_bit(const MatchTable& M, PlanError& err) {
    if (M.patterns.size() + M.preds.size() + M.string_lists + M.strfns.size() < kMatchBits) return true;
    err.unsupported = true;
    err.msg = "more than " + std::to_string(kMatchBits) + " distinct LIKE patterns, ANY / EVERY predicates, IN lists of strings and string-function predicates in one plan";
    return false;
}

int MatchTable::add_like(const std::string& pattern, PlanError& err) {
    for (size_t ix = 0; ix < patterns.size(); ix++)
        if (patterns[ix].text == pattern) return (int)ix;
    if (!take_bit(*this, err)) return -1;
    LikePattern lp;
    if (!like_compile(pattern.data(), pattern.size(), lp)) {
        err.unsupported = true;
        err.msg = "LIKE pattern is not valid UTF-8 (the reference's regexp.Compile fails on it)";
        return -1;
    }
    patterns.push_back(std::move(lp));
    return (int)patterns.size() - 1;
}

int MatchTable::add_coll(const Expr* e, PlanError& err) {  // (the text holds the binding expression too)
    for (size_t ix = 0; ix < preds.size(); ix++)
        if (preds[ix].text == e->text) return (int)ix;
    if (!take_bit(*this, err)) return -1;
    CollPred cp;
    cp.text = e->text;
    if (!coll_compile(e, cp.prog, err)) return -1;
    preds.push_back(std::move(cp));
    return (int)preds.size() - 1;
}

int MatchTable::add_in(const Expr* e, PlanError& err) {
    for (size_t ix = 0; ix < lists.size(); ix++)
        if (lists[ix].text == e->text) return (int)ix;
    InList il;
    if (!in_compile(e, il, err)) return -1;
    if (!il.strings.empty() && !take_bit(*this, err)) return -1;  // (a list without strings takes no bit)
    if (in_numbers.size() + il.numbers.size() > kInMaxNumbers) {
        err.unsupported = true;
        err.msg = "more than " + std::to_string(kInMaxNumbers) + " distinct number constants in the IN lists of one plan";
        return -1;
    }
    il.num_begin = (uint32_t)in_numbers.size();
    in_numbers.insert(in_numbers.end(), il.numbers.begin(), il.numbers.end());
    il.num_end = (uint32_t)in_numbers.size();
    if (!il.strings.empty()) string_lists++;
    lists.push_back(std::move(il));
    return (int)lists.size() - 1;
}

int MatchTable::add_strfn(const Expr* e, const Expr*& path, PlanError& err) {
    StrFnPred sp;
    if (!strfn_compile(e, sp.prog, path, err)) return -1;
    for (size_t ix = 0; ix < strfns.size(); ix++)  // (equal programs, whatever their text: ("a" < f(x)) and (f(x) > "a") share)
        if (!memcmp(&strfns[ix].prog, &sp.prog, sizeof sp.prog)) return (int)ix;
    if (!take_bit(*this, err)) return -1;
    strfns.push_back(sp);
    return (int)strfns.size() - 1;
}

// THE bit scheme: LIKE pattern p owns bit p; the IN lists that hold strings own the next bits above, in the order of their
// first use; the string-function predicates the bits above those, in the order of their first use; collection predicate q
// owns bit coll_top - q, from bit 7 down.  A TERM_IN carries its list's flags beside the mask.
void MatchTable::finalize_bits(Program& P) {
    uint32_t in_bit = (uint32_t)patterns.size();
    for (InList& l : lists)
        if (!l.strings.empty()) l.mask = (uint8_t)(1u << in_bit++);
    strfn_first = in_bit;
    for (uint32_t t = 0; t < P.nterms; t++) {
        uint64_t& ix = P.terms[t].b.cpayload;  // the predicate's index (compile_cond) -> what the row test reads
        if (P.terms[t].op == TERM_COLL) ix = coll_top - ix;
        if (P.terms[t].op == TERM_STRFN) ix = strfn_first + ix;
        if (P.terms[t].op == TERM_IN) {
            const InList& l = lists[(size_t)ix];
            ix = l.mask | (l.has_true ? IN_HAS_TRUE : 0u) | (l.has_false ? IN_HAS_FALSE : 0u) | (l.has_null ? IN_HAS_NULL : 0u) | (l.empty ? IN_EMPTY : 0u);
        }
    }
    in_build_table(lists, in_table);
    in_uploaded = false;
}

}  // namespace n1k_eng

// ---- the driver

namespace {

struct EntryBlock {
    uint64_t n;
    const uint64_t* off;   // n + 1; entry i = bytes[off[i] - off[0], off[i + 1] - off[0])
    const uint8_t* bytes;
    const uint8_t* at(uint64_t i) const { return bytes + (off[i] - off[0]); }
};

#define HIP_RET(expr)                      \
    do {                                   \
        const hipError_t _e = (expr);      \
        if (_e != hipSuccess) return _e;   \
    } while (0)

// where each kind of one block goes; like: the LIKE kernel's arguments, its patterns filled in when LIKE goes to the device
enum Route : uint8_t { R_NONE, R_HOST, R_DEVICE };
struct Routes {
    Route r[MK_COUNT];
    uint32_t ndev = 0, nhost = 0;
    LikeKernelArgs like{};
};

// What a kind tells the driver: whether the plan holds it, ...
bool kind_present(const MatchTable& M, int k) {
    switch (k) {
        case MK_LIKE: return !M.patterns.empty();
        case MK_COLL: return !M.preds.empty();
        case MK_IN: return M.string_lists != 0;
        default: return !M.strfns.empty();
    }
}

// ... how many of a block's entries are its business (what its two counters add up to), ...
uint64_t kind_business(int k, const EntryBlock& B) {
    if (k != MK_COLL) return B.n;
    uint64_t narr = 0;
    for (uint64_t i = 0; i < B.n; i++) narr += coll_array_text(B.at(i), B.off[i + 1] - B.off[i]);
    return narr;
}

// ... its host matcher over entries [0, n) of (off, bytes) — every one ORs its bits into bits[i], none assumes a zeroed
// destination — ...
void kind_host(const MatchTable& M, int k, uint64_t n, const uint64_t* off, const uint8_t* bytes, uint8_t* bits) {
    switch (k) {
        case MK_LIKE: like_match_block_host(M.patterns, n, off, bytes, bits); break;
        case MK_COLL: coll_eval_block_host(M.preds, M.coll_top, n, off, bytes, bits); break;
        case MK_IN: in_match_block_host(M.in_table.view(), n, off, bytes, bits); break;
        default: strfn_eval_block_host(M.strfns, M.strfn_first, n, off, bytes, bits);
    }
}

// ... and its kernel over the uploaded block
hipError_t kind_launch(MatchTable& M, Routes& R, int k, const EntryBlockArgs& blk, hipStream_t st) {
    switch (k) {
        case MK_LIKE: R.like.blk = blk; return launch_like_match(R.like, st);
        case MK_COLL: return launch_coll_match(CollKernelArgs{blk, (uint32_t)M.preds.size(), M.coll_top, (const CollProg*)M.scratch.progs.p}, st);
        case MK_IN: return launch_in_match(InKernelArgs{blk, in_table_at(M.in_table, M.d_in_table.p)}, st);
        default: return launch_strfn_match(StrFnKernelArgs{blk, (uint32_t)M.strfns.size(), M.strfn_first, (const StrFnProg*)M.scratch.sprogs.p}, st);
    }
}

// A kind the plan holds goes to the device where the caller wants it there (the thresholds; the device flavour of a
// diagnostic entry point) — LIKE only with programs its kernel takes — and to the host otherwise.
void choose_routes(const MatchTable& M, const bool want_dev[MK_COUNT], Routes& R) {
    for (int k = 0; k < MK_COUNT; k++) {
        const bool dev = kind_present(M, k) && want_dev[k] && (k != MK_LIKE || like_dev_patterns(M.patterns, R.like.pat));
        R.r[k] = dev ? R_DEVICE : (kind_present(M, k) ? R_HOST : R_NONE);
        R.ndev += R.r[k] == R_DEVICE;
        R.nhost += R.r[k] == R_HOST;
    }
}

// The constants of the plan's IN lists — the numbers the row term searches, the strings in_match_kernel probes — go to the
// device once, before the first launch.
hipError_t upload_in_constants(MatchTable& M, hipStream_t st) {
    if (M.lists.empty() || M.in_uploaded) return hipSuccess;
    HIP_RET(hipStreamSynchronize(st));
    if (!M.in_numbers.empty()) {
        HIP_RET(M.d_in_nums.ensure(M.in_numbers.size()));
        HIP_RET(hipMemcpy(M.d_in_nums.p, M.in_numbers.data(), M.in_numbers.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    if (M.string_lists) {
        std::vector<uint8_t> blob;
        in_table_blob(M.in_table, blob);
        HIP_RET(M.d_in_table.ensure(blob.size()));
        HIP_RET(hipMemcpy(M.d_in_table.p, blob.data(), blob.size(), hipMemcpyHostToDevice));
    }
    M.in_uploaded = true;
    return hipSuccess;
}

// One block of entries through every kind's route.  The kinds on the device: ONE upload, one launch per kind, one
// synchronisation; what a kernel flagged `left` (it wrote 0 for it) goes through that kind's host matcher one by one.  The
// kinds on the host: their matchers over the whole block.  The final bytes land at d_dst (device memory; nullptr: nowhere)
// and, unless the direct rule held and nothing was left, in bits[0, n).
// The direct rule: exactly one kind on the device and none on the host — its kernel writes straight to d_dst, only its
// flags come back, and the bytes are read back and patched only if some entry was left.  Otherwise the host merges the
// kinds' bits and writes d_dst once.
hipError_t match_block(MatchTable& M, const EntryBlock& B, Routes& R, hipStream_t st, uint8_t* d_dst, uint8_t* bits) {
    MatchScratch& S = M.scratch;
    const uint64_t n = B.n, nbytes = B.off[n] - B.off[0];
    const bool direct = d_dst && R.ndev == 1 && R.nhost == 0;
    std::vector<uint8_t> left, kbits;  // the kernels' flags and bits, kind k at k * n
    if (R.ndev) {
        HIP_RET(hipStreamSynchronize(st));  // (the scratch buffers may still be read by the last extension)
        HIP_RET(S.bytes.ensure(nbytes + 16));
        HIP_RET(S.off.ensure(n + 1));
        HIP_RET(S.left.ensure(MK_COUNT * n));
        if (!direct) HIP_RET(S.bits.ensure(MK_COUNT * n));
        if (nbytes) HIP_RET(hipMemcpy(S.bytes.p, B.bytes, nbytes, hipMemcpyHostToDevice));
        HIP_RET(hipMemcpy(S.off.p, B.off, (n + 1) * 8, hipMemcpyHostToDevice));
        if (R.r[MK_COLL] == R_DEVICE) {
            HIP_RET(S.progs.ensure(M.preds.size() * sizeof(CollProg)));
            for (size_t q = 0; q < M.preds.size(); q++)
                HIP_RET(hipMemcpy(S.progs.p + q * sizeof(CollProg), &M.preds[q].prog, sizeof(CollProg), hipMemcpyHostToDevice));
        }
        if (R.r[MK_STRFN] == R_DEVICE) {
            HIP_RET(S.sprogs.ensure(M.strfns.size() * sizeof(StrFnProg)));
            for (size_t q = 0; q < M.strfns.size(); q++)
                HIP_RET(hipMemcpy(S.sprogs.p + q * sizeof(StrFnProg), &M.strfns[q].prog, sizeof(StrFnProg), hipMemcpyHostToDevice));
        }
        left.resize(MK_COUNT * n);
        kbits.resize(direct ? 0 : MK_COUNT * n);
        for (int k = 0; k < MK_COUNT; k++)
            if (R.r[k] == R_DEVICE)
                HIP_RET(kind_launch(M, R, k, EntryBlockArgs{S.bytes.p, S.off.p, (uint32_t)n, 0, direct ? d_dst : S.bits.p + k * n, S.left.p + k * n}, st));
        for (int k = 0; k < MK_COUNT; k++) {  // only the slices of the kinds that ran
            if (R.r[k] != R_DEVICE) continue;
            HIP_RET(hipMemcpyAsync(left.data() + k * n, S.left.p + k * n, n, hipMemcpyDeviceToHost, st));
            if (!direct) HIP_RET(hipMemcpyAsync(kbits.data() + k * n, S.bits.p + k * n, n, hipMemcpyDeviceToHost, st));
        }
        HIP_RET(hipStreamSynchronize(st));
    }
    uint64_t nleft[MK_COUNT] = {}, any_left = 0;
    for (int k = 0; k < MK_COUNT; k++) {
        if (R.r[k] != R_DEVICE) continue;
        for (uint64_t i = 0; i < n; i++) nleft[k] += left[k * n + i];
        any_left += nleft[k];
    }
    if (!direct) {
        memset(bits, 0, n);
        for (int k = 0; k < MK_COUNT; k++)
            for (uint64_t i = 0; i < n && R.r[k] == R_DEVICE; i++) bits[i] |= kbits[k * n + i];
    } else if (any_left) {
        HIP_RET(hipMemcpy(bits, d_dst, n, hipMemcpyDeviceToHost));
    }
    for (int k = 0; k < MK_COUNT; k++) {
        if (R.r[k] == R_NONE) continue;
        const uint64_t business = kind_business(k, B);
        if (R.r[k] == R_HOST) {
            kind_host(M, k, n, B.off, B.bytes, bits);
            M.counts[k].host += business;
            continue;
        }
        for (uint64_t i = 0; i < n && nleft[k]; i++)
            if (left[k * n + i]) kind_host(M, k, 1, &B.off[i], B.at(i), &bits[i]);
        M.counts[k].dev += business - nleft[k];
        M.counts[k].host += nleft[k];
    }
    if (d_dst && (!direct || any_left)) HIP_RET(hipMemcpy(d_dst, bits, n, hipMemcpyHostToDevice));
    return hipSuccess;
}

}  // namespace

namespace n1k_eng {

// The handle's table.  Same rules as the rank table (ensure_rank), except that a grown dictionary EXTENDS it: the entries
// of the old codes stay as they are (equal bytes, equal code), only the new codes are evaluated — per kind on the host
// below kLikeDeviceThreshold / kCollDeviceThreshold / kInDeviceThreshold / kStrFnDeviceThreshold of them, by the kernels
// from there on.
n1k_status ensure_match_table(n1k_handle* h) {
    Program& P = h->prog;
    MatchTable& M = h->match;
    HIP_TRY(h, upload_in_constants(M, h->stream));
    P.in_nums = M.in_numbers.empty() ? nullptr : M.d_in_nums.p;  // (bound also when the plan holds no kind of the table)
    P.in_n = (uint32_t)M.in_numbers.size();
    if (M.patterns.empty() && M.preds.empty() && !M.string_lists && M.strfns.empty()) {
        P.match_bits = nullptr;
        P.match_n = 0;
        return N1K_OK;
    }
    const size_t n = h->dict.size(), first = M.built_for;
    if (n > first) {
        if (n + 4 > M.d_bits.n) {  // (4 spare bytes: the kernels that stage the table in LDS copy whole words)
            // the table moves: launches in flight may still read the old allocation
            DevBuf<uint8_t> nb;
            HIP_TRY(h, nb.ensure(std::max(n, M.d_bits.n * 2) + 4));
            hipError_t e = hipStreamSynchronize(h->stream);
            if (e == hipSuccess && first) e = hipMemcpy(nb.p, M.d_bits.p, first, hipMemcpyDeviceToDevice);
            HIP_TRY(h, e);
            M.d_bits = std::move(nb);
        }
        const size_t cnt = n - first;
        std::vector<uint64_t> off(cnt + 1);
        off[0] = 0;
        for (size_t i = 0; i < cnt; i++) off[i + 1] = off[i] + h->dict[first + i].size();
        std::vector<uint8_t> bytes(off[cnt] + 1), bits(cnt);
        for (size_t i = 0; i < cnt; i++) memcpy(bytes.data() + off[i], h->dict[first + i].data(), h->dict[first + i].size());
        const bool want_dev[MK_COUNT] = {cnt >= kLikeDeviceThreshold, cnt >= kCollDeviceThreshold, cnt >= kInDeviceThreshold, cnt >= kStrFnDeviceThreshold};
        Routes R;
        choose_routes(M, want_dev, R);
        // (d_bits + first: entries no launch has been told about yet, match_n grows below)
        HIP_TRY(h, match_block(M, EntryBlock{cnt, off.data(), bytes.data()}, R, h->stream, M.d_bits.p + first, bits.data()));
        M.built_for = n;
    }
    P.match_bits = M.d_bits.p;
    P.match_n = (uint32_t)M.built_for;
    return N1K_OK;
}

}  // namespace n1k_eng

// ---- the diagnostic entry points: one kind's matcher on its own, over a table of that one predicate (bit 0)

// what all eight check of their arguments (device: the kernels count entries in 32 bits)
static bool block_args_ok(const char* text, size_t text_len, uint64_t n, const uint64_t* offsets, const char* bytes, const uint8_t* out_bits,
                          bool device) {
    if ((text_len && !text) || (n && (!offsets || !out_bits)) || (device && n >= 0xFFFFFFF0ull)) return false;
    for (uint64_t i = 0; i < n; i++)
        if (offsets[i + 1] < offsets[i] || offsets[i + 1] - offsets[i] > 0x7FFFFFFFull) return false;
    return !(n && offsets[n] > offsets[0] && !bytes);
}

// the pattern -> its program
static n1k_status like_parse(const char* text, size_t len, MatchTable& M) {
    M.patterns.resize(1);
    return like_compile(text ? text : "", len, M.patterns[0]) ? N1K_OK : N1K_INVALID;
}

// one whole `any ... end` term -> program; N1K_UNSUPPORTED for what n1k_create refuses in a plan, N1K_INVALID for text
// that is no such term
static n1k_status coll_parse(const char* text, size_t len, MatchTable& M) {
    PlanError err;
    const std::string src(text ? text : "", len);
    auto e = parse_expression(src, err);
    if (!e) return err.unsupported ? N1K_UNSUPPORTED : N1K_INVALID;
    if (e->kind != EK::Coll) return N1K_INVALID;
    M.preds.resize(1);
    M.preds[0].text = src;
    M.coll_top = 0;
    if (!coll_compile(e.get(), M.preds[0].prog, err)) return err.unsupported ? N1K_UNSUPPORTED : N1K_INVALID;
    return N1K_OK;
}

// the bracketed list alone -> the table of its strings; N1K_UNSUPPORTED for what n1k_create refuses in a plan,
// N1K_INVALID for text that is no list.  (A list without strings holds no entry: not present, zeros without a launch.)
static n1k_status in_parse(const char* text, size_t len, MatchTable& M) {
    PlanError err;
    const std::string src = "(`x` in " + std::string(text ? text : "", len) + ")";
    auto e = parse_expression(src, err);
    if (!e) return err.unsupported ? N1K_UNSUPPORTED : N1K_INVALID;
    if (e->kind != EK::In) return N1K_INVALID;
    M.lists.resize(1);
    if (!in_compile(e.get(), M.lists[0], err)) return err.unsupported ? N1K_UNSUPPORTED : N1K_INVALID;
    M.string_lists = M.lists[0].strings.empty() ? 0 : 1;
    M.lists[0].mask = (uint8_t)M.string_lists;
    in_build_table(M.lists, M.in_table);
    return N1K_OK;
}

// one whole term over a path -> program; N1K_UNSUPPORTED for what n1k_create refuses in a plan, N1K_INVALID for text that
// is no such term
static n1k_status strfn_parse(const char* text, size_t len, MatchTable& M) {
    PlanError err;
    const std::string src(text ? text : "", len);
    auto e = parse_expression(src, err);
    if (!e) return err.unsupported ? N1K_UNSUPPORTED : N1K_INVALID;
    if (!strfn_term(e.get())) return N1K_INVALID;
    M.strfns.resize(1);
    const Expr* path = nullptr;
    if (!strfn_compile(e.get(), M.strfns[0].prog, path, err)) return err.unsupported ? N1K_UNSUPPORTED : N1K_INVALID;
    return N1K_OK;
}

// All eight: the block through the driver with the one kind `parse` compiles — through its host matcher, or (on_device) through
// its kernel on `device` with scratch of its own; a LIKE program the kernel does not take sends every string to the host.
static n1k_status match_alone(int kind, n1k_status (*parse)(const char*, size_t, MatchTable&), bool on_device, int device, const char* text,
                              size_t text_len, uint64_t n, const uint64_t* offsets, const char* bytes, uint8_t* out_bits, uint64_t* out_left_to_host) {
    return guarded(nullptr, [&]() -> n1k_status {
    if (!block_args_ok(text, text_len, n, offsets, bytes, out_bits, on_device)) return N1K_INVALID;
    MatchTable M;
    const n1k_status st = parse(text, text_len, M);
    if (st != N1K_OK) return st;
    if (out_left_to_host) *out_left_to_host = 0;
    if (n == 0) return N1K_OK;
    bool want_dev[MK_COUNT] = {};
    want_dev[kind] = on_device;
    Routes R;
    choose_routes(M, want_dev, R);
    if (R.ndev) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev || hipSetDevice(device) != hipSuccess) return N1K_DEVICE_ERROR;
        if (upload_in_constants(M, nullptr) != hipSuccess) return N1K_DEVICE_ERROR;
    }
    if (match_block(M, EntryBlock{n, offsets, (const uint8_t*)bytes}, R, nullptr, nullptr, out_bits) != hipSuccess) return N1K_DEVICE_ERROR;
    if (out_left_to_host) *out_left_to_host = M.counts[kind].host;
    return N1K_OK;
    });
}

extern "C" {

n1k_status n1k_like_match(const char* pattern, size_t pattern_len, uint64_t n, const uint64_t* offsets, const char* bytes, uint8_t* out_bits) {
    return match_alone(MK_LIKE, like_parse, false, 0, pattern, pattern_len, n, offsets, bytes, out_bits, nullptr);
}

n1k_status n1k_like_match_device(int device, const char* pattern, size_t pattern_len, uint64_t n, const uint64_t* offsets, const char* bytes,
                                 uint8_t* out_bits, uint64_t* out_left_to_host) {
    return match_alone(MK_LIKE, like_parse, true, device, pattern, pattern_len, n, offsets, bytes, out_bits, out_left_to_host);
}

n1k_status n1k_coll_eval(const char* predicate_text, size_t len, uint64_t n, const uint64_t* offsets, const char* bytes, uint8_t* out_bits) {
    return match_alone(MK_COLL, coll_parse, false, 0, predicate_text, len, n, offsets, bytes, out_bits, nullptr);
}

n1k_status n1k_coll_eval_device(int device, const char* predicate_text, size_t len, uint64_t n, const uint64_t* offsets, const char* bytes,
                                uint8_t* out_bits, uint64_t* out_left_to_host) {
    return match_alone(MK_COLL, coll_parse, true, device, predicate_text, len, n, offsets, bytes, out_bits, out_left_to_host);
}

n1k_status n1k_strfn_eval(const char* term_text, size_t len, uint64_t n, const uint64_t* offsets, const char* bytes, uint8_t* out_bits) {
    return match_alone(MK_STRFN, strfn_parse, false, 0, term_text, len, n, offsets, bytes, out_bits, nullptr);
}

n1k_status n1k_strfn_eval_device(int device, const char* term_text, size_t len, uint64_t n, const uint64_t* offsets, const char* bytes,
                                 uint8_t* out_bits, uint64_t* out_left_to_host) {
    return match_alone(MK_STRFN, strfn_parse, true, device, term_text, len, n, offsets, bytes, out_bits, out_left_to_host);
}

n1k_status n1k_in_match(const char* list_text, size_t len, uint64_t n, const uint64_t* offsets, const char* bytes, uint8_t* out_bits) {
    return match_alone(MK_IN, in_parse, false, 0, list_text, len, n, offsets, bytes, out_bits, nullptr);
}

n1k_status n1k_in_match_device(int device, const char* list_text, size_t len, uint64_t n, const uint64_t* offsets, const char* bytes,
                               uint8_t* out_bits, uint64_t* out_left_to_host) {
    return match_alone(MK_IN, in_parse, true, device, list_text, len, n, offsets, bytes, out_bits, out_left_to_host);
}

}  // extern "C"
