// n1k_matchtable.cpp — the match table on the host side: like_bits[code] bit p = LIKE pattern p matches dictionary entry
// `code`, bit 7 - q = collection predicate q holds for it, the bits between = the IN lists that hold it.  One driver for
// "evaluate a block of entries on the device" (match_block_device), the handle's table around it (ensure_like) and the six
// diagnostic entry points of the C ABI.
#include "n1k_engine.h"

using namespace n1k;
using namespace n1k_eng;

namespace {

struct EntryBlock {
    uint64_t n;
    const uint64_t* off;   // n + 1; entry i = bytes[off[i] - off[0], off[i + 1] - off[0])
    const uint8_t* bytes;
    const uint8_t* at(uint64_t i) const { return bytes + (off[i] - off[0]); }
};

struct MatchCounts {
    uint64_t like_dev = 0, like_host = 0;  // strings matched by like_match_kernel / by the host matcher
    uint64_t coll_dev = 0, coll_host = 0;  // arrays evaluated by coll_match_kernel / by the host evaluator
    uint64_t in_dev = 0, in_host = 0;      // strings looked up by in_match_kernel / by the host matcher
};

uint64_t count_array_text(const EntryBlock& B) {
    uint64_t k = 0;
    for (uint64_t i = 0; i < B.n; i++) k += coll_array_text(B.at(i), B.off[i + 1] - B.off[i]);
    return k;
}

#define HIP_RET(expr)                      \
    do {                                   \
        const hipError_t _e = (expr);      \
        if (_e != hipSuccess) return _e;   \
    } while (0)

// The block through the kernels: `like` (its patterns filled in by like_dev_patterns; nullptr: no LIKE here), `coll`
// (nullptr: no ANY / EVERY here) and / or `in` (its table in device memory, `in_host` the same table on the host; nullptr:
// no IN here), ONE upload, one launch per kind, one synchronisation; what a kernel left goes through the
// host matchers.  The final bytes land at d_dst (device; nullptr: nowhere) and, whenever the host came to hold them, in
// bits[0, n) — always with d_dst == nullptr.  LIKE alone writes d_dst from the kernel, and the bytes come back only when
// some string was left; ANY / EVERY and IN (alone or beside LIKE) are merged on the host and written once.
hipError_t match_block_device(MatchScratch& S, const EntryBlock& B, LikeKernelArgs* like, const std::vector<LikePattern>& pats,
                              const std::vector<CollPred>* coll, uint32_t first_bit, InKernelArgs* in, const InTable* in_host,
                              hipStream_t st, uint8_t* d_dst, uint8_t* bits, MatchCounts& c) {
    const uint64_t n = B.n, nbytes = B.off[n] - B.off[0];
    HIP_RET(hipStreamSynchronize(st));  // (the scratch buffers may still be read by the last extension)
    HIP_RET(S.bytes.ensure(nbytes + 16));
    HIP_RET(S.off.ensure(n + 1));
    HIP_RET(S.left.ensure(3 * n));
    if (coll || in || !d_dst) HIP_RET(S.bits.ensure(3 * n));
    if (nbytes) HIP_RET(hipMemcpy(S.bytes.p, B.bytes, nbytes, hipMemcpyHostToDevice));
    HIP_RET(hipMemcpy(S.off.p, B.off, (n + 1) * 8, hipMemcpyHostToDevice));
    if (coll) {
        HIP_RET(S.progs.ensure(coll->size() * sizeof(CollProg)));
        for (size_t q = 0; q < coll->size(); q++)
            HIP_RET(hipMemcpy(S.progs.p + q * sizeof(CollProg), &(*coll)[q].prog, sizeof(CollProg), hipMemcpyHostToDevice));
    }
    const EntryBlockArgs blk{S.bytes.p, S.off.p, (uint32_t)n, 0, nullptr, nullptr};
    uint8_t* const d_like_bits = d_dst ? d_dst : S.bits.p;
    const bool merge = coll || in;                         // kinds whose bits the host merges and writes once
    const bool like_bits_up = like && (merge || !d_dst);  // the host merges or returns them: read with the flags
    if (like) {
        like->blk = blk;
        like->blk.out_bits = d_like_bits;
        like->blk.out_left = S.left.p;
        HIP_RET(launch_like_match(*like, st));
    }
    std::vector<uint8_t> left(3 * n), cb(coll ? n : 0), ib(in ? n : 0);
    if (coll) {
        CollKernelArgs C{blk, (uint32_t)coll->size(), first_bit, (const CollProg*)S.progs.p};
        C.blk.out_bits = S.bits.p + n;
        C.blk.out_left = S.left.p + n;
        HIP_RET(launch_coll_match(C, st));
        HIP_RET(hipMemcpyAsync(cb.data(), S.bits.p + n, n, hipMemcpyDeviceToHost, st));
    }
    if (in) {
        in->blk = blk;
        in->blk.out_bits = S.bits.p + 2 * n;
        in->blk.out_left = S.left.p + 2 * n;
        HIP_RET(launch_in_match(*in, st));
        HIP_RET(hipMemcpyAsync(ib.data(), S.bits.p + 2 * n, n, hipMemcpyDeviceToHost, st));
    }
    const uint64_t lo = like ? 0 : (coll ? n : 2 * n), hi = in ? 3 * n : (coll ? 2 * n : n);  // the flags of the kinds that ran (and of one that did not, between two that did: never read)
    HIP_RET(hipMemcpyAsync(left.data() + lo, S.left.p + lo, hi - lo, hipMemcpyDeviceToHost, st));
    if (like_bits_up) HIP_RET(hipMemcpyAsync(bits, d_like_bits, n, hipMemcpyDeviceToHost, st));
    HIP_RET(hipStreamSynchronize(st));
    uint64_t like_left = 0, coll_left = 0;
    if (like) {
        for (uint64_t i = 0; i < n; i++) like_left += left[i];
        if (like_left && !like_bits_up) HIP_RET(hipMemcpy(bits, d_like_bits, n, hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < n && like_left; i++)
            if (left[i]) like_match_block_host(pats, 1, &B.off[i], B.at(i), &bits[i]);
        c.like_dev += n - like_left;
        c.like_host += like_left;
    }
    if (coll) {
        for (uint64_t i = 0; i < n; i++) {
            if (left[n + i]) {  // (the kernel wrote 0 for it)
                coll_left++;
                coll_eval_block_host(*coll, first_bit, 1, &B.off[i], B.at(i), &cb[i]);
            }
            bits[i] = (uint8_t)((like ? bits[i] : 0) | cb[i]);
        }
        const uint64_t narr = count_array_text(B);
        c.coll_dev += narr - coll_left;
        c.coll_host += coll_left;
    }
    if (in) {
        uint64_t in_left = 0;
        for (uint64_t i = 0; i < n; i++) {
            if (left[2 * n + i]) {  // (the kernel wrote 0 for it)
                in_left++;
                in_match_block_host(*in_host, 1, &B.off[i], B.at(i), &ib[i]);
            }
            bits[i] = (uint8_t)((like || coll ? bits[i] : 0) | ib[i]);
        }
        c.in_dev += n - in_left;
        c.in_host += in_left;
    }
    if (d_dst && (merge || like_left)) HIP_RET(hipMemcpy(d_dst, bits, n, hipMemcpyHostToDevice));
    return hipSuccess;
}

}  // namespace

namespace n1k_eng {

// The handle's table.  Same rules as the rank table (ensure_rank), except that a grown dictionary EXTENDS it: the entries
// of the old codes stay as they are (equal bytes, equal code), only the new codes are evaluated — per kind on the host
// below kLikeDeviceThreshold / kCollDeviceThreshold / kInDeviceThreshold of them, by the kernels from there on (what a
// kernel leaves goes through the host matchers either way; patterns whose programs the LIKE kernel does not take stay with
// the host).  The constants of the plan's IN lists — the numbers the row term searches, the strings in_match_kernel
// probes — go to the device once, here, before the first launch.
n1k_status ensure_like(n1k_handle* h) {
    Program& P = h->prog;
    const std::vector<LikePattern>& pats = h->like_patterns;
    const std::vector<CollPred>& preds = h->coll_preds;
    const bool in_strings = h->in_string_lists != 0;
    InKernelArgs I{};
    if (!h->in_lists.empty() && !h->in_uploaded) {
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        if (!h->in_numbers.empty()) {
            HIP_TRY(h, h->d_in_nums.ensure(h->in_numbers.size()));
            HIP_TRY(h, hipMemcpy(h->d_in_nums.p, h->in_numbers.data(), h->in_numbers.size() * sizeof(double), hipMemcpyHostToDevice));
        }
        if (in_strings) {
            std::vector<uint8_t> blob;
            in_table_blob(h->in_table, blob);
            HIP_TRY(h, h->d_in_table.ensure(blob.size()));
            HIP_TRY(h, hipMemcpy(h->d_in_table.p, blob.data(), blob.size(), hipMemcpyHostToDevice));
        }
        h->in_uploaded = true;
    }
    P.in_nums = h->in_numbers.empty() ? nullptr : h->d_in_nums.p;
    P.in_n = (uint32_t)h->in_numbers.size();
    if (pats.empty() && preds.empty() && !in_strings) {
        P.like_bits = nullptr;
        P.like_n = 0;
        return N1K_OK;
    }
    const size_t n = h->dict.size(), first = h->like_built_for;
    if (n > first) {
        if (n + 4 > h->d_like.n) {  // (4 spare bytes: the kernels that stage the table in LDS copy whole words)
            // the table moves: launches in flight may still read the old allocation
            DevBuf<uint8_t> nb;
            HIP_TRY(h, nb.ensure(std::max(n, h->d_like.n * 2) + 4));
            hipError_t e = hipStreamSynchronize(h->stream);
            if (e == hipSuccess && first) e = hipMemcpy(nb.p, h->d_like.p, first, hipMemcpyDeviceToDevice);
            if (e != hipSuccess) nb.release();
            HIP_TRY(h, e);
            h->d_like.release();
            h->d_like = nb;
        }
        const size_t cnt = n - first;
        std::vector<uint64_t> off(cnt + 1);
        off[0] = 0;
        for (size_t i = 0; i < cnt; i++) off[i + 1] = off[i] + h->dict[first + i].size();
        std::vector<uint8_t> bytes(off[cnt] + 1);
        for (size_t i = 0; i < cnt; i++) memcpy(bytes.data() + off[i], h->dict[first + i].data(), h->dict[first + i].size());
        const EntryBlock B{cnt, off.data(), bytes.data()};
        const uint32_t top = kLikeMaxPatterns - 1;
        LikeKernelArgs A{};
        const bool like_dev = !pats.empty() && cnt >= kLikeDeviceThreshold && like_dev_patterns(pats, A.pat);
        const bool coll_dev = !preds.empty() && cnt >= kCollDeviceThreshold;
        const bool in_dev = in_strings && cnt >= kInDeviceThreshold;
        const bool like_host = !pats.empty() && !like_dev, coll_host = !preds.empty() && !coll_dev, in_host = in_strings && !in_dev;
        const bool dev = like_dev || coll_dev || in_dev, host = like_host || coll_host || in_host;
        const InTable in_tab = h->in_table.view();
        if (in_dev) I.tab = in_table_at(h->in_table, h->d_in_table.p);
        uint8_t* const dst = h->d_like.p + first;  // (entries no launch has been told about yet: like_n grows below)
        std::vector<uint8_t> bits(host ? cnt : 0, 0), dev_bits(dev ? cnt : 0);
        MatchCounts c;
        // the device's part goes straight to the table unless the host has bits of the other kind to add
        if (dev)
            HIP_TRY(h, match_block_device(h->match_scratch, B, like_dev ? &A : nullptr, pats, coll_dev ? &preds : nullptr, top,
                                          in_dev ? &I : nullptr, &in_tab, h->stream, host ? nullptr : dst, dev_bits.data(), c));
        if (like_host) {
            like_match_block_host(pats, cnt, B.off, B.bytes, bits.data());
            c.like_host += cnt;
        }
        if (coll_host) {
            coll_eval_block_host(preds, top, cnt, B.off, B.bytes, bits.data());
            c.coll_host += count_array_text(B);
        }
        if (in_host) {
            in_match_block_host(in_tab, cnt, B.off, B.bytes, bits.data());
            c.in_host += cnt;
        }
        if (host) {
            for (size_t i = 0; i < cnt && dev; i++) bits[i] |= dev_bits[i];
            HIP_TRY(h, hipMemcpy(dst, bits.data(), cnt, hipMemcpyHostToDevice));
        }
        h->like_on_device += c.like_dev;
        h->like_on_host += c.like_host;
        h->coll_on_device += c.coll_dev;
        h->coll_on_host += c.coll_host;
        h->in_on_device += c.in_dev;
        h->in_on_host += c.in_host;
        h->like_built_for = n;
    }
    P.like_bits = h->d_like.p;
    P.like_n = (uint32_t)h->like_built_for;
    return N1K_OK;
}

}  // namespace n1k_eng

// ---- the diagnostic entry points: the matchers on their own

// what all four check of their arguments (device: the kernels count entries in 32 bits)
static bool block_args_ok(const char* text, size_t text_len, uint64_t n, const uint64_t* offsets, const char* bytes, const uint8_t* out_bits,
                          bool device) {
    if ((text_len && !text) || (n && (!offsets || !out_bits)) || (device && n >= 0xFFFFFFF0ull)) return false;
    for (uint64_t i = 0; i < n; i++)
        if (offsets[i + 1] < offsets[i] || offsets[i + 1] - offsets[i] > 0x7FFFFFFFull) return false;
    return !(n && offsets[n] > offsets[0] && !bytes);
}

// one whole `any ... end` term -> program; N1K_UNSUPPORTED for what n1k_create refuses in a plan, N1K_INVALID for text
// that is no such term
static n1k_status coll_parse(const char* text, size_t len, std::vector<CollPred>& preds) {
    PlanError err;
    const std::string src(text ? text : "", len);
    auto e = parse_expression(src, err);
    if (!e) return err.unsupported ? N1K_UNSUPPORTED : N1K_INVALID;
    if (e->kind != EK::Coll) return N1K_INVALID;
    preds.resize(1);
    preds[0].text = src;
    if (!coll_compile(e.get(), preds[0].prog, err)) return err.unsupported ? N1K_UNSUPPORTED : N1K_INVALID;
    return N1K_OK;
}

// the bracketed list alone -> the table of its strings (bit 0); N1K_UNSUPPORTED for what n1k_create refuses in a plan,
// N1K_INVALID for text that is no list
static n1k_status in_parse(const char* text, size_t len, InTableHost& T) {
    PlanError err;
    const std::string src = "(`x` in " + std::string(text ? text : "", len) + ")";
    auto e = parse_expression(src, err);
    if (!e) return err.unsupported ? N1K_UNSUPPORTED : N1K_INVALID;
    if (e->kind != EK::In) return N1K_INVALID;
    std::vector<InList> lists(1);
    if (!in_compile(e.get(), lists[0], err)) return err.unsupported ? N1K_UNSUPPORTED : N1K_INVALID;
    lists[0].mask = lists[0].strings.empty() ? 0 : 1;
    in_build_table(lists, T);
    return N1K_OK;
}

// one kind through the driver on `device`, with scratch of its own
static n1k_status block_on_device(int device, const EntryBlock& B, LikeKernelArgs* like, const std::vector<LikePattern>& pats,
                                  const std::vector<CollPred>* coll, const InTableHost* in, uint8_t* out_bits, uint64_t* out_left_to_host) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev || hipSetDevice(device) != hipSuccess) return N1K_DEVICE_ERROR;
    struct Scratch : MatchScratch {
        DevBuf<uint8_t> in_table;
        ~Scratch() {
            release();
            in_table.release();
        }
    } S;
    MatchCounts c;
    InKernelArgs I{};
    InTable in_host{};
    if (in) {
        std::vector<uint8_t> blob;
        in_table_blob(*in, blob);
        if (S.in_table.ensure(blob.size()) != hipSuccess || hipMemcpy(S.in_table.p, blob.data(), blob.size(), hipMemcpyHostToDevice) != hipSuccess)
            return N1K_DEVICE_ERROR;
        I.tab = in_table_at(*in, S.in_table.p);
        in_host = in->view();
    }
    if (match_block_device(S, B, like, pats, coll, 0, in ? &I : nullptr, &in_host, nullptr, nullptr, out_bits, c) != hipSuccess) return N1K_DEVICE_ERROR;
    if (out_left_to_host) *out_left_to_host = c.like_host + c.coll_host + c.in_host;
    return N1K_OK;
}

extern "C" {

n1k_status n1k_like_match(const char* pattern, size_t pattern_len, uint64_t n, const uint64_t* offsets, const char* bytes, uint8_t* out_bits) {
    return guarded(nullptr, [&]() -> n1k_status {
    if (!block_args_ok(pattern, pattern_len, n, offsets, bytes, out_bits, false)) return N1K_INVALID;
    std::vector<LikePattern> pats(1);
    if (!like_compile(pattern ? pattern : "", pattern_len, pats[0])) return N1K_INVALID;
    like_match_block_host(pats, n, offsets, (const uint8_t*)bytes, out_bits);
    return N1K_OK;
    });
}

n1k_status n1k_like_match_device(int device, const char* pattern, size_t pattern_len, uint64_t n, const uint64_t* offsets, const char* bytes,
                                 uint8_t* out_bits, uint64_t* out_left_to_host) {
    return guarded(nullptr, [&]() -> n1k_status {
    if (!block_args_ok(pattern, pattern_len, n, offsets, bytes, out_bits, true)) return N1K_INVALID;
    std::vector<LikePattern> pats(1);
    if (!like_compile(pattern ? pattern : "", pattern_len, pats[0])) return N1K_INVALID;
    if (out_left_to_host) *out_left_to_host = 0;
    if (n == 0) return N1K_OK;
    LikeKernelArgs A{};
    if (!like_dev_patterns(pats, A.pat)) {  // a program the kernel does not take: every string is the host's
        like_match_block_host(pats, n, offsets, (const uint8_t*)bytes, out_bits);
        if (out_left_to_host) *out_left_to_host = n;
        return N1K_OK;
    }
    return block_on_device(device, EntryBlock{n, offsets, (const uint8_t*)bytes}, &A, pats, nullptr, nullptr, out_bits, out_left_to_host);
    });
}

n1k_status n1k_coll_eval(const char* predicate_text, size_t len, uint64_t n, const uint64_t* offsets, const char* bytes, uint8_t* out_bits) {
    return guarded(nullptr, [&]() -> n1k_status {
    if (!block_args_ok(predicate_text, len, n, offsets, bytes, out_bits, false)) return N1K_INVALID;
    std::vector<CollPred> preds;
    const n1k_status st = coll_parse(predicate_text, len, preds);
    if (st != N1K_OK) return st;
    if (n) memset(out_bits, 0, n);
    coll_eval_block_host(preds, 0, n, offsets, (const uint8_t*)bytes, out_bits);
    return N1K_OK;
    });
}

n1k_status n1k_coll_eval_device(int device, const char* predicate_text, size_t len, uint64_t n, const uint64_t* offsets, const char* bytes,
                                uint8_t* out_bits, uint64_t* out_left_to_host) {
    return guarded(nullptr, [&]() -> n1k_status {
    if (!block_args_ok(predicate_text, len, n, offsets, bytes, out_bits, true)) return N1K_INVALID;
    std::vector<CollPred> preds;
    const n1k_status st = coll_parse(predicate_text, len, preds);
    if (st != N1K_OK) return st;
    if (out_left_to_host) *out_left_to_host = 0;
    if (n == 0) return N1K_OK;
    return block_on_device(device, EntryBlock{n, offsets, (const uint8_t*)bytes}, nullptr, {}, &preds, nullptr, out_bits, out_left_to_host);
    });
}

n1k_status n1k_in_match(const char* list_text, size_t len, uint64_t n, const uint64_t* offsets, const char* bytes, uint8_t* out_bits) {
    return guarded(nullptr, [&]() -> n1k_status {
    if (!block_args_ok(list_text, len, n, offsets, bytes, out_bits, false)) return N1K_INVALID;
    InTableHost T;
    const n1k_status st = in_parse(list_text, len, T);
    if (st != N1K_OK) return st;
    if (n) memset(out_bits, 0, n);
    in_match_block_host(T.view(), n, offsets, (const uint8_t*)bytes, out_bits);
    return N1K_OK;
    });
}

n1k_status n1k_in_match_device(int device, const char* list_text, size_t len, uint64_t n, const uint64_t* offsets, const char* bytes,
                               uint8_t* out_bits, uint64_t* out_left_to_host) {
    return guarded(nullptr, [&]() -> n1k_status {
    if (!block_args_ok(list_text, len, n, offsets, bytes, out_bits, true)) return N1K_INVALID;
    InTableHost T;
    const n1k_status st = in_parse(list_text, len, T);
    if (st != N1K_OK) return st;
    if (out_left_to_host) *out_left_to_host = 0;
    if (n == 0) return N1K_OK;
    if (T.c_mask.empty()) {  // a list without strings holds no entry: nothing to launch
        memset(out_bits, 0, n);
        return N1K_OK;
    }
    return block_on_device(device, EntryBlock{n, offsets, (const uint8_t*)bytes}, nullptr, {}, nullptr, &T, out_bits, out_left_to_host);
    });
}

}  // extern "C"
