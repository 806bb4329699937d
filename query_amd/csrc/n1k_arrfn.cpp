// n1k_arrfn.cpp — the array functions on the host side ("Array functions"): a term's program from its
// expression (arrfn_compile), the plan's distinct terms (ArrFnTable::add), ONE driver that takes a block of dictionary
// entries through the host evaluator or through arrfn_table_kernel (arrfn_block), the handle's value tables around it
// (ensure_value_table) and the diagnostic entry points of the C ABI.  The evaluator itself, both flavours: n1k_arrfn.hip.
#include <cerrno>
#include <cstdlib>

#include "n1k_engine.h"

using namespace n1k;
using namespace n1k_eng;

namespace n1k {

bool arrfn_name(const std::string& f) {
    return f == "array_length" || f == "array_count" || f == "array_sum" || f == "array_avg" || f == "array_contains" || f == "array_position";
}

// the reference's decoder makes a float64 of every number (encoding/json into interface{}), value.NewValue folds an
// integral one to int64 (value/value.go:375-380; IsInt, value/integer.go:354-356)
int arrfn_number_host(const uint8_t* s, uint32_t b, uint32_t e, uint32_t& tag, uint64_t& payload) {
    const std::string z((const char*)s + b, (const char*)s + e);
    char* endp = nullptr;
    const double d = strtod(z.c_str(), &endp);
    if (z.empty() || !endp || *endp != 0) return 0;
    if (d >= -9223372036854775808.0 && d < 9223372036854775808.0 && d == (double)(int64_t)d) {
        tag = T_INT;
        payload = (uint64_t)(int64_t)d;
    } else {
        tag = T_FLOAT;
        memcpy(&payload, &d, 8);
    }
    return 1;
}

bool arrfn_compile(const Expr* e, ArrFnProg& out, PlanError& err) {
    memset(&out, 0, sizeof out);
    if (!e || e->kind != EK::Func || !arrfn_name(e->fname) || e->ch.empty() || e->ch[0]->kind != EK::Path) {
        err.msg = "not an array-function term";
        return false;
    }
    const std::string& f = e->fname;
    out.fn = f == "array_length" ? AF_LENGTH : f == "array_count" ? AF_COUNT : f == "array_sum" ? AF_SUM : f == "array_avg" ? AF_AVG
             : f == "array_contains" ? AF_CONTAINS : AF_POSITION;
    const bool binary = out.fn == AF_CONTAINS || out.fn == AF_POSITION;
    if (e->ch.size() != (binary ? 2u : 1u) || (binary && e->ch[1]->kind != EK::Const)) {
        err.msg = "not an array-function term";
        return false;
    }
    if (binary) {
        const Expr* c = e->ch[1].get();
        out.ctag = (uint8_t)c->ctag;
        out.c = c->ctag == T_INT || c->ctag == T_FLOAT ? c->cpayload : 0;
        if (c->ctag == T_STRING) {
            if (c->cstr.size() > kArrFnConstBytes) {
                err.unsupported = true;
                err.msg = f + " with a STRING constant of more than " + std::to_string(kArrFnConstBytes) + " bytes does not run on the device";
                return false;
            }
            out.clen = (uint16_t)c->cstr.size();
            memcpy(out.cstr, c->cstr.data(), c->cstr.size());
        }
    }
    return true;
}

}  // namespace n1k

namespace n1k_eng {

int ArrFnTable::add(const Expr* e, PlanError& err) {
    for (size_t ix = 0; ix < terms.size(); ix++)
        if (terms[ix].text == e->text) return (int)ix;
    if (terms.size() >= kArrFnMaxTerms) {
        err.unsupported = true;
        err.msg = "more than " + std::to_string(kArrFnMaxTerms) + " distinct array-function terms (array_length ... array_position) in one plan";
        return -1;
    }
    ArrFnTerm t;
    t.text = e->text;
    if (!arrfn_compile(e, t.prog, err)) return -1;
    terms.push_back(std::move(t));
    return (int)terms.size() - 1;
}

}  // namespace n1k_eng

namespace {

#define HIP_RET(expr)                      \
    do {                                   \
        const hipError_t _e = (expr);      \
        if (_e != hipSuccess) return _e;   \
    } while (0)

// One block of n entries (off: n + 1, bytes) through the terms of T: tags[q * n + i], payload[q * n + i].  on_device: through
// arrfn_table_kernel — one upload, one launch, one synchronisation — and what it flagged `left` through the host evaluator
// entry by entry; else the host evaluator over the whole block.  T's counters take the block's array entries.
hipError_t arrfn_block(ArrFnTable& T, bool on_device, uint64_t n, const uint64_t* off, const uint8_t* bytes, hipStream_t st, uint8_t* tags, uint64_t* payload) {
    const uint32_t nq = (uint32_t)T.terms.size();
    std::vector<ArrFnProg> progs(nq);
    for (uint32_t q = 0; q < nq; q++) progs[q] = T.terms[q].prog;
    uint64_t narr = 0;
    for (uint64_t i = 0; i < n; i++) narr += coll_array_text(bytes + (off[i] - off[0]), off[i + 1] - off[i]);
    if (!on_device) {
        arrfn_eval_block_host(progs.data(), nq, n, off, bytes, tags, payload, n);
        T.host += narr;
        return hipSuccess;
    }
    auto& S = T.scratch;
    const uint64_t nbytes = off[n] - off[0];
    HIP_RET(hipStreamSynchronize(st));  // (the scratch buffers may still be read by the last extension)
    HIP_RET(S.bytes.ensure(nbytes + 16));
    HIP_RET(S.off.ensure(n + 1));
    HIP_RET(S.left.ensure(n));
    HIP_RET(S.tags.ensure((uint64_t)nq * n));
    HIP_RET(S.payload.ensure((uint64_t)nq * n));
    HIP_RET(S.progs.ensure(nq * sizeof(ArrFnProg)));
    if (nbytes) HIP_RET(hipMemcpy(S.bytes.p, bytes, nbytes, hipMemcpyHostToDevice));
    HIP_RET(hipMemcpy(S.off.p, off, (n + 1) * 8, hipMemcpyHostToDevice));
    HIP_RET(hipMemcpy(S.progs.p, progs.data(), nq * sizeof(ArrFnProg), hipMemcpyHostToDevice));
    HIP_RET(launch_arrfn_table(ArrFnKernelArgs{S.bytes.p, S.off.p, (uint32_t)n, nq, (const ArrFnProg*)S.progs.p, S.tags.p, S.payload.p, n, S.left.p}, st));
    std::vector<uint8_t> left(n);
    HIP_RET(hipMemcpyAsync(left.data(), S.left.p, n, hipMemcpyDeviceToHost, st));
    HIP_RET(hipMemcpyAsync(tags, S.tags.p, (uint64_t)nq * n, hipMemcpyDeviceToHost, st));
    HIP_RET(hipMemcpyAsync(payload, S.payload.p, (uint64_t)nq * n * 8, hipMemcpyDeviceToHost, st));
    HIP_RET(hipStreamSynchronize(st));
    uint64_t nleft = 0;
    for (uint64_t i = 0; i < n; i++) {
        if (!left[i]) continue;
        nleft++;
        arrfn_eval_block_host(progs.data(), nq, 1, &off[i], bytes + (off[i] - off[0]), tags + i, payload + i, n);
    }
    T.dev += narr - nleft;
    T.host += nleft;
    return hipSuccess;
}

}  // namespace

namespace n1k_eng {

// The handle's value tables.  The match table's rules (ensure_match_table): a grown dictionary EXTENDS them — the entries
// of the old codes stay as they are, only the new codes are evaluated, on the host below kArrFnDeviceThreshold of them and
// by the kernel from there on.  Called by materialize_derived before the first lookup of a batch.
n1k_status ensure_value_table(n1k_handle* h) {
    ArrFnTable& T = h->arrfn;
    if (T.terms.empty()) return N1K_OK;
    const size_t n = h->dict.size(), first = T.built_for, nq = T.terms.size();
    if (n <= first) return N1K_OK;
    if (n > T.d_tags[0].n) {
        // the tables move: launches in flight may still read the old allocations
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        const size_t cap = std::max(n, T.d_tags[0].n * 2);
        for (size_t q = 0; q < nq; q++) {
            DevBuf<uint8_t> nt;
            DevBuf<uint64_t> np;
            HIP_TRY(h, nt.ensure(cap));
            HIP_TRY(h, np.ensure(cap));
            if (first) {
                HIP_TRY(h, hipMemcpy(nt.p, T.d_tags[q].p, first, hipMemcpyDeviceToDevice));
                HIP_TRY(h, hipMemcpy(np.p, T.d_payload[q].p, first * 8, hipMemcpyDeviceToDevice));
            }
            T.d_tags[q] = std::move(nt);
            T.d_payload[q] = std::move(np);
        }
    }
    const size_t cnt = n - first;
    std::vector<uint64_t> off(cnt + 1);
    off[0] = 0;
    for (size_t i = 0; i < cnt; i++) off[i + 1] = off[i] + h->dict[first + i].size();
    std::vector<uint8_t> bytes(off[cnt] + 1), tags(nq * cnt);
    std::vector<uint64_t> payload(nq * cnt);
    for (size_t i = 0; i < cnt; i++) memcpy(bytes.data() + off[i], h->dict[first + i].data(), h->dict[first + i].size());
    HIP_TRY(h, arrfn_block(T, cnt >= kArrFnDeviceThreshold, cnt, off.data(), bytes.data(), h->stream, tags.data(), payload.data()));
    // (entries no launch has been told about yet: a lookup's extent grows below)
    for (size_t q = 0; q < nq; q++) {
        HIP_TRY(h, hipMemcpy(T.d_tags[q].p + first, tags.data() + q * cnt, cnt, hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemcpy(T.d_payload[q].p + first, payload.data() + q * cnt, cnt * 8, hipMemcpyHostToDevice));
    }
    T.built_for = n;
    return N1K_OK;
}

}  // namespace n1k_eng

// ---- the diagnostic entry points: the evaluator on its own, over one term

// one whole term as the stringer writes it -> program; N1K_UNSUPPORTED for what n1k_create refuses in a plan, N1K_INVALID
// for text that is no such term
static n1k_status arrfn_parse(const char* text, size_t len, ArrFnTable& T) {
    PlanError err;
    const std::string src(text ? text : "", len);
    auto e = parse_expression(src, err);
    if (!e) return err.unsupported ? N1K_UNSUPPORTED : N1K_INVALID;
    if (e->kind != EK::Func || !arrfn_name(e->fname)) return N1K_INVALID;
    if (T.add(e.get(), err) < 0) return err.unsupported ? N1K_UNSUPPORTED : N1K_INVALID;
    return N1K_OK;
}

static n1k_status arrfn_alone(bool on_device, int device, const char* text, size_t text_len, uint64_t n, const uint64_t* offsets, const char* bytes,
                              uint8_t* out_tags, uint64_t* out_payload, uint64_t* out_left_to_host) {
    return guarded(nullptr, [&]() -> n1k_status {
    if ((text_len && !text) || (n && (!offsets || !out_tags || !out_payload)) || (on_device && n >= 0xFFFFFFF0ull)) return N1K_INVALID;
    for (uint64_t i = 0; i < n; i++)
        if (offsets[i + 1] < offsets[i] || offsets[i + 1] - offsets[i] > 0x7FFFFFFFull) return N1K_INVALID;
    if (n && offsets[n] > offsets[0] && !bytes) return N1K_INVALID;
    ArrFnTable T;
    const n1k_status st = arrfn_parse(text, text_len, T);
    if (st != N1K_OK) return st;
    if (out_left_to_host) *out_left_to_host = 0;
    if (n == 0) return N1K_OK;
    if (on_device) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev || hipSetDevice(device) != hipSuccess) return N1K_DEVICE_ERROR;
    }
    if (arrfn_block(T, on_device, n, offsets, (const uint8_t*)bytes, nullptr, out_tags, out_payload) != hipSuccess) return N1K_DEVICE_ERROR;
    if (out_left_to_host) *out_left_to_host = T.host;
    return N1K_OK;
    });
}

extern "C" {

n1k_status n1k_arrfn_eval(const char* term_text, size_t len, uint64_t n, const uint64_t* offsets, const char* bytes, uint8_t* out_tags,
                          uint64_t* out_payload) {
    return arrfn_alone(false, 0, term_text, len, n, offsets, bytes, out_tags, out_payload, nullptr);
}

n1k_status n1k_arrfn_eval_device(int device, const char* term_text, size_t len, uint64_t n, const uint64_t* offsets, const char* bytes,
                                 uint8_t* out_tags, uint64_t* out_payload, uint64_t* out_left_to_host) {
    return arrfn_alone(true, device, term_text, len, n, offsets, bytes, out_tags, out_payload, out_left_to_host);
}

n1k_status n1k_arrfn_stats(const n1k_handle* h, uint64_t out[4]) {
    return guarded(h, [&]() -> n1k_status {
    if (!h || !out) return N1K_INVALID;
    out[0] = h->arrfn.dev;
    out[1] = h->arrfn.host;
    out[2] = h->arrfn.terms.size();
    out[3] = kArrFnDeviceThreshold;
    return N1K_OK;
    });
}

}  // extern "C"
