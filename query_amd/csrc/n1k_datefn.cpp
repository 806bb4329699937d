// n1k_datefn.cpp — the date functions on the host side ("Date functions"): the names and the part of a call as
// n1k_create checks them (datefn_op, datestr_name, datefn_part), a string term's program (datestr_compile), the plan's
// distinct string terms (DateStrTable::add), ONE driver that takes a block of dictionary entries through the host evaluator
// or through datestr_table_kernel (datestr_block), the handle's value tables around it (ensure_datestr_table) and the
// diagnostic entry points of the C ABI.  The evaluators themselves, both flavours: n1k_device.h, n1k_datefn.h, n1k_datefn.hip.
#include "n1k_engine.h"

using namespace n1k;
using namespace n1k_eng;

namespace n1k {

uint32_t datefn_op(const std::string& f) {
    return f == "date_part_millis" ? AR_DATE_PART : f == "date_trunc_millis" ? AR_DATE_TRUNC : f == "date_add_millis" ? AR_DATE_ADD : AR_OP_COUNT;
}
bool datestr_name(const std::string& f) { return f == "str_to_millis" || f == "date_part_str"; }

// The part of a date call, checked at create: a STRING constant, lower-cased as datePart / dateAdd / dateTrunc do
// (func_date.go:2441, 2505, 2542), one of the names that function's switch knows — the reference fails the query on any
// other.  DATE_PART_MILLIS's third argument: the constant "UTC" and nothing else (time.LoadLocation of any other name needs
// the zone database).  A part that is the constant MISSING makes every call MISSING: part_out DP_COUNT and true.
bool datefn_part(const Expr* e, uint32_t& part_out, PlanError& err) {
    static const char* const names[DP_COUNT] = {"millennium", "century", "decade", "year", "quarter", "month", "week", "day", "hour", "minute",
                                                "second", "millisecond", "day_of_year", "day_of_week", "iso_week", "iso_year", "iso_dow",
                                                "timezone", "timezone_hour", "timezone_minute"};
    const std::string& f = e->fname;
    const uint32_t op = datefn_op(f);  // (AR_OP_COUNT: date_part_str, which takes datePart's names)
    auto refuse = [&](const std::string& what) {
        err.unsupported = true;
        err.msg = f + ": " + what;
        return false;
    };
    const Expr* pe = e->ch[op == AR_DATE_ADD ? 2 : 1].get();
    if (op == AR_DATE_PART && e->ch.size() == 3) {
        const Expr* tz = e->ch[2].get();
        if (tz->kind != EK::Const || tz->ctag != T_STRING || tz->cstr != "UTC")
            return refuse("a time zone other than the constant \"UTC\" needs the zone database and does not run on the device");
    }
    part_out = DP_COUNT;
    if (pe->kind == EK::Const && pe->ctag == T_MISSING) return true;
    if (pe->kind != EK::Const || pe->ctag != T_STRING) return refuse("the date part must be a STRING constant to run on the device");
    std::string p = pe->cstr;
    for (char& c : p)
        if (c >= 'A' && c <= 'Z') c = (char)(c - 'A' + 'a');
    if (p == "doy") p = "day_of_year";
    else if (p == "dow") p = "day_of_week";
    uint32_t id = DP_COUNT;
    for (uint32_t i = 0; i < DP_COUNT; i++)
        if (p == names[i]) id = i;
    const bool known = op == AR_DATE_ADD ? id <= DP_MILLISECOND : op == AR_DATE_TRUNC ? (id <= DP_MILLISECOND && id != DP_WEEK) : id < DP_COUNT;
    if (!known) return refuse("unsupported date part '" + pe->cstr + "' (the reference fails the query)");
    part_out = id;
    return true;
}

bool datestr_compile(const Expr* e, DateStrProg& out, bool& missing_out, PlanError& err) {
    memset(&out, 0, sizeof out);
    missing_out = false;
    if (!e || e->kind != EK::Func || !datestr_name(e->fname) || e->ch.size() != (e->fname == "str_to_millis" ? 1u : 2u)) {
        err.msg = "not a str_to_millis / date_part_str term";
        return false;
    }
    out.fn = e->fname == "str_to_millis" ? DS_TO_MILLIS : DS_PART;
    if (out.fn == DS_PART) {
        uint32_t part;
        if (!datefn_part(e, part, err)) return false;
        missing_out = part == DP_COUNT;
        out.part = (uint8_t)part;
    }
    return true;
}

}  // namespace n1k

namespace n1k_eng {

int DateStrTable::add(const Expr* e, PlanError& err) {
    for (size_t ix = 0; ix < terms.size(); ix++)
        if (terms[ix].text == e->text) return (int)ix;
    DateStrTerm t;
    t.text = e->text;
    bool missing;
    if (!datestr_compile(e, t.prog, missing, err)) return -1;
    if (missing) return -2;
    if (terms.size() >= kDateStrMaxTerms) {
        err.unsupported = true;
        err.msg = "more than " + std::to_string(kDateStrMaxTerms) + " distinct str_to_millis / date_part_str terms in one plan";
        return -1;
    }
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
// datestr_table_kernel — one upload, one launch, one synchronisation — and what it flagged `left` (entries beyond
// kDateStrDevMaxLen) through the host evaluator entry by entry; else the host evaluator over the whole block.  T's
// counters take the block's entries.
hipError_t datestr_block(DateStrTable& T, bool on_device, uint64_t n, const uint64_t* off, const uint8_t* bytes, hipStream_t st, uint8_t* tags,
                         uint64_t* payload) {
    const uint32_t nq = (uint32_t)T.terms.size();
    std::vector<DateStrProg> progs(nq);
    for (uint32_t q = 0; q < nq; q++) progs[q] = T.terms[q].prog;
    if (!on_device) {
        datestr_eval_block_host(progs.data(), nq, n, off, bytes, tags, payload, n);
        T.host += n;
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
    if (nbytes) HIP_RET(hipMemcpy(S.bytes.p, bytes, nbytes, hipMemcpyHostToDevice));
    HIP_RET(hipMemcpy(S.off.p, off, (n + 1) * 8, hipMemcpyHostToDevice));
    DateStrKernelArgs A{};
    A.bytes = S.bytes.p;
    A.offsets = S.off.p;
    A.n = (uint32_t)n;
    A.nprog = nq;
    for (uint32_t q = 0; q < nq; q++) A.progs[q] = progs[q];
    A.out_tags = S.tags.p;
    A.out_payload = S.payload.p;
    A.stride = n;
    A.out_left = S.left.p;
    HIP_RET(launch_datestr_table(A, st));
    std::vector<uint8_t> left(n);
    HIP_RET(hipMemcpyAsync(left.data(), S.left.p, n, hipMemcpyDeviceToHost, st));
    HIP_RET(hipMemcpyAsync(tags, S.tags.p, (uint64_t)nq * n, hipMemcpyDeviceToHost, st));
    HIP_RET(hipMemcpyAsync(payload, S.payload.p, (uint64_t)nq * n * 8, hipMemcpyDeviceToHost, st));
    HIP_RET(hipStreamSynchronize(st));
    uint64_t nleft = 0;
    for (uint64_t i = 0; i < n; i++) {
        if (!left[i]) continue;
        nleft++;
        datestr_eval_block_host(progs.data(), nq, 1, &off[i], bytes + (off[i] - off[0]), tags + i, payload + i, n);
    }
    T.dev += n - nleft;
    T.host += nleft;
    return hipSuccess;
}

}  // namespace

namespace n1k_eng {

// The handle's value tables.  The match table's rules (ensure_match_table, ensure_value_table): a grown dictionary EXTENDS
// them — the entries of the old codes stay as they are, only the new codes are evaluated, on the host below
// kDateStrDeviceThreshold of them and by the kernel from there on.  Called by materialize_derived before the first lookup of
// a batch.
n1k_status ensure_datestr_table(n1k_handle* h) {
    DateStrTable& T = h->datestr;
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
    HIP_TRY(h, datestr_block(T, cnt >= kDateStrDeviceThreshold, cnt, off.data(), bytes.data(), h->stream, tags.data(), payload.data()));
    // (entries no launch has been told about yet: a lookup's extent grows below)
    for (size_t q = 0; q < nq; q++) {
        HIP_TRY(h, hipMemcpy(T.d_tags[q].p + first, tags.data() + q * cnt, cnt, hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemcpy(T.d_payload[q].p + first, payload.data() + q * cnt, cnt * 8, hipMemcpyHostToDevice));
    }
    T.built_for = n;
    return N1K_OK;
}

}  // namespace n1k_eng

// ---- the diagnostic entry points: one call over n values

namespace {

struct DateCall {
    uint32_t op = AR_OP_COUNT;  // AR_DATE_*: a millis function; AR_DATESTR: a string function (T holds its program)
    uint32_t part = DP_COUNT;   // DP_COUNT: the part is the constant MISSING
    Operand n{};                // date_add_millis: its constant n
    DateStrTable T;
};

// one whole call as the stringer writes it, its first argument a leaf path, the others constants -> DateCall;
// N1K_UNSUPPORTED for what n1k_create refuses in a plan, N1K_INVALID for text that is no such call
n1k_status datefn_parse(const char* text, size_t len, DateCall& c) {
    PlanError err;
    const std::string src(text ? text : "", len);
    auto e = parse_expression(src, err);
    if (!e) return err.unsupported ? N1K_UNSUPPORTED : N1K_INVALID;
    if (e->kind != EK::Func || e->ch.empty() || e->ch[0]->kind != EK::Path) return N1K_INVALID;
    if (datestr_name(e->fname)) {
        c.op = AR_DATESTR;
        const int ix = c.T.add(e.get(), err);
        if (ix == -1) return err.unsupported ? N1K_UNSUPPORTED : N1K_INVALID;
        c.part = ix == -2 ? (uint32_t)DP_COUNT : (uint32_t)c.T.terms[0].prog.part;
        return N1K_OK;
    }
    c.op = datefn_op(e->fname);
    if (c.op == AR_OP_COUNT) return N1K_INVALID;
    if (!datefn_part(e.get(), c.part, err)) return err.unsupported ? N1K_UNSUPPORTED : N1K_INVALID;
    if (c.op == AR_DATE_ADD) {
        const Expr* ne = e->ch[1].get();
        if (ne->kind != EK::Const) return N1K_INVALID;
        c.n.is_const = 1;
        c.n.ctag = ne->ctag;
        c.n.cpayload = ne->ctag == T_INT || ne->ctag == T_FLOAT ? ne->cpayload : 0;
    }
    return N1K_OK;
}

n1k_status datefn_alone(bool on_device, int device, const char* text, size_t text_len, uint64_t n, const uint8_t* in_tags, const uint64_t* in_payload,
                        const uint64_t* offsets, const char* bytes, uint8_t* out_tags, uint64_t* out_payload, uint8_t* out_raise,
                        uint32_t* out_any_raise, uint64_t* out_left_to_host) {
    return guarded(nullptr, [&]() -> n1k_status {
    if ((text_len && !text) || (n && (!in_tags || !out_tags || !out_payload || !out_raise)) || (on_device && n >= 0xFFFFFFF0ull)) return N1K_INVALID;
    DateCall c;
    const n1k_status st = datefn_parse(text, text_len, c);
    if (st != N1K_OK) return st;
    if (out_any_raise) *out_any_raise = 0;
    if (out_left_to_host) *out_left_to_host = 0;
    if (n == 0) return N1K_OK;
    if (on_device) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev || hipSetDevice(device) != hipSuccess) return N1K_DEVICE_ERROR;
    }
    memset(out_raise, 0, n);
    if (c.part == DP_COUNT) {  // (a MISSING part: MISSING whatever the value)
        for (uint64_t i = 0; i < n; i++) {
            out_tags[i] = T_MISSING;
            out_payload[i] = 0;
        }
        return N1K_OK;
    }
    if (c.op == AR_DATESTR) {
        // the STRING values as one block of entries; every other value by the lookup's rule
        std::vector<uint64_t> idx, off(1, 0);
        std::vector<uint8_t> blk;
        for (uint64_t i = 0; i < n; i++) {
            out_tags[i] = in_tags[i] == T_MISSING ? T_MISSING : T_NULL;
            out_payload[i] = 0;
            if (in_tags[i] != T_STRING) continue;
            if (!offsets || offsets[i + 1] < offsets[i] || offsets[i + 1] - offsets[i] > 0x7FFFFFFFull || (offsets[i + 1] > offsets[i] && !bytes))
                return N1K_INVALID;
            idx.push_back(i);
            blk.insert(blk.end(), (const uint8_t*)bytes + (offsets[i] - offsets[0]), (const uint8_t*)bytes + (offsets[i + 1] - offsets[0]));
            off.push_back(blk.size());
        }
        const uint64_t m = idx.size();
        if (m == 0) return N1K_OK;
        blk.push_back(0);
        std::vector<uint8_t> tg(m);
        std::vector<uint64_t> pv(m);
        if (datestr_block(c.T, on_device, m, off.data(), blk.data(), nullptr, tg.data(), pv.data()) != hipSuccess) return N1K_DEVICE_ERROR;
        for (uint64_t k = 0; k < m; k++) {
            const bool unsure = tg[k] == DS_UNSURE;
            out_tags[idx[k]] = unsure ? (uint8_t)T_NULL : tg[k];
            out_payload[idx[k]] = unsure ? 0 : pv[k];
            out_raise[idx[k]] = unsure;
            if (unsure && out_any_raise) *out_any_raise = 1;
        }
        if (out_left_to_host) *out_left_to_host = on_device ? c.T.host : 0;
        return N1K_OK;
    }
    if (!in_payload) return N1K_INVALID;
    const uint32_t nops = c.op == AR_DATE_ADD ? 3u : 2u;
    Operand pc{};
    pc.is_const = 1;
    pc.ctag = T_INT;
    pc.cpayload = c.part;
    if (!on_device) {
        for (uint64_t i = 0; i < n; i++) {
            uint32_t tg[4] = {in_tags[i], T_MISSING, T_MISSING, T_MISSING}, rt;
            uint64_t pv[4] = {in_payload[i], 0, 0, 0}, rp;
            if (c.op == AR_DATE_ADD) {
                tg[1] = c.n.ctag;
                pv[1] = c.n.cpayload;
            }
            tg[nops - 1] = pc.ctag;
            pv[nops - 1] = pc.cpayload;
            out_raise[i] = datefn_eval_host(c.op, tg, pv, rt, rp);
            out_tags[i] = (uint8_t)rt;
            out_payload[i] = rp;
            if (out_raise[i] && out_any_raise) *out_any_raise = 1;
        }
        return N1K_OK;
    }
    // datefn_kernel<op> over one TAGGED64 column.  The kernel has one flag for all rows: out_raise stays 0, *out_any_raise says
    // whether some row raised (its slot then holds NULL).
    DevBuf<uint8_t> dt, ot;
    DevBuf<uint64_t> dp, op;
    DevBuf<uint32_t> flag;
    auto ok = [](hipError_t e) { return e == hipSuccess; };
    if (!ok(dt.ensure(n)) || !ok(ot.ensure(n)) || !ok(dp.ensure(n)) || !ok(op.ensure(n)) || !ok(flag.ensure(1))) return N1K_DEVICE_ERROR;
    if (!ok(hipMemcpy(dt.p, in_tags, n, hipMemcpyHostToDevice)) || !ok(hipMemcpy(dp.p, in_payload, n * 8, hipMemcpyHostToDevice)) ||
        !ok(hipMemset(flag.p, 0, 4)))
        return N1K_DEVICE_ERROR;
    ArithArgs A{};
    A.op = c.op;
    A.nops = nops;
    A.ops[0].is_const = 0;
    A.ops[0].col = 0;
    if (c.op == AR_DATE_ADD) A.ops[1] = c.n;
    A.ops[nops - 1] = pc;
    A.cols[0].kind = COLK_TAGGED64;
    A.cols[0].tags = dt.p;
    A.cols[0].payload = dp.p;
    A.nrows = n;
    A.out_tags = ot.p;
    A.out_payload = op.p;
    A.err_flags = flag.p;
    uint32_t raised = 0;
    if (!ok(launch_datefn(A, nullptr)) || !ok(hipDeviceSynchronize()) || !ok(hipMemcpy(out_tags, ot.p, n, hipMemcpyDeviceToHost)) ||
        !ok(hipMemcpy(out_payload, op.p, n * 8, hipMemcpyDeviceToHost)) || !ok(hipMemcpy(&raised, flag.p, 4, hipMemcpyDeviceToHost)))
        return N1K_DEVICE_ERROR;
    if (out_any_raise) *out_any_raise = (raised & ERR_UNSUPPORTED_VALUE) ? 1 : 0;
    return N1K_OK;
    });
}

}  // namespace

extern "C" {

n1k_status n1k_datefn_eval(const char* call_text, size_t len, uint64_t n, const uint8_t* in_tags, const uint64_t* in_payload,
                           const uint64_t* offsets, const char* bytes, uint8_t* out_tags, uint64_t* out_payload, uint8_t* out_raise) {
    return datefn_alone(false, 0, call_text, len, n, in_tags, in_payload, offsets, bytes, out_tags, out_payload, out_raise, nullptr, nullptr);
}

n1k_status n1k_datefn_eval_device(int device, const char* call_text, size_t len, uint64_t n, const uint8_t* in_tags, const uint64_t* in_payload,
                                  const uint64_t* offsets, const char* bytes, uint8_t* out_tags, uint64_t* out_payload, uint8_t* out_raise,
                                  uint32_t* out_any_raise, uint64_t* out_left_to_host) {
    return datefn_alone(true, device, call_text, len, n, in_tags, in_payload, offsets, bytes, out_tags, out_payload, out_raise, out_any_raise,
                        out_left_to_host);
}

n1k_status n1k_datefn_stats(const n1k_handle* h, uint64_t out[4]) {
    return guarded(h, [&]() -> n1k_status {
    if (!h || !out) return N1K_INVALID;
    out[0] = h->datestr.dev;
    out[1] = h->datestr.host;
    out[2] = h->datestr.terms.size();
    out[3] = kDateStrDeviceThreshold;
    return N1K_OK;
    });
}

}  // extern "C"
