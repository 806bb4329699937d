// n1k_datefn.h — the date functions (expression/func_date.go) this path evaluates, DESIGN.md §4 "Date functions".
//
// Over a millis NUMBER, one value per row: date_part_millis, date_trunc_millis, date_add_millis — date_apply<OP>
// (n1k_device.h), datefn_kernel<OP> (n1k_datefn.hip), fusable into the run-time-built scan.
//
// Over ONE dictionary string, a leaf path of the row: str_to_millis(s) and date_part_str(s, part).  The result is a
// function of the string's dictionary code, so it is computed once per distinct string into the term's VALUE TABLE — one
// tag byte and one 8-byte payload per code, the array functions' layout (n1k_arrfn.h) with STRING as the expected tag —
// and a row reads its entry (datestr_lookup_kernel).
//
// The date text is classed once, the same way on host and device (datestr_parse):
//   VALUE   the whole string is   DATE | [DATE ('T' | ' ')] TIME [FRACTION] [ZONE]   — the union of the 13 _DATE_FORMATS
//           (func_date.go:2410-2424): Go accepts a fraction behind the seconds whether or not the layout shows one.
//           DATE yyyy-mm-dd, 4 digits, month 01-12, day 01 .. the month's length (Feb 29 in leap years only); TIME hh:mm:ss,
//           2 digits each, 00-23 / 00-59 / 00-59; FRACTION '.' and 1 to 9 digits; ZONE 'Z' or +-hh:mm with hh 00-23, mm 00-59.
//           A time-only string is year 0, January 1.  A string without a zone is UTC (time.Local is UTC here).
//   UNSURE  the same shape with one or more of: a 1-digit hour, day 00, zone hh 24-99 or mm 60-99, a fraction of more than
//           9 digits, ',' in place of the fraction's '.'.  Go's answer depends on the toolchain's version: the entry carries
//           the mark DS_UNSURE in its tag byte and a row that reads it raises ERR_UNSUPPORTED_VALUE.
//   NULL    everything else: Go's parser certainly rejects it.
// The longest VALUE string has 35 bytes; an entry of more than kDateStrDevMaxLen bytes goes to the host evaluator, which
// runs the same template.
#pragma once
#include "n1k_types.h"

namespace n1k {

enum : uint8_t { DS_TO_MILLIS = 0, DS_PART };
constexpr uint32_t kDateStrMaxTerms = 4;       // distinct str_to_millis / date_part_str terms of one plan
constexpr uint32_t kDateStrDevMaxLen = 64;     // bytes of an entry the table kernel takes
constexpr uint8_t DS_UNSURE = 0xFE;            // a table entry's tag byte: the row that reads it raises (no N1K_T_* tag)
// New dictionary entries from which the device route is taken.  Measured ("Date functions: measured",
// tools/exp_datefn.py route; strings of 24 B, two terms): the host route costs 0.081 ms for 1 Ki new strings, 0.286 for 4 Ki, 4.43
// for 64 Ki; the device route 0.178 ms, 0.225 and 1.07 — a fixed 0.18 ms, which the host route reaches near 3 Ki strings.  The
// array functions' 8192 is more than 2 x off that, so the feature has its own constant.
constexpr uint32_t kDateStrDeviceThreshold = 4096;

struct DateStrProg {
    uint8_t fn;    // DS_*
    uint8_t part;  // DS_PART: DP_* (n1k_device.h)
    uint8_t pad[6];
};

struct DateStrKernelArgs {
    const uint8_t* bytes;     // the block's bytes (+ 4 spare: whole words are staged)
    const uint64_t* offsets;  // n + 1
    uint32_t n, nprog;
    DateStrProg progs[kDateStrMaxTerms];
    uint8_t* out_tags;        // term q: out_tags[q * stride + i], out_payload[q * stride + i]
    uint64_t* out_payload;
    uint64_t stride;
    uint8_t* out_left;        // [n]: 1 = the entry is longer than kDateStrDevMaxLen: the host evaluator's
};

// One lookup per row: the operand column's (tag, payload) -> the term's value.
struct DateStrLookupArgs {
    DevCol col;               // the operand: an input column, DICT32 codes or TAGGED64
    const uint8_t* tab_tags;  // the term's value table, tab_n entries
    const uint64_t* tab_payload;
    uint32_t tab_n, pad;
    uint64_t nrows;
    // which of the nrows rows the batch really holds (CondArgs, n1k_cond.h)
    const unsigned long long* nrows_dev;
    const unsigned long long* seg_counts;
    uint64_t seg_rows;
    uint32_t nseg, pad2;
    uint8_t* out_tags;
    uint64_t* out_payload;
    uint32_t* err_flags;
};

#if defined(N1K_DATEFN_EVAL)
// (the evaluator itself: only the unit that holds both of its flavours, n1k_datefn.hip, compiles it — it needs n1k_device.h)

enum : uint32_t { DSC_NULL = 0, DSC_VALUE, DSC_UNSURE };

struct DateFields {
    int32_t year, month, day, hour, minute, second, ns, zone;  // zone: seconds east of UTC
};

N1K_HDEV bool datestr_digit(const uint8_t* s, uint32_t n, uint32_t p) { return p < n && s[p] >= '0' && s[p] <= '9'; }
// exactly two digits at p -> their value, or -1
N1K_HDEV int32_t datestr_two(const uint8_t* s, uint32_t n, uint32_t p) {
    return datestr_digit(s, n, p) && datestr_digit(s, n, p + 1) ? (s[p] - '0') * 10 + (s[p + 1] - '0') : -1;
}

// The class of s[0, n) and, for VALUE, its fields.
N1K_HDEV uint32_t datestr_parse(const uint8_t* s, uint32_t n, DateFields& f) {
    f = DateFields{0, 1, 1, 0, 0, 0, 0, 0};
    bool unsure = false;
    uint32_t p = 0;
    // DATE: the fifth byte tells it from a TIME (hh:mm:ss has ':' at 1 or 2)
    const bool has_date = n >= 5 && s[4] == '-';
    if (has_date) {
        if (n < 10 || s[7] != '-') return DSC_NULL;
        const int32_t y0 = datestr_two(s, n, 0), y1 = datestr_two(s, n, 2), mo = datestr_two(s, n, 5), d = datestr_two(s, n, 8);
        if (y0 < 0 || y1 < 0 || mo < 1 || mo > 12 || d < 0) return DSC_NULL;
        const int32_t y = y0 * 100 + y1;
        const bool leap = y % 4 == 0 && (y % 100 != 0 || y % 400 == 0);
        const int32_t mlen = mo == 2 ? (leap ? 29 : 28) : (mo == 4 || mo == 6 || mo == 9 || mo == 11 ? 30 : 31);
        if (d > mlen) return DSC_NULL;
        if (d == 0) unsure = true;
        f.year = y;
        f.month = mo;
        f.day = d;
        p = 10;
        if (p == n) return unsure ? DSC_UNSURE : DSC_VALUE;
        if (s[p] != 'T' && s[p] != ' ') return DSC_NULL;
        p++;
    }
    // TIME
    int32_t h = datestr_two(s, n, p);
    if (h >= 0) p += 2;
    else if (datestr_digit(s, n, p)) {  // a 1-digit hour
        h = s[p] - '0';
        p += 1;
        unsure = true;
    } else return DSC_NULL;
    if (h > 23 || p >= n || s[p] != ':') return DSC_NULL;
    const int32_t mi = datestr_two(s, n, p + 1);
    if (mi < 0 || mi > 59 || p + 3 >= n || s[p + 3] != ':') return DSC_NULL;
    const int32_t sc = datestr_two(s, n, p + 4);
    if (sc < 0 || sc > 59) return DSC_NULL;
    p += 6;
    f.hour = h;
    f.minute = mi;
    f.second = sc;
    // FRACTION
    if (p < n && (s[p] == '.' || s[p] == ',')) {
        if (s[p] == ',') unsure = true;
        p++;
        uint32_t digits = 0;
        int32_t ns = 0;
        while (datestr_digit(s, n, p)) {
            if (digits < 9) ns = ns * 10 + (s[p] - '0');
            digits++;
            p++;
        }
        if (digits == 0) return DSC_NULL;
        if (digits > 9) unsure = true;
        for (uint32_t k = digits; k < 9; k++) ns *= 10;
        f.ns = ns;
    }
    // ZONE
    if (p < n) {
        if (s[p] == 'Z') p++;
        else if (s[p] == '+' || s[p] == '-') {
            const int32_t zh = datestr_two(s, n, p + 1), zm = datestr_two(s, n, p + 4);
            if (zh < 0 || zm < 0 || s[p + 3] != ':') return DSC_NULL;  // (datestr_two(p + 4) >= 0: p + 3 < n)
            if (zh > 23 || zm > 59) unsure = true;
            f.zone = (zh * 3600 + zm * 60) * (s[p] == '-' ? -1 : 1);
            p += 6;
        } else return DSC_NULL;
    }
    if (p != n) return DSC_NULL;
    return unsure ? DSC_UNSURE : DSC_VALUE;
}

// str_to_millis / date_part_str over the STRING s[0, n) -> a table entry (tag byte, payload): StrToMillis.Apply
// (func_date.go:1888-1902) and DatePartStr.Apply (:828-848) behind their argument tests, which the lookup makes.
N1K_HDEV void datestr_eval(const DateStrProg& g, const uint8_t* s, uint32_t n, uint32_t& tag, uint64_t& payload) {
    DateFields f;
    const uint32_t cls = datestr_parse(s, n, f);
    tag = cls == DSC_UNSURE ? (uint32_t)DS_UNSURE : (uint32_t)T_NULL;
    payload = 0;
    if (cls != DSC_VALUE) return;
    const int64_t wall = days_from_civil(f.year, f.month, f.day) * 86400 + f.hour * 3600 + f.minute * 60 + f.second;
    if (g.fn == DS_PART) {
        tag = T_INT;
        payload = (uint64_t)date_part(wall, f.ns, f.zone, g.part);
    } else {
        const Num r = num_new_value(date_time_to_millis(DateTime{wall - f.zone, f.ns}));
        tag = r.tag;
        payload = r.p;
    }
}
#endif

}  // namespace n1k

#if !defined(__HIPCC_RTC__)
#include <string>
#include <vector>

namespace n1k {

struct Expr;
struct PlanError;

struct DateStrTerm {
    std::string text;  // the whole term as the stringer wrote it
    DateStrProg prog;
};

// date_part_millis / date_trunc_millis / date_add_millis -> AR_DATE_*, anything else AR_OP_COUNT
uint32_t datefn_op(const std::string& f);
// str_to_millis / date_part_str?
bool datestr_name(const std::string& f);
// The part of a date call (EK::Func over one of the five names), checked as n1k_create checks it: part_out is DP_*, or
// DP_COUNT for a part that is the constant MISSING (the call is then MISSING).  false + err (unsupported, the part named).
bool datefn_part(const Expr* e, uint32_t& part_out, PlanError& err);
// A str_to_millis / date_part_str term over a leaf path -> program; false + err.  missing_out: the part is the constant MISSING.
bool datestr_compile(const Expr* e, DateStrProg& out, bool& missing_out, PlanError& err);
// date_apply<op> on the host (n1k_datefn.hip holds both flavours): true when a row holding these operands raises
bool datefn_eval_host(uint32_t op, const uint32_t (&tg)[4], const uint64_t (&pv)[4], uint32_t& rt, uint64_t& rp);
// tags[q * stride + i], payload[q * stride + i] = term q over entry i taken as a STRING
void datestr_eval_block_host(const DateStrProg* progs, uint32_t nprog, uint64_t n, const uint64_t* offsets, const uint8_t* bytes, uint8_t* tags,
                             uint64_t* payload, uint64_t stride);
hipError_t launch_datestr_table(const DateStrKernelArgs& A, hipStream_t st);
hipError_t launch_datestr_lookup(const DateStrLookupArgs& A, hipStream_t st);

}  // namespace n1k
#endif
