// n1k_order.cpp — ORDER BY / OFFSET / LIMIT over the rows a Filter-only plan selects (execution/order.go:121-169, offset.go,
// limit.go; the select route ≙ order_limit.go's heap): the host driver of n1k_order.hip.  The ascending 32-bit selection of
// n1k_filter_device_batch goes in; the same kind of selection — ordered, cut — comes out, still in device memory.
//
// Keys first (one kernel: every term's key and residual per survivor, and the histograms of all their digits), one small wait
// for the histograms, then LSD radix passes from the last term to the first — only those whose digit has more than one
// non-empty bin.  The permutation starts as the identity over the ascending selection, every pass is stable: rows that tie on
// every term stay in ascending ordinal.
#include "n1k_engine.h"

using namespace n1k;
using namespace n1k_eng;

static_assert(kOrdMaxTerms == kOrderMaxTerms, "n1k_order.h and n1k_plan.h agree on the number of sort terms");

namespace {

constexpr size_t kHistWords = (size_t)kOrdHists * kOrdDigits * 256;
constexpr size_t PIN_ERR = kHistWords, PIN_NCAND = kHistWords + 2;  // (an 8-byte aligned word pair for the candidate count)
constexpr size_t kPinWords = kHistWords + 4;

uint32_t order_grid(const n1k_handle* h) { return (uint32_t)h->num_cus * (h->opt.grid_blocks ? h->opt.grid_blocks : 4u); }

n1k_status unsupported_value(n1k_handle* h) {
    // (the flags go back to zero: the handle is as after n1k_reset whatever this call answers)
    HIP_TRY(h, hipMemsetAsync(h->groups.errp, 0, sizeof(uint32_t), h->stream));
    return fail(h, N1K_UNSUPPORTED_DATA, "a value outside the device subset was met (an array or object as a sort value)");
}

void key_args(n1k_handle* h, const uint32_t* sel, OrderKeyArgs& A) {
    const ParsedPlan& pl = h->plan;
    RowOrder& O = h->order;
    A = OrderKeyArgs{};
    A.rows = sel;
    A.nterms = (uint32_t)pl.row_order.size();
    for (uint32_t t = 0; t < A.nterms; t++) {
        A.cols[t] = h->prog.cols[pl.row_order[t].col];
        A.desc[t] = pl.row_order[t].desc ? 1u : 0u;
        A.key[t] = O.key[t].p;
        A.res[t] = O.res[t].p;
    }
    A.key[A.nterms] = O.key[A.nterms].p;
    A.str_rank = h->d_rank.p;
    A.err_flags = h->groups.errp;
}

// The passes over `n` keyed elements whose histograms lie in pin_hist (and on the device in hist): terms last to first (the
// selection position, when it is a term, is the last), a term's residual digits before its key digits.  *perm_out: the
// permutation (element i of the order is element perm[i] of the keyed ones), null when no pass had anything to move.
n1k_status sort_passes(n1k_handle* h, uint64_t n, uint32_t nterms, bool pos_term, const uint32_t** perm_out) {
    RowOrder& O = h->order;
    const uint32_t* H = O.pin_hist.p;
    auto live = [&](uint32_t t, uint32_t d) {
        const uint32_t* b = H + ((size_t)t * kOrdDigits + d) * 256;
        uint32_t nz = 0;
        for (uint32_t i = 0; i < 256; i++) nz += b[i] != 0;
        return nz > 1;
    };
    *perm_out = nullptr;
    bool any = false;
    for (uint32_t t = 0; t < nterms + (pos_term ? 1u : 0u); t++)
        for (uint32_t d = 0; d < kOrdDigits; d++) any = any || live(t, d);
    if (!any) return N1K_OK;
    for (int i = 0; i < 2; i++) {
        HIP_TRY(h, O.kbuf[i].ensure(n));
        HIP_TRY(h, O.vbuf[i].ensure(n));
    }
    HIP_TRY(h, O.tile_hist.ensure(256 * ((n + kOrdTile - 1) / kOrdTile)));
    const uint32_t grid = order_grid(h);
    const uint32_t* perm = nullptr;
    int vcur = 1;  // (the first pass writes vbuf[0])
    for (int t = (int)(nterms + (pos_term ? 1u : 0u)) - 1; t >= 0; t--) {
        for (int residual = 1; residual >= 0; residual--) {
            if (residual && t == (int)nterms) continue;  // (the position has none)
            std::vector<uint32_t> digits;
            for (uint32_t d = residual ? kOrdKeyDigits : 0u; d < (residual ? kOrdDigits : kOrdKeyDigits); d++)
                if (live((uint32_t)t, d)) digits.push_back(d);
            if (digits.empty()) continue;
            // the term's keys in the order reached so far: as they lie while that is still the identity, else one gather
            const uint64_t* kin = O.key[t].p;
            int kcur = 1;
            if (residual || perm) {
                HIP_TRY(h, launch_order_gather(residual ? nullptr : O.key[t].p, residual ? O.res[t].p : nullptr, perm, n, O.kbuf[0].p, h->stream));
                kin = O.kbuf[0].p;
                kcur = 0;
            }
            for (size_t li = 0; li < digits.size(); li++) {
                const uint32_t d = digits[li], shift = 8u * (residual ? d - kOrdKeyDigits : d);
                const int ko = kcur ^ 1, vo = vcur ^ 1;
                const bool last = li + 1 == digits.size();  // (the next term gathers its own keys)
                HIP_TRY(h, launch_order_pass(kin, perm, last ? nullptr : O.kbuf[ko].p, O.vbuf[vo].p, n, shift, O.hist.p + ((size_t)t * kOrdDigits + d) * 256,
                                             O.tile_hist.p, grid, h->stream));
                kin = O.kbuf[ko].p;
                kcur = ko;
                perm = O.vbuf[vo].p;
                vcur = vo;
                O.passes++;
            }
        }
    }
    *perm_out = perm;
    return N1K_OK;
}

n1k_status order_rows(n1k_handle* h, const uint32_t* sel, uint64_t total, uint64_t first, uint64_t last, const uint32_t** out_rows) {
    const ParsedPlan& pl = h->plan;
    RowOrder& O = h->order;
    const uint32_t nterms = (uint32_t)pl.row_order.size();
    const uint64_t keep = pl.limit >= 0 ? (uint64_t)pl.offset + (uint64_t)pl.limit : total;
    // ≙ order_limit.go: fewer rows wanted than selected, and enough of them for the select to pay (the grouped tail's option)
    const bool select = pl.limit >= 0 && keep > 0 && keep < total && total >= h->opt.topk_min_groups;
    HIP_TRY(h, O.hist.ensure(kHistWords));
    HIP_TRY(h, O.pin_hist.ensure(kPinWords));
    for (uint32_t t = 0; t < nterms; t++) {
        if (select && t > 0) break;  // (the candidates' keys come later, and are fewer)
        HIP_TRY(h, O.key[t].ensure(total));
        HIP_TRY(h, O.res[t].ensure(total));
    }
    uint32_t* pin = O.pin_hist.p;
    OrderKeyArgs A;
    const uint32_t* perm = nullptr;
    const uint32_t* cand = nullptr;
    if (!select) {
        key_args(h, sel, A);
        A.n = total;
        A.store = (1u << nterms) - 1u;
        A.hist = O.hist.p;
        HIP_TRY(h, hipMemsetAsync(O.hist.p, 0, kHistWords * sizeof(uint32_t), h->stream));
        HIP_TRY(h, launch_order_keys(A, order_grid(h), h->stream));
        HIP_TRY(h, hipMemcpyAsync(pin, O.hist.p, kHistWords * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipMemcpyAsync(pin + PIN_ERR, h->groups.errp, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        if (pin[PIN_ERR] & ERR_UNSUPPORTED_VALUE) return unsupported_value(h);
        ST_TRY(sort_passes(h, total, nterms, false, &perm));
    } else {
        // the first term's keys of every survivor (all terms are evaluated: an array is refused whichever route runs), the
        // threshold = the keep-th smallest of them, the candidates at or below it, and the full sort of those alone — with
        // the candidate's selection position as the least significant term, since the select leaves them in no order
        HIP_TRY(h, O.cand.ensure(topk_cand_entries(total)));
        HIP_TRY(h, O.state.ensure(topk_state_bytes()));
        key_args(h, sel, A);
        A.n = total;
        A.store = 1u;
        HIP_TRY(h, launch_order_keys(A, order_grid(h), h->stream));
        const bool sampled = h->opt.topk_sample && topk_can_sample(total, keep);
        unsigned long long ncand = 0;
        for (int attempt = sampled ? 0 : 1; attempt < 2; attempt++) {
            HIP_TRY(h, launch_topk_select_images(O.key[0].p, total, keep, O.state.p, O.cand.p, h->stream, attempt == 0));
            HIP_TRY(h, hipMemcpyAsync(pin + PIN_NCAND, O.state.p + topk_ncand_offset(), sizeof ncand, hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(h, hipMemcpyAsync(pin + PIN_ERR, h->groups.errp, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(h, hipStreamSynchronize(h->stream));
            if (pin[PIN_ERR] & ERR_UNSUPPORTED_VALUE) return unsupported_value(h);
            memcpy(&ncand, pin + PIN_NCAND, sizeof ncand);
            if (ncand >= keep) break;
        }
        if (ncand < keep || ncand > total) return fail(h, N1K_DEVICE_ERROR, "the select left %llu candidates of %llu rows for the first %llu", ncand, (unsigned long long)total, (unsigned long long)keep);
        h->timing.stats.topk_candidates = ncand;
        for (uint32_t t = 1; t <= nterms; t++) {
            HIP_TRY(h, O.key[t].ensure(ncand));
            if (t < nterms) HIP_TRY(h, O.res[t].ensure(ncand));
        }
        key_args(h, sel, A);
        cand = A.cand = O.cand.p;
        A.n = ncand;
        A.store = (1u << nterms) - 1u;
        A.pos_term = 1;
        A.hist = O.hist.p;
        HIP_TRY(h, hipMemsetAsync(O.hist.p, 0, kHistWords * sizeof(uint32_t), h->stream));
        HIP_TRY(h, launch_order_keys(A, order_grid(h), h->stream));
        HIP_TRY(h, hipMemcpyAsync(pin, O.hist.p, kHistWords * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        ST_TRY(sort_passes(h, ncand, nterms, true, &perm));
    }
    if (last <= first) {
        *out_rows = nullptr;
        return N1K_OK;
    }
    if (!perm && !cand && first % 4 == 0) {  // nothing moved: the ascending selection is the order
        *out_rows = sel + first;
        return N1K_OK;
    }
    HIP_TRY(h, O.rows_out.ensure(last - first));
    HIP_TRY(h, launch_order_finish(sel, cand, perm, first, last, O.rows_out.p, h->stream));
    *out_rows = O.rows_out.p;
    return N1K_OK;
}

}  // namespace

namespace n1k_eng {

n1k_status order_selection(n1k_handle* h, const uint32_t* sel, uint64_t total, const uint32_t** out_rows, uint64_t* out_count) {
    const ParsedPlan& pl = h->plan;
    h->order.passes = 0;
    h->timing.stats.topk_candidates = 0;
    const uint64_t first = std::min<uint64_t>(total, (uint64_t)pl.offset);
    const uint64_t last = pl.limit >= 0 ? std::min<uint64_t>(total, first + (uint64_t)pl.limit) : total;
    *out_count = last - first;
    *out_rows = nullptr;
    if (!total) return N1K_OK;
    if (pl.row_order.empty()) {
        // Offset / Limit alone cut the ascending selection: pointer arithmetic — unless the offset would leave the ordinals off
        // the 16-byte alignment that n1k_gather_selected loads them with; those few are copied
        if (last > first && first % 4 == 0) *out_rows = sel + first;
        else if (last > first) {
            HIP_TRY(h, h->order.rows_out.ensure(last - first));
            HIP_TRY(h, launch_order_finish(sel, nullptr, nullptr, first, last, h->order.rows_out.p, h->stream));
            HIP_TRY(h, hipStreamSynchronize(h->stream));
            *out_rows = h->order.rows_out.p;
        }
        return N1K_OK;
    }
    hipEvent_t e0 = get_event(h), e1 = get_event(h);
    if (e0) (void)hipEventRecord(e0, h->stream);
    const n1k_status st = order_rows(h, sel, total, first, last, out_rows);
    h->timing.stats.order_passes = h->order.passes;
    if (e1) (void)hipEventRecord(e1, h->stream);
    h->timing.events.emplace_back(e0, e1);
    if (h->timing.q0_recorded && h->timing.ev_q1 && hipEventRecord(h->timing.ev_q1, h->stream) == hipSuccess) h->timing.q1_recorded = true;
    if (st != N1K_OK) return st;
    HIP_TRY(h, hipStreamSynchronize(h->stream));  // the selection is complete when the call returns, as it is without Order
    drain_events(h);
    return N1K_OK;
}

n1k_status refuse_ordered_rows(n1k_handle* h, const char* call) {
    if (h->plan.has_row_distinct) return fail(h, N1K_UNSUPPORTED, "%s: a plan with Distinct over its rows takes one batch through n1k_filter_device_batch", call);
    if (!h->plan.ordered_rows()) return N1K_OK;
    return fail(h, N1K_UNSUPPORTED, "%s: a Filter-only plan with Order / Offset / Limit takes one batch through n1k_filter_device_batch", call);
}

}  // namespace n1k_eng

extern "C" {

// The order key of one value on the host (the function the key kernel compiles): tests of the key need no device.
n1k_status n1k_order_key(uint32_t tag, uint64_t payload, uint32_t rank, int desc, uint64_t* key, uint32_t* residual) {
    if (!key || !residual || tag > N1K_T_OBJECT) return N1K_INVALID;
    const OrderKey k = order_key(tag, payload, rank, desc != 0);
    *key = k.key;
    *residual = k.res;
    return k.unsupported ? N1K_UNSUPPORTED_DATA : N1K_OK;
}

}  // extern "C"
