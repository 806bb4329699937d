// n1k_select.cpp — a Filter-only plan whose answer stays on the device (execution/filter.go:49-61): the selection as 32-bit
// batch-local ordinals in the handle's memory, its copy to the host, and the gather of the survivors' rows of any resident batch —
// what lets a Filter feed the next operator (a projection, n1k_push_device_batch of a group handle, an exchange) without a host
// round trip of the ordinals.
#include "n1k_engine.h"

using namespace n1k;
using namespace n1k_eng;

namespace {

// the columns of `b` as the API takes them: kinds known, arrays present where there are rows to read or write
n1k_status check_cols(n1k_handle* h, const char* what, const n1k_col* cols, uint32_t ncols, uint64_t rows) {
    for (uint32_t c = 0; c < ncols; c++) {
        const n1k_col& col = cols[c];
        if (col.kind == N1K_COL_DICT32) {
            if (rows && !col.codes) return fail(h, N1K_INVALID, "%s column %u: null codes", what, c);
        } else if (col.kind == N1K_COL_TAGGED64) {
            if (rows && (!col.tags || !col.payload)) return fail(h, N1K_INVALID, "%s column %u: null tags/payload", what, c);
        } else
            return fail(h, N1K_INVALID, "%s column %u: unknown kind %u", what, c, col.kind);
    }
    return N1K_OK;
}

}  // namespace

extern "C" {

n1k_status n1k_filter_device_batch(n1k_handle* h, const n1k_batch* batch, n1k_selection* out) {
    return guarded(h, [&]() -> n1k_status {
    if (!h) return N1K_INVALID;
    if (!batch || !out) return fail(h, N1K_INVALID, "null %s", !batch ? "batch" : "selection");
    out->nselected = 0;
    out->rows = nullptr;
    // arguments and plan first: none of this needs a device
    if (h->plan.has_group) return fail(h, N1K_INVALID, "n1k_filter_device_batch runs Filter-only plans; this plan has a group");
    if (batch->nrows >> 32) return fail(h, N1K_INVALID, "batch of %llu rows: 32-bit ordinals take fewer than 2^32", (unsigned long long)batch->nrows);
    if (batch->ncols && !batch->cols) return fail(h, N1K_INVALID, "null column array");
    n1k_status st = validate_batch(h, batch);
    if (st != N1K_OK) return st;
    if (h->stop_flag.load()) return fail(h, N1K_STOPPED, "operator was stopped");
    st = ensure_device(h);
    if (st != N1K_OK) return st;
    // reopen(): stats, counters and flags of this execution alone (a stop is not forgotten: it answers this call)
    st = reset_handle(h, false);
    if (st != N1K_OK) return st;
    h->device_clean = false;
    if (!h->layout_fixed) {
        st = fix_layout(h, batch);
        if (st != N1K_OK) return st;
    }
    st = bind_columns(h, batch);
    if (st != N1K_OK) return st;
    st = ensure_rank(h);
    if (st != N1K_OK) return st;
    st = ensure_match_table(h);
    if (st != N1K_OK) return st;
    st = ensure_pinned_counters(h);
    if (st != N1K_OK) return st;
    const uint64_t n = batch->nrows;
    unsigned long long total = 0;
    uint32_t err_flags = 0;
    if (n && !h->plan.has_filter) {
        total = n;  // a DISTINCT plan without Filter: every row is a survivor, the selection is the identity and is not written
    } else if (n) {
        const uint64_t ntiles = (n + kFilterStreamTile - 1) / kFilterStreamTile;
        HIP_TRY(h, h->filter.tile_off.ensure(ntiles + 1));
        HIP_TRY(h, h->filter.sel32.ensure(n));
        const bool fast = filter_stream_fast(h);
        const uint32_t grid = filter_stream_grid(h, ntiles, fast);
        hipEvent_t e0 = get_event(h), e1 = get_event(h);
        if (e0) (void)hipEventRecord(e0, h->stream);
        HIP_TRY(h, launch_filter_stream(h->prog, n, h->filter.sel32.p, (unsigned long long*)h->filter.tile_off.p,
                                        (unsigned long long*)h->filter.tile_off.p + ntiles, h->groups.counters.p + CTR_FILTER_TOTAL, h->groups.errp, grid,
                                        h->stream, fast));
        if (e1) (void)hipEventRecord(e1, h->stream);
        h->timing.events.emplace_back(e0, e1);
        h->timing.stats.spec_kernel = fast ? 1u : 0u;
        // the survivor count and the error flags through the pinned counter words: the call's ONE wait; no ordinal moves
        HIP_TRY(h, hipMemcpyAsync(h->res.pin_counters.p, h->groups.counters.p, kCounters * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
        if (h->timing.q0_recorded && h->timing.ev_q1 && hipEventRecord(h->timing.ev_q1, h->stream) == hipSuccess) h->timing.q1_recorded = true;
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        total = h->res.pin_counters.p[CTR_FILTER_TOTAL];
        err_flags = (uint32_t)h->res.pin_counters.p[CTR_ERR_FLAGS];
        drain_events(h);
    }
    h->timing.stats.rows_in = n;
    h->timing.stats.batches = 1;
    h->timing.stats.bytes_scanned = n * batch_bytes_per_row(h);
    if (err_flags & ERR_UNSUPPORTED_VALUE) {
        // (the flags go back to zero: the handle is as after n1k_reset whatever this call answers)
        HIP_TRY(h, hipMemsetAsync(h->groups.errp, 0, sizeof(uint32_t), h->stream));
        return fail(h, N1K_UNSUPPORTED_DATA, "a value outside the device subset was met (ordering of arrays/objects)");
    }
    if (h->stop_flag.load()) return fail(h, N1K_STOPPED, "operator was stopped");
    if (total > n) return fail(h, N1K_DEVICE_ERROR, "the Filter kernel counted %llu survivors of %llu rows", total, (unsigned long long)n);
    const uint32_t* rows = total ? h->filter.sel32.p : nullptr;
    // a plan with Distinct: per distinct row of the result terms the survivor with the smallest ordinal (n1k_rowdistinct.cpp)
    if (h->plan.has_row_distinct) {
        uint64_t reps = 0;
        ST_TRY(distinct_selection(h, h->plan.has_filter ? rows : nullptr, total, &rows, &reps));
        if (h->stop_flag.load()) return fail(h, N1K_STOPPED, "operator was stopped");
        total = reps;
    }
    // a plan with Order / Offset / Limit: the survivors in ORDER BY order, cut to [offset, offset + limit) (n1k_order.cpp)
    if (h->plan.ordered_rows()) {
        uint64_t cut = 0;
        ST_TRY(order_selection(h, rows, total, &rows, &cut));
        total = cut;
    }
    h->timing.stats.rows_selected = total;
    h->filter.has_sel32 = true;
    h->filter.sel32_count = total;
    h->filter.sel32_rows = n;
    h->filter.sel32_out = rows;
    out->nselected = total;
    out->rows = rows;
    return N1K_OK;
    });
}

n1k_status n1k_selected_to_host32(n1k_handle* h, uint32_t* out, uint64_t capacity) {
    return guarded(h, [&]() -> n1k_status {
    if (!h) return N1K_INVALID;
    if (!h->filter.has_sel32) return fail(h, N1K_INVALID, "no selection: n1k_filter_device_batch comes first");
    const uint64_t n = h->filter.sel32_count;
    if (capacity < n) return fail(h, N1K_INVALID, "room for %llu ordinals, the selection holds %llu", (unsigned long long)capacity, (unsigned long long)n);
    if (!n) return N1K_OK;
    if (!out) return fail(h, N1K_INVALID, "null output");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipMemcpyAsync(out, h->filter.sel32_out, n * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return N1K_OK;
    });
}

n1k_status n1k_gather_selected(n1k_handle* h, const n1k_batch* src, uint64_t capacity_rows, const n1k_col* out_cols) {
    return guarded(h, [&]() -> n1k_status {
    if (!h) return N1K_INVALID;
    if (!h->filter.has_sel32) return fail(h, N1K_INVALID, "no selection: n1k_filter_device_batch comes first");
    if (!src || !out_cols || !src->cols) return fail(h, N1K_INVALID, "null %s", !src ? "batch" : "column array");
    if (src->ncols < 1 || src->ncols > kGatherMaxCols) return fail(h, N1K_INVALID, "%u columns: a gather takes 1 to %u", src->ncols, kGatherMaxCols);
    const uint64_t n = h->filter.sel32_count;
    if (src->nrows != h->filter.sel32_rows)
        return fail(h, N1K_INVALID, "batch of %llu rows, the selection was taken from %llu", (unsigned long long)src->nrows, (unsigned long long)h->filter.sel32_rows);
    if (capacity_rows < n) return fail(h, N1K_INVALID, "room for %llu rows, the selection holds %llu", (unsigned long long)capacity_rows, (unsigned long long)n);
    n1k_status st = check_cols(h, "source", src->cols, src->ncols, src->nrows);
    if (st == N1K_OK) st = check_cols(h, "output", out_cols, src->ncols, n);
    if (st != N1K_OK) return st;
    GatherArgs A{};
    for (uint32_t c = 0; c < src->ncols; c++) {
        if (out_cols[c].kind != src->cols[c].kind) return fail(h, N1K_INVALID, "column %u: output kind %u, source kind %u", c, out_cols[c].kind, src->cols[c].kind);
        GatherCol& g = A.cols[c];
        g.kind = src->cols[c].kind == N1K_COL_DICT32 ? COLK_DICT32 : COLK_TAGGED64;
        g.src_tags = src->cols[c].tags;
        g.src_payload = src->cols[c].payload;
        g.src_codes = src->cols[c].codes;
        g.dst_tags = const_cast<uint8_t*>(out_cols[c].tags);  // (n1k_col serves both directions; these are the caller's output arrays)
        g.dst_payload = const_cast<uint64_t*>(out_cols[c].payload);
        g.dst_codes = const_cast<uint32_t*>(out_cols[c].codes);
    }
    if (!n) return N1K_OK;
    A.rows = h->filter.sel32_out;
    A.n = n;
    A.ncols = src->ncols;
    HIP_TRY(h, hipSetDevice(h->device));
    hipEvent_t e0 = get_event(h), e1 = get_event(h);
    if (e0) (void)hipEventRecord(e0, h->stream);
    HIP_TRY(h, launch_gather_rows(A, h->stream));  // asynchronous: n1k_sync waits (and adds the kernel's time to device_ms)
    if (e1) (void)hipEventRecord(e1, h->stream);
    h->timing.events.emplace_back(e0, e1);
    return N1K_OK;
    });
}

}  // extern "C"
