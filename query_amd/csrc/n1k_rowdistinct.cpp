// n1k_rowdistinct.cpp — SELECT DISTINCT over the rows a Filter-only plan selects (execution/distinct.go:60-71): the host driver
// of n1k_rowdistinct.hip.  The ascending 32-bit selection of n1k_filter_device_batch goes in (or none: a plan without Filter
// selects every row); the representatives — per distinct row key the survivor with the smallest ordinal — come out, ascending,
// in a buffer of their own.  One wait: for their count and the error flags.
#include "n1k_engine.h"

using namespace n1k;
using namespace n1k_eng;

static_assert(kRdMaxTerms == kDistinctMaxTerms, "n1k_rowdistinct.h and n1k_plan.h agree on the number of result terms");

namespace n1k_eng {

bool rowdistinct_option(n1k_handle* h, const std::string& name, int64_t value) {
    if (name == "rowdistinct_slots") h->opt.rowdistinct_slots = (uint64_t)std::min<int64_t>(std::max<int64_t>(value, 0), (int64_t)kRdMaxSlots);  // (0: from the survivors)
    else if (name == "rowdistinct_lds_slots") h->opt.rowdistinct_lds_slots = (uint32_t)std::min<int64_t>(std::max<int64_t>(value, 0), kRdLdsMaxSlots);
    else return false;
    return true;
}

n1k_status distinct_selection(n1k_handle* h, const uint32_t* sel, uint64_t total, const uint32_t** out_rows, uint64_t* out_count) {
    const ParsedPlan& pl = h->plan;
    RowDistinct& R = h->rowdistinct;
    *out_rows = nullptr;
    *out_count = 0;
    R.stats[0] = total;
    R.stats[1] = R.stats[2] = R.stats[3] = 0;
    if (!total) return N1K_OK;
    // default: the next power of two that leaves the table at most half full; a forced capacity is taken as it is
    const uint64_t slots = std::min<uint64_t>(h->opt.rowdistinct_slots ? h->opt.rowdistinct_slots : next_pow2(2 * total), kRdMaxSlots);
    const uint64_t ntiles = (total + kRdTile - 1) / kRdTile;
    HIP_TRY(h, R.table.ensure(slots));
    HIP_TRY(h, R.slot_of.ensure(total));
    HIP_TRY(h, R.tile_count.ensure(ntiles + 1));
    HIP_TRY(h, R.rows_out.ensure(total));
    RowDistinctArgs A{};
    A.sel = sel;
    A.n = total;
    A.nterms = (uint32_t)pl.row_distinct.size();
    A.lds_slots = h->opt.rowdistinct_lds_slots;
    for (uint32_t t = 0; t < A.nterms; t++) A.cols[t] = h->prog.cols[pl.row_distinct[t].col];
    A.table = R.table.p;
    A.slots = slots;
    A.slot_of = R.slot_of.p;
    A.tile_count = R.tile_count.p;
    A.out = R.rows_out.p;
    A.count = h->groups.counters.p + CTR_ROWDISTINCT_COUNT;
    A.reached = h->groups.counters.p + CTR_ROWDISTINCT_REACHED;
    A.err_flags = h->groups.errp;
    hipEvent_t e0 = get_event(h), e1 = get_event(h);
    if (e0) (void)hipEventRecord(e0, h->stream);
    // no entry of an earlier call survives: the table is cleared on the stream, every call
    HIP_TRY(h, hipMemsetAsync(R.table.p, 0xFF, slots * sizeof(uint32_t), h->stream));
    HIP_TRY(h, hipMemsetAsync(h->groups.counters.p + CTR_ROWDISTINCT_COUNT, 0, 2 * sizeof(unsigned long long), h->stream));
    HIP_TRY(h, launch_row_distinct(A, (uint32_t)h->num_cus * (h->opt.grid_blocks ? h->opt.grid_blocks : 4u), h->stream));
    if (e1) (void)hipEventRecord(e1, h->stream);
    h->timing.events.emplace_back(e0, e1);
    HIP_TRY(h, hipMemcpyAsync(h->res.pin_counters.p, h->groups.counters.p, kCounters * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    if (h->timing.q0_recorded && h->timing.ev_q1 && hipEventRecord(h->timing.ev_q1, h->stream) == hipSuccess) h->timing.q1_recorded = true;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    drain_events(h);
    const uint64_t reps = h->res.pin_counters.p[CTR_ROWDISTINCT_COUNT];
    R.stats[2] = slots;
    R.stats[3] = h->res.pin_counters.p[CTR_ROWDISTINCT_REACHED];
    if ((uint32_t)h->res.pin_counters.p[CTR_ERR_FLAGS] & ERR_TABLE_FULL) {
        // (the flags go back to zero: the handle is as after n1k_reset whatever this call answers)
        HIP_TRY(h, hipMemsetAsync(h->groups.errp, 0, sizeof(uint32_t), h->stream));
        return fail(h, N1K_OOM, "the DISTINCT table of %llu slots has no room for the distinct rows of %llu survivors (option rowdistinct_slots)",
                    (unsigned long long)slots, (unsigned long long)total);
    }
    if (!reps || reps > total) return fail(h, N1K_DEVICE_ERROR, "the DISTINCT kernels left %llu representatives of %llu survivors", (unsigned long long)reps, (unsigned long long)total);
    R.stats[1] = reps;
    *out_rows = R.rows_out.p;
    *out_count = reps;
    return N1K_OK;
}

}  // namespace n1k_eng

extern "C" {

n1k_status n1k_rowdistinct_stats(const n1k_handle* h, uint64_t out[4]) {
    return guarded(h, [&]() -> n1k_status {
    if (!h || !out) return N1K_INVALID;
    for (int i = 0; i < 4; i++) out[i] = h->rowdistinct.stats[i];
    return N1K_OK;
    });
}

}  // extern "C"
