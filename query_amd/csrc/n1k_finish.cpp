// n1k_finish.cpp — afterItems: IntermediateGroup / FinalGroup over what the batches left on the device, then the grouped tail
// (execution/group_intermediate.go:56-104, group_final.go:55-118).  The stages stand in the order n1k_finish (at the end) runs them.
#include "n1k_engine.h"

using namespace n1k;
using namespace n1k_eng;

// stats.query_ms: the last device work of the query is behind this point of the stream (the wait that follows completes it)
static void mark_query_end(n1k_handle* h) {
    if (h->timing.q0_recorded && h->timing.ev_q1 && hipEventRecord(h->timing.ev_q1, h->stream) == hipSuccess) h->timing.q1_recorded = true;
}

// FinalGroup's output for N groups in one allocation: [keys][aggs][partials][rep rows] (Results::d_out and its host copies)
struct OutLayout {
    size_t aggs, parts, rep, total;
    OutLayout(uint64_t groups = 0, size_t nk = 0, size_t na = 0)
        : aggs(groups * nk * sizeof(OutValue)), parts(aggs + groups * na * sizeof(OutValue)), rep(parts + groups * na * sizeof(OutPartial)), total(rep + groups * 8) {}
    OutValue* k(char* b) const { return (OutValue*)b; }
    OutValue* a(char* b) const { return (OutValue*)(b + aggs); }
    OutPartial* p(char* b) const { return (OutPartial*)(b + parts); }
    uint64_t* r(char* b) const { return (uint64_t*)(b + rep); }
};

// What the stages hand on.
struct Finish {
    unsigned long long counters[kCounters] = {0};  // host copy of the device counters, as read_counters found them
    uint32_t err_flags = 0;
    uint64_t ng = 0;           // groups: in the table or the kept region, then those the top-k selection left
    uint64_t spec_groups = 0;  // > 0: a speculative FinalGroup wrote up to this many groups into pin_out
    char* d_rows = nullptr;    // the result rows on the device,
    char* rows = nullptr;      // ... on the host,
    OutLayout lay;             // ... and how either is laid out
    bool sets_exact = false;   // COUNT(DISTINCT): the optimistic path is not to be tried (again)
    bool sets_deferred = false, vetoed = false;  // ... it was taken and reports with the results; it reported an overflow
    std::chrono::steady_clock::time_point wait_end{};  // (host trace: the end of a speculative hit's one wait, if there was one)
};

// small reads of the sized pass, in the words behind the counters' pinned copy (Results::pin_counters)
enum : uint32_t { PIN_NCAND = kCounters, PIN_ERR_FLAGS, PIN_VETO };

// The speculative FinalGroup of a small table: for how many groups, 0 where the plan or the handle's state does not allow it.
static uint64_t speculative_groups(const n1k_handle* h) {
    const ParsedPlan& pl = h->plan;
    const bool topk_forced = pl.has_order && pl.limit >= 0 && !pl.has_having && h->opt.topk_min_groups < 4096;  // tests
    // (a table of millions of slots is not worth scanning twice: the sized pass alone then)
    if (!pl.has_group || h->has_distinct || !h->groups.table.capacity || h->groups.table.capacity > (1u << 20) || topk_forced || h->part.pending.count)
        return 0;
    return std::min<uint64_t>(h->groups.table.capacity, 4096);
}

namespace n1k_eng {
bool slabs_to_rows(const n1k_handle* h, const FastArgs& F, uint32_t g, bool only_chunk, bool whole) {
    // a one-call execution on a device that n1k_reset found clean: the table is empty and the counters are zero, before
    // the scan and — the table never touched — after the fold
    if (!h->clear_on_finish || !h->groups.pending.clean_at_push || !only_chunk || !whole || h->push_nrows_dev || h->push_nseg) return false;
    if (!F.slabs || F.hashed || g <= 1 || h->opt.merge_chunks != 0 || h->prog.wide_int || h->has_array_agg) return false;
    const uint64_t spec = speculative_groups(h), cap = h->groups.table.capacity;
    // every slot that can be a group has its row in the pinned buffer (and ERR_TABLE_FULL could not arise with the table
    // either): there is no table to run a sized second pass from
    return spec && cap <= kFinalizeSmallMax && F.lds_slots <= std::min<uint64_t>(std::min<uint64_t>(cap, spec), h->opt.max_groups);
}
}  // namespace n1k_eng

// FinalGroup's position counter starts from zero (reopen zeroes every counter in its one launch)
static n1k_status zero_out_count(n1k_handle* h) {
    if (h->res.out_count_dirty) HIP_TRY(h, hipMemsetAsync(h->groups.counters.p + CTR_OUT_COUNT, 0, sizeof(unsigned long long), h->stream));
    h->res.out_count_dirty = true;
    return N1K_OK;
}

// Stage: the counters to the host.  When the plan has no DISTINCT step the finalize kernel does not depend on anything the host
// has to read first, so it is launched for up to `spec_groups` groups together with the copy of the counters: ONE host
// synchronisation per query when the result fits (else the sized pass runs as well).
static n1k_status read_counters(n1k_handle* h, Finish& F) {
    // no batch was ever pushed: nothing ran on the device; only the empty-input row can be produced
    if (!h->device_ready) return h->timing.stats.rows_in == 0 ? ensure_device(h) : N1K_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    ST_TRY(ensure_pinned_counters(h));
    GroupTable::PendingSlabs& ps = h->groups.pending;
    const bool fold = ps.grid && slabs_to_rows(h, ps.F, ps.grid, true, true);
    if (ps.grid && !fold) {
        // (not reached: launch_chunk asked the same predicate.)  IntermediateGroup into the table after all, as the push would have
        HIP_TRY(h, launch_merge_slabs(h->prog, ps.F, h->groups.table, ps.grid, h->groups.counters.p + CTR_GROUPS, h->stream, h->opt.merge_chunks));
        ps.grid = 0;
    }
    F.spec_groups = speculative_groups(h);
    if (F.spec_groups) {
        F.lay = OutLayout(F.spec_groups, h->plan.keys.size(), h->plan.aggs.size());
        HIP_TRY(h, h->res.pin_out.ensure(F.lay.total + kCounters * sizeof(unsigned long long)));
        // The few groups of a speculative FinalGroup are written by the kernel straight into the pinned host buffer (posted
        // stores over PCIe), the counters behind them: no copy engine in the query's critical path (two hipMemcpyAsync D2H
        // cost ~ 21 us of a 0.33 ms query: 2 x 4.7 us + a 12 us gap).
        char* d = F.rows = h->res.pin_out.p;
        unsigned long long* host_counters = (unsigned long long*)(d + F.lay.total);
        if (fold) {
            // slabs -> rows in the query's one kernel behind the scan; the table stays empty, the counters come back zero
            HIP_TRY(h, launch_fold_rows(h->prog, ps.F, h->groups.table, ps.grid, F.lay.k(d), F.lay.a(d), F.lay.p(d), F.lay.r(d), h->groups.counters.p, CTR_TAIL_TICKET,
                                        host_counters, F.spec_groups, h->stream));
            ps.grid = 0;
            h->res.out_count_dirty = false;
            h->device_clean = true;
        } else if (h->groups.table.capacity <= kFinalizeSmallMax) {
            // small tables: FinalGroup, the counters behind it and — for a one-call execution, when nothing else on the
            // device needs a reset (no wide-value tables) — the state the next execution starts from, in ONE last kernel
            const bool clear = h->clear_on_finish && !h->prog.wide_int;
            HIP_TRY(h, launch_finalize_small(h->prog, h->groups.table, F.lay.k(d), F.lay.a(d), F.lay.p(d), F.lay.r(d), h->groups.counters.p,
                                             host_counters, F.spec_groups, h->groups.errp, clear, h->stream));
            h->res.out_count_dirty = !clear;
            h->device_clean = clear;
        } else {
            // larger tables: finalize_kernel, then a one-wave kernel publishes the counters
            ST_TRY(zero_out_count(h));
            HIP_TRY(h, launch_finalize(h->prog, h->groups.table, F.lay.k(d), F.lay.a(d), F.lay.p(d), F.lay.r(d),
                                       h->groups.counters.p + CTR_OUT_COUNT, F.spec_groups, h->groups.errp, h->stream));
            HIP_TRY(h, launch_publish_counters(h->groups.counters.p, host_counters, kCounters, h->stream));
        }
        mark_query_end(h);
        const auto w0 = std::chrono::steady_clock::now();
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        F.wait_end = std::chrono::steady_clock::now();
        h->timing.host_us[3] += std::chrono::duration<double, std::micro>(F.wait_end - w0).count();
        memcpy(F.counters, host_counters, sizeof F.counters);
        if (fold && F.counters[CTR_TAIL_TICKET]) {  // the scan's bypass put rows into the table: n1k_reset has to clear it
            h->device_clean = false;
            F.counters[CTR_TAIL_TICKET] = 0;
        }
    } else {
        HIP_TRY(h, hipMemcpyAsync(h->res.pin_counters.p, h->groups.counters.p, sizeof F.counters, hipMemcpyDeviceToHost, h->stream));
        mark_query_end(h);
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        memcpy(F.counters, h->res.pin_counters.p, sizeof F.counters);
    }
    F.err_flags = (uint32_t)F.counters[CTR_ERR_FLAGS];
    drain_events(h);
    return N1K_OK;
}

// Stage (K6): de-duplicate the logged (group, value) pairs of every DISTINCT aggregate (≙ Set.Len(), value/set.go:198-215)
static n1k_status build_distinct_sets(n1k_handle* h, Finish& F) {
    h->distinct.path = 0;
    if (h->distinct.wregion_used) HIP_TRY(h, hipMemsetAsync(h->groups.counters.p + CTR_OPTIMISTIC_OVERFLOW, 0, 8, h->stream));
    for (size_t a = 0; a < h->plan.aggs.size(); a++) {
        const AggSpec& ag = h->prog.aggs[a];
        if (!ag.distinct || ag.kind == AGG_ARRAY) continue;  // (ARRAY_AGG: after FinalGroup, array_agg_groups)
        const uint64_t npairs = std::min<uint64_t>(F.counters[CTR_PAIR_LOG_CURSORS + ag.log_index], h->distinct.log_capacity);
        const uint64_t nwords = h->distinct.words[ag.log_index] ? std::min<uint64_t>(F.counters[CTR_WORD_LOG_CURSORS + ag.log_index], h->distinct.log_capacity) : 0;
        DistinctArgs D{};
        D.log_key = h->distinct.log_key[ag.log_index].p;
        D.log_val = h->distinct.log_val[ag.log_index].p;
        D.log_cls = h->distinct.log_cls[ag.log_index].p;
        D.npairs = npairs;
        D.glob_off = ag.glob_off;
        D.kind = ag.kind;
        D.total_words = h->groups.counters.p + CTR_DISTINCT_REGION_WORDS;
        HIP_TRY(h, h->distinct.regions.ensure(h->groups.table.capacity * 6));
        D.regions = h->distinct.regions.p;
        HIP_TRY(h, hipMemsetAsync(D.total_words, 0, sizeof(unsigned long long), h->stream));
        HIP_TRY(h, launch_distinct_layout(h->prog, h->groups.table, D, h->stream));  // also zeroes the set sizes
        if (npairs) {
            // pairs of two words (floats, wide values, SUM/AVG DISTINCT): per-(group, class) sets in global memory
            unsigned long long words = 0;
            HIP_TRY(h, hipMemcpyAsync(&words, D.total_words, sizeof words, hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(h, hipStreamSynchronize(h->stream));
            HIP_TRY(h, h->distinct.set_table.ensure(std::max<uint64_t>(words, 1)));
            D.set_table = h->distinct.set_table.p;
            if (words) HIP_TRY(h, hipMemsetAsync(h->distinct.set_table.p, 0xFF, words * 8, h->stream));
            HIP_TRY(h, launch_distinct_insert(h->prog, h->groups.table, D, h->groups.errp, h->stream));
            h->distinct.path |= 1u;
        }
        if (h->distinct.wregion_used && h->distinct.words[ag.log_index]) ST_TRY(distinct_regions_finish(h, ag, nwords, F.sets_exact, &F.sets_deferred));
        else if (nwords) ST_TRY(distinct_words_finish(h, ag, nwords));
    }
    h->timing.stats.distinct_path = h->distinct.path;
    return N1K_OK;
}

// ORDER BY ... LIMIT: only the groups that can be among the first offset+limit rows leave the device (select_topk)
struct TopKPlan { bool on = false, lean = false; uint64_t keep = 0; };

static TopKPlan plan_topk(const n1k_handle* h, uint64_t ng) {
    const ParsedPlan& pl = h->plan;
    TopKPlan t;
    t.keep = pl.limit >= 0 ? (uint64_t)pl.offset + (uint64_t)pl.limit : ng;
    t.on = pl.has_order && pl.limit >= 0 && !pl.has_having && pl.order[0].proj_index < 0 && t.keep > 0 && t.keep < ng &&
           ng >= h->opt.topk_min_groups && ng < (1ull << 32);
    // groups kept in their compact region + a top-k filter: only the first ORDER BY term's value of every group is
    // written (16 B per group, not the whole output row), the candidates' rows are finalised after the selection
    t.lean = t.on && h->part.pending.count && h->opt.lean_topk;
    return t;
}

// Stage: FinalGroup sized for the F.ng groups the counters told of, out of the table or the kept region, into d_out.
static n1k_status sized_final_group(n1k_handle* h, Finish& F, bool lean) {
    F.lay = OutLayout(F.ng, h->plan.keys.size(), h->plan.aggs.size());
    HIP_TRY(h, h->res.d_out.ensure((lean ? F.ng * sizeof(OutValue) : F.lay.total) + 16));
    char* d = F.d_rows = h->res.d_out.p;
    ST_TRY(zero_out_count(h));
    if (lean) {
        // (the order image of the first ORDER BY term straight from FinalGroup: 8 B per group written, one kernel less)
        const OrderTerm& t0 = h->plan.order[0];
        HIP_TRY(h, h->topk.images.ensure(F.ng));
        ST_TRY(ensure_rank(h));
        HIP_TRY(h, launch_finalize_region(h->prog, h->part.emit.p, h->part.pending.cap, F.ng, nullptr, nullptr, nullptr, nullptr, h->groups.errp,
                                          h->stream, nullptr, nullptr, t0.key_index >= 0,
                                          (uint32_t)(t0.key_index >= 0 ? t0.key_index : t0.agg_index), h->topk.images.p, t0.desc));
    } else if (h->part.pending.count)
        HIP_TRY(h, launch_finalize_region(h->prog, h->part.emit.p, h->part.pending.cap, F.ng, F.lay.k(d), F.lay.a(d), F.lay.p(d), F.lay.r(d),
                                          h->groups.errp, h->stream));
    else
        HIP_TRY(h, launch_finalize(h->prog, h->groups.table, F.lay.k(d), F.lay.a(d), F.lay.p(d), F.lay.r(d), h->groups.counters.p + CTR_OUT_COUNT,
                                   F.ng, h->groups.errp, h->stream));
    return N1K_OK;
}

// Stage: the device top-k filter over the first ORDER BY term of FinalGroup's rows.  Leaves the candidates' rows compacted in
// out2 and F.ng / F.lay telling of them.
static n1k_status select_topk(n1k_handle* h, Finish& F, const TopKPlan& tk) {
    const OrderTerm& t0 = h->plan.order[0];
    const uint32_t nk = (uint32_t)h->plan.keys.size(), na = (uint32_t)h->plan.aggs.size();
    HIP_TRY(h, h->topk.images.ensure(F.ng));
    HIP_TRY(h, h->topk.cand.ensure(topk_cand_entries(F.ng)));
    HIP_TRY(h, h->topk.state.ensure(topk_state_bytes()));
    ST_TRY(ensure_rank(h));
    char* d = F.d_rows;
    const OutLayout all = F.lay;
    const bool by_key = t0.key_index >= 0;
    const OutValue* vals = tk.lean || by_key ? all.k(d) : all.a(d);
    const uint32_t stride = tk.lean ? 1u : (by_key ? nk : na), index = tk.lean ? 0u : (uint32_t)(by_key ? t0.key_index : t0.agg_index);
    // the threshold from a sample of the groups first (one small kernel instead of eight histogram passes); exact
    // whenever at least `keep` candidates come out, else the radix select over all images
    const bool sampled = h->opt.topk_sample && topk_can_sample(F.ng, tk.keep);
    unsigned long long ncand = 0;
    for (int attempt = sampled ? 0 : 1; attempt < 2; attempt++) {
        HIP_TRY(h, launch_topk_select(h->prog, vals, stride, index, F.ng, t0.desc, tk.keep, h->topk.images.p, h->topk.state.p, h->topk.cand.p,
                                      h->stream, attempt == 0, tk.lean || (attempt == 1 && sampled)));
        HIP_TRY(h, hipMemcpyAsync(h->res.pin_counters.p + PIN_NCAND, h->topk.state.p + topk_ncand_offset(), sizeof ncand, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        ncand = h->res.pin_counters.p[PIN_NCAND];
        if (ncand >= tk.keep) break;
    }
    F.lay = OutLayout(ncand, nk, na);
    HIP_TRY(h, h->topk.out2.ensure(F.lay.total + 16));
    char* c = F.d_rows = h->topk.out2.p;
    if (tk.lean)
        HIP_TRY(h, launch_finalize_region(h->prog, h->part.emit.p, h->part.pending.cap, ncand, F.lay.k(c), F.lay.a(c), F.lay.p(c), F.lay.r(c),
                                          h->groups.errp, h->stream, h->topk.cand.p));
    else
        HIP_TRY(h, launch_topk_compact(h->topk.cand.p, ncand, nk, na, all.k(d), all.a(d), all.p(d), all.r(d), F.lay.k(c), F.lay.a(c), F.lay.p(c),
                                       F.lay.r(c), h->stream));
    h->timing.stats.topk_candidates = ncand;
    F.ng = ncand;
    return N1K_OK;
}

// Stage: the rows to the host, the error flags and the veto words of an optimistic COUNT(DISTINCT) with them; the wait.
static n1k_status land_rows(n1k_handle* h, Finish& F) {
    const size_t bytes = F.lay.total;
    // results up to a few MB land in pinned memory (grown on demand); larger ones — millions of groups without a LIMIT —
    // in the pageable vector, whose copy the link's time dominates anyway
    const bool pinned_rows = bytes <= (8u << 20);
    if (pinned_rows && h->res.pin_rows.n < bytes) HIP_TRY(h, h->res.pin_rows.ensure(std::max<size_t>(bytes, 64u << 10)));
    if (!pinned_rows) h->res.out_host.resize(bytes);
    F.rows = pinned_rows ? h->res.pin_rows.p : h->res.out_host.data();
    unsigned long long* const pin = h->res.pin_counters.p;
    HIP_TRY(h, hipMemcpyAsync(F.rows, F.d_rows, bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(pin + PIN_ERR_FLAGS, h->groups.errp, 4, hipMemcpyDeviceToHost, h->stream));
    if (F.sets_deferred) HIP_TRY(h, hipMemcpyAsync(pin + PIN_VETO, h->groups.counters.p + CTR_OPTIMISTIC_OVERFLOW, 8, hipMemcpyDeviceToHost, h->stream));
    mark_query_end(h);
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    memcpy(&F.err_flags, pin + PIN_ERR_FLAGS, 4);
    F.vetoed = F.sets_deferred && pin[PIN_VETO] != 0;  // a set or a bin overflowed on the optimistic path: no counts were added
    return N1K_OK;
}

// Stage: rows -> h->res.{keys, aggs, rep, parts}
static void unpack_rows(n1k_handle* h, const Finish& F) {
    const size_t nk = h->plan.keys.size(), na = h->plan.aggs.size(), ng = F.ng;
    h->res.keys.assign((const n1k_value*)F.lay.k(F.rows), (const n1k_value*)F.lay.k(F.rows) + ng * nk);
    h->res.aggs.assign((const n1k_value*)F.lay.a(F.rows), (const n1k_value*)F.lay.a(F.rows) + ng * na);
    h->res.rep.assign(F.lay.r(F.rows), F.lay.r(F.rows) + ng);
    const OutPartial* parts = F.lay.p(F.rows);
    h->res.parts.resize(ng * na);
    for (size_t i = 0; i < ng * na; i++) {
        n1k_partial& p = h->res.parts[i];
        memset(&p, 0, sizeof p);
        p.count = parts[i].count;
        p.isum = parts[i].isum;
        p.fsum = parts[i].fsum;
        p.int_exact = parts[i].flags & 1u;
        p.has_float = (parts[i].flags >> 1) & 1u;
        p.extreme.tag = (uint8_t)parts[i].ext_tag;
        p.extreme.v.code = parts[i].ext_payload;
        p.distinct = parts[i].distinct;
    }
}

// Stage: what the error flags say.  What the verdict words of a multi-GPU exchange said comes first: every rank read the same
// verdicts, so every rank returns from here with the same status (n1k_failure_is_global) and none of them goes on to the gather.
static n1k_status flags_status(n1k_handle* h, const Finish& F) {
    if (F.err_flags & kErrFromVerdict) {
        h->failure_global = true;
        if (F.err_flags & ERR_PEER_FAILED) {
            const int ps = (int)(F.counters[CTR_PEER_STATUS] & 0xFF);
            return fail(h, ps > 0 && ps <= N1K_REGION_FULL ? (n1k_status)ps : N1K_DEVICE_ERROR,
                        "a rank failed before the exchange (its status: %d); the step is void on every rank", ps);
        }
        if (F.err_flags & ERR_EXCHANGE_WIDE)
            return fail(h, N1K_UNSUPPORTED, "a sender's group keys hold float / wide integer values: use the row exchange");
        if (F.err_flags & ERR_EXCHANGE_OVERFLOW)
            return fail(h, N1K_REGION_FULL, "a sender's region overflowed: raise the region capacity (on every rank)");
        if (F.err_flags & ERR_PEER_UNPACKABLE)
            return fail(h, N1K_UNSUPPORTED_DATA, "a sender met a group key value that does not fit the packed key (option wide_values, or a key layout too narrow)");
        return fail(h, N1K_UNSUPPORTED_DATA, "a sender met a value outside the device subset (ordering of arrays/objects)");
    }
    if (F.err_flags & ERR_TABLE_FULL)
        return fail(h, N1K_OOM, "group table capacity exceeded: raise the max_groups option (now %llu)",
                    (unsigned long long)h->opt.max_groups);
    if (F.err_flags & ERR_UNPACKABLE_KEY)
        return fail(h, N1K_UNSUPPORTED_DATA,
                    "a group key value does not fit the packed key: more than %llu distinct float / wide integer key "
                    "values (option wide_values), or a key layout too narrow for them",
                    (unsigned long long)((1ull << h->prog.wide_bits) / 2));
    if (F.err_flags & ERR_UNSUPPORTED_VALUE)
        return fail(h, N1K_UNSUPPORTED_DATA, "a value outside the device subset was met (ordering of arrays/objects)");
    return N1K_OK;
}

// Stage: what follows FinalGroup on the host, and the result
static n1k_status host_tail(n1k_handle* h, uint64_t ng, n1k_result* out) {
    const ParsedPlan& pl = h->plan;
    if (ng == 0 && pl.keys.empty()) {
        // FinalGroup.afterItems: no keys and no input -> one row of Default() values (execution/group_final.go:108-117)
        h->res.aggs.resize(pl.aggs.size());
        h->res.parts.resize(pl.aggs.size());
        h->res.rep.assign(1, ~0ull);
        for (size_t a = 0; a < pl.aggs.size(); a++) default_value(pl.aggs[a], h->res.aggs[a], h->res.parts[a]);
        ng = 1;
    }
    if (pl.has_having) ST_TRY(having_groups(h, ng));
    h->tail.r_proj.clear();
    if (pl.has_project) ST_TRY(project_groups(h, ng));
    if (pl.has_order || pl.limit >= 0 || pl.offset > 0) ST_TRY(order_groups(h, ng));
    publish_result(h, ng, true, out);
    h->timing.stats.groups_out = ng;
    return N1K_OK;
}

extern "C" {

n1k_status n1k_finish(n1k_handle* h, n1k_result* out) {
    return guarded(h, [&]() -> n1k_status {
    if (!h || !out) return N1K_INVALID;
    memset(out, 0, sizeof *out);
    h->failure_global = false;
    if (h->stop_flag.load()) return fail(h, N1K_STOPPED, "operator was stopped");
    Finish F;
    struct AfterWait {  // (host trace: what n1k_finish does behind its wait)
        n1k_handle* h; const Finish* F;
        ~AfterWait() { if (F->wait_end != std::chrono::steady_clock::time_point{}) h->timing.host_us[4] += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - F->wait_end).count(); }
    } after_wait{h, &F};
    const ParsedPlan& pl = h->plan;
    out->nkeys = (uint32_t)pl.keys.size();
    out->naggs = (uint32_t)pl.aggs.size();
    ST_TRY(read_counters(h, F));
    if (!pl.has_group) {
        if (F.err_flags & ERR_UNSUPPORTED_VALUE)
            return fail(h, N1K_UNSUPPORTED_DATA, "a value outside the device subset was met (ordering of arrays/objects)");
        out->nselected = h->filter.selected.size();
        out->selected = h->filter.selected.data();
        h->timing.stats.groups_out = 0;
        return N1K_OK;
    }
    h->timing.stats.rows_selected = F.counters[CTR_ROWS_SELECTED];
    h->timing.stats.wide_key_values = F.counters[CTR_WIDE_VALUES];
    h->timing.stats.distinct_path = 0;
    h->res.keys.clear();
    h->res.aggs.clear();
    h->res.parts.clear();
    h->res.rep.clear();
    // Twice at most: an optimistic COUNT(DISTINCT) reports its overflows with the results (F.vetoed); then once more, exactly.
    for (int pass = 0; pass < 2; pass++) {
        F.sets_exact = pass == 1;
        F.sets_deferred = F.vetoed = false;
        // (a kept region: the table is empty.  Never on the second pass: partition_eligible refuses plans with DISTINCT)
        F.ng = h->part.pending.count ? h->part.pending.count : F.counters[CTR_GROUPS];
        if (F.ng == 0) break;
        if (h->has_distinct) ST_TRY(build_distinct_sets(h, F));
        h->timing.stats.topk_candidates = 0;
        if (F.spec_groups && F.ng <= F.spec_groups) break;  // a speculative hit: the rows are in pin_out already
        const TopKPlan tk = plan_topk(h, F.ng);
        ST_TRY(sized_final_group(h, F, tk.lean));
        if (tk.on) ST_TRY(select_topk(h, F, tk));
        ST_TRY(land_rows(h, F));
        if (!F.vetoed) break;
    }
    if (F.ng > 0) unpack_rows(h, F);
    if (F.ng > 0 && h->has_array_agg && !(F.err_flags & ERR_TABLE_FULL)) ST_TRY(array_agg_groups(h, F.ng, F.counters));
    ST_TRY(flags_status(h, F));
    return host_tail(h, F.ng, out);
    });
}

}  // extern "C"
