// n1k_distinct.cpp — the DISTINCT aggregates: the pair and word logs and the hash regions the scan fills, grown before each
// batch, and the sets built of them at finish (value/set.go:65-110, algebra/agg_count_distinct.go:84-126).
#include "n1k_engine.h"

using namespace n1k;
using namespace n1k_eng;

namespace n1k_eng {

// The pair and word logs with room for every row up to row_base + nrows, and A's log fields.
n1k_status distinct_grow_logs(n1k_handle* h, uint64_t nrows, ScanArgs& A) {
    // every qualifying operand appends one (group key, value, class) pair: at most one per row and aggregate
    uint64_t need = h->row_base + nrows;
    if (need > h->distinct.log_capacity) {
        uint64_t cap = std::max<uint64_t>(need, h->distinct.log_capacity * 2);
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        for (uint32_t d = 0; d < h->n_distinct; d++) {
            DevBuf<uint64_t> nk, nv, nw;
            DevBuf<uint8_t> nc;
            HIP_TRY(h, nk.ensure(cap));
            HIP_TRY(h, nv.ensure(cap));
            HIP_TRY(h, nc.ensure(cap));
            if (h->distinct.words[d]) HIP_TRY(h, nw.ensure(cap));
            if (h->distinct.log_capacity) {
                HIP_TRY(h, hipMemcpy(nk.p, h->distinct.log_key[d].p, h->distinct.log_capacity * 8, hipMemcpyDeviceToDevice));
                HIP_TRY(h, hipMemcpy(nv.p, h->distinct.log_val[d].p, h->distinct.log_capacity * 8, hipMemcpyDeviceToDevice));
                HIP_TRY(h, hipMemcpy(nc.p, h->distinct.log_cls[d].p, h->distinct.log_capacity, hipMemcpyDeviceToDevice));
                if (h->distinct.words[d])
                    HIP_TRY(h, hipMemcpy(nw.p, h->distinct.log_word[d].p, h->distinct.log_capacity * 8, hipMemcpyDeviceToDevice));
            }
            h->distinct.log_key[d] = std::move(nk);
            h->distinct.log_val[d] = std::move(nv);
            h->distinct.log_cls[d] = std::move(nc);
            h->distinct.log_word[d] = std::move(nw);
        }
        h->distinct.log_capacity = cap;
    }
    for (uint32_t d = 0; d < h->n_distinct; d++) {
        A.log_key[d] = h->distinct.log_key[d].p;
        A.log_val[d] = h->distinct.log_val[d].p;
        A.log_cls[d] = h->distinct.log_cls[d].p;
        A.log_word[d] = h->distinct.words[d] ? h->distinct.log_word[d].p : nullptr;
    }
    A.log_cursor = h->groups.counters.p + CTR_PAIR_LOG_CURSORS;
    A.word_cursor = h->groups.counters.p + CTR_WORD_LOG_CURSORS;
    A.log_capacity = h->distinct.log_capacity;
    A.nw_key_bits = h->distinct.nw_key_bits;
    A.nw_val_bits = h->distinct.nw_val_bits;
    if (!h->distinct.word_hist.p) {
        HIP_TRY(h, h->distinct.word_hist.ensure(kMaxDistinct * 256));
        HIP_TRY(h, hipMemsetAsync(h->distinct.word_hist.p, 0, kMaxDistinct * 256 * sizeof(unsigned long long), h->stream));
    }
    A.word_hist = h->distinct.word_hist.p;
    bool any_words = false;
    for (uint32_t d = 0; d < h->n_distinct; d++) any_words |= h->distinct.words[d];
    A.dcache_aggs = any_words ? h->n_distinct : 0;
    A.dcache_slots = any_words ? 4096u / (h->n_distinct > 2 ? 4u : h->n_distinct) : 0;  // 32 KB of LDS in all
    return N1K_OK;
}

// The hash regions of the plan-specialised scan's COUNT(DISTINCT), sized or regrown for nrows more rows, and L.
n1k_status distinct_grow_regions(n1k_handle* h, const Program& P, uint64_t nrows, const ScanArgs& A, uint32_t dcache_slots, WordLogArgs& L) {
    // hash regions: 256 x kRecSubs sub-regions per DISTINCT aggregate, each with room for its share of all rows
    // pushed so far plus a quarter (mix64 spreads distinct words evenly; many copies of few words overflow into the
    // plain word log)
    const uint64_t rows_total = h->row_base + nrows;
    uint64_t need = h->opt.region_cap ? h->opt.region_cap : (rows_total + rows_total / 4) / kWordSubs + 4096;
    need = (need + 15) / 16 * 16;  // whole 128-byte lines
    if (!h->distinct.wcursor.p) {
        HIP_TRY(h, h->distinct.wcursor.ensure(kMaxDistinct * kWordSubs * kCursorStride));
        HIP_TRY(h, hipMemsetAsync(h->distinct.wcursor.p, 0, kMaxDistinct * kWordSubs * kCursorStride * sizeof(unsigned long long), h->stream));
    }
    if (need > h->distinct.wregion_cap) {
        const uint64_t ncap = (std::max<uint64_t>(need, h->distinct.wregion_cap * 2) + 15) / 16 * 16;
        if (ncap >= 0xFFFFFF00ull) return fail(h, N1K_OOM, "COUNT(DISTINCT): more than 2^32 words per hash region");
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        for (uint32_t a = 0; a < P.naggs; a++) {
            if (!P.aggs[a].distinct) continue;
            const uint32_t li = P.aggs[a].log_index;
            DevBuf<uint64_t> nb;
            HIP_TRY(h, nb.ensure(kWordSubs * ncap));
            if (h->distinct.wregion_cap && h->distinct.wregion_used)
                HIP_TRY(h, launch_regrow_regions(h->distinct.wregion[li].p, kWordSubs, h->distinct.wregion_cap, nb.p, ncap,
                                                 h->distinct.wcursor.p + (size_t)li * kWordSubs * kCursorStride, h->stream));  // (clamps the cursors of regions that had overflowed)
            HIP_TRY(h, hipStreamSynchronize(h->stream));
            h->distinct.wregion[li] = std::move(nb);
        }
        h->distinct.wregion_cap = ncap;
    }
    uint32_t d = 0;
    for (uint32_t a = 0; a < P.naggs; a++) {
        if (!P.aggs[a].distinct) continue;
        const uint32_t li = P.aggs[a].log_index;
        L.region[d] = h->distinct.wregion[li].p;
        L.region_cursor[d] = h->distinct.wcursor.p + (size_t)li * kWordSubs * kCursorStride;
        L.over_word[d] = A.log_word[li];
        L.log_key[d] = A.log_key[li];
        L.log_val[d] = A.log_val[li];
        L.log_cls[d] = A.log_cls[li];
        L.log_index[d] = li;
        d++;
    }
    L.region_cap = h->distinct.wregion_cap;
    L.over_cursor = A.word_cursor;
    L.over_hist = A.word_hist;
    L.over_capacity = A.log_capacity;
    L.log_cursor = A.log_cursor;
    L.log_capacity = A.log_capacity;
    L.nw_key_bits = h->distinct.nw_key_bits;
    L.nw_val_bits = h->distinct.nw_val_bits;
    L.dcache_slots = dcache_slots;
    h->distinct.wregion_used = true;
    return N1K_OK;
}

// where the de-duplication kernel counts the new members of each group: by the packed key itself when the plan has one
// dictionary key of a small domain, in an LDS hash table while the group table is small, else per member in HBM
static void dedupe_counters(const n1k_handle* h, DedupeArgs& D) {
    D.direct_keys = 0;
    D.lds_counters = 0;
    const Program& P = h->prog;
    if (P.nkeys == 1 && P.keys[0].mode == KEYM_DICT && P.keys[0].shift == 0 && h->dict.size() + 2 <= 8192)
        D.direct_keys = (uint32_t)h->dict.size() + 2;
    else if (P.nkeys == 0)
        D.direct_keys = 1;
    else if (h->groups.table.capacity <= 4096)
        D.lds_counters = (uint32_t)h->groups.table.capacity;
}

// workgroups of the de-duplication kernel: as many per CU as their LDS (set + member counters) and threads allow
static uint32_t dedupe_grid(const n1k_handle* h, const DedupeArgs& D, uint32_t nbins) {
    const size_t shmem = distinct_dedupe_lds(D) + 512 + 4096;  // (+ the kernel's static arrays: the bounds of its bins)
    const uint32_t by_threads = 2048u / std::max(256u, h->opt.dedupe_block & ~3u);
    const uint32_t per_cu = (uint32_t)std::max<size_t>(1, std::min<size_t>(by_threads, (160 * 1024) / shmem));
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(nbins, (uint64_t)h->num_cus * per_cu));
}

// COUNT(DISTINCT) over the one-word members of one aggregate: radix partition of the word log until a bin's distinct
// words fit an LDS set, per-bin LDS sets, member counts added to the groups' set sizes (see n1k_kernels.hip).
n1k_status distinct_words_finish(n1k_handle* h, const AggSpec& ag, uint64_t nwords, bool hist_counted,
                                 const uint64_t* log) {
    const uint32_t set_slots = h->opt.distinct_set_slots;
    const uint64_t per_bin = std::max<uint64_t>((uint64_t)set_slots * h->opt.distinct_fill_pct / 100, 16);  // expected distinct words per final bin
    const uint32_t levels = h->opt.distinct_levels >= 0 ? (uint32_t)h->opt.distinct_levels
                                                        : (nwords <= per_bin ? 0u : (nwords <= 256 * per_bin ? 1u : 2u));
    if (!log) log = h->distinct.log_word[ag.log_index].p;
    const uint64_t* words = log;
    HIP_TRY(h, h->distinct.seg[0].ensure(2));
    HIP_TRY(h, h->distinct.seg[1].ensure(257));
    HIP_TRY(h, h->distinct.seg[2].ensure(65537));
    HIP_TRY(h, h->distinct.hist.ensure(65536));
    HIP_TRY(h, h->distinct.cursor.ensure(65536));
    HIP_TRY(h, h->distinct.dcounts.ensure(h->groups.table.capacity + 2));
    const uint64_t seg0[2] = {0, nwords};
    HIP_TRY(h, hipMemcpyAsync(h->distinct.seg[0].p, seg0, sizeof seg0, hipMemcpyHostToDevice, h->stream));
    const uint64_t* bin_start = h->distinct.seg[0].p;
    uint32_t nbins = 1;
    for (uint32_t l = 0; l < levels; l++) {
        // (the number of logged words varies a little from run to run — racing duplicates in the scan's cache — so the
        //  buffers get slack: growing them by a few words would mean a fresh 800 MB allocation each time)
        HIP_TRY(h, h->distinct.part[l].ensure(nwords + nwords / 8 + (1u << 20)));
        RadixArgs R{};
        R.src = words;
        R.dst = h->distinct.part[l].p;
        R.seg_start = h->distinct.seg[l].p;
        R.nseg = nbins;
        R.shift = 56 - 8 * l;
        // the scan kernels counted the first digit of every word they logged (ScanArgs::word_hist)
        const bool counted = l == 0 && hist_counted && h->distinct.word_hist.p != nullptr;
        R.hist = counted ? h->distinct.word_hist.p + (size_t)ag.log_index * 256 : h->distinct.hist.p;
        R.cursor = h->distinct.cursor.p;
        R.cursor_stride = nbins == 1 ? kCursorStride : 1u;  // one segment: its 256 cursors would share 16 lines
        R.out_start = h->distinct.seg[l + 1].p;
        // slices per segment: enough workgroups to fill the GPU, never less than one tile each on average
        uint64_t tiles = (nwords + 8191) / 8192;
        uint32_t slices = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)h->num_cus * 8 / nbins + (nbins > 1 ? 8 : 0), tiles));
        HIP_TRY(h, launch_radix_pass(R, slices, h->stream, counted));
        words = R.dst;
        bin_start = R.out_start;
        nbins *= 256;
    }
    uint32_t* d_overflow = (uint32_t*)(h->groups.counters.p + CTR_EXACT_OVERFLOW);
    HIP_TRY(h, hipMemsetAsync(h->distinct.dcounts.p, 0, (h->groups.table.capacity + 2) * sizeof(unsigned long long), h->stream));
    HIP_TRY(h, hipMemsetAsync(d_overflow, 0, 8, h->stream));
    DedupeArgs D{};
    D.words = words;
    D.bin_start = bin_start;
    D.nbins = nbins;
    D.set_slots = set_slots;
    D.key_shift = h->distinct.nw_val_bits + 3;
    D.glob_off = ag.glob_off;
    D.counts = h->distinct.dcounts.p;
    D.overflow = d_overflow;
    dedupe_counters(h, D);
    HIP_TRY(h, launch_distinct_dedupe(h->prog, h->groups.table, D, dedupe_grid(h, D, nbins), h->opt.dedupe_block | (h->opt.dedupe_unroll == 4 ? 2u : 0u), h->stream));
    uint32_t overflow = 0;
    HIP_TRY(h, hipMemcpyAsync(&overflow, d_overflow, 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->distinct.path |= 2u;
    if (overflow) {
        // some bin holds more distinct words than an LDS set takes (more than ~65536 * set_slots / 2 distinct members
        // in all): one open-addressed set in global memory over the whole word log instead
        uint64_t cap = next_pow2(std::max<uint64_t>(nwords * 2, 1024));
        HIP_TRY(h, h->distinct.wtable.ensure(cap));
        HIP_TRY(h, hipMemsetAsync(h->distinct.wtable.p, 0xFF, cap * 8, h->stream));
        HIP_TRY(h, hipMemsetAsync(h->distinct.dcounts.p, 0, (h->groups.table.capacity + 2) * sizeof(unsigned long long), h->stream));
        HIP_TRY(h, launch_distinct_words_global(h->groups.table, log, nwords, h->distinct.wtable.p, cap - 1,
                                                h->distinct.nw_val_bits + 3, h->distinct.dcounts.p, h->groups.errp, h->num_cus * 8, h->stream));
        h->distinct.path |= 4u;
    }
    HIP_TRY(h, launch_distinct_add_counts(h->prog, h->groups.table, h->distinct.dcounts.p, ag.glob_off, h->stream));
    return N1K_OK;
}

// The same when the specialised scan scattered the words into its hash regions already (the first partition pass is
// done): one more pass into bins of fixed capacity — no histogram, mix64 spreads distinct words evenly — and the LDS
// sets, without a host synchronisation (nothing here depends on a count the host would have to read).  Whenever that
// optimism fails (a sub-region or a bin overflowed: many copies of few words; an LDS set too small; words of the
// interpreter kernel in the plain log as well) everything is gathered into one log and the exact path above runs
// instead.  `nover` = words in the plain log.
n1k_status distinct_regions_finish(n1k_handle* h, const AggSpec& ag, uint64_t nover, bool force_exact, bool* deferred) {
    const uint32_t li = ag.log_index;
    const uint64_t cap = h->distinct.wregion_cap;
    unsigned long long* const cursors = h->distinct.wcursor.p + (size_t)li * kWordSubs * kCursorStride;
    const uint32_t set_slots = h->opt.distinct_set_slots;
    const uint64_t per_bin = std::max<uint64_t>((uint64_t)set_slots * h->opt.distinct_fill_pct / 100, 16);
    const bool exact = force_exact || nover > 0 || h->opt.distinct_levels == 0;
    uint32_t* d_overflow = (uint32_t*)(h->groups.counters.p + CTR_OPTIMISTIC_OVERFLOW);  // [0] an LDS set overflowed, [1] a bin of the second pass
    if (!exact) {
        // Optimistic: the member counts are only added to the groups when neither flag came up (the kernel checks), and
        // n1k_finish reads the flags together with the results (*deferred).  The rows pushed bound the words.
        const uint64_t bound = std::max<uint64_t>(h->row_base, 1);
        uint32_t bps = 1;  // bins per region: a bin's words should fit an LDS set at a quarter of its slots
        while (bps < 256 && 256ull * bps * per_bin < bound) bps *= 2;
        if (h->opt.distinct_levels == 2) bps = 256;
        else if (h->opt.distinct_levels == 1) bps = 1;
        const uint64_t nbins = 256ull * bps, mean = bound / nbins + 1, bin_cap = mean + mean / 2 + 256;
        HIP_TRY(h, h->distinct.dcounts.ensure(h->groups.table.capacity + 2));
        HIP_TRY(h, hipMemsetAsync(h->distinct.dcounts.p, 0, (h->groups.table.capacity + 2) * sizeof(unsigned long long), h->stream));
        HIP_TRY(h, h->distinct.part[0].ensure(nbins * bin_cap));
        HIP_TRY(h, h->distinct.cursor.ensure(65536));
        RadixArgs R{};
        R.src = h->distinct.wregion[li].p;
        R.dst = h->distinct.part[0].p;
        R.seg_count = cursors;
        R.seg_stride = cap;
        R.nseg = (uint32_t)kWordSubs;
        R.shift = 48;
        R.cursor = h->distinct.cursor.p;
        R.bin_cap = bin_cap;
        R.overflow = d_overflow + 1;
        const uint64_t region_tiles = (bound / 256 + 8191) / 8192 + kRecSubs;
        // workgroups per region: about three tiles each, 8 to 32 (measured at 100 M rows: 8 / 16 / 32 / 64 workgroups per region take
        // 714 / 670 / 660 / 750 us over 16-byte records — 95 tiles a region — and 382 / 375 / 393 / 452 us over 8-byte words — 48)
        const uint64_t wpr_auto = std::min<uint64_t>(32, std::max<uint64_t>(8, region_tiles / 3));
        const uint32_t wpr = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(h->opt.rec_slices ? h->opt.rec_slices : wpr_auto, region_tiles));
        HIP_TRY(h, launch_radix_scatter_words(R, wpr, bps, h->stream));
        DedupeArgs D{};
        D.words = R.dst;
        D.bin_count = h->distinct.cursor.p;
        D.count_stride = 1;
        D.bin_stride = bin_cap;
        D.nbins = (uint32_t)nbins;
        D.set_slots = set_slots;
        D.key_shift = h->distinct.nw_val_bits + 3;
        D.glob_off = ag.glob_off;
        D.counts = h->distinct.dcounts.p;
        D.overflow = d_overflow;
        dedupe_counters(h, D);
        HIP_TRY(h, launch_distinct_dedupe(h->prog, h->groups.table, D, dedupe_grid(h, D, D.nbins), h->opt.dedupe_block | (h->opt.dedupe_unroll == 4 ? 2u : 0u), h->stream));
        HIP_TRY(h, launch_distinct_add_counts(h->prog, h->groups.table, h->distinct.dcounts.p, ag.glob_off, h->stream, d_overflow));
        h->distinct.path |= 2u;
        *deferred = true;
        return N1K_OK;
    }
    // exact path: the sub-regions' words join the plain log (behind its own words), then partition by histogram
    std::vector<unsigned long long> rc((size_t)kWordSubs * kCursorStride);
    HIP_TRY(h, hipMemcpyAsync(rc.data(), cursors, rc.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    std::vector<uint64_t> off(kWordSubs);
    uint64_t at = nover;
    for (uint32_t b = 0; b < kWordSubs; b++) {
        off[b] = at;
        at += std::min<uint64_t>(rc[(size_t)b * kCursorStride], cap);
    }
    if (at == 0) return N1K_OK;
    HIP_TRY(h, h->distinct.wgather.ensure(at));
    HIP_TRY(h, h->distinct.woff.ensure(kWordSubs));
    if (nover) HIP_TRY(h, hipMemcpyAsync(h->distinct.wgather.p, h->distinct.log_word[li].p, nover * 8, hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->distinct.woff.p, off.data(), kWordSubs * 8, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, launch_compact_regions(h->distinct.wregion[li].p, (uint32_t)kWordSubs, cap, cursors, h->distinct.woff.p, h->distinct.wgather.p, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));  // (`off` lives on this stack frame)
    return distinct_words_finish(h, ag, at, false, h->distinct.wgather.p);
}

}  // namespace n1k_eng
