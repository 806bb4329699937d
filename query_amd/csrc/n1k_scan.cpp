// n1k_scan.cpp — one column batch through Filter + InitialGroup: the one lookup from a plan shape to its plan-specialised
// kernel, prebuilt or built at run time (shape_kernel: for the scan, the records front end and the row exchange's partition);
// which kernel family runs a batch (choose_scan: specialised, bounded-shape, interpreter) and its launches (run_group_batch);
// Filter-only batches, derived columns, staging of host batches.
#include "n1k_engine.h"

using namespace n1k;
using namespace n1k_eng;

namespace n1k_eng {

// Can this plan run on the fast kernel (bounded shape, every descriptor static)?  Fills F when it can.
// fuse: the plan's arithmetic nodes stay out of HBM — the kernel (a run-time-built plan-specialised one) evaluates them in
// registers from the input columns; otherwise they are materialised derived columns and count as inputs.
// partition_only: only columns, terms and keys matter (the row exchange's partition kernels: no aggregate runs there).
bool build_fast_args(n1k_handle* h, uint32_t max_slots, FastArgs& F, bool fuse, bool partition_only) {
    const Program& P = h->prog;
    memset(&F, 0, sizeof F);
    const uint32_t ni = (uint32_t)h->plan.paths.size(), nd = (uint32_t)h->derived.size();
    if (fuse) {
        if (nd == 0 || nd > (uint32_t)kFastDerived || ni == 0 || ni > (uint32_t)kFastCols) return false;
        for (uint32_t d = 0; d < nd; d++) {
            // (collation needs the string ranks, a conditional node its program and cond_kernel: materialised derived columns)
            if (!ar_fuses(h->derived[d].op)) return false;
            for (uint32_t k = 0; k < h->derived[d].nops; k++) {
                const Operand& o = h->derived[d].ops[k];
                if (!o.is_const && o.col >= ni + d) return false;
                if (o.is_const) F.dconst[d][k] = o.cpayload;
            }
        }
        F.nderived = nd;
    }
    if (h->opt.fast == 0 || P.want_rep_row || P.ncols == 0 || (!fuse && P.ncols > (uint32_t)kFastCols)) return false;
    if (P.nkeys > (uint32_t)kFastKeys || (!partition_only && (P.naggs > (uint32_t)kFastAggs || P.naggs == 0))) return false;
    // predicate: none, one term, or AND of two terms
    uint32_t term_ix[2] = {0, 0};
    if (P.nlogic == 0) F.nterms = 0;
    else if (P.nlogic == 1 && P.logic[0].op == LOGIC_PUSH) { F.nterms = 1; term_ix[0] = P.logic[0].arg; }
    else if (P.nlogic == 3 && P.logic[0].op == LOGIC_PUSH && P.logic[1].op == LOGIC_PUSH && P.logic[2].op == LOGIC_AND &&
             P.logic[2].arg == 2) { F.nterms = 2; term_ix[0] = P.logic[0].arg; term_ix[1] = P.logic[1].arg; }
    else return false;
    for (uint32_t i = 0; i < F.nterms; i++) {
        const Term& t = P.terms[term_ix[i]];
        FastTerm& ft = F.terms[i];
        if (t.op >= TERM_NUM_LT && t.op <= TERM_NUM_EQ) {
            if (t.a.is_const) return false;
            ft.op = t.op; ft.col = t.a.col; ft.ctag = t.b.ctag; ft.cpayload = t.b.cpayload;
        } else if (t.op >= TERM_IS_NULL && t.op <= TERM_IS_NOT_VALUED) {
            if (t.a.is_const) return false;
            ft.op = t.op; ft.col = t.a.col;
        } else if (term_is_table_bit(t.op)) {  // column LIKE "pattern", ANY / EVERY over a column, column IN [constants]: the table and its extent travel in the term
            if (t.a.is_const) return false;
            ft.op = t.op; ft.col = t.a.col; ft.match_n = P.match_n; ft.match_mask = 1u << (uint32_t)t.b.cpayload;
            ft.match_bits = P.match_bits;
            if (t.op == TERM_IN) {  // its mask and flags as the term holds them, and its range of the plan's number constants
                const uint32_t begin = (uint32_t)t.c.cpayload, end = (uint32_t)(t.c.cpayload >> 32);
                ft.match_mask = (uint32_t)t.b.cpayload;
                ft.in_nums = P.in_nums + begin;
                ft.in_n = end - begin;
            }
            // (the kernels stage a small table in LDS, kMatchLdsBytes beside the workgroup's table)
            max_slots = (uint32_t)std::min<uint64_t>(max_slots, (156u * 1024u - kMatchLdsBytes) / (P.lds_words * 8));
        } else if (t.op == TERM_EQ) {  // column = "string constant" (either side)
            const Operand *c = nullptr, *k = nullptr;
            if (!t.a.is_const && t.b.is_const && t.b.ctag == T_STRING) { c = &t.a; k = &t.b; }
            else if (!t.b.is_const && t.a.is_const && t.a.ctag == T_STRING) { c = &t.b; k = &t.a; }
            else return false;
            ft.op = TERM_STR_EQ; ft.col = c->col; ft.ctag = T_STRING; ft.cpayload = k->cpayload;
        } else return false;
    }
    // keys: dictionary columns whose domain fits the LDS table are addressed by perfect hash (DIRECT); anything else
    // (integer keys, big dictionaries) goes through an open-addressed LDS table on the packed key (hashed)
    uint64_t domain = 1;
    bool direct = true;
    F.nkeys = P.nkeys;
    for (uint32_t k = 0; k < P.nkeys; k++) {
        const KeySpec& ks = P.keys[k];
        if (ks.src.is_const) return false;
        F.keys[k].col = ks.src.col;
        F.keys[k].shift = ks.shift;
        if (ks.mode != KEYM_DICT) { direct = false; continue; }
        uint64_t radix = (uint64_t)h->dict.size() + 2;
        if (ks.bits < 64 && radix > (1ull << ks.bits)) return false;
        F.keys[k].stride = (uint32_t)std::min<uint64_t>(domain, 0xFFFFFFFFull);
        F.keys[k].radix = (uint32_t)radix;
        domain *= radix;
        if (domain > max_slots) direct = false;
    }
    if (direct) {
        F.hashed = 0;
        F.lds_slots = (uint32_t)std::max<uint64_t>(domain, 2);
    } else {
        F.hashed = 1;
        uint32_t slots = (uint32_t)std::min<uint64_t>(h->opt.lds_bytes / (P.lds_words * 8), 1u << 15);
        if (slots < 16) return false;
        F.lds_slots = slots;
        F.lds_max_fill = std::max(1u, (uint32_t)((uint64_t)slots * 5 / 8));
    }
    F.naggs = partition_only ? 0u : P.naggs;
    uint32_t ndist = 0;
    for (uint32_t a = 0; a < F.naggs; a++) {
        const AggSpec& ag = P.aggs[a];
        if (ag.distinct) {
            // COUNT(DISTINCT column) whose members leave as one word: the specialised kernels scatter them into hash
            // regions; anything else DISTINCT stays with the interpreter kernel
            if (ag.kind != AGG_COUNT || !ag.has_operand || ag.src.is_const || !h->layout_fixed || !h->distinct.words[ag.log_index] ||
                ++ndist > kSpecDistinct)
                return false;
        }
        if (ag.has_operand) {
            if (ag.src.is_const) return false;
            F.agg_col[a] = ag.src.col;
        }
    }
    F.ncols = fuse ? ni : P.ncols;
    for (uint32_t c = 0; c < F.ncols; c++) F.cols[c] = P.cols[c];
    return true;
}

// shape of the compiled plan (what a plan-specialised kernel is instantiated for), as the use's kernels are built for it
static SpecSig make_plan_sig(const n1k_handle* h, const FastArgs& F, ShapeUse use) {
    const Program& P = h->prog;
    SpecSig g{};
    g.ncols = (int)F.ncols; g.nterms = (int)F.nterms; g.nkeys = (int)F.nkeys; g.naggs = (int)F.naggs;
    g.hashed = (int)F.hashed;  // a dictionary domain beyond the LDS has no prebuilt kernel: interpreter
    for (uint32_t c = 0; c < F.ncols; c++) g.col_kind[c] = F.cols[c].kind;
    for (uint32_t t = 0; t < F.nterms; t++) {
        g.terms[t].op = F.terms[t].op;
        g.terms[t].col = F.terms[t].col;
        bool num = F.terms[t].op >= TERM_NUM_LT && F.terms[t].op <= TERM_NUM_EQ;
        g.terms[t].const_int = num && F.terms[t].ctag == T_INT ? 1u : 0u;
    }
    for (uint32_t k = 0; k < F.nkeys; k++) g.key_col[k] = F.keys[k].col;
    for (uint32_t a = 0; a < F.naggs; a++) {
        g.aggs[a].kind = P.aggs[a].kind;
        g.aggs[a].has_operand = P.aggs[a].has_operand;
        g.aggs[a].col = P.aggs[a].has_operand ? F.agg_col[a] : 0u;
        g.aggs[a].distinct = P.aggs[a].distinct ? 1u : 0u;
    }
    g.nderived = (int)F.nderived;
    for (uint32_t d = 0; d < F.nderived; d++) {
        g.derived[d].op = h->derived[d].op;
        g.derived[d].nops = h->derived[d].nops;
        for (uint32_t k = 0; k < h->derived[d].nops; k++) {
            const Operand& o = h->derived[d].ops[k];
            g.derived[d].ops[k].is_const = o.is_const ? 1u : 0u;
            g.derived[d].ops[k].v = o.is_const ? o.ctag : o.col;
        }
    }
    // (segmented batches — a received row region — have their own variant of the scan kernels)
    if (use == ShapeUse::Scan) g.seg = h->push_nseg > 1 ? 1 : 0;
    if (use == ShapeUse::Partition) {
        g.mode = 1;
        g.hashed = 0;  // (no table in this mode)
    }
    return g;
}

bool shape_compiles(const n1k_handle* h, const FastArgs& F, ShapeUse use, std::string* log) {
    return jit_compile_check(make_plan_sig(h, F, use), log);
}

// The one place that knows which plan-specialised kernel serves a shape.  Prebuilt kernels exist for the scan and the
// records front end only, and carry none of the segment bookkeeping; otherwise the same template is instantiated at run
// time — for the scan and the partition from jit_min_rows rows on (or forced: jit = 2), for the records at any row count.
ShapeKernel shape_kernel(n1k_handle* h, const FastArgs& F, ShapeUse use, uint64_t nrows, size_t table_bytes) {
    if (!h->opt.spec) return {};
    const SpecSig g = make_plan_sig(h, F, use);
    // exact-shape lookup among the ahead-of-time instantiated plan shapes (n1k_spec.h)
    if (use != ShapeUse::Partition && !g.seg)
        for (const SpecEntry& e : spec_registry())
            if (memcmp(&e.sig, &g, sizeof g) == 0) return {&e, nullptr, 1u};
    bool build = h->opt.jit && (use == ShapeUse::Records || h->opt.jit == 2 || nrows >= h->opt.jit_min_rows);
    if (use == ShapeUse::Scan) {
        // run-time instantiations take tables of at most 64 KiB, and hash exactly when some key is not a DICT32 input column
        bool key_kinds_hashed = false;
        for (uint32_t k = 0; k < F.nkeys; k++) key_kinds_hashed |= F.keys[k].col >= F.ncols || F.cols[F.keys[k].col].kind != COLK_DICT32;  // (a fused node is a TAGGED64 value)
        build = build && table_bytes <= 64 * 1024 && key_kinds_hashed == (F.hashed != 0);
    } else if (use == ShapeUse::Partition) {
        // what the staging needs in LDS (n1k_spec.h PartLds: 2048 rows x (9 B per TAGGED64 column, 4 B per DICT32 column, 1))
        size_t lds = 2048 + 2048 + 4096;  // (+ the per-destination tables of PartLds)
        for (uint32_t c = 0; c < F.ncols; c++) lds += 2048u * (F.cols[c].kind == COLK_DICT32 ? 4u : 9u);
        build = build && lds + match_lds_bytes(F) <= 60 * 1024;
    }
    if (!build) return {};
    const JitKernel* k = jit_get(g);
    if (k->failed || !(use == ShapeUse::Scan ? k->wide : (use == ShapeUse::Records ? k->rec_wide : k->part_wide))) {
        h->jit_log = k->log;
        return {};
    }
    return {nullptr, k, F.nderived ? 3u : 2u};
}

// What run_group_batch decided for a batch, before it allocates or launches anything.
struct ScanChoice {
    bool interpreter = true;  // the family: the interpreter, else `kernel` (prebuilt or built at run time), else the bounded-shape kernel
    bool shaped = false;  // the plan is of the bounded shape: F, kernel and the LDS sums below are set
    bool fuse = false;    // the kernel evaluates the arithmetic nodes in registers: no derived columns
    ShapeKernel kernel;
    FastArgs F;
    uint32_t ndist = 0;   // DISTINCT aggregates ...
    Program compact;      // ... and the program the specialised kernels run on then (compact LDS layout)
    uint32_t fblock = 0, per_cu = 0, grid_cap = 0;
    bool use_slabs = false;
    uint32_t table_bytes = 0, scatter_bytes = 0, match_lds = 0, dcache_slots = 0, lds_total = 0;
    // the interpreter
    uint32_t max_slots = 0, slots = 0, block = 0, rpl = 0, direct_stride[kMaxKeys] = {}, direct_radix[kMaxKeys] = {};
    bool direct = false;
};

// No allocation, no launch: the only side effects are shape_kernel's (a run-time build, h->jit_log).
static ScanChoice choose_scan(n1k_handle* h, uint64_t nrows) {
    const Program& P = h->prog;
    ScanChoice c;
    FastArgs& F = c.F;
    c.block = h->opt.block ? h->opt.block : 1024;
    c.rpl = c.block == 1024 ? h->opt.rows_per_lane : 4;
    c.max_slots = (uint32_t)std::min<uint64_t>(h->opt.lds_bytes / (P.lds_words * 8), 1u << 15);
    if (c.max_slots < 2) return c;
    // DIRECT tables may take (almost) the whole 160 KiB LDS of a CU: occupancy is chosen from the table size
    const uint32_t direct_max_slots = (uint32_t)std::min<uint64_t>((156u * 1024u) / (P.lds_words * 8), 1u << 15);
    // Shapes with COUNT(DISTINCT): the specialised kernels keep nothing of a DISTINCT aggregate in the workgroup
    // table (its member words go to the hash regions), so they run on a copy of the program with a compact LDS layout
    for (uint32_t a = 0; a < P.naggs; a++) c.ndist += P.aggs[a].distinct ? 1u : 0u;
    if (c.ndist) {
        c.compact = P;
        uint32_t w = 1;
        for (uint32_t a = 0; a < c.compact.naggs; a++) {
            AggSpec& ag = c.compact.aggs[a];
            ag.lds_off = w;
            if (ag.distinct) ag.lds_n = 0;
            else w += (ag.kind == AGG_COUNT || ag.kind == AGG_COUNTN) ? 1u : (ag.kind == AGG_SUM ? kLdsWordsSum : (ag.kind == AGG_AVG ? kLdsWordsAvg : kWordsMinMax));
        }
        c.compact.lds_words = w;
    }
    const uint32_t ndist = c.ndist, lds_words = ndist ? c.compact.lds_words : P.lds_words;
    if (h->opt.agg_mode != N1K_MODE_LDS_HASH) {
        // Arithmetic nodes not materialised yet: first the shape that evaluates them in registers, which exists built at
        // run time only.  Its table is bounded as the handle's program lays it out, compacted or not.  With no such kernel
        // the nodes become derived columns, and the choice is made for the shape that reads them as inputs.
        if (!h->derived_ready && h->opt.fuse_arith && build_fast_args(h, direct_max_slots, F, true)) {
            c.kernel = shape_kernel(h, F, ShapeUse::Scan, nrows, (size_t)F.lds_slots * P.lds_words * 8);
            c.fuse = c.shaped = (bool)c.kernel;
        }
        if (!c.fuse && (c.shaped = build_fast_args(h, direct_max_slots, F, false)))
            c.kernel = shape_kernel(h, F, ShapeUse::Scan, nrows, (size_t)F.lds_slots * lds_words * 8);
    }
    // the bounded-shape kernel is DIRECT only, no DISTINCT, and reads its row count from its arguments
    c.interpreter = !c.shaped || (!c.kernel && (F.hashed || ndist || h->push_nrows_dev || h->push_nseg));
    if (c.interpreter) {
        // DIRECT: every key is dictionary coded and the whole key domain fits the LDS table -> perfect hash
        c.direct = h->opt.agg_mode != N1K_MODE_LDS_HASH;
        uint64_t domain = 1;
        for (uint32_t k = 0; k < P.nkeys && c.direct; k++) {
            if (P.keys[k].mode != KEYM_DICT) c.direct = false;
            uint64_t radix = (uint64_t)h->dict.size() + 2;
            c.direct_stride[k] = (uint32_t)domain;
            c.direct_radix[k] = (uint32_t)std::min<uint64_t>(radix, 0xFFFFFFFFull);
            domain *= radix;
            if (domain > c.max_slots) c.direct = false;
        }
        c.slots = c.direct ? (uint32_t)std::max<uint64_t>(domain, 2) : c.max_slots;
        if (P.nkeys == 0) c.slots = 2;
        return c;
    }
    c.table_bytes = F.lds_slots * lds_words * 8;
    c.match_lds = match_lds_bytes(F);  // static LDS of the staged match table: part of every budget below
    // the word scatter's LDS (per DISTINCT aggregate one ScatterLds<uint64_t, 512, 4>, n1k_scatter.h: 2048 staged words,
    // counters, run starts) and, in what is left of the workgroup's share of the CU, its "already logged" caches
    c.scatter_bytes = ndist * (2048u * 8u + 2u * 256u * 4u + 256u * 4u + 256u * 8u + 2048u) + (ndist ? 64u : 0u);
    if (ndist) {
        const uint32_t without = c.table_bytes + c.scatter_bytes + c.match_lds;
        const uint32_t share = 160u * 1024u / std::max(1u, std::min(3u, 160u * 1024u / (without + 512u)));
        for (uint32_t sl = 4096; sl >= 64; sl >>= 1)
            if (without + ndist * sl * 8u + 512u <= share) { c.dcache_slots = sl; break; }
    }
    c.lds_total = c.table_bytes + c.scatter_bytes + ndist * c.dcache_slots * 8u + c.match_lds;
    // workgroups per CU that fit: 512 threads x 3 (<= 48 KiB each), x 2 (<= 72 KiB), else 1024 threads x 1
    c.fblock = h->opt.block == 1024 || h->opt.block == 512 ? h->opt.block : (c.table_bytes <= 72 * 1024 ? 512u : 1024u);
    if (ndist) c.fblock = 512;
    c.per_cu = c.fblock == 512 ? (c.lds_total <= 48 * 1024 ? 3u : (c.lds_total <= 72 * 1024 ? 2u : 1u))
                               : (c.lds_total <= 72 * 1024 ? 2u : 1u);
    if (ndist) c.per_cu = std::max(1u, std::min(3u, 160u * 1024u / (c.lds_total + 512u)));  // (two workgroups of 80 KiB fit a CU)
    if (c.kernel.jit && c.fblock != 512) {  // run-time instantiations are built for 512-thread workgroups
        c.fblock = 512;
        c.per_cu = c.table_bytes + c.match_lds <= 48 * 1024 ? 3u : 2u;
    }
    c.grid_cap = h->opt.grid_blocks ? h->opt.grid_blocks : (uint32_t)(h->num_cus * c.per_cu);
    // slabs + merge kernel pay off once the table is more than a few KiB
    c.use_slabs = !F.hashed && (h->opt.slabs == 1 ? c.table_bytes >= 4096 : h->opt.slabs == 2);
    return c;
}

// Every LDS accumulator keeps an int SUM / AVG as ONE wrapping 64-bit word per slot and takes |x| < 2^40 into it (acc_lds,
// acc_lds_value, spec_acc): a workgroup whose share of a launch is at most 2^23 rows cannot wrap that word, whatever the
// rows hold.  Workgroup b takes the tiles b, b + grid, b + 2 grid, ...: the smallest grid that keeps its
// ceil(tiles / grid) tiles within 2^23 rows.  It overrides grid_blocks; the default grids are above it up to 2^31 rows.
static uint32_t min_grid_for_narrow_sums(uint64_t tiles, uint64_t tile_rows) {
    const uint64_t per_workgroup = std::max<uint64_t>(1, (1ull << 23) / tile_rows);
    return (uint32_t)((tiles + per_workgroup - 1) / per_workgroup);
}

// Rows [off, off + n) of the bound columns through the chosen kernel on program P: slabs for the grid, the launch, the
// merge — or, slabs_to_rows, none: the slabs stay for n1k_finish.
// A specialised kernel takes its WIDE form (2 adjacent rows per lane and load) over the even prefix of aligned
// columns, and an odd last row through a second, scalar launch.
static n1k_status launch_chunk(n1k_handle* h, const ScanChoice& c, const Program& P, FastArgs& F, const WordLogArgs& L, uint64_t off, uint64_t n, bool only_chunk) {
    unsigned long long* ngroups = h->groups.counters.p + CTR_GROUPS;
    auto launch = [&](uint32_t g, bool wide) {
        if (c.kernel.spec) return c.kernel.spec->launch(P, F, h->groups.table, ngroups, g, c.fblock, wide, L, h->stream);
        if (c.kernel.jit) return jit_launch(c.kernel.jit, P, F, h->groups.table, ngroups, g, wide, L, c.ndist, h->stream);
        return launch_scan_fast(P, F, h->groups.table, ngroups, g, c.fblock, h->opt.rows_per_lane, h->stream);
    };
    F.row_base = h->row_base + off;
    std::copy_n(P.cols, F.ncols, F.cols);
    advance_cols(F.cols, F.ncols, off);
    const bool wide = c.kernel && cols_wide_aligned(F.cols, F.ncols) && h->opt.wide && n >= 2;
    // (a row count that lives on the device may be odd: the kernel masks the last item's second row itself)
    const uint64_t n_main = wide && !h->push_nrows_dev && !h->push_nseg ? (n & ~1ull) : n;
    F.nrows = (uint32_t)n_main;
    const uint64_t items = wide ? (n_main + 1) / 2 : n_main;
    const uint32_t rpl = !c.kernel ? h->opt.rows_per_lane : (wide ? 2 : 4);
    uint64_t tiles = (items + (uint64_t)c.fblock * rpl - 1) / ((uint64_t)c.fblock * rpl);
    if (c.ndist) tiles = (tiles + 3) / 4;  // a workgroup reserves chunks in every hash region: give it a few tiles to fill them
    const uint64_t tile_rows = (uint64_t)c.fblock * rpl * (wide ? 2u : 1u) * (c.ndist ? 4u : 1u);
    // (a segmented batch numbers its tiles segment by segment: up to one partial tile more per segment)
    const uint64_t share_tiles = tiles + (h->push_nseg > 1 ? h->push_nseg : 0u);
    const uint32_t g = (uint32_t)std::max<uint64_t>(std::max<uint32_t>(1, min_grid_for_narrow_sums(share_tiles, tile_rows)), std::min<uint64_t>(c.grid_cap, tiles));
    if (c.use_slabs && g > 1) {  // (F.slabs is null here: build_fast_args, and below)
        HIP_TRY(h, h->groups.slabs.ensure((size_t)g * P.lds_words * F.lds_slots));
        HIP_TRY(h, h->groups.block_sel.ensure(g));
        F.slabs = h->groups.slabs.p;
        F.block_selected = h->groups.block_sel.p;
    }
    HIP_TRY(h, launch(g, wide));
    if (F.slabs && &P == &h->prog && slabs_to_rows(h, F, g, only_chunk, n_main == n)) {
        // a one-call execution's only launch: n1k_finish folds the slabs straight into result rows (read_counters)
        h->groups.pending.grid = g;
        h->groups.pending.F = F;
    } else if (F.slabs)
        HIP_TRY(h, launch_merge_slabs(P, F, h->groups.table, g, ngroups, h->stream, h->opt.merge_chunks));
    F.slabs = nullptr;
    if (n_main < n) {
        advance_cols(F.cols, F.ncols, n_main);
        F.nrows = (uint32_t)(n - n_main);
        F.row_base += n_main;
        HIP_TRY(h, launch(1, false));
    }
    return N1K_OK;
}

// The batch through the chosen specialised or bounded-shape kernel, in launches of at most 2^31 rows.
static n1k_status run_shaped(n1k_handle* h, ScanChoice& c, const ScanArgs& A, uint64_t nrows) {
    const Program& P = c.ndist ? c.compact : h->prog;
    FastArgs& F = c.F;
    F.err_flags = h->groups.errp;
    F.rows_selected = h->groups.counters.p + CTR_ROWS_SELECTED;
    F.nrows_dev = h->push_nrows_dev;
    if (h->push_nseg > 1) {
        if (h->push_nseg > kMaxSegments || nrows >= (1ull << 31)) return fail(h, N1K_INVALID, "segmented batch too large");
        F.nseg = h->push_nseg;
        F.seg_rows = (uint32_t)h->push_seg_rows;
        F.seg_count_stride = kCursorStride;
        F.seg_counts = h->push_seg_counts;
    }
    WordLogArgs L{};
    if (c.ndist) {
        n1k_status st = distinct_grow_regions(h, P, nrows, A, c.dcache_slots, L);
        if (st != N1K_OK) return st;
    }
    hipEvent_t e0 = get_event(h), e1 = get_event(h);
    if (e0) (void)hipEventRecord(e0, h->stream);
    const uint64_t chunk = 1ull << 31;  // 32-bit row indices inside one launch
    for (uint64_t off = 0; off < nrows; off += chunk) {
        n1k_status st = launch_chunk(h, c, P, F, L, off, std::min<uint64_t>(chunk, nrows - off), nrows <= chunk);
        if (st != N1K_OK) return st;
    }
    if (e1) (void)hipEventRecord(e1, h->stream);
    h->timing.events.emplace_back(e0, e1);
    h->timing.stats.agg_mode = F.hashed ? N1K_MODE_LDS_HASH : N1K_MODE_LDS_DIRECT;
    return N1K_OK;
}

// The batch through the interpreter kernel.
static n1k_status run_interpreter(n1k_handle* h, const ScanChoice& c, ScanArgs& A, uint64_t nrows) {
    const Program& P = h->prog;
    memcpy(A.direct_stride, c.direct_stride, sizeof A.direct_stride);
    memcpy(A.direct_radix, c.direct_radix, sizeof A.direct_radix);
    A.lds_slots = c.slots;
    A.lds_max_fill = std::max(1u, (uint32_t)((uint64_t)c.slots * 5 / 8));
    A.err_flags = h->groups.errp;
    A.rows_selected = h->groups.counters.p + CTR_ROWS_SELECTED;
    uint64_t tile_rows = (uint64_t)c.block * c.rpl;
    uint64_t ntiles = (nrows + tile_rows - 1) / tile_rows;
    uint32_t per_cu = c.block == 1024 ? 1 : (c.block == 512 ? 2 : 4);
    uint32_t grid = h->opt.grid_blocks ? h->opt.grid_blocks : (uint32_t)(h->num_cus * per_cu);
    grid = (uint32_t)std::max<uint64_t>(std::max<uint32_t>(1, min_grid_for_narrow_sums(ntiles, tile_rows)), std::min<uint64_t>(grid, ntiles));
    hipEvent_t e0 = get_event(h), e1 = get_event(h);
    if (e0) (void)hipEventRecord(e0, h->stream);
    if (h->push_nseg > 1) {
        // a segmented batch on the interpreter: one launch per segment, its row count read on the device
        Program Ps = P;
        for (uint32_t sg = 0; sg < h->push_nseg; sg++) {
            std::copy_n(P.cols, P.ncols, Ps.cols);  // (derived columns too: they were evaluated over the whole capacity, row for row)
            advance_cols(Ps.cols, P.ncols, (uint64_t)sg * h->push_seg_rows);
            ScanArgs As = A;
            As.nrows = h->push_seg_rows;
            As.nrows_dev = h->push_seg_counts + (size_t)sg * kCursorStride;
            const uint64_t nt = (h->push_seg_rows + tile_rows - 1) / tile_rows;
            const uint32_t g = (uint32_t)std::max<uint64_t>(std::max<uint32_t>(1, min_grid_for_narrow_sums(nt, tile_rows)), std::min<uint64_t>(grid, nt));
            HIP_TRY(h, launch_scan_group(Ps, As, h->groups.table, h->groups.counters.p + CTR_GROUPS, g, c.block, c.rpl, c.direct, h->stream));
        }
    } else
        HIP_TRY(h, launch_scan_group(P, A, h->groups.table, h->groups.counters.p + CTR_GROUPS, grid, c.block, c.rpl, c.direct, h->stream));
    if (e1) (void)hipEventRecord(e1, h->stream);
    h->timing.events.emplace_back(e0, e1);
    h->timing.stats.agg_mode = c.direct ? N1K_MODE_LDS_DIRECT : N1K_MODE_LDS_HASH;
    return N1K_OK;
}

// One batch through Filter + InitialGroup: room in the table and the DISTINCT logs, the choice, derived columns unless the
// chosen kernel evaluates the arithmetic nodes itself, the launches.
n1k_status run_group_batch(n1k_handle* h, const n1k_batch* b) {
    n1k_status st = ensure_table(h, b->nrows);
    if (st != N1K_OK) return st;
    ScanArgs A{};
    A.nrows = b->nrows;
    A.nrows_dev = h->push_nrows_dev;
    A.row_base = h->row_base;
    if (h->has_distinct) {
        st = distinct_grow_logs(h, b->nrows, A);
        if (st != N1K_OK) return st;
    }
    ScanChoice c = choose_scan(h, b->nrows);
    if (c.max_slots < 2) return fail(h, N1K_UNSUPPORTED, "accumulator row too wide for LDS");
    if (!c.fuse) {
        st = materialize_derived(h, b);
        if (st != N1K_OK) return st;
        if (c.ndist) std::copy_n(h->prog.cols, h->prog.ncols, c.compact.cols);  // (copied before the derived columns were bound)
    }
    if (c.shaped) h->timing.stats.spec_kernel = c.kernel.stat;
    return c.interpreter ? run_interpreter(h, c, A, b->nrows) : run_shaped(h, c, A, b->nrows);
}

// one comparison of a TAGGED64 column with a NUMBER constant, arrays aligned for two rows per load: the wide variant
bool filter_stream_fast(const n1k_handle* h) {
    const Program& P = h->prog;
    if (!(h->opt.wide && P.nlogic == 1 && P.logic[0].op == LOGIC_PUSH)) return false;
    const Term& t = P.terms[P.logic[0].arg];
    return t.op >= TERM_NUM_LT && t.op <= TERM_NUM_EQ && !t.a.is_const && t.a.col < (uint32_t)h->plan.paths.size() &&
           P.cols[t.a.col].kind == COLK_TAGGED64 && (uintptr_t)P.cols[t.a.col].payload % 16 == 0 && (uintptr_t)P.cols[t.a.col].tags % 2 == 0;
}

uint32_t filter_stream_grid(const n1k_handle* h, uint64_t ntiles, bool fast) {
    if (fast)  // (84 VGPRs; measured 4: 0.43, 5: 0.39, 6: 0.40, 8: 0.40 ms per 100 M rows)
        return (uint32_t)std::min<uint64_t>(ntiles, (uint64_t)h->num_cus * (h->opt.grid_blocks ? h->opt.grid_blocks : 5));
    return (uint32_t)std::min<uint64_t>(ntiles, (uint64_t)h->num_cus * 4);  // (124 VGPRs: four 256-thread workgroups per CU)
}

n1k_status run_filter_batch(n1k_handle* h, const n1k_batch* b) {
    Program& P = h->prog;
    if (b->nrows == 0) return N1K_OK;
    hipEvent_t e0 = get_event(h), e1 = get_event(h);
    unsigned long long total = 0;
    // ONE pass (filter_stream_kernel): predicate, ordered compaction and the tiles' offsets by a chained scan; the ordinals
    // land in a buffer sized for every row, the host reads the count and copies that many
    const uint64_t ntiles = (b->nrows + kFilterStreamTile - 1) / kFilterStreamTile;
    HIP_TRY(h, h->filter.tile_off.ensure(ntiles + 1));
    HIP_TRY(h, h->filter.sel.ensure(b->nrows));
    const bool fast = filter_stream_fast(h);
    const uint32_t grid = filter_stream_grid(h, ntiles, fast);
    if (e0) (void)hipEventRecord(e0, h->stream);
    HIP_TRY(h, launch_filter_stream(P, b->nrows, h->row_base, h->filter.sel.p, (unsigned long long*)h->filter.tile_off.p,
                                    (unsigned long long*)h->filter.tile_off.p + ntiles, h->groups.counters.p + CTR_FILTER_TOTAL, h->groups.errp, grid, h->stream, fast));
    h->timing.stats.spec_kernel = fast ? 1u : 0u;
    if (e1) (void)hipEventRecord(e1, h->stream);  // device time excludes the PCIe copy of the ordinals
    HIP_TRY(h, hipMemcpyAsync(&total, h->groups.counters.p + CTR_FILTER_TOTAL, sizeof total, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (total) {
        size_t old = h->filter.selected.size();
        h->filter.selected.resize(old + total);
        HIP_TRY(h, hipMemcpyAsync(h->filter.selected.data() + old, h->filter.sel.p, total * 8, hipMemcpyDeviceToHost, h->stream));
    }
    h->timing.events.emplace_back(e0, e1);
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->timing.stats.rows_selected += total;
    return N1K_OK;
}

// Point the program at this batch's input columns and evaluate the arithmetic nodes into derived columns (defer: not
// yet — run_group_batch first looks for a kernel that evaluates them in registers, and materialises them otherwise).
n1k_status bind_columns(n1k_handle* h, const n1k_batch* b, bool defer) {
    Program& P = h->prog;
    // first push: give the plan's string constants their dictionary codes
    auto resolve = [&](Operand& o) {
        if (o.is_const && o.ctag == T_STRING && o.pad == 1) {
            o.cpayload = intern(h, h->const_strings[(size_t)o.cpayload]);
            o.pad = 0;
        }
    };
    for (uint32_t t = 0; t < P.nterms; t++) { resolve(P.terms[t].a); resolve(P.terms[t].b); resolve(P.terms[t].c); }
    for (uint32_t k = 0; k < P.nkeys; k++) resolve(P.keys[k].src);
    for (uint32_t a = 0; a < P.naggs; a++) resolve(P.aggs[a].src);
    for (auto& d : h->derived)
        for (uint32_t k = 0; k < d.nops; k++) resolve(d.ops[k]);
    // (a THEN constant equal to a string the dictionary holds gets that string's code: the two are one group key)
    for (auto& n : h->cond_nodes) {
        for (uint32_t t = 0; t < n.nterms; t++) { resolve(n.terms[t].a); resolve(n.terms[t].b); resolve(n.terms[t].c); }
        for (uint32_t a = 0; a < n.narms; a++) resolve(n.arms[a].then);
        resolve(n.els);
    }
    const uint32_t ni = (uint32_t)h->plan.paths.size();
    for (uint32_t c = 0; c < ni; c++) {
        P.cols[c].kind = b->cols[c].kind == N1K_COL_DICT32 ? COLK_DICT32 : COLK_TAGGED64;
        P.cols[c].tags = b->cols[c].tags;
        P.cols[c].payload = b->cols[c].payload;
        P.cols[c].codes = b->cols[c].codes;
    }
    bool tagged_key = false;
    for (uint32_t k = 0; k < P.nkeys; k++) tagged_key |= P.keys[k].mode == KEYM_TAGGED;  // (fix_layout came first)
    if (tagged_key) {  // FLOAT group keys that are NaN / +-Inf are the strings they marshal to (n1k_device.h pack_key_field)
        P.nan_code = intern(h, "NaN");
        P.pinf_code = intern(h, "+Infinity");
        P.ninf_code = intern(h, "-Infinity");
    }
    P.dict_size = (uint32_t)h->dict.size();
    P.empty_str_code = lookup_code(h, "");
    P.empty_arr_code = lookup_code(h, "[]");
    P.empty_obj_code = lookup_code(h, "{}");
    h->derived_ready = h->derived.empty();
    if (h->derived_ready) return N1K_OK;
    for (size_t i = 0; i < h->derived.size(); i++) {
        DevCol& d = P.cols[ni + i];
        d.kind = COLK_TAGGED64;
        d.tags = nullptr;
        d.payload = nullptr;
        d.codes = nullptr;
    }
    return defer ? N1K_OK : materialize_derived(h, b);
}

// one element-wise launch per node — arith_kernel, cond_kernel for a conditional node, arrfn_lookup_kernel for an array
// function: the node's values as a TAGGED64 column in HBM
n1k_status materialize_derived(n1k_handle* h, const n1k_batch* b) {
    Program& P = h->prog;
    if (h->derived_ready) return N1K_OK;
    const uint32_t ni = (uint32_t)h->plan.paths.size();
    for (const auto& d : h->derived)
        if (ar_needs_rank(d.op)) {  // GREATEST / LEAST, and a WHEN that orders strings, collate them by rank: the table must cover this batch's dictionary
            n1k_status rst = ensure_rank(h);
            if (rst != N1K_OK) return rst;
            break;
        }
    ST_TRY(ensure_value_table(h));  // array functions: their value tables must cover this batch's dictionary
    ST_TRY(ensure_datestr_table(h));  // str_to_millis / date_part_str: likewise
    if (!h->cond_nodes.empty() && !h->cond_uploaded) {  // once per plan: bind_columns has given the string constants their codes
        HIP_TRY(h, h->d_cond.ensure(h->cond_nodes.size()));
        HIP_TRY(h, hipMemcpy(h->d_cond.p, h->cond_nodes.data(), h->cond_nodes.size() * sizeof(CondNode), hipMemcpyHostToDevice));
        h->cond_uploaded = true;
    }
    h->dv_tags.resize(h->derived.size());
    h->dv_payload.resize(h->derived.size());
    for (size_t i = 0; i < h->derived.size(); i++) {
        // an earlier launch may still read the previous batch's derived columns
        if (h->dv_tags[i].n < b->nrows) HIP_TRY(h, hipStreamSynchronize(h->stream));
        HIP_TRY(h, h->dv_tags[i].ensure(std::max<uint64_t>(b->nrows, 1)));
        HIP_TRY(h, h->dv_payload[i].ensure(std::max<uint64_t>(b->nrows, 1)));
        if (h->derived[i].op == AR_COND) {
            // (the program by value, as the scan kernels take it: its columns, earlier nodes' among them, the ranks, the codes of
            //  the empty string / array / object)
            CondArgs C{};
            C.node = h->d_cond.p + h->derived[i].node;
            C.nrows = b->nrows;
            C.nrows_dev = h->push_nrows_dev;
            if (h->push_nseg > 1) {
                C.seg_counts = h->push_seg_counts;
                C.seg_rows = h->push_seg_rows;
                C.nseg = h->push_nseg;
            }
            C.out_tags = h->dv_tags[i].p;
            C.out_payload = h->dv_payload[i].p;
            C.err_flags = h->groups.errp;
            HIP_TRY(h, launch_cond(P, C, h->stream));
            DevCol& d = P.cols[ni + i];
            d.kind = COLK_TAGGED64;
            d.tags = C.out_tags;
            d.payload = C.out_payload;
            d.codes = nullptr;
            continue;
        }
        if (h->derived[i].op == AR_ARRFN) {  // one lookup per row in the term's value table (n1k_arrfn.h)
            const ArrFnTable& T = h->arrfn;
            ArrFnLookupArgs L{};
            L.col = P.cols[h->derived[i].ops[0].col];  // (a leaf path: an input column)
            L.tab_tags = T.d_tags[h->derived[i].node].p;
            L.tab_payload = T.d_payload[h->derived[i].node].p;
            L.tab_n = (uint32_t)T.built_for;
            L.nrows = b->nrows;
            L.nrows_dev = h->push_nrows_dev;
            if (h->push_nseg > 1) {
                L.seg_counts = h->push_seg_counts;
                L.seg_rows = h->push_seg_rows;
                L.nseg = h->push_nseg;
            }
            L.out_tags = h->dv_tags[i].p;
            L.out_payload = h->dv_payload[i].p;
            HIP_TRY(h, launch_arrfn_lookup(L, h->stream));
            DevCol& d = P.cols[ni + i];
            d.kind = COLK_TAGGED64;
            d.tags = L.out_tags;
            d.payload = L.out_payload;
            d.codes = nullptr;
            continue;
        }
        if (h->derived[i].op == AR_DATESTR) {  // one lookup per row in the term's value table (n1k_datefn.h)
            const DateStrTable& T = h->datestr;
            DateStrLookupArgs L{};
            L.col = P.cols[h->derived[i].ops[0].col];  // (a leaf path: an input column)
            L.tab_tags = T.d_tags[h->derived[i].node].p;
            L.tab_payload = T.d_payload[h->derived[i].node].p;
            L.tab_n = (uint32_t)T.built_for;
            L.nrows = b->nrows;
            L.nrows_dev = h->push_nrows_dev;
            if (h->push_nseg > 1) {
                L.seg_counts = h->push_seg_counts;
                L.seg_rows = h->push_seg_rows;
                L.nseg = h->push_nseg;
            }
            L.out_tags = h->dv_tags[i].p;
            L.out_payload = h->dv_payload[i].p;
            L.err_flags = h->groups.errp;
            HIP_TRY(h, launch_datestr_lookup(L, h->stream));
            DevCol& d = P.cols[ni + i];
            d.kind = COLK_TAGGED64;
            d.tags = L.out_tags;
            d.payload = L.out_payload;
            d.codes = nullptr;
            continue;
        }
        ArithArgs A{};
        A.op = h->derived[i].op;
        A.nops = h->derived[i].nops;
        for (uint32_t k = 0; k < A.nops; k++) A.ops[k] = h->derived[i].ops[k];
        for (uint32_t c = 0; c < ni + i; c++) A.cols[c] = P.cols[c];
        A.nrows = b->nrows;
        A.out_tags = h->dv_tags[i].p;
        A.out_payload = h->dv_payload[i].p;
        A.str_rank = h->d_rank.p;
        A.err_flags = h->groups.errp;
        if (ar_is_datefn(A.op)) {  // (it can raise: the rows a received region does not hold are skipped, as cond_kernel skips them)
            A.nrows_dev = h->push_nrows_dev;
            if (h->push_nseg > 1) {
                A.seg_counts = h->push_seg_counts;
                A.seg_rows = h->push_seg_rows;
                A.nseg = h->push_nseg;
            }
        }
        // (a library or date function has a kernel of its own, which carries that routine alone)
        HIP_TRY(h, ar_is_datefn(A.op) ? launch_datefn(A, h->stream) : ar_is_mathfn(A.op) ? launch_mathfn(A, h->stream) : launch_arith(A, h->stream));
        DevCol& d = P.cols[ni + i];
        d.kind = COLK_TAGGED64;
        d.tags = A.out_tags;
        d.payload = A.out_payload;
        d.codes = nullptr;
    }
    h->derived_ready = true;
    return N1K_OK;
}

n1k_status push_device(n1k_handle* h, const n1k_batch* b) {
    if (h->stop_flag.load()) return fail(h, N1K_STOPPED, "operator was stopped");
    // (the first push behind a reset that left the device clean; a second push finds device_clean false)
    h->groups.pending.clean_at_push = h->device_clean && h->row_base == 0 && h->groups.merged_bound == 0 && !h->groups.pending.grid;
    h->device_clean = false;
    n1k_status st = ensure_device(h);
    if (st != N1K_OK) return st;
    st = validate_batch(h, b);
    if (st != N1K_OK) return st;
    if (!h->layout_fixed) {
        st = fix_layout(h, b);
        if (st != N1K_OK) return st;
    }
    // High-cardinality GROUP BY: beyond a few ten thousand groups the scan's LDS stage absorbs nothing and every row
    // costs atomics on a table in HBM.  Whether a batch is like that is learnt from the data: the first rows of a
    // large batch run through the scan kernels; if they bring many new groups, the rest is partitioned (below).
    st = flush_pending(h);  // a region kept from the previous batch joins the table before more rows arrive
    if (st != N1K_OK) return st;
    const bool first_rows = h->row_base == 0 && h->groups.merged_bound == 0;  // nothing in the handle yet
    PartitionPlan pp;
    const bool can_partition = h->plan.has_group && !h->push_nrows_dev && !h->push_nseg && partition_eligible(h, pp);
    uint64_t head = b->nrows;
    bool decide = false;
    if (can_partition && h->opt.agg_mode == N1K_MODE_PARTITIONED) head = 0;
    else if (can_partition && h->opt.agg_mode == N1K_MODE_AUTO && b->nrows >= h->opt.partition_min_rows && !small_key_domain(h)) {
        head = std::min<uint64_t>(b->nrows, h->opt.partition_probe_rows);
        decide = true;
    }
    auto view = [&](uint64_t off, uint64_t n, std::vector<n1k_col>& cols, n1k_batch& v) {
        cols.assign(b->cols, b->cols + b->ncols);
        advance_cols(cols.data(), b->ncols, off);
        v.nrows = n;
        v.ncols = b->ncols;
        v.cols = cols.data();
    };
    std::vector<n1k_col> cols;
    n1k_batch v{};
    view(0, b->nrows, cols, v);
    // (the probe, the partitioned path and the Filter-only kernels read derived columns; run_group_batch decides itself)
    const bool defer = h->plan.has_group && !decide && !(can_partition && head == 0);
    st = bind_columns(h, &v, defer);
    if (st != N1K_OK) return st;
    st = ensure_rank(h);
    if (st != N1K_OK) return st;
    st = ensure_match_table(h);
    if (st != N1K_OK) return st;
    bool partition = can_partition && head == 0 && b->nrows > 0;
    uint64_t groups_est = b->nrows;
    if (decide && first_rows && h->opt.partition_sticky && h->part.sticky.valid && b->nrows >= h->part.sticky.rows / 2 && b->nrows <= h->part.sticky.rows * 2) {
        decide = false;  // as the last execution over a batch of this size went: no probe (see n1k_handle::sticky)
        partition = true;
        groups_est = std::min<uint64_t>(b->nrows, h->part.sticky.groups_est * b->nrows / std::max<uint64_t>(h->part.sticky.rows, 1) + 1024);
    }
    if (decide) {
        h->groups.pending.clean_at_push = false;  // (the probe's keys are in the table)
        // probe: Filter + group key of the first `head` rows into the table (keys only), counted before and after
        st = ensure_table(h, head);
        if (st != N1K_OK) return st;
        unsigned long long before = 0, after = 0;
        HIP_TRY(h, hipMemcpyAsync(&before, h->groups.counters.p + CTR_GROUPS, sizeof before, hipMemcpyDeviceToHost, h->stream));
        const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)h->num_cus * 4, (head + 1023) / 1024));
        HIP_TRY(h, launch_probe_keys(h->prog, head, h->groups.table, h->groups.errp, h->groups.counters.p + CTR_GROUPS, grid, h->stream));
        HIP_TRY(h, hipMemcpyAsync(&after, h->groups.counters.p + CTR_GROUPS, sizeof after, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        const uint64_t fresh = after > before ? after - before : 0;
        partition = fresh >= h->opt.partition_min_groups;
        // how many groups will the batch bring?  If the keys are draws from a universe of U values, m draws show
        // d = U (1 - e^(-m/U)) of them: solve for U from the probe (m = head rows, d = fresh groups) and evaluate at
        // the batch.  (All-distinct probes have no finite U: the row count stays the bound.)  Only the number of
        // partition passes and the size of the per-bin LDS tables hang on it; a low guess costs speed, not results.
        const double m = (double)head, d = (double)std::max<uint64_t>(1, fresh);
        if (d < 0.98 * m) {
            double lo = d, hi = 1e18;
            for (int it = 0; it < 200; it++) {
                const double U = std::sqrt(lo * hi);
                if (U * (1.0 - std::exp(-m / U)) < d) lo = U; else hi = U;
            }
            const double U = lo, nn = (double)b->nrows;
            groups_est = std::min<uint64_t>(groups_est, (uint64_t)(2.0 * U * (1.0 - std::exp(-nn / U))) + 1024);
        }
        if (partition && first_rows && h->groups.table.capacity) {
            // the probe's keys are all the handle holds: drop them, so that the partitioned path's groups can stay in
            // their compact region (no table at all for this query)
            HIP_TRY(h, launch_init_table(h->prog, h->groups.table, 0, h->groups.table.capacity, nullptr, h->stream));
            HIP_TRY(h, hipMemsetAsync(h->groups.counters.p + CTR_GROUPS, 0, sizeof(unsigned long long), h->stream));
        }
    }
    if (b->nrows) {
        if (!h->plan.has_group) st = run_filter_batch(h, &v);
        else if (partition) {
            bool done = false;
            st = run_group_records(h, &v, pp, groups_est, first_rows, &done);
            h->part.sticky.valid = st == N1K_OK && done && first_rows && h->opt.agg_mode == N1K_MODE_AUTO;
            h->part.sticky.rows = b->nrows;
            h->part.sticky.groups_est = groups_est;
            if (st == N1K_OK && !done) st = run_group_partitioned(h, &v, pp, groups_est, first_rows);
        } else
            st = run_group_batch(h, &v);
        if (st != N1K_OK) return st;
    }
    h->row_base += b->nrows;
    h->timing.stats.rows_in += b->nrows;
    h->timing.stats.batches += 1;
    h->timing.stats.bytes_scanned += b->nrows * batch_bytes_per_row(h);
    return N1K_OK;
}

// host columns -> the handle's staging buffers on the device (the caller's memory is not retained after return: cgo rule)
n1k_status stage_host_batch(n1k_handle* h, const n1k_batch* batch, std::vector<n1k_col>& dcols) {
    uint32_t nc = batch->ncols;
    const int set = h->stage.cur;
    auto& s_tags = h->stage.tags[set];
    auto& s_payload = h->stage.payload[set];
    auto& s_codes = h->stage.codes[set];
    s_tags.resize(std::max<size_t>(s_tags.size(), nc));
    s_payload.resize(std::max<size_t>(s_payload.size(), nc));
    s_codes.resize(std::max<size_t>(s_codes.size(), nc));
    if (!h->stage.copy_stream) {
        HIP_TRY(h, hipStreamCreateWithFlags(&h->stage.copy_stream, hipStreamNonBlocking));
        HIP_TRY(h, hipEventCreateWithFlags(&h->stage.copied, hipEventDisableTiming));
        for (int i = 0; i < 2; i++) HIP_TRY(h, hipEventCreateWithFlags(&h->stage.free_ev[i], hipEventDisableTiming));
    }
    // the kernels of the batch before last may still read this set: the COPIES wait for them on the device, the host
    // does not (a buffer that has to grow is freed by hipFree, which waits for the device itself)
    if (h->stage.busy[set]) HIP_TRY(h, hipStreamWaitEvent(h->stage.copy_stream, h->stage.free_ev[set], 0));
    dcols.assign(nc, n1k_col{});
    uint64_t n = batch->nrows;
    for (uint32_t c = 0; c < nc; c++) {
        const n1k_col& col = batch->cols[c];
        dcols[c] = col;
        if (col.kind == N1K_COL_DICT32) {
            HIP_TRY(h, s_codes[c].ensure(n));
            if (n) HIP_TRY(h, hipMemcpyAsync(s_codes[c].p, col.codes, n * 4, hipMemcpyHostToDevice, h->stage.copy_stream));
            dcols[c].codes = s_codes[c].p;
        } else {
            HIP_TRY(h, s_tags[c].ensure(n));
            HIP_TRY(h, s_payload[c].ensure(n));
            if (n) {
                HIP_TRY(h, hipMemcpyAsync(s_tags[c].p, col.tags, n, hipMemcpyHostToDevice, h->stage.copy_stream));
                HIP_TRY(h, hipMemcpyAsync(s_payload[c].p, col.payload, n * 8, hipMemcpyHostToDevice, h->stage.copy_stream));
            }
            dcols[c].tags = s_tags[c].p;
            dcols[c].payload = s_payload[c].p;
        }
    }
    // the caller's memory is not retained after return (cgo rule): wait for the copies — not for the compute stream
    HIP_TRY(h, hipEventRecord(h->stage.copied, h->stage.copy_stream));
    HIP_TRY(h, hipStreamWaitEvent(h->stream, h->stage.copied, 0));
    HIP_TRY(h, hipEventSynchronize(h->stage.copied));
    return N1K_OK;
}

// behind the kernels of a staged batch: its set may be overwritten once this event has passed
n1k_status staged_batch_issued(n1k_handle* h) {
    const int set = h->stage.cur;
    HIP_TRY(h, hipEventRecord(h->stage.free_ev[set], h->stream));
    h->stage.busy[set] = true;
    h->stage.cur ^= 1;
    return N1K_OK;
}

}  // namespace n1k_eng
