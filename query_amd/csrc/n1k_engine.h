// n1k_engine.h — what the translation units of the host engine share.  In this order: the match table; the options; then,
// stage by stage (engine, JSON, scan, partitioned GROUP BY, DISTINCT sets, finish, grouped tail), the struct that holds the
// stage's state beside the functions of the translation unit that runs it; the handle, which is one member per stage struct
// plus what every stage reads.  Device and pinned memory is owned by DevBuf / PinBuf (n1k_buf.h) and freed by scope exit or
// with the handle, never by name.  Internal: nothing here is part of the C ABI (include/n1k.h).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <numeric>
#include <string>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/n1k.h"
#include "n1k_buf.h"
#include "n1k_jit.h"
#include "n1k_json.h"
#include "n1k_kernels.h"
#include "n1k_arrfn.h"
#include "n1k_datefn.h"
#include "n1k_coll.h"
#include "n1k_cond.h"
#include "n1k_in.h"
#include "n1k_like.h"
#include "n1k_order.h"
#include "n1k_plan.h"
#include "n1k_rowdistinct.h"
#include "n1k_strfn.h"


using namespace n1k;

static_assert(sizeof(n1k_value) == 16, "n1k_value layout");
static_assert(sizeof(OutValue) == sizeof(n1k_value), "OutValue must alias n1k_value");
static_assert(sizeof(Program) + sizeof(ScanArgs) + sizeof(GlobalTable) + 64 <= 4096, "kernel arguments exceed 4 KiB");

namespace n1k_eng {

extern thread_local std::string g_create_error;

// device scratch of the match table's device route (n1k_matchtable.cpp), kept from one extension of the table to the next
struct MatchScratch {
    DevBuf<uint8_t> bytes;   // the block's bytes
    DevBuf<uint64_t> off;    // its n + 1 offsets
    DevBuf<uint8_t> left;    // MK_COUNT * n: the kernels' left-to-host flags, kind k at k * n
    DevBuf<uint8_t> bits;    // MK_COUNT * n: the kernels' bits where they do not go straight into the table, kind k at k * n
    DevBuf<uint8_t> progs;   // CollProg[]
    DevBuf<uint8_t> sprogs;  // StrFnProg[]
};

// the kinds of predicate that own bits of a match-table entry
enum MatchKind { MK_LIKE, MK_COLL, MK_IN, MK_STRFN, MK_COUNT };

// The match table ("The match table"): one byte per dictionary code, a predicate evaluated once per distinct
// entry, one bit per row in the scan.  The plan's compiled predicates of the four kinds, the constants of its IN lists and
// the table in device memory: built before the first launch that needs it and EXTENDED when the dictionary has grown
// (ensure_match_table), kept across n1k_reset, freed with the handle.
struct MatchTable {
    std::vector<LikePattern> patterns;  // distinct LIKE patterns: pattern p owns bit p
    std::vector<CollPred> preds;        // distinct ANY / EVERY predicates: predicate q owns bit coll_top - q
    std::vector<InList> lists;          // distinct IN lists; those that hold strings own the bits above the patterns', in order of first use
    uint32_t string_lists = 0;          // lists that hold strings
    std::vector<StrFnPred> strfns;      // distinct string-function predicates: predicate q owns the bit above the lists', in order of first use
    uint32_t strfn_first = 0;           // ... which is bit strfn_first + q (finalize_bits)
    uint32_t coll_top = kMatchBits - 1; // (the diagnostic entry points evaluate one predicate into bit 0)
    std::vector<double> in_numbers;     // the numbers of all lists, list by list (Program::in_nums)
    InTableHost in_table;               // the strings of all lists in one open-addressed table
    DevBuf<uint8_t> d_in_table;         // both device copies are made before the first launch (upload_in_constants)
    DevBuf<double> d_in_nums;
    bool in_uploaded = false;
    DevBuf<uint8_t> d_bits;             // the table (+ 4 spare bytes: the kernels that stage it in LDS copy whole words)
    size_t built_for = 0;               // dictionary codes it covers
    MatchScratch scratch;
    struct { uint64_t dev = 0, host = 0; } counts[MK_COUNT];  // entries evaluated by the kind's kernel / by its host matcher

    // plan side (n1k_matchtable.cpp): find the predicate by its text or compile and append it; the index, or -1 and err
    int add_like(const std::string& pattern, PlanError& err);
    int add_coll(const Expr* e, PlanError& err);
    int add_in(const Expr* e, PlanError& err);
    int add_strfn(const Expr* e, const Expr*& path, PlanError& err);  // (path: the leaf path the term reads)
    void finalize_bits(Program& P);  // once the condition is compiled: the bit of every predicate, into the terms that read them
    void clear_plan() {
        patterns.clear();
        preds.clear();
        lists.clear();
        strfns.clear();
        in_numbers.clear();
        string_lists = strfn_first = 0;
    }
};

// The array functions' value tables ("Array functions"; n1k_arrfn.h): per distinct term of the plan one tag byte
// and one 8-byte payload per dictionary code.  The match table's life cycle: built before the first launch that needs it
// and EXTENDED when the dictionary has grown (ensure_value_table), kept across n1k_reset, freed with the handle.
struct ArrFnTable {
    std::vector<ArrFnTerm> terms;  // distinct by their stringer text: equal text shares one table
    DevBuf<uint8_t> d_tags[kArrFnMaxTerms];
    DevBuf<uint64_t> d_payload[kArrFnMaxTerms];
    size_t built_for = 0;  // dictionary codes the tables cover
    struct {               // device scratch of the device route, kept from one extension to the next
        DevBuf<uint8_t> bytes, left, tags, progs;
        DevBuf<uint64_t> off, payload;
    } scratch;
    uint64_t dev = 0, host = 0;  // array entries evaluated by the kernel / by the host evaluator (n1k_arrfn_stats)
    int add(const Expr* e, PlanError& err);  // find the term by its text or compile and append it; the index, or -1 and err
    void clear_plan() {
        terms.clear();
        built_for = 0;
    }
};

// str_to_millis / date_part_str: their value tables ("Date functions"; n1k_datefn.h), ArrFnTable's sibling with
// STRING as the expected tag and the same life cycle: built before the first launch that needs them, EXTENDED when the
// dictionary has grown (ensure_datestr_table), kept across n1k_reset, freed with the handle.
struct DateStrTable {
    std::vector<DateStrTerm> terms;  // distinct by their stringer text: equal text shares one table
    DevBuf<uint8_t> d_tags[kDateStrMaxTerms];
    DevBuf<uint64_t> d_payload[kDateStrMaxTerms];
    size_t built_for = 0;  // dictionary codes the tables cover
    struct {               // device scratch of the device route, kept from one extension to the next
        DevBuf<uint8_t> bytes, left, tags;
        DevBuf<uint64_t> off, payload;
    } scratch;
    uint64_t dev = 0, host = 0;  // entries evaluated by the kernel / by the host evaluator (n1k_datefn_stats)
    // find the term by its text or compile and append it; the index, -1 and err, or -2: the part is the constant MISSING
    int add(const Expr* e, PlanError& err);
    void clear_plan() {
        terms.clear();
        built_for = 0;
    }
};

// LDS the kernels of a bounded shape carry for the staged match table: kMatchLdsBytes when some term reads the table (n1k_spec.h:
// present by shape, whatever the table's size), else none
inline uint32_t match_lds_bytes(const FastArgs& F) {
    for (uint32_t t = 0; t < F.nterms; t++)
        if (term_is_table_bit(F.terms[t].op)) return kMatchLdsBytes;
    return 0;
}

inline uint64_t next_pow2(uint64_t x) {
    uint64_t p = 1;
    while (p < x) p <<= 1;
    return p;
}
inline uint32_t ceil_log2(uint64_t x) {
    uint32_t b = 0;
    while ((1ull << b) < x) b++;
    return b;
}

n1k_status fail(n1k_handle* h, n1k_status st, const char* fmt, ...);

#define HIP_TRY(h, expr)                                                                                  \
    do {                                                                                                  \
        hipError_t _e = (expr);                                                                           \
        if (_e != hipSuccess)                                                                             \
            return fail(h, _e == hipErrorOutOfMemory ? N1K_OOM : N1K_DEVICE_ERROR, "%s failed: %s", #expr, \
                        hipGetErrorString(_e));                                                           \
    } while (0)

// the same for a callee that has reported its failure itself
#define ST_TRY(expr) do { n1k_status _st = (expr); if (_st != N1K_OK) return _st; } while (0)

constexpr uint32_t kPinScratch = 16;
constexpr uint64_t kWordSubs = 256ull * kRecSubs;  // sub-regions of a DISTINCT aggregate's member words

// ---------------------------------------------------------------------------------------------------------------------------
// The state of a handle, stage by stage: one plain struct per stage, followed by the functions of the translation unit that
// runs the stage.  n1k_handle (below them) holds one of each, and flat only what every stage reads.  Every device buffer is a
// DevBuf and every pinned one a PinBuf: they free themselves with the handle, nothing is released by name.

// n1k_set_option, in its order (device, stream: on the handle)
struct Options {
    int64_t agg_mode = N1K_MODE_AUTO;
    uint64_t max_groups = 1ull << 26;
    uint32_t grid_blocks = 0;
    uint32_t fast = 1, spec = 1, wide = 1;
    uint32_t fuse_arith = 1;   // arithmetic nodes evaluated in registers by the run-time-built scan (no derived columns)
    uint32_t lean_topk = 1;    // ORDER BY ... LIMIT over a kept region: order values first, rows for the candidates only
    uint32_t topk_sample = 1;  // ORDER BY ... LIMIT: threshold of the device top-k filter from a sample first (0: always the exact radix select)
    uint32_t distinct_fill_pct = 25;     // a final bin's expected words, in % of the LDS set's slots (tuning)
    uint32_t dedupe_unroll = 0;          // words per thread and chunk of the de-duplication kernel at 1024 threads: 2 (0) or 4 (tuning)
    uint32_t agg_spec = 1;      // agg_bins16_kernel: the plan's one aggregate fixed at compile time (0: the generic kernel, A/B)
    uint32_t merge_chunks = 0;  // merge_slabs_kernel: block rows (0 = from the grid)
    uint32_t inject_failure = 0;  // tests: the exchange pretends that its site 1 (buffers) / 2 (partition, export) / 3 (receiving part) failed, once
    uint32_t part_block = 256; // workgroup size of the run-time-built partition kernel (256 | 512; measured 0.43 vs 0.58 ms per 100 M rows)
    uint32_t part_subs = 1;    // row exchange: sub-regions per destination with their own counters (0: one dense run)
    uint32_t part_per_cu = 0;  // workgroups per CU of the run-time-built partition kernel (0 = 2)
    uint32_t jit = 1;                 // 0 off, 1 auto (large batches only), 2 always
    uint64_t jit_min_rows = 4u << 20;
    uint32_t distinct_words = 1;      // 0: every pair takes the (key, value, class) log and the global sets
    uint32_t distinct_set_slots = 8192;  // LDS set size of the de-duplication kernel (power of two; 64 KB: two workgroups per CU)
    uint32_t records = 1;  // 0: always the three-array records of the interpreter front end (ablation, tests)
    uint32_t rec_slots = 0, rec_bins = 0, rec_slices = 0, rec_scan_per_cu = 0, rec_block = 0, rec_unroll = 0;  // tuning (0 = chosen from the data)
    uint64_t region_cap = 0;           // forced capacity of a hash region (tests: overflow into the plain log), 0 = from the rows
    uint32_t dedupe_block = 1025;      // workgroup size of the de-duplication kernel, +1: probe word by word (tuning)
    uint32_t json_device = 1;  // n1k_push_json through the device extractor (n1k_jsondev.hip)
    uint32_t json_device_left_pct = 12;  // more documents than this left to the host: the host path takes the whole batch
    uint64_t json_device_min_docs = 4096;
    uint32_t json_threads = 0;  // 0 = hardware concurrency (at most 16)
    // (measured, 100 M rows, GROUP BY cat, region_id: 6 400 groups 11.3 ms scan kernels vs 6.6 ms partitioned; 64 000 groups
    //  14.4 vs 9.8 ms: the LDS hash stage holds about a thousand groups, beyond that rows turn into global atomics)
    uint64_t partition_min_rows = 8u << 20, partition_probe_rows = 512u << 10, partition_min_groups = 4096;
    uint32_t partition_sticky = 1;  // (Partitioned::sticky)
    int32_t partition_levels = -1;
    uint64_t topk_min_groups = 65536;  // device top-k filter from this many groups on
    int32_t distinct_levels = -1;        // partition passes before the LDS sets: -1 = by log size, 0..2 forced (tests)
    uint64_t wide_values = 1u << 20;  // capacity of the wide key value tables (distinct big ints / floats)
    uint32_t slabs = 1;
    uint32_t block = 0, rows_per_lane = 4;
    uint32_t lds_bytes = 64 * 1024;   // HASH mode: LDS table bytes per workgroup
    uint32_t rep_row = 0;
    uint64_t rowdistinct_slots = 0;  // DISTINCT over rows: forced capacity of the table, any value >= 1, not rounded (0 = from the survivors; tests)
    uint32_t rowdistinct_lds_slots = 0;  // ... size of the LDS set ahead of the table; 0 = no pre-filter, the default: measured, it costs more than it saves
};

// ---- n1k_engine.cpp: plan binding, device and table management
// The words of GroupTable::counters, on the device and in their host copies.  Device code is handed pointers to single words
// and fixes only the distance from the error flags to the peer status (kPeerStatusFromErr).
enum Counter : uint32_t {
    CTR_ROWS_SELECTED = 0,
    CTR_GROUPS = 1,              // groups in the table
    CTR_OUT_COUNT = 2,           // FinalGroup's output position (Results::out_count_dirty)
    CTR_FILTER_TOTAL = 3,        // survivors of a Filter-only batch
    CTR_REHASH_SCRATCH = 4,
    CTR_DISTINCT_REGION_WORDS = 5,  // K6: set-table words the layout kernel asks for
    CTR_TAIL_TICKET = 6,         // fold_rows_kernel: workgroups done (the last one publishes and zeroes the counters, this one too)
    CTR_PAIR_LOG_CURSORS = 8,    // + log_index (kMaxDistinct words): the (key, value, class) pair logs
    CTR_ERR_FLAGS = 12,          // ERR_* (n1k_types.h), low 32 bits: GroupTable::errp
    CTR_WIDE_VALUES = 13,        // distinct wide key values met so far (Program::wide_count)
    CTR_WORD_LOG_CURSORS = 16,   // + log_index (kMaxDistinct words): the COUNT(DISTINCT) member-word logs
    // two 32-bit overflow flags of an optimistic path ([0] a hash region / an LDS set, [1] a bin).  Two users: the records front
    // end of the partitioned GROUP BY (run_group_records) and the optimistic COUNT(DISTINCT) sets (distinct_regions_finish).
    // They never meet in one query: partition_eligible refuses plans with DISTINCT aggregates.
    CTR_OPTIMISTIC_OVERFLOW = 20,
    CTR_PART_RECORDS = 21,       // records of the partitioned path
    CTR_SINGLETONS = 22,         // ... its singleton partial groups
    CTR_EXACT_OVERFLOW = 24,     // COUNT(DISTINCT) exact path: an LDS set overflowed
    CTR_SAVED_ROWS_SELECTED = 25,  // CTR_ROWS_SELECTED before the optimistic records path, to undo it
    CTR_REGION_GROUPS = 26,      // ... its region's group count, copied beside the others for the host
    CTR_PEER_STATUS = 27,        // the n1k_status a peer's verdict carried (ERR_PEER_FAILED)
    CTR_ROWDISTINCT_COUNT = 28,  // DISTINCT over rows: the representatives
    CTR_ROWDISTINCT_REACHED = 29 // ... and the rows that reached the global table (the word behind the count: cleared together)
};
static_assert(CTR_ERR_FLAGS + kPeerStatusFromErr == CTR_PEER_STATUS, "the verdict kernel writes the peer status this far behind the flags");
static_assert(CTR_ROWDISTINCT_REACHED < kCounters && CTR_ROWDISTINCT_REACHED == CTR_ROWDISTINCT_COUNT + 1, "every counter word lies inside the buffer (CTR_ROWDISTINCT_REACHED is the last)");
static_assert(CTR_ROWS_SELECTED == 0 && CTR_GROUPS == 1 && CTR_OUT_COUNT == 2 && CTR_TAIL_TICKET > CTR_DISTINCT_REGION_WORDS && CTR_TAIL_TICKET < CTR_PAIR_LOG_CURSORS,
              "the query's last kernels (finalize_small_kernel, fold_rows_kernel) write words [0], [1] and [2] by number");
static_assert(CTR_PAIR_LOG_CURSORS + kMaxDistinct <= CTR_ERR_FLAGS && CTR_WORD_LOG_CURSORS + kMaxDistinct <= CTR_OPTIMISTIC_OVERFLOW, "cursor words overlap their neighbours");

// The group table and the device words every stage reports through.
struct GroupTable {
    GlobalTable table{};
    DevBuf<uint64_t> keys, acc, rep;        // (n1k_engine.cpp alone: alloc_table, grow_table)
    DevBuf<uint64_t> slabs;                 // (n1k_scan.cpp)
    DevBuf<unsigned long long> block_sel;   // (n1k_scan.cpp)
    uint32_t* errp = nullptr;  // lives inside counters (CTR_ERR_FLAGS) so one copy reads counters and flags
    DevBuf<unsigned long long> counters;  // kCounters words, named by Counter (above)
    DevBuf<uint64_t> wide_int, wide_flt;  // the wide key value tables, Options::wide_values entries (n1k_engine.cpp alone)
    uint64_t merged_bound = 0;  // groups that may have arrived through merges (bounds the table like rows do)
    // One-call executions: the slabs of the batch's only scan launch, left unmerged by launch_chunk for n1k_finish to fold
    // straight into result rows (fold_rows_kernel; slabs_to_rows is the one predicate of both).  The program is the handle's
    // (no DISTINCT on this path).  reset_handle forgets them.
    struct PendingSlabs {
        bool clean_at_push = false;  // the device was as n1k_reset leaves it when the push began, and nothing before the scan touched it
        uint32_t grid = 0;           // > 0: slabs of this many workgroups are pending
        FastArgs F{};                // ... the scan's arguments: slabs, survivor counts, slot -> key, error flags
    } pending;
};
uint32_t intern(n1k_handle* h, const std::string& s);
uint32_t lookup_code(const n1k_handle* h, const char* s);
bool to_operand(n1k_handle* h, const Expr* e, Operand& o, PlanError& err);
bool compile_plan(n1k_handle* h, PlanError& err);
n1k_status ensure_device(n1k_handle* h);
n1k_status reset_handle(n1k_handle* h, bool clear_stop);  // n1k_reset (clear_stop: and forget an earlier n1k_stop, as reopen() does)
n1k_status ensure_rank(n1k_handle* h);
n1k_status fix_layout(n1k_handle* h, const n1k_batch* b);
n1k_status ensure_table(n1k_handle* h, uint64_t incoming_rows);
n1k_status ensure_table_groups(n1k_handle* h, uint64_t groups);
hipEvent_t get_event(n1k_handle* h);
n1k_status ensure_pinned_counters(n1k_handle* h);
void drain_events(n1k_handle* h);
n1k_status validate_batch(n1k_handle* h, const n1k_batch* b);
uint64_t batch_bytes_per_row(const n1k_handle* h);
void default_value(const AggDef& d, n1k_value& v, n1k_partial& p);

// Host-side timing and the statistics of a query.
struct Timing {
    // host-side timing of the one-call path (N1K_HOST_TRACE=1: printed at destroy): [0] reset [1] push (launches) [2] finish up to
    // the wait [3] the wait [4] finish after the wait, in microseconds, and the number of calls
    double host_us[6] = {0, 0, 0, 0, 0, 0};
    hipEvent_t ev_q0 = nullptr, ev_q1 = nullptr;  // the whole query on the stream: recorded by n1k_reset / before n1k_finish's last wait
    bool q0_recorded = false, q1_recorded = false;
    n1k_stats stats{};
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
    std::vector<hipEvent_t> event_pool;
};

// raw documents -> columns
struct Json {
    // n1k_extract_json (n1k_engine.cpp alone): leaf paths as field chains, the extracted batch
    std::vector<JsonPath> paths;
    int paths_state = 0;  // 0 not parsed, 1 ok, -1 some path is not a field chain
    std::vector<std::vector<uint8_t>> tags;
    std::vector<std::vector<uint64_t>> payload;
    std::vector<n1k_col> cols;
    // n1k_push_json through the device extractor (n1k_jsonpush.cpp alone): the batch's bytes, offsets, status, columns, string table
    DevBuf<char> d_bytes;
    DevBuf<uint64_t> d_offsets, d_new_first, d_patch_docs, d_patch_pay, d_tab;
    DevBuf<uint8_t> d_status, d_patch_tags;
    DevBuf<uint32_t> d_new_list, d_code_of, d_codes;
    std::vector<DevBuf<uint8_t>> d_tags;
    std::vector<DevBuf<uint64_t>> d_payload;
    std::vector<uint8_t> host_status;
};
// n1k_jsonpush.cpp: n1k_push_json through the device extractor (done = false: the host path takes the batch)
n1k_status push_json_device(n1k_handle* h, uint64_t ndocs, const uint64_t* offsets, const char* bytes, bool* done);

// n1k_matchtable.cpp: the match table of the LIKE, ANY / EVERY, IN and string-function terms, built and extended before the launches that read it
n1k_status ensure_match_table(n1k_handle* h);
// n1k_arrfn.cpp: the value tables of the array-function terms, built and extended before the lookups that read them
n1k_status ensure_value_table(n1k_handle* h);
// n1k_datefn.cpp: the value tables of the str_to_millis / date_part_str terms, likewise
n1k_status ensure_datestr_table(n1k_handle* h);

// ---- n1k_scan.cpp: one batch through Filter + InitialGroup (kernel choice), Filter-only batches, staging of host batches
// Staging for host batches (n1k_scan.cpp alone).
// Two sets, used in turn: the H2D copies of batch k + 1 run on their own stream while the kernels of batch k still read
// the other set; n1k_push_batch waits for its copies only (the caller's memory is free on return), never for kernels.
struct Staging {
    std::vector<DevBuf<uint8_t>> tags[2];
    std::vector<DevBuf<uint64_t>> payload[2];
    std::vector<DevBuf<uint32_t>> codes[2];
    hipStream_t copy_stream = nullptr;
    hipEvent_t free_ev[2] = {nullptr, nullptr};  // recorded on the compute stream behind the kernels that read the set
    bool busy[2] = {false, false};
    hipEvent_t copied = nullptr;
    int cur = 0;
};
// The Filter-only path: run_filter_batch fills them, n1k_finish reads `selected`.
// n1k_filter_device_batch (n1k_select.cpp) leaves its selection in `sel32` instead: 32-bit batch-local ordinals that stay on the
// device, for n1k_selected_to_host32 and n1k_gather_selected.  Both paths use tile_off, one after the other on the stream.
struct FilterOnly {
    DevBuf<uint64_t> tile_off, sel;
    std::vector<uint64_t> selected;
    DevBuf<uint32_t> sel32;
    bool has_sel32 = false;               // a selection exists: until the next n1k_filter_device_batch / n1k_reset
    uint64_t sel32_count = 0, sel32_rows = 0;  // its survivors; the rows of the batch it was taken from
    const uint32_t* sel32_out = nullptr;  // where the selection lies: sel32, or — a plan with Order / Offset / Limit — what
                                          // order_selection left (n1k_order.cpp); sel32_count is then the cut count
};

// ---- n1k_order.cpp: ORDER BY / OFFSET / LIMIT over the rows of a Filter-only plan, sorted on the device (n1k_order.hip)
struct RowOrder {
    DevBuf<uint64_t> key[kOrdHists];     // per term (and for the selection position, the select route): the survivors' keys
    DevBuf<uint16_t> res[kOrdMaxTerms];  // ... and residuals
    DevBuf<uint64_t> kbuf[2];            // the passes' keys, ping-pong
    DevBuf<uint32_t> vbuf[2];            // ... and positions
    DevBuf<uint32_t> hist, tile_hist;    // [term][digit][256]; 256 x tiles
    DevBuf<uint32_t> cand;               // the select route: candidate positions (+ the sampled route's segment lists)
    DevBuf<char> state;                  // ... and the select's state
    DevBuf<uint32_t> rows_out;           // the ordered, cut selection
    PinBuf<uint32_t> pin_hist;           // host copy of the histograms, then the error flags and the candidate count
    uint32_t passes = 0;                 // digit passes the last ordering launched (diagnostics: tools/exp_order.py)
};
// the ascending selection `sel` of `total` survivors (the Filter's, or the representatives DISTINCT left of it) -> ordered and
// cut as the plan says; *out_rows (null when *out_count is 0) is what n1k_selection.rows returns
n1k_status order_selection(n1k_handle* h, const uint32_t* sel, uint64_t total, const uint32_t** out_rows, uint64_t* out_count);
// the multi-batch calls on a plan whose rows are de-duplicated, ordered or cut: N1K_UNSUPPORTED
n1k_status refuse_ordered_rows(n1k_handle* h, const char* call);

// ---- n1k_rowdistinct.cpp: SELECT DISTINCT over the rows of a Filter-only plan, de-duplicated on the device (n1k_rowdistinct.hip)
struct RowDistinct {
    DevBuf<uint32_t> table;       // the open-addressed table of ordinals, cleared every call
    DevBuf<uint32_t> slot_of;     // per survivor: the slot of its key, then whether it is the representative
    DevBuf<uint32_t> tile_count;  // the tiles' representatives and their scan
    DevBuf<uint32_t> rows_out;    // the representatives, ascending
    uint64_t stats[4] = {0, 0, 0, 0};  // n1k_rowdistinct_stats: survivors, distinct rows, table slots, rows that reached the table
};
// the ascending selection `sel` (null: the identity, a plan without Filter) of `total` survivors -> *out_rows: per distinct row
// key of the plan's result terms the survivor with the smallest ordinal, ascending (null when there is none), *out_count of them
n1k_status distinct_selection(n1k_handle* h, const uint32_t* sel, uint64_t total, const uint32_t** out_rows, uint64_t* out_count);
// the stage's options ("rowdistinct_slots", "rowdistinct_lds_slots"; checked by tests/test_gpu_distinct_rows.py): false when
// `name` is none of them
bool rowdistinct_option(n1k_handle* h, const std::string& name, int64_t value);
bool filter_stream_fast(const n1k_handle* h);  // the condition and the bound columns take filter_stream_kernel's FAST variant
uint32_t filter_stream_grid(const n1k_handle* h, uint64_t ntiles, bool fast);
bool build_fast_args(n1k_handle* h, uint32_t max_slots, FastArgs& F, bool fuse = false, bool partition_only = false);
// Columns (DevCol or n1k_col) from row `off` on: an array a column does not have stays null.
template <class Col> inline void advance_cols(Col* cols, uint32_t n, uint64_t off) {
    for (uint32_t c = 0; c < n; c++) {
        if (cols[c].tags) cols[c].tags += off;
        if (cols[c].payload) cols[c].payload += off;
        if (cols[c].codes) cols[c].codes += off;
    }
}
// Every array aligned for the WIDE form of the plan-specialised kernels (two adjacent rows per lane and load)?
template <class Col> inline bool cols_wide_aligned(const Col* cols, uint32_t n) {
    for (uint32_t c = 0; c < n; c++)
        if ((uintptr_t)cols[c].tags % 2 || (uintptr_t)cols[c].payload % 16 || (uintptr_t)cols[c].codes % 8) return false;
    return true;
}
// The plan-specialised kernel of a plan shape, for one of its three uses: the scan (run_group_batch), the records front end
// of the partitioned GROUP BY (run_group_records), the hash partition of the row exchange (run_partition).
enum class ShapeUse { Scan, Records, Partition };
struct ShapeKernel {
    const SpecEntry* spec = nullptr;  // instantiated ahead of time (n1k_spec.h), or
    const JitKernel* jit = nullptr;   // the same template built at run time (n1k_jit.h)
    uint32_t stat = 0;                // stats.spec_kernel: 0 none, 1 prebuilt, 2 built at run time, 3 ... with the arithmetic nodes in registers
    explicit operator bool() const { return spec || jit; }
};
// table_bytes (Scan): the workgroup's LDS table as the kernel would lay it out
ShapeKernel shape_kernel(n1k_handle* h, const FastArgs& F, ShapeUse use, uint64_t nrows, size_t table_bytes = 0);
bool shape_compiles(const n1k_handle* h, const FastArgs& F, ShapeUse use, std::string* log);  // n1k_jit_check: compiles only, no device
n1k_status run_group_batch(n1k_handle* h, const n1k_batch* b);
n1k_status run_filter_batch(n1k_handle* h, const n1k_batch* b);
n1k_status bind_columns(n1k_handle* h, const n1k_batch* b, bool defer = false);
n1k_status materialize_derived(n1k_handle* h, const n1k_batch* b);
n1k_status push_device(n1k_handle* h, const n1k_batch* b);
n1k_status stage_host_batch(n1k_handle* h, const n1k_batch* batch, std::vector<n1k_col>& dcols);
n1k_status staged_batch_issued(n1k_handle* h);

// ---- n1k_partitioned.cpp: GROUP BY with many groups (records -> partition passes -> per-bin LDS tables)
struct Partitioned {
    // record arrays (ping-pong per partition pass)
    DevBuf<uint64_t> rec_key[3], rec_pay[3][kRecOperands];
    DevBuf<uint8_t> rec_tag[3][kRecOperands];
    DevBuf<uint64_t> emit;  // the bins' partial groups before they are merged into the table
    // the same path with the plan-specialised front end: 16-byte records (Rec16) written straight into 256 hash regions
    // by the scan (projection + first partition pass in one kernel), then into bins of fixed capacity
    DevBuf<uint64_t> rregion, rbins;
    DevBuf<unsigned long long> rcursor;
    // ... or instead of it: while the table is empty and their keys are unique, the region IS the set of groups;
    // n1k_finish finalizes it directly, anything else that needs the table merges it first (flush_pending)
    struct { uint64_t count = 0, cap = 0; } pending;
    // A handle that has just run a batch of about this size through the partitioned path (groups estimated from a probe of its
    // first rows) takes the next execution's batch the same way without probing again (a prepared statement executed again over
    // the same keyspace): the path checks itself (fixed-capacity regions and bins raise flags: exact path), and a batch that
    // would have been better off on the scan kernels is only slower, never wrong.  Forgotten when the path falls back.
    struct { bool valid = false; uint64_t rows = 0, groups_est = 0; } sticky;  // (n1k_scan.cpp; Options::partition_sticky)
    uint64_t groups_seen = 0;
};
struct PartitionPlan {
    Operand src[kRecOperands];
    uint32_t nsrc = 0;
    uint32_t agg_src[kMaxAggs];
};
bool partition_eligible(n1k_handle* h, PartitionPlan& pp);
bool small_key_domain(const n1k_handle* h);
n1k_status flush_pending(n1k_handle* h);
n1k_status run_group_partitioned(n1k_handle* h, const n1k_batch* b, const PartitionPlan& pp, uint64_t groups_est, bool may_keep_region);
n1k_status run_group_records(n1k_handle* h, const n1k_batch* b, const PartitionPlan& pp, uint64_t groups_est, bool may_keep_region, bool* done);

// ---- n1k_distinct.cpp: the logs and hash regions the scan fills for the DISTINCT aggregates, and their sets at finish
struct Distinct {
    // the (key, value, class) pair logs and the global sets n1k_finish builds of them
    DevBuf<uint64_t> log_key[kMaxDistinct], log_val[kMaxDistinct], regions, set_table;
    DevBuf<uint8_t> log_cls[kMaxDistinct];
    // COUNT(DISTINCT) member words (ScanArgs::log_word) and the scratch of their partition / de-duplication at finish
    DevBuf<uint64_t> log_word[kMaxDistinct], part[2], seg[3], wtable;
    DevBuf<unsigned long long> hist, cursor, dcounts, word_hist;
    // hash regions of the specialised scan's COUNT(DISTINCT) (WordLogArgs): per aggregate 256 regions x kRecSubs sub-regions
    // (kWordSubs in all) of wregion_cap words each
    DevBuf<uint64_t> wregion[kMaxDistinct], woff, wgather;
    DevBuf<unsigned long long> wcursor;  // kMaxDistinct x kWordSubs counters, kCursorStride apart
    uint64_t wregion_cap = 0;
    bool wregion_used = false;             // some batch of this query went through the regions
    uint32_t nw_key_bits = 0, nw_val_bits = 0;
    bool words[kMaxDistinct] = {false, false, false, false};
    uint32_t path = 0;  // how the last finish built the sets: bit 0 global pair sets, bit 1 LDS word sets, bit 2 global word set
    uint64_t log_capacity = 0;
};
// before a batch of nrows rows is scanned: room for its pairs in the logs (A's log fields) / for its member words in the hash
// regions of the plan-specialised scan (L; P: the program that scan runs on)
n1k_status distinct_grow_logs(n1k_handle* h, uint64_t nrows, ScanArgs& A);
n1k_status distinct_grow_regions(n1k_handle* h, const Program& P, uint64_t nrows, const ScanArgs& A, uint32_t dcache_slots, WordLogArgs& L);
n1k_status distinct_words_finish(n1k_handle* h, const AggSpec& ag, uint64_t nwords, bool hist_counted = true, const uint64_t* log = nullptr);
n1k_status distinct_regions_finish(n1k_handle* h, const AggSpec& ag, uint64_t nover, bool force_exact, bool* deferred);

// ---- n1k_finish.cpp: FinalGroup and the result
// ORDER BY ... LIMIT on the device (n1k_finish.cpp alone): order images, candidate indices, select state, compacted records
struct TopK {
    DevBuf<uint64_t> images;
    DevBuf<uint32_t> cand;
    DevBuf<char> state, out2;
};
struct Results {
    std::vector<n1k_value> keys, aggs;
    std::vector<n1k_partial> parts;
    std::vector<uint64_t> rep;
    DevBuf<char> d_out;            // finalize output: [keys][aggs][partials][rep rows], copied to the host at once
    std::vector<char> out_host;
    std::vector<char> export_blob;  // (n1k_exchange.cpp: n1k_export_groups)
    bool out_count_dirty = true;  // the finalize position counter holds a previous finish's count
    PinBuf<char> pin_out;  // pinned host copy of a speculative FinalGroup (n1k_finish)
    PinBuf<unsigned long long> pin_counters;  // pinned host copy of the device counters (one D2H per decision point): kCounters words,
                                              // then kPinScratch words for the small reads of n1k_finish (candidate count, flags)
    PinBuf<char> pin_rows;                    // pinned landing place of n1k_finish's sized output copy (pageable D2H copies are staged
                                              //  by the runtime: ~ 35 us per copy + wait where the pinned one takes ~ 10)
};

// ---- n1k_tail.cpp: what follows FinalGroup (HAVING, projection, ORDER BY / OFFSET / LIMIT, ARRAY_AGG assembly)
struct Tail {
    // InitialProject over the final groups: an inner operator that only carries the derived columns of the terms'
    // expressions (its input columns are group keys / aggregates, like HAVING's)
    n1k_handle* project = nullptr;
    std::vector<int> project_cols;        // per inner column: key index k (>= 0) or -(aggregate index) - 1
    std::vector<Operand> project_ops;     // one per result term, in the inner operator's column space
    std::vector<n1k_value> r_proj;        // [ngroups][nterms]
    // HAVING: an inner Filter-only operator over the final groups (its columns are group keys / aggregates)
    n1k_handle* having = nullptr;
    std::vector<int> having_cols;        // per inner column: key index k (>= 0) or -(aggregate index) - 1
    std::vector<uint32_t> having_codes;  // dictionary code of this handle -> code of the inner handle (lazy)
};
n1k_status build_projection(n1k_handle* h);
n1k_status having_groups(n1k_handle* h, uint64_t& ng);
n1k_status project_groups(n1k_handle* h, uint64_t ng);
n1k_status order_groups(n1k_handle* h, uint64_t& ng);
n1k_status array_agg_groups(n1k_handle* h, uint64_t ng, const unsigned long long* counters);
// A scan launch of g workgroups with slabs of F.lds_slots slots may leave them unmerged, and n1k_finish turns them into result
// rows without the table: the one predicate of launch_chunk and read_counters.  only_chunk: the launch is the
// batch's only one; whole: it covers every row of it (no odd last row, whose scalar launch merges into the table).
bool slabs_to_rows(const n1k_handle* h, const FastArgs& F, uint32_t g, bool only_chunk, bool whole);
// the ng groups of h->res (and the projection of h->tail) into the caller's n1k_result; partials only where FinalGroup made them
void publish_result(n1k_handle* h, uint64_t ng, bool partials, n1k_result* out);

}  // namespace n1k_eng

using namespace n1k_eng;

// What every stage reads lies flat; the rest is one member per stage struct above.  Members are destroyed in reverse order
// of declaration, after n1k_destroy has waited for the stream: no buffer outlives work that uses it.
struct n1k_handle {
    ParsedPlan plan;
    std::string last_error;
    std::atomic<int> stop_flag{0};
    Options opt;
    bool failure_global = false;  // the last failure reported on this handle was learnt from (or told through) the verdict words of an
                                  // exchange: every rank's step fails alike, nobody enters the gather (n1k_failure_is_global)
    // One-call executions (n1k_run_device_batch): the query's last kernel (finalize_small_kernel) leaves table and counters as
    // n1k_reset would, so the next execution starts with its scan — device_clean says that the device state is what a reset
    // produces (any push / merge / partition clears it), clear_on_finish asks n1k_finish for that last kernel
    bool device_clean = false, clear_on_finish = false;
    std::string jit_log;
    int device = -1;
    bool device_ready = false;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int num_cus = 256;

    // dictionary (all STRING/ARRAY/OBJECT payloads are codes into it)
    std::vector<std::string> dict;
    std::unordered_map<std::string, uint32_t> dict_index;
    bool need_rank = false;
    size_t rank_built_for = (size_t)-1;
    DevBuf<uint32_t> d_rank;

    MatchTable match;  // LIKE, ANY / EVERY, IN, string functions: the plan's predicates over dictionary entries and their table
    ArrFnTable arrfn;  // array_length ... array_position: the plan's terms over dictionary entries and their value tables
    DateStrTable datestr;  // str_to_millis / date_part_str: the plan's terms over dictionary strings and their value tables

    // compiled program (column pointers are patched per batch)
    Program prog{};
    bool layout_fixed = false;
    uint32_t col_kinds[kMaxCols]{};
    std::vector<std::string> agg_names;
    bool has_distinct = false, has_minmax = false, has_array_agg = false;
    uint32_t n_distinct = 0;
    // arithmetic operands -> derived columns (input columns first, then one per arithmetic node)
    struct Derived { uint32_t op, nops; Operand ops[4]; uint32_t node; };  // node: op AR_COND, the node's index in cond_nodes; op AR_ARRFN, the term's in arrfn.terms; op AR_DATESTR, the term's in datestr.terms
    std::vector<Derived> derived;
    // CASE and the conditional functions (n1k_cond.h): the nodes' programs, in device memory once their string constants have
    // their codes (materialize_derived) and until the plan is compiled again
    std::vector<CondNode> cond_nodes;
    DevBuf<CondNode> d_cond;
    bool cond_uploaded = false;
    uint32_t cond_depth = 0;  // (compile time: inside how many conditional nodes to_operand is)
    std::vector<std::string> const_strings;  // string constants of the plan, interned lazily (see to_operand)
    std::vector<DevBuf<uint8_t>> dv_tags;
    std::vector<DevBuf<uint64_t>> dv_payload;
    bool derived_ready = true;     // the derived columns of the batch being pushed are materialised (or there are none)

    // the batch being pushed
    uint64_t row_base = 0;
    const unsigned long long* push_nrows_dev = nullptr;  // the batch being pushed holds min(nrows, *this) rows (n1k_exchange_rows)
    // the batch being pushed is segmented (a row region received from another GPU: kRowSubs sub-regions of push_seg_rows rows
    // capacity, their row counts on the device kCursorStride words apart)
    const unsigned long long* push_seg_counts = nullptr;
    uint32_t push_nseg = 0;
    uint64_t push_seg_rows = 0;

    GroupTable groups;
    Distinct distinct;
    Partitioned part;
    TopK topk;
    Tail tail;
    Json json;
    Staging stage;
    FilterOnly filter;
    RowDistinct rowdistinct;
    RowOrder order;
    Results res;
    Timing timing;
};

namespace n1k_eng {

// No C++ exception leaves the library ("no C++ exceptions or abort() across the ABI"; a Go caller cannot
// unwind through cgo): allocation failures of the host containers become N1K_OOM, anything else N1K_DEVICE_ERROR.
template <class F>
n1k_status guarded(const n1k_handle* ch, F&& f) noexcept {
    n1k_handle* h = const_cast<n1k_handle*>(ch);
    try {
        return f();
    } catch (const std::bad_alloc&) {
        try { if (h) h->last_error = "out of host memory"; else g_create_error = "out of host memory"; } catch (...) {}
        return N1K_OOM;
    } catch (const std::exception& e) {
        try { if (h) h->last_error = std::string("internal error: ") + e.what(); else g_create_error = e.what(); } catch (...) {}
        return N1K_DEVICE_ERROR;
    } catch (...) {
        return N1K_DEVICE_ERROR;
    }
}

}  // namespace n1k_eng

