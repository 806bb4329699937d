// n1k_kernels.h — launch interface between the host engine and n1k_kernels.hip
#pragma once
#include <hip/hip_runtime.h>
#include <vector>
#include "n1k_types.h"
#include "n1k_cond.h"

namespace n1k {

constexpr int kFilterStreamTile = 8192;  // rows per tile of the one-pass Filter-only kernel (4 passes of 256 threads x 8 rows)
constexpr uint32_t kFinalizeSmallMax = 8192;  // table slots up to which FinalGroup is the query's one last kernel (finalize_small_kernel, fold_rows_kernel)

struct OutValue {  // same 16-byte layout as n1k_value
    uint64_t tag;  // low byte = tag (little endian), rest zero
    uint64_t payload;
};

struct OutPartial {
    int64_t count;
    int64_t isum;
    double fsum;
    uint32_t flags;  // bit0 int_exact, bit1 has_float
    uint32_t ext_tag;
    uint64_t ext_payload;
    int64_t distinct;
};

struct SynthArgs {
    uint64_t seed, first_row, nrows, total_rows;
    uint32_t k_cat, pad;
    const double* cat_cdf;
    uint32_t* cat_codes;
    uint8_t* price_tags;
    uint64_t* price_payload;
    uint8_t* user_tags;
    uint64_t* user_payload;
    uint8_t* region_tags;
    uint64_t* region_payload;
};

hipError_t launch_init_table(const Program& P, const GlobalTable& G, uint64_t first, uint64_t count,
                             unsigned long long* counters, hipStream_t st);
hipError_t launch_restamp_ranks(const Program& P, const GlobalTable& G, hipStream_t st);
hipError_t launch_rehash(const Program& P, const GlobalTable& oldt, const GlobalTable& newt, uint32_t* err_flags,
                         unsigned long long* ngroups_scratch, hipStream_t st);
hipError_t launch_scan_group(const Program& P, const ScanArgs& A, const GlobalTable& G, unsigned long long* ngroups,
                             uint32_t grid, uint32_t block, uint32_t rows_per_lane, bool direct, hipStream_t st);
hipError_t launch_scan_fast(const Program& P, const FastArgs& F, const GlobalTable& G, unsigned long long* ngroups,
                            uint32_t grid, uint32_t block, uint32_t rows_per_lane, hipStream_t st);
hipError_t launch_merge_slabs(const Program& P, const FastArgs& F, const GlobalTable& G, uint32_t nblocks,
                              unsigned long long* ngroups, hipStream_t st, uint32_t ychunks_opt = 0);
// ORDER BY ... LIMIT over the finalised groups: order images of the first sort term, radix select of the keep-th image,
// candidate indices (image <= threshold) and compaction of their records
// high-cardinality GROUP BY: rows -> records (key + operands), [radix passes], per-bin LDS aggregation
hipError_t launch_finalize_region(const Program& P, const uint64_t* region, uint64_t cap, uint64_t count, OutValue* out_keys,
                                  OutValue* out_aggs, OutPartial* out_parts, uint64_t* out_rep, uint32_t* err_flags, hipStream_t st,
                                  const uint32_t* cand = nullptr, OutValue* ord = nullptr, bool ord_is_key = false, uint32_t ord_index = 0,
                                  uint64_t* images = nullptr, bool desc = false);  // (images: order images of the ORDER BY term instead of ord)
hipError_t launch_add_counter(unsigned long long* p, unsigned long long v, hipStream_t st);
hipError_t launch_probe_keys(const Program& P, uint64_t nrows, const GlobalTable& G, uint32_t* err_flags, unsigned long long* ngroups,
                             uint32_t grid, hipStream_t st);
hipError_t launch_project_records(const Program& P, const ProjectArgs& A, uint32_t grid, hipStream_t st);
hipError_t launch_agg_bins(const Program& P, const BinAggArgs& A, const GlobalTable& G, unsigned long long* ngroups, uint32_t grid,
                           hipStream_t st);
size_t topk_state_bytes();
size_t topk_ncand_offset();
hipError_t launch_topk_select(const Program& P, const OutValue* vals, uint32_t stride, uint32_t index, uint64_t n, bool desc,
                              uint64_t keep, uint64_t* images, void* state, uint32_t* cand, hipStream_t st, bool sampled = false, bool images_done = false);
hipError_t launch_topk_select_images(const uint64_t* images, uint64_t n, uint64_t keep, void* state, uint32_t* cand, hipStream_t st, bool sampled);
bool topk_can_sample(uint64_t n, uint64_t keep);
uint64_t topk_cand_entries(uint64_t n);  // entries of the candidate buffer launch_topk_select needs for n groups  // enough groups for the sampled threshold (else the exact radix select)
hipError_t launch_topk_compact(const uint32_t* cand, uint64_t ncand, uint32_t nk, uint32_t na, const OutValue* keys,
                               const OutValue* aggs, const OutPartial* parts, const uint64_t* rep, OutValue* okeys, OutValue* oaggs,
                               OutPartial* oparts, uint64_t* orep, hipStream_t st);
hipError_t launch_distinct_layout(const Program& P, const GlobalTable& G, const DistinctArgs& D, hipStream_t st);
// COUNT(DISTINCT) over one-word members: one 256-bin partition pass (histogram, offsets, LDS-staged scatter) ...
hipError_t launch_radix_pass(const RadixArgs& A, uint32_t slices, hipStream_t st, bool have_hist = false);
// ... the per-bin LDS sets, the global-memory fallback, and the hand-over of the member counts to the set sizes
hipError_t launch_distinct_dedupe(const Program& P, const GlobalTable& G, const DedupeArgs& D, uint32_t grid, uint32_t block, hipStream_t st);
size_t distinct_dedupe_lds(const DedupeArgs& D);
// (`nreg` regions of fixed capacity: the 256 x kRecSubs sub-regions of a DISTINCT aggregate's member words)
hipError_t launch_compact_regions(const uint64_t* region, uint32_t nreg, uint64_t cap, const unsigned long long* count, const uint64_t* off,
                                  uint64_t* dst, hipStream_t st);
hipError_t launch_regrow_regions(const uint64_t* src, uint32_t nreg, uint64_t src_cap, uint64_t* dst, uint64_t dst_cap,
                                 unsigned long long* count, hipStream_t st);
hipError_t launch_distinct_words_global(const GlobalTable& G, const uint64_t* words, uint64_t n, uint64_t* table, uint64_t mask,
                                        uint32_t key_shift, unsigned long long* counts, uint32_t* err_flags, uint32_t grid,
                                        hipStream_t st);
hipError_t launch_distinct_add_counts(const Program& P, const GlobalTable& G, const unsigned long long* counts, uint32_t glob_off,
                                      hipStream_t st, const uint32_t* veto = nullptr);
hipError_t launch_distinct_insert(const Program& P, const GlobalTable& G, const DistinctArgs& D, uint32_t* err_flags,
                                  hipStream_t st);
hipError_t launch_export_partials(const Program& P, const GlobalTable& G, uint32_t nparts, uint64_t cap, uint64_t* out,
                                  uint64_t region_words, uint32_t* err_flags, hipStream_t st);
hipError_t launch_merge_partials(const Program& P, const GlobalTable& G, uint32_t nregions, uint64_t cap, const uint64_t* in,
                                 uint64_t region_words, uint32_t* err_flags, unsigned long long* ngroups, hipStream_t st,
                                 uint64_t limit = 0, bool unique_keys = false);
hipError_t launch_arith(const ArithArgs& A, hipStream_t st);
hipError_t launch_mathfn(const ArithArgs& A, hipStream_t st);  // ar_is_mathfn(A.op): mathfn_kernel<A.op>, the same arguments and layout
hipError_t launch_datefn(const ArithArgs& A, hipStream_t st);  // ar_is_datefn(A.op): datefn_kernel<A.op> (n1k_datefn.hip); rows outside the batch are skipped
hipError_t launch_cond(const Program& P, const CondArgs& C, hipStream_t st);  // one conditional node (n1k_cond.h) over P's columns
hipError_t launch_publish_counters(const unsigned long long* src, unsigned long long* dst, uint32_t n, hipStream_t st);
hipError_t launch_partition(const Program& P, const PartArgs& A, uint32_t grid, hipStream_t st);
struct HeaderList { unsigned long long* h[kMaxParts]; };  // the headers of the row regions a rank received (one per source)
hipError_t launch_exchange_verdict(const HeaderList& H, uint32_t nregions, uint32_t* err_flags, hipStream_t st);
hipError_t launch_stamp_verdict(unsigned long long* headers, uint32_t nregions, uint64_t stride_words, const uint32_t* err_flags,
                                uint32_t host_status, hipStream_t st);
hipError_t launch_dense_to_segments(unsigned long long* headers, uint32_t nregions, uint64_t stride_words, uint64_t sub_rows, hipStream_t st,
                                    const uint32_t* dest_cap = nullptr);  // dest_cap: regions of their own capacities (PartArgs::per_dest)
struct SpecEntry {
    const char* name;
    SpecSig sig;
    hipError_t (*launch)(const Program& P, const FastArgs& F, const GlobalTable& G, unsigned long long* ngroups,
                         uint32_t grid, uint32_t block, bool wide, const WordLogArgs& L, hipStream_t st);
    // records mode (partitioned GROUP BY): Filter + packed key -> 16-byte records in the hash regions
    hipError_t (*launch_records)(const Program& P, const FastArgs& F, uint32_t grid, bool wide, const WordLogArgs& L, hipStream_t st);
};
size_t spec_records_lds_bytes();
// n1k_bins.hip: the partitioned GROUP BY over 16-byte records — second partition pass (`bins_per_seg` bins of fixed capacity
// per hash region, a power of two <= 256) and the per-bin LDS tables (`block` threads per bin, `per_thread` = records a thread loads at once)
hipError_t launch_radix_scatter16(const RadixArgs& A, uint32_t wpr, uint32_t bins_per_region, hipStream_t st);
hipError_t launch_radix_scatter_words(const RadixArgs& A, uint32_t wpr, uint32_t bins_per_region, hipStream_t st);  // the same for 8-byte member words
size_t agg_bins16_lds_bytes(const Program& P, uint32_t slots);  // LDS of one agg_bins16 workgroup with `slots` table slots
hipError_t launch_agg_bins16(const Program& P, const BinAggArgs& A, uint32_t grid, uint32_t block, uint32_t per_thread, hipStream_t st,
                             bool specialise = true);  // (specialise: the plan's one aggregate as a compile-time constant)
const std::vector<SpecEntry>& spec_registry();
hipError_t launch_finalize(const Program& P, const GlobalTable& G, OutValue* out_keys, OutValue* out_aggs,
                           OutPartial* out_parts, uint64_t* out_rep, unsigned long long* out_count, uint64_t max_out,
                           uint32_t* err_flags, hipStream_t st);
// one workgroup, tables of at most 8192 slots: FinalGroup + the counters published to the host (+ table and counters left as
// n1k_reset leaves them): the one last kernel of a query
hipError_t launch_finalize_small(const Program& P, const GlobalTable& G, OutValue* out_keys, OutValue* out_aggs, OutPartial* out_parts,
                                 uint64_t* out_rep, unsigned long long* counters, unsigned long long* host_counters, uint64_t max_out,
                                 uint32_t* err_flags, bool clear, hipStream_t st);
// The slabs of a one-call execution's only scan launch (F.slabs, F.block_selected: nslabs workgroups) folded straight into
// result rows, the counters published behind them and zeroed (fold_rows_kernel): instead of launch_merge_slabs +
// launch_finalize_small.  counters[ticket_word] is the kernel's own; it must be zero before and is zero after.  The table G is
// only read: rows the scan's bypass of the narrow LDS sums left there join their groups, and host_counters[ticket_word] is
// then their number (not zero: the table is not empty behind this query).
hipError_t launch_fold_rows(const Program& P, const FastArgs& F, const GlobalTable& G, uint32_t nslabs, OutValue* out_keys, OutValue* out_aggs,
                            OutPartial* out_parts, uint64_t* out_rep, unsigned long long* counters, uint32_t ticket_word,
                            unsigned long long* host_counters, uint64_t max_out, hipStream_t st);
// Filter alone in one pass: predicate + ordered compaction, tile offsets by a chained scan (tile_state: ntiles + 1 words, the
// last one the tile counter; zeroed here)
hipError_t launch_filter_stream(const Program& P, uint64_t nrows, uint64_t row_base, uint64_t* out_rows, unsigned long long* tile_state,
                                unsigned long long* tile_counter, unsigned long long* total, uint32_t* err_flags, uint32_t grid,
                                hipStream_t st, bool fast = false);  // fast: ONE TERM_NUM_* comparison of a TAGGED64 column, wide loads
// ... with 32-bit batch-local ordinals (the first row of the batch is 0; nrows < 2^32): the selection that stays on the device
hipError_t launch_filter_stream(const Program& P, uint64_t nrows, uint32_t* out_rows, unsigned long long* tile_state,
                                unsigned long long* tile_counter, unsigned long long* total, uint32_t* err_flags, uint32_t grid,
                                hipStream_t st, bool fast);
// The rows a selection names, of up to kGatherMaxCols columns of either kind, in one launch: row i of dst = row rows[i] of src,
// i < n (n < 2^32; `rows` 16-byte aligned; no requirement on any column pointer)
constexpr uint32_t kGatherMaxCols = 16;
struct GatherCol {
    uint32_t kind, pad;  // COLK_*
    const uint8_t* src_tags;
    const uint64_t* src_payload;
    const uint32_t* src_codes;
    uint8_t* dst_tags;
    uint64_t* dst_payload;
    uint32_t* dst_codes;
};
struct GatherArgs {
    const uint32_t* rows;
    uint64_t n;
    uint32_t ncols, pad;
    GatherCol cols[kGatherMaxCols];
};
hipError_t launch_gather_rows(const GatherArgs& A, hipStream_t st);
// ---- raw JSON documents -> leaf columns on the device (n1k_jsondev.hip)
constexpr uint32_t kJsonMaxSteps = 4;  // field names of a leaf path below the keyspace alias
struct JsonDevPath {
    uint32_t nsteps;
    uint32_t name_off[kJsonMaxSteps], name_len[kJsonMaxSteps];  // the names' bytes in JsonDevArgs::names
};
struct JsonDevArgs {
    const uint8_t* bytes;     // the batch's documents, back to back (+ 32 spare bytes); document d = [offsets[d] - base, offsets[d + 1] - base)
    const uint64_t* offsets;  // ndocs + 1
    uint64_t base, ndocs;
    uint32_t npaths, tab_bits;
    JsonDevPath paths[kMaxCols];
    char names[1024];
    uint8_t* out_tags[kMaxCols];
    uint64_t* out_payload[kMaxCols];
    uint8_t* status;                    // per document: 0 extracted here, 1 left to the host's scalar extractor
    unsigned long long* tab_hash;       // the batch's string table: 1 << tab_bits slots, 0 = free
    unsigned long long* tab_first;      // [63] valid [offset of the first occurrence in `bytes` : 39][length : 24]
    uint32_t* new_list;                 // slots taken by this batch, in no particular order
    unsigned long long* new_count;
    uint32_t new_cap;
};
hipError_t launch_json_extract(const JsonDevArgs& A, uint32_t num_cus, hipStream_t st);
hipError_t launch_json_remap(const JsonDevArgs& A, const uint32_t* code_of, hipStream_t st);
hipError_t launch_json_gather_first(const JsonDevArgs& A, uint64_t n, unsigned long long* out, hipStream_t st);
hipError_t launch_json_scatter_codes(const uint32_t* new_list, const uint32_t* codes, uint64_t n, uint32_t* code_of, hipStream_t st);
hipError_t launch_json_patch(const JsonDevArgs& A, const uint64_t* docs, const uint8_t* tags, const uint64_t* payload, uint64_t n, hipStream_t st);
hipError_t launch_synth(const SynthArgs& a, hipStream_t st);

}  // namespace n1k
