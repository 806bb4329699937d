/*
 * n1k.h — C ABI of the MI355X-native Filter -> Group -> Aggregate pipeline.
 *
 * This is the drop-in boundary for ONE hot path of the N1QL engine
 * (pavel-paulau/query): the chain
 *
 *     Parallel{ Sequence[ Filter, InitialGroup ] } -> IntermediateGroup -> FinalGroup
 *
 * Every entry point names the reference interface it replaces (paths are
 * relative to the reference tree).  The reference has no FFI of its own (it is
 * 100 % Go); the cgo stub a maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions
 *   - plain C, no C++/torch types; all pointers are caller-owned unless stated;
 *   - every function returns an n1k_status; the message for the last failure
 *     of a handle is n1k_last_error(h);
 *   - one handle == one operator copy (reference: Operator.Copy(),
 *     execution/parallel.go:67-73).  A handle is NOT re-entrant, different
 *     handles may be driven from different OS threads concurrently;
 *     n1k_stop() alone may be called concurrently with a push on the same
 *     handle (reference: SendStop, execution/base.go:313-338).
 *   - the library never falls back to a CPU implementation: if no HIP device
 *     is usable every compute call fails with N1K_DEVICE_ERROR.
 */
#ifndef N1K_H
#define N1K_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define N1K_ABI_VERSION 3 /* 2: n1k_result.nproj / proj, projection and communicator entry points; 3: n1k_stats.query_ms,
                             N1K_REGION_FULL, n1k_partials_step, n1k_failure_is_global.  Entry points that only add to the ABI
                             (the Filter-only calls, n1k_order_key, n1k_rowdistinct_stats) and new plan forms leave it at 3: no
                             struct changed its layout and no call its meaning */

/* ---------------------------------------------------------------- status -- */

typedef enum n1k_status {
    N1K_OK = 0,
    N1K_UNSUPPORTED = 1,      /* plan/expression outside the device subset: caller keeps the reference operators */
    N1K_EVAL_ERROR = 2,       /* ≙ errors.NewEvaluationError (execution/filter.go:51-54, group_initial.go:62-65) */
    N1K_DEVICE_ERROR = 3,     /* HIP failure or no device; ≙ context.Fatal */
    N1K_OOM = 4,              /* host/device allocation failed or group-table capacity exceeded */
    N1K_STOPPED = 5,          /* n1k_stop() was observed (≙ processItem returning false after SendStop) */
    N1K_INVALID = 6,          /* bad argument / batch shape */
    N1K_UNSUPPORTED_DATA = 7, /* a value met at run time is outside the device subset (see n1k_tag) */
    N1K_REGION_FULL = 8       /* multi-GPU: a fixed-capacity region of an exchange overflowed; the step is void on EVERY rank alike —
                                 repeat it with a larger capacity on every rank (never an allocation failure: that is N1K_OOM) */
} n1k_status;

/* ------------------------------------------------------------ value tags -- */

/*
 * Value tags.  Order == N1QL type order (value/value.go:69-79:
 * MISSING < NULL < BOOLEAN < NUMBER < STRING < ARRAY < OBJECT < BINARY), with
 * BOOLEAN and NUMBER split into their two representations:
 * FALSE<TRUE (value/boolean.go:99-113), INT/FLOAT = intValue/floatValue
 * (value/integer.go, value/float.go).
 */
typedef enum n1k_tag {
    N1K_T_MISSING = 0,
    N1K_T_NULL = 1,
    N1K_T_FALSE = 2,
    N1K_T_TRUE = 3,
    N1K_T_INT = 4,    /* payload = int64 */
    N1K_T_FLOAT = 5,  /* payload = IEEE-754 binary64 bits; never integral-in-int64-range for parsed input
                         (NewValue folds those to INT, value/value.go:377-382) */
    N1K_T_STRING = 6, /* payload = code in the handle's string dictionary */
    N1K_T_ARRAY = 7,  /* payload = dictionary code of the canonical JSON text (group keys / COUNT only) */
    N1K_T_OBJECT = 8  /* idem */
} n1k_tag;

/* DICT32 columns carry no tag byte: these two codes stand for MISSING / NULL */
#define N1K_CODE_MISSING 0xFFFFFFFFu
#define N1K_CODE_NULL 0xFFFFFFFEu

/* A tagged scalar as returned in results (16 bytes). */
typedef struct n1k_value {
    uint8_t tag; /* n1k_tag */
    uint8_t pad[7];
    union {
        int64_t i;
        double f;
        uint64_t code; /* STRING/ARRAY/OBJECT: dictionary code */
    } v;
} n1k_value;

/* --------------------------------------------------------- column batches -- */

typedef enum n1k_col_kind {
    N1K_COL_TAGGED64 = 0, /* tags[nrows] (1 B) + payload[nrows] (8 B) */
    N1K_COL_DICT32 = 1    /* codes[nrows] (4 B): string code, N1K_CODE_MISSING or N1K_CODE_NULL */
} n1k_col_kind;

typedef struct n1k_col {
    uint32_t kind;           /* n1k_col_kind */
    uint32_t reserved;
    const uint8_t *tags;     /* TAGGED64 */
    const uint64_t *payload; /* TAGGED64 */
    const uint32_t *codes;   /* DICT32 */
} n1k_col;

/*
 * One batch of rows, column-wise.  Column i holds, for every row, the value of
 * leaf path i of the plan (n1k_num_columns / n1k_column_path): what
 * Field.Apply / Identifier.Evaluate would return for that row
 * (expression/nav_field.go:134-160, identifier.go:48-51).
 */
typedef struct n1k_batch {
    uint64_t nrows;
    uint32_t ncols;
    uint32_t reserved;
    const n1k_col *cols;
} n1k_batch;

/* ----------------------------------------------------------------- results -- */

/* Raw, mergeable accumulators of one aggregate of one group (the reference's
 * "partial" values: algebra/aggregate.go:25-40). */
typedef struct n1k_partial {
    int64_t count;      /* COUNT/COUNTN: the count.  SUM/AVG: number of NUMBER operands */
    int64_t isum;       /* SUM/AVG: exact integer part of the sum when int_exact != 0 */
    double fsum;        /* SUM/AVG: sum of the FLOAT operands (plus the integer part when int_exact == 0) */
    uint8_t int_exact;  /* 1: no FLOAT operand seen and the integer sum fits int64 */
    uint8_t has_float;  /* 1: at least one FLOAT operand */
    uint8_t pad[6];
    n1k_value extreme;  /* MIN/MAX: current winner (NULL when none) */
    int64_t distinct;   /* COUNT(DISTINCT)/COUNTN(DISTINCT): set size; SUM/AVG(DISTINCT): set size */
} n1k_partial;

typedef struct n1k_result {
    uint64_t ngroups;
    uint32_t nkeys;
    uint32_t naggs;
    const n1k_value *keys;       /* [ngroups][nkeys]  group key values (MISSING keys stay MISSING) */
    const n1k_value *aggs;       /* [ngroups][naggs]  ComputeFinal() values, plan order */
    const n1k_partial *partials; /* [ngroups][naggs]  */
    const uint64_t *rep_row;     /* [ngroups] smallest input row ordinal of the group (the reference keeps the
                                    first row it met as carrier, execution/group_initial.go:69-72) */
    uint64_t nselected;          /* Filter-only plans: number of rows that passed */
    const uint64_t *selected;    /* Filter-only plans: their row ordinals, ascending */
    uint32_t nproj;              /* plans with an InitialProject: number of result terms, else 0 */
    uint32_t reserved1;
    const n1k_value *proj;       /* [ngroups][nproj]  value of every result term (≙ the "projection" attachment,
                                    execution/project_initial.go:100-144; a MISSING term is left out of the row) */
} n1k_result;

typedef struct n1k_stats {
    uint64_t rows_in;       /* ≙ #itemsIn  (execution/base.go:32-46) */
    uint64_t rows_selected; /* rows that passed the Filter (≙ Filter #itemsOut) */
    uint64_t groups_out;    /* ≙ FinalGroup #itemsOut */
    uint64_t batches;
    double device_ms;       /* hipEvent time of all device work (≙ execTime) */
    uint64_t bytes_scanned; /* algorithmic column bytes read by the scan kernel */
    uint32_t agg_mode;      /* n1k_agg_mode actually used by the last batch */
    uint32_t spec_kernel;   /* plan-specialised kernel that ran the last batch: 0 none, 1 prebuilt, 2 built at run time, 3 built at run time with the plan's arithmetic nodes evaluated in registers */
    uint64_t wide_key_values; /* distinct key numbers held in the wide-value tables (floats, |int| beyond the field); set by finish/export */
    uint32_t distinct_path;  /* how the last finish built the DISTINCT sets: bit 0 per-group sets in global memory (two-word
                                pairs), bit 1 radix partition + LDS sets (one-word members), bit 2 global one-word set (fallback) */
    uint32_t order_passes;   /* ordered Filter-only plans: radix passes the last n1k_filter_device_batch launched (a digit whose
                                histogram has one non-empty bin costs none) */
    uint64_t topk_candidates; /* ORDER BY ... LIMIT: groups that left the device after the top-k filter (0 = filter not used) */
    uint64_t json_device_docs; /* documents of n1k_push_json whose leaf values the DEVICE extractor produced (the rest: the host's) */
    double query_ms;        /* hipEvent time of the last WHOLE query on the handle's stream: from n1k_reset (reopen) to the last
                               kernel / copy of n1k_finish — every kernel of the query and the gaps between them; 0 until a
                               finish has completed.  device_ms above covers the batches' kernels only. */
} n1k_stats;

typedef enum n1k_agg_mode {
    N1K_MODE_AUTO = 0,
    N1K_MODE_LDS_HASH = 1,  /* open-addressed LDS table per workgroup, global atomic merge */
    N1K_MODE_LDS_DIRECT = 2,/* perfect-hash LDS table (small dictionary-coded key domain), slab merge */
    N1K_MODE_GLOBAL = 3,    /* no LDS stage: global open-addressed table only */
    N1K_MODE_PARTITIONED = 4 /* high cardinality: rows -> records, radix partition on the key hash, per-bin LDS tables */
} n1k_agg_mode;

typedef struct n1k_handle n1k_handle;

/* ------------------------------------------------------------ life cycle -- */

/*
 * Build an operator from the reference's own plan JSON.
 * Replaces: execution.builder.VisitParallel / VisitFilter / VisitInitialGroup
 *           (execution/build.go:281-296, 457-491) + NewFilter / NewInitialGroup /
 *           NewIntermediateGroup / NewFinalGroup.
 * plan_json is ONE of
 *   {"#operator":"Sequence","~children":[{"#operator":"Filter","condition":"…"},
 *                                        {"#operator":"InitialGroup","group_keys":[…],"aggregates":[…]}]}
 *   {"#operator":"InitialGroup", …}            (no Filter)
 *   {"#operator":"Filter","condition":"…"}     (Filter only: result = selected row ordinals)
 *   {"#operator":"Sequence","~children":[<Filter only, bare or under Parallel / Sequence>,       (ORDER BY / OFFSET / LIMIT over
 *        {"#operator":"Order","sort_terms":[{"expr":"…","desc":true}],"offset":"…","limit":"…"},  the rows of a Filter-only plan:
 *        {"#operator":"Offset","expr":"…"}, {"#operator":"Limit","expr":"…"}]}                    n1k_filter_device_batch)
 *     1 to 4 sort terms, each a leaf path of the row in the text form a condition uses (its path joins the plan's columns
 *     behind the condition's); offset / limit are integer constants; Offset / Limit may come without Order.  Arithmetic,
 *     functions, aggregates or constants as sort terms, more than 4 terms, Order with neither Filter nor group before it,
 *     and InitialProject / FinalProject in a plan without a group (the caller projects with n1k_gather_selected) are
 *     N1K_UNSUPPORTED.  Such a plan runs through n1k_filter_device_batch alone: n1k_push_batch, n1k_push_device_batch,
 *     n1k_push_json and n1k_run_device_batch answer N1K_UNSUPPORTED.
 *   {"#operator":"Sequence","~children":[                                                     (SELECT DISTINCT over the rows,
 *        {"#operator":"Parallel","~child":{"#operator":"Sequence","~children":[                planner/build_select_sub.go:217-240,
 *             {"#operator":"Filter",…},                                                        plan/project.go:69-108,
 *             {"#operator":"InitialProject","distinct":true,"result_terms":[{"expr":"…","as":"…"}]},   plan/distinct.go:32-40:
 *             {"#operator":"Distinct"}, {"#operator":"FinalProject"}]}},                       n1k_filter_device_batch)
 *        {"#operator":"Distinct"}, Order, Offset, Limit, {"#operator":"FinalProject"}]}
 *     also bare, without the outer Sequence or the Parallel; the Filter, the FinalProjects and the tail are optional, the two
 *     Distinct nodes are one stage.  1 to 4 result terms, each a leaf path of the row in the text form a condition uses, each
 *     with an optional alias (n1k_num_projection_terms / n1k_projection_expr / n1k_projection_alias report them); their paths
 *     join the plan's columns behind the condition's and before the sort terms', none twice.  A sort term is a leaf path or
 *     `alias`, which names a result term — by its explicit alias, else by the last field name of its path — and resolves to that
 *     term's path.  Without Filter every row is a survivor.  Expressions, functions or constants as terms, star or raw
 *     projections, more than 4 terms, a Distinct without the InitialProject{distinct} before it or after Order / Offset / Limit,
 *     an InitialProject{distinct} that no Distinct follows, and distinct over groups are N1K_UNSUPPORTED; so is an InitialProject
 *     without distinct in a plan without a group.  One batch through n1k_filter_device_batch, as for the ordered plans.
 *   {"#operator":"Parallel","~child":<one of the above>, "maxParallelism":n}
 *   {"#operator":"Sequence","~children":[<one of the above>, IntermediateGroup, FinalGroup,      (the grouped tail:
 *        {"#operator":"Filter","condition":"…"},                                       HAVING, plan/filter.go
 *        {"#operator":"Order","sort_terms":[{"expr":"…","desc":true}],"offset":"…","limit":"…"},  plan/order.go:51-79
 *        {"#operator":"Offset","expr":"…"}, {"#operator":"Limit","expr":"…"}]}               plan/limit.go:46-53)
 *        {"#operator":"Parallel","~child":{"#operator":"Sequence","~children":[                   (HAVING and projection
 *             {"#operator":"Filter",…}, {"#operator":"InitialProject","result_terms":[{"expr":"…","as":"…"}]}]}},    as the planner
 *        {"#operator":"FinalProject"}]}                                                            nests them, plan/project.go:73-110)
 *     IntermediateGroup / FinalGroup must repeat the InitialGroup's lists (plan/group.go:106-273) and are subsumed;
 *     the result terms of an InitialProject are expressions over group keys and aggregates (constants, arithmetic,
 *     round / trunc / abs / ceil / floor / sign / sqrt, the library functions and ifinf / ifnan / ifnanorinf listed below):
 *     n1k_result.proj then holds their values per group, and a sort
 *     term may name a term's alias (`alias`) or repeat its expression; star / raw / distinct projections are N1K_UNSUPPORTED;
 *     the HAVING condition and the sort terms may name only group keys and aggregates of the plan (by their text);
 *     offset / limit are integer constants.  n1k_finish then returns the groups filtered, ordered and cut.
 * A VALUE of the Filter / InitialGroup part — a group key, an aggregate's operand, an operand of a comparison or of arithmetic, a
 * bare condition — may be, besides a leaf path, a constant, arithmetic, round / trunc / abs / ceil / floor / sign / sqrt and
 * greatest / least:
 *     case when <cond> then <value> [when … then …]* [else <value>] end            (expression/case_searched.go:73-100)
 *     case <value> when <value> then <value> … [else <value>] end                  (case_simple.go:78-110)
 *     ifmissing(a, b, …)  ifnull(a, b, …)  ifmissingornull(a, b, …)  with 2 to 4 arguments,   (func_cond_unknown.go)
 *     nullif(a, b)  missingif(a, b)
 *   evaluated per row on the device, the arms of a CASE in order and each row only up to its first taken arm.  Their operands are
 *   values again (paths, constants, arithmetic, another of these).  A STRING they return is a code of the handle's dictionary:
 *   a THEN constant equal to a string the columns hold is that string.  N1K_UNSUPPORTED, each named in n1k_create_error: more
 *   than 8 WHEN arms; more than 16 predicate terms or 32 logic ops in the WHENs of one CASE; more than 4 arguments; LIKE,
 *   ANY / EVERY, IN or a string function inside a WHEN; greatest / least inside one of them; one of them in HAVING, in a
 *   projection over the groups, as a sort term or as a DISTINCT term of a Filter-only plan; more than 16 columns counting the
 *   plan's leaf paths, its arithmetic nodes and these.  A WHEN that orders two arrays / objects is N1K_UNSUPPORTED_DATA at run
 *   time, for the rows that reach that arm only.  Text that is no CASE (a missing THEN or END) is N1K_INVALID.
 * Numeric library functions (expression/func_num.go), values wherever round(...) is one — HAVING and projections over the groups
 * included:
 *     acos asin atan cos sin tan exp ln log degrees radians (one argument; ln is math.Log, log is math.Log10)
 *     atan2(y, x)  power(x, y)
 *     pi()  e()  nan()  posinf()  neginf()      constants at n1k_create: FLOAT payloads, no node and no column
 *     ifinf(a, b, …)  ifnan(a, b, …)  ifnanorinf(a, b, …)  with 2 to 4 arguments, in argument order      (func_cond_num.go:64-79)
 *     nanif(a, b)  posinfif(a, b)  neginfif(a, b)   like nullif, giving FLOAT NaN / +Inf / -Inf; refused where nullif is
 *   A MISSING argument gives MISSING, any other non-number NULL; the arguments go through float64 and the result through
 *   value.NewValue (power(12, 2) is INT 144).  Out-of-domain results are values: acos(3) and ln(-1) are FLOAT NaN, ln(0) is
 *   -Inf, exp(1000) is +Inf.  The eleven library routines are the device's, within a few ulp of Go's and not bit-identical.
 *   random is N1K_UNSUPPORTED, as are more than 4 arguments of ifinf / ifnan / ifnanorinf; a wrong argument count is N1K_INVALID.
 * exactly as plan.(*Filter).MarshalJSON (plan/filter.go:46-53),
 * plan.(*InitialGroup).MarshalJSON (plan/group.go:54-70), plan/sequence.go:48-57 and
 * plan/parallel.go:54-67 emit them; expressions are expression.Stringer text.
 * Returns N1K_UNSUPPORTED (and *out == NULL) for anything outside the device subset.
 */
n1k_status n1k_create(const char *plan_json, size_t len, n1k_handle **out);

/* ≙ Operator.Done() (execution/execution.go:26-64): frees host + device state. */
void n1k_destroy(n1k_handle *h);

/* ≙ reopen() (execution/group_initial.go:117-120): drop all groups, keep plan + dictionary. */
n1k_status n1k_reset(n1k_handle *h);

/* ≙ SendStop() (execution/base.go:313-338): safe from any thread. */
void n1k_stop(n1k_handle *h);

const char *n1k_last_error(const n1k_handle *h);
/* message of a failed n1k_create (thread-local) */
const char *n1k_create_error(void);

/* --------------------------------------------------------------- binding -- */

/* Leaf paths of the plan, in column order: stringer text such as
 * "(`default`.`price`)".  The caller evaluates exactly these per row. */
uint32_t n1k_num_columns(const n1k_handle *h);
const char *n1k_column_path(const n1k_handle *h, uint32_t i);
uint32_t n1k_num_keys(const n1k_handle *h);
uint32_t n1k_num_aggregates(const n1k_handle *h);
/* agg.String() of aggregate i — the key of the reference's "aggregates"
 * attachment map (execution/group_initial.go:74-79). */
const char *n1k_aggregate_name(const n1k_handle *h, uint32_t i);

/* Result terms of the plan's InitialProject — over the final groups, or the one of a DISTINCT over the rows — (0 when it has
 * none): expression text and explicit alias ("" = none; the caller derives one as algebra.ResultTerm does: the last name of
 * a path, else $1, $2, ...). */
uint32_t n1k_num_projection_terms(const n1k_handle *h);
const char *n1k_projection_expr(const n1k_handle *h, uint32_t i);
const char *n1k_projection_alias(const n1k_handle *h, uint32_t i);

/* ------------------------------------------------------------ dictionary -- */

/* Intern n strings (bytes[offsets[i]..offsets[i+1])) into the handle's
 * dictionary; out_codes[i] receives the code.  Equal byte strings always get
 * equal codes (string equality ≙ value/string.go:82-96).  Codes are handed out in
 * interning order starting at 0; the plan's own string constants are interned at the
 * first push, so a dictionary interned right after n1k_create keeps code == index. */
n1k_status n1k_dict_intern(n1k_handle *h, uint32_t n, const uint64_t *offsets, const char *bytes,
                           uint32_t *out_codes);
uint32_t n1k_dict_size(const n1k_handle *h);
n1k_status n1k_dict_get(const n1k_handle *h, uint32_t code, const char **ptr, size_t *len);

/* ---------------------------------------------------------------- options -- */

/* name ∈ {"device" (ordinal) | "stream" (hipStream_t) | "rep_row" (0/1): before the first push;
 *         "max_groups" (group-table capacity bound, default 1<<26; the table itself grows with the rows pushed), "agg_mode" (n1k_agg_mode),
 *         "grid_blocks" / "block" / "rows_per_lane" / "lds_bytes" (launch tuning, 0 = auto),
 *         "fast" / "spec" / "wide" / "slabs" (0/1: kernel selection switches used by the ablation tests),
 *         "jit" (0 off, 1 = compile a specialised kernel for large batches of unregistered shapes, 2 = always),
 *         "jit_min_rows", "distinct_words" (0/1, before the first push: COUNT(DISTINCT) members that fit one word are
 *         de-duplicated by radix partition + LDS sets), "partition_min_rows" / "partition_probe_rows" / "partition_min_groups" / "partition_levels" (when AUTO takes the
 *         partitioned high-cardinality path: batches of at least min_rows (8 Mi) rows whose first probe_rows (512 Ki) rows
 *         bring at least min_groups (4096) new groups; forced number of passes), "topk_min_groups" (ORDER BY ... LIMIT: the device top-k filter runs from this many groups on, default 65536),
 *         "distinct_set_slots" / "distinct_levels" (LDS set size, forced number of partition passes: tests),
 *         "rowdistinct_slots" (DISTINCT over rows: forced capacity of the table of ordinals, any value >= 1, not rounded; 0 = the
 *         next power of two >= 2 x survivors: tests) / "rowdistinct_lds_slots" (size of an LDS set ahead of it that passes on only the smallest
 *         ordinal a workgroup has met of a key, at most 4096; default 0 = none),
 *         "distinct_region_cap" (forced capacity of the specialised scan's hash regions: tests), "dedupe_block" (256 / 512 / 1024: tuning), "wide_values" (before the first push: how many distinct float / wide-integer group key
 *         values the handle can code, default 1<<20; 0 = such keys are N1K_UNSUPPORTED_DATA),
 *         "inject_failure" (tests of the multi-GPU failure rules, one shot, on the SENDING handle: the next exchange call
 *         pretends that 1 = its buffers, 2 = its partition / export, 3 = its receiving part failed)} */
n1k_status n1k_set_option(n1k_handle *h, const char *name, int64_t value);

/* ----------------------------------------------------------------- data ---- */

/*
 * Raw documents -> the plan's leaf columns.
 * Replaces: the per-row, per-field leaf accesses of the operators over a parsedValue — Field.Apply
 *           (expression/nav_field.go:134-160) -> parsedValue.Field (value/parsed.go:159-207: go_json FirstFind of the
 *           field in the raw bytes) -> value.NewValue typing (value/value.go:367-430: integer literals that fit
 *           int64 are INT, a float64 with no fraction folds to INT) — done once per batch.
 * Document d is bytes[offsets[d] .. offsets[d+1]) (one UTF-8 JSON value, the file datastore's <key>.json content,
 * datastore/file/file.go:732-749).  Leaf paths must be chains of field names; the first field of a name counts;
 * a field of a non-object is MISSING; strings and the canonical text of arrays / objects (sorted names, compact:
 * value/object.go:30-78) are interned in the handle's dictionary.  The columns (TAGGED64) belong to the handle
 * until the next extract / destroy.  Parsing is multi-threaded ("json_threads" option, default = the cores, <= 16).
 * N1K_INVALID names the first malformed document.  Needs no device.
 */
n1k_status n1k_extract_json(n1k_handle *h, uint64_t ndocs, const uint64_t *offsets, const char *bytes, n1k_batch *out);

/* n1k_extract_json + n1k_push_batch */
n1k_status n1k_push_json(n1k_handle *h, uint64_t ndocs, const uint64_t *offsets, const char *bytes);

/*
 * ≙ processItem() over a batch (execution/filter.go:49-61 +
 * execution/group_initial.go:56-100).  Host pointers; the call copies them to
 * the device before returning (cgo rule: no Go pointer is retained).
 */
n1k_status n1k_push_batch(n1k_handle *h, const n1k_batch *batch);

/* Same, but every pointer in the batch is a DEVICE pointer on the handle's
 * device (columns already resident in HBM); nothing is copied.  The call is
 * asynchronous on the handle's stream; the buffers must stay valid until
 * n1k_finish / n1k_sync. */
n1k_status n1k_push_device_batch(n1k_handle *h, const n1k_batch *batch);

/* One whole execution of the operator over a device-resident batch: n1k_reset + n1k_push_device_batch + n1k_finish in one
 * call (≙ reopen() + processItem()* + afterItems() of a re-opened operator, execution/base.go:119-135: what a prepared
 * statement executed again over the same resident columns does).  Same results and errors as the three calls. */
n1k_status n1k_run_device_batch(n1k_handle *h, const n1k_batch *batch, n1k_result *out);

/* ------------------------------------------- Filter-only plans on the device -- */

/*
 * The answer of a Filter-only plan that stays on the device: what lets the Filter feed the next operator (a projection,
 * n1k_push_device_batch of a group handle, an exchange) without its ordinals crossing to the host and back.  The three-call
 * path and n1k_run_device_batch keep returning 64-bit host ordinals in n1k_result.selected.
 */
typedef struct n1k_selection {
    uint64_t nselected;     /* rows whose condition is TRUE; a plan with Offset / Limit: those left after the cut */
    const uint32_t *rows;   /* DEVICE pointer: their ordinals inside the batch — ascending for a plan without Order, else in
                               ORDER BY order (rows that tie on every term in ascending ordinal) — cut to [offset, offset + limit);
                               owned by the handle, valid until the next n1k_filter_device_batch / n1k_reset / n1k_destroy;
                               NULL when 0 */
} n1k_selection;

/*
 * One whole execution of a Filter-only plan over a device-resident batch (≙ reopen() + processItem()* of a Filter,
 * execution/filter.go:49-61 — the counterpart of n1k_run_device_batch): one launch and one wait, which brings back the
 * survivor count and the error flags only; no ordinal leaves the device.  Ordinals are local to the batch (its first row
 * is 0), so batch->nrows must be below 2^32.  N1K_INVALID: a NULL argument, a plan that has a group, 2^32 rows or more, a
 * batch that does not validate (all checked before a device is touched); N1K_STOPPED: n1k_stop was observed;
 * N1K_UNSUPPORTED_DATA: as n1k_finish reports it.  Afterwards n1k_get_stats describes this call (rows_in, rows_selected,
 * batches, device_ms, query_ms, spec_kernel); the handle is otherwise as after n1k_reset: a following n1k_finish returns an
 * empty selection.  One batch per selection.
 *
 * A plan with Order / Offset / Limit (n1k_create): the selection comes back ordered and cut, from this same call (≙
 * execution/order.go:121-169, order_limit.go, offset.go, limit.go).  The order is value.Collate term by term, DESC flipping a
 * term, with an INT and a FLOAT compared exactly and rows that tie on every term in ascending ordinal (the reference's
 * sort.Sort is not stable: any tie order is admissible there); -0.0, 0.0 and INT 0 tie; a NaN sorts before every number.  The
 * sort runs on the device — radix passes over 64-bit keys (n1k_order_key), a radix select of the offset + limit smallest
 * first when that is fewer rows than were selected and at least "topk_min_groups" were — behind a few more small waits.
 * An ARRAY or OBJECT met as a sort value: N1K_UNSUPPORTED_DATA.  n1k_get_stats: rows_in, rows_selected = the cut count,
 * topk_candidates = the rows the select passed on to the sort (0: it did not run).
 *
 * A plan with Distinct (n1k_create): between the Filter and the tail the survivors are de-duplicated on the device (≙
 * execution/distinct.go:60-71, whose set is keyed by the JSON text of the projected object, value/set.go:100-103).  Two rows
 * are equal when every result term is: a MISSING term is left out of the object, so MISSING != NULL; FALSE, TRUE and NULL are
 * each a value of their own; numbers are equal when numerically equal, compared exactly — INT 2 = FLOAT 2.0 and -0.0 = 0.0 =
 * INT 0 (value/float.go:41-45), INT 2^53+1 != FLOAT 2^53, INT 2^63-1 != FLOAT 2^63; STRING / ARRAY / OBJECT are equal by
 * dictionary code within the same tag.  Divergence: all NaNs are one value and each infinity its own, where the reference
 * would also collide them with the strings "NaN" / "+Infinity" / "-Infinity" (value/float.go:31-39).  The representative of
 * a distinct row is the survivor with the smallest ordinal (the reference keeps whichever a Parallel copy met first: any is
 * admissible there).  Without Order the selection is the representatives in ascending ordinal; with Order the sort terms
 * are read at the representative; Offset / Limit cut after that; nselected and rows_selected are the counts after the cut.
 * n1k_selected_to_host32 and n1k_gather_selected work on the result as on any selection.  The table of ordinals takes the
 * next power of two >= 2 x survivors slots ("rowdistinct_slots" forces another capacity); a table with no room: N1K_OOM, the
 * handle as after n1k_reset.  One more wait, for the representatives' count.
 */
n1k_status n1k_filter_device_batch(n1k_handle *h, const n1k_batch *batch, n1k_selection *out);

/* Diagnostics of the last DISTINCT over rows of this handle: out[0] survivors of the Filter, [1] distinct rows before the
 * cut, [2] slots of the table, [3] rows that reached the table (all of them, unless "rowdistinct_lds_slots" is set: the others then
 * fell to a smaller ordinal of their key in the LDS set of their workgroup). */
n1k_status n1k_rowdistinct_stats(const n1k_handle *h, uint64_t out[4]);

/* The last selection's ordinals to the caller's host buffer (pinned or not) of `capacity` entries: 4 bytes per survivor of
 * execution/filter.go:49-61, one copy, one wait.  N1K_INVALID: no selection, or capacity below nselected. */
n1k_status n1k_selected_to_host32(n1k_handle *h, uint32_t *out, uint64_t capacity);

/*
 * The survivors' rows of any device-resident batch (the items a Filter sends on, execution/filter.go:49-61, column-wise):
 * for i below nselected, row i of out_cols[c] becomes row rows[i] of src->cols[c].  `src` holds 1 to 16 columns of either
 * kind — not necessarily the plan's: `asin` and `title` for a plan that filters on `type` — and as many rows as the
 * filtered batch; out_cols[c] has the kind of src->cols[c] and points to device memory with room for capacity_rows rows.
 * Exactly nselected rows of every output array are written, nothing else; no pointer needs any alignment.  Asynchronous on
 * the handle's stream: n1k_sync waits for it.  N1K_INVALID: no selection, a NULL array, more than 16 columns, kinds or row
 * counts that do not match, capacity_rows below nselected.
 */
n1k_status n1k_gather_selected(n1k_handle *h, const n1k_batch *src, uint64_t capacity_rows, const n1k_col *out_cols);

/*
 * The sort key of one value of a sort term, as the device computes it for an ordered Filter-only plan: comparing
 * (key, residual) as unsigned integers is value.Collate with an INT and a FLOAT compared exactly.  Classes from the bottom:
 * MISSING, NULL, FALSE, TRUE, NaN, the numbers (the sortable form of their float64, either zero as +0.0), the strings by
 * `rank` (the bytewise rank of the string among the dictionary's).  residual: an INT's distance from its float64, biased by
 * 1024 — other than 1024 only beyond +-2^53.  desc: both complemented.  Needs no device.  N1K_UNSUPPORTED_DATA: an ARRAY or
 * OBJECT; N1K_INVALID: a NULL pointer, an unknown tag.
 */
n1k_status n1k_order_key(uint32_t tag, uint64_t payload, uint32_t rank, int desc, uint64_t *key, uint32_t *residual);

/* Wait for all queued device work of the handle. */
n1k_status n1k_sync(n1k_handle *h);

/*
 * ≙ afterItems() of InitialGroup + the whole IntermediateGroup and FinalGroup
 * (execution/group_intermediate.go:56-104, group_final.go:55-118): merges,
 * finalises (ComputeFinal) and returns all groups; emits the default row when
 * there are no keys and no input (group_final.go:108-117).  The result memory
 * is owned by the handle and valid until the next finish/reset/destroy.
 */
n1k_status n1k_finish(n1k_handle *h, n1k_result *out);

n1k_status n1k_get_stats(const n1k_handle *h, n1k_stats *out);

/*
 * Build (but do not run) the plan-specialised scan kernel of this plan for the given column kinds through the
 * in-process compiler (hiprtc): what the engine does lazily for large batches of a plan shape that has no
 * ahead-of-time instantiation.  Needs no GPU; a prepared-statement cache (plan/prepared.go) would call it at
 * PREPARE time.  `log` receives the compiler output.  N1K_UNSUPPORTED when the shape is outside the bounded family
 * (the interpreter kernel then runs the plan).
 */
n1k_status n1k_jit_check(n1k_handle *h, const uint32_t *col_kinds, uint32_t ncols, char *log, size_t loglen);

/* ------------------------------------------------------------------- LIKE -- */

/*
 * `a LIKE "pattern"` (expression/comp_like.go) runs on the device as one match per DISTINCT dictionary string — a
 * table of one byte per code, one bit per pattern of the plan — and one bit test per row.  The two entry points below
 * run the matchers on their own (tests, diagnostics); n1k_like_stats says which route built a handle's table.
 *
 * n1k_like_match: the host matcher, no GPU needed.  String i is bytes[offsets[i] - offsets[0], offsets[i + 1] -
 * offsets[0]); out_bits[i] = 1 when it matches.  N1K_INVALID for a pattern that is not valid UTF-8 (n1k_create
 * answers N1K_UNSUPPORTED for a plan that holds one).
 */
n1k_status n1k_like_match(const char *pattern, size_t pattern_len, uint64_t n, const uint64_t *offsets, const char *bytes,
                          uint8_t *out_bits);
/* The same through like_match_kernel on `device`.  *out_left_to_host counts the strings the kernel left to the host
 * matcher: longer than 128 bytes, or not valid UTF-8.  The results are those of n1k_like_match. */
n1k_status n1k_like_match_device(int device, const char *pattern, size_t pattern_len, uint64_t n, const uint64_t *offsets,
                                 const char *bytes, uint8_t *out_bits, uint64_t *out_left_to_host);
/* out[0] dictionary strings matched on the device so far, out[1] on the host, out[2] distinct patterns of the plan,
 * out[3] the number of new dictionary entries from which the device route is taken */
n1k_status n1k_like_stats(const n1k_handle *h, uint64_t out[4]);

/* ----------------------------------------------------------- ANY / EVERY -- */

/*
 * `ANY v IN a SATISFIES P END`, `EVERY ...`, `ANY AND EVERY ...` (expression/coll_any.go:42-85, coll_every.go:42-85,
 * coll_any_every.go:42-85 over collEval, coll_util.go:17-120) with `a` a leaf path of the row and P a tree of AND / OR /
 * NOT over `<e> cmp constant`, `<e> between c and c`, `<e> like "pattern"`, `<e> is [not] null | missing | valued`, <e>
 * the variable followed by at most two field names.  Such a term is a function of the ARRAY alone, so it runs as one
 * evaluation per DISTINCT array — one bit of the byte LIKE keeps per dictionary code, for the entries that are the
 * canonical text of an array — and one bit test per row: MISSING for MISSING, NULL for anything but an ARRAY.  LIKE
 * patterns and collection predicates share the eight bits of an entry.  The two entry points below run the evaluators
 * on their own (tests, diagnostics); n1k_coll_stats says which route built a handle's table.
 *
 * n1k_coll_eval: the host evaluator, no GPU needed.  predicate_text is one whole term as expression/stringer.go
 * writes it (any `v` in (`d`.`tags`) satisfies (`v` = "x") end); the binding expression is parsed and otherwise unused.
 * Entry i is the canonical JSON text (compact, names sorted) bytes[offsets[i] - offsets[0], offsets[i + 1] - offsets[0]);
 * out_bits[i] = 1 when the term is TRUE for that array, 0 when it is FALSE or the text is no array.  N1K_UNSUPPORTED
 * for a term n1k_create refuses in a plan, N1K_INVALID for text that is no such term.
 */
n1k_status n1k_coll_eval(const char *predicate_text, size_t len, uint64_t n, const uint64_t *offsets, const char *bytes,
                         uint8_t *out_bits);
/* The same through coll_match_kernel on `device`.  *out_left_to_host counts the arrays the kernel left to the host
 * evaluator: text longer than 192 bytes, a compared or matched string (or a member name) with a backslash escape, a
 * compared number beyond the exact conversions (over 18 digits; over 15 with a fraction), a string under LIKE that is not
 * valid UTF-8.  The results are those of n1k_coll_eval. */
n1k_status n1k_coll_eval_device(int device, const char *predicate_text, size_t len, uint64_t n, const uint64_t *offsets,
                                const char *bytes, uint8_t *out_bits, uint64_t *out_left_to_host);
/* out[0] arrays of the dictionary evaluated on the device so far, out[1] on the host, out[2] distinct collection
 * predicates of the plan, out[3] the number of new dictionary entries from which the device route is taken */
n1k_status n1k_coll_stats(const n1k_handle *h, uint64_t out[4]);

/* -------------------------------------------------------- array functions -- */

/*
 * array_length(a) (expression/func_array.go:888-897), array_count(a) (:376-393), array_sum(a) (:1911-1928, adding with
 * value/integer.go:266-352), array_avg(a) (:141-164), array_contains(a, c) (:307-323) and array_position(a, c)
 * (:1094-1110), with `a` a leaf path of the row and `c` a constant (NUMBER, STRING, TRUE, FALSE, null, missing), are
 * values wherever a plan takes one.  Such a term is a function of the ARRAY alone, so it runs as one evaluation per
 * DISTINCT array — one tag byte and one 8-byte payload per dictionary code and term, for the entries that are the
 * canonical text of an array — and one lookup per row: MISSING for MISSING, NULL for anything but an ARRAY.  Elements
 * are typed as the reference types them, value.NewValue over the decoded array (value/value.go:367-381,
 * value/parsed.go:120-122, 362): every number is a float64 first.  At most 4 distinct terms per plan.  The two entry
 * points below run the evaluators on their own (tests, diagnostics); n1k_arrfn_stats says which route built a handle's
 * tables.
 *
 * n1k_arrfn_eval: the host evaluator, no GPU needed.  term_text is one whole term as expression/stringer.go writes it
 * (array_contains((`d`.`tags`), "x")); the path is parsed and otherwise unused.  Entry i is the canonical JSON text
 * bytes[offsets[i] - offsets[0], offsets[i + 1] - offsets[0]); out_tags[i] / out_payload[i] are the term's value for that
 * array (N1K_T_*; INT: int64, FLOAT: float64 bits), N1K_T_NULL when the text is no array.  N1K_UNSUPPORTED for a term
 * n1k_create refuses in a plan, N1K_INVALID for text that is no such term.
 */
n1k_status n1k_arrfn_eval(const char *term_text, size_t len, uint64_t n, const uint64_t *offsets, const char *bytes,
                          uint8_t *out_tags, uint64_t *out_payload);
/* The same through arrfn_table_kernel on `device`.  *out_left_to_host counts the arrays the kernel left to the host
 * evaluator: text longer than 192 bytes; under array_sum, array_avg and array_contains / array_position with a NUMBER
 * constant a number beyond the exact conversions (over 18 digits; over 15 digits or a decimal exponent beyond +-22 with
 * a fraction) or an integer that float64 does not hold exactly; under array_contains / array_position with a STRING
 * constant a STRING element with a backslash escape that is reached before a match.  array_length and array_count hand
 * over nothing but the long texts.  The results are those of n1k_arrfn_eval. */
n1k_status n1k_arrfn_eval_device(int device, const char *term_text, size_t len, uint64_t n, const uint64_t *offsets,
                                 const char *bytes, uint8_t *out_tags, uint64_t *out_payload, uint64_t *out_left_to_host);
/* out[0] arrays of the dictionary evaluated on the device so far, out[1] on the host, out[2] distinct array-function
 * terms of the plan, out[3] the number of new dictionary entries from which the device route is taken */
n1k_status n1k_arrfn_stats(const n1k_handle *h, uint64_t out[4]);

/* --------------------------------------------------------- date functions -- */

/*
 * Five date functions (expression/func_date.go) are values wherever round(...) is one — operands of a Filter or HAVING
 * comparison and of arithmetic, group keys, aggregate operands, projection terms over the groups:
 *     date_part_millis(x, part [, "UTC"])   date_trunc_millis(x, part)   date_add_millis(x, n, part)
 *         x (and n) any NUMBER-valued operand; evaluated per row, fusable into the run-time-built scan
 *     str_to_millis(s)   date_part_str(s, part)
 *         s a leaf path of the row; evaluated once per DISTINCT dictionary string into the term's value table (one tag byte
 *         and one 8-byte payload per code), one lookup per row.  At most 4 distinct terms per plan.
 * `part` is a STRING constant, lower-cased; datePart's names: millennium century decade year quarter month day hour minute
 * second millisecond week day_of_year (doy) day_of_week (dow) iso_week iso_year iso_dow timezone timezone_hour
 * timezone_minute; dateAdd's: millennium ... millisecond and week; dateTrunc's: the same without week.  Any other name, a
 * part that is no constant and a third argument other than the constant "UTC" are N1K_UNSUPPORTED, the part named.
 * A MISSING argument gives MISSING, otherwise a wrong type NULL, a non-integral n NULL.  A call of constants is a constant.
 * time.Local is UTC on this path — the one divergence: a string without a zone is read as UTC, the timezone parts of a millis
 * value are 0; a string that carries an offset keeps it.  Results are exact (integer and plain float64 arithmetic).
 * Where the reference's answer would depend on wrapped or out-of-range arithmetic the ROW raises and the call that meets it
 * answers N1K_UNSUPPORTED_DATA: a millis operand or a result outside years 1 to 9999 UTC (-62135596800000 ...
 * 253402300799999), NaN or an infinity, |n| beyond 2^31, n * unit beyond int64 nanoseconds, and a date string whose
 * reading depends on the reference's toolchain (a 1-digit hour, day 00, a zone hour over 23 or minute over 59, more than 9
 * fraction digits, ',' for the fraction's '.').  Every other string that is no date of the 13 _DATE_FORMATS is NULL.
 * Hence the five are N1K_UNSUPPORTED inside CASE and the conditional functions (an arm that is not taken is evaluated all
 * the same), as are: every other date function (date_diff_*, date_add_str, date_trunc_str, millis_to_*, date_format_str,
 * weekday_*, date_range_*, now_*, clock_*, str_to_utc / _zone_name / _tz / _duration, duration_to_str), a first argument of
 * the string functions that is neither a leaf path nor a constant, and any of them inside SATISFIES.
 *
 * n1k_datefn_eval: the host evaluator, no GPU needed.  call_text is one whole call as expression/stringer.go writes it, its
 * first argument a leaf path that stands for the value, the others constants (date_add_millis((`d`.`t`), 3, "month")).
 * Value i is (in_tags[i], in_payload[i]) (N1K_T_*; INT: int64, FLOAT: float64 bits); where in_tags[i] is N1K_T_STRING the
 * string is bytes[offsets[i] - offsets[0], offsets[i + 1] - offsets[0]) (offsets: n + 1; needed by the string functions
 * only).  out_tags[i] / out_payload[i]: the call's value; out_raise[i] = 1 where a row holding the value raises (its value
 * is then NULL).  N1K_UNSUPPORTED for a call n1k_create refuses in a plan, N1K_INVALID for text that is no such call.
 */
n1k_status n1k_datefn_eval(const char *call_text, size_t len, uint64_t n, const uint8_t *in_tags, const uint64_t *in_payload,
                           const uint64_t *offsets, const char *bytes, uint8_t *out_tags, uint64_t *out_payload,
                           uint8_t *out_raise);
/* The same through the kernels on `device`: datefn_kernel for the millis functions — it has one flag for all rows, so
 * out_raise stays 0 and *out_any_raise says whether some value raised —, datestr_table_kernel for the string functions,
 * with out_raise per value; *out_left_to_host counts the strings of more than 64 bytes, which the kernel leaves to the host
 * evaluator.  The results are those of n1k_datefn_eval. */
n1k_status n1k_datefn_eval_device(int device, const char *call_text, size_t len, uint64_t n, const uint8_t *in_tags,
                                  const uint64_t *in_payload, const uint64_t *offsets, const char *bytes, uint8_t *out_tags,
                                  uint64_t *out_payload, uint8_t *out_raise, uint32_t *out_any_raise,
                                  uint64_t *out_left_to_host);
/* out[0] dictionary entries evaluated by datestr_table_kernel so far, out[1] by the host evaluator, out[2] distinct
 * str_to_millis / date_part_str terms of the plan, out[3] the number of new dictionary entries from which the device route
 * is taken */
n1k_status n1k_datefn_stats(const n1k_handle *h, uint64_t out[4]);

/* --------------------------------------------------------------------- IN -- */

/*
 * `a IN [c, c, ...]` over a list of constants (expression/coll_in.go:61-91) runs on the device.  The list falls apart by
 * type class, since Equals is FALSE across classes: its numbers are searched per row in a sorted array the handle keeps
 * in device memory (at most 1024 distinct numbers in the lists of one plan, each within +-2^53), its booleans and its
 * `null` are flags, and its STRINGS are one more predicate of the match table — "is this dictionary entry one of the
 * list's strings", one hash lookup per DISTINCT entry, one bit test per row.  A list that holds strings takes one of the
 * eight bits LIKE patterns and collection predicates share; at most 4096 distinct strings in one list.  The two entry
 * points below run the string matchers on their own (tests, diagnostics); n1k_in_stats says which route built a handle's table.
 *
 * n1k_in_match: the host matcher, no GPU needed.  list_text is the bracketed list alone, as expression/stringer.go writes
 * it (["a", "b"]) or as the JSON of a folded constant (["a","b"]); its elements that are not strings are parsed and
 * otherwise unused.  String i is bytes[offsets[i] - offsets[0], offsets[i + 1] - offsets[0]); out_bits[i] = 1 when the list
 * holds it, bytes compared as bytes.  N1K_UNSUPPORTED for a list n1k_create refuses in a plan, N1K_INVALID for text that
 * is no list.
 */
n1k_status n1k_in_match(const char *list_text, size_t len, uint64_t n, const uint64_t *offsets, const char *bytes,
                        uint8_t *out_bits);
/* The same through in_match_kernel on `device`.  *out_left_to_host counts the strings the kernel left to the host
 * matcher: exactly those longer than 128 bytes.  The results are those of n1k_in_match. */
n1k_status n1k_in_match_device(int device, const char *list_text, size_t len, uint64_t n, const uint64_t *offsets,
                               const char *bytes, uint8_t *out_bits, uint64_t *out_left_to_host);
/* out[0] distinct IN lists of the plan, out[1] dictionary strings looked up on the device so far, out[2] on the host,
 * out[3] the number of new dictionary entries from which the device route is taken */
n1k_status n1k_in_stats(const n1k_handle *h, uint64_t out[4]);

/* ------------------------------------------------------- string functions -- */

/*
 * A condition term over string functions of ONE leaf path (expression/func_str.go) runs on the device: the path wrapped in
 * up to four of lower (func_str.go:204), upper (:1155), trim / ltrim / rtrim with an optional constant cutset (:255-275,
 * :672-676, :1085-1089; default " \t\n\f\r", :301), then compared with STRING constants (=, <, <=, either side, BETWEEN),
 * matched by LIKE with a constant pattern or searched by contains (:81); or position / pos / position0 / pos0 / position1 /
 * pos1 (:1168-1177, func_registry.go:148-153) of the bare path compared with NUMBER constants.  Such a term is MISSING for
 * MISSING, NULL for a non-STRING and a plain boolean for a STRING — a function of the string alone, so it is one more
 * predicate of the match table: one evaluation per DISTINCT dictionary string, one bit test per row, one of the eight
 * bits the kinds share.  Under lower / upper every constant of the term must be pure ASCII; n1k_create answers
 * N1K_UNSUPPORTED for that and for length, substr, replace, regexp_* and the other string functions.  The two entry points
 * below run the evaluators on their own (tests, diagnostics); n1k_strfn_stats says which route built a handle's table.
 *
 * n1k_strfn_eval: the host evaluator, no GPU needed.  term_text is one whole term as expression/stringer.go writes it
 * ((lower((`d`.`name`)) like "%phone%"), contains((`d`.`s`), "amazon")); the path is parsed and otherwise unused.
 * String i is bytes[offsets[i] - offsets[0], offsets[i + 1] - offsets[0]); out_bits[i] = 1 when the term is TRUE for it.
 * N1K_UNSUPPORTED for a term n1k_create refuses in a plan, N1K_INVALID for text that is no such term.
 */
n1k_status n1k_strfn_eval(const char *term_text, size_t len, uint64_t n, const uint64_t *offsets, const char *bytes,
                          uint8_t *out_bits);
/* The same through strfn_match_kernel on `device`.  *out_left_to_host counts the strings the kernel left to the host
 * evaluator: longer than 128 bytes; holding U+0130 or U+212A under lower, U+017F or U+0131 under upper (the four
 * non-ASCII runes whose simple case mapping is ASCII); not valid UTF-8 under LIKE.  The results are those of
 * n1k_strfn_eval. */
n1k_status n1k_strfn_eval_device(int device, const char *term_text, size_t len, uint64_t n, const uint64_t *offsets,
                                 const char *bytes, uint8_t *out_bits, uint64_t *out_left_to_host);
/* out[0] dictionary strings evaluated on the device so far, out[1] on the host, out[2] distinct string-function
 * predicates of the plan, out[3] the number of new dictionary entries from which the device route is taken */
n1k_status n1k_strfn_stats(const n1k_handle *h, uint64_t out[4]);

/* Diagnostics: the bytes of device memory that the handles, communicators and calls of this process hold at this moment.
 * Exact (counted where the library allocates and frees, not read from the device, whose free memory moves under other
 * processes' work): back at its earlier value once everything created since then has been destroyed. */
uint64_t n1k_device_bytes_live(void);

/* ------------------------------------------------- multi-GPU (one per rank) -- */

/*
 * Hash-partition step of the 8-GPU path (no reference analogue: replaces the
 * Parallel -> IntermediateGroup fan-in, execution/exchange.go:161-251).
 * Evaluates the Filter on a device-resident batch and scatters every surviving
 * row's referenced columns into `nparts` (<= 64) regions by a hash of the group key VALUES.
 * Each column keeps its own layout, so the receiving rank can hand the received
 * buffers straight to n1k_push_device_batch of a handle built from the same plan
 * without its Filter.
 *
 * out_cols[c] are device buffers with room for `capacity_rows` rows per part
 * (part p starts at row p*capacity_rows); out_counts (device, nparts x u64)
 * receives the number of rows written to each part.
 */
n1k_status n1k_partition_device_batch(n1k_handle *h, const n1k_batch *batch, uint32_t nparts,
                                      uint64_t capacity_rows, const n1k_col *out_cols, uint64_t *out_counts);

/*
 * Partial groups (the reference's Initial -> Intermediate hand-over, algebra/aggregate.go:25-40).
 *
 * n1k_export_partials_device: write every group of the handle (packed key + raw accumulators) into `nparts`
 * regions of `out` (device memory) by a hash of the packed group key.  Region d (region_bytes = n1k_partial_region_bytes(h, capacity_groups)) is
 *     [count u64][verdict u64][keys: capacity x u64][accumulators: capacity x n1k_partial_words(h) x u64]
 * so that ONE all-to-all with equal splits moves all regions.  N1K_REGION_FULL when a region overflows; N1K_UNSUPPORTED
 * when the keys hold float / wide-integer values (their codes are local to the handle).
 *
 * n1k_export_partials_async: the same, ordered on the handle's stream with no host synchronisation.  The two
 * failures above are written into the `verdict` word of EVERY region instead (bit 0 overflow, bit 1 wide values),
 * so that each receiver learns them from the exchange itself: n1k_merge_partials_device then merges nothing and
 * the receiver's n1k_finish returns N1K_REGION_FULL / N1K_UNSUPPORTED — on all ranks alike, which lets them retry in step.
 *
 * n1k_merge_partials_device: ≙ CumulateIntermediate (execution/group_intermediate.go:91-101) over `nregions`
 * regions of that layout (device memory), e.g. what the all-to-all delivered.  The handle must have the same
 * plan, column kinds and dictionary as the exporters.  DISTINCT aggregates cannot be merged this way
 * (N1K_UNSUPPORTED): their sets would have to travel; use the row exchange instead.
 *
 * n1k_export_groups / n1k_merge_groups: the same through a host blob (one region), for merging operator copies
 * inside one process.
 */
uint32_t n1k_partial_words(const n1k_handle *h);
uint64_t n1k_partial_region_bytes(const n1k_handle *h, uint64_t capacity_groups);
n1k_status n1k_export_partials_device(n1k_handle *h, uint32_t nparts, uint64_t capacity_groups, void *out);
n1k_status n1k_export_partials_async(n1k_handle *h, uint32_t nparts, uint64_t capacity_groups, void *out);
n1k_status n1k_merge_partials_device(n1k_handle *h, uint32_t nregions, uint64_t capacity_groups, const void *in);
n1k_status n1k_export_groups(n1k_handle *h, const void **blob, size_t *len);

/*
 * The multi-GPU tail of ORDER BY ... OFFSET ... LIMIT: when groups are owned by several handles of the same plan and
 * dictionary (disjoint key ranges after the hash partition), each owner returns its first offset+limit rows and
 * rank 0 applies the plan's Order / Offset / Limit to their union (≙ execution/order.go:121-169 over the gathered rows).
 * Host only; `out` belongs to the handle like n1k_finish's.
 */
n1k_status n1k_order_rows(n1k_handle *h, uint64_t ngroups, const n1k_value *keys, const n1k_value *aggs, n1k_result *out);
n1k_status n1k_merge_groups(n1k_handle *h, const void *blob, size_t len);

/* ------------------------------------------ multi-GPU: RCCL collectives behind the ABI -- */

/*
 * One communicator per rank, one rank per GPU (no reference analogue: the reference is single-process and fans its
 * Parallel copies in through one in-memory queue, execution/exchange.go:161-251).  Rank 0 makes an id
 * (n1k_comm_unique_id, N1K_COMM_ID_BYTES bytes = ncclUniqueId), hands it to the other ranks by whatever channel the
 * host has, and every rank calls n1k_comm_create — a collective, like ncclCommInitRank.
 *
 * The exchange calls are collectives too: every rank makes the same call.  They are enqueued on the sending handle's
 * stream with no host synchronisation; the receiving handle's n1k_finish is the step's one wait.  Several exchanges may
 * be issued on one communicator per step (one per batch): each waits, on the device, for the owner's kernels that still
 * read the previous one's regions.
 *
 * Failures.  A rank never leaves its peers waiting in a collective:
 *   - whatever fails on a rank BEFORE the collective (a stopped operator, a batch that does not validate, buffers that
 *     cannot be allocated, the partition or the export itself) does not keep it from entering: it ships regions that
 *     hold only its n1k_status in their verdict word, returns that status from the exchange call, and every receiver's
 *     n1k_finish then fails with the same status;
 *   - what a sender's kernels find (a region that overflows: N1K_REGION_FULL; rows whose group key does not pack, values its
 *     Filter cannot order: N1K_UNSUPPORTED_DATA) travels in the same verdict word;
 *   in both cases the step is void on EVERY rank alike — n1k_failure_is_global(handle) says so after the failing call —
 *   and no rank goes on to n1k_gather_groups: all of them retry (N1K_REGION_FULL: with a larger capacity) or give up in step;
 *   - what fails on a rank AFTER the collective (the owner's InitialGroup / merge / n1k_finish over what it received) is
 *     that rank's alone: it enters n1k_gather_groups_status with its status, and every rank learns it there.
 * n1k_rows_step / n1k_partials_step run one whole step by these rules.  Not carried (the peers are left waiting; bound
 * such a wait with the host's own watchdog): a rank without a usable device, a rank that cannot allocate even one
 * region, and the first n1k_exchange_rows of a handle whose batch does not have the plan's column count / kinds (the
 * region size is a function of the column kinds; N1K_INVALID).  Nor is an exchange whose regions would not lie inside the
 * communicator's own buffers: every collective is handed the extents of its buffers and refuses such a call on the host
 * (N1K_INVALID, the message names the extents) instead of touching memory outside them — an error of the library, not of the
 * caller; over the loopback transport the peers' collective then fails with N1K_DEVICE_ERROR, over RCCL they are left waiting.
 *
 * n1k_exchange_partials: per-GPU partial groups (≙ the Initial -> Intermediate hand-over, algebra/aggregate.go:25-40):
 *   the sender's groups are exported (n1k_export_partials_async), moved by ONE collective — all-gather when `gathered`
 *   (every rank merges every rank's groups and ends with the whole result), else all-to-all of regions hash-partitioned
 *   on the group key (each key is merged and finished by one owner) — and merged into the receiver
 *   (n1k_merge_partials_device).  Not for plans with DISTINCT aggregates (sets do not travel).
 * n1k_exchange_rows: the sender evaluates its Filter over `batch` (device-resident) and scatters the survivors' columns
 *   by a hash of the group key VALUES into one packed region per destination rank ([count][verdict] header + every
 *   column's rows); ONE all-to-all moves counts and rows together; the receiver — a handle of the same plan without the
 *   Filter — runs InitialGroup over each received region, whose row count stays on the device.  Each group then
 *   lives on exactly one rank: COUNT(DISTINCT) needs no set merge.  capacity_rows: rows a region takes — like
 *   capacity_groups of n1k_exchange_partials it is part of the collective's shape and MUST be the same on every rank
 *   (agree on it with n1k_comm_max_u64, e.g. from the largest shard's row count; the regions are split into 8
 *   sub-regions with their own counts, which a receiver aggregates as one segmented batch).
 * n1k_gather_groups: every rank's finished groups (`local`, its n1k_finish result) to every rank with one all-gather of
 *   fixed-size slots (the slot size only changes on counts every rank reads in the gathered headers), then the handle's Order / Offset / Limit / projection over the union
 *   (≙ n1k_order_rows).  `out` belongs to the handle like n1k_finish's.
 */
#define N1K_COMM_ID_BYTES 128
typedef struct n1k_comm n1k_comm;
n1k_status n1k_comm_unique_id(void *id);
n1k_status n1k_comm_create(const void *id, int rank, int world, int device, n1k_comm **out);
/* Loopback transport: `world` communicators (out[0 .. world)) whose ranks are THREADS of this process sharing one device;
 * every collective is a rendezvous plus device-to-device copies.  For tests of the world_size > 1 paths on a single GPU
 * (RCCL refuses two ranks on one device) and for hosts that run several operator copies per GPU.  Each rank must be driven
 * from its own thread (a collective blocks until every rank has entered it). */
n1k_status n1k_comm_create_loopback(int world, int device, n1k_comm **out);
void n1k_comm_destroy(n1k_comm *c);
const char *n1k_comm_last_error(const n1k_comm *c);
int n1k_comm_rank(const n1k_comm *c);
int n1k_comm_world(const n1k_comm *c);
/* largest `value` over the ranks (a collective; waits): how the ranks agree on a region capacity from what each one holds */
n1k_status n1k_comm_max_u64(n1k_comm *c, n1k_handle *h, uint64_t value, uint64_t *out);
n1k_status n1k_exchange_partials(n1k_comm *c, n1k_handle *sender, n1k_handle *receiver, uint64_t capacity_groups, int gathered);
n1k_status n1k_exchange_rows(n1k_comm *c, n1k_handle *sender, const n1k_batch *batch, n1k_handle *receiver, uint64_t capacity_rows);
/* The same with one capacity PER DESTINATION (capacity_rows[world], the same vector on every rank): every sender's region for
 * owner d holds capacity_rows[d] rows, so an owner that receives more than its share (skewed keys) only enlarges the regions
 * sent to IT, not all world x world of them.  n1k_exchange_sent_rows: the rows this rank's last exchange wrote per destination
 * (waits for the stream); the ranks size the next steps' regions from the largest over the senders, per destination
 * (n1k_comm_max_u64_v: element-wise n1k_comm_max_u64 over n <= 64 values). */
n1k_status n1k_exchange_rows_v(n1k_comm *c, n1k_handle *sender, const n1k_batch *batch, n1k_handle *receiver,
                               const uint64_t *capacity_rows);
n1k_status n1k_exchange_sent_rows(n1k_comm *c, n1k_handle *sender, uint64_t *out);
n1k_status n1k_comm_max_u64_v(n1k_comm *c, n1k_handle *h, uint32_t n, const uint64_t *values, uint64_t *out);
n1k_status n1k_gather_groups(n1k_comm *c, n1k_handle *h, const n1k_result *local, n1k_result *out);
/* The same, carrying every rank's verdict on its own step: a rank whose n1k_finish failed (data its shard alone holds, say)
 * still enters the collective with local_status != N1K_OK (local may be NULL) instead of leaving its peers waiting in it;
 * every rank gets the first failing rank's status in *worst_status (N1K_OK: `out` holds the gathered groups). */
n1k_status n1k_gather_groups_status(n1k_comm *c, n1k_handle *h, const n1k_result *local, int local_status, n1k_result *out,
                                    int *worst_status);
/* 1 when the last failure reported on this handle (by an exchange call on a sender, by n1k_finish on a receiver) was told
 * to / learnt from the verdict words of an exchange: every rank's step failed alike and no rank enters the gather. */
int n1k_failure_is_global(const n1k_handle *h);
/* One whole step of the row exchange in one call: n1k_reset(receiver), n1k_reset(sender), n1k_exchange_rows,
 * n1k_finish(receiver), n1k_gather_groups_status(merger) — what a host runs per query.  A failure with
 * n1k_failure_is_global(receiver) or n1k_failure_is_global(sender): the step is void on every rank alike and no gather took
 * place (N1K_REGION_FULL: a region overflowed — enlarge capacity_rows on every rank and repeat); otherwise the rank's own status,
 * with *worst_status as n1k_gather_groups_status reports it. */
n1k_status n1k_rows_step(n1k_comm *c, n1k_handle *sender, const n1k_batch *batch, n1k_handle *receiver, n1k_handle *merger,
                         uint64_t capacity_rows, n1k_result *out, int *worst_status);
n1k_status n1k_rows_step_v(n1k_comm *c, n1k_handle *sender, const n1k_batch *batch, n1k_handle *receiver, n1k_handle *merger,
                           const uint64_t *capacity_rows, n1k_result *out, int *worst_status); /* capacities per destination */
/* The same for partial groups: n1k_reset(receiver), n1k_reset(sender), n1k_push_device_batch(sender, batch) (InitialGroup
 * over the shard), n1k_exchange_partials, n1k_finish(receiver) and — unless `gathered`, where every rank merged every rank's
 * groups and `receiver` (a handle that carries the plan's grouped tail) holds the result — the gather through `merger`. */
n1k_status n1k_partials_step(n1k_comm *c, n1k_handle *sender, const n1k_batch *batch, n1k_handle *receiver, n1k_handle *merger,
                             uint64_t capacity_groups, int gathered, n1k_result *out, int *worst_status);

/* ------------------------------------------------------------- utilities -- */

/* Device-side synthetic column generator of SURVEY.md §8(d) (bench/test input;
 * the same generator exists on the CPU in oracle/ for parity).  All outputs are
 * device pointers with room for nrows elements; any may be NULL. */
typedef struct n1k_synth_spec {
    uint64_t seed;
    uint64_t first_row;  /* global ordinal of row 0 of this call (sharding) */
    uint64_t nrows;
    uint64_t total_rows; /* N of the whole data set (user_id range = N/10) */
    uint32_t k_cat;      /* number of categories */
    uint32_t zipf;       /* 0 = uniform, 1 = Zipf(s=1) via cdf */
    const double *cat_cdf; /* device pointer, k_cat entries, only for zipf */
} n1k_synth_spec;
n1k_status n1k_synth_columns(int device, void *stream, const n1k_synth_spec *spec, uint32_t *cat_codes,
                             uint8_t *price_tags, uint64_t *price_payload, uint8_t *user_tags,
                             uint64_t *user_payload, uint8_t *region_tags, uint64_t *region_payload);

/* The same rows as raw JSON documents (bench / test input for n1k_push_json): from HOST copies of the arrays
 * n1k_synth_columns filled, document i = {"id":"d<i>","cat":"cat_<c>","price":<p>,"user_id":<u>,"region_id":<r>,"pad":"x..."}
 * (a MISSING value leaves its field out, NULL prints null, floats print their shortest round-trip digits; `pad` x's).
 * offsets: nrows + 1 entries.  N1K_OOM: `cap` bytes do not hold them (*used then says how many it takes). */
n1k_status n1k_synth_documents(uint64_t nrows, uint64_t first_id, const uint32_t *cat_codes, const uint8_t *price_tags,
                               const uint64_t *price_payload, const uint64_t *user_payload, const uint64_t *region_payload,
                               uint32_t pad, char *bytes, size_t cap, uint64_t *offsets, size_t *used);

int n1k_abi_version(void);
/* number of visible HIP devices (0 when none); never initialises a context */
int n1k_device_count(void);

#ifdef __cplusplus
}
#endif
#endif /* N1K_H */
