// n1k_cond.h — CASE and the conditional functions as VALUES: the program of one conditional node ("CASE and
// the conditional functions").  A node is a derived column like an arithmetic node (n1k_handle::Derived, op AR_COND): its
// operands are input columns, constants or EARLIER derived columns, and cond_kernel (n1k_kernels.hip) writes the chosen
// operand's tag and payload, one row per lane, into the node's TAGGED64 column.
//
//   COND_CASE             searched CASE (expression/case_searched.go:73-100): the arms in order, the first whose WHEN is TRUE
//                         gives its THEN; none: ELSE, and without one NULL.  A simple CASE (case_simple.go:78-110) is the
//                         same node with TERM_EQ(search, when_k) as arm k's condition.
//   COND_IFMISSING        the first operand that is not MISSING          (func_cond_unknown.go:61-69)
//   COND_IFNULL           the first operand that is not NULL — a MISSING one IS returned   (:132-140)
//   COND_IFMISSINGORNULL  the first operand above NULL                    (:209-217);  none in all three: NULL
//   COND_NULLIF           eq = a.Equals(b): MISSING / NULL -> eq, TRUE -> NULL, else a      (:278-290)
//   COND_MISSINGIF        ... TRUE -> MISSING                                               (:347-359)
//   COND_NANIF / COND_POSINFIF / COND_NEGINFIF   ... TRUE -> FLOAT NaN / +Inf / -Inf   (func_cond_num.go:293-305 and siblings)
//
// The WHEN conditions are compiled by compile_cond, the Filter's own compiler, into the node's terms and postfix logic,
// and evaluated by eval_term and the logic_* helpers, the Filter's own evaluator: a WHEN answers what the Filter answers.
#pragma once
#include "n1k_types.h"

namespace n1k {

// Choices, not measurements: a node of this size is 1.7 KiB of wave-uniform data that stays in the scalar cache.
constexpr int kCondMaxArms = 8;     // WHEN arms of a CASE (the functions take 2 to 4 operands, one per arm)
constexpr int kCondMaxTerms = 16;   // predicate terms of all WHEN conditions of one node
constexpr int kCondMaxLogic = 32;   // postfix logic ops of all WHEN conditions of one node

enum : uint32_t { COND_CASE = 0, COND_IFMISSING, COND_IFNULL, COND_IFMISSINGORNULL, COND_NULLIF, COND_MISSINGIF,
                  COND_NANIF, COND_POSINFIF, COND_NEGINFIF };
constexpr bool cond_is_eq_mode(uint32_t m) { return m == COND_NULLIF || m == COND_MISSINGIF || m == COND_NANIF || m == COND_POSINFIF || m == COND_NEGINFIF; }

struct CondArm {
    uint32_t logic_begin, logic_end;  // COND_CASE / NULLIF / MISSINGIF: the arm's condition, logic[logic_begin .. logic_end)
    Operand then;                     // what the arm gives (IF*: the operand that is tested and given)
};

struct CondNode {
    uint32_t mode, narms, nterms, nlogic;
    uint32_t has_else, pad;
    Operand els;
    CondArm arms[kCondMaxArms];
    Term terms[kCondMaxTerms];
    LogicOp logic[kCondMaxLogic];
};

// Where compile_cond writes: the Filter's program, or a conditional node's own arrays.
struct CondTarget {
    Term* terms;
    LogicOp* logic;
    uint32_t* nterms;
    uint32_t* nlogic;
    uint32_t max_terms, max_logic;
    bool in_node;  // a WHEN of a conditional node: no match-table terms (their bits are laid out over the Filter's program only)
};

struct CondArgs {
    const CondNode* node;  // device memory, uploaded once per plan
    uint64_t nrows;
    // Which of the nrows rows the batch really holds, as the scan kernels take it (FastArgs / ScanArgs): min(nrows, *nrows_dev)
    // when set; with nseg > 1, segments of seg_rows rows capacity holding seg_counts[s * kCursorStride] rows each (a row
    // region received from another GPU).  The other rows are not evaluated: what they hold is not data.
    const unsigned long long* nrows_dev;
    const unsigned long long* seg_counts;
    uint64_t seg_rows;
    uint32_t nseg, pad;
    uint8_t* out_tags;
    uint64_t* out_payload;
    uint32_t* err_flags;
};

}  // namespace n1k
