// n1k_plan.h — host side: the reference's plan JSON and expression.Stringer text -> compiled plan.
//
// Mirrors, for the hot path only, what plan.(*Filter).UnmarshalJSON (plan/filter.go:55-71) and
// plan.(*InitialGroup).UnmarshalJSON (plan/group.go:72-103) do with expression/parser: parse the
// stringified expressions back into trees.  Anything outside the device subset is reported as
// "unsupported" so that the caller keeps the reference operators (N1K_UNSUPPORTED).
#pragma once
#include <cstdint>
#include <memory>
#include <string>
#include <vector>
#include "n1k_types.h"

namespace n1k {

struct PlanError {
    bool unsupported = false;  // valid but outside the device subset
    std::string msg;
};

// expression tree (subset of expression/*.go)
enum class EK {
    Const, Path, Add, Sub, Mult, Div, Mod, Neg, IDiv, IMod, Eq, LT, LE, Between, And, Or, Not,
    IsNull, IsNotNull, IsMissing, IsNotMissing, IsValued, IsNotValued,
    Like,  // (a like b), expression/comp_like.go; NOT LIKE arrives as (not (a like b))
    Coll,  // any | every | any and every `v` in <leaf path> satisfies <P> end (expression/coll_any.go, coll_every.go,
           // coll_any_every.go): ch[0] the binding expression, coll_* the rest
    In,    // (a in [c, c, ...]), expression/coll_in.go, over a constant list: ch[0] the left operand, ch[1..] the elements
           // (Const), `text` the bracketed list as the stringer wrote it; NOT IN arrives as (not (a in [...]))
    Case,  // case [search] when .. then .. [else ..] end (expression/case_searched.go, case_simple.go): ch = [search] (when, then)*
           // [else], case_simple / case_else say which of the optional ones are there
    Func  // numeric functions of one or two arguments (expression/func_num.go) and the string functions a term may hold
          // (expression/func_str.go; n1k_strfn.h), and the conditional functions ifmissing / ifnull / ifmissingornull / nullif /
          // missingif (expression/func_cond_unknown.go), the library functions acos ... power (func_num.go; pi() / e() / nan() /
          // posinf() / neginf() parse to Const) and ifinf / ifnan / ifnanorinf / nanif / posinfif / neginfif (func_cond_num.go), and
          // array_length / array_count / array_sum / array_avg / array_contains / array_position over a leaf path (expression/
          // func_array.go; n1k_arrfn.h; `text` is then the whole term as the stringer wrote it): fname
};

struct Expr {
    EK kind;
    std::vector<std::unique_ptr<Expr>> ch;
    // Const
    uint32_t ctag = T_NULL;
    uint64_t cpayload = 0;   // INT: int64, FLOAT: bits; STRING: filled with the dictionary code at bind time
    std::string cstr;        // STRING constant bytes
    // Path
    std::string text;        // exact stringer text, e.g. (`default`.`price`)
    // Func
    std::string fname;       // round | trunc | abs | ceil | floor | sign | sqrt | greatest | least | lower | upper | trim | ltrim |
                             // rtrim | contains | position[0|1] | pos[0|1] | ifmissing | ifnull | ifmissingornull | nullif | missingif
                             // | acos | asin | atan | cos | sin | tan | exp | ln | log | degrees | radians | atan2 | power | ifinf | ifnan |
                             // ifnanorinf | nanif | posinfif | neginfif
    // Case
    bool case_simple = false, case_else = false;
    // Coll: `text` is the whole term as the stringer wrote it.  The SATISFIES tree is kept apart from ch: its paths name
    // the bound variable, not the row, so collect_paths must not meet them.
    uint32_t coll_mode = 0;  // COLL_ANY | COLL_EVERY | COLL_ANY_EVERY (n1k_coll.h)
    std::string coll_var;    // the bound variable
    std::unique_ptr<Expr> coll_pred;
};

struct AggDef {
    uint32_t kind;  // AGG_*
    bool distinct = false;
    std::unique_ptr<Expr> operand;  // null for count(*)
    std::string text;               // agg.String(): key of the reference's "aggregates" attachment map
};

// one ORDER BY term over the groups (plan/order.go:51-79): its expression must be, text for text, one of the group
// keys or one of the aggregates (the Go glue resolves projection aliases before handing the plan over)
struct OrderTerm {
    std::string text;
    bool desc = false;
    int key_index = -1;  // >= 0: group key
    int agg_index = -1;  // >= 0: aggregate
    int proj_index = -1; // >= 0: a projection term (by its alias, or by its expression text)
};

// one ORDER BY term over the rows of a Filter-only plan: a leaf path of the row, in the text form a Filter condition uses
constexpr uint32_t kOrderMaxTerms = 4;
struct RowOrderTerm {
    std::string text;
    bool desc = false;
    int col = -1;  // its column: index into ParsedPlan::paths
};

// one result term of SELECT DISTINCT over the rows of a plan without a group (InitialProject{"distinct":true} + Distinct,
// plan/project.go:69-108, plan/distinct.go:32-40): a leaf path of the row, like a sort term
constexpr uint32_t kDistinctMaxTerms = 4;
struct RowDistinctTerm {
    std::string text;
    std::string as;  // explicit alias ("" = none)
    int col = -1;    // its column: index into ParsedPlan::paths
};

// one result term of the InitialProject after the group operators (plan/project.go:73-110): its expression reads group
// keys and aggregates (algebra/aggregate.go:97-118 looks an aggregate up by its text in the "aggregates" attachment)
struct ProjectTerm {
    std::string text;  // expression.Stringer text
    std::string as;    // explicit alias ("" = none: the caller derives one as algebra.ResultTerm does)
};

struct ParsedPlan {
    bool has_filter = false;
    bool has_group = false;
    std::unique_ptr<Expr> condition;
    std::vector<std::unique_ptr<Expr>> keys;
    std::vector<std::string> key_texts;  // stringer text of every group key
    std::vector<AggDef> aggs;
    std::vector<std::string> paths;  // distinct leaf paths in column order
    int max_parallelism = 0;
    // Order / Offset / Limit over the final groups (execution/order.go, order_limit.go, offset.go, limit.go)
    bool has_order = false;
    std::vector<OrderTerm> order;
    int64_t limit = -1;  // < 0: none
    int64_t offset = 0;
    // Order over the ROWS a Filter-only plan selects (no group): 1 to kOrderMaxTerms leaf paths; limit / offset above then cut
    // the ordered (without Order: the ascending) selection
    std::vector<RowOrderTerm> row_order;
    bool ordered_rows() const { return !has_group && (!row_order.empty() || limit >= 0 || offset > 0); }
    // SELECT DISTINCT over the rows (no group): the InitialProject's 1 to kDistinctMaxTerms leaf paths, and whether the Distinct
    // operator followed it (the parallel and the serial Distinct of the planner fold into one); Order / Offset / Limit come after
    std::vector<RowDistinctTerm> row_distinct;
    bool has_row_distinct = false;
    // HAVING: a Filter after the group operators (planner/build_select_sub.go:295), over group keys and aggregates
    bool has_having = false;
    std::string having_text;
    // InitialProject / FinalProject over the final groups (execution/project_initial.go:52-144, project_final.go:51-59)
    bool has_project = false;
    std::vector<ProjectTerm> project;
};

// Parse plan JSON (Sequence / Parallel / Filter / InitialGroup nodes, optionally followed by IntermediateGroup /
// FinalGroup — which the device operator subsumes — and Order / Offset / Limit over the groups; or, without a group,
// Filter? / InitialProject{distinct} / Distinct / Order / Offset / Limit over the rows).  Returns false and fills err on failure.
bool parse_plan_json(const char* json, size_t len, ParsedPlan& out, PlanError& err);

// Parse one stringified expression / aggregate.
std::unique_ptr<Expr> parse_expression(const std::string& s, PlanError& err);
bool parse_aggregate(const std::string& s, AggDef& out, PlanError& err);

// value.Collate of two arrays / objects given as canonical JSON text (numbers through float64); false when a text does
// not parse
bool json_text_collate(const std::string& a, const std::string& b, int& out);

}  // namespace n1k
