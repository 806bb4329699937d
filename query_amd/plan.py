"""Host-side mirror of the reference's plan nodes for the hot path.

Same names and JSON shapes as plan/filter.go:46-53, plan/group.go:54-70,
plan/sequence.go:48-57 and plan/parallel.go:54-67, so a plan built here is
byte-compatible with what the reference planner marshals (EXPLAIN golden:
test/filestore/json/default/cases/case_by_id.json:369-456).  Expressions are
expression.Stringer text.
"""
from __future__ import annotations

import json
from dataclasses import dataclass, field
from typing import List, Optional, Sequence


def field_path(alias: str, *names: str) -> str:
    """Stringer text of a field navigation: field_path("default", "price") -> (`default`.`price`)"""
    s = "`%s`" % alias
    for n in names:
        s = "(%s.`%s`)" % (s, n)
    return s


def in_list(path: str, values: Sequence) -> str:
    """Stringer text of `path IN [values]` over constants (stringer.go VisitIn, VisitArrayConstruct):
    in_list(field_path("d", "cat"), ["a", 3, None]) -> ((`d`.`cat`) in ["a", 3, null]).  Values: str, int, float, bool,
    None (null).  Negative numbers come out in parentheses, as the reference writes a negation."""
    def const(v):
        if isinstance(v, (str, bool)) or v is None:
            return json.dumps(v, ensure_ascii=False)
        if isinstance(v, (int, float)):
            t = json.dumps(v)
            return "(%s)" % t if t.startswith("-") else t
        raise TypeError("in_list takes str, int, float, bool and None, not %r" % (v,))
    return "(%s in [%s])" % (path, ", ".join(const(v) for v in values))


def case_when(arms: Sequence[tuple], else_: Optional[str] = None) -> str:
    """Stringer text of a searched CASE (stringer.go VisitSearchedCase): arms = [(condition text, value text)];
    case_when([("(50 < (`d`.`price`))", "(`d`.`price`)")], "0") -> case when (50 < (`d`.`price`)) then (`d`.`price`) else 0 end.
    The operands are expression text already (field_path, a JSON constant, arithmetic in parentheses, another case_when)."""
    if not arms:
        raise ValueError("a CASE needs at least one WHEN arm")
    s = "case" + "".join(" when %s then %s" % (w, t) for w, t in arms)
    return s + (" else %s" % else_ if else_ is not None else "") + " end"


def case_of(search: str, arms: Sequence[tuple], else_: Optional[str] = None) -> str:
    """Stringer text of a simple CASE (VisitSimpleCase): case <search> when <value> then <value> ... [else <value>] end."""
    if not arms:
        raise ValueError("a CASE needs at least one WHEN arm")
    s = "case %s" % search + "".join(" when %s then %s" % (w, t) for w, t in arms)
    return s + (" else %s" % else_ if else_ is not None else "") + " end"


COND_FUNCTIONS = ("ifmissing", "ifnull", "ifmissingornull", "nullif", "missingif",  # expression/func_registry.go:321-325
                  "nanif", "posinfif", "neginfif")  # :337-339 (func_cond_num.go): Equals, like nullif, giving NaN / +Inf / -Inf

# expression/func_registry.go:191-219, 334-336 -> (least, most) arguments.  Values, usable wherever round(...) is.
NUM_FUNCTIONS = {"acos": (1, 1), "asin": (1, 1), "atan": (1, 1), "cos": (1, 1), "sin": (1, 1), "tan": (1, 1), "exp": (1, 1), "ln": (1, 1),
                 "log": (1, 1), "degrees": (1, 1), "radians": (1, 1), "atan2": (2, 2), "power": (2, 2),
                 "pi": (0, 0), "e": (0, 0), "nan": (0, 0), "posinf": (0, 0), "neginf": (0, 0),
                 "ifinf": (2, 4), "ifnan": (2, 4), "ifnanorinf": (2, 4)}


def num_fn(name: str, *args: str) -> str:
    """Stringer text of a numeric function (VisitFunction): num_fn("power", "(`d`.`x`)", "2") -> power((`d`.`x`), 2);
    num_fn("pi") -> pi().  ln is the natural logarithm and log the decimal one; ifinf / ifnan / ifnanorinf take 2 to 4
    arguments on the device."""
    lo_hi = NUM_FUNCTIONS.get(name.lower())
    if lo_hi is None:
        raise ValueError("num_fn takes one of %s, not %r" % (", ".join(sorted(NUM_FUNCTIONS)), name))
    if not lo_hi[0] <= len(args) <= lo_hi[1]:
        raise ValueError("%s takes %d to %d arguments, not %d" % (name, lo_hi[0], lo_hi[1], len(args)))
    return "%s(%s)" % (name.lower(), ", ".join(args))


# expression/func_registry.go:111-135 -> (least, most) arguments: the date functions the device evaluates
DATE_FUNCTIONS = {"date_part_millis": (2, 3), "date_trunc_millis": (2, 2), "date_add_millis": (3, 3), "str_to_millis": (1, 1), "date_part_str": (2, 2)}
DATE_PARTS = ("millennium", "century", "decade", "year", "quarter", "month", "week", "day", "hour", "minute", "second", "millisecond",
              "day_of_year", "doy", "day_of_week", "dow", "iso_week", "iso_year", "iso_dow", "timezone", "timezone_hour", "timezone_minute")


def date_fn(name: str, *args: str) -> str:
    """Stringer text of a date function (VisitFunction): date_fn("date_trunc_millis", "(`d`.`ts`)", '"day"') ->
    date_trunc_millis((`d`.`ts`), "day").  The arguments are expression text already; the part is a STRING constant
    (date_part("day") writes one), date_part_millis's optional third argument the constant "UTC"."""
    lo_hi = DATE_FUNCTIONS.get(name.lower())
    if lo_hi is None:
        raise ValueError("date_fn takes one of %s, not %r" % (", ".join(sorted(DATE_FUNCTIONS)), name))
    if not lo_hi[0] <= len(args) <= lo_hi[1]:
        raise ValueError("%s takes %d to %d arguments, not %d" % (name, lo_hi[0], lo_hi[1], len(args)))
    return "%s(%s)" % (name.lower(), ", ".join(args))


def date_part(part: str) -> str:
    """A date part as the STRING constant a date function takes: date_part("iso_week") -> "iso_week" (quoted)."""
    if part.lower() not in DATE_PARTS:
        raise ValueError("date part %r: one of %s" % (part, ", ".join(DATE_PARTS)))
    return json.dumps(part)


def cond_fn(name: str, *args: str) -> str:
    """Stringer text of a conditional function (VisitFunction): cond_fn("ifmissing", "(`d`.`x`)", "0") -> ifmissing((`d`.`x`), 0)."""
    if name.lower() not in COND_FUNCTIONS:
        raise ValueError("cond_fn takes one of %s, not %r" % (", ".join(COND_FUNCTIONS), name))
    return "%s(%s)" % (name.lower(), ", ".join(args))


@dataclass
class Filter:
    condition: str

    def marshal(self) -> dict:
        return {"#operator": "Filter", "condition": self.condition}


@dataclass
class InitialGroup:
    group_keys: List[str] = field(default_factory=list)
    aggregates: List[str] = field(default_factory=list)

    def marshal(self) -> dict:
        # aggregates are de-duplicated and sorted by text, as planner/build_select_sub.go:551-558 does
        return {"#operator": "InitialGroup", "aggregates": list(self.aggregates), "group_keys": list(self.group_keys)}


@dataclass
class IntermediateGroup(InitialGroup):
    def marshal(self) -> dict:
        d = super().marshal()
        d["#operator"] = "IntermediateGroup"
        return d


@dataclass
class FinalGroup(InitialGroup):
    def marshal(self) -> dict:
        d = super().marshal()
        d["#operator"] = "FinalGroup"
        return d


@dataclass
class Sequence:
    children: Sequence[object]

    def marshal(self) -> dict:
        return {"#operator": "Sequence", "~children": [c.marshal() for c in self.children]}


@dataclass
class Parallel:
    child: object
    max_parallelism: int = 0

    def marshal(self) -> dict:
        d = {"#operator": "Parallel", "~child": self.child.marshal()}
        if self.max_parallelism:
            d["maxParallelism"] = self.max_parallelism
        return d


@dataclass
class Order:
    """plan/order.go:51-79: sort_terms [{expr, desc?}], optional offset / limit expression strings."""
    sort_terms: Sequence[tuple]  # (expression text, descending)
    offset: Optional[int] = None
    limit: Optional[int] = None

    def marshal(self) -> dict:
        terms = []
        for expr, desc in self.sort_terms:
            t = {"expr": expr}
            if desc:
                t["desc"] = True
            terms.append(t)
        d = {"#operator": "Order", "sort_terms": terms}
        if self.offset is not None:
            d["offset"] = str(int(self.offset))
        if self.limit is not None:
            d["limit"] = str(int(self.limit))
        return d


@dataclass
class Limit:
    expr: int

    def marshal(self) -> dict:
        return {"#operator": "Limit", "expr": str(int(self.expr))}


@dataclass
class Offset:
    expr: int

    def marshal(self) -> dict:
        return {"#operator": "Offset", "expr": str(int(self.expr))}


@dataclass
class InitialProject:
    """plan/project.go:73-110: result_terms [{expr, as?}], distinct (star / raw projections are not built here)."""
    result_terms: Sequence[tuple]  # (expression text, alias or None)
    distinct: bool = False

    def marshal(self) -> dict:
        terms = []
        for expr, alias in self.result_terms:
            t = {"expr": expr}
            if alias:
                t["as"] = alias
            terms.append(t)
        d = {"#operator": "InitialProject", "result_terms": terms}
        if self.distinct:  # (plan/project.go:84-86: marshalled only when set)
            d["distinct"] = True
        return d


@dataclass
class Distinct:
    """plan/distinct.go:32-40: no data; the set is keyed by the projection the InitialProject before it attached."""

    def marshal(self) -> dict:
        return {"#operator": "Distinct"}


@dataclass
class FinalProject:
    def marshal(self) -> dict:
        return {"#operator": "FinalProject"}


def marshal_json(op) -> str:
    return json.dumps(op.marshal(), sort_keys=True)


def filter_group_plan(condition: Optional[str], group_keys: Optional[Sequence[str]],
                      aggregates: Optional[Sequence[str]], *, filter_only: bool = False,
                      order: Optional[Sequence[tuple]] = None, limit: Optional[int] = None,
                      offset: Optional[int] = None, having: Optional[str] = None,
                      project: Optional[Sequence[tuple]] = None, distinct: Optional[Sequence[tuple]] = None) -> str:
    """Plan JSON of Parallel{Sequence[Filter?, InitialGroup?]} as the planner emits it
    (planner/build_select_sub.go:209-211, 276-296).  With `order` / `limit` / `offset` the whole grouped tail
    follows: IntermediateGroup, FinalGroup, Order (which carries offset and limit, plan/order.go:51-79), Offset,
    Limit (planner/build_select.go) — the sort terms must be group keys or aggregates of the plan.  With `filter_only`
    the same three follow the Filter directly, over the rows it selects: `order` = [(leaf path of the row, descending)],
    1 to 4 terms; n1k_filter_device_batch then returns the selection ordered and cut.  With `filter_only` and `distinct` =
    [(leaf path of the row, alias or None)], 1 to 4 terms, it is SELECT DISTINCT over the rows (planner/build_select_sub.go:
    217-240): InitialProject{distinct}, Distinct and FinalProject follow the Filter inside the Parallel, the serial Distinct, the
    tail and the last FinalProject come behind it; a sort term may then name a term by `alias`."""
    children: List[object] = []
    if condition:
        children.append(Filter(condition))
    if distinct is not None:
        if not filter_only or having is not None or project is not None:
            raise ValueError("distinct goes with filter_only, without having / project")
        children += [InitialProject(list(distinct), distinct=True), Distinct(), FinalProject()]
        tail = [Parallel(Sequence(children)), Distinct()]
        if order:
            tail.append(Order(list(order), offset, limit))
        if offset is not None:
            tail.append(Offset(offset))
        if limit is not None:
            tail.append(Limit(limit))
        return marshal_json(Sequence(tail + [FinalProject()]))
    if not filter_only:
        children.append(InitialGroup(list(group_keys or []), list(aggregates or [])))
    par = Parallel(Sequence(children))
    if order is None and limit is None and offset is None and having is None and project is None:
        return marshal_json(par)
    if filter_only:
        # a Filter-only plan: Order / Offset / Limit over the rows it selects; the sort terms are leaf paths of the row
        # (the caller projects with n1k_gather_selected: no InitialProject here)
        if having is not None or project is not None:
            raise ValueError("a Filter-only plan takes order / offset / limit, not having / project")
        tail: List[object] = [par]
    else:
        tail = [par, IntermediateGroup(list(group_keys or []), list(aggregates or [])),
                FinalGroup(list(group_keys or []), list(aggregates or []))]
    if project is not None:
        # HAVING and the projection share the Parallel after FinalGroup (planner/build_select_sub.go:217-235, :295);
        # `project` = [(expression text, alias or None)]
        sub: List[object] = ([Filter(having)] if having is not None else []) + [InitialProject(list(project))]
        tail.append(Parallel(Sequence(sub)))
    elif having is not None:  # HAVING is a Filter over the final groups (planner/build_select_sub.go:295)
        tail.append(Filter(having))
    if order:
        tail.append(Order(list(order), offset, limit))
    else:
        if offset is not None:
            tail.append(Offset(offset))
        if limit is not None:
            tail.append(Limit(limit))
    if project is not None:
        tail.append(FinalProject())
    return marshal_json(Sequence(tail))
