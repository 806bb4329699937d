"""SELECT DISTINCT over the rows of a Filter-only plan, the part that needs no GPU: the plan contract (what n1k_create accepts,
in which order it reports column paths and projection terms, what it refuses and how), what plan.filter_group_plan marshals,
and the reference of tests/test_gpu_distinct_rows.py (distinct_util) against the reference's own results and against the
equality rules of n1k.h, pair by pair."""
import ctypes as C
import itertools
import json

import numpy as np
import pytest

import distinct_util as du
import golden_util as gu
import order_util as ou
import query_amd
from query_amd import _ffi, plan

D = lambda *n: plan.field_path("default", *n)
PRICE, CAT, A, B, X, Y = D("price"), D("cat"), D("a"), D("b"), D("x"), D("y")
COND = "(50 < %s)" % PRICE


def distinct(terms, cond=COND, **kw):
    return plan.filter_group_plan(cond, [], [], filter_only=True, distinct=terms, **kw)


def refused(pj):
    with pytest.raises(query_amd.N1kError) as ei:
        query_amd.GpuFilterGroup(pj if isinstance(pj, str) else json.dumps(pj))
    return ei.value


def node(op, **kw):
    return dict({"#operator": op}, **kw)


def project(terms, **kw):
    return node("InitialProject", distinct=True, result_terms=[dict({"expr": e}, **({"as": a} if a else {})) for e, a in terms], **kw)


FILTER = node("Filter", condition=COND)


# ------------------------------------------------------------------------------------------------ 1. accepted forms
@pytest.mark.parametrize("terms,kw,paths", [
    ([(CAT, None)], {}, [PRICE, CAT]),                                                   # the condition's path, then the term's
    ([(PRICE, "p")], {}, [PRICE]),                                                       # the condition's own path: no new column
    ([(A, None), (CAT, "c"), (A, "again"), (B, None)], {}, [PRICE, A, CAT, B]),          # 4 terms, none twice
    ([(CAT, None)], {"order": [(X, True), (CAT, False)]}, [PRICE, CAT, X]),              # terms before the sort terms
    ([(CAT, "c"), (A, None)], {"order": [("`c`", False)], "offset": 2, "limit": 5}, [PRICE, CAT, A]),  # an alias names a term
    ([(CAT, None)], {"limit": 3}, [PRICE, CAT]),
    ([(CAT, None)], {"offset": 3}, [PRICE, CAT]),
])
def test_accepted_forms_their_column_paths_and_terms(terms, kw, paths):
    pj = distinct(terms, **kw)
    top = json.loads(pj)["~children"]
    inner = [c["#operator"] for c in top[0]["~child"]["~children"]]
    assert inner == ["Filter", "InitialProject", "Distinct", "FinalProject"]
    assert [c["#operator"] for c in top][:2] == ["Parallel", "Distinct"] and top[-1]["#operator"] == "FinalProject"
    op = query_amd.GpuFilterGroup(pj)
    assert op.column_paths == paths
    assert op.projection_terms == [(e, a or "") for e, a in terms]
    assert op.num_keys == 0 and op.aggregate_names == []
    op.done()


@pytest.mark.parametrize("pj,paths", [
    (node("Sequence", **{"~children": [FILTER, project([(CAT, None)]), node("Distinct")]}), [PRICE, CAT]),            # bare
    (node("Sequence", **{"~children": [project([(CAT, None)]), node("Distinct")]}), [CAT]),                            # no Filter
    (node("Parallel", **{"~child": node("Sequence", **{"~children": [project([(CAT, "c")]), node("Distinct"), node("FinalProject")]})}), [CAT]),
    (node("Sequence", **{"~children": [project([(CAT, None), (A, None)]), node("Distinct"), node("Distinct"),
                                       node("Order", sort_terms=[{"expr": A, "desc": True}]), node("Offset", expr="1"), node("Limit", expr="2")]}), [CAT, A]),
])
def test_bare_forms_and_plans_without_filter(pj, paths):
    op = query_amd.GpuFilterGroup(json.dumps(pj))
    assert op.column_paths == paths and [e for e, _ in op.projection_terms] == [p for p in paths if p != PRICE]
    op.done()


def test_an_alias_sort_term_resolves_to_its_terms_path():
    # explicit alias; the alias the reference derives from a path's last name; a leaf path as before
    for order, paths in (([("`k`", True)], [PRICE, CAT]), ([("`cat`", False)], [PRICE, CAT]), ([(CAT, False)], [PRICE, CAT]),
                         ([("`nobody`", False)], [PRICE, CAT, "`nobody`"])):
        alias = "k" if order[0][0] == "`k`" else None
        op = query_amd.GpuFilterGroup(distinct([(CAT, alias)], order=order))
        assert op.column_paths == paths, order
        op.done()
    # an explicit alias hides the derived one
    op = query_amd.GpuFilterGroup(distinct([(CAT, "k")], order=[("`cat`", False)]))
    assert op.column_paths == [PRICE, CAT, "`cat`"]
    op.done()


def test_filter_group_plan_marshals_what_the_reference_marshals():
    got = json.loads(distinct([(CAT, None), (A, "x")], order=[("`x`", True)], offset=1, limit=2))
    want = node("Sequence", **{"~children": [
        node("Parallel", **{"~child": node("Sequence", **{"~children": [
            FILTER, node("InitialProject", distinct=True, result_terms=[{"expr": CAT}, {"expr": A, "as": "x"}]), node("Distinct"), node("FinalProject")]})}),
        node("Distinct"), node("Order", sort_terms=[{"expr": "`x`", "desc": True}], offset="1", limit="2"),
        node("Offset", expr="1"), node("Limit", expr="2"), node("FinalProject")]})
    assert got == want
    assert plan.Distinct().marshal() == {"#operator": "Distinct"}
    assert "distinct" not in plan.InitialProject([(CAT, None)]).marshal()  # (marshalled only when set, plan/project.go)
    assert json.loads(distinct([(CAT, None)], cond=None))["~children"][0]["~child"]["~children"][0]["#operator"] == "InitialProject"
    with pytest.raises(ValueError):
        plan.filter_group_plan(COND, [], [], filter_only=True, project=[(PRICE, "p")])
    with pytest.raises(ValueError):
        plan.filter_group_plan(COND, [], [], filter_only=True, distinct=[(CAT, None)], project=[(PRICE, "p")])
    with pytest.raises(ValueError):
        plan.filter_group_plan(COND, [CAT], ["count(*)"], distinct=[(CAT, None)])


# ------------------------------------------------------------------------------------------------ 2. refusals
@pytest.mark.parametrize("term", ["lower(%s)" % CAT, "(%s + 1)" % PRICE, "5", "\"x\"", "count(*)",
                                  "array `v` for `v` in %s end" % A])
def test_a_term_that_is_no_leaf_path_is_unsupported(term):
    e = refused(distinct([(term, None)]))
    assert e.status == _ffi.UNSUPPORTED and "leaf path" in e.message and term in e.message


def test_the_other_refusals_name_their_construct():
    seq = lambda *ch: node("Sequence", **{"~children": list(ch)})
    cases = [
        (seq(FILTER, node("InitialProject", distinct=True, result_terms=[{"star": True, "expr": "`default`"}]), node("Distinct")), "star"),
        (seq(FILTER, project([(CAT, None)], raw=True), node("Distinct")), "raw"),
        (seq(FILTER, project([(D("t%d" % i), None) for i in range(5)]), node("Distinct")), "5 result terms"),
        (seq(FILTER, node("Distinct")), "Distinct without the InitialProject"),
        (seq(node("Distinct")), "Distinct without the InitialProject"),
        (seq(FILTER, project([(CAT, None)])), "InitialProject"),                                     # no Distinct follows
        (seq(FILTER, node("Order", sort_terms=[{"expr": CAT}]), project([(CAT, None)]), node("Distinct")), "Order / Offset / Limit"),
        (seq(FILTER, node("Limit", expr="3"), project([(CAT, None)]), node("Distinct")), "Order / Offset / Limit"),
        (seq(FILTER, project([(CAT, None)]), node("Distinct"), node("Limit", expr="3"), node("Distinct")), "Distinct after Order / Offset / Limit"),
        (seq(FILTER, project([(CAT, None)]), node("Distinct"), node("Order", sort_terms=[{"expr": CAT}]), node("Distinct")), "Distinct after Order / Offset / Limit"),
        (seq(FILTER, project([(CAT, None)]), node("Limit", expr="3"), node("Distinct")), "Limit between"),
        (seq(FILTER, node("InitialProject", result_terms=[{"expr": CAT}]), node("Distinct")), "InitialProject"),   # not distinct: stays refused
        (seq(FILTER, node("InitialProject", result_terms=[{"expr": CAT}])), "InitialProject"),
        (seq(FILTER, node("FinalProject")), "FinalProject"),
    ]
    for pj, word in cases:
        e = refused(pj)
        assert e.status == _ffi.UNSUPPORTED and word in e.message, (pj, e.message)
    # distinct over groups: unchanged
    grouped = json.loads(plan.filter_group_plan(COND, [CAT], ["count(*)"], project=[(CAT, "c")]))
    grouped["~children"][3]["~child"]["~children"][0]["distinct"] = True
    e = refused(grouped)
    assert e.status == _ffi.UNSUPPORTED and "distinct" in e.message
    e = refused(seq(node("InitialGroup", group_keys=[CAT], aggregates=[]), node("Distinct")))
    assert e.status == _ffi.UNSUPPORTED and "Distinct" in e.message


@pytest.mark.parametrize("kw", [{}, {"order": [(CAT, False)]}, {"limit": 3}])
def test_the_multi_batch_calls_are_unsupported(kw):
    op = query_amd.GpuFilterGroup(distinct([(PRICE, None)], **kw))
    L = _ffi.lib()
    tags, pay = np.full(4, _ffi.T_INT, np.uint8), np.arange(4, dtype=np.uint64)
    b = op.make_device_batch(4, [(_ffi.COL_TAGGED64, tags.ctypes.data, pay.ctypes.data, None)])  # (host memory: the calls stop before it)
    res = _ffi.Result()
    doc = b'{"price": 60}'
    offs = np.array([0, len(doc)], dtype=np.uint64)
    calls = {"n1k_push_batch": lambda: L.n1k_push_batch(op._h, C.byref(b[0])),
             "n1k_push_device_batch": lambda: L.n1k_push_device_batch(op._h, C.byref(b[0])),
             "n1k_run_device_batch": lambda: L.n1k_run_device_batch(op._h, C.byref(b[0]), C.byref(res)),
             "n1k_push_json": lambda: L.n1k_push_json(op._h, 1, offs.ctypes.data_as(C.POINTER(C.c_uint64)), doc)}
    for name, call in calls.items():
        assert call() == _ffi.UNSUPPORTED, name
        msg = L.n1k_last_error(op._h).decode()
        assert name in msg and "one batch" in msg and "n1k_filter_device_batch" in msg
    op.done()


def test_options_and_stats_exist():
    L = _ffi.lib()
    assert "n1k_rowdistinct_stats" in _ffi.SYMBOLS and hasattr(L, "n1k_rowdistinct_stats")
    op = query_amd.GpuFilterGroup(distinct([(CAT, None)]), rowdistinct_slots=7, rowdistinct_lds_slots=0)
    op.set_option("rowdistinct_lds_slots", 100)
    assert op.rowdistinct_stats() == {"survivors": 0, "distinct_rows": 0, "table_slots": 0, "reached_table": 0}
    op.done()


# the stage parses its own options (rowdistinct_option, n1k_rowdistinct.cpp); as test_options_cpu.py asks of the engine's, each
# one names the GPU test that checks it against the reference
STAGE_OPTIONS = {
    "rowdistinct_slots": "test_a_full_table_wraps_and_a_table_one_slot_short_is_oom_and_the_handle_goes_on",
    "rowdistinct_lds_slots": "test_tiles_at_under_and_over_the_lds_sets_size",
}


def test_every_option_of_the_stage_has_a_reference_check():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "query_amd", "csrc", "n1k_rowdistinct.cpp")).read()
    body = src[src.index("bool rowdistinct_option("):src.index("n1k_status distinct_selection(")]
    assert set(re.findall(r'\bname\s*==\s*"([A-Za-z0-9_]+)"', body)) == set(STAGE_OPTIONS)
    tests = open(os.path.join(root, "tests", "test_gpu_distinct_rows.py")).read()
    for option, test in STAGE_OPTIONS.items():
        at = tests.index("def %s(" % test)
        end = tests.find("\ndef ", at + 1)
        assert re.search(r"""["']%s["']|\b%s=""" % (option, option), tests[at:end if end > 0 else None]), "%s does not set %s" % (test, option)
    op = query_amd.GpuFilterGroup(distinct([(CAT, None)]))
    with pytest.raises(query_amd.N1kError) as ei:
        op.set_option("rowdistinct_nothing", 1)
    assert ei.value.status == _ffi.INVALID and "unknown option" in ei.value.message
    op.done()


# ------------------------------------------------------------------------------------------------ 3. the check of the checker
I, F = (lambda x: (du.T_INT, x)), (lambda x: (du.T_FLOAT, x))
MISSING, NULL, FALSE, TRUE = (du.T_MISSING, None), (du.T_NULL, None), (du.T_FALSE, None), (du.T_TRUE, None)
NAN2 = float(np.uint64(0xFFF8000000000001).view(np.float64))
S5, A5, O5 = (du.T_STRING, b"five"), (du.T_ARRAY, b"five"), (du.T_OBJECT, b"five")
# every value of the equality list of n1k.h, by the class it must fall into
CLASSES = [[MISSING], [NULL], [FALSE], [TRUE], [I(0), F(-0.0), F(0.0)], [F(0.5)], [I(2), F(2.0)], [I(2 ** 53 + 1)], [F(2.0 ** 53), I(2 ** 53)],
           [I(2 ** 63 - 1)], [F(2.0 ** 63)], [F(float("nan")), F(NAN2)], [F(float("inf"))], [F(float("-inf"))], [S5], [A5], [O5],
           [(du.T_STRING, b"NaN")], [(du.T_STRING, b"+Infinity")], [I(-2 ** 63), F(-2.0 ** 63)]]


def test_the_reference_gets_every_pair_of_the_equality_list_right():
    flat = [(c, v) for c, vs in enumerate(CLASSES) for v in vs]
    for (ca, a), (cb, b) in itertools.product(flat, repeat=2):
        assert (du.normalise(a) == du.normalise(b)) == (ca == cb), (a, b)
    values = [[v for _, v in flat]]
    reps = du.representatives(values)
    assert len(reps) == len(CLASSES) and [flat[i][0] for i in reps] == list(range(len(CLASSES)))  # the first of each class, ascending
    # several terms: a row is its terms in their order
    two = [[I(1), I(2), I(1), F(1.0)], [I(2), I(1), I(2), F(2.0)]]
    assert list(du.representatives(two)) == [0, 1] and list(du.representatives(two, sel=[1, 2, 3])) == [1, 2]
    # the vectorised form agrees with the pairs
    rng = np.random.default_rng(7)
    a, b = rng.integers(0, 5, 500), rng.integers(-2, 2, 500)
    sel = np.nonzero(rng.random(500) < 0.7)[0]
    pairs = [[I(int(x)) for x in a], [I(int(x)) for x in b]]
    assert np.array_equal(du.representatives([a, b], sel), du.representatives(pairs, sel))


@pytest.mark.parametrize("case", du.golden_cases(), ids=[c["id"] for c in du.golden_cases()])
def test_the_reference_reproduces_the_golden_results(case):
    table, terms, order, proj, sel = du.golden_setup(case)
    by = {c.name: c for c in table.columns}
    col = lambda p: ou.column_values(by[p].tags, by[p].payload, table.dictionary)
    reps = du.representatives([col(p) for p, _ in terms], sel)
    want = ou.expected([col(p) for p, _ in order], [d for _, d in order], sel=reps)
    rows = ou.golden_rows(table, proj, want)
    assert rows == case["results"] and gu.same_json(rows, case["results"])
    if case["plan"]["condition"] is None:
        assert rows[0] == {} and len(sel) == len(gu.load_docs(case["keyspace"]))  # the MISSING parent: one row, an empty object
        assert len(reps) == 3 < len(sel) == 5  # (the orders statement's four survivors are four customers: nothing falls there)
    # the plan the device gets for it creates, with these columns
    op = query_amd.GpuFilterGroup(plan.filter_group_plan(case["plan"]["condition"], [], [], filter_only=True, distinct=terms, order=order))
    assert op.column_paths == [c.name for c in table.columns]
    op.done()
