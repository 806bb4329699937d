"""CASE and IFMISSING / IFNULL / IFMISSINGORNULL / NULLIF / MISSINGIF as values, without a GPU: what n1k_create accepts and
refuses, and the yardstick (tests/cond_util.py) against hand-written truth tables."""
import json
import os

import pytest

import cond_util as cn
import golden_util as gu
import query_amd
from query_amd import _ffi, plan

M = cn.MISSING
D = lambda name: plan.field_path("d", name)  # noqa: E731

with open(os.path.join(gu.GOLDEN, "cases_cond.json")) as fh:
    COND_CASES = json.load(fh)["cases"]


def create(condition, keys, aggs, **kw):
    return query_amd.GpuFilterGroup(plan.filter_group_plan(condition, keys, aggs, **kw))


def paths_of(condition, keys, aggs, **kw):
    op = create(condition, keys, aggs, **kw)
    try:
        return op.column_paths
    finally:
        op.done()


def refusal(condition, keys, aggs, **kw):
    with pytest.raises(query_amd.N1kError) as ei:
        create(condition, keys, aggs, **kw).done()
    return ei.value


PRICE_CASE = plan.case_when([("(50 < %s)" % D("price"), D("price"))], "0")
BUCKET = plan.case_when([("(%s < 10)" % D("price"), '"low"'), ("(%s < 100)" % D("price"), '"mid"')], '"high"')

# (condition, keys, aggregates, column paths in first-use text order)
ACCEPTED = [
    (None, [D("cat")], ["sum(%s)" % PRICE_CASE], [D("cat"), D("price")]),
    (None, [D("cat")], ["count(%s)" % plan.case_when([("(50 < %s)" % D("price"), "1")])], [D("cat"), D("price")]),
    (None, [BUCKET], ["count(*)"], [D("price")]),
    (None, [plan.case_of(D("kind"), [('"a"', D("x")), ("3", D("y"))], D("z"))], ["count(*)"], [D("kind"), D("x"), D("y"), D("z")]),
    (None, [plan.case_of(D("kind"), [(D("other"), "1")])], ["count(*)"], [D("kind"), D("other")]),
    (None, [D("cat")], ["sum(%s)" % plan.cond_fn("ifmissing", D("x"), "0")], [D("cat"), D("x")]),
    (None, [plan.cond_fn("ifnull", D("a"), D("b"), D("c"), '"none"')], ["count(*)"], [D("a"), D("b"), D("c")]),
    (None, [plan.cond_fn("ifmissingornull", D("b"), D("a"), "0")], ["count(*)"], [D("b"), D("a")]),
    (None, [plan.cond_fn("nullif", D("score"), "100")], ["count(*)"], [D("score")]),
    (None, [plan.cond_fn("missingif", D("score"), D("top"))], ["max(%s)" % D("score")], [D("score"), D("top")]),
    # as an operand of a Filter comparison, as a bare condition, nested, with arithmetic in WHEN and THEN
    ("(%s = 3)" % plan.cond_fn("nullif", D("a"), D("b")), [], ["count(*)"], [D("a"), D("b")]),
    (plan.case_when([("(%s is missing)" % D("flag"), "true")], D("flag")), [D("k")], ["count(*)"], [D("flag"), D("k")]),
    ("(%s < %s)" % (D("lo"), plan.case_when([("((%s + 1) < 10)" % D("x"), "(%s * 2)" % D("x"))], plan.cond_fn("ifmissing", D("y"), "0"))),
     [], ["count(*)"], [D("lo"), D("x"), D("y")]),
    (None, [plan.case_when([("(%s and (not (%s between 1 and 5)))" % (D("t"), D("x")), plan.case_when([("(%s = \"a\")" % D("s"), "1")], "2"))])],
     ["avg(%s)" % plan.cond_fn("ifnull", D("x"), "(%s - 1)" % D("y"))], [D("t"), D("x"), D("s"), D("y")]),
    ("(%s is not null)" % plan.cond_fn("missingif", D("a"), '"x"'), [], [], [D("a")]),
]


@pytest.mark.parametrize("i", range(len(ACCEPTED)))
def test_every_form_is_accepted_with_its_paths_in_text_order(i):
    condition, keys, aggs, want = ACCEPTED[i]
    assert paths_of(condition, keys, aggs, filter_only=not keys and not aggs) == want


def test_upper_case_keywords_and_names_are_the_same_expression():
    text = "CASE WHEN (%s < 10) THEN 1 ELSE IFMISSING(%s, 0) END" % (D("a"), D("b"))
    assert paths_of(None, [text], ["count(*)"]) == [D("a"), D("b")]


def arms(n):
    return [("(%s < %d)" % (D("a"), i), str(i)) for i in range(n)]


REFUSED = {
    "a ninth arm": (None, [plan.case_when(arms(9))], ["count(*)"], {}, "9 WHEN arms"),
    "a 17th term": (None, [plan.case_when([("(%s)" % " or ".join("(%s = %d)" % (D("a"), i) for i in range(9)), "1"),
                                           ("(%s)" % " or ".join("(%s = %d)" % (D("b"), i) for i in range(8)), "2")])], ["count(*)"], {}, "16 terms"),
    "a fifth ifnull argument": (None, [plan.cond_fn("ifnull", D("a"), D("b"), D("c"), D("e"), "1")], ["count(*)"], {}, "ifnull with 5 arguments"),
    "LIKE in a WHEN": (None, [plan.case_when([('(%s like "a%%")' % D("a"), "1")])], ["count(*)"], {}, "LIKE in the WHEN"),
    "ANY in a WHEN": (None, [plan.case_when([('any `v` in %s satisfies (`v` = "x") end' % D("a"), "1")])], ["count(*)"], {}, "ANY / EVERY in the WHEN"),
    "IN in a WHEN": (None, [plan.case_when([(plan.in_list(D("a"), ["x", 3]), "1")])], ["count(*)"], {}, "IN in the WHEN"),
    "lower in a WHEN": (None, [plan.case_when([('(lower(%s) = "x")' % D("a"), "1")])], ["count(*)"], {}, "a string function in the WHEN"),
    "greatest as an operand": (None, [plan.case_when([("(%s < 1)" % D("a"), "greatest(%s, 1)" % D("b"))])], ["count(*)"], {}, "'greatest' inside CASE"),
    "least as an argument": (None, [plan.cond_fn("ifmissing", D("a"), "least(%s, 1)" % D("b"))], ["count(*)"], {}, "'least' inside CASE"),
    "CASE in HAVING": (None, [D("a")], ["count(*)"], {"having": plan.case_when([("(count(*) < 1)", "true")], "false")}, "HAVING: CASE"),
    "CASE in a projection over groups": (None, [D("a")], ["count(*)"], {"project": [(plan.case_when([("(count(*) < 1)", "1")], "2"), "x")]}, "CASE or a conditional function as a projection term"),
    "CASE as a sort term": ("(0 < %s)" % D("a"), [], [], {"filter_only": True, "order": [(plan.case_when([("(%s < 1)" % D("a"), "1")]), False)]}, "case when"),
    "CASE as a DISTINCT term": ("(0 < %s)" % D("a"), [], [], {"filter_only": True, "distinct": [(plan.case_when([("(%s < 1)" % D("a"), "1")]), "x")]}, "case when"),
    "too many columns": (None, [plan.cond_fn("ifmissing", "(%s + %s)" % (D("c0"), D("c1")), "(%s + %s)" % (D("c2"), D("c3")))] +
                         [plan.cond_fn("ifnull", "(%s + %s)" % (D("c%d" % (4 + 2 * i)), D("c%d" % (5 + 2 * i))), "0") for i in range(3)],
                         ["count(*)"], {}, "too many columns"),
}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_each_limit_is_refused_as_unsupported_and_names_its_construct(what):
    condition, keys, aggs, kw, names = REFUSED[what]
    e = refusal(condition, keys, aggs, **kw)
    assert e.status == _ffi.UNSUPPORTED, (e.status, e.message)
    assert names in e.message, e.message


def test_the_limits_themselves_are_taken():
    """eight arms, sixteen terms, four arguments"""
    assert paths_of(None, [plan.case_when(arms(8))], ["count(*)"]) == [D("a")]
    sixteen = plan.case_when([("(%s)" % " or ".join("(%s = %d)" % (D("a"), i) for i in range(8)), "1"),
                              ("(%s)" % " or ".join("(%s = %d)" % (D("b"), i) for i in range(8)), "2")])
    assert paths_of(None, [sixteen], ["count(*)"]) == [D("a"), D("b")]
    assert paths_of(None, [plan.cond_fn("ifmissingornull", D("a"), D("b"), D("c"), D("e"))], ["count(*)"]) == [D("a"), D("b"), D("c"), D("e")]


MALFORMED = ["case when %s end" % D("a"), "case when %s then 1" % D("a"), "case %s end" % D("a"), "case when %s then 1 else end" % D("a"),
             "nullif(%s)" % D("a"), "missingif(%s, 1, 2)" % D("a"), "ifmissing(%s)" % D("a"), "ifnull(%s, 1" % D("a")]


@pytest.mark.parametrize("text", MALFORMED)
def test_malformed_text_is_invalid(text):
    e = refusal(None, [text], ["count(*)"])
    assert e.status == _ffi.INVALID, (e.status, e.message)


# ---------------------------------------------------------------- the mirror against hand-written truth tables
#
# One representative per tag: MISSING, NULL, FALSE, TRUE, INT, FLOAT, STRING, ARRAY — the INT and the FLOAT equal (3 and 3.0), so
# that Equals across the two number tags is in the tables.  A cell names the result: a / b the argument, N NULL, M MISSING.
REPS = [M, None, False, True, 3, 3.0, "s", [1]]
TABLES = {
    #                 b: M    N    F    T    3   3.0   s   [1]
    "ifmissing": ["N b b b b b b b".split(),   # a MISSING: b, and NULL when b is MISSING too
                  "a a a a a a a a".split(), "a a a a a a a a".split(), "a a a a a a a a".split(), "a a a a a a a a".split(),
                  "a a a a a a a a".split(), "a a a a a a a a".split(), "a a a a a a a a".split()],
    "ifnull": ["a a a a a a a a".split(),      # a MISSING IS returned
               "b N b b b b b b".split(),      # a NULL: b — a MISSING b too —, and NULL when b is NULL
               "a a a a a a a a".split(), "a a a a a a a a".split(), "a a a a a a a a".split(), "a a a a a a a a".split(),
               "a a a a a a a a".split(), "a a a a a a a a".split()],
    "ifmissingornull": ["N N b b b b b b".split(), "N N b b b b b b".split(),
                        "a a a a a a a a".split(), "a a a a a a a a".split(), "a a a a a a a a".split(), "a a a a a a a a".split(),
                        "a a a a a a a a".split(), "a a a a a a a a".split()],
    "nullif": ["M M M M M M M M".split(),      # eq MISSING
               "M N N N N N N N".split(),      # eq MISSING for a MISSING b, else NULL
               "M N N a a a a a".split(),      # FALSE = FALSE: NULL
               "M N a N a a a a".split(),
               "M N a a N N a a".split(),      # 3 = 3 and 3 = 3.0
               "M N a a N N a a".split(),
               "M N a a a a N a".split(),
               "M N a a a a a N".split()],
    "missingif": ["M M M M M M M M".split(),
                  "M N N N N N N N".split(),
                  "M N M a a a a a".split(),
                  "M N a M a a a a".split(),
                  "M N a a M M a a".split(),
                  "M N a a M M a a".split(),
                  "M N a a a a M a".split(),
                  "M N a a a a a M".split()],
}


@pytest.mark.parametrize("name", sorted(TABLES))
def test_the_mirror_gives_the_hand_written_truth_table(name):
    for i, a in enumerate(REPS):
        for j, b in enumerate(REPS):
            got = cn.cond_fn_apply(name, [a, b])
            cell = TABLES[name][i][j]
            want = {"a": a, "b": b, "N": None, "M": M}[cell]
            assert got is want or (cell in "ab" and got == want and type(got) is type(want)), (name, a, b, got, cell)
            # the expression evaluator agrees with the function
            row = {"a": a, "b": b}
            assert cn.eval_value(("fn", name, [("col", "a"), ("col", "b")]), row) is got


def test_the_mirror_on_case():
    """Searched CASE: the first TRUE arm, NULL / MISSING / FALSE conditions pass by, no arm: ELSE or NULL.  Simple CASE:
    Equals of the search value, which a NULL or MISSING search never satisfies."""
    lt = lambda c: ("cmp", "<", ("col", "a"), ("const", c))  # noqa: E731
    case = ("case", [(lt(5), ("const", "low")), (lt(50), ("const", "mid")), (("truth", ("col", "a")), ("col", "a"))], None)
    for a, want in [(1, "low"), (5, "mid"), (70, 70), (M, None), (None, None), (False, "low"), ("x", "x"), ("", None), ([], None), ([0], [0])]:
        assert cn.eval_value(case, {"a": a}) == want, a
    both = ("case", [(lt(50), ("const", 1)), (lt(500), ("const", 2))], ("const", 3))
    assert [cn.eval_value(both, {"a": a}) for a in (7, 70, 700, None)] == [1, 2, 3, 3]
    simple = ("simple", ("col", "a"), [(("const", 3), ("const", "three")), (("const", "s"), ("const", "ess")), (("col", "a"), ("const", "self"))], ("const", "else"))
    assert [cn.eval_value(simple, {"a": a}) for a in (3, 3.0, "s", True, None, M)] == ["three", "three", "ess", "self", "else", "else"]
    assert cn.eval_value(("simple", ("col", "a"), [(("const", 1), ("const", 1))], None), {"a": 2}) is None


def test_the_text_writers_round_trip_through_the_parser():
    node = ("case", [(("and", [("cmp", "<", ("col", "x"), ("const", 5)), ("not", ("is", ("col", "s"), "missing"))]), ("arith", "+", ("col", "x"), ("col", "g")))],
            ("fn", "ifnull", [("col", "a"), ("const", "none")]))
    text = cn.value_text(node)
    assert text == ("case when (((`default`.`x`) < 5) and (not ((`default`.`s`) is missing))) then ((`default`.`x`) + (`default`.`g`)) "
                    "else ifnull((`default`.`a`), \"none\") end")
    assert paths_of(None, [text], ["count(*)"]) == [cn.D(c) for c in cn.columns_of(node)] == [cn.D(c) for c in ("x", "s", "g", "a")]


# ---------------------------------------------------------------- what the GPU tests push

def test_the_library_takes_every_plan_of_the_gpu_differential():
    """tests/test_gpu_cond.py counts a refusal as a failure: every plan it draws is created here, device side and oracle side
    alike, and the device's columns are the node's and the rest's in text order."""
    import test_gpu_cond as tg
    uses = set()
    kinds = set()
    for seed in range(tg.NSEEDS):
        p = cn.draw_plan(seed)
        dcond, dkeys, daggs = p["device"]
        paths = paths_of(dcond, dkeys, daggs)
        assert set(paths) <= {cn.D(c) for c in ("a", "x", "s", "k", "g")}, (seed, paths)
        ocond, okeys, oaggs = p["oracle"]
        assert cn.D("h") in paths_of(ocond, okeys, oaggs)
        uses.add(p["use"])
        kinds.add(p["node"][0] if p["node"][0] != "fn" else p["node"][1])
        text = json.dumps(p["node"], default=str)
        kinds.update(k for k in ("arith",) if '"arith"' in text)
        kinds.update(["nested"] if max(text.count('"case"') + text.count('"simple"') + text.count('"fn"'), 0) > 1 else [])
    assert uses == set(cn.USES)
    assert {"case", "simple", "arith", "nested"} | set(cn.FUNCTIONS) <= kinds, kinds


@pytest.mark.parametrize("case", COND_CASES, ids=[c["id"] for c in COND_CASES])
def test_the_golden_plans_are_accepted_with_the_fixtures_columns(case):
    p = case["plan"]
    assert paths_of(p["condition"], p["group_keys"], p["aggregates"]) == case["columns"]


# the entries of tests/golden/plans.json that n1k_create accepted before CASE and the conditional functions were values
PLANS_ACCEPTED_BEFORE = [
    1, 3, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 29, 31, 33, 37, 43, 45, 47, 49, 51, 53, 55, 59, 61, 63,
]


def test_the_explain_goldens_give_the_outcome_they_gave_before():
    with open(os.path.join(gu.GOLDEN, "plans.json")) as fh:
        plans = json.load(fh)
    accepted = []
    for i, entry in enumerate(plans):
        try:
            query_amd.GpuFilterGroup(json.dumps(entry["plan"])).done()
            accepted.append(i)
        except query_amd.N1kError as e:
            assert e.status == _ffi.UNSUPPORTED, (i, e.message)
    assert accepted == PLANS_ACCEPTED_BEFORE
