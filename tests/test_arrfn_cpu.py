"""array_length / array_count / array_sum / array_avg / array_contains / array_position as values, without a GPU: the yardstick
(tests/arrfn_util.py) against a hand-written table and the reference's recorded results, the host evaluator against the
yardstick, and what n1k_create accepts and refuses."""
import json
import os

import numpy as np
import pytest

import arrfn_util as au
import golden_util as gu
import query_amd
from query_amd import _ffi, plan

M = au.MISSING
D = lambda name: plan.field_path("d", name)  # noqa: E731
I, F = au.r_int, au.r_float
NULL, MISS, TRUE, FALSE = au.R_NULL, au.R_MISSING, au.R_TRUE, au.R_FALSE

with open(os.path.join(gu.GOLDEN, "cases_arr.json")) as fh:
    ARR = json.load(fh)


# ---------------------------------------------------------------- the yardstick against a hand-written table
# input -> (length, count, sum, avg, contains(x, 1), position(x, 1)); every entry written by hand from func_array.go

HAND = [
    ("empty", [], (I(0), I(0), I(0), NULL, FALSE, I(-1))),
    ("only nulls", [None, None, None], (I(3), I(0), I(0), NULL, FALSE, I(-1))),
    ("nested", [[1], {"a": 1}, [[1]], 1], (I(4), I(4), I(1), I(1), TRUE, I(3))),
    ("nested only", [[1, 2], {"f": 1}], (I(2), I(2), I(0), NULL, FALSE, I(-1))),
    # INT 0 + INT 1 = INT 1, + FLOAT 2.5 = FLOAT 3.5; avg 3.5 / 2
    ("mixed int / float", [1, 2.5], (I(2), I(2), F(3.5), F(1.75), TRUE, I(0))),
    # an integral float IS an int (NewValue): 1 + 2 = INT 3; 3 / 2 = 1.5
    ("an integral float", [1.0, 2.0], (I(2), I(2), I(3), F(1.5), TRUE, I(0))),
    # 0 + 2^62 + 2^62 wraps: FLOAT 2^63 (value/integer.go:266-277); avg 2^63 / 2 = 2^62, which folds back to INT
    ("an INT sum that overflows", [2 ** 62, 2 ** 62], (I(2), I(2), F(2.0 ** 63), I(2 ** 62), FALSE, I(-1))),
    # INT 0 and INT -3 differ in sign: float64(0) + float64(-3), a FLOAT from the first step on
    ("a leading negative", [-3, 4], (I(2), I(2), F(1.0), F(0.5), FALSE, I(-1))),
    # -0.0 is float64 -0.0, IsInt, int64(-0.0) = INT 0
    ("-0.0", [-0.0], (I(1), I(1), I(0), I(0), FALSE, I(-1))),
    # 2^53 + 1 decodes to float64 2^53, then INT 2^53
    ("2^53 + 1", [2 ** 53 + 1], (I(1), I(1), I(2 ** 53), I(2 ** 53), FALSE, I(-1))),
    ("strings and booleans", ["1", True, None, 1], (I(4), I(3), I(1), I(1), TRUE, I(3))),
    ("a non-array", 5, (NULL,) * 6),
    ("a string", "[1]", (NULL,) * 6),
    ("an object", {"a": [1]}, (NULL,) * 6),
    ("null", None, (NULL,) * 6),
    ("MISSING", M, (MISS,) * 6),
]


@pytest.mark.parametrize("row", HAND, ids=[r[0] for r in HAND])
def test_the_yardstick_gives_the_hand_written_table(row):
    _name, a, want = row
    got = tuple(au.apply(fn, a, 1 if fn in au.BINARY else None) for fn in au.FUNCTIONS)
    assert got == want


def test_the_yardstick_on_the_second_argument():
    a = [1, "a", True, 2.5, None, 2 ** 53 + 1]
    assert au.apply("array_contains", a, M) == MISS and au.apply("array_position", a, M) == MISS
    assert au.apply("array_contains", M, None) == MISS  # MISSING is tested first (func_array.go:308-312)
    assert au.apply("array_contains", a, None) == NULL and au.apply("array_position", 5, None) == NULL and au.apply("array_position", 5, M) == MISS
    assert au.apply("array_position", a, "a") == I(1) and au.apply("array_position", a, True) == I(2) and au.apply("array_position", a, 2.5) == I(3)
    assert au.apply("array_contains", a, False) == FALSE and au.apply("array_contains", a, "1") == FALSE and au.apply("array_contains", a, 1.0) == TRUE
    # the element 2^53 + 1 IS 2^53; the constant 2^53 + 1 is an exact INT, and two INTs compare exactly (value/integer.go:68-87)
    assert au.apply("array_position", a, 2 ** 53) == I(5) and au.apply("array_position", a, 2 ** 53 + 1) == I(-1)
    assert au.apply("array_contains", [float("1e300")], 1e300) == TRUE


def test_the_yardstick_adds_like_number_value_add():
    assert au.num_add(0, 5) == 5 and isinstance(au.num_add(0, 5), int)
    assert au.num_add(0, -5) == -5.0 and isinstance(au.num_add(0, -5), float)
    assert au.num_add(-2, -5) == -7 and isinstance(au.num_add(-2, -5), int)
    assert au.num_add(2 ** 63 - 1, 1) == 2.0 ** 63 and isinstance(au.num_add(2 ** 63 - 1, 1), float)
    assert au.num_add(-(2 ** 63), -1) == -(2.0 ** 63) and isinstance(au.num_add(-(2 ** 63), -1), float)
    assert au.num_add(1, 0.5) == 1.5 and au.num_add(0.5, 1) == 1.5


@pytest.mark.parametrize("row", ARR["rows"], ids=[r["id"] for r in ARR["rows"]])
def test_the_yardstick_gives_the_references_recorded_results(row):
    got = au.result_json(au.apply(row["function"], row["array"], row["second"]))
    assert gu.same_json(got, row["result"]), (got, row["result"])


def test_the_recorded_rows_are_the_ones_the_issue_names():
    by_fn = {(r["function"], json.dumps(r["array"]), json.dumps(r["second"])): r["result"] for r in ARR["rows"]}
    assert by_fn[("array_length", json.dumps([None, None, None, "append", "avg", None, "max"]), "null")] == 7
    assert by_fn[("array_sum", json.dumps(list(range(-3, 5))), "null")] == 4
    assert by_fn[("array_count", "[7, 18, 16]", "null")] == 3 and by_fn[("array_avg", "[7, 18, 16]", "null")] == 13.666666666666666
    assert by_fn[("array_contains", "[7, 18, 16]", "7")] is True and by_fn[("array_avg", "7", "null")] is None
    assert by_fn[("array_position", json.dumps(["coffee01", "coffee01", "coffee01", "sugar22"]), '"sugar22"')] == 3
    assert len(ARR["cases"]) == 1 and "HAVING ARRAY_LENGTH(orderlines) >=2" in ARR["cases"][0]["statement"]


# ---------------------------------------------------------------- the host evaluator

CPU_PAIRS = (20261020, 600, 40)  # seed, terms, arrays per term: tests/test_gpu_arrfn.py runs the same pairs through the kernel


def test_host_evaluator_equals_the_yardstick_on_seeded_pairs():
    total, seen = 0, set()
    for fn, c, arrays in au.random_pairs(*CPU_PAIRS):
        term, texts = au.term_text(fn, c), au.texts_of(arrays)
        tags, pay = au.host_eval(term, texts)
        wt, wp = au.want_block(fn, c, texts)
        bad = np.nonzero((tags != wt) | (pay != wp))[0]
        assert bad.size == 0, (term, texts[bad[0]], (tags[bad[0]], hex(int(pay[bad[0]]))), (wt[bad[0]], hex(int(wp[bad[0]]))))
        total += len(texts)
        seen.update((fn, int(t)) for t in wt)
    assert total >= 20000
    # every function reached every kind of result it has
    for fn, tags in (("array_sum", (au.T_INT, au.T_FLOAT)), ("array_avg", (au.T_INT, au.T_FLOAT, au.T_NULL)),
                     ("array_contains", (au.T_TRUE, au.T_FALSE, au.T_NULL, au.T_MISSING)), ("array_position", (au.T_INT, au.T_NULL, au.T_MISSING))):
        assert all((fn, t) in seen for t in tags), (fn, sorted(seen))


RAW_TEXTS = [
    (b"[-0.0]", "array_sum", None, I(0)), (b"[-0]", "array_sum", None, I(0)), (b"[1e2,0.5]", "array_sum", None, F(100.5)),
    (b"[9007199254740993]", "array_sum", None, I(2 ** 53)), (b"[9007199254740993]", "array_contains", 2 ** 53, TRUE),
    (b"[-9223372036854775808]", "array_sum", None, F(-(2.0 ** 63))),  # 0 + MinInt64: signs differ, through float64
    (b"[9223372036854775807]", "array_sum", None, F(2.0 ** 63)),  # decodes to float64 2^63, which is no int64
    (b"[18446744073709551616,1]", "array_avg", None, F((2.0 ** 64 + 1.0) / 2.0)),
    (b'["a\\u0062",1]', "array_position", "ab", I(0)), (b'["\\"",1]', "array_contains", '"', TRUE),
    (b"", "array_length", None, NULL), (b"[", "array_length", None, NULL), (b"x", "array_count", None, NULL), (b'"[1]"', "array_length", None, NULL),
    (b"{}", "array_length", None, NULL), (b"[[],[[]],{}]", "array_count", None, I(3)), (b'[",]",","]', "array_length", None, I(2)),
]


@pytest.mark.parametrize("i", range(len(RAW_TEXTS)))
def test_host_evaluator_on_texts_written_by_hand(i):
    text, fn, c, want = RAW_TEXTS[i]
    tags, pay = au.host_eval(au.term_text(fn, c), [b"[]", text, b"[1]"])
    assert (int(tags[1]), int(pay[1])) == want


def test_an_empty_block_and_a_block_of_empty_entries():
    tags, pay = au.host_eval(au.term_text("array_length"), [])
    assert len(tags) == 0
    tags, pay = au.host_eval(au.term_text("array_length"), [b"", b"", b"[]"])
    assert tags.tolist() == [au.T_NULL, au.T_NULL, au.T_INT] and pay.tolist() == [0, 0, 0]


def test_the_diagnostic_entry_point_tells_unsupported_from_invalid():
    ok = [au.term_text(fn, 1 if fn in au.BINARY else None) for fn in au.FUNCTIONS] + ["ARRAY_LENGTH((`d`.`a`))", "array_contains((`d`.`a`), null)",
          "array_position((`d`.`a`), missing)", "array_contains(((`d`.`x`).`y`), (-2.5))", "array_length(meta(`d`))"]
    for t in ok:
        assert au.host_status(t.encode()) == _ffi.OK, t
    unsupported = ["array_min((`d`.`a`))", "array_max((`d`.`a`))", "array_sort((`d`.`a`))", "array_length([1, 2])", "array_length(((`d`.`a`) + 1))",
                   "array_contains((`d`.`a`), (`d`.`b`))", "array_contains((`d`.`a`), [1])", "array_position((`d`.`a`), ((`d`.`b`) + 1))",
                   "array_length(array_agg((`d`.`a`)))", "array_length(array `v` for `v` in (`d`.`a`) end)", "array_pos((`d`.`a`), 1)",
                   "array_contains((`d`.`a`), \"%s\")" % ("x" * 200)]
    for t in unsupported:
        assert au.host_status(t.encode()) == _ffi.UNSUPPORTED, t
    invalid = ["abs((`d`.`a`))", "(`d`.`a`)", "array_length(", "array_length()", "array_length((`d`.`a`), 1)", "array_contains((`d`.`a`))",
               "array_position((`d`.`a`), 1, 2)", "", "(array_length((`d`.`a`)) < 2)", "array_length((`d`.`a`)) trailing"]
    for t in invalid:
        assert au.host_status(t.encode()) == _ffi.INVALID, t


# ---------------------------------------------------------------- what n1k_create accepts

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


def call(fn, col="a"):
    return au.term_text(fn, "t_1" if fn in au.BINARY else None, over=D(col))


@pytest.mark.parametrize("fn", au.FUNCTIONS)
def test_every_function_is_accepted_in_each_place_with_its_paths_in_text_order(fn):
    f, a, k, x = call(fn), D("a"), D("k"), D("x")
    # operand of a Filter comparison, bare condition, operand of arithmetic, group key, aggregate operand
    assert paths_of("(1 < %s)" % f, [k], ["count(*)"]) == [a, k]
    assert paths_of("(%s and (%s < 5))" % (f, x), [k], ["count(*)"]) == [a, x, k]
    assert paths_of("((%s + %s) = 3)" % (f, x), [], ["count(*)"]) == [a, x]
    assert paths_of(None, [f], ["count(*)"]) == [a]
    assert paths_of(None, [k], ["sum(%s)" % f, "max((%s * 2))" % f]) == [k, a]
    assert paths_of("(0 <= %s)" % f, [], [], filter_only=True) == [a]
    # HAVING over a key and over ARRAY_AGG; a projection term over the groups, and ORDER BY through its alias
    agg = "array_agg(%s)" % x
    assert paths_of(None, [a], ["count(*)"], having="(2 <= %s)" % f) == [a]
    assert paths_of(None, [k], [agg], having="(%s is not null)" % au.term_text(fn, 3 if fn in au.BINARY else None, over=agg)) == [k, x]
    assert paths_of(None, [k], [agg], project=[(k, "k"), (au.term_text(fn, 3 if fn in au.BINARY else None, over=agg), "v")], order=[("`v`", True)]) == [k, x]
    assert paths_of(None, [a], ["count(*)"], project=[("(%s + 1)" % f, "v")]) == [a]
    # an operand inside a conditional node and an argument of a numeric function: they run
    assert paths_of(None, [k], ["max(%s)" % plan.case_when([("(%s < 2)" % f, f)], x)]) == [k, a, x]
    assert paths_of(None, [plan.cond_fn("ifnull", f, "0")], ["count(*)"]) == [a]
    assert paths_of(None, [k], ["sum(round(%s, 1))" % f]) == [k, a]


def test_equal_text_shares_one_table_and_a_fifth_distinct_term_is_refused():
    a = D("a")
    four = [au.term_text("array_length", over=a), au.term_text("array_sum", over=a), au.term_text("array_contains", "x", over=a), au.term_text("array_contains", "y", over=a)]
    cond = "(%s)" % " and ".join("(0 <= %s)" % t for t in four + four[:2])
    op = create(cond, [four[0]], ["max(%s)" % four[1]])
    try:
        st = op.arrfn_stats()
        assert st["terms"] == 4 and st["device_arrays"] == 0 and st["host_arrays"] == 0 and st["device_threshold"] > 0, st
    finally:
        op.done()
    e = refusal("(%s and (0 <= %s))" % (cond, au.term_text("array_count", over=a)), [], ["count(*)"])
    assert e.status == _ffi.UNSUPPORTED and "more than 4 distinct array-function terms" in e.message
    # a MISSING second argument folds to the constant MISSING: no term and no node; the path is parsed and otherwise unused
    op = create("(%s is missing)" % au.term_text("array_contains", M, over=a), [], ["count(*)"])
    try:
        assert op.arrfn_stats()["terms"] == 0 and op.column_paths == [a]
    finally:
        op.done()


A, B, K = D("a"), D("b"), D("k")
OTHER_FUNCTIONS = ["array_add", "array_append", "array_concat", "array_distinct", "array_flatten", "array_ifnull", "array_insert", "array_intersect",
                   "array_max", "array_min", "array_pos", "array_prepend", "array_put", "array_range", "array_remove", "array_repeat", "array_replace",
                   "array_reverse", "array_sort", "array_star", "array_symdiff", "array_symdiff1", "array_symdiffn", "array_union"]
REFUSED = {
    "an array constructor": (None, ["array_length([1, 2])"], ["count(*)"], {}, "array constructor"),
    "a comprehension": (None, ["array_length(array `v` for `v` in %s end)" % A], ["count(*)"], {}, "'array'"),
    "array_agg outside the grouped tail": (None, [K], ["max(array_length(array_agg(%s)))" % A], {}, "'array_agg'"),
    "arithmetic": ("(array_sum((%s + 1)) < 3)" % A, [], ["count(*)"], {}, "not a leaf path"),
    "a function of the path": (None, ["array_count(abs(%s))" % A], ["count(*)"], {}, "'abs'"),
    "a path as the second argument": ("array_contains(%s, %s)" % (A, B), [], ["count(*)"], {}, "second argument is not a constant"),
    "an expression as the second argument": ("array_contains(%s, (%s + 1))" % (A, B), [], ["count(*)"], {}, "second argument is not a constant"),
    "an array as the second argument": (None, ["array_position(%s, [1])" % A], ["count(*)"], {}, "array constructor"),
    "an object as the second argument": (None, ["array_position(%s, {\"f\": 1})" % A], ["count(*)"], {}, "'{'"),
    "inside SATISFIES": ("any `v` in %s satisfies (array_length(`v`) = 2) end" % A, [], ["count(*)"], {}, "function 'array_length' inside SATISFIES"),
    "a sort term of a Filter-only plan": ("(%s is not missing)" % A, [], [], {"filter_only": True, "order": [("array_length(%s)" % A, False)]}, "sort term of a plan without a group is not a leaf path"),
    "a DISTINCT term of a Filter-only plan": ("(%s is not missing)" % A, [], [], {"filter_only": True, "distinct": [("array_length(%s)" % A, "n")]}, "result term of a DISTINCT over rows is not a leaf path"),
    "a long STRING constant": ("array_contains(%s, \"%s\")" % (A, "x" * 105), [], ["count(*)"], {}, "STRING constant of more than 104 bytes"),
}
REFUSED.update({"the other function " + f: (None, ["%s(%s)" % (f, A)], ["count(*)"], {}, "array function '%s'" % f) for f in OTHER_FUNCTIONS})


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_each_refusal_is_unsupported_and_names_its_construct(what):
    condition, keys, aggs, kw, names = REFUSED[what]
    e = refusal(condition, keys, aggs, **kw)
    assert e.status == _ffi.UNSUPPORTED, (e.status, e.message)
    assert names in e.message, e.message


def test_array_min_and_array_max_are_named_as_the_follow_up():
    for f in ("array_min", "array_max"):
        assert "can be a new string" in refusal(None, ["%s(%s)" % (f, A)], ["count(*)"]).message


MALFORMED = ["array_length()", "array_length(%s, 1)" % A, "array_contains(%s)" % A, "array_position(%s, 1, 2)" % A, "array_sum(%s" % A]


@pytest.mark.parametrize("text", MALFORMED)
def test_a_wrong_argument_count_is_invalid(text):
    e = refusal(None, [text], ["count(*)"])
    assert e.status == _ffi.INVALID, (e.status, e.message)


# ---------------------------------------------------------------- what the GPU tests push

def test_the_library_takes_every_plan_of_the_gpu_suite():
    """tests/test_gpu_arrfn.py counts a refusal as a failure: every plan it draws or states is created here, device side and
    oracle side alike; every function and every use turns up."""
    import test_gpu_arrfn as tg
    uses, fns = set(), set()
    for seed in range(tg.NSEEDS):
        p = au.draw_plan(seed)
        dcond, dkeys, daggs = p["device"]
        assert set(paths_of(dcond, dkeys, daggs)) <= {au.D(c) for c in ("a", "x", "g", "k", "s")}, seed
        ocond, okeys, oaggs = p["oracle"]
        assert au.D("h") in paths_of(ocond, okeys, oaggs)
        uses.add(p["use"])
        fns.add(p["fn"])
    assert uses == set(au.USES) and fns == set(au.FUNCTIONS)
    for cond, keys, aggs, kw in tg.stated_plans():
        paths_of(cond, keys, aggs, **kw)
    case = ARR["cases"][0]
    assert paths_of(case["plan"]["condition"], case["plan"]["group_keys"], case["plan"]["aggregates"], having=case["having_text"]) == case["columns"]
