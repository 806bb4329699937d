"""ANY / EVERY ... SATISFIES without a GPU: the yardstick itself, the host evaluator against it, what n1k_create accepts and
refuses, and the run-time-built kernels of a plan with such a term (compile only, gfx950).

The yardstick is tests/coll_util.py's Python restatement of collEval + Any / Every / AnyEvery.Evaluate
(expression/coll_util.go:17-120, coll_any.go, coll_every.go, coll_any_every.go) and of the leaf semantics."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import coll_util as cu
import golden_util as gu
import query_amd
from query_amd import _ffi, plan

M = cu.MISSING
EQ_T1 = ("cmp", "=", [], "t_1", False)

# (mode, condition, array, result) — the rules one by one
TRUTHS = [
    # 1. the empty array: ANY is FALSE, EVERY is TRUE, ANY AND EVERY is FALSE (coll_any_every.go:84, `n > 0`)
    (cu.ANY, EQ_T1, [], False), (cu.EVERY, EQ_T1, [], True), (cu.ANY_EVERY, EQ_T1, [], False),
    # 2. one hit / one miss decides
    (cu.ANY, EQ_T1, ["a", "t_1"], True), (cu.ANY, EQ_T1, ["a", "b"], False), (cu.EVERY, EQ_T1, ["t_1", "t_1"], True),
    (cu.EVERY, EQ_T1, ["t_1", "a"], False), (cu.ANY_EVERY, EQ_T1, ["t_1"], True), (cu.ANY_EVERY, EQ_T1, ["t_1", 1], False),
    # 3. Truth() of NULL / MISSING is false: EVERY over an array holding one NULL fails, ANY goes on to the next element
    (cu.EVERY, EQ_T1, [None], False), (cu.EVERY, EQ_T1, ["t_1", None], False), (cu.ANY, EQ_T1, [None, "t_1"], True),
    (cu.EVERY, ("is", [], "null"), [None, None], True), (cu.EVERY, ("not", EQ_T1), [None], False), (cu.EVERY, ("not", EQ_T1), ["a", 1, [], {}], True),
    # 4. = is FALSE across types, numbers by value; < / <= follow the type order: BOOLEAN < NUMBER < STRING < ARRAY < OBJECT
    (cu.ANY, ("cmp", "=", [], 1, False), ["1", True, 1.5], False), (cu.ANY, ("cmp", "=", [], 1, False), [1], True),
    (cu.ANY, ("cmp", "=", [], 2 ** 53, False), [2 ** 53 + 1], False), (cu.ANY, ("cmp", "=", [], 0.5, False), [0.5], True),
    (cu.EVERY, ("cmp", "<", [], "a", False), [True, 7, -1.5], True), (cu.ANY, ("cmp", "<", [], "a", False), [["a"], {"f": 1}, "a", "b"], False),
    (cu.EVERY, ("cmp", "<", [], "a", True), [["a"], {"f": 1}, "ab", "b"], True), (cu.EVERY, ("cmp", "<=", [], "é", False), ["a", "z", "é"], True),
    (cu.EVERY, ("cmp", "<", [], True, False), [False], True), (cu.ANY, ("cmp", "<", [], False, False), [False, True, 1], False),
    (cu.ANY, ("between", [], "a", "b"), ["ab"], True), (cu.ANY, ("between", [], "a", "b"), ["c", 1, None], False),
    (cu.ANY, ("between", ["f"], 1, 2.5), [{"f": 2.5}], True), (cu.ANY, ("between", ["f"], 1, 2.5), [{"f": 3}, {"g": 2}, 2], False),
    # 5. a field of an element that is no object, or lacks the name, is MISSING
    (cu.EVERY, ("is", ["f"], "missing"), [1, "a", [], {"g": 1}], True), (cu.ANY, ("is", ["f"], "missing"), [{"f": None}], False),
    (cu.ANY, ("cmp", "=", ["g", "h"], "t_1", False), [{"g": {"h": "t_1"}}], True), (cu.ANY, ("cmp", "=", ["g", "h"], "t_1", False), [{"g": "t_1"}, {"h": "t_1"}], False),
    (cu.ANY, ("cmp", "<", ["f"], 3, False), [{"f": 2}], True), (cu.ANY, ("cmp", "<", ["f"], 3, True), [{"f": 2}, {"f": 3}], False),
    (cu.ANY, ("is", ["f"], "not valued"), [{"f": None}], True), (cu.EVERY, ("is", ["f"], "valued"), [{"f": 0}, {"f": ""}], True),
    # 6. LIKE inside: NULL for a non-string, so NOT LIKE keeps only strings
    (cu.ANY, ("like", [], "t\\_%"), ["t_1"], True), (cu.ANY, ("like", [], "t\\_%"), ["tx1", 5], False), (cu.ANY, ("not", ("like", [], "a%")), [5, None, "ab"], False),
    (cu.ANY, ("not", ("like", [], "a%")), [5, "b"], True), (cu.ANY, ("like", ["f"], "%b"), [{"f": "ab"}], True),
    # 7. strings with escapes, nested arrays, numbers beyond 2^53 and beyond int64, floats
    (cu.ANY, ("cmp", "=", [], 'x"y', False), ['x"y'], True), (cu.ANY, ("cmp", "=", [], "a\\b", False), ["a\\b"], True), (cu.ANY, ("cmp", "=", [], "a\nb", False), ["a\nb"], True),
    (cu.ANY, ("like", [], "a_b"), ["a\nb"], True), (cu.ANY, EQ_T1, [["t_1"]], False), (cu.ANY, ("cmp", "=", ["f"], 2 ** 53 + 1, False), [{"f": 2 ** 53 + 1}], True),
    (cu.ANY, ("cmp", "=", ["f"], 2 ** 53 + 1, False), [{"f": 2 ** 53}], False), (cu.ANY, ("cmp", "=", [], 2 ** 63, False), [2 ** 63], True),
    (cu.ANY, ("cmp", "<", ["f"], 10 ** 20, False), [{"f": 2 ** 63}], True), (cu.ANY, ("cmp", "=", [], 123456789012345.5, False), [123456789012345.5], True),
    (cu.ANY, ("cmp", "=", ['q"'], 1, False), [{'q"': 1}], True),
    # 8. AND / OR / NOT in four values
    (cu.ANY, ("or", [("cmp", "=", ["f"], 1, False), ("cmp", "=", [], "a", False)]), ["a"], True),   # MISSING or TRUE
    (cu.ANY, ("and", [("cmp", "=", ["f"], 1, False), ("cmp", "=", [], "a", False)]), ["a"], False),  # MISSING and TRUE
    (cu.EVERY, ("not", ("and", [("cmp", "=", ["f"], 1, False), ("cmp", "=", [], "b", False)])), ["a"], True),  # not (MISSING and FALSE)
    (cu.EVERY, ("not", ("or", [("is", ["f"], "null"), ("cmp", "=", [], "b", False)])), ["a"], False),  # not (MISSING or FALSE) = MISSING
]


@pytest.mark.parametrize("mode,cond,array,want", TRUTHS, ids=[str(i) for i in range(len(TRUTHS))])
def test_the_directed_rules(mode, cond, array, want):
    assert cu.coll_mirror(mode, cond, array) is want
    assert cu.coll_mirror(mode, cond, array, early_exit=False) is want  # early exit does not change the answer
    assert bool(cu.host_eval(cu.term_text(mode, cond), cu.texts_of([array]))[0]) is want


def test_the_mirror_types_the_binding_value_as_collEval_does():
    for mode in (cu.ANY, cu.EVERY, cu.ANY_EVERY):
        assert cu.coll_mirror(mode, EQ_T1, M) is M
        for v in (None, "t_1", 5, True, {"a": ["t_1"]}):  # an OBJECT too: no name variable, no descend
            assert cu.coll_mirror(mode, EQ_T1, v) is None


def test_the_mirror_gives_the_references_filestore_rows():
    """case_where.json 11 and 13 and the Filter of case_group_by_having.json 8 over the catalog documents, by the mirror alone."""
    docs = [d["doc"] for d in gu.load_docs("catalog")]
    genre = lambda d: d.get("details", {}).get("genre", M)  # noqa: E731
    crime = lambda d: cu.coll_mirror(cu.ANY, ("cmp", "=", [], "Crime", False), genre(d)) is True  # noqa: E731
    english = lambda d: cu.coll_mirror(cu.ANY, ("cmp", "=", [], "english", False), d.get("tags", M)) is True  # noqa: E731
    assert [d["title"] for d in docs if crime(d) and english(d) and d["pricing"]["pct_savings"] > 10.55] == ["Sherlock: Series 1"]
    thriller = [d["title"] for d in docs if d["dimensions"]["height"] > 0.5 and cu.coll_mirror(cu.ANY, ("cmp", "=", [], "Thriller", False), genre(d)) is True]
    assert sorted(thriller) == ["Inferno", "Sherlock: Series 1", "Zero Dark Thirty"]


def test_host_evaluator_equals_the_mirror_on_seeded_pairs():
    import test_gpu_coll as tg
    total = hits = 0
    seen = set()
    for mode, cond, arrays in cu.random_pairs(*tg.CPU_PAIRS):
        got = cu.host_eval(cu.term_text(mode, cond), cu.texts_of(arrays))
        for g, a in zip(got, arrays):
            want = cu.coll_mirror(mode, cond, a)
            assert bool(g) is want and g in (0, 1), (cu.term_text(mode, cond), cu.canon(a), int(g), want)
            hits += want
            total += 1
            seen.update(type(x).__name__ for x in a)
            seen.add("empty" if not a else "nonempty")
    assert total >= 20000 and 0.1 < hits / total < 0.9, (total, hits)  # the alphabet makes both answers common
    assert {"empty", "str", "int", "float", "NoneType", "bool", "list", "dict"} <= seen


def test_not_around_the_term_and_the_row_rule():
    """NOT ANY is not EVERY NOT: over [NULL] ANY (v = x) is FALSE, so NOT ANY is TRUE, while EVERY (NOT v = x) is FALSE."""
    assert cu.coll_mirror(cu.ANY, EQ_T1, [None]) is False and cu.coll_mirror(cu.EVERY, ("not", EQ_T1), [None]) is False
    bits = cu.host_eval(cu.term_text(cu.ANY, EQ_T1), [b"[null]", b"[\"t_1\"]", b"\"t_1\"", b"{\"a\":[\"t_1\"]}", b"[", b"", b"[\"t_1\""])
    assert bits.tolist() == [0, 1, 0, 0, 0, 0, 1]  # text that is no array gives no bit; an unterminated one does no harm


D = lambda name: "(`d`.`%s`)" % name  # noqa: E731


def accepted(cond, keys=(), aggs=(), filter_only=True):
    return query_amd.GpuFilterGroup(plan.filter_group_plan(cond, list(keys), list(aggs), filter_only=filter_only))


ACCEPTED = [
    'any `v` in %s satisfies (`v` = "x") end' % D("a"),
    'every `v` in %s satisfies (`v` = "x") end' % D("a"),
    'any and every `v` in %s satisfies (`v` = "x") end' % D("a"),
    'any `a` in %s satisfies ("x" = `a`) end' % D("a"),
    'any `v` in ((`d`.`b`).`a`) satisfies (not (`v` = 1.5)) end',
    'any `ord` in %s satisfies ((`ord`.`productId`) = "tea111") end' % D("a"),
    'any `v` in %s satisfies (20 < (`v`.`x`)) end' % D("a"),
    'every `v` in %s satisfies (((`v`.`f`).`g`) between 1 and 2.5) end' % D("a"),
    'any `v` in %s satisfies (`v` between "a" and "b") end' % D("a"),
    'any `v` in %s satisfies ((`v` like "%%0") or (`v` is not null) or ((`v`.`f`) is missing) or (`v` is valued)) end' % D("a"),
    'any `v` in %s satisfies (`v` < "m") end' % D("a"),
    'any `v` in %s satisfies (true = `v`) end' % D("a"),
    'any `v` in cover (%s) satisfies (`v` = 3) end' % D("a"),
]


@pytest.mark.parametrize("term", ACCEPTED)
def test_create_accepts_the_subset_and_reports_the_binding_expression_as_a_column(term):
    want = term.split(" in ")[1].split(" satisfies ")[0]
    for cond, paths in ((term, [want]), ("(%s and (3 < %s))" % (term, D("n")), [want, D("n")]),
                        ("((not %s) or (%s is null))" % (term, D("n")), [want, D("n")])):
        op = accepted(cond)
        assert op.column_paths == paths and op.coll_stats()["predicates"] == 1, (cond, op.column_paths)
        op.done()
    assert cu.host_status(term.encode()) == _ffi.OK


REFUSED = [
    ('any `v` within %s satisfies (`v` = 1) end' % D("a"), "WITHIN"),
    ('any `n` : `v` in %s satisfies (`v` = 1) end' % D("a"), "name variable"),
    ('any `v` in %s, `w` in %s satisfies (`v` = 1) end' % (D("a"), D("b")), "several bindings"),
    ('any `v` in ["a", "b"] satisfies (`v` = "a") end', "constant array"),
    ('any `v` in tokens(%s) satisfies (`v` = "a") end' % D("a"), "tokens"),
    ('any `v` in array (`o`.`p`) for `o` in %s end satisfies (`v` = "a") end' % D("a"), "array"),
    ('any `v` in (%s + 1) satisfies (`v` = "a") end' % D("a"), "not a leaf path"),
    ('every `c` in %s satisfies (%s < (`c`.`name`)) end' % (D("a"), D("name")), "outer reference"),
    ('any `v` in %s satisfies ((meta(`d`).`id`) = `v`) end' % D("a"), "meta()"),
    ('any `v` in %s satisfies ((meta(`d`).`id`) = "k") end' % D("a"), "meta()"),
    ('every `v` in %s satisfies (5 < length(`v`)) end' % D("a"), "length"),
    ('any `v` in %s satisfies (lower(to_string(`v`)) = "a") end' % D("a"), "lower"),
    ('any `v` in %s satisfies contains(`v`, "a") end' % D("a"), "contains"),
    ('any `v` in %s satisfies (`v` = [1]) end' % D("a"), "array constructor"),
    ('any `v` in %s satisfies `v` end' % D("a"), "truth"),
    ('any `v` in %s satisfies any `w` in `v` satisfies (`w` = 1) end end' % D("a"), "nested"),
    ('any `v` in %s satisfies (`v` = null) end' % D("a"), "NULL"),
    ('any `v` in %s satisfies (30 < ((`v`.`x`) + (`v`.`y`))) end' % D("a"), "arithmetic"),
    ('any `v` in %s satisfies ((((`v`.`f`).`g`).`h`) = 1) end' % D("a"), "field names"),
    ('any `v` in %s satisfies ((`v`[0]) = 1) end' % D("a"), "element access"),
    ('any `v` in %s satisfies (10 < `v`) end' % D("a"), "bare variable"),
    ('any `v` in %s satisfies (`v` between 1 and 5) end' % D("a"), "bare variable"),
    ('any `v` in %s satisfies (`v` like (`v`.`p`)) end' % D("a"), "constant"),
    ('any `v` in %s satisfies (%s) end' % (D("a"), " or ".join('(`v` = "c%d")' % i for i in range(18))), "16 nodes"),
    ('any `v` in %s satisfies (`v` = "%s") end' % (D("a"), "x" * 300), "256 bytes"),
]


@pytest.mark.parametrize("term,word", REFUSED, ids=[w.replace(" ", "_") + str(i) for i, (_, w) in enumerate(REFUSED)])
def test_create_refuses_everything_else_and_names_the_construct(term, word):
    for cond in (term, "(%s and (3 < %s))" % (term, D("n"))):
        with pytest.raises(query_amd.N1kError) as ei:
            accepted(cond)
        assert ei.value.status == _ffi.UNSUPPORTED and word in ei.value.message, ei.value.message
    assert cu.host_status(term.encode()) == _ffi.UNSUPPORTED
    assert cu.host_status(b"(3 < 4)") == _ffi.INVALID and cu.host_status(b"any `v` in") == _ffi.INVALID


def test_like_patterns_and_collection_predicates_share_eight_bits():
    terms = ['any `v` in %s satisfies (`v` = "c%d") end' % (D("a"), i) for i in range(5)]
    likes = ['(%s like "p%d%%")' % (D("s"), i) for i in range(3)]
    op = accepted("(%s)" % " or ".join(terms + likes + terms[:2] + likes[:1]))  # (a repeated term or pattern shares its bit)
    assert op.coll_stats()["predicates"] == 5 and op.like_stats()["patterns"] == 3
    op.done()
    for extra in ('any `v` in %s satisfies (`v` = "c9") end' % D("a"), 'any `v` in %s satisfies (`v` = "c0") end' % D("b"), '(%s like "q%%")' % D("s")):
        for cond in ("(%s)" % " or ".join(terms + likes + [extra]), "(%s)" % " or ".join([extra] + likes + terms)):
            with pytest.raises(query_amd.N1kError) as ei:
                accepted(cond)
            assert ei.value.status == _ffi.UNSUPPORTED and "more than 8" in ei.value.message, ei.value.message


def test_having_takes_the_term_over_a_group_key():
    term = 'any `v` in %s satisfies (`v` = "x") end' % D("a")
    op = query_amd.GpuFilterGroup(plan.filter_group_plan(None, [D("a")], ["count(*)"], having="(not %s)" % term))
    assert op.column_paths == [D("a")]
    op.done()


@pytest.mark.parametrize("kind", ["TAGGED64", "DICT32"])
def test_two_term_collection_plan_compiles_for_gfx950_without_a_gpu(kind):
    """scan_spec_kernel / scan_spec_records_kernel / scan_spec_partition_body with a collection term, through hiprtc."""
    pj = plan.filter_group_plan('(any `v` in %s satisfies (`v` = "t_1") end and (5 < %s))' % (D("a"), D("x")), [D("k")], ["sum(%s)" % D("x")])
    op = query_amd.GpuFilterGroup(pj)
    assert op.column_paths == [D("a"), D("x"), D("k")]
    akind = _ffi.COL_DICT32 if kind == "DICT32" else _ffi.COL_TAGGED64
    kinds = np.array([akind, _ffi.COL_TAGGED64, _ffi.COL_DICT32], dtype=np.uint32)
    log = C.create_string_buffer(8192)
    st = _ffi.lib().n1k_jit_check(op._h, kinds.ctypes.data, 3, log, 8192)
    assert st == _ffi.OK, log.value.decode(errors="replace")
    op.done()


def test_golden_any_fixture_holds_the_references_statements():
    with open(os.path.join(gu.GOLDEN, "cases_any.json")) as fh:
        fx = json.load(fh)
    assert [(c["source"], c["index"]) for c in fx["cases"]] == [("filestore/case_where.json", 11), ("filestore/case_where.json", 13),
                                                                ("filestore/case_group_by_having.json", 8)]
    for c in fx["cases"]:  # each plan is one the library takes, over the leaf paths the fixture names
        p = c["plan"]
        op = query_amd.GpuFilterGroup(plan.filter_group_plan(p["condition"], p.get("group_keys", []), p.get("aggregates", []),
                                                             filter_only=bool(p.get("filter_only")), having=c.get("having_text")))
        assert op.column_paths == c["columns"] and all(k == "catalog" for k in [c["keyspace"]])
        op.done()


def test_the_library_takes_every_plan_of_the_gpu_differential():
    """tests/test_gpu_coll.py counts a skip or N1K_UNSUPPORTED as a failure; that its generator draws only the accepted subset
    is checked here, without a GPU, by creating every plan of its seeds.  Its bounded plans run with `spec` off and read
    stats["spec_kernel"] == 0, which the interpreter reports too: n1k_jit_check answers N1K_UNSUPPORTED unless
    build_fast_args takes the plan — here every distinct bounded shape those seeds draw, collection term included."""
    import test_gpu_coll as tg
    seen = set()
    classes = set()
    for seed in range(tg.NSEEDS):
        _, t, opts, bounded, _, sub, dcond, ocond, keys, aggs = tg.draw(seed)
        assert " satisfies " in dcond and " satisfies " not in ocond
        for fo in (True, False):
            op = query_amd.GpuFilterGroup(plan.filter_group_plan(dcond, [] if fo else keys, [] if fo else aggs, filter_only=fo))
            assert 1 <= op.coll_stats()["predicates"] <= 3
            paths = op.column_paths
            op.done()
        classes.update(k for k in ("(`default`.`a`) satisfies", "(`default`.`s`) satisfies", " like ", " between ", "every ", "any and every ") if k in dcond)
        if not bounded or opts != {"spec": 0}:
            continue
        op = query_amd.GpuFilterGroup(plan.filter_group_plan(dcond, keys, aggs))
        by_name = {c.name: c for c in t.columns}
        kinds = np.array([by_name[p].kind for p in op.column_paths], dtype=np.uint32)
        shape = (tuple(kinds.tolist()), tuple(op.column_paths), dcond.startswith("(any") or dcond.startswith("(every"), " and " in dcond, tuple(aggs))
        if shape not in seen and len(seen) < 6:
            seen.add(shape)
            log = C.create_string_buffer(4096)
            st = _ffi.lib().n1k_jit_check(op._h, kinds.ctypes.data, len(kinds), log, 4096)
            assert st == _ffi.OK, (st, dcond, keys, aggs, log.value.decode(errors="replace"))
        op.done()
    assert len(seen) >= 4 and len(classes) == 6, (len(seen), classes)


def test_the_count_distinct_plan_of_the_gpu_suite_is_a_bounded_shape():
    import test_gpu_coll as tg
    t, _, dcond, _, keys, aggs = tg.distinct_plan(1500, n=64)
    op = query_amd.GpuFilterGroup(plan.filter_group_plan(dcond, keys, aggs))
    by_name = {c.name: c for c in t.columns}
    kinds = np.array([by_name[p].kind for p in op.column_paths], dtype=np.uint32)
    log = C.create_string_buffer(4096)
    st = _ffi.lib().n1k_jit_check(op._h, kinds.ctypes.data, len(kinds), log, 4096)
    assert st == _ffi.OK, (st, log.value.decode(errors="replace"))
    op.done()
