"""Trig, EXP / LN / LOG / POWER, DEGREES / RADIANS, the five constants and IFINF ... NEGINFIF as values, without a GPU: what
n1k_create accepts and refuses, and the yardstick (tests/mathfn_util.py) against the reference's statements and a hand-written
table of special cases."""
import math

import pytest

import golden_util as gu
import mathfn_util as mu
import query_amd
from query_amd import _ffi, plan

M = mu.MISSING
D = lambda name: plan.field_path("d", name)  # noqa: E731
NUM_CASES = mu.load_cases()


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


def call(name, a="a", b="b"):
    """the function over columns, with as many arguments as it takes at least"""
    lo = plan.NUM_FUNCTIONS[name][0] if name in plan.NUM_FUNCTIONS else 2
    return (plan.num_fn if name in plan.NUM_FUNCTIONS else plan.cond_fn)(name, *[D(a), D(b)][:lo])


def cols(name, a="a", b="b"):
    lo = plan.NUM_FUNCTIONS[name][0] if name in plan.NUM_FUNCTIONS else 2
    return [D(a), D(b)][:lo]


VALUE_FUNCTIONS = mu.UNARY + mu.BINARY + mu.IFNUM  # arithmetic-style nodes: everywhere round(...) may stand
ALL_FUNCTIONS = VALUE_FUNCTIONS + tuple(mu.EQNUM)  # ... and the three CondNode modes: everywhere nullif(...) may stand


@pytest.mark.parametrize("name", ALL_FUNCTIONS)
def test_every_function_is_accepted_in_each_place_with_its_paths_in_text_order(name):
    f, c = call(name), cols(name)
    k = D("k")
    rest = [p for p in [k] if p not in c]
    # operand of a Filter comparison, group key, aggregate operand, operand of arithmetic, WHEN operand and THEN / ELSE of a CASE
    assert paths_of("(%s < 2)" % f, [k], ["count(*)"]) == c + rest
    assert paths_of(None, [f], ["count(*)"]) == c
    assert paths_of(None, [k], ["sum(%s)" % f]) == [k] + c
    assert paths_of(None, [k], ["max((%s + 1))" % f]) == [k] + c
    case = plan.case_when([("(%s < 1)" % f, f)], "(%s * 2)" % f)
    assert paths_of(None, [k], ["min(%s)" % case]) == [k] + c
    # argument of one another, and of round
    assert paths_of(None, [k], ["sum(round(%s, 2))" % plan.num_fn("atan", f)]) == [k] + c
    assert paths_of("(0 < %s)" % f, [], [], filter_only=True) == c


@pytest.mark.parametrize("name", VALUE_FUNCTIONS)
def test_the_value_functions_stand_in_having_and_in_a_projection_over_groups(name):
    two = name in mu.BINARY or name in mu.IFNUM
    over = "%s(sum(%s)%s)" % (name, D("x"), ", 2" if two else "")
    assert paths_of(None, [D("k")], ["sum(%s)" % D("x")], having="(%s < 5)" % over) == [D("k"), D("x")]
    assert paths_of(None, [D("k")], ["sum(%s)" % D("x")], project=[("round(%s, 3)" % over, "v"), (D("k"), None)]) == [D("k"), D("x")]


def test_upper_case_names_are_the_same_functions():
    text = "POWER(LN(%s), ATAN2(%s, PI()))" % (D("a"), D("b"))
    assert paths_of("(IFNAN(%s, 0) < DEGREES(E()))" % text, [], ["count(*)"]) == [D("a"), D("b")]
    assert paths_of(None, ["NANIF(%s, NegInf())" % D("a")], ["count(*)"]) == [D("a")]


@pytest.mark.parametrize("name", sorted(mu.NULLARY))
def test_a_nullary_function_is_a_constant_and_leaves_no_column(name):
    assert paths_of("(%s < %s)" % (D("a"), plan.num_fn(name)), [], ["count(*)"]) == [D("a")]
    assert paths_of(None, [plan.num_fn(name)], ["count(*)"]) == []


REFUSED = {
    "random with a seed": (None, ["random(5)"], ["count(*)"], {}, "random"),
    "random without one": ("(random() < 0.5)", [], ["count(*)"], {}, "random"),
    "a fifth ifinf argument": (None, ["ifinf(%s, %s, %s, %s, 1)" % (D("a"), D("b"), D("c"), D("e"))], ["count(*)"], {}, "ifinf with 5 arguments"),
    "a fifth ifnanorinf argument": (None, [D("k")], ["sum(ifnanorinf(%s, %s, %s, %s, 0))" % (D("a"), D("b"), D("c"), D("e"))], {}, "ifnanorinf with 5 arguments"),
    "a sort term": ("(0 < %s)" % D("a"), [], [], {"filter_only": True, "order": [(plan.num_fn("sin", D("a")), False)]}, "sin("),
    "a DISTINCT term": ("(0 < %s)" % D("a"), [], [], {"filter_only": True, "distinct": [(plan.num_fn("exp", D("a")), "x")]}, "exp("),
    "inside SATISFIES": ("any `v` in %s satisfies (ln(`v`) < 1) end" % D("a"), [], ["count(*)"], {}, "ln"),
    "nanif in HAVING": (None, [D("a")], ["count(*)"], {"having": "(nanif(count(*), 1) < 3)"}, "HAVING: CASE or a conditional function"),
    "posinfif in a projection over groups": (None, [D("a")], ["count(*)"], {"project": [("posinfif(count(*), 1)", "x")]}, "CASE or a conditional function as a projection term"),
}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_each_refusal_is_unsupported_and_names_its_construct(what):
    condition, keys, aggs, kw, names = REFUSED[what]
    e = refusal(condition, keys, aggs, **kw)
    assert e.status == _ffi.UNSUPPORTED, (e.status, e.message)
    assert names in e.message, e.message


def test_four_arguments_are_taken():
    for name in mu.IFNUM:
        assert paths_of(None, [plan.num_fn(name, D("a"), D("b"), D("c"), D("e"))], ["count(*)"]) == [D("a"), D("b"), D("c"), D("e")]


MALFORMED = ["sin()", "sin(%s, 1)" % D("a"), "power(%s)" % D("a"), "atan2(%s, 1, 2)" % D("a"), "pi(1)", "nan(%s)" % D("a"), "ifinf(%s)" % D("a"),
             "nanif(%s)" % D("a"), "neginfif(%s, 1, 2)" % D("a"), "ln(%s" % D("a"), "exp(%s, )" % D("a")]


@pytest.mark.parametrize("text", MALFORMED)
def test_a_wrong_argument_count_is_invalid(text):
    e = refusal(None, [text], ["count(*)"])
    assert e.status == _ffi.INVALID, (e.status, e.message)


def test_num_fn_writes_the_stringers_text_and_checks_its_arguments():
    assert plan.num_fn("POWER", D("x"), "2") == "power((`d`.`x`), 2)"
    assert plan.num_fn("pi") == "pi()"
    for bad in (("power", D("x")), ("pi", "1"), ("round", D("x")), ("ifinf", D("x"))):
        with pytest.raises(ValueError):
            plan.num_fn(*bad)
    assert plan.cond_fn("nanif", D("x"), "3") == "nanif((`d`.`x`), 3)"


# ---------------------------------------------------------------- the yardstick

def eval_text_case(case):
    """the yardstick's rows for a golden case: its expression parsed by hand below (the texts are few and regular)"""
    docs = gu.load_docs(case["keyspace"])
    p = case["plan"]
    if "exprs" in p:
        (alias, text), = p["exprs"]
        return [{alias: eval_text(text, None)}]
    alias, text = p["row_expr"]
    vals = [eval_text(text, d["doc"]["score"]) for d in docs]
    return [{alias: v} for v in mu.nan_first(vals)]


def eval_text(text, score):
    """a tiny evaluator of the fixture's stringer texts over the yardstick"""
    import re
    toks = re.findall(r"`game`\.`score`|[a-z0-9_]+(?=\()|-?\d+(?:\.\d+)?|[()/,\-]", text)
    pos = [0]

    def peek():
        return toks[pos[0]] if pos[0] < len(toks) else None

    def take(t=None):
        x = toks[pos[0]]
        assert t is None or x == t, (text, x, t)
        pos[0] += 1
        return x

    def primary():
        t = take()
        if t == "(":
            if peek() == "-":
                take()
                v = primary()
                take(")")
                return mu.arith("-", 0, v) if v != 0 else v
            if peek() == "`game`.`score`":
                take()
                take(")")
                return score
            a = primary()
            if peek() == "/":
                take()
                b = primary()
                take(")")
                return mu.arith("/", a, b)
            take(")")
            return a
        if re.fullmatch(r"-?\d+(?:\.\d+)?", t):
            return mu.new_value(float(t))
        take("(")
        args = []
        while peek() != ")":
            args.append(primary())
            if peek() == ",":
                take()
        take(")")
        if t == "sign":
            return mu.new_value(-1.0 if args[0] < 0 else (1.0 if args[0] > 0 else 0.0))
        return mu.fn_apply(t, args)

    v = primary()
    assert pos[0] == len(toks), (text, toks)
    return v


@pytest.mark.parametrize("case", NUM_CASES, ids=[c["id"] for c in NUM_CASES])
def test_the_yardstick_gives_the_references_results(case):
    got = eval_text_case(case)
    want = case["results"]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        (alias, wv), = w.items()
        assert mu.same_value(g[alias], mu.as_number(wv) if wv == "NaN" else wv, case["exact"]), (case["id"], g, w)


@pytest.mark.parametrize("i", range(len(mu.SPECIALS)))
def test_the_yardstick_gives_the_hand_written_special_cases(i):
    name, args, want = mu.SPECIALS[i]
    got = mu.fn_apply(name, args)
    assert mu.special_matches(got, want), (name, args, got, want)
    row = {"c%d" % k: a for k, a in enumerate(args)}
    assert mu.special_matches(mu.eval_value(("num", name, [("col", "c%d" % k) for k in range(len(args))]), row), want)


@pytest.mark.parametrize("name", sorted(mu.EQNUM))
def test_the_yardstick_on_nanif_and_its_siblings(name):
    for (a, b), want in mu.EQ_SPECIALS:
        got = mu.cond_apply(name, [a, b])
        if isinstance(want, str) and want == "hit":
            assert isinstance(got, float) and (got != got if name == "nanif" else got == mu.EQNUM[name]), (name, a, b, got)
        elif isinstance(want, float) and want != want:  # NaN equals nothing, itself included: `first` comes back
            assert got != got
        else:
            assert got is want or (got == want and type(got) is type(want)), (name, a, b, got)


@pytest.mark.parametrize("name", mu.UNARY + mu.BINARY)
def test_the_element_wise_table_holds_every_special_case_of_the_function(name):
    """what tests/test_gpu_mathfn.py runs on the device at 769 rows (and from 64 rows on) includes every argument list of the
    hand-written table — for POWER and ATAN2 every (first, second) pair — unchanged by the input rules"""
    want = mu.special_args(name)
    assert want and (name not in mu.BINARY or len(want) >= 25)
    same = lambda a, b: a is b or (type(a) is type(b) and (a == b or (a != a and b != b)) and  # noqa: E731
                                   (not isinstance(a, float) or math.copysign(1, a) == math.copysign(1, b)))
    for n in (64, 769):
        rows = mu.elem_rows(n, name)
        for args in want:
            assert any(same(r["v"], args[0]) and (len(args) == 1 or same(r["w"], args[1])) for r in rows), (name, args, n)
    # ... and behind them every first argument of the pool meets every second one
    if name in mu.BINARY:
        pairs = {(repr(r["v"]), repr(r["w"])) for r in mu.elem_rows(769, "atan2")}
        assert len(pairs) >= 43 * 16 - 8


def test_new_value_folds_like_the_reference():
    assert [mu.new_value(v) for v in (144.0, -0.0, 2.5, 2.0 ** 62)] == [144, 0, 2.5, 2 ** 62] and type(mu.new_value(-0.0)) is int
    assert type(mu.new_value(2.0 ** 63)) is float and math.isinf(mu.new_value(mu.PINF)) and mu.new_value(mu.NAN) != mu.new_value(mu.NAN)


def test_the_comparer_is_exact_where_it_must_be():
    assert mu.same_value(144, 144.0, exact=False) and not mu.same_value(144.0, 144, exact=True)
    assert mu.same_value(143.99999999999997, 144, exact=False) and not mu.same_value(144.0001, 144, exact=False)
    assert mu.same_value("NaN", mu.NAN, exact=True) and not mu.same_value(0.0, mu.NAN, exact=False)
    assert not mu.same_value(1e-17, 0, exact=False) and mu.same_value(0, 0.0, exact=False)
    assert mu.same_value(mu.PINF, mu.PINF, False) and not mu.same_value(1e308, mu.PINF, False)
    assert mu.same_value(M, M, True) and not mu.same_value(None, M, True) and not mu.same_value(None, 0, False)
    assert not mu.same_value(1.0000001, 1.0, exact=False)  # (a single-precision routine is caught)
    # an exact zero keeps its kind: NewValue folds 0.0 and -0.0 to INT 0
    assert mu.same_value(0, 0, exact=True) and not mu.same_value(0.0, 0, exact=True) and not mu.same_value(-0.0, 0, exact=True)


# ---------------------------------------------------------------- what the GPU tests push

def test_the_library_takes_every_plan_of_the_gpu_differential():
    """tests/test_gpu_mathfn.py counts a refusal as a failure: every plan it draws is created here, device side and oracle
    side alike; every function and every use turns up; the input rules hold."""
    import test_gpu_mathfn as tg
    uses, names = set(), set()
    for seed in range(tg.NSEEDS):
        p = mu.draw_plan(seed)
        dcond, dkeys, daggs = p["device"]
        paths = paths_of(dcond, dkeys, daggs)
        assert set(paths) <= {mu.D(c) for c in ("a", "x", "s", "k", "g")}, (seed, paths)
        ocond, okeys, oaggs = p["oracle"]
        assert mu.D("h") in paths_of(ocond, okeys, oaggs)
        uses.add(p["use"])
        text = repr(p["node"])
        names.update(n for n in ALL_FUNCTIONS + tuple(mu.NULLARY) if "'%s'" % n in text)
        if p["use"] == "key_exact":
            assert not p["numeric"], (seed, p["node"])
    assert uses == set(mu.USES)
    assert set(mu.LIBRARY) | set(mu.EXACT) <= names, sorted((set(mu.LIBRARY) | set(mu.EXACT)) - names)
    for plans in (tg.ELEMENT_PLANS, tg.FUSED_SHAPES.values()):
        for cond, keys, aggs in plans:
            paths_of(cond, keys, aggs)


@pytest.mark.parametrize("case", NUM_CASES, ids=[c["id"] for c in NUM_CASES])
def test_the_golden_expressions_are_accepted(case):
    p = case["plan"]
    if "exprs" in p:
        assert paths_of(None, [t for _a, t in p["exprs"]], ["count(*)"]) == []
    else:
        assert paths_of(None, ["(`game`.`id`)"], ["max(%s)" % p["row_expr"][1]]) == ["(`game`.`id`)", "(`game`.`score`)"]


@pytest.mark.parametrize("name", ["unary-in-where", "power-operand", "chain"])
def test_the_fused_shapes_compile_without_a_gpu(name):
    """math_apply<OP> inside the run-time-built scan: the three shapes tests/test_gpu_mathfn.py runs fused are instantiated
    through hiprtc (compile only, gfx950)."""
    import ctypes as C

    import numpy as np

    import test_gpu_mathfn as tg
    cond, keys, aggs = tg.FUSED_SHAPES[name]
    op = create(cond, keys, aggs)
    try:
        kinds = np.array([_ffi.COL_DICT32 if p == tg.CAT else _ffi.COL_TAGGED64 for p in op.column_paths], dtype=np.uint32)
        log = C.create_string_buffer(8192)
        st = _ffi.lib().n1k_jit_check(op._h, kinds.ctypes.data, len(kinds), log, 8192)
        assert st == _ffi.OK, log.value.decode(errors="replace")
    finally:
        op.done()
