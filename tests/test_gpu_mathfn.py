"""Trig, EXP / LN / LOG / POWER, DEGREES / RADIANS, the constants and IFINF ... NEGINFIF on the device: the reference's
statements, every function element-wise against the yardstick (tests/mathfn_util.py), the fused route, the grouped tail, and a
differential against the oracle BY SUBSTITUTION as tests/test_gpu_cond.py does it — the oracle does not know these functions,
so where the device's plan holds one the oracle's reads a TAGGED64 helper column with the yardstick's value of every row.

mathfn_kernel<OP> (n1k_mathfn.hip) has arith_kernel's geometry: one row per lane, 64-lane waves, 256-lane workgroups.  Its
edges are therefore 1, 63, 64, 65, 255, 256, 257 rows and 3 workgroups + 1 = 769."""
import collections
import functools
import math

import numpy as np
import pytest

import cond_util as cn
import golden_util as gu
import mathfn_util as mu
import parity_util as pu
import query_amd
from oracle import n1o
from query_amd import plan

pytestmark = pytest.mark.gpu

D = mu.D
M = mu.MISSING
NUM_CASES = mu.load_cases()
NSEEDS = 120  # NOTE: tests/test_mathfn_cpu.py creates every plan drawn here without a GPU
KERNEL_EDGES = [1, 63, 64, 65, 255, 256, 257, 769]


def must_run(fn, *a, **kw):
    """a refusal is a failure here, never a skip"""
    try:
        return fn(*a, **kw)
    except query_amd.N1kError as e:
        raise AssertionError("the device refused: %s" % e.message)


# ------------------------------------------------------------------ the reference's statements

@pytest.mark.parametrize("case", NUM_CASES, ids=[c["id"] for c in NUM_CASES])
def test_the_references_numeric_statements(case):
    """The routes tests/test_gpu_parity.py uses: a constant expression as the group key of a one-row table, a per-document one
    as the operand of MAX with one group per document."""
    docs = gu.load_docs(case["keyspace"])
    p = case["plan"]
    if "exprs" in p:
        (alias, text), = p["exprs"]
        rows, _ = must_run(pu.run_gpu, gu.build_table(docs[:1], []), None, [text], ["count(*)"])
        assert len(rows.keys) == 1
        got = [{alias: gu.decode_value(rows.keys[0][0])}]
    else:
        alias, text = p["row_expr"]
        idp = "(`game`.`id`)"
        table = gu.build_table(docs, gu.leaf_paths({"condition": None, "group_keys": [idp, text], "aggregates": []}))
        rows, _ = must_run(pu.run_gpu, table, None, [idp], ["max(%s)" % text])
        assert len(rows.keys) == len(docs)
        vals = [gu.decode_value(a[0]) for a in rows.aggs]
        got = [{alias: v} for v in mu.nan_first(vals)]
    want = case["results"]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        wv = w[alias]
        assert mu.same_value(g[alias], mu.NAN if wv == "NaN" else wv, case["exact"]), (case["id"], got, want)


# ------------------------------------------------------------------ element-wise, per function

ELEMENT_FUNCTIONS = mu.UNARY + mu.BINARY + mu.IFNUM


def element_plan(name, first="v"):
    return (None, [D("id")], ["max(%s)" % mu.value_text(mu.elem_node(name, first=first))])


ELEMENT_PLANS = [element_plan(n) for n in ELEMENT_FUNCTIONS] + [element_plan(n, "s") for n in ELEMENT_FUNCTIONS]


@functools.lru_cache(maxsize=None)
def element_rows(name, n):
    rows = mu.elem_rows(n, name)
    return rows, mu.elem_table(rows)


def check_element_wise(name, n, first):
    rows, table = element_rows(name, n)
    node = mu.elem_node(name, first=first)
    cond, keys, aggs = element_plan(name, first)
    out, st = must_run(pu.run_gpu, table, cond, keys, aggs)
    assert st["rows_in"] == n and len(out.keys) == n
    got = {gu.decode_value(k[0]): gu.decode_value(a[0]) for k, a in zip(out.keys, out.aggs)}
    exact = name not in mu.LIBRARY
    for r in rows:
        want = mu.eval_value(node, r)
        g = got[r["id"]]
        if want is M:  # (MAX skips MISSING and NULL alike: a group of one such row is NULL)
            want = None
        assert mu.same_value(g, want, exact), "%s row %d of %d: v %r w %r s %r: device %r yardstick %r" % (name, r["id"], n, r["v"], r["w"], r["s"], g, want)


@pytest.mark.parametrize("n", KERNEL_EDGES)
@pytest.mark.parametrize("name", ELEMENT_FUNCTIONS)
def test_every_row_of_the_element_wise_kernel(name, n):
    """MAX(f(v[, w])) GROUP BY id, a TAGGED64 operand with every value class and the special-case table's numbers"""
    check_element_wise(name, n, "v")


@pytest.mark.parametrize("name", ELEMENT_FUNCTIONS)
def test_a_dictionary_coded_operand_is_null_or_missing(name):
    """f(s) over a DICT32 column: NULL for every string and for NULL, MISSING by its code"""
    check_element_wise(name, 257, "s")


def test_missing_and_null_are_told_apart():
    """(MAX folds both to NULL: COUNT over `is missing` / `is null` of the node tells them apart, per function)"""
    rows, table = element_rows("sin", 769)
    for name in ELEMENT_FUNCTIONS:
        node = mu.elem_node(name)
        text = mu.value_text(node)
        vals = [mu.eval_value(node, r) for r in rows]
        for pred, want in (("missing", sum(v is M for v in vals)), ("null", sum(v is None for v in vals))):
            out, st = must_run(pu.run_gpu, table, "(%s is %s)" % (text, pred), [], ["count(*)"])
            assert st["rows_selected"] == want, (name, pred, st["rows_selected"], want)


# ------------------------------------------------------------------ the fused route

PRICE, CAT = D("price"), D("cat")
# name -> (condition, keys, aggregates) of the device, with {h} where the oracle reads the helper column
FUSED_NODES = {
    "unary-in-where": (("num", "exp", [("arith", "/", ("col", "price"), ("const", 10))]), "(2 < {h})", ["sum(%s)" % PRICE]),
    "power-operand": (("num", "power", [("col", "price"), ("const", 2)]), None, ["sum({h})"]),
    "chain": (("num", "ln", [("arith", "+", ("num", "exp", [("col", "price")]), ("const", 1))]), "(50 < %s)" % PRICE, ["sum({h})"]),
}


def fused_plan(name, h):
    _node, cond, aggs = FUSED_NODES[name]
    return (cond.format(h=h) if cond else None, [CAT], [a.format(h=h) for a in aggs])


FUSED_SHAPES = {name: fused_plan(name, mu.value_text(FUSED_NODES[name][0])) for name in FUSED_NODES}


@functools.lru_cache(maxsize=None)
def fused_table():
    t = n1o.synth_table(70_001, k_cat=12)
    price = next(c for c in t.columns if c.name == PRICE)
    assert set(price.tags.tolist()) <= {n1o.T_MISSING, n1o.T_NULL, n1o.T_INT, n1o.T_FLOAT, n1o.T_STRING}
    # (a STRING price — the synthetic column holds some, and they pass `50 < price` — is any string to the yardstick: NULL under every function)
    vals = [M if tg == n1o.T_MISSING else None if tg == n1o.T_NULL else "a" if tg == n1o.T_STRING else int(np.uint64(p).view(np.int64)) if tg == n1o.T_INT
            else float(np.uint64(p).view(np.float64)) for tg, p in zip(price.tags.tolist(), price.payload.tolist())]
    return t, vals


@pytest.mark.parametrize("name", sorted(FUSED_NODES))
def test_library_functions_fused_into_the_runtime_built_scan(name):
    """jit = 2 at the sizes of test_arithmetic_fused_into_the_runtime_built_scan: the nodes in the scan's registers
    (spec_kernel 3), and the same plan materialised (fuse_arith off); both against the oracle by substitution."""
    t, prices = fused_table()
    node = FUSED_NODES[name][0]
    values = [mu.eval_value(node, {"price": p}) for p in prices]
    if name == "unary-in-where":  # the input rule: the constant keeps 1e-6 relative off every value the node takes
        assert all(abs(v - 2) > 2e-6 for v in values if mu.is_num(v))
    ot = n1o.Table(list(t.columns) + [cn.helper_column("h", values)], t.dictionary)
    ocond, okeys, oaggs = fused_plan(name, D("h"))
    ora = n1o.run(ot, ocond, okeys, oaggs)
    cond, keys, aggs = FUSED_SHAPES[name]
    for batches in (1, 2):
        gpu, st = must_run(pu.run_gpu, t, cond, keys, aggs, batches=batches, jit=2)
        mu.assert_same_groups(gpu, ora, oaggs, numeric=True)
        assert st["rows_selected"] == ora.rows_passed
        assert st["spec_kernel"] == 3, st
    unfused, st = must_run(pu.run_gpu, t, cond, keys, aggs, batches=2, jit=2, fuse_arith=0)
    mu.assert_same_groups(unfused, ora, oaggs, numeric=True)
    assert st["spec_kernel"] != 3 and st["rows_selected"] == ora.rows_passed


# ------------------------------------------------------------------ the grouped tail

def test_having_and_a_projection_over_the_groups():
    """HAVING ln(sum(x)) > c and round(power(avg(x), 2), 3) over the groups, against the yardstick over the oracle's groups"""
    rows = cn.make_rows(__import__("random").Random(4242), 3000)
    t = cn.make_table(rows)
    keys, aggs = [D("k")], sorted(["avg(%s)" % D("x"), "sum(%s)" % D("x")])
    ora = n1o.run(t, None, keys, aggs)
    sums = {gu.decode_value(k[0]): gu.decode_value(a[1]) for k, a in zip(ora.keys, ora.aggs)}
    avgs = {gu.decode_value(k[0]): gu.decode_value(a[0]) for k, a in zip(ora.keys, ora.aggs)}
    assert all(mu.is_num(s) and s > 0 for s in sums.values()) and len(sums) > 3
    lns = sorted(math.log(s) for s in sums.values())
    c = mu.threshold_for(lns)
    assert lns[0] < c < lns[-1]
    gpu, _ = must_run(pu.run_gpu, t, None, keys, aggs, having="(%s < ln(sum(%s)))" % (c, D("x")),
                      project=[(D("k"), "k"), ("round(power(avg(%s), 2), 3)" % D("x"), "p")])
    got = {gu.decode_value(r[0]): gu.decode_value(r[1]) for r in gpu.proj}
    want = {k: mu.new_value(gu.round_float(mu.fn_float("power", avgs[k], 2), 3)) for k in sums if math.log(sums[k]) > c}
    assert set(got) == set(want) and 0 < len(want) < len(sums)
    for k in want:
        assert mu.same_value(got[k], want[k], exact=False), (k, got[k], want[k])


# ------------------------------------------------------------------ IFINF / IFNAN / IFNANORINF and NANIF / POSINFIF / NEGINFIF

def key_name(v):
    """a value as a group key: an integral float IS the int (both print alike), NaN and the infinities by their float"""
    if v is M or v is gu.MISSING:
        return "MISSING"
    n = mu.as_number(v)
    if n is None:
        return repr(v)
    return repr(n) if n != n or math.isinf(n) else repr(mu.new_value(n))


def key_counts(rows):
    out = collections.Counter()
    for k, a in zip(rows.keys, rows.aggs):
        out[key_name(gu.decode_value(k[0]))] += a[0][1]
    return dict(out)


def want_counts(values):
    return dict(collections.Counter(key_name(v) for v in values))


IF_POOL = [1, 2.5, 3.0, mu.PINF, mu.NINF, mu.NAN, M, None, "a", True, 0, -0.0]


@pytest.mark.parametrize("nargs", [2, 3, 4])
@pytest.mark.parametrize("name", mu.IFNUM)
def test_ifinf_ifnan_ifnanorinf_in_argument_order(name, nargs):
    """every pair / triple / quadruple of the pool (sampled with co-prime strides): a MISSING behind a taken argument is not
    reached, one in front of it is; checked exactly, as group keys"""
    n = len(IF_POOL)
    rows = [{"c%d" % k: IF_POOL[(i // n ** k + 5 * k * i) % n] for k in range(4)} for i in range(n * n * 4)]
    node = ("num", name, [("col", "c%d" % k) for k in range(nargs)])
    t = n1o.Table([cn.helper_column("c%d" % k, [r["c%d" % k] for r in rows]) for k in range(4)], list(cn.DICT))
    out, _ = must_run(pu.run_gpu, t, None, [mu.value_text(node)], ["count(*)"])
    values = [mu.eval_value(node, r) for r in rows]
    assert any(v is M for v in values) and any(v is None for v in values) and any(isinstance(v, int) for v in values)
    assert key_counts(out) == want_counts(values)
    # the order matters: (1, MISSING) is 1, (MISSING, 1) is MISSING
    assert mu.fn_apply(name, [1, M]) == 1 and mu.fn_apply(name, [M, 1]) is M


@pytest.mark.parametrize("name", sorted(mu.EQNUM))
def test_nanif_posinfif_neginfif(name):
    pool = [3, 3.0, 4, 2.5, "a", "ab", None, M, True, mu.PINF, mu.NINF]
    rows = [{"a": a, "b": b} for a in pool for b in pool]
    t = n1o.Table([cn.helper_column("a", [r["a"] for r in rows]), cn.helper_column("b", [r["b"] for r in rows])], list(cn.DICT))
    for second in (("col", "b"), ("const", 3), ("const", "a")):
        node = ("cond", name, [("col", "a"), second])
        out, _ = must_run(pu.run_gpu, t, None, [mu.value_text(node)], ["count(*)"])
        assert key_counts(out) == want_counts([mu.eval_value(node, r) for r in rows]), (name, second)


def test_the_existing_conditional_modes_did_not_move():
    """tests/test_gpu_cond.py's directed NULLIF / MISSINGIF case, rerun unchanged"""
    import test_gpu_cond as tc
    tc.test_nullif_compares_numbers_by_value_and_missingif_gives_a_missing_key()


# ------------------------------------------------------------------ differential by substitution

FAMILIES = [{"fast": 0}, {}, {"spec": 0}, {"jit": 0}]


@pytest.mark.parametrize("seed", range(NSEEDS))
def test_numeric_function_plans_agree_with_the_oracle_by_substitution(seed):
    p = mu.draw_plan(seed)
    opts = FAMILIES[seed % len(FAMILIES)]
    t = cn.make_table(p["rows"])
    ot = n1o.Table(list(t.columns) + [cn.helper_column("h", p["values"])], t.dictionary)
    (dcond, dkeys, daggs), (ocond, okeys, oaggs) = p["device"], p["oracle"]
    what = "seed %d use %s device %r %r %r opts %r" % (seed, p["use"], dcond, dkeys, daggs, opts)
    ora = n1o.run(ot, ocond, okeys, oaggs, threads=2)
    gpu, st = must_run(pu.run_gpu, t, dcond, dkeys, daggs, batches=1 + seed % 3, **opts)
    try:
        mu.assert_same_groups(gpu, ora, oaggs, numeric=p["numeric"])
    except AssertionError as e:
        raise AssertionError("%s | %s" % (e, what))
    assert st["rows_selected"] == ora.rows_passed, what
    if p["use"].startswith("filter"):  # the Filter alone: the selected row ordinals, as they come
        gsel, _ = must_run(pu.run_gpu, t, dcond, [], [], filter_only=True, batches=1 + seed % 2)
        osel = n1o.run(ot, ocond, [], [], has_group=False)
        assert np.array_equal(np.asarray(gsel.selected, dtype=np.uint64), osel.selected), what
