"""The date functions on the device: the reference's statements, the edge pools through datefn_kernel<OP> and through the fused
scan, the string half's table kernel and lookup at their edges, the rows that must raise, and a differential against the oracle
BY SUBSTITUTION as tests/test_gpu_mathfn.py does it — the oracle does not know these functions, so where the device's plan holds
one the oracle's reads a TAGGED64 helper column with the yardstick's value (tests/datefn_util.py) of every row.  Everything is
compared exactly: tag and payload.

datefn_kernel<OP> and datestr_lookup_kernel have arith_kernel's geometry (one row per lane, 256-lane workgroups): batches of 1,
255, 256, 257 and 8193 rows.  datestr_table_kernel gives a wave 64 consecutive entries: 63, 64, 65 and 129 entries, strings of 64
and 65 bytes on both sides of what it takes."""
import functools
import json
import os
import random

import numpy as np
import pytest

import datefn_util as du
import golden_util as gu
import parity_util as pu
import query_amd
from oracle import n1o
from query_amd import _ffi, plan

pytestmark = pytest.mark.gpu

D = du.D
M = du.MISSING
T, S, K, G, W, ID = D("t"), D("s"), D("k"), D("g"), D("w"), D("id")
BATCH_EDGES = [1, 255, 256, 257, 8193]
BASE = 1463284740000

with open(os.path.join(gu.GOLDEN, "cases_date.json")) as _fh:
    GOLDEN = json.load(_fh)


def must_run(fn, *a, **kw):
    """a refusal is a failure here, never a skip"""
    try:
        return fn(*a, **kw)
    except query_amd.N1kError as e:
        raise AssertionError("the device refused: %s" % e.message)


def must_raise(table, cond, keys, aggs, **kw):
    with pytest.raises(query_amd.N1kError) as ei:
        pu.run_gpu(table, cond, keys, aggs, **kw)
    assert ei.value.status == _ffi.UNSUPPORTED_DATA, (ei.value.status, ei.value.message)


def decoded(v):
    v = gu.decode_value(v)
    return M if v is gu.MISSING else v


def P(part):
    return json.dumps(part)


# ------------------------------------------------------------------ the reference's statements

@pytest.mark.parametrize("row", GOLDEN["rows"], ids=[r["id"] for r in GOLDEN["rows"]])
def test_the_references_statements_over_constants(row):
    """a constant call as the group key of a one-row table, and the same call with its first argument in a column"""
    text = plan.date_fn(row["function"], *[du.const_text(a) for a in row["args"]])
    one = du.date_table([{"x": 1}], names_tagged=("x",), names_dict=())
    out, _ = must_run(pu.run_gpu, one, None, [text], ["count(*)"])
    assert [(k[0][0], k[0][1]) for k in out.keys] == [(n1o.T_INT, row["result"])], (row["statement"], out.keys)
    string = row["function"] in du.STRING_FUNCTIONS
    col = S if string else T
    t = du.date_table([{"s" if string else "t": row["args"][0]}], names_tagged=("t",), names_dict=("s",))
    out, _ = must_run(pu.run_gpu, t, None, [plan.date_fn(row["function"], col, *[du.const_text(a) for a in row["args"][1:]])], ["count(*)"])
    assert [(k[0][0], k[0][1]) for k in out.keys] == [(n1o.T_INT, row["result"])], (row["statement"], out.keys)


def test_the_references_statement_over_a_column():
    (c,) = GOLDEN["columns"]
    rows = [{"s": M if isinstance(v, dict) else v, "id": i} for i, v in enumerate(c["inputs"])]
    t = du.date_table(rows, names_tagged=("id",), names_dict=("s",))
    out, _ = must_run(pu.run_gpu, t, None, [du.call_text(c["function"], S, c["part"])], ["count(*)"])
    got = [{} if decoded(k[0]) is M else {c["alias"]: decoded(k[0])} for k in out.keys]
    counts = {json.dumps(g, sort_keys=True): a[0][1] for g, a in zip(got, out.aggs)}
    want = {}
    for r in c["results"]:
        want[json.dumps(r, sort_keys=True)] = want.get(json.dumps(r, sort_keys=True), 0) + 1
    assert counts == want


# ------------------------------------------------------------------ the pools through datefn_kernel<OP>

def parts_of(fn):
    return du.PART_NAMES if fn in ("date_part_millis", "date_part_str") else du.ADD_PARTS if fn == "date_add_millis" else du.TRUNC_PARTS


@pytest.mark.parametrize("fn", du.MILLIS_FUNCTIONS)
def test_the_device_evaluator_is_the_yardstick_over_the_millis_edges(fn):
    """n1k_datefn_eval_device: every part x the edge pool (x every n) through datefn_kernel<OP>.  The kernel has one flag for
    all rows: it is up exactly when the yardstick raises on some value, and such a value's slot holds NULL."""
    ups = 0
    for part in parts_of(fn):
        for n in (du.ADD_NS if fn == "date_add_millis" else [None]):
            if isinstance(n, float) and (n != n or n in (du.PINF, du.NINF)):
                continue  # (no constant text: test_nan_and_infinite_operands_from_a_column)
            text = plan.date_fn(fn, T, du.const_text(n), P(part)) if fn == "date_add_millis" else du.call_text(fn, T, part)
            st, got, extra = du.eval_call(text, du.MILLIS_EDGES, device=0)
            assert st == _ffi.OK, text
            want = [du.apply_millis(fn, v, part, n=n) for v in du.MILLIS_EDGES]
            assert extra["any_raise"] == int(du.RAISE in want), (text, extra)
            assert got == [du.R_NULL if w == du.RAISE else w for w in want], [(text, v, g, w) for v, g, w in zip(du.MILLIS_EDGES, got, want) if g != w][:4]
            ups += extra["any_raise"]
    assert ups > 0


def safe_rows(fn, part, n):
    """n rows (t, w, id) over the edge pools on which fn never raises: a raising pair is replaced by a harmless one"""
    rows = []
    for i in range(n):
        t = du.MILLIS_EDGES[(i * 7 + 3) % len(du.MILLIS_EDGES)]
        w = du.ADD_NS[(i * 5 + i // len(du.MILLIS_EDGES)) % len(du.ADD_NS)]
        if isinstance(t, (list, dict)):
            t = None
        if isinstance(w, str):
            w = True
        if du.apply_millis(fn, t, part, n=w) == du.RAISE:
            t, w = (BASE + i, 1 + i % 5) if du.apply_millis(fn, BASE + i, part, n=w) == du.RAISE else (BASE + i, w)
        rows.append({"t": t, "w": w, "id": i})
    return rows


def node_text(fn, part, first=T):
    return plan.date_fn(fn, first, W, P(part)) if fn == "date_add_millis" else du.call_text(fn, first, part)


@pytest.mark.parametrize("n", BATCH_EDGES)
@pytest.mark.parametrize("fn", du.MILLIS_FUNCTIONS)
def test_every_row_of_the_element_wise_kernel(fn, n):
    """MAX(f(t[, w])) GROUP BY id over the edge pools, the node materialised (datefn_kernel<OP>), one part per batch size"""
    part = parts_of(fn)[BATCH_EDGES.index(n) * 2 % len(parts_of(fn))]
    rows = safe_rows(fn, part, n)
    t = du.date_table(rows, names_tagged=("t", "w", "id"), names_dict=())
    out, st = must_run(pu.run_gpu, t, None, [ID], ["max(%s)" % node_text(fn, part)], fuse_arith=0)
    assert st["rows_in"] == n and len(out.keys) == n
    got = {k[0][1]: a[0] for k, a in zip(out.keys, out.aggs)}
    for r in rows:
        want = du.apply_millis(fn, r["t"], part, n=r["w"])
        want = du.R_NULL if want == du.R_MISSING else want  # (MAX skips MISSING and NULL alike)
        g = got[r["id"]]
        assert (g[0], (g[1] & 0xFFFFFFFFFFFFFFFF) if g[0] == n1o.T_INT else 0) == want, (fn, part, r, g, want)


@pytest.mark.parametrize("n", BATCH_EDGES)
@pytest.mark.parametrize("fn", du.MILLIS_FUNCTIONS)
def test_every_row_of_the_edge_pools_through_the_fused_scan(fn, n):
    """the same batches with the node in the run-time-built scan's registers (jit = 2, spec_kernel 3): the range ends, -1,
    +-0.5, -0.0, the lost carry, Feb 28 / 29 and every n of the pool, tag and payload exactly"""
    part = parts_of(fn)[BATCH_EDGES.index(n) * 2 % len(parts_of(fn))]
    rows = safe_rows(fn, part, n)
    t = du.date_table(rows, names_tagged=("t", "w", "id"), names_dict=())
    out, st = must_run(pu.run_gpu, t, None, [ID], ["max(%s)" % node_text(fn, part)], jit=2)
    assert st["spec_kernel"] == 3, st
    assert st["rows_in"] == n and len(out.keys) == n
    got = {k[0][1]: a[0] for k, a in zip(out.keys, out.aggs)}
    for r in rows:
        want = du.apply_millis(fn, r["t"], part, n=r["w"])
        want = du.R_NULL if want == du.R_MISSING else want  # (MAX skips MISSING and NULL alike)
        g = got[r["id"]]
        assert (g[0], (g[1] & 0xFFFFFFFFFFFFFFFF) if g[0] == n1o.T_INT else 0) == want, (fn, part, r, g, want)


@pytest.mark.parametrize("pred", ["missing", "null"])
@pytest.mark.parametrize("fn", du.MILLIS_FUNCTIONS)
def test_missing_and_null_are_told_apart_in_the_fused_scan(fn, pred):
    """(MAX folds both to NULL) the rows the fused Filter `f(t[, w]) IS MISSING / IS NULL` keeps, by their ids"""
    rows = safe_rows(fn, "day", 769)
    t = du.date_table(rows, names_tagged=("t", "w", "id"), names_dict=())
    out, st = must_run(pu.run_gpu, t, "(%s is %s)" % (node_text(fn, "day"), pred), [ID], ["count(*)"], jit=2)
    assert st["spec_kernel"] == 3, st
    tag = du.R_MISSING if pred == "missing" else du.R_NULL
    want = {r["id"] for r in rows if du.apply_millis(fn, r["t"], "day", n=r["w"]) == tag}
    assert {k[0][1] for k in out.keys} == want and 0 < len(want) < len(rows)


def test_missing_and_null_are_told_apart():
    for fn in du.MILLIS_FUNCTIONS:
        part = "day"
        rows = safe_rows(fn, part, 769)
        t = du.date_table(rows, names_tagged=("t", "w", "id"), names_dict=())
        vals = [du.apply_millis(fn, r["t"], part, n=r["w"]) for r in rows]
        for pred, tag in (("missing", du.R_MISSING), ("null", du.R_NULL)):
            _out, st = must_run(pu.run_gpu, t, "(%s is %s)" % (node_text(fn, part), pred), [], ["count(*)"])
            assert st["rows_selected"] == vals.count(tag) > 0, (fn, pred)


def test_nan_and_infinite_operands_from_a_column():
    """a NaN n is NULL (it is not integral); an infinite n, and a NaN or infinite millis, raise"""
    ok = du.date_table([{"t": BASE, "w": du.NAN, "id": 0}, {"t": BASE, "w": 2.5, "id": 1}], names_tagged=("t", "w", "id"), names_dict=())
    out, _ = must_run(pu.run_gpu, ok, None, [node_text("date_add_millis", "day")], ["count(*)"])
    assert [(k[0][0], a[0][1]) for k, a in zip(out.keys, out.aggs)] == [(n1o.T_NULL, 2)]
    for t, w in ((BASE, du.PINF), (BASE, du.NINF), (du.NAN, 1), (du.PINF, 1), (du.NINF, 1)):
        bad = du.date_table([{"t": BASE, "w": 1, "id": 0}, {"t": t, "w": w, "id": 1}], names_tagged=("t", "w", "id"), names_dict=())
        for opts in ({}, {"fuse_arith": 0}):
            must_raise(bad, None, [node_text("date_add_millis", "day")], ["count(*)"], **opts)


RAISING = {
    "one past the range": ("date_part_millis", du.MAX_MILLIS + 1, 1, "year"),
    "one before the range": ("date_trunc_millis", du.MIN_MILLIS - 1, 1, "day"),
    "half a millisecond past the range": ("date_part_millis", float(du.MAX_MILLIS) + 0.5, 1, "year"),
    "a millennium that begins in year 0": ("date_trunc_millis", du.ms_of(999, 6, 15), 1, "millennium"),
    "a result beyond year 9999": ("date_add_millis", BASE, 8000, "year"),
    "a result before year 1": ("date_add_millis", BASE, -2016, "year"),
    "n beyond 2^31": ("date_add_millis", BASE, 2 ** 31 + 1, "millisecond"),
    "hours beyond int64 nanoseconds": ("date_add_millis", BASE, 2562048, "hour"),
    "minutes beyond int64 nanoseconds": ("date_add_millis", BASE, -153722868, "minute"),
}


@pytest.mark.parametrize("what", sorted(RAISING))
def test_a_row_whose_answer_would_be_wrapped_raises_on_both_routes(what):
    """one such row among 600 good ones: N1K_UNSUPPORTED_DATA from the materialised node and from the fused scan; without the
    row the same plan runs"""
    fn, t, w, part = RAISING[what]
    assert du.apply_millis(fn, t, part, n=w) == du.RAISE
    rows = [{"t": BASE + 86400000 * i, "w": 1, "cat": "c%d" % (i % 5)} for i in range(601)]
    good = du.date_table(rows, names_tagged=("t", "w"), names_dict=("cat",))
    rows[389].update(t=t, w=w)
    bad = du.date_table(rows, names_tagged=("t", "w"), names_dict=("cat",))
    cond, keys, aggs = "(0 <= %s)" % node_text(fn, part), [D("cat")], ["count(*)"]  # (t, w, cat: the three columns a fused shape takes)
    for opts in ({"jit": 2}, {"fuse_arith": 0}):
        _out, st = must_run(pu.run_gpu, good, cond, keys, aggs, **opts)
        assert (st["spec_kernel"] == 3) == ("jit" in opts), (opts, st)
        must_raise(bad, cond, keys, aggs, **opts)


# ------------------------------------------------------------------ the fused route

PRICE, CAT = D("price"), D("cat")
# name -> (node, device condition / keys / aggregates with {h} where the oracle reads the helper column)
FUSED_NODES = {
    "part-in-where": (("date", "date_part_millis", [("col", "t"), ("const", "month")]), "({h} <= 6)", [CAT], ["sum(%s)" % PRICE, "count(*)"]),
    "trunc-operand": (("date", "date_trunc_millis", [("col", "t"), ("const", "quarter")]), None, [CAT], ["count(*)", "max({h})"]),
    "add-chain": (("date", "date_part_millis", [("date", "date_add_millis", [("col", "t"), ("col", "g"), ("const", "month")]), ("const", "day")]),
                  None, [CAT], ["count(*)", "sum({h})"]),  # (three input columns and — every use is a node of its own — three nodes at the most)
    "trunc-key": (("date", "date_trunc_millis", [("col", "t"), ("const", "year")]), None, ["{h}"], ["sum(%s)" % PRICE]),
}


def fused_plan(name, h):
    _node, cond, keys, aggs = FUSED_NODES[name]
    return (cond.format(h=h) if cond else None, [k.format(h=h) for k in keys], [a.format(h=h) for a in aggs])


FUSED_SHAPES = {name: fused_plan(name, du.value_text(FUSED_NODES[name][0])) for name in FUSED_NODES}


@functools.lru_cache(maxsize=None)
def fused_table():
    rng = random.Random(31)
    base, span = du.ms_of(1990, 1, 1), du.ms_of(2030, 1, 1) - du.ms_of(1990, 1, 1)
    rows = []
    for i in range(20_001):
        r = rng.random()
        t = M if r < 0.03 else None if r < 0.06 else "a" if r < 0.08 else base + rng.randrange(span) + (0.75 if r < 0.2 else 0)
        rows.append({"t": t, "g": rng.randrange(7), "price": rng.randrange(100), "cat": "cat_%d" % rng.randrange(12)})
    return rows, du.date_table(rows, names_tagged=("t", "g", "price"), names_dict=("cat",))


@pytest.mark.parametrize("name", sorted(FUSED_NODES))
def test_date_functions_fused_into_the_runtime_built_scan(name):
    """jit = 2: the nodes in the scan's registers (spec_kernel 3), and the same plan materialised (fuse_arith off); both
    against the oracle by substitution, exactly"""
    rows, t = fused_table()
    node = FUSED_NODES[name][0]
    values = [du.eval_value(node, r) for r in rows]
    ot = n1o.Table(list(t.columns) + [du.helper_column("h", values)], t.dictionary)
    ocond, okeys, oaggs = fused_plan(name, D("h"))
    ora = n1o.run(ot, ocond, okeys, oaggs)
    cond, keys, aggs = FUSED_SHAPES[name]
    for batches in (1, 2):
        gpu, st = must_run(pu.run_gpu, t, cond, keys, aggs, batches=batches, jit=2)
        pu.assert_same_groups(gpu, ora, aggs=oaggs)
        assert st["rows_selected"] == ora.rows_passed
        assert st["spec_kernel"] == 3, st
    unfused, st = must_run(pu.run_gpu, t, cond, keys, aggs, batches=2, jit=2, fuse_arith=0)
    pu.assert_same_groups(unfused, ora, aggs=oaggs)
    assert st["spec_kernel"] != 3 and st["rows_selected"] == ora.rows_passed


# ------------------------------------------------------------------ the string half: the table kernel

STRING_POOL = du.VALUE_STRINGS + du.NULL_STRINGS + [s for v in du.UNSURE_STRINGS.values() for s in v]


def pool_strings(n, long_at=()):
    """n strings cycling through the pool; at the indices of long_at strings of 64 and 65 bytes alternately"""
    out = [STRING_POOL[(i * 11 + 5) % len(STRING_POOL)] for i in range(n)]
    for k, i in enumerate(long_at):
        out[i] = "2006-01-02T15:04:05.999+07:00" + " " * ((64 if k % 2 == 0 else 65) - 29)
    return out


@pytest.mark.parametrize("n", [63, 64, 65, 129])
@pytest.mark.parametrize("fn", du.STRING_FUNCTIONS)
def test_the_table_kernel_at_its_edges(fn, n):
    """n1k_datefn_eval_device over n strings: the last wave holds 63, 64, 1 and 1 entries; strings of 64 bytes are the kernel's,
    of 65 the host evaluator's, and a wave that holds one reads its other entries from global memory"""
    long_at = (0, 1, n - 2, n - 1) if n >= 64 else (5, n - 1)
    strings = pool_strings(n, long_at)
    for part in (["iso_week", "timezone", "millisecond"] if fn == "date_part_str" else [None]):
        text = du.call_text(fn, S, *([part] if part else []))
        st, got, extra = du.eval_call(text, strings, device=0)
        assert st == _ffi.OK
        want = [du.apply_string(fn, s, part) for s in strings]
        assert got == want, [(text, s, g, w) for s, g, w in zip(strings, got, want) if g != w][:4]
        assert extra["left"] == sum(len(s.encode()) > du.DEV_MAX_LEN for s in strings) == len(long_at) // 2
        assert extra["any_raise"] == int(du.RAISE in want)
        assert du.eval_call(text, strings)[1] == want  # (the host evaluator, over the same block)


def test_values_that_are_no_string_and_an_empty_block():
    vals = [M, None, 5, 2.5, True, [1], {"a": 1}, "2004-07-09", ""]
    st, got, extra = du.eval_call(du.call_text("date_part_str", S, "year"), vals, device=0)
    assert st == _ffi.OK and got == [du.R_MISSING] + [du.R_NULL] * 6 + [du.r_int(2004), du.R_NULL] and extra["left"] == 0
    assert du.eval_call(du.call_text("str_to_millis", S), [], device=0)[0] == _ffi.OK


# ------------------------------------------------------------------ the string half: the lookup and the handle's tables

@pytest.mark.parametrize("kind", ["dict32", "tagged"])
@pytest.mark.parametrize("n", BATCH_EDGES)
def test_every_row_of_the_lookup_kernel(n, kind):
    """MAX(f(s)) GROUP BY id, two terms in one plan; s a DICT32 column of codes, or a TAGGED64 column that holds numbers,
    booleans and arrays beside the strings"""
    safe = du.VALUE_STRINGS + du.NULL_STRINGS
    others = [M, None] if kind == "dict32" else [M, None, 5, 2.5, True, [1, 2]]
    rows = [{"s": (others[i % len(others)] if i % 9 == 4 else safe[(i * 7) % len(safe)]), "id": i} for i in range(n)]
    t = du.date_table(rows, names_tagged=("id",), names_dict=("s",) if kind == "dict32" else (), tagged_strings=("s",) if kind == "tagged" else ())
    f1, f2 = du.call_text("str_to_millis", S), du.call_text("date_part_str", S, "iso_year")
    out, st = must_run(pu.run_gpu, t, None, [ID], sorted(["max(%s)" % f1, "max(%s)" % f2]))
    assert st["rows_in"] == n and len(out.keys) == n
    got = {k[0][1]: a for k, a in zip(out.keys, out.aggs)}
    order = sorted(["max(%s)" % f1, "max(%s)" % f2]).index("max(%s)" % f1)
    for r in rows:
        for fn, part, at in (("str_to_millis", None, order), ("date_part_str", "iso_year", 1 - order)):
            want = du.apply_string(fn, r["s"], part)
            want = du.R_NULL if want == du.R_MISSING else want
            g = got[r["id"]][at]
            assert (g[0], (g[1] & 0xFFFFFFFFFFFFFFFF) if g[0] == n1o.T_INT else 0) == want, (fn, r, g, want)


def numbered_dates(tag, n):
    """n distinct VALUE strings: day i of an era that `tag` picks"""
    y0 = {"a": 1000, "b": 4000}[tag]
    out = []
    for i in range(n):
        days = du.days_of(y0, 1, 1) + i
        y, m, d, _yd = du.civil(days)
        out.append("%04d-%02d-%02dT10:00:00Z" % (y, m, d))
    return out


@pytest.mark.parametrize("route", ["host", "device"])
def test_a_table_extended_between_two_pushes(route):
    """str_to_millis(s) and date_part_str(s, "year") in one plan.  The first push interns a dictionary below the threshold: the
    host evaluator.  The second brings new entries — threshold - 1 of them: the host route again; threshold + 1: the kernel,
    which hands over the two strings of more than 64 bytes — and the old entries keep their values."""
    f1, f2 = du.call_text("str_to_millis", S), du.call_text("date_part_str", S, "year")
    op = query_amd.GpuFilterGroup(plan.filter_group_plan("((%s < 0) and (%s < 4500))" % (f1, f2), [], ["count(*)"]))
    try:
        thr = op.datefn_stats()["device_threshold"]
        dictionary, want_dev, want_host = [], 0, 0
        for tag, n in (("a", 50), ("b", thr - 3 if route == "host" else thr - 1)):
            new = numbered_dates(tag, n) + ["2006-01-02T15:04:05Z" + " " * 50 + tag, "not a date " + tag]
            if tag == "b":
                new[7] = "2006-01-02 15:04:05.999999999+07:00" + " " * 30  # 65 bytes
            on_device = len(new) >= thr
            dictionary += [s.encode() for s in new]
            rng = np.random.default_rng(len(dictionary))
            codes = np.concatenate([np.arange(len(dictionary)), rng.integers(0, len(dictionary), 5000)]).astype(np.uint32)
            assert op.column_paths == [S]
            op.process_items([n1o.Column(S, n1o.COL_DICT32, codes=codes)], dictionary)
            got = op.after_items().aggs[0][0][1]
            assert int(_ffi.lib().n1k_dict_size(op._h)) == len(dictionary)
            hit = np.array([du.apply_string("str_to_millis", s.decode())[0] == n1o.T_INT and du.result_value(du.apply_string("str_to_millis", s.decode())) < 0
                            and du.result_value(du.apply_string("date_part_str", s.decode(), "year")) < 4500 for s in dictionary])
            want = int(hit[codes.astype(np.int64)].sum())
            assert 0 < want < len(codes) and got == want, (tag, got, want)
            nlong = sum(len(s) > du.DEV_MAX_LEN for s in new)
            if on_device:
                want_dev, want_host = want_dev + len(new) - nlong, want_host + nlong
            else:
                want_host += len(new)
            st = op.datefn_stats()
            assert (st["device_strings"], st["host_strings"], st["terms"]) == (want_dev, want_host, 2), (tag, st, want_dev, want_host)
            op.reopen()  # (keeps the tables)
        assert (want_dev > 0) == (route == "device")
    finally:
        op.done()


@pytest.mark.parametrize("why", sorted(du.UNSURE_STRINGS))
def test_a_row_that_reads_an_unsure_string_raises(why):
    """N1K_UNSUPPORTED_DATA when a row holds the string; the same dictionary with no row that reads it harms nobody"""
    for bad in du.UNSURE_STRINGS[why]:
        words = ["2004-07-09", bad, "2016-09-26T11:33:16.209-04:00"]
        rows = [{"s": words[i % 3], "id": i} for i in range(300)]
        for fn, part in (("str_to_millis", None), ("date_part_str", "day")):
            text = du.call_text(fn, S, *([part] if part else []))
            must_raise(du.date_table(rows, names_tagged=("id",), names_dict=("s",)), None, [text], ["count(*)"])
            unread = [dict(r, s=words[0] if r["s"] == bad else r["s"]) for r in rows]
            out, _ = must_run(pu.run_gpu, du.date_table(unread, names_tagged=("id",), names_dict=("s",), dictionary=words), None, [text], ["count(*)"])
            assert sorted(a[0][1] for a in out.aggs) == [100, 200]


# ------------------------------------------------------------------ the grouped tail, directed

def test_having_and_a_projection_over_a_group_key_and_over_min():
    """date_part_str over the group key in HAVING, str_to_millis over MIN(s) and date_trunc_millis over MAX(t) as projection
    terms, the alias an ORDER BY term"""
    rng = random.Random(7)
    rows = du.make_rows(rng, 2000)
    t = du.date_table(rows)
    ora = n1o.run(t, None, [S], ["count(*)"])
    f = du.call_text("date_part_str", S, "year")
    gpu, _ = must_run(pu.run_gpu, t, None, [S], ["count(*)"], having="(2010 <= %s)" % f)
    want = {decoded(k[0]) for k in ora.keys if du.is_number(du.result_value(du.apply_string("date_part_str", decoded(k[0]), "year")))
            and du.result_value(du.apply_string("date_part_str", decoded(k[0]), "year")) >= 2010}
    assert {decoded(k[0]) for k in gpu.keys} == want and 0 < len(want) < len(ora.keys)
    aggs = sorted(["min(%s)" % S, "max(%s)" % T])
    ora = n1o.run(t, None, [K], aggs)
    p1, p2 = du.call_text("str_to_millis", "min(%s)" % S), du.call_text("date_trunc_millis", "max(%s)" % T, "month")
    gpu, _ = must_run(pu.run_gpu, t, None, [K], aggs, project=[(K, "k"), (p1, "a"), (p2, "b")], order=[("`b`", False), ("`k`", False)])
    got = {decoded(r[0]): (r[1], r[2]) for r in gpu.proj}
    imax, imin = aggs.index("max(%s)" % T), aggs.index("min(%s)" % S)
    assert len(got) == len(ora.keys) > 1
    for k, a in zip(ora.keys, ora.aggs):
        w1 = du.apply_string("str_to_millis", decoded(a[imin]))
        w2 = du.apply_millis("date_trunc_millis", decoded(a[imax]), "month")
        g1, g2 = got[decoded(k[0])]
        assert (g1[0], g1[1] & 0xFFFFFFFFFFFFFFFF if g1[0] == n1o.T_INT else 0) == w1 and (g2[0], g2[1] & 0xFFFFFFFFFFFFFFFF if g2[0] == n1o.T_INT else 0) == w2


# ------------------------------------------------------------------ differential by substitution

FAMILIES = [{"fast": 0}, {}, {"spec": 0}, {"jit": 0}]


def tail_expectation(p, ora):
    """the node over the source — a group key or an aggregate — of every group of the oracle: {key: (tag, payload)}"""
    keys, aggs = p["base"]
    at = None if p["how"] == "key" else aggs.index(p["source"])
    out = {}
    for k, a in zip(ora.keys, ora.aggs):
        src = decoded(k[0]) if at is None else decoded(a[at])
        row = {p["col"]: src}
        try:
            v = du.eval_value(p["node"], row)
        except du.Raised:
            v = du.RAISE
        out[json.dumps(decoded(k[0]) if decoded(k[0]) is not M else "\0missing")] = v
    return out


@pytest.mark.parametrize("seed", range(du.NSEEDS))
def test_date_function_plans_agree_with_the_oracle_by_substitution(seed):
    p = du.draw_plan(seed)
    opts = FAMILIES[seed % len(FAMILIES)]
    t = du.date_table(p["rows"])
    what = "seed %d place %s node %s opts %r" % (seed, p["place"], du.value_text(p["node"]), opts)
    if p["place"] in ("having", "project"):
        keys, aggs = p["base"]
        ora = n1o.run(t, None, keys, aggs, threads=2)
        want = tail_expectation(p, ora)
        assert du.RAISE not in want.values(), what  # (the seeded pools hold nothing that raises)
        kname = lambda k: json.dumps(decoded(k) if decoded(k) is not M else "\0missing")  # noqa: E731
        if p["place"] == "having":
            nums = sorted(v for v in want.values() if du.is_number(v))
            c = nums[len(nums) // 2] if nums else 0
            gpu, _ = must_run(pu.run_gpu, t, None, keys, aggs, having="(%s %s %s)" % (p["over"], p["op"], du.const_text(c)), **opts)
            keep = {k for k, v in want.items() if du.is_number(v) and (v < c or (p["op"] == "<=" and v == c))}
            assert {kname(k[0]) for k in gpu.keys} == keep, what
        else:
            gpu, _ = must_run(pu.run_gpu, t, None, keys, aggs, project=[(keys[0], "k"), (p["over"], "p")], **opts)
            got = {kname(r[0]): decoded(r[1]) for r in gpu.proj}
            assert set(got) == set(want), what
            for k, v in want.items():
                assert got[k] is v or (got[k] == v and type(got[k]) is type(v)), (what, k, got[k], v)
        return
    ot = n1o.Table(list(t.columns) + [du.helper_column("h", p["values"])], t.dictionary)
    (dcond, dkeys, daggs), (ocond, okeys, oaggs) = p["device"], p["oracle"]
    ora = n1o.run(ot, ocond, okeys, oaggs, threads=2)
    gpu, st = must_run(pu.run_gpu, t, dcond, dkeys, daggs, batches=1 + seed % 3, **opts)
    try:
        pu.assert_same_groups(gpu, ora, aggs=oaggs)
    except AssertionError as e:
        raise AssertionError("%s | %s" % (e, what))
    assert st["rows_selected"] == ora.rows_passed, what
    if p["place"] == "filter":  # the Filter alone: the selected row ordinals, as they come
        gsel, _ = must_run(pu.run_gpu, t, dcond, [], [], filter_only=True, batches=1 + seed % 2)
        osel = n1o.run(ot, ocond, [], [], has_group=False)
        assert np.array_equal(np.asarray(gsel.selected, dtype=np.uint64), osel.selected), what
