"""array_length / array_count / array_sum / array_avg / array_contains / array_position on the device: arrfn_table_kernel at its
edges and on seeded arrays against the host evaluator and the yardstick (tests/arrfn_util.py), bit for bit; the hand-overs
with exact counts; arrfn_lookup_kernel at its edges; the value table extended across batches; the reference's statements; one
plan per placement; and a differential against the oracle BY SUBSTITUTION as tests/test_gpu_mathfn.py does it — the oracle
does not know these functions, so where the device's plan holds one the oracle's reads a TAGGED64 helper column with the
yardstick's value of every row.

Both kernels have 256-lane workgroups of 64-lane waves, one entry / one row per lane: their edges are 1, 63, 64, 65, 255, 256,
257 entries and 3 workgroups + 1 = 769.  A refusal is a failure here, never a skip."""
import functools
import json
import os
import random
import struct

import numpy as np
import pytest

import arrfn_util as au
import coll_util as cu
import golden_util as gu
import parity_util as pu
import query_amd
from oracle import n1o
from query_amd import _ffi, plan

pytestmark = pytest.mark.gpu

D = au.D
M = au.MISSING
NSEEDS = 120  # NOTE: tests/test_arrfn_cpu.py creates every plan drawn or stated here without a GPU
KERNEL_EDGES = [1, 63, 64, 65, 255, 256, 257, 769]
DEV_MAX_LEN = au.DEV_MAX_LEN

with open(os.path.join(gu.GOLDEN, "cases_arr.json")) as fh:
    ARR = json.load(fh)


def must_run(fn, *a, **kw):
    try:
        return fn(*a, **kw)
    except query_amd.N1kError as e:
        raise AssertionError("the device refused: %s" % e.message)


def result_pair(tv):
    """a (tag, python value) of a result as the yardstick's (tag, payload bits)"""
    t, v = tv
    if t == n1o.T_INT:
        return au.r_int(v)
    if t == n1o.T_FLOAT:
        return au.r_float(v)
    return (t, 0)


# ------------------------------------------------------------------ the table kernel at its edges

# every (function, constant) the edge tests run: both kinds of constant for the binary ones
EDGE_TERMS = [(fn, None) for fn in au.UNARY] + [(fn, c) for fn in au.BINARY for c in ("t_1", 2)]
# elements the kernel decides itself under every function: no escape, no number beyond the exact conversions
CLEAN = [[], [None], [1, 2], ["t_1"], [2, "a"], ["a", "t_1", 2.5], [[1, "t_1"], {"f": 2}], [None, True, 7, 18, 16], [-3, -2, -1, 0, 1, 2, 3, 4], [0.5, 0.25, 2],
         [2 ** 59, 2 ** 59], [1.5, "b", None, 2]]
# an INT sum that overflows to FLOAT inside the kernel's limits: ten 18-digit integers that float64 holds exactly, 191 bytes
OVERFLOW = [10 ** 18 - 128] * 10


def sized_array_text(length):
    """array text of exactly `length` bytes, a number and a string in it"""
    t = b'[2,"' + b"x" * (length - 6) + b'"]'
    assert len(t) == length
    return t


def edge_block(n, long_last):
    """n entries: arrays of the clean pool, each made distinct by a trailing number, with entries of 0 bytes, entries that are
    no array text and array texts of 190 to 194 bytes among them; long_last: the last one is an array text of 15 KB"""
    out = []
    for i in range(n):
        k = i % 23
        if k == 5:
            out.append(b"")
        elif k == 9:
            out.append(b"zz%d" % i)
        elif k == 13:
            out.append(b'{"f":[%d]}' % i)
        elif k == 17:
            out.append(b"[")  # one byte: no array text
        elif k == 21:
            out.append(cu.canon(OVERFLOW).encode())
        elif k == 20 and n > 64:
            out.append(sized_array_text(190 + (i // 23) % 5))
        else:
            out.append(cu.canon(CLEAN[i % len(CLEAN)] + [i]).encode())
    if long_last:
        out[-1] = cu.canon(["t_1", 2] + ["y" * 50] * 280).encode()
        assert len(out[-1]) > 14_000
    return out


assert len(cu.canon(OVERFLOW)) == 191 and au.apply("array_sum", OVERFLOW)[0] == au.T_FLOAT and au.apply("array_sum", OVERFLOW[:9])[0] == au.T_INT


def is_array_text(t):
    return len(t) >= 2 and t[:1] == b"["


def check_block(texts, terms=EDGE_TERMS):
    want_left = sum(1 for t in texts if is_array_text(t) and len(t) > DEV_MAX_LEN)
    for fn, c in terms:
        term = au.term_text(fn, c)
        dt, dp, left = au.device_eval(term, texts)
        ht, hp = au.host_eval(term, texts)
        wt, wp = au.want_block(fn, c, texts)
        assert np.array_equal(dt, ht) and np.array_equal(dp, hp), (term, len(texts))
        bad = np.nonzero((dt != wt) | (dp != wp))[0]
        assert bad.size == 0, (term, texts[bad[0]][:80], (dt[bad[0]], hex(int(dp[bad[0]]))), (wt[bad[0]], hex(int(wp[bad[0]]))))
        assert left == want_left, (term, left, want_left)
    return want_left


@pytest.mark.parametrize("long_last", [False, True], ids=["plain", "last-entry-15KB"])
@pytest.mark.parametrize("n", KERNEL_EDGES)
def test_table_kernel_at_its_edges(n, long_last):
    """device = host = yardstick for every function, and exactly the texts beyond 192 bytes are left to the host: with a last
    entry of 15 KB the final wave spans more than its slab and reads its other entries from global memory"""
    texts = edge_block(n, long_last)
    want_left = check_block(texts)
    assert want_left >= (1 if long_last else 0)
    if n >= 257:
        assert sum(1 for t in texts if is_array_text(t) and len(t) in (193, 194)) >= 1 and any(len(t) == 0 for t in texts)


def test_array_texts_on_both_sides_of_the_limit():
    texts = [sized_array_text(n) for n in (190, 191, 192, 193, 194)]
    assert check_block(texts) == 2
    # the same lengths as text that is no array: nobody's business, NULL, not handed over
    assert check_block([b'"' + t[1:] for t in texts]) == 0


def test_entries_of_zero_bytes_and_entries_that_are_no_array_text():
    texts = [b"", b"", b"[1,2]", b"", b"x", b"[", b"]", b"{}", b'"[1,2]"', b"[]", b"", b"null", b"12", b"[2]"]
    assert check_block(texts) == 0
    assert check_block([b""] * 70) == 0
    assert check_block([b"abc"] * 65 + [b""]) == 0


# ------------------------------------------------------------------ seeded arrays

def test_device_evaluator_equals_host_evaluator_and_yardstick_on_the_cpu_tests_pairs():
    import test_arrfn_cpu as tc
    total, handed = 0, 0
    for fn, c, arrays in au.random_pairs(*tc.CPU_PAIRS):
        term, texts = au.term_text(fn, c), au.texts_of(arrays)
        dt, dp, left = au.device_eval(term, texts)
        ht, hp = au.host_eval(term, texts)
        wt, wp = au.want_block(fn, c, texts)
        assert np.array_equal(dt, ht) and np.array_equal(dp, hp) and np.array_equal(dt, wt) and np.array_equal(dp, wp), (term, texts[:4])
        assert left <= len(texts)
        if fn in ("array_length", "array_count"):  # they hand over nothing but the long texts
            assert left == sum(1 for t in texts if len(t) > DEV_MAX_LEN), term
        total += len(texts)
        handed += left
    assert total >= 20000 and 0 < handed < total


# ------------------------------------------------------------------ directed hand-overs

ESCAPED_FIRST = ['x"y', "x"]
ESCAPED_LAST = ["x", 'x"y']
NINETEEN = [1234567890123456789, 1]
INEXACT = [2 ** 53 + 1, 1]
HANDOVERS = [
    # (function, constant, arrays, left)
    ("array_contains", "x", [ESCAPED_FIRST, NINETEEN, ["x"]], 1),        # the escaped string is compared before the match
    ("array_position", "x", [ESCAPED_FIRST, ESCAPED_LAST, NINETEEN], 1),  # ... behind the match it is not reached; numbers are not read
    ("array_contains", "q", [ESCAPED_FIRST, ESCAPED_LAST], 2),            # no match: the walk reaches both
    ("array_sum", None, [ESCAPED_FIRST, NINETEEN, [1, 2]], 1),           # a 19-digit integer
    ("array_avg", None, [NINETEEN, INEXACT, [123456789012345.5], [1.5]], 3),  # ... an integer float64 does not hold, 16 digits with a fraction
    ("array_contains", 1, [NINETEEN, INEXACT, [1, 2 ** 53 + 1], ESCAPED_FIRST], 2),  # a NUMBER constant reads numbers — up to the match — and no string
    ("array_position", 2.5, [[10 ** 20], [2 ** 54], ["a"]], 1),           # 21 digits; 2^54 is exactly a float64
    ("array_length", None, [ESCAPED_FIRST, NINETEEN, INEXACT, [10 ** 20]], 0),  # neither reads a number nor decodes a string
    ("array_count", None, [ESCAPED_FIRST, NINETEEN, INEXACT, [10 ** 20]], 0),
    ("array_contains", None, [ESCAPED_FIRST, NINETEEN], 0),              # a NULL constant: NULL without a walk
    ("array_contains", True, [ESCAPED_FIRST, NINETEEN], 0),              # a boolean constant compares tags
]


@pytest.mark.parametrize("i", range(len(HANDOVERS)))
def test_directed_hand_overs_with_exact_counts(i):
    fn, c, arrays, want_left = HANDOVERS[i]
    # in a block of 70: the hand-overs sit in two waves, among entries the kernel keeps
    filler = [[k, "a"] for k in range(70 - len(arrays))]
    block = filler[:40] + arrays + filler[40:]
    term, texts = au.term_text(fn, c), au.texts_of(block)
    dt, dp, left = au.device_eval(term, texts)
    ht, hp = au.host_eval(term, texts)
    wt, wp = au.want_block(fn, c, texts)
    assert np.array_equal(dt, ht) and np.array_equal(dp, hp) and np.array_equal(dt, wt) and np.array_equal(dp, wp), term
    assert left == want_left, (term, left, want_left)


# ------------------------------------------------------------------ the lookup kernel

LOOKUP_POOL = au.TABLE_ARRAYS[:12] + au.OTHERS


@functools.lru_cache(maxsize=None)
def lookup_table(n):
    rows = [{"id": i, "a": LOOKUP_POOL[(i * 7 + i // len(LOOKUP_POOL)) % len(LOOKUP_POOL)], "s": [M, None, "a", "t_1", ""][i % 5]} for i in range(n)]
    cols = [au.column("id", [r["id"] for r in rows]), au.column("a", [r["a"] for r in rows]),
            n1o.Column(D("s"), n1o.COL_DICT32, codes=au.dict_codes([r["s"] for r in rows]))]
    return rows, n1o.Table(cols, list(au.ROW_DICT))


def lookup_plan(fn, col):
    return (None, [D("id")], ["max(%s)" % au.term_text(fn, "a" if fn in au.BINARY else None, over=D(col))])


@pytest.mark.parametrize("n", KERNEL_EDGES)
def test_every_row_of_the_lookup_kernel(n):
    """MAX(f(a)) GROUP BY id over a TAGGED64 operand that holds every tag class, every function, bit for bit (MAX folds MISSING
    and NULL to NULL: the next test tells them apart)"""
    rows, table = lookup_table(n)
    for fn in au.FUNCTIONS:
        cond, keys, aggs = lookup_plan(fn, "a")
        out, st = must_run(pu.run_gpu, table, cond, keys, aggs)
        assert st["rows_in"] == n and len(out.keys) == n
        got = {k[0][1]: result_pair(a[0]) for k, a in zip(out.keys, out.aggs)}
        for r in rows:
            want = au.apply(fn, r["a"], "a")
            if want == au.R_MISSING:
                want = au.R_NULL
            assert got[r["id"]] == want, (fn, n, r, got[r["id"]], want)


@pytest.mark.parametrize("n", [65, 769])
def test_missing_and_null_are_told_apart_and_a_dictionary_coded_operand_is_never_an_array(n):
    rows, table = lookup_table(n)
    for fn in au.FUNCTIONS:
        for col in ("a", "s"):
            text = au.term_text(fn, "a" if fn in au.BINARY else None, over=D(col))
            vals = [au.apply(fn, r[col], "a") for r in rows]
            if col == "s":
                assert all(v in (au.R_NULL, au.R_MISSING) for v in vals)
            for pred, want in (("missing", sum(v == au.R_MISSING for v in vals)), ("null", sum(v == au.R_NULL for v in vals))):
                out, st = must_run(pu.run_gpu, table, "(%s is %s)" % (text, pred), [], ["count(*)"])
                assert st["rows_selected"] == want, (fn, col, pred, st["rows_selected"], want)


# ------------------------------------------------------------------ a table extended across two batches

def numbered_arrays(tag, n):
    """n distinct arrays the kernel decides itself, and three it does not: over 192 bytes, an escape first, a 19-digit integer"""
    arrays = [[tag, i, "t_1"] if i % 3 else [tag, i] for i in range(n)]
    arrays[1] = [tag] + ["w" * 20] * 12
    arrays[2] = ['x"y', tag]
    arrays[3] = [1234567890123456789, tag]
    return arrays


@pytest.mark.parametrize("route", ["host", "device"])
def test_a_table_extended_across_two_batches(route):
    """array_contains(a, "t_1") and array_sum(a) in one plan.  The first batch interns a dictionary below the threshold: the host
    evaluator.  The second brings new entries — threshold - 1 of them: the host route again; threshold + 1: the kernel, which
    hands over the three arrays it does not decide — and the old entries keep their values."""
    contains, total = au.term_text("array_contains", "t_1", over=D("a")), au.term_text("array_sum", over=D("a"))
    cond = "(%s and (%s < 1000))" % (contains, total)
    op = query_amd.GpuFilterGroup(plan.filter_group_plan(cond, [], ["count(*)"]))
    try:
        T = op.arrfn_stats()["device_threshold"]
        dictionary, arrays = [], []
        want_dev = want_host = 0
        for tag, n in (("s", 50), ("u", T - 2 if route == "host" else T)):  # (+ 1: the entry that is no array)
            new = numbered_arrays(tag, n)
            texts = au.texts_of(new) + [b"not an array " + tag.encode()]
            on_device = len(texts) >= T
            dictionary += texts
            arrays += new + [None]
            rng = np.random.default_rng(len(dictionary))
            codes = np.concatenate([np.arange(len(dictionary)), rng.integers(0, len(dictionary), 5000)]).astype(np.uint64)
            tags = np.where(np.array([a is None for a in arrays])[codes.astype(np.int64)], n1o.T_STRING, n1o.T_ARRAY).astype(np.uint8)
            col = n1o.Column(D("a"), n1o.COL_TAGGED64, tags=tags, payload=codes)
            assert op.column_paths == [D("a")]
            op.process_items([col], dictionary)
            got = op.after_items().aggs[0][0][1]
            assert int(_ffi.lib().n1k_dict_size(op._h)) == len(dictionary)  # (the handle interned nothing of its own)
            hit = np.array([a is not None and au.apply("array_contains", a, "t_1") == au.R_TRUE and
                            au.result_json(au.apply("array_sum", a)) < 1000 for a in arrays])
            want = int(hit[codes.astype(np.int64)].sum())
            assert 0 < want < len(codes) and got == want, (tag, got, want)
            if on_device:
                want_dev, want_host = want_dev + n - 3, want_host + 3
            else:
                want_host += n
            st = op.arrfn_stats()
            assert (st["device_arrays"], st["host_arrays"], st["terms"]) == (want_dev, want_host, 2), (tag, st, want_dev, want_host)
            op.reopen()  # (keeps the tables)
        assert (want_dev > 0) == (route == "device")
    finally:
        op.done()


# ------------------------------------------------------------------ the reference's statements

@pytest.mark.parametrize("case", ARR["cases"], ids=[c["id"] for c in ARR["cases"]])
def test_the_references_having_statement_end_to_end(case):
    docs = gu.load_docs(case["keyspace"])
    table = gu.build_table(docs, case["columns"])
    p = case["plan"]
    rows, _ = must_run(pu.run_gpu, table, p["condition"], p["group_keys"], p["aggregates"], having=case["having_text"])
    got = gu.replay_post(case, gu.groups_from_result(rows), having_done=True)
    assert gu.same_json(got, case["results"]), (got, case["results"])


def recorded_plan(row):
    return (None, [au.term_text(row["function"], row["second"], over="(`t`.`a`)")], ["count(*)"])


@pytest.mark.parametrize("row", ARR["rows"], ids=[r["id"] for r in ARR["rows"]])
def test_the_recorded_rows_with_the_array_as_a_column_value(row):
    table = gu.build_table([{"doc": {"a": row["array"]}}], ["(`t`.`a`)"])
    cond, keys, aggs = recorded_plan(row)
    out, _ = must_run(pu.run_gpu, table, cond, keys, aggs)
    assert len(out.keys) == 1 and out.aggs[0][0][1] == 1
    assert gu.same_json(gu.decode_value(out.keys[0][0]), row["result"]), (out.keys[0][0], row["result"])


# ------------------------------------------------------------------ one plan per placement

A, K, X, G = D("a"), D("k"), D("x"), D("g")
LEN, SUM, CNT = au.term_text("array_length", over=A), au.term_text("array_sum", over=A), au.term_text("array_count", over=A)
HAS = au.term_text("array_contains", "a", over=A)
POS = au.term_text("array_position", "a", over=A)
# name -> ((function, constant) of the helper column, plan text with {h} where the term stands)
PLACEMENTS = {
    "filter-operand": (("array_length", None), ("(1 < {h})", [K], ["count(*)", "max(%s)" % X])),
    "filter-bare": (("array_contains", "a"), ("({h} and (10 < %s))" % X, [K], ["count(*)"])),
    "group-key": (("array_count", None), (None, ["{h}", K], ["count(*)"])),
    "aggregate-operand": (("array_position", "a"), (None, [K], ["count(*)", "max({h})", "sum({h})"])),
    "operand-of-arithmetic": (("array_length", None), ("(({h} + %s) < 6)" % G, [], ["count(*)", "sum(({h} * 2))"])),
    "argument-of-round": (("array_avg", None), ("(round({h}, 1) <= 2)", [K], ["count(*)"])),
}


def placement_plan(name, h):
    cond, keys, aggs = PLACEMENTS[name][1]
    return (cond.format(h=h) if cond else None, [k.format(h=h) for k in keys], [a.format(h=h) for a in aggs])


@functools.lru_cache(maxsize=None)
def placement_rows():
    rows = au.make_rows(random.Random(20261021), 3000)
    return rows, au.make_table(rows)


@pytest.mark.parametrize("name", sorted(PLACEMENTS))
def test_one_plan_per_placement_against_the_oracle_by_substitution(name):
    rows, t = placement_rows()
    fn, c = PLACEMENTS[name][0]
    values = [au.result_value(au.apply(fn, r["a"], c)) for r in rows]
    ot = n1o.Table(list(t.columns) + [au.column("h", values)], t.dictionary)
    dcond, dkeys, daggs = placement_plan(name, au.term_text(fn, c, over=A))
    ocond, okeys, oaggs = placement_plan(name, D("h"))
    ora = n1o.run(ot, ocond, okeys, oaggs)
    for batches in (1, 3):
        gpu, st = must_run(pu.run_gpu, t, dcond, dkeys, daggs, batches=batches)
        pu.assert_same_groups(gpu, ora, aggs=oaggs)
        assert st["rows_selected"] == ora.rows_passed and ora.rows_passed > 0


def case_plan():
    n = au.term_text("array_length", over=A)
    return (None, [D("id")], ["max(%s)" % plan.case_when([("(%s < 2)" % n, n)], D("id")), "max(%s)" % plan.cond_fn("ifnull", au.term_text("array_avg", over=A), "(-1)")])


def test_an_operand_inside_a_conditional_node():
    """CASE WHEN array_length(a) < 2 THEN array_length(a) ELSE id END and IFNULL(array_avg(a), -1) per row: the array function
    is a derived column in front of the conditional node's (the oracle knows no CASE: against the yardstick)"""
    rows, table = lookup_table(257)
    cond, keys, aggs = case_plan()
    out, _ = must_run(pu.run_gpu, table, cond, keys, aggs)
    got = {k[0][1]: (result_pair(a[0]), result_pair(a[1])) for k, a in zip(out.keys, out.aggs)}
    assert len(got) == len(rows)
    for r in rows:
        n, avg = au.apply("array_length", r["a"]), au.apply("array_avg", r["a"])
        want_case = n if n[0] == au.T_INT and au.result_json(n) < 2 else au.r_int(r["id"])
        want_ifnull = au.r_int(-1) if avg == au.R_NULL else (au.R_NULL if avg == au.R_MISSING else avg)  # (a MISSING operand IS returned; MAX folds it to NULL)
        assert got[r["id"]] == (want_case, want_ifnull), (r, got[r["id"]], want_case, want_ifnull)


def key_value(k):
    if k[0] == n1o.T_MISSING:
        return M
    if k[0] in (n1o.T_ARRAY, n1o.T_OBJECT):
        return json.loads(k[1].decode())
    return gu.decode_value(k)


def test_having_over_an_array_valued_group_key():
    rows, t = placement_rows()
    keys, aggs = [A], ["count(*)"]
    ora = n1o.run(t, None, keys, aggs)
    for having, keep in (("(2 <= %s)" % LEN, lambda a: isinstance(a, list) and len(a) >= 2),
                         (HAS, lambda a: au.apply("array_contains", a, "a") == au.R_TRUE),
                         ("(%s is missing)" % CNT, lambda a: a is M),
                         ("(%s is null)" % SUM, lambda a: a is not M and not isinstance(a, list))):
        gpu, _ = must_run(pu.run_gpu, t, None, keys, aggs, having=having)
        want = sorted((k[0], a[0][1]) for k, a in zip(ora.keys, ora.aggs) if keep(key_value(k[0])))
        got = sorted((k[0], a[0][1]) for k, a in zip(gpu.keys, gpu.aggs))
        assert got == want and 1 <= len(want) < len(ora.keys), (having, got, want)


def test_a_projection_and_having_over_array_agg():
    """array_length / array_sum / array_contains of ARRAY_AGG(g) per group, projected and in HAVING, ordered through the alias"""
    rows, t = placement_rows()
    keys, aggs = [K], ["array_agg(%s)" % G]
    ora = n1o.run(t, None, keys, aggs)
    agg = aggs[0]
    arrays = {gu.decode_value(k[0]) if k[0][0] != n1o.T_MISSING else "MISSING": json.loads(a[0][1].decode()) for k, a in zip(ora.keys, ora.aggs)}
    assert len(arrays) >= 4
    lengths = sorted(len(a) for a in arrays.values())
    cut = lengths[len(lengths) // 2]
    project = [(K, "k"), (au.term_text("array_length", over=agg), "n"), (au.term_text("array_sum", over=agg), "s"),
               (au.term_text("array_contains", 3, over=agg), "c"), ("(%s + 1)" % au.term_text("array_position", 6, over=agg), "p")]
    gpu, _ = must_run(pu.run_gpu, t, None, keys, aggs, having="(%d <= %s)" % (cut, au.term_text("array_length", over=agg)), project=project,
                      order=[("`n`", True)])
    got = [[(M if v[0] == n1o.T_MISSING else gu.decode_value(v)) if i == 0 else result_pair(v) for i, v in enumerate(r)] for r in gpu.proj]
    want = {}
    for k, a in arrays.items():
        if len(a) >= cut:
            pos = au.result_json(au.apply("array_position", a, 6))  # (Add.Apply folds from INT 0: -1 + 1 is the FLOAT 0.0)
            want[k] = [au.apply("array_length", a), au.apply("array_sum", a), au.apply("array_contains", a, 3),
                       au.result_of_number(au.num_add(au.num_add(0, pos), 1))]
    assert 1 <= len(want) < len(arrays) and len(got) == len(want)
    for r in got:
        assert want["MISSING" if r[0] is M else r[0]] == r[1:], (r, want)
    ns = [au.result_json(r[1]) for r in got]
    assert ns == sorted(ns, reverse=True)


def stated_plans():
    """every plan this file states (not the seeded ones): tests/test_arrfn_cpu.py creates them without a GPU"""
    out = [lookup_plan(fn, col) + ({},) for fn in au.FUNCTIONS for col in ("a", "s")]
    out += [placement_plan(name, au.term_text(*PLACEMENTS[name][0], over=A)) + ({},) for name in PLACEMENTS]
    out += [recorded_plan(row) + ({},) for row in ARR["rows"]] + [case_plan() + ({},)]
    return out


# ------------------------------------------------------------------ differential by substitution

FAMILIES = [{"fast": 0}, {}, {"spec": 0}, {"jit": 0}]


@pytest.mark.parametrize("seed", range(NSEEDS))
def test_array_function_plans_agree_with_the_oracle_by_substitution(seed):
    p = au.draw_plan(seed)
    opts = FAMILIES[seed % len(FAMILIES)]
    t = au.make_table(p["rows"])
    ot = n1o.Table(list(t.columns) + [au.column("h", p["values"])], t.dictionary)
    (dcond, dkeys, daggs), (ocond, okeys, oaggs) = p["device"], p["oracle"]
    what = "seed %d use %s device %r %r %r opts %r" % (seed, p["use"], dcond, dkeys, daggs, opts)
    ora = n1o.run(ot, ocond, okeys, oaggs, threads=2)
    gpu, st = must_run(pu.run_gpu, t, dcond, dkeys, daggs, batches=1 + seed % 3, **opts)
    try:
        pu.assert_same_groups(gpu, ora, aggs=oaggs)
    except AssertionError as e:
        raise AssertionError("%s | %s" % (e, what))
    assert st["rows_selected"] == ora.rows_passed, what
    if p["use"].startswith("filter"):  # the Filter alone: the selected row ordinals, as they come
        gsel, _ = must_run(pu.run_gpu, t, dcond, [], [], filter_only=True, batches=1 + seed % 2)
        osel = n1o.run(ot, ocond, [], [], has_group=False)
        assert np.array_equal(np.asarray(gsel.selected, dtype=np.uint64), osel.selected), what
