"""CASE and IFMISSING / IFNULL / IFMISSINGORNULL / NULLIF / MISSINGIF as values, on the device: the reference's statements, and
a differential against the oracle BY SUBSTITUTION as tests/test_gpu_coll.py does it — the oracle has no conditional
expressions, so where the device's plan holds one the oracle's reads a TAGGED64 helper column with the mirror's value of
every row (tests/cond_util.py)."""
import collections
import json
import os

import numpy as np
import pytest

import coll_util as cu
import cond_util as cn
import golden_util as gu
import parity_util as pu
import query_amd
from oracle import n1o
from query_amd import _ffi, plan
from query_amd.gpu_operator import GroupRows

pytestmark = pytest.mark.gpu

D = cn.D
M = cn.MISSING

with open(os.path.join(gu.GOLDEN, "cases_cond.json")) as fh:
    COND_CASES = json.load(fh)["cases"]


def key_text(v):
    """a value as a dictionary key: numbers as value.NewValue holds them (an integral float IS the int)"""
    return "MISSING" if (v is M or v is gu.MISSING) else json.dumps(cu.norm(v), sort_keys=True)


@pytest.mark.parametrize("case", COND_CASES, ids=[c["id"] for c in COND_CASES])
def test_the_references_conditional_statements(case):
    """GROUP BY <the expression>, count(*): the groups are the multiset of the values the reference's statement returns."""
    docs = gu.load_docs(case["keyspace"])
    table = gu.build_table(docs, case["columns"])
    p = case["plan"]
    rows, _ = pu.run_gpu(table, p["condition"], p["group_keys"], p["aggregates"])
    got = {key_text(gu.decode_value(k[0])): a[0][1] for k, a in zip(rows.keys, rows.aggs)}
    want = collections.Counter(key_text(r.get(case["alias"], M)) for r in case["results"])
    assert got == dict(want), (got, want)


# ------------------------------------------------------------------ differential by substitution

# NOTE: tests/test_cond_cpu.py creates every plan drawn here (cond_util.draw_plan over range(NSEEDS)) without a GPU.
# (options, run through n1k_run_device_batch instead of the three calls)
FAMILIES = [({"fast": 0}, False), ({}, False), ({"spec": 0}, True), ({"jit": 2}, False), ({"fast": 0}, True), ({"jit": 2}, True)]
NSEEDS = 120


def device_batch(op, table):
    """the table's columns in device memory, in the plan's order: (n1k_batch, what keeps the memory alive)"""
    import torch
    codes = op.intern(list(table.dictionary))
    assert np.array_equal(codes, np.arange(len(table.dictionary), dtype=np.uint32))
    by = {c.name: c for c in table.columns}
    keep, cols = [], []
    for p in op.column_paths:
        c = by[p]
        if c.kind == n1o.COL_DICT32:
            x = torch.from_numpy(np.ascontiguousarray(c.codes).view(np.int32)).cuda()
            keep.append(x)
            cols.append((_ffi.COL_DICT32, None, None, x.data_ptr()))
        else:
            a, b = torch.from_numpy(np.ascontiguousarray(c.tags)).cuda(), torch.from_numpy(np.ascontiguousarray(c.payload).view(np.int64)).cuda()
            keep += [a, b]
            cols.append((_ffi.COL_TAGGED64, a.data_ptr(), b.data_ptr(), None))
    torch.cuda.synchronize()
    return op.make_device_batch(table.nrows, cols), keep


def run_one_call(table, cond, keys, aggs, **options):
    op = query_amd.GpuFilterGroup(plan.filter_group_plan(cond, keys, aggs), **options)
    try:
        batch, keep = device_batch(op, table)
        out = []
        for _ in range(2):  # (a handle's second execution starts from the state its first one left)
            raw = op.run_device_batch_raw(batch)
            cache = {}
            out.append(GroupRows(len(keys), len(aggs), op._py_values(raw["keys"], cache), op._py_values(raw["aggs"], cache), []))
        return out, op.stats()
    finally:
        op.done()


@pytest.mark.parametrize("seed", range(NSEEDS))
def test_conditional_plans_agree_with_the_oracle_by_substitution(seed):
    p = cn.draw_plan(seed)
    opts, one_call = FAMILIES[seed % len(FAMILIES)]
    t = cn.make_table(p["rows"])
    ot = n1o.Table(list(t.columns) + [cn.helper_column("h", p["values"])], t.dictionary)
    (dcond, dkeys, daggs), (ocond, okeys, oaggs) = p["device"], p["oracle"]
    what = "seed %d use %s device %r %r %r opts %r one_call %r" % (seed, p["use"], dcond, dkeys, daggs, opts, one_call)
    ora = n1o.run(ot, ocond, okeys, oaggs, threads=2)
    if one_call:
        results, st = run_one_call(t, dcond, dkeys, daggs, **opts)
    else:
        gpu, st = pu.run_gpu(t, dcond, dkeys, daggs, batches=1 + seed % 3, **opts)
        results = [gpu]
    for gpu in results:
        try:
            pu.assert_same_groups(gpu, ora, aggs=oaggs)
        except AssertionError as e:
            raise AssertionError("%s | %s" % (e, what))
    assert st["rows_selected"] == ora.rows_passed, what
    assert st["spec_kernel"] != 3, what  # (3: arithmetic nodes in registers — a plan with a conditional node never fuses)
    if p["use"] in ("filter_cmp", "filter_bare"):  # the Filter alone: the selected row ordinals, as they come
        gsel, _ = pu.run_gpu(t, dcond, [], [], filter_only=True, batches=1 + seed % 2)
        osel = n1o.run(ot, ocond, [], [], has_group=False)
        assert np.array_equal(np.asarray(gsel.selected, dtype=np.uint64), osel.selected), what


def test_the_substitution_is_sound_on_the_cpu_side_of_this_test():
    """The oracle over the helper column groups by exactly the mirror's values."""
    p = cn.draw_plan(0)
    assert p["use"] == "key"
    t = cn.make_table(p["rows"])
    ot = n1o.Table(list(t.columns) + [cn.helper_column("h", p["values"])], t.dictionary)
    ora = n1o.run(ot, None, [D("h")], ["count(*)"])
    want = collections.Counter(key_text(v) for v in p["values"])
    got = collections.Counter()
    for k, a in zip(ora.keys, ora.aggs):
        got[key_text(gu.decode_value(k[0]))] += a[0][1]
    assert got == want and len(want) > 3


# ------------------------------------------------------------------ directed

def int_table(values, name="x", extra=None):
    cols = [cn.helper_column(name, values)] + [cn.helper_column(n, v) for n, v in (extra or {}).items()]
    return n1o.Table(cols, list(cn.DICT))


def groups_of(rows):
    return {key_text(gu.decode_value(k[0])): a[0][1] for k, a in zip(rows.keys, rows.aggs)}


BUCKET = plan.case_when([("(%s < 10)" % D("x"), '"low"'), ("(%s < 100)" % D("x"), '"mid"')], '"high"')


def bucket_of(v):
    return "low" if v < 10 else ("mid" if v < 100 else "high")


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 3 * 256 + 17])
def test_row_counts_around_the_launch_geometry(n):
    values = [(i * 37) % 150 for i in range(n)]
    rows, st = pu.run_gpu(int_table(values), None, [BUCKET], ["count(*)"])
    assert groups_of(rows) == {key_text(k): c for k, c in collections.Counter(bucket_of(v) for v in values).items()}
    assert st["rows_in"] == n


def test_three_uneven_batches_regrow_the_derived_columns():
    """700, 1 and 4099 rows: the node's buffers grow twice, behind the stream synchronisation of materialize_derived."""
    sizes = [700, 1, 4099]
    values = [(i * 37) % 150 for i in range(sum(sizes))]
    op = query_amd.GpuFilterGroup(plan.filter_group_plan(None, [BUCKET], ["count(*)", "sum(%s)" % plan.cond_fn("nullif", D("x"), "36")]))
    try:
        for round_ in range(2):
            lo = 0
            for s in sizes:
                t = int_table(values[lo:lo + s])
                op.process_items(t.columns, t.dictionary)
                lo += s
            rows = op.after_items()
            want = collections.Counter(bucket_of(v) for v in values)
            assert groups_of(rows) == {key_text(k): c for k, c in want.items()}
            sums = {gu.decode_value(k[0]): a[1][1] for k, a in zip(rows.keys, rows.aggs)}
            assert sums == {b: sum(v for v in values if bucket_of(v) == b and v != 36) for b in want}
            op.reopen()
    finally:
        op.done()


def test_arm_order():
    values = list(range(40)) + [None, M]
    # two arms both TRUE: the first wins
    both = plan.case_when([("(%s < 30)" % D("x"), '"first"'), ("(%s < 20)" % D("x"), '"second"')], '"else"')
    rows, _ = pu.run_gpu(int_table(values), None, [both], ["count(*)"])
    assert groups_of(rows) == {'"first"': 30, '"else"': 12}
    # no arm taken: ELSE, and NULL without one
    none = plan.case_when([("(%s < 0)" % D("x"), "1")])
    rows, _ = pu.run_gpu(int_table(values), None, [none], ["count(*)"])
    assert groups_of(rows) == {"null": 42}
    rows, _ = pu.run_gpu(int_table(values), None, [plan.case_when([("(%s < 0)" % D("x"), "1")], D("x"))], ["count(*)"])
    assert groups_of(rows) == {key_text(v): 1 for v in values}
    # eight arms, each taken by some row
    eight = plan.case_when([("(%s = %d)" % (D("x"), i), str(100 + i)) for i in range(8)], "0")
    rows, _ = pu.run_gpu(int_table(values), None, [eight], ["count(*)"])
    assert groups_of(rows) == dict([(str(100 + i), 1) for i in range(8)] + [("0", 34)])
    simple = plan.case_of(D("x"), [(str(i), str(100 + i)) for i in range(8)], "0")
    rows, _ = pu.run_gpu(int_table(values), None, [simple], ["count(*)"])
    assert groups_of(rows) == dict([(str(100 + i), 1) for i in range(8)] + [("0", 34)])


def test_a_later_arm_is_evaluated_only_for_the_rows_that_reach_it():
    """Arm 2 orders an array-valued column against an array-valued one: with every such row taken by arm 1 the query
    succeeds; one row that reaches arm 2 is N1K_UNSUPPORTED_DATA, and the handle goes on working."""
    arr, other = [1, 2], ["a"]
    a = [arr if i % 3 == 0 else i for i in range(600)]
    b = [other if i % 3 == 0 else 5 for i in range(600)]
    x = [1 if i % 3 == 0 else 0 for i in range(600)]  # arm 1 takes every row whose a is an array
    node = plan.case_when([("(%s = 1)" % D("x"), '"taken"'), ("(%s < %s)" % (D("a"), D("b")), '"lt"')], '"ge"')
    op = query_amd.GpuFilterGroup(plan.filter_group_plan(None, [node], ["count(*)"]))
    try:
        t = int_table(x, extra={"a": a, "b": b})
        by = {c.name: c for c in t.columns}
        cols = lambda tt: [{c.name: c for c in tt.columns}[p] for p in op.column_paths]  # noqa: E731
        op.process_items(cols(t), t.dictionary)
        want = {'"taken"': 200, '"lt"': sum(1 for i in range(600) if i % 3 and i < 5), '"ge"': sum(1 for i in range(600) if i % 3 and i >= 5)}
        assert groups_of(op.after_items()) == want and by
        op.reopen()
        x[300] = 0  # this row now reaches arm 2 with two arrays under <
        t2 = int_table(x, extra={"a": a, "b": b})
        with pytest.raises(query_amd.N1kError) as ei:
            op.process_items(cols(t2), t2.dictionary)
            op.after_items()
        assert ei.value.status == _ffi.UNSUPPORTED_DATA, ei.value
        op.reopen()
        op.process_items(cols(t), t.dictionary)
        assert groups_of(op.after_items()) == want
    finally:
        op.done()


def cat_table(cats, prices, dictionary):
    code = {w: i for i, w in enumerate(dictionary)}
    codes = np.array([code[c.encode()] for c in cats], np.uint32)
    n = len(prices)
    return n1o.Table([n1o.Column(D("cat"), n1o.COL_DICT32, codes=codes),
                      n1o.Column(D("price"), n1o.COL_TAGGED64, tags=np.full(n, n1o.T_INT, np.uint8), payload=np.array(prices, np.int64).view(np.uint64))], list(dictionary))


def test_string_results_are_dictionary_codes_of_the_handles_dictionary():
    """CASE WHEN price > 50 THEN cat ELSE "cat_1" END over a table that holds "cat_1": ONE group for it.  A THEN constant no row
    holds gets its own group.  Both still hold after the dictionary has grown between two batches."""
    node = plan.case_when([("(50 < %s)" % D("price"), D("cat"))], '"cat_1"')
    fresh = plan.case_when([("(50 < %s)" % D("price"), D("cat"))], '"nowhere"')
    d1 = [b"cat_0", b"cat_1", b"cat_2"]
    d2 = d1 + [b"cat_3", b"nowhere_else"]
    cats1, prices1 = ["cat_0", "cat_1", "cat_2", "cat_1", "cat_2"], [60, 70, 10, 20, 90]
    cats2, prices2 = ["cat_3", "cat_1", "cat_3", "cat_0"], [99, 51, 1, 2]
    for text, other in ((node, "cat_1"), (fresh, "nowhere")):
        op = query_amd.GpuFilterGroup(plan.filter_group_plan(None, [text], ["count(*)"]))
        try:
            want = collections.Counter()
            for cats, prices, d in ((cats1, prices1, d1), (cats2, prices2, d2)):
                t = cat_table(cats, prices, d)
                op.process_items([{c.name: c for c in t.columns}[p] for p in op.column_paths], t.dictionary)
                want.update(c if p > 50 else other for c, p in zip(cats, prices))
            got = groups_of(op.after_items())
            assert got == {key_text(k): c for k, c in want.items()}, (text, got)
            assert (other == "nowhere") == ('"nowhere"' in got)
        finally:
            op.done()


def test_ifnull_returns_a_missing_first_argument():
    values = [M, None, 3, M, None, 4]
    rows, _ = pu.run_gpu(int_table(values), None, [plan.cond_fn("ifnull", D("x"), "7")], ["count(*)"])
    assert groups_of(rows) == {"MISSING": 2, "7": 2, "3": 1, "4": 1}
    rows, _ = pu.run_gpu(int_table(values), None, [plan.cond_fn("ifmissing", D("x"), "7")], ["count(*)"])
    assert groups_of(rows) == {"7": 2, "null": 2, "3": 1, "4": 1}
    rows, _ = pu.run_gpu(int_table(values), None, [plan.cond_fn("ifmissingornull", D("x"), D("x"), "7")], ["count(*)"])
    assert groups_of(rows) == {"7": 4, "3": 1, "4": 1}


def test_nullif_compares_numbers_by_value_and_missingif_gives_a_missing_key():
    score = [1, 8, 10, 10, 100, 100.0, 100.5, None, M, "zz"]
    t = int_table(score, name="score")
    by_float, _ = pu.run_gpu(t, None, [plan.cond_fn("nullif", D("score"), "100.0")], ["count(*)"])
    by_int, _ = pu.run_gpu(t, None, [plan.cond_fn("nullif", D("score"), "100")], ["count(*)"])
    assert groups_of(by_float) == groups_of(by_int) == {"1": 1, "8": 1, "10": 2, "null": 3, "100.5": 1, "MISSING": 1, '"zz"': 1}
    rows, _ = pu.run_gpu(t, None, [plan.cond_fn("missingif", D("score"), "100")], ["count(*)"])
    assert groups_of(rows) == {"1": 1, "8": 1, "10": 2, "MISSING": 3, "100.5": 1, "null": 1, '"zz"': 1}


@pytest.mark.timeout(600)
def test_a_conditional_plan_across_two_ranks_over_the_loopback_transport():
    """World size 2, row exchange: the sender's Filter reads a conditional node — a derived column materialised before the
    partition kernel — and the receiver evaluates the aggregate's node over the rows it was sent; every rank ends with the
    substituted oracle's groups."""
    import random

    from query_amd import distributed as qd
    from test_gpu_distributed import _device_cols, _run_ranks
    world, n = 2, 20_011
    rows = cn.make_rows(random.Random(77), n)
    t = cn.make_table(rows)
    cond_node = ("fn", "ifmissingornull", [("col", "x"), ("const", 0)])
    agg_node = ("case", [(("cmp", "<", ("col", "x"), ("const", 50)), ("col", "x"))], ("const", 0))
    dcond, ocond = "(10 < %s)" % cn.value_text(cond_node), "(10 < %s)" % D("h0")
    keys = [D("k")]
    daggs, oaggs = ["count(*)", "sum(%s)" % cn.value_text(agg_node)], ["count(*)", "sum(%s)" % D("h1")]
    ot = n1o.Table(list(t.columns) + [cn.helper_column("h0", [cn.eval_value(cond_node, r) for r in rows]),
                                      cn.helper_column("h1", [cn.eval_value(agg_node, r) for r in rows])], t.dictionary)
    ora = n1o.run(ot, ocond, keys, oaggs)
    assert 0 < ora.rows_passed < n
    comms = qd.Comm.loopback(world, 0)
    probe = query_amd.GpuFilterGroup(plan.filter_group_plan(dcond, keys, daggs))
    paths = probe.column_paths
    probe.done()
    shards, keep = [], []
    for r in range(world):
        dev, k = _device_cols(t.slice(n * r // world, n * (r + 1) // world), paths)
        keep.append(k)
        shards.append((n * (r + 1) // world - n * r // world, dev))

    def rank_body(r):
        op = qd.ShardedFilterGroup(dcond, keys, daggs, t.dictionary, r, world, 0, comm=comms[r])
        for h in (op.sender, op.receiver):
            h.set_option("jit", 0)
        op.row_capacity = 2 * n
        raw, info = op.run_rows(*shards[r])
        cache = {}
        return GroupRows(1, len(daggs), op.merger._py_values(raw["keys"], cache), op.merger._py_values(raw["aggs"], cache), []), info

    outs = _run_ranks(world, rank_body)
    for got, info in outs:
        pu.assert_same_groups(got, ora, aggs=oaggs)
        assert info["mode"] == "rows"
    assert sum(info["recv_rows"] for _, info in outs) == ora.rows_passed
