"""One-call executions (n1k_run_device_batch) whose only scan launch leaves slabs: n1k_finish folds the slabs straight into
result rows (fold_rows_kernel) instead of merging them into the table and finalising that.  Every case runs the one-call
path and the same handle's three-call path (reset / push / finish: merge_slabs_kernel + finalize_small_kernel) and holds both
against the oracle: the groups, the survivors, and every float SUM / AVG against the exact sum within n * 2^-53 * sum|x|.

Which of the two tails a case takes is decided by slabs_to_rows (n1k_finish.cpp) and is NOT observable through the ABI: both
return the same rows, counters and statistics (that is the point), and the tests may add no option or statistic.  The cases
are therefore chosen on both sides of every term of that predicate — an odd row count, one workgroup, slabs off, an explicit
merge_chunks, a 16384-slot table take the old tail — and the sequence test proves what can be proved from outside: the device
really is clean behind the new kernel (the next execution starts without a reset kernel and is right) and really is
re-initialised behind the old one.  Which kernels ran is read off the committed profile (profiles/r04_*).

The bounded and the plan-specialised kernels take at most five aggregates, and a run-time-built scan a table of at most
64 KiB (eight words per slot at 1000 categories), so "every aggregate kind and count(*) with jit = 2" is three shapes that
fit a run-time-built scan at K_cat = 1000 plus one of five aggregates, which is run-time-built at 37 categories and takes the
bounded-shape kernel (1024 threads, one workgroup per CU) at 1000."""
import functools

import numpy as np
import pytest

import geometry_util as gu
import parity_util as pu
import query_amd
from oracle import n1o
from query_amd import _ffi, plan
from query_amd.gpu_operator import GroupRows, N1kError

pytestmark = pytest.mark.gpu

D = gu.D
PRICE, CAT, USER, V = D("price"), D("cat"), D("user_id"), D("v")
COND = "(50 < %s)" % PRICE
TILE = 2048  # rows of a scan tile at 512 threads

SHAPES = {
    # name: (condition, aggregates, operand column checked against exact sums, options)
    "prebuilt_sum": (COND, ["sum(%s)" % PRICE], PRICE, {}),
    "jit_sum_avg": (COND, sorted(["sum(%s)" % PRICE, "avg(%s)" % PRICE]), PRICE, {"jit": 2}),
    "jit_min_count_countn": (COND, sorted(["min(%s)" % PRICE, "count(*)", "countn(%s)" % PRICE]), None, {"jit": 2}),
    "jit_max_count": (COND, sorted(["max(%s)" % USER, "count(%s)" % PRICE]), None, {"jit": 2}),
    "five_aggregates": (COND, sorted(["sum(%s)" % PRICE, "avg(%s)" % PRICE, "min(%s)" % PRICE, "max(%s)" % PRICE, "count(*)"]), PRICE, {"jit": 2}),
    "bounded_count_min": (COND, sorted(["count(*)", "min(%s)" % PRICE]), None, {"spec": 0}),
}


@functools.lru_cache(maxsize=None)
def synth(n, k_cat):
    return n1o.synth_table(n, k_cat=k_cat)


@functools.lru_cache(maxsize=None)
def mixed(n, k_cat):
    """records_table's operand column (ints of both signs, ints >= 2^40, floats, NULL, MISSING, a boolean, a string) over a
    dictionary-coded key."""
    r = gu.records_table(n, key_range=k_cat)
    by = {c.name: c for c in r.columns}
    codes = by[D("k")].payload.astype(np.uint32)
    return n1o.Table([n1o.Column(CAT, n1o.COL_DICT32, codes=codes), by[V]], [b"cat_%d" % i for i in range(k_cat)])


@functools.lru_cache(maxsize=None)
def oracle(tkey, cond, keys, aggs):
    return n1o.run(TABLES[tkey[0]](*tkey[1:]), cond, list(keys), list(aggs), threads=4)


@functools.lru_cache(maxsize=None)
def selected(tkey, cond):
    t = TABLES[tkey[0]](*tkey[1:])
    return np.arange(t.nrows) if cond is None else n1o.run(t, cond, [], [], has_group=False).selected


TABLES = {"synth": synth, "mixed": mixed}


def device_batch(op, t):
    import torch
    codes = op.intern(list(t.dictionary))
    assert np.array_equal(codes, np.arange(len(t.dictionary), dtype=np.uint32))
    by = {c.name: c for c in t.columns}
    keep, cols = [], []
    for p in op.column_paths:
        c = by[p]
        if c.kind == n1o.COL_DICT32:
            a = torch.from_numpy(np.ascontiguousarray(c.codes).view(np.int32)).cuda()
            keep.append(a)
            cols.append((_ffi.COL_DICT32, None, None, a.data_ptr()))
        else:
            a = torch.from_numpy(np.ascontiguousarray(c.tags)).cuda()
            b = torch.from_numpy(np.ascontiguousarray(c.payload).view(np.int64)).cuda()
            keep += [a, b]
            cols.append((_ffi.COL_TAGGED64, a.data_ptr(), b.data_ptr(), None))
    torch.cuda.synchronize()
    return op.make_device_batch(t.nrows, cols), keep


def rows_of(op, raw):
    cache = {}
    return GroupRows(raw["nkeys"], raw["naggs"], op._py_values(raw["keys"], cache) if raw["ngroups"] else [],
                     op._py_values(raw["aggs"], cache) if raw["ngroups"] else [], [])


def hold(op, raw, stats, tkey, cond, keys, aggs, val):
    """One result of the handle against the oracle."""
    ora = oracle(tkey, cond, tuple(keys), tuple(aggs))
    got = rows_of(op, raw)
    assert raw["ngroups"] == len(ora.keys)
    pu.assert_same_groups(got, ora, aggs=aggs)
    assert stats["rows_selected"] == ora.rows_passed
    assert stats["groups_out"] == len(ora.keys)
    if val and any(a.startswith(("sum(", "avg(")) for a in aggs):
        exact = gu.exact_sums(TABLES[tkey[0]](*tkey[1:]), selected(tkey, cond), keys[0], val)
        assert gu.assert_float_sums_exact(got, exact, aggs, val) > 0 or not exact
    return ora


def one_call_and_three_calls(tkey, cond, aggs, val, expect_direct=True, **opts):
    t = TABLES[tkey[0]](*tkey[1:])
    keys = [CAT]
    op = query_amd.GpuFilterGroup(plan.filter_group_plan(cond, keys, aggs), **opts)
    try:
        batch, _keep = device_batch(op, t)
        raw = op.run_device_batch_raw(batch)
        st = op.stats()
        if expect_direct:
            assert st["agg_mode"] == _ffi.MODE_LDS_DIRECT
        hold(op, raw, st, tkey, cond, keys, aggs, val)
        # A handle's FIRST execution finds no device state at its reset (device_clean is false) and takes the old tail; it
        # leaves the device clean, so this second one is the run that goes through fold_rows_kernel.  Keep both.
        again = op.run_device_batch_raw(batch)
        hold(op, again, op.stats(), tkey, cond, keys, aggs, val)
        assert op.stats()["query_ms"] > 0  # (a handle's first execution creates its device state after the query's first event)
        op.reopen()
        op.process_device_batch(batch)
        three = op.after_items_raw()
        st3 = op.stats()
        hold(op, three, st3, tkey, cond, keys, aggs, val)
        assert (st3["spec_kernel"], st3["agg_mode"], st3["rows_selected"], st3["groups_out"]) == \
            (st["spec_kernel"], st["agg_mode"], st["rows_selected"], st["groups_out"])
        return st
    finally:
        op.done()


# rows: two slabs; odd (the scalar launch of the last row: old tail); six tiles and a bit; more tiles than a small grid; 782
# tiles over the default grid of 768
ROWS = [2 * TILE, 2 * TILE + 1, 6 * TILE + 2, 200_000, 1_600_000]


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_shapes_by_rows(shape, rows):
    cond, aggs, val, opts = SHAPES[shape]
    st = one_call_and_three_calls(("synth", rows, 1000), cond, aggs, val, **opts)
    if shape == "prebuilt_sum":
        assert st["spec_kernel"] == 1
    elif shape.startswith("jit"):
        assert st["spec_kernel"] in (1, 2)  # (1: the shape is among the prebuilt ones as well)
    elif shape == "bounded_count_min":
        assert st["spec_kernel"] == 0


@pytest.mark.parametrize("shape,k_cat,opts,direct", [
    ("prebuilt_sum", 37, {"slabs": 2}, True),     # under one wave of slots, slabs forced
    ("five_aggregates", 37, {"slabs": 2}, True),
    ("prebuilt_sum", 1000, {}, True),             # S not a multiple of 16
    ("five_aggregates", 1000, {}, True),
    ("prebuilt_sum", 4000, {}, True),             # capacity 8192: the last table the new tail takes; 128 KB of LDS table: a
                                                  # 1024-thread scan, one workgroup per CU
    ("bounded_count_min", 4000, {}, False),       # ... (6 words per slot: beyond the LDS, an open-addressed table, no slabs)
    ("prebuilt_sum", 5000, {}, False),            # capacity 16384: the old tail
    ("jit_max_count", 5000, {"jit": 0, "spec": 0}, False),
], ids=lambda v: str(v))
def test_key_domains(shape, k_cat, opts, direct):
    cond, aggs, val, sopts = SHAPES[shape]
    one_call_and_three_calls(("synth", 200_000, k_cat), cond, aggs, val, expect_direct=direct, **dict(sopts, **opts))


@pytest.mark.parametrize("grid", [3, 64, 65, 0])
@pytest.mark.parametrize("k_cat", [37, 1000])
def test_slab_counts(k_cat, grid):
    """The slab count under, at and one past the fold kernel's 64 slab-lanes, and the default grid."""
    for shape in ("prebuilt_sum", "jit_sum_avg"):  # 98 tiles of 2048 rows
        cond, aggs, val, opts = SHAPES[shape]
        one_call_and_three_calls(("synth", 200_000, k_cat), cond, aggs, val, slabs=2, grid_blocks=grid, **opts)


@pytest.mark.parametrize("rows", [6 * TILE + 2, 200_000])
@pytest.mark.parametrize("jit", [1, 2])
def test_mixed_operands_over_a_dictionary_key(rows, jit):
    """Ints >= 2^40 leave the workgroup's narrow sum for the group's table row while everything else of the group is in the
    slabs: both parts reach the result, and the execution after it starts from a table that was cleared."""
    aggs = sorted(["sum(%s)" % V, "avg(%s)" % V, "min(%s)" % V, "max(%s)" % V, "count(%s)" % V])
    for k_cat in (37, 1000):
        one_call_and_three_calls(("mixed", rows, k_cat), None, aggs, V, slabs=2, jit=jit)


def test_no_survivor_one_group_and_lonely_slots():
    price_sum = ["sum(%s)" % PRICE]
    # a condition nothing passes: no group, no row
    one_call_and_three_calls(("synth", 200_000, 1000), "(1000000000 < %s)" % PRICE, price_sum, PRICE)
    # every row in one group
    one_call_and_three_calls(("synth", 200_000, 1), COND, price_sum, PRICE, slabs=2)
    # 4096 rows over 4000 categories: most groups are touched in exactly one of the two slabs
    # (four words per slot: 4003 slots are 128 KB of LDS table, the most a DIRECT table gets)
    one_call_and_three_calls(("synth", 2 * TILE, 4000), None, price_sum, PRICE, slabs=2)


def test_explicit_merge_chunks_takes_the_two_kernel_path():
    cond, aggs, val, opts = SHAPES["prebuilt_sum"]
    one_call_and_three_calls(("synth", 200_000, 1000), cond, aggs, val, merge_chunks=3, **opts)


def test_one_handle_through_both_tails():
    """one-call x 3, three calls, a one-call over another row count, a stop, a one-call again — each against the oracle.  The
    new kernel leaves the device clean (the executions behind it run no reset kernel and must find an empty table and zeroed
    counters to be right); the three-call finish does not, and the one-call behind it must start from a reset.

    n1k_run_device_batch is n1k_reset + push + finish, and n1k_reset forgets an earlier n1k_stop (include/n1k.h: reopen()): a
    stop sent BEFORE a one-call does not stop it.  The stop that is observed here is the one a push meets (three-call path),
    which leaves the handle in the middle of a query; the one-call after it must start clean all the same."""
    cond, aggs, val, _ = SHAPES["prebuilt_sum"]
    keys = [CAT]
    big, small = ("synth", 200_000, 1000), ("synth", 6 * TILE + 2, 1000)
    op = query_amd.GpuFilterGroup(plan.filter_group_plan(cond, keys, aggs))
    try:
        b_big, _k1 = device_batch(op, synth(*big[1:]))
        b_small, _k2 = device_batch(op, synth(*small[1:]))
        for _ in range(3):
            hold(op, op.run_device_batch_raw(b_big), op.stats(), big, cond, keys, aggs, val)
        op.reopen()
        op.process_device_batch(b_big)
        hold(op, op.after_items_raw(), op.stats(), big, cond, keys, aggs, val)
        hold(op, op.run_device_batch_raw(b_small), op.stats(), small, cond, keys, aggs, val)
        op.send_stop()  # before a one-call: its reset forgets the stop
        hold(op, op.run_device_batch_raw(b_big), op.stats(), big, cond, keys, aggs, val)
        op.reopen()
        op.process_device_batch(b_small)  # rows in the table, no finish
        op.send_stop()
        with pytest.raises(N1kError) as e:
            op.process_device_batch(b_small)
        assert e.value.status == 5  # N1K_STOPPED
        hold(op, op.run_device_batch_raw(b_big), op.stats(), big, cond, keys, aggs, val)
        hold(op, op.run_device_batch_raw(b_small), op.stats(), small, cond, keys, aggs, val)
    finally:
        op.done()
