"""n1k_finish on both sides of every boundary that decides which of its stages run: the speculative FinalGroup of small
tables (fused up to 8192 slots, finalize + publish up to 2^20, none above; a hit up to 4096 groups, the sized pass beyond),
the pinned landing of a sized result up to 8 MiB and the pageable one above, the default row of a plan without keys that
never saw a batch, and an empty batch.  One TAGGED64 integer key and sum() over small integers, no Filter, one
device-resident batch: the table then has next_pow2(max(2 * rows, 1024)) slots (ensure_table), so the row count fixes the
branch.  Expected values come from the oracle alone."""
import ctypes as C
import functools

import numpy as np
import pytest

import parity_util as pu
import query_amd
from oracle import n1o
from query_amd import _ffi
from query_amd.gpu_operator import GroupRows

pytestmark = pytest.mark.gpu

KEYS = [query_amd.plan.field_path("default", "k")]
AGGS = ["sum(%s)" % query_amd.plan.field_path("default", "v")]

# A sized result row as FinalGroup writes it: key, aggregate, the aggregate's partial (n1k_partial with the extreme's tag
# folded into the flag word: 8 bytes less), representative row.  Results up to 8 MiB land in pinned memory.
ROW_BYTES = 2 * C.sizeof(_ffi.Value) + (C.sizeof(_ffi.Partial) - 8) + 8
LAST_PINNED = (8 << 20) // ROW_BYTES


@functools.lru_cache(maxsize=None)
def _table_and_oracle(rows, distinct):
    rng = np.random.default_rng(rows * 31 + distinct)
    k = (np.arange(rows, dtype=np.int64) % max(distinct, 1)) * 7 - 11  # every key at least once, some negative
    rng.shuffle(k)
    v = rng.integers(-3, 10, size=rows, dtype=np.int64)
    tags = np.full(rows, n1o.T_INT, np.uint8)
    t = n1o.Table([n1o.Column(KEYS[0], n1o.COL_TAGGED64, tags=tags, payload=k.view(np.uint64)),
                   n1o.Column(query_amd.plan.field_path("default", "v"), n1o.COL_TAGGED64, tags=tags.copy(), payload=v.view(np.uint64))], [])
    ora = n1o.run(t, None, KEYS, AGGS)
    assert len(ora.keys) == distinct
    return t, ora


def _device_batch(op, t):
    import torch
    by = {c.name: c for c in t.columns}
    keep, cols = [], []
    for p in op.column_paths:
        c = by[p]
        # (an empty batch still names device memory)
        a = torch.from_numpy(c.tags if t.nrows else np.zeros(1, np.uint8)).cuda()
        b = torch.from_numpy(c.payload.view(np.int64) if t.nrows else np.zeros(1, np.int64)).cuda()
        keep += [a, b]
        cols.append((_ffi.COL_TAGGED64, a.data_ptr(), b.data_ptr(), None))
    torch.cuda.synchronize()
    return op.make_device_batch(t.nrows, cols), keep


def _sorted_raw(raw):
    order = np.argsort(raw["keys"]["v"][:, 0].view(np.int64), kind="stable")
    return raw["keys"][order], raw["aggs"][order], raw["partials"][order]


def _check(rows, distinct):
    t, ora = _table_and_oracle(rows, distinct)
    op = query_amd.GpuFilterGroup(query_amd.plan.filter_group_plan(None, KEYS, AGGS))
    try:
        batch, _keep = _device_batch(op, t)
        # twice in a row through the one-call path: the second execution starts from what the first one's finish left
        first = op.run_device_batch_raw(batch)
        second = op.run_device_batch_raw(batch)
        assert first["ngroups"] == second["ngroups"] == distinct
        for x, y in zip(_sorted_raw(first), _sorted_raw(second)):
            assert x.tobytes() == y.tobytes()
        if distinct:
            cache = {}
            got = GroupRows(1, 1, op._py_values(second["keys"], cache), op._py_values(second["aggs"], cache), [])
            pu.assert_same_groups(got, ora, aggs=AGGS)
            assert op.stats()["rows_selected"] == rows
        # ... and once batch by batch
        op.reopen()
        op.process_device_batch(batch)
        pu.assert_same_groups(op.after_items(), ora, aggs=AGGS)
        assert op.stats()["groups_out"] == distinct
    finally:
        op.done()


@pytest.mark.parametrize("rows,distinct", [
    (4096, 4096),      # 8192 slots: the fused speculative FinalGroup, hit exactly at its bound
    (4097, 4096),      # 16384 slots: finalize + publish, hit at the bound
    (4097, 4097),      # ... missed by one: the sized pass follows and reuses the out-count word
    (524288, 7),       # 2^20 slots, the last capacity that speculates: a hit,
    (524288, 5000),    # ... and a miss
    (524289, 7),       # 2^21 slots, the first that does not: the sized pass alone
    (524289, 5000),
], ids=lambda v: str(v))
def test_speculative_final_group_edges(rows, distinct):
    _check(rows, distinct)


def test_eight_mib_edge_follows_the_row_layout():
    """The two row counts of test_landing_edges are the edge only while a result row has this size."""
    assert ROW_BYTES == 88 and LAST_PINNED == 95325
    assert LAST_PINNED * ROW_BYTES == 8388600 <= (8 << 20) < (LAST_PINNED + 1) * ROW_BYTES == 8388688


@pytest.mark.parametrize("groups", [LAST_PINNED, LAST_PINNED + 1], ids=["pinned", "pageable"])
def test_landing_edges(groups):
    """2^18 slots, every row its own group: the last sized result that lands in pinned memory, the first that does not."""
    _check(groups, groups)


def test_empty_batch_on_a_keyed_plan():
    _check(0, 0)


def test_default_row_without_any_batch():
    """No keys, two aggregates, nothing pushed: FinalGroup's one row of Default() values, the device untouched before finish."""
    aggs = sorted(AGGS + ["count(*)"])
    t, _ = _table_and_oracle(0, 0)
    ora = n1o.run(t, None, [], aggs)
    assert len(ora.aggs) == 1
    op = query_amd.GpuFilterGroup(query_amd.plan.filter_group_plan(None, [], aggs))
    try:
        pu.assert_same_groups(op.after_items(), ora, aggs=aggs)
        assert op.stats()["groups_out"] == 1
    finally:
        op.done()
