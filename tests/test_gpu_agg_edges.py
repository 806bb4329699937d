"""Every accumulator route (CumulateInitial / CumulateIntermediate of COUNT, COUNTN, SUM, AVG, MIN, MAX) at the value edges, against
the yardstick of tests/agg_util.py: tag and payload bit for bit, a float SUM / AVG within its derived bound (agg_util.same_value).

Many small groups, each a chosen multiset of operands: every singleton, every well-defined ordered pair of the numeric pool and
the directed multisets of agg_util.  tests/test_agg_cpu.py holds the yardstick to a hand table and to the oracle, and asserts
that every group drawn here is well defined: no case is left out.  Each route asserts from stats() that its kernel ran.

The bounded kernel shape has at most five aggregates (kFastAggs), so the shaped routes run the six as two plans, PLAN_SUM and
PLAN_MM; the interpreter and the records path run all six at once.

The last tests are the workgroup-share overflow: one group of 2^23 + 64 rows in one workgroup's
share of a scan and in one bin of the partitioned path."""
import functools

import numpy as np
import pytest

import agg_util as ag
import parity_util as pu
import query_amd
from oracle import n1o
from query_amd import _ffi

pytestmark = pytest.mark.gpu

V, W, G = ag.V, ag.W, ag.G
HASH, DIRECT, PARTITIONED = 1, 2, 4  # N1K_MODE_* (include/n1k.h)
PLAN_ALL = ag.AGGS
PLAN_SUM = sorted("%s(%s)" % (k, V) for k in ("count", "countn", "sum", "avg", "max"))
PLAN_MM = sorted("%s(%s)" % (k, V) for k in ("min", "max", "count"))
ONE = {k: ["%s(%s)" % (k, V)] for k in ag.KINDS}


def must_run(fn, *a, **kw):
    """a refusal is a failure here, never a skip"""
    try:
        return fn(*a, **kw)
    except query_amd.N1kError as e:
        raise AssertionError("the device refused: %s" % e.message)


@functools.lru_cache(maxsize=None)
def drawn(n, offset, key, pad_to=0, second=False):
    names, groups = ag.window(n, offset)
    return names, groups, ag.table(groups, key=key, pad_to=pad_to, second=second), [ag.yardstick(g) for g in groups]


def check(names, groups, yards, got, aggs, what):
    kinds = [a.split("(")[0] for a in aggs]
    rows = ag.by_group(got, len(groups), aggs)
    bad = []
    for name, ops, y, r in zip(names, groups, yards, rows):
        bad += [(name, ops) + d for d in ag.differences(ops, r, y, kinds)]
    assert not bad, ("%s: %d values differ" % (what, len(bad)), bad[:6])


def run_and_check(n, offset, key, aggs, expect, what, pad_to=0, batches=1, second=False, **opts):
    names, groups, table, yards = drawn(n, offset, key, pad_to, second)
    got, st = must_run(pu.run_gpu, table, None, [G], aggs, batches=batches, **opts)
    for field, want in expect.items():
        ok = st[field] != 0 if want == "nonzero" else st[field] == want
        assert ok, ("%s: %s is %r, not %r: another kernel ran" % (what, field, st[field], want), opts)
    assert st["rows_in"] == table.nrows and st["groups_out"] == len(groups), (what, st)
    check(names, groups, yards, got, aggs, "%s, %d groups from %d, %d rows, %d batches" % (what, n, offset, table.nrows, batches))


# the sizes of one route: wave and workgroup edges, windows that together hold every group, one padded run whose rounds lie
# tiles apart (20 001 rows: ten tiles of 2048, more than one workgroup and slab hold parts of one group), and three batches
# with the rows of every pair / multiset on both sides of a boundary (merge_slot and the table's second visit)
NGROUPS = len(ag.all_groups())


def sizes(max_n):
    out = [(1, 11, 0, 1), (63, 0, 0, 1), (64, 40, 0, 1), (65, NGROUPS - 40, 0, 1)]  # (n, offset, pad_to, batches)
    if max_n >= 769:
        out += [(257, 300, 0, 1), (769, 0, 0, 1), (769, 0, 20_001, 1), (769, 0, 0, 3)]
    else:
        out += [(257, off, 0, 1) for off in range(0, NGROUPS, 257)]
        out += [(257, NGROUPS - 200, 20_001, 1)] + [(257, off, 0, 3) for off in range(0, NGROUPS, 257)]
    return out


# id -> (key kind, options, plans, expected stats, most groups a run may hold).  A plan is its aggregates, or (aggregates,
# further expected stats of that plan alone).  The stats have no field that says whether slabs were used: slabs-0 / slabs-2
# assert the table mode and the kernel of each plan, and rest on choose_scan's use_slabs for the slabs themselves.
SUM_PREBUILT = (ONE["sum"], {"spec_kernel": 1})
ROUTES = {
    # no prebuilt kernel has these shapes and the batches are far below jit_min_rows: the bounded-shape kernel, DIRECT, slabs
    # from 4096 table bytes on (37 groups), folded by fold_rows_kernel (one batch) or merge_slabs_kernel (three)
    "default-bounded-slabs": ("dict", {}, [PLAN_SUM, PLAN_MM], {"agg_mode": DIRECT, "spec_kernel": 0}, 769),
    # the prebuilt plan-specialised kernels (spec_acc): Spec_sum / Spec_avg over a dictionary key, Spec_ik_sum hashed
    "prebuilt-direct": ("dict", {}, [ONE["sum"], ONE["avg"]], {"agg_mode": DIRECT, "spec_kernel": 1}, 769),
    "prebuilt-hashed": ("int", {}, [ONE["sum"]], {"agg_mode": HASH, "spec_kernel": 1}, 769),
    "slabs-0": ("dict", {"slabs": 0}, [(PLAN_SUM, {"spec_kernel": 0}), (PLAN_MM, {"spec_kernel": 0}), SUM_PREBUILT], {"agg_mode": DIRECT}, 769),
    "slabs-2": ("dict", {"slabs": 2}, [(PLAN_SUM, {"spec_kernel": 0}), (PLAN_MM, {"spec_kernel": 0}), SUM_PREBUILT], {"agg_mode": DIRECT}, 769),
    "spec-0": ("dict", {"spec": 0}, [PLAN_SUM, PLAN_MM, ONE["sum"]], {"agg_mode": DIRECT, "spec_kernel": 0}, 769),
    # the interpreter: DIRECT while the key domain fits lds_bytes (65536 / 144 bytes: 455 slots), HASHED when told to
    "interpreter-direct": ("dict", {"fast": 0, "spec": 0}, [PLAN_ALL], {"agg_mode": DIRECT, "spec_kernel": 0}, 257),
    "interpreter-hash": ("int", {"fast": 0, "agg_mode": 1}, [PLAN_ALL], {"agg_mode": HASH, "spec_kernel": 0}, 769),
    # the scan built at run time (tables of at most 64 KiB: 585 slots of 112 bytes)
    "jit-direct": ("dict", {"jit": 2}, [PLAN_SUM, PLAN_MM], {"agg_mode": DIRECT, "spec_kernel": 2}, 257),
    "jit-hashed": ("int", {"jit": 2}, [PLAN_SUM, PLAN_MM], {"agg_mode": HASH, "spec_kernel": 2}, 769),
    # more groups than LDS slots: rows take acc_global while their neighbours take the LDS.  1024 bytes are 32 slots of
    # Spec_ik_sum (20 filled at most) and 7 of the interpreter's; 2048 bytes are 18 / 25 slots of the run-time-built scans
    "lds-1024-prebuilt": ("int", {"lds_bytes": 1024}, [ONE["sum"]], {"agg_mode": HASH, "spec_kernel": 1}, 769),
    "lds-1024-interpreter": ("int", {"lds_bytes": 1024}, [PLAN_ALL], {"agg_mode": HASH, "spec_kernel": 0}, 769),
    "lds-2048-jit": ("int", {"lds_bytes": 2048, "jit": 2}, [PLAN_SUM, PLAN_MM], {"agg_mode": HASH, "spec_kernel": 2}, 769),
    # 16-byte records into per-bin tables: each kind fixed at compile time (agg_spec 1), the generic kernel, tiny tables
    "records-specialised": ("int", {"agg_mode": 4, "jit": 2, "agg_spec": 1}, [ONE[k] for k in ag.KINDS], {"agg_mode": PARTITIONED, "spec_kernel": "nonzero"}, 769),
    "records-generic": ("int", {"agg_mode": 4, "jit": 2, "agg_spec": 0}, [PLAN_SUM, PLAN_MM, ONE["sum"]], {"agg_mode": PARTITIONED, "spec_kernel": "nonzero"}, 769),
    "records-64-slots": ("int", {"agg_mode": 4, "jit": 2, "rec_slots": 64}, [PLAN_SUM, PLAN_MM, ONE["avg"]], {"agg_mode": PARTITIONED, "spec_kernel": "nonzero"}, 769),
    # six aggregates are no bounded shape: rows -> (key, operand) arrays -> radix passes -> agg_bins_kernel, the exact partitioned path
    "partitioned-exact": ("int", {"agg_mode": 4}, [PLAN_ALL], {"agg_mode": PARTITIONED, "spec_kernel": 0}, 769),
    "partitioned-exact-64-slots": ("int", {"agg_mode": 4, "rec_slots": 64}, [PLAN_ALL], {"agg_mode": PARTITIONED, "spec_kernel": 0}, 769),
}


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_every_group_on_every_route(route):
    key, opts, plans, expect, max_n = ROUTES[route]
    for plan in plans:
        aggs, more = plan if isinstance(plan, tuple) else (plan, {})
        for n, offset, pad_to, batches in sizes(max_n):
            run_and_check(n, offset, key, aggs, dict(expect, **more), route, pad_to=pad_to, batches=batches, **opts)


def test_two_operand_columns_take_the_exact_partitioned_path():
    """(key, v, w): sum over one operand column and max over the other, w = v.  Two operand columns are no 16-byte record
    (run_group_records returns early for nsrc > 1; the engine has no wider record): the arrays of the exact partitioned path, 8 + 2 x (1 + 8) bytes a row, into agg_bins_kernel."""
    aggs = sorted(["sum(%s)" % V, "max(%s)" % W])
    names, groups, table, yards = drawn(769, 0, "int", 0, True)
    for opts in ({}, {"rec_slots": 64}):
        for batches in (1, 3):
            got, st = must_run(pu.run_gpu, table, None, [G], aggs, batches=batches, agg_mode=4, jit=2, **opts)
            assert st["agg_mode"] == PARTITIONED and st["spec_kernel"] == 0, (opts, st)
            check(names, groups, yards, got, aggs, "two operand columns %r" % (opts,))


def test_rehash_moves_populated_rows():
    """The table holds next_pow2(2 x rows pushed so far), at least 1024 slots (ensure_table): three batches of ~500 rows over
    769 int-keyed groups make it 1024, 2048 and 4096 slots, and rehash_kernel moves the rows the earlier batches filled."""
    names, groups, table, yards = drawn(769, 0, "int")
    assert 3 * 1024 // 2 > table.nrows > 1024 and table.nrows // 3 < 512
    for aggs, opts in ((PLAN_ALL, {}), (PLAN_SUM, {"jit": 2}), (PLAN_MM, {"jit": 2})):
        got, st = must_run(pu.run_gpu, table, None, [G], aggs, batches=3, **opts)
        assert st["agg_mode"] == HASH and st["batches"] == 3, st
        check(names, groups, yards, got, aggs, "rehash %r" % (opts,))


def test_an_array_operand_is_refused_not_returned():
    table = ag.table([ag.ARRAY_GROUP, [ag.I(1)]])
    for key_opts in ({}, {"jit": 2}, {"fast": 0}):
        with pytest.raises(query_amd.N1kError) as e:
            pu.run_gpu(table, None, [G], PLAN_MM, **key_opts)
        assert e.value.status == _ffi.UNSUPPORTED_DATA, e.value


@pytest.mark.timeout(300)
def test_partial_groups_split_between_two_ranks():
    """export_partials_kernel -> merge_partials_kernel over the loopback transport at world size 2: the interleaved table is cut
    in half, so the rows of every pair / multiset lie on both ranks, and every rank ends with every group."""
    from query_amd import distributed as qd
    from query_amd.gpu_operator import GroupRows
    from test_gpu_distributed import _device_cols, _run_ranks
    world = 2
    names, groups, table, yards = drawn(769, 0, "int")
    n = table.nrows
    for aggs in (PLAN_SUM, PLAN_MM):
        comms = qd.Comm.loopback(world, 0)
        probe = query_amd.GpuFilterGroup(query_amd.plan.filter_group_plan(None, [G], aggs))
        paths = probe.column_paths
        probe.done()
        shards, keep = [], []
        for r in range(world):
            lo, hi = n * r // world, n * (r + 1) // world
            dev, k = _device_cols(table.slice(lo, hi), paths)
            keep.append(k)
            shards.append((hi - lo, dev))

        def rank_body(r):
            op = qd.ShardedFilterGroup(None, [G], aggs, table.dictionary, r, world, 0, comm=comms[r])
            raw, info = op.run_partials(*shards[r])
            cache = {}
            return GroupRows(1, len(aggs), op.merger._py_values(raw["keys"], cache), op.merger._py_values(raw["aggs"], cache), []), info

        for rows, info in _run_ranks(world, rank_body):
            assert info["mode"] == "partials", info
            check(names, groups, yards, rows, aggs, "partials of two ranks")


# ------------------------------------------------------------------ the workgroup-share overflow
#
# Every LDS route keeps an int SUM as ONE wrapping 64-bit word per workgroup and takes |x| < 2^40 (acc_lds, acc_lds_value,
# spec_acc): more than 2^23 such rows of one group in one workgroup's share wrap it, and merge_slot / fold_slab sign-extend the
# wrapped word into the 128-bit total.  A scan's workgroup b takes the tiles b, b + grid, b + 2 grid, ... of 2048 rows each
# (n1k_spec.h: `base = blockIdx.x * tile; base += gridDim.x * tile`; scan_fast_kernel and the interpreter:
# `for (tile = blockIdx.x; tile < ntiles; tile += gridDim.x)`), so with grid_blocks = 1 one workgroup used to take every row.

BIG = 2 ** 40 - 1
N23 = 2 ** 23 + 64
SHARE_AGGS = sorted("%s(%s)" % (k, V) for k in ("sum", "avg", "min", "max", "count"))
SHARE_ROUTES = [pytest.param({}, id="default"), pytest.param({"spec": 0}, id="spec-0")]


def one_group(values):
    """a DICT32 key with one string (4 bytes a row) and the operand column"""
    n = len(values)
    return n1o.Table([n1o.Column(G, n1o.COL_DICT32, codes=np.zeros(n, np.uint32)),
                      n1o.Column(V, n1o.COL_TAGGED64, tags=np.full(n, ag.T_INT, np.uint8), payload=values.view(np.uint64))], [b"k"])


def share_run(values, opts, grid_blocks):
    got, st = must_run(pu.run_gpu, one_group(values), None, [G], SHARE_AGGS, device_resident=True, grid_blocks=grid_blocks, **opts)
    assert st["agg_mode"] == DIRECT and st["rows_in"] == len(values) and len(got.aggs) == 1, st
    return dict(zip([a.split("(")[0] for a in SHARE_AGGS], got.aggs[0]))


@pytest.mark.timeout(120)
@pytest.mark.parametrize("opts", SHARE_ROUTES)
@pytest.mark.parametrize("sign", [1, -1], ids=["positive", "negative"])
def test_2p23_rows_of_one_sign_in_one_workgroup(sign, opts):
    """n (2^40 - 1) is beyond int64: SUM is the FLOAT of the exact total, AVG folds back to the INT"""
    got = share_run(np.full(N23, sign * BIG, np.int64), opts, 1)
    assert got["sum"] == (ag.T_FLOAT, float(sign * N23 * BIG)), got
    assert got["avg"] == (ag.T_INT, sign * BIG) and got["min"] == got["max"] == (ag.T_INT, sign * BIG), got
    assert got["count"] == (ag.T_INT, N23), got


@pytest.mark.timeout(180)
@pytest.mark.parametrize("opts", SHARE_ROUTES)
def test_mixed_signs_recover_from_a_wrapped_share(opts):
    """A total of 0 over mixed signs is the FLOAT 0.
    (a) grid_blocks = 1, the first half positive and the second negative.
    (b) grid_blocks = 2, 8194 tiles of 2048 rows alternating in sign.
    Before min_grid_for_narrow_sums these layouts wrapped: in (a) one workgroup's word wrapped on the way and came back; in (b)
    workgroup 0 took the even tiles (all positive, 2^23 + 2048 rows) and workgroup 1 the odd ones, each share ALONE beyond
    +-2^63, and the two wraps of 2^64 cancelled in the 128-bit total: both passed then too.  Now the bound overrides
    grid_blocks (three workgroups for both layouts: shares of mixed signs, none wraps), and what this test holds is that the
    override is harmless."""
    half = np.full(N23, BIG, np.int64)
    want = {"sum": (ag.T_FLOAT, 0.0), "avg": (ag.T_INT, 0), "min": (ag.T_INT, -BIG), "max": (ag.T_INT, BIG)}
    got = share_run(np.concatenate([half, -half]), opts, 1)
    assert {k: got[k] for k in want} == want and got["count"] == (ag.T_INT, 2 * N23), got
    tiles = 2 * (2 ** 23 // 2048 + 1)
    values = np.where((np.arange(tiles * 2048) // 2048) % 2 == 0, BIG, -BIG).astype(np.int64)
    got = share_run(values, opts, 2)
    assert {k: got[k] for k in want} == want and got["count"] == (ag.T_INT, tiles * 2048), got


def records_run(keys, values):
    n = len(values)
    table = n1o.Table([n1o.Column(G, n1o.COL_TAGGED64, tags=np.full(n, ag.T_INT, np.uint8), payload=keys.astype(np.uint64)),
                       n1o.Column(V, n1o.COL_TAGGED64, tags=np.full(n, ag.T_INT, np.uint8), payload=values.view(np.uint64))], [])
    got, st = must_run(pu.run_gpu, table, None, [G], SHARE_AGGS, agg_mode=4, jit=2, rec_bins=1)
    assert st["agg_mode"] == PARTITIONED and st["rows_in"] == n, st
    # the exact path answered (run_group_partitioned sets 0, run_group_records its kernel's number): see the tests
    assert st["spec_kernel"] == 0, st
    kinds = [a.split("(")[0] for a in SHARE_AGGS]
    return {k[0][1]: dict(zip(kinds, a)) for k, a in zip(got.keys, got.aggs)}


def check_one_key(got, n, sign):
    assert got["sum"] == (ag.T_FLOAT, float(sign * n * BIG)), got
    assert got["avg"] == (ag.T_INT, sign * BIG) and got["min"] == got["max"] == (ag.T_INT, sign * BIG), got
    assert got["count"] == (ag.T_INT, n), got


@pytest.mark.timeout(120)
@pytest.mark.parametrize("sign", [1, -1], ids=["positive", "negative"])
def test_2p23_records_of_one_key_in_one_bin(sign):
    """The per-bin tables (agg_mode 4, rec_bins = 1).  One key's 2^23 + 64 records are more than a bin of agg_bins16_kernel
    holds for this table (about 3.2 M, with or without the 2^23 limit of run_group_records): the batch takes the exact path,
    asserted from spec_kernel, and there all of them are ONE bin of agg_bins_kernel, which scans a bin in segments of 2^23
    records."""
    got = records_run(np.full(N23, 5, np.int64), np.full(N23, sign * BIG, np.int64))
    assert list(got) == [5]
    check_one_key(got[5], N23, sign)


@pytest.mark.timeout(180)
def test_four_keys_of_2p23_records_each_in_segments():
    """Four keys of 2^23 + 64 rows each, of both signs, rows dealt round-robin (n = 2^25 + 256, rec_bins = 1): more than one
    key whose records are scanned in segments, their partial groups merged per key.  The exact path answers, here and
    before the limit of 2^23 records on a bin of agg_bins16_kernel (run_group_records) alike: where the records path keeps
    one key's 2^23 records in one of ITS bins has not been found at a size a test can run, and that limit stays unverified
    (DESIGN.md section 8, item 20)."""
    keys = np.array([3, 1000003, 77, 123456789], np.int64)
    signs = {3: 1, 1000003: -1, 77: 1, 123456789: -1}
    n = 4 * N23
    k = np.tile(keys, N23)
    v = np.tile(np.array([signs[int(x)] * BIG for x in keys], np.int64), N23)
    got = records_run(k, v)
    assert sorted(got) == sorted(signs)
    for key, sign in signs.items():
        check_one_key(got[key], N23, sign)
